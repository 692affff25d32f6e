"""vad_scan_refine, vad_refine_device, Engine.refine / refine_device, SegmentRefine and refine= of scan_recordings / sweep_recordings /
cut_recordings on the host side: exports, byte equality with tests/refine_ref.py (written from the header's rule) on the cases of
tests/refine_cases.py and on scripted scans - the resident table and a host table, tails folded in, truncation - the mark, every
refusal with its message and an untouched output, and the brute-force property of the split on the reference alone - the real
csrc/engine.cpp over the HIP stand-in (tests/standin.py: p = |first sample of a frame|, so the audio scripts the probabilities; the
stand-in states the rule in plain C++, list by list).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import refine_cases as cases
from tests import refine_ref, standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _ffi.VAD_ERR_INVALID_ARG
SENT = cases.SENT
DTYPE = refine_ref.DTYPE
THR = (0.5, 0.5, 0.8, 0.95, 2, 2)                 # a START after two high frames, an END after two low ones
OTHER = (0.6, 0.4, 0.7, 0.9, 3, 4)
RULE = (3, 4, 2, 3, 12, 0)                        # pad 3 / 4, join across 2 frames, drop below 3, split above 12: gaps of 3 .. 6 are shared
SEG_P = C.POINTER(_ffi.Segment)


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    handle = C.CDLL(standin.build(tmp_path_factory.mktemp("standin")))
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


@pytest.fixture(scope="module")
def make_engine(lib):
    from cutter_vad_amd.engine import Engine
    made = []

    def make(version=5, rate=16000, max_streams=128, shared_gpu=False):
        with open(weights_io.packaged_blob_path(version, rate), "rb") as f:
            blob = f.read()
        saved = _ffi._lib
        _ffi._lib = lib
        try:
            e = Engine(blob, model_version=version, max_streams=max_streams, sample_rate=rate, shared_gpu=shared_gpu)
        finally:
            _ffi._lib = saved
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


# ---- helpers ----------------------------------------------------------------------------------------------------------
def untouched(a):
    return a is None or bool((a.view(np.uint8) == SENT).all())


def script(p, frame, hop, tail=3):
    """a float32 recording whose frame t begins with p[t] - the stand-in's probability of that frame"""
    x = np.zeros((len(p) - 1) * hop + frame + tail if len(p) else 0, np.float32)
    x[np.arange(len(p)) * hop] = p
    return x


def speechy(rng, nframes):
    p = []
    voiced = bool(rng.integers(2))
    while len(p) < nframes:
        run = int(rng.integers(1, 13))
        p += list(rng.uniform(0.5, 0.95, run) if voiced else rng.uniform(0.0, 0.45, run))
        voiced = not voiced
    return np.asarray(p[:nframes], np.float32)


def corpus(frame, hop, seed=11):
    """scripted recordings of 0 .. 160 frames, one with a rejected frame inside speech, one that ends in a long segment"""
    rng = np.random.default_rng(seed)
    recs = [script(speechy(rng, n), frame, hop) for n in [0, 1, 160, 2, 159] + [int(v) for v in rng.integers(3, 159, 19)]]
    long = script([0.0, 0.0] + [0.9, 0.8, 0.7, 0.95, 0.6] * 9, frame, hop)
    long[20 * hop + 5] = np.nan
    return recs + [long]


def per_frame(make_engine, recs, hop, **kw):
    """Engine.scan on a twin engine -> the flat events and probs in item order and out_start"""
    twin = make_engine()
    slots = np.asarray(twin.open_streams(len(recs)))
    try:
        probs, ev, _ = twin.scan(slots, recs, hop=hop, denoise=None, **kw)
    finally:
        for s in slots:
            twin.close_stream(int(s))
    start = np.concatenate([[0], np.cumsum([len(p) for p in probs])]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt) for x in xs]) if len(xs) else np.zeros(0, dt)
    return cat(ev, np.uint8), cat(probs, np.float32), start


def scan_on(eng, recs, hop, thr=THR, **kw):
    slots = np.asarray(eng.open_streams(len(recs)))
    eng.set_thresholds_many(slots, thr)
    return slots, eng.scan_segments(slots, recs, hop=hop, denoise=None, **kw)


def close(eng, slots):
    for s in slots:
        eng.close_stream(int(s))


def rule_struct(rule):
    return None if rule is None else _ffi.Refine(*rule)


def raw_refine(lib, eng, rule=RULE, table=None, nin=None, tails=None, cap=None, out="own", count="own"):
    """vad_scan_refine itself, the output between sentinels -> (rc, message, out, count)"""
    cap = 64 if cap is None else cap
    if isinstance(out, str):
        out = cases.aligned(max(cap, 0) + 2, DTYPE, SENT)
    if isinstance(count, str):
        count = np.full(1, -7, np.int64)
    r = rule_struct(rule)
    rc = lib.vad_scan_refine(eng.handle, None if table is None else table.ctypes.data_as(SEG_P), (0 if table is None else len(table)) if nin is None else nin,
                             None if tails is None else tails.ctypes.data_as(SEG_P), None if r is None else C.byref(r),
                             None if out is None else out.ctypes.data_as(SEG_P), cap, None if count is None else count.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, lib.vad_last_error(eng.handle).decode(), out, count


def same(got, want):
    return refine_ref.same(np.ascontiguousarray(got), np.ascontiguousarray(want))


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    proto = lambda name: re.sub(r"/\*.*?\*/", "", re.search(r"VAD_API int %s\((.*?)\);" % name, header, re.S).group(1))
    for name, nargs in (("vad_refine_device", 14), ("vad_scan_refine", 8)):
        assert declared.count(name) == 1, name
        assert hasattr(lib, name), name
        assert len(proto(name).split(",")) == len(_ffi.SIGNATURES[name][1]) == nargs, name
    assert "#define VAD_ABI_VERSION 5" in header
    fields = re.search(r"typedef struct vad_refine \{(.*?)\} vad_refine;", header, re.S).group(1)
    assert re.findall(r"int32_t (\w+);", fields) == [f for f, _ in _ffi.Refine._fields_] and C.sizeof(_ffi.Refine) == 24
    import cutter_vad_amd
    from cutter_vad_amd import _build
    from cutter_vad_amd.engine import Engine
    assert "scan_refine.hip" in _build.HIP_SOURCES
    assert callable(Engine.refine) and callable(Engine.refine_device)
    assert "SegmentRefine" in cutter_vad_amd.__all__
    r = cutter_vad_amd.SegmentRefine()
    assert (r.pad_before, r.pad_after, r.merge_gap, r.min_frames, r.max_frames, r.reserved) == refine_ref.NEUTRAL


def test_segment_refine_from_durations_rounds_to_frames():
    from cutter_vad_amd import SegmentRefine
    r = SegmentRefine.from_durations(256, 16000, pad_ms=30, merge_gap_ms=100, min_speech_ms=250, max_speech_s=30)
    assert r == SegmentRefine(2, 2, 6, 16, 1875, 0)                       # 1.875, 6.25, 15.625 hops; 30 s = 1875 hops
    assert SegmentRefine.from_durations(256, 16000) == SegmentRefine()
    assert SegmentRefine.from_durations(768, 48000, max_speech_s=0.01).max_frames == 2
    assert SegmentRefine.from_durations(128, 8000, merge_gap_ms=0, max_speech_s=29.999).max_frames == 1874


# ---- the rule, on the reference alone ---------------------------------------------------------------------------------
def test_the_split_keeps_every_piece_between_one_frame_and_the_limit():
    """every boundary at either end of its window, max_frames 2 .. 79, every length up to 8 max_frames + 2: pieces of 1 .. max_frames
    frames that tile the segment, windows that never meet - and refine_item's pieces for probabilities that pull every cut one way"""
    for mf in range(2, 80):
        for length in range(1, 8 * mf + 3):
            if length <= mf:
                continue
            k, h, cuts = refine_ref.split_plan(length, mf)
            assert k == -(-length // mf) and h >= 0
            lo = [0] + [c - h for c in cuts] + [length]
            hi = [0] + [c + h for c in cuts] + [length]
            for j in range(k):
                assert lo[j + 1] - hi[j] >= 1 and hi[j + 1] - lo[j] <= mf, (mf, length, j)
    ev = np.zeros(700, np.uint8)
    for mf in (2, 3, 7, 20, 79):
        for length in (mf + 1, 2 * mf, 2 * mf + 1, 7 * mf - 1, 8 * mf + 2):
            for probs in (np.linspace(0.9, 0.1, 700, dtype=np.float32), np.linspace(0.1, 0.9, 700, dtype=np.float32)):
                pieces = refine_ref.refine_item([(5, length)], 700, (0, 0, -1, 0, mf, 0), probs, ev)
                assert pieces[0][0] == 5 and sum(L for _, L in pieces) == length and all(1 <= L <= mf for _, L in pieces)
                assert all(a + L == b for (a, L), (b, _) in zip(pieces, pieces[1:]))


# ---- the device form, case by case ------------------------------------------------------------------------------------
CASES = {
    "corpus": lambda: cases.corpus37(np.random.default_rng(1), (3, 5, 6, 4, 25, 0)),
    "corpus_ties": lambda: cases.corpus37(np.random.default_rng(2), (4, 1, 2, 0, 9, 0), ties=True),
    "corpus_neutral": lambda: cases.corpus37(np.random.default_rng(3), refine_ref.NEUTRAL, with_tails=False),
    "chain": lambda: cases.chain(np.random.default_rng(4)),
    "pads": lambda: cases.pads(np.random.default_rng(5)),
    "drops": lambda: cases.drops(np.random.default_rng(6)),
    "splits": lambda: cases.splits(np.random.default_rng(7)),
    "pairs": lambda: cases.pairs(np.random.default_rng(8)),
    "garbage": lambda: cases.garbage(np.random.default_rng(9)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_device_form_equals_the_reference(make_engine, name):
    eng = make_engine()
    c = CASES[name]()
    want = cases.want(c)
    seen = refine_ref.census(c.table[:min(c.nsegs, c.in_cap)], c.tails, c.start, c.rule)
    assert len(want) >= 2 and (name == "corpus_neutral" or sum(seen.values()) >= 1), seen
    for cap in (len(want) + 3, len(want), len(want) // 2, 0):
        count, got, clean = cases.run(eng, c, cap)
        assert count == len(want) and clean and same(got, want[:cap]), (name, cap, count, len(want))


@pytest.mark.parametrize("name", cases.PAST)
def test_the_cases_past_a_wave_a_workgroup_and_a_grid(make_engine, name):
    """the GPU suite's structural cases (tests/refine_cases.py: past) with every condition they are for asserted on the reference, and
    the stand-in's records at their caps: item counts around 64 and 256, windows wider than a wave, more records than the cut
    kernel's grid, heads at workgroup edges, the bit patterns of +0.0, denormals and 1.0"""
    eng = make_engine()
    c, want, caps = cases.past(name)
    for cap in tuple(caps) + (0,):
        count, got, clean = cases.run(eng, c, cap)
        assert count == len(want) and clean and same(got, want[:cap]), (name, cap, count, len(want))


def test_every_cap_of_a_small_table(make_engine):
    eng = make_engine()
    c = cases.splits(np.random.default_rng(7))
    want = cases.want(c)
    for cap in cases.every_cap(c, want):
        count, got, clean = cases.run(eng, c, cap)
        assert count == len(want) and clean and same(got, want[:cap]), cap


def test_negative_probabilities_order_by_bit_pattern(make_engine):
    """the header's sentence on a caller's own d_probs: -0.0 and negative values lie above every non-negative probability.  The
    reference states the rule for the sign bit clear only and takes the -0.0 as a minimum; stand-in and kernel follow the header."""
    c, rows = cases.negzero(np.random.default_rng(0))
    by_value = [tuple(r)[:3] for r in cases.want(c).tolist()]
    assert by_value == [(0, 8, 7), (0, 15, 14), (1, 8, 7), (1, 15, 14)] != rows
    count, got, clean = cases.run(make_engine(), c, 6)
    assert count == 4 and clean and [tuple(r)[:3] for r in got.tolist()] == rows


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_has_the_device_form(make_engine, kw):
    eng = make_engine(**kw)
    c = cases.corpus37(np.random.default_rng(12), (3, 5, 6, 4, 25, 0))
    want = cases.want(c)
    count, got, clean = cases.run(eng, c, len(want) + 1)
    assert count == len(want) > 20 and clean and same(got, want)


def test_the_named_cases_hold_what_their_names_say():
    """by the reference alone"""
    rng = np.random.default_rng(0)
    c = cases.pads(rng)
    w = cases.want(c)
    rows = [tuple(r)[:3] for r in w.tolist()]
    # gaps 5, 4 and 1 shared as floor(g 3 / 7) behind and the rest in front; the overlapping pair unpadded between them; clipped at 100
    assert rows[:7] == [(0, 0, 14), (0, 14, 10), (0, 24, 8), (0, 32, 5), (0, 37, 8), (0, 40, 13), (0, 92, 8)]
    assert rows[7:] == [(1, 0, 8), (1, 26, 14), (2, 0, 50)]
    c = cases.drops(rng)
    assert [tuple(r)[:3] for r in cases.want(c).tolist()] == [(0, 19, 8), (0, 59, 8)]
    c = cases.splits(rng)
    w = cases.want(c)
    per = lambda i: [int(v) for v in w["nframes"][w["item"] == i]]
    assert [len(per(i)) for i in range(4)] == [2 + 2 + 3, 7, 1, 3] and max(w["nframes"]) <= 20 and per(0)[2:4] == [20, 20]
    first = w[w["item"] == 3]
    k, h, cuts = refine_ref.split_plan(50, 20)
    assert int(first["first_frame"][1]) == 10 + cuts[0] - 1                 # equal minima: the lower frame
    assert int(first["first_frame"][2]) == 10 + cuts[1]                     # a window of rejected frames: the nominal cut
    assert (first["counted"] < first["nframes"]).any()
    c = cases.pairs(rng)
    assert set(cases.want(c)["nframes"].tolist()) <= {1, 2} and len(cases.want(c)) == 31 + 5
    c = cases.chain(rng)
    seen = refine_ref.census(c.table, c.tails, c.start, c.rule)
    assert seen["merges"] == 329 and seen["splits"] == 1
    c = cases.garbage(rng)
    w = cases.want(c)
    spans = []
    for i, f, L in [tuple(r)[:3] for r in w.tolist()]:
        if spans and spans[-1][0] == i and spans[-1][2] == f:
            spans[-1][2] = f + L
        else:
            spans.append([i, f, f + L])
    # item 0: [2, 7) and [20, 24) padded by 2 and split by 7 (its later run [30, 35) is absent); item 1 clipped at its 10 frames;
    # item 2: [1, 7) and [9, 13), two frames apart, join and are padded to [0, 15), the records outside the item and the later run
    # absent; item 3: [0, 2) behind [5, 10) joins it into a group of no frames
    assert spans == [[0, 0, 9], [0, 18, 26], [1, 0, 6], [2, 0, 15]] and len(w) == 8 and max(w["nframes"]) <= 7


def test_device_form_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    c = cases.drops(np.random.default_rng(6))
    ev, probs, start = cases.aligned(len(c.events), np.uint8), cases.aligned(len(c.probs), np.float32), c.start
    ev[:], probs[:] = c.events, c.probs
    tab = cases.aligned(len(c.table), DTYPE)
    tab[:] = c.table
    nin = np.asarray([len(tab)], np.int64)

    def refused(pattern, rule=RULE, tab=tab, nin=nin, in_cap=len(tab), tails=None, ev=ev, probs=probs, start=start, n=None, cap=8, out="own", cnt="own"):
        st = None if start is None else np.ascontiguousarray(start, np.int64)
        n = (st.size - 1) if n is None else n
        if isinstance(out, str):
            out = cases.aligned(10, DTYPE, SENT)
        if isinstance(cnt, str):
            cnt = cases.aligned(2, np.int64, SENT)
        r = rule_struct(rule)
        rc = lib.vad_refine_device(eng.handle, cases.ptr(tab), cases.ptr(nin), in_cap, cases.ptr(tails), cases.ptr(ev), cases.ptr(probs),
                                   None if st is None else st.ctypes.data_as(C.POINTER(C.c_int64)), n, None if r is None else C.byref(r),
                                   cases.ptr(out), cap, cases.ptr(cnt), None)
        msg = lib.vad_last_error(eng.handle).decode()
        assert rc == INV and msg.startswith("Model prediction failed: vad_refine_device: ") and re.search(pattern, msg), (rc, msg)
        assert untouched(out) and untouched(cnt)

    refused("null rule", rule=None)
    refused("pad_before = -1, pad_after = 3: a pad is 0 or more", rule=(-1, 3, 0, 0, 0, 0))
    refused("pad_before = 2, pad_after = -5", rule=(2, -5, 0, 0, 0, 0))
    refused("merge_gap = -2: -1 \\(never join\\)", rule=(0, 0, -2, 0, 0, 0))
    refused("max_frames = 1: 0 \\(no limit\\) or at least 2", rule=(0, 0, 0, 0, 1, 0))
    refused("max_frames = -4", rule=(0, 0, 0, 0, -4, 0))
    refused("reserved = 9: must be 0", rule=(0, 0, 0, 0, 0, 9))
    refused("seg_cap = -1: bad count", cap=-1)
    refused("n = -1, in_cap = 7: bad count", n=-1)
    refused("n = 1, in_cap = -2: bad count", in_cap=-2)
    refused("more than 2\\^31 - 1 items", n=1 << 31)
    refused("more than 2\\^31 - 1 input records", in_cap=1 << 31)
    refused("null buffer", start=None, n=1)
    refused("null buffer", nin=None)
    refused("null buffer", cnt=None)
    refused("null buffer", tab=None)
    refused("null buffer", out=None)
    refused("null buffer", ev=None)
    refused("null buffer", probs=None)
    refused("out_start\\[0\\] is negative", start=[-4, 100])
    refused("out_start decreases at item 1 \\(50 after 100\\)", start=[0, 100, 50])
    refused("more than 2\\^31 - 1 frames", start=[0, 1 << 31])
    off = lambda a: a.view(np.uint8)[8:8 + (a.size - 1) * a.itemsize].view(a.dtype)
    refused("must be 16-byte aligned", ev=cases.aligned(len(ev) + 8, np.uint8)[8:])
    refused("must be 16-byte aligned", tab=off(cases.aligned(len(tab) + 1, DTYPE)))
    refused("must be 16-byte aligned", tails=off(cases.aligned(2, DTYPE)))
    refused("must be 16-byte aligned", out=off(cases.aligned(11, DTYPE, SENT)))
    refused("probs must be 4-byte aligned", probs=cases.aligned(4 * len(probs) + 2, np.uint8)[2:2 + 4 * len(probs)].view(np.float32))
    refused("counts must be 8-byte aligned", cnt=cases.aligned(4, np.int32, SENT)[1:3].view(np.int64))
    refused("counts must be 8-byte aligned", nin=cases.aligned(4, np.int32)[1:3].view(np.int64))
    assert lib.vad_refine_device(None, None, None, 0, None, None, None, None, 0, None, None, 0, None, None) == INV
    # no items: the count alone
    cnt = np.full(1, -7, np.int64)
    r = rule_struct(RULE)
    assert lib.vad_refine_device(eng.handle, None, cases.ptr(nin), 0, None, None, None, None, 0, C.byref(r), None, 0, cases.ptr(cnt), None) == 0
    eng.synchronize()
    assert cnt[0] == 0


# ---- the host form ----------------------------------------------------------------------------------------------------
def test_the_resident_table_a_host_table_and_the_tails(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = corpus(frame, hop)
    ev, probs, start = per_frame(make_engine, recs, hop)
    slots, table = scan_on(eng, recs, hop)
    try:
        tails = eng.scan_tails()
        assert len(table) > 30 and int((tails["nframes"] > 0).sum()) >= 5 and (ev & 0x80).any()
        for rule in (RULE, (0, 0, 2, 0, 0, 0), (5, 0, -1, 6, 0, 0), (0, 0, -1, 0, 7, 0), refine_ref.NEUTRAL):
            want = refine_ref.refine(table, None, ev, probs, start, rule)
            folded = refine_ref.refine(table, tails, ev, probs, start, rule)
            assert len(folded) > len(want) - 3 and folded.tobytes() != want.tobytes()
            assert same(eng.refine(rule), want) and same(eng.refine(rule, table), want)          # resident, then host
            assert same(eng.refine(rule, None, tails), folded) and same(eng.refine(rule, table, tails), folded)
            # a tail is its item's last record: the table with the tails sorted in gives the same
            rows = np.concatenate([table, tails[tails["nframes"] > 0]])
            rows = rows[np.argsort(rows["item"], kind="stable")]
            assert same(eng.refine(rule, rows), folded)
        assert same(eng.refine(refine_ref.NEUTRAL), table)
        seen = refine_ref.census(table, tails, start, RULE)
        assert min(seen.values()) >= 1, seen
        # another set's table goes in through segs_in, with that set's tails
        other, otails = eng.resegment([OTHER])[0], eng.resegment_tails([OTHER])[0]
        assert other.tobytes() != np.ascontiguousarray(table).tobytes()
        assert same(eng.refine(RULE, other, otails), refine_ref.refine(other, otails, ev, probs, start, RULE))
        assert len(eng.refine(RULE, table[:0])) == 0 and same(eng.refine(RULE, table[:0], tails), refine_ref.refine(table[:0], tails, ev, probs, start, RULE))
        # truncation: the first records, the true count
        want = refine_ref.refine(table, tails, ev, probs, start, RULE)
        for cap in (0, 1, len(want) - 1, len(want), len(want) + 5):
            rc, msg, out, count = raw_refine(lib, eng, RULE, None, tails=np.ascontiguousarray(tails), cap=cap)
            k = min(cap, len(want))
            assert rc == 0 and count[0] == len(want) and same(out[:k], want[:k]) and untouched(out[k:]), (cap, msg)
    finally:
        close(eng, slots)


def test_a_refinement_leaves_tables_streams_and_the_resident_block_alone(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = corpus(frame, hop)
    slots, table = scan_on(eng, recs, hop)
    try:
        read = lambda out, k: lib.vad_scan_segments_read(eng.handle, 0, k, out.ctypes.data_as(SEG_P))
        own = cases.aligned(len(table), DTYPE)
        assert read(own, len(table)) == 0
        before = own.tobytes()
        tails = eng.scan_tails().copy()
        reseg = np.ascontiguousarray(eng.resegment([OTHER])[0]).tobytes()
        saved = [eng.save_stream(int(s)) for s in slots]
        info = eng.info()
        fine = eng.refine(RULE, None, tails)
        assert [eng.save_stream(int(s)) for s in slots] == saved
        assert (eng.info()["steps"], eng.info()["frames"]) == (info["steps"], info["frames"])
        assert read(own, len(table)) == 0 and own.tobytes() == before
        assert same(eng.scan_tails(), tails) and np.ascontiguousarray(eng.resegment([OTHER])[0]).tobytes() == reseg
        # the resident block cuts the refined records
        offs = eng.last_scan["offsets"]
        pcm, where = eng.cut([(int(offs[i]), int(f), int(n)) for i, f, n in zip(fine["item"], fine["first_frame"], fine["nframes"])], hop=hop, denoise=None)
        assert pcm.size == frame * int(fine["nframes"].sum()) and where[-1] == pcm.size
        r = fine[3]
        hand = np.concatenate([np.nan_to_num(recs[int(r["item"])][f * hop:f * hop + frame]) for f in range(int(r["first_frame"]), int(r["first_frame"] + r["nframes"]))])
        assert pcm[where[3]:where[4]].tolist() == (hand * np.float32(32767.0)).astype(np.int16).tolist()
    finally:
        close(eng, slots)


def test_the_mark_and_the_refusals_of_the_host_form(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = [script([0.0] * 2 + [0.9] * 6 + [0.0] * 3, frame, hop), script([0.9] * 5 + [0.0] * 4 + [0.9] * 3, frame, hop)]

    def gone():
        rc, msg, out, count = raw_refine(lib, eng)
        assert rc == INV and "vad_scan_refine: no scan results are resident" in msg and msg.startswith("Model prediction failed: "), msg
        assert untouched(out) and count[0] == -7
        with pytest.raises(Exception, match="no scan results are resident"):
            eng.refine(RULE)
        with pytest.raises(Exception, match="vad_scan_resegment: no scan results are resident"):
            eng.resegment([OTHER])

    gone()                                                  # a fresh engine
    slots = np.asarray(eng.open_streams(2))
    extra = int(eng.open_stream())
    try:
        def rescan():
            eng.reset(slots)
            eng.set_thresholds_many(slots, THR)
            table = eng.scan_segments(slots, recs, hop=hop, denoise=None)
            assert [tuple(r)[:3] for r in table.tolist()] == [(0, 2, 8), (1, 0, 7)]
            assert [tuple(r)[:3] for r in eng.refine((1, 1, -1, 0, 5, 0), None, eng.scan_tails()).tolist()][-1] == (1, 8, 4)
            return table

        writers = {                                         # whatever drops the mark for vad_scan_resegment
            "vad_step": lambda: eng.step([extra], np.zeros((1, frame), np.float32)),
            "vad_step_multi, past the small-call path": lambda: eng.step_multi(slots, np.zeros((2, 80, frame), np.float32)),
            "vad_scan": lambda: eng.scan(slots, recs, hop=hop, denoise=None),
            "vad_debug_sm_replay": lambda: eng.debug_sm_replay(extra, [0.1, 0.9, 0.2]),
            "vad_tick_run": lambda: (eng.tick_push(extra, np.zeros(frame, np.float32)), eng.tick_run()),
            "vad_step_submit": lambda: eng.collect(eng.submit([extra], np.zeros((1, frame), np.float32))),
            "vad_step_rates": lambda: eng.step_rates([(np.zeros((1, 1536), np.float32), 48000)], [extra]),
        }
        for name, write in writers.items():
            rescan()
            write()
            gone()
        rescan()
        with pytest.raises(Exception, match="hop"):
            eng.scan_segments(slots, recs, hop=6, denoise=None)
        gone()
        # calls that write neither array keep the mark: a cut, thresholds, a replay, the tails, a refinement
        table = rescan()
        eng.cut([(0, 2, 6)], hop=hop, denoise=None)
        eng.set_thresholds_many(slots, OTHER)
        eng.resegment([OTHER])
        eng.scan_tails()
        assert same(eng.refine(refine_ref.NEUTRAL), table) and same(eng.refine(refine_ref.NEUTRAL), table)

        def refused(pattern, **kw):
            rc, msg, out, count = raw_refine(lib, eng, **kw)
            assert rc == INV and msg.startswith("Model prediction failed: vad_scan_refine: ") and re.search(pattern, msg), (rc, msg)
            assert untouched(out) and (count is None or count[0] == -7)

        tab = np.ascontiguousarray(table)
        bad = lambda k, **f: (lambda t: (t.__setitem__(k, tuple(f.get(n, t[k][n]) for n in DTYPE.names)), t)[1])(tab.copy())
        refused("null rule", rule=None)
        refused("pad_before = -1", rule=(-1, 0, 0, 0, 0, 0))
        refused("pad_before = 0, pad_after = -2", rule=(0, -2, 0, 0, 0, 0))
        refused("merge_gap = -3", rule=(0, 0, -3, 0, 0, 0))
        refused("max_frames = 1:", rule=(0, 0, 0, 0, 1, 0))
        refused("max_frames = -1:", rule=(0, 0, 0, 0, -1, 0))
        refused("reserved = 1: must be 0", rule=(0, 0, 0, 0, 0, 1))
        refused("seg_cap = -1: bad count", cap=-1)
        refused("null buffer", count=None)
        refused("null buffer", out=None, cap=4)
        refused("nsegs_in = -1: bad count", table=tab, nin=-1)
        refused("record 1 names item 2: the scan had 2 items", table=bad(1, item=2))
        refused("record 0 names item -1", table=bad(0, item=-1))
        refused("the items decrease at record 1 \\(0 after 1\\)", table=tab[::-1].copy())
        refused("record 1 has nframes = 0", table=bad(1, nframes=0))
        assert lib.vad_scan_refine(None, None, 0, None, None, None, 0, None) == INV
        with pytest.raises(Exception, match="3 tails for the 2 items"):
            eng.refine(RULE, None, np.zeros(3, DTYPE))
        # a scan without frames, or without items, is a valid result without records
        eng.scan_segments(slots, [np.zeros(0, np.float32), np.zeros(100, np.float32)], hop=hop, denoise=None)
        assert len(eng.refine(RULE)) == 0 and len(eng.refine(RULE, None, eng.scan_tails())) == 0
        eng.scan_segments(slots[:0], [], hop=hop, denoise=None)
        assert len(eng.refine(RULE)) == 0
    finally:
        close(eng, list(slots) + [extra])


# ---- the Python surface -----------------------------------------------------------------------------------------------
def cfg_of(s, frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=s[0], vad_end_probability=s[1], voice_start_ratio=s[2],
                     voice_end_ratio=s[3], voice_start_frame_count=s[4], voice_end_frame_count=s[5], **{"enable_denoising": False, **kw})


def expected_lists(make_engine, recs, thr, frame, hop, rule, stats, open_end):
    """scan_recordings(refine=rule) by the reference: the unrefined scan of a twin, its tails, refine_ref, then the ranges"""
    twin = make_engine()
    ev, probs, start = per_frame(make_engine, recs, hop)
    slots, table = scan_on(twin, recs, hop, thr=thr)
    try:
        tails = twin.scan_tails() if open_end else None
    finally:
        close(twin, slots)
    fine = refine_ref.refine(table, tails, ev, probs, start, rule)
    out = [[] for _ in recs]
    for r in fine:
        a = int(r["first_frame"]) * hop
        rg = (a, (int(r["first_frame"]) + int(r["nframes"]) - 1) * hop + frame)
        out[int(r["item"])].append(rg + (float(r["mean_prob"]), float(r["max_prob"])) if stats else rg)
    return out, fine


def test_refine_in_scan_sweep_and_cut_recordings(lib, make_engine):
    from cutter_vad_amd import ConfigurationError, SegmentRefine, cut_recordings, scan_recordings, sweep_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame // 2
    recs = corpus(frame, hop, seed=23)
    rule = SegmentRefine(*RULE)
    cfgs = [cfg_of(THR, frame), cfg_of(OTHER, frame)]
    for stats in (False, True):
        for open_end in (False, True):
            want, fine = expected_lists(make_engine, recs, THR, frame, hop, rule, stats, open_end)
            assert len(fine) > 20
            got = scan_recordings(recs, cfgs[0], engine=eng, hop=hop, stats=stats, open_end=open_end, refine=rule)
            assert got == want, (stats, open_end)
            plain = scan_recordings(recs, cfgs[0], engine=eng, hop=hop, stats=stats, open_end=open_end)
            assert plain == scan_recordings(recs, cfgs[0], engine=eng, hop=hop, stats=stats, open_end=open_end, refine=None) != got
            assert scan_recordings(recs, cfgs[0], engine=eng, hop=hop, stats=stats, open_end=open_end, refine=SegmentRefine()) == plain
            swept = sweep_recordings(recs, cfgs, engine=eng, hop=hop, stats=stats, open_end=open_end, refine=rule)
            assert swept[0] == want and swept[1] == expected_lists(make_engine, recs, OTHER, frame, hop, rule, stats, open_end)[0] != want
            assert sweep_recordings(recs, cfgs, engine=eng, hop=hop, stats=stats, open_end=open_end, refine=None) == \
                sweep_recordings(recs, cfgs, engine=eng, hop=hop, stats=stats, open_end=open_end)
    want, _ = expected_lists(make_engine, recs, THR, frame, hop, rule, False, True)
    cut = cut_recordings(recs, cfgs[0], engine=eng, hop=hop, wav=False, layout="range", open_end=True, refine=rule)
    assert [[(a, b) for a, b, _ in one] for one in cut] == want
    for rec, one in zip(recs, cut):
        for a, b, pcm in one:
            assert pcm.tolist() == (np.nan_to_num(rec[a:b]) * np.float32(32767.0)).astype(np.int16).tolist()
    plain = cut_recordings(recs, cfgs[0], engine=eng, hop=hop, wav=False, layout="range", open_end=True)
    again = cut_recordings(recs, cfgs[0], engine=eng, hop=hop, wav=False, layout="range", open_end=True, refine=None)
    assert [[(a, b, p.tobytes()) for a, b, p in one] for one in plain] == [[(a, b, p.tobytes()) for a, b, p in one] for one in again]

    class Old:
        frame_samples, sample_rate = frame, 16000

    for call in (lambda: scan_recordings(recs, cfgs[0], engine=Old(), refine=rule), lambda: cut_recordings(recs, cfgs[0], engine=Old(), refine=rule)):
        with pytest.raises(ConfigurationError, match="refine"):
            call()

    class NoRefine:
        """an engine object from before the refinement"""
        def __init__(self, e):
            self._e = e

        def __getattr__(self, k):
            if k in ("refine", "refine_device"):
                raise AttributeError(k)
            return getattr(self._e, k)

    with pytest.raises(ConfigurationError, match="sweep_recordings: refine= needs an engine with refine"):
        sweep_recordings(recs, cfgs, engine=NoRefine(eng), hop=hop, refine=rule)
    assert sweep_recordings(recs, cfgs, engine=NoRefine(eng), hop=hop) == sweep_recordings(recs, cfgs, engine=eng, hop=hop)


def _hipcc():
    import shutil
    return next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_the_new_kernels_compile_without_scratch_or_spills(tmp_path):
    """from the compiler's own metadata"""
    import subprocess
    from cutter_vad_amd import _build
    out = tmp_path / "scan_refine.s"
    subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "cutter_vad_amd", "csrc", "scan_refine.hip")], check=True, capture_output=True, timeout=600)
    seen = {}
    for m in re.findall(r"\.name:\s*_Z\d+(vadk_\w+?)N4vadk.*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                        out.read_text(), re.S):
        seen[m[0]] = m[1:]
    assert set(seen) == {"vadk_refine_init", "vadk_refine_heads", "vadk_refine_count", "vadk_refine_prefix", "vadk_refine_fill", "vadk_refine_cuts"}, seen
    assert all(v == ("0", "0", "0") for v in seen.values()), seen


# ---- the order of the refusals ----------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, make_engine):
    """The order of the checks is behaviour.  vad_refine_device: the rule's fields in their order and seg_cap; the counts; 2^31 items,
    2^31 input records; the null arguments; the positions; the null per-frame arrays; the 16-, 4- and 8-byte alignments.
    vad_scan_refine: the rule and seg_cap, the null arguments, the resident results, then the caller's table - nsegs_in, an item out
    of range, items that decrease, a record without frames.  (The refusal of a null segs_in without a resident table lies where the
    caller's table is checked; a scan leaves results and table together, so no call reaches it behind the resident check.)  Every
    fault at once, then one mended at a time; and a resident scan without a frame gives *nsegs_out = 0."""
    from tests import refusal_order as RO
    eng = make_engine()
    rules = (
        (INV, "null rule", "rule", (-1, -2, -3, 0, 1, 9)),
        (INV, "pad_before = -1, pad_after = -2: a pad is 0 or more", "rule", (0, -2, -3, 0, 1, 9)),
        (INV, "pad_before = 0, pad_after = -2: a pad is 0 or more", "rule", (0, 0, -3, 0, 1, 9)),
        (INV, "merge_gap = -3: -1", "rule", (0, 0, -1, 0, 1, 9)),
        (INV, "max_frames = 1: 0", "rule", (0, 0, -1, 0, 0, 9)),
        (INV, "reserved = 9: must be 0", "rule", (0, 0, -1, 0, 0, 0)),
        (INV, "seg_cap = -1: bad count", "cap", 4))
    table = lambda *rows: np.array([r + (0, 0.0, 0.0) for r in rows], DTYPE)

    def device(tab, nin, in_cap, tails, ev, probs, start, n, rule, out, cap, cnt):
        r = rule_struct(rule)
        return lib.vad_refine_device(eng.handle, RO.addr(tab), RO.addr(nin), in_cap, RO.addr(tails), RO.addr(ev), RO.addr(probs), RO.i64p(start), n,
                                     None if r is None else C.byref(r), RO.addr(out), cap, RO.addr(cnt), None)

    def rows(off=0):
        b = RO.buf(48, off)
        b.view(DTYPE)[:] = table((0, 0, 1), (0, 2, 1))
        return b

    nin = lambda off=0: (lambda b: (b.view(np.int64).__setitem__(0, 2), b)[1])(RO.buf(8, off))
    who = "vad_refine_device: "
    faults = dict(tab=None, nin=None, in_cap=-2, tails=RO.buf(48, 8), ev=None, probs=None, start=None, n=-1, rule=None, out=None, cap=-1, cnt=None)
    RO.walk_one(lib, eng, device, faults, rules + (
        (INV, "n = -1, in_cap = -2: bad count", "n", 1 << 31),
        (INV, "n = 2147483648, in_cap = -2: bad count", "in_cap", 1 << 31),
        (INV, r"more than 2\^31 - 1 items", "n", 2),
        (INV, r"more than 2\^31 - 1 input records", "in_cap", 2),
        (INV, who + "null buffer$", "start", RO.i64(-1, 3, 2)),
        (INV, who + "null buffer$", "nin", nin(4)),
        (INV, who + "null buffer$", "cnt", RO.buf(8, 4)),
        (INV, who + "null buffer$", "tab", rows(8)),
        (INV, who + "null buffer$", "out", RO.buf(96, 8)),
        (INV, r"out_start\[0\] is negative", "start", RO.i64(0, 3, 2)),
        (INV, r"out_start decreases at item 1 \(2 after 3\)", "start", RO.i64(0, 3, 1 << 31)),
        (INV, r"more than 2\^31 - 1 frames in one call", "start", RO.i64(0, 3, 3)),
        (INV, who + "null buffer$", "ev", RO.buf(16, 8)),
        (INV, who + "null buffer$", "probs", RO.buf(16, 2)),
        (INV, "the events, the segment tables and the tails must be 16-byte aligned", "ev", RO.buf(16)),
        (INV, "the events, the segment tables and the tails must be 16-byte aligned", "tab", rows()),
        (INV, "the events, the segment tables and the tails must be 16-byte aligned", "tails", RO.buf(48)),
        (INV, "the events, the segment tables and the tails must be 16-byte aligned", "out", RO.buf(96)),
        (INV, who + "probs must be 4-byte aligned", "probs", RO.buf(16)),
        (INV, "the counts must be 8-byte aligned", "nin", nin()),
        (INV, "the counts must be 8-byte aligned", "cnt", RO.buf(8))))

    slots = eng.open_streams(2)
    count = np.full(1, -7, np.int64)

    def host(resident, tab, nin, tails, rule, out, cap, cnt):
        if resident:
            RO.resident(lib, eng, slots, resident)
        r = rule_struct(rule)
        return lib.vad_scan_refine(eng.handle, RO.segp(tab), nin, RO.segp(tails), None if r is None else C.byref(r), RO.segp(out), cap, RO.i64p(cnt))

    try:
        faults = dict(resident=None, tab=table((2, 0, 0), (0, 0, 0)), nin=-1, tails=np.zeros(2, DTYPE), rule=None, out=None, cap=-1, cnt=None)
        RO.walk_one(lib, eng, host, faults, rules + (
            (INV, "vad_scan_refine: null buffer$", "cnt", count),
            (INV, "vad_scan_refine: null buffer$", "out", RO.buf(96)),
            (INV, "vad_scan_refine: no scan results are resident: the engine's last vad_scan_segments or vad_scan_rate_segments failed, "
                  "or a later call has reused its per-frame arrays$", "resident", ((0.0, 0.0, 0.0), ())),
            (INV, "nsegs_in = -1: bad count", "nin", 2),
            (INV, "record 0 names item 2: the scan had 2 items", "tab", table((1, 0, 0), (0, 0, 0))),
            (INV, "record 0 has nframes = 0", "tab", table((1, 0, 1), (0, 0, 0))),
            (INV, r"the items decrease at record 1 \(0 after 1\)", "tab", table((0, 0, 1), (0, 2, 0))),
            (INV, "record 1 has nframes = 0", "tab", table((0, 0, 1), (0, 2, 1)))))
        assert count[0] == 2
        # a resident scan of no frames: no record, whatever the table
        count[0] = -7
        out = RO.buf(96)
        out[:] = SENT
        assert host(((), ()), table((0, 0, 1), (0, 2, 1)), 2, None, (0, 0, -1, 0, 0, 0), out, 4, count) == 0 and count[0] == 0 and untouched(out)
    finally:
        close(eng, slots)
