"""vad_resegment_device, vad_scan_resegment, Engine.resegment and sweep_recordings on the host side: exports, the equality with
vad_scan_segments on freshly opened streams for 1, 3, 8 and 64 threshold sets, rejected frames, item order and split channels,
truncation, the device form on every kind of engine against the oracle's state machine, the walk over everything that drops the
"results resident" mark, every refusal with its message and an untouched output, and what the call leaves alone - the real
csrc/engine.cpp over the HIP stand-in (tests/standin.py: p = |first sample of a frame|, so the audio scripts the probabilities;
the replay's stand-in runs the real sm_step).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import reseg_cases, reseg_ref, seg_ref, standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_resegment_device", "vad_scan_resegment"]
INV = _ffi.VAD_ERR_INVALID_ARG
SENT = 0x5A
# eight sets that differ in every one of the six fields; EMPTY starts nowhere (no scripted probability reaches 0.99)
EMPTY = (0.99, 0.98, 1.0, 1.0, 19, 60)
DEFAULTS = (0.7, 0.7, 0.8, 0.95, 10, 50)
BASE = [(0.5, 0.5, 0.8, 0.95, 2, 2), (0.6, 0.4, 0.7, 0.9, 3, 4), (0.8, 0.3, 0.5, 0.6, 1, 1), EMPTY, DEFAULTS, (0.3, 0.2, 0.9, 0.85, 4, 3),
        (0.55, 0.45, 0.6, 0.75, 5, 6), (0.65, 0.35, 0.75, 1.0, 2, 8)]
SCAN_THR = (0.62, 0.41, 0.66, 0.77, 3, 5)          # what the scan itself runs with: none of the sets


def sets_of(nt):
    """nt sets: the base ones, then variations of them in all six fields"""
    out = []
    for k in range(nt):
        a, b, c, d, m, n = BASE[k % 8]
        j = k // 8
        out.append((a - 0.011 * j, b - 0.007 * j, max(c - 0.03 * j, 0.1), max(d - 0.02 * j, 0.1), m + j % 3, n + j % 4))
    return out


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
def aligned(n, dtype, fill=None, off=0):
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 32, np.uint8)
    a = raw[(-raw.ctypes.data) % 16 + off:][:n * item].view(dtype)
    assert a.ctypes.data % 16 == off
    if fill is not None:
        a.view(np.uint8)[:] = fill
    return a


def untouched(a):
    return a is None or bool((a.view(np.uint8) == SENT).all())


def thr_array(sets):
    return None if sets is None else (_ffi.Thresholds * max(1, len(sets)))(*[_ffi.Thresholds(*s) for s in sets])


def raw_reseg(lib, eng, sets, cap, nt=None, tab="own", start="own"):
    """vad_scan_resegment -> (rc, message, table buffer, set_start buffer), both pre-filled with a sentinel"""
    nt = len(sets) if nt is None else nt
    if isinstance(tab, str):
        tab = aligned(max(min(cap, 1 << 16), 0) + 2, seg_ref.DTYPE, SENT)
    if isinstance(start, str):
        start = aligned(max(nt, 0) + 2, np.int64, SENT)
    rc = lib.vad_scan_resegment(eng.handle, thr_array(sets), nt, None if tab is None else tab.ctypes.data_as(C.POINTER(_ffi.Segment)), cap,
                                None if start is None else start.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, lib.vad_last_error(eng.handle).decode(), tab, start


def script(p, frame, hop, tail=3):
    """a float32 recording whose frame t begins with p[t] - the stand-in's probability of that frame - and whose last `tail`
    samples no frame holds"""
    x = np.zeros((len(p) - 1) * hop + frame + tail if len(p) else 0, np.float32)
    x[np.arange(len(p)) * hop] = p
    return x


def speechy(rng, nframes):
    """probabilities in runs: speech (0.5 .. 0.95) and silence (0 .. 0.45) of 1 .. 12 frames, so that segments start, end and
    start again under the base sets"""
    p = []
    voiced = bool(rng.integers(2))
    while len(p) < nframes:
        run = int(rng.integers(1, 13))
        p += list(rng.uniform(0.5, 0.95, run) if voiced else rng.uniform(0.0, 0.45, run))
        voiced = not voiced
    return np.asarray(p[:nframes], np.float32)


def corpus(frame, hop, seed=5):
    """40 recordings of 0 .. 60 frames: 0 and 1 among them, one shorter than a frame, every one with a tail that framing drops"""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, 60, 2, 59] + [int(v) for v in rng.integers(3, 59, 35)]
    recs = [script(speechy(rng, n), frame, hop) for n in lengths]
    recs[0] = np.zeros(frame - 8, np.float32)              # samples, but no frame
    return recs


def fresh_tables(make_engine, sets, recs, hop, shape=None, **kw):
    """what the issue's contract names: scan_segments on freshly opened streams whose thresholds are the set, per set"""
    twin = make_engine()
    out = []
    n = len(recs) * (2 if shape == "split" else 1)
    for s in sets:
        slots = np.asarray(twin.open_streams(n))
        try:
            twin.set_thresholds_many(slots, s)
            out.append(twin.scan_segments(slots.reshape(len(recs), 2) if shape == "split" else slots, recs, hop=hop, **kw))
        finally:
            for k in slots:
                twin.close_stream(int(k))
    return out


def scan_then(eng, recs, hop, shape=None, dirty=False, **kw):
    """the scan whose results the replay reads, on thresholds of its own -> the slots (the caller closes them)"""
    n = len(recs) * (2 if shape == "split" else 1)
    slots = np.asarray(eng.open_streams(n))
    eng.set_thresholds_many(slots, SCAN_THR)
    sl = slots.reshape(len(recs), 2) if shape == "split" else slots
    if dirty:           # the slots come out of an earlier call inside a segment: the replay starts every recording afresh all the same
        head = [script([0.9] * 7, eng.frame_samples, hop) for _ in recs]
        if shape == "split":
            head = [np.ascontiguousarray(np.stack([h, h], axis=1)) for h in head]
        eng.scan_segments(sl, head, hop=hop, **kw)
    eng.scan_segments(sl, recs, hop=hop, **kw)
    return slots


def check_equal(eng, sets, want):
    got = eng.resegment(sets)
    assert len(got) == len(sets) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert seg_ref.same(np.ascontiguousarray(g), w), (k, sets[k], len(g), len(w))
        assert len(g) == 0 or int(g["first_frame"].min()) >= 0
    return got


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header and "#define VAD_RESEGMENT_MAX_SETS 64" in header
    proto = lambda name: re.sub(r"/\*.*?\*/", "", re.search(r"VAD_API int %s\((.*?)\);" % name, header, re.S).group(1))
    assert len(proto("vad_resegment_device").split(",")) == len(_ffi.SIGNATURES["vad_resegment_device"][1]) == 11
    assert len(proto("vad_scan_resegment").split(",")) == len(_ffi.SIGNATURES["vad_scan_resegment"][1]) == 6
    import cutter_vad_amd
    from cutter_vad_amd.scan import sweep_recordings
    assert cutter_vad_amd.sweep_recordings is sweep_recordings and "sweep_recordings" in cutter_vad_amd.__all__
    from cutter_vad_amd import _build
    assert "scan_resegment.hip" in _build.HIP_SOURCES


# ---- the equality -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh64(make_engine):
    """the 64 sets' fresh scans of the corpus, once"""
    frame = 512
    recs = corpus(frame, frame)
    return recs, sets_of(64), fresh_tables(make_engine, sets_of(64), recs, frame, denoise=None)


@pytest.mark.parametrize("nt", [1, 3, 8, 64])
def test_every_set_s_table_equals_the_scan_of_fresh_streams_with_that_set(lib, make_engine, fresh64, nt):
    recs, sets, want = fresh64
    pick = [0, 1, 3] if nt == 3 else list(range(nt))
    sets, want = [sets[k] for k in pick], [want[k] for k in pick]
    # not vacuous, by the fresh scans alone: sets with segments, pairwise different tables, and (from three sets on) an empty one
    full = [k for k, w in enumerate(want) if len(w)]
    assert len(full) >= min(3, nt - (nt >= 3))
    assert len({want[k].tobytes() for k in full}) == len(full) or nt == 64
    if nt >= 8:
        assert len({want[k].tobytes() for k in full}) >= 6 and sum(len(want[k]) for k in full) > 100
    assert nt < 3 or any(len(w) == 0 for w in want)
    assert any(len(set(w["item"].tolist())) < len(w) for w in want)              # a recording whose segments start again
    eng = make_engine()
    slots = scan_then(eng, recs, 512, dirty=(nt == 8), denoise=None)
    try:
        check_equal(eng, sets, want)
        rc, msg, tab, start = raw_reseg(lib, eng, sets, 1 << 15)
        assert rc == 0, msg
        assert start[:nt + 1].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and untouched(start[nt + 1:])
        total = int(start[nt])
        assert tab[:total].tobytes() == b"".join(w.tobytes() for w in want) and untouched(tab[total:])
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_rejected_frames_are_skipped_and_enter_no_statistic(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    p = [0.0] * 2 + [0.9, 0.6, 0.9, 0.7, 0.9, 0.8] + [0.0] * 6 + [0.9] * 4 + [0.0] * 5
    a = script(p, frame, hop)
    b = a.copy()
    b[4 * hop + 17] = np.nan                      # inside a segment
    b[6 * hop + 5] = np.inf
    c = a.copy()
    c[1 * hop + 9] = np.nan                       # before a START
    c[(len(p) - 1) * hop + 3] = np.nan            # the recording's last frame
    d = script([0.9, 0.9, 0.9], frame, hop)
    d[2 * hop] = np.nan                           # a last frame that would have continued the run
    recs = [a, b, c, d]
    sets = [BASE[0], BASE[2], BASE[5], EMPTY]
    want = fresh_tables(make_engine, sets, recs, hop, denoise=None)
    slots = scan_then(eng, recs, hop, denoise=None)
    try:
        got = check_equal(eng, sets, want)
        t0 = got[0]
        assert sorted(set(t0["item"].tolist())) == [0, 1, 2]
        clean, holed = t0[t0["item"] == 0][0], t0[t0["item"] == 1][0]
        assert holed["first_frame"] <= 4 and holed["first_frame"] + holed["nframes"] > 6
        assert clean["counted"] == clean["nframes"] and holed["counted"] < clean["counted"] and np.isfinite(holed["mean_prob"])
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("shape", ["unsorted", "split"])
def test_item_order_is_the_call_s_whatever_the_lengths(lib, make_engine, shape):
    eng = make_engine()
    frame = hop = eng.frame_samples
    rng = np.random.default_rng(11)
    lengths = [7, 41, 0, 23, 58, 1, 33, 12]                # not their length order: the scan sorts its table, the replay must not
    sets = [BASE[0], BASE[1], BASE[2], BASE[5], EMPTY]
    if shape == "split":
        recs = [np.ascontiguousarray(np.stack([script(speechy(rng, n), frame, hop), script(speechy(rng, n), frame, hop)], axis=1)) for n in lengths]
        kw = dict(channel="split", denoise=None)
    else:
        recs = [script(speechy(rng, n), frame, hop) for n in lengths]
        kw = dict(denoise=None)
    sh = "split" if shape == "split" else None
    want = fresh_tables(make_engine, sets, recs, hop, shape=sh, **kw)
    slots = scan_then(eng, recs, hop, shape=sh, **kw)
    try:
        got = check_equal(eng, sets, want)
        items = got[0]["item"].tolist()
        assert items == sorted(items) and len(set(items)) >= 4
        if shape == "split":
            assert {i % 2 for i in items} == {0, 1}        # item = 2 i + c: both channels have segments of their own
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_truncation_keeps_the_counts_and_writes_the_first_records(lib, make_engine, fresh64):
    recs, sets, want = fresh64
    sets, want = sets[:8], want[:8]
    whole = np.concatenate(want)
    counts = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    total = int(counts[-1])
    inside_set_1 = int(counts[1]) + max(1, len(want[1]) // 2)
    assert counts[1] < inside_set_1 < counts[2]
    eng = make_engine()
    slots = scan_then(eng, recs, 512, denoise=None)
    try:
        for cap in (0, 1, inside_set_1, total, total + 5):
            rc, msg, tab, start = raw_reseg(lib, eng, sets, cap)
            assert rc == 0, msg
            assert start[:9].tolist() == counts.tolist() and untouched(start[9:])
            k = min(cap, total)
            assert tab[:k].tobytes() == whole[:k].tobytes() and untouched(tab[k:]), cap
        rc, msg, _, start = raw_reseg(lib, eng, sets, 0, tab=None)       # seg_cap = 0 needs no table
        assert rc == 0 and int(start[8]) == total, msg
    finally:
        for s in slots:
            eng.close_stream(int(s))


# ---- the device form --------------------------------------------------------------------------------------------------
def device_arrays(rng, total):
    """hand-built CSR arrays: speechy probabilities, a few rejected frames, and START / END / CONTINUE bits that mean nothing"""
    probs = speechy(rng, total)
    ev = aligned(total, np.uint8)
    ev[:] = rng.choice([0, 1, 2, 4, 6], total).astype(np.uint8)
    bad = rng.random(total) < 0.03
    ev[bad] |= 0x80
    probs[bad] = np.nan
    return ev, probs


def raw_device(lib, eng, ev, probs, start, sets, cap, nt=None, n=None, tab="own", set_start="own"):
    nt = len(sets) if nt is None else nt
    if isinstance(tab, str):
        tab = aligned(max(min(cap, 1 << 16), 0) + 2, seg_ref.DTYPE, SENT)
    if isinstance(set_start, str):
        set_start = aligned(max(nt, 0) + 2, np.int64, SENT)
    ptr = lambda a: None if a is None else a.ctypes.data
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    rc = lib.vad_resegment_device(eng.handle, ptr(ev), ptr(probs), None if st is None else st.ctypes.data_as(C.POINTER(C.c_int64)),
                                  (st.size - 1 if n is None else n), thr_array(sets), nt, ptr(tab), cap, ptr(set_start), None)
    if rc == 0:
        eng.synchronize()
    return rc, lib.vad_last_error(eng.handle).decode(), tab, set_start


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_replays_on_device_pointers(lib, make_engine, kw):
    eng = make_engine(**kw)
    rng = np.random.default_rng(21)
    total = 700
    ev, probs = device_arrays(rng, total)
    sets = [BASE[0], BASE[1], BASE[2], EMPTY, BASE[5]]
    for start in ([0, 90, 90, 400, 401, 700], [37, 160, 420, 655]):           # the second: out_start[0] > 0, and a tail no item owns
        want = reseg_ref.tables(ev, probs, start, sets)
        assert sum(1 for w in want if len(w)) >= 3 and len(want[3]) == 0
        counts = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        total_rec = int(counts[-1])
        for cap in (total_rec + 3, total_rec // 2, 0):
            rc, msg, tab, set_start = raw_device(lib, eng, ev, probs, start, sets, cap)
            assert rc == 0, msg
            assert set_start[:6].tolist() == counts.tolist() and untouched(set_start[6:])
            k = min(cap, total_rec)
            assert tab[:k].tobytes() == np.concatenate(want)[:k].tobytes() and untouched(tab[k:]), (kw, start, cap)
    # no frames, no items: the counts alone, all zero
    for st, n in (([0, 0, 0], None), ([5], None), (None, 0)):
        rc, msg, tab, set_start = raw_device(lib, eng, None, None, st, sets, 4, n=n)
        assert rc == 0 and set_start[:6].tolist() == [0] * 6 and untouched(tab), msg


@pytest.mark.parametrize("n,nsets", [(n, 5) for n in reseg_cases.NS] + [(257, 1), (257, 64)])
def test_tables_past_a_wave_and_a_workgroup(lib, make_engine, n, nsets):
    """the GPU suite's hand-built arrays (tests/reseg_cases.py) with every condition they are for asserted on the reference, and the
    stand-in's tables at their caps"""
    eng = make_engine()
    ev0, probs, start, sets, want, (counts, caps) = reseg_cases.built(n, nsets)
    ev = aligned(len(ev0), np.uint8)
    ev[:] = ev0
    whole = np.concatenate(want)
    for cap in caps:
        rc, msg, tab, set_start = raw_device(lib, eng, ev, probs, start, sets, cap)
        assert rc == 0, msg
        assert set_start[:len(sets) + 1].tolist() == counts.tolist() and untouched(set_start[len(sets) + 1:])
        k = min(cap, len(whole))
        assert tab[:k].tobytes() == whole[:k].tobytes() and untouched(tab[k:]), (n, nsets, cap)


def test_device_form_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    rng = np.random.default_rng(3)
    ev, probs = device_arrays(rng, 500)
    start = [0, 200, 200, 500]
    sets = [BASE[0], BASE[1]]

    def refused(pattern, ev=ev, probs=probs, start=start, sets=sets, cap=100, **kw):
        rc, msg, tab, set_start = raw_device(lib, eng, ev, probs, start, sets, cap, **kw)
        assert rc == INV, (rc, msg)
        assert msg.startswith("Model prediction failed: vad_resegment_device: ") and re.search(pattern, msg), msg
        assert untouched(tab) and untouched(set_start)

    refused("nt = 0: 1 .. 64 threshold sets", nt=0)
    refused("nt = -2: 1 .. 64 threshold sets", nt=-2)
    refused("nt = 65: 1 .. 64 threshold sets", sets=sets_of(65))
    refused("seg_cap = -1: bad count", cap=-1)
    refused("null buffer", sets=None, nt=2)
    refused("n = -1: bad count", n=-1)
    refused("more than 2\\^31 - 1 replays", n=(1 << 30), sets=sets_of(3))
    refused("null buffer", start=None, n=3)
    refused("null buffer", set_start=None)
    refused("null buffer", tab=None)
    refused("null buffer", ev=None)
    refused("null buffer", probs=None)
    refused("out_start\\[0\\] is negative", start=[-4, 200, 200, 500])
    refused("out_start decreases at item 1 \\(100 after 200\\)", start=[0, 200, 100, 500])
    refused("more than 2\\^31 - 1 frames", start=[0, 200, 200, 1 << 31])
    for off in (1, 4, 8):
        e2 = aligned(500, np.uint8, off=off)
        e2[:] = ev
        refused("events and the segment table must be 16-byte aligned", ev=e2)
    refused("must be 16-byte aligned", tab=aligned(102, seg_ref.DTYPE, SENT, off=8))
    raw = aligned(4 * 500 + 2, np.uint8)[2:2 + 4 * 500]
    refused("probs must be 4-byte aligned", probs=raw.view(np.float32))
    cnt = aligned(7, np.int32, SENT)[1:7].view(np.int64)
    assert cnt.ctypes.data % 8 == 4
    refused("the set counts must be 8-byte aligned", set_start=cnt)
    assert lib.vad_resegment_device(None, None, None, None, 0, None, 1, None, 0, None, None) == INV
    rc, msg, _, set_start = raw_device(lib, eng, ev, probs, start, sets, 0, tab=None)       # seg_cap = 0 needs no table
    assert rc == 0 and set_start[2] > 0, msg


# ---- the mark ---------------------------------------------------------------------------------------------------------
def test_whatever_writes_the_per_frame_arrays_drops_the_mark(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = [script([0.0] * 2 + [0.9] * 6 + [0.0] * 6, frame, hop), script([0.9] * 5 + [0.0] * 4, frame, hop)]
    sets = [BASE[0], BASE[2]]
    gone = "vad_scan_resegment: no scan results are resident"

    def refused():
        rc, msg, tab, start = raw_reseg(lib, eng, sets, 8)
        assert rc == INV and gone in msg and msg.startswith("Model prediction failed: ") and untouched(tab) and untouched(start), (rc, msg)

    refused()                                               # a fresh engine
    slots = np.asarray(eng.open_streams(2))
    extra = int(eng.open_stream())
    want = None
    try:
        def rescan():
            nonlocal want
            eng.reset(slots)
            eng.set_thresholds_many(slots, SCAN_THR)
            eng.scan_segments(slots, recs, hop=hop, denoise=None)
            got = eng.resegment(sets)
            assert want is None or all(seg_ref.same(np.ascontiguousarray(g), w) for g, w in zip(got, want))
            want = [np.ascontiguousarray(g) for g in got]
            assert len(want[0]) == 2 and len(want[1]) >= 2

        writers = {
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
            refused()
        # a vad_scan_segments that fails its checks leaves no results either
        rescan()
        with pytest.raises(Exception, match="hop"):
            eng.scan_segments(slots, recs, hop=6, denoise=None)
        refused()
        # calls that write neither array keep the mark: a cut of the resident block, the table's read, thresholds, a replay
        rescan()
        eng.cut([(0, int(want[0][0]["first_frame"]), int(want[0][0]["nframes"]))], hop=hop, denoise=None)
        eng.set_thresholds_many(slots, BASE[1])
        one = aligned(1, seg_ref.DTYPE)
        assert lib.vad_scan_segments_read(eng.handle, 0, 1, one.ctypes.data_as(C.POINTER(_ffi.Segment))) == 0
        assert all(seg_ref.same(np.ascontiguousarray(g), w) for g, w in zip(eng.resegment(sets), want))
        # an empty corpus is a valid, empty result
        for empty in ([np.zeros(0, np.float32), np.zeros(100, np.float32)], []):
            eng.scan_segments(slots[:len(empty)], empty, hop=hop, denoise=None)
            rc, msg, tab, start = raw_reseg(lib, eng, sets, 8)
            assert rc == 0 and start[:3].tolist() == [0, 0, 0] and untouched(start[3:]) and untouched(tab), msg
            assert [len(t) for t in eng.resegment(sets)] == [0, 0]
    finally:
        for s in list(slots) + [extra]:
            eng.close_stream(int(s))


# ---- refusals, and what a call leaves alone ---------------------------------------------------------------------------
def test_refusals_have_a_message_and_a_call_leaves_the_engine_as_it_was(lib, make_engine, fresh64):
    recs, sets, want = fresh64
    sets, want = sets[:8], want[:8]
    eng = make_engine()
    slots = scan_then(eng, recs, 512, denoise=None)
    try:
        def refused(pattern, sets=sets, cap=100, **kw):
            rc, msg, tab, start = raw_reseg(lib, eng, sets, cap, **kw)
            assert rc == INV, (rc, msg)
            assert msg.startswith("Model prediction failed: vad_scan_resegment: ") and re.search(pattern, msg), msg
            assert untouched(tab) and untouched(start)

        refused("nt = 0: 1 .. 64 threshold sets", nt=0)
        refused("nt = -1: 1 .. 64 threshold sets", nt=-1)
        refused("nt = 65: 1 .. 64 threshold sets", sets=sets_of(65))
        refused("seg_cap = -3: bad count", cap=-3)
        refused("null buffer", sets=None, nt=8)
        refused("null buffer", start=None)
        refused("null buffer", tab=None)
        assert lib.vad_scan_resegment(None, None, 1, None, 0, None) == INV
        # the scan's own table, the streams and the counters before ...
        own = aligned(1 << 12, seg_ref.DTYPE)
        read = lambda out, k: lib.vad_scan_segments_read(eng.handle, 0, k, out.ctypes.data_as(C.POINTER(_ffi.Segment)))
        nown = 0
        while read(own, nown + 1) == 0:
            nown += 1
        assert nown > 10 and read(own, nown) == 0
        before = own[:nown].tobytes()
        saved = [eng.save_stream(int(s)) for s in slots]
        info = eng.info()
        last = dict(eng.last_scan)
        check_equal(eng, sets, want)
        # ... and after: nothing moved, and the resident block still cuts
        assert [eng.save_stream(int(s)) for s in slots] == saved
        assert (eng.info()["steps"], eng.info()["frames"]) == (info["steps"], info["frames"])
        again = aligned(1 << 12, seg_ref.DTYPE)
        assert read(again, nown) == 0 and again[:nown].tobytes() == before and read(again, nown + 1) == INV
        assert eng.last_scan.keys() == last.keys() and eng.last_scan["samples"] == last["samples"]
        t = want[0]
        offs = eng.last_scan["offsets"]
        pcm, where = eng.cut([(int(offs[i]), int(f), int(n)) for i, f, n in zip(t["item"], t["first_frame"], t["nframes"])], hop=512, denoise=None)
        assert pcm.size == 512 * int(t["nframes"].sum()) and np.abs(pcm).max() > 1000 and where[-1] == pcm.size
    finally:
        for s in slots:
            eng.close_stream(int(s))


# ---- sweep_recordings -------------------------------------------------------------------------------------------------
def test_sweep_recordings_is_scan_recordings_per_config(lib, make_engine):
    from cutter_vad_amd import ConfigurationError, VADConfig, scan_recordings, sweep_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(2)
    mono = lambda n: script(speechy(rng, n), frame, hop)
    st = lambda n: np.ascontiguousarray(np.stack([mono(n), mono(n)], axis=1))
    recs = [mono(40), st(55), mono(0), st(31), np.zeros((0, 2), np.float32), mono(58), mono(1)]
    cfg = lambda s, **kw: VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=s[0], vad_end_probability=s[1],
                                    voice_start_ratio=s[2], voice_end_ratio=s[3], voice_start_frame_count=s[4], voice_end_frame_count=s[5],
                                    **{"enable_denoising": False, **kw})
    cfgs = [cfg(s) for s in (BASE[0], BASE[1], BASE[2], EMPTY, BASE[5])]
    calls = []
    real = eng.scan_segments
    eng.scan_segments = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for channel in ("mix", 1, "split"):
            calls.clear()
            got = sweep_recordings(recs, cfgs, engine=eng, hop=hop, channel=channel, stats=True)
            assert len(calls) == 2                        # one scan per kind of recording, whatever the number of configs
            want = [scan_recordings(recs, c, engine=eng, hop=hop, channel=channel, stats=True) for c in cfgs]
            assert got == want
            flat = lambda res: [s for r in res for lst in (r if channel == "split" else [r]) for s in (lst if channel == "split" else [lst])]
            sizes = [sum(len(x) for x in flat(w)) for w in want]
            assert sizes[3] == 0 and min(sizes[:3]) > 3 and len({repr(w) for w in want}) == 5
        assert sweep_recordings(recs, cfgs, engine=eng, hop=hop) == [scan_recordings(recs, c, engine=eng, hop=hop) for c in cfgs]
    finally:
        del eng.scan_segments
    assert sweep_recordings(recs, [], engine=eng) == [] and sweep_recordings([], cfgs, engine=eng) == [[]] * 5
    with pytest.raises(ConfigurationError, match="enable_denoising"):
        sweep_recordings(recs, [cfgs[0], cfg(BASE[1], enable_denoising=True)], engine=eng, hop=hop)
    with pytest.raises(ConfigurationError, match="buffer_size"):
        sweep_recordings(recs, [cfgs[0], cfgs[1].model_copy(update={"buffer_size": 256})], engine=eng, hop=hop)


def _hipcc():
    import shutil
    return next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_the_kernel_file_compiles_without_scratch_or_spills(tmp_path):
    """count, prefix and fill keep their state machine in registers: from the compiler's own metadata"""
    import subprocess
    from cutter_vad_amd import _build
    out = tmp_path / "scan_resegment.s"
    subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "cutter_vad_amd", "csrc", "scan_resegment.hip")], check=True, capture_output=True, timeout=600)
    meta = re.findall(r"\.name:\s*(_Z\d+vadk_reseg_\w+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                      out.read_text(), re.S)
    assert {m[0].split("vadk_reseg_")[1][:4] for m in meta} == {"coun", "pref", "fill"} and len(meta) == 3, meta
    for name, scratch, sspill, vspill in meta:
        assert (scratch, sspill, vspill) == ("0", "0", "0"), (name, scratch, sspill, vspill)


# ---- the order of the refusals ----------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, make_engine):
    """The order of the checks is behaviour.  vad_resegment_device: the sets, seg_cap and the null sets; n; n x nt; the null
    arguments; the positions; the null per-frame arrays; the 16-, 4- and 8-byte alignments.  vad_scan_resegment: the sets, the null
    arguments, then the resident results.  Every fault at once, then one mended at a time; and a resident scan without a frame."""
    from tests import refusal_order as RO
    eng = make_engine()
    two = [BASE[0], BASE[1]]

    def device(ev, probs, start, n, sets, nt, segs, cap, set_start):
        return lib.vad_resegment_device(eng.handle, RO.addr(ev), RO.addr(probs), RO.i64p(start), n, RO.thr(sets), nt, RO.addr(segs), cap,
                                        RO.addr(set_start), None)

    faults = dict(ev=None, probs=None, start=None, n=-1, sets=None, nt=0, segs=None, cap=-1, set_start=None)
    RO.walk_one(lib, eng, device, faults, (
        (INV, r"nt = 0: 1 \.\. 64 threshold sets", "nt", 2),
        (INV, "seg_cap = -1: bad count", "cap", 4),
        (INV, "vad_resegment_device: null buffer$", "sets", two),
        (INV, "n = -1: bad count", "n", 1 << 31),
        (INV, r"2147483648 items x 2 sets: more than 2\^31 - 1 replays", "n", 2),
        (INV, "vad_resegment_device: null buffer$", "start", RO.i64(-1, 3, 2)),
        (INV, "vad_resegment_device: null buffer$", "set_start", RO.buf(24, 4)),
        (INV, "vad_resegment_device: null buffer$", "segs", RO.buf(96, 8)),
        (INV, r"out_start\[0\] is negative", "start", RO.i64(0, 3, 2)),
        (INV, r"out_start decreases at item 1 \(2 after 3\)", "start", RO.i64(0, 3, 1 << 31)),
        (INV, r"more than 2\^31 - 1 frames in one call", "start", RO.i64(0, 3, 3)),
        (INV, "vad_resegment_device: null buffer$", "ev", RO.buf(16, 8)),
        (INV, "vad_resegment_device: null buffer$", "probs", RO.buf(16, 2)),
        (INV, "the events and the segment table must be 16-byte aligned", "ev", RO.buf(16)),
        (INV, "the events and the segment table must be 16-byte aligned", "segs", RO.buf(96)),
        (INV, "vad_resegment_device: probs must be 4-byte aligned", "probs", RO.buf(16)),
        (INV, "the set counts must be 8-byte aligned", "set_start", RO.buf(24))))

    slots = eng.open_streams(2)
    set_start = np.full(3, -7, np.int64)

    def host(resident, sets, nt, segs, cap, set_start):
        if resident:
            RO.resident(lib, eng, slots, resident)
        return lib.vad_scan_resegment(eng.handle, RO.thr(sets), nt, RO.segp(segs), cap, RO.i64p(set_start))

    try:
        RO.walk_one(lib, eng, host, dict(resident=None, sets=None, nt=65, segs=None, cap=-1, set_start=None), (
            (INV, r"nt = 65: 1 \.\. 64 threshold sets", "nt", 2),
            (INV, "seg_cap = -1: bad count", "cap", 4),
            (INV, "vad_scan_resegment: null buffer$", "sets", two),
            (INV, "vad_scan_resegment: null buffer$", "set_start", set_start),
            (INV, "vad_scan_resegment: null buffer$", "segs", RO.buf(96)),
            (INV, "vad_scan_resegment: no scan results are resident: the engine's last vad_scan_segments or vad_scan_rate_segments failed, "
                  "or a later call has reused its per-frame arrays$", "resident", ((0.0, 0.0, 0.0), ()))))
        assert set_start.tolist() == [0, 0, 0]
        # a resident scan of no frames: all-zero counts, the table untouched
        set_start[:] = -7
        segs = RO.buf(96)
        segs[:] = SENT
        assert host(((), ()), two, 2, segs, 4, set_start) == 0 and set_start.tolist() == [0, 0, 0] and untouched(segs)
    finally:
        for s in slots:
            eng.close_stream(int(s))
