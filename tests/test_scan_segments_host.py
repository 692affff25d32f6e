"""vad_segments_device, vad_scan_segments and vad_scan_segments_read on the host side: exports and the record's layout, every
refusal with its message and an untouched output, V4 and shared-GPU engines, scripted recordings in every wire format x channel
mode x hop against Engine.scan on a twin engine and the numpy reference of tests/seg_ref.py, truncation and the retained table,
a segment that began before its recording, rejected frames, and the Python faces - the real csrc/engine.cpp over the HIP stand-in
(tests/standin.py: tools/san_tick/fake_kernels.cpp restates the kernels' arithmetic in plain C++; p = |first sample of a frame|, so
the audio scripts the events).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.scan import segment_ranges, speech_segments
from tests import g711_ref as G
from tests import seg_ref, standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_segments_device", "vad_scan_segments", "vad_scan_segments_read"]
INV, UNSUP = _ffi.VAD_ERR_INVALID_ARG, _ffi.VAD_ERR_UNSUPPORTED
THR = (0.5, 0.5, 0.8, 0.95, 2, 2)
SENT = 0x5A


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
    """n items of dtype whose first byte lies `off` bytes behind a 16-byte boundary"""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 32, np.uint8)
    a = raw[(-raw.ctypes.data) % 16 + off:][:n * item].view(dtype)
    assert a.ctypes.data % 16 == off
    if fill is not None:
        a.view(np.uint8)[:] = fill
    return a


def raw_segments(lib, eng, ev, seg, probs, start, cap, segs="own", nsegs="own", n=None):
    """vad_segments_device on host memory (the stand-in's device memory) -> (rc, message, table buffer, count buffer), both
    pre-filled with a sentinel"""
    if isinstance(segs, str):
        segs = aligned(max(min(cap, 1 << 16), 0) + 2, seg_ref.DTYPE, SENT)
    if isinstance(nsegs, str):
        nsegs = aligned(1, np.int64, SENT)
    ptr = lambda a: None if a is None else a.ctypes.data
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    rc = lib.vad_segments_device(eng.handle, ptr(ev), ptr(seg), ptr(probs), None if st is None else st.ctypes.data_as(C.POINTER(C.c_int64)),
                                 (st.size - 1 if n is None else n), ptr(segs), cap, ptr(nsegs), None)
    if rc == 0:
        eng.synchronize()
    return rc, lib.vad_last_error(eng.handle).decode(), segs, nsegs


def untouched(a):
    return a is None or bool((a.view(np.uint8) == SENT).all())


def flat_arrays(rng, total, p_end=0.05):
    """hand-built CSR arrays: any pattern is legal input of the extraction"""
    ev = aligned(total, np.uint8)
    ev[:] = np.where(rng.random(total) < p_end, 0x02, rng.choice([0, 1, 4, 0x80, 0x82], total)).astype(np.uint8)
    seg = np.where(ev == 0x02, rng.integers(1, 40, total), 0).astype(np.int32)
    probs = np.where(ev & 0x80, np.float32(np.nan), rng.random(total, np.float32)).astype(np.float32)
    return ev, seg, probs


def encode(x, kind):
    if kind == "f32":
        return x.astype(np.float32)
    if kind == "i16":
        return np.round(x * 32767.0).astype(np.int16)
    return G.encode(x, kind)


def script(p, frame, hop, kind):
    """a recording whose frame t begins with a sample that decodes to about p[t]: the stand-in's probability of that frame"""
    x = np.zeros((len(p) - 1) * hop + frame + 3 if len(p) else 0, np.float64)
    x[np.arange(len(p)) * hop] = p
    return encode(x, kind)


def stereo(left, right, frame, hop, kind):
    """[nsamples, 2]: the two scripts side by side, the shorter one padded with silence"""
    n = max(len(left), len(right))
    return np.ascontiguousarray(np.stack([script(list(p) + [0.0] * (n - len(p)), frame, hop, kind) for p in (left, right)], axis=1))


ONE = [0.0] * 2 + [0.9] * 5 + [0.0] * 6
TWO = [0.9] * 4 + [0.0] * 4 + [0.8, 0.9, 0.7] + [0.0] * 5
THREE = ONE + TWO
NONE = [0.0] * 9
LAW = {"ulaw": "ulaw", "alaw": "alaw"}


def flatten(per_item):
    """the per-recording arrays of Engine.scan ([nf], or [2, nf] for 'split') -> (flat, out_start), in the call's item order"""
    rows = [r for a in per_item for r in (list(a) if np.asarray(a).ndim == 2 else [a])]
    start = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return (np.concatenate(rows) if rows else np.zeros(0, per_item[0].dtype if per_item else np.uint8)), start, rows


def twin_table(twin, slots, recs, frame, hop, **kw):
    """Engine.scan on the twin -> (seg_ref's table, per item: speech_segments' ranges)"""
    probs, ev, seg = twin.scan(slots, recs, hop=hop, **kw)
    fp, start, _ = flatten(probs)
    fe, _, erows = flatten(ev)
    fs, _, srows = flatten(seg)
    return seg_ref.table(fe, fs, fp, start), [speech_segments(e, g, frame, hop) for e, g in zip(erows, srows)]


def by_item(table, nitems, frame, hop):
    out = [[] for _ in range(nitems)]
    for it, rg in zip(table["item"].tolist(), segment_ranges(table, frame, hop)):
        out[it].append(rg)
    return out


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header
    m = re.search(r"typedef struct vad_segment \{(.*?)\} vad_segment;", header, re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))
    assert fields == [("int32_t", "item"), ("int32_t", "first_frame"), ("int32_t", "nframes"), ("int32_t", "counted"),
                      ("float", "mean_prob"), ("float", "max_prob")]
    assert C.sizeof(_ffi.Segment) == 24 and _ffi.SEGMENT_DTYPE.itemsize == 24 and seg_ref.DTYPE.itemsize == 24
    assert [f[0] for f in _ffi.Segment._fields_] == [f[1] for f in fields] == list(_ffi.SEGMENT_DTYPE.names)
    assert [getattr(_ffi.Segment, f[1]).offset for f in fields] == [_ffi.SEGMENT_DTYPE.fields[f[1]][1] for f in fields] == [0, 4, 8, 12, 16, 20]
    assert _ffi.SEGMENT_DTYPE == seg_ref.DTYPE
    import cutter_vad_amd
    assert cutter_vad_amd.segment_ranges is segment_ranges and "segment_ranges" in cutter_vad_amd.__all__


# ---- vad_segments_device ----------------------------------------------------------------------------------------------
def test_segments_device_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    rng = np.random.default_rng(1)
    total = 5000
    ev, seg, probs = flat_arrays(rng, total)
    start = [0, 1200, 1200, 5000]
    rc, msg, segs, nsegs = raw_segments(lib, eng, ev, seg, probs, start, 1000)
    want = seg_ref.table(ev, seg, probs, start)
    assert rc == 0 and int(nsegs[0]) == len(want) > 100 and seg_ref.same(segs[:len(want)].copy(), want) and untouched(segs[len(want):]), msg

    def refused(pattern, ev=ev, seg=seg, probs=probs, start=start, cap=1000, **kw):
        rc, msg, segs, nsegs = raw_segments(lib, eng, ev, seg, probs, start, cap, **kw)
        assert rc == INV, (rc, msg)
        assert msg.startswith("Model prediction failed: vad_segments_device: ") and re.search(pattern, msg), msg
        assert untouched(segs) and untouched(nsegs)

    refused("n = -1, seg_cap = 1000: bad count", n=-1)
    refused("n = 3, seg_cap = -1: bad count", cap=-1)
    refused("null buffer", ev=None)
    refused("null buffer", seg=None)
    refused("null buffer", probs=None)
    refused("null buffer", start=None, n=3)
    refused("null buffer", segs=None)
    refused("null buffer", nsegs=None)
    refused("out_start\\[0\\] is negative", start=[-4, 1200, 1200, 5000])
    refused("out_start decreases at item 1 \\(1100 after 1200\\)", start=[0, 1200, 1100, 5000])
    refused("more than 2\\^31 - 1 frames", start=[0, 1200, 1200, 1 << 31])
    rc, msg, _, nsegs = raw_segments(lib, eng, ev, seg, probs, [0, 0, 0], 10)      # 2^31 - 1 itself passes the check; here: no frames
    assert rc == 0 and int(nsegs[0]) == 0, msg
    for off in (1, 4, 8):
        e2 = aligned(total, np.uint8, off=off)
        e2[:] = ev
        refused("events and the segment table must be 16-byte aligned", ev=e2)
    refused("must be 16-byte aligned", segs=aligned(1002, seg_ref.DTYPE, SENT, off=8))
    for arr in ("seg", "probs"):
        raw = aligned(4 * total + 2, np.uint8, off=0)[2:2 + 4 * total]
        assert raw.ctypes.data % 4 == 2
        mis = raw.view(np.int32 if arr == "seg" else np.float32)
        refused("seg_frames and probs must be 4-byte aligned", **{arr: mis})
    cnt = aligned(3, np.int32, SENT)[1:3].view(np.int64)
    assert cnt.ctypes.data % 8 == 4
    refused("the count must be 8-byte aligned", nsegs=cnt)
    assert lib.vad_segments_device(None, None, None, None, None, 0, None, 0, None, None) == INV
    # no frames: the count alone is written, whatever else is null
    for st, n in (([0], None), ([0, 0, 0], None), (None, 0)):
        rc, msg, segs, nsegs = raw_segments(lib, eng, None, None, None, st, 4, n=n)
        assert rc == 0 and int(nsegs[0]) == 0 and untouched(segs), msg
    # seg_cap = 0 needs no table
    rc, msg, _, nsegs = raw_segments(lib, eng, ev, seg, probs, start, 0, segs=None)
    assert rc == 0 and int(nsegs[0]) == len(want), msg


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17])
def test_segments_device_matches_the_reference_at_chunk_edges(lib, make_engine, total):
    eng = make_engine()
    rng = np.random.default_rng(total)
    ev, seg, probs = flat_arrays(rng, total, p_end=0.2)
    if total:
        ev[-1], seg[-1], probs[-1] = 0x02, 1, 0.5
    cuts = np.sort(rng.integers(0, total + 1, 5))
    start = np.concatenate([[0], cuts, [total]])
    want = seg_ref.table(ev, seg, probs, start)
    for cap in sorted({0, max(len(want) - 1, 0), len(want), len(want) + 3}):
        rc, msg, segs, nsegs = raw_segments(lib, eng, ev if total else None, seg if total else None, probs if total else None, start, cap)
        assert rc == 0, msg
        assert int(nsegs[0]) == len(want)
        k = min(cap, len(want))
        assert seg_ref.same(segs[:k].copy(), want[:k]) and untouched(segs[k:])
    # a call whose items begin behind index 0 leaves the frames before them alone
    if total > 64:
        want = seg_ref.table(ev, seg, probs, start[2:])
        rc, msg, segs, nsegs = raw_segments(lib, eng, ev, seg, probs, start[2:], len(want) + 1)
        assert rc == 0 and int(nsegs[0]) == len(want) and seg_ref.same(segs[:len(want)].copy(), want) and untouched(segs[len(want):]), msg


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_extracts_and_only_v5_tile_engines_scan(lib, make_engine, kw):
    eng = make_engine(**kw)
    ev, seg, probs = flat_arrays(np.random.default_rng(9), 9000)
    start = [0, 10, 4100, 9000]
    want = seg_ref.table(ev, seg, probs, start)
    rc, msg, segs, nsegs = raw_segments(lib, eng, ev, seg, probs, start, len(want))
    assert rc == 0 and int(nsegs[0]) == len(want) > 50 and seg_ref.same(segs[:len(want)].copy(), want), (kw, msg)
    frame = eng.frame_samples
    x = script(ONE, frame, frame, "f32")
    slot = eng.open_stream()
    eng.set_thresholds_many([slot], THR)
    try:
        items = (_ffi.ScanChItem * 1)(_ffi.ScanChItem(int(slot), 0, x.size, 0, 0))
        out = np.full(8, SENT, np.uint8).view(np.int64)
        tab = aligned(4, seg_ref.DTYPE, SENT)
        rc = lib.vad_scan_segments(eng.handle, items, 1, x.ctypes.data, x.size, 1, _ffi.VAD_FMT_F32, frame, -1.0,
                                   tab.ctypes.data_as(C.POINTER(_ffi.Segment)), 4, out.ctypes.data_as(C.POINTER(C.c_int64)))
        msg = lib.vad_last_error(eng.handle).decode()
        if "rate" in kw:
            assert rc == 0 and int(out[0]) == 1 and tab[0]["nframes"] >= 5, msg
        else:
            assert rc == UNSUP and "vad_scan_segments" in msg and untouched(tab) and untouched(out), msg
            with pytest.raises(Exception, match="vad_scan_segments"):
                eng.scan_segments([slot], [x], hop=frame)
    finally:
        eng.close_stream(int(slot))


# ---- vad_scan_segments ------------------------------------------------------------------------------------------------
def test_scan_segments_refusals_are_the_scan_s_and_write_nothing(lib, make_engine):
    eng = make_engine(max_streams=8)
    frame = eng.frame_samples
    x = np.ascontiguousarray(np.stack([script(THREE, frame, frame, "f32")] * 2, axis=1))
    ns = x.shape[0]
    slots = eng.open_streams(2)
    eng.set_thresholds_many(slots, THR)
    saved = [eng.save_stream(int(s)) for s in slots]

    def call(items, n=None, audio=x, audio_samples=ns, channels=2, fmt=_ffi.VAD_FMT_F32, hop=frame, cap=8, tab="own", cnt="own"):
        arr = (_ffi.ScanChItem * max(1, len(items)))(*[_ffi.ScanChItem(*map(int, it)) for it in items])
        tab = aligned(10, seg_ref.DTYPE, SENT) if isinstance(tab, str) else tab
        cnt = aligned(1, np.int64, SENT) if isinstance(cnt, str) else cnt
        rc = lib.vad_scan_segments(eng.handle, arr, len(items) if n is None else n, None if audio is None else audio.ctypes.data, audio_samples,
                                   channels, fmt, hop, -1.0, None if tab is None else tab.ctypes.data_as(C.POINTER(_ffi.Segment)), cap,
                                   None if cnt is None else cnt.ctypes.data_as(C.POINTER(C.c_int64)))
        return rc, lib.vad_last_error(eng.handle).decode(), tab, cnt

    ok = [(slots[0], 0, ns, 0, 0), (slots[1], 0, ns, 1, 0)]

    def refused(pattern, items=ok, code=INV, **kw):
        rc, msg, tab, cnt = call(items, **kw)
        assert rc == code, (rc, msg)
        assert msg.startswith("Model prediction failed: ") and re.search(pattern, msg) and ("vad_scan_segments" in msg or "format" in msg), msg
        assert untouched(tab) and untouched(cnt)
        assert [eng.save_stream(int(s)) for s in slots] == saved

    try:
        refused("null buffer or bad count", n=-1)
        refused("null buffer or bad count", audio_samples=-1)
        refused("unknown frame format", fmt=7)
        for ch in (0, 3):
            refused(r"channels = \d, the block holds 1 or 2", channels=ch)
        refused("9 recordings, max_streams = 8", items=[ok[0]] * 9)
        for h in (0, 2, 6, -256):
            refused(r"hop = -?\d+ must be a positive multiple of 4", hop=h)
        refused("2 GiB", audio_samples=1 << 28)
        refused("starts at sample 2, not a multiple of 4", items=[(slots[0], 2, 600, 0, 0)])
        refused("leaves the audio block", items=[(slots[0], 0, ns + 1, 0, 0)])
        refused("leaves the audio block", items=[(slots[0], 0, -5, 0, 0)])
        refused("leaves the audio block", items=[(slots[0], 0, 1 << 62, 0, 0)])
        refused("names channel 2 of 2", items=[(slots[0], 0, ns, 2, 0)])
        refused("reserved = 3 must be 0", items=[(slots[0], 0, ns, 0, 3)])
        refused("seg_cap = -1: bad count", cap=-1)
        refused("null buffer", audio=None)
        refused("null buffer", tab=None)
        refused("null buffer", cnt=None)
        rc, msg, tab, cnt = call([(slots[0], 0, ns, 0, 0), (slots[0], 0, ns, 1, 0)])
        assert rc == _ffi.VAD_ERR_BAD_SLOT and untouched(tab) and untouched(cnt), msg
        # refused calls have built no table
        assert lib.vad_scan_segments_read(eng.handle, 0, 0, None) == INV
        assert "holds no segment table" in lib.vad_last_error(eng.handle).decode()
        # seg_cap = 0 with no table is a complete call: the count, and the table stays for _read
        rc, msg, _, cnt = call(ok, cap=0, tab=None)
        assert rc == 0 and int(cnt[0]) == 6, msg
        assert lib.vad_scan_segments(None, None, 0, None, 0, 1, 0, 256, -1.0, None, 0, None) == INV
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("hop_div", [1, 2], ids=["hop_frame", "hop_half"])
@pytest.mark.parametrize("mode", ["mono", 0, 1, "mix", "split"])
@pytest.mark.parametrize("kind", ["f32", "i16", "ulaw", "alaw"])
def test_scripted_recordings_equal_the_scan_of_a_twin(lib, make_engine, kind, mode, hop_div):
    eng, twin = make_engine(), make_engine()
    frame = eng.frame_samples
    hop = frame // hop_div
    left = [NONE, ONE, THREE, [], TWO, [0.9] * 12]        # 0, 1, 3, (no frame), 2 segments, and one still open at the end
    right = [TWO, NONE, ONE, [], THREE, NONE]
    both = [ONE, TWO, NONE, [], ONE, THREE]               # the mix of equal channels is the channel
    if mode == "mono":
        recs = [script(p, frame, hop, kind) for p in left]
    elif mode == "mix":
        recs = [stereo(p, p, frame, hop, kind) for p in both]
    else:
        recs = [stereo(l, r, frame, hop, kind) for l, r in zip(left, right)]
    per = 2 if mode == "split" else 1
    kw = dict(law=LAW.get(kind), denoise=0.01, channel="mix" if mode == "mono" else mode)
    opened = []
    try:
        for e in (eng, twin):
            s = np.asarray(e.open_streams(len(recs) * per))
            opened.append(s)
            e.set_thresholds_many(s, THR)
        shape = (len(recs), 2) if per == 2 else (len(recs),)
        got = eng.scan_segments(opened[0].reshape(shape), recs, hop=hop, **kw)
        want, ranges = twin_table(twin, opened[1].reshape(shape), recs, frame, hop, **kw)
        assert seg_ref.same(got, want)
        assert by_item(got, len(recs) * per, frame, hop) == ranges
        counts = sorted(len(r) for r in ranges)
        assert counts[0] == 0 and 1 in counts and counts[-1] >= 2 and sum(counts) >= 6      # no comparison of empty tables
        assert (got["counted"] == np.minimum(got["nframes"], got["first_frame"] + got["nframes"])).all() and (got["max_prob"] > 0.6).all()
        assert (got["mean_prob"] <= got["max_prob"]).all() and (got["mean_prob"] > 0.05).all()
        assert [eng.save_stream(int(s)) for s in opened[0]] == [twin.save_stream(int(s)) for s in opened[1]]
        assert eng.info()["frames"] == twin.info()["frames"] and eng.info()["steps"] == twin.info()["steps"]
        # the block is resident: the cut behind the table is the cut behind the scan
        offs = eng.last_scan["offsets"]
        assert np.array_equal(offs, twin.last_scan["offsets"]) and eng.last_scan["samples"] == twin.last_scan["samples"]
        chan = lambda it: () if mode == "mono" else ((it % 2,) if mode == "split" else (mode,))
        segs = [(int(offs[it // per]), int(f), int(n)) + chan(it) for it, f, n in zip(got["item"], got["first_frame"], got["nframes"])]
        a, sa = eng.cut(segs, hop=hop, denoise=0.01)
        b, sb = twin.cut(segs, hop=hop, denoise=0.01)
        assert a.size == frame * int(got["nframes"].sum()) and np.array_equal(a, b) and np.array_equal(sa, sb) and np.abs(a).max() > 1000
    finally:
        for e, s in zip((eng, twin), opened):
            for k in s:
                e.close_stream(int(k))


def test_truncation_keeps_the_count_and_read_delivers_the_rest(lib, make_engine):
    eng = make_engine()
    frame = eng.frame_samples
    recs = [script(p, frame, frame, "f32") for p in (THREE, NONE, TWO, ONE)]
    ns = [r.size for r in recs]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in ns])])
    block = np.zeros(int(offs[-1]), np.float32)
    for o, r in zip(offs, recs):
        block[o:o + r.size] = r
    read = lambda first, count, out: lib.vad_scan_segments_read(eng.handle, first, count, None if out is None else out.ctypes.data_as(C.POINTER(_ffi.Segment)))
    err = lambda: lib.vad_last_error(eng.handle).decode()
    assert read(0, 1, aligned(1, seg_ref.DTYPE)) == INV and "vad_scan_segments_read: the engine holds no segment table" in err()
    slots = eng.open_streams(4)
    try:
        full = None
        for cap in (6, 0, 5, 6, 9):
            eng.reset(slots)
            eng.set_thresholds_many(slots, THR)
            items = (_ffi.ScanChItem * 4)(*[_ffi.ScanChItem(int(s), int(o), int(n), 0, 0) for s, o, n in zip(slots, offs, ns)])
            tab = aligned(cap + 2, seg_ref.DTYPE, SENT)
            cnt = C.c_int64(-1)
            rc = lib.vad_scan_segments(eng.handle, items, 4, block.ctypes.data, block.size, 1, _ffi.VAD_FMT_F32, frame, -1.0,
                                       tab.ctypes.data_as(C.POINTER(_ffi.Segment)), cap, C.byref(cnt))
            assert rc == 0 and cnt.value == 6, err()
            if full is None:
                full = tab[:6].copy()
                assert full["item"].tolist() == [0, 0, 0, 2, 2, 3] and (full["nframes"] >= 3).all()
            k = min(cap, 6)
            assert tab[:k].tobytes() == full[:k].tobytes() and untouched(tab[k:])
            rest = aligned(6 - k + 1, seg_ref.DTYPE, SENT)
            assert read(k, 6 - k, rest) == 0, err()
            assert rest[:6 - k].tobytes() == full[k:].tobytes() and untouched(rest[6 - k:])
            one = aligned(2, seg_ref.DTYPE, SENT)
            assert read(3, 1, one) == 0 and one[:1].tobytes() == full[3:4].tobytes() and untouched(one[1:])
            assert read(6, 0, None) == 0 and read(0, 0, None) == 0
            for first, count in ((0, 7), (6, 1), (7, 0), (-1, 1), (0, -1), (5, 1 << 62)):
                assert read(first, count, one) == INV and "leave the table of 6" in err(), (first, count)
            assert read(0, 2, None) == INV and "null buffer" in err()
            assert untouched(one[1:])
        # Engine.scan_segments guesses a capacity and reads what did not fit: a corpus denser than its guess
        eng.reset(slots)
        eng.set_thresholds_many(slots, (0.5, 0.5, 0.5, 0.5, 1, 1))
        twin = make_engine()
        ts = twin.open_streams(1)
        twin.set_thresholds_many(ts, (0.5, 0.5, 0.5, 0.5, 1, 1))
        dense = script([0.9, 0.0] * 1400, frame, frame, "f32")
        got = eng.scan_segments(slots[:1], [dense], hop=frame, denoise=None)
        want, _ = twin_table(twin, ts, [dense], frame, frame, denoise=None)
        # more than the wrapper's first capacity (a segment per 64 frames) and than the engine's (one per 16 frames, + 256)
        assert len(want) > 2800 // 16 + 256 and seg_ref.same(got, want)
        twin.close_stream(int(ts[0]))
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_a_segment_that_began_in_an_earlier_scan_has_a_negative_first_frame(lib, make_engine):
    eng, twin = make_engine(), make_engine()
    frame = hop = eng.frame_samples
    head = script([0.0] * 3 + [0.9] * 6, frame, hop, "f32")                 # ends inside a segment
    tail = script([0.8, 0.7, 0.9] + [0.0] * 5 + ONE, frame, hop, "f32")     # ends it at frame 4 or so, then one more
    s, t = eng.open_streams(1), twin.open_streams(1)
    try:
        for e, k in ((eng, s), (twin, t)):
            e.set_thresholds_many(k, THR)
        assert len(eng.scan_segments(s, [head], hop=hop, denoise=None)) == 0
        twin.scan(t, [head], hop=hop, denoise=None)
        got = eng.scan_segments(s, [tail], hop=hop, denoise=None)
        probs, ev, seg = twin.scan(t, [tail], hop=hop, denoise=None)
        want = seg_ref.table(ev[0], seg[0], probs[0], [0, probs[0].size])
        assert seg_ref.same(got, want) and len(got) == 2
        first, L = int(got[0]["first_frame"]), int(got[0]["nframes"])
        assert first < 0 and L >= 6 and first + L - 1 >= 3
        assert segment_ranges(got, frame, hop) == speech_segments(ev[0], seg[0], frame, hop)
        # the statistics cover the recording's frames 0 .. e alone
        e = first + L - 1
        assert got[0]["counted"] == e + 1 < L
        assert got[0]["max_prob"] == probs[0][:e + 1].max() == np.float32(0.9)
        assert got[0]["mean_prob"] == np.float32(np.rint(probs[0][:e + 1].astype(np.float64) * 2 ** 30).sum() / ((e + 1) * 2.0 ** 30))
        assert got[1]["first_frame"] > e and got[1]["counted"] == got[1]["nframes"]
        assert eng.save_stream(int(s[0])) == twin.save_stream(int(t[0]))
    finally:
        eng.close_stream(int(s[0]))
        twin.close_stream(int(t[0]))


def test_a_rejected_frame_inside_a_segment_enters_no_statistic(lib, make_engine):
    eng, twin = make_engine(), make_engine()
    frame = hop = eng.frame_samples
    p = [0.0] * 2 + [0.9, 0.6, 0.9, 0.7, 0.9, 0.8] + [0.0] * 6
    x = script(p, frame, hop, "f32")
    y = x.copy()
    y[4 * hop + 17] = np.nan                      # frame 4: rejected, the state machine never sees it
    y[6 * hop + 5] = np.inf
    s, t = eng.open_streams(2), twin.open_streams(2)
    try:
        for e, k in ((eng, s), (twin, t)):
            e.set_thresholds_many(k, THR)
        got = eng.scan_segments(s, [x, y], hop=hop, denoise=None)
        probs, ev, seg = twin.scan(t, [x, y], hop=hop, denoise=None)
        assert ev[1][4] == ev[1][6] == _ffi.VAD_EV_REJECTED and np.isnan(probs[1][[4, 6]]).all()
        fp, start, _ = flatten(probs)
        want = seg_ref.table(flatten(ev)[0], flatten(seg)[0], fp, start)
        assert seg_ref.same(got, want) and got["item"].tolist() == [0, 1]
        clean, holed = got
        assert holed["first_frame"] + holed["nframes"] > 6 and holed["first_frame"] <= 4       # both rejected frames lie inside
        inside = np.arange(holed["first_frame"], holed["first_frame"] + holed["nframes"])
        keep = inside[(inside != 4) & (inside != 6)]
        assert holed["counted"] == keep.size == holed["nframes"] - 2
        assert holed["max_prob"] == probs[1][keep].max() and np.isfinite(holed["mean_prob"])
        assert holed["mean_prob"] == np.float32(np.rint(probs[1][keep].astype(np.float64) * 2 ** 30).sum() / (keep.size * 2.0 ** 30))
        assert clean["counted"] == clean["nframes"]
    finally:
        for e, k in ((eng, s), (twin, t)):
            for q in k:
                e.close_stream(int(q))


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_scan_and_cut_recordings_take_the_table_and_give_what_the_frames_gave(lib, make_engine):
    from cutter_vad_amd import VADConfig, cut_recordings, scan_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame // 2
    st = lambda l, r: stereo(l, r, frame, hop, "f32")
    corpus = [script(ONE, frame, hop, "f32"), st(TWO, NONE), script(NONE, frame, hop, "f32"), st(THREE, THREE), np.zeros((0, 2), np.float32),
              script(THREE, frame, hop, "f32")]
    cfg = VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5, voice_start_frame_count=2,
                    voice_end_frame_count=2, enable_denoising=False)

    class FramesOnly:
        """the engine as it was before scan_segments: scan_recordings and cut_recordings fall back to the per-frame path"""
        def __init__(self, e):
            self._e = e

        def __getattr__(self, name):
            if name in ("scan_segments", "segments_device"):
                raise AttributeError(name)
            return getattr(self._e, name)

    old = FramesOnly(eng)
    assert hasattr(eng, "scan_segments") and not hasattr(old, "scan_segments")
    calls = []
    real = eng.scan_segments
    eng.scan_segments = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for channel in (0, 1, "mix", "split"):
            new = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel)
            assert new == scan_recordings(corpus, cfg, engine=old, hop=hop, channel=channel)
            assert sum(len(s) for r in new for s in (r if channel == "split" else [r])) >= 6
            with_stats = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, stats=True)
            assert with_stats == scan_recordings(corpus, cfg, engine=old, hop=hop, channel=channel, stats=True)
            flat = lambda res: [s for r in res for lst in (r if channel == "split" else [r]) for s in lst]
            assert [s[:2] for s in flat(with_stats)] == flat(new)
            for s in flat(with_stats):
                assert len(s) == 4 and isinstance(s[2], float) and isinstance(s[3], float) and 0.05 < s[2] <= s[3] <= 0.9001
            a = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel)
            b = cut_recordings(corpus, cfg, engine=old, hop=hop, channel=channel)
            assert a == b and sum(len(p) for *_, p in flat(a)) > 6 * 44
        assert len(calls) == 4 * 3 * 2                # every call above, once per kind of recording
    finally:
        del eng.scan_segments
    assert scan_recordings([], cfg, engine=eng, stats=True) == []
    assert scan_recordings([script(NONE, frame, hop, "f32")], cfg, engine=eng, hop=hop, stats=True) == [[]]


def _hipcc():
    import shutil
    return next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_the_kernel_file_compiles_without_scratch_or_spills(tmp_path):
    """count, prefix, fill and statistics, from the compiler's own metadata"""
    import subprocess
    from cutter_vad_amd import _build
    cc = _hipcc()
    assert "scan_segments.hip" in _build.HIP_SOURCES
    out = tmp_path / "scan_segments.s"
    subprocess.run([cc, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "cutter_vad_amd", "csrc", "scan_segments.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = re.findall(r"\.name:\s*(_Z\d+vadk_seg_\w+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                      text, re.S)
    assert len(meta) == 4 and {m[0].split("vadk_seg_")[1][:4] for m in meta} == {"pass", "pref", "stat"}, meta
    for name, scratch, sspill, vspill in meta:
        assert (scratch, sspill, vspill) == ("0", "0", "0"), (name, scratch, sspill, vspill)
    # the pass kernel reads its 16 event bytes with ONE 16-byte load through the buffer descriptor
    for flavour in ("Lb0", "Lb1"):
        name = next(m[0] for m in meta if flavour in m[0])
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)
        assert re.findall(r"\bbuffer_load_\w+", body) == ["buffer_load_dwordx4"], (name, re.findall(r"\bbuffer_load_\w+", body))


# ---- the order of the refusals ----------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, make_engine):
    """The order of the checks is behaviour.  vad_segments_device: the counts, 2^31 items, the null arguments, the positions (first not
    negative, never decreasing, at most 2^31 - 1 frames), the null per-frame arrays, then the 16-, 4- and 8-byte alignments.
    vad_scan_segments and vad_scan_rate_segments: the rate, then the scan's own checks in the scan's order, seg_cap, the null
    arguments.  vad_scan_segments_read: the table, the range, the null output.  Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    eng = make_engine(max_streams=8)
    seg = lambda off=0: RO.buf(24 * 4, off).view(np.uint8)

    def device(ev, sf, probs, start, n, segs, cap, nsegs):
        return lib.vad_segments_device(eng.handle, RO.addr(ev), RO.addr(sf), RO.addr(probs), RO.i64p(start), n, RO.addr(segs), cap, RO.addr(nsegs), None)

    faults = dict(ev=None, sf=None, probs=None, start=None, n=-1, segs=None, cap=-1, nsegs=None)
    RO.walk_one(lib, eng, device, faults, (
        (INV, "n = -1, seg_cap = -1: bad count", "n", 1 << 31),
        (INV, "n = 2147483648, seg_cap = -1: bad count", "cap", 4),
        (INV, r"more than 2\^31 - 1 items", "n", 2),
        (INV, "vad_segments_device: null buffer$", "start", RO.i64(-1, 3, 2)),
        (INV, "vad_segments_device: null buffer$", "nsegs", RO.buf(8, 4)),
        (INV, "vad_segments_device: null buffer$", "segs", seg(8)),
        (INV, r"out_start\[0\] is negative", "start", RO.i64(0, 3, 2)),
        (INV, r"out_start decreases at item 1 \(2 after 3\)", "start", RO.i64(0, 3, 1 << 31)),
        (INV, r"more than 2\^31 - 1 frames in one call", "start", RO.i64(0, 3, 3)),
        (INV, "vad_segments_device: null buffer$", "ev", RO.buf(16, 8)),
        (INV, "vad_segments_device: null buffer$", "sf", RO.buf(16, 2)),
        (INV, "vad_segments_device: null buffer$", "probs", RO.buf(16, 2)),
        (INV, "the events and the segment table must be 16-byte aligned", "ev", RO.buf(16)),
        (INV, "the events and the segment table must be 16-byte aligned", "segs", seg()),
        (INV, "seg_frames and probs must be 4-byte aligned", "sf", RO.buf(16)),
        (INV, "seg_frames and probs must be 4-byte aligned", "probs", RO.buf(16)),
        (INV, "the count must be 8-byte aligned", "nsegs", RO.buf(8))))

    # the host forms: one recording with a segment, one without a frame
    frame = eng.frame_samples
    assert lib.vad_scan_segments_read(eng.handle, -1, 5, None) == INV                     # before any table: whatever the range
    assert "holds no segment table" in lib.vad_last_error(eng.handle).decode()
    slots = eng.open_streams(2)
    eng.set_thresholds_many(slots, THR)
    x = script(ONE, frame, frame, "f32")
    ns = x.size
    s0, s1 = int(slots[0]), int(slots[1])
    count = np.full(1, -7, np.int64)

    def host(rate, sr_in, items, n, audio, audio_samples, channels, fmt, hop, tab, cap, cnt):
        args = (eng.handle, RO.scan_items(items), len(items) if n is None else n, RO.addr(audio), audio_samples, channels, fmt)
        if rate:
            return lib.vad_scan_rate_segments(*args, sr_in, hop, -1.0, RO.segp(tab), cap, RO.i64p(cnt))
        return lib.vad_scan_segments(*args, hop, -1.0, RO.segp(tab), cap, RO.i64p(cnt))

    rest = lambda *first: [first, (s0, 0, 0, 0, 0)]
    steps = (
        (INV, "null buffer or bad count", "n", None),
        (INV, "unknown frame format 9", "fmt", _ffi.VAD_FMT_F32),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "9 recordings, max_streams = 8", "items", rest(s0, 2, ns + 4, 1, 3)),
        (INV, "hop = 6 must be a positive multiple of 4", "hop", frame),
        (INV, "2 GiB", "audio_samples", ns),
        (INV, "recording 0 starts at sample 2, not a multiple of 4", "items", rest(s0, 0, ns + 4, 1, 3)),
        (INV, "recording 0 .*leaves the audio block", "items", rest(s0, 0, ns, 1, 3)),
        (INV, "recording 0 names channel 1 of 1", "items", rest(s0, 0, ns, 0, 3)),
        (INV, "recording 0: reserved = 3 must be 0", "items", rest(s0, 0, ns, 0, 0)),
        (_ffi.VAD_ERR_BAD_SLOT, f"slot {s0} appears twice", "items", [(s0, 0, ns, 0, 0), (s1, 0, 0, 0, 0)]),
        (INV, "seg_cap = -1: bad count", "cap", 4),
        (INV, "segments: null buffer$", "cnt", count),
        (INV, "segments: null buffer$", "tab", seg()),
        (INV, "segments: null buffer$", "audio", x))
    faults = dict(sr_in=11025, items=[(s0, 2, ns + 4, 1, 3)] * 9, n=-1, audio=None, audio_samples=1 << 30, channels=3, fmt=9, hop=6, tab=None,
                  cap=-1, cnt=None)
    try:
        for rate in (False, True):
            first = ((_ffi.VAD_ERR_UNSUPPORTED, "from 11025Hz to 16000Hz", "sr_in", 8000),) if rate else ()
            count[0] = -7
            RO.walk_one(lib, eng, host, dict(faults, rate=rate), first + steps)
            assert count[0] >= 1
            eng.reset(slots)
            eng.set_thresholds_many(slots, THR)
        read = lambda first, k, out: lib.vad_scan_segments_read(eng.handle, first, k, RO.segp(out))
        RO.walk_one(lib, eng, read, dict(first=-1, k=5, out=None), (
            (INV, r"records -1 \.\. \+5 leave the table of 1", "first", 0),
            (INV, r"records 0 \.\. \+5 leave the table of 1", "k", 1),
            (INV, "vad_scan_segments_read: null buffer$", "out", seg())))
    finally:
        for s in slots:
            eng.close_stream(int(s))
