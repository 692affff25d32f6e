"""vad_scan_tails, vad_scan_resegment_tails, vad_tails_device, vad_resegment_tails_device, the Engine methods and open_end=True of
scan_recordings / sweep_recordings / cut_recordings on the host side: exports, byte equality with tests/tail_ref.py (the oracle's
state machine, tests/seg_ref.py's statistics) on a scripted corpus - ends in speech, ends on an END, starts again, starts on the
last frame, never starts, rejected frames, continued slots, split channels, 8 and 48 kHz rate scans - for 1, 5 and 64 sets, the
snapshot's isolation from what happens to the streams behind the scan, what a call leaves alone, the mark, every refusal with its
message and an untouched output - the real csrc/engine.cpp over the HIP stand-in (tests/standin.py: p = |first sample of a frame|,
so the audio scripts the probabilities; the stand-in's tails run the real sm_step).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import seg_ref, standin, tail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_tails", "vad_scan_resegment_tails", "vad_tails_device", "vad_resegment_tails_device"]
INV = _ffi.VAD_ERR_INVALID_ARG
SENT = 0x5A
ZERO = np.zeros(1, seg_ref.DTYPE)[0]
EMPTY = (0.99, 0.98, 1.0, 1.0, 19, 60)            # starts nowhere: no scripted probability reaches 0.99
DEFAULTS = (0.7, 0.7, 0.8, 0.95, 10, 50)
THR = (0.5, 0.5, 0.8, 0.95, 2, 2)                 # what the scans run with: a START after two high frames, an END after two low ones
BASE = [THR, (0.6, 0.4, 0.7, 0.9, 3, 4), (0.8, 0.3, 0.5, 0.6, 1, 1), EMPTY, DEFAULTS, (0.3, 0.2, 0.9, 0.85, 4, 3),
        (0.55, 0.45, 0.6, 0.75, 5, 6), (0.65, 0.35, 0.75, 1.0, 2, 8)]


def sets_of(nt):
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


def same(got, want):
    return seg_ref.same(np.ascontiguousarray(got), np.ascontiguousarray(want))


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


# the named cases, under THR; what each must give is asserted on the REFERENCE in the test below
IN_SPEECH, ON_END, AGAIN, LAST_START, NEVER, HOLE, LAST_BAD, WHOLE = range(8)


def corpus(frame, hop, seed=5):
    """the named cases, then recordings of 0 .. 120 frames (0, 1 and 120 among them): 40 in all"""
    rng = np.random.default_rng(seed)
    named = [script([0.0, 0.0, 0.9, 0.8, 0.9, 0.7], frame, hop),                            # ends in speech
             script([0.0, 0.9, 0.9, 0.9, 0.0, 0.0], frame, hop),                            # its END is the last frame
             script([0.9, 0.9, 0.9, 0.0, 0.0, 0.0, 0.9, 0.6, 0.9], frame, hop),             # END, then a new START
             script([0.0, 0.0, 0.9, 0.9], frame, hop),                                      # START on the last frame
             script([0.1] * 30, frame, hop),                                                # never starts
             script([0.0, 0.9, 0.9, 0.8, 0.7, 0.9, 0.6], frame, hop),                       # a rejected frame inside the tail
             script([0.0, 0.9, 0.9, 0.8, 0.7, 0.9, 0.1], frame, hop),                       # ... and one as the last frame
             script([0.9, 0.8, 0.9], frame, hop)]                                           # the tail is the whole recording
    named[HOLE][4 * hop + 7] = np.nan
    named[LAST_BAD][6 * hop + 2] = np.inf
    lengths = [0, 1, 120, 2, 119] + [int(v) for v in rng.integers(3, 119, 27)]
    return named + [script(speechy(rng, n), frame, hop) for n in lengths]


def per_frame(make_engine, recs, hop, split=False, **kw):
    """Engine.scan on a twin engine -> the flat events and probs in item order and out_start (of the events the REJECTED bit alone is read)"""
    twin = make_engine()
    slots = np.asarray(twin.open_streams(len(recs) * (2 if split else 1)))
    try:
        probs, ev, _ = twin.scan(slots.reshape(len(recs), 2) if split else slots, recs, hop=hop, denoise=None, **kw)
    finally:
        for s in slots:
            twin.close_stream(int(s))
    if split:
        probs, ev = [p[c] for p in probs for c in (0, 1)], [e[c] for e in ev for c in (0, 1)]
    start = np.concatenate([[0], np.cumsum([len(p) for p in probs])]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt) for x in xs]) if len(xs) else np.zeros(0, dt)
    return cat(ev, np.uint8), cat(probs, np.float32), start


def scan_on(eng, recs, hop, thr=THR, split=False, slots=None, **kw):
    if slots is None:
        slots = np.asarray(eng.open_streams(len(recs) * (2 if split else 1)))
        eng.set_thresholds_many(slots, thr)
    table = eng.scan_segments(slots.reshape(len(recs), 2) if split else slots, recs, hop=hop, denoise=None, **kw)
    return slots, table


def close(eng, slots):
    for s in slots:
        eng.close_stream(int(s))


def raw_tails(lib, eng, n, out="own"):
    if isinstance(out, str):
        out = aligned(max(n, 0) + 2, seg_ref.DTYPE, SENT)
    rc = lib.vad_scan_tails(eng.handle, None if out is None else out.ctypes.data_as(C.POINTER(_ffi.Segment)), n)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def raw_reseg_tails(lib, eng, sets, n, nt=None, out="own"):
    nt = len(sets) if nt is None else nt
    if isinstance(out, str):
        out = aligned(max(n, 0) * max(min(nt, 70), 0) + 2, seg_ref.DTYPE, SENT)
    rc = lib.vad_scan_resegment_tails(eng.handle, thr_array(sets), nt, None if out is None else out.ctypes.data_as(C.POINTER(_ffi.Segment)), n)
    return rc, lib.vad_last_error(eng.handle).decode(), out


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    proto = lambda name: re.sub(r"/\*.*?\*/", "", re.search(r"VAD_API int %s\((.*?)\);" % name, header, re.S).group(1))
    for name, nargs in zip(NEW, (3, 5, 8, 9)):
        assert declared.count(name) == 1, name
        assert hasattr(lib, name), name
        assert len(proto(name).split(",")) == len(_ffi.SIGNATURES[name][1]) == nargs, name
    assert "#define VAD_ABI_VERSION 5" in header
    assert "has no END and no record in this table; vad_scan_tails" in header
    from cutter_vad_amd import _build
    from cutter_vad_amd.engine import Engine
    assert "scan_tails.hip" in _build.HIP_SOURCES
    for m in ("scan_tails", "resegment_tails", "tails_device", "resegment_tails_device"):
        assert callable(getattr(Engine, m))


# ---- the equality -----------------------------------------------------------------------------------------------------
def test_the_reference_sees_every_named_case(make_engine):
    """the corpus is not vacuous, by the reference alone"""
    frame = hop = 512
    recs = corpus(frame, hop)
    assert len(recs) == 40
    ev, probs, start = per_frame(make_engine, recs, hop)
    want = tail_ref.fresh(ev, probs, start, [THR])[0]
    nf = np.diff(start)
    assert nf.min() == 0 and nf.max() == 120 and sorted(nf.tolist())[1] == 1
    assert want[IN_SPEECH].tolist()[:4] == (IN_SPEECH, 2, 4, 4)
    assert want[ON_END] == ZERO and want[NEVER] == ZERO
    assert want[AGAIN].tolist()[:4] == (AGAIN, 6, 3, 3)
    assert want[LAST_START].tolist()[:4] == (LAST_START, 2, 2, 2)                 # the buffered frame and the START itself
    # a rejected frame is no step of the state machine: L does not count it, and first_frame = nf - L moves up by one
    assert want[HOLE].tolist()[:4] == (HOLE, 2, 5, 4) and want[LAST_BAD].tolist()[:4] == (LAST_BAD, 2, 5, 4)
    assert (ev[start[HOLE] + 4], ev[start[LAST_BAD] + 6]) == (0x80, 0x80)
    assert want[WHOLE].tolist()[:4] == (WHOLE, 0, 3, 3)
    assert 8 <= int((want["nframes"] > 0).sum()) <= 32 and np.isfinite(want["mean_prob"]).all()
    assert want[want["nframes"] == 0].tobytes() == bytes(24 * int((want["nframes"] == 0).sum()))


@pytest.mark.parametrize("shape", ["mono", "split", "8k", "48k", "hop256"])
def test_scan_tails_equal_the_reference_and_the_replay_of_the_same_set(lib, make_engine, shape):
    eng = make_engine()
    rate = {"8k": 8000, "48k": 48000}.get(shape)
    kw = {} if rate is None else {"sample_rate": rate}
    frame = eng.scan_chunk_samples(rate) if rate else eng.frame_samples
    hop = frame // 2 if shape in ("hop256", "48k") else frame
    recs = corpus(frame, hop)
    if shape == "split":
        other = corpus(frame, hop, seed=9)[::-1]
        recs = [np.ascontiguousarray(np.stack([a[:min(len(a), len(b))], b[:min(len(a), len(b))]], axis=1)) for a, b in zip(recs, other)]
        kw["channel"] = "split"
    ev, probs, start = per_frame(make_engine, recs, hop, split=shape == "split", **kw)
    want = tail_ref.fresh(ev, probs, start, [THR])[0]
    assert 6 <= int((want["nframes"] > 0).sum()) < len(want)
    slots, table = scan_on(eng, recs, hop, split=shape == "split", **kw)
    try:
        got = eng.scan_tails()
        assert got.dtype == _ffi.SEGMENT_DTYPE and same(got, want), shape
        assert same(eng.resegment_tails([THR])[0], want)
        # a tail is no record of the table, and the table is what it was
        assert same(table, eng.resegment([THR])[0])
        ends = {(int(r["item"]), int(r["first_frame"])) for r in table}
        assert not ends & {(int(r["item"]), int(r["first_frame"])) for r in got if r["nframes"]}
        rc, msg, out = raw_tails(lib, eng, len(want))
        assert rc == 0 and same(out[:len(want)], want) and untouched(out[len(want):]), msg
    finally:
        close(eng, slots)


@pytest.mark.parametrize("nt", [1, 5, 64])
def test_replayed_tails_equal_the_reference_for_every_set(lib, make_engine, nt):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = corpus(frame, hop)
    ev, probs, start = per_frame(make_engine, recs, hop)
    sets = sets_of(nt) if nt != 5 else [BASE[k] for k in (1, 0, 3, 5, 2)]
    want = tail_ref.fresh(ev, probs, start, sets)
    assert nt == 1 or len({w.tobytes() for w in want}) >= min(nt, 4)
    assert nt < 5 or any(not w["nframes"].any() for w in want)
    slots, _ = scan_on(eng, recs, hop, thr=(0.62, 0.41, 0.66, 0.77, 3, 5))           # the scan's own set is none of them
    try:
        got = eng.resegment_tails(sets)
        assert len(got) == nt and all(same(g, w) for g, w in zip(got, want))
        rc, msg, out = raw_reseg_tails(lib, eng, sets, len(recs))
        assert rc == 0 and out[:nt * len(recs)].tobytes() == b"".join(w.tobytes() for w in want) and untouched(out[nt * len(recs):]), msg
    finally:
        close(eng, slots)


def test_continued_slots_give_a_negative_first_frame(lib, make_engine):
    from oracle import oracle
    eng = make_engine()
    frame = hop = eng.frame_samples
    heads = [[0.9] * 7, [0.9] * 4 + [0.0] * 2, [0.0, 0.9], [0.9] * 3, []]
    bodies = [[0.8] * 5, [0.9] * 6, [0.9, 0.9, 0.7], [0.9, 0.0, 0.0, 0.1], [0.9] * 4]
    slots, _ = scan_on(eng, [script(h, frame, hop) for h in heads], hop)
    try:
        recs = [script(b, frame, hop) for b in bodies]
        scan_on(eng, recs, hop, slots=slots)
        machines = [tail_ref.step_item(oracle.StateMachine(*THR), [0] * len(h), h) for h in heads]
        ev, probs, start = per_frame(make_engine, recs, hop)
        want = tail_ref.tails(ev, probs, start, machines)
        assert want["first_frame"].tolist() == [-7, 0, -1, 0, 0] and want["nframes"].tolist() == [12, 6, 4, 0, 4]
        assert want["counted"].tolist() == [5, 6, 3, 0, 4]                              # from the recording's frame 0 on
        assert same(eng.scan_tails(), want)
        # the replay starts every recording afresh
        assert same(eng.resegment_tails([THR])[0], tail_ref.fresh(ev, probs, start, [THR])[0])
    finally:
        close(eng, slots)


# ---- the snapshot -----------------------------------------------------------------------------------------------------
def test_the_snapshot_is_immune_to_what_happens_to_the_streams_behind_the_scan(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = corpus(frame, hop)[:12]
    slots, table = scan_on(eng, recs, hop)
    try:
        want = eng.scan_tails().copy()
        assert want["nframes"].astype(bool).sum() >= 5
        eng.reset(slots)
        assert same(eng.scan_tails(), want)
        eng.set_thresholds_many(slots, EMPTY)
        assert same(eng.scan_tails(), want)
        blob = eng.save_stream(int(slots[0]))
        eng.restore_stream(int(slots[1]), blob)
        eng.close_stream(int(slots[2]))
        slots = np.delete(slots, 2)
        assert same(eng.scan_tails(), want)
        info = eng.info()
        assert same(eng.scan_tails(), want) and (eng.info()["steps"], eng.info()["frames"]) == (info["steps"], info["frames"])
    finally:
        close(eng, slots)


def test_the_snapshot_launch_counts_as_no_model_launch(lib, make_engine):
    a, b = make_engine(), make_engine()
    frame = hop = a.frame_samples
    recs = corpus(frame, hop)[:10]
    sa, _ = scan_on(a, recs, hop)
    sb = np.asarray(b.open_streams(len(recs)))
    try:
        b.set_thresholds_many(sb, THR)
        b.scan(sb, recs, hop=hop, denoise=None)
        ia, ib = a.info(), b.info()
        assert (ia["steps"], ia["frames"]) == (ib["steps"], ib["frames"])
    finally:
        close(a, sa)
        close(b, sb)


# ---- what a call leaves alone -----------------------------------------------------------------------------------------
def test_a_tails_call_leaves_tables_streams_and_the_resident_block_alone(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = corpus(frame, hop)
    sets = [BASE[1], BASE[2], THR]
    slots, table = scan_on(eng, recs, hop)
    try:
        read = lambda out, k: lib.vad_scan_segments_read(eng.handle, 0, k, out.ctypes.data_as(C.POINTER(_ffi.Segment)))
        own = aligned(len(table) + 1, seg_ref.DTYPE)
        assert len(table) > 10 and read(own, len(table)) == 0 and read(own, len(table) + 1) == INV
        before = own[:len(table)].tobytes()
        assert before == np.ascontiguousarray(table).tobytes()
        reseg = [np.ascontiguousarray(t).tobytes() for t in eng.resegment(sets)]
        saved = [eng.save_stream(int(s)) for s in slots]
        info, last = eng.info(), dict(eng.last_scan)
        tails = eng.scan_tails()
        more = eng.resegment_tails(sets)
        assert same(more[2], tails)
        assert [eng.save_stream(int(s)) for s in slots] == saved
        assert (eng.info()["steps"], eng.info()["frames"]) == (info["steps"], info["frames"])
        again = aligned(len(table) + 1, seg_ref.DTYPE)
        assert read(again, len(table)) == 0 and again[:len(table)].tobytes() == before and read(again, len(table) + 1) == INV
        assert [np.ascontiguousarray(t).tobytes() for t in eng.resegment(sets)] == reseg
        assert eng.last_scan.keys() == last.keys() and eng.last_scan["samples"] == last["samples"]
        # the resident block still cuts, tail rows included
        rows = np.concatenate([table, tails[tails["nframes"] > 0]])
        offs = eng.last_scan["offsets"]
        pcm, where = eng.cut([(int(offs[i]), int(f), int(n)) for i, f, n in zip(rows["item"], rows["first_frame"], rows["nframes"])], hop=hop, denoise=None)
        assert pcm.size == frame * int(rows["nframes"].sum()) and where[-1] == pcm.size
        t = tails[IN_SPEECH]
        cut = pcm[where[len(table)]:where[len(table) + 1]]                             # the first tail row is the first item's
        hand = np.concatenate([recs[IN_SPEECH][f * hop:f * hop + frame] for f in range(int(t["first_frame"]), int(t["first_frame"] + t["nframes"]))])
        assert int(rows[len(table)]["item"]) == IN_SPEECH and cut.tolist() == (hand * np.float32(32767.0)).astype(np.int16).tolist()
    finally:
        close(eng, slots)


# ---- the device forms -------------------------------------------------------------------------------------------------
def device_arrays(rng, total):
    probs = speechy(rng, total)
    ev = aligned(total, np.uint8)
    ev[:] = rng.choice([0, 1, 2, 4, 6], total).astype(np.uint8)
    bad = rng.random(total) < 0.03
    ev[bad] |= 0x80
    probs[bad] = np.nan
    return ev, probs


def raw_tails_device(lib, eng, slots, ev, probs, start, n=None, out="own"):
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    n = (st.size - 1) if n is None else n
    if isinstance(out, str):
        out = aligned(max(min(n, 1 << 12), 0) + 2, seg_ref.DTYPE, SENT)
    sl = None if slots is None else np.ascontiguousarray(slots, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data
    i64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))
    rc = lib.vad_tails_device(eng.handle, i64(sl), ptr(ev), ptr(probs), i64(st), n, ptr(out), None)
    if rc == 0:
        eng.synchronize()
    return rc, lib.vad_last_error(eng.handle).decode(), out


def raw_reseg_tails_device(lib, eng, ev, probs, start, sets, nt=None, n=None, out="own"):
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    n = (st.size - 1) if n is None else n
    nt = len(sets) if nt is None else nt
    if isinstance(out, str):
        out = aligned(max(min(n, 1 << 12), 0) * max(min(nt, 70), 0) + 2, seg_ref.DTYPE, SENT)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib.vad_resegment_tails_device(eng.handle, ptr(ev), ptr(probs), None if st is None else st.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                        thr_array(sets), nt, ptr(out), None)
    if rc == 0:
        eng.synchronize()
    return rc, lib.vad_last_error(eng.handle).decode(), out


@pytest.mark.parametrize("kw", [dict(), dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v5", "v4", "shared_gpu", "v5_8k"])
def test_every_engine_has_the_device_forms(lib, make_engine, kw):
    from oracle import oracle
    eng = make_engine(**kw)
    rng = np.random.default_rng(21)
    ev, probs = device_arrays(rng, 700)
    sets = [BASE[0], BASE[1], BASE[2], EMPTY, BASE[5]]
    for start in ([0, 90, 90, 400, 401, 700], [37, 160, 420, 655]):
        n = len(start) - 1
        want = tail_ref.fresh(ev, probs, start, sets)
        assert sum(1 for w in want if w["nframes"].any()) >= 3 and not want[3]["nframes"].any()
        rc, msg, out = raw_reseg_tails_device(lib, eng, ev, probs, start, sets)
        assert rc == 0 and out[:5 * n].tobytes() == b"".join(w.tobytes() for w in want) and untouched(out[5 * n:]), (kw, msg)
        # the slot form: each slot's state machine is brought to where a scan of the item would leave it
        slots = np.asarray(eng.open_streams(n))[::-1].copy()
        try:
            eng.set_thresholds_many(slots, BASE[0])
            for i, s in enumerate(slots):
                lo, hi = start[i], start[i + 1]
                keep = (ev[lo:hi] & 0x80) == 0
                if keep.any():
                    eng.debug_sm_replay(int(s), probs[lo:hi][keep])
            rc, msg, out = raw_tails_device(lib, eng, slots, ev, probs, start)
            assert rc == 0 and same(out[:n], want[0]) and untouched(out[n:]), (kw, msg)
            eng.tails_device(slots, ev.ctypes.data, probs.ctypes.data, start, out.ctypes.data)
            eng.resegment_tails_device(ev.ctypes.data, probs.ctypes.data, start, sets[:1], out.ctypes.data)
            eng.synchronize()
            assert same(out[:n], want[0])
        finally:
            close(eng, slots)
    # a seg_frames larger than the item (a continued slot): the record says so, the statistics stay inside the item
    s = int(eng.open_stream())
    try:
        eng.set_thresholds_many([s], BASE[0])
        eng.debug_sm_replay(s, [0.9] * 50)
        st = [0, 0, 6]
        ev2, p2 = aligned(6, np.uint8), np.asarray([0.9, 0.8, np.nan, 0.7, 0.9, 0.8], np.float32)
        ev2[2] = 0x80
        eng.debug_sm_replay(s, p2[[0, 1, 3, 4, 5]])
        m = tail_ref.step_item(oracle.StateMachine(*BASE[0]), [0] * 50, [0.9] * 50)
        want = tail_ref.tails(ev2, p2, st, [oracle.StateMachine(*BASE[0]), m])
        t2 = int(eng.open_stream())
        try:
            rc, msg, out = raw_tails_device(lib, eng, [t2, s], ev2, p2, st)
        finally:
            eng.close_stream(t2)
        assert rc == 0 and same(out[:2], want) and out[0] == ZERO, msg
        assert want[1].tolist()[:4] == (1, 6 - 55, 55, 5) and want[1]["max_prob"] == np.float32(0.9)
    finally:
        eng.close_stream(s)
    # no frames, no items
    rc, msg, out = raw_reseg_tails_device(lib, eng, None, None, [0, 0, 0], sets)
    assert rc == 0 and out[:10].tobytes() == bytes(240) and untouched(out[10:]), msg
    rc, msg, out = raw_reseg_tails_device(lib, eng, None, None, None, sets, n=0)
    assert rc == 0 and untouched(out), msg
    rc, msg, out = raw_tails_device(lib, eng, None, None, None, None, n=0)
    assert rc == 0 and untouched(out), msg


def test_device_form_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    rng = np.random.default_rng(3)
    ev, probs = device_arrays(rng, 500)
    start = [0, 200, 200, 500]
    sets = [BASE[0], BASE[1]]
    slots = np.asarray(eng.open_streams(3))
    try:
        def refused(pattern, who="vad_resegment_tails_device", code=INV, slots=slots, ev=ev, probs=probs, start=start, sets=sets, **kw):
            if who == "vad_tails_device":
                rc, msg, out = raw_tails_device(lib, eng, slots, ev, probs, start, **kw)
            else:
                rc, msg, out = raw_reseg_tails_device(lib, eng, ev, probs, start, sets, **kw)
            assert rc == code, (rc, msg)
            assert re.search(pattern, msg) and (code != INV or msg.startswith(f"Model prediction failed: {who}: ")), msg
            assert untouched(out)

        refused("nt = 0: 1 .. 64 threshold sets", nt=0)
        refused("nt = 65: 1 .. 64 threshold sets", sets=sets_of(65))
        refused("null buffer", sets=None, nt=2)
        refused("more than 2\\^31 - 1 replays", n=(1 << 30), sets=sets_of(3))
        for who in ("vad_resegment_tails_device", "vad_tails_device"):
            refused("n = -1: bad count", who, n=-1)
            refused("null buffer", who, start=None, n=3)
            refused("null buffer", who, out=None)
            refused("null buffer", who, ev=None)
            refused("null buffer", who, probs=None)
            refused("out_start\\[0\\] is negative", who, start=[-4, 200, 200, 500])
            refused("out_start decreases at item 1 \\(100 after 200\\)", who, start=[0, 200, 100, 500])
            refused("more than 2\\^31 - 1 frames", who, start=[0, 200, 200, 1 << 31])
            e2 = aligned(500, np.uint8, off=4)
            e2[:] = ev
            refused("events and the tails must be 16-byte aligned", who, ev=e2)
            refused("must be 16-byte aligned", who, out=aligned(8, seg_ref.DTYPE, SENT, off=8))
            raw = aligned(4 * 500 + 2, np.uint8)[2:2 + 4 * 500]
            refused("probs must be 4-byte aligned", who, probs=raw.view(np.float32))
        refused("null buffer", "vad_tails_device", slots=None)
        refused("more than 2\\^31 - 1 items", "vad_tails_device", n=1 << 31)
        bad = _ffi.VAD_ERR_BAD_SLOT
        refused("slot 99 is not an open stream", "vad_tails_device", code=bad, slots=[int(slots[0]), 99, int(slots[1])])
        refused("appears twice", "vad_tails_device", code=bad, slots=[int(slots[0]), int(slots[1]), int(slots[0])])
        assert lib.vad_tails_device(None, None, None, None, None, 0, None, None) == INV
        assert lib.vad_resegment_tails_device(None, None, None, None, 0, None, 1, None, None) == INV
    finally:
        close(eng, slots)


# ---- the mark, and the host forms' refusals ---------------------------------------------------------------------------
def test_the_mark_and_the_refusals_of_the_host_forms(lib, make_engine):
    eng = make_engine()
    frame = hop = eng.frame_samples
    recs = [script([0.0] * 2 + [0.9] * 6, frame, hop), script([0.9] * 5 + [0.0] * 4, frame, hop)]
    sets = [BASE[0], BASE[2]]

    def gone():
        rc, msg, out = raw_tails(lib, eng, 2)
        assert rc == INV and "vad_scan_tails: no scan results are resident" in msg and msg.startswith("Model prediction failed: ") and untouched(out), msg
        rc, msg, out = raw_reseg_tails(lib, eng, sets, 2)
        assert rc == INV and "vad_scan_resegment_tails: no scan results are resident" in msg and untouched(out), msg
        with pytest.raises(Exception, match="no scan results are resident"):
            eng.scan_tails()

    gone()                                                  # a fresh engine
    slots = np.asarray(eng.open_streams(2))
    extra = int(eng.open_stream())
    want = None
    try:
        def rescan():
            nonlocal want
            eng.reset(slots)
            eng.set_thresholds_many(slots, THR)
            eng.scan_segments(slots, recs, hop=hop, denoise=None)
            got = [eng.scan_tails()] + eng.resegment_tails(sets)
            assert want is None or all(same(g, w) for g, w in zip(got, want))
            want = [np.ascontiguousarray(g) for g in got]
            assert want[0]["nframes"].tolist() == [6, 0] and same(want[1], want[0])

        writers = {                                         # DESIGN 2.1m's list
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
        # calls that write neither array keep the mark: a cut, the table's read, thresholds, a replay, the tails themselves
        rescan()
        eng.cut([(0, 2, 6)], hop=hop, denoise=None)
        eng.set_thresholds_many(slots, BASE[1])
        eng.resegment(sets)
        assert same(eng.scan_tails(), want[0]) and all(same(g, w) for g, w in zip(eng.resegment_tails(sets), want[1:]))

        def refused(pattern, who, **kw):
            rc, msg, out = raw_tails(lib, eng, **kw) if who == "vad_scan_tails" else raw_reseg_tails(lib, eng, **kw)
            assert rc == INV and msg.startswith(f"Model prediction failed: {who}: ") and re.search(pattern, msg) and untouched(out), (rc, msg)

        refused("n = 3: the scan had 2 items", "vad_scan_tails", n=3)
        refused("n = 0: the scan had 2 items", "vad_scan_tails", n=0)
        refused("n = -1: the scan had 2 items", "vad_scan_tails", n=-1)
        refused("null buffer", "vad_scan_tails", n=2, out=None)
        who = "vad_scan_resegment_tails"
        refused("nt = 0: 1 .. 64 threshold sets", who, sets=sets, n=2, nt=0)
        refused("nt = -1: 1 .. 64 threshold sets", who, sets=sets, n=2, nt=-1)
        refused("nt = 65: 1 .. 64 threshold sets", who, sets=sets_of(65), n=2)
        refused("null buffer", who, sets=None, n=2, nt=2)
        refused("n = 1: the scan had 2 items", who, sets=sets, n=1)
        refused("null buffer", who, sets=sets, n=2, out=None)
        assert lib.vad_scan_tails(None, None, 0) == INV and lib.vad_scan_resegment_tails(None, None, 1, None, 0) == INV
        # an empty corpus is a valid result without tails
        eng.scan_segments(slots, [np.zeros(0, np.float32), np.zeros(100, np.float32)], hop=hop, denoise=None)
        assert eng.scan_tails().tobytes() == bytes(48) and [t.tobytes() for t in eng.resegment_tails(sets)] == [bytes(48)] * 2
        eng.scan_segments(slots[:0], [], hop=hop, denoise=None)
        assert len(eng.scan_tails()) == 0 and [len(t) for t in eng.resegment_tails(sets)] == [0, 0]
    finally:
        close(eng, list(slots) + [extra])


# ---- the Python surface -----------------------------------------------------------------------------------------------
def cfg_of(s, frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=s[0], vad_end_probability=s[1], voice_start_ratio=s[2],
                     voice_end_ratio=s[3], voice_start_frame_count=s[4], voice_end_frame_count=s[5], **{"enable_denoising": False, **kw})


def test_open_end_appends_the_tail_ranges_and_nothing_else(lib, make_engine):
    from cutter_vad_amd import ConfigurationError, scan_recordings, sweep_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(2)
    mono = lambda n: script(speechy(rng, n), frame, hop)
    st = lambda n: np.ascontiguousarray(np.stack([mono(n), mono(n)], axis=1))
    recs = [mono(40), st(55), mono(0), st(31), np.zeros((0, 2), np.float32), mono(58), mono(1), script([0.0, 0.9, 0.9, 0.8], frame, hop)]
    cfgs = [cfg_of(s, frame) for s in (BASE[0], BASE[1], BASE[2], EMPTY, BASE[5])]
    for channel in ("mix", "split"):
        lists = lambda res: [lst for r in res for lst in (r if channel == "split" else [r])]
        added = 0
        for stats in (False, True):
            closed = scan_recordings(recs, cfgs[0], engine=eng, hop=hop, channel=channel, stats=stats)
            assert scan_recordings(recs, cfgs[0], engine=eng, hop=hop, channel=channel, stats=stats, open_end=False) == closed
            opened = scan_recordings(recs, cfgs[0], engine=eng, hop=hop, channel=channel, stats=stats, open_end=True)
            for c, o in zip(lists(closed), lists(opened)):
                assert o[:len(c)] == c and len(o) - len(c) in (0, 1)
                if len(o) > len(c):
                    added += 1
                    a, b = o[-1][:2]
                    assert not c or a >= c[-1][1] - frame + hop          # behind the last END's frame
                    assert len(o[-1]) == (4 if stats else 2) and (not stats or 0.0 < o[-1][2] <= o[-1][3] <= 1.0)
        assert added >= 4
        last = lists(scan_recordings(recs, cfgs[0], engine=eng, hop=hop, channel=channel, open_end=True))[-1]
        assert last[-1] == (hop, 3 * hop + frame)                       # frames 1 .. 3: the recording's end
        got = sweep_recordings(recs, cfgs, engine=eng, hop=hop, channel=channel, stats=True, open_end=True)
        want = [scan_recordings(recs, c, engine=eng, hop=hop, channel=channel, stats=True, open_end=True) for c in cfgs]
        assert got == want and got != sweep_recordings(recs, cfgs, engine=eng, hop=hop, channel=channel, stats=True)
        assert not any(lists(got[3]))

    class Old:
        frame_samples, sample_rate = frame, 16000

    for call in (lambda: scan_recordings(recs, cfgs[0], engine=Old(), open_end=True),
                 lambda: sweep_recordings(recs, cfgs, engine=Old(), open_end=True)):
        with pytest.raises(ConfigurationError, match="open_end"):
            call()


def test_cut_recordings_open_end_cuts_the_tail_like_any_segment(lib, make_engine):
    from cutter_vad_amd import ConfigurationError, cut_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(4)
    recs = [script([0.0, 0.9, 0.9, 0.0, 0.0, 0.0, 0.8, 0.9, 0.7], frame, hop), script(speechy(rng, 50), frame, hop), script([0.1] * 9, frame, hop)]
    recs[0][frame:2 * frame] += rng.uniform(-0.3, 0.3, frame).astype(np.float32) * (np.arange(frame) % hop != 0)
    recs[0][3 * frame:5 * frame] += rng.uniform(-0.3, 0.3, 2 * frame).astype(np.float32) * (np.arange(2 * frame) % hop != 0)
    cfg = cfg_of(THR, frame)
    closed = cut_recordings(recs, cfg, engine=eng, hop=hop, wav=False)
    opened = cut_recordings(recs, cfg, engine=eng, hop=hop, wav=False, open_end=True)
    assert [(a, b) for a, b, _ in opened[0]] == [(hop, 4 * hop + frame), (6 * hop, 8 * hop + frame)] and len(closed[0]) == 1
    for c, o in zip(closed, opened):
        assert len(o) - len(c) in (0, 1) and all(x[:2] == y[:2] and np.array_equal(x[2], y[2]) for x, y in zip(c, o))
    hand = np.concatenate([recs[0][f * hop:f * hop + frame] for f in range(6, 9)])
    assert opened[0][1][2].tolist() == (hand * np.float32(32767.0)).astype(np.int16).tolist() and np.abs(opened[0][1][2]).max() > 1000
    assert opened[2] == []
    ranged = cut_recordings(recs, cfg, engine=eng, hop=hop, wav=False, layout="range", open_end=True)
    assert ranged[0][1][2].tolist() == (recs[0][6 * hop:8 * hop + frame] * np.float32(32767.0)).astype(np.int16).tolist()

    class Old:
        frame_samples, sample_rate = frame, 16000

    with pytest.raises(ConfigurationError, match="open_end"):
        cut_recordings(recs, cfg, engine=Old(), open_end=True)


def _hipcc():
    import shutil
    return next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_the_new_kernels_compile_without_scratch_or_spills(tmp_path):
    """the snapshot, the tails and the replay that keeps its last state machine: from the compiler's own metadata"""
    import subprocess
    from cutter_vad_amd import _build
    seen = {}
    for f in ("scan_tails.hip", "scan_resegment.hip"):
        out = tmp_path / (f + ".s")
        subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only",
                        "-o", str(out), os.path.join(ROOT, "cutter_vad_amd", "csrc", f)], check=True, capture_output=True, timeout=600)
        for m in re.findall(r"\.name:\s*_Z\d+(vadk_\w+?)N4vadk.*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                            out.read_text(), re.S):
            seen[m[0]] = m[1:]
    assert {"vadk_tail_snapshot", "vadk_seg_tails", "vadk_tails_reseg_count"} <= set(seen), seen
    assert all(v == ("0", "0", "0") for v in seen.values()), seen


# ---- the order of the refusals ----------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, make_engine):
    """The order of the checks is behaviour.  The host forms: the sets (the replay form), the resident results, the scan's item
    count, the null output.  The device forms: the sets (the replay form), n, 2^31 items or n x nt, the null arguments, the
    positions, the null per-frame arrays, the 16- and 4-byte alignments, the slots; a call without items comes behind all of them
    and writes nothing.  Every fault at once, then one mended at a time; and a resident scan without a frame gives zeroed tails."""
    from tests import refusal_order as RO
    eng = make_engine()
    two = [BASE[0], BASE[1]]
    slots = eng.open_streams(2)
    s0, s1 = int(slots[0]), int(slots[1])
    null = lambda who: f"{who}: null buffer$"

    def tails_device(sl, ev, probs, start, n, out):
        return lib.vad_tails_device(eng.handle, RO.i64p(sl), RO.addr(ev), RO.addr(probs), RO.i64p(start), n, RO.addr(out), None)

    def reseg_device(ev, probs, start, n, sets, nt, out):
        return lib.vad_resegment_tails_device(eng.handle, RO.addr(ev), RO.addr(probs), RO.i64p(start), n, RO.thr(sets), nt, RO.addr(out), None)

    def host(resident, n, out):
        if resident:
            RO.resident(lib, eng, slots, resident)
        return lib.vad_scan_tails(eng.handle, RO.segp(out), n)

    def reseg_host(resident, sets, nt, n, out):
        if resident:
            RO.resident(lib, eng, slots, resident)
        return lib.vad_scan_resegment_tails(eng.handle, RO.thr(sets), nt, RO.segp(out), n)

    positions = (
        (INV, r"out_start\[0\] is negative", "start", RO.i64(0, 3, 2)),
        (INV, r"out_start decreases at item 1 \(2 after 3\)", "start", RO.i64(0, 3, 1 << 31)),
        (INV, r"more than 2\^31 - 1 frames in one call", "start", RO.i64(0, 3, 3)))
    arrays = lambda who: (
        (INV, null(who), "ev", RO.buf(16, 8)),
        (INV, null(who), "probs", RO.buf(16, 2)),
        (INV, "the events and the tails must be 16-byte aligned", "ev", RO.buf(16)),
        (INV, "the events and the tails must be 16-byte aligned", "out", RO.buf(96)),
        (INV, f"{who}: probs must be 4-byte aligned", "probs", RO.buf(16)))
    gone = "no scan results are resident: the engine's last vad_scan_segments or vad_scan_rate_segments failed, or a later call has reused " \
           "its per-frame arrays$"
    three = ((0.0, 0.0, 0.0), ())
    try:
        who = "vad_tails_device"
        RO.walk_one(lib, eng, tails_device, dict(sl=None, ev=None, probs=None, start=None, n=-1, out=None), (
            (INV, "n = -1: bad count", "n", 1 << 31),
            (INV, r"more than 2\^31 - 1 items", "n", 2),
            (INV, null(who), "sl", RO.i64(s0, s0)),
            (INV, null(who), "start", RO.i64(-1, 3, 2)),
            (INV, null(who), "out", RO.buf(96, 8))) + positions + arrays(who) + (
            (_ffi.VAD_ERR_BAD_SLOT, f"slot {s0} appears twice", "sl", RO.i64(s0, s1)),))
        who = "vad_resegment_tails_device"
        RO.walk_one(lib, eng, reseg_device, dict(ev=None, probs=None, start=None, n=-1, sets=None, nt=0, out=None), (
            (INV, r"nt = 0: 1 \.\. 64 threshold sets", "nt", 2),
            (INV, null(who), "sets", two),
            (INV, "n = -1: bad count", "n", 1 << 31),
            (INV, r"2147483648 items x 2 sets: more than 2\^31 - 1 replays", "n", 2),
            (INV, null(who), "start", RO.i64(-1, 3, 2)),
            (INV, null(who), "out", RO.buf(96, 8))) + positions + arrays(who))
        # no items: behind every check, VAD_OK, nothing written (a misaligned output is still refused)
        out = RO.buf(96)
        out[:] = SENT
        assert tails_device(None, None, None, None, 0, out[8:]) == INV and reseg_device(None, None, None, 0, two, 2, out[8:]) == INV
        assert tails_device(None, None, None, None, 0, out) == 0 and reseg_device(None, None, None, 0, two, 2, out) == 0
        eng.synchronize()
        assert untouched(out)

        out = RO.buf(96)
        RO.walk_one(lib, eng, host, dict(resident=None, n=5, out=None), (
            (INV, "vad_scan_tails: " + gone, "resident", three),
            (INV, "n = 5: the scan had 2 items", "n", 2),
            (INV, null("vad_scan_tails"), "out", out)))
        eng.step([s0], np.zeros((1, eng.frame_samples), np.float32))          # writes the per-frame arrays: the results are gone
        RO.walk_one(lib, eng, reseg_host, dict(resident=None, sets=None, nt=65, n=5, out=None), (
            (INV, r"nt = 65: 1 \.\. 64 threshold sets", "nt", 2),
            (INV, null("vad_scan_resegment_tails"), "sets", two),
            (INV, "vad_scan_resegment_tails: " + gone, "resident", three),
            (INV, "n = 5: the scan had 2 items", "n", 2),
            (INV, null("vad_scan_resegment_tails"), "out", out)))
        # a resident scan of no frames: zeroed tails
        for call, nbytes in ((lambda: host(((), ()), 2, out), 48), (lambda: reseg_host(((), ()), two, 2, 2, out), 96)):
            out[:] = SENT
            assert call() == 0 and out[:nbytes].tobytes() == bytes(nbytes) and untouched(out[nbytes:])
    finally:
        close(eng, slots)
