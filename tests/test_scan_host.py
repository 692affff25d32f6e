"""vad_scan on the host side: exports, frame counts, refusals, the plan (sorting, windows, CSR positions) and the segment helper -
the real csrc/engine.cpp over the HIP stand-in (tests/standin.py: p = |first sample of the frame|, the real state machine, a
stream held past its recording's end) - and the scan kernels' code-object budget from the compiler's own metadata.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.scan import speech_segments
from cutter_vad_amd.utils.audio import AudioUtils
from tests import g711_ref as G
from tests import standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_frame_count", "vad_scan", "vad_scan_device", "vad_debug_scan_launch_frames"]
FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}


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
    """Engine objects over the stand-in library (the product's loader knows one library: it is swapped for the constructor only)"""
    from cutter_vad_amd.engine import Engine
    made = []

    def make(version=5, rate=16000, max_streams=64, shared_gpu=False):
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


@pytest.fixture(scope="module")
def rate_engine(make_engine):
    """one engine per sample rate for the cases that open their slots, scan and close them again"""
    made = {}

    def get(rate):
        if rate not in made:
            made[rate] = make_engine(rate=rate)
        return made[rate]

    return get


def _raw(lib, eng, items, audio, fmt, hop, out_start, audio_samples=None, n_out=None, fill=None, device=False):
    """vad_scan (or vad_scan_device: the stand-in's device memory is host memory) -> (rc, message, probs, events, seg)"""
    arr = (_ffi.ScanItem * max(1, len(items)))(*[_ffi.ScanItem(*map(int, it)) for it in items])
    start = np.ascontiguousarray(out_start, np.int64)
    n_out = int(start[-1]) if n_out is None else n_out
    probs = np.full(n_out, np.float32(-7.0) if fill is None else fill, np.float32)
    ev = np.full(n_out, 0x55, np.uint8)
    seg = np.full(n_out, -9, np.int32)
    audio = np.ascontiguousarray(audio)
    ns = audio.size if audio_samples is None else audio_samples
    if device:
        rc = lib.vad_scan_device(eng.handle, arr, len(items), audio.ctypes.data, ns, fmt, hop, -1.0, start.ctypes.data_as(C.POINTER(C.c_int64)),
                                 probs.ctypes.data, ev.ctypes.data, seg.ctypes.data, None)
    else:
        rc = lib.vad_scan(eng.handle, arr, len(items), audio.ctypes.data, ns, fmt, hop, -1.0, start.ctypes.data_as(C.POINTER(C.c_int64)),
                          probs.ctypes.data_as(C.POINTER(C.c_float)), ev.ctypes.data_as(C.POINTER(C.c_uint8)),
                          seg.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, lib.vad_last_error(eng.handle).decode(), probs, ev, seg


def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header
    assert C.sizeof(_ffi.ScanItem) == 24


@pytest.mark.parametrize("rate", [16000, 8000])
def test_frame_count_is_split_into_frames(lib, make_engine, rate):
    eng = make_engine(rate=rate)
    frame = eng.frame_samples
    assert frame == (512 if rate == 16000 else 256)
    for hop in (frame // 2, frame, 4):
        for ns in (0, frame - 1, frame, frame + hop - 1, frame + hop, 7 * frame + 3):
            try:
                want = len(AudioUtils.split_into_frames(np.zeros(ns, np.float32), frame, hop))
            except ValueError:
                # shorter than frame - hop: the reference's count goes negative and numpy raises (utils/audio.py); such a
                # recording has no frame
                assert ns < frame - hop
                want = 0
            assert lib.vad_scan_frame_count(eng.handle, ns, hop) == want, (ns, hop)
            assert eng.scan_frame_count(ns, hop) == want
    assert lib.vad_scan_frame_count(eng.handle, 100, 0) == -1
    assert lib.vad_scan_frame_count(eng.handle, -1, 256) == -1
    assert lib.vad_scan_frame_count(None, 100, 256) == -1


def test_refusals_have_a_status_and_a_message(lib, make_engine):
    eng = make_engine()
    a, b = (int(s) for s in eng.open_streams(2))
    x = np.zeros(4096, np.float32)
    ok = [(a, 0, 1024), (b, 1024, 1536)]
    start = [0, 3, 8]                                   # hop 256: 3 and 5 frames
    rc, _, _, _, _ = _raw(lib, eng, ok, x, FMT["f32"], 256, start)
    assert rc == _ffi.VAD_OK

    def refused(code, pattern, *args, **kw):
        rc, msg, probs, _, _ = _raw(lib, eng, *args, **kw)
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert (probs == np.float32(-7.0)).all()        # a refused call writes nothing

    for hop in (0, 2, 6, -256, 258):
        refused(_ffi.VAD_ERR_INVALID_ARG, "hop", ok, x, FMT["f32"], hop, start)
    refused(_ffi.VAD_ERR_INVALID_ARG, "multiple of 4", [(a, 2, 1024), (b, 1024, 1536)], x, FMT["f32"], 256, start)
    refused(_ffi.VAD_ERR_INVALID_ARG, "leaves the audio block", [(a, 0, 1024), (b, 3072, 1536)], x, FMT["f32"], 256, start)
    refused(_ffi.VAD_ERR_INVALID_ARG, "leaves the audio block", [(a, 0, 1024), (b, 4100, 0)], x, FMT["f32"], 256, [0, 3, 3])
    refused(_ffi.VAD_ERR_INVALID_ARG, "leaves the audio block", [(a, 0, -4), (b, 1024, 1536)], x, FMT["f32"], 256, start)
    refused(_ffi.VAD_ERR_INVALID_ARG, "2 GiB", ok, x, FMT["f32"], 256, start, audio_samples=1 << 29)
    refused(_ffi.VAD_ERR_INVALID_ARG, "2 GiB", ok, x.view(np.uint8), FMT["ulaw"], 256, start, audio_samples=1 << 31)
    refused(_ffi.VAD_ERR_INVALID_ARG, "out_start", ok, x, FMT["f32"], 256, [0, 3, 7], n_out=8)
    refused(_ffi.VAD_ERR_INVALID_ARG, "out_start", ok, x, FMT["f32"], 256, [0, 4, 8])
    refused(_ffi.VAD_ERR_INVALID_ARG, "format", ok, x, 9, 256, start)
    refused(_ffi.VAD_ERR_BAD_SLOT, "twice", [(a, 0, 1024), (a, 1024, 1536)], x, FMT["f32"], 256, start)
    refused(_ffi.VAD_ERR_BAD_SLOT, "not an open stream", [(a, 0, 1024), (63, 1024, 1536)], x, FMT["f32"], 256, start)
    refused(_ffi.VAD_ERR_BAD_SLOT, "twice", [(a, 0, 1024), (a, 1024, 1536)], x, FMT["f32"], 256, start, device=True)
    assert lib.vad_debug_scan_launch_frames(eng.handle, -1) == _ffi.VAD_ERR_INVALID_ARG
    with pytest.raises(Exception, match="hop"):
        eng.scan([a, b], [x[:1024], x[:1536]], hop=6)

    for kw in (dict(version=4), dict(shared_gpu=True)):
        other = make_engine(**kw)
        s = [(int(v), o, n) for v, (_, o, n) in zip(other.open_streams(2), ok)]
        rc, msg, probs, _, _ = _raw(lib, other, s, x, FMT["f32"], 256, start)
        assert rc == _ffi.VAD_ERR_UNSUPPORTED and "vad_step_multi" in msg, (kw, rc, msg)
        rc, msg, _, _, _ = _raw(lib, other, s, x, FMT["f32"], 256, start, device=True)
        assert rc == _ffi.VAD_ERR_UNSUPPORTED and "vad_step_multi" in msg, (kw, rc, msg)
        assert (probs == np.float32(-7.0)).all()


def _ragged(frame, hop, kind, seed, counts=None):
    """37 recordings (the last tile is partial) with 0, 1 and up to 23 frames, in no order of length (or the frame counts given);
    every frame's first sample is its own scripted value.  -> (recordings, per recording the probabilities the stand-in gives)"""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = [0, 1, 0, 23, 2, 1] + [int(c) for c in rng.integers(0, 20, 31)]
        assert len(counts) == 37
    recs, want = [], []
    for i, c in enumerate(counts):
        ns = (frame + (c - 1) * hop + int(rng.integers(0, hop))) if c else int(rng.integers(0, frame))
        if kind == "f32":
            x = rng.uniform(-0.9, 0.9, ns).astype(np.float32)
            p = np.abs(x)
        elif kind.startswith("i16"):
            x = rng.integers(-32768, 32768, ns).astype(np.int16)
            p = np.abs(x.astype(np.float32) / np.float32(32767.0 if kind == "i16_32767" else 32768.0))
        else:
            x = rng.integers(0, 256, ns).astype(np.uint8)
            p = np.abs(G.table(kind)[x].astype(np.float32) / np.float32(32768.0))
        recs.append(x)
        want.append(np.minimum(p[:c * hop:hop][:c], np.float32(1.0)).astype(np.float32) if c else np.zeros(0, np.float32))
        assert want[-1].size == c
    return recs, want


HOPS = {"half": lambda f: f // 2, "hop4": lambda f: 4, "quarter4": lambda f: f // 4 + 4, "frame4": lambda f: f + 4,
        "16frames4": lambda f: 16 * f + 4}


def _scan_and_check(eng, recs, want, hop, kind, cap, launches):
    """eng.scan(recs) on fresh slots under launch cap `cap`: the stand-in's probabilities at the CSR positions, every stream
    stepped once per frame of its own recording, `launches` launches and sum(counts) frames on the engine's counters"""
    slots = eng.open_streams(len(recs))
    eng.set_scan_launch_frames(cap)
    try:
        before = eng.info()
        law = kind if kind in G.LAWS else None
        probs, ev, seg = eng.scan(slots, recs, hop=hop, law=law, i16_scale=32768 if kind == "i16_32768" else 32767, denoise=None)
        after = eng.info()
        assert len(probs) == len(recs)
        for i in range(len(recs)):
            assert np.array_equal(probs[i], want[i]), (i, probs[i], want[i])
            assert ev[i].shape == want[i].shape and seg[i].shape == want[i].shape
        # the stand-in's "h" counts the frames a stream has seen: none past the recording's end
        seen = [eng.get_state(int(s))[0] for s in slots]
        assert seen == [w.size for w in want]
        assert after["steps"] - before["steps"] == launches
        assert after["frames"] - before["frames"] == sum(w.size for w in want)
    finally:
        eng.set_scan_launch_frames(0)
        for s in slots:
            eng.close_stream(int(s))


def _ragged_cases():
    """every format x launch caps 1, 3 and the default, at every hop the argument check has a path for and both sub-models (the
    cases at 16 kHz and hop = frame / 2 keep the ids they had before the hop and the rate became parameters)"""
    out = []
    for rate in (16000, 8000):
        for hop_name in HOPS:
            for kind in FMT:
                for cap in (1, 3, 0):
                    first = rate == 16000 and hop_name == "half"
                    out.append(pytest.param(kind, cap, rate, hop_name, id=f"{kind}-{cap}" if first else f"{kind}-{cap}-{rate}-{hop_name}"))
    return out


@pytest.mark.parametrize("kind,cap,rate,hop_name", _ragged_cases())
def test_ragged_batch_lands_at_the_callers_csr_positions(lib, rate_engine, kind, cap, rate, hop_name):
    eng = rate_engine(rate)
    frame = eng.frame_samples
    hop = HOPS[hop_name](frame)
    recs, want = _ragged(frame, hop, kind, seed=len(kind) + cap)
    longest = max(w.size for w in want)
    per = cap if cap else 192
    _scan_and_check(eng, recs, want, hop, kind, cap, -(-longest // per))


@pytest.mark.parametrize("hop_name", ["hop4", "quarter4"])
@pytest.mark.parametrize("rate", [16000, 8000])
def test_default_cap_cuts_385_frames_into_three_launches(lib, rate_engine, rate, hop_name):
    """the product's own windows t0 = 0, 192, 384: recordings that end exactly on a window's edge (192, 384), one frame behind it
    (193, 385) and far in front of it"""
    eng = rate_engine(rate)
    frame = eng.frame_samples
    hop = HOPS[hop_name](frame)
    counts = [0, 1, 193, 2, 385, 192, 384, 40, 0, 17, 191, 33, 3, 385, 5, 194, 8, 1, 29, 383]
    recs, want = _ragged(frame, hop, "f32", seed=41, counts=counts)
    _scan_and_check(eng, recs, want, hop, "f32", 0, 3)


def test_4100_recordings_on_16_stream_tiles(lib, make_engine):
    """more recordings WITH a frame than any other multi-frame path keeps on 16-stream tiles: a launch covers the recordings that
    still have frames in its window, so 4 100 of them are 257 tiles, the last one with 4 streams; 8 more have no frame"""
    eng = make_engine(max_streams=8192)
    frame = eng.frame_samples
    hop = frame // 4 + 4
    rng = np.random.default_rng(43)
    counts = [int(c) for c in rng.integers(1, 7, 4100)]
    for k in rng.choice(4100, 8, replace=False):
        counts.insert(int(k), 0)
    assert set(counts) == set(range(7)) and sum(c > 0 for c in counts) == 4100 > 4096
    recs, want = _ragged(frame, hop, "f32", seed=44, counts=counts)
    for cap in (0, 2):
        _scan_and_check(eng, recs, want, hop, "f32", cap, -(-6 // (cap or 192)))


def test_a_batch_without_frames_launches_nothing_and_touches_nothing(lib, make_engine):
    """recordings that all have 0 frames, and n = 0: VAD_OK, no launch, the outputs and every stream's state as they were"""
    eng = make_engine()
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    rng = np.random.default_rng(47)
    slots = eng.open_streams(5)
    try:
        eng.set_thresholds_many(slots, (0.5, 0.5, 0.8, 0.95, 2, 2))
        for _ in range(3):                                 # a history: neither (h, c) nor the state machine is the fresh one
            eng.step(slots, rng.uniform(0.6, 0.9, (5, frame)).astype(np.float32), denoise=None)
        saved = [eng.save_stream(int(s)) for s in slots]
        state = [eng.get_state(int(s)).copy() for s in slots]
        assert all(st[0] == 3 for st in state)
        steps = eng.info()["steps"]
        frames = eng.info()["frames"]
        lens = [0, frame - 1, 17, frame - 4, 3]
        audio = rng.uniform(0.5, 0.9, 4 * frame).astype(np.float32)
        offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens[:-1]])])
        items = [(int(s), int(o), n) for s, o, n in zip(slots, offs, lens)]
        for device in (False, True):
            rc, msg, probs, ev, seg = _raw(lib, eng, items, audio, FMT["f32"], hop, [0] * 6, n_out=9, device=device)
            assert rc == _ffi.VAD_OK, msg
            assert (probs == np.float32(-7.0)).all() and (ev == 0x55).all() and (seg == -9).all()
            rc, msg, probs, ev, seg = _raw(lib, eng, [], audio, FMT["f32"], hop, [0], n_out=9, device=device)
            assert rc == _ffi.VAD_OK, msg
            assert (probs == np.float32(-7.0)).all() and (ev == 0x55).all() and (seg == -9).all()
        got = eng.scan(slots, [audio[o:o + n] for o, n in zip(offs, lens)], hop=hop, denoise=None)
        assert all(len(part) == 5 and all(a.size == 0 for a in part) for part in got)
        got = eng.scan([], [], hop=hop)
        assert got == ([], [], [])
        assert eng.info()["steps"] == steps and eng.info()["frames"] == frames
        assert [eng.save_stream(int(s)) for s in slots] == saved
        for s, st in zip(slots, state):
            assert np.array_equal(eng.get_state(int(s)), st)
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nothing_is_written_outside_the_recordings_entries(lib, make_engine, device):
    eng = make_engine()
    frame, hop = eng.frame_samples, eng.frame_samples
    recs, want = _ragged(frame, hop, "f32", seed=5)
    slots = eng.open_streams(len(recs))
    try:
        offs = np.concatenate([[0], np.cumsum([(r.size + 3) & ~3 for r in recs])])
        audio = np.full(int(offs[-1]) + 8, 0.77, np.float32)
        for r, o in zip(recs, offs):
            audio[o:o + r.size] = r
        base = 0 if device else 5                       # the host entry point accepts a CSR that starts anywhere
        start = base + np.concatenate([[0], np.cumsum([w.size for w in want])])
        items = [(int(s), int(o), r.size) for s, o, r in zip(slots, offs, recs)]
        lib.vad_debug_scan_launch_frames(eng.handle, 4)
        rc, msg, probs, ev, seg = _raw(lib, eng, items, audio, FMT["f32"], hop, start, n_out=int(start[-1]) + 11, device=device)
        assert rc == _ffi.VAD_OK, msg
        for i, w in enumerate(want):
            assert np.array_equal(probs[start[i]:start[i + 1]], w), i
        out = np.ones(probs.size, bool)
        out[start[0]:start[-1]] = False
        assert (probs[out] == np.float32(-7.0)).all() and (ev[out] == 0x55).all() and (seg[out] == -9).all()
        assert (seg[~out] >= 0).all() and (ev[~out] != 0x55).all()
    finally:
        lib.vad_debug_scan_launch_frames(eng.handle, 0)
        for s in slots:
            eng.close_stream(int(s))


def test_every_segment_length_comes_back_and_matches_a_replay(lib, make_engine):
    """two utterances in one recording, next to a short one: seg_frames on every END = vad_debug_sm_replay of the probabilities"""
    eng = make_engine()
    frame = eng.frame_samples
    script = np.array([0.0] * 3 + [0.9] * 6 + [0.0] * 5 + [0.9] * 4 + [0.0] * 4 + [0.9] * 2, np.float32)
    other = np.array([0.9] * 5, np.float32)
    recs = []
    for s in (script, other):
        x = np.zeros(s.size * frame, np.float32)
        x[::frame] = s
        recs.append(x)
    slots = eng.open_streams(3)
    thr = (0.5, 0.5, 0.8, 0.95, 2, 2)
    try:
        eng.set_thresholds_many(slots, thr)
        eng.set_scan_launch_frames(5)
        probs, ev, seg = eng.scan(slots[:2], recs, hop=frame, denoise=None)
        assert np.array_equal(probs[0], script)
        ev_r, seg_r = eng.debug_sm_replay(int(slots[2]), script)
        assert np.array_equal(ev[0], ev_r) and np.array_equal(seg[0], seg_r)
        ends = np.flatnonzero(ev[0] & _ffi.VAD_EV_END)
        assert ends.size == 2 and (seg[0][ends] > 0).all() and not seg[0][np.setdiff1d(np.arange(script.size), ends)].any()
        segs = speech_segments(ev[0], seg[0], frame, frame)
        assert segs == [((int(e) - int(seg[0][e]) + 1) * frame, int(e) * frame + frame) for e in ends]
        assert speech_segments(ev[1], seg[1], frame, frame) == []       # still open at the end: no END
    finally:
        eng.set_scan_launch_frames(0)
        for s in slots:
            eng.close_stream(int(s))


def test_two_threads_scan_different_batches_on_one_engine(lib, make_engine):
    """engines are shared between the threads of a process (the pool hands every caller the same one): Engine.scan packs into one
    page-locked block per engine, so packing and the call are one critical section - concurrent scans, of sizes that make the block
    grow, each get their own recordings' results"""
    import threading
    eng = make_engine(max_streams=128)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    errors = []

    def worker(k):
        try:
            rng = np.random.default_rng(k)
            slots = eng.open_streams(20)
            for it in range(25):
                counts = rng.integers(0, 4 + 6 * it * (k + 1), 20)
                recs = [rng.uniform(-0.9, 0.9, frame + (int(c) - 1) * hop if c else 17).astype(np.float32) for c in counts]
                probs, _, _ = eng.scan(slots, recs, hop=hop, denoise=None)
                for c, r, p in zip(counts, recs, probs):
                    if not np.array_equal(p, np.abs(r[:int(c) * hop:hop][:int(c)])):
                        errors.append((k, it, int(c)))
            for s in slots:
                eng.close_stream(int(s))
        except Exception as e:                          # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]


def test_speech_segments_on_hand_built_arrays():
    E, S = _ffi.VAD_EV_END, _ffi.VAD_EV_START
    ev = np.array([0, S, 4, 4, 4 | E, 0, S, 4, 4 | E], np.uint8)
    seg = np.array([0, 0, 0, 0, 4, 0, 0, 0, 3], np.int32)
    # hop = frame / 2: END at frame 4, length 4 -> frames 1..4 -> samples [256, 4 * 256 + 512); END on the last frame, length 3
    assert speech_segments(ev, seg, 512, 256) == [(256, 1536), (6 * 256, 8 * 256 + 512)]
    assert speech_segments(ev, seg, 512, 512) == [(512, 5 * 512), (6 * 512, 9 * 512)]
    assert speech_segments(ev, seg, 256, 128) == [(128, 768), (768, 1280)]
    assert speech_segments(np.zeros(0, np.uint8), np.zeros(0, np.int32), 512, 256) == []
    rej = np.array([_ffi.VAD_EV_REJECTED, 4 | E], np.uint8)
    assert speech_segments(rej, np.array([0, 2], np.int32), 512, 256) == [(0, 768)]


@pytest.mark.parametrize("rate", [16000, 8000])
def test_segments_at_a_hop_longer_than_the_frame(lib, make_engine, rate):
    """hop = frame + 4: 4 samples between consecutive frames belong to none.  Each range is [(e - L + 1) hop, e hop + frame) and
    lies inside its recording - on hand-built event arrays, and from scan_recordings on scripted audio"""
    from cutter_vad_amd import VADConfig
    from cutter_vad_amd.scan import scan_recordings
    E, S = _ffi.VAD_EV_END, _ffi.VAD_EV_START
    frame = 512 if rate == 16000 else 256
    hop = frame + 4
    ev = np.array([0, S, 4, 4, 4 | E, 0, S, 4, 4 | E], np.uint8)
    seg = np.array([0, 0, 0, 0, 4, 0, 0, 0, 3], np.int32)
    ns = frame + 8 * hop + 3                            # a recording of 9 frames and a tail
    got = speech_segments(ev, seg, frame, hop)
    assert got == [(hop, 4 * hop + frame), (6 * hop, 8 * hop + frame)]
    assert all(0 <= a < b <= ns for a, b in got)
    assert got[1][1] == ns - 3                          # the last frame's last sample: the tail is in no segment

    eng = make_engine(rate=rate)
    assert eng.frame_samples == frame
    scripts = [np.array([0.0] * 3 + [0.9] * 6 + [0.0] * 5 + [0.9] * 4 + [0.0] * 4 + [0.9] * 2, np.float32),
               np.array([0.9] * 5, np.float32), np.zeros(0, np.float32), np.array([0.9] * 4 + [0.0] * 3, np.float32)]
    recs = []
    for k, s in enumerate(scripts):
        x = np.zeros(frame + (s.size - 1) * hop + k if s.size else 9, np.float32)
        x[:s.size * hop:hop] = s                        # the stand-in's p = |first sample of the frame|
        recs.append(x)
    cfg = VADConfig(sample_rate=rate, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5,
                    voice_start_frame_count=2, voice_end_frame_count=2, enable_denoising=False)
    got = scan_recordings(recs, cfg, engine=eng, hop=hop)
    slot = eng.open_streams(1)
    try:
        eng.set_thresholds_many(slot, (0.5, 0.5, 0.8, 0.95, 2, 2))
        want = []
        for s in scripts:
            eng.reset(slot)
            eng.set_thresholds_many(slot, (0.5, 0.5, 0.8, 0.95, 2, 2))
            if s.size == 0:
                want.append([])
                continue
            ev_r, seg_r = eng.debug_sm_replay(int(slot[0]), s)
            ends = np.flatnonzero(ev_r & E)
            want.append([((int(e) - int(seg_r[e]) + 1) * hop, int(e) * hop + frame) for e in ends])
    finally:
        eng.close_stream(int(slot[0]))
    assert got == want
    assert [len(g) for g in got] == [2, 0, 0, 1], got
    for x, segs in zip(recs, got):
        for a, b in segs:
            assert 0 <= a < b <= x.size and a % hop == 0 and (b - frame) % hop == 0


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_scan_instantiations_fit_the_code_object_budget(tmp_path):
    """{4 formats} x {16, 8 kHz}: no scratch, at most 160 KB of LDS (one workgroup per CU, like the other frame-loop instantiations)"""
    from cutter_vad_amd import _build
    out = tmp_path / "t16.s"
    flags = ["-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=8"]
    subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", *flags, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16.hip")], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?"
                         r"\.vgpr_spill_count:\s*(\d+)", text, re.S):
        meta[m.group(2)] = (int(m.group(1)), int(m.group(3)), int(m.group(4)))
    # _Z16silero_v5_scan16ILi<FMT>ELb<K8>EEv...
    scan = {re.match(r"_Z16silero_v5_scan16ILi(\d)ELb([01])EE", k).groups(): v for k, v in meta.items() if "silero_v5_scan16" in k}
    assert sorted(scan) == sorted((str(f), k) for f in range(4) for k in "01"), sorted(meta)
    for key, (lds, scratch, spills) in scan.items():
        assert scratch == 0 and spills == 0, (key, scratch, spills)
        assert lds <= 160 * 1024, (key, lds)
