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


def _ragged(frame, hop, kind, seed):
    """37 recordings (the last tile is partial) with 0, 1 and up to 23 frames, in no order of length; every frame's first sample
    is its own scripted value.  -> (recordings, per recording the probabilities the stand-in gives)"""
    rng = np.random.default_rng(seed)
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


@pytest.mark.parametrize("cap", [1, 3, 0])
@pytest.mark.parametrize("kind", list(FMT))
def test_ragged_batch_lands_at_the_callers_csr_positions(lib, make_engine, kind, cap):
    eng = make_engine()
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs, want = _ragged(frame, hop, kind, seed=len(kind) + cap)
    slots = eng.open_streams(len(recs))
    eng.set_scan_launch_frames(cap)
    try:
        before = eng.info()
        law = kind if kind in G.LAWS else None
        probs, ev, seg = eng.scan(slots, recs, hop=hop, law=law, i16_scale=32768 if kind == "i16_32768" else 32767, denoise=None)
        after = eng.info()
        for i in range(len(recs)):
            assert np.array_equal(probs[i], want[i]), (i, probs[i], want[i])
            assert ev[i].shape == want[i].shape and seg[i].shape == want[i].shape
            # the stand-in's "h" counts the frames a stream has seen: none past the recording's end
            assert eng.get_state(int(slots[i]))[0] == want[i].size
        longest = max(w.size for w in want)
        per = cap if cap else 192
        assert after["steps"] - before["steps"] == -(-longest // per)
        assert after["frames"] - before["frames"] == sum(w.size for w in want)
    finally:
        eng.set_scan_launch_frames(0)
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
