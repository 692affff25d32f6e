"""vad_scan_rate on the host side: exports, chunk counts, refusals, the plan on chunks (CSR positions, window splitting) and what the
call leaves resident - the real csrc/engine.cpp over the HIP stand-in (tests/standin.py).  The stand-in's resample launch writes
frames whose first sample is the chunk's first decoded sample, and its model makes p = |first sample of the frame|: a recording's
probabilities are |x[t * hop]|.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from cutter_vad_amd.utils.audio import AudioUtils
from tests import g711_ref as G
from tests import standin
from tests.cut_ref import FRAMES, INV, PCM16, raw_cut, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_rate_frame_count", "vad_scan_rate", "vad_scan_rate_device"]
FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}
CHUNK = {8000: 256, 24000: 768, 48000: 1536}
UNSUPPORTED = _ffi.VAD_ERR_UNSUPPORTED


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


def _raw(lib, eng, items, audio, fmt, sr, hop, out_start, channels=1, audio_samples=None, n_out=None, device=False):
    """vad_scan_rate (or vad_scan_rate_device: the stand-in's device memory is host memory) on sentinel-filled outputs
    -> (rc, message, probs, events, seg)"""
    arr = (_ffi.ScanChItem * max(1, len(items)))(*[_ffi.ScanChItem(*map(int, (tuple(it) + (0, 0))[:5])) for it in items])
    start = np.ascontiguousarray(out_start, np.int64)
    n_out = int(start[-1]) if n_out is None else n_out
    probs = np.full(n_out, np.float32(-7.0), np.float32)
    ev = np.full(n_out, 0x55, np.uint8)
    seg = np.full(n_out, -9, np.int32)
    audio = np.ascontiguousarray(audio)
    ns = audio.shape[0] if audio_samples is None else audio_samples
    sp = start.ctypes.data_as(C.POINTER(C.c_int64))
    if device:
        rc = lib.vad_scan_rate_device(eng.handle, arr, len(items), audio.ctypes.data, ns, channels, fmt, sr, hop, -1.0, sp,
                                      probs.ctypes.data, ev.ctypes.data, seg.ctypes.data, None)
    else:
        rc = lib.vad_scan_rate(eng.handle, arr, len(items), audio.ctypes.data, ns, channels, fmt, sr, hop, -1.0, sp,
                               probs.ctypes.data_as(C.POINTER(C.c_float)), ev.ctypes.data_as(C.POINTER(C.c_uint8)),
                               seg.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, lib.vad_last_error(eng.handle).decode(), probs, ev, seg


def _untouched(probs, ev, seg):
    return (probs == np.float32(-7.0)).all() and (ev == 0x55).all() and (seg == -9).all()


def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header


def test_frame_count_is_split_into_frames_at_the_input_rate(lib, make_engine):
    eng = make_engine()
    for sr, chunk in CHUNK.items():
        assert eng.scan_chunk_samples(sr) == chunk == 512 * sr // 16000
        for hop in (chunk // 2, chunk, 4, chunk + 4):
            for ns in (0, chunk - 1, chunk, chunk + hop - 1, chunk + hop, 7 * chunk + 3):
                want = 0 if ns < chunk else (ns - chunk) // hop + 1
                if ns >= chunk - hop and hop <= chunk:
                    assert want == len(AudioUtils.split_into_frames(np.zeros(ns, np.float32), chunk, hop))
                assert lib.vad_scan_rate_frame_count(eng.handle, ns, sr, hop) == want, (sr, ns, hop)
                assert eng.scan_frame_count(ns, hop, sample_rate=sr) == want
        assert eng.scan_frame_count(3 * chunk, sample_rate=sr) == 5            # the default hop: half a chunk
    # 16 kHz: the engine's own frames
    assert lib.vad_scan_rate_frame_count(eng.handle, 2048, 16000, 256) == lib.vad_scan_frame_count(eng.handle, 2048, 256) == 7
    assert eng.scan_frame_count(2048, 256, sample_rate=16000) == eng.scan_frame_count(2048, 256) == 7
    for bad in ((100, 8000, 0), (-1, 8000, 128), (100, 44100, 128), (100, 0, 128)):
        assert lib.vad_scan_rate_frame_count(eng.handle, *bad) == -1, bad
    assert lib.vad_scan_rate_frame_count(None, 100, 8000, 128) == -1


def test_refusals_have_a_status_the_functions_name_and_write_nothing(lib, make_engine):
    eng = make_engine()
    a, b = (int(s) for s in eng.open_streams(2))
    sr, chunk, hop = 24000, 768, 384
    x = np.zeros(8192, np.float32)
    ok = [(a, 0, 1536), (b, 1536, 2304)]
    start = [0, 3, 8]                                   # 3 and 5 chunks
    for device in (False, True):
        rc, msg, probs, _, _ = _raw(lib, eng, ok, x, FMT["f32"], sr, hop, start, device=device)
        assert rc == _ffi.VAD_OK and (probs == 0).all(), msg

    def refused(code, pattern, *args, **kw):
        for device in (False, True):
            rc, msg, probs, ev, seg = _raw(lib, eng, *args, device=device, **kw)
            assert rc == code, (rc, msg)
            assert re.search(pattern, msg), msg
            if code != _ffi.VAD_ERR_BAD_SLOT:           # (the slot check is every entry point's, and names the slot)
                assert "vad_scan_rate_device" in msg if device else re.search(r"vad_scan_rate\b(?!_)", msg), msg
            assert _untouched(probs, ev, seg)           # a refused call writes nothing

    for h in (0, 2, 6, -384, 386):
        refused(INV, "hop", ok, x, FMT["f32"], sr, h, start)
    refused(INV, "multiple of 4", [(a, 2, 1536), (b, 1536, 2304)], x, FMT["f32"], sr, hop, start)
    refused(INV, "leaves the audio block", [(a, 0, 1536), (b, 6144, 2304)], x, FMT["f32"], sr, hop, start)
    refused(INV, "leaves the audio block", [(a, 0, -4), (b, 1536, 2304)], x, FMT["f32"], sr, hop, start)
    refused(INV, "2 GiB", ok, x, FMT["f32"], sr, hop, start, audio_samples=1 << 29)
    refused(INV, "2 GiB", ok, x, FMT["f32"], sr, hop, start, channels=2, audio_samples=1 << 28)
    refused(INV, "2 GiB", ok, x.view(np.uint8), FMT["ulaw"], sr, hop, start, audio_samples=1 << 31)
    refused(INV, "out_start", ok, x, FMT["f32"], sr, hop, [0, 3, 7], n_out=8)
    refused(INV, "out_start", ok, x, FMT["f32"], sr, hop, [0, 4, 8])
    refused(INV, "out_start", ok, x, FMT["f32"], sr, 256, start)     # the counts of 16 kHz frames are not the chunks'
    refused(INV, "channels = 3", ok, x, FMT["f32"], sr, hop, start, channels=3)
    refused(INV, "names channel 1 of 1", [(a, 0, 1536, 1), (b, 1536, 2304)], x, FMT["f32"], sr, hop, start)
    refused(INV, "reserved", [(a, 0, 1536, 0, 5), (b, 1536, 2304)], x, FMT["f32"], sr, hop, start)
    refused(_ffi.VAD_ERR_BAD_SLOT, "twice", [(a, 0, 1536), (a, 1536, 2304)], x, FMT["f32"], sr, hop, start)
    refused(_ffi.VAD_ERR_BAD_SLOT, "not an open stream", [(a, 0, 1536), (63, 1536, 2304)], x, FMT["f32"], sr, hop, start)
    for rate in (44100, 32000, 0, -8000, 16001):
        refused(UNSUPPORTED, "supported input rates are 8000, 16000, 24000, 48000", ok, x, FMT["f32"], rate, hop, start)
    rc, msg, probs, ev, seg = _raw(lib, eng, ok, x, 9, sr, hop, start)
    assert rc == INV and "format" in msg and _untouched(probs, ev, seg), msg
    # the device block's alignment: 4 bytes, 8 for two channels
    base = np.zeros(2 * 8192 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 8192]
    rc, msg, probs, ev, seg = _raw(lib, eng, ok, odd, FMT["ulaw"], sr, hop, start, channels=2, audio_samples=8192, device=True)
    assert rc == INV and "vad_scan_rate_device: the audio block must be 8-byte aligned" in msg and _untouched(probs, ev, seg), msg
    rc, msg, probs, ev, seg = _raw(lib, eng, ok, odd[2:], FMT["ulaw"], sr, hop, start, audio_samples=8192, device=True)
    assert rc == INV and "must be 4-byte aligned" in msg and _untouched(probs, ev, seg), msg
    with pytest.raises(Exception, match="hop"):
        eng.scan([a, b], [x[:1536], x[:2304]], hop=6, sample_rate=sr)
    with pytest.raises(Exception, match="supported input rates"):
        eng.scan([a, b], [x[:1536], x[:2304]], sample_rate=44100)

    for kw, pattern in ((dict(version=4), "needs a Silero V5 engine"), (dict(shared_gpu=True), "VAD_ENGINE_SHARED_GPU"),
                        (dict(rate=8000), "8 kHz sub-model")):
        other = make_engine(**kw)
        s = [(int(v), o, n) for v, (_, o, n) in zip(other.open_streams(2), ok)]
        for device in (False, True):
            for rate in (8000, 24000, 48000) + ((16000,) if kw.get("rate") == 8000 else ()):
                ch = CHUNK.get(rate, 512)
                items = [(s[0][0], 0, 2 * ch), (s[1][0], 2 * ch, 3 * ch)]
                rc, msg, probs, ev, seg = _raw(lib, other, items, x, FMT["f32"], rate, ch // 2, start, device=device)
                assert rc == UNSUPPORTED and re.search(pattern, msg) and "vad_scan_rate" in msg, (kw, rate, rc, msg)
                assert _untouched(probs, ev, seg)


def test_the_rate_is_settled_before_the_plan_checks_anything(lib, make_engine):
    """A call with an unsupported rate AND arguments the plan refuses hears about the rate, on both entry points."""
    eng = make_engine()
    a = int(eng.open_streams(1)[0])
    x = np.zeros(2048, np.float32)
    for device in (False, True):
        rc, msg, probs, ev, seg = _raw(lib, eng, [(a, 2, 1536)], x, 9, 44100, 6, [0, 1], channels=3, device=device)
        assert rc == UNSUPPORTED and "supported input rates" in msg and _untouched(probs, ev, seg), (device, rc, msg)


def _ragged(chunk, hop, kind, seed, two=False, counts=None):
    """37 recordings with 0, 1 and up to 23 chunks in no order of length, most with a tail that is dropped; every chunk's first
    sample is its own value -> (recordings, per recording the float32 values of the first samples, decoded: [chunks] or [chunks, 2])"""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = [0, 1, 0, 23, 2, 1] + [int(c) for c in rng.integers(0, 20, 31)]
        assert len(counts) == 37
    recs, first = [], []
    for c in counts:
        ns = (chunk + (c - 1) * hop + int(rng.integers(0, min(hop, 64)))) if c else int(rng.integers(0, chunk))
        shape = (ns, 2) if two else (ns,)
        if kind == "f32":
            x = rng.uniform(-0.9, 0.9, shape).astype(np.float32)
            d = x
        elif kind.startswith("i16"):
            x = rng.integers(-32768, 32768, shape).astype(np.int16)
            d = x.astype(np.float32) / np.float32(32767.0 if kind == "i16_32767" else 32768.0)
        else:
            x = rng.integers(0, 256, shape).astype(np.uint8)
            d = G.table(kind)[x].astype(np.float32) / np.float32(32768.0)
        recs.append(x)
        first.append(d[:c * hop:hop][:c].astype(np.float32))
        assert first[-1].shape[0] == c
    return recs, first


def _scan(eng, recs, hop, kind, sr, cap, **kw):
    """eng.scan(recs, sample_rate=sr) on fresh slots under launch cap `cap` -> (probs, model launches, frames counted, frames each
    stream has seen: the stand-in's "h")"""
    slots = eng.open_streams(len(recs))
    eng.set_scan_launch_frames(cap)
    try:
        before = eng.info()
        law = kind if kind in G.LAWS else None
        probs, ev, seg = eng.scan(slots, recs, hop=hop, law=law, i16_scale=32768 if kind == "i16_32768" else 32767, denoise=None,
                                  sample_rate=sr, **kw)
        after = eng.info()
        assert [e.shape for e in ev] == [p.shape for p in probs] == [g.shape for g in seg]
        seen = [int(eng.get_state(int(s))[0]) for s in slots]
        return probs, after["steps"] - before["steps"], after["frames"] - before["frames"], seen
    finally:
        eng.set_scan_launch_frames(0)
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("sr,kind,hop_name", [(8000, "f32", "half"), (24000, "i16_32767", "half"), (48000, "ulaw", "half"),
                                              (24000, "alaw", "chunk"), (8000, "i16_32768", "chunk4"), (48000, "f32", "hop4")])
def test_caps_1_2_and_5_give_the_ragged_corpus_identical_results_at_the_csr_positions(lib, make_engine, sr, kind, hop_name):
    eng = make_engine()
    chunk = CHUNK[sr]
    hop = {"half": chunk // 2, "chunk": chunk, "chunk4": chunk + 4, "hop4": 4}[hop_name]
    recs, first = _ragged(chunk, hop, kind, seed=sr // 1000 + len(kind))
    longest = max(f.shape[0] for f in first)
    assert longest == 23
    for cap in (1, 2, 5, 0):
        probs, launches, frames, seen = _scan(eng, recs, hop, kind, sr, cap)
        for i, f in enumerate(first):
            assert np.array_equal(probs[i], np.minimum(np.abs(f), np.float32(1.0))), (cap, i)
        assert seen == [f.shape[0] for f in first]      # no stream stepped past its recording's last chunk
        assert launches == -(-longest // (cap or 192)) and frames == sum(f.shape[0] for f in first)


def test_a_window_cut_by_the_window_buffer_not_by_the_cap(lib, make_engine):
    """1 366 live recordings of up to 100 chunks (tests/test_gpu_scan_rate_edges.py's batch, 8 kHz, hop 4): the 256 MiB window buffer
    holds 131 072 // 1 366 = 95 chunks of each, so the scan is two windows - t0 = 0 with W = 95, and t0 = 95 over the recordings that
    go on - where the cap of 192 and the longest recording would give one.  The stand-in's model reads frame t of item i at row
    i * W + t - t0 of the window through the window's item table, so a wrong W, live count or t0 in either launch moves a
    probability; no stream steps past its last chunk.  Windows of 32 chunks (the cap binds): four launches, the same results."""
    from tests.test_gpu_scan_rate_edges import WIN_ROWS, buffer_window_counts, launches
    eng = make_engine(max_streams=2048)
    sr, chunk, hop = 8000, 256, 4
    counts = [int(c) for c in buffer_window_counts()]
    live, longest = sum(c > 0 for c in counts), max(counts)
    fit = WIN_ROWS // live
    assert live == 1366 and fit == 95 < longest == 100 and {0, 1, 95, 96} <= set(counts)
    recs, first = _ragged(chunk, hop, "f32", seed=19, counts=counts)
    perm = np.random.default_rng(20).permutation(len(recs))
    for cap, want in ((0, -(-longest // fit)), (32, -(-longest // 32))):
        assert want == launches(counts, cap) == (4 if cap else 2)
        probs, got, frames, seen = _scan(eng, [recs[i] for i in perm], hop, "f32", sr, cap)
        for k, i in enumerate(perm):
            assert np.array_equal(probs[k], np.abs(first[i])), (cap, i)
        assert seen == [counts[i] for i in perm]
        assert got == want and frames == sum(counts)


@pytest.mark.parametrize("channel", ["mix", 0, 1, "split"])
def test_two_channel_recordings_are_selected_before_the_chunk_is_resampled(lib, make_engine, channel):
    eng = make_engine()
    sr, chunk = 24000, 768
    hop = chunk // 2
    recs, first = _ragged(chunk, hop, "i16_32767", seed=11, two=True, counts=[3, 0, 7, 1, 12, 5])
    pick = {"mix": lambda f: (f[:, 0] + f[:, 1]) * np.float32(0.5), 0: lambda f: f[:, 0], 1: lambda f: f[:, 1],
            "split": lambda f: f.T}[channel]
    slots = eng.open_streams(12 if channel == "split" else 6)
    try:
        sl = slots.reshape(6, 2) if channel == "split" else slots
        for cap in (2, 0):
            eng.reset(slots)
            eng.set_scan_launch_frames(cap)
            probs, _, _ = eng.scan(sl, recs, hop=hop, denoise=None, channel=channel, sample_rate=sr)
            for p, f in zip(probs, first):
                assert np.array_equal(p, np.abs(pick(f)).astype(np.float32)), (channel, cap)
    finally:
        eng.set_scan_launch_frames(0)
        for s in slots:
            eng.close_stream(int(s))


def test_nothing_is_written_outside_the_recordings_entries_and_16k_is_vad_scan_channels(lib, make_engine):
    eng = make_engine()
    sr, chunk = 8000, 256
    hop = chunk // 2
    recs, first = _ragged(chunk, hop, "f32", seed=5)
    slots = eng.open_streams(len(recs))
    try:
        offs = np.concatenate([[0], np.cumsum([(r.size + 3) & ~3 for r in recs])])
        audio = np.full(int(offs[-1]) + 8, 0.77, np.float32)
        for r, o in zip(recs, offs):
            audio[o:o + r.size] = r
        items = [(int(s), int(o), r.size) for s, o, r in zip(slots, offs, recs)]
        lib.vad_debug_scan_launch_frames(eng.handle, 4)
        for device in (False, True):
            eng.reset(slots)
            base = 0 if device else 5                   # the host entry point accepts a CSR that starts anywhere
            start = base + np.concatenate([[0], np.cumsum([f.size for f in first])])
            rc, msg, probs, ev, seg = _raw(lib, eng, items, audio, FMT["f32"], sr, hop, start, n_out=int(start[-1]) + 11, device=device)
            assert rc == _ffi.VAD_OK, msg
            for i, f in enumerate(first):
                assert np.array_equal(probs[start[i]:start[i + 1]], np.abs(f)), i
            out = np.ones(probs.size, bool)
            out[start[0]:start[-1]] = False
            assert _untouched(probs[out], ev[out], seg[out])
            assert (seg[~out] >= 0).all() and (ev[~out] != 0x55).all()
        # sr_in = 16000: vad_scan_channels on the same arguments, frames of 512 samples
        start16 = np.concatenate([[0], np.cumsum([eng.scan_frame_count(r.size, 256) for r in recs])])
        arr = (_ffi.ScanChItem * len(items))(*[_ffi.ScanChItem(*it, 0, 0) for it in items])
        want = np.zeros(int(start16[-1]), np.float32)
        eng.reset(slots)
        rc = lib.vad_scan_channels(eng.handle, arr, len(items), audio.ctypes.data, audio.size, 1, FMT["f32"], 256, -1.0,
                                   start16.ctypes.data_as(C.POINTER(C.c_int64)), want.ctypes.data_as(C.POINTER(C.c_float)), None, None)
        assert rc == _ffi.VAD_OK
        eng.reset(slots)
        rc, msg, probs, _, _ = _raw(lib, eng, items, audio, FMT["f32"], 16000, 256, start16)
        assert rc == _ffi.VAD_OK and np.array_equal(probs, want) and want.any(), msg
    finally:
        lib.vad_debug_scan_launch_frames(eng.handle, 0)
        for s in slots:
            eng.close_stream(int(s))


def test_a_chunk_with_a_nan_or_inf_is_rejected_and_the_stream_goes_on(lib, make_engine):
    eng = make_engine()
    sr, chunk = 48000, 1536
    x = np.full(5 * chunk, 0.25, np.float32)
    x[2 * chunk + 700] = np.nan                         # chunk 2 alone (hop = chunk)
    x[4 * chunk + 1535] = np.inf
    probs, launches, frames, seen = _scan(eng, [x], chunk, "f32", sr, 2)
    assert np.array_equal(np.isnan(probs[0]), [False, False, True, False, True])
    assert seen == [3] and launches == 3 and frames == 5


def test_a_rate_scan_leaves_no_block_for_a_cut_of_the_resident_one(lib, make_engine):
    eng = make_engine()
    slots = eng.open_streams(1)
    x = np.zeros(6000, np.int16)
    items = [(0, 1, 4, 0, 0)]
    try:
        probs, _, _ = eng.scan(slots, [x], hop=256, denoise=None)              # 16 kHz: the block stays
        rc, msg, out = raw_cut(lib, eng, items, None, 1, FMT["i16_32767"], 256, FRAMES, PCM16, 2048, thr=0.01, audio_samples=6000)
        assert rc == _ffi.VAD_OK, msg
        probs, _, _ = eng.scan(slots, [x], denoise=None, sample_rate=24000)    # 24 kHz: 14 chunks, and no block
        assert probs[0].size == 14 and eng.last_scan is None
        rc, msg, out = raw_cut(lib, eng, items, None, 1, FMT["i16_32767"], 256, FRAMES, PCM16, 2048, thr=0.01, audio_samples=6000)
        assert rc == INV and "no resident block" in msg and "vad_scan_cut" in msg and untouched(out), msg
    finally:
        eng.close_stream(int(slots[0]))


def test_scan_recordings_reports_ranges_in_input_rate_samples(lib, make_engine):
    from cutter_vad_amd import VADConfig
    from cutter_vad_amd.scan import scan_recordings
    eng = make_engine()
    sr, chunk = 48000, 1536
    hop = chunk // 2
    scripts = [np.array([0.0] * 3 + [0.9] * 6 + [0.0] * 5 + [0.9] * 4 + [0.0] * 4 + [0.9] * 2, np.float32),
               np.array([0.9] * 5, np.float32), np.zeros(0, np.float32), np.array([0.9] * 4 + [0.0] * 3, np.float32)]
    recs = []
    for k, s in enumerate(scripts):
        x = np.zeros(chunk + (s.size - 1) * hop + k if s.size else 9, np.float32)
        x[:s.size * hop:hop] = s
        recs.append(np.stack([x, x], axis=1) if k == 3 else x)          # a 2-D recording in a 1-D corpus
    cfg = VADConfig(sample_rate=16000, buffer_size=512, vad_start_probability=0.5, vad_end_probability=0.5,
                    voice_start_frame_count=2, voice_end_frame_count=2, enable_denoising=False)
    got = scan_recordings(recs, cfg, engine=eng, sample_rate=sr)
    slot = eng.open_streams(1)
    try:
        want = []
        for s in scripts:
            eng.reset(slot)
            eng.set_thresholds_many(slot, (0.5, 0.5, 0.8, 0.95, 2, 2))
            if s.size == 0:
                want.append([])
                continue
            ev_r, seg_r = eng.debug_sm_replay(int(slot[0]), s)
            want.append([((int(e) - int(seg_r[e]) + 1) * hop, int(e) * hop + chunk) for e in np.flatnonzero(ev_r & _ffi.VAD_EV_END)])
    finally:
        eng.close_stream(int(slot[0]))
    assert got == want and [len(g) for g in got] == [2, 0, 0, 1], got
    stats = scan_recordings(recs, cfg, engine=eng, sample_rate=sr, stats=True, channel=1)
    assert [[sg[:2] for sg in one] for one in stats] == want and all(len(sg) == 4 and sg[3] == pytest.approx(0.9) for one in stats for sg in one)
    assert scan_recordings(recs, cfg, engine=eng, sample_rate=16000, hop=hop) == scan_recordings(recs, cfg, engine=eng, hop=hop)
    with pytest.raises(ConfigurationError):
        scan_recordings(recs, cfg, engine=eng, sample_rate=44100)
