"""vad_scan_channels on the host side: exports, refusals, the one-channel case against vad_scan, the plan on interleaved two-channel
recordings (left, right, mix, split, modes interleaved item by item) and the Python faces - the real csrc/engine.cpp over the HIP
stand-in (tests/standin.py: p = |first sample of the frame| of the chosen channel, or of the float32 mean of the decoded pair) -
and the two-channel kernels' code-object budget from the compiler's own metadata.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import g711_ref as G
from tests import standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_channels", "vad_scan_channels_device"]
FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}
MIX = _ffi.VAD_SCAN_MIX


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


@pytest.fixture(scope="module")
def eng(make_engine):
    return make_engine()


def _raw(lib, eng, items, audio, channels, fmt, hop, out_start, audio_samples=None, n_out=None, device=False):
    """vad_scan_channels (or _device: the stand-in's device memory is host memory) -> (rc, message, probs, events, seg);
    items: (slot, sample_offset, nsamples, channel[, reserved])"""
    arr = (_ffi.ScanChItem * max(1, len(items)))(*[_ffi.ScanChItem(*map(int, it)) for it in items])
    start = np.ascontiguousarray(out_start, np.int64)
    n_out = int(start[-1]) if n_out is None else n_out
    probs = np.full(n_out, np.float32(-7.0), np.float32)
    ev = np.full(n_out, 0x55, np.uint8)
    seg = np.full(n_out, -9, np.int32)
    audio = np.ascontiguousarray(audio)
    ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    sp = start.ctypes.data_as(C.POINTER(C.c_int64))
    if device:
        rc = lib.vad_scan_channels_device(eng.handle, arr, len(items), audio.ctypes.data, ns, channels, fmt, hop, -1.0, sp,
                                          probs.ctypes.data, ev.ctypes.data, seg.ctypes.data, None)
    else:
        rc = lib.vad_scan_channels(eng.handle, arr, len(items), audio.ctypes.data, ns, channels, fmt, hop, -1.0, sp,
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
    assert re.search(r"#define\s+VAD_SCAN_MIX\s+\(-1\)", header) and _ffi.VAD_SCAN_MIX == -1
    assert C.sizeof(_ffi.ScanChItem) == 32
    assert C.sizeof(_ffi.ScanItem) == 24
    m = re.search(r"typedef struct vad_scan_ch_item \{(.*?)\} vad_scan_ch_item;", header, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    assert fields == [("int64_t", "slot"), ("int64_t", "sample_offset"), ("int64_t", "nsamples"), ("int32_t", "channel"),
                      ("int32_t", "reserved")]
    assert [f[0] for f in _ffi.ScanChItem._fields_] == [f[1] for f in fields]


def test_refusals_have_a_status_and_a_message(lib, make_engine):
    eng = make_engine()
    a, b = (int(s) for s in eng.open_streams(2))
    x = np.zeros((4096, 2), np.float32)
    ok = [(a, 0, 1024, 0), (b, 1024, 1536, MIX)]
    start = [0, 3, 8]                                   # hop 256: 3 and 5 frames
    for device in (False, True):
        rc, msg, _, _, _ = _raw(lib, eng, ok, x, 2, FMT["f32"], 256, start, device=device)
        assert rc == _ffi.VAD_OK, msg

    def refused(code, pattern, *args, **kw):
        for device in (False, True):
            rc, msg, probs, ev, seg = _raw(lib, eng, *args, device=device, **kw)
            assert rc == code, (rc, msg)
            assert re.search(pattern, msg), msg
            assert "vad_scan_channels" in msg or "format" in msg or "slot" in msg.lower(), msg
            assert (probs == np.float32(-7.0)).all() and (ev == 0x55).all() and (seg == -9).all()   # a refused call writes nothing

    inv = _ffi.VAD_ERR_INVALID_ARG
    for channels in (0, 3, -1, 8):
        refused(inv, r"channels = -?\d+", ok, x, channels, FMT["f32"], 256, start, audio_samples=4096)
    refused(inv, "channel 2 of 2", [(a, 0, 1024, 0), (b, 1024, 1536, 2)], x, 2, FMT["f32"], 256, start)
    refused(inv, "channel -2 of 2", [(a, 0, 1024, -2), (b, 1024, 1536, 1)], x, 2, FMT["f32"], 256, start)
    refused(inv, "channel 1 of 1", [(a, 0, 1024, 1), (b, 1024, 1536, 0)], x, 1, FMT["f32"], 256, start)
    refused(inv, "reserved", [(a, 0, 1024, 0, 0), (b, 1024, 1536, 1, 7)], x, 2, FMT["f32"], 256, start)
    # the limit is on sample frames x channels x bytes per sample
    refused(inv, "2 GiB", ok, x, 2, FMT["f32"], 256, start, audio_samples=1 << 28)
    refused(inv, "2 GiB", ok, x, 2, FMT["i16_32768"], 256, start, audio_samples=1 << 29)
    refused(inv, "2 GiB", ok, x, 2, FMT["ulaw"], 256, start, audio_samples=1 << 30)
    # one quad below the limit is accepted (the device entry point: nothing is copied, and the items stay inside the real array)
    rc, msg, _, _, _ = _raw(lib, eng, ok, x, 2, FMT["ulaw"], 256, start, audio_samples=(1 << 30) - 4, device=True)
    assert rc == _ffi.VAD_OK, msg
    # vad_scan's own refusals, counted in sample frames
    for hop in (0, 2, 6, -256, 258):
        refused(inv, "hop", ok, x, 2, FMT["f32"], hop, start)
    refused(inv, "multiple of 4", [(a, 2, 1024, 0), (b, 1024, 1536, 1)], x, 2, FMT["f32"], 256, start)
    refused(inv, "leaves the audio block", [(a, 0, 1024, 0), (b, 3072, 1536, 1)], x, 2, FMT["f32"], 256, start)
    refused(inv, "out_start", ok, x, 2, FMT["f32"], 256, [0, 4, 8])
    refused(inv, "format", ok, x, 2, 9, 256, start)
    refused(_ffi.VAD_ERR_BAD_SLOT, "twice", [(a, 0, 1024, 0), (a, 0, 1024, 1)], x, 2, FMT["f32"], 256, [0, 3, 6])
    # the device entry point's alignment: 8 bytes for two channels, and it says so
    base = np.zeros(2 * 4096 + 16, np.uint8)
    off = (4 - base.ctypes.data) % 8
    odd = base[off:off + 2 * 4096]
    assert odd.ctypes.data % 8 == 4
    rc, msg, probs, _, _ = _raw(lib, eng, ok, odd, 2, FMT["ulaw"], 256, start, audio_samples=4096, device=True)
    assert rc == inv and "8-byte aligned" in msg, (rc, msg)
    assert (probs == np.float32(-7.0)).all()


def test_a_call_with_several_faults_gets_the_first_refusal_of_the_plan(lib, make_engine):
    """The order of the plan's checks is behaviour: frame format, channels, max_streams, hop, the 2 GiB limit, then the items.
    Every fault at once, then one mended at a time."""
    eng = make_engine(max_streams=2)
    slots = [int(s) for s in eng.open_streams(2)]
    x = np.zeros((64, 2), np.float32)
    items = [(slots[0], 2, 16, 0), (slots[1], 0, 16, 0), (slots[0], 0, 16, 0)]     # three recordings, the first at an odd sample
    faults = dict(fmt=9, channels=3, n=3, hop=6, audio_samples=1 << 30)
    mended = dict(fmt=FMT["f32"], channels=2, n=2, hop=256, audio_samples=64)
    inv = _ffi.VAD_ERR_INVALID_ARG
    for key, pattern in (("fmt", "unknown frame format 9"), ("channels", "channels = 3"), ("n", "3 recordings, max_streams = 2"),
                         ("hop", "hop = 6 must be"), ("audio_samples", "exceed the 2 GiB"), (None, "starts at sample 2")):
        for device in (False, True):
            kw = faults
            rc, msg, probs, _, _ = _raw(lib, eng, items[:kw["n"]], x, kw["channels"], kw["fmt"], kw["hop"], [0] * (kw["n"] + 1), n_out=4,
                                        audio_samples=kw["audio_samples"], device=device)
            assert rc == inv and re.search(pattern, msg), (key, device, rc, msg)
            assert (probs == np.float32(-7.0)).all()
        if key:
            faults = dict(faults, **{key: mended[key]})


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True)], ids=["v4", "shared_gpu"])
def test_v4_and_shared_gpu_engines_are_unsupported(lib, make_engine, kw):
    other = make_engine(**kw)
    x = np.zeros((4096, 2), np.float32)
    a, b = (int(v) for v in other.open_streams(2))
    items = [(a, 0, 1024, 0), (b, 1024, 1536, MIX)]
    for device in (False, True):
        rc, msg, probs, ev, seg = _raw(lib, other, items, x, 2, FMT["f32"], 256, [0, 3, 8], device=device)
        assert rc == _ffi.VAD_ERR_UNSUPPORTED and "vad_step_multi" in msg and "vad_scan_channels" in msg, (kw, rc, msg)
        assert (probs == np.float32(-7.0)).all() and (ev == 0x55).all() and (seg == -9).all()


def _decode(x, kind):
    if kind == "f32":
        return x
    if kind.startswith("i16"):
        return x.astype(np.float32) / np.float32(32767.0 if kind == "i16_32767" else 32768.0)
    return G.table(kind)[x].astype(np.float32) / np.float32(32768.0)


def _values(rng, kind, ns):
    if kind == "f32":
        return rng.uniform(-0.9, 0.9, ns).astype(np.float32)
    if kind.startswith("i16"):
        return rng.integers(-32768, 32768, ns).astype(np.int16)
    return rng.integers(0, 256, ns).astype(np.uint8)


def _ragged2(frame, hop, kind, seed):
    """tests/test_scan_host.py's _ragged per channel: 37 two-channel recordings (the last tile is partial) with 0, 1 and up to 23
    frames in no order of length, the two channels' values independent.  -> (recordings [ns, 2], per recording the stand-in's
    probabilities {0: left, 1: right, MIX: of the float32 mean of the decoded pair})"""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 0, 23, 2, 1] + [int(c) for c in rng.integers(0, 20, 31)]
    assert len(counts) == 37
    recs, want = [], []
    for c in counts:
        ns = (frame + (c - 1) * hop + int(rng.integers(0, hop))) if c else int(rng.integers(0, frame))
        x = np.ascontiguousarray(np.stack([_values(rng, kind, ns), _values(rng, kind, ns)], axis=1))
        dl, dr = _decode(x[:, 0], kind), _decode(x[:, 1], kind)
        heard = {0: dl, 1: dr, MIX: ((dl + dr) * np.float32(0.5)).astype(np.float32)}
        if kind == "f32":
            assert np.array_equal(heard[MIX], np.mean(x, axis=1))
        recs.append(x)
        want.append({m: np.minimum(np.abs(v)[:c * hop:hop][:c], np.float32(1.0)).astype(np.float32) for m, v in heard.items()})
        assert all(w.size == c for w in want[-1].values())
    return recs, want


MODES = {"left": 0, "right": 1, "mix": "mix", "split": "split", "cycle": None}
KEY = {0: 0, 1: 1, "mix": MIX}


@pytest.mark.parametrize("cap", [1, 7, 0])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(FMT))
def test_ragged_stereo_batch_lands_at_the_callers_csr_positions(lib, eng, kind, mode, cap):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs, want = _ragged2(frame, hop, kind, seed=3 * len(kind) + cap + len(mode))
    n = len(recs)
    split = mode == "split"
    channel = [(0, 1, "mix")[i % 3] for i in range(n)] if mode == "cycle" else MODES[mode]
    slots = np.asarray(eng.open_streams(2 * n if split else n))
    eng.set_scan_launch_frames(cap)
    try:
        before = eng.info()
        law = kind if kind in G.LAWS else None
        probs, ev, seg = eng.scan(slots.reshape(n, 2) if split else slots, recs, hop=hop, law=law,
                                  i16_scale=32768 if kind == "i16_32768" else 32767, denoise=None, channel=channel)
        after = eng.info()
        assert len(probs) == len(ev) == len(seg) == n
        seen = [int(eng.get_state(int(s))[0]) for s in slots]
        for i in range(n):
            c = want[i][0].size
            if split:
                assert probs[i].shape == ev[i].shape == seg[i].shape == (2, c)
                assert np.array_equal(probs[i][0], want[i][0]), i
                assert np.array_equal(probs[i][1], want[i][1]), i
                assert seen[2 * i] == seen[2 * i + 1] == c
            else:
                m = KEY[channel[i] if mode == "cycle" else channel]
                assert probs[i].shape == ev[i].shape == seg[i].shape == (c,)
                assert np.array_equal(probs[i], want[i][m]), (i, m)
                assert seen[i] == c                     # the stand-in's "h" counts frames: none past the recording's end
        longest = max(w[0].size for w in want)
        assert after["steps"] - before["steps"] == -(-longest // (cap or 192))
        assert after["frames"] - before["frames"] == sum(w[0].size for w in want) * (2 if split else 1)
    finally:
        eng.set_scan_launch_frames(0)
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("kind", list(FMT))
def test_one_channel_is_vad_scan(lib, eng, kind):
    """vad_scan_channels(channels = 1), channel 0 and VAD_SCAN_MIX: the bytes vad_scan writes for the same block"""
    from tests.test_scan_host import _ragged
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    recs, want = _ragged(frame, hop, kind, seed=11)
    offs = np.concatenate([[0], np.cumsum([(r.size + 3) & ~3 for r in recs])])
    audio = np.zeros(int(offs[-1]) + 4, recs[0].dtype)
    for r, o in zip(recs, offs):
        audio[o:o + r.size] = r
    start = np.concatenate([[0], np.cumsum([w.size for w in want])])
    thr = (0.5, 0.5, 0.8, 0.95, 2, 2)
    got = []
    for which in ("scan", 0, MIX, "device"):
        slots = eng.open_streams(len(recs))
        try:
            eng.set_thresholds_many(slots, thr)
            if which == "scan":
                arr = (_ffi.ScanItem * len(recs))(*[_ffi.ScanItem(int(s), int(o), r.size) for s, o, r in zip(slots, offs, recs)])
                probs = np.full(int(start[-1]), np.float32(-7.0), np.float32)
                ev = np.full(probs.size, 0x55, np.uint8)
                seg = np.full(probs.size, -9, np.int32)
                rc = lib.vad_scan(eng.handle, arr, len(recs), audio.ctypes.data, audio.size, FMT[kind], hop, -1.0,
                                  start.ctypes.data_as(C.POINTER(C.c_int64)), probs.ctypes.data_as(C.POINTER(C.c_float)),
                                  ev.ctypes.data_as(C.POINTER(C.c_uint8)), seg.ctypes.data_as(C.POINTER(C.c_int32)))
                assert rc == _ffi.VAD_OK
            else:
                ch = 0 if which == "device" else which
                items = [(int(s), int(o), r.size, ch) for s, o, r in zip(slots, offs, recs)]
                rc, msg, probs, ev, seg = _raw(lib, eng, items, audio, 1, FMT[kind], hop, start, device=which == "device")
                assert rc == _ffi.VAD_OK, msg
            got.append((probs.tobytes(), ev.tobytes(), seg.tobytes(), [eng.save_stream(int(s)) for s in slots]))
        finally:
            for s in slots:
                eng.close_stream(int(s))
    for i, w in enumerate(want):
        assert np.array_equal(np.frombuffer(got[0][0], np.float32)[start[i]:start[i + 1]], w)
    for g in got[1:]:
        assert g[:3] == got[0][:3]
        assert g[3] == got[0][3]                        # every stream's saved state: (h, c) and the state machine's slot


def test_vad_scan_device_keeps_the_wording_of_its_refusals(lib, make_engine):
    """The plan is shared by four entry points now; what it refuses for vad_scan_device still reads "vad_scan: ...", and the
    entry point's own two checks "vad_scan_device: ...", as before there were four."""
    eng = make_engine()
    slot = int(eng.open_streams(1)[0])
    x = np.zeros(2048, np.float32)
    probs = np.zeros(8, np.float32)
    start = np.array([0, 4], np.int64)               # 2 048 samples back to back: 4 frames

    def call(audio, offset=0, hop=512):
        item = (_ffi.ScanItem * 1)(_ffi.ScanItem(slot, offset, 2048 - offset))
        rc = lib.vad_scan_device(eng.handle, item, 1, audio, 2048, FMT["f32"], hop, -1.0, start.ctypes.data_as(C.POINTER(C.c_int64)),
                                 probs.ctypes.data, None, None, None)
        return rc, lib.vad_last_error(eng.handle).decode()

    rc, msg = call(x.ctypes.data, hop=3)
    assert rc == _ffi.VAD_ERR_INVALID_ARG and msg == "Model prediction failed: vad_scan: hop = 3 must be a positive multiple of 4 samples"
    rc, msg = call(x.ctypes.data, offset=2)
    assert rc == _ffi.VAD_ERR_INVALID_ARG and msg.startswith("Model prediction failed: vad_scan: recording 0 starts at sample 2")
    rc, msg = call(x.ctypes.data + 2)
    assert rc == _ffi.VAD_ERR_INVALID_ARG and msg == "Model prediction failed: vad_scan_device: the audio block must be 4-byte aligned"
    rc, msg = call(None)
    assert rc == _ffi.VAD_ERR_INVALID_ARG and msg == "Model prediction failed: vad_scan_device: null buffer"
    eng.close_stream(slot)


def test_engine_scan_shapes_and_refusals_of_the_python_face(lib, eng):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(5)
    recs = [rng.uniform(-0.9, 0.9, (frame + 3 * hop + 5, 2)).astype(np.float32), np.zeros((0, 2), np.float32),
            rng.uniform(-0.9, 0.9, (frame, 2)).astype(np.float32)]
    slots = np.asarray(eng.open_streams(6))
    try:
        probs, ev, seg = eng.scan(slots.reshape(3, 2), recs, hop=hop, denoise=None, channel="split")
        assert [p.shape for p in probs] == [(2, 4), (2, 0), (2, 1)]
        assert [e.shape for e in ev] == [(2, 4), (2, 0), (2, 1)] and [g.shape for g in seg] == [(2, 4), (2, 0), (2, 1)]
        assert probs[0].dtype == np.float32 and ev[0].dtype == np.uint8 and seg[0].dtype == np.int32
        for c in range(2):
            assert np.array_equal(probs[0][c], np.abs(recs[0][:4 * hop:hop, c]))
        # the default is the mix, as VADWrapper mixes such an array down
        probs, _, _ = eng.scan(slots[:3], recs, hop=hop, denoise=None)
        assert np.array_equal(probs[0], np.abs(np.mean(recs[0], axis=1))[:4 * hop:hop])
        # 1-D input: as before, whatever `channel` is
        mono = [np.ascontiguousarray(r[:, 0]) for r in recs]
        for channel in ("mix", 1, "split"):
            probs, _, _ = eng.scan(slots[:3], mono, hop=hop, denoise=None, channel=channel)
            assert [p.shape for p in probs] == [(4,), (0,), (1,)]
            assert np.array_equal(probs[0], np.abs(mono[0][:4 * hop:hop]))
        with pytest.raises(Exception, match="all 1-D or all"):
            eng.scan(slots[:3], [recs[0], mono[1], recs[2]], hop=hop)
        with pytest.raises(Exception, match=r"\(3, 2\)"):
            eng.scan(slots[:3], recs, hop=hop, channel="split")
        with pytest.raises(Exception, match="channel must be"):
            eng.scan(slots[:3], recs, hop=hop, channel=2)
        with pytest.raises(Exception, match="channel must be"):
            eng.scan(slots[:3], recs, hop=hop, channel="left")
        with pytest.raises(Exception, match="2 channels for 3"):
            eng.scan(slots[:3], recs, hop=hop, channel=[0, 1])
        with pytest.raises(Exception, match="C-contiguous"):
            eng.scan(slots[:3], [recs[0][:, ::-1], recs[1], recs[2]], hop=hop)
        with pytest.raises(Exception, match="C-contiguous"):
            eng.scan(slots[:1], [np.zeros((frame, 3), np.float32)], hop=hop)
        # scan_device: two items on the same samples, one per channel
        block = np.ascontiguousarray(recs[0])
        n_f = 4
        out = np.full(2 * n_f, np.float32(-7.0), np.float32)
        start = eng.scan_device(slots[:2], [0, 0], [block.shape[0]] * 2, block.ctypes.data, block.shape[0], out.ctypes.data, hop=hop,
                                denoise=None, channels=2, channel=[1, "mix"])
        eng.synchronize()
        assert list(start) == [0, n_f, 2 * n_f]
        assert np.array_equal(out[:n_f], np.abs(block[:n_f * hop:hop, 1]))
        assert np.array_equal(out[n_f:], np.abs(np.mean(block, axis=1))[:n_f * hop:hop])
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_scan_recordings_on_a_corpus_of_both_kinds_keeps_the_callers_order(lib, make_engine):
    from cutter_vad_amd import VADConfig
    from cutter_vad_amd.scan import scan_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame

    def script(s):
        s = list(s) + [0.0] * (15 - len(s))             # one length, so that any two stack into a two-channel recording
        x = np.zeros(frame * len(s) + 3, np.float32)
        x[:len(s) * hop:hop] = s                        # the stand-in's p = |first sample of the frame|
        return x

    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4             # one utterance
    two = [0.9] * 4 + [0.0] * 4 + [0.9] * 3 + [0.0] * 4  # two
    none = [0.0] * 9
    loud = [1.0] * 4 + [0.0] * 5                        # against `anti`, the mix is silent
    anti = [-1.0] * 4 + [0.0] * 5
    st = lambda l, r: np.ascontiguousarray(np.stack([script(l), script(r)], axis=1))
    corpus = [script(one), st(two, none), script(none), st(none, one), st(loud, anti), np.zeros((0, 2), np.float32), script(two)]
    cfg = VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5,
                    voice_start_frame_count=2, voice_end_frame_count=2, enable_denoising=False)
    mono = lambda s: scan_recordings([script(s)], cfg, engine=eng, hop=hop)[0]
    s_one, s_two = mono(one), mono(two)
    assert len(s_one) == 1 and len(s_two) == 2 and mono(none) == []
    half = lambda s: scan_recordings([script(s) * np.float32(0.5)], cfg, engine=eng, hop=hop)[0]
    opened = eng.info()["open_streams"] if "open_streams" in eng.info() else None

    got = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=0)
    assert got == [s_one, s_two, [], [], mono(loud), [], s_two]
    got = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=1)
    assert got == [s_one, [], [], s_one, mono(loud), [], s_two]
    got = scan_recordings(corpus, cfg, engine=eng, hop=hop)             # mix: 0.9 against silence is 0.45, under the thresholds
    assert got == [s_one, half(two), [], half(one), [], [], s_two]
    assert half(two) == [] and got[4] == []
    got = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel="split")
    assert got == [[s_one], [s_two, []], [[]], [[], s_one], [mono(loud), mono(loud)], [[], []], [s_two]]
    if opened is not None:
        assert eng.info()["open_streams"] == opened     # every stream it opened is closed again
    with pytest.raises(Exception, match="channel"):
        scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=[0, 1])
    # a bad value is refused whatever the corpus holds: 1-D recordings alone never show it to Engine.scan
    for bad in ("left", 2, -1, None, 0.5):
        for some in (corpus, [script(one)], []):
            with pytest.raises(Exception, match="channel is 'mix', 0, 1 or 'split'"):
                scan_recordings(some, cfg, engine=eng, hop=hop, channel=bad)


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_stereo_instantiations_fit_the_code_object_budget(tmp_path):
    """{4 formats} x {16, 8 kHz} of silero_v5_stereo16: no scratch, no spills, at most 160 KB of LDS (one workgroup per CU)"""
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
    # _Z18silero_v5_stereo16ILi<FMT>ELb<K8>EEv...
    st = {re.match(r"_Z18silero_v5_stereo16ILi(\d)ELb([01])EE", k).groups(): v for k, v in meta.items() if "silero_v5_stereo16" in k}
    assert sorted(st) == sorted((str(f), k) for f in range(4) for k in "01"), sorted(meta)
    for key, (lds, scratch, spills) in st.items():
        assert scratch == 0 and spills == 0, (key, scratch, spills)
        assert lds <= 160 * 1024, (key, lds)
    sgpr_spills = dict(re.findall(r"\.name:\s*(\S*silero_v5_stereo16\S*).*?\.sgpr_spill_count:\s*(\d+)", text, re.S))
    assert len(sgpr_spills) == 8 and all(v == "0" for v in sgpr_spills.values()), sgpr_spills
