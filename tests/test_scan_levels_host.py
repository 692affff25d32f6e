"""vad_scan_levels and vad_scan_cut_gain on the host side: exports, every refusal with its message and untouched outputs, the
resident-block rules for both kinds of block, n == 0, every kind of engine, values against tests/levels_ref.py, and the Python
faces (Engine.levels, Engine.cut(gains=), scan_recordings(levels=True), cut_recordings(normalize=), the AudioUtils helpers) - the
real csrc/engine.cpp over the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp restates the kernels' rule in plain
C++).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import standin
from tests.cut_ref import F32, FMT, FRAMES, INV, MIX, PCM16, RANGE, SENT16, SENT32, gate, heard, pcm16, raw_cut, untouched, values
from tests.levels_ref import levels_ref, of_cut, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_levels", "vad_scan_levels_device", "vad_scan_cut_gain", "vad_scan_cut_gain_device"]
SENT_LV = (0x5A5A5A5A5A5A5A5A, np.float32(-7.0), 0x5A5A5A5A)


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


def _items(items):
    return (_ffi.CutItem * max(1, len(items)))(*[_ffi.CutItem(*map(int, it)) for it in items])


def _block(audio, channels, audio_samples):
    if audio is None:
        return None, None, audio_samples
    audio = np.ascontiguousarray(audio)
    return audio, audio.ctypes.data, audio.size // max(channels, 1) if audio_samples is None else audio_samples


def raw_levels(lib, eng, items, audio, channels, fmt, hop, thr=-1.0, clip=0.95, sr_in=0, audio_samples=None, device=False, out="own"):
    """vad_scan_levels (or _device) -> (rc, message, records); items as tests/cut_ref.py's raw_cut; the records are pre-filled"""
    if isinstance(out, str):
        out = np.zeros(len(items) + 1, _ffi.LEVEL_DTYPE)
        out[:] = SENT_LV
    keep, ptr, ns = _block(audio, channels, audio_samples)
    optr = None if out is None else out.ctypes.data_as(C.POINTER(_ffi.Level))
    if device:
        rc = lib.vad_scan_levels_device(eng.handle, _items(items), len(items), ptr, ns, channels, fmt, sr_in, hop, thr, clip,
                                        None if out is None else out.ctypes.data, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_levels(eng.handle, _items(items), len(items), ptr, ns, channels, fmt, sr_in, hop, thr, clip, optr)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def raw_gain(lib, eng, items, gains, audio, channels, fmt, hop, layout, out_fmt, out_samples, thr=-1.0, sr_in=0, audio_samples=None,
             device=False):
    out = np.full(max(out_samples, 0) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)
    keep, ptr, ns = _block(audio, channels, audio_samples)
    g = None if gains is None else np.ascontiguousarray(gains, np.float32)
    gp = None if g is None else g.ctypes.data_as(C.POINTER(C.c_float))
    args = (eng.handle, _items(items), len(items), gp, ptr, ns, channels, fmt, sr_in, hop, thr, layout, out_fmt, out.ctypes.data, out_samples)
    if device:
        rc = lib.vad_scan_cut_gain_device(*args, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_cut_gain(*args)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def lv_untouched(out):
    return all((out[name] == v).all() for name, v in zip(("energy_q32", "peak", "clipped"), SENT_LV))


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
    m = re.search(r"typedef struct vad_level \{(.*?)\} vad_level;", header, re.S)
    fields = re.findall(r"(int64_t|int32_t|float)\s+(\w+);", m.group(1))
    assert fields == [("int64_t", "energy_q32"), ("float", "peak"), ("int32_t", "clipped")]
    assert [f[0] for f in _ffi.Level._fields_] == [f[1] for f in fields] == list(_ffi.LEVEL_DTYPE.names)
    assert C.sizeof(_ffi.Level) == 16 == _ffi.LEVEL_DTYPE.itemsize
    assert [_ffi.LEVEL_DTYPE.fields[n][1] for n in _ffi.LEVEL_DTYPE.names] == [getattr(_ffi.Level, n).offset for n in _ffi.LEVEL_DTYPE.names]
    from cutter_vad_amd import _build
    assert "scan_levels.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    assert "level_stats" in cutter_vad_amd.__all__


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_levels_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    x = np.zeros((4096, 2), np.float32) + np.float32(0.25)
    hop = 256
    ok = [(0, 0, 3, 0, 0), (1024, 2, 2, 0, MIX)]            # out_sample is not read: both say 0
    for device in (False, True):
        rc, msg, out = raw_levels(lib, eng, ok, x, 2, FMT["f32"], hop, device=device)
        assert rc == _ffi.VAD_OK, msg
        assert out[:2].tobytes() == records([np.full(1024, 0.25, np.float32), np.full(768, 0.25, np.float32)]).tobytes()
        assert lv_untouched(out[2:])

    def refused(pattern, items, audio=x, channels=2, fmt=FMT["f32"], hop=hop, **kw):
        for device in (False, True):
            rc, msg, out = raw_levels(lib, eng, items, audio, channels, fmt, hop, device=device, **kw)
            assert rc == INV, (rc, msg)
            assert re.search(pattern, msg), msg
            assert msg.startswith("Model prediction failed: ") and ("vad_scan_levels" in msg or "format" in msg), msg
            if out is not None:
                assert lv_untouched(out)

    for fmt in (5, -1, 9):
        refused("unknown frame format", ok, fmt=fmt)
    for channels in (0, 3, -1):
        refused(r"channels = -?\d", ok, channels=channels, audio_samples=4096)
    for h in (0, 2, 6, -256, 258):
        refused("hop = -?\\d+ must be a positive multiple of 4", ok, hop=h)
    refused("starts at sample 2, not a multiple of 4", [(2, 0, 3, 0, 0)])
    refused("starts at sample -4, not a multiple of 4", [(-4, 0, 3, 0, 0)])
    refused("first_frame = -1", [(0, -1, 3, 0, 0)])
    refused("nframes = 0", [(0, 0, 0, 0, 0)])
    refused("nframes = -2", [(0, 0, -2, 0, 0)])
    refused("leaves the audio block of 4096 samples", [(1024, 2, 11, 0, 0)])
    rc, msg, _ = raw_levels(lib, eng, [(1024, 2, 9, 0, 0)], x, 2, FMT["f32"], hop)
    assert rc == _ffi.VAD_OK, msg                           # ends ON the block's last sample
    refused("leaves the audio block", [(1 << 40, 0, 1, 0, 0)])
    refused("leaves the audio block", [(0, 1 << 40, 1, 0, 0)])
    refused("leaves the audio block", [(0, 0, 1 << 40, 0, 0)])
    refused("channel 2 of 2", [(0, 0, 3, 0, 2)])
    refused("channel -2 of 2", [(0, 0, 3, 0, -2)])
    refused("channel 1 of 1", [(0, 0, 3, 0, 1)], audio=x.reshape(-1), channels=1)
    refused("reserved = 7 must be 0", [(0, 0, 3, 0, 0, 7)])
    refused("2 GiB", ok, audio_samples=1 << 28)
    refused("2 GiB", ok, fmt=FMT["ulaw"], audio_samples=1 << 30)
    refused("clip_thresh is NaN", ok, clip=float("nan"))
    refused("null buffer", ok, out=None)
    # what a cut says about out_sample is no refusal here: negative, odd, overlapping
    rc, msg, out = raw_levels(lib, eng, [(0, 0, 3, -4, 0), (0, 0, 3, 2, 0), (0, 0, 3, 2, 0)], x, 2, FMT["f32"], hop)
    assert rc == _ffi.VAD_OK and out[0].tobytes() == out[1].tobytes() == out[2].tobytes(), msg
    # the device form's pointers
    for device, pat in ((True, "null buffer"), (False, "no resident block|resident block has")):
        rc, msg, out = raw_levels(lib, eng, ok, None, 2, FMT["f32"], hop, audio_samples=4095, device=device)
        assert rc == INV and re.search(pat, msg) and lv_untouched(out), msg
    base = np.zeros(2 * 4096 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 4096]
    rc, msg, out = raw_levels(lib, eng, [(0, 0, 3, 0, 0)], odd, 2, FMT["ulaw"], hop, audio_samples=4096, device=True)
    assert rc == INV and "vad_scan_levels_device: the audio block must be 8-byte aligned" in msg and lv_untouched(out), msg
    buf = np.zeros(64, np.uint8)
    mis = buf[(4 - buf.ctypes.data) % 8:][:32].view(_ffi.LEVEL_DTYPE)
    assert mis.ctypes.data % 8 == 4
    rc, msg, _ = raw_levels(lib, eng, [(0, 0, 3, 0, 0)], x, 2, FMT["f32"], hop, device=True, out=mis)
    assert rc == INV and "the levels must be 8-byte aligned" in msg and not buf.any(), msg
    rc, msg, _ = raw_levels(lib, eng, [(0, 0, 3, 0, 0)], x, 2, FMT["f32"], hop, device=False, out=mis)
    assert rc == _ffi.VAD_OK and mis[0].tobytes() == records([np.full(1024, 0.25, np.float32)]).tobytes(), msg
    # no segments: fine, and nothing is written - but the call's own arguments are still checked
    for device in (False, True):
        rc, msg, out = raw_levels(lib, eng, [], x, 2, FMT["f32"], hop, device=device)
        assert rc == _ffi.VAD_OK and lv_untouched(out), msg
        rc, msg, out = raw_levels(lib, eng, [], None, 2, FMT["f32"], hop, audio_samples=0, device=device, out=None)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = raw_levels(lib, eng, [], x, 2, FMT["f32"], 6, device=device)
        assert rc == INV and "hop = 6" in msg
    assert lib.vad_scan_levels(None, None, 0, None, 0, 1, 0, 0, 256, -1.0, 0.95, None) == INV
    # rates: 0 and the engine's own are the same call; others are vad_scan_rate_cut's
    rc, msg, a = raw_levels(lib, eng, ok, x, 2, FMT["f32"], hop, sr_in=16000)
    assert rc == _ffi.VAD_OK and a[:2].tobytes() == records([np.full(1024, 0.25, np.float32), np.full(768, 0.25, np.float32)]).tobytes()
    rc, msg, _ = raw_levels(lib, eng, ok, x, 2, FMT["f32"], hop, sr_in=44100)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "supported input rates" in msg and "vad_scan_levels" in msg, msg
    small = make_engine(rate=8000)
    rc, msg, _ = raw_levels(lib, small, ok, x, 2, FMT["f32"], hop, sr_in=48000)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "8 kHz sub-model" in msg, msg
    rc, msg, b = raw_levels(lib, small, ok, x, 2, FMT["f32"], hop, sr_in=8000)
    assert rc == _ffi.VAD_OK and b[:2].tobytes() == records([np.full(768, 0.25, np.float32), np.full(512, 0.25, np.float32)]).tobytes(), msg


def test_gain_refusals(lib, make_engine):
    eng = make_engine()
    x = np.zeros((4096, 2), np.float32) + np.float32(0.25)
    hop = 256
    ok = [(0, 0, 3, 0, 0), (1024, 2, 2, 1536, MIX)]
    n_out = 2560
    for device in (False, True):
        rc, msg, out = raw_gain(lib, eng, ok, [2.0, -1.0], x, 2, FMT["f32"], hop, FRAMES, F32, n_out, device=device)
        assert rc == _ffi.VAD_OK, msg
        assert (out[:1536] == np.float32(0.5)).all() and (out[1536:n_out] == np.float32(-0.25)).all() and untouched(out[n_out:])

        def refused(pattern, items=ok, gains=(1.0, 1.0), **kw):
            a = dict(audio=x, channels=2, fmt=FMT["f32"], hop=hop, layout=FRAMES, out_fmt=F32, out_samples=n_out)
            a.update(kw)
            rc, msg, out = raw_gain(lib, eng, items, gains, a["audio"], a["channels"], a["fmt"], a["hop"], a["layout"], a["out_fmt"],
                                    a["out_samples"], device=device, **{k: v for k, v in a.items() if k in ("audio_samples", "sr_in")})
            assert rc == INV and re.search(pattern, msg) and untouched(out), (rc, msg)
            assert msg.startswith("Model prediction failed: ") and ("vad_scan_cut_gain" in msg or "format" in msg), msg

        refused("null gains", gains=None)
        refused("segment 1: its gain is NaN", gains=(1.0, float("nan")))
        refused("segment 0: its gain is infinite", gains=(float("inf"), float("nan")))
        refused("segment 1: its gain is infinite", gains=(0.0, -float("inf")))
        # the cut's own refusals, under the new name
        refused(r"layout = 2", layout=2)
        refused(r"out_fmt = -1", out_fmt=-1)
        refused("unknown frame format", fmt=9)
        refused("hop = 6 must be", hop=6)
        refused("starts at sample 2", items=[(2, 0, 3, 0, 0)], gains=(1.0,))
        refused("leaves the audio block of 4096 samples", items=[(1024, 2, 11, 0, 0)], gains=(1.0,), out_samples=11 * 512)
        refused("out_sample = 2 .* multiple of 4", items=[(0, 0, 3, 2, 0)], gains=(1.0,))
        refused("output ranges of segments 0 and 1 overlap", items=[(0, 0, 3, 0, 0), (1024, 2, 2, 1532, MIX)])
        rc, msg, out = raw_gain(lib, eng, [], None, x, 2, FMT["f32"], hop, FRAMES, F32, n_out, device=device)
        assert rc == _ffi.VAD_OK and untouched(out), msg
    assert lib.vad_scan_cut_gain(None, None, 0, None, None, 0, 1, 0, 0, 256, -1.0, 0, 0, None, 0) == INV


# ---- the resident block -----------------------------------------------------------------------------------------------
def test_null_audio_names_the_resident_block_of_the_right_kind(lib, make_engine):
    eng = make_engine()
    hop = 256
    rng = np.random.default_rng(7)
    x = values(rng, "i16_32767", (6000, 2))
    items = [(0, 1, 4, 0, 1), (1024, 3, 2, 0, MIX)]
    i16 = FMT["i16_32767"]

    def null(ns=6000, channels=2, fmt=i16, sr_in=0, hop=hop, its=items):
        return raw_levels(lib, eng, its, None, channels, fmt, hop, thr=0.01, sr_in=sr_in, audio_samples=ns)

    rc, msg, out = null()
    assert rc == INV and "no resident block" in msg and "vad_scan_levels" in msg and lv_untouched(out), msg
    rc, msg, out = null(sr_in=48000)
    assert rc == INV and "no resident rate block" in msg and lv_untouched(out), msg
    # an explicit block becomes the resident one: own-rate ...
    rc, msg, want = raw_levels(lib, eng, items, x, 2, i16, hop, thr=0.01)
    assert rc == _ffi.VAD_OK, msg
    rc, msg, got = null()
    assert rc == _ffi.VAD_OK and got.tobytes() == want.tobytes(), msg
    rc, msg, got = null(sr_in=16000)
    assert rc == _ffi.VAD_OK and got.tobytes() == want.tobytes(), msg
    rc, msg, out = null(fmt=FMT["i16_32768"])
    assert rc == INV and "resident block has frame format 1, not 2" in msg and lv_untouched(out), msg
    rc, msg, out = null(channels=1, ns=12000, its=[(0, 1, 4, 0, 0)])
    assert rc == INV and "resident block has 2 channels, not 1" in msg and lv_untouched(out), msg
    rc, msg, out = null(ns=6008)
    assert rc == INV and "resident block has 24000 bytes, not the 24032 of 6008 samples" in msg and lv_untouched(out), msg
    rc, msg, out = null(sr_in=48000, hop=772)
    assert rc == INV and "no resident rate block" in msg and lv_untouched(out), msg          # an own-rate block named as a rate block
    # ... and the cut behind it reads the same block
    rc, msg, pay = raw_cut(lib, eng, [(0, 1, 4, 0, 1), (1024, 3, 2, 1280, MIX)], None, 2, i16, hop, RANGE, F32, 2048, thr=0.01, audio_samples=6000)
    assert rc == _ffi.VAD_OK and want[:2].tobytes() == records([pay[:1280], pay[1280:2048]]).tobytes(), msg
    # a rate block
    items48 = [(0, 0, 3, 0, 0), (4, 1, 2, 0, MIX)]
    rc, msg, want = raw_levels(lib, eng, items48, x, 2, i16, 772, thr=0.3, sr_in=48000)
    assert rc == _ffi.VAD_OK, msg
    ungated = [heard(x, "i16_32767", 0)[:2 * 772 + 1536], heard(x, "i16_32767", MIX)[4 + 772:4 + 2 * 772 + 1536]]
    assert want[:2].tobytes() == records(ungated).tobytes()
    rc, msg, got = raw_levels(lib, eng, items48, None, 2, i16, 772, sr_in=48000, audio_samples=6000)
    assert rc == _ffi.VAD_OK and got.tobytes() == want.tobytes(), msg
    rc, msg, out = raw_levels(lib, eng, items48, None, 2, i16, 772, sr_in=24000, audio_samples=6000)
    assert rc == INV and "resident block has sample rate 48000, not 24000" in msg and lv_untouched(out), msg
    rc, msg, out = null()
    assert rc == INV and "no resident block" in msg and lv_untouched(out), msg                # a rate block named as own-rate
    rc, msg, pay = raw_gain(lib, eng, [(0, 0, 3, 0, 0)], [0.5], None, 2, i16, 772, RANGE, F32, 3080, sr_in=48000, audio_samples=6000)
    assert rc == _ffi.VAD_OK and np.array_equal(pay[:3080], ungated[0] * np.float32(0.5)), msg


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_measures_and_gains(lib, make_engine, kw):
    other = make_engine(**kw)
    frame = other.frame_samples
    hop = frame // 2
    x = values(np.random.default_rng(3), "alaw", (4096, 2))
    items = [(4, 1, 3, 0, 1), (4, 0, 2, 3 * frame + 4, MIX)]
    for device in (False, True):
        rc, msg, out = raw_levels(lib, other, items, x, 2, FMT["alaw"], hop, thr=0.01, device=device)
        assert rc == _ffi.VAD_OK, (kw, msg)
        want = [gate(heard(x, "alaw", 1), 0.01)[4 + hop:4 + 3 * hop + frame], gate(heard(x, "alaw", MIX), 0.01)[4:4 + hop + frame]]
        assert out[:2].tobytes() == records(want).tobytes() and lv_untouched(out[2:])
        rc, msg, pay = raw_gain(lib, other, items, [1.0, 1.0], x, 2, FMT["alaw"], hop, FRAMES, PCM16, 5 * frame + 4, thr=0.01, device=device)
        rc2, msg2, plain = raw_cut(lib, other, items, x, 2, FMT["alaw"], hop, FRAMES, PCM16, 5 * frame + 4, thr=0.01, device=device)
        assert rc == rc2 == _ffi.VAD_OK and pay.tobytes() == plain.tobytes(), (msg, msg2)


# ---- values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [None, 0.3], ids=["nogate", "gate"])
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", list(FMT))
def test_levels_and_gains_against_numpy(eng, kind, channels, denoise):
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    rng = np.random.default_rng(len(kind) + 10 * channels)
    x = values(rng, kind, (20000, 2) if channels == 2 else 20000)
    chans = (0, 1, "mix") if channels == 2 else (0,)
    segs = [(off, 2 * k, 1 + 5 * k, chans[k % len(chans)]) for k, off in enumerate((0, 1028, 5000, 0, 1028))]
    kw = dict(hop=hop, audio=x, denoise=denoise, law=kind if kind in ("ulaw", "alaw") else None, i16_scale=32768 if kind == "i16_32768" else 32767)
    got = eng.levels(segs, clip=0.9, **kw)
    assert got.tobytes() == of_cut(eng, segs, 0.9, **kw).tobytes()
    want = []
    for sg in segs:
        a = sg[0] + sg[1] * hop
        want.append(gate(heard(x, kind, MIX if sg[3] == "mix" else sg[3]), denoise)[a:a + (sg[2] - 1) * hop + frame])
    assert got.tobytes() == records(want, 0.9).tobytes()
    gains = np.array([0.5, -3.0, 1.0, 2.0 ** -12, 40.0], np.float32)
    for layout in ("frames", "range"):
        f32, start = eng.cut(segs, layout=layout, out="f32", **kw)
        for out in ("f32", "pcm16"):
            plain, _ = eng.cut(segs, layout=layout, out=out, **kw)
            ones, _ = eng.cut(segs, layout=layout, out=out, gains=np.ones(5, np.float32), **kw)
            assert ones.tobytes() == plain.tobytes()
            g, _ = eng.cut(segs, layout=layout, out=out, gains=gains, **kw)
            scaled = np.concatenate([f32[start[i]:start[i + 1]] * gains[i] for i in range(5)]).astype(np.float32)
            assert g.tobytes() == (scaled if out == "f32" else pcm16(scaled)).tobytes()


def test_a_rate_frames_cut_with_gains_window_by_window(eng):
    rng = np.random.default_rng(48)
    kw = dict(hop=772, audio=values(rng, "i16_32767", (1536 + 40 * 772 + 40, 2)), denoise=0.01, sample_rate=48000)
    segs = [(0, 0, 15, 0), (0, 3, 1, 1), (4, 2, 39, "mix"), (0, 14, 20, "mix")]
    gains = np.array([0.5, 3.0, -0.75, 1.0], np.float32)
    whole, start = eng.cut(segs, layout="frames", out="f32", **kw)
    want = np.concatenate([whole[start[i]:start[i + 1]] * gains[i] for i in range(4)]).astype(np.float32)
    eng.set_scan_launch_frames(1)
    try:
        got, _ = eng.cut(segs, layout="frames", out="f32", gains=gains, **kw)
    finally:
        eng.set_scan_launch_frames(0)
    assert got.tobytes() == want.tobytes()
    assert eng.cut(segs, layout="frames", out="f32", gains=gains, **kw)[0].tobytes() == want.tobytes()


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_engine_levels_and_its_argument_errors(eng):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(5)
    recs = [values(rng, "f32", (frame + 5 * hop + 3, 2)), values(rng, "f32", (frame, 2))]
    slots = np.asarray(eng.open_streams(2))
    try:
        with eng.scan_session():
            eng.scan(slots, recs, hop=hop, denoise=None)
            last = eng.last_scan
            segs = [(0, 1, 3), (int(last["offsets"][1]), 0, 1, 1), (0, 0, 2, 0)]
            got = eng.levels(segs, hop=hop, denoise=0.3)
            assert got.tobytes() == of_cut(eng, segs, hop=hop, denoise=0.3).tobytes()
        assert got.dtype == _ffi.LEVEL_DTYPE and got.shape == (3,)
        block = np.zeros((last["samples"], 2), np.float32)
        block[:recs[0].shape[0]] = recs[0]
        block[int(last["offsets"][1]):] = recs[1]
        assert eng.levels(segs, hop=hop, denoise=0.3, audio=block).tobytes() == got.tobytes()
        assert eng.last_scan is None
        assert eng.levels([], hop=hop, audio=block).shape == (0,)
        out = np.zeros(4, _ffi.LEVEL_DTYPE)
        eng.levels_device(segs, block.ctypes.data, block.shape[0], out.ctypes.data, hop=hop, channels=2, denoise=0.3)
        eng.synchronize()
        assert out[:3].tobytes() == got.tobytes()
        with pytest.raises(Exception, match="follows a scan"):
            eng.levels(segs, hop=hop)
        with pytest.raises(Exception, match="a segment is"):
            eng.levels([(0, 1)], hop=hop, audio=block)
        with pytest.raises(Exception, match="1-D or"):
            eng.levels(segs, hop=hop, audio=np.zeros((64, 3), np.float32))
        with pytest.raises(Exception, match="leaves the audio block"):
            eng.levels([(0, 40, 3)], hop=hop, audio=block)
        with pytest.raises(Exception, match="clip_thresh is NaN"):
            eng.levels(segs, hop=hop, audio=block, clip=float("nan"))
        with pytest.raises(Exception, match="gains has 2 entries for 3 segments"):
            eng.cut(segs, hop=hop, audio=block, gains=[1.0, 2.0])
        with pytest.raises(Exception, match="segment 2: its gain is NaN"):
            eng.cut(segs, hop=hop, audio=block, gains=[1.0, 2.0, float("nan")])
    finally:
        for s in slots:
            eng.close_stream(int(s))


def _script(frame, s, amp=1.0, fill=0.125):
    """the stand-in's p = |first sample of the frame|: a recording whose frames have the probabilities `s`"""
    s = list(s) + [0.0] * (15 - len(s))
    x = np.full(frame * len(s) + 3, np.float32(fill), np.float32)
    x[:len(s) * frame:frame] = np.asarray(s, np.float32) * np.float32(amp)
    return x


def _cfg(frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5, voice_start_frame_count=2,
                     voice_end_frame_count=2, output_wav_sample_rate=8000, **kw)


def test_scan_recordings_levels_and_cut_recordings_normalize(make_engine):
    from cutter_vad_amd import SegmentRefine, cut_recordings, level_stats, scan_recordings, sweep_recordings
    eng = make_engine()
    frame = hop = eng.frame_samples
    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
    none = [0.0] * 9
    tail = [0.0] * 10 + [0.8] * 5                      # stops inside speech
    st = lambda l, r: np.ascontiguousarray(np.stack([_script(frame, l), _script(frame, r)], axis=1))
    corpus = [_script(frame, one), st(two, none), _script(frame, none), st(none, one), _script(frame, two, fill=0.0), _script(frame, tail)]
    for gate_on in (False, True):
        cfg = _cfg(frame, enable_denoising=gate_on)
        thr = 0.01 if gate_on else None
        for channel in (0, "mix", "split"):
            for kw in (dict(), dict(open_end=True), dict(open_end=True, refine=SegmentRefine(pad_before=1, pad_after=1, max_frames=3))):
                bare = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, stats=True, **kw)
                got = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, stats=True, levels=True, **kw)
                short = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, levels=True, **kw)
                n = 0
                for x, rb, rg, rs in zip(corpus, bare, got, short):
                    per = [(c, rb[c], rg[c], rs[c]) for c in range(len(rg))] if channel == "split" else [(channel, rb, rg, rs)]
                    for c, b_, g_, s_ in per:
                        assert [r[:4] for r in g_] == b_ and [r[:2] + r[4:] for r in g_] == s_
                        h = gate(x if x.ndim == 1 else heard(x, "f32", MIX if c == "mix" else c), thr)
                        for r in g_:
                            q, peak, clipped = levels_ref(h[r[0]:r[1]])
                            assert r[4:] == (float(np.sqrt(q / 2.0 ** 32 / (r[1] - r[0]))), float(peak), clipped), r
                            n += 1
                assert n >= 3      # (0.9 against silence mixes to 0.45, under the thresholds)
                if kw.get("open_end"):
                    assert len(got[5][0] if channel == "split" else got[5]) >= 1
                swept = sweep_recordings(corpus, [cfg, cfg], engine=eng, hop=hop, channel=channel, stats=True, levels=True, **kw)
                assert swept == [got, got]
    # clipped counts: the 0.96 frames of `two`
    cfg = _cfg(frame, enable_denoising=False)
    lv = scan_recordings([corpus[4]], cfg, engine=eng, hop=hop, levels=True)[0]
    assert [r[3:] for r in lv] == [(float(np.float32(0.7)), 0), (float(np.float32(0.96)), 3)]
    # normalize: the reference expression, segment by segment; the silent recording has no segment
    for layout in ("frames", "range"):
        for channel in ("mix", "split"):
            plain = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout=layout, wav=False, open_end=True)
            got = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout=layout, wav=False, open_end=True, normalize=0.9)
            wavs = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout=layout, open_end=True, normalize=0.9)
            n = 0
            for x, rp, rg, rw in zip(corpus, plain, got, wavs):
                per = [(c, rp[c], rg[c], rw[c]) for c in range(len(rg))] if channel == "split" else [(channel, rp, rg, rw)]
                for c, p_, g_, w_ in per:
                    assert [(a, b) for a, b, _ in g_] == [(a, b) for a, b, _ in p_]
                    h = x if x.ndim == 1 else heard(x, "f32", MIX if c == "mix" else c)
                    for (a, b, pcm), (_, _, wav) in zip(g_, w_):
                        peak = np.abs(h[a:b]).max()
                        assert pcm.tobytes() == pcm16(h[a:b] * np.float32(np.float32(0.9) / peak)).tobytes() == wav[44:]
                        assert np.abs(pcm.astype(np.int32)).max() == 29490
                        n += 1
            assert n >= 4 and got[2] == ([[]] if channel == "split" else [])
    with pytest.raises(Exception, match="its gain is"):
        cut_recordings(corpus[:1], cfg, engine=eng, hop=hop, normalize=float("inf"))
    assert level_stats(np.zeros(0, _ffi.LEVEL_DTYPE), [])[1].shape == (0,)
    e, rms = level_stats(np.array([(1 << 32, 1.0, 1), (0, 0.0, 0), (3 << 30, 0.5, 0)], _ffi.LEVEL_DTYPE), [4, 0, 3])
    assert e.tolist() == [1.0, 0.0, 0.75] and rms.tolist() == [0.5, 0.0, 0.5]


class _NoLevels:
    """an engine object of another make: everything a scan needs, no levels"""
    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        if name == "levels":
            raise AttributeError(name)
        return getattr(self._e, name)


def test_an_engine_object_without_levels_is_a_configuration_error(make_engine):
    from cutter_vad_amd import cut_recordings, scan_recordings, sweep_recordings
    eng = make_engine()
    frame = eng.frame_samples
    cfg = _cfg(frame, enable_denoising=False)
    corpus = [_script(frame, [0.0] * 2 + [0.9] * 5 + [0.0] * 4)]
    bare = _NoLevels(eng)
    assert scan_recordings(corpus, cfg, engine=bare, hop=frame) == scan_recordings(corpus, cfg, engine=eng, hop=frame) != [[]]
    opened = eng.info()["open_streams"]
    with pytest.raises(ConfigurationError, match="scan_recordings: levels=True needs an engine with levels.*_NoLevels has none"):
        scan_recordings(corpus, cfg, engine=bare, hop=frame, levels=True)
    with pytest.raises(ConfigurationError, match="sweep_recordings: levels=True needs an engine with levels"):
        sweep_recordings(corpus, [cfg], engine=bare, hop=frame, levels=True)
    with pytest.raises(ConfigurationError, match="cut_recordings: normalize= needs an engine with levels"):
        cut_recordings(corpus, cfg, engine=bare, hop=frame, normalize=0.9)
    assert eng.info()["open_streams"] == opened


class _Silent:
    """levels that report a silent and a non-finite segment: the factor is 1 for both"""
    def __init__(self, eng):
        self._e, self.gains = eng, None

    def __getattr__(self, name):
        return getattr(self._e, name)

    def levels(self, table, **kw):
        out = self._e.levels(table, **kw)
        out["peak"][0] = 0
        out["peak"][1] = np.nan
        return out

    def cut(self, table, gains=None, **kw):
        self.gains = np.array(gains)
        return self._e.cut(table, gains=gains, **kw)


def test_normalize_leaves_silent_and_non_finite_segments_alone(make_engine):
    from cutter_vad_amd import cut_recordings
    eng = make_engine()
    frame = eng.frame_samples
    cfg = _cfg(frame, enable_denoising=False)
    corpus = [_script(frame, [0.8] * 4 + [0.0] * 4 + [0.9] * 3 + [0.0] * 4 + [0.5] * 3 + [0.0] * 3)]
    fake = _Silent(eng)
    got = cut_recordings(corpus, cfg, engine=fake, hop=frame, wav=False, normalize=0.9)[0]
    plain = cut_recordings(corpus, cfg, engine=eng, hop=frame, wav=False)[0]
    assert fake.gains.dtype == np.float32 and fake.gains.tolist() == [1.0, 1.0, float(np.float32(0.9) / np.float32(0.5))]
    assert [p.tobytes() for _, _, p in got[:2]] == [p.tobytes() for _, _, p in plain[:2]]


def test_the_kernel_file_compiles_without_scratch_stores_or_float_atomics(tmp_path):
    """all 8 instantiations {4 loaders} x {1, 2 channels} from the compiler's own output: the cut's loads, all requested before the
    first wait; nothing is stored; per workgroup one 64-bit add, one unsigned maximum and one 32-bit add, and no other atomic"""
    import shutil
    import subprocess
    from cutter_vad_amd import _build
    cc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not found")
    out = tmp_path / "scan_levels.s"
    subprocess.run([cc, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "cutter_vad_amd", "csrc", "scan_levels.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = re.findall(r"\.name:\s*(_Z15vadk_seg_levelsILi(\d)ELi(\d)EE\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+)"
                      r".*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)", text, re.S)
    assert sorted(m[1:3] for m in meta) == sorted((str(f), str(c)) for f in range(4) for c in (1, 2)), meta
    width = {("0", "1"): "dwordx4", ("1", "1"): "dwordx2", ("2", "1"): "dword", ("3", "1"): "dword",
             ("0", "2"): "dwordx4", ("1", "2"): "dwordx4", ("2", "2"): "dwordx2", ("3", "2"): "dwordx2"}
    for name, f, c, scratch, sspill, vgprs, vspill in meta:
        assert (scratch, sspill, vspill) == ("0", "0", "0") and int(vgprs) <= 64, (name, scratch, sspill, vspill, vgprs)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)
        ops = re.findall(r"\b(buffer_load_\w+|global_store_\w+|flat_store_\w+|buffer_store_\w+|scratch_\w+|global_atomic_\w+|flat_atomic_\w+|"
                         r"buffer_atomic_\w+|ds_\w*atomic\w*|s_waitcnt vmcnt)", body)
        nload = 8 if (f, c) == ("0", "2") else 4
        assert ops[:nload] == ["buffer_load_" + width[(f, c)]] * nload and ops[nload] == "s_waitcnt vmcnt", (name, ops)
        rest = [x for x in ops[nload:] if x != "s_waitcnt vmcnt"]
        assert rest == ["global_atomic_add_x2", "global_atomic_umax", "global_atomic_add"], (name, rest)


# ---- AudioUtils -------------------------------------------------------------------------------------------------------
def test_audio_utils_level_helpers_by_hand():
    from cutter_vad_amd import AudioUtils
    x = np.array([0.5, -0.25, 0.0, 0.25], np.float32)
    assert AudioUtils.calculate_energy(x) == 0.375                     # 0.25 + 0.0625 + 0 + 0.0625
    assert AudioUtils.calculate_rms(x) == np.float32(np.sqrt(0.09375))
    assert AudioUtils.calculate_rms(np.array([3.0, 4.0, 0.0, 0.0])) == 2.5
    assert AudioUtils.detect_clipping(np.array([0.1, -0.95], np.float64)) and not AudioUtils.detect_clipping(np.array([0.1, -0.9]))
    assert AudioUtils.detect_clipping(x, threshold=0.5) and not AudioUtils.detect_clipping(x, threshold=0.51)
    y = AudioUtils.normalize_audio(x)
    assert y.dtype == np.float32 and y.tolist() == (x * np.float32(0.9 / 0.5)).tolist() and np.abs(y).max() == np.float32(0.9)
    assert AudioUtils.normalize_audio(x, target_level=0.25).tolist() == [0.25, -0.125, 0.0, 0.125]
    z = np.zeros(5, np.float32)
    assert AudioUtils.normalize_audio(z) is z
    assert AudioUtils.normalize_audio(np.array([-2.0, 1.0]), 1.0).tolist() == [-1.0, 0.5]
    # the GPU's fixed-point sum says the same as calculate_energy where float32 is exact
    q, peak, clipped = levels_ref(x, 0.25)
    assert q / 2.0 ** 32 == AudioUtils.calculate_energy(x) and peak == 0.5 and clipped == 3


def test_the_rule_is_exact_for_int16_over_32768():
    s = np.random.default_rng(0).integers(-32768, 32768, 100000).astype(np.int16)
    q, peak, _ = levels_ref(s.astype(np.float32) / np.float32(32768))
    assert q == 4 * int((s.astype(np.int64) ** 2).sum()) and peak == np.abs(s.astype(np.int64)).max() / 32768


# ---- the order of the checks ------------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_scan_levels's checks is behaviour: the rate, frame format, channels, hop, the clip threshold, the segments,
    the output pointer, and last the device form's two alignments.  Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    good, far = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 0, 0, 0)], [(0, 0, 1, 0, 0, 0), (0, 7, 2, 0, 0, 0)]

    def call(device, sr_in, fmt, channels, hop, clip, items, out, audio):
        args = (eng.handle, RO.cut_items(items), len(items), RO.addr(audio), RO.NS, channels, fmt, sr_in, hop, -1.0, clip)
        if device:
            return lib.vad_scan_levels_device(*args, RO.addr(out), None)
        return lib.vad_scan_levels(*args, None if out is None else C.cast(RO.addr(out), C.POINTER(_ffi.Level)))

    faults = dict(sr_in=44100, fmt=9, channels=3, hop=6, clip=float("nan"), items=far, out=None, audio=RO.buf(4 * RO.NS, 2))
    RO.walk(lib, eng, call, faults, (
        (RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 0),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "clip_thresh is NaN", "clip", 0.95),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", good),
        (INV, "vad_scan_levels(_device)?: null buffer$", "out", RO.buf(2 * 16, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the levels must be 8-byte aligned", "out", RO.buf(2 * 16), RO.DEVICE)))
