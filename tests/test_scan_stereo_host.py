"""vad_scan_cut_stereo / vad_scan_render_stereo on the host side: exports, their own refusals and the mono calls' under the new
names with an untouched output, the mono entry points still refusing VAD_SCAN_BOTH, bytes against tests/stereo_ref.py (the mono
references per channel, interleaved) and against the mono calls of the same library, the resident block, every kind of engine,
and the Python faces (Engine.cut_stereo / render_stereo and their _device forms, cut_recordings / render_recordings with
keep_channels) - the real csrc/engine.cpp over the HIP stand-in (tests/standin.py).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import standin
from tests.cut_ref import F32, FMT, FRAMES, INV, MIX, PCM16, RANGE, raw_cut, untouched, values
from tests.render_ref import raw_render
from tests.stereo_ref import BOTH, cut_stereo_ref, interleave, raw_cut_stereo, raw_render_stereo, render_stereo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_cut_stereo", "vad_scan_cut_stereo_device", "vad_scan_render_stereo", "vad_scan_render_stereo_device"]


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


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_the_four_symbols_exist(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header
    assert int(re.search(r"#define\s+VAD_SCAN_BOTH\s+\((-\d+)\)", header).group(1)) == _ffi.VAD_SCAN_BOTH == BOTH == -2
    # same argument lists as the gained cut and the render
    for new, old in (("vad_scan_cut_stereo", "vad_scan_cut_gain"), ("vad_scan_render_stereo", "vad_scan_render")):
        for tail in ("", "_device"):
            assert _ffi.SIGNATURES[new + tail] == _ffi.SIGNATURES[old + tail]
    from cutter_vad_amd import _build
    assert "scan_cut.hip" in _build.HIP_SOURCES and "scan_render.hip" in _build.HIP_SOURCES      # (they hold the stereo kernels)
    from cutter_vad_amd.engine import Engine
    for name in ("cut_stereo", "cut_stereo_device", "render_stereo", "render_stereo_device"):
        assert callable(getattr(Engine, name))


# ---- refusals ---------------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(2)
X = np.ascontiguousarray(np.stack([RNG.uniform(-0.9, 0.9, 4096), RNG.uniform(-0.2, 0.2, 4096)], axis=1).astype(np.float32))
HOP = 256
CUT_OK = [(0, 0, 3, 0), (1024, 2, 2, 1024)]                     # 1 024 sample frames at 0, 768 at 1 024
REN_OK = [(0, 0, 3, 0), (1024, 2, 2, 768)]                      # ... at 768: 256 shared
TRIPLE = [(0, 0, 3, 0), (0, 0, 3, 512), (0, 0, 3, 1020)]
N_OUT = 2048


def _cut(lib, eng, device, items=CUT_OK, audio=X, channels=2, fmt=FMT["f32"], hop=HOP, layout=RANGE, out_fmt=F32, out_samples=N_OUT, **kw):
    return raw_cut_stereo(lib, eng, items, audio, channels, fmt, hop, layout, out_fmt, out_samples, device=device, **kw)


def _render(lib, eng, device, items=REN_OK, audio=X, channels=2, fmt=FMT["f32"], hop=HOP, out_fmt=F32, out_samples=N_OUT, **kw):
    kw.pop("layout", None)
    return raw_render_stereo(lib, eng, items, audio, channels, fmt, hop, out_fmt, out_samples, device=device, **kw)


def test_refusals_carry_the_name_and_write_nothing(lib, make_engine):
    eng = make_engine()

    def refused(call, name, pattern, code=INV, **kw):
        for device in (False, True):
            rc, msg, out = call(lib, eng, device, **kw)
            assert rc == code, (name, rc, msg, kw)
            assert re.search(pattern, msg), msg
            assert msg.startswith("Model prediction failed: ") or code != INV, msg
            assert (name + ("_device" if device else "") + ":") in msg, msg
            assert untouched(out)

    for call, name in ((_cut, "vad_scan_cut_stereo"), (_render, "vad_scan_render_stereo")):
        # their own
        refused(call, name, "channels = 1: two-channel blocks only", audio=X[:, 0].copy(), channels=1)
        for ch in (0, 1, MIX):
            refused(call, name, f"segment 1 names channel {ch}: .*VAD_SCAN_BOTH", items=[(0, 0, 3, 0), (1024, 2, 2, 1024, ch)])
        # the mono calls', under this name
        refused(call, name, r"out_sample = 2 .* multiple of 4", items=[(0, 0, 3, 2)])
        refused(call, name, r"out_sample = 1028 \(\+1024 samples\)", items=[(0, 0, 3, 1028)])
        refused(call, name, "starts at sample 2, not a multiple of 4", items=[(2, 0, 3, 0)])
        refused(call, name, "leaves the audio block of 4096 samples", items=[(1024, 2, 11, 0)], out_samples=8192)
        refused(call, name, "reserved = 7 must be 0", items=[(0, 0, 3, 0, BOTH, 7)])
        refused(call, name, "hop = 6 must be a positive multiple of 4", hop=6)
        refused(call, name, r"channels = 3", channels=3, audio_samples=4096)
        refused(call, name, "segment 1: its gain is NaN", gains=(1.0, float("nan")))
        refused(call, name, "null buffer", null_out=True)
    refused(_cut, "vad_scan_cut_stereo", "output ranges of segments 0 and 1 overlap", items=REN_OK)
    refused(_render, "vad_scan_render_stereo", "output sample 1020 is covered by the segments 0, 1 and 2", items=TRIPLE)
    refused(_render, "vad_scan_render_stereo", "out_samples = 2046 must be a multiple of 4", out_samples=2046, items=[])
    refused(_render, "vad_scan_render_stereo", "nramp = 3 must be a multiple of 4", ramp=np.ones(8, np.float32), nramp=3)
    # VAD_CUT_FRAMES on a rate block: unsupported, with a message; the range works
    x48 = np.zeros((8192, 2), np.float32) + np.float32(0.25)
    for sr in (8000, 24000, 48000):
        chunk = 512 * sr // 16000
        refused(_cut, "vad_scan_cut_stereo", f"VAD_CUT_FRAMES on a block at {sr} Hz", code=_ffi.VAD_ERR_UNSUPPORTED, items=[(0, 0, 2, 0)],
                audio=x48, sr_in=sr, hop=chunk, layout=FRAMES)
        for device in (False, True):
            rc, msg, out = _cut(lib, eng, device, items=[(0, 0, 2, 0)], audio=x48, sr_in=sr, hop=chunk, layout=RANGE, out_samples=2 * chunk)
            assert rc == _ffi.VAD_OK and (out[:4 * chunk] == np.float32(0.25)).all() and untouched(out[4 * chunk:]), msg
    rc, msg, out = _cut(lib, eng, False, sr_in=44100)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "supported input rates" in msg and "vad_scan_cut_stereo" in msg and untouched(out), msg
    # the device form's pointers: the block 8-byte aligned, the output 16-byte aligned
    base = np.zeros(2 * 4096 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 4096]
    for call, name in ((_cut, "vad_scan_cut_stereo_device"), (_render, "vad_scan_render_stereo_device")):
        rc, msg, out = call(lib, eng, True, items=[(0, 0, 3, 0)], audio=odd, fmt=FMT["ulaw"], audio_samples=4096)
        assert rc == INV and name + ": the audio block must be 8-byte aligned" in msg and untouched(out), msg
    room = np.full(2 * N_OUT + 16, -7.0, np.float32)
    off = room[((16 - room.ctypes.data % 16) % 16) // 4 + 1:]
    rc, msg, out = raw_cut_stereo(lib, eng, CUT_OK, X, 2, FMT["f32"], HOP, RANGE, F32, N_OUT, device=True, out=off)
    assert rc == INV and "vad_scan_cut_stereo_device: the output must be 16-byte aligned" in msg and untouched(room), msg
    # no block is resident for audio = NULL
    fresh = make_engine()
    for call in (_cut, _render):
        rc, msg, out = call(lib, fresh, False, audio=None, audio_samples=4096)
        assert rc == INV and "no resident block" in msg and untouched(out), msg
    assert lib.vad_scan_cut_stereo(None, None, 0, None, None, 0, 2, 0, 0, 256, -1.0, 1, 0, None, 0) == INV
    assert lib.vad_scan_render_stereo(None, None, 0, None, None, 0, None, 0, 2, 0, 0, 256, -1.0, 0, None, 0) == INV


def test_the_mono_entry_points_still_refuse_both(lib, eng):
    for device in (False, True):
        rc, msg, out = raw_cut(lib, eng, [(0, 0, 3, 0, BOTH)], X, 2, FMT["f32"], HOP, RANGE, F32, N_OUT, device=device)
        assert rc == INV and "segment 0 names channel -2 of 2 (0 .. channels - 1, or VAD_SCAN_MIX)" in msg and untouched(out), msg
        rc, msg, out = raw_render(lib, eng, [(0, 0, 3, 0, BOTH)], X, 2, FMT["f32"], HOP, F32, N_OUT, device=device)
        assert rc == INV and "segment 0 names channel -2 of 2 (0 .. channels - 1, or VAD_SCAN_MIX)" in msg and untouched(out), msg


# ---- values -----------------------------------------------------------------------------------------------------------
def _two(rng, kind, n):
    """left and right differ in seed and in scale, neither is silent"""
    if kind == "f32":
        return interleave(rng.uniform(-1.2, 1.2, n).astype(np.float32), rng.uniform(-0.3, 0.3, n).astype(np.float32))
    if kind.startswith("i16"):
        return interleave(rng.integers(-32768, 32768, n).astype(np.int16), rng.integers(-3000, 3000, n).astype(np.int16))
    return interleave(values(rng, kind, n), values(rng, kind, n))


@pytest.mark.parametrize("thr", [None, 0.1], ids=["nogate", "gate"])
@pytest.mark.parametrize("kind", list(FMT))
def test_cut_bytes_against_numpy_and_against_the_mono_calls(lib, eng, kind, thr):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(7 + len(kind))
    x = _two(rng, kind, 12000)
    # listed out of order, gaps between their outputs
    items = [(1028, 1, 2, 4096 + 8), (0, 0, 1, 0), (2052, 3, 9, 8192), (8, 2, 3, 1024)]
    total = 16384
    gains = np.array([0.5, -3.0, 1.0, 2.0 ** -12], np.float32)
    t = -1.0 if thr is None else thr
    for layout in (RANGE, FRAMES):
        for out_fmt in (PCM16, F32):
            for g in (None, gains):
                want = {}
                for k, it in enumerate(items):
                    want[k] = cut_stereo_ref(x, kind, it, frame, hop, layout, out_fmt, thr, None if g is None else g[k])
                mono = []
                for c in (0, 1):
                    its = [it + (c,) for it in items]
                    if g is None:
                        rc, msg, m = raw_cut(lib, eng, its, x, 2, FMT[kind], hop, layout, out_fmt, total, thr=t)
                    else:
                        from tests.test_scan_levels_host import raw_gain
                        rc, msg, m = raw_gain(lib, eng, its, g, x, 2, FMT[kind], hop, layout, out_fmt, total, thr=t)
                    assert rc == _ffi.VAD_OK, msg
                    mono.append(m[:total])
                for device in (False, True):
                    rc, msg, out = raw_cut_stereo(lib, eng, items, x, 2, FMT[kind], hop, layout, out_fmt, total, thr=t, gains=g, device=device)
                    assert rc == _ffi.VAD_OK, msg
                    assert out[:2 * total].tobytes() == interleave(*mono).tobytes(), (layout, out_fmt, device)
                    written = np.zeros(total, bool)
                    for k, it in enumerate(items):
                        n = want[k].shape[0]
                        assert out[2 * it[3]:2 * (it[3] + n)].tobytes() == want[k].tobytes(), (k, layout, out_fmt, device)
                        written[it[3]:it[3] + n] = True
                    assert untouched(out[:2 * total].reshape(-1, 2)[~written]) and untouched(out[2 * total:]) and (~written).any()


@pytest.mark.parametrize("kind", list(FMT))
def test_render_bytes_against_numpy_and_against_the_mono_call(lib, eng, kind):
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    rng = np.random.default_rng(11 + len(kind))
    x = _two(rng, kind, 12000)
    c = lambda nf: (nf - 1) * hop + frame
    items = [(0, 0, 1, 4), (4, 2, 3, 4 + c(1) - 32), (1028, 1, 2, 4 + c(1) - 32 + c(3) + 4), (2052, 0, 5, 4 + c(1) + c(3) + c(2))]
    total = items[3][3] + c(5) + 4
    ramp = (0.5 - 0.5 * np.cos(np.pi * (np.arange(32) + 0.5) / 32)).astype(np.float32)
    gains = np.array([0.5, -3.0, 1.0, 40.0], np.float32)
    for thr in (None, 0.1):
        t = -1.0 if thr is None else thr
        for out_fmt in (PCM16, F32):
            for r, g in ((ramp, gains), (None, None)):
                want = render_stereo_ref(x, kind, items, frame, hop, out_fmt, thr, total, r, g)
                mono = [raw_render(lib, eng, [it + (ch,) for it in items], x, 2, FMT[kind], hop, out_fmt, total, thr=t, ramp=r, gains=g)[2][:total]
                        for ch in (0, 1)]
                assert want.tobytes() == interleave(*mono).tobytes()
                for device in (False, True):
                    rc, msg, out = raw_render_stereo(lib, eng, items, x, 2, FMT[kind], hop, out_fmt, total, thr=t, ramp=r, gains=g, device=device)
                    assert rc == _ffi.VAD_OK, msg
                    assert out[:2 * total].tobytes() == want.tobytes() and untouched(out[2 * total:]), (out_fmt, device)
                rc, msg, rev = raw_render_stereo(lib, eng, items[::-1], x, 2, FMT[kind], hop, out_fmt, total, thr=t, ramp=r,
                                                 gains=None if g is None else g[::-1])
                assert rc == _ffi.VAD_OK and rev.tobytes() == out.tobytes(), msg
    rc, msg, out = raw_render_stereo(lib, eng, [], x, 2, FMT[kind], hop, F32, 64)
    assert rc == _ffi.VAD_OK and not out[:128].any() and not np.signbit(out[:128]).any() and untouched(out[128:]), msg


def test_the_gate_acts_per_channel(lib, eng):
    frame = eng.frame_samples
    x = np.zeros((frame, 2), np.float32)
    x[:, 0], x[:, 1] = 0.01, 0.5                        # the left channel sits at the threshold: gated; the right one is kept
    x[1::2] = x[1::2, ::-1]
    rc, msg, out = raw_cut_stereo(lib, eng, [(0, 0, 1, 0)], x, 2, FMT["f32"], frame, RANGE, F32, frame, thr=0.01)
    assert rc == _ffi.VAD_OK, msg
    got = out[:2 * frame].reshape(-1, 2)
    assert (got[0::2, 0] == 0).all() and (got[0::2, 1] == 0.5).all() and (got[1::2, 0] == 0.5).all() and (got[1::2, 1] == 0).all()


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_cuts_and_renders_both_channels(lib, make_engine, kw):
    other = make_engine(**kw)
    frame = other.frame_samples
    hop = frame // 2
    x = _two(np.random.default_rng(3), "alaw", 4096)
    items = [(4, 1, 3, 8), (4, 0, 2, 8 + 2 * frame - 32)]
    total = 4 * frame
    for device in (False, True):
        rc, msg, out = raw_render_stereo(lib, other, items, x, 2, FMT["alaw"], hop, PCM16, total, thr=0.01, device=device)
        assert rc == _ffi.VAD_OK, (kw, msg)
        assert out[:2 * total].tobytes() == render_stereo_ref(x, "alaw", items, frame, hop, PCM16, 0.01, total).tobytes()
        rc, msg, out = raw_cut_stereo(lib, other, items[:1], x, 2, FMT["alaw"], hop, FRAMES, PCM16, total, thr=0.01, device=device)
        assert rc == _ffi.VAD_OK, (kw, msg)
        assert out[16:16 + 6 * frame].tobytes() == cut_stereo_ref(x, "alaw", items[0], frame, hop, FRAMES, PCM16, 0.01).tobytes()


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_engine_cut_stereo_and_render_stereo(make_engine):
    eng = make_engine()
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(5)
    block = _two(rng, "i16_32767", frame + 9 * hop + 3)
    segs = [(0, 1, 3), (0, 5, 1), (0, 0, 2)]
    for out, of in (("pcm16", PCM16), ("f32", F32)):
        for layout, lay in (("frames", FRAMES), ("range", RANGE)):
            data, start = eng.cut_stereo(segs, hop=hop, denoise=0.05, layout=layout, out=out, audio=block, gains=[1.0, 0.5, 2.0])
            assert data.ndim == 2 and data.shape == (int(start[-1]), 2) and data.dtype == (np.int16 if of == PCM16 else np.float32)
            mono = [eng.cut([sg + (c,) for sg in segs], hop=hop, denoise=0.05, layout=layout, out=out, audio=block, gains=[1.0, 0.5, 2.0])
                    for c in (0, 1)]
            assert np.array_equal(start, mono[0][1]) and data.tobytes() == interleave(mono[0][0], mono[1][0]).tobytes()
            for k, sg in enumerate(segs):
                want = cut_stereo_ref(block, "i16_32767", sg + (0,), frame, hop, lay, of, 0.05, [1.0, 0.5, 2.0][k])
                assert data[start[k]:start[k + 1]].tobytes() == want.tobytes()
            dev = np.full((int(start[-1]) + 4, 2), 77, data.dtype)
            st = eng.cut_stereo_device(segs, block.ctypes.data, block.shape[0], dev.ctypes.data, int(start[-1]), hop=hop,
                                       fmt=FMT["i16_32767"], denoise=0.05, layout=layout, out=out, gains=[1.0, 0.5, 2.0])
            eng.synchronize()
            assert np.array_equal(st, start) and dev[:int(start[-1])].tobytes() == data.tobytes() and (dev[int(start[-1]):] == 77).all()
        starts = [0, 2 * hop + frame - 16, 2 * hop + 2 * frame]
        total = starts[2] + hop + frame
        ramp = np.linspace(0.0, 1.0, 16).astype(np.float32)
        got = eng.render_stereo(segs, starts, total, hop=hop, ramp=ramp, denoise=0.05, out=out, audio=block, gains=[1.0, 0.5, 2.0])
        assert got.shape == (total, 2)
        mono = [eng.render([sg + (c,) for sg in segs], starts, total, hop=hop, ramp=ramp, denoise=0.05, out=out, audio=block, gains=[1.0, 0.5, 2.0])
                for c in (0, 1)]
        assert got.tobytes() == interleave(*mono).tobytes()
        dev = np.full((total + 4, 2), 77, got.dtype)
        eng.render_stereo_device(segs, starts, block.ctypes.data, block.shape[0], dev.ctypes.data, total, hop=hop, ramp=ramp,
                                 gains=[1.0, 0.5, 2.0], fmt=FMT["i16_32767"], denoise=0.05, out=out)
        eng.synchronize()
        assert dev[:total].tobytes() == got.tobytes() and (dev[total:] == 77).all()
    with pytest.raises(Exception, match=r"a segment of a stereo cut is \(sample_offset, first_frame, nframes\)"):
        eng.cut_stereo([(0, 1, 3, 0)], hop=hop, audio=block)
    with pytest.raises(Exception, match=r"a segment of a stereo cut"):
        eng.render_stereo([(0, 1, 3, "mix")], [0], 2048, hop=hop, audio=block)
    with pytest.raises(Exception, match="two-channel blocks only"):
        eng.cut_stereo(segs, hop=hop, audio=np.ascontiguousarray(block[:, 0]))
    with pytest.raises(Exception, match="VAD_CUT_FRAMES on a block at 48000 Hz"):
        eng.cut_stereo([(0, 0, 1)], audio=np.zeros((4096, 2), np.float32), sample_rate=48000)
    # the resident block of a scan
    recs = [_two(rng, "i16_32767", frame + 9 * hop + 2), _two(rng, "i16_32767", frame + 3 * hop)]
    slots = np.asarray(eng.open_streams(2))
    try:
        with eng.scan_session():
            eng.scan_segments(slots, recs, hop=hop, denoise=0.01, channel="mix")
            o1 = int(eng.last_scan["offsets"][1])
            sg2 = [(0, 1, 4), (o1, 0, 3)]
            data, start = eng.cut_stereo(sg2, hop=hop, layout="range", denoise=None)
            ren = eng.render_stereo(sg2, [0, int(start[1])], int(start[2]), hop=hop, denoise=None)
        want = np.concatenate([cut_stereo_ref(recs[0], "i16_32767", (0, 1, 4, 0), frame, hop, RANGE, PCM16, None),
                               cut_stereo_ref(recs[1], "i16_32767", (0, 0, 3, 0), frame, hop, RANGE, PCM16, None)])
        assert data.tobytes() == want.tobytes() == ren.tobytes()
    finally:
        for s in slots:
            eng.close_stream(int(s))


def _script2(frame, left, right, amp_r=0.5, fill=(0.125, -0.0625)):
    """the stand-in's p = |first sample of the frame|: a two-channel recording whose channels' frames have the probabilities
    `left` and `right`; the channels differ everywhere"""
    n = max(len(left), len(right), 15)
    x = np.zeros((frame * n + 3, 2), np.float32)
    x[:, 0], x[:, 1] = fill
    x[:, 0] += (np.arange(x.shape[0]) % 7).astype(np.float32) / 64
    for c, s in ((0, left), (1, right)):
        s = list(s) + [0.0] * (n - len(s))
        x[:n * frame:frame, c] = np.asarray(s, np.float32) * (1.0 if c == 0 else amp_r)
    return x


def _cfg(frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5, voice_start_frame_count=2,
                     voice_end_frame_count=2, output_wav_sample_rate=8000, **kw)


def _corpus(frame):
    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
    mono = np.full(frame * 15 + 3, np.float32(0.125), np.float32)
    mono[:15 * frame:frame] = np.asarray(one + [0.0] * 4, np.float32)
    return [_script2(frame, one, two), mono, _script2(frame, two, one), _script2(frame, [0.0] * 9, two, amp_r=1.0)]


def test_cut_recordings_keeps_both_channels(make_engine):
    from cutter_vad_amd import cut_recordings
    eng = make_engine()
    frame = hop = eng.frame_samples
    corpus = _corpus(frame)
    n = 0
    for gate_on, channel, layout in ((False, "mix", "range"), (True, 0, "frames"), (True, 1, "range")):
        cfg = _cfg(frame, enable_denoising=gate_on)
        kw = dict(engine=eng, hop=hop, layout=layout)
        both = cut_recordings(corpus, cfg, channel=channel, keep_channels=True, **kw)
        raw = cut_recordings(corpus, cfg, channel=channel, keep_channels=True, wav=False, **kw)
        plain = cut_recordings(corpus, cfg, channel=channel, **kw)
        assert both[1] == plain[1] and len(plain[1]) >= 1                      # the 1-D recording goes the mono way
        for i in (0, 2, 3):
            x = corpus[i]
            # the scan's ranges, then each channel cut on its own from a block that holds this recording alone
            rgs = [(a, b) for a, b, _ in plain[i]]
            assert [(a, b) for a, b, _ in both[i]] == rgs == [(a, b) for a, b, _ in raw[i]]
            segs = [(0, a // hop, (b - a - frame) // hop + 1) for a, b in rgs]
            for (a, b, wav), (_, _, arr), sg in zip(both[i], raw[i], segs):
                cols = [eng.cut([sg + (c,)], hop=hop, denoise=0.01 if gate_on else None, layout=layout, audio=x)[0] for c in (0, 1)]
                want = interleave(*cols)
                assert arr.dtype == np.int16 and arr.ndim == 2 and arr.shape[1] == 2 and arr.tobytes() == want.tobytes()
                assert not np.array_equal(cols[0], cols[1]) and cols[0].any() and cols[1].any()
                assert wav[:4] == b"RIFF" and wav[44:] == want.tobytes() and len(wav) == 44 + want.nbytes
                assert int.from_bytes(wav[22:24], "little") == 2 and int.from_bytes(wav[24:28], "little") == 8000
                assert int.from_bytes(wav[32:34], "little") == 4 and int.from_bytes(wav[40:44], "little") == want.nbytes
                n += 1
    assert n >= 6
    # normalize: one factor per segment from the larger of the two channel peaks
    cfg = _cfg(frame, enable_denoising=False)
    got = cut_recordings(corpus, cfg, engine=eng, hop=hop, layout="range", wav=False, keep_channels=True, normalize=0.9, channel=0)
    n = 0
    for i in (0, 2, 3):
        x = corpus[i]
        for a, b, arr in got[i]:
            g = np.float32(np.float32(0.9) / np.abs(x[a:b]).max())
            want = np.clip((x[a:b] * g).astype(np.float32) * 32767, -32768, 32767).astype(np.int16)
            assert arr.tobytes() == want.tobytes()
            n += 1
    assert n >= 3
    assert cut_recordings(corpus, cfg, engine=eng, hop=hop, wav=False, normalize=0.9)[1][0][2].tobytes() == got[1][0][2].tobytes()


def test_render_recordings_keeps_both_channels(make_engine):
    from cutter_vad_amd import render_recordings
    eng = make_engine()
    frame = hop = eng.frame_samples
    corpus = _corpus(frame)
    cfg = _cfg(frame, enable_denoising=True)
    pieces = 0
    for mode in ("join", "mask"):
        for norm in (None, 0.9):
            kw = dict(engine=eng, hop=hop, mode=mode, fade_ms=10.0, channel="mix")
            both = render_recordings(corpus, cfg, keep_channels=True, normalize=norm, **kw)
            raw = render_recordings(corpus, cfg, keep_channels=True, wav=False, normalize=norm, **kw)
            plain = render_recordings(corpus, cfg, normalize=norm, **kw)
            assert both[1] == plain[1]
            for i in (0, 2, 3):
                x = corpus[i]
                wav, tl = both[i]
                arr, tl2 = raw[i]
                assert tl == tl2 == plain[i][1]
                if not tl:
                    assert not arr.any() and arr.shape == ((x.shape[0] if mode == "mask" else 0), 2)
                    continue
                pieces += 1
                # the same places through Engine.render per channel, on a block that holds this recording alone
                segs = [(0, a // hop, (n - frame) // hop + 1) for _, a, n in tl]
                size = (x.shape[0] + 3) // 4 * 4 if mode == "mask" else tl[-1][0] + tl[-1][2]
                gains = None
                if norm is not None:
                    gains = [np.float32(np.float32(norm) / np.abs(np.where(np.abs(x[a:a + n]) > np.float32(0.01), x[a:a + n], 0)).max())
                             for _, a, n in tl]
                from cutter_vad_amd.scan import fade_ramp
                cols = [eng.render([sg + (c,) for sg in segs], [p for p, _, _ in tl], size, hop=hop, ramp=fade_ramp(160), gains=gains,
                                   denoise=0.01, audio=x) for c in (0, 1)]
                want = interleave(*cols)[:x.shape[0] if mode == "mask" else size]
                assert arr.dtype == np.int16 and arr.shape == want.shape and arr.tobytes() == want.tobytes(), (mode, norm, i)
                assert wav[44:] == want.tobytes() and int.from_bytes(wav[22:24], "little") == 2 and int.from_bytes(wav[24:28], "little") == 8000
    assert pieces >= 8


def test_the_python_refusals(make_engine):
    from cutter_vad_amd import cut_recordings, render_recordings
    eng = make_engine()
    frame = eng.frame_samples
    cfg = _cfg(frame, enable_denoising=False)
    corpus = _corpus(frame)
    opened = eng.info()["open_streams"]
    for fn in (cut_recordings, render_recordings):
        with pytest.raises(ConfigurationError, match="keep_channels=True delivers both channels.*'split'"):
            fn(corpus, cfg, engine=eng, hop=frame, channel="split", keep_channels=True)
    with pytest.raises(ConfigurationError, match='layout="range"'):
        cut_recordings(corpus, cfg, engine=eng, layout="frames", sample_rate=48000, keep_channels=True)
    got = cut_recordings([np.zeros((8192, 2), np.float32)], cfg, engine=eng, layout="range", sample_rate=48000, keep_channels=True)
    assert got == [[]]
    assert eng.info()["open_streams"] == opened


class _Recorder:
    """a stand-in engine object that notes how cut / render / levels are called, and has no stereo method"""
    def __init__(self, eng):
        self._e = eng
        self.calls = []

    def __getattr__(self, name):
        if name in ("cut_stereo", "render_stereo", "cut_stereo_device", "render_stereo_device"):
            raise AttributeError(name)
        fn = getattr(self._e, name)
        if name not in ("cut", "render", "levels"):
            return fn

        def noted(*a, **kw):
            self.calls.append((name, len(a), tuple(sorted(kw))))
            return fn(*a, **kw)
        return noted


def test_without_keep_channels_nothing_new_reaches_the_engine(make_engine):
    from cutter_vad_amd import cut_recordings, render_recordings
    eng = make_engine()
    frame = eng.frame_samples
    cfg = _cfg(frame, enable_denoising=False)
    corpus = _corpus(frame)
    rec = _Recorder(eng)
    for kc in (dict(), dict(keep_channels=False)):
        assert cut_recordings(corpus, cfg, engine=rec, hop=frame, normalize=0.9, **kc) == cut_recordings(corpus, cfg, engine=eng, hop=frame, normalize=0.9)
        a = render_recordings(corpus, cfg, engine=rec, hop=frame, **kc)
        b = render_recordings(corpus, cfg, engine=eng, hop=frame)
        assert [(p, t) for p, t in a] == [(p, t) for p, t in b]
    assert {c for c in rec.calls} == {("cut", 1, ("denoise", "gains", "hop", "layout")), ("levels", 1, ("denoise", "hop")),
                                      ("render", 3, ("denoise", "gains", "hop", "ramp"))}
    for fn, what in ((cut_recordings, "cut_stereo"), (render_recordings, "render_stereo")):
        with pytest.raises(ConfigurationError, match=f"keep_channels=True needs an engine with {what}.*_Recorder has none"):
            fn(corpus, cfg, engine=rec, hop=frame, keep_channels=True)


# ---- the order of the checks ------------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_scan_cut_stereo's checks is behaviour: the rate, frame format, channels (1 or 2, then 2), layout, out_fmt,
    hop, per segment its place in the block, its channel, its out_sample and its gain, the output pointer, and last the device
    form's two alignments.  Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    far = [(0, 0, 1, 0, BOTH, 0), (0, 7, 2, 514, 0, 0)]
    left = [(0, 0, 1, 0, BOTH, 0), (0, 1, 2, 514, 0, 0)]
    odd = [(0, 0, 1, 0, BOTH, 0), (0, 1, 2, 514, BOTH, 0)]
    good = [(0, 0, 1, 0, BOTH, 0), (0, 1, 2, 512, BOTH, 0)]          # the range once: 512 and 768 sample frames

    def call(device, sr_in, fmt, channels, layout, out_fmt, hop, items, gains, out, audio):
        args = (eng.handle, RO.cut_items(items), len(items), RO.f32p(gains), RO.addr(audio), RO.NS, channels, fmt, sr_in, hop, -1.0, layout,
                out_fmt, RO.addr(out), 1280)
        return lib.vad_scan_cut_stereo_device(*args, None) if device else lib.vad_scan_cut_stereo(*args)

    faults = dict(sr_in=44100, fmt=9, channels=3, layout=2, out_fmt=2, hop=6, items=far, gains=RO.f32(1.0, float("nan")), out=None,
                  audio=RO.buf(8 * RO.NS, 4))
    RO.walk(lib, eng, call, faults, (
        (RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 0),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "channels = 1: two-channel blocks only", "channels", 2),
        (INV, "layout = 2 is neither", "layout", RANGE),
        (INV, "out_fmt = 2 is neither", "out_fmt", F32),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", left),
        (INV, "segment 1 names channel 0: both channels are written", "items", odd),
        (INV, r"segment 1: out_sample = 514 \(\+768 samples\)", "items", good),
        (INV, "segment 1: its gain is NaN", "gains", RO.f32(1.0, 0.5)),
        (INV, "vad_scan_cut_stereo(_device)?: null buffer$", "out", RO.buf(8 * 1280, 4)),
        (INV, "the audio block must be 8-byte aligned", "audio", RO.buf(8 * RO.NS), RO.DEVICE),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(8 * 1280), RO.DEVICE)))
