"""vad_scan_render on the host side: exports, every refusal with its message, the order of the checks and an untouched output,
the resident block of a scan and of a rate scan, every kind of engine, bytes against tests/render_ref.py for every format x
channel mode x output format x gate, the invariants of the rule, and the Python faces (Engine.render, Engine.render_device,
fade_ramp, render_recordings in both modes against a host assembly of what cut_recordings cuts) - the real csrc/engine.cpp over
the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp restates the kernel's rule in plain C++).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import standin
from tests.cut_ref import F32, FMT, INV, MIX, PCM16, RANGE, gate, heard, pcm16, raw_cut, untouched, values
from tests.render_ref import faded, raw_render, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_render", "vad_scan_render_device"]


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
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header
    m = int(re.search(r"#define\s+VAD_RENDER_MAX_RAMP\s+(\d+)", header).group(1))
    assert m == _ffi.VAD_RENDER_MAX_RAMP == 65536
    from cutter_vad_amd import _build
    assert "scan_render.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    assert "render_recordings" in cutter_vad_amd.__all__ and cutter_vad_amd.render_recordings is not None


# ---- refusals ---------------------------------------------------------------------------------------------------------
X = np.zeros((4096, 2), np.float32) + np.float32(0.25)
HOP = 256
OK = [(0, 0, 3, 0, 0), (1024, 2, 2, 768, MIX)]                  # 1 024 samples at 0 and 768 at 768: 256 shared
TRIPLE = [(0, 0, 3, 0, 0), (0, 0, 3, 512, 0), (0, 0, 3, 1020, 1)]
N_OUT = 2048
RAMP = np.linspace(0.125, 0.875, 8).astype(np.float32)


def _call(lib, eng, device, items=OK, audio=X, channels=2, fmt=FMT["f32"], hop=HOP, out_fmt=F32, out_samples=N_OUT, **kw):
    return raw_render(lib, eng, items, audio, channels, fmt, hop, out_fmt, out_samples, device=device, **kw)


def test_two_segments_may_overlap_and_every_sample_is_written(lib, make_engine):
    eng = make_engine()
    for device in (False, True):
        rc, msg, out = _call(lib, eng, device)
        assert rc == _ffi.VAD_OK, msg
        want = np.zeros(N_OUT, np.float32)
        want[:1536] = 0.25
        want[768:1024] = 0.5
        assert out[:N_OUT].tobytes() == want.tobytes() and untouched(out[N_OUT:])
        rc, msg, _ = raw_cut(lib, eng, [it + (0,) for it in OK], X, 2, FMT["f32"], HOP, RANGE, F32, N_OUT, device=device)
        assert rc == INV and "output ranges of segments 0 and 1 overlap" in msg       # the cut still refuses it
        # no segments: zeros, and nothing else is needed
        rc, msg, out = _call(lib, eng, device, items=[], out_samples=4096)
        assert rc == _ffi.VAD_OK and not out[:4096].any() and not np.signbit(out[:4096]).any() and untouched(out[4096:]), msg
        rc, msg, out = _call(lib, eng, device, items=[], audio=None, audio_samples=0, out_samples=8, out_fmt=PCM16)
        assert rc == _ffi.VAD_OK and not out[:8].any() and untouched(out[8:]), msg
        rc, msg, out = _call(lib, eng, device, items=[], out_samples=0, null_out=True)
        assert rc == _ffi.VAD_OK and untouched(out), msg


def test_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()

    def refused(pattern, **kw):
        for device in (False, True):
            rc, msg, out = _call(lib, eng, device, **kw)
            assert rc == INV, (rc, msg, kw)
            assert re.search(pattern, msg), msg
            assert msg.startswith("Model prediction failed: ") and ("vad_scan_render" in msg or "format" in msg), msg
            assert ("vad_scan_render_device" in msg) == device or "format" in msg, msg
            assert untouched(out)

    # the cut's refusals about the block, the items and the gains, under this name
    for out_fmt in (2, -1):
        refused(r"out_fmt = -?\d", out_fmt=out_fmt)
    for fmt in (5, -1, 9):
        refused("unknown frame format", fmt=fmt)
    for channels in (0, 3, -1):
        refused(r"channels = -?\d", channels=channels, audio_samples=4096)
    for h in (0, 2, 6, -256, 258):
        refused("hop = -?\\d+ must be a positive multiple of 4", hop=h)
    refused("null buffer or bad count", out_samples=-4)
    refused("starts at sample 2, not a multiple of 4", items=[(2, 0, 3, 0, 0)])
    refused("first_frame = -1", items=[(0, -1, 3, 0, 0)])
    refused("nframes = 0", items=[(0, 0, 0, 0, 0)])
    refused("leaves the audio block of 4096 samples", items=[(1024, 2, 11, 0, 0)], out_samples=8192)
    refused("leaves the audio block", items=[(0, 0, 1 << 40, 0, 0)], out_samples=1 << 50)
    refused("channel 2 of 2", items=[(0, 0, 3, 0, 2)])
    refused("channel 1 of 1", items=[(0, 0, 3, 0, 1)], audio=X.reshape(-1), channels=1)
    refused("reserved = 7 must be 0", items=[(0, 0, 3, 0, 0, 7)])
    refused("out_sample = 2 .* multiple of 4", items=[(0, 0, 3, 2, 0)])
    refused("out_sample = -4", items=[(0, 0, 3, -4, 0)])
    refused(r"out_sample = 1028 \(\+1024 samples\)", items=[(0, 0, 3, 1028, 0)])
    refused("2 GiB", audio_samples=1 << 28)
    refused("segment 1: its gain is NaN", gains=(1.0, float("nan")))
    refused("segment 0: its gain is infinite", gains=(float("inf"), float("nan")))
    # ... and its own
    for n in (2, 6, 2046, -2):
        refused(f"out_samples = {n} must be a multiple of 4" if n > 0 else "bad count", out_samples=n, items=[])
    for nramp in (-4, -1, 3, 6, _ffi.VAD_RENDER_MAX_RAMP + 4, 1 << 30):
        refused(f"nramp = {nramp} must be a multiple of 4 from 0 to 65536", ramp=RAMP, nramp=nramp)
    refused("null ramp", ramp=RAMP, null_ramp=True)
    bad = RAMP.copy()
    bad[5] = np.nan
    bad[7] = np.inf
    refused(r"ramp\[5\] is NaN", ramp=bad)
    bad[5] = -np.inf
    refused(r"ramp\[5\] is infinite", ramp=bad)
    refused("output sample 1020 is covered by the segments 0, 1 and 2", items=TRIPLE)
    refused("output sample 1020 is covered by the segments 2, 1 and 0", items=TRIPLE[::-1])
    refused(r"more than 2\^31 - 1 workgroups of 4096 samples", out_samples=1 << 50)          # refused before a workgroup is listed
    refused("null buffer", null_out=True)
    # the longest ramp and three segments that only touch are fine
    long_ramp = np.full(_ffi.VAD_RENDER_MAX_RAMP, 0.5, np.float32)
    for device in (False, True):
        rc, msg, out = _call(lib, eng, device, ramp=long_ramp, items=[(0, 0, 3, 0, 0), (0, 0, 3, 512, 0), (0, 0, 3, 1024, 1)])
        assert rc == _ffi.VAD_OK, msg
    # the pointers come last
    for device, pat in ((True, "null buffer"), (False, "no resident block|resident block has")):
        rc, msg, out = _call(lib, eng, device, audio=None, audio_samples=4095)
        assert rc == INV and re.search(pat, msg) and untouched(out), msg
    base = np.zeros(2 * 4096 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 4096]
    rc, msg, out = _call(lib, eng, True, items=[(0, 0, 3, 0, 0)], audio=odd, fmt=FMT["ulaw"], audio_samples=4096)
    assert rc == INV and "vad_scan_render_device: the audio block must be 8-byte aligned" in msg and untouched(out), msg
    assert lib.vad_scan_render(None, None, 0, None, None, 0, None, 0, 1, 0, 0, 256, -1.0, 0, None, 0) == INV
    # rates: 0 and the engine's own are the same call; others are the rate cut's
    rc, msg, a = _call(lib, eng, False, sr_in=16000)
    rc2, msg2, b = _call(lib, eng, False)
    assert rc == rc2 == _ffi.VAD_OK and a.tobytes() == b.tobytes(), (msg, msg2)
    rc, msg, out = _call(lib, eng, False, sr_in=44100)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "supported input rates" in msg and "vad_scan_render" in msg and untouched(out), msg
    small = make_engine(rate=8000)
    rc, msg, out = _call(lib, small, False, sr_in=48000)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "8 kHz sub-model" in msg and untouched(out), msg


def test_the_order_of_the_checks(lib, make_engine):
    """a call with several faults gets the first of the header's list"""
    eng = make_engine()
    nan_ramp = RAMP.copy()
    nan_ramp[0] = np.nan
    bad_item = [(2, 0, 3, 0, 0)] + TRIPLE
    faults = [                                                   # in the header's order
        ("sr_in", dict(sr_in=44100), "supported input rates"),
        ("count", dict(out_samples=-2), "null buffer or bad count"),
        ("format", dict(fmt=9), "unknown frame format"),
        ("out_fmt", dict(out_fmt=2), "out_fmt = 2"),
        ("hop", dict(hop=6), "hop = 6"),
        ("out_samples", dict(out_samples=2046), "out_samples = 2046"),
        ("nramp", dict(nramp=3), "nramp = 3"),
        ("null ramp", dict(null_ramp=True), "null ramp"),
        ("ramp entry", dict(ramp=nan_ramp), r"ramp\[0\] is NaN"),
        ("item", dict(items=bad_item), "starts at sample 2"),
        ("triple", dict(items=TRIPLE), "covered by the segments"),
        ("null out", dict(null_out=True), "null buffer"),
        ("block", dict(audio=None, audio_samples=4096), "no resident block|null buffer"),
    ]
    for device in (False, True):
        for first in range(len(faults)):
            kw = dict(ramp=RAMP)
            for _, more, _ in reversed(faults[first:]):          # every later fault too; the earlier one's arguments win
                kw.update(more)
            rc, msg, out = _call(lib, eng, device, **kw)
            assert rc != _ffi.VAD_OK and re.search(faults[first][2], msg), (faults[first][0], msg)
            assert untouched(out)


# ---- the resident block -----------------------------------------------------------------------------------------------
def test_null_audio_names_the_resident_block_of_a_scan_and_of_a_rate_scan(make_engine):
    eng = make_engine()
    rng = np.random.default_rng(21)
    for rate, hop in ((None, 256), (48000, 772)):
        chunk = eng.frame_samples if rate is None else eng.scan_chunk_samples(rate)
        recs = [values(rng, "i16_32767", (chunk + 9 * hop + 2, 2)), values(rng, "i16_32767", (chunk + 3 * hop, 2))]
        slots = np.asarray(eng.open_streams(2))
        kw = {} if rate is None else {"sample_rate": rate}
        try:
            with eng.scan_session():
                eng.scan_segments(slots, recs, hop=hop, denoise=0.01, channel="mix", **kw)
                last = eng.last_scan
                o1 = int(last["offsets"][1])
                segs = [(0, 1, 4, 1), (o1, 0, 3, "mix"), (0, 3, 6, 0)]
                counts = [(n - 1) * hop + chunk for _, _, n, _ in segs]
                starts = [0, counts[0] - 64, counts[0] + counts[1] + 8]
                total = starts[2] + counts[2] + 4
                ramp = np.linspace(0.1, 0.9, 64).astype(np.float32)
                got = eng.render(segs, starts, total, hop=hop, ramp=ramp, denoise=0.3, out="f32", **kw)
                with pytest.raises(Exception, match="the block of the last scan is at"):
                    eng.render(segs, starts, total, hop=hop, sample_rate=24000 if rate else 48000)
            block = np.zeros((last["samples"], 2), np.int16)
            block[:recs[0].shape[0]] = recs[0]
            block[o1:o1 + recs[1].shape[0]] = recs[1]
            items = [(sg[0], sg[1], sg[2], st, MIX if sg[3] == "mix" else sg[3]) for sg, st in zip(segs, starts)]
            want = render(block, "i16_32767", items, chunk, hop, F32, 0.3 if rate is None else None, total, ramp)
            assert got.tobytes() == want.tobytes()
            assert eng.render(segs, starts, total, hop=hop, ramp=ramp, denoise=0.3, out="f32", audio=block, **kw).tobytes() == want.tobytes()
            assert eng.last_scan is None
            with pytest.raises(Exception, match="follows a scan"):
                eng.render(segs, starts, total, hop=hop)
        finally:
            for s in slots:
                eng.close_stream(int(s))


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_renders(lib, make_engine, kw):
    other = make_engine(**kw)
    frame = other.frame_samples
    hop = frame // 2
    x = values(np.random.default_rng(3), "alaw", (4096, 2))
    items = [(4, 1, 3, 8, 1), (4, 0, 2, 2 * frame - 32 + 8, MIX)]
    total = 4 * frame
    ramp = np.linspace(0.0, 1.0, 32).astype(np.float32)
    for device in (False, True):
        for out_fmt in (PCM16, F32):
            rc, msg, out = raw_render(lib, other, items, x, 2, FMT["alaw"], hop, out_fmt, total, thr=0.01, ramp=ramp, device=device)
            assert rc == _ffi.VAD_OK, (kw, msg)
            assert out[:total].tobytes() == render(x, "alaw", items, frame, hop, out_fmt, 0.01, total, ramp).tobytes() and untouched(out[total:])


# ---- values -----------------------------------------------------------------------------------------------------------
def _layout(frame, hop, chans, n_block):
    """eight segments of ragged lengths in every kind of neighbourhood: two that start at output sample 0, an overlap of one quad,
    a gap of one quad, an overlap of exactly the 32-entry ramp, a longer gap, one segment wholly inside another, and a last
    overlap that reaches the end of the output"""
    nfs = [1, 3, 9, 2, 1, 17, 4, 2]
    offs = [0, 4, 1028, 0, 2052, 8, 516, 12]
    c = [(nf - 1) * hop + frame for nf in nfs]
    at = [0, 0]
    at.append(at[1] + c[1] - 4)
    at.append(at[2] + c[2] + 4)
    at.append(at[3] + c[3] - 32)
    at.append(at[4] + c[4] + 64)
    at.append(at[5] + 8)
    at.append(at[5] + c[5] - 8)
    assert at[6] + c[6] <= at[7]
    total = at[7] + c[7]
    items = [(offs[k], 2 * k % 5, nfs[k], at[k], chans[k % len(chans)]) for k in range(8)]
    assert all(o + (f + n - 1) * hop + frame <= n_block for o, f, n, _, _ in items)
    return items, total


@pytest.mark.parametrize("thr", [None, 0.3], ids=["nogate", "gate"])
@pytest.mark.parametrize("mode", ["mono", "left", "right", "mix"])
@pytest.mark.parametrize("kind", list(FMT))
def test_bytes_against_numpy(lib, eng, kind, mode, thr):
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    rng = np.random.default_rng(len(kind) + 10 * len(mode))
    channels = 1 if mode == "mono" else 2
    x = values(rng, kind, (12000, 2) if channels == 2 else 12000)
    chans = {"mono": (0,), "left": (0,), "right": (1,), "mix": (MIX, 0, 1)}[mode]
    items, total = _layout(frame, hop, chans, 12000)
    cover = np.zeros(total, np.int32)
    for o, f, n, at, _ in items:
        cover[at:at + (n - 1) * hop + frame] += 1
    assert cover.max() == 2 and (cover == 0).any() and cover[0] == 2
    ramp = (0.5 - 0.5 * np.cos(np.pi * (np.arange(32) + 0.5) / 32)).astype(np.float32)
    gains = np.array([0.5, -3.0, 1.0, 2.0 ** -12, 40.0, 1.5, -1.0, 0.75], np.float32)
    t = -1.0 if thr is None else thr
    for out_fmt in (PCM16, F32):
        for r, g in ((ramp, gains), (None, None), (ramp[:4], None)):
            want = render(x, kind, items, frame, hop, out_fmt, thr, total, r, g)
            for device in (False, True):
                rc, msg, out = raw_render(lib, eng, items, x, channels, FMT[kind], hop, out_fmt, total, thr=t, ramp=r, gains=g, device=device)
                assert rc == _ffi.VAD_OK, msg
                assert out[:total].tobytes() == want.tobytes() and untouched(out[total:]), (out_fmt, device)
            # the order of the items does not matter; two calls agree; no gains is gains of ones
            rc, msg, rev = raw_render(lib, eng, items[::-1], x, channels, FMT[kind], hop, out_fmt, total, thr=t, ramp=r,
                                      gains=None if g is None else g[::-1])
            assert rc == _ffi.VAD_OK and rev.tobytes() == out.tobytes(), msg
        rc, msg, ones = raw_render(lib, eng, items, x, channels, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp[:4], gains=np.ones(8, np.float32))
        assert rc == _ffi.VAD_OK and ones.tobytes() == out.tobytes(), msg


def test_without_ramp_and_overlap_the_segments_are_the_gained_cut(lib, eng):
    frame, hop = eng.frame_samples, 4
    rng = np.random.default_rng(17)
    x = values(rng, "i16_32768", (9000, 2))
    items = [(0, 3, 1, 8, 1), (1024, 0, 900, 8 + frame, MIX), (0, 1, 2, 8 + frame + 899 * 4 + frame + 4, 0)]
    total = items[2][3] + 4 + frame + 12
    gains = np.array([2.0, 0.5, -1.0], np.float32)
    from tests.test_scan_levels_host import raw_gain
    for out_fmt in (PCM16, F32):
        rc, msg, cut = raw_gain(lib, eng, items, gains, x, 2, FMT["i16_32768"], hop, RANGE, out_fmt, total, thr=0.01)
        rc2, msg2, out = raw_render(lib, eng, items, x, 2, FMT["i16_32768"], hop, out_fmt, total, thr=0.01, gains=gains)
        assert rc == rc2 == _ffi.VAD_OK, (msg, msg2)
        covered = np.zeros(total, bool)
        for it in items:
            covered[it[3]:it[3] + (it[2] - 1) * hop + frame] = True
        assert out[:total][covered].tobytes() == cut[:total][covered].tobytes()
        assert not out[:total][~covered].any() and untouched(cut[:total][~covered]) and (~covered).sum() == 8 + 4 + 12


def test_a_ramp_longer_than_the_segment_fades_it_from_both_ends(lib, eng):
    frame, hop = eng.frame_samples, 4
    x = np.full(2048, 0.5, np.float32)
    for nramp in (4, frame // 2, frame // 2 + 4, frame, 4096):
        ramp = ((np.arange(nramp) + 0.5) / nramp).astype(np.float32)
        rc, msg, out = raw_render(lib, eng, [(0, 0, 1, 4, 0)], x, 1, FMT["f32"], hop, F32, frame + 8, ramp=ramp)
        assert rc == _ffi.VAD_OK, msg
        m = min(nramp, frame)
        a, b = np.ones(frame, np.float32), np.ones(frame, np.float32)
        a[:m] = ramp[:m]
        b[frame - m:] = ramp[:m][::-1]
        want = np.concatenate([np.zeros(4, np.float32), (np.float32(0.5) * a) * b, np.zeros(4, np.float32)])
        assert out[:frame + 8].tobytes() == want.tobytes() == render(x, "f32", [(0, 0, 1, 4, 0)], frame, hop, F32, None, frame + 8, ramp).tobytes()
        assert np.array_equal(out[4:4 + frame], out[4:4 + frame][::-1])          # one table, read from both ends


def test_sums_saturate_in_pcm16(lib, eng):
    frame = eng.frame_samples
    x = np.concatenate([np.full(frame, 0.9, np.float32), np.full(frame, -0.9, np.float32)])
    items = [(0, 0, 1, 0, 0), (0, 0, 1, 0, 0), (0, 1, 1, frame, 0), (0, 1, 1, frame, 0)]
    rc, msg, out = raw_render(lib, eng, items, x, 1, FMT["f32"], frame, PCM16, 2 * frame)
    assert rc == _ffi.VAD_OK, msg
    assert (out[:frame] == 32767).all() and (out[frame:2 * frame] == -32768).all()


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_fade_ramp():
    from cutter_vad_amd.scan import fade_ramp
    for n in (0, 4, 160, 480):
        k = np.arange(n, dtype=np.float64)
        lin, cos = fade_ramp(n), fade_ramp(n, "cosine")
        assert lin.dtype == cos.dtype == np.float32 and lin.shape == cos.shape == (n,)
        assert lin.tobytes() == ((k + 0.5) / max(n, 1)).astype(np.float32).tobytes()
        assert cos.tobytes() == (0.5 - 0.5 * np.cos(np.pi * (k + 0.5) / max(n, 1))).astype(np.float32).tobytes()
        if n:
            assert 0 < lin[0] < lin[-1] < 1 and 0 < cos[0] < cos[-1] < 1
            assert np.allclose(lin.astype(np.float64) + lin[::-1], 1.0, atol=2e-7) and np.allclose(cos.astype(np.float64) + cos[::-1], 1.0, atol=2e-7)
    with pytest.raises(ConfigurationError, match="shape is 'linear' or 'cosine'"):
        fade_ramp(8, "sqrt")
    with pytest.raises(ConfigurationError, match="n is 0 or more"):
        fade_ramp(-4)


def test_engine_render_and_its_argument_errors(eng):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(5)
    block = values(rng, "f32", (frame + 9 * hop + 3, 2))
    segs = [(0, 1, 3), (0, 5, 1, 1), (0, 0, 2, 0)]
    starts = [0, 2 * hop + frame - 16, 2 * hop + 2 * frame]
    total = starts[2] + hop + frame
    ramp = np.linspace(0.0, 1.0, 16).astype(np.float32)
    items = [(0, 1, 3, starts[0], MIX), (0, 5, 1, starts[1], 1), (0, 0, 2, starts[2], 0)]
    for out, of in (("pcm16", PCM16), ("f32", F32)):
        got = eng.render(segs, starts, total, hop=hop, ramp=ramp, denoise=0.3, out=out, audio=block, gains=[1.0, 0.5, 2.0])
        assert got.dtype == (np.int16 if of == PCM16 else np.float32) and got.shape == (total,)
        assert got.tobytes() == render(block, "f32", items, frame, hop, of, 0.3, total, ramp, [1.0, 0.5, 2.0]).tobytes()
        dev = np.full(total + 4, 77, got.dtype)
        eng.render_device(segs, starts, block.ctypes.data, block.shape[0], dev.ctypes.data, total, hop=hop, ramp=ramp, gains=[1.0, 0.5, 2.0],
                          channels=2, denoise=0.3, out=out)
        eng.synchronize()
        assert dev[:total].tobytes() == got.tobytes() and (dev[total:] == 77).all()
    assert eng.render([], [], 64, audio=block).tobytes() == np.zeros(64, np.int16).tobytes()
    with pytest.raises(Exception, match="gains has 2 entries for 3 segments"):
        eng.render(segs, starts, total, hop=hop, audio=block, gains=[1.0, 2.0])
    with pytest.raises(Exception, match="covered by the segments 0, 1 and 2"):
        eng.render(segs, [0, 4, 8], total, hop=hop, audio=block)
    with pytest.raises(Exception, match="out is one of"):
        eng.render(segs, starts, total, hop=hop, audio=block, out="wav")
    with pytest.raises(Exception, match=r"ramp\[1\] is NaN"):
        eng.render(segs, starts, total, hop=hop, audio=block, ramp=[0.0, float("nan"), 1.0, 1.0])
    with pytest.raises(Exception, match="out_samples = 6 must be a multiple of 4"):
        eng.render([], [], 6, audio=block)


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


def _assemble(h, ranges, mode, nramp, gap, ramp, size, gains=None):
    """the host's way to the same bytes: the float32 ranges, faded, overlap-added in float32, converted"""
    from cutter_vad_amd.scan import _join_places
    if mode == "mask":
        merged = []
        for a, b in sorted(ranges):
            if merged and a <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        ranges, at = merged, [a for a, _ in merged]
        total = (size + 3) // 4 * 4
    else:
        at = _join_places([b - a for a, b in ranges], nramp, gap)
        total = at[-1] + ranges[-1][1] - ranges[-1][0] if ranges else 0
    acc, cover = np.zeros(total, np.float32), np.zeros(total, np.int32)
    for k, ((a, b), p) in enumerate(zip(ranges, at)):
        v = h[a:b] if gains is None else (h[a:b] * gains(h[a:b])).astype(np.float32)
        w = faded(v, ramp)
        sl = slice(p, p + b - a)
        acc[sl] = np.where(cover[sl] == 0, w, (acc[sl] + w).astype(np.float32))
        cover[sl] += 1
    assert cover.max(initial=0) <= 2
    pcm = pcm16(acc)
    return (pcm[:size] if mode == "mask" else pcm), [(p, a, b - a) for (a, b), p in zip(ranges, at)], cover


def test_render_recordings_against_a_host_assembly_of_the_cut(make_engine):
    from cutter_vad_amd import SegmentRefine, cut_recordings, render_recordings
    from cutter_vad_amd.scan import fade_ramp
    eng = make_engine()
    frame = hop = eng.frame_samples
    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
    none = [0.0] * 9
    tail = [0.0] * 10 + [0.8] * 5                      # stops inside speech
    st = lambda l, r: np.ascontiguousarray(np.stack([_script(frame, l), _script(frame, r)], axis=1))
    corpus = [_script(frame, one), st(two, none), _script(frame, none), st(none, one), _script(frame, two, fill=0.0), _script(frame, tail)]
    split3 = SegmentRefine(pad_before=1, pad_after=1, max_frames=3)          # neighbours from a split touch: mask merges them
    overlaps = crossfades = 0
    for gate_on, channel, kw in ((False, "mix", dict()), (True, 0, dict(open_end=True)), (False, "split", dict(open_end=True, refine=split3)),
                                 (True, "split", dict())):
        cfg = _cfg(frame, enable_denoising=gate_on)
        thr = 0.01 if gate_on else None
        cuts = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout="range", wav=False, **kw)
        for mode, fade_ms, gap_ms, shape in (("join", 10.0, 0.0, "linear"), ("join", 40.0, 0.0, "cosine"), ("join", 10.0, 25.0, "linear"),
                                             ("join", 0.0, 0.0, "linear"), ("mask", 10.0, 0.0, "cosine"), ("mask", 0.0, 0.0, "linear")):
            nramp, gap = int(round(fade_ms * 16)) // 4 * 4, int(round(gap_ms * 16)) // 4 * 4
            ramp = fade_ramp(nramp, shape)
            got = render_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, mode=mode, fade_ms=fade_ms, gap_ms=gap_ms, shape=shape,
                                    wav=False, **kw)
            wavs = render_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, mode=mode, fade_ms=fade_ms, gap_ms=gap_ms, shape=shape, **kw)
            assert len(got) == len(corpus)
            for x, rc, rg, rw in zip(corpus, cuts, got, wavs):
                per = [(c, rc[c], rg[c], rw[c]) for c in range(len(rg))] if channel == "split" else [(channel, rc, rg, rw)]
                for c, c_, g_, w_ in per:
                    h = gate(x if x.ndim == 1 else heard(x, "f32", MIX if c == "mix" else c), thr)
                    for a, b, pcm in c_:
                        assert pcm.tobytes() == pcm16(h[a:b]).tobytes()          # what the cut delivers for the range
                    want, timeline, cover = _assemble(h, [(a, b) for a, b, _ in c_], mode, nramp, gap, ramp, x.shape[0])
                    payload, tl = g_
                    assert payload.dtype == np.int16 and payload.tobytes() == want.tobytes(), (mode, fade_ms, gap_ms, c)
                    assert tl == timeline
                    assert w_[1] == tl and w_[0][44:] == payload.tobytes() and w_[0][:4] == b"RIFF"
                    assert int.from_bytes(w_[0][24:28], "little") == 8000
                    if mode == "mask":
                        assert payload.size == x.shape[0] and len(tl) <= len(c_)
                        overlaps += len(c_) - len(tl)
                        assert not payload[cover[:payload.size] == 0].any()
                    else:
                        crossfades += int((cover == 2).any())
                        assert gap == 0 or not (cover == 2).any()
                    for p, a, n in tl:                            # the timeline maps the output back to the recording
                        mid = slice(p + nramp, p + n - nramp)
                        if mode == "mask" or gap > 0 or nramp == 0:
                            assert payload[mid].tobytes() == pcm16(h[a + nramp:a + n - nramp]).tobytes()
            silent = got[2][0] if channel == "split" else got[2]
            assert silent[1] == [] and silent[0].size == (corpus[2].shape[0] if mode == "mask" else 0) and not silent[0].any()
    assert overlaps >= 1 and crossfades >= 2
    # normalize: the factor of cut_recordings, per listed segment, ahead of the ramp
    cfg = _cfg(frame, enable_denoising=False)
    got = render_recordings(corpus, cfg, engine=eng, hop=hop, mode="join", fade_ms=10.0, wav=False, normalize=0.9, open_end=True)
    cuts = cut_recordings(corpus, cfg, engine=eng, hop=hop, layout="range", wav=False, open_end=True)
    n = 0
    for x, c_, (payload, tl) in zip(corpus, cuts, got):
        h = x if x.ndim == 1 else heard(x, "f32", MIX)
        want, timeline, _ = _assemble(h, [(a, b) for a, b, _ in c_], "join", 160, 0, fade_ramp(160), x.shape[0],
                                      gains=lambda v: np.float32(np.float32(0.9) / np.abs(v).max()))
        assert payload.tobytes() == want.tobytes() and tl == timeline
        n += len(tl)
    assert n >= 4
    with pytest.raises(ConfigurationError, match="mode is 'join' or 'mask'"):
        render_recordings(corpus, cfg, engine=eng, hop=hop, mode="gate")
    with pytest.raises(ConfigurationError, match="a ramp has 65536 at the most"):
        render_recordings(corpus, cfg, engine=eng, hop=hop, fade_ms=5000.0)
    assert render_recordings([], cfg, engine=eng) == []


def test_render_recordings_at_48_khz(make_engine):
    from cutter_vad_amd import cut_recordings, render_recordings
    from cutter_vad_amd.scan import fade_ramp
    eng = make_engine()
    chunk = hop = 1536
    cfg = _cfg(512, enable_denoising=True)
    rng = np.random.default_rng(48)
    recs = []
    for s in ([0.0] * 2 + [0.9] * 4 + [0.0] * 4 + [0.8] * 3 + [0.0] * 4, [0.9] * 5 + [0.0] * 6):
        x = rng.uniform(-0.005, 0.005, chunk * len(s) + 5).astype(np.float32)      # under the gate: a rate range is NOT gated
        x[:len(s) * chunk:chunk] = np.asarray(s, np.float32)
        recs.append(x)
    cuts = cut_recordings(recs, cfg, engine=eng, hop=hop, layout="range", wav=False, sample_rate=48000)
    assert sum(len(c) for c in cuts) >= 3
    for mode in ("join", "mask"):
        got = render_recordings(recs, cfg, engine=eng, hop=hop, mode=mode, fade_ms=10.0, sample_rate=48000)
        for x, c_, (wav, tl) in zip(recs, cuts, got):
            for a, b, pcm in c_:
                assert pcm.tobytes() == pcm16(x[a:b]).tobytes()
            want, timeline, _ = _assemble(x, [(a, b) for a, b, _ in c_], mode, 480, 0, fade_ramp(480), x.shape[0])
            assert wav[44:] == want.tobytes() and tl == timeline and int.from_bytes(wav[24:28], "little") == 48000


class _NoRender:
    """an engine object of another make: everything a scan and a cut need, no render"""
    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        if name == "render":
            raise AttributeError(name)
        return getattr(self._e, name)


def test_an_engine_object_without_render_is_a_configuration_error(make_engine):
    from cutter_vad_amd import cut_recordings, render_recordings
    eng = make_engine()
    frame = eng.frame_samples
    cfg = _cfg(frame, enable_denoising=False)
    corpus = [_script(frame, [0.0] * 2 + [0.9] * 5 + [0.0] * 4)]
    bare = _NoRender(eng)
    assert cut_recordings(corpus, cfg, engine=bare, hop=frame) == cut_recordings(corpus, cfg, engine=eng, hop=frame) != [[]]
    opened = eng.info()["open_streams"]
    with pytest.raises(ConfigurationError, match="render_recordings needs an engine with render.*_NoRender has none"):
        render_recordings(corpus, cfg, engine=bare, hop=frame)
    assert eng.info()["open_streams"] == opened
