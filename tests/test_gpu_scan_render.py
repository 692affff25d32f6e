"""vad_scan_render on the GPU (csrc/scan_render.hip: vadk_scan_render).  The bar is equality: the output is BYTE FOR BYTE the rule
of tests/render_ref.py - the float32 the gained cut writes for the sample range, times the fade-in entry, times the fade-out entry,
the float32 sum where two segments meet, zero where none lies, then the cut's conversion - at the shapes where an output-driven
kernel can go wrong: ramps apart, touching, crossing and longer than the segment, lengths around a workgroup's share, overlaps of
one quad, of the whole ramp, of a whole segment and across a workgroup boundary, at both ends of the output, gaps of one quad,
no segment at all, saturating sums, every format and channel mode, rate blocks, and more workgroups than one wave of them.
hop = 4 makes every multiple of 4 from one frame up a reachable segment length."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests.cut_ref import F32, FMT, MIX, PCM16, RANGE, SENT16, SENT32, untouched, values
from tests.render_ref import raw_render, render
from tests.test_gpu_scan import _engine

pytestmark = pytest.mark.gpu

W = _ffi.VAD_CUT_WG_SAMPLES
THR = float(np.float32(0.01))
OUTS = pytest.mark.parametrize("out_fmt", [PCM16, F32], ids=["pcm16", "f32"])


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def block():
    """one stereo float32 block for the shape cases: values across the gate and beyond full scale"""
    return values(np.random.default_rng(2024), "f32", (40000, 2))


def _cos(n):
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(n) + 0.5) / max(n, 1))).astype(np.float32)


def _check(eng, items, x, channels, kind, hop, out_fmt, total, thr=THR, ramp=None, gains=None, frame=None, sr_in=0, ref_thr="same"):
    """the host form against the rule, the sentinel behind the output, and the invariants: the items reversed, a second call"""
    frame = eng.frame_samples if frame is None else frame
    t = -1.0 if thr is None else thr
    want = render(x, kind, items, frame, hop, out_fmt, thr if ref_thr == "same" else ref_thr, total, ramp, gains)
    rc, msg, out = raw_render(eng._lib, eng, items, x, channels, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp, gains=gains, sr_in=sr_in)
    assert rc == _ffi.VAD_OK, msg
    assert out[:total].tobytes() == want.tobytes(), (kind, hop, out_fmt, np.flatnonzero(out[:total] != want)[:8])
    assert untouched(out[total:])
    rc, msg, rev = raw_render(eng._lib, eng, items[::-1], x, channels, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp,
                              gains=None if gains is None else np.asarray(gains)[::-1], sr_in=sr_in)
    assert rc == _ffi.VAD_OK and rev.tobytes() == out.tobytes(), msg
    rc, msg, again = raw_render(eng._lib, eng, items, x, channels, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp, gains=gains, sr_in=sr_in)
    assert rc == _ffi.VAD_OK and again.tobytes() == out.tobytes(), msg
    return out[:total]


# ---- segment lengths --------------------------------------------------------------------------------------------------
@OUTS
@pytest.mark.parametrize("nramp", [4, 256, 260, 512, _ffi.VAD_RENDER_MAX_RAMP], ids=["apart", "touching", "crossing", "whole", "longer"])
def test_one_frame_under_every_ramp(eng, block, out_fmt, nramp):
    frame = eng.frame_samples
    assert nramp in (4, frame // 2, frame // 2 + 4, frame, _ffi.VAD_RENDER_MAX_RAMP)
    items = [(0, 5 + 200 * k, 1, 8 + (frame + 4) * k, (0, 1, MIX)[k % 3]) for k in range(6)]
    out = _check(eng, items, block, 2, "f32", 4, out_fmt, 8 + (frame + 4) * 6 + 4, ramp=_cos(nramp))
    assert out.any() or (out_fmt == PCM16 and nramp > frame)      # (both ends of the longest ramp's head: under one PCM step)


@OUTS
def test_lengths_around_a_workgroups_share(eng, block, out_fmt):
    frame, at, items = eng.frame_samples, 4, []
    for k, s in enumerate((W - 4, W, W + 4, 2 * W, 2 * W + 4)):
        items.append((4 * k, 3 * k, (s - frame) // 4 + 1, at, (MIX, 0, 1)[k % 3]))
        at += s + 4
    _check(eng, items, block, 2, "f32", 4, out_fmt, at + 8, ramp=_cos(64), gains=[1.0, -0.5, 2.0, 0.25, 1.5])


# ---- overlaps and gaps ------------------------------------------------------------------------------------------------
def _nf(s, frame):
    return (s - frame) // 4 + 1


@OUTS
def test_overlaps_of_every_kind(eng, block, out_fmt):
    frame, nramp = eng.frame_samples, 128
    n = lambda s: _nf(s, frame)
    items = [
        (0, 0, n(1000), 0, 0), (1024, 7, n(600), 0, 1),                      # an overlap at output sample 0
        (0, 50, n(2000), 1000 - 4, MIX),                                     # one quad
        (2048, 9, n(1500), 2996 - nramp, 0),                                 # exactly the ramp
        # one segment wholly inside another: a pair region of three shares, the middle one outside every fade
        (0, 400, n(4 * W), 4400, 1), (4096, 11, n(2 * W + 8), 4400 + W - 8, MIX),
    ]
    a = 4400 + 4 * W
    items += [(0, 900, n(2 * W), a + 12, 0), (1028, 1, n(frame), a + 12 + W - 100, 1),      # a frame wholly inside, off the share's grid
              (0, 77, n(700), a + 12 + 2 * W - 700, MIX)]                    # ... and an overlap that ends at out_samples
    total = a + 12 + 2 * W
    cover = np.zeros(total, np.int32)
    for it in items:
        cover[it[3]:it[3] + (it[2] - 1) * 4 + frame] += 1
    assert cover.max() == 2 and cover[0] == 2 and cover[-1] == 2 and (cover == 0).sum() == 32 + 12 and (cover[996:1000] == 2).all()
    assert (cover[2996 - nramp:2996] == 2).all() and cover[2996] == 1
    _check(eng, items, block, 2, "f32", 4, out_fmt, total, ramp=_cos(nramp), gains=np.linspace(-1.5, 1.5, len(items)))
    _check(eng, items, block, 2, "f32", 4, out_fmt, total)                   # no ramp, no gains: plain sums


@OUTS
def test_gaps_of_one_quad_at_both_ends_and_no_segment_at_all(eng, block, out_fmt):
    frame = eng.frame_samples
    items = [(0, 3, _nf(900, frame), 4, 0), (0, 300, _nf(frame, frame), 908, 1), (0, 700, _nf(W + 4, frame), 908 + frame + 2 * W + 8, MIX)]
    total = items[2][3] + W + 4 + 4
    out = _check(eng, items, block, 2, "f32", 4, out_fmt, total, ramp=_cos(32))
    assert not out[:4].any() and not out[904:908].any() and not out[908 + frame:items[2][3]].any() and not out[-4:].any()
    assert out[4:904].any()
    rc, msg, zeros = raw_render(eng._lib, eng, [], block, 2, FMT["f32"], 4, out_fmt, 4096, ramp=_cos(32))
    assert rc == _ffi.VAD_OK and not zeros[:4096].any() and untouched(zeros[4096:]), msg
    assert zeros[:4096].tobytes() == bytes(4096 * zeros.itemsize)            # +0.0f, never -0.0f


def test_sums_saturate_in_pcm16(eng):
    frame = eng.frame_samples
    x = np.concatenate([np.full(frame, 0.9, np.float32), np.full(frame, -0.9, np.float32)])
    items = [(0, 0, 1, 0, 0), (0, 0, 1, 0, 0), (0, 1, 1, frame, 0), (0, 1, 1, frame, 0)]
    out = _check(eng, items, x, 1, "f32", frame, PCM16, 2 * frame, thr=None)
    assert (out[:frame] == 32767).all() and (out[frame:] == -32768).all()
    f = _check(eng, items, x, 1, "f32", frame, F32, 2 * frame, thr=None)
    assert (f[:frame] == np.float32(0.9) + np.float32(0.9)).all()


# ---- formats and blocks -----------------------------------------------------------------------------------------------
def _mixed(frame, hop, chans):
    """five segments: two crossfading, a gap, one inside another, all with ragged lengths"""
    nfs, offs = [3, 9, 40, 5, 1], [0, 4, 1028, 8, 2052]
    c = [(nf - 1) * hop + frame for nf in nfs]
    at = [4, 4 + c[0] - 64]
    at.append(at[1] + c[1] + 12)
    at.append(at[2] + 8)
    at.append(at[2] + c[2] - 4)
    assert at[3] + c[3] <= at[4]
    return [(offs[k], 2 * k, nfs[k], at[k], chans[k % len(chans)]) for k in range(5)], at[4] + c[4] + 4


@OUTS
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", list(FMT))
def test_every_format_and_channel_mode(eng, kind, channels, out_fmt):
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    x = values(np.random.default_rng(len(kind) + channels), kind, (9000, 2) if channels == 2 else 9000)
    items, total = _mixed(frame, hop, (0, 1, MIX) if channels == 2 else (0,))
    for thr in (None, 0.3):
        _check(eng, items, x, channels, kind, hop, out_fmt, total, thr=thr, ramp=_cos(64), gains=[0.5, -3.0, 1.0, 2.0 ** -12, 40.0])


@OUTS
@pytest.mark.parametrize("rate,chunk", [(8000, 256), (48000, 1536)], ids=["8k", "48k"])
def test_rate_blocks_are_never_gated(eng, rate, chunk, out_fmt):
    hop = chunk // 2 + 4
    x = values(np.random.default_rng(rate), "i16_32767", (chunk + 60 * hop, 2))
    items, total = _mixed(chunk, hop, (MIX, 1, 0))
    out = _check(eng, items, x, 2, "i16_32767", hop, out_fmt, total, thr=0.3, ramp=_cos(64), frame=chunk, sr_in=rate, ref_thr=None)
    gated = render(x, "i16_32767", items, chunk, hop, out_fmt, 0.3, total, _cos(64))
    assert out.tobytes() != gated.tobytes()
    assert eng._lib.vad_rate_cut_samples(eng.handle, items[2][2], rate, hop, RANGE) == (items[2][2] - 1) * hop + chunk


# ---- the grid ---------------------------------------------------------------------------------------------------------
def test_more_workgroups_than_one_wave_of_them(eng, block):
    frame = eng.frame_samples
    rng = np.random.default_rng(300)
    firsts = rng.integers(0, (40000 - frame) // 4, 300)
    items, at = [], 0
    for k in range(300):
        items.append((0, int(firsts[k]), 1, at, (0, 1, MIX)[k % 3]))
        at += frame + (-64 if k % 4 == 0 else 8 if k % 4 == 1 else 0)          # crossfaded, a gap, back to back
    total = at + 64
    gains = rng.uniform(-2.0, 2.0, 300).astype(np.float32)
    _check(eng, items, block, 2, "f32", 4, PCM16, total, ramp=_cos(64), gains=gains)


# ---- the invariants ---------------------------------------------------------------------------------------------------
@OUTS
def test_without_ramp_and_overlap_the_segments_are_the_gained_cut(eng, block, out_fmt):
    frame, hop = eng.frame_samples, 4
    items = [(0, 3, 1, 8, 1), (1024, 0, 2500, 8 + frame, MIX), (0, 1, 2, 8 + frame + 2499 * 4 + frame + 4, 0)]
    total = items[2][3] + 4 + frame + 12
    gains = np.array([2.0, 0.5, -1.0], np.float32)
    segs = [(o, f, n, c if c != MIX else "mix") for o, f, n, _, c in items]
    cut, start = eng.cut(segs, hop=hop, denoise=THR, layout="range", out="pcm16" if out_fmt == PCM16 else "f32", audio=block, gains=gains)
    out = _check(eng, items, block, 2, "f32", hop, out_fmt, total, gains=gains)
    covered = np.zeros(total, bool)
    for k, it in enumerate(items):
        assert out[it[3]:it[3] + start[k + 1] - start[k]].tobytes() == cut[start[k]:start[k + 1]].tobytes()
        covered[it[3]:it[3] + start[k + 1] - start[k]] = True
    assert not out[~covered].any() and (~covered).sum() == 8 + 4 + 12
    ones = _check(eng, items, block, 2, "f32", hop, out_fmt, total, gains=np.ones(3, np.float32))
    assert ones.tobytes() == _check(eng, items, block, 2, "f32", hop, out_fmt, total).tobytes()      # no gains: gains of ones


@OUTS
def test_the_device_form_equals_the_host_form(eng, block, out_fmt):
    import torch
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    items, total = _mixed(frame, hop, (MIX, 0, 1))
    segs = [(o, f, n, c if c != MIX else "mix") for o, f, n, _, c in items]
    starts = [it[3] for it in items]
    ramp, gains = _cos(64), [0.5, -3.0, 1.0, 0.25, 4.0]
    out = "pcm16" if out_fmt == PCM16 else "f32"
    want = eng.render(segs, starts, total, hop=hop, ramp=ramp, gains=gains, denoise=THR, out=out, audio=block)
    assert want.tobytes() == render(block, "f32", items, frame, hop, out_fmt, THR, total, ramp, gains).tobytes()
    d_audio = torch.from_numpy(block).cuda()
    sent = SENT16 if out_fmt == PCM16 else SENT32
    d_out = torch.full((total + 8,), float(sent) if out_fmt == F32 else int(sent), dtype=torch.int16 if out_fmt == PCM16 else torch.float32,
                       device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.render_device(segs, starts, d_audio.data_ptr(), block.shape[0], d_out.data_ptr(), total, hop=hop, ramp=ramp, gains=gains, channels=2,
                      denoise=THR, out=out, stream=stream.cuda_stream)
    stream.synchronize()
    got = d_out.cpu().numpy()
    assert got[:total].tobytes() == want.tobytes() and untouched(got[total:])
    # the resident block of the host call above is still there for audio=None through the C ABI
    rc, msg, again = raw_render(eng._lib, eng, items, None, 2, FMT["f32"], hop, out_fmt, total, thr=THR, ramp=ramp, gains=gains,
                                audio_samples=block.shape[0])
    assert rc == _ffi.VAD_OK and again[:total].tobytes() == want.tobytes(), msg
