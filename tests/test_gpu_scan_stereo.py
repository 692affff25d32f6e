"""vad_scan_cut_stereo / vad_scan_render_stereo on the GPU (csrc/scan_cut.hip, csrc/scan_render.hip).  The bar is
equality, twice: every case is BYTE FOR BYTE the numpy rule of tests/stereo_ref.py (the mono references per channel, interleaved)
AND what Engine.cut / Engine.render give per channel on the same GPU, interleaved - at the shapes where the kernels can go wrong:
segment lengths around one lane's pass, one pass of the workgroup, a workgroup's share and two shares, frames at both hops, every
wire format with the gate acting on one channel of a sample frame only, rate blocks, every kind of share of the render, the device
form, the resident block of a scan, and the corpus functions with keep_channels.  Left and right differ in seed and scale and
neither is silent: a kernel that writes one channel twice, or swaps them, fails every case."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import g711_ref as G
from tests.cut_ref import F32, FMT, FRAMES, PCM16, RANGE, SENT16, SENT32, decode, gate, pcm16, untouched, values
from tests.stereo_ref import cut_stereo_ref, interleave, raw_cut_stereo, raw_render_stereo, render_stereo_ref
from tests.test_gpu_scan import GOLD, _engine

pytestmark = pytest.mark.gpu

W = _ffi.VAD_CUT_WG_SAMPLES
THR = float(np.float32(0.01))
OUTS = pytest.mark.parametrize("out_fmt", [PCM16, F32], ids=["pcm16", "f32"])
GAINS5 = [0.5, -3.0, 1.0, 2.0 ** -12, 40.0]
OUT_NAME = {PCM16: "pcm16", F32: "f32"}
LAY_NAME = {FRAMES: "frames", RANGE: "range"}


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


def _two(rng, kind, n):
    """[n, 2] in the wire format `kind`: left and right differ in seed and in scale, neither is silent"""
    if kind == "f32":
        return interleave(rng.uniform(-1.2, 1.2, n).astype(np.float32), rng.uniform(-0.3, 0.3, n).astype(np.float32))
    if kind.startswith("i16"):
        return interleave(rng.integers(-32768, 32768, n).astype(np.int16), rng.integers(-3000, 3000, n).astype(np.int16))
    return interleave(values(rng, kind, n), values(rng, kind, n))


@pytest.fixture(scope="module")
def block():
    """one two-channel float32 block for the shape cases: values across the gate and, on the left, beyond full scale"""
    return _two(np.random.default_rng(2025), "f32", 40000)


def _engine_kw(kind):
    return dict(law=kind if kind in ("ulaw", "alaw") else None, i16_scale=32768 if kind == "i16_32768" else 32767)


def _check_cut(eng, items, x, kind, hop, layout, out_fmt, total, thr=THR, gains=None, frame=None, sr_in=0, ref_thr="same"):
    """the host form against the rule per segment, the sentinel everywhere else, and Engine.cut per channel on this GPU"""
    frame = eng.frame_samples if frame is None else frame
    t = -1.0 if thr is None else thr
    rc, msg, out = raw_cut_stereo(eng._lib, eng, items, x, 2, FMT[kind], hop, layout, out_fmt, total, thr=t, gains=gains, sr_in=sr_in)
    assert rc == _ffi.VAD_OK, msg
    segs = [tuple(it[:3]) for it in items]
    mono = [eng.cut([sg + (c,) for sg in segs], hop=hop, denoise=thr, layout=LAY_NAME[layout], out=OUT_NAME[out_fmt], audio=x, gains=gains,
                    sample_rate=sr_in or None, **_engine_kw(kind)) for c in (0, 1)]
    start = mono[0][1]
    written = np.zeros(total, bool)
    for k, it in enumerate(items):
        want = cut_stereo_ref(x, kind, it, frame, hop, layout, out_fmt, thr if ref_thr == "same" else ref_thr, None if gains is None else gains[k])
        n, o = want.shape[0], it[3]
        got = out[2 * o:2 * (o + n)]
        assert got.tobytes() == want.tobytes(), (kind, k, layout, out_fmt, np.flatnonzero(got != want.reshape(-1))[:8])
        assert got.tobytes() == interleave(mono[0][0][start[k]:start[k + 1]], mono[1][0][start[k]:start[k + 1]]).tobytes(), (kind, k)
        assert not written[o:o + n].any()
        written[o:o + n] = True
    assert untouched(out[:2 * total].reshape(-1, 2)[~written]) and untouched(out[2 * total:])
    return out[:2 * total].reshape(-1, 2), written


def _check_render(eng, items, x, kind, hop, out_fmt, total, thr=THR, ramp=None, gains=None, frame=None, sr_in=0, ref_thr="same"):
    """the host form against the rule and against Engine.render per channel on this GPU; the items reversed; a second call"""
    frame = eng.frame_samples if frame is None else frame
    t = -1.0 if thr is None else thr
    want = render_stereo_ref(x, kind, items, frame, hop, out_fmt, thr if ref_thr == "same" else ref_thr, total, ramp, gains)
    rc, msg, out = raw_render_stereo(eng._lib, eng, items, x, 2, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp, gains=gains, sr_in=sr_in)
    assert rc == _ffi.VAD_OK, msg
    assert out[:2 * total].tobytes() == want.tobytes(), (kind, hop, out_fmt, np.flatnonzero(out[:2 * total] != want.reshape(-1))[:8])
    assert untouched(out[2 * total:])
    segs = [tuple(it[:3]) for it in items]
    mono = [eng.render([sg + (c,) for sg in segs], [it[3] for it in items], total, hop=hop, ramp=ramp, gains=gains, denoise=thr,
                       out=OUT_NAME[out_fmt], audio=x, sample_rate=sr_in or None, **_engine_kw(kind)) for c in (0, 1)]
    assert out[:2 * total].tobytes() == interleave(*mono).tobytes()
    rc, msg, rev = raw_render_stereo(eng._lib, eng, items[::-1], x, 2, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp,
                                     gains=None if gains is None else np.asarray(gains)[::-1], sr_in=sr_in)
    assert rc == _ffi.VAD_OK and rev.tobytes() == out.tobytes(), msg
    rc, msg, again = raw_render_stereo(eng._lib, eng, items, x, 2, FMT[kind], hop, out_fmt, total, thr=t, ramp=ramp, gains=gains, sr_in=sr_in)
    assert rc == _ffi.VAD_OK and again.tobytes() == out.tobytes(), msg
    return out[:2 * total].reshape(-1, 2)


def _cos(n):
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(n) + 0.5) / max(n, 1))).astype(np.float32)


# ---- the cut: lengths -------------------------------------------------------------------------------------------------
QUADS = [128, 255, 256, 257, 1023, 1024, 1025, 2049]      # one lane's pass | one pass of the workgroup | its share | two shares


@OUTS
@pytest.mark.parametrize("gained", [False, True], ids=["plain", "gains"])
def test_cut_lengths_around_a_pass_a_share_and_two(eng, block, out_fmt, gained):
    frame = eng.frame_samples
    assert frame == 512
    order = [5, 0, 7, 2, 4, 1, 6, 3]                      # listed out of order ...
    at, place = 8, {}
    for k in range(len(QUADS)):                           # ... with gaps between their outputs
        place[k] = at
        at += 4 * QUADS[k] + 4 * (1 + k % 3)
    total = at + 4
    items = [(4 * k, 3 * k, QUADS[k] - 127, place[k]) for k in order]
    assert all((it[2] - 1) * 4 + frame == 4 * QUADS[k] for it, k in zip(items, order))
    gains = [GAINS5[j % 5] for j in range(len(items))] if gained else None
    got, written = _check_cut(eng, items, block, "f32", 4, RANGE, out_fmt, total, gains=gains)
    assert (~written).sum() == 8 + 4 + sum(4 * (1 + k % 3) for k in range(8))
    assert not np.array_equal(got[written][:, 0], got[written][:, 1]) and got[written][:, 0].any() and got[written][:, 1].any()


@OUTS
@pytest.mark.parametrize("hop", [256, 512])
def test_cut_frames_at_both_hops(eng, block, out_fmt, hop):
    frame = eng.frame_samples
    items, at = [], 0
    for k, nf in enumerate((9, 1, 2)):
        items.append((8 * k, 5 * k, nf, at + 4))
        at += 4 + nf * frame
    _check_cut(eng, items, block, "f32", hop, FRAMES, out_fmt, at + 8, gains=GAINS5[:3])
    _check_cut(eng, items, block, "f32", hop, FRAMES, out_fmt, at + 8)


# ---- formats and the gate ---------------------------------------------------------------------------------------------
def _near_gate_code(kind):
    """a sample of the wire format whose decoded magnitude is the gate's 0.01 (float32: exactly; else the nearest code)"""
    if kind == "f32":
        return np.float32(0.01)
    if kind.startswith("i16"):
        return np.int16(328)
    tab = G.table(kind).astype(np.float64) / 32768.0
    return np.uint8(np.argmin(np.abs(tab - 0.01)))


@OUTS
@pytest.mark.parametrize("kind", list(FMT))
def test_every_format_and_the_gate_per_channel(eng, kind, out_fmt):
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    x = _two(np.random.default_rng(len(kind) + 40), kind, 9000)
    v = _near_gate_code(kind)
    x[1::7, 0] = v                                        # at the threshold on the LEFT only ...
    x[3::7, 1] = v                                        # ... and on the RIGHT only
    at_gate = float(decode(np.array([v]), kind)[0])
    assert abs(at_gate - 0.01) < 3e-4 and (kind != "f32" or at_gate == THR)
    d = decode(x, kind)
    assert (np.abs(d[1::7, 1]) != np.float32(at_gate)).any() and (np.abs(d[3::7, 0]) > np.float32(at_gate)).any()
    items = [(1028, 1, 2, 520), (0, 0, 1, 0), (2052, 3, 9, 1552), (8, 2, 40, 6164)]      # out of order, gaps in either layout
    total = 6164 + 39 * hop + frame + 4
    for thr in (None, THR, at_gate):
        for layout in (RANGE, FRAMES) if thr == THR else (RANGE,):
            tot = total if layout == RANGE else 6164 + 40 * frame + 4
            got, written = _check_cut(eng, items, x, kind, hop, layout, out_fmt, tot, thr=thr, gains=GAINS5[:4] if thr == THR else None)
        if thr == at_gate:
            # the range of items[1] is x[0:512]: a frame at the threshold on one channel is zero there and kept on the other
            seg = got[0:frame]
            assert not seg[1::7, 0].any() and not seg[3::7, 1].any()
            assert (seg[1::7, 1] != 0).any() and (seg[3::7, 0] != 0).any()
    items_r = [(0, 0, 3, 4), (4, 2, 9, 4 + 2 * hop + frame - 64), (1028, 1, 2, 4 + 10 * hop + 2 * frame - 64 + 12)]
    total_r = items_r[2][3] + hop + frame + 4
    for thr in (None, at_gate):
        _check_render(eng, items_r, x, kind, hop, out_fmt, total_r, thr=thr, ramp=_cos(64), gains=GAINS5[:3])


@OUTS
@pytest.mark.parametrize("rate,chunk", [(8000, 256), (24000, 768), (48000, 1536)], ids=["8k", "24k", "48k"])
def test_rate_blocks_give_the_range_ungated(eng, rate, chunk, out_fmt):
    hop = chunk // 2 + 4
    x = _two(np.random.default_rng(rate), "i16_32767", chunk + 30 * hop)
    items = [(4, 3, 9, 8), (0, 0, 1, 8 + 8 * hop + chunk + 4), (8, 20, 5, 8 + 8 * hop + 2 * chunk + 12)]
    total = items[2][3] + 4 * hop + chunk + 4
    got, written = _check_cut(eng, items, x, "i16_32767", hop, RANGE, out_fmt, total, thr=0.3, gains=GAINS5[:3], frame=chunk, sr_in=rate,
                              ref_thr=None)
    gated = cut_stereo_ref(x, "i16_32767", items[1], chunk, hop, RANGE, out_fmt, 0.3, GAINS5[1])
    o = items[1][3]
    assert got[o:o + chunk].tobytes() != gated.tobytes()
    rc, msg, out = raw_cut_stereo(eng._lib, eng, items, x, 2, FMT["i16_32767"], hop, FRAMES, out_fmt, total, sr_in=rate)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "VAD_CUT_FRAMES on a block at" in msg and untouched(out), msg
    items_r = [(4, 3, 9, 8), (0, 0, 1, 8 + 8 * hop + chunk - 32)]
    _check_render(eng, items_r, x, "i16_32767", hop, out_fmt, items_r[1][3] + chunk + 8, thr=0.3, ramp=_cos(32), frame=chunk, sr_in=rate,
                  ref_thr=None)


# ---- the render -------------------------------------------------------------------------------------------------------
def _nf(s, frame):
    return (s - frame) // 4 + 1


@OUTS
@pytest.mark.parametrize("nramp", [4, 260, _ffi.VAD_RENDER_MAX_RAMP], ids=["shorter", "crossing", "longer"])
def test_render_one_frame_under_ramps_shorter_and_longer_than_the_segment(eng, block, out_fmt, nramp):
    frame = eng.frame_samples
    items = [(0, 5 + 200 * k, 1, 8 + (frame + 4) * k) for k in range(3)]
    _check_render(eng, items, block, "f32", 4, out_fmt, 8 + (frame + 4) * 3 + 4, ramp=_cos(nramp))


@OUTS
def test_render_overlaps_of_every_kind_gaps_and_a_workgroups_share(eng, block, out_fmt):
    frame, nramp = eng.frame_samples, 128
    n = lambda s: _nf(s, frame)
    items = [
        (0, 0, n(1000), 4), (1024, 7, n(600), 4),                            # a gap of one quad, then an overlap from its first sample
        (0, 50, n(2000), 1004 - 4),                                          # one quad
        (2048, 9, n(1500), 3000 - nramp),                                    # exactly the ramp
        # one segment wholly inside another: a pair region across a share's boundary, its middle outside every fade
        (0, 400, n(2 * W + 8), 4400), (4096, 11, n(W + 8), 4400 + W - 8),
    ]
    a = 4400 + 2 * W + 8
    for k, s in enumerate((W - 4, W, W + 4)):                                # lengths around a workgroup's share, a quad apart
        items.append((4 * k, 3 * k, n(s), a + 4))
        a += 4 + s
    items.append((0, 77, n(700), a - 100))                                   # an overlap that ends 4 samples before out_samples
    total = a - 100 + 700 + 4
    cover = np.zeros(total, np.int32)
    for it in items:
        cover[it[3]:it[3] + (it[2] - 1) * 4 + frame] += 1
    assert cover.max() == 2 and not cover[:4].any() and not cover[-4:].any() and cover[4] == 2 and (cover[1000:1004] == 2).all()
    out = _check_render(eng, items, block, "f32", 4, out_fmt, total, ramp=_cos(nramp), gains=np.linspace(-1.5, 1.5, len(items)))
    assert not out[cover == 0].any() and out[cover == 0].tobytes() == bytes(out[cover == 0].nbytes)      # +0.0f in both channels
    _check_render(eng, items, block, "f32", 4, out_fmt, total)               # no ramp, no gains: plain sums
    rc, msg, zeros = raw_render_stereo(eng._lib, eng, [], block, 2, FMT["f32"], 4, out_fmt, 4096, ramp=_cos(32))
    assert rc == _ffi.VAD_OK and zeros[:8192].tobytes() == bytes(8192 * zeros.itemsize) and untouched(zeros[8192:]), msg


def test_render_saturates_in_pcm16_on_one_channel_only(eng):
    frame = eng.frame_samples
    x = np.zeros((2 * frame, 2), np.float32)
    x[:frame, 0], x[frame:, 0] = 0.9, -0.9                # the left channel's sums pass full scale ...
    x[:frame, 1], x[frame:, 1] = 0.25, -0.125             # ... the right one's do not
    items = [(0, 0, 1, 0), (0, 0, 1, 0), (0, 1, 1, frame), (0, 1, 1, frame)]
    out = _check_render(eng, items, x, "f32", frame, PCM16, 2 * frame, thr=None)
    assert (out[:frame, 0] == 32767).all() and (out[frame:, 0] == -32768).all()
    assert (out[:frame, 1] == pcm16(np.float32(0.5))).all() and (out[frame:, 1] == pcm16(np.float32(-0.25))).all()
    f = _check_render(eng, items, x, "f32", frame, F32, 2 * frame, thr=None)
    assert (f[:frame, 0] == np.float32(0.9) + np.float32(0.9)).all() and (f[:frame, 1] == np.float32(0.5)).all()


# ---- the device form and the resident block ---------------------------------------------------------------------------
@OUTS
def test_the_device_forms_equal_the_host_forms(eng, block, out_fmt):
    import torch
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    segs = [(0, 0, 3), (4, 2, 9), (1028, 1, 40)]
    gains, ramp, out = GAINS5[:3], _cos(64), OUT_NAME[out_fmt]
    sent = SENT16 if out_fmt == PCM16 else SENT32
    dt = torch.int16 if out_fmt == PCM16 else torch.float32
    d_audio = torch.from_numpy(block).cuda()
    stream = torch.cuda.Stream()
    try:
        for layout in ("range", "frames"):
            want, start = eng.cut_stereo(segs, hop=hop, denoise=THR, layout=layout, out=out, audio=block, gains=gains)
            n = int(start[-1])
            d_out = torch.full((n + 4, 2), float(sent) if out_fmt == F32 else int(sent), dtype=dt, device="cuda")
            torch.cuda.synchronize()
            st = eng.cut_stereo_device(segs, d_audio.data_ptr(), block.shape[0], d_out.data_ptr(), n, hop=hop, denoise=THR, layout=layout,
                                       out=out, stream=stream.cuda_stream, gains=gains)
            stream.synchronize()
            got = d_out.cpu().numpy()
            assert np.array_equal(st, start) and got[:n].tobytes() == want.tobytes() and untouched(got[n:])
        starts = [4, 4 + 2 * hop + frame - 64, 4 + 10 * hop + 2 * frame - 64 + 12]
        total = starts[2] + 39 * hop + frame + 4
        want = eng.render_stereo(segs, starts, total, hop=hop, ramp=ramp, gains=gains, denoise=THR, out=out, audio=block)
        d_out = torch.full((total + 4, 2), float(sent) if out_fmt == F32 else int(sent), dtype=dt, device="cuda")
        torch.cuda.synchronize()
        eng.render_stereo_device(segs, starts, d_audio.data_ptr(), block.shape[0], d_out.data_ptr(), total, hop=hop, ramp=ramp, gains=gains,
                                 denoise=THR, out=out, stream=stream.cuda_stream)
        stream.synchronize()
        got = d_out.cpu().numpy()
        assert got[:total].tobytes() == want.tobytes() and untouched(got[total:])
        items = [sg + (st,) for sg, st in zip(segs, starts)]
        assert want.tobytes() == render_stereo_ref(block, "f32", items, frame, hop, out_fmt, THR, total, ramp, gains).tobytes()
    finally:
        del d_audio
        torch.cuda.empty_cache()


def test_the_resident_block_of_a_scan_of_two_channel_recordings(eng):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(77)
    recs = [_two(rng, "i16_32767", frame + 9 * hop + 2), _two(rng, "i16_32767", frame + 3 * hop)]
    slots = np.asarray(eng.open_streams(2))
    try:
        with eng.scan_session():
            eng.scan_segments(slots, recs, hop=hop, denoise=THR, channel="mix")
            o1 = int(eng.last_scan["offsets"][1])
            segs = [(0, 1, 4), (o1, 0, 3)]
            data, start = eng.cut_stereo(segs, hop=hop, layout="range", denoise=THR, gains=[2.0, 0.5])
            frames, fstart = eng.cut_stereo(segs, hop=hop, layout="frames", denoise=THR)
            ren = eng.render_stereo(segs, [0, int(start[1]) - 32], int(start[2]) - 32, hop=hop, ramp=_cos(32), denoise=THR, out="f32")
            mono = [eng.cut([sg + (c,) for sg in segs], hop=hop, layout="range", denoise=THR, gains=[2.0, 0.5])[0] for c in (0, 1)]
    finally:
        for s in slots:
            eng.close_stream(int(s))
    src = [(recs[0], (0, 1, 4, 0)), (recs[1], (0, 0, 3, 0))]
    want = np.concatenate([cut_stereo_ref(r, "i16_32767", it, frame, hop, RANGE, PCM16, THR, g) for (r, it), g in zip(src, (2.0, 0.5))])
    assert data.tobytes() == want.tobytes() == interleave(*mono).tobytes()
    assert frames.tobytes() == np.concatenate([cut_stereo_ref(r, "i16_32767", it, frame, hop, FRAMES, PCM16, THR) for r, it in src]).tobytes()
    block = np.zeros((o1 + recs[1].shape[0], 2), np.int16)
    block[:recs[0].shape[0]] = recs[0]
    block[o1:] = recs[1]
    items = [(0, 1, 4, 0), (o1, 0, 3, int(start[1]) - 32)]
    assert ren.tobytes() == render_stereo_ref(block, "i16_32767", items, frame, hop, F32, THR, int(start[2]) - 32, _cos(32)).tobytes()


# ---- the corpus functions ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """three short two-channel recordings and a 1-D one out of the speech golden: the right channel is other speech at half the
    level, so the channels differ everywhere and both have speech"""
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float32) / np.float32(32767.0)
    s = lambda a, b: pcm[int(a * 16000):int(b * 16000)]
    two = lambda l, r: interleave(l, (r * np.float32(0.5)).astype(np.float32))
    return [two(s(0, 4), s(4, 8)), s(4, 8).copy(), two(s(8.5, 13), s(4, 8.5)), two(s(13, 16.5), s(0.5, 4))]


def _header_is_two_channel(wav, nbytes, rate=16000):
    return (wav[:4] == b"RIFF" and int.from_bytes(wav[22:24], "little") == 2 and int.from_bytes(wav[24:28], "little") == rate
            and int.from_bytes(wav[32:34], "little") == 4 and int.from_bytes(wav[40:44], "little") == nbytes == len(wav) - 44)


def test_cut_recordings_keeps_both_channels(eng, corpus):
    """Column c of the payload is the payload of cut_recordings(channel=c) without keep_channels - the same function, the same
    scan - and the whole payload is Engine.cut per channel over the same ranges at gain 1, interleaved, behind a two-channel
    header.  normalize=0.9: np.float32(0.9) / max(peak_L, peak_R) of the gated range, one factor for both channels."""
    from cutter_vad_amd import VADConfig, cut_recordings
    cfg = VADConfig()
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    thr = 0.01 if cfg.enable_denoising else None
    seen = 0
    for channel in (0, 1, "mix"):
        for layout in ("range", "frames"):
            both = cut_recordings(corpus, cfg, engine=eng, channel=channel, layout=layout, keep_channels=True)
            plain = cut_recordings(corpus, cfg, engine=eng, channel=channel, layout=layout)
            assert both[1] == plain[1]                    # the 1-D recording goes the mono way
            for i in (0, 2, 3):
                x = corpus[i]
                assert [(a, b) for a, b, _ in both[i]] == [(a, b) for a, b, _ in plain[i]]
                for (a, b, wav), (_, _, one) in zip(both[i], plain[i]):
                    sg = (0, a // hop, (b - a - frame) // hop + 1)
                    cols = [eng.cut([sg + (c,)], hop=hop, denoise=thr, layout=layout, audio=x)[0] for c in (0, 1)]
                    want = interleave(*cols)
                    assert _header_is_two_channel(wav, want.nbytes, cfg.output_wav_sample_rate) and wav[44:] == want.tobytes()
                    if channel != "mix":
                        assert np.frombuffer(wav[44:], np.int16).reshape(-1, 2)[:, channel].tobytes() == one[44:]
                    assert cols[0].any() and cols[1].any() and not np.array_equal(cols[0], cols[1])
                    seen += 1
    assert seen >= 6, seen
    n = 0
    got = cut_recordings(corpus, cfg, engine=eng, layout="range", wav=False, keep_channels=True, normalize=0.9)
    for i in (0, 2, 3):
        for a, b, arr in got[i]:
            h = gate(corpus[i][a:b], thr)
            g = np.float32(np.float32(0.9) / np.abs(h).max())
            assert arr.shape == (b - a, 2) and arr.tobytes() == pcm16((h * g).astype(np.float32)).tobytes()
            assert max(np.abs(arr[:, 0]).max(), np.abs(arr[:, 1]).max()) >= 29489 and np.abs(arr[:, 1]).max() > 0      # 0.9 of full scale
            n += 1
    assert n >= 1


@pytest.mark.parametrize("mode", ["join", "mask"])
def test_render_recordings_keeps_both_channels(eng, corpus, mode):
    """as above for the pieces: column c is render_recordings(channel=c)'s payload, the whole is Engine.render per channel at the
    timeline's places; normalize=0.9 applies the joint-peak gain of each listed segment to both channels"""
    from cutter_vad_amd import VADConfig, render_recordings
    from cutter_vad_amd.scan import fade_ramp
    cfg = VADConfig()
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    thr = 0.01 if cfg.enable_denoising else None
    ramp = fade_ramp(160)
    seen = 0
    for channel, norm in ((0, None), (1, None), ("mix", 0.9)):
        both = render_recordings(corpus, cfg, engine=eng, channel=channel, mode=mode, keep_channels=True, normalize=norm)
        plain = render_recordings(corpus, cfg, engine=eng, channel=channel, mode=mode, normalize=norm)
        assert both[1] == plain[1]
        for i in (0, 2, 3):
            x = corpus[i]
            (wav, tl), (one, tl1) = both[i], plain[i]
            assert tl == tl1
            if not tl:
                continue
            segs = [(0, a // hop, (n - frame) // hop + 1) for _, a, n in tl]
            size = (x.shape[0] + 3) // 4 * 4 if mode == "mask" else tl[-1][0] + tl[-1][2]
            gains = None if norm is None else [np.float32(np.float32(norm) / np.abs(gate(x[a:a + n], thr)).max()) for _, a, n in tl]
            cols = [eng.render([sg + (c,) for sg in segs], [p for p, _, _ in tl], size, hop=hop, ramp=ramp, gains=gains, denoise=thr, audio=x)
                    for c in (0, 1)]
            want = interleave(*cols)[:x.shape[0] if mode == "mask" else size]
            assert _header_is_two_channel(wav, want.nbytes, cfg.output_wav_sample_rate) and wav[44:] == want.tobytes(), (channel, i)
            if norm is None:
                assert np.frombuffer(wav[44:], np.int16).reshape(-1, 2)[:, channel].tobytes() == one[44:]
            assert cols[0].any() and cols[1].any()
            seen += 1
    assert seen >= 3, seen
