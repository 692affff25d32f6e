"""vad_scan_mel on the GPU (csrc/scan_mel.hip: vadk_seg_mel).  Layout is tested byte for byte: on samples |s| <= 8 of 32768,
operators with at most four +-1 per column and filters in {0, 1, 2} every float32 operation is exact in any order of summation
(tests/mel_ref.py asserts that precondition on its own int64 evaluation before anything is compared), so a wrong sample, bin, frame,
filter or row is a wrong byte.  Numerics on real operators are held to the derived bound |E - E_f64| <= (2 n_fft + n_bins + 8) u D,
the logarithms to 4 u max(|y|, 1) where their argument is exact and to the bound's own shift where it is not.  MEL_TILE is 16: the
segments around a tile have 15, 16, 17 and 35 frames."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import mel_ref as R
from tests.cut_ref import FMT, MIX, gate, heard
from tests.test_gpu_scan import GOLD, _engine
from tests.test_scan_mel_host import EXACT_KINDS, GEO, _exact_block, want_plain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


def _kw(kind):
    return dict(law=kind if kind in ("ulaw", "alaw") else None, i16_scale=32768)


def _exact(eng, segs, f, ops, x, kind, hop, denoise=None):
    """Engine.mel against the exact reference, byte for byte -> (features, start)"""
    got, start = eng.mel(segs, (f, *ops), hop=hop, audio=x, denoise=denoise, **_kw(kind))
    want = []
    for sg in segs:
        a = sg[0] + sg[1] * hop
        ch = MIX if len(sg) > 3 and sg[3] == "mix" else sg[3] if len(sg) > 3 else (MIX if x.ndim == 2 else 0)
        want.append(gate(heard(x, kind, ch), denoise)[a:a + (sg[2] - 1) * hop + eng.frame_samples])
    rows, rstart = R.rows_of(want, f, *ops, exact=True)
    assert start.tolist() == rstart.tolist() and got.shape == rows.shape and got.dtype == np.float32
    if f["log"] == R.LINEAR:
        assert got.tobytes() == rows.astype(np.float32).tobytes(), (f, np.argwhere(got != rows.astype(np.float32))[:4].tolist())
    else:
        assert (np.abs(got - rows) <= R.log_tolerance(rows)).all(), f
    return got, start


# ---- exact cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_formats_and_channels_byte_for_byte(eng, kind, channels):
    """n_fft = 64, hop = 16, 33 bins and 5 mels: both paddings to 16 are live; left, right and mix; the gate off and zeroing samples"""
    frame, hop = eng.frame_samples, 132
    rng = np.random.default_rng(len(kind) + 10 * channels)
    ns = 9000
    x = _exact_block(rng, kind, (ns, 2) if channels == 2 else ns)
    chans = (0, 1, "mix") if channels == 2 else (0,)
    segs = []
    for k in range(9):
        off = (0, 1028, 2000)[k % 3]
        room = (ns - off - frame) // hop + 1
        nf = int(rng.integers(1, min(room, 12) + 1))
        segs.append((off, int(rng.integers(0, room - nf + 1)), nf, chans[k % len(chans)]))
    thr = 2.5 / 32768 if kind in ("f32", "i16_32768") else 16.5 / 32768
    for pad in (R.NONE, R.REFLECT):
        ops = R.exact_operators(rng, 64, 33, 5)
        plain, _ = _exact(eng, segs, R.fields(**GEO, pad=pad), ops, x, kind, hop)
        gated, _ = _exact(eng, segs, R.fields(**GEO, pad=pad), ops, x, kind, hop, denoise=thr)
        assert plain.tobytes() != gated.tobytes()           # the gate zeroed samples that entered a frame
    lin = _exact(eng, segs, R.fields(**GEO, pad=R.REFLECT), ops, x, kind, hop)[0]
    floor = 2.0 ** round(np.log2(np.median(lin[lin > 0])))   # about half of the entries sit on the floor
    for log in (R.LN, R.LOG10):
        got, _ = _exact(eng, segs, R.fields(**GEO, pad=R.REFLECT, log=log, floor=floor), ops, x, kind, hop)
        assert (got == got.min()).sum() > 5 and (got > got.min()).sum() > 5


def test_tiles_frames_and_edges(eng):
    rng = np.random.default_rng(16)
    frame = eng.frame_samples
    x = _exact_block(rng, "i16_32768", 4096)
    # at scan hop 32, n_fft 64 and analysis hop 32 a segment of nf frames has nf + 14 analysis frames: 15, 16, 17 and 35 - one
    # short of a tile, a tile, one more, two tiles and three; the last ends ON the block's last sample; two items name the same samples
    last = (4096 - frame) // 32
    segs = [(0, 0, 1), (4, 1, 2), (1028, 3, 3), (0, 5, 21), (4, 1, 2), (0, last - 20, 21)]
    f = R.fields(64, 32, 33, 5)
    ops = R.exact_operators(rng, 64, 33, 5)
    got, start = _exact(eng, segs, f, ops, x, "i16_32768", 32)
    assert np.diff(start).tolist() == [15, 16, 17, 35, 16, 35]
    assert got[start[1]:start[2]].tobytes() == got[start[4]:start[5]].tobytes()
    got, start = _exact(eng, segs, {**f, "pad": R.REFLECT}, ops, x, "i16_32768", 32)     # the right edge inside the last tile
    assert np.diff(start).tolist() == [17, 18, 19, 37, 18, 37]
    # hop == n_fft and hop == 4
    _exact(eng, segs, R.fields(64, 64, 33, 5, pad=R.REFLECT), ops, x, "i16_32768", 32)
    small = R.exact_operators(rng, 64, 17, 20)
    got, start = _exact(eng, segs[:3], R.fields(64, 4, 17, 20), small, x, "i16_32768", 32)
    assert np.diff(start).tolist() == [113, 121, 129]
    # no frame (legal without padding, writes nothing) and one frame; reflect padding at S = n_fft / 2 + 4
    big = R.exact_operators(rng, 1024, 513, 5)
    got, start = _exact(eng, [(0, 0, 1), (0, 2, 17), (4, 0, 1)], R.fields(1024, 512, 513, 5), big, x, "i16_32768", 32)
    assert np.diff(start).tolist() == [0, 1, 0]
    mid = R.exact_operators(rng, 512, 257, 128)
    got, start = _exact(eng, [(0, 3, 1), (8, 0, 1)], R.fields(512, 512, 257, 128), mid, x, "i16_32768", 32)
    assert np.diff(start).tolist() == [1, 1]
    got, start = _exact(eng, [(0, 7, 2), (8, 0, 2)], R.fields(1024, 1024, 513, 5, pad=R.REFLECT), big, x, "i16_32768", 4)
    assert np.diff(start).tolist() == [1, 1] and eng.cut_samples(2, 4, "range") == 1024 // 2 + 4


# ---- bound cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", [(400, 160, 80), (1024, 1024, 128)], ids=["whisper", "maxima"])
def test_real_operators_within_the_derived_bound(eng, geo):
    """Whisper's geometry on a speech-like signal and the maxima on one segment of three frames; LINEAR against the bound, LOG10
    where E >= 16 bound D (tests/mel_ref.py: noise_and_tone keeps nine entries in ten inside, by the float64 reference alone).
    Prints the measured maximum of |dE| / (u D) next to numpy float32's."""
    from cutter_vad_amd.scan import MelSpec
    n_fft, mhop, n_mels = geo
    hop = 256
    segs = [(0, 0, 11)] if n_fft == 1024 else [(0, 0, 30), (1000, 2, 9), (4000, 1, 1)]
    for pad, log in (("reflect", "linear"), ("none", "linear"), ("reflect", "log10"), ("none", "log10")):
        if n_fft == 1024 and pad == "reflect" and log == "linear":
            continue                                        # (three frames: the unpadded segment)
        rng = np.random.default_rng(n_fft)
        real = np.load(GOLD + "/speech16k_i16.npz")["pcm"][16000:26000].astype(np.float32) / np.float32(32768)
        x, thr = (real, 0.01) if log == "linear" else (R.noise_and_tone(rng, 10000), None)
        spec = MelSpec(16000, n_fft=n_fft, hop=mhop, n_mels=n_mels, pad=pad, log=log)
        flds, a, b, w = spec.operators()
        f = R.fields(n_fft, mhop, n_fft // 2 + 1, n_mels, _ffi.MEL_PADS[pad], _ffi.MEL_LOGS[log], 1e-10)
        got, start = eng.mel(segs, spec, hop=hop, audio=x, denoise=thr)
        at, inside, worst, worst32 = 0, [], 0.0, 0.0
        for sg in segs:
            s0 = sg[0] + sg[1] * hop
            v = gate(x, thr)[s0:s0 + (sg[2] - 1) * hop + eng.frame_samples]
            E, D = R.energies(v, f, a, b, w)
            g = got[at:at + E.shape[0]].astype(np.float64)
            at += E.shape[0]
            if log == "linear":
                fr = R.frames(v, f)
                E32 = ((fr @ a) ** 2 + (fr @ b) ** 2) @ w.T
                ok = D > 0
                worst = max(worst, float((np.abs(g - E)[ok] / (R.U * D[ok])).max()))
                worst32 = max(worst32, float((np.abs(E32 - E)[ok] / (R.U * D[ok])).max()))
                assert (np.abs(g - E) <= R.bound(f) * D).all(), (geo, pad, worst)
            else:
                mask, diff, tol = R.log_of_bounded(g, E, D, f)
                inside.append(mask.ravel())
                assert (diff[mask] <= tol[mask]).all(), (geo, pad, log)
        assert at == got.shape[0] == start[-1] and (n_fft != 1024 or pad != "none" or at == 3)
        if log == "linear":
            print(f"scan_mel {geo} pad={pad}: max |dE| / (u D) = {worst:.3f} on the GPU, {worst32:.3f} in numpy float32, "
                  f"{R.bound(f) / R.U:.0f} allowed")
        else:
            assert np.concatenate(inside).mean() >= 0.9, (geo, pad, np.concatenate(inside).mean())


# ---- forms ------------------------------------------------------------------------------------------------------------
def test_host_form_device_form_and_two_runs(eng):
    import torch
    from cutter_vad_amd.scan import MelSpec
    rng = np.random.default_rng(5)
    x = R.speechlike(rng, 20000).reshape(-1, 2)
    segs = [(0, 3, 9, 0), (1028, 0, 20, "mix"), (1028, 1, 1, 1), (0, 0, 30, 1)]
    spec = MelSpec(16000)
    want, start = eng.mel(segs, spec, hop=260, audio=x)
    again, _ = eng.mel(segs, spec, hop=260, audio=x)
    assert want.tobytes() == again.tobytes() and np.isfinite(want).all() and want.shape == (int(start[-1]), 80)
    d_audio = torch.from_numpy(x).cuda()
    d_out = torch.full((want.shape[0] + 2, 80), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert eng.mel_device(segs, spec, d_audio.data_ptr(), 10000, d_out.data_ptr(), want.shape[0] + 2, hop=260, channels=2,
                          stream=stream.cuda_stream).tolist() == start.tolist()
    stream.synchronize()
    out = d_out.cpu().numpy()
    assert out[:-2].tobytes() == want.tobytes() and (out[-2:] == -7.0).all()
    # another operator, then the first again: the cached pack is replaced and rebuilt
    other, _ = eng.mel(segs, MelSpec(16000, n_mels=128), hop=260, audio=x)
    assert other.shape == (want.shape[0], 128) and eng.mel(segs, spec, hop=260, audio=x)[0].tobytes() == want.tobytes()


def test_the_resident_block_behind_scan_segments(eng):
    from cutter_vad_amd.scan import MelSpec
    frame, hop = eng.frame_samples, 256
    rec = np.ascontiguousarray((np.load(GOLD + "/speech16k_i16.npz")["pcm"][:12 * 256 + 512 + 5].reshape(-1, 1).clip(-32767, 32767) * np.array([[1, -1]])).astype(np.int16))
    slots = eng.open_streams(1)
    spec = MelSpec(16000, n_mels=40, log="ln")
    try:
        with eng.scan_session():
            eng.scan_segments(slots, [rec], hop=hop, denoise=0.01)
            off = int(eng.last_scan["offsets"][0])
            segs = [(off, 1, 9, 0), (off, 0, 12), (off, 11, 1, 1)]
            got, start = eng.mel(segs, spec, hop=hop, denoise=0.01)
            total = eng.last_scan["samples"]
        block = np.zeros((total, 2), np.int16)
        block[off:off + rec.shape[0]] = rec
        want, wstart = eng.mel(segs, spec, hop=hop, denoise=0.01, audio=block)
        assert got.tobytes() == want.tobytes() and start.tolist() == wstart.tolist() and np.diff(start).tolist() == [17, 21, 4]
        y = np.log(float(np.float32(1e-10)))                                                # L - L: the mix is silence, on the floor
        assert (np.abs(got[start[1]:start[2]] - y) <= R.log_tolerance(y)).all()
    finally:
        for s in slots:
            eng.close_stream(int(s))


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_features_recordings_against_the_cut_and_the_reference(eng):
    from cutter_vad_amd import VADConfig, cut_recordings, features_recordings
    from cutter_vad_amd.scan import MelSpec
    pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"].astype(np.float32) / np.float32(32767.0)
    delayed = np.concatenate([np.zeros(3 * 16000, np.float32), pcm[:-3 * 16000]])
    recs = [pcm[:pcm.size // 2], np.zeros(20000, np.float32), np.ascontiguousarray(np.stack([pcm * np.float32(0.5), delayed], axis=1))]
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    spec = MelSpec(16000, log="linear")
    flds, a, b, w = spec.operators()
    f = R.fields(400, 160, 201, 80, R.REFLECT, R.LINEAR)
    n = 0
    for channel in ("mix", "split"):
        got = features_recordings(recs, spec, cfg, engine=eng, channel=channel, open_end=True)
        # the f32 payload of the same segments, through the existing cut
        cuts = cut_recordings(recs, cfg, engine=eng, channel=channel, layout="range", wav=False, open_end=True)
        for x, rg, rc in zip(recs, got, cuts):
            per = list(zip(rg, rc)) if channel == "split" else [(rg, rc)]
            for c, (g_, c_) in enumerate(per):
                assert [r[:2] for r in g_] == [r[:2] for r in c_]
                ch = () if x.ndim == 1 else ("mix" if channel == "mix" else c,)
                for s0, s1, feat in g_:
                    data, _ = eng.cut([(0, s0 // 256, (s1 - s0 - 512) // 256 + 1) + ch], hop=256, layout="range", out="f32", audio=x, denoise=0.01)
                    assert data.size == s1 - s0
                    E, D = R.energies(data, f, a, b, w)
                    assert feat.shape == E.shape and (np.abs(feat - E) <= R.bound(f) * D).all()
                    n += 1
        assert got[1] == ([[]] if channel == "split" else [])
    assert n >= 4
