"""vad_scan_resample_cut and vad_scan_rate_mel on the GPU (csrc/scan_resample_cut.hip: vadk_resample_cut).  Layout is tested byte
for byte: on samples |s| <= 8 of 32768 and integer taps in -2 .. 2 every float32 operation is exact in any order of summation
(tests/resample_cut_ref.py asserts that precondition on its own int64 evaluation before anything is compared), so a wrong sample,
tap, phase, row-block or quad is a wrong byte.  Numerics on real taps are held to the derived bound |y - y_f64| <= (ceil(N / L) + 4)
u D.  W = VAD_RESAMPLE_CUT_WG_SAMPLES outputs per workgroup: segments of W - 4, W, W + 4 and 2 W + 4 samples surround its edges."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import mel_ref as MR
from tests import resample_cut_ref as R
from tests.cut_ref import F32, FMT, MIX, PCM16, SENT16, SENT32, heard, untouched
from tests.test_gpu_scan import GOLD, _engine
from tests.test_scan_resample_cut_host import CHUNK, GEO, exact_block, exact_taps, rsc

pytestmark = pytest.mark.gpu
W = _ffi.VAD_RESAMPLE_CUT_WG_SAMPLES
KINDS = ("f32", "i16_32768", "ulaw", "alaw")


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


def _want(block, kind, item, taps, sr, hop, of, gain=None):
    off, first, nf, _, ch = item
    x = heard(block, kind, ch)[off + first * hop:off + first * hop + R.s_in(nf, sr, hop)]
    y = R.gained(R.assert_exact(x, taps, sr), gain)
    return y if of == F32 else R.pcm16(y)


# ---- exact cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_formats_channels_taps_outputs_and_gains_byte_for_byte(eng, sr, kind):
    """mono, and left, right and mix of a two-channel block; 1, 3 and 31 taps; float32 and PCM16; gains of +-2^k, two of which
    saturate PCM16 at either end; a segment on the block's first sample, one on its last, one chunk, the whole block, and two items
    naming the same samples; the gaps of `out` keep their sentinel"""
    rng = np.random.default_rng(sr + len(kind))
    chunk = CHUNK[sr]
    hop = chunk // 2
    for two in (False, True):
        block = exact_block(rng, kind, (12 * chunk, 2) if two else 12 * chunk)
        for ntaps in (1, 3, 31):
            taps = exact_taps(rng, ntaps)
            taps[0] = taps[-1] = 2
            items, at = [], 0
            for off, first, nf, ch in ((0, 0, 3, 0), (4 * chunk, 2, 13, 1 if two else 0), (0, 0, 1, MIX if two else 0),
                                       (4 * chunk, 2, 13, MIX if two else 0), (11 * chunk, 0, 1, 0), (0, 0, 23, 0), (0, 0, 3, 0)):
                items.append((off, first, nf, at, ch))
                at += R.s16(R.s_in(nf, sr, hop), sr) + 8
            gains = [1.0, -2.0, 0.5, 4.0, -0.25, 2.0 ** 16, -2.0 ** 16]
            for of in (F32, PCM16):
                for g in (None, gains):
                    rc, msg, out = rsc(eng._lib, eng, items, taps, block, 2 if two else 1, FMT[kind], sr, hop, of, at, gains=g)
                    assert rc == _ffi.VAD_OK, msg
                    for i, it in enumerate(items):
                        want = _want(block, kind, it, taps, sr, hop, of, None if g is None else g[i])
                        o = it[3]
                        assert out[o:o + want.size].tobytes() == want.tobytes(), (two, ntaps, of, i, np.flatnonzero(out[o:o + want.size] != want)[:8])
                        assert untouched(out[o + want.size:o + want.size + 8])
                    if g is not None and of == PCM16 and ntaps > 1:
                        sat = out[items[5][3]:items[6][3] - 8]
                        assert (sat == 32767).any() and (sat == -32768).any()
            a, b = items[0][3], items[6][3]
            n = R.s16(R.s_in(3, sr, hop), sr)
            assert out[a:a + n].tobytes() != out[b:b + n].tobytes() and untouched(out[at:])     # (the same samples, gains 1 and -2^16)


@pytest.mark.parametrize("sr", R.RATES)
def test_workgroup_edges_odd_hops_and_loud_neighbours(eng, sr):
    """S16 around one and two workgroups; a hop for which S_in L / M is no integer; every segment lies between LOUD samples of the
    block that the rule never reads: the reference zero-extends, a kernel that reads its neighbours fails here"""
    rng = np.random.default_rng(sr + 7)
    chunk = CHUNK[sr]
    L, M = R.ratio(sr)
    hop = 4
    taps = exact_taps(rng, 31)
    taps[0] = taps[-1] = 2
    # at 8 kHz S16 = 2 S_in is a multiple of 8: the counts next to W that exist there
    wants = (W - 8, W, W + 8, 2 * W + 8) if sr == 8000 else (W - 4, W, W + 4, 2 * W + 4)
    seen = 0
    for want in wants:
        nf = next(k for k in range(1, 1 << 16) if R.s16(R.s_in(k + 1, sr, hop), sr) > want)      # the longest segment with this count
        S = R.s_in(nf, sr, hop)
        assert R.s16(S, sr) == want, (sr, want)
        seen += (S * L) % M != 0
        block = np.full(S + 2 * chunk, 8192, np.int16)
        block[1::2] = -8192
        block[chunk:chunk + S] = exact_block(rng, "i16_32768", S)
        rc, msg, out = rsc(eng._lib, eng, [(chunk, 0, nf, 8, 0)], taps, block, 1, FMT["i16_32768"], sr, hop, F32, want + 16)
        y = R.assert_exact(block[chunk:chunk + S].astype(np.float32) / np.float32(32768.0), taps, sr)
        assert rc == _ffi.VAD_OK and y.size == want, msg
        assert out[8:8 + want].tobytes() == y.tobytes(), (sr, want, np.flatnonzero(out[8:8 + want] != y)[:8])
        assert untouched(out[:8]) and untouched(out[8 + want:])
    assert sr == 8000 or seen > 0


# ---- real taps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", R.RATES)
def test_real_taps_within_the_derived_bound(eng, sr):
    """resample_taps' defaults and a 511-tap design on full-scale int16 noise plus a tone, as float32: every sample within
    (ceil(N / L) + 4) u D of float64.  Prints the measured maximum of |dy| / (u D) next to numpy float32's (ascending k)."""
    from cutter_vad_amd.scan import resample_taps
    rng = np.random.default_rng(sr)
    chunk = CHUNK[sr]
    hop = chunk // 2
    L, M = R.ratio(sr)
    n = 12 * chunk
    tone = np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)
    block = np.clip(rng.integers(-32768, 32768, n) * 0.5 + 16000 * tone, -32768, 32767).astype(np.int16)
    x = block.astype(np.float32) / np.float32(32767.0)
    segs = [(0, 0, 23), (chunk, 1, 9)]
    long = resample_taps(sr, half_width=255 // max(L, M))
    long = np.pad(long, (511 - long.size) // 2)             # (8 kHz: 4 * 127 + 1 = 509 taps, and a zero at either end)
    for taps in (resample_taps(sr), long):
        assert taps.size in (65, 97, 511)
        data, start = eng.resample_cut(segs, sr, taps, hop=hop, out="f32", audio=block)
        worst = mine = 0.0
        for i, (off, first, nf) in enumerate(segs):
            xs = x[off + first * hop:off + first * hop + R.s_in(nf, sr, hop)]
            y, D = R.evaluate(xs, taps, sr)
            got = data[start[i]:start[i + 1]].astype(np.float64)
            assert got.size == y.size and (D > 0).all()
            worst = max(worst, float((np.abs(got - y) / (R.U * D)).max()))
            mine = max(mine, float((np.abs(R.evaluate_f32(xs, taps, sr).astype(np.float64) - y) / (R.U * D)).max()))
            assert (np.abs(got - y) <= R.bound(taps.size, sr) * D).all(), (sr, taps.size, worst)
        print(f"resample_cut {sr} Hz, {taps.size} taps: max |dy| / (u D) = {worst:.2f} on the GPU, {mine:.2f} in numpy float32, "
              f"{R.bound(taps.size, sr) / R.U:.0f} allowed")


# ---- forms ------------------------------------------------------------------------------------------------------------
def test_host_form_device_form_and_two_runs(eng):
    import torch
    from cutter_vad_amd.scan import resample_taps
    rng = np.random.default_rng(5)
    sr, hop = 48000, 768
    x = MR.speechlike(rng, 40000).reshape(-1, 2)
    segs = [(0, 3, 9, 0), (1028, 0, 20, "mix"), (1028, 1, 1, 1), (0, 0, 24, 1)]
    gains = [0.5, 1.0, -1.0, 2.0]
    for of in ("f32", "pcm16"):
        want, start = eng.resample_cut(segs, sr, hop=hop, out=of, audio=x, gains=gains)
        again, _ = eng.resample_cut(segs, sr, hop=hop, out=of, audio=x, gains=gains)
        assert want.tobytes() == again.tobytes() and want.size == int(start[-1]) and np.abs(want.astype(np.float64)).max() > 0
        d_audio = torch.from_numpy(x).cuda()
        d_out = torch.from_numpy(np.full(want.size + 8, SENT32 if of == "f32" else SENT16, want.dtype)).cuda()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert eng.resample_cut_device(segs, sr, d_audio.data_ptr(), 20000, d_out.data_ptr(), want.size + 8, hop=hop, channels=2, out=of,
                                       stream=stream.cuda_stream, gains=gains).tolist() == start.tolist()
        stream.synchronize()
        out = d_out.cpu().numpy()
        assert out[:-8].tobytes() == want.tobytes() and untouched(out[-8:])
    # other taps, then the first again: the cached pack is replaced and rebuilt
    other, _ = eng.resample_cut(segs, sr, resample_taps(sr, half_width=8), hop=hop, out="pcm16", audio=x, gains=gains)
    assert other.tobytes() != want.tobytes()
    assert eng.resample_cut(segs, sr, hop=hop, out="pcm16", audio=x, gains=gains)[0].tobytes() == want.tobytes()


def _speech_at(sr, n16):
    """the golden clip's first n16 samples at `sr`: repeated, or decimated"""
    pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"][:n16]
    return np.ascontiguousarray(pcm[(np.arange(n16 * sr // 16000) * 16000) // sr].clip(-32767, 32767).astype(np.int16))


def test_the_resident_rate_block_behind_scan_segments(eng):
    sr, chunk = 24000, 768
    hop = chunk // 2
    rec = _speech_at(sr, 8 * 512 + 100)
    slots = eng.open_streams(1)
    try:
        with eng.scan_session():
            eng.scan_segments(slots, [rec], hop=hop, denoise=0.01, sample_rate=sr)
            off = int(eng.last_scan["offsets"][0])
            segs = [(off, 1, 9), (off, 0, 12), (off, 11, 1)]
            got, start = eng.resample_cut(segs, sr, hop=hop, out="f32")
            total = eng.last_scan["samples"]
        block = np.zeros(total, np.int16)
        block[off:off + rec.size] = rec
        want, wstart = eng.resample_cut(segs, sr, hop=hop, out="f32", audio=block)
        assert got.tobytes() == want.tobytes() and start.tolist() == wstart.tolist() and np.diff(start).tolist() == [2560, 3328, 512]
        assert np.abs(got).max() > 0
    finally:
        for s in slots:
            eng.close_stream(int(s))


# ---- vad_scan_rate_mel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["exact", "whisper"])
def test_rate_mel_is_resample_cut_then_mel_byte_for_byte(eng, geo):
    """the header's recipe run by hand: Engine.resample_cut(f32) into one array, Engine.mel on it as a mono block at 16 kHz with the
    items (o_i, 0, (S16 - 512) / 4 + 1), hop = 4, gate off"""
    from cutter_vad_amd.scan import MelSpec, resample_taps
    rng = np.random.default_rng(len(geo))
    rates = R.RATES if geo == "exact" else (48000,)
    for sr in rates:
        chunk = CHUNK[sr]
        hop = chunk // 2
        if geo == "exact":
            block = exact_block(rng, "i16_32768", (10 * chunk, 2))
            taps = exact_taps(rng, 31)
            specs = [(MR.fields(**GEO, pad=pad), *MR.exact_operators(rng, 64, 33, 5)) for pad in (MR.REFLECT, MR.NONE)]
        else:
            block = (MR.speechlike(rng, 20 * chunk).reshape(-1, 2) * 20000).astype(np.int16)
            taps = resample_taps(sr)
            specs = [MelSpec(16000)]
        segs = [(0, 0, 3, 0), (4 * chunk, 1, 7, "mix"), (0, 0, 3, 0), (9 * chunk, 0, 1, 1)]
        mid, start = eng.resample_cut(segs, sr, taps, hop=hop, out="f32", audio=block, i16_scale=32768)
        second = [(int(start[i]), 0, (int(start[i + 1] - start[i]) - 512) // 4 + 1) for i in range(len(segs))]
        for spec in specs:
            want, wstart = eng.mel(second, spec, hop=4, denoise=None, audio=mid)
            got, gstart = eng.mel(segs, spec, hop=hop, audio=block, i16_scale=32768, sample_rate=sr, taps=taps)
            assert got.tobytes() == want.tobytes() and gstart.tolist() == wstart.tolist() and got.shape[0] > 0 and np.isfinite(got).all()
            assert got[gstart[0]:gstart[1]].tobytes() == got[gstart[2]:gstart[3]].tobytes()
            if geo == "exact":
                f, ops = spec[0], spec[1:]
                rows, _ = MR.rows_of([mid[start[i]:start[i + 1]] for i in range(len(segs))], f, *ops, exact=True)
                assert got.tobytes() == rows.astype(np.float32).tobytes()


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_cut_recordings_and_features_recordings_against_the_cut_and_the_reference(eng):
    from cutter_vad_amd import VADConfig, cut_recordings, features_recordings, resample_taps
    from cutter_vad_amd.scan import MelSpec
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    n16 = 6 * 16000
    n = 0
    # cut_recordings at 48 kHz: the 16 kHz PCM of Engine.cut's input-rate samples through the rule
    sr = 48000
    chunk, hop = CHUNK[sr], CHUNK[sr] // 2
    speech = _speech_at(sr, n16)
    recs = [speech, np.zeros(3 * chunk, np.int16), np.ascontiguousarray(np.stack([speech // 2, np.zeros_like(speech)], axis=1))]
    taps = resample_taps(sr)
    got = cut_recordings(recs, cfg, engine=eng, channel=0, layout="range", wav=False, sample_rate=sr, resample=True, open_end=True)
    plain = cut_recordings(recs, cfg, engine=eng, channel=0, layout="range", wav=False, sample_rate=sr, open_end=True)
    assert [[r[:2] for r in rc] for rc in got] == [[r[:2] for r in rc] for rc in plain] and got[1] == []
    for x, rc in zip(recs, got):
        for s0, s1, pcm in rc:
            data, _ = eng.cut([(0, s0 // hop, (s1 - s0 - chunk) // hop + 1) + (() if x.ndim == 1 else (0,))], hop=hop, layout="range", out="f32",
                              audio=x, sample_rate=sr)
            assert data.size == s1 - s0
            y, D = R.evaluate(data, taps, sr)
            assert pcm.dtype == np.int16 and pcm.size == R.s16(s1 - s0, sr) and np.abs(pcm).max() > 100
            # the rule's bound, then one float32 multiply (1 ulp of a value below 2^15) and the truncation toward zero
            assert (np.abs(pcm - np.clip(y * 32767, -32768, 32767)) <= 1.0 + 32767 * R.bound(taps.size, sr) * D + 2.0 ** -8).all()
            n += 1
    # features_recordings at 8 kHz
    sr = 8000
    chunk, hop = CHUNK[sr], CHUNK[sr] // 2
    speech = _speech_at(sr, n16)
    recs = [speech, np.zeros(3 * chunk, np.int16)]
    taps = resample_taps(sr)
    spec = MelSpec(16000, log="linear")
    flds, a, b, w = spec.operators()
    f = MR.fields(400, 160, 201, 80, MR.REFLECT, MR.LINEAR)
    feats = features_recordings(recs, spec, cfg, engine=eng, sample_rate=sr, open_end=True)
    assert feats[1] == []
    for s0, s1, feat in feats[0]:
        data, _ = eng.cut([(0, s0 // hop, (s1 - s0 - chunk) // hop + 1)], hop=hop, layout="range", out="f32", audio=recs[0], sample_rate=sr)
        y, Dy = R.evaluate(data, taps, sr)
        # the 16 kHz signal the kernel made, from the GPU itself: the mel bound holds on ITS float32 values
        y32, _ = eng.resample_cut([(0, s0 // hop, (s1 - s0 - chunk) // hop + 1)], sr, taps, hop=hop, out="f32", audio=recs[0])
        assert (np.abs(y32 - y) <= R.bound(taps.size, sr) * Dy).all()
        E, D = MR.energies(y32, f, a, b, w)
        assert feat.shape == E.shape and (np.abs(feat - E) <= MR.bound(f) * D).all()
        n += 1
    assert n >= 3
