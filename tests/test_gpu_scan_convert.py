"""vad_convert, vad_convert_device and vad_scan_convert_segments on the GPU (csrc/scan_convert.hip: vadk_convert).  Layout is tested
byte for byte: on small integer samples and small integer taps every float32 operation is exact in any order of summation
(tests/convert_ref.py asserts that precondition on its own int64 evaluation before anything is compared), so a wrong sample, tap,
row-tile, period, column group or quad is a wrong byte.  Numerics on real taps are held to the derived bound |y - y_f64| <=
(ceil(N / L) + 4) u D.  Lengths surround one period and one workgroup's run of periods."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import convert_ref as CR
from tests.cut_ref import F32, FMT, MIX, RANGE, SENT32, raw_cut, untouched
from tests.test_gpu_scan import GOLD, THR, _engine
from tests.test_scan_convert_host import RATES, _check, conv, exact_taps, scan_conv, scan_segs, want_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


# ---- exact cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_rates_tap_counts_and_lengths_byte_for_byte(eng, sr):
    """N = 1, 3, 2 L + 1 (and the largest accepted, at 44.1 kHz); S_in around one period's inputs, around one workgroup's run and two
    runs plus 5; the first item starts on the block's first sample, the last ends on its last, and every gap between two items is
    LOUD: the rule zero-extends an item, a kernel that reads a neighbour fails the equality"""
    rng = np.random.default_rng(sr)
    L, M = CR.ratio(sr)
    PI = CR.period_inputs(sr)
    counts = [1, 3, 2 * L + 1] + ([CR.MAX_REACH * L - 1] if sr == 44100 else [])
    for N in counts:
        taps = exact_taps(rng, N)
        span = CR.run_periods(N, sr) * PI
        assert span >= PI
        lens = [1, 3, PI - 1, PI, PI + 1, span - 1, span, span + 1, 2 * span + 5]
        offs, at = [], 0
        for n in lens:
            offs.append(at)
            at = (at + n + 3 + 8) & ~3                      # a gap of 8 .. 11 loud samples
        total = offs[-1] + lens[-1]
        block = np.where(np.arange(total) % 2 == 0, 16384, -16384).astype(np.int16)
        for o, n in zip(offs, lens):
            block[o:o + n] = rng.integers(-64, 65, n)
        items = [(0, o, n, 0) for o, n in zip(offs, lens)]
        want_off = CR.layout(lens, sr)
        rc, msg, out, off = conv(eng._lib, eng, items, taps, block, 1, FMT["i16_32768"], sr, int(want_off[-1]))
        assert rc == _ffi.VAD_OK and off.tolist() == want_off.tolist(), msg
        _check(out, off, block, "i16_32768", items, lens, taps, sr)


@pytest.mark.parametrize("kind", ["f32", "i16_32768", "ulaw", "alaw"])
def test_formats_channels_and_the_mix(eng, kind):
    """the four wire formats, mono and both channels and the mix of a two-channel block, at 44.1 and 12 kHz; G.711 takes every code,
    with taps in -1 .. 2"""
    rng = np.random.default_rng(len(kind))
    for sr in (44100, 12000):
        L, M = CR.ratio(sr)
        PI = CR.period_inputs(sr)
        g711 = kind in ("ulaw", "alaw")
        taps = exact_taps(rng, 3, lo=-1) if g711 else exact_taps(rng, 2 * L + 1)
        span = CR.run_periods(taps.size, sr) * PI
        lens = [3, PI + 1, span + 1, 2 * PI + 2, 1027]
        for two in (False, True):
            offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
            shape = (int(offs[-2]) + lens[-1], 2) if two else int(offs[-2]) + lens[-1]
            if kind == "f32":
                block = rng.integers(-64, 65, shape).astype(np.float32)
            elif kind == "i16_32768":
                block = rng.integers(-64, 65, shape).astype(np.int16)
            else:
                block = rng.integers(0, 256, shape).astype(np.uint8)
            chans = [0] * len(lens) if not two else [0, 1, MIX, 1, MIX]
            items = [(0, int(offs[i]), lens[i], chans[i]) for i in range(len(lens))]
            rc, msg, out, off = conv(eng._lib, eng, items, taps, block, 2 if two else 1, FMT[kind], sr, int(CR.layout(lens, sr)[-1]))
            assert rc == _ffi.VAD_OK and off.tolist() == CR.layout(lens, sr).tolist(), msg
            _check(out, off, block, kind, items, lens, taps, sr)


# ---- real taps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [44100, 22050])
def test_real_taps_within_the_derived_bound(eng, sr):
    """convert_taps' default design on Gaussian noise: every sample within (ceil(N / L) + 4) u D of float64.  Prints the measured
    maximum of |dy| / (u D)."""
    from cutter_vad_amd.scan import convert_taps
    rng = np.random.default_rng(sr)
    L, M = CR.ratio(sr)
    h = convert_taps(sr)
    x = (0.3 * rng.standard_normal(3 * CR.period_inputs(sr) * 16 + 77)).astype(np.float32)
    data, start = eng.convert([x], sr, taps=h)
    y, D = CR.convert_f64(x, h, sr), CR.convert_f64(x, h, sr, absolute=True)
    got = data[:y.size].astype(np.float64)
    assert start.tolist() == [0, (y.size + 3) & ~3] and (D > 0).all()
    worst = float((np.abs(got - y) / (CR.U * D)).max())
    print(f"convert {sr} Hz, {h.size} taps: max |dy| / (u D) = {worst:.2f} on the GPU, {CR.bound(h.size, L)} allowed")
    assert (np.abs(got - y) <= CR.bound(h.size, L) * CR.U * D).all(), (sr, worst)


# ---- forms ------------------------------------------------------------------------------------------------------------
def test_two_runs_and_the_device_form_give_the_same_bytes(eng):
    import torch
    rng = np.random.default_rng(11)
    sr = 44100
    recs = [np.ascontiguousarray((8000 * rng.standard_normal((n, 2))).astype(np.int16)) for n in (20011, 3, 7056, 30001)]
    want, start = eng.convert(recs, sr, channel=["mix", 0, 1, "mix"])
    again, _ = eng.convert(recs, sr, channel=["mix", 0, 1, "mix"])
    assert want.tobytes() == again.tobytes() and want.size == start[-1] and np.abs(want).max() > 0.1
    offs = np.concatenate([[0], np.cumsum([(r.shape[0] + 3) & ~3 for r in recs])])
    block = np.zeros((int(offs[-1]), 2), np.int16)
    for o, r in zip(offs, recs):
        block[o:o + r.shape[0]] = r
    d_audio = torch.from_numpy(block).cuda()
    d_out = torch.from_numpy(np.full(want.size + 8, SENT32, np.float32)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = eng.convert_device(offs[:-1], [r.shape[0] for r in recs], sr, d_audio.data_ptr(), block.shape[0], d_out.data_ptr(), want.size + 8,
                            fmt=_ffi.VAD_FMT_I16_32767, channels=2, channel=["mix", 0, 1, "mix"], stream=stream.cuda_stream)
    stream.synchronize()
    out = d_out.cpu().numpy()
    assert st.tolist() == start.tolist() and out[:-8].tobytes() == want.tobytes() and untouched(out[-8:])
    # other taps, then the default again: the cached operators are replaced and rebuilt
    from cutter_vad_amd.scan import convert_taps
    other, _ = eng.convert(recs, sr, taps=convert_taps(sr, half_width=8), channel=["mix", 0, 1, "mix"])
    assert other.tobytes() != want.tobytes()
    assert eng.convert(recs, sr, channel=["mix", 0, 1, "mix"])[0].tobytes() == want.tobytes()


def test_one_nan_sample_poisons_its_tap_window_and_nothing_beyond_the_reach(eng):
    from cutter_vad_amd.scan import convert_taps
    rng = np.random.default_rng(12)
    for sr in (44100, 48000):
        L, M = CR.ratio(sr)
        h = convert_taps(sr, half_width=8)
        N, C = h.size, (h.size - 1) // 2
        K = CR.reach(N, sr)
        x = (0.3 * rng.standard_normal(40000)).astype(np.float32)
        for k in (0, 17001, x.size - 1):
            bad, zero = x.copy(), x.copy()
            bad[k], zero[k] = np.nan, 0.0
            got, _ = eng.convert([bad], sr, taps=h)
            ref, _ = eng.convert([zero], sr, taps=h)
            S_out = CR.samples(x.size, sr)
            m = np.arange(S_out)
            t = m * M - k * L + C
            inside = (t >= 0) & (t < N)                                  # the output's tap window holds the sample
            beyond = np.abs(k - m * M / L) >= K                          # the documented reach
            assert inside.any() and not (inside & beyond).any() and beyond.sum() > S_out // 2
            assert not np.isfinite(got[:S_out][inside]).any(), (sr, k)
            assert got[:S_out][beyond].tobytes() == ref[:S_out][beyond].tobytes(), (sr, k)
            assert np.isfinite(ref).all()


# ---- the definitional equality ----------------------------------------------------------------------------------------
def _recordings_44k():
    """three recordings of about 1 s at 44.1 kHz: the golden clip's speech stretched by index (bursts of speech, a silent second half
    in the first), and harmonic bursts from tests/signals.py"""
    from tests.signals import make_streams
    pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"]
    loud = int(np.argmax(np.convolve(np.abs(pcm.astype(np.float64)), np.ones(8000), "valid")))
    at = lambda n16, first: pcm[min(first, pcm.size - n16 - 1) + (np.arange(n16 * 441 // 160) * 160) // 441]
    a = at(16000, loud).copy()
    a[a.size // 2:] = 0
    b = at(18000, max(loud - 4000, 0)).copy()
    tone = make_streams(2, 40, seed=77)[1].reshape(-1)[:16000]
    c = (tone[(np.arange(44100) * 160) // 441] * 30000 * ((np.arange(44100) // 11025) % 2 == 0)).astype(np.int16)
    return [np.ascontiguousarray(a.astype(np.int16)), np.ascontiguousarray(b.astype(np.int16)), c]


def test_scan_convert_segments_is_convert_then_scan_segments(eng):
    from cutter_vad_amd.scan import MelSpec, convert_taps
    sr, hop = 44100, 256
    recs = _recordings_44k()
    lens = [r.size for r in recs]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
    block = np.zeros(int(offs[-1]), np.int16)
    for o, r in zip(offs, recs):
        block[o:o + r.size] = r
    h = convert_taps(sr)
    twin = _engine(16000)
    try:
        sa, sb = eng.open_streams(3), twin.open_streams(3)
        eng.set_thresholds_many(sa, THR)
        twin.set_thresholds_many(sb, THR)
        items = [(int(sa[i]), int(offs[i]), lens[i], 0) for i in range(3)]
        rc, msg, table, count, off = scan_conv(eng._lib, eng, items, h, block, 1, FMT["i16_32767"], sr, hop, thr=0.01)
        assert rc == _ffi.VAD_OK and count >= 1, (msg, count)
        total = int(CR.layout(lens, sr)[-1])
        rc, msg, out, off2 = conv(twin._lib, twin, items, h, block, 1, FMT["i16_32767"], sr, total)
        assert rc == _ffi.VAD_OK and off.tolist() == off2.tolist() == CR.layout(lens, sr).tolist(), msg
        y = out[:total]
        second = [(int(sb[i]), int(off[i]), CR.samples(lens[i], sr), 0) for i in range(3)]
        rc, msg, table2, count2 = scan_segs(twin._lib, twin, second, y, hop, thr=0.01)
        assert rc == _ffi.VAD_OK and count2 == count and table[:count].tobytes() == table2[:count].tobytes(), (msg, count, count2)
        # the resident block: a cut and the mel features of audio = NULL against the same calls given the converted bytes
        segs = [(int(off[int(t["item"])]), max(int(t["first_frame"]), 0), int(t["nframes"]) - max(-int(t["first_frame"]), 0)) for t in table[:count]]
        segs += [(int(off[1]), 2, 5), (int(off[2]), 0, 1)]
        places = np.concatenate([[0], np.cumsum([(nf - 1) * hop + 512 for _, _, nf in segs])])
        cuts = [sg + (int(places[i]), 0) for i, sg in enumerate(segs)]
        cap = int(places[-1])
        ra = raw_cut(eng._lib, eng, cuts, None, 1, FMT["f32"], hop, RANGE, F32, cap, thr=0.01, audio_samples=total)
        rb = raw_cut(twin._lib, twin, cuts, y, 1, FMT["f32"], hop, RANGE, F32, cap, thr=0.01)
        assert ra[0] == rb[0] == _ffi.VAD_OK and ra[2].tobytes() == rb[2].tobytes(), (ra[1], rb[1])
        assert np.abs(ra[2][:cap]).max() > 0.01 and untouched(ra[2][cap:])
        eng._scan_last = {"samples": total, "channels": 1, "fmt": _ffi.VAD_FMT_F32, "offsets": off[:-1], "lengths": None}
        spec = MelSpec(16000)
        ma, sta = eng.mel(segs, spec, hop=hop, audio=None)
        mb, stb = twin.mel(segs, spec, hop=hop, audio=y)
        assert ma.tobytes() == mb.tobytes() and sta.tolist() == stb.tolist() and ma.shape[0] > 0 and np.isfinite(ma).all()
        # the resident per-frame results: resegment and the tails run behind it, and agree
        eng._tail_items = twin._tail_items = 3
        sets = [THR, (0.5, 0.35, 0.8, 0.95, 3, 3)]
        ga, gb = eng.resegment(sets), twin.resegment(sets)
        assert [t.tobytes() for t in ga] == [t.tobytes() for t in gb] and ga[0].tobytes() == table[:count].tobytes()
        assert eng.scan_tails().tobytes() == twin.scan_tails().tobytes()
        # Engine.scan_segments(convert=...) is the same call
        for e, s in ((eng, sa), (twin, sb)):
            e.reset(s)
        t1 = eng.scan_segments(sa, recs, hop=hop, sample_rate=sr, convert=True)
        assert t1.tobytes() == table[:count].tobytes() and eng.last_scan["offsets"].tolist() == off[:-1].tolist()
    finally:
        twin.close()
        for s in sa:
            eng.close_stream(int(s))


def test_scan_recordings_convert_is_scan_recordings_of_the_converted_arrays(eng):
    from cutter_vad_amd import VADConfig, scan_recordings
    sr = 44100
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=3, voice_end_frame_count=6)
    recs = _recordings_44k()
    got = scan_recordings(recs, cfg, engine=eng, sample_rate=sr, convert=True, open_end=True, stats=True)
    data, start = eng.convert(recs, sr)
    pieces = [data[start[i]:start[i] + eng.convert_samples(recs[i].size, sr)] for i in range(3)]
    assert got == scan_recordings(pieces, cfg, engine=eng, open_end=True, stats=True)
    assert sum(len(rc) for rc in got) >= 1 and all(b <= p.size for rc, p in zip(got, pieces) for _, b, *_ in rc)
