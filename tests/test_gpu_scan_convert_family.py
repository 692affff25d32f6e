"""vadk_convert (csrc/scan_convert.hip) at every rate its argument check accepts.  tests/test_gpu_scan_convert.py runs the kernel at
eight rates in six classes of L; everything in it that depends on the ratio - the period and its inputs, the number of row-tiles,
cv_base, the LDS skew, cv_nper's run and the clamped columns of a run shorter than a column group, the operator pack - is run here
at all 3 440 accepted rates of a 16 kHz engine (one period plus one input each) and in depth at the covering set of
tests/convert_cases.py, whose census is asserted on the reference alone before the engine is touched.  Layout is byte equality with
the int64 reference (tests/convert_ref.py asserts on its own evaluation that float32 is exact in any order); numerics on the
engine's default taps are held to the derived bound (ceil(N / L) + 4) u D.  The bodies are the ones tests/test_scan_convert_host.py
runs on the stand-in."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import convert_cases as CC
from tests import convert_ref as CR
from tests.cut_ref import FMT, MIX
from tests.test_gpu_scan import GOLD, THR, _engine
from tests.test_gpu_scan_convert import _check, conv, scan_conv, scan_segs
from tests.test_scan_convert_host import cache_body, depth_body, engine_8k_body, every_rate_body, exact_taps

pytestmark = pytest.mark.gpu

REAL = (4000, 4500, 5120, 13600, 4025, 15975, 38640, 161920, 186800, 191680, 192000)


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


# ---- exact cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", CC.CLASSES)
def test_every_accepted_rate_of_a_class_byte_for_byte(eng, L):
    c = CC.cover_census()
    rates = CC.family()[L]
    assert c["family_size"] == 3440 and L in c["family_classes"] and rates and all(CR.ratio(sr)[0] == L for sr in rates)
    every_rate_body(eng._lib, eng, rates)


@pytest.mark.parametrize("sr", CC.COVER)
def test_the_covering_set_in_depth(eng, sr):
    """N = 1, 3, 2 L + 1 and 128 L - 1; S_in = 1, 3, around one period's inputs, around one workgroup's run and two runs plus 5; the
    first item on the block's first sample, the last on its last, every gap LOUD"""
    CC.cover_census()
    depth_body(eng._lib, eng, sr)


@pytest.mark.parametrize("kind", ["f32", "i16_32768", "ulaw", "alaw"])
@pytest.mark.parametrize("sr", [4500, 13600, 161920])
def test_formats_channels_and_the_partial_end_quad(eng, sr, kind):
    """PI = 9, skew 0 on 5 row-tiles, and runs of 3 periods: the four wire formats, mono and channel 0, channel 1 and the mix of a
    two-channel block, with S_in mod 4 = 1, 2 and 3 in each, so that the byte-wise end quad runs at every frame width from 1 to 8
    bytes with one, two and three frames in it; G.711 takes every code, with taps in -1 .. 2"""
    c = CC.census([sr])
    CC.hold(c, {4500: "pi_not_mult4", 13600: "skew0", 161920: "run_le3"}[sr])
    assert sr != 13600 or c["tiles"] == {5}
    rng = np.random.default_rng(sr + len(kind))
    L, M = CR.ratio(sr)
    PI = CR.period_inputs(sr)
    g711 = kind in ("ulaw", "alaw")
    taps = exact_taps(rng, 3, lo=-1) if g711 else exact_taps(rng, 2 * L + 1)
    span = CR.run_periods(taps.size, sr) * PI
    lens = [5, PI + 1 + (-(PI + 1) % 4 + 2) % 4, span + (-span % 4 + 3) % 4, 2 * PI + (-2 * PI % 4 + 1) % 4, 1027]
    assert [n % 4 for n in lens] == [1, 2, 3, 1, 3]
    for two in (False, True):
        for chans in ([0] * 5,) if not two else ([0, 1, MIX, 1, MIX], [MIX, 0, 1, MIX, 0], [1, MIX, 0, 0, 1]):
            offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
            shape = (int(offs[-2]) + lens[-1], 2) if two else int(offs[-2]) + lens[-1]
            if kind == "f32":
                block = rng.integers(-64, 65, shape).astype(np.float32)
            elif kind == "i16_32768":
                block = rng.integers(-64, 65, shape).astype(np.int16)
            else:
                block = rng.integers(0, 256, shape).astype(np.uint8)
            items = [(0, int(offs[i]), lens[i], chans[i]) for i in range(len(lens))]
            rc, msg, out, off = conv(eng._lib, eng, items, taps, block, 2 if two else 1, FMT[kind], sr, int(CR.layout(lens, sr)[-1]))
            assert rc == _ffi.VAD_OK and off.tolist() == CR.layout(lens, sr).tolist(), msg
            _check(out, off, block, kind, items, lens, taps, sr)


def test_an_8k_engine_converts_against_its_own_rate():
    e8 = _engine(8000)
    try:
        engine_8k_body(e8._lib, e8)
    finally:
        e8.close()


def test_the_operator_cache_keys_on_L_and_on_M(eng):
    cache_body(eng._lib, eng)


# ---- real taps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", REAL)
def test_default_taps_within_the_derived_bound(eng, sr):
    """the engine's own default design on Gaussian noise: every sample within (ceil(N / L) + 4) u D of float64.  Prints the measured
    maximum of |dy| / (u D)."""
    assert set(REAL) <= set(CC.COVER)
    rng = np.random.default_rng(sr)
    L, M = CR.ratio(sr)
    h = eng._convert_taps(sr, None)
    x = (0.3 * rng.standard_normal(min(3 * 16 * CR.period_inputs(sr) + 77, 40000))).astype(np.float32)
    data, start = eng.convert([x], sr, taps=h)
    y, D = CR.convert_f64(x, h, sr), CR.convert_f64(x, h, sr, absolute=True)
    got = data[:y.size].astype(np.float64)
    assert start.tolist() == [0, (y.size + 3) & ~3] and (D > 0).all()
    worst = float((np.abs(got - y) / (CR.U * D)).max())
    print(f"convert {sr} Hz, {h.size} taps: max |dy| / (u D) = {worst:.2f} on the GPU, {CR.bound(h.size, L)} allowed")
    assert (np.abs(got - y) <= CR.bound(h.size, L) * CR.U * D).all(), (sr, worst)


@pytest.mark.parametrize("sr", [4000, 161920])
def test_one_nan_sample_poisons_its_tap_window_and_nothing_beyond_the_reach(eng, sr):
    """tests/test_gpu_scan_convert.py's test of the same name at x4 upsampling with PI = 4 and at runs of 3 periods of 4 048 inputs"""
    rng = np.random.default_rng(12)
    L, M = CR.ratio(sr)
    h = eng._convert_taps(sr, None)
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
def _recordings(sr):
    """three recordings of about 1 s at `sr`, built as tests/test_gpu_scan_convert.py's _recordings_44k: the golden clip's speech
    stretched by index, and harmonic bursts from tests/signals.py"""
    from tests.signals import make_streams
    L, M = CR.ratio(sr)
    pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"]
    loud = int(np.argmax(np.convolve(np.abs(pcm.astype(np.float64)), np.ones(8000), "valid")))
    at = lambda n16, first: pcm[min(first, pcm.size - n16 - 1) + (np.arange(n16 * M // L) * L) // M]
    a = at(16000, loud).copy()
    a[a.size // 2:] = 0
    b = at(18000, max(loud - 4000, 0)).copy()
    tone = make_streams(2, 40, seed=77)[1].reshape(-1)[:16000]
    c = (tone[(np.arange(sr) * L) // M] * 30000 * ((np.arange(sr) // (sr // 4)) % 2 == 0)).astype(np.int16)
    return [np.ascontiguousarray(a.astype(np.int16)), np.ascontiguousarray(b.astype(np.int16)), c]


@pytest.mark.parametrize("sr", [6400, 176400])
def test_scan_convert_segments_is_convert_then_scan_segments(eng, sr):
    """x2.5 upsampling on 5 row-tiles, and runs of exactly 16 periods of 882 inputs: the table's bytes and the offsets"""
    c = CC.census([sr])
    CC.hold(c, {6400: "upsampling_over2", 176400: "run_16"}[sr])
    assert c["tiles"] == {5}
    hop = 256
    recs = _recordings(sr)
    lens = [r.size for r in recs]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
    block = np.zeros(int(offs[-1]), np.int16)
    for o, r in zip(offs, recs):
        block[o:o + r.size] = r
    h = eng._convert_taps(sr, None)
    twin = _engine(16000)
    sa = eng.open_streams(3)
    try:
        sb = twin.open_streams(3)
        eng.set_thresholds_many(sa, THR)
        twin.set_thresholds_many(sb, THR)
        items = [(int(sa[i]), int(offs[i]), lens[i], 0) for i in range(3)]
        rc, msg, table, count, off = scan_conv(eng._lib, eng, items, h, block, 1, FMT["i16_32767"], sr, hop, thr=0.01)
        assert rc == _ffi.VAD_OK and count >= 1, (msg, count)
        total = int(CR.layout(lens, sr)[-1])
        rc, msg, out, off2 = conv(twin._lib, twin, items, h, block, 1, FMT["i16_32767"], sr, total)
        assert rc == _ffi.VAD_OK and off.tolist() == off2.tolist() == CR.layout(lens, sr).tolist(), msg
        second = [(int(sb[i]), int(off[i]), CR.samples(lens[i], sr), 0) for i in range(3)]
        rc, msg, table2, count2 = scan_segs(twin._lib, twin, second, out[:total], hop, thr=0.01)
        assert rc == _ffi.VAD_OK and count2 == count and table[:count].tobytes() == table2[:count].tobytes(), (msg, count, count2)
    finally:
        twin.close()
        for s in sa:
            eng.close_stream(int(s))
