"""vad_resample_generic on the GPU against the exact references of tests/resample_exact.py: both kernels on every parity of the
lengths, the direct kernel's small-angle branch, FFT stage mixes and lengths up to the FFT path's limit, the direct kernel past
that limit, and every split of a call into launches (output ranges, row groups) that engine.cpp's rsg_run and rsf_run can make.
Every assertion is |got - y| <= tolerance(y, amp) per output sample (one float32 rounding of the float64 answer, plus the measured
float64 slack); each test prints the largest |got - y| / tolerance it saw (DESIGN 2.3b records them)."""
import numpy as np
import pytest

from tests import resample_exact as X

pytestmark = pytest.mark.gpu
DIRECT, FFT = 1, 2
NAME = {0: "by size", DIRECT: "direct", FFT: "fft"}


@pytest.fixture(scope="module")
def engine():
    """an engine of this module's own: the FFT path's work buffers reach 1 GB each here and go with it"""
    from cutter_vad_amd import weights_io
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        e = Engine(f.read(), max_streams=64)
    yield e
    e.close()


def run(engine, mode, x, n_out):
    x = x if x.ndim == 2 else x.reshape(1, -1)
    try:
        engine.set_resample_path(mode)
        return engine.resample_generic(x, n_out)
    finally:
        engine.set_resample_path(0)


class Worst:
    """the largest |got - y| / tolerance per kernel, for the line a test prints"""
    def __init__(self, what):
        self.what, self.r = what, {}

    def check(self, kernel, got, y, amp, where):
        assert got.dtype == np.float32 and got.shape == y.shape, where
        ratio = np.abs(got.astype(np.float64) - y) / X.tolerance(y, amp)
        self.r[kernel] = max(self.r.get(kernel, 0.0), float(ratio.max()))
        assert (ratio <= 1.0).all(), (where, kernel, float(ratio.max()), int(np.argmax(ratio)))

    def report(self):
        print(f"resample_exact {self.what}: max |got - y| / tolerance = " + ", ".join(f"{v:.3f} ({k})" for k, v in sorted(self.r.items())))


def long_spec(n_in, n_out):
    """three tones: one in the middle of the kept band, the last kept bin K, and K + 1 (dropped) - or K - 1 where K is n_in // 2"""
    K = min(n_in, n_out) // 2
    return [(K // 3 + 1, 0.5, 0.3), (K, 0.25, 1.0), (K + 1 if K + 1 <= n_in // 2 else K - 1, 0.125, 1.7)]


def picks(n_out, count, extra=()):
    m = np.concatenate([np.linspace(0, n_out - 1, count).astype(np.int64), np.asarray(list(extra), np.int64).reshape(-1)])
    return np.unique(m[(m >= 0) & (m < n_out)])


def peak(n, n_in, n_out):
    return (n * n_out + n_in // 2) // n_in % n_out


@pytest.fixture(scope="module")
def parity():
    out = []
    for n_in, n_out in X.PARITY:
        spec = X.tone_spec(n_in, n_out)
        xt, yt = X.tones(n_in, n_out, spec)
        xi, yi, ai = X.impulses(n_in, n_out, X.impulse_positions(n_in, n_in * 7919 + n_out), np.arange(n_out))
        for a in (xt, yt, xi, yi):
            a.setflags(write=False)
        out.append((n_in, n_out, xt, yt, X.tone_amp(spec), xi, yi, ai))
    return out


def test_parity_matrix_on_both_kernels(engine, parity):
    """every parity of growing, shrinking and equal lengths, every output: tones as float64 input, impulses as float32 input"""
    w = Worst("parity matrix")
    for n_in, n_out, xt, yt, at, xi, yi, ai in parity:
        assert len(X.direct_launches(1, n_in, n_out)) == 1
        for mode in (DIRECT, FFT):
            got = run(engine, mode, xt, n_out)
            w.check(NAME[mode], got[0], yt, at, ("tones", n_in, n_out))
            assert got.tobytes() == run(engine, mode, xt, n_out).tobytes(), (mode, n_in, n_out)
            goti = run(engine, mode, xi, n_out)
            w.check(NAME[mode], goti[0], yi, ai, ("impulses", n_in, n_out))
            assert goti.tobytes() == run(engine, mode, xi, n_out).tobytes(), (mode, n_in, n_out)
    w.report()


@pytest.mark.parametrize("n_in,n_out", [(99991, 100003), (48000, 16000)])
def test_small_angle_branch_around_every_peak(engine, n_in, n_out):
    """the direct kernel takes sin(pi t) from its series where |t| < 2^-10: |m - peak| < n_out / 1024.  Every output within
    n_out / 512 + 2 of each impulse's peak has both sides of that test on both flanks; coprime lengths never have t == 0 away from
    (0, 0), 48 000 -> 16 000 has it at n = 3 q, m = q (n = 24 000 here)."""
    pos = [0, 1, n_in // 2, n_in - 1]
    half = n_out // 512 + 2
    assert half > n_out / 1024 + 1
    near = np.concatenate([(peak(p, n_in, n_out) + np.arange(-half, half + 1)) % n_out for p in pos])
    ms = np.unique(np.concatenate([near, picks(n_out, 64)]))
    x, y, amp = X.impulses(n_in, n_out, pos, ms)
    if n_in == 48000:
        assert (n_in // 2) * n_out % n_in == 0 and peak(n_in // 2, n_in, n_out) == 8000
    w = Worst(f"small-angle window {n_in} -> {n_out}")
    for mode in (DIRECT, FFT):
        w.check(NAME[mode], run(engine, mode, x, n_out)[0, ms], y, amp, (n_in, n_out))
    w.report()


@pytest.mark.parametrize("n_in,n_out,p1,p2", [(40000, 20001, 17, 16), (70000, 140001, 18, 19), (600000, 1200001, 21, 22)])
def test_fft_stage_mixes(engine, n_in, n_out, p1, p2):
    """log2 P = 16 .. 22 with every remainder mod 3: the radix-2 / radix-4 first stages in front of the radix-8 ones"""
    assert X.by_size_fft(1, n_in, n_out) and X.fft_groups(1, n_in, n_out) == (p1, p2, [(0, 1)])
    w = Worst(f"fft stages {n_in} -> {n_out} (log2 P = {p1}, {p2})")
    spec = long_spec(n_in, n_out)
    x, y = X.tones(n_in, n_out, spec)
    w.check("fft", run(engine, 0, x, n_out)[0], y, X.tone_amp(spec), "tones")
    pos = X.impulse_positions(n_in, n_in)
    ms = picks(n_out, 1024, [peak(p, n_in, n_out) + d for p in pos for d in (-1, 0, 1)])
    xi, yi, ai = X.impulses(n_in, n_out, pos, ms)
    w.check("fft", run(engine, 0, xi, n_out)[0, ms], yi, ai, "impulses")
    w.report()


@pytest.mark.parametrize("n_in,n_out,p1,p2,with_impulses", [(1 << 25, 11184811, 26, 25, True), ((1 << 24) + 3, 1 << 25, 26, 26, False)])
def test_fft_at_its_length_limit(engine, n_in, n_out, p1, p2, with_impulses):
    """P = 2^26 is the longest transform the FFT path takes (n <= 2^25); 2^24 was the longest a test had run"""
    assert X.by_size_fft(1, n_in, n_out) and X.fft_groups(1, n_in, n_out) == (p1, p2, [(0, 1)])
    w = Worst(f"fft length limit {n_in} -> {n_out} (log2 P = {p1}, {p2})")
    spec = long_spec(n_in, n_out)
    x, y = X.tones(n_in, n_out, spec)
    w.check("fft", run(engine, 0, x, n_out)[0], y, X.tone_amp(spec), "tones")
    del x, y
    if with_impulses:
        pos = [0, n_in - 1]
        ms = picks(n_out, 4096, [peak(p, n_in, n_out) + d for p in pos for d in (-1, 0, 1)])
        xi, yi, ai = X.impulses(n_in, n_out, pos, ms)
        w.check("fft", run(engine, 0, xi, n_out)[0, ms], yi, ai, "impulses")
    w.report()


BIG = (1 << 25) + 1


@pytest.mark.parametrize("n_in,n_out", [(BIG, 1000), (1000, BIG)])
def test_direct_kernel_past_the_fft_limit(engine, n_in, n_out):
    """one sample more than the FFT path takes: the direct kernel by the size rule, 3.4e10 entries in output-range launches"""
    assert not X.by_size_fft(1, n_in, n_out)
    launches = X.direct_launches(1, n_in, n_out)
    if n_in == BIG:
        assert [(l.m_end - l.m_begin, l.nslice) for l in launches] == [(448, 586), (448, 586), (104, 2048)]
    else:
        assert [(l.m_begin, l.m_end) for l in launches] == [(0, 17179840), (17179840, BIG)]
    w = Worst(f"direct past the fft limit {n_in} -> {n_out}")
    spec = long_spec(n_in, n_out) + ([(1 << 24, 0.125, 0.5)] if n_in == BIG else [])
    x, y = X.tones(n_in, n_out, spec)
    w.check("direct", run(engine, 0, x, n_out)[0], y, X.tone_amp(spec), "tones")
    del x, y
    pos = [0, n_in - 1]
    edges = [l.m_begin + d for l in launches for d in (-1, 0, 1)] + [peak(p, n_in, n_out) + d for p in pos for d in (-1, 0, 1)]
    ms = np.arange(n_out) if n_out == 1000 else picks(n_out, 4096, edges)
    xi, yi, ai = X.impulses(n_in, n_out, pos, ms)
    w.check("direct", run(engine, 0, xi, n_out)[0, ms], yi, ai, "impulses")
    w.report()


def test_direct_kernel_two_output_ranges(engine):
    """131 073 -> 131 137 pinned to the direct kernel: 2 047 tiles in three slices of n, then 3 tiles in 1 366"""
    n_in, n_out = 131073, 131137
    launches = X.direct_launches(1, n_in, n_out)
    assert [(l.m_begin, l.m_end, l.nslice) for l in launches] == [(0, 131008, 3), (131008, n_out, 1366)]
    w = Worst(f"direct output ranges {n_in} -> {n_out}")
    spec = long_spec(n_in, n_out)
    x, y = X.tones(n_in, n_out, spec)
    w.check("direct", run(engine, DIRECT, x, n_out)[0], y, X.tone_amp(spec), "tones")
    pos = X.impulse_positions(n_in, 1)
    ms = picks(n_out, 1024, list(range(131008 - 8, n_out)) + [peak(p, n_in, n_out) + d for p in pos for d in (-1, 0, 1)])
    xi, yi, ai = X.impulses(n_in, n_out, pos, ms)
    w.check("direct", run(engine, DIRECT, xi, n_out)[0, ms], yi, ai, "impulses")
    w.report()


def mixed_rows(rows, n_in, n_out, spec1, spec2, seed):
    """rows that all differ: row r = c_r x1 + d_r x2 of two tone sets, c_r and d_r seeded non-zero multiples of 1 / 8 -> x, y, amp [rows, 1]"""
    rng = np.random.default_rng(seed)
    c, d = (rng.integers(1, 9, (2, rows, 1)) * rng.choice([-1.0, 1.0], (2, rows, 1))) / 8.0
    (x1, y1), (x2, y2) = X.tones(n_in, n_out, spec1), X.tones(n_in, n_out, spec2)
    return c * x1 + d * x2, c * y1 + d * y2, np.abs(c) * X.tone_amp(spec1) + np.abs(d) * X.tone_amp(spec2)


def check_rows(w, kernel, got, y, amp, where):
    assert got.dtype == np.float32 and got.shape == y.shape, where
    ratio = np.abs(got - y)
    ratio /= 2.0 ** -24 * np.abs(y) + X.SLACK * amp                 # X.tolerance with one amp per row
    w.r[kernel] = max(w.r.get(kernel, 0.0), float(ratio.max()))
    assert (ratio <= 1.0).all(), (where, kernel, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))


def test_direct_kernel_row_groups_by_the_entry_budget(engine):
    """5 x 65 537 -> 65 536 pinned to the direct kernel: 2^34 entries allow three rows per launch"""
    rows, n_in, n_out = 5, 65537, 65536
    assert [(l.row0, l.rows, l.m_begin, l.m_end) for l in X.direct_launches(rows, n_in, n_out)] == [(0, 3, 0, n_out), (3, 2, 0, n_out)]
    K = n_out // 2
    x, y, amp = mixed_rows(rows, n_in, n_out, [(5, 0.5, 0.3), (K, 0.25, 1.0)], [(K - 1, 0.5, 2.0), (K - 2, 0.25, 0.7), (12345, 0.125, 4.0)], 65537)
    w = Worst(f"direct row groups {rows} x {n_in} -> {n_out}")
    got = run(engine, DIRECT, x, n_out)
    check_rows(w, "direct", got, y, amp, "rows")
    assert got[3].tobytes() == run(engine, DIRECT, x[3:4], n_out).tobytes()
    w.report()


def test_direct_kernel_row_groups_by_grid_z(engine):
    """65 537 x 8 -> 5 by the size rule: more rows than grid.z takes"""
    rows, n_in, n_out = 65537, 8, 5
    assert not X.by_size_fft(rows, n_in, n_out)
    assert [(l.row0, l.rows) for l in X.direct_launches(rows, n_in, n_out)] == [(0, 65535), (65535, 2)]
    x, y, amp = mixed_rows(rows, n_in, n_out, [(0, 0.5, 0.3), (2, 0.25, 1.0)], [(1, 0.5, 2.0), (3, 0.25, 0.7), (4, 0.125, 4.0)], 8)
    w = Worst(f"direct row groups {rows} x {n_in} -> {n_out}")
    got = run(engine, 0, x, n_out)
    check_rows(w, "direct", got, y, amp, "rows")
    assert got[65535].tobytes() == run(engine, 0, x[65535:65536], n_out).tobytes()
    w.report()


def test_fft_row_groups_float32(engine):
    """65 537 x 300 -> 512 by the size rule, float32 input: groups of 65 535 (grid.y) and 2.  The tones sit on bins 0, n_in / 4 and
    n_in / 2 with phase 0, so their samples - and the rows' - are float32 values but for float64's own cos(pi / 2) = 6e-17: the
    cast to float32 moves no sample by more than 2^-50, 2^-11 of SLACK."""
    rows, n_in, n_out = 65537, 300, 512
    assert X.by_size_fft(rows, n_in, n_out) and X.fft_groups(rows, n_in, n_out) == (10, 10, [(0, 65535), (65535, 2)])
    x, y, amp = mixed_rows(rows, n_in, n_out, [(0, 0.5, 0.0), (75, 0.25, 0.0)], [(150, 0.5, 0.0), (75, 0.125, 0.0)], 300)
    x32 = x.astype(np.float32)
    assert np.abs(x32 - x).max() <= 2.0 ** -50
    w = Worst(f"fft row groups {rows} x {n_in} -> {n_out}, float32")
    got = run(engine, 0, x32, n_out)
    check_rows(w, "fft", got, y, amp, "rows")
    assert got[65535].tobytes() == run(engine, FFT, x32[65535:65536], n_out).tobytes()
    w.report()


def test_fft_row_groups_float64_on_device_pointers(engine):
    """16 385 x 1 411 -> 512 through vad_resample_generic_device, float64 input: P = 4 096 allows 16 384 rows per group, and the
    second group's input offset is in 8-byte elements"""
    import torch
    rows, n_in, n_out = 16385, 1411, 512
    assert X.by_size_fft(rows, n_in, n_out) and X.fft_groups(rows, n_in, n_out) == (12, 10, [(0, 16384), (16384, 1)])
    K = n_out // 2
    x, y, amp = mixed_rows(rows, n_in, n_out, [(7, 0.5, 0.3), (K, 0.25, 1.0)], [(K - 1, 0.5, 2.0), (K + 1, 0.25, 0.7), (n_in // 2, 0.125, 4.0)], 1411)
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.full((rows, n_out), float("nan"), device="cuda")
    torch.cuda.synchronize()
    engine.resample_generic_device(d_x.data_ptr(), rows, n_in, n_out, d_y.data_ptr(), f64=True)
    got = d_y.cpu().numpy()
    del d_x, d_y
    w = Worst(f"fft row groups {rows} x {n_in} -> {n_out}, float64, device pointers")
    check_rows(w, "fft", got, y, amp, "rows")
    assert got[16384].tobytes() == run(engine, FFT, x[16384:16385], n_out).tobytes()
    w.report()
