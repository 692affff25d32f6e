"""Exact references for vad_resample_generic (scipy.signal.resample(x, n_out): real input, no window) that need no FFT on the
host, and the launch-split rules of its two host paths restated.  No tests in here; importing it loads neither the engine nor the
library, and nothing in it calls vad_debug_resample_generic_entries (the host half of the code under test).

  tones      dense input: a sum of cosines on the input's own bins is resampled to the same cosines on the output grid, with the
             two rules scipy has for a tone on the Nyquist bin.  O(n) on the host at any length.
  entries    sparse input: the operator's entries D(m, n) / n_in from the closed form, phases reduced in Python integers (they
             reach 2^76 at the lengths the tests use), evaluated in np.longdouble.
  tolerance  2^-24 |y| + SLACK * amp: one round-to-nearest cast of a float64 value to float32 (derived), plus SLACK for the
             float64 arithmetic in front of it (measured, below).  amp is sum |A| for tones, sum |x[n]| for impulses.

SLACK.  tests/test_resample_exact.py measures how far float64 scipy.signal.resample is from these references, relative to amp,
over the parity matrix (tones on bins 0, 1, K - 1, K, K + 1, n_in / 2 - 1, n_in / 2 and up to seven impulses per shape): 9.5e-16
at the worst (tones, at 30 011 -> 10 007, where the float64 phase 2 pi f + phi has that much error of its own; impulses through
`entries`: 9.2e-17, at 512 -> 1 411).  SLACK is 1024 times that, rounded up to a power of two: the chirp-z path runs four FFTs at
up to four times scipy's length, plus chirp products, and their error grows with log P.  That gives 2^-39 = 1.8e-12, below the
2^-34 at which the float64 term would stop being 2^10 under the float32 half-ulp of a full-scale sample: the comparison stays a test
of float32 rounding.  The CPU test asserts both relations, so a scipy whose float64 error is different says so.
"""
import math
from collections import namedtuple

import numpy as np

SLACK = 2.0 ** -39
MARGIN = 1024.0
SLACK_LIMIT = 2.0 ** -34

_LD = np.longdouble
_PI = _LD("3.14159265358979323846264338327950288")


def tolerance(y, amp):
    return 2.0 ** -24 * np.abs(np.asarray(y, np.float64)) + SLACK * float(amp)


# ---- dense input: tones -----------------------------------------------------------------------------------------------------------
def _cos_bin(k, length, phi):
    """cos(2 pi (k i mod length) / length + phi), i < length, the phase reduced in int64: k i mod length by a table of one block and
    each block's start, both below length, so nothing is ever near 2^63; in blocks that stay in cache (a 33 M-sample tone: 0.5 s)"""
    k, length, B = int(k), int(length), 1 << 16
    base = (k * np.arange(min(B, length), dtype=np.int64)) % length
    out = np.empty(length)
    start, step = 0, (k * B) % length
    for i0 in range(0, length, B):
        r = base[:min(B, length - i0)] + start
        r[r >= length] -= length
        f = out[i0:i0 + len(r)]
        f[:] = r
        f *= 2.0 * math.pi / length
        f += phi
        np.cos(f, out=f)
        start = (start + step) % length
    return out


def tones(n_in, n_out, spec, nyquist=True):
    """spec: [(k, A, phi), ...] with 0 <= k <= n_in // 2 -> (x [n_in], y [n_out]) float64, y = scipy.signal.resample(x, n_out) of the exact
    x.  nyquist=False leaves scipy's rule for a tone on the input's Nyquist bin out (a wrong reference, for the tests' own teeth)."""
    n_in, n_out = int(n_in), int(n_out)
    K = min(n_in, n_out) // 2
    x, y = np.zeros(n_in), np.zeros(n_out)
    for k, A, phi in spec:
        assert 0 <= k <= n_in // 2, (k, n_in)
        x += A * _cos_bin(k, n_in, phi)
        if k > K:
            continue                                             # not among the bins scipy keeps
        if nyquist and 2 * k == n_in and n_out >= n_in:
            y += A * math.cos(phi) * _cos_bin(k, n_out, 0.0)     # X[n_in / 2] is real, and halved when the array grows
        elif nyquist and 2 * k == n_out and n_out < n_in:
            y += A * math.cos(phi) * (1.0 - 2.0 * (np.arange(n_out) & 1))   # Y[n_out / 2] doubled, irfft reads its real part once
        else:
            y += A * _cos_bin(k, n_out, phi)
    return x, y


def tone_amp(spec):
    return float(sum(abs(A) for _, A, _ in spec))


# the shapes both test modules run in full: every parity of growing, shrinking and equal lengths
PARITY = [(1, 1), (1, 5), (2, 1), (8, 8), (9, 9), (8, 6), (8, 5), (9, 6), (9, 4), (6, 8), (6, 9), (5, 8), (5, 9), (255, 256), (256, 255),
          (1000, 500), (500, 1000), (1411, 512), (512, 1411), (30011, 10007)]


def tone_spec(n_in, n_out):
    """bins 0, 1, K - 1, K, K + 1, n_in / 2 - 1, n_in / 2 where they exist; phases away from 0, so that the cos(phi) rules are live"""
    K = min(n_in, n_out) // 2
    bins = [0, 1, K - 1, K, K + 1, n_in // 2 - 1, n_in // 2]
    bins = [k for i, k in enumerate(bins) if 0 <= k <= n_in // 2 and k not in bins[:i]]
    return [(k, 0.5 / (1 + i % 3), 0.3 + 0.7 * i) for i, k in enumerate(bins)]


# ---- sparse input: operator entries ----------------------------------------------------------------------------------------------
def _ld(v):
    """object array of Python ints, |v| < 2^95 -> longdouble without passing through a double"""
    neg = (v < 0).astype(bool)
    a = np.where(neg, -v, v)
    hi, lo = (a >> 32).astype(np.float64).astype(_LD), (a & 0xFFFFFFFF).astype(np.int64).astype(_LD)   # hi < 2^53: exact in a double
    r = hi * _LD(2.0 ** 32) + lo
    return np.where(neg, -r, r)


def _sincos_pi(r, L):
    """sin and cos of pi r / L for object-int r in [0, 2 L): the quadrant in integers, the rest |f| <= 1/4 in longdouble"""
    q = (4 * r + L) // (2 * L)
    f = _ld(2 * r - q * L) / _LD(2 * L)
    s, c = np.sin(_PI * f), np.cos(_PI * f)
    q = (q & 3).astype(np.int64)
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def entries(n_in, n_out, ms, ns):
    """D(m, n) / n_in in np.longdouble for broadcastable integer arrays ms, ns:
    D = sin(P pi t) / sin(pi t) - [corr] cos(2 pi K t), t = ((m a - n b) mod L) / L, D(0) = P - corr, where n_in = g a, n_out = g b,
    L = g a b, K = min(n_in, n_out) // 2, P = 2 K + 1, corr = (n_out >= n_in and n_in even)."""
    n_in, n_out = int(n_in), int(n_out)
    g = math.gcd(n_in, n_out)
    a, b = n_in // g, n_out // g
    L = a * n_out
    K = min(n_in, n_out) // 2
    P = 2 * K + 1
    corr = 1 if (n_out >= n_in and n_in % 2 == 0) else 0
    m, n = np.broadcast_arrays(np.asarray(ms).astype(object), np.asarray(ns).astype(object))
    shape, m, n = m.shape, m.reshape(-1), n.reshape(-1)
    j = (m * a - n * b) % L
    zero = (j == 0).astype(bool)
    sP, _ = _sincos_pi((P * j) % (2 * L), L)
    s1, _ = _sincos_pi(j, L)
    d = sP / np.where(zero, _LD(1), s1)
    if corr:
        d = d - _sincos_pi((2 * K * j) % (2 * L), L)[1]
    return (np.where(zero, _LD(P - corr), d) / _LD(n_in)).reshape(shape)


IMPULSE_AMPS = (1.0, -0.5, 0.25, -1.0, 0.5, -0.25, 0.125)        # exact in float32


def impulse_positions(n_in, seed):
    """n = 0, 1, n_in // 2, n_in - 1 and three seeded positions, without repeats"""
    rng = np.random.default_rng(seed)
    pos = [0, 1, n_in // 2, n_in - 1] + [int(v) for v in rng.integers(0, n_in, 3)]
    return [p for i, p in enumerate(pos) if 0 <= p < n_in and p not in pos[:i]]


def impulses(n_in, n_out, positions, ms):
    """-> (x [n_in] float32 with IMPULSE_AMPS at the positions, y float64 at the outputs ms, amp)"""
    x = np.zeros(int(n_in), np.float32)
    ms = np.asarray(ms, np.int64)
    y = np.zeros(ms.shape, _LD)
    for i, p in enumerate(positions):
        v = IMPULSE_AMPS[i % len(IMPULSE_AMPS)]
        x[p] = v
        y += _LD(v) * entries(n_in, n_out, ms, p)
    return x, y.astype(np.float64), float(np.abs(x).sum())


# ---- the launch splits of engine.cpp, restated -------------------------------------------------------------------------------------
Launch = namedtuple("Launch", "row0 rows m_begin m_end nslice")
RSF_MAX_LEN = 1 << 25            # resample_generic.h: RSF_MAX_LEN


def by_size_fft(rows, n_in, n_out):
    """engine.cpp:4545-4550, rsf_fits / rsg_use_fft with no path pinned: the FFT path from 2^25 entries, where its lengths allow"""
    return n_in <= RSF_MAX_LEN and n_out <= RSF_MAX_LEN and max(rows, 1) * n_in * n_out >= 1 << 25


def direct_launches(rows, n_in, n_out):
    """engine.cpp:4659-4682, rsg_run (`constexpr int64_t BUDGET = 1ll << 34` down to `p.slice_len = ...`): (row group) x (output range)
    launches of at most 2^34 entries, at most 65 535 rows (grid.z), whole 64-output tiles; per launch the slices of n."""
    budget = 1 << 34
    tiles_all = (n_out + 63) // 64
    per_tile = n_in * 64
    rows_per = max(1, min(rows, 65535, budget // max(1, per_tile * tiles_all)))
    tiles_per = tiles_all if rows_per > 1 else max(1, min(tiles_all, budget // per_tile))
    out = []
    for r0 in range(0, rows, rows_per):
        rc = min(rows_per, rows - r0)
        for t0 in range(0, tiles_all, tiles_per):
            tc = min(tiles_per, tiles_all - t0)
            ns = max(1, min((4096 + tc * rc - 1) // (tc * rc), max(1, n_in // 64)))
            sl = (n_in + ns - 1) // ns
            out.append(Launch(r0, rc, t0 * 64, min(n_out, (t0 + tc) * 64), (n_in + sl - 1) // sl))
    return out


def fft_groups(rows, n_in, n_out):
    """engine.cpp:4566-4569 and 4605-4606, rsf_run (`P1 = pow2(2 * n_in)`, `rows_per = ... (1ll << 26) / Pmax` and the loop over r0):
    -> (log2 P1, log2 P2, [(row0, rows), ...])"""
    def pow2(v):
        q = 1
        while q < v:
            q <<= 1
        return q
    P1, P2 = pow2(2 * n_in), pow2(2 * n_out)
    rows_per = max(1, min(rows, 65535, (1 << 26) // max(P1, P2)))
    return P1.bit_length() - 1, P2.bit_length() - 1, [(r0, min(rows_per, rows - r0)) for r0 in range(0, rows, rows_per)]
