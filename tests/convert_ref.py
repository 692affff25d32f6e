"""The rule of vad_convert (include/vad_engine.h), written from the header alone in int64 / float64: the ratio and the accepted rates,
S_out, y[m] = sum_k x[k] h[m M - k L + C] over the k in [0, S_in) whose tap index lies in [0, N), D[m] = sum_k |x[k]| |h[.]|, the
layout out_offset[i] = sum of roundup4(S_out_j), and the reach K of the kernel's operator windows.  No engine code is imported."""
import math

import numpy as np

MAX_REACH, MIN_RATE, MAX_RATE, MAX_PERIOD = 128, 4000, 192000, 640
U = 2.0 ** -24


def ratio(sr_in, R=16000):
    g = math.gcd(int(sr_in), int(R))
    return R // g, sr_in // g


def period(L):
    return L * 16 // math.gcd(L, 16)


def accepted(sr_in, R=16000):
    if sr_in < MIN_RATE or sr_in > MAX_RATE or sr_in == R:
        return False
    L, M = ratio(sr_in, R)
    return period(L) <= MAX_PERIOD and M <= MAX_PERIOD


def samples(S_in, sr_in, R=16000):
    L, M = ratio(sr_in, R)
    return S_in * L // M


def period_inputs(sr_in, R=16000):
    L, M = ratio(sr_in, R)
    return period(L) * M // L


def reach(ntaps, sr_in, R=16000):
    """K of the header: an output m is untouched by input k when |k - m M / L| >= K"""
    L, M = ratio(sr_in, R)
    return ((15 * M + ntaps - 1) // L + 2 + 15) & ~15


def layout(S_in_list, sr_in, R=16000):
    off = [0]
    for s in S_in_list:
        off.append(off[-1] + ((samples(s, sr_in, R) + 3) & ~3))
    return np.array(off, np.int64)


def _windows(S_in, N, L, M, m):
    """k range [k0, k1) with tap index m M - k L + C in [0, N), clipped to [0, S_in)"""
    C = (N - 1) // 2
    k0 = -((-(m * M + C - N + 1)) // L)      # ceil
    k1 = (m * M + C) // L + 1
    return max(k0, 0), min(k1, S_in)


def convert_f64(x, h, sr_in, R=16000, absolute=False):
    """y (or D with absolute=True) of one item in float64: x the decoded float32 samples, h the taps"""
    L, M = ratio(sr_in, R)
    x = np.abs(np.asarray(x, np.float64)) if absolute else np.asarray(x, np.float64)
    h = np.abs(np.asarray(h, np.float64)) if absolute else np.asarray(h, np.float64)
    S_in, N = x.size, h.size
    C = (N - 1) // 2
    S_out = S_in * L // M
    y = np.zeros(S_out, np.float64)
    for m in range(S_out):
        k0, k1 = _windows(S_in, N, L, M, m)
        if k1 > k0:
            k = np.arange(k0, k1)
            y[m] = np.dot(x[k], h[m * M - k * L + C])
    return y


def convert_exact(xi, hi, sr_in, R=16000, limit=1 << 24):
    """int64: xi the samples in units (integers), hi integer taps -> y in units; asserts that the sum of |products| of every output
    stays under 2^24 units, so that every partial sum in ANY order is an exactly representable float32"""
    L, M = ratio(sr_in, R)
    xi, hi = np.asarray(xi, np.int64), np.asarray(hi, np.int64)
    S_in, N = xi.size, hi.size
    C = (N - 1) // 2
    S_out = S_in * L // M
    y = np.zeros(S_out, np.int64)
    for m in range(S_out):
        k0, k1 = _windows(S_in, N, L, M, m)
        if k1 > k0:
            k = np.arange(k0, k1)
            t = hi[m * M - k * L + C]
            assert int(np.abs(xi[k] * t).sum()) < limit, (m, int(np.abs(xi[k] * t).sum()))
            y[m] = int(np.dot(xi[k], t))
    return y


def bound(N, L):
    return -(-N // L) + 4


def run_periods(ntaps, sr_in, R=16000, wg_samples=2048, lds_floats=16384):
    """periods of one workgroup's run, restated from csrc/vad_layout.h (cv_nper): 2048 outputs in whole groups of 16 periods, cut to
    what 64 KiB of local memory hold.  The tests only use it to aim lengths at a workgroup's edge."""
    L, M = ratio(sr_in, R)
    P, PI = period(L), period_inputs(sr_in, R)
    C = (ntaps - 1) // 2
    K = reach(ntaps, sr_in, R)
    lead = -(-C // L)
    bmax = (16 * (P // 16 - 1) * M - C) // L
    skew = (4 - PI % 64) % 64

    def floats(nper):
        span = (lead + 3 + (nper - 1) * PI + K + bmax + 3) & ~3
        return span + skew * (span // PI + 1)
    nper = (-(-wg_samples // P) + 15) & ~15
    while nper > 0 and floats(nper) > lds_floats:
        nper = nper - 16 if nper > 16 else nper - 1
    return nper
