"""The rule of vad_mel_project (include/vad_engine.h) in numpy float64, and its bound: y[r][c] = bias[c] + sum_k x[r][k] op[k][c].
project() is the exact value up to float64's own rounding - about 2^-29 of float32's: its error is (n_in + 1) 2^-53 D, against the
kernel's (n_in + 2) 2^-24 D.  Shared by tests/test_mel_project_host.py and tests/test_gpu_mel_project.py."""
import numpy as np

U = 2.0 ** -24


def project(x, op, bias=None):
    """-> float64 [rows, n_out]"""
    x, op = np.asarray(x, np.float32).astype(np.float64), np.asarray(op, np.float32).astype(np.float64)
    b = np.zeros(op.shape[1]) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    return x @ op + b[None, :]


def _fmaf(a, b, c):
    """float32 fmaf(a, b, c), correctly rounded, on float64 arrays that hold float32 values: a * b is exact in float64; the sum is
    taken with its rounding error (TwoSum) and rounded to ODD, which makes the second rounding, to float32, the only one that counts"""
    p = a * b
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even & np.isfinite(s), np.nextafter(s, toward), s)
    return s.astype(np.float32).astype(np.float64)


def fma_chain(x, op, bias=None):
    """the header's rule to the bit: acc = bias[c], then acc = fmaf(x[r][k], op[k][c], acc) for k ascending -> float32 [rows, n_out]"""
    x, op = np.asarray(x, np.float32).astype(np.float64), np.asarray(op, np.float32).astype(np.float64)
    b = np.zeros(op.shape[1]) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    acc = np.broadcast_to(b[None, :], (x.shape[0], op.shape[1])).copy()
    for k in range(op.shape[0]):
        acc = _fmaf(x[:, k:k + 1], op[k:k + 1, :], acc)
    return acc.astype(np.float32)


def magnitude(x, op, bias=None):
    """D[r][c] = |bias[c]| + sum_k |x[r][k]| |op[k][c]|"""
    return project(np.abs(np.asarray(x, np.float32)), np.abs(np.asarray(op, np.float32)), None if bias is None else np.abs(np.asarray(bias, np.float32)))


def bound(x, op, bias=None):
    """the header's guarantee for a fused-multiply-add chain: (n_in + 2) u D"""
    return (np.asarray(op).shape[0] + 2) * U * magnitude(x, op, bias)


def ratio(got, x, op, bias=None):
    """|got - exact| / (u D), elementwise (0 where D is 0 and got is exact)"""
    err = np.abs(np.asarray(got, np.float64) - project(x, op, bias))
    D = magnitude(x, op, bias)
    return np.where(D > 0, err / (U * np.where(D > 0, D, 1.0)), np.where(err > 0, np.inf, 0.0))


def integers(rng, rows, n_in, n_out, bias=True):
    """integer x, op and bias with |x|, |op| <= 64: every partial sum stays below 128 * 4096 + 2^20 < 2^24, so float32 is exact"""
    x = rng.integers(-64, 65, (rows, n_in)).astype(np.float32)
    op = rng.integers(-64, 65, (n_in, n_out)).astype(np.float32)
    b = rng.integers(-(1 << 20), (1 << 20) + 1, n_out).astype(np.float32) if bias else None
    return x, op, b


def logmel_like(rng, rows, n_in):
    """rows like log10-mel frames: a smooth spectral tilt plus noise, -10 (the floor) in places"""
    tilt = np.linspace(1.0, -4.0, n_in)[None, :] + rng.uniform(-2.0, 1.0, (rows, 1))
    x = tilt + rng.normal(0.0, 0.8, (rows, n_in))
    x[rng.uniform(size=x.shape) < 0.03] = -10.0
    return x.astype(np.float32)
