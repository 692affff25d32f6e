"""The rule of vad_scan_resample_cut (include/vad_engine.h) in numpy, for tests/test_scan_resample_cut_host.py (the CPU stand-in) and
tests/test_gpu_scan_resample_cut.py (the GPU): y[m] = sum_k x[k] h[m M - k L + C] over the segment's own samples, zero outside them.
An int64 evaluation for the cases in which float32 is exact in any order (assert_exact checks that precondition first), float64 with
the error scale D for the derived bound, and float32 accumulated in ascending k for comparison.  No test, no library: importing it
loads neither the stand-in nor the engine."""
import numpy as np

U = 2.0 ** -24
RATES = (8000, 24000, 48000)
CHUNK = {8000: 256, 24000: 768, 48000: 1536}


def ratio(sr):
    """L / M = 16000 / sr in lowest terms"""
    return {8000: (2, 1), 24000: (2, 3), 48000: (1, 3)}[sr]


def s_in(nframes, sr, hop):
    return (nframes - 1) * hop + CHUNK[sr]


def s16(S_in, sr):
    L, M = ratio(sr)
    return (S_in * L // M) & ~3


def bound(ntaps, sr):
    """|y - y_exact| <= bound * D for any order of the float32 sum"""
    L, _ = ratio(sr)
    return (-(-ntaps // L) + 4) * U


def _band(S_in, ntaps, sr):
    """per output m the input indices k that can meet a tap, their tap indices, and which of the pairs exist"""
    L, M = ratio(sr)
    C = (ntaps - 1) // 2
    m = np.arange(s16(S_in, sr), dtype=np.int64)[:, None]
    kmin = -((-(m * M + C - ntaps + 1)) // L)
    k = kmin + np.arange(-(-ntaps // L) + 1, dtype=np.int64)[None, :]
    t = m * M - k * L + C
    ok = (t >= 0) & (t < ntaps) & (k >= 0) & (k < S_in)
    return np.where(ok, k, 0), np.where(ok, t, 0), ok


def products(x, taps, sr, dtype):
    """[S16, J]: the terms of every output's sum in ascending k, zeros where there is none"""
    x, taps = np.asarray(x), np.asarray(taps)
    k, t, ok = _band(x.size, taps.size, sr)
    return np.where(ok, x.astype(dtype)[k] * taps.astype(dtype)[t], dtype(0))


def evaluate(x, taps, sr):
    """the float32 samples of one segment and float32 taps -> (y, D) in float64"""
    p = products(np.asarray(x, np.float32), np.asarray(taps, np.float32), sr, np.float64)
    return p.sum(axis=1), np.abs(p).sum(axis=1)


def evaluate_f32(x, taps, sr):
    """the same sum in float32, accumulated in ascending k"""
    p = products(np.asarray(x, np.float32), np.asarray(taps, np.float32), sr, np.float32)
    acc = np.zeros(p.shape[0], np.float32)
    for j in range(p.shape[1]):
        acc = (acc + p[:, j]).astype(np.float32)
    return acc


def assert_exact(x, taps, sr, scale=2.0 ** 16):
    """The precondition under which the float32 sum is exact in any order: samples are integer multiples of 1 / scale, taps are
    integers, and the sum of the MAGNITUDES of an output's terms, in units of 1 / scale, stays below 2^24 - so does every partial sum.
    Evaluated in int64; raises AssertionError where a case violates it.  -> y as float32 (exact)."""
    q = np.asarray(x, np.float32).astype(np.float64) * scale
    h = np.asarray(taps, np.float32).astype(np.float64)
    assert np.array_equal(q, np.rint(q)) and np.array_equal(h, np.rint(h)), "not on the grid"
    p = products(q.astype(np.int64), h.astype(np.int64), sr, np.int64)
    assert int(np.abs(p).sum(axis=1).max(initial=0)) < 2 ** 24, "a partial sum could leave 24 bits"
    y = p.sum(axis=1).astype(np.float64) / scale
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    return y.astype(np.float32)


def gained(y, g):
    """one float32 multiply of its own"""
    return y if g is None else (np.asarray(y, np.float32) * np.float32(g)).astype(np.float32)


def pcm16(y):
    """utils/wav_writer.py:41"""
    return np.clip(np.asarray(y, np.float32) * 32767, -32768, 32767).astype(np.int16)
