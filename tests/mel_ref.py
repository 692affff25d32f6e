"""The rule of vad_scan_mel (include/vad_engine.h: vad_mel) in numpy float64, for tests/test_scan_mel_host.py (the CPU stand-in)
and tests/test_gpu_scan_mel.py (the GPU): padding, framing, the two products around a square, the error scale D of the derived bound
and the precondition under which float32 is exact in any order of summation.  No test, no library: importing it loads neither the
stand-in nor the engine."""
import math

import numpy as np

from cutter_vad_amd import _ffi

U = 2.0 ** -24
NONE, REFLECT = _ffi.VAD_MEL_PAD_NONE, _ffi.VAD_MEL_PAD_REFLECT
LINEAR, LN, LOG10 = _ffi.VAD_MEL_LINEAR, _ffi.VAD_MEL_LN, _ffi.VAD_MEL_LOG10


def fields(n_fft, hop, n_bins, n_mels, pad=NONE, log=LINEAR, floor=1e-10):
    return dict(n_fft=n_fft, hop=hop, n_bins=n_bins, n_mels=n_mels, pad=pad, log=log, floor=floor)


def mel_struct(f, reserved=0):
    return _ffi.Mel(f["n_fft"], f["hop"], f["n_bins"], f["n_mels"], f["pad"], f["log"], f["floor"], reserved)


def nframes(f, S):
    """the header's M"""
    n = S + (f["n_fft"] if f["pad"] == REFLECT else 0)
    return 0 if n < f["n_fft"] else (n - f["n_fft"]) // f["hop"] + 1


def padded(v, f):
    v = np.asarray(v)
    if f["pad"] != REFLECT:
        return v
    assert v.size > f["n_fft"] // 2
    return np.pad(v, f["n_fft"] // 2, mode="reflect")


def frames(v, f):
    """the float32 samples of one segment -> [M, n_fft], in the samples' dtype"""
    p = padded(v, f)
    M = nframes(f, np.asarray(v).size)
    if M == 0:
        return np.zeros((0, f["n_fft"]), p.dtype)
    return np.stack([p[i * f["hop"]:i * f["hop"] + f["n_fft"]] for i in range(M)])


def energies(v, f, op_re, op_im, filters):
    """-> (E, D) in float64 from the float32 inputs: E[M, n_mels] and the bound's scale D"""
    x = frames(np.asarray(v, np.float32), f).astype(np.float64)
    a, b, w = (np.asarray(t, np.float32).astype(np.float64) for t in (op_re, op_im, filters))
    re, im = x @ a, x @ b
    E = (re * re + im * im) @ w.T
    D = ((np.abs(x) @ np.abs(a) + np.abs(x) @ np.abs(b)) ** 2) @ np.abs(w).T
    return E, D


def bound(f):
    """|E - E_exact| <= bound * D for any order of the float32 sums"""
    return (2 * f["n_fft"] + f["n_bins"] + 8) * U


def logged(E, f):
    """the output for energies E, in float64"""
    if f["log"] == LINEAR:
        return E
    m = np.maximum(E, float(np.float32(f["floor"])))
    return np.log(m) if f["log"] == LN else np.log10(m)


def log_tolerance(y):
    """|out - y| allowed where the logarithm's argument is bit-identical: a 1-ulp log2, one multiply, one rounding"""
    return 4 * U * np.maximum(np.abs(y), 1.0)


def assert_exact(v, f, op_re, op_im, filters):
    """The precondition under which every float32 sum is exact in any order: all values are integer multiples of one power of two,
    and the sum of the MAGNITUDES of every sum's terms stays below 2^24 (so does every partial sum, in any order).  Evaluated in
    int64 / float64 on its own; raises AssertionError where a case violates it.  -> E in float64 (exact)."""
    x = frames(np.asarray(v, np.float32), f).astype(np.float64)
    q = x * 2.0 ** 16                                               # (the mean of two int16 / 32768 is a multiple of 2^-16)
    assert np.array_equal(q, np.rint(q)), "samples are not multiples of 2^-16"
    q = q.astype(np.int64)
    a, b, w = (np.asarray(t, np.float32).astype(np.float64) for t in (op_re, op_im, filters))
    for t in (a, b, w):
        assert np.array_equal(t, np.rint(t)), "operators and filters are not integers"
    a, b, w = a.astype(np.int64), b.astype(np.int64), w.astype(np.int64)
    g = 1
    while q.size and g < 2 ** 16 and not (q % (2 * g)).any():
        g *= 2
    q //= g
    mag = np.abs(q) @ np.abs(a), np.abs(q) @ np.abs(b)
    assert max(mag[0].max(initial=0), mag[1].max(initial=0)) < 2 ** 24
    re, im = q @ a, q @ b
    P = re * re + im * im
    assert P.max(initial=0) < 2 ** 24
    assert (P @ np.abs(w).T).max(initial=0) < 2 ** 24
    E = (P @ w.T).astype(np.float64) * (g * 2.0 ** -16) ** 2
    assert (E == 0).all() or E[E != 0].min() > 2.0 ** -100          # far from float32's underflow
    return E


def exact_operators(rng, n_fft, n_bins, n_mels):
    """integer operators for which float32 is exact on small integer samples: at most 4 entries of +-1 per column, filters in {0, 1, 2}"""
    op = np.zeros((2, n_fft, n_bins), np.float32)
    for part in range(2):
        for k in range(n_bins):
            rows = rng.choice(n_fft, size=int(rng.integers(1, 5)), replace=False)
            op[part, rows, k] = rng.choice(np.array([-1.0, 1.0], np.float32), size=rows.size)
    return op[0], op[1], rng.integers(0, 3, (n_mels, n_bins)).astype(np.float32)


def rows_of(segments_samples, f, op_re, op_im, filters, exact=False):
    """the packed matrix vad_scan_mel writes for segments with these float32 samples, in float64 -> (rows, start [n + 1])"""
    out, start = [], [0]
    for v in segments_samples:
        E = assert_exact(v, f, op_re, op_im, filters) if exact else energies(v, f, op_re, op_im, filters)[0]
        out.append(logged(E, f))
        start.append(start[-1] + E.shape[0])
    rows = np.concatenate(out) if out else np.zeros((0, f["n_mels"]))
    return rows.reshape(-1, f["n_mels"]), np.asarray(start, np.int64)


def log_of_bounded(got, E, D, f):
    """LOG10 / LN on real operators: where E >= 16 bound D the relative error d = bound D / E <= 1 / 16 moves the logarithm by at
    most -log(1 - d), plus the logarithm's own tolerance -> (mask of the entries checked, |difference|, tolerance), all in float64"""
    B = bound(f)
    mask = (E >= 16 * B * D) & (E > float(np.float32(f["floor"])))
    d = np.where(mask, B * D / np.where(mask, E, 1.0), 0.0)
    y = logged(E, f)
    shift = -np.log1p(-d) / (math.log(10.0) if f["log"] == LOG10 else 1.0)
    return mask, np.abs(got - y), shift + log_tolerance(y)


def speechlike(rng, n, rate=16000):
    """a seeded signal with speech's shape: a 140 Hz pulse train through three formant-like resonances, syllable-rate envelope, noise"""
    t = np.arange(n) / float(rate)
    voiced = sum(a * np.sin(2 * np.pi * f0 * t + ph) for a, f0, ph in ((0.2, 140.0, 0.0), (0.12, 700.0, 1.0), (0.08, 1220.0, 2.0), (0.04, 2600.0, 0.5)))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)
    return (env * voiced + 0.02 * rng.standard_normal(n)).astype(np.float32)


def noise_and_tone(rng, n, rate=16000):
    """The signal of the logarithm's bound cases: white noise kept on one sample in sixteen, plus a weak 440 Hz tone.  A logarithm is
    checked where E >= 16 bound D, and E / D of a bin is about 2.3 / (the non-zero terms of its sum) for white noise under a Hann
    window: dense noise leaves more than a tenth of Whisper's entries - and almost all at n_fft = 1024 - outside the condition by
    the float64 reference alone; the sparse one keeps 93 % or more inside at every geometry tested."""
    t = np.arange(n)
    return (0.01 * np.sin(2 * np.pi * 440.0 / rate * t) + 0.5 * rng.standard_normal(n) * (rng.random(n) < 0.0625)).astype(np.float32)
