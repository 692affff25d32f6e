"""The rule of vad_mel_stats / vad_mel_batch (include/vad_engine.h) in numpy, float32 operation by float32 operation: every
product, sum and difference below is one numpy float32 ufunc, which rounds where it stands - what the kernel does with contraction
off.  The statistics are integers.  Nothing here has a tolerance: the tests compare bytes."""
import numpy as np

F32, F16, BF16 = 0, 1, 2
CHANNEL, TIME = 0, 1
PAD_VALUE, PAD_FEATURE = 0, 1
f32 = np.float32


def key(x):
    """float32 -> uint32 whose unsigned order is the order of the values, -0.0 below +0.0"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def seg_max(x):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return f32(-np.inf) if x.size == 0 else x[int(np.argmax(key(x)))]


def q_of(x):
    return np.rint(np.clip(np.asarray(x, np.float32), f32(-2048), f32(2048)) * f32(4096)).astype(np.int64)


def stats(x, start):
    """-> (max float32 [n], sum int64 [n, n_mels], sumsq uint64 [n, n_mels])"""
    x = np.asarray(x, np.float32)
    n = len(start) - 1
    mx = np.array([seg_max(x[start[i]:start[i + 1]]) for i in range(n)], np.float32).reshape(n)
    q = q_of(x)
    s = np.array([q[start[i]:start[i + 1]].sum(axis=0) for i in range(n)], np.int64).reshape(n, x.shape[1])
    s2 = np.array([(q[start[i]:start[i + 1]] ** 2).sum(axis=0) for i in range(n)], np.int64).reshape(n, x.shape[1]).astype(np.uint64)
    return mx, s, s2


def normalise(x, lo, shift, scale):
    """(fmaxf(x, lo) + shift) * scale on rows x [M, n_mels]; lo a float32, shift / scale [n_mels]"""
    return (np.maximum(np.asarray(x, np.float32), f32(lo)) + np.asarray(shift, np.float32)) * np.asarray(scale, np.float32)


def delta(v):
    """d[t] = ((v[c(t + 1)] - v[c(t - 1)]) + 2 (v[c(t + 2)] - v[c(t - 2)])) * 0.1f over the rows of v [M, n_mels]"""
    M = v.shape[0]
    c = lambda k: np.clip(np.arange(M) + k, 0, M - 1)
    return ((v[c(1)] - v[c(-1)]) + f32(2) * (v[c(2)] - v[c(-2)])) * f32(0.1)


def bf16_bits(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7fff) + ((b >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return np.where(nan, ((b >> 16) | np.uint32(0x40)).astype(np.uint16), r)


def convert(a, dtype):
    if dtype == F32:
        return np.ascontiguousarray(a, np.float32)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(a, np.float32).astype(np.float16)
    return bf16_bits(a)


def batch(x, start, windows, n_mels, frames, deltas=0, layout=CHANNEL, dtype=F32, pad_mode=PAD_VALUE, pad_value=0.0, lo=None,
          shift=None, scale=None):
    """windows: (seg, nrows, row0) each -> [B, C, T] or [B, T, C] in the dtype's numpy form (bfloat16: uint16 bits)"""
    x = np.asarray(x, np.float32).reshape(-1, n_mels)
    n = len(start) - 1
    lo = np.full(n, -np.inf, np.float32) if lo is None else np.asarray(lo, np.float32).reshape(n)
    sh = np.zeros((1, n_mels), np.float32) if shift is None else np.asarray(shift, np.float32).reshape(-1, n_mels)
    sc = np.ones((1, n_mels), np.float32) if scale is None else np.asarray(scale, np.float32).reshape(-1, n_mels)
    C = n_mels * (deltas + 1)
    out = np.zeros((len(windows), frames, C), np.float32)
    chans = {}
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (seg, nrows, row0) in enumerate(windows):
            seg, nrows, row0 = int(seg), int(nrows), int(row0)
            s_, c_ = sh[seg if sh.shape[0] > 1 else 0], sc[seg if sc.shape[0] > 1 else 0]
            if seg not in chans and start[seg + 1] > start[seg]:
                v = normalise(x[start[seg]:start[seg + 1]], lo[seg], s_, c_)
                parts = [v]
                for _ in range(deltas):
                    parts.append(delta(parts[-1]))
                chans[seg] = np.concatenate(parts, axis=1)
            if nrows:
                out[k, :nrows] = chans[seg][row0:row0 + nrows]
            padv = normalise(np.full((1, n_mels), pad_value, np.float32), lo[seg], s_, c_)[0] if pad_mode == PAD_FEATURE else f32(pad_value)
            out[k, nrows:, :n_mels] = padv
    if layout == CHANNEL:
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
    return convert(out, dtype)
