"""The rules of vad_mel_pack_plan / vad_mel_batch_packed / vad_mel_stats_grouped (include/vad_engine.h) in numpy, on top of
tests/batch_ref.py: the planner as the header's five steps, the packed batch as pad cells everywhere and then each piece's cells
out of batch_ref.batch of a one-piece window with the window's affine, the grouped statistics as batch_ref.stats over the groups'
rows.  Nothing here has a tolerance: the tests compare bytes."""
import numpy as np

from tests import batch_ref as B

f32 = np.float32


def up4(x):
    return (int(x) + 3) & ~3


def plan(start, frames, gap=0, group=None):
    """-> (pieces [(seg, nrows, row0, window, offset)], nw)"""
    T, pieces, nw, used, cur = int(frames), [], 0, 0, None
    for i in range(len(start) - 1):
        M, g = int(start[i + 1] - start[i]), 0 if group is None else int(group[i])
        for r in range(0, M, T):
            k = min(T, M - r)
            offset = up4(used + gap)
            if nw == 0 or g != cur or offset + k > T:
                nw, cur, offset = nw + 1, g, 0
            pieces.append((i, k, r, nw - 1, offset))
            used = offset + k
    return pieces, nw


def piece_bounds(start, pieces):
    """the pieces of plan() tile the rows in order: their bounds as a start array"""
    return np.concatenate([[0], np.cumsum([p[1] for p in pieces])]).astype(np.int64) + int(start[0])


def batch(x, start, pieces, nw, n_mels, frames, deltas=0, layout=B.CHANNEL, dtype=B.F32, pad_mode=B.PAD_VALUE, pad_value=0.0, lo=None,
          shift=None, scale=None):
    """pieces: (seg, nrows, row0, window, offset) each; lo [nw], shift / scale [1 or nw, n_mels] by WINDOW -> [nw, C, T] or [nw, T, C]
    in the dtype's numpy form"""
    x = np.asarray(x, np.float32).reshape(-1, n_mels)
    n = len(start) - 1
    lo = np.full(nw, -np.inf, np.float32) if lo is None else np.asarray(lo, np.float32).reshape(nw)
    sh = np.zeros((1, n_mels), np.float32) if shift is None else np.asarray(shift, np.float32).reshape(-1, n_mels)
    sc = np.ones((1, n_mels), np.float32) if scale is None else np.asarray(scale, np.float32).reshape(-1, n_mels)
    C = n_mels * (deltas + 1)
    out = np.zeros((nw, frames, C), np.float32)
    of = lambda w: (lo[w], sh[w if sh.shape[0] > 1 else 0], sc[w if sc.shape[0] > 1 else 0])
    with np.errstate(over="ignore", invalid="ignore"):
        for w in range(nw):
            l, s_, c_ = of(w)
            out[w, :, :n_mels] = B.normalise(np.full((1, n_mels), pad_value, np.float32), l, s_, c_)[0] if pad_mode == B.PAD_FEATURE else f32(pad_value)
    for seg, nrows, row0, w, offset in pieces:
        seg, nrows, row0, w, offset = int(seg), int(nrows), int(row0), int(w), int(offset)
        l, s_, c_ = of(w)
        # the window's affine at the piece's segment, in float32 and time-major: conversion and layout come last
        one = B.batch(x, start, [(seg, nrows, row0)], n_mels, up4(nrows), deltas, B.TIME, B.F32, lo=np.full(n, l, np.float32), shift=s_, scale=c_)
        out[w, offset:offset + nrows] = one[0, :nrows]
    if layout == B.CHANNEL:
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
    return B.convert(out, dtype)


def stats_grouped(x, start, group, ngroups):
    """-> (max float32 [ngroups], sum int64 [ngroups, n_mels], sumsq uint64 [ngroups, n_mels])"""
    x = np.asarray(x, np.float32)
    rows = [np.concatenate([x[start[i]:start[i + 1]] for i in range(len(start) - 1) if group[i] == g] + [x[:0]]) for g in range(ngroups)]
    bounds = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
    return B.stats(np.concatenate(rows + [x[:0]]), bounds)
