"""Synthetic inputs for the refinement's device form (vad_refine_device), shared by tests/test_scan_refine_host.py (the stand-in, whose
"device" pointers are host memory) and tests/test_gpu_scan_refine.py: per-frame arrays, a table, tails and a rule per case, every
shape chosen on the CPU and checked against tests/refine_ref.py's census so that no case is vacuous.  No test, no library."""
from collections import namedtuple

import numpy as np

from tests import refine_ref

DTYPE = refine_ref.DTYPE
SENT = 0x5A
Case = namedtuple("Case", "name start events probs table tails rule nsegs in_cap")


def aligned(n, dtype, fill=None):
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 32, np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:n * item].view(dtype)
    if fill is not None:
        a.view(np.uint8)[:] = fill
    return a


def frames(rng, total, ties=False, bad=0.03):
    """events and probs [total]: random START / END / CONTINUE bits (the refinement reads none of them), `bad` of the frames rejected
    with a NaN probability; ties: probabilities on a grid of 1 / 8, so that windows hold equal minima"""
    probs = rng.uniform(0.0, 1.0, total).astype(np.float32)
    if ties:
        probs = (np.floor(probs * 8) / 8).astype(np.float32)
    ev = rng.choice([0, 1, 2, 4, 6], total).astype(np.uint8)
    rej = rng.random(total) < bad
    ev[rej] |= 0x80
    probs[rej] = np.nan
    return ev, probs


def table_of(rows):
    t = np.zeros(len(rows), DTYPE)
    for k, (i, f, L) in enumerate(rows):
        t[k] = (i, f, L, 7, 0.25, 0.5)          # statistics that are not the answer
    return t


def case(name, nfs, rows, rule, rng, tails=None, ties=False, bad=0.03, nsegs=None, in_cap=None, first=0):
    start = first + np.concatenate([[0], np.cumsum(nfs)]).astype(np.int64)
    ev, probs = frames(rng, int(start[-1]), ties, bad)
    tl = None
    if tails is not None:
        tl = np.zeros(len(nfs), DTYPE)
        for i, L in tails.items():
            tl[i] = (i, nfs[i] - L, L, 3, 0.5, 0.75)
    return Case(name, start, ev, probs, table_of(rows), tl, tuple(rule), len(rows) if nsegs is None else nsegs, len(rows) if in_cap is None else in_cap)


def random_rows(rng, nfs):
    """per item 0, 1 or a few records in frame order: gaps of 0 .. 12 frames, now and then an overlap, a first record that starts
    before frame 0 and a last one that runs past the item"""
    rows = []
    for i, nf in enumerate(nfs):
        count = 0 if nf == 0 or i % 7 == 3 else 1 if i % 5 == 1 else int(rng.integers(2, 9))
        t = int(rng.integers(-6, 10))
        for _ in range(count):
            L = int(rng.integers(1, 60))
            rows.append((i, t, L))
            t += L + int(rng.integers(-2, 13))
            if t >= nf + 5:
                break
    return rows


def corpus37(rng, rule, with_tails=True, ties=False):
    """37 items of 0 .. ~400 frames - 0, 1 and 400 among them, empty items, items with no and with one record"""
    nfs = [0, 1, 400, 2, 0, 397] + [int(v) for v in rng.integers(3, 400, 31)]
    rows = random_rows(rng, nfs)
    tails = {i: int(rng.integers(1, min(nfs[i], 50) + 1)) for i in range(len(nfs)) if nfs[i] and i % 3 == 0} if with_tails else None
    return case("corpus37", nfs, rows, rule, rng, tails, ties)


def chain(rng):
    """item 1: 330 records of 2 frames, a frame apart - one merge chain, longer than a wave and a workgroup - then a lone record"""
    rows = [(0, 4, 9)] + [(1, 3 * k, 2) for k in range(330)] + [(1, 1010, 6), (2, 0, 5)]
    return case("chain", [30, 1030, 12], rows, (2, 3, 1, 0, 200, 0), rng)


def pads(rng):
    """pad sharing: gaps of 5 (odd), 4 (even), 1, and - merge_gap = -1 - 0 and below 0; pad_before != pad_after; padding clipped at
    frame 0 and at nf; a record that starts before frame 0"""
    rows = [(0, 2, 10), (0, 17, 6), (0, 27, 5), (0, 33, 4), (0, 37, 8), (0, 40, 10), (0, 96, 3),
            (1, -4, 9), (1, 30, 8),
            (2, 0, 50)]
    return case("pads", [100, 40, 50], rows, (4, 3, -1, 0, 0, 0), rng)


def drops(rng):
    """min_frames = 6: groups of 5 frames go, groups of 6 stay - a single record of each, and two records that reach either by merging"""
    rows = [(0, 3, 5), (0, 20, 6), (0, 40, 2), (0, 43, 2), (0, 60, 2), (0, 63, 3), (0, 80, 1)]
    return case("drops", [100], rows, (1, 1, 1, 6, 0, 0), rng)


def splits(rng, ties=True):
    """max_frames = 20: lengths 21 (k = 2), 40 (k = 2, h = 0), 41 (k = 3), 139 (k = 7), 20 (none); equal minima from the grid of
    probabilities; item 3's second window is rejected as a whole, its first in part"""
    rows = [(0, 5, 21), (0, 40, 40), (0, 100, 41), (1, 1, 139), (2, 0, 20), (3, 10, 50)]
    c = case("splits", [150, 141, 20, 70], rows, (0, 0, -1, 0, 20, 0), rng, ties=ties)
    base = int(c.start[3])
    k, h, cuts = refine_ref.split_plan(50, 20)
    assert (k, h) == (3, 1)
    for t in range(10 + cuts[1] - h, 10 + cuts[1] + h + 1):
        c.events[base + t] |= 0x80
        c.probs[base + t] = np.nan
    c.events[base + 10 + cuts[0]] |= 0x80
    c.probs[base + 10 + cuts[0]] = np.nan
    for t in (10 + cuts[0] - 1, 10 + cuts[0] + 1):
        c.events[base + t] &= 0x7F
        c.probs[base + t] = np.float32(0.375)              # equal minima either side of a rejected nominal cut
    return c


def pairs(rng):
    """max_frames = 2: every piece is 1 or 2 frames, h = 0 throughout"""
    return case("pairs", [64, 9], [(0, 1, 61), (1, 0, 9)], (0, 0, -1, 0, 2, 0), rng)


def garbage(rng):
    """a device table no call wrote: an item out of range either way, nframes = 0 and below, an item that comes back after another,
    records far outside their items, a count above in_cap"""
    rows = [(0, 2, 5), (0, 10, 0), (0, 12, -3), (0, 20, 4), (7, 0, 5), (-1, 0, 5), (0, 30, 5), (2, 1, 6), (2, 1 << 30, 1 << 30),
            (2, -(1 << 31), 5), (2, 2147483647, 2147483647), (2, 9, 4), (1, 0, 4), (2, 20, 3), (3, 5, 5), (3, 0, 2), (99999, 1, 1)]
    return case("garbage", [40, 10, 60, 12], rows + [(3, 9, 2)], (2, 2, 3, 0, 7, 0), rng, nsegs=1 << 40, in_cap=len(rows), first=16)


def ptr(a):
    return None if a is None else a.ctypes.data


def run(eng, c, cap, dev=None, back=None, sync=None):
    """the device form on a case, the output buffer between canaries -> (count, the records written, canaries intact).  dev(array) ->
    (handle, address) puts an array where the engine's kernels read it, back(handle) -> numpy brings it home (default: host memory,
    for the stand-in)."""
    dev = dev or (lambda a: (a, a.ctypes.data))
    back = back or (lambda h: h)
    put = lambda a, dt: dev(np.ascontiguousarray(a, dt) if a is not None and len(a) else np.zeros(1, dt))
    h_ev, p_ev = put(c.events, np.uint8)
    h_pr, p_pr = put(c.probs, np.float32)
    h_in, p_in = put(c.table, DTYPE)
    h_tl, p_tl = put(c.tails, DTYPE) if c.tails is not None else (None, 0)
    h_n, p_n = dev(np.asarray([c.nsegs], np.int64))
    out = np.zeros(cap + 4, DTYPE)
    out.view(np.uint8)[:] = SENT
    h_out, p_out = dev(out)
    h_cnt, p_cnt = dev(np.asarray([-7, -7, -7], np.int64))
    eng.refine_device(p_in, p_n, c.in_cap, p_tl, p_ev, p_pr, c.start, c.rule, p_out + 48, cap, p_cnt + 8)
    (sync or eng.synchronize)()
    cnt = back(h_cnt)
    got = back(h_out)
    count = int(cnt[1])
    k = min(count, cap)
    raw = got.view(np.uint8).reshape(-1, 24)
    clean = cnt[0] == -7 and cnt[2] == -7 and bool((raw[:2] == SENT).all()) and bool((raw[2 + k:] == SENT).all())
    # the inputs are inputs
    clean = clean and back(h_in).tobytes() == (np.ascontiguousarray(c.table) if len(c.table) else np.zeros(1, DTYPE)).tobytes()
    return count, np.ascontiguousarray(got[2:2 + k]), clean


def want(c):
    rows = c.table[:min(c.nsegs, c.in_cap)]
    return refine_ref.refine(rows, c.tails, c.events, c.probs, c.start, c.rule)
