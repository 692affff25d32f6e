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


# ---- past one wave, one workgroup and one grid ------------------------------------------------------------------------------------
EDGE_RULE = (2, 3, 2, 3, 12, 0)                   # pads 2 / 3, joins across 2 frames, drops below 3, splits above 12
EDGE_NS = (63, 64, 65, 255, 256, 257, 600)
RICH = [(2, 30), (40, 5)]                         # under EDGE_RULE on 60 frames: [0, 35) in k = 3 pieces, then [38, 48)


def edge_rich(n):
    """the items that must produce a split and another record: either side of the wave and of the workgroup, and the last"""
    return sorted({i for i in (63, 64, 255, 256, n - 1) if i < n})


def edge_none(n):
    """the items that must produce nothing: item 0 (no frames), 61 (a record below min_frames), 62 (frames, no record) and, where
    there are as many items, 127 (a record, no frames) and 128 (two records that neither join nor survive) either side of a wave"""
    return sorted({i for i in (0, 61, 62, 127, 128) if i < n} - set(edge_rich(n)))


def edges(n, rng):
    """n items of 0 .. 60 frames with 0 .. 3 records each and a tail here and there, under EDGE_RULE: the prefix's cross-wave sums
    (n > 64) and its second round (n > 256), and init / count / fill with more than one workgroup"""
    nfs, rows, tails = [], [], {}
    rich, none = edge_rich(n), edge_none(n)
    for i in range(n):
        if i in rich:
            nfs.append(60)
            rows += [(i, f, L) for f, L in RICH]
        elif i in none:
            nfs.append({0: 0, 61: 20, 62: 33, 127: 0, 128: 30}[i])
            rows += {0: [], 61: [(i, 3, 2)], 62: [], 127: [(i, 0, 9)], 128: [(i, 5, 1), (i, 10, 2)]}[i]
        else:
            nf = int(rng.integers(0, 61))
            nfs.append(nf)
            t = int(rng.integers(-3, 8))
            for _ in range(int(rng.integers(0, 4)) if nf and rng.random() > 0.12 else 0):
                L = int(rng.integers(1, 26))
                rows.append((i, t, L))
                t += L + int(rng.integers(0, 9))
            if nf > 4 and i % 5 == 2:
                tails[i] = int(rng.integers(1, min(nf, 10) + 1))
    return case(f"edges{n}", nfs, rows, EDGE_RULE, rng, tails)


def per_item(c, want_rows):
    """the reference's records per item"""
    return np.bincount(want_rows["item"], minlength=len(c.start) - 1)


def edges_hold(c, w):
    """what `edges` is for, by the reference alone -> the caps to try"""
    n = len(c.start) - 1
    cnt = per_item(c, w)
    nf = np.diff(c.start)
    assert n in EDGE_NS and nf.max() <= 60 and np.bincount(c.table["item"], minlength=n).max() <= 3
    assert all(cnt[k:k + 64].sum() > 0 for k in range(0, n, 64)), "a wave that contributes nothing"
    for i in edge_rich(n):
        assert cnt[i] >= 2 and max(w["nframes"][w["item"] == i]) <= 12 and cnt[i] > len(RICH), (i, cnt[i])      # more pieces than groups: a split
    for i in edge_none(n):
        assert cnt[i] == 0, i
    assert (cnt == 0).sum() * 10 >= n and ((cnt == 0) & (nf == 0)).any() and ((cnt == 0) & (nf > 0)).any()
    if n == 600:
        assert cnt[:256].sum() > 0 and cnt[256:512].sum() > 0 and cnt[:256].sum() != cnt[256:512].sum()
    seen = refine_ref.census(c.table, c.tails, c.start, c.rule)
    assert min(seen.values()) >= 3, seen
    inside = min(256, n - 1)                       # a cap inside the output of item 256 (of the last item, where there are fewer)
    cap = int(cnt[:inside].sum()) + 2
    assert cnt[:inside].sum() < cap < cnt[:inside + 1].sum()
    return (len(w) + 3, len(w), cap)


WIDE = {"w199": (400, 401, 2, 99), "w499": (1000, 1001, 2, 249), "w133": (400, 801, 3, 66)}      # max_frames, length, k, h
WIDE_VARIANTS = ("min_lo", "min_63", "min_64", "min_hi", "tie_5_69", "tie_64_63", "tie_70_134", "head_rejected", "only_hi", "none")
LOW = np.float32(0.25)


def wide(name, rng):
    """windows wider than a wave: one segment alone in each item, seven frames from either end of it, every frame accepted with a
    probability of 0.5 .. 1 - and per item one variant of where the minimum LOW = 0.25 lies in each of the segment's windows
    [lo, hi] = [c - h, c + h] -> (case, [(item, variant, [expected boundary per window], [nominal cut per window])]).  A window of
    133 frames has no frame lo + 134: that variant is left out there.  w499 starts far from frame 0 of the arrays."""
    mf, length, k, h = WIDE[name]
    plan = refine_ref.split_plan(length, mf)
    assert plan[:2] == (k, h) and len(plan[2]) == k - 1
    variants = [v for v in WIDE_VARIANTS if v != "tie_70_134" or 2 * h >= 134]
    nfs = [length + 14] * len(variants)
    c = case(name, nfs, [(i, 7, length) for i in range(len(variants))], (0, 0, -1, 0, mf, 0), rng, bad=0.0,
             first=4112 if name == "w499" else 0)
    c.probs[:] = rng.uniform(0.5, 1.0, len(c.probs)).astype(np.float32)
    expect = []
    for i, v in enumerate(variants):
        base = int(c.start[i])
        hits = []
        for cut in plan[2]:
            lo, hi = 7 + cut - h, 7 + cut + h
            assert 0 <= lo and hi < nfs[i] and hi - lo == 2 * h

            def reject(a, b):
                c.events[base + a:base + b] |= 0x80
                c.probs[base + a:base + b] = np.nan

            low = {"min_lo": [lo], "min_63": [lo + 63], "min_64": [lo + 64], "min_hi": [hi], "tie_5_69": [lo + 69, lo + 5],
                   "tie_64_63": [lo + 64, lo + 63], "tie_70_134": [lo + 134, lo + 70], "head_rejected": [lo + 100], "only_hi": [], "none": []}[v]
            if v == "head_rejected":
                reject(lo, lo + 64)
            elif v == "only_hi":
                reject(lo, hi)
            elif v == "none":
                reject(lo, hi + 1)
            for t in low:
                assert lo <= t <= hi
                c.probs[base + t] = LOW
            hits.append(min(low) if low else hi if v == "only_hi" else 7 + cut)
        expect.append((i, v, hits, [7 + cut for cut in plan[2]]))
    return c, expect


def wide_holds(c, expect, w):
    """every boundary lands on its planted frame, away from the nominal cut except where the whole window is rejected"""
    for i, v, hits, nominal in expect:
        got = [int(f) for f in w["first_frame"][w["item"] == i]]
        assert got == [7] + hits, (c.name, v, got, hits)
        assert all((b != n0) == (v != "none") for b, n0 in zip(hits, nominal)), (c.name, v)
    seen = refine_ref.census(c.table, c.tails, c.start, c.rule, c.events, c.probs)
    assert seen["moved"] == sum(len(hits) for _, v, hits, _ in expect if v != "none"), seen


def many(rng):
    """more records than the capped grid of the cut kernel has waves: 44 items of 100 records of 21 frames, 2 .. 4 frames apart,
    each cut in two (k = 2, sz = 11, h = 4: windows of 9 frames) where the grid of probabilities has its first minimum"""
    nfs, rows = [], []
    for i in range(44):
        t = int(rng.integers(0, 4))
        for _ in range(100):
            rows.append((i, t, 21))
            t += 21 + int(rng.integers(2, 5))
        nfs.append(t + int(rng.integers(0, 3)))
    return case("many", nfs, rows, (0, 0, -1, 0, 20, 0), rng, ties=True)


GRID = 8192                                       # records the cut kernel's grid reaches without its stride: 2048 workgroups of 4 waves


def many_holds(c, w):
    assert refine_ref.split_plan(21, 20)[:2] == (2, 4)
    assert len(w) > GRID + 200 and len(c.start) - 1 >= 24 and int(c.start[-1]) > 100000
    seen = refine_ref.census(c.table, c.tails, c.start, c.rule, c.events, c.probs, index_range=(GRID, len(w)))
    assert seen["splits"] == len(c.table) and seen["moved_in_range"] >= 100 and seen["moved"] > 2000, seen
    return (len(w), GRID + 1)


HEAD_ROWS = (255, 256, 257, 512)


def heads(rng):
    """items whose first record is the first or the last row of a workgroup of the heads kernel, or next to one: item 0 holds rows
    0 .. 254, item 1 row 255, item 2 row 256, item 3 rows 257 .. 511, item 4 rows 512 .. 514; item 1 comes back in rows 515 and 516,
    on the far side of row 512 (a later run: absent), item 5 follows"""
    counts = [(0, 255), (1, 1), (2, 1), (3, 255), (4, 3), (1, 2), (5, 4)]
    rows, nfs = [], [0] * 6
    for it, k in counts:
        t = int(rng.integers(0, 5)) if nfs[it] == 0 else 2
        for q in range(k):
            L = int(rng.integers(1 if q else 2, 8))                              # a run of one record survives min_frames = 2
            rows.append((it, t, L))
            t += L + int(rng.integers(1, 7))
        nfs[it] = max(nfs[it], t + 3)
    return case("heads", nfs, rows, (2, 3, 2, 2, 9, 0), rng)


def heads_hold(c, w):
    items = c.table["item"].tolist()
    first = {it: items.index(it) for it in set(items)}
    assert [first[it] for it in (1, 2, 3, 4)] == list(HEAD_ROWS)
    for it in (1, 2, 3, 4):
        assert items[first[it] - 1] == it - 1                                   # the item before ends at the row just above
    assert items[515:517] == [1, 1] and first[5] == 517 and len(items) == 521
    # the later run is absent: the reference on the table without it gives the same, and not the same as with the run moved up
    assert w.tobytes() == refine_ref.refine(np.delete(c.table, [515, 516]), c.tails, c.events, c.probs, c.start, c.rule).tobytes()
    moved_up = np.concatenate([c.table[:256], c.table[515:517], c.table[256:515], c.table[517:]])
    assert w.tobytes() != refine_ref.refine(moved_up, c.tails, c.events, c.probs, c.start, c.rule).tobytes()
    cnt = per_item(c, w)
    assert cnt.min() >= 1 and min(refine_ref.census(c.table, c.tails, c.start, c.rule).values()) >= 1
    return (len(w) + 3, len(w) // 2)


BIT_VALUES = (0.0, 1e-45, 1e-40, 1.1754944e-38, 1.0)       # +0.0, the smallest denormal, a denormal, the smallest normal, 1.0


def bits(rng):
    """the cut key orders bit patterns, the reference values: items 0 .. 4, one segment of 21 frames at frame 8 under max_frames = 20
    (window [14, 22]).  Item 0's window holds all five values, +0.0 twice, the larger ones at the lower frames; item j's window
    holds BIT_VALUES[j:], so each value is the minimum of a window; item 4's only accepted frame is the 1.0
    -> (case, [expected boundary per item])"""
    c = case("bits", [40] * 5, [(i, 8, 21) for i in range(5)], (0, 0, -1, 0, 20, 0), rng, bad=0.0)
    assert refine_ref.split_plan(21, 20) == (2, 4, [10])
    c.probs[:] = rng.uniform(0.5, 0.99, len(c.probs)).astype(np.float32)
    where = {1.0: 14, 1.1754944e-38: 15, 1e-40: 16, 1e-45: 20, 0.0: 17}
    for i in range(5):
        base = int(c.start[i])
        for v in BIT_VALUES[i:]:
            c.probs[base + where[v]] = np.float32(v)
        if i == 0:
            c.probs[base + 21] = np.float32(0.0)                               # the second +0.0, behind the first
        if i == 4:
            for t in [t for t in range(14, 23) if t != 14]:
                c.events[base + t] |= 0x80
                c.probs[base + t] = np.nan
    assert not np.signbit(c.probs[~np.isnan(c.probs)]).any()
    assert np.float32(1e-45).view(np.uint32) == 1 and 0 < np.float32(1e-40) < np.float32(1.1754944e-38) == np.finfo(np.float32).tiny
    return c, [17, 20, 16, 15, 14]


def bits_hold(c, expect, w):
    assert [int(w["first_frame"][w["item"] == i][1]) for i in range(5)] == expect and len(w) == 10 and 18 not in expect


def negzero(rng):
    """outside the reference's rule (include/vad_engine.h, step 5): a caller's -0.0 and -0.5 order by bit pattern, above every
    non-negative probability and -0.5 above -0.0 -> (case, [(first_frame, nframes)] by hand).  Item 0: -0.0 at 15 and 0.75 at 19,
    the rest 0.875: the cut is 19.  Item 1: -0.5 at 15, -0.0 at 20, the rest rejected: the cut is 20."""
    c = case("negzero", [40] * 2, [(i, 8, 21) for i in range(2)], (0, 0, -1, 0, 20, 0), rng, bad=0.0)
    c.probs[:] = np.float32(0.875)
    c.probs[15], c.probs[19] = np.float32(-0.0), np.float32(0.75)
    for t in range(14, 23):
        c.events[40 + t] |= 0x80
    c.events[40 + 15] = c.events[40 + 20] = 0
    c.probs[40 + 15], c.probs[40 + 20] = np.float32(-0.5), np.float32(-0.0)
    return c, [(0, 8, 11), (0, 19, 10), (1, 8, 12), (1, 20, 9)]


PAST = [f"edges{n}" for n in EDGE_NS] + list(WIDE) + ["many", "heads", "bits"]
_past = {}


def past(name):
    """a case of the list above with its seed -> (case, the reference's table, the caps to try), every condition the case is for
    asserted on the reference alone; built once"""
    if name not in _past:
        rng = np.random.default_rng(700 + PAST.index(name))
        if name.startswith("edges"):
            c = edges(int(name[5:]), rng)
            w = want(c)
            caps = edges_hold(c, w)
        elif name in WIDE:
            c, expect = wide(name, rng)
            w = want(c)
            wide_holds(c, expect, w)
            caps = (len(w) + 3, len(w) // 2)
        elif name == "bits":
            c, expect = bits(rng)
            w = want(c)
            bits_hold(c, expect, w)
            caps = (len(w) + 3, len(w) // 2)
        else:
            c = {"many": many, "heads": heads}[name](rng)
            w = want(c)
            caps = {"many": many_holds, "heads": heads_hold}[name](c, w)
        _past[name] = (c, w, caps)
    return _past[name]


def every_cap(c, w):
    """caps 0 .. len(w) of the `splits` case: the caps that end on the first, a middle and the last piece of its k = 7 group"""
    assert c.name == "splits" and len(w) < 40
    seven = np.flatnonzero(w["item"] == 1)
    assert len(seven) == 7 and refine_ref.split_plan(139, 20)[0] == 7
    caps = list(range(len(w) + 1))
    assert {int(seven[0]) + 1, int(seven[3]) + 1, int(seven[6]) + 1} <= set(caps)
    return caps


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
