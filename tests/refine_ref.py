"""The numpy reference of the refinement (vad_refine_device, vad_scan_refine; include/vad_engine.h: vad_refine) for
tests/test_scan_refine_host.py (CPU stand-in) and tests/test_gpu_scan_refine.py: the six steps of the header's text, one after the
other on whole lists, the statistics by cutter_vad_amd.scan._frame_stats' fixed-point formula - never the code under test.  It is
the rule for probabilities with the sign bit clear, which is what the engine's kernels write: step 5 compares values (np.argmin),
and the header's order of a caller's negative values and -0.0 - by bit pattern, above every non-negative one - is not stated here.
No test, no library: importing it loads neither the stand-in nor the engine."""
import numpy as np

DTYPE = np.dtype([("item", np.int32), ("first_frame", np.int32), ("nframes", np.int32), ("counted", np.int32),
                  ("mean_prob", np.float32), ("max_prob", np.float32)])
REJECTED = 0x80
NEUTRAL = (0, 0, -1, 0, 0, 0)


def rule_of(rule):
    """a SegmentRefine, or a 6-sequence in the struct's order -> (pad_before, pad_after, merge_gap, min_frames, max_frames)"""
    if hasattr(rule, "pad_before"):
        rule = (rule.pad_before, rule.pad_after, rule.merge_gap, rule.min_frames, rule.max_frames, rule.reserved)
    return tuple(int(v) for v in rule)[:5]


def item_records(table, n):
    """per item, its records (first_frame, nframes) in table order.  A sorted table: every record that names the item.  Any other
    (the device form): the item's first run - from the first record that names it behind one that does not, to the next record of
    another item value."""
    items = [int(v) for v in table["item"]]
    rows = list(zip(items, table["first_frame"].tolist(), table["nframes"].tolist()))
    out = [[] for _ in range(n)]
    seen = set()
    for r, (it, f, L) in enumerate(rows):
        if not 0 <= it < n:
            continue
        head = r == 0 or items[r - 1] != it
        if head and it in seen:
            continue                     # a later run
        if head:
            seen.add(it)
            k = r
            while k < len(rows) and items[k] == it:
                out[it].append((rows[k][1], rows[k][2]))
                k += 1
    return out


def split_plan(length, max_frames):
    """step 5 without the probabilities: (k, h, [c_1 .. c_{k-1}]) relative to the segment's start"""
    k = -(-length // max_frames)
    sz = -(-length // k)
    return k, (max_frames - sz) // 2, [j * length // k for j in range(1, k)]


def refine_item(records, nf, rule, probs, events):
    """steps 1 - 5 on ONE item: records [(first_frame, nframes)], the tail last -> [(first_frame, nframes)]"""
    pb, pa, gap, min_frames, max_frames = rule_of(rule)
    clipped = []
    for f, L in records:                                                       # 1
        s, e = max(f, 0), min(f + L, nf)
        if L >= 1 and s < e:
            clipped.append((s, e))
    groups = []
    for q, (s, e) in enumerate(clipped):                                       # 2
        if q and gap >= 0 and s - clipped[q - 1][1] <= gap:
            groups[-1] = (groups[-1][0], e)
        else:
            groups.append((s, e))
    kept = [(s, e) for s, e in groups if e - s >= 1 and e - s >= min_frames]   # 3
    padded = []
    for q, (s, e) in enumerate(kept):                                          # 4
        left, right = pb, pa
        if q:
            g = s - kept[q - 1][1]
            if g < pb + pa:
                left = 0 if g <= 0 else g - g * pa // (pb + pa)
        if q + 1 < len(kept):
            g = kept[q + 1][0] - e
            if g < pb + pa:
                right = 0 if g <= 0 else g * pa // (pb + pa)
        padded.append((max(s - left, 0), min(e + right, nf)))
    out = []
    for s, e in padded:                                                        # 5
        if max_frames <= 0 or e - s <= max_frames:
            out.append((s, e - s))
            continue
        k, h, cuts = split_plan(e - s, max_frames)
        bounds = [s]
        for c in cuts:
            c += s
            lo, hi = max(c - h, 0), min(c + h, nf - 1)
            ok = np.flatnonzero((events[lo:hi + 1] & REJECTED) == 0)
            # argmin: the first of equals.  By VALUE: the rule for probabilities with the sign bit clear, which is what every kernel
            # of the engine writes (+0.0, denormals and 1.0 included: value and bit pattern order them alike).  The header orders a
            # caller's negative values and -0.0 by bit pattern, above every non-negative one; this reference does not state that case.
            bounds.append(c if ok.size == 0 else lo + int(ok[np.argmin(probs[lo:hi + 1][ok])]))
        bounds.append(e)
        out += [(a, b - a) for a, b in zip(bounds, bounds[1:])]
    return out


def stats(probs, events, first_frame, nframes):
    """cutter_vad_amd.scan._frame_stats' formula over the frames max(first_frame, 0) .. first_frame + nframes - 1 of ONE item"""
    t0 = max(first_frame, 0)
    p = probs[t0:first_frame + nframes][(events[t0:first_frame + nframes] & REJECTED) == 0]
    if p.size == 0:
        return 0, np.float32(0), np.float32(0)
    fixed = int(np.rint(p.astype(np.float64) * 2.0 ** 30).astype(np.int64).sum())
    return p.size, np.float32(fixed / (p.size * 2.0 ** 30)), p.max()


def refine(table, tails, events, probs, out_start, rule):
    """the whole call: table (DTYPE), tails (DTYPE [n]) or None, the flat per-frame arrays and out_start [n + 1] -> the refined table"""
    events, probs = np.asarray(events, np.uint8), np.asarray(probs, np.float32)
    start = np.asarray(out_start, np.int64)
    n = max(start.size - 1, 0)
    per = item_records(table, n)
    rows = []
    for i in range(n):
        recs = list(per[i])
        if tails is not None and int(tails["nframes"][i]) > 0:
            recs.append((int(tails["first_frame"][i]), int(tails["nframes"][i])))
        ev, pr = events[start[i]:start[i + 1]], probs[start[i]:start[i + 1]]
        for f, L in refine_item(recs, int(start[i + 1] - start[i]), rule, pr, ev):
            rows.append((i, f, L) + stats(pr, ev, f, L))
    return np.array(rows, DTYPE)


def census(table, tails, out_start, rule, events=None, probs=None, index_range=None):
    """what a rule does to a table, by the reference alone: the number of merges (records that joined a predecessor), drops, pairs
    of neighbours that shared a gap, and segments that were split.  With the per-frame arrays also `moved`: the boundaries of step 5
    with b_j != c_j - and `moved_in_range`, those among them whose piece [b_j, b_j+1) has an output index in index_range = (lo, hi),
    lo <= index < hi"""
    pb, pa, gap, min_frames, max_frames = rule_of(rule)
    start = np.asarray(out_start, np.int64)
    n = max(start.size - 1, 0)
    per = item_records(table, n)
    seen = {"merges": 0, "drops": 0, "shared": 0, "splits": 0}
    if probs is not None:
        events, probs = np.asarray(events, np.uint8), np.asarray(probs, np.float32)
        seen["moved"] = seen["moved_in_range"] = 0
    lo_idx, hi_idx = index_range if index_range is not None else (0, 1 << 62)
    at = 0
    for i in range(n):
        nf = int(start[i + 1] - start[i])
        recs = list(per[i])
        if tails is not None and int(tails["nframes"][i]) > 0:
            recs.append((int(tails["first_frame"][i]), int(tails["nframes"][i])))
        dummy_p, dummy_e = np.zeros(nf, np.float32), np.zeros(nf, np.uint8)
        if probs is not None:           # a window of rejected frames leaves the nominal cut: the same pieces, every b_j = c_j
            real = refine_item(recs, nf, rule, probs[start[i]:start[i + 1]], events[start[i]:start[i + 1]])
            nominal = refine_item(recs, nf, rule, dummy_p, dummy_e | REJECTED)
            assert len(real) == len(nominal)
            for j, ((b, _), (c, _)) in enumerate(zip(real, nominal)):
                seen["moved"] += b != c
                seen["moved_in_range"] += b != c and lo_idx <= at + j < hi_idx
            at += len(real)
        merged = refine_item(recs, nf, (0, 0, gap, 0, 0, 0), dummy_p, dummy_e)
        present = refine_item(recs, nf, NEUTRAL, dummy_p, dummy_e)
        kept = refine_item(recs, nf, (0, 0, gap, min_frames, 0, 0), dummy_p, dummy_e)
        padded = refine_item(recs, nf, (pb, pa, gap, min_frames, 0, 0), dummy_p, dummy_e)
        seen["merges"] += len(present) - len(merged)
        seen["drops"] += len(merged) - len(kept)
        seen["shared"] += sum(1 for (s, L), (s2, _) in zip(kept, kept[1:]) if 0 < s2 - (s + L) < pb + pa)
        seen["splits"] += sum(1 for s, L in padded if max_frames > 0 and L > max_frames)
    return seen


def same(got, want):
    """record for record, the statistics bit for bit"""
    return got.dtype == DTYPE and want.dtype == DTYPE and got.shape == want.shape and got.tobytes() == want.tobytes()
