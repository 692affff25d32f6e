"""Hand-built per-frame arrays for the replay's device form (vad_resegment_device), shared by tests/test_scan_resegment_host.py (the
stand-in) and tests/test_gpu_scan_resegment.py: item counts around a wave (64) and a workgroup (256) of vadk_reseg_prefix, items of
0 .. 12 frames so that the replay's groups of four end in every remainder, ENDs on the last frames of items - every shape chosen on
the CPU and checked against tests/reseg_ref.py so that no case is vacuous.  No test, no library."""
import numpy as np

from tests import reseg_ref

NS = (63, 64, 65, 256, 257, 600)
# a START after 1 - 2 high frames and an END after 1 - 3 low ones, so that items of a few frames hold segments; NEVER starts nowhere
NEVER = (0.99, 0.98, 1.0, 1.0, 19, 60)
SETS = [(0.5, 0.5, 0.5, 0.95, 1, 1), (0.5, 0.5, 0.8, 0.95, 2, 2), (0.6, 0.4, 0.7, 0.9, 1, 3), NEVER, (0.3, 0.2, 0.9, 0.85, 2, 1)]
FIRE = [0, 1, 2, 4]


def sets64():
    """the five sets repeated with small changes in the probabilities and END counts of 1 .. 3"""
    out = []
    for k in range(64):
        a, b, c, d, m, n = SETS[k % 5]
        j = k // 5
        out.append((a - 0.004 * j, b - 0.003 * j, c, d, m, 1 + (n - 1 + j) % 3))
    return out


def arrays(n, rng):
    """-> (events, probs, out_start).  Item i has (5 i) mod 13 frames - every length 0 .. 12 in every run of 13 items - and one of
    four shapes by i // 13: high frames, then 1, 2 or 3 low ones (an END of the set with that voice_end_frame_count on the item's
    LAST frame), or random runs of 1 .. 3 frames at levels between the sets' thresholds.  The last item holds a segment of every set
    that can fire.  Every 17th item of five frames or more has a rejected fourth frame with a NaN probability."""
    probs, start = [], [0]
    hi = lambda k: rng.choice(np.asarray([0.9, 0.75, 0.65], np.float32), k)
    lo = lambda k: rng.choice(np.asarray([0.02, 0.1, 0.15], np.float32), k)
    for i in range(n):
        nf, shape = (5 * i) % 13, (i // 13) % 4
        if i == n - 1:
            p = np.concatenate([lo(1), hi(8), lo(3)])
        elif shape < 3 and nf >= shape + 3:
            p = np.concatenate([hi(nf - shape - 1), lo(shape + 1)])
        else:
            p, voiced = np.zeros(0, np.float32), bool(rng.integers(2))
            while len(p) < nf:
                k = int(rng.integers(1, 4))
                p = np.concatenate([p, rng.choice(np.asarray([0.9, 0.55, 0.45, 0.35] if voiced else [0.05, 0.25, 0.45], np.float32), k)])
                voiced = not voiced
            p = p[:nf]
        probs.append(p.astype(np.float32))
        start.append(start[-1] + len(p))
    probs = np.concatenate(probs + [np.zeros(0, np.float32)]).astype(np.float32)
    start = np.asarray(start, np.int64)
    ev = rng.choice(np.asarray([0, 1, 2, 4, 6], np.uint8), len(probs)).astype(np.uint8)      # bits that mean nothing to a replay
    for i in range(5, n, 17):
        if start[i + 1] - start[i] >= 5:
            ev[start[i] + 3] |= 0x80
            probs[start[i] + 3] = np.nan
    return ev, probs, start


_built = {}


def built(n, nsets=5):
    """-> (events, probs, out_start, sets, the reference's table per set, caps), the conditions below asserted on the reference
    alone; built once"""
    if (n, nsets) not in _built:
        ev, probs, start = arrays(n, np.random.default_rng(900 + n))
        sets = {1: SETS[1:2], 5: SETS, 64: sets64()}[nsets]
        want = reseg_ref.tables(ev, probs, start, sets)
        _built[(n, nsets)] = (ev, probs, start, sets, want, hold(n, ev, probs, start, sets, want))
    return _built[(n, nsets)]


def hold(n, ev, probs, start, sets, want):
    nf = np.diff(start)
    assert n in NS and nf.max() == 12 and set((nf % 4).tolist()) == {0, 1, 2, 3} and (nf == 0).any()
    fire = [k for k, w in enumerate(want) if len(w)]
    if len(sets) == 5:
        assert fire == FIRE
    assert len(fire) >= (40 if len(sets) == 64 else 1)
    for k in fire:                                  # records either side of every wave and workgroup edge the prefix has
        items = want[k]["item"]
        for edge in (64, 256, 512):
            if n > edge:
                assert (items < edge).any() and (items >= edge).any(), (k, edge)
        assert (items == n - 1).any()
    if len(sets) > 1:
        assert len({want[k].tobytes() for k in fire}) >= 2
    counts = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    assert all(counts[k + 1] > 0 for k in fire)     # the set behind a non-empty one starts above 0
    # ENDs in the remainder loop of the replay, behind a full group of four: END frame = first_frame + nframes - 1
    ends = {(int(r["item"]), int(r["first_frame"] + r["nframes"] - 1)) for w in want for r in w}
    for r in (1, 2, 3):
        assert any(nf[i] > 4 and nf[i] % 4 == r and e >= nf[i] - r for i, e in ends), r
        assert any(nf[i] > 4 and nf[i] % 4 == r and e == nf[i] - 1 for i, e in ends), r            # ... and on the very last frame
        assert len(sets) == 1 or any(nf[i] > 4 and nf[i] % 4 == 3 and e == nf[i] - 1 - (3 - r) for i, e in ends), r  # each frame of a remainder of 3
    for whole in (4, 8):
        assert any(nf[i] == whole and e == whole - 1 for i, e in ends), whole
    bad = np.flatnonzero(ev & 0x80)
    assert len(bad) >= 3 and np.isnan(probs[bad]).all()
    inside = 0
    for k in bad:
        i = int(np.searchsorted(start, k, side="right")) - 1
        t = int(k - start[i])
        inside += any(int(r["item"]) == i and r["first_frame"] < t < r["first_frame"] + r["nframes"] - 1 for w in want for r in w)
    assert inside >= 3, inside
    total = int(counts[-1])
    caps = [total + 2, total - 1, 0]
    if len(sets) > 1:
        second = [k for k in range(1, len(sets)) if len(want[k])][0]
        caps.append(int(counts[second]) + max(1, len(want[second]) // 2))
        assert counts[second] < caps[-1] < counts[second + 1]
    return counts, caps
