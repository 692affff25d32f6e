"""The segment still open at a recording's last frame on the GPU (csrc/scan_tails.hip: vadk_tail_snapshot, vadk_seg_tails;
csrc/scan_resegment.hip: vadk_tails_reseg_count; vad_scan_tails, vad_scan_resegment_tails and the two device forms).  The bar is
BYTE equality with tests/tail_ref.py - the oracle's state machine, tests/seg_ref.py's statistics - on hand-built arrays that hit
every path of the kernels (item counts around a wave and a workgroup, tails around the statistics' stride of 64, rejected frames,
counted == 0, a seg_frames larger than its item), on prefixes of the speech clip cut behind a START and on an END, and - without
any reference - against the scan of the same prefix followed by silence."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import seg_ref, tail_ref
from tests.test_gpu_scan import GOLD, THR, _engine

pytestmark = pytest.mark.gpu

DEFAULTS = (0.7, 0.7, 0.8, 0.95, 10, 50)
ONE = (0.5, 0.5, 0.5, 0.95, 1, 50)               # a START on the first high frame (L = 1), no END inside the arrays below
SETS = [ONE, (0.6, 0.4, 0.7, 0.9, 3, 4), DEFAULTS, (0.99, 0.98, 1.0, 1.0, 19, 60), (0.3, 0.2, 0.9, 0.85, 2, 3)]      # five: padded to 8 lanes
SENT = 0x5A
TAILS = (1, 63, 64, 65, 129, 9000)


def sets64():
    out = []
    for k in range(64):
        a, b, c, d, m, n = SETS[k % 5]
        j = k // 5
        out.append((a - 0.004 * j, b - 0.003 * j, max(c - 0.01 * j, 0.1), max(d - 0.01 * j, 0.1), m + j % 3, n + j % 4))
    return out


def _same(got, want, what=""):
    assert seg_ref.same(np.ascontiguousarray(got), np.ascontiguousarray(want)), (what, got[:4], want[:4])


# ---- hand-built arrays ------------------------------------------------------------------------------------------------
def _items(n, special, longest=9000):
    """n items as (head, probs, rejected): `head` = probabilities the item's slot has seen before (a continued slot), `probs` the
    item's frames, `rejected` the indices of its rejected frames.  Items of 0 .. 3 frames; every fourth enters inside a segment
    longer than itself.  special: the last 11 are the long tails (5 low frames, then T high ones), a tail that is the whole item,
    a rejected frame inside a tail and one on the last frame, counted == 0, and a seg_frames far larger than its item."""
    rng = np.random.default_rng(100 + n)
    hi = lambda k: rng.uniform(0.55, 0.95, k).astype(np.float32)
    lo = lambda k: rng.uniform(0.0, 0.4, k).astype(np.float32)
    items = []
    for i in range(n - (11 if special else 0)):
        k = i % 4
        p = np.where(rng.random(k) < 0.7, hi(k), lo(k)).astype(np.float32)
        head = hi(1 + i % 13) if i % 4 == 3 else np.zeros(0, np.float32)
        items.append((head, p, [1] if (i % 16 == 7 and k > 1) else []))
    if special:
        none = np.zeros(0, np.float32)
        for T in TAILS:
            if T <= longest:
                items.append((none, np.concatenate([lo(5), hi(T)]), []))
            else:
                items.append((none, hi(2), []))
        items.append((none, hi(64), []))                                    # the whole item
        items.append((none, np.concatenate([lo(3), hi(70)]), [40]))         # a rejected frame inside the tail
        items.append((none, np.concatenate([lo(3), hi(66)]), [68]))         # ... and as the last frame
        items.append((hi(10), hi(2), [0, 1]))                               # a tail none of whose frames counts
        items.append((hi(200), hi(3), []))                                  # seg_frames = 203 on an item of 3 frames
    assert len(items) == n
    return items


def _arrays(items):
    probs = np.concatenate([p for _, p, _ in items] + [np.zeros(0, np.float32)]).astype(np.float32)
    start = np.concatenate([[0], np.cumsum([len(p) for _, p, _ in items])]).astype(np.int64)
    ev = np.zeros(len(probs), np.uint8)
    ev[::3] |= 0x04                                                         # bits that mean nothing to the tails
    for (_, _, bad), lo in zip(items, start[:-1]):
        for b in bad:
            ev[lo + b] |= 0x80
            probs[lo + b] = np.nan
    return ev, probs, start


def _slot_want(items, ev, probs, start, thr):
    from oracle import oracle
    machines = [tail_ref.step_item(oracle.StateMachine(*thr), [0] * len(h), h) for h, _, _ in items]
    return tail_ref.tails(ev, probs, start, machines)


def _prime(eng, slots, items, thr):
    """every slot where a scan of its item would leave it: the head, then the item's accepted frames"""
    eng.set_thresholds_many(slots, thr)
    for s, (head, p, bad) in zip(slots, items):
        seen = np.concatenate([head, np.delete(p, bad)]).astype(np.float32)
        if len(seen):
            eng.debug_sm_replay(int(s), seen)


def _device(eng, items, thr, sets):
    """both device forms on the arrays of `items` -> (tails of the slots, tails per set), each with the bytes behind them"""
    import torch
    ev, probs, start = _arrays(items)
    n = len(items)
    slots = np.asarray(eng.open_streams(n))[::-1].copy()                    # not the identity
    try:
        _prime(eng, slots, items, thr)
        d_ev = torch.from_numpy(ev).cuda() if len(ev) else torch.zeros(16, dtype=torch.uint8, device="cuda")
        d_p = torch.from_numpy(probs).cuda() if len(probs) else torch.zeros(4, dtype=torch.float32, device="cuda")
        a = torch.full(((n + 2) * 24,), SENT, dtype=torch.uint8, device="cuda")
        b = torch.full(((len(sets) * n + 2) * 24,), SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.tails_device(slots, d_ev.data_ptr(), d_p.data_ptr(), start, a.data_ptr())
        eng.resegment_tails_device(d_ev.data_ptr(), d_p.data_ptr(), start, sets, b.data_ptr())
        eng.synchronize()
        a, b = a.cpu().numpy(), b.cpu().numpy()
    finally:
        for s in slots:
            eng.close_stream(int(s))
    assert (a[n * 24:] == SENT).all() and (b[len(sets) * n * 24:] == SENT).all()
    got = b[:len(sets) * n * 24].view(seg_ref.DTYPE)
    return (ev, probs, start), a[:n * 24].view(seg_ref.DTYPE), [got[k * n:(k + 1) * n] for k in range(len(sets))]


@pytest.fixture(scope="module")
def engine():
    eng = _engine(16000, max_streams=512)
    yield eng
    eng.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_device_forms_on_hand_built_arrays(engine, n):
    special = n == 300
    items = _items(n, special) if n > 1 else [(np.zeros(0, np.float32), np.asarray([0.1, 0.9, 0.8, 0.9], np.float32), [2])]
    sets = SETS if n != 64 else SETS[:1]
    (ev, probs, start), by_slot, by_set = _device(engine, items, ONE, sets)
    want = _slot_want(items, ev, probs, start, ONE)
    fresh = tail_ref.fresh(ev, probs, start, sets)
    print(f"tails [n = {n}]: {int((want['nframes'] > 0).sum())} tails of the slots, per set {[int((w['nframes'] > 0).sum()) for w in fresh]}")
    if special:
        rows = want[-11:]
        assert rows["nframes"].tolist() == list(TAILS) + [64, 69, 65, 10, 203]
        assert rows["first_frame"].tolist() == [5] * 6 + [0, 4, 4, -8, -200]       # a rejected frame is no step: nf - L moves up by one
        assert rows["counted"].tolist() == list(TAILS) + [64, 68, 64, 0, 3] and rows[9]["mean_prob"] == 0.0 == rows[9]["max_prob"]
        assert fresh[0][-11:]["nframes"].tolist() == list(TAILS) + [64, 69, 65, 0, 3] and not fresh[3]["nframes"].any()
    if n >= 63:
        assert (want["first_frame"] < 0).any() and (want["nframes"] == 0).any() and (np.diff(start) == 0).any()
        assert want[want["nframes"] == 0].tobytes() == bytes(24 * int((want["nframes"] == 0).sum()))
    else:
        assert want[0].tolist()[:4] == (0, 2, 2, 1)                      # START at frame 1, frame 2 rejected: L = 2 behind frame 3
    _same(by_slot, want, "slots")
    for k, (g, w) in enumerate(zip(by_set, fresh)):
        _same(g, w, f"set {k}")


def test_sixty_four_sets_one_wave_per_item(engine):
    items = _items(76, True, longest=129)
    sets = sets64()
    (ev, probs, start), _, by_set = _device(engine, items, ONE, sets)
    fresh = tail_ref.fresh(ev, probs, start, sets)
    assert len({w.tobytes() for w in fresh}) >= 8
    for k, (g, w) in enumerate(zip(by_set, fresh)):
        _same(g, w, f"set {k}")


def test_the_device_forms_on_a_v4_engine():
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(4, 16000), "rb") as f:
        v4 = Engine(f.read(), model_version=4, max_streams=128, sample_rate=16000)
    try:
        items = _items(76, True, longest=129)
        (ev, probs, start), by_slot, by_set = _device(v4, items, ONE, SETS)
        _same(by_slot, _slot_want(items, ev, probs, start, ONE), "slots")
        for k, (g, w) in enumerate(zip(by_set, tail_ref.fresh(ev, probs, start, SETS))):
            _same(g, w, f"set {k}")
    finally:
        v4.close()


# ---- the speech clip ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    eng, twin = _engine(16000, max_streams=128), _engine(16000, max_streams=128)
    yield eng, twin
    eng.close()
    twin.close()


def _clip(kind, sr=16000):
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"]
    if sr != 16000:
        pcm = pcm[(np.arange(pcm.size * sr // 16000) * 16000) // sr]        # the 16 kHz sample under every input sample
    return pcm.copy() if kind == "i16" else (pcm.astype(np.float32) / np.float32(32768.0))


def _per_frame(twin, recs, hop, thr, **kw):
    """Engine.scan on freshly opened streams -> flat events, probs, out_start"""
    slots = twin.open_streams(len(recs))
    try:
        twin.set_thresholds_many(slots, thr)
        probs, ev, _ = twin.scan(slots, recs, hop=hop, **kw)
    finally:
        for s in slots:
            twin.close_stream(int(s))
    start = np.concatenate([[0], np.cumsum([len(p) for p in probs])]).astype(np.int64)
    return np.concatenate([np.asarray(e, np.uint8) for e in ev]), np.concatenate([np.asarray(p, np.float32) for p in probs]), start


_prefix_cache = {}


def _prefixes(twin, kind, hop, sr=16000):
    """prefixes of the clip that end 1, 12 and 60 frames behind a START of its own scan and one that ends on an END frame, from
    two STARTs each -> (recordings, their frame counts)"""
    key = (kind, hop, sr)
    if key not in _prefix_cache:
        x = _clip(kind, sr)
        frame = 512 * sr // 16000
        kw = {} if sr == 16000 else {"sample_rate": sr}
        ev, _, _ = _per_frame(twin, [x], hop, THR, denoise=0.01, **kw)
        starts, ends = np.flatnonzero(ev & 1), np.flatnonzero((ev & 0x82) == 2)
        assert len(starts) >= 2 and len(ends) >= 1, (len(starts), len(ends))
        counts = sorted({int(s) + 1 + k for s in (starts[0], starts[len(starts) // 2]) for k in (1, 12, 60) if s + 1 + k <= len(ev)}
                        | {int(ends[0]) + 1, int(starts[-1]) + 1})
        _prefix_cache[key] = ([x[:frame + (c - 1) * hop].copy() for c in counts], counts)
    return _prefix_cache[key]


@pytest.mark.parametrize("kind,hop,sr", [("i16", 256, 16000), ("f32", 256, 16000), ("i16", 512, 16000), ("f32", 512, 16000), ("f32", 768, 48000)])
def test_scan_tails_of_clip_prefixes_equal_the_reference(engines, kind, hop, sr):
    eng, twin = engines
    kw = {} if sr == 16000 else {"sample_rate": sr}
    recs, counts = _prefixes(twin, kind, hop, sr)
    ev, probs, start = _per_frame(twin, recs, hop, THR, denoise=0.01, **kw)
    assert np.diff(start).tolist() == counts
    want = tail_ref.fresh(ev, probs, start, [THR, DEFAULTS])
    print(f"scan_tails [{kind}, hop {hop}, {sr} Hz]: frames {counts}, tails {want[0]['nframes'].tolist()}")
    assert (want[0]["nframes"] > 0).sum() >= 2 and (want[0]["nframes"] == 0).any()      # behind a START; on an END
    slots = eng.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, THR)
        with eng.scan_session():
            table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01, **kw)
            info = eng.info()
            got = eng.scan_tails()
            _same(got, want[0], "scan_tails")
            eng.reset(slots)                                                 # the snapshot is the scan's
            _same(eng.scan_tails(), want[0], "scan_tails behind a reset")
            for g, w in zip(eng.resegment_tails([THR, DEFAULTS]), want):
                _same(g, w, "resegment_tails")
            assert (eng.info()["steps"], eng.info()["frames"]) == (info["steps"], info["frames"])
            _same(eng.resegment([THR])[0], table, "the table")
            # the resident block cuts a tail like any other record
            rows = got[got["nframes"] > 0]
            offs = eng.last_scan["offsets"]
            pcm, where = eng.cut([(int(offs[r["item"]]), int(r["first_frame"]), int(r["nframes"])) for r in rows], hop=hop, denoise=0.01)
            assert pcm.size == 512 * int(rows["nframes"].sum()) and where[-1] == pcm.size and pcm.any()
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("kind,hop", [("i16", 256), ("f32", 512)])
def test_a_tail_is_the_segment_the_same_recording_ends_once_silence_follows(engines, kind, hop):
    """no reference: R's tail starts where the scan of R + 2 s of zeros starts the segment it ENDs at or behind R's last frame"""
    eng, twin = engines
    recs, counts = _prefixes(twin, kind, hop)
    longer = [np.concatenate([r, np.zeros(32000, r.dtype)]) for r in recs]
    slots = eng.open_streams(len(recs))
    try:
        with eng.scan_session():
            eng.set_thresholds_many(slots, THR)
            eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
            tails = eng.scan_tails()
            eng.reset(slots)
            eng.set_thresholds_many(slots, THR)
            table = eng.scan_segments(slots, longer, hop=hop, denoise=0.01)
    finally:
        for s in slots:
            eng.close_stream(int(s))
    seen = 0
    for i, (t, nf) in enumerate(zip(tails, counts)):
        across = [r for r in table if r["item"] == i and r["first_frame"] <= nf - 1 <= r["first_frame"] + r["nframes"] - 1]
        if t["nframes"]:
            seen += 1
            assert (int(t["item"]), int(t["first_frame"]) + int(t["nframes"])) == (i, nf)
            assert len(across) == 1 and int(across[0]["first_frame"]) == int(t["first_frame"]), (i, t, across)
    assert seen >= 2


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_open_end_on_the_default_pool(engines):
    from cutter_vad_amd import VADConfig, cut_recordings, scan_recordings, sweep_recordings
    _, twin = engines
    recs, counts = _prefixes(twin, "i16", 256)
    cfg = lambda s: VADConfig(vad_start_probability=s[0], vad_end_probability=s[1], voice_start_ratio=s[2], voice_end_ratio=s[3],
                              voice_start_frame_count=s[4], voice_end_frame_count=s[5])
    cfgs = [cfg(THR), cfg(DEFAULTS), cfg(SETS[4])]
    closed = scan_recordings(recs, cfgs[0], stats=True)
    opened = scan_recordings(recs, cfgs[0], stats=True, open_end=True)
    extra = [len(o) - len(c) for c, o in zip(closed, opened)]
    assert all(o[:len(c)] == c for c, o in zip(closed, opened)) and set(extra) == {0, 1} and sum(extra) >= 2
    for o, nf, k in zip(opened, counts, extra):
        assert not k or o[-1][1] == (nf - 1) * 256 + 512                    # an open segment ends with the recording's last frame
    got = sweep_recordings(recs, cfgs, stats=True, open_end=True)
    assert got == [scan_recordings(recs, c, stats=True, open_end=True) for c in cfgs] and got[0] == opened
    cut = cut_recordings(recs, cfgs[0], wav=False, open_end=True)
    assert [[s[:2] for s in r] for r in cut] == [[s[:2] for s in r] for r in opened]
    assert all(s[2].size == ((s[1] - s[0] - 512) // 256 + 1) * 512 for r in cut for s in r)
    # the payload of a tail is the head of the payload the same segment has once silence follows and it ENDs
    longer = cut_recordings([np.concatenate([r, np.zeros(32000, r.dtype)]) for r in recs], cfgs[0], wav=False)
    for r, l, k in zip(cut, longer, extra):
        if k:
            a, _, pcm = r[-1]
            (whole,) = [s[2] for s in l if s[0] == a]
            assert pcm.any() and np.array_equal(whole[:pcm.size], pcm)      # the prefix holds every one of the tail's frames whole
