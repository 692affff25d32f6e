"""vad_scan on the GPU at the hops, launch windows, addresses, sizes and item tables that its argument check accepts and
tests/test_gpu_scan.py does not reach (silero_v5_scan16's loader requests frame t at quad quad0 + (t0 + t) hop / 4 in 32-bit unsigned
arithmetic, through a descriptor over the whole block).  The contract is that file's, and so are the helpers: a scan gives byte for
byte what vad_step_multi gives on the 16-stream tile for the frames AudioUtils.split_into_frames cuts, saved state included.

Hops: 4, frame / 4 + 4 (frames start on no lane group's boundary and overlap by no simple fraction), frame + 4 (4 samples between
two frames belong to none) and 16 frame + 4.  Windows: the default cap of 192 frames with recordings of 192, 193, 384 and 385.
Addresses: a block of 2^31 - 16 bytes.  Size: 4 100 recordings with a frame = 257 tiles in one launch.  Tables: any order, gaps, items over the same samples."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.utils.audio import AudioUtils
from tests import g711_ref as G
from tests.test_gpu_scan import (KINDS, THR, _args, _check_against_twin, _close, _engine, _open, _recordings, _same_bytes,
                                 engines)  # noqa: F401 - engines is the module's fixture
from tests.test_gpu_v5 import TOL_P, TOL_S
from tests.test_gpu_v5_8k import TOL_P as TOL_P_8K

pytestmark = pytest.mark.gpu

HOPS = {"hop4": lambda f: 4, "quarter4": lambda f: f // 4 + 4, "frame4": lambda f: f + 4, "16frames4": lambda f: 16 * f + 4}
SEED = {"hop4": 31, "quarter4": 32, "frame4": 33, "16frames4": 34}
FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}
RATES = pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])


def _long_counts():
    """37 recordings around the default launch cap of 192 frames: one that ends on a window's last frame (192, 384), one a frame
    behind it (193, 385), the rest at most 40.  A window is launched over the recordings that still have frames in it - a prefix
    of the table sorted by count: 37 items at t0 = 0, 3 at t0 = 192 (193, 384, 385), 1 at t0 = 384, so the later windows are one
    tile whose other streams have ended (ncol <= 0: held)"""
    rng = np.random.default_rng(7)
    c = [0, 1, 385, 2, 0, 384, 40, 193, 192] + [int(v) for v in rng.integers(0, 41, 28)]
    assert len(c) == 37 and sorted(c)[-5] <= 40
    return c


def _short_counts():
    rng = np.random.default_rng(9)
    c = [0, 1, 40, 2, 0, 33, 17, 0, 40] + [int(v) for v in rng.integers(0, 41, 28)]
    assert len(c) == 37
    return c


def edge_counts(hop_name):
    """hop = 4: 40 frames span 668 samples, too few for a segment to start and end - the long batch there"""
    return _long_counts() if hop_name == "hop4" else _short_counts()


def _assert_events_are_compared(hop_name, probs, ev):
    """the comparison of events and seg_frames with the twin is not between empty sets (established on the CPU with the f64 oracle
    and oracle.StateMachine on the same frames: DESIGN 2.1f); 16 frame + 4: consecutive frames are half a second apart"""
    allp = np.concatenate(probs)
    assert np.isfinite(allp).all() and (allp >= 0).all() and (allp <= 1).all()
    if hop_name == "16frames4":
        assert np.unique(allp).size > 1
        return
    assert sum(int(((e & _ffi.VAD_EV_START) != 0).sum()) for e in ev) >= 1, "no segment started"
    assert sum(int(((e & _ffi.VAD_EV_END) != 0).sum()) for e in ev) >= 1, "no segment ended: the comparison of seg_frames would be empty"


def _hop_cases():
    out = []
    for hop_name in HOPS:
        for kind in (KINDS if hop_name == "quarter4" else ("f32", "ulaw")):
            for gate in ((0.01, None) if hop_name == "quarter4" else (0.01,)):
                out.append(pytest.param(hop_name, kind, gate, id=f"{hop_name}-{kind}-{'gate' if gate else 'nogate'}"))
    return out


# ---- a. hops (c: with events) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop_name,kind,gate", _hop_cases())
@RATES
def test_scan_equals_step_multi_at_hops_that_align_with_nothing(engines, rate, hop_name, kind, gate):
    eng, twin = engines(rate)
    frame = eng.frame_samples
    hop = HOPS[hop_name](frame)
    assert hop % 4 == 0 and (hop_name == "hop4" or (hop // 4) % 2 == 1)
    counts = edge_counts(hop_name)
    recs = _recordings(kind, frame, hop, rate, seed=SEED[hop_name], counts=counts)
    assert {0, 1, 2} <= set(counts) and [r.size >= frame and (r.size - frame) // hop + 1 or 0 for r in recs] == counts
    assert any((r.size - frame) % hop for r in recs if r.size >= frame)            # tails that framing drops
    probs, ev, seg = _check_against_twin(eng, twin, recs, frame, hop, kind, gate)
    assert [p.size for p in probs] == counts
    _assert_events_are_compared(hop_name, probs, ev)
    for e, g in zip(ev, seg):
        assert ((g > 0) == ((e & _ffi.VAD_EV_END) != 0)).all()


# ---- b. the default launch cap ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop_name", ["hop4", "quarter4"])
@RATES
def test_default_cap_windows_at_192_and_384(engines, rate, hop_name):
    """t0 = 192 and 384 of the product's own cap: xq0 = quad0 + t0 hopq, ncol = nframes - t0, obase = out0 + t0"""
    eng, twin = engines(rate)
    frame = eng.frame_samples
    hop = HOPS[hop_name](frame)
    counts = _long_counts()
    recs = _recordings("f32", frame, hop, rate, seed=SEED[hop_name], counts=counts)
    assert {0, 192, 193, 384, 385} <= set(counts)
    eng.set_scan_launch_frames(0)
    base = _check_against_twin(eng, twin, recs, frame, hop, "f32", 0.01)       # the twin's step_multi takes T = 385 for one stream
    assert [p.size for p in base[0]] == counts
    _assert_events_are_compared(hop_name, base[0], base[1])
    slots = _open(eng, len(recs))
    try:
        before = eng.info()
        got = eng.scan(slots, recs, hop=hop, denoise=0.01)
        after = eng.info()
        assert after["steps"] - before["steps"] == 3
        assert after["frames"] - before["frames"] == sum(counts)
        for a, b in zip(base, got):
            for i in range(len(recs)):
                _same_bytes(a[i], b[i], ("second scan", i))
    finally:
        _close(eng, slots)
    try:
        for cap in (1, 64):
            eng.set_scan_launch_frames(cap)
            got = _check_against_twin(eng, twin, recs, frame, hop, "f32", 0.01, replay_seg=False)
            for a, b in zip(base, got):
                for i in range(len(recs)):
                    _same_bytes(a[i], b[i], ("cap", cap, i))
    finally:
        eng.set_scan_launch_frames(0)


# ---- d. the f64 oracle at an odd hop ---------------------------------------------------------------------------------------
@RATES
def test_probabilities_match_the_f64_oracle_at_an_odd_hop(engines, rate):
    from oracle import oracle
    eng, _ = engines(rate)
    with open(weights_io.packaged_blob_path(5, rate), "rb") as f:
        om = oracle.OracleModel(f.read(), "f64")
    frame = eng.frame_samples
    hop = frame // 4 + 4
    counts = [40, 40, 40, 38, 37, 36, 33, 31, 25, 2, 1, 0]                 # descending: the oracle's live streams are a prefix
    recs = _recordings("f32", frame, hop, rate, seed=35, counts=counts)
    slots = eng.open_streams(len(recs))
    try:
        probs, _, _ = eng.scan(slots, recs, hop=hop, denoise=0.01)
        frames = [AudioUtils.split_into_frames(r, frame, hop) if c else None for r, c in zip(recs, counts)]
        st = np.zeros((len(recs), 256), np.float32)
        ref = [np.zeros(c, np.float32) for c in counts]
        for t in range(max(counts)):
            k = sum(c > t for c in counts)
            x = np.ascontiguousarray(np.stack([frames[i][t] for i in range(k)]), np.float32)
            p = om.step_batch(oracle.denoise(x, 0.01).reshape(k, frame), st[:k], nthreads=8)
            for i in range(k):
                ref[i][t] = p[i]
        worst = worst_s = 0.0
        for i, c in enumerate(counts):
            assert probs[i].shape == ref[i].shape
            if c:
                worst = max(worst, float(np.abs(probs[i] - ref[i]).max()))
            worst_s = max(worst_s, float(np.abs(eng.get_state(int(slots[i])) - st[i]).max()))
        tol = TOL_P if rate == 16000 else TOL_P_8K
        print(f"scan vs f64 oracle, {rate} Hz, hop {hop}: max |dp| = {worst:.3e}, max |dstate| = {worst_s:.3e} over {sum(counts)} "
              f"frames of {len(recs)} recordings (bars {tol}, {TOL_S})")
        assert sum(counts) == 323 and len(recs) >= 8
        assert worst <= tol and worst_s <= TOL_S
    finally:
        _close(eng, slots)


# ---- scans of a block that lies in HBM -------------------------------------------------------------------------------------
def _device_scan(eng, items, d_audio, audio_samples, hop, fmt, gate):
    """vad_scan_device on fresh slots: items = [(sample offset, samples)], slot k scans item k -> (probs, events, seg: one array
    per item; the saved state per item).  The three arrays are 8 entries longer than the CSR: those keep their fill values."""
    import torch
    slots = _open(eng, len(items))
    try:
        total = sum(eng.scan_frame_count(n, hop) for _, n in items)
        d_p = torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda")
        d_e = torch.full((total + 8,), 0x55, dtype=torch.uint8, device="cuda")
        d_s = torch.full((total + 8,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        start = eng.scan_device(slots, [o for o, _ in items], [n for _, n in items], d_audio.data_ptr(), audio_samples,
                                d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), hop=hop, fmt=fmt, denoise=gate)
        eng.synchronize()
        p, e, s = d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()
        assert int(start[-1]) == total
        assert (p[total:] == -7.0).all() and (e[total:] == 0x55).all() and (s[total:] == -9).all()
        cut = lambda a: [a[start[i]:start[i + 1]] for i in range(len(items))]
        return cut(p), cut(e), cut(s), [eng.save_stream(int(v)) for v in slots]
    finally:
        _close(eng, slots)


def _host_scan(eng, recs, hop, kind, gate):
    """Engine.scan on fresh slots -> (probs, events, seg, saved states)"""
    slots = _open(eng, len(recs))
    try:
        p, e, s = eng.scan(slots, recs, hop=hop, **_args(kind, gate))
        return p, e, s, [eng.save_stream(int(v)) for v in slots]
    finally:
        _close(eng, slots)


def _same_results(a, b, what, pairs=None):
    """(probs, events, seg, states) a == b; pairs: [(index in a, index in b)], default: item by item"""
    pairs = [(i, i) for i in range(len(a[3]))] if pairs is None else pairs
    for i, j in pairs:
        for k, name in enumerate(("probs", "events", "seg")):
            _same_bytes(a[k][i], b[k][j], (what, name, i, j))
        assert a[3][i] == b[3][j], (what, "state", i, j)


# ---- e. poison outside the frames ------------------------------------------------------------------------------------------
@RATES
def test_non_finite_samples_in_no_frame_reject_nothing(engines, rate):
    """hop = frame + 4, float32: the reject flag is a maximum over what the loader loaded, and it must have loaded the frames alone.
    NaN / +Inf / -Inf on EVERY sample that is in no frame: the 4 between two frames, a recording's tail, the padding between two
    recordings, 64 guard samples in front of the first and behind the last recording."""
    import torch
    eng, _ = engines(rate)
    frame = eng.frame_samples
    hop, guard = frame + 4, 64
    counts = [7, 0, 12, 1, 3, 9, 2, 0, 5, 12, 4, 6, 1, 8, 3, 10, 2, 11, 6, 5]
    recs = _recordings("f32", frame, hop, rate, seed=36, counts=counts)
    offs, pos = [], guard
    for r in recs:
        offs.append(pos)
        pos += (r.size + 3) & ~3
    last_end = offs[-1] + recs[-1].size
    nsamp = ((last_end + 3) & ~3) + guard
    clean = np.zeros(nsamp, np.float32)             # the reference block: the frames' samples, zeros everywhere else
    where = np.zeros(nsamp, np.uint8)               # 0 in a frame, 1 between frames, 2 tail, 3 padding, 4 guard
    where[:guard] = 4
    where[last_end:] = 4
    for i, (r, o, c) in enumerate(zip(recs, offs, counts)):
        clean[o:o + r.size] = r
        where[o:o + r.size] = 1
        for t in range(c):
            where[o + t * hop:o + t * hop + frame] = 0
        used = frame + (c - 1) * hop if c else 0
        where[o + used:o + r.size] = 2
        if i + 1 < len(recs):
            where[o + r.size:offs[i + 1]] = 3
    n_out = [int((where == k).sum()) for k in (1, 2, 3, 4)]
    assert min(n_out) > 0 and n_out[0] == 4 * sum(max(c - 1, 0) for c in counts) and n_out[3] >= 2 * guard, n_out
    clean[where != 0] = 0.0
    poisoned = clean.copy()
    idx = np.flatnonzero(where)
    poisoned[idx] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), idx.size)
    assert np.isfinite(poisoned[where == 0]).all() and not np.isfinite(poisoned[where != 0]).any()
    items = [(o, r.size) for o, r in zip(offs, recs)]
    want = _device_scan(eng, items, torch.from_numpy(clean).cuda(), nsamp, hop, FMT["f32"], 0.01)
    got = _device_scan(eng, items, torch.from_numpy(poisoned).cuda(), nsamp, hop, FMT["f32"], 0.01)
    _same_results(got, want, "poisoned against zeros")
    assert [p.size for p in got[0]] == counts
    assert np.isfinite(np.concatenate(got[0])).all()
    assert not (np.concatenate(got[1]) & _ffi.VAD_EV_REJECTED).any()
    # and they are Engine.scan's of the recordings as they were, their own samples between the frames and in the tails, which (a)
    # ties to the twin
    _same_results(want, _host_scan(eng, recs, hop, "f32", 0.01), "device against host")


# ---- f. poison on a frame's edges ------------------------------------------------------------------------------------------
@RATES
def test_a_non_finite_sample_rejects_exactly_the_frames_that_hold_it(engines, rate):
    eng, twin = engines(rate)
    frame = eng.frame_samples
    hop = frame // 4 + 4
    counts = [12, 9, 5, 12, 0, 7] + [6] * 14
    clean = _recordings("f32", frame, hop, rate, seed=37, counts=counts)
    recs = [r.copy() for r in clean]
    bad = {0: 5 * hop, 3: 3 * hop + frame - 1, 1: 7 * hop - 1}     # first sample of frame 5; last of frame 3; the one before frame 7
    recs[0][bad[0]] = np.nan
    recs[3][bad[3]] = np.inf
    recs[1][bad[1]] = np.nan
    holds = {i: [t for t in range(counts[i]) if t * hop <= s < t * hop + frame] for i, s in bad.items()}
    assert holds == {0: [2, 3, 4, 5], 3: [3, 4, 5, 6], 1: [4, 5, 6]} and len(recs) == 20
    for gate in (0.01, None):
        probs, ev, seg = _check_against_twin(eng, twin, recs, frame, hop, "f32", gate, replay_seg=False)
        ref = _check_against_twin(eng, twin, clean, frame, hop, "f32", gate)
        for i, want in holds.items():
            rej = (ev[i] & _ffi.VAD_EV_REJECTED) != 0
            assert list(np.flatnonzero(rej)) == want, (i, np.flatnonzero(rej))
            assert (ev[i][rej] == _ffi.VAD_EV_REJECTED).all() and np.isnan(probs[i][rej]).all() and not seg[i][rej].any()
            assert np.isfinite(probs[i][~rej]).all()
            _same_bytes(probs[i][:want[0]], ref[0][i][:want[0]], ("before the rejected frames", i))
        for i in range(len(recs)):
            if i not in holds:
                for a, b in zip((probs, ev, seg), ref):
                    _same_bytes(a[i], b[i], ("neighbour", i))


# ---- g. high addresses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "i16_32768", "ulaw"])
@RATES
def test_recordings_up_to_the_last_byte_below_2_gib(engines, rate, kind):
    """a block of 2^31 - 16 bytes, the most the argument check accepts to within a quad: the quad index shifted to a byte offset
    (<< 4 / 3 / 2) reaches bit 30, the descriptor's range and the offsets stay positive as 32-bit integers"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the block and torch's copies need 6 GiB")
    eng, _ = engines(rate)
    frame = eng.frame_samples
    hop = frame // 4 + 4
    counts = [12, 7, 3, 9, 5]
    recs = _recordings(kind, frame, hop, rate, seed=38, counts=counts)
    recs[4] = recs[4][:frame + (counts[4] - 1) * hop]                  # no tail: its last sample is the block's last
    size = recs[0].dtype.itemsize
    nsamp = ((1 << 31) - 16) // size
    at = lambda byte: (byte // size) & ~3
    offs = [0, at(1 << 30) - (recs[1].size // 2 & ~3), 0, at(3 << 29) - 260, nsamp - recs[4].size]
    offs[2] = ((offs[1] + recs[1].size + 3) & ~3) + 4
    assert 0 < at(1 << 30) - offs[1] < frame + (counts[1] - 1) * hop                # one of its frames straddles byte 2^30
    assert 1 << 30 < offs[2] * size < (1 << 30) + (1 << 16)
    assert all(o % 4 == 0 for o in offs) and offs[4] + recs[4].size == nsamp and nsamp * size == (1 << 31) - 16
    want = _host_scan(eng, recs, hop, kind, 0.01)                       # the same five arrays packed into a small block
    assert [p.size for p in want[0]] == counts
    d_audio = torch.zeros(nsamp, dtype={4: torch.float32, 2: torch.int16, 1: torch.uint8}[size], device="cuda")
    try:
        for r, o in zip(recs, offs):
            d_audio[o:o + r.size] = torch.from_numpy(r).cuda()
        torch.cuda.synchronize()
        items = [(o, r.size) for o, r in zip(offs, recs)]
        got = _device_scan(eng, items, d_audio, nsamp, hop, FMT[kind], 0.01)
        _same_results(got, want, ("high addresses", kind))
        # the offsets of two items change places: slot 1 scans the top of the block, slot 4 the samples around byte 2^30
        items[1], items[4] = items[4], items[1]
        got = _device_scan(eng, items, d_audio, nsamp, hop, FMT[kind], 0.01)
        _same_results(got, want, ("swapped", kind), pairs=[(0, 0), (1, 4), (2, 2), (3, 3), (4, 1)])
    finally:
        del d_audio
        torch.cuda.empty_cache()


# ---- h. more than 4 096 recordings -----------------------------------------------------------------------------------------
def test_4100_recordings_stay_on_16_stream_tiles():
    """A launch covers the recordings that still have frames in its window, 16 to a tile: 4 100 recordings WITH a frame are 257
    tiles (two rounds per CU; block 256 reads the items 4 096 .. 4 099 and has 4 streams), where every other multi-frame path
    takes 32-stream tiles.  8 more recordings have no frame and are never launched."""
    n_live, n, rate = 4100, 4108, 16000
    eng, twin = _engine(rate, max_streams=8192), _engine(rate, max_streams=8192)
    try:
        twin.set_tile(16)
        frame = eng.frame_samples
        hop = frame // 4 + 4
        rng = np.random.default_rng(39)
        counts = np.insert(rng.integers(1, 7, n_live), np.sort(rng.choice(n_live, n - n_live, replace=False)), 0)
        assert counts.size == n and (counts > 0).sum() == n_live > 4096 and set(counts) == set(range(7))
        tiles = lambda t0: -(-int((counts > t0).sum()) // 16)               # of the window that starts at frame t0
        assert tiles(0) == 257 and (counts > 0).sum() % 16 == 4
        lens = np.where(counts > 0, frame + (counts - 1) * hop + rng.integers(0, hop, n), rng.integers(0, frame, n))
        pool = G.speechlike(1, 64, frame, 40).reshape(-1).astype(np.float32)
        recs = [pool[o:o + m] for o, m in zip(rng.integers(0, pool.size - int(lens.max()), n), lens)]
        slots, tslots = _open(eng, n), _open(twin, n)
        before = eng.info()["steps"]
        base = eng.scan(slots, recs, hop=hop, denoise=0.01)
        assert eng.info()["steps"] - before == 1
        assert [p.size for p in base[0]] == list(counts)
        # the twin: one vad_step_multi per distinct count
        for c in range(1, 7):
            idx = np.flatnonzero(counts == c)
            assert idx.size > 16
            fr = np.stack([AudioUtils.split_into_frames(recs[i], frame, hop) for i in idx])
            assert fr.shape == (idx.size, c, frame)
            p, ev = twin.step_multi(tslots[idx], fr, denoise=0.01)
            for k, i in enumerate(idx):
                _same_bytes(base[0][i], p[k], ("probs", int(i)))
                _same_bytes(base[1][i], ev[k], ("events", int(i)))
        allp = np.concatenate(base[0])
        assert np.isfinite(allp).all() and np.unique(allp).size > 1000
        order = np.argsort(-counts, kind="stable")                          # the engine's table: stable, descending
        last_tile = order[4096:n_live]                                      # the streams of block 256
        assert last_tile.size == 4 and (counts[last_tile] == 1).all()
        empty = order[n_live:]
        rest = np.setdiff1d(np.arange(n), np.concatenate([last_tile, empty]))
        picked = np.concatenate([last_tile, empty, np.random.default_rng(41).choice(rest, 52, replace=False)])
        assert picked.size == 64 and (counts[picked] == 0).sum() == 8 and (counts[picked] == 6).sum() >= 1
        saved = {int(i): eng.save_stream(int(slots[i])) for i in picked}
        fresh = eng.save_stream(int(slots[empty[0]]))
        for i in picked:
            assert saved[int(i)] == twin.save_stream(int(tslots[i])), ("state", int(i))
            assert (saved[int(i)] == fresh) == (counts[i] == 0), ("state moved", int(i))
        # two frames per launch (257, then fewer tiles), the recordings listed in another order: the same bytes
        perm = np.random.default_rng(42).permutation(n)
        eng.reset(slots)
        eng.set_thresholds_many(slots, THR)
        eng.set_scan_launch_frames(2)
        assert tiles(0) == 257 and tiles(2) > tiles(4) > 64
        before = eng.info()["steps"]
        got = eng.scan(slots[perm], [recs[i] for i in perm], hop=hop, denoise=0.01)
        assert eng.info()["steps"] - before == 3
        for k in range(3):
            a = np.concatenate([base[k][i] for i in perm])
            b = np.concatenate(got[k])
            _same_bytes(a, b, ("cap 2, permuted", k))
        # (in the permuted table other recordings make up block 256; the picked ones keep their results and states all the same)
        for i in picked:
            assert eng.save_stream(int(slots[i])) == saved[int(i)], ("state, cap 2, permuted", int(i))
    finally:
        eng.close()
        twin.close()


# ---- i. item tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "ulaw"])
@RATES
def test_items_in_any_order_with_gaps_and_over_the_same_samples(engines, rate, kind):
    """offsets descending with gaps of 4 .. 4 000 samples, two slots with the same (offset, length), two items that overlap by half:
    each item gives what its samples give when they are scanned alone"""
    import torch
    eng, _ = engines(rate)
    frame = eng.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(43)
    counts = [9, 0, 14, 3, 1, 12, 6, 2, 11, 5, 7, 4]
    recs = _recordings(kind, frame, hop, rate, seed=44, counts=counts)
    gaps = 4 * rng.integers(1, 1001, len(recs))
    assert gaps.min() >= 4 and gaps.max() <= 4000
    offs, pos = [0] * len(recs), 0
    for i in reversed(range(len(recs))):                                # the first recording lies highest
        offs[i] = pos
        pos += ((recs[i].size + 3) & ~3) + int(gaps[i])
    assert all(offs[i] > offs[i + 1] + recs[i + 1].size for i in range(len(recs) - 1))
    block = np.zeros(pos, recs[0].dtype)
    for r, o in zip(recs, offs):
        block[o:o + r.size] = r
    items = [(o, r.size) for o, r in zip(offs, recs)]
    items += [items[2], items[2]]                                       # three slots over recording 2's samples
    half = (recs[5].size // 2) & ~3
    items += [(offs[5] + half, recs[5].size)]                           # the second half of recording 5 and what lies behind it
    items += [(offs[8] - 4 * (recs[8].size // 8), recs[8].size)]        # from inside recording 9's gap into recording 8
    assert all(o >= 0 and o % 4 == 0 and o + m <= block.size for o, m in items)
    got = _device_scan(eng, items, torch.from_numpy(block).cuda(), block.size, hop, FMT[kind], 0.01)
    _same_results(got, got, "the same item twice", pairs=[(2, 12), (2, 13)])
    assert got[0][2].size == 14 and got[0][14].size == 12 and got[0][15].size == 11
    for k, (o, m) in enumerate(items):
        alone = _host_scan(eng, [block[o:o + m].copy()], hop, kind, 0.01)
        _same_results(got, alone, ("scanned alone", kind, k), pairs=[(k, 0)])
    assert np.isfinite(np.concatenate(got[0])).all() and np.unique(np.concatenate(got[0])).size > 20
