"""vad_scan_rate and vad_scan_rate_cut on the GPU at the hops, windows and addresses that their argument checks accept and
tests/test_gpu_scan_rate.py / tests/test_gpu_scan_rate_cut.py do not reach.  vadk_scan_resample and vadk_cut_resample do their own
row -> chunk -> byte offset arithmetic in 32-bit unsigned (quad0 + (t0 + tt) hopq, quad << qsh, row g = (item g / W, chunk g % W),
the tile_seg / row0 walk) in front of the shared body of resample_512.h, so tests/test_gpu_scan_edges.py's coverage of the 16 kHz
loader does not transfer.  The contract and the helpers are those two files': a rate scan gives byte for byte what
AudioUtils.split_into_frames -> Engine.resample -> vad_step_multi on the 16-stream tile gives (the twin), saved state included; a cut
of frames gives the twin's frames through cut_ref, a cut of a range cut_ref.reference with frame = chunk and no gate.

Hops: 4, chunk / 4 + 4 (hopq odd), chunk + 4 (4 samples between two chunks belong to none) and 16 chunk + 4, at 8 / 24 / 48 kHz.
Windows: the default cap of 192 with recordings of 192, 193, 384 and 385 chunks; a window of 95 chunks that the 256 MiB window
buffer decides (1 366 live recordings); cut windows of 32, 64 and 160 rows.  Addresses: a block of 2^31 - 16 bytes.  The f64 oracle
chain (oracle.resample -> OracleModel) behind a scan at the odd hop.  NaN / Inf outside every chunk and on the samples that the
resampler's fold treats apart."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.utils.audio import AudioUtils
from tests import cut_ref as R
from tests import g711_ref as G
from tests.cut_ref import F32, FRAMES, PCM16, RANGE, untouched
from tests.rate_cut_ref import rate_cut
from tests.test_gpu_scan import _close, _engine, _open, _same_bytes
from tests.test_gpu_scan_edges import HOPS, SEED, _assert_events_are_compared, edge_counts
from tests.test_gpu_scan_rate import CHUNK, CYCLE, FMT, _check_seg_and_ends, _compare, _heard, _recordings, _scan, _twin_of
from tests.test_gpu_scan_rate_cut import COUNTS, SEGS, _block, _frames, _items, _payload

pytestmark = pytest.mark.gpu

RATES = (8000, 24000, 48000)
WIN_ROWS = (256 << 20) // 2048                # frames of 2 KiB in the engine's window buffer
DEFAULT_CAP = 192                             # chunks of every recording per launch
TWO_KIND = {8000: "ulaw", 24000: "i16_32767", 48000: "f32"}
TOL_P = 1e-4                                  # the bar of the resample + V5 chain against the f64 oracle (tests/test_gpu_resample.py)


@pytest.fixture(scope="module")
def engines():
    """(the engine that scans and cuts at other rates, its twin with the tile pinned to 16 streams for vad_resample + vad_step_multi)"""
    eng, twin = _engine(16000), _engine(16000)
    twin.set_tile(16)
    yield eng, twin
    eng.close()
    twin.close()


def launches(counts, cap=0):
    """model launches of a rate scan by the window rule of scan_rate_launches: W = min(cap, longest, WIN_ROWS // live) chunks"""
    live, longest = sum(c > 0 for c in counts), max(counts)
    if live == 0:
        return 0
    return -(-longest // max(1, min(cap or DEFAULT_CAP, longest, WIN_ROWS // live)))


def hop_case(sr, hop_name, kind, two):
    """the batch of one case of (a) -> (hop, counts, recordings, per-item channel modes or None, what a host would have prepared)"""
    hop = HOPS[hop_name](CHUNK[sr])
    counts = edge_counts(hop_name)
    recs = _recordings(kind, sr, hop, seed=SEED[hop_name], counts=counts, two=two)
    modes = [CYCLE[i % 3] for i in range(len(recs))] if two else None
    heard = [_heard(r, kind, modes[i] if two else None) for i, r in enumerate(recs)]
    return hop, counts, recs, modes, heard


def hop_cases():
    """(sr, hop name, kind, gate, two channels)"""
    out = []
    for sr in RATES:
        for hop_name in HOPS:
            for kind in (tuple(FMT) if hop_name == "quarter4" else ("f32", "ulaw")):
                for gate in ((0.01, None) if hop_name == "quarter4" else (0.01,)):
                    out.append((sr, hop_name, kind, gate, False))
        out.append((sr, "quarter4", TWO_KIND[sr], 0.01, True))
    return out


def _id(case):
    sr, hop_name, kind, gate, two = case
    return f"{sr}-{hop_name}-{kind}-{'gate' if gate else 'nogate'}" + ("-two_channels" if two else "")


# ---- a. hops -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hop_cases(), ids=_id)
def test_rate_scan_equals_the_twin_at_hops_that_align_with_nothing(engines, case):
    """that START and END events exist in every batch but 16 chunk + 4's was established on the CPU first, with the f64 oracle chain
    (oracle.resample -> oracle.denoise -> OracleModel) and oracle.StateMachine on the same chunks, the probabilities moved by +-2e-3 as well"""
    eng, twin = engines
    sr, hop_name, kind, gate, two = case
    chunk = CHUNK[sr]
    hop, counts, recs, modes, heard = hop_case(sr, hop_name, kind, two)
    assert hop % 4 == 0 and (hop_name == "hop4" or (hop // 4) % 2 == 1)
    assert len(recs) == 37 and {0, 1, 2} <= set(counts)
    assert [r.shape[0] >= chunk and (r.shape[0] - chunk) // hop + 1 or 0 for r in recs] == counts
    assert any(0 < r.shape[0] < chunk for r in recs) and any(r.shape[0] == 0 for r in recs)
    assert any((r.shape[0] - chunk) % hop for r in recs if r.shape[0] >= chunk)       # tails that framing drops
    want = _twin_of(twin, ("edges", hop_name, kind, two), heard, sr, hop, gate)
    steps = eng.info()["steps"]
    got = _scan(eng, recs, kind, sr, hop, gate, channel=modes if two else "mix")
    assert eng.info()["steps"] - steps == launches(counts) == (3 if hop_name == "hop4" else 1)
    _compare(got, want, case)
    assert [g[0].size for g in got] == counts
    _assert_events_are_compared(hop_name, [g[0] for g in got], [g[1] for g in got])
    if hop_name == "16frames4":
        for p, e, g, _ in got:
            assert g.dtype == np.int32 and g.shape == e.shape == p.shape and ((g > 0) == ((e & _ffi.VAD_EV_END) != 0)).all()
    else:
        _check_seg_and_ends(eng, got, case)


# ---- b. the f64 oracle behind a rate scan at an odd hop ----------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_probabilities_match_the_f64_oracle_chain_at_an_odd_hop(engines, sr):
    """host float32 chunks -> oracle.resample(chunk, 512) -> OracleModel f64, free-running from zero state; gate off: the gate is
    a discontinuity at |x| = threshold, and the resampler's float32 rounding may land on its other side than the f64 reference's.
    Measured on an MI355X: max |dp| = 1.3e-6 (8 kHz), 4.4e-6 (24 kHz), 3.5e-6 (48 kHz) over 323 chunks, bar 1e-4"""
    from oracle import oracle
    eng, _ = engines
    with open(weights_io.packaged_blob_path(5, 16000), "rb") as f:
        om = oracle.OracleModel(f.read(), "f64")
    chunk = CHUNK[sr]
    hop = chunk // 4 + 4
    counts = [40, 40, 40, 38, 37, 36, 33, 31, 25, 2, 1, 0]                 # descending: the oracle's live streams are a prefix
    recs = _recordings("f32", sr, hop, seed=35, counts=counts)
    got = _scan(eng, recs, "f32", sr, hop, None)
    assert [g[0].size for g in got] == counts and sum(counts) == 323
    chunks = [AudioUtils.split_into_frames(r, chunk, hop) if c else None for r, c in zip(recs, counts)]
    st = np.zeros((len(recs), 256), np.float32)
    ref = [np.zeros(c, np.float32) for c in counts]
    for t in range(max(counts)):
        k = sum(c > t for c in counts)
        x = np.ascontiguousarray(np.stack([oracle.resample(chunks[i][t], 512) for i in range(k)]), np.float32)
        p = om.step_batch(x, st[:k], nthreads=8)
        for i in range(k):
            ref[i][t] = p[i]
    allp = np.concatenate([g[0] for g in got])
    worst = float(np.abs(allp - np.concatenate(ref)).max())
    print(f"rate scan vs f64 oracle chain, {sr} Hz, hop {hop}: max |dp| = {worst:.3e} over {sum(counts)} chunks (bar {TOL_P})")
    assert np.isfinite(allp).all() and np.unique(allp).size > 100
    assert worst <= TOL_P


# ---- scans and cuts of a block that lies in HBM ------------------------------------------------------------------------------
def _device_scan(eng, items, d_audio, audio_samples, sr, hop, fmt, gate, channels=1, modes=None):
    """vad_scan_rate_device on fresh slots: items = [(sample offset, samples)], slot k scans item k -> per item (probs, events, seg,
    saved state).  The three arrays are 8 entries longer than the CSR: those keep their fill values."""
    import torch
    slots = _open(eng, len(items))
    try:
        total = sum(eng.scan_frame_count(n, hop, sample_rate=sr) for _, n in items)
        d_p = torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda")
        d_e = torch.full((total + 8,), 0x55, dtype=torch.uint8, device="cuda")
        d_s = torch.full((total + 8,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        start = eng.scan_device(slots, [o for o, _ in items], [n for _, n in items], d_audio.data_ptr(), audio_samples, d_p.data_ptr(),
                                d_e.data_ptr(), d_s.data_ptr(), hop=hop, fmt=fmt, denoise=gate, channels=channels, channel=modes,
                                sample_rate=sr)
        eng.synchronize()
        p, e, s = d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()
        assert int(start[-1]) == total
        assert (p[total:] == -7.0).all() and (e[total:] == 0x55).all() and (s[total:] == -9).all()
        return [(p[start[i]:start[i + 1]], e[start[i]:start[i + 1]], s[start[i]:start[i + 1]], eng.save_stream(int(slots[i])))
                for i in range(len(items))]
    finally:
        _close(eng, slots)


def _device_cut(eng, segs, d_audio, audio_samples, sr, hop, fmt, gate, layout, out, channels=1):
    """vad_scan_rate_cut_device, the payloads packed in the order listed -> the output with 8 samples behind it, which keep their fill"""
    import torch
    total = sum(eng.cut_samples(sg[2], hop, layout, sample_rate=sr) for sg in segs)
    fill, dt = (R.SENT16, torch.int16) if out == "pcm16" else (R.SENT32, torch.float32)
    d_out = torch.full((total + 8,), fill.item(), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    start = eng.cut_device(segs, d_audio.data_ptr(), audio_samples, d_out.data_ptr(), total, hop=hop, fmt=fmt, channels=channels, denoise=gate,
                           layout=layout, out=out, sample_rate=sr)
    eng.synchronize()
    got = d_out.cpu().numpy()
    assert int(start[-1]) == total and untouched(got[total:])
    return got


def _pack(recs, guard=0):
    """recordings on multiples of 4 sample frames behind `guard` of them -> (block of zeros elsewhere, offsets, the last one's end)"""
    offs, pos = [], guard
    for r in recs:
        offs.append(pos)
        pos += (r.shape[0] + 3) & ~3
    end = offs[-1] + recs[-1].shape[0]
    block = np.zeros((((end + 3) & ~3) + guard,) + recs[0].shape[1:], recs[0].dtype)
    for r, o in zip(recs, offs):
        block[o:o + r.shape[0]] = r
    return block, offs, end


# ---- c. poison outside the chunks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_non_finite_samples_in_no_chunk_reject_nothing_and_reach_no_cut(engines, sr):
    """hop = chunk + 4, float32: a resampled frame is a contraction over what the loader loaded, and it must have loaded the chunk
    alone.  NaN / +Inf / -Inf on EVERY sample that is in no chunk: the 4 between two chunks, a recording's tail, the padding
    between two recordings, 64 guard samples in front of the first and behind the last recording."""
    import torch
    eng, _ = engines
    chunk = CHUNK[sr]
    hop, guard = chunk + 4, 64
    counts = [7, 0, 12, 1, 3, 9, 2, 0, 5, 12, 4, 6, 1, 8, 3, 10, 2, 11, 6, 5]
    recs = _recordings("f32", sr, hop, seed=36, counts=counts)
    clean, offs, last_end = _pack(recs, guard)
    nsamp = clean.size
    where = np.zeros(nsamp, np.uint8)               # 0 in a chunk, 1 between chunks, 2 tail, 3 padding, 4 guard
    where[:guard] = 4
    where[last_end:] = 4
    for i, (r, o, c) in enumerate(zip(recs, offs, counts)):
        where[o:o + r.size] = 1
        for t in range(c):
            where[o + t * hop:o + t * hop + chunk] = 0
        used = chunk + (c - 1) * hop if c else 0
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
    d_clean, d_poisoned = torch.from_numpy(clean).cuda(), torch.from_numpy(poisoned).cuda()
    want = _device_scan(eng, items, d_clean, nsamp, sr, hop, FMT["f32"], 0.01)
    got = _device_scan(eng, items, d_poisoned, nsamp, sr, hop, FMT["f32"], 0.01)
    _compare(got, want, ("poisoned against zeros", sr), seg=True)
    assert [g[0].size for g in got] == counts
    assert np.isfinite(np.concatenate([g[0] for g in got])).all()
    assert not (np.concatenate([g[1] for g in got]) & _ffi.VAD_EV_REJECTED).any()
    # and they are Engine.scan's of the recordings as they were, their own samples between the chunks and in the tails, which (a)
    # ties to the twin
    _compare(want, _scan(eng, recs, "f32", sr, hop, 0.01), ("device against host", sr), seg=True)
    # the frames of a hand-built segment table: every chunk of every recording, in segments that start at chunk 0, 1 and 2
    segs = [(o, i % 3 if c > 3 else 0, c - (i % 3 if c > 3 else 0)) for i, (o, c) in enumerate(zip(offs, counts)) if c]
    assert {sg[1] for sg in segs} == {0, 1, 2} and sum(sg[2] for sg in segs) > 64
    for gate, out in ((0.01, "pcm16"), (None, "f32")):
        a = _device_cut(eng, segs, d_clean, nsamp, sr, hop, FMT["f32"], gate, "frames", out)
        b = _device_cut(eng, segs, d_poisoned, nsamp, sr, hop, FMT["f32"], gate, "frames", out)
        assert a.tobytes() == b.tobytes(), (sr, out, int((a != b).sum()))
        assert np.isfinite(a.astype(np.float64)).all() and np.unique(a).size > 100


# ---- c. poison on the samples that the fold treats apart ---------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_a_non_finite_sample_rejects_exactly_the_chunks_that_hold_it(engines, sr):
    """hop = chunk / 4 + 4.  One non-finite sample per recording, at chunk-relative position 0, chunk / 4, chunk / 2, 3 chunk / 4
    and chunk - 1 of a chunk t - x[0] and x[H] have no mirror partner in the resampler's fold, x[Q] and x[3Q] go through its rank-1
    term and the loader's tail() path, 0 and chunk - 1 are the chunk's edges - and one on the sample in front of chunk t"""
    import torch
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // 4 + 4
    counts = [12, 9, 12, 12, 0, 7, 10, 11] + [6] * 12
    clean = _recordings("f32", sr, hop, seed=37, counts=counts)
    recs = [r.copy() for r in clean]
    # recording -> (chunk t, position relative to its first sample)
    at = {0: (5, 0), 1: (7, -1), 2: (4, chunk // 4), 3: (3, chunk - 1), 6: (6, chunk // 2), 7: (5, 3 * chunk // 4)}
    bad = {i: t * hop + rel for i, (t, rel) in at.items()}
    for k, (i, s) in enumerate(bad.items()):
        recs[i][s] = (np.nan, np.inf, -np.inf)[k % 3]
    holds = {i: [t for t in range(counts[i]) if t * hop <= s < t * hop + chunk] for i, s in bad.items()}
    assert holds == {0: [2, 3, 4, 5], 1: [4, 5, 6], 2: [2, 3, 4], 3: [3, 4, 5, 6], 6: [5, 6, 7], 7: [5, 6, 7]}
    assert all((t in holds[i]) == (rel >= 0) for i, (t, rel) in at.items()) and len(recs) == 20
    block, offs, _ = _pack(recs)
    block0, offs0, _ = _pack(clean)
    assert offs == offs0
    items = [(o, r.size) for o, r in zip(offs, recs)]
    for gate in (0.01, None):
        got = _device_scan(eng, items, torch.from_numpy(block).cuda(), block.size, sr, hop, FMT["f32"], gate)
        _compare(got, _twin_of(twin, ("inside",), recs, sr, hop, gate), ("inside", sr, gate))
        ref = _device_scan(eng, items, torch.from_numpy(block0).cuda(), block0.size, sr, hop, FMT["f32"], gate)
        for i, want in holds.items():
            p, e, g, _ = got[i]
            rej = (e & _ffi.VAD_EV_REJECTED) != 0
            assert list(np.flatnonzero(rej)) == want, (i, np.flatnonzero(rej))
            assert (e[rej] == _ffi.VAD_EV_REJECTED).all() and np.isnan(p[rej]).all() and not g[rej].any()
            assert np.isfinite(p[~rej]).all()
            _same_bytes(p[:want[0]], ref[i][0][:want[0]], ("before the rejected chunks", i))
        for i in range(len(recs)):
            if i not in holds:
                _compare([got[i]], [ref[i]], ("neighbour", i), seg=True)


# ---- d. cuts at the same hops ------------------------------------------------------------------------------------------------
def cut_cases():
    """(sr, hop name, kind, two channels, gate, out format): formats, channels, gate and output paired as in
    tests/test_gpu_scan_rate_cut.py's _cases(), with the hop in the rotation - every value at every rate, no full product"""
    out = []
    for sr in RATES:
        for h, hop_name in enumerate(HOPS):
            for k, kind in enumerate(("f32", "i16_32767", "ulaw")):
                if kind == "i16_32767" and hop_name != "quarter4":
                    continue
                pairs = ((False, 0.01, PCM16), (True, None, F32)) if (k + h + sr // 8000) % 2 else ((False, None, F32), (True, 0.01, PCM16))
                out += [(sr, hop_name, kind) + p for p in pairs]
    out.append((24000, "quarter4", "i16_32768", True, 0.01, PCM16))
    out.append((8000, "quarter4", "alaw", False, 0.01, PCM16))
    return out


def _cut_id(case):
    sr, hop_name, kind, two, gate, _ = case
    return f"{sr}-{hop_name}-{kind}-{'stereo' if two else 'mono'}-{'gate' if gate else 'nogate'}"


def _twin_payloads(twin, block, offs, lens, items, kind, sr, hop, gate, out_fmt):
    """the twin's frames of every (recording, channel) that SEGS names, gated and converted -> one payload per item"""
    frames, out = {}, []
    for (rec, first, nf), it in zip(SEGS, items):
        key = (rec, it[4])
        if key not in frames:
            frames[key] = _frames(twin, R.heard(block[offs[rec]:offs[rec] + lens[rec]], kind, it[4]), sr, hop)
            assert frames[key].shape == (COUNTS[rec], 512)
        out.append(_payload(frames[key], first, nf, gate, out_fmt))
    return out, frames


def _check_written(out, items, wants, what):
    written = np.zeros(out.size, bool)
    for it, want in zip(items, wants):
        got = out[it[3]:it[3] + want.size]
        assert got.tobytes() == want.tobytes(), (what, it, int((got != want).sum()))
        written[it[3]:it[3] + want.size] = True
    assert untouched(out[~written]) and (~written).sum() >= 12 + 8            # the gaps and the tail keep the sentinel


@pytest.mark.parametrize("case", cut_cases(), ids=_cut_id)
def test_cut_frames_equal_the_twin_and_ranges_the_block_at_hops_that_align_with_nothing(engines, case):
    eng, twin = engines
    sr, hop_name, kind, two, gate, out_fmt = case
    chunk = CHUNK[sr]
    hop = HOPS[hop_name](chunk)
    block, offs, lens = _block(kind, sr, hop, two, seed=sr // 1000 + len(kind) + len(hop_name))
    thr = -1.0 if gate is None else gate
    items, total = _items(SEGS, offs, hop, chunk, FRAMES, two)
    rc, msg, out = rate_cut(eng._lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, FRAMES, out_fmt, total, thr=thr)
    assert rc == _ffi.VAD_OK, msg
    wants, frames = _twin_payloads(twin, block, offs, lens, items, kind, sr, hop, gate, out_fmt)
    assert all(w.size == nf * 512 == eng.cut_samples(nf, hop, "frames", sample_rate=sr) for w, (_, _, nf) in zip(wants, SEGS))
    _check_written(out, items, wants, "frames")
    if gate is not None:
        assert any((_payload(f, 0, len(f), None, F32) != _payload(f, 0, len(f), gate, F32)).any() for f in frames.values()), "the gate gated nothing"
    # RANGE: the segment's own samples at the input rate (for hop > chunk those between the chunks too), NOT gated
    items, total = _items(SEGS, offs, hop, chunk, RANGE, two)
    rc, msg, out = rate_cut(eng._lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, RANGE, out_fmt, total, thr=0.01)
    assert rc == _ffi.VAD_OK, msg
    wants = [R.reference(block, kind, it, chunk, hop, RANGE, out_fmt, None) for it in items]
    assert all(w.size == (it[2] - 1) * hop + chunk == eng.cut_samples(it[2], hop, "range", sample_rate=sr) for w, it in zip(wants, items))
    _check_written(out, items, wants, "range")


# ---- e. capped cut windows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,kind,two,gate,out_fmt", [(24000, "i16_32767", False, 0.01, PCM16), (48000, "f32", True, None, F32)],
                         ids=["24000-i16-mono-gate-pcm16", "48000-f32-stereo-nogate-f32"])
def test_cut_windows_of_32_64_and_160_rows_change_no_byte(engines, sr, kind, two, gate, out_fmt):
    """the launch-frames knob shrinks a cut's window to 32 rows per frame of the cap: SEGS' 300 rows in 10, 5 and 2 windows, every
    boundary inside a segment (the per-window CutSeg starts (lo - r0) rows into the window and (lo - row0) rows into the payload),
    tiles that three segments share (the tile_seg / row0 walk of CutRows), the 70-row segment over three windows at cap 1"""
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // 2
    row0 = np.concatenate([[0], np.cumsum([nf for _, _, nf in SEGS])])
    assert row0[-1] == 300
    for cap in (1, 2, 5):
        assert all(b not in row0 for b in range(32 * cap, 300, 32 * cap))
    assert SEGS[0][2] == 70 and {r // 32 for r in range(70)} == {0, 1, 2}             # the first segment: windows 0, 1, 2 at cap 1
    assert max(sum(32 * t < r < 32 * t + 32 for r in row0[:-1]) for t in range(10)) >= 2       # two segments begin inside a tile that a third began
    block, offs, lens = _block(kind, sr, hop, two, seed=53)
    thr = -1.0 if gate is None else gate
    items, total = _items(SEGS, offs, hop, chunk, FRAMES, two)
    rc, msg, base = rate_cut(eng._lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, FRAMES, out_fmt, total, thr=thr)
    assert rc == _ffi.VAD_OK, msg
    wants, _ = _twin_payloads(twin, block, offs, lens, items, kind, sr, hop, gate, out_fmt)
    _check_written(base, items, wants, "uncapped")
    try:
        for cap in (1, 2, 5):
            eng.set_scan_launch_frames(cap)
            rc, msg, out = rate_cut(eng._lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, FRAMES, out_fmt, total, thr=thr)
            assert rc == _ffi.VAD_OK, msg
            assert out.tobytes() == base.tobytes(), (cap, int((out != base).sum()))
            _check_written(out, items, wants, ("cap", cap))
    finally:
        eng.set_scan_launch_frames(0)


# ---- f. a window that the window buffer decides ------------------------------------------------------------------------------
def buffer_window_counts():
    """1 366 recordings with a chunk, most of 96 .. 100, in no order; four without one"""
    rng = np.random.default_rng(61)
    live = 1366
    counts = rng.integers(96, 101, live)
    counts[rng.choice(live, 40, replace=False)] = np.resize([95, 96, 1, 2, 3, 5, 7, 10], 40)
    return np.insert(counts, np.sort(rng.choice(live, 4, replace=False)), 0)


def test_a_window_of_95_chunks_cut_by_the_window_buffer_changes_no_byte():
    """8 kHz, float32, hop 4.  The 256 MiB window buffer holds 131 072 frames: 1 366 live recordings get 95 chunks each per window,
    where the launch cap (192) and the longest recording (100) would allow one window.  Rows g = (item g / 95, chunk g % 95): tiles
    of 32 rows straddle items; the item table of the model launch is {i * 95 * 128, min(nframes - t0, 95)}; the second window
    (t0 = 95) runs the recordings of 96 and more chunks alone."""
    sr, kind, chunk, hop = 8000, "f32", 256, 4
    counts = buffer_window_counts()
    n, live, longest = counts.size, int((counts > 0).sum()), int(counts.max())
    fit = WIN_ROWS // live
    assert n == 1370 and live >= 683 and fit < longest <= 2 * fit < DEFAULT_CAP and fit % 32 and fit == 95
    assert {1, 95, 96, 100} <= set(counts) and (counts == 0).sum() == 4 and ((counts >= 96).sum() > 1300)
    assert launches(list(counts)) == -(-longest // fit) == 2 and launches(list(counts), 32) == 4
    rng = np.random.default_rng(62)
    lens = np.where(counts > 0, chunk + (counts - 1) * hop + rng.integers(0, hop, n), rng.integers(0, chunk, n))
    lens[np.flatnonzero(counts == 0)[0]] = 0
    pool = G.speechlike(1, 64, 512, 63).reshape(-1).astype(np.float32)
    recs = [pool[o:o + m] for o, m in zip(rng.integers(0, pool.size - int(lens.max()), n), lens)]
    eng, twin = _engine(16000, max_streams=2048), _engine(16000)
    try:
        twin.set_tile(16)
        perm = np.random.default_rng(64).permutation(n)
        fresh_slots = _open(eng, 1)
        fresh = eng.save_stream(int(fresh_slots[0]))
        _close(eng, fresh_slots)
        steps = eng.info()["steps"]
        base = _scan(eng, recs, kind, sr, hop, 0.01, order=perm)
        assert eng.info()["steps"] - steps == 2
        assert [b[0].size for b in base] == list(counts)
        try:
            eng.set_scan_launch_frames(32)
            steps = eng.info()["steps"]
            capped = _scan(eng, recs, kind, sr, hop, 0.01, order=perm)
            assert eng.info()["steps"] - steps == 4
        finally:
            eng.set_scan_launch_frames(0)
        _compare(base, capped, "window of 95 against windows of 32", seg=True)
        allp = np.concatenate([b[0] for b in base])
        assert np.isfinite(allp).all() and np.unique(allp).size > 1000
        # the twin of 64: the engine's table is sorted by count, stable and descending, in the order the recordings were listed
        order = perm[np.argsort(-counts[perm], kind="stable")]
        last_tile = order[live - live % 16:live]
        empty = order[live:]
        assert last_tile.size == 6 and counts[last_tile].max() == 2 and counts[last_tile].min() == 1 and (counts[empty] == 0).all()
        named = np.concatenate([np.flatnonzero(counts == 95)[:3], np.flatnonzero(counts == 96)[:3], last_tile, empty])
        rest = np.setdiff1d(np.arange(n), named)
        picked = np.concatenate([named, np.random.default_rng(65).choice(rest, 64 - named.size, replace=False)])
        assert picked.size == np.unique(picked).size == 64 and counts[picked].min() == 0 and counts[picked].max() == longest
        want = _twin_of(twin, ("buffer window",), [recs[i] for i in picked], sr, hop, 0.01)
        _compare([base[i] for i in picked], want, "picked against the twin")
        for i in range(n):
            assert (base[i][3] == fresh) == (counts[i] == 0), ("state moved", i)
    finally:
        eng.close()
        twin.close()


# ---- g. high addresses -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,kind,two", [(8000, "ulaw", False), (24000, "i16_32767", True), (48000, "f32", False)],
                         ids=["8000-ulaw-mono", "24000-i16-two_channels", "48000-f32-mono"])
def test_rate_scans_and_cuts_up_to_the_last_byte_below_2_gib(engines, sr, kind, two):
    """a block of 2^31 - 16 bytes, the most the argument check accepts to within a quad: the quad index shifted to a byte offset
    (quad << qsh) reaches bit 30, the descriptor's range and the offsets stay positive as 32-bit integers"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the block and torch's copies need 6 GiB")
    eng, _ = engines
    chunk = CHUNK[sr]
    hop = chunk // 4 + 4
    counts = [12, 7, 3, 9, 5]
    recs = _recordings(kind, sr, hop, seed=38, counts=counts, two=two)
    recs[4] = recs[4][:chunk + (counts[4] - 1) * hop]                  # no tail: its last sample is the block's last
    modes = [0, "mix", 1, "mix", 1] if two else None
    channels = 2 if two else 1
    size = recs[0].dtype.itemsize * channels                           # bytes of a sample frame
    nsamp = ((1 << 31) - 16) // size
    at = lambda byte: (byte // size) & ~3
    offs = [0, at(1 << 30) - (recs[1].shape[0] // 2 & ~3), 0, at(3 << 29) - 260, nsamp - recs[4].shape[0]]
    offs[2] = ((offs[1] + recs[1].shape[0] + 3) & ~3) + 4
    assert 0 < at(1 << 30) - offs[1] < chunk + (counts[1] - 1) * hop                # one of its chunks straddles byte 2^30
    assert 1 << 30 < offs[2] * size < (1 << 30) + (1 << 16)
    assert offs[3] * size < 3 << 29 < (offs[3] + recs[3].shape[0]) * size
    assert all(o % 4 == 0 for o in offs) and offs[4] + recs[4].shape[0] == nsamp and nsamp * size == (1 << 31) - 16
    want = _scan(eng, recs, kind, sr, hop, 0.01, channel=modes if two else "mix")     # the same five arrays packed into a small block
    assert [w[0].size for w in want] == counts
    small, soffs, _ = _pack(recs)
    d_small = torch.from_numpy(small).cuda()
    shape = (nsamp, 2) if two else (nsamp,)
    d_audio = torch.zeros(shape, dtype={4: torch.float32, 2: torch.int16, 1: torch.uint8}[recs[0].dtype.itemsize], device="cuda")
    try:
        for r, o in zip(recs, offs):
            d_audio[o:o + r.shape[0]] = torch.from_numpy(r).cuda()
        torch.cuda.synchronize()
        items = [(o, r.shape[0]) for o, r in zip(offs, recs)]
        got = _device_scan(eng, items, d_audio, nsamp, sr, hop, FMT[kind], 0.01, channels, modes)
        _compare(got, want, ("high addresses", kind), seg=True)
        # the offsets of two items change places: slot 1 scans the top of the block, slot 4 the samples around byte 2^30
        swapped = [items[k] for k in (0, 4, 2, 3, 1)]
        smodes = [modes[k] for k in (0, 4, 2, 3, 1)] if two else None
        got = _device_scan(eng, swapped, d_audio, nsamp, sr, hop, FMT[kind], 0.01, channels, smodes)
        _compare([got[k] for k in (0, 4, 2, 3, 1)], want, ("swapped", kind), seg=True)
        # a short segment table: the first recording, the last one up to its (and the block's) last chunk, the straddling one
        table = [(4, 1, counts[4] - 1), (0, 0, counts[0]), (1, 2, counts[1] - 2), (4, 0, 2)]
        ch = (lambda k: (modes[k],)) if two else (lambda k: ())
        for layout in ("frames", "range"):
            for gate, out in ((0.01, "pcm16"), (None, "f32")):
                a = _device_cut(eng, [(soffs[k], f, nf) + ch(k) for k, f, nf in table], d_small, small.shape[0], sr, hop, FMT[kind], gate,
                                layout, out, channels)
                b = _device_cut(eng, [(offs[k], f, nf) + ch(k) for k, f, nf in table], d_audio, nsamp, sr, hop, FMT[kind], gate, layout, out,
                                channels)
                assert a.tobytes() == b.tobytes(), (layout, out, int((a != b).sum()))
                assert np.unique(a).size > 100
    finally:
        del d_audio
        torch.cuda.empty_cache()
