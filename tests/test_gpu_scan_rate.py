"""Whole recordings at 8 / 24 / 48 kHz on the GPU (vad_scan_rate, csrc/scan_resample.hip: vadk_scan_resample in front of the
unchanged silero_v5_scan16).  Every bar is BYTE equality with paths that are already held to scipy and to the f64 oracle.  The twin
of a recording: decoded and channel-selected on the host to float32 (the exact IEEE quotient float32(s) / float32(scale), the G.711
table / 32768, np.float32 mean of the decoded pair), AudioUtils.split_into_frames(x, chunk, hop), Engine.resample(chunks, sr_in)
(tests/test_gpu_resample.py), then vad_step_multi on a second engine pinned to 16-stream tiles with the same gate
(tests/test_gpu_scan.py's twin).

Inputs follow tests/test_gpu_scan.py at the input rate: 37 recordings of 0 .. 40 chunks in no order - three 16-stream tiles and two
32-row resample tiles per window frame, both with a partial last one - most with a tail that is dropped, one shorter than a chunk,
one empty; every third real speech from the clip's loudest stretches, repeated or decimated to the input rate and silent in its
second half, the others Gaussian bursts."""
import ctypes as C
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from cutter_vad_amd.scan import speech_segments
from cutter_vad_amd.utils.audio import AudioUtils
from tests import g711_ref as G
from tests.test_gpu_scan import NREC, THR, _args, _close, _counts, _engine, _open, _same_bytes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}
CHUNK = {8000: 256, 24000: 768, 48000: 1536}
CYCLE = (0, 1, "mix")


@pytest.fixture(scope="module")
def engines():
    """(the engine that scans at other rates, its twin with the tile pinned to 16 streams for vad_resample + vad_step_multi)"""
    eng, twin = _engine(16000), _engine(16000)
    twin.set_tile(16)
    yield eng, twin
    eng.close()
    twin.close()


def _recordings(kind, sr, hop, seed, counts=None, two=False):
    """NREC recordings at `sr`, lengths in input samples; two: [nsamples, 2], on the right the content of recording (i + 3) mod n"""
    chunk = CHUNK[sr]
    counts = _counts(seed) if counts is None else counts
    rng = np.random.default_rng(1000 + seed)
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float64) / 32768.0
    recs = []
    for i, c in enumerate(counts):
        # without a chunk: the first such recording is empty, the others shorter than a chunk
        ns = (chunk + (c - 1) * hop + int(rng.integers(0, hop))) if c else (int(rng.integers(1, chunk)) if 0 in counts[:i] else 0)
        at16 = (np.arange(ns) * 16000) // sr              # the 16 kHz sample under every input sample: repeated, or decimated
        n16 = int(at16[-1]) + 1 if ns else 0
        if i % 3 == 2 and ns:
            L = 2048
            energy = (pcm[:pcm.size // L * L].reshape(-1, L) ** 2).mean(axis=1)
            o = int(np.argsort(-energy, kind="stable")[(i // 3) % 8]) * L
            x = np.resize(pcm[o:o + n16], n16)[at16]
            if c >= 8:
                x[ns // 2:] = 0.0                         # speech, then silence: the segment ends inside the recording
        else:
            x = G.speechlike(1, -(-max(n16, 1) // 512), 512, seed * 100 + i).reshape(-1)[:n16][at16]
        if kind == "f32":
            recs.append(x.astype(np.float32))
        elif kind.startswith("i16"):
            recs.append(np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))
        else:
            recs.append(G.encode(x, kind))
    if two:
        n = len(recs)
        recs = [np.ascontiguousarray(np.stack([recs[i], np.resize(recs[(i + 3) % n], recs[i].size)], axis=1)) for i in range(n)]
    return recs


def _decoded(x, kind):
    if kind == "f32":
        return x
    if kind.startswith("i16"):
        return x.astype(np.float32) / np.float32(32767.0 if kind == "i16_32767" else 32768.0)
    return G.table(kind)[x].astype(np.float32) / np.float32(32768.0)


def _heard(x, kind, m=None):
    """the float32 array a host would have prepared of recording x (mode m of a two-channel one)"""
    d = _decoded(x, kind)
    assert d.dtype == np.float32
    if x.ndim == 1:
        return d
    if m in (0, 1):
        return np.ascontiguousarray(d[:, m])
    with np.errstate(over="ignore", invalid="ignore"):
        return np.mean(d, axis=1)


def _twin_run(twin, tslots, heard, sr, hop, gate):
    """split_into_frames -> Engine.resample (one call for the batch) -> vad_step_multi per stream -> per recording (probs, events)"""
    chunk = CHUNK[sr]
    chunks = [AudioUtils.split_into_frames(x, chunk, hop) if x.size >= chunk else np.zeros((0, chunk), np.float32) for x in heard]
    allc = np.ascontiguousarray(np.concatenate(chunks), np.float32)
    frames = twin.resample(allc, sr) if len(allc) else np.zeros((0, 512), np.float32)
    out, at = [], 0
    for s, c in zip(tslots, chunks):
        fr = frames[at:at + len(c)]
        at += len(c)
        if len(c) == 0:
            out.append((np.zeros(0, np.float32), np.zeros(0, np.uint8)))
            continue
        p, ev = twin.step_multi([int(s)], np.ascontiguousarray(fr)[None], denoise=gate)
        out.append((p[0], ev[0]))
    return out


_TWINS = {}


def _twin_of(twin, key, heard, sr, hop, gate):
    """the twin of a batch on fresh slots, once -> per recording (probs, events, saved state)"""
    key = key + (sr, hop, gate)
    if key not in _TWINS:
        tslots = _open(twin, len(heard))
        try:
            run = _twin_run(twin, tslots, heard, sr, hop, gate)
            _TWINS[key] = [(p.copy(), e.copy(), twin.save_stream(int(s))) for (p, e), s in zip(run, tslots)]
        finally:
            _close(twin, tslots)
    return _TWINS[key]


def _scan(eng, recs, kind, sr, hop, gate, order=None, channel="mix"):
    """Engine.scan(sample_rate=sr) on fresh slots -> per recording (probs, events, seg, saved state), in the recordings' order"""
    n = len(recs)
    order = np.arange(n) if order is None else np.asarray(order)
    slots = _open(eng, n)
    try:
        ch = channel if isinstance(channel, (str, int)) else [channel[i] for i in order]
        p, e, g = eng.scan(slots[order], [recs[i] for i in order], hop=hop, sample_rate=sr, channel=ch, **_args(kind, gate))
        back = np.argsort(order)
        return [(p[int(back[i])], e[int(back[i])], g[int(back[i])], eng.save_stream(int(slots[i]))) for i in range(n)]
    finally:
        _close(eng, slots)


def _compare(got, want, what, seg=False):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        _same_bytes(a[0], b[0], ("probs", what, i))
        _same_bytes(a[1], b[1], ("events", what, i))
        if seg:
            _same_bytes(a[2], b[2], ("seg_frames", what, i))
        assert a[3] == b[-1], ("state", what, i)


def _check_seg_and_ends(eng, got, what):
    """seg_frames = vad_debug_sm_replay of the probabilities, on every END frame and nowhere else; at least one END"""
    spare = _open(eng, 1)
    try:
        ends = 0
        for i, (p, e, g, _) in enumerate(got):
            assert g.dtype == np.int32 and g.shape == e.shape == p.shape
            assert ((g > 0) == ((e & _ffi.VAD_EV_END) != 0)).all()
            ends += int(((e & _ffi.VAD_EV_END) != 0).sum())
            if p.size and np.isfinite(p).all():
                eng.reset(spare)
                eng.set_thresholds_many(spare, THR)
                ev_r, seg_r = eng.debug_sm_replay(int(spare[0]), p)
                assert np.array_equal(ev_r, e) and np.array_equal(seg_r, g), ("seg", what, i)
        assert ends >= 1, (what, "no segment ended: the comparison of seg_frames would be empty")
    finally:
        _close(eng, spare)


def _equality_cases():
    out = []
    for sr in (8000, 24000, 48000):
        for kind in ("f32", "i16_32767", "ulaw"):
            for gate in (0.01, None):
                out.append(pytest.param(sr, kind, gate, 2, id=f"{sr}-{kind}-{'gate' if gate else 'nogate'}"))
    out.append(pytest.param(24000, "i16_32768", 0.01, 2, id="24000-i16_32768-gate"))
    out.append(pytest.param(8000, "alaw", 0.01, 2, id="8000-alaw-gate"))
    out.append(pytest.param(48000, "i16_32767", 0.01, 1, id="48000-i16_32767-gate-hop_chunk"))
    return out


@pytest.mark.parametrize("sr,kind,gate,hop_div", _equality_cases())
def test_rate_scan_equals_resample_and_step_multi_on_split_chunks(engines, sr, kind, gate, hop_div):
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // hop_div
    recs = _recordings(kind, sr, hop, seed=3 + hop_div)
    assert len(recs) == NREC and max(r.size for r in recs) >= chunk + 39 * hop and min(r.size for r in recs) == 0
    assert any(0 < r.size < chunk for r in recs)
    want = _twin_of(twin, ("mono", kind, 3 + hop_div), [_heard(r, kind) for r in recs], sr, hop, gate)
    got = _scan(eng, recs, kind, sr, hop, gate)
    _compare(got, want, (sr, kind, gate, hop))
    allp = np.concatenate([g[0] for g in got])
    assert np.isfinite(allp).all() and (allp >= 0).all() and (allp <= 1).all()
    _check_seg_and_ends(eng, got, (sr, kind, gate, hop))


def test_order_window_and_device_audio_do_not_change_a_byte(engines):
    import torch
    eng, twin = engines
    sr, kind = 24000, "i16_32767"
    chunk = CHUNK[sr]
    hop = chunk // 2
    recs = _recordings(kind, sr, hop, seed=11, counts=_counts(11)[:-1] + [9])
    recs[-1] = recs[-1][:chunk + 8 * hop]                 # no tail: the block below ends with the last chunk's last sample
    want = _twin_of(twin, ("caps", kind), [_heard(r, kind) for r in recs], sr, hop, 0.01)
    base = _scan(eng, recs, kind, sr, hop, 0.01)
    _compare(base, want, "default window")
    assert base[-1][0].size == 9
    perm = np.random.default_rng(5).permutation(len(recs))
    steps = eng.info()["steps"]
    try:
        for cap, order in ((0, perm), (1, None), (3, perm), (7, None)):
            eng.set_scan_launch_frames(cap)
            got = _scan(eng, recs, kind, sr, hop, 0.01, order=order)
            _compare(got, base, ("cap", cap), seg=True)
    finally:
        eng.set_scan_launch_frames(0)
    assert eng.info()["steps"] - steps == 1 + 40 + 14 + 6                   # the model launches of 40 chunks under each cap
    # vad_scan_rate_device on a block that already lies in HBM, device result arrays
    lens = np.array([r.size for r in recs])
    offs = np.concatenate([[0], np.cumsum((lens[:-1] + 3) & ~3)])
    block = np.zeros(int(offs[-1] + lens[-1]), recs[0].dtype)
    for r, o in zip(recs, offs):
        block[o:o + r.size] = r
    slots = _open(eng, len(recs))
    try:
        d_audio = torch.from_numpy(block).cuda()
        total = sum(b[0].size for b in base)
        d_p = torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda")
        d_e = torch.full((total + 8,), 0x55, dtype=torch.uint8, device="cuda")
        d_s = torch.full((total + 8,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        start = eng.scan_device(slots, offs, lens, d_audio.data_ptr(), block.size, d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(),
                                hop=hop, fmt=FMT[kind], denoise=0.01, sample_rate=sr)
        eng.synchronize()
        p, e, s = d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()
        assert int(start[-1]) == total
        got = [(p[start[i]:start[i + 1]], e[start[i]:start[i + 1]], s[start[i]:start[i + 1]], eng.save_stream(int(slots[i])))
               for i in range(len(recs))]
        _compare(got, base, "device", seg=True)
        assert (p[total:] == -7.0).all() and (e[total:] == 0x55).all() and (s[total:] == -9).all()
    finally:
        _close(eng, slots)


def test_more_than_256_resample_tiles_in_a_window(engines):
    """220 recordings of 38 .. 40 chunks: a window of 40 chunks is 8 800 rows = 275 tiles of 32, past the 256 up to which two
    workgroups share a tile - the kernel's other instantiation (as vadk_resample_512's).  Equal to the twin, whose own resample
    call takes that path too."""
    eng, twin = engines
    sr, kind = 8000, "f32"
    chunk = CHUNK[sr]
    hop = chunk // 2
    counts = [40 - (i % 3) for i in range(220)]
    assert -(-len(counts) * max(counts) // 32) > 256
    recs = _recordings(kind, sr, hop, seed=29, counts=counts)
    want = _twin_of(twin, ("wide",), recs, sr, hop, 0.01)
    steps = eng.info()["steps"]
    got = _scan(eng, recs, kind, sr, hop, 0.01)
    assert eng.info()["steps"] - steps == 1                # one window: all 8 800 rows in one resample launch
    _compare(got, want, "275 tiles")


def test_the_window_buffers_bound_cuts_the_window_and_changes_no_byte():
    """704 recordings of 192 chunks: 704 x 192 frames of 2 KiB are more than the 256 MiB the engine keeps for one window, so the
    default window of 192 is cut to 186 chunks - two model launches where the cap alone would give one.  Byte-equal to the same
    scan in windows of 64."""
    sr, chunk = 8000, 256
    hop = chunk // 2
    n, nf = 704, 192
    assert n * nf * 2048 > 256 << 20 and (256 << 20) // (n * 2048) == 186
    rng = np.random.default_rng(31)
    recs = [G.encode(0.2 * rng.standard_normal(chunk + (nf - 1) * hop + int(k)), "ulaw") for k in rng.integers(0, hop, n)]
    eng = _engine(16000, max_streams=1024)
    try:
        runs = []
        for cap, launches in ((0, 2), (64, 3)):
            eng.set_scan_launch_frames(cap)
            steps = eng.info()["steps"]
            runs.append(_scan(eng, recs, "ulaw", sr, hop, 0.01))
            assert eng.info()["steps"] - steps == launches, cap
        assert all(r[0].size == nf for r in runs[0])
        _compare(runs[0], runs[1], "bound", seg=True)
    finally:
        eng.close()


@pytest.mark.parametrize("sr,kind", [(48000, "f32"), (24000, "i16_32767"), (8000, "ulaw")])
def test_two_channels_equal_the_mono_rate_scan_of_the_prepared_array(engines, sr, kind):
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // 2
    recs = _recordings(kind, sr, hop, seed=3, two=True)
    n = len(recs)
    # the mono vad_scan_rate of what a host would have prepared: the channel's own samples in the wire format, or the float32 mean
    refs = {}
    for m in CYCLE:
        mono = [np.ascontiguousarray(x[:, m]) for x in recs] if m in (0, 1) else [_heard(x, kind, "mix") for x in recs]
        refs[m] = _scan(twin, mono, kind if m in (0, 1) else "f32", sr, hop, 0.01)
    differ = lambda a, b: sum(refs[a][i][0].tobytes() != refs[b][i][0].tobytes() for i in range(n))
    assert differ(0, 1) >= 10 and differ("mix", 0) >= 10 and differ("mix", 1) >= 10
    for m in CYCLE:
        _compare(_scan(eng, recs, kind, sr, hop, 0.01, channel=m), refs[m], (sr, kind, m), seg=True)
    modes = [CYCLE[i % 3] for i in range(n)]
    _compare(_scan(eng, recs, kind, sr, hop, 0.01, channel=modes), [refs[m][i] for i, m in enumerate(modes)], (sr, kind, "cycle"), seg=True)
    # both channels of every recording on two slots in one call
    slots = np.asarray(_open(eng, 2 * n)).reshape(n, 2)
    try:
        p, e, g = eng.scan(slots, recs, hop=hop, sample_rate=sr, channel="split", **_args(kind, 0.01))
        got = [(p[i][c], e[i][c], g[i][c], eng.save_stream(int(slots[i, c]))) for i in range(n) for c in (0, 1)]
        _compare(got, [refs[c][i] for i in range(n) for c in (0, 1)], (sr, kind, "split"), seg=True)
    finally:
        _close(eng, slots.reshape(-1))


def test_held_streams_and_a_second_scan_go_on_like_the_twin(engines):
    eng, twin = engines
    sr, kind = 48000, "f32"
    chunk = CHUNK[sr]
    hop = chunk // 2
    first = _recordings(kind, sr, hop, seed=8)
    counts2 = list(reversed(_counts(9)))
    second = _recordings(kind, sr, hop, seed=9, counts=counts2)
    empty = [i for i, c in enumerate(counts2) if c == 0]
    assert len(empty) >= 2
    n = len(first)
    slots, tslots = _open(eng, n), _open(twin, n)
    try:
        eng.set_scan_launch_frames(9)
        for recs in (first, second):
            before = [eng.save_stream(int(s)) for s in slots]
            probs, ev, _ = eng.scan(slots, recs, hop=hop, sample_rate=sr)
            want = _twin_run(twin, tslots, recs, sr, hop, 0.01)
            after = [eng.save_stream(int(s)) for s in slots]
            for i in range(n):
                _same_bytes(probs[i], want[i][0], ("probs", i))
                _same_bytes(ev[i], want[i][1], ("events", i))
                assert after[i] == twin.save_stream(int(tslots[i])), i
                if recs is second:
                    assert (after[i] == before[i]) == (i in empty), i
    finally:
        eng.set_scan_launch_frames(0)
        _close(eng, slots)
        _close(twin, tslots)


def _rejected(ev):
    return list(np.flatnonzero((ev & _ffi.VAD_EV_REJECTED) != 0))


@pytest.mark.parametrize("sr", [8000, 48000])
def test_a_nan_or_inf_rejects_every_chunk_that_holds_it(engines, sr):
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // 2
    counts = [12, 9, 5, 12, 0, 7] + [6] * 14
    clean = _recordings("f32", sr, hop, seed=13, counts=counts)
    recs = [r.copy() for r in clean]
    # sample 5 hop + 17 lies in the overlap of chunks 4 and 5; sample 3 hop - 1 in that of chunks 1 and 2
    recs[0][5 * hop + 17] = np.nan
    recs[3][3 * hop - 1] = np.inf
    for gate in (0.01, None):
        want = _twin_of(twin, ("nonfinite",), recs, sr, hop, gate)
        got = _scan(eng, recs, "f32", sr, hop, gate)
        _compare(got, want, ("nonfinite", sr, gate))
        ref = _scan(eng, clean, "f32", sr, hop, gate)
        for i, bad in ((0, [4, 5]), (3, [1, 2])):
            p, e, g, _ = got[i]
            assert _rejected(e) == bad, (i, _rejected(e))
            rej = (e & _ffi.VAD_EV_REJECTED) != 0
            assert (e[rej] == _ffi.VAD_EV_REJECTED).all() and np.isnan(p[rej]).all() and not g[rej].any()
            assert np.isfinite(p[~rej]).all()
            _same_bytes(p[:bad[0]], ref[i][0][:bad[0]], ("before the rejected chunks", i))
        for i in range(len(recs)):
            if i not in (0, 3):                           # the neighbours in the tiles: the clean run's bytes
                _compare([got[i]], [ref[i]], ("neighbour", i), seg=True)
    # two channels: a NaN in the channel that is not selected rejects nothing; in the mix it does
    two = [np.ascontiguousarray(np.stack([c, r], axis=1)) for c, r in zip(clean, recs)]
    left = _scan(eng, two, "f32", sr, hop, 0.01, channel=0)
    _compare(left, _scan(eng, clean, "f32", sr, hop, 0.01), ("left", sr), seg=True)
    assert all(_rejected(e) == [] for _, e, _, _ in left)
    mix = _scan(eng, two, "f32", sr, hop, 0.01, channel="mix")
    assert _rejected(mix[0][1]) == [4, 5] and _rejected(mix[3][1]) == [1, 2]


def test_16_khz_is_vad_scan_channels(engines):
    eng, _ = engines
    lib = eng._lib
    hop = 256
    recs = _recordings("i16_32767", 8000, hop, seed=4, two=True)        # lengths for 512-sample frames at hop 256 as well
    lens = np.array([r.shape[0] for r in recs])
    offs = np.concatenate([[0], np.cumsum((lens[:-1] + 3) & ~3)])
    block = np.zeros((int(offs[-1] + lens[-1]), 2), np.int16)
    for r, o in zip(recs, offs):
        block[o:o + r.shape[0]] = r
    n = len(recs)
    slots = _open(eng, n)
    try:
        items = (_ffi.ScanChItem * n)(*[_ffi.ScanChItem(int(slots[i]), int(offs[i]), int(lens[i]), (0, 1, _ffi.VAD_SCAN_MIX)[i % 3], 0)
                                        for i in range(n)])
        start = np.concatenate([[0], np.cumsum([eng.scan_frame_count(int(v), hop) for v in lens])]).astype(np.int64)
        assert start[-1] > 300
        outs = []
        for call in ("channels", "rate"):
            eng.reset(slots)
            eng.set_thresholds_many(slots, THR)
            p = np.full(int(start[-1]), -7.0, np.float32)
            e = np.full(int(start[-1]), 0x55, np.uint8)
            g = np.full(int(start[-1]), -9, np.int32)
            tail = (start.ctypes.data_as(C.POINTER(C.c_int64)), p.ctypes.data_as(C.POINTER(C.c_float)),
                    e.ctypes.data_as(C.POINTER(C.c_uint8)), g.ctypes.data_as(C.POINTER(C.c_int32)))
            head = (eng.handle, items, n, block.ctypes.data_as(C.c_void_p), block.shape[0], 2, FMT["i16_32767"])
            if call == "channels":
                rc = lib.vad_scan_channels(*head, hop, 0.01, *tail)
            else:
                rc = lib.vad_scan_rate(*head, 16000, hop, 0.01, *tail)
            assert rc == _ffi.VAD_OK, lib.vad_last_error(eng.handle).decode()
            outs.append((p, e, g, [eng.save_stream(int(s)) for s in slots]))
        for a, b in zip(outs[0][:3], outs[1][:3]):
            _same_bytes(a, b, "16 kHz")
        assert outs[0][3] == outs[1][3]
        assert ((outs[0][1] & _ffi.VAD_EV_END) != 0).any()
    finally:
        _close(eng, slots)


@pytest.mark.parametrize("sr", [24000, 48000])
def test_scan_recordings_gives_the_twins_segments_in_input_rate_samples(engines, sr):
    from cutter_vad_amd import VADConfig, scan_recordings
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // 2
    counts = [20, 0, 33, 7, 1, 40, 12, 3, 26]
    mono = _recordings("f32", sr, hop, seed=17, counts=counts)
    stereo = _recordings("f32", sr, hop, seed=17, counts=counts, two=True)
    recs = [stereo[i] if i % 2 else mono[i] for i in range(len(counts))]          # 1-D and 2-D mixed
    cfg = VADConfig(vad_start_probability=THR[0], vad_end_probability=THR[1], voice_start_ratio=THR[2], voice_end_ratio=THR[3],
                    voice_start_frame_count=THR[4], voice_end_frame_count=THR[5], enable_denoising=True)
    got = scan_recordings(recs, cfg, engine=eng, sample_rate=sr)
    heard = [_heard(r, "f32", "mix") for r in recs]
    want = _twin_of(twin, ("corpus",), heard, sr, hop, 0.01)
    spare = _open(eng, 1)
    try:
        segs = []
        for p, e, _ in want:
            eng.reset(spare)
            eng.set_thresholds_many(spare, THR)
            ev_r, seg_r = (eng.debug_sm_replay(int(spare[0]), p) if p.size else (np.zeros(0, np.uint8), np.zeros(0, np.int32)))
            assert np.array_equal(ev_r, e)
            segs.append(speech_segments(e, seg_r, chunk, hop))
    finally:
        _close(eng, spare)
    assert got == segs
    assert sum(len(s) for s in segs) >= 2, "no segment: the comparison would be between empty lists"
    for x, one in zip(recs, got):
        assert all(0 <= a < b <= x.shape[0] and a % hop == 0 and (b - chunk) % hop == 0 for a, b in one)
    stats = scan_recordings(recs, cfg, engine=eng, sample_rate=sr, stats=True)
    assert [[s[:2] for s in one] for one in stats] == segs and all(0 < s[2] <= s[3] <= 1 for one in stats for s in one)
    assert scan_recordings(recs, cfg, engine=eng, sample_rate=sr, channel=0)[::2] == got[::2]     # 1-D recordings ignore the channel
