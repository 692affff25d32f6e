"""Whole recordings on the GPU (vad_scan, csrc/silero_v5_t16.hip: silero_v5_scan16).  The bar is equality: a recording that the
kernel's loader frames gives BYTE FOR BYTE what vad_step_multi gives on the 16-stream tile for the same samples cut into frames by
AudioUtils.split_into_frames - probabilities, event bits, the stream's saved state - whatever the other streams of the tile do,
in which order the recordings are listed and however many launches the scan is cut into; a stream whose recording has ended is
held exactly where its last frame left it."""
import io
import os
import wave

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.utils.audio import AudioUtils
from tests import g711_ref as G
from tests.test_gpu_v5 import TOL_P       # the bar of the V5 GPU tests against the f64 oracle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = (0.3, 0.2, 0.8, 0.95, 2, 2)         # low enough for START / END events inside a few frames (tests/test_gpu_g711.py)
KINDS = ("f32", "i16_32767", "i16_32768", "ulaw", "alaw")
NREC = 37                                 # three tiles, the last one partial


def _engine(rate, max_streams=256):
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(5, rate), "rb") as f:
        return Engine(f.read(), model_version=5, max_streams=max_streams, sample_rate=rate)


@pytest.fixture(scope="module")
def engines():
    """rate -> (the scanning engine, its twin with the tile pinned to 16 streams for vad_step_multi)"""
    made = {}

    def get(rate):
        if rate not in made:
            twin = _engine(rate)
            twin.set_tile(16)
            made[rate] = (_engine(rate), twin)
        return made[rate]

    yield get
    for a, b in made.values():
        a.close()
        b.close()


def _counts(seed):
    rng = np.random.default_rng(seed)
    c = [0, 1, 40, 2, 0, 33] + [int(v) for v in rng.integers(0, 41, NREC - 6)]
    return c


def _recordings(kind, frame, hop, rate, seed, counts=None):
    """NREC recordings of 0 .. 40 frames, lengths in no order, most with a tail that framing drops; every third real speech from
    the clip's loudest stretches (events fire), the longer ones silent in their second half (segments end), the others Gaussian bursts.  G.711: recording 2 holds a frame of all 256 codes."""
    counts = _counts(seed) if counts is None else counts
    rng = np.random.default_rng(1000 + seed)
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float64) / 32768.0
    if rate == 8000:
        pcm = pcm[::2]
    recs = []
    for i, c in enumerate(counts):
        ns = (frame + (c - 1) * hop + int(rng.integers(0, hop))) if c else int(rng.integers(0, frame))
        if i % 3 == 2 and ns:
            L = 4 * frame
            energy = (pcm[:pcm.size // L * L].reshape(-1, L) ** 2).mean(axis=1)
            o = int(np.argsort(-energy, kind="stable")[(i // 3) % 8]) * L
            x = np.resize(pcm[o:o + max(ns, 1)], ns)
            if c >= 8:
                x[ns // 2:] = 0.0                        # speech, then silence: the segment ends inside the recording
        else:
            nf = -(-max(ns, 1) // frame)
            x = G.speechlike(1, nf, frame, seed * 100 + i).reshape(-1)[:ns]
        if kind == "f32":
            recs.append(x.astype(np.float32))
        elif kind.startswith("i16"):
            recs.append(np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))
        else:
            codes = G.encode(x, kind)
            if i == 2:
                codes[hop:hop + frame] = G.all_codes_frame(frame)
                assert np.unique(codes).size == 256
            recs.append(codes)
    return recs


def _args(kind, gate):
    return dict(law=kind if kind in G.LAWS else None, i16_scale=32768 if kind == "i16_32768" else 32767, denoise=gate)


def _twin_run(twin, slots, recs, frame, hop, kind, gate):
    """vad_step_multi per stream on the frames AudioUtils.split_into_frames cuts -> per recording (probs, events)"""
    out = []
    for s, r in zip(slots, recs):
        fr = AudioUtils.split_into_frames(r, frame, hop) if r.size >= frame else np.zeros((0, frame), r.dtype)
        if len(fr) == 0:
            out.append((np.zeros(0, np.float32), np.zeros(0, np.uint8)))
            continue
        p, ev = twin.step_multi([int(s)], np.ascontiguousarray(fr)[None], **_args(kind, gate))
        out.append((p[0], ev[0]))
    return out


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()))


def _open(eng, n):
    slots = eng.open_streams(n)
    eng.set_thresholds_many(slots, THR)
    return slots


def _close(eng, slots):
    for s in slots:
        eng.close_stream(int(s))


def _check_against_twin(eng, twin, recs, frame, hop, kind, gate, order=None, replay_seg=True):
    """scan(recs) on fresh slots of eng == step_multi per stream on fresh slots of twin; -> (probs, events, seg) of the scan"""
    n = len(recs)
    order = np.arange(n) if order is None else np.asarray(order)
    slots, tslots = _open(eng, n), _open(twin, n)
    spare = _open(eng, 1)
    try:
        probs, ev, seg = eng.scan(slots[order], [recs[i] for i in order], hop=hop, **_args(kind, gate))
        back = np.argsort(order)
        probs, ev, seg = ([a[int(k)] for k in back] for a in (probs, ev, seg))
        want = _twin_run(twin, tslots, recs, frame, hop, kind, gate)
        for i in range(n):
            _same_bytes(probs[i], want[i][0], ("probs", kind, i))
            _same_bytes(ev[i], want[i][1], ("events", kind, i))
            assert eng.save_stream(int(slots[i])) == twin.save_stream(int(tslots[i])), ("state", kind, i)
            assert seg[i].dtype == np.int32 and seg[i].shape == ev[i].shape
            if replay_seg and probs[i].size and np.isfinite(probs[i]).all():
                eng.reset(spare)
                eng.set_thresholds_many(spare, THR)
                ev_r, seg_r = eng.debug_sm_replay(int(spare[0]), probs[i])
                assert np.array_equal(ev_r, ev[i]) and np.array_equal(seg_r, seg[i]), ("seg", kind, i)
        return probs, ev, seg
    finally:
        _close(eng, slots)
        _close(eng, spare)
        _close(twin, tslots)


@pytest.mark.parametrize("hop_div", [2, 1], ids=["hop_half", "hop_frame"])
@pytest.mark.parametrize("gate", [0.01, None], ids=["gate", "nogate"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
def test_scan_equals_step_multi_on_split_frames(engines, rate, kind, gate, hop_div):
    eng, twin = engines(rate)
    frame = eng.frame_samples
    hop = frame // hop_div
    recs = _recordings(kind, frame, hop, rate, seed=3 + hop_div)
    probs, ev, seg = _check_against_twin(eng, twin, recs, frame, hop, kind, gate)
    allp = np.concatenate(probs)
    assert np.isfinite(allp).all() and (allp >= 0).all() and (allp <= 1).all()
    assert sum(int(((e & _ffi.VAD_EV_END) != 0).sum()) for e in ev) >= 1, "no segment ended: the comparison of seg_frames would be empty"
    for e, g in zip(ev, seg):
        assert ((g > 0) == ((e & _ffi.VAD_EV_END) != 0)).all()


@pytest.mark.parametrize("kind", ["f32", "i16_32767", "ulaw"])
def test_order_launch_cap_and_device_audio_do_not_change_a_byte(engines, kind):
    import torch
    eng, twin = engines(16000)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs = _recordings(kind, frame, hop, 16000, seed=11, counts=_counts(11)[:-1] + [9])
    # the last recording has no tail and the block below ends with its last sample: the descriptor's range ends there too, and an
    # int16 quad is a 16-byte load of which 8 bytes are used - the final one is half out of range (range-checked per dword)
    recs[-1] = recs[-1][:frame + 8 * hop]
    base = _check_against_twin(eng, twin, recs, frame, hop, kind, 0.01)
    assert base[0][-1].size == 9
    perm = np.random.default_rng(5).permutation(len(recs))
    try:
        for cap, order in ((0, perm), (1, None), (7, perm), (0, None)):
            eng.set_scan_launch_frames(cap)
            got = _check_against_twin(eng, twin, recs, frame, hop, kind, 0.01, order=order, replay_seg=False)
            for a, b in zip(base, got):
                for i in range(len(recs)):
                    _same_bytes(a[i], b[i], (kind, cap, i))
    finally:
        eng.set_scan_launch_frames(0)
    # vad_scan_device on audio that already lies in HBM
    lens = np.array([r.size for r in recs])
    offs = np.concatenate([[0], np.cumsum((lens[:-1] + 3) & ~3)])
    block = np.zeros(int(offs[-1] + lens[-1]), recs[0].dtype)
    assert block.size == offs[-1] + frame + 8 * hop
    for r, o in zip(recs, offs):
        block[o:o + r.size] = r
    fmt = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "ulaw": _ffi.VAD_FMT_ULAW8}[kind]
    slots = _open(eng, len(recs))
    try:
        d_audio = torch.from_numpy(block).cuda()
        total = sum(p.size for p in base[0])
        d_p = torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda")
        d_e = torch.full((total + 8,), 0x55, dtype=torch.uint8, device="cuda")
        d_s = torch.full((total + 8,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        start = eng.scan_device(slots, offs, lens, d_audio.data_ptr(), block.size, d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(),
                                hop=hop, fmt=fmt, denoise=0.01)
        eng.synchronize()
        p, e, s = d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()
        assert int(start[-1]) == total
        for i in range(len(recs)):
            for got, want in ((p, base[0]), (e, base[1]), (s, base[2])):
                _same_bytes(got[start[i]:start[i + 1]], want[i], ("device", kind, i))
        assert (p[total:] == -7.0).all() and (e[total:] == 0x55).all() and (s[total:] == -9).all()
    finally:
        _close(eng, slots)


@pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
def test_ended_streams_are_held_and_go_on_like_the_twin(engines, rate):
    eng, twin = engines(rate)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(21)
    counts = _counts(8)
    recs = _recordings("f32", frame, hop, rate, seed=8, counts=counts)
    n = len(recs)
    slots, tslots = _open(eng, n), _open(twin, n)
    try:
        for _ in range(3):                               # every stream has a history: (h, c) and state machine are not the fresh ones
            x = (rng.standard_normal((n, frame)) * 0.3).astype(np.float32)
            eng.step(slots, x)
            twin.step(tslots, x)
        before = [eng.save_stream(int(s)) for s in slots]
        eng.set_scan_launch_frames(9)
        probs, ev, _ = eng.scan(slots, recs, hop=hop)
        want = _twin_run(twin, tslots, recs, frame, hop, "f32", 0.01)
        after = [eng.save_stream(int(s)) for s in slots]
        empty = [i for i, c in enumerate(counts) if c == 0]
        assert len(empty) >= 2
        for i in range(n):
            _same_bytes(probs[i], want[i][0], ("probs", i))
            _same_bytes(ev[i], want[i][1], ("events", i))
            assert after[i] == twin.save_stream(int(tslots[i])), i
            assert (after[i] == before[i]) == (i in empty), i
        x = (rng.standard_normal((n, frame)) * 0.3).astype(np.float32)
        a, b = eng.step_events(slots, x), twin.step_events(tslots, x)
        for u, v in zip(a, b):
            _same_bytes(u, v, "the step after the scan")
    finally:
        eng.set_scan_launch_frames(0)
        _close(eng, slots)
        _close(twin, tslots)


@pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
def test_non_finite_samples_reject_both_frames_that_hold_them(engines, rate):
    eng, twin = engines(rate)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    counts = [12, 9, 5, 12, 0, 7] + [6] * 14
    clean = _recordings("f32", frame, hop, rate, seed=13, counts=counts)
    recs = [r.copy() for r in clean]
    # sample 5 hop + 17 lies in the overlap of frames 4 and 5; sample 3 hop - 1 in that of frames 1 and 2
    recs[0][5 * hop + 17] = np.nan
    recs[3][3 * hop - 1] = np.inf
    for gate in (0.01, None):
        probs, ev, seg = _check_against_twin(eng, twin, recs, frame, hop, "f32", gate, replay_seg=False)
        ref = _check_against_twin(eng, twin, clean, frame, hop, "f32", gate)
        for i, bad in ((0, (4, 5)), (3, (1, 2))):
            rej = (ev[i] & _ffi.VAD_EV_REJECTED) != 0
            assert list(np.flatnonzero(rej)) == list(bad), (i, np.flatnonzero(rej))
            assert (ev[i][rej] == _ffi.VAD_EV_REJECTED).all() and np.isnan(probs[i][rej]).all() and not seg[i][rej].any()
            assert np.isfinite(probs[i][~rej]).all()
            # the frames before the first rejected one are the clean run's
            _same_bytes(probs[i][:bad[0]], ref[0][i][:bad[0]], ("before the rejected frames", i))
        for i in range(len(recs)):
            if i not in (0, 3):                          # the neighbours in the tile: the clean run's bytes
                for a, b in zip((probs, ev, seg), ref):
                    _same_bytes(a[i], b[i], ("neighbour", i))


def test_probabilities_match_the_f64_oracle(engines):
    from oracle import oracle
    eng, _ = engines(16000)
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        om = oracle.OracleModel(f.read(), "f64")
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs = _recordings("f32", frame, hop, 16000, seed=17)
    slots = eng.open_streams(len(recs))
    try:
        probs, _, _ = eng.scan(slots, recs, hop=hop, denoise=0.01)
        worst, checked = 0.0, 0
        for i, r in enumerate(recs):
            if r.size < frame:
                assert probs[i].size == 0
                continue
            fr = AudioUtils.split_into_frames(r, frame, hop)
            st = np.zeros((1, 256), np.float32)
            ref = np.array([om.step_batch(oracle.denoise(f[None], 0.01).reshape(1, frame), st, nthreads=8)[0] for f in fr], np.float32)
            assert probs[i].shape == ref.shape
            worst = max(worst, float(np.abs(probs[i] - ref).max()))
            checked += ref.size
            st_gpu = eng.get_state(int(slots[i]))
            assert np.abs(st_gpu - st[0]).max() <= 2e-4            # tests/test_gpu_v5.py TOL_S
        print(f"scan vs f64 oracle: max |dp| = {worst:.3e} over {checked} frames (bar {TOL_P})")
        assert checked > 400 and worst <= TOL_P
    finally:
        _close(eng, slots)


def _wav_samples(w):
    with wave.open(io.BytesIO(w)) as f:
        return f.getnframes()


@pytest.mark.parametrize("cfg_kw", [{}, dict(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6,
                                             voice_end_frame_count=12)], ids=["default", "client"])
def test_scan_recordings_gives_the_wrappers_segments(cfg_kw):
    """the speech golden, whole and in parts, as one ragged batch: per recording the number of segments and each one's length are
    what VADWrapper.process_audio_data's voice_end callbacks deliver for the same array (payload = seg_frames * frame samples)"""
    from cutter_vad_amd import VADConfig, VADWrapper, scan_recordings
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float32) / np.float32(32767.0)
    cfg = VADConfig(**cfg_kw)
    frame, hop = 512, 256
    recs = [pcm, pcm[:pcm.size // 2], pcm[pcm.size // 3:], pcm[:300]]
    got = scan_recordings(recs, cfg)
    assert len(got) == len(recs)
    total = 0
    for x, segs in zip(recs, got):
        wavs = []
        with VADWrapper(config=cfg) as vad:
            vad.set_callbacks(None, wavs.append, None)
            if x.size >= frame:
                vad.process_audio_data(x)
        assert len(segs) == len(wavs), (len(segs), len(wavs))
        for (a, b), w in zip(segs, wavs):
            L = (b - a - frame) // hop + 1
            assert (L - 1) * hop + frame == b - a and 0 <= a and b <= x.size
            assert _wav_samples(w) == L * frame, (a, b, L, _wav_samples(w))
        total += len(segs)
    print(f"scan_recordings [{'client' if cfg_kw else 'default'}]: segments per recording {[len(g) for g in got]}")
    # the comparison is not between empty lists: the clip holds utterances that either configuration finds
    assert total >= (4 if cfg_kw else 1), total
