"""Interleaved two-channel recordings on the GPU (vad_scan_channels, csrc/silero_v5_t16.hip: silero_v5_stereo16).  The bar is
equality with the mono scan, which tests/test_gpu_scan.py holds to vad_step_multi and the f64 oracle: for every item the
probabilities, the events, seg_frames and the stream's saved state are BYTE FOR BYTE what Engine.scan gives, on a second engine,
for the 1-D array a host would have prepared - np.ascontiguousarray(x[:, c]) for a selected channel; for the mix np.mean over the
channels of the float32 array, and for int16 / G.711 input the mean of the decoded channels (float32(s) / float32(scale),
table / 32768), scanned as float32.

Inputs: the recordings of tests/test_gpu_scan.py on the left, on the right the content of recording (i + 3) mod 37 resized to the
same length - speech faces bursts, so a loader that reads the wrong channel, or the right one for the wrong item, cannot pass."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import g711_ref as G
from tests.test_gpu_scan import KINDS, THR, _args, _close, _counts, _engine, _open, _recordings, _same_bytes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}
RATES = pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
MODES = ("left", "right", "mix", "split", "cycle")
SEED = 3
CYCLE = (0, 1, "mix")


@pytest.fixture(scope="module")
def engines():
    """rate -> (the engine that scans two-channel blocks, the engine of the mono references)"""
    made = {}

    def get(rate):
        if rate not in made:
            made[rate] = (_engine(rate), _engine(rate))
        return made[rate]

    yield get
    for a, b in made.values():
        a.close()
        b.close()


def _stereo(kind, frame, hop, rate, seed, counts=None):
    left = _recordings(kind, frame, hop, rate, seed, counts)
    n = len(left)
    return [np.ascontiguousarray(np.stack([left[i], np.resize(left[(i + 3) % n], left[i].size)], axis=1)) for i in range(n)]


def _decoded(x, kind):
    if kind == "f32":
        return x
    if kind.startswith("i16"):
        return x.astype(np.float32) / np.float32(32767.0 if kind == "i16_32767" else 32768.0)
    return G.table(kind)[x].astype(np.float32) / np.float32(32768.0)


def _mono(x, kind, m):
    """what a host would have prepared for mode m of the two-channel recording x -> (1-D array, its kind)"""
    if m in (0, 1):
        return np.ascontiguousarray(x[:, m]), kind
    d = _decoded(x, kind)
    assert d.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):              # the non-finite cases: a sum that overflows, Inf - Inf
        return np.mean(d, axis=1), "f32"


_REFS = {}


def _reference(ref, tag, recs, kind, hop, gate, m):
    """the mono scan of mode m of every recording, once per batch -> per recording (probs, events, seg, saved state)"""
    key = (tag, kind, hop, gate, m)
    if key not in _REFS:
        mono = [_mono(x, kind, m) for x in recs]
        mkind = mono[0][1]
        slots = _open(ref, len(recs))
        try:
            p, e, g = ref.scan(slots, [a for a, _ in mono], hop=hop, **_args(mkind, gate))
            saved = [ref.save_stream(int(s)) for s in slots]
        finally:
            _close(ref, slots)
        _REFS[key] = [(p[i].copy(), e[i].copy(), g[i].copy(), saved[i]) for i in range(len(recs))]
    return _REFS[key]


def _items(mode, n):
    """the (recording, mode) pairs of a case, in the order of its streams"""
    if mode == "split":
        return [(i, c) for i in range(n) for c in (0, 1)]
    if mode == "cycle":
        return [(i, CYCLE[i % 3]) for i in range(n)]
    return [(i, {"left": 0, "right": 1, "mix": "mix"}[mode]) for i in range(n)]


def _scan(eng, recs, kind, hop, gate, mode, order=None):
    """Engine.scan on fresh slots -> per item of _items(mode) (probs, events, seg, saved state)"""
    n = len(recs)
    order = np.arange(n) if order is None else np.asarray(order)
    items = _items(mode, n)
    slots = np.asarray(_open(eng, len(items)))
    try:
        if mode == "split":
            sl = slots.reshape(n, 2)
            p, e, g = eng.scan(sl[order], [recs[i] for i in order], hop=hop, channel="split", **_args(kind, gate))
            back = np.argsort(order)
            out = []
            for i in range(n):
                k = int(back[i])
                assert p[k].shape == e[k].shape == g[k].shape and p[k].shape[0] == 2
                for c in range(2):
                    out.append((p[k][c], e[k][c], g[k][c], eng.save_stream(int(sl[i, c]))))
            return out
        channel = [m for _, m in items]
        p, e, g = eng.scan(slots[order], [recs[i] for i in order], hop=hop, channel=[channel[i] for i in order], **_args(kind, gate))
        back = np.argsort(order)
        return [(p[int(back[i])], e[int(back[i])], g[int(back[i])], eng.save_stream(int(slots[i]))) for i in range(n)]
    finally:
        _close(eng, slots)


def _compare(got, items, refs, what):
    assert len(got) == len(items)
    for (i, m), (p, e, g, saved) in zip(items, got):
        rp, re_, rg, rsaved = refs[m][i]
        _same_bytes(p, rp, ("probs", what, i, m))
        _same_bytes(e, re_, ("events", what, i, m))
        _same_bytes(g, rg, ("seg_frames", what, i, m))
        assert saved == rsaved, ("state", what, i, m)


def _assert_batch_tells_the_channels_apart(refs, what):
    """a batch that fails one of these is a broken test: events in every mode, and the three modes give different bytes"""
    for m in (0, 1, "mix"):
        ev = np.concatenate([r[1] for r in refs[m]])
        assert ((ev & _ffi.VAD_EV_START) != 0).sum() >= 1 and ((ev & _ffi.VAD_EV_END) != 0).sum() >= 1, (what, m, "no START / END")
        seg = np.concatenate([r[2] for r in refs[m]])
        assert ((seg > 0) == ((ev & _ffi.VAD_EV_END) != 0)).all()
    differ = lambda a, b: sum(refs[a][i][0].tobytes() != refs[b][i][0].tobytes() for i in range(len(refs[0])))
    assert differ(0, 1) >= 10, (what, differ(0, 1))
    assert differ("mix", 0) >= 10 and differ("mix", 1) >= 10, (what, differ("mix", 0), differ("mix", 1))


def _all_refs(ref, tag, recs, kind, hop, gate):
    refs = {m: _reference(ref, tag, recs, kind, hop, gate, m) for m in (0, 1, "mix")}
    _assert_batch_tells_the_channels_apart(refs, (tag, kind, hop, gate))
    return refs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@RATES
def test_every_mode_equals_the_mono_scan_of_the_prepared_array(engines, rate, kind, mode):
    eng, ref = engines(rate)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs = _stereo(kind, frame, hop, rate, SEED)
    assert len(recs) == 37 and max(r.shape[0] for r in recs) >= frame + 39 * hop
    refs = _all_refs(ref, ("half", rate), recs, kind, hop, 0.01)
    _compare(_scan(eng, recs, kind, hop, 0.01, mode), _items(mode, len(recs)), refs, (rate, kind, mode))


@pytest.mark.parametrize("mode", ["split", "cycle"])
@pytest.mark.parametrize("kind", ["f32", "i16_32767", "ulaw"])
@pytest.mark.parametrize("variant", ["nogate", "odd_hop"])
@RATES
def test_gate_off_and_an_odd_hop(engines, rate, variant, kind, mode):
    """hop = frame / 4 + 4: hop / 4 is odd, so consecutive frames start on sample-frame quads of alternating parity"""
    eng, ref = engines(rate)
    frame = eng.frame_samples
    hop = frame // 2 if variant == "nogate" else frame // 4 + 4
    gate = None if variant == "nogate" else 0.01
    assert variant == "nogate" or (hop // 4) % 2 == 1
    recs = _stereo(kind, frame, hop, rate, SEED + 1)
    refs = _all_refs(ref, (variant, rate), recs, kind, hop, gate)
    _compare(_scan(eng, recs, kind, hop, gate, mode), _items(mode, len(recs)), refs, (rate, variant, kind, mode))


@pytest.mark.parametrize("kind", ["f32", "i16_32768", "alaw"])
@RATES
def test_launch_cap_item_order_and_device_audio_do_not_change_a_byte(engines, rate, kind):
    import torch
    eng, ref = engines(rate)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs = _stereo(kind, frame, hop, rate, SEED)
    recs[-1] = recs[-1][:frame + (recs[-1].shape[0] - frame) // hop * hop] if recs[-1].shape[0] >= frame else recs[-1]
    tag = ("caps", rate)
    refs = _all_refs(ref, tag, recs, kind, hop, 0.01)
    n = len(recs)
    perm = np.random.default_rng(5).permutation(n)
    try:
        for cap, order, mode in ((1, None, "cycle"), (7, perm, "cycle"), (0, perm, "split"), (7, None, "split"), (0, perm, "cycle")):
            eng.set_scan_launch_frames(cap)
            _compare(_scan(eng, recs, kind, hop, 0.01, mode, order=order), _items(mode, n), refs, (rate, kind, cap, mode))
    finally:
        eng.set_scan_launch_frames(0)
    # vad_scan_channels_device on a block that already lies in HBM and ends with the last recording's last sample frame; every
    # recording is listed three times - left, right, mix - over the same samples, in a permuted order
    lens = np.array([r.shape[0] for r in recs])
    offs = np.concatenate([[0], np.cumsum((lens[:-1] + 3) & ~3)])
    block = np.zeros((int(offs[-1] + lens[-1]), 2), recs[0].dtype)
    for r, o in zip(recs, offs):
        block[o:o + r.shape[0]] = r
    items = [(i, m) for i in range(n) for m in CYCLE]
    items = [items[k] for k in np.random.default_rng(6).permutation(len(items))]
    slots = _open(eng, len(items))
    try:
        d_audio = torch.from_numpy(block).cuda()
        assert d_audio.data_ptr() % 8 == 0
        total = sum(refs[m][i][0].size for i, m in items)
        d_p = torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda")
        d_e = torch.full((total + 8,), 0x55, dtype=torch.uint8, device="cuda")
        d_s = torch.full((total + 8,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        fmt = FMT[kind]
        start = eng.scan_device(slots, [offs[i] for i, _ in items], [lens[i] for i, _ in items], d_audio.data_ptr(), block.shape[0],
                                d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), hop=hop, fmt=fmt, denoise=0.01, channels=2,
                                channel=[m for _, m in items])
        eng.synchronize()
        p, e, s = d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()
        assert int(start[-1]) == total
        got = [(p[start[k]:start[k + 1]], e[start[k]:start[k + 1]], s[start[k]:start[k + 1]], eng.save_stream(int(slots[k])))
               for k in range(len(items))]
        _compare(got, items, refs, ("device", rate, kind))
        assert (p[total:] == -7.0).all() and (e[total:] == 0x55).all() and (s[total:] == -9).all()
    finally:
        _close(eng, slots)


def _rejected(ev):
    return list(np.flatnonzero((ev & _ffi.VAD_EV_REJECTED) != 0))


@pytest.mark.parametrize("gate", [0.01, None], ids=["gate", "nogate"])
@RATES
def test_non_finite_samples_reject_what_the_stream_hears(engines, rate, gate):
    """The non-finite check runs over the samples the model would see.  A NaN and a -Inf in the RIGHT channel only, each in the
    overlap of two frames: nothing rejected for left, exactly those two frames for right and for mix.  Two finite values whose sum
    overflows: rejected for mix, for neither channel.  +Inf left with -Inf right: rejected for mix (Inf - Inf = NaN) - and, each
    sample being non-finite itself, for the channel that holds it, as the mono scan of that channel rejects it.  In every mode
    the state is untouched and the following frames are the mono scan's: all bytes and the saved state are compared."""
    eng, ref = engines(rate)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    counts = [12, 9, 5, 12, 0, 7] + [6] * 14
    recs = _stereo("f32", frame, hop, rate, seed=13, counts=counts)
    # sample 5 hop + 17 lies in the overlap of frames 4 and 5; sample 3 hop - 1 in that of frames 1 and 2
    recs[0][5 * hop + 17, 1] = np.nan
    recs[3][3 * hop - 1, 1] = -np.inf
    big = np.float32(np.finfo(np.float32).max) * np.float32(0.75)
    recs[1][4 * hop + 2] = (big, big)                   # frames 3 and 4
    recs[5][2 * hop + 5] = (np.inf, -np.inf)            # frames 1 and 2
    assert np.isinf(_mono(recs[1], "f32", "mix")[0][4 * hop + 2]) and np.isnan(_mono(recs[5], "f32", "mix")[0][2 * hop + 5])
    tag = ("nonfinite", rate)
    refs = {m: _reference(ref, tag, recs, "f32", hop, gate, m) for m in (0, 1, "mix")}
    want = {0: {0: [], 3: [], 1: [], 5: [1, 2]}, 1: {0: [4, 5], 3: [1, 2], 1: [], 5: [1, 2]},
            "mix": {0: [4, 5], 3: [1, 2], 1: [3, 4], 5: [1, 2]}}
    for mode in ("split", "cycle", "mix"):
        items = _items(mode, len(recs))
        got = _scan(eng, recs, "f32", hop, gate, mode)
        _compare(got, items, refs, (rate, mode))
        for (i, m), (p, e, g, _) in zip(items, got):
            rej = _rejected(e)
            assert rej == want[m].get(i, []), (mode, i, m, rej)
            mask = (e & _ffi.VAD_EV_REJECTED) != 0
            assert (e[mask] == _ffi.VAD_EV_REJECTED).all() and np.isnan(p[mask]).all() and not g[mask].any()
            if i in (0, 3, 5):
                assert np.isfinite(p[~mask]).all(), (mode, i, m)
    # every (recording, mode) of `want` was reached by one of the three cases
    seen = {(i, m) for mode in ("split", "cycle", "mix") for i, m in _items(mode, len(recs))}
    assert all((i, m) in seen for m in want for i in want[m])


@pytest.mark.parametrize("gate", [0.01, None], ids=["gate", "nogate"])
@RATES
def test_the_mix_rounds_as_numpy_mean(engines, rate, gate):
    """(dL + dR) * 0.5f against np.mean(x, axis=1) where the two could part: a sum that rounds (1, 2^-24), exact cancellation,
    subnormal pairs whose halved sum rounds again, and a sum that reaches FLT_MAX without overflowing"""
    eng, ref = engines(rate)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    x = _stereo("f32", frame, hop, rate, seed=19, counts=[9, 6, 6, 9])[0]
    rng = np.random.default_rng(23)
    tiny = np.float32(np.finfo(np.float32).tiny)
    sub = np.float32(1.401298464324817e-45)             # the smallest subnormal
    fmax = np.float32(np.finfo(np.float32).max)
    pairs = [(np.float32(1.0), np.float32(2.0 ** -24)), (np.float32(1.0), np.float32(-(2.0 ** -24))), (np.float32(0.37), np.float32(-0.37)),
             (sub, np.float32(0.0)), (sub, sub), (np.float32(3) * sub, sub), (sub, -sub), (tiny, sub), (tiny * np.float32(0.5), np.float32(3) * sub),
             (-tiny, np.float32(5) * sub), (np.float32(0.011), np.float32(0.0091)), (np.float32(0.01), np.float32(0.01))]
    where = rng.choice(np.arange(hop, 5 * hop), len(pairs), replace=False)
    for k, pr in zip(where, pairs):
        x[k] = pr
    x[7 * hop + 3] = (fmax * np.float32(0.5), fmax * np.float32(0.5))      # frames 6 and 7: the sum is FLT_MAX, finite
    mean = np.mean(x, axis=1)
    assert mean.dtype == np.float32 and np.isfinite(mean).all() and mean[7 * hop + 3] == fmax * np.float32(0.5)
    recs = [x]
    refs = {m: _reference(ref, ("rounding", rate), recs, "f32", hop, gate, m) for m in (0, 1, "mix")}
    for mode in ("mix", "split"):
        got = _scan(eng, recs, "f32", hop, gate, mode)
        _compare(got, _items(mode, 1), refs, (rate, mode))
        assert all(_rejected(e) == [] for _, e, _, _ in got)
    assert refs["mix"][0][0].size == 9


@pytest.mark.parametrize("kind", ["f32", "ulaw"])
@RATES
def test_a_two_channel_block_up_to_the_last_byte_below_2_gib(engines, rate, kind):
    """a device block of 2^31 - 32 bytes, the most the argument check accepts to within a quad of float32 sample frames: the
    sample-frame quad shifted to a byte offset (<< 5 for float32, << 3 for G.711) reaches bit 30 and stays a positive 32-bit
    integer; one recording lies across byte 2^30, one ends on the block's last sample frame.  The memory is allocated and
    zeroed on the device, only the recordings are copied in."""
    import torch
    eng, ref = engines(rate)
    frame = eng.frame_samples
    hop = frame // 4 + 4
    counts = [12, 7, 3, 9, 5]
    recs = _stereo(kind, frame, hop, rate, seed=38, counts=counts)
    recs[4] = np.ascontiguousarray(recs[4][:frame + (counts[4] - 1) * hop])         # no tail: its last sample frame is the block's
    size = 2 * recs[0].dtype.itemsize                                                # bytes per sample frame
    nbytes = (1 << 31) - 32
    nsamp = nbytes // size
    at = lambda byte: (byte // size) & ~3
    offs = [0, at(1 << 30) - (recs[1].shape[0] // 2 & ~3), 0, at(3 << 29) - 260, nsamp - recs[4].shape[0]]
    offs[2] = ((offs[1] + recs[1].shape[0] + 3) & ~3) + 4
    assert 0 < at(1 << 30) - offs[1] < frame + (counts[1] - 1) * hop                 # one of its frames straddles byte 2^30
    assert 1 << 30 < offs[2] * size < (1 << 30) + (1 << 16)
    assert all(o % 4 == 0 for o in offs) and offs[4] + recs[4].shape[0] == nsamp and nsamp * size == nbytes
    refs = {m: _reference(ref, ("high", rate), recs, kind, hop, 0.01, m) for m in (0, 1, "mix")}
    assert [r[0].size for r in refs[0]] == counts
    items = [(i, m) for i in range(5) for m in CYCLE]
    d_audio = torch.zeros(nsamp * 2, dtype={4: torch.float32, 1: torch.uint8}[recs[0].dtype.itemsize], device="cuda")
    slots = _open(eng, len(items))
    try:
        assert d_audio.data_ptr() % 8 == 0
        for r, o in zip(recs, offs):
            d_audio[2 * o:2 * (o + r.shape[0])] = torch.from_numpy(r.reshape(-1)).cuda()
        total = sum(refs[m][i][0].size for i, m in items)
        d_p = torch.full((total,), -7.0, dtype=torch.float32, device="cuda")
        d_e = torch.full((total,), 0x55, dtype=torch.uint8, device="cuda")
        d_s = torch.full((total,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        start = eng.scan_device(slots, [offs[i] for i, _ in items], [recs[i].shape[0] for i, _ in items], d_audio.data_ptr(), nsamp,
                                d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), hop=hop, fmt=FMT[kind], denoise=0.01, channels=2,
                                channel=[m for _, m in items])
        eng.synchronize()
        p, e, s = d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()
        got = [(p[start[k]:start[k + 1]], e[start[k]:start[k + 1]], s[start[k]:start[k + 1]], eng.save_stream(int(slots[k])))
               for k in range(len(items))]
        _compare(got, items, refs, ("high addresses", rate, kind))
        # the five recordings hold different audio: a byte offset that wrapped would have read another one, or zeros
        assert len({refs[0][i][0].tobytes() for i in range(5)}) == 5 and all(np.any(refs[1][i][0] != refs[0][i][0]) for i in range(5))
    finally:
        _close(eng, slots)
        del d_audio
        torch.cuda.empty_cache()


def _wav_samples(w):
    import io
    import wave
    with wave.open(io.BytesIO(w)) as f:
        return f.getnframes()


@pytest.mark.parametrize("cfg_kw", [{}, dict(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6,
                                             voice_end_frame_count=12)], ids=["default", "client"])
def test_scan_recordings_mixes_as_the_wrapper_does_and_splits_into_the_channels(cfg_kw):
    """the speech golden on the left against itself 3 s later on the right (two speakers who talk over each other), as [N, 2]
    float32: the default (mix) gives, in count and length, the segments VADWrapper.process_audio_data delivers through voice_end
    for the same 2-D array (tests/test_gpu_scan.py's comparison); 'split' gives per channel what scan_recordings gives for that
    channel alone.  (With the f32 oracle and oracle.StateMachine on the CPU the whole clip has 3 segments on the left, on the
    right and in the mix under the default configuration, 5 / 4 / 9 under the client's.)"""
    from cutter_vad_amd import VADConfig, VADWrapper, scan_recordings
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float32) / np.float32(32767.0)
    cfg = VADConfig(**cfg_kw)
    frame, hop = 512, 256
    delayed = np.concatenate([np.zeros(3 * 16000, np.float32), pcm[:-3 * 16000]])
    whole = np.ascontiguousarray(np.stack([pcm, delayed], axis=1))
    recs = [whole, np.ascontiguousarray(whole[:pcm.size // 2]), np.ascontiguousarray(whole[pcm.size // 3:]), pcm]
    got = scan_recordings(recs, cfg)
    assert len(got) == len(recs)
    for x, segs in zip(recs, got):
        wavs = []
        with VADWrapper(config=cfg) as vad:
            vad.set_callbacks(None, wavs.append, None)
            vad.process_audio_data(x)
        assert len(segs) == len(wavs), (len(segs), len(wavs))
        for (a, b), w in zip(segs, wavs):
            L = (b - a - frame) // hop + 1
            assert (L - 1) * hop + frame == b - a and 0 <= a and b <= x.shape[0]
            assert _wav_samples(w) == L * frame, (a, b, L, _wav_samples(w))
    assert len(got[0]) >= 1, "no segment in the mix: the comparison with the wrapper would be between empty lists"
    split = scan_recordings(recs, cfg, channel="split")
    assert [len(s) for s in split] == [2, 2, 2, 1]
    for x, per_channel in zip(recs, split):
        for c, segs in enumerate(per_channel):
            alone = scan_recordings([np.ascontiguousarray(x[:, c]) if x.ndim == 2 else x], cfg)[0]
            assert segs == alone, (c, segs, alone)
    assert len(split[0][0]) >= 1 and len(split[0][1]) >= 1 and split[0][0] != split[0][1]
    assert scan_recordings(recs, cfg, channel=1)[:3] == [s[1] for s in split[:3]]
    print(f"scan_recordings on two channels: mix {[len(g) for g in got]}, split {[[len(s) for s in r] for r in split]} segments")
