"""vad_scan_cut on the GPU (csrc/scan_cut.hip: vadk_scan_cut).  The bar is equality: a segment's payload is BYTE FOR BYTE the numpy
reference of tests/test_scan_cut_host.py - the wire format decoded as the model's loader decodes it (utils/g711.py's tables,
s / 32767, s / 32768), np.mean of a two-channel pair, the strict gate np.where(|x| > thr, x, 0), then the float32 itself or
np.clip(x * 32767, -32768, 32767).astype(np.int16) - at every value a sample can take, both frame sizes, hops that align with
nothing, segments on the block's last sample, on shared frames and around the workgroup's share, with sentinels between and
behind the payloads, at addresses up to 2 GiB, and end to end against what VADWrapper's voice_end callback delivers."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests.test_gpu_scan import GOLD, _engine
from tests.cut_ref import F32, FMT, FRAMES, MIX, PCM16, RANGE, SENT16, SENT32, decode, gate, pcm16, raw_cut, reference, untouched, values

pytestmark = pytest.mark.gpu

KINDS = tuple(FMT)
W = _ffi.VAD_CUT_WG_SAMPLES
HOPS = {"hop4": lambda f: 4, "quarter4": lambda f: f // 4 + 4, "half": lambda f: f // 2, "frame": lambda f: f, "frame4": lambda f: f + 4}
RATES = pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
THR = float(np.float32(0.01))


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(rate):
        if rate not in made:
            made[rate] = _engine(rate)
        return made[rate]

    yield get
    for e in made.values():
        e.close()


def _count(frame, hop, nf, layout):
    return nf * frame if layout == FRAMES else (nf - 1) * hop + frame


def _cut(eng, items, audio, channels, kind, hop, layout, out_fmt, n_out, thr):
    rc, msg, out = raw_cut(eng._lib, eng, items, audio, channels, FMT[kind], hop, layout, out_fmt, n_out, thr=-1.0 if thr is None else thr)
    assert rc == _ffi.VAD_OK, msg
    return out


def _check(eng, items, audio, channels, kind, hop, layout, out_fmt, n_out, thr):
    """the call's output against the reference, segment by segment; everything outside the segments keeps its sentinel"""
    frame = eng.frame_samples
    out = _cut(eng, items, audio, channels, kind, hop, layout, out_fmt, n_out, thr)
    covered = np.zeros(out.size, bool)
    for it in items:
        want = reference(audio, kind, it, frame, hop, layout, out_fmt, thr)
        assert out[it[3]:it[3] + want.size].tobytes() == want.tobytes(), (it, kind, hop, layout, out_fmt, thr)
        covered[it[3]:it[3] + want.size] = True
    assert untouched(out[~covered]) and (~covered).sum() >= 8
    return out


# ---- every value ------------------------------------------------------------------------------------------------------
def _f32_probes():
    one = np.float32(1.0)
    thr = np.float32(THR)
    v = [1.0, 1.5, one - np.float32(2.0 ** -24), np.float32(32767.5) / np.float32(32767.0), 2.0 ** -16, 1e-40, 1.4e-45, 1.1754942e-38,
         0.0, thr, np.nextafter(thr, one), np.nextafter(thr, np.float32(0.0)), 0.5, 0.999969482421875, 1.0000305, 2.0, 40000.0 / 32767.0]
    rng = np.random.default_rng(11)
    ks = np.concatenate([[0, 1, 2, 327, 328, 16383, 32765, 32766, 32767], rng.integers(0, 32768, 400)]).astype(np.float64)
    v += list((ks + 0.5) / 32767.0) + list((ks + 0.999) / 32767.0) + list((ks + 0.001) / 32767.0) + list(ks / 32767.0)
    v = np.asarray(v, np.float32)
    v = np.concatenate([v, -v])
    # products that land exactly on k + 0.5 in float32, found by search around each k (x * 32767 is one rounded multiply)
    exact = []
    for k in (0, 1, 100, 1000, 12345, 32766):
        c = np.float32((k + 0.5) / 32767.0)
        near = c
        for _ in range(64):
            if np.float32(near * np.float32(32767.0)) == np.float32(k + 0.5):
                exact.append(near)
                break
            near = np.nextafter(near, np.float32(2.0))
    assert len(exact) >= 3
    v = np.concatenate([v, np.asarray(exact, np.float32), -np.asarray(exact, np.float32)])
    assert np.isfinite(v).all() and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()      # +0 and -0
    return v


def _value_blocks(frame):
    """kind -> a mono recording that holds every value of the format (float32: the probes), a whole number of frames"""
    allv = np.arange(-32768, 32768).astype(np.int16)
    codes = np.resize(np.arange(256).astype(np.uint8), 2 * frame)
    pr = _f32_probes()
    pr = np.concatenate([pr, np.zeros(-pr.size % frame, np.float32)])
    return {"f32": pr, "i16_32767": allv, "i16_32768": allv, "ulaw": codes, "alaw": codes}


@pytest.mark.parametrize("thr", [None, THR], ids=["nogate", "gate"])
@pytest.mark.parametrize("kind", KINDS)
@RATES
def test_every_value_of_every_format(engines, rate, kind, thr):
    eng = engines(rate)
    frame = eng.frame_samples
    x = _value_blocks(frame)[kind]
    nf = x.size // frame
    assert nf * frame == x.size
    d = decode(x, kind)
    if kind.startswith("i16"):
        assert np.unique(x).size == 65536
    elif kind != "f32":
        assert np.unique(x).size == 256
    else:
        assert (np.abs(d) == np.float32(THR)).sum() == 2 and (np.abs(d * 32767) > 32768).any()
    for out_fmt in (PCM16, F32):
        for layout in (FRAMES, RANGE):
            out = _check(eng, [(0, 0, nf, 0, 0)], x, 1, kind, frame, layout, out_fmt, x.size + 4, thr)
            want = gate(d, thr)
            assert out[:x.size].tobytes() == (pcm16(want) if out_fmt == PCM16 else want).tobytes()
    # the same values as the right channel and in the mix with their own reverse
    st = np.ascontiguousarray(np.stack([x[::-1], x], axis=1))
    for out_fmt in (PCM16, F32):
        _check(eng, [(0, 0, nf, 0, 1), (0, 0, nf, x.size + 4, MIX), (0, 0, nf, 2 * x.size + 8, 0)], st, 2, kind, frame, FRAMES, out_fmt,
               3 * x.size + 12, thr)


# ---- frame sizes, hops, lengths, positions, sentinels -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop_name", list(HOPS))
@RATES
def test_hops_lengths_positions_and_sentinels(engines, rate, hop_name, kind):
    eng = engines(rate)
    frame = eng.frame_samples
    hop = HOPS[hop_name](frame)
    rng = np.random.default_rng(len(kind) + 7 * hop)
    rec0 = frame + 11 * hop + 8                              # a recording with a tail, then one that ends the block
    off1 = (rec0 + 3) & ~3
    ns = off1 + frame + 8 * hop
    x = values(rng, kind, ns)
    for layout in (FRAMES, RANGE):
        items, o = [], 0
        # L = 1, 2, 9; two segments that share frames 3 .. 4 of recording 0; the last one ends on the block's last sample
        for off, first, nf in ((0, 0, 1), (0, 1, 2), (0, 3, 9), (0, 2, 3), (off1, 8, 1), (off1, 0, 9)):
            items.append((off, first, nf, o, 0))
            o += _count(frame, hop, nf, layout) + 4          # 4 sentinel samples between two payloads
        assert off1 + 8 * hop + frame == ns
        n_out = o + 8                                        # and a tail behind the last
        for out_fmt in (PCM16, F32):
            for thr in (None, 0.3):
                _check(eng, items, x, 1, kind, hop, layout, out_fmt, n_out, thr)
                _check(eng, items[::-1], x, 1, kind, hop, layout, out_fmt, n_out, thr)


# ---- the workgroup's share --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "i16_32767", "alaw"])
@RATES
def test_segments_around_the_workgroups_share(engines, rate, kind):
    eng = engines(rate)
    frame = eng.frame_samples
    assert W == 4096
    rng = np.random.default_rng(21)
    x = values(rng, kind, 3 * W + 64)
    hop = 4
    items, o = [], 0
    for k, total in enumerate((W - 4, W, W + 4, 3 * W)):
        nf = (total - frame) // hop + 1
        assert _count(frame, hop, nf, RANGE) == total
        items.append((4 * k, k, nf, o, 0))
        o += total + 4
    for out_fmt in (PCM16, F32):
        _check(eng, items, x, 1, kind, hop, RANGE, out_fmt, o + 8, 0.3)
    # FRAMES: 9 frames = 4 608 (16 kHz) / 2 304 (8 kHz) samples, 24 frames: whole shares and a partial last one
    for nf in (8, 9, 16, 24):
        _check(eng, [(0, 1, nf, 4, 0)], x, 1, kind, frame // 2, FRAMES, PCM16, nf * frame + 12, None)


@RATES
def test_300_one_frame_segments_in_one_call(engines, rate):
    eng = engines(rate)
    frame = eng.frame_samples
    hop = frame // 4 + 4
    rng = np.random.default_rng(22)
    x = values(rng, "i16_32768", (frame + 320 * hop, 2))
    order = rng.permutation(300)
    items = [(0, int(f), 1, int(k) * (frame + 4), (0, 1, MIX)[int(f) % 3]) for k, f in enumerate(order)]
    for out_fmt in (PCM16, F32):
        _check(eng, items, x, 2, "i16_32768", hop, FRAMES, out_fmt, 300 * (frame + 4) + 8, THR)


# ---- two channels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@RATES
def test_an_interleaved_block_cut_three_times(engines, rate, kind):
    """left, right and mix of the same samples by three items, as the scan's split mode lists a recording"""
    eng = engines(rate)
    frame = eng.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(23 + len(kind))
    ns = 1028 + frame + 9 * hop + 3
    x = values(rng, kind, (ns, 2))
    for layout in (FRAMES, RANGE):
        n1 = _count(frame, hop, 7, layout)
        items = [(1028, 2, 7, k * (n1 + 4), ch) for k, ch in enumerate((0, 1, MIX))]
        for out_fmt in (PCM16, F32):
            for thr in (None, 0.3):
                out = _check(eng, items, x, 2, kind, hop, layout, out_fmt, 3 * (n1 + 4) + 8, thr)
                if thr is None and out_fmt == F32 and layout == RANGE:
                    d = decode(x, kind)[1028 + 2 * hop:1028 + 2 * hop + n1]
                    assert np.array_equal(out[:n1], d[:, 0]) and np.array_equal(out[n1 + 4:2 * n1 + 4], d[:, 1])
                    assert np.array_equal(out[2 * (n1 + 4):2 * (n1 + 4) + n1], np.mean(d, axis=1))


# ---- entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,channels", [("f32", 1), ("i16_32767", 2), ("ulaw", 2), ("alaw", 1)])
def test_the_device_entry_on_a_callers_stream_gives_the_host_entrys_bytes(engines, kind, channels):
    import torch
    eng = engines(16000)
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    rng = np.random.default_rng(24)
    x = values(rng, kind, (9000, 2) if channels == 2 else 9000)
    items = [(0, 3, 9, 0, 0), (1028, 0, 2, 9 * frame + 4, MIX if channels == 2 else 0), (1028, 1, 1, 11 * frame + 8, channels - 1)]
    n_out = 12 * frame + 16
    for out_fmt in (PCM16, F32):
        want = _check(eng, items, x, channels, kind, hop, FRAMES, out_fmt, n_out, THR)
        d_audio = torch.from_numpy(x).cuda()
        d_out = torch.from_numpy(np.full(n_out + 8, SENT32 if out_fmt == F32 else SENT16, want.dtype)).cuda()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        start = eng.cut_device([(it[0], it[1], it[2], "mix" if it[4] == MIX else it[4]) for it in items], d_audio.data_ptr(), 9000,
                               d_out.data_ptr(), n_out, hop=hop, fmt=FMT[kind], channels=channels, denoise=THR,
                               out="f32" if out_fmt == F32 else "pcm16", stream=stream.cuda_stream, out_start=[it[3] for it in items])
        stream.synchronize()
        assert list(start) == [0, 9 * frame, 11 * frame, 12 * frame]
        assert d_out.cpu().numpy().tobytes() == want.tobytes()
        # the next call on the engine waits for the launch on the caller's stream by itself
        again = _cut(eng, items, x, channels, kind, hop, FRAMES, out_fmt, n_out, THR)
        assert again.tobytes() == want.tobytes()


@pytest.mark.parametrize("kind", ["i16_32767", "ulaw"])
def test_the_resident_block_after_engine_scan(engines, kind):
    eng = engines(16000)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(25)
    recs = [values(rng, kind, (frame + 9 * hop + 5, 2)), values(rng, kind, (frame + 2 * hop, 2)), values(rng, kind, (100, 2))]
    slots = eng.open_streams(3)
    law = kind if kind in ("ulaw", "alaw") else None
    try:
        with eng.scan_session():
            eng.scan(slots, recs, hop=hop, law=law, denoise=THR)
            last = eng.last_scan
            offs = [int(o) for o in last["offsets"]]
            segs = [(offs[0], 1, 9, 0), (offs[1], 0, 3), (offs[0], 0, 2, 1), (offs[1], 2, 1, "mix")]
            data, start = eng.cut(segs, hop=hop, denoise=THR)
            f32, _ = eng.cut(segs, hop=hop, denoise=THR, out="f32", layout="range")
        block = np.zeros((last["samples"], 2), recs[0].dtype)
        for r, o in zip(recs, offs):
            block[o:o + r.shape[0]] = r
        data2, start2 = eng.cut(segs, hop=hop, denoise=THR, audio=block, law=law)
        assert data.tobytes() == data2.tobytes() and list(start) == list(start2) == [0, 9 * frame, 12 * frame, 14 * frame, 15 * frame]
        for k, sg in enumerate(segs):
            it = (sg[0], sg[1], sg[2], 0, MIX if len(sg) == 3 or sg[3] == "mix" else sg[3])
            assert np.array_equal(data[start[k]:start[k + 1]], reference(block, kind, it, frame, hop, FRAMES, PCM16, THR)), k
        assert np.array_equal(f32[:8 * hop + frame], reference(block, kind, (offs[0], 1, 9, 0, 0), frame, hop, RANGE, F32, THR))
        assert np.abs(data).max() > 1000
    finally:
        for s in slots:
            eng.close_stream(int(s))


# ---- high addresses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,channels", [("f32", 1), ("ulaw", 2)])
@RATES
def test_segments_up_to_the_last_sample_of_a_block_below_2_gib(engines, rate, kind, channels):
    """a block of 2^31 - 32 bytes in device memory: segments across byte 2^30, across 3 * 2^29 and ending on the last sample frame"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the block and torch's copies need 6 GiB")
    eng = engines(rate)
    frame = eng.frame_samples
    hop = frame // 4 + 4
    fb = channels * (4 if kind == "f32" else 1)                       # bytes per sample frame
    nsamp = ((1 << 31) - 32) // fb
    assert nsamp * fb == (1 << 31) - 32 and nsamp % 4 == 0
    rng = np.random.default_rng(26)
    nf = 9
    span = frame + (nf - 1) * hop
    at = lambda byte: (byte // fb) & ~3
    starts = [at(1 << 30) - (span // 2 & ~3), at(3 << 29) - (span // 2 & ~3), nsamp - span]
    assert all(s % 4 == 0 and s * fb < b < (s + span) * fb for s, b in zip(starts[:2], (1 << 30, 3 << 29)))
    shape = (span, 2) if channels == 2 else span
    parts = [values(rng, kind, shape) for _ in starts]
    d_audio = torch.zeros((nsamp, 2) if channels == 2 else nsamp, dtype=torch.float32 if kind == "f32" else torch.uint8, device="cuda")
    try:
        for p, s in zip(parts, starts):
            d_audio[s:s + span] = torch.from_numpy(p).cuda()
        for layout in (FRAMES, RANGE):
            n1 = _count(frame, hop, nf, layout)
            chans = (0, 0, 0) if channels == 1 else (0, 1, MIX)
            # the recording's offset and the segment's first frame share the distance: sample_offset + first_frame * hop = start
            segs = [(s - 2 * hop * k, 2 * k, nf, "mix" if c == MIX else c) for k, (s, c) in enumerate(zip(starts, chans))]
            for out_fmt in (PCM16, F32):
                n_out = 3 * (n1 + 4) + 8
                d_out = torch.from_numpy(np.full(n_out, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)).cuda()
                torch.cuda.synchronize()
                eng.cut_device(segs, d_audio.data_ptr(), nsamp, d_out.data_ptr(), n_out, hop=hop, fmt=FMT[kind], channels=channels,
                               denoise=THR, layout="frames" if layout == FRAMES else "range", out="f32" if out_fmt == F32 else "pcm16",
                               out_start=[k * (n1 + 4) for k in range(3)])
                eng.synchronize()
                out = d_out.cpu().numpy()
                for k, (p, c) in enumerate(zip(parts, chans)):
                    want = reference(p, kind, (0, 0, nf, 0, c), frame, hop, layout, out_fmt, THR)
                    assert out[k * (n1 + 4):k * (n1 + 4) + n1].tobytes() == want.tobytes(), (k, layout, out_fmt)
                    assert untouched(out[k * (n1 + 4) + n1:(k + 1) * (n1 + 4)])
                assert untouched(out[3 * (n1 + 4):])
    finally:
        del d_audio
        torch.cuda.empty_cache()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _wrapper_wavs(cfg, x, frame):
    from cutter_vad_amd import VADWrapper
    wavs = []
    with VADWrapper(config=cfg) as vad:
        vad.set_callbacks(None, wavs.append, None)
        if x.shape[0] >= frame:
            vad.process_audio_data(x)
    return wavs


@pytest.mark.parametrize("cfg_kw", [{}, dict(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6,
                                             voice_end_frame_count=12)], ids=["default", "client"])
def test_cut_recordings_delivers_the_wrappers_payloads(cfg_kw):
    """the speech golden, whole and in parts, mono and as [N, 2] against itself 3 s later: every WAV payload of cut_recordings is
    byte for byte what VADWrapper.process_audio_data's voice_end callback delivered for the same array; layout="range" payloads
    are the int16 conversion of the gated x[a:b]"""
    from cutter_vad_amd import VADConfig, cut_recordings
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float32) / np.float32(32767.0)
    cfg = VADConfig(**cfg_kw)
    frame = 512
    delayed = np.concatenate([np.zeros(3 * 16000, np.float32), pcm[:-3 * 16000]])
    whole = np.ascontiguousarray(np.stack([pcm, delayed], axis=1))
    mono = [pcm, pcm[:pcm.size // 2], pcm[pcm.size // 3:], pcm[:300]]
    recs = mono + [whole]
    got = cut_recordings(recs, cfg)
    ranges = cut_recordings(recs, cfg, layout="range", wav=False)
    assert len(got) == len(ranges) == len(recs)
    counts = []
    for x, segs, rg in zip(recs, got, ranges):
        wavs = _wrapper_wavs(cfg, x, frame)
        assert len(segs) == len(wavs) == len(rg), (len(segs), len(wavs))
        for (a, b, payload), w, (a2, b2, pcm16_range) in zip(segs, wavs, rg):
            assert isinstance(payload, bytes) and payload == w, (a, b, len(payload), len(w))
            assert (a, b) == (a2, b2)
            h = gate(x if x.ndim == 1 else np.mean(x, axis=1), 0.01 if cfg.enable_denoising else None)
            assert np.array_equal(pcm16_range, pcm16(h[a:b]))
        counts.append(len(segs))
    print(f"cut_recordings [{'client' if cfg_kw else 'default'}]: segments per recording {counts}")
    assert sum(counts[:4]) >= (4 if cfg_kw else 1), counts
    assert counts[4] >= 1, "no segment in the mix: the comparison with the wrapper would be between empty lists"
