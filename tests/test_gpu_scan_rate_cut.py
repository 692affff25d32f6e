"""Segment tables and segment audio behind a rate scan on the GPU (vad_scan_rate_segments, vad_scan_rate_cut;
csrc/scan_cut_resample.hip: vadk_cut_resample in front of the unchanged vadk_scan_cut).  Every bar is BYTE equality.  The twin of a
VAD_CUT_FRAMES payload: cut_ref.heard (the wire format decoded and channel-selected to float32), AudioUtils.split_into_frames(x, chunk,
hop), Engine.resample(chunks, sr) on a second engine (tests/test_gpu_resample.py holds that to scipy), cut_ref.gate on the resampled
value, then cut_ref.pcm16 or the float32 itself.  VAD_CUT_RANGE is cut_ref.reference with frame = chunk and no gate.  The cut tests
use hand-built segment tables over random blocks - no model is involved; the table tests use the corpus of
tests/test_gpu_scan_rate.py's scan_recordings test."""
import ctypes as C

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from cutter_vad_amd.utils.audio import AudioUtils
from tests import cut_ref as R
from tests import seg_ref
from tests.cut_ref import F32, FMT, FRAMES, MIX, PCM16, RANGE, SENT16, untouched
from tests.rate_cut_ref import rate_cut, rate_segments
from tests.test_gpu_scan import THR, _close, _engine, _open
from tests.test_gpu_scan_rate import _heard, _recordings

pytestmark = pytest.mark.gpu

CHUNK = {8000: 256, 24000: 768, 48000: 1536}
COUNTS = [70, 64, 40, 33, 5, 70]                                            # chunks of the six recordings of a block
# (recording, first_frame, nframes): every length of {1, 2, 31, 32, 33, 64, 70}, first frames 0 and odd, two segments over the same
# chunks (recording 3, 1 .. 31), the listing in no order of position or length
SEGS = [(5, 0, 70), (0, 3, 1), (3, 1, 31), (1, 0, 64), (0, 0, 2), (2, 7, 33), (3, 1, 31), (4, 3, 2), (2, 0, 32), (0, 37, 33), (4, 0, 1)]


@pytest.fixture(scope="module")
def engines():
    """(the engine that cuts, a second engine for the twin's Engine.resample)"""
    eng, twin = _engine(16000), _engine(16000)
    yield eng, twin
    eng.close()
    twin.close()


def _block(kind, sr, hop, two, seed):
    """six recordings of COUNTS chunks (+ a tail that framing drops), packed on multiples of 4 -> (block, offsets)"""
    rng = np.random.default_rng(seed)
    chunk = CHUNK[sr]
    lens = [chunk + (c - 1) * hop + int(t) for c, t in zip(COUNTS, rng.integers(0, min(hop, 97), len(COUNTS)))]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
    block = R.values(rng, kind, (int(offs[-1]), 2) if two else (int(offs[-1]),))
    return block, offs[:-1], lens


def _frames(twin, x, sr, hop):
    """the float32 stream of one recording -> the frames the model reads of it [chunks, 512]"""
    chunks = np.ascontiguousarray(AudioUtils.split_into_frames(x, CHUNK[sr], hop), np.float32)
    return twin.resample(chunks, sr)


def _payload(frames, first, nf, gate, out_fmt):
    seg = R.gate(np.ascontiguousarray(frames[first:first + nf]).reshape(-1), gate)
    return seg.astype(np.float32) if out_fmt == F32 else R.pcm16(seg)


def _cases():
    out = []
    for sr in (8000, 24000, 48000):
        for k, kind in enumerate(("f32", "i16_32767", "ulaw")):
            # mono and two-channel, gate and none, PCM16 and F32: every pair of values at every rate, every value for every format
            for two, gate, of in ((False, 0.01, PCM16), (True, None, F32)) if (k + sr // 8000) % 2 else ((False, None, F32), (True, 0.01, PCM16)):
                out.append(pytest.param(sr, kind, two, gate, of, 2, id=f"{sr}-{kind}-{'stereo' if two else 'mono'}-{'gate' if gate else 'nogate'}"))
    out.append(pytest.param(24000, "i16_32768", True, 0.01, PCM16, 2, id="24000-i16_32768-stereo-gate"))
    out.append(pytest.param(8000, "alaw", False, 0.01, PCM16, 2, id="8000-alaw-mono-gate"))
    out.append(pytest.param(48000, "i16_32767", False, 0.01, PCM16, 1, id="48000-i16_32767-mono-gate-hop_chunk"))
    return out


def _items(SEGS, offs, hop, chunk, layout, two):
    """the cut items of SEGS with explicit output positions: gaps of 0, 4 and 8 samples in front of the segments
    -> (items, output samples with a tail of 12)"""
    items, pos = [], 0
    for k, (rec, first, nf) in enumerate(SEGS):
        count = nf * 512 if layout == FRAMES else (nf - 1) * hop + chunk
        pos += 4 * (k % 3)
        items.append((int(offs[rec]), first, nf, pos, (0, 1, MIX)[k % 3] if two else 0))
        pos += (count + 3) & ~3
    return items, pos + 12


@pytest.mark.parametrize("sr,kind,two,gate,out_fmt,hop_div", _cases())
def test_frames_equal_the_twin_and_range_the_block(engines, sr, kind, two, gate, out_fmt, hop_div):
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // hop_div
    block, offs, lens = _block(kind, sr, hop, two, seed=sr // 1000 + len(kind) + hop_div)
    thr = -1.0 if gate is None else gate
    # FRAMES: the twin's frames of every (recording, channel) a segment names
    items, total = _items(SEGS, offs, hop, chunk, FRAMES, two)
    rc, msg, out = rate_cut(eng._lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, FRAMES, out_fmt, total, thr=thr)
    assert rc == _ffi.VAD_OK, msg
    frames = {}
    written = np.zeros(out.size, bool)
    for (rec, first, nf), it in zip(SEGS, items):
        key = (rec, it[4])
        if key not in frames:
            frames[key] = _frames(twin, R.heard(block[offs[rec]:offs[rec] + lens[rec]], kind, it[4]), sr, hop)
            assert frames[key].shape == (COUNTS[rec], 512)
        want = _payload(frames[key], first, nf, gate, out_fmt)
        assert want.size == nf * 512 == eng.cut_samples(nf, hop, "frames", sample_rate=sr)
        got = out[it[3]:it[3] + want.size]
        assert got.tobytes() == want.tobytes(), ("frames", rec, first, nf, int((got != want).sum()))
        written[it[3]:it[3] + want.size] = True
    assert untouched(out[~written]) and (~written).sum() >= 12 + 8        # the gaps and the tail keep the sentinel
    if gate is not None:
        assert any((_payload(f, 0, len(f), None, F32) != _payload(f, 0, len(f), gate, F32)).any() for f in frames.values()), "the gate gated nothing"
    # RANGE: the segment's own samples at the input rate, NOT gated whatever threshold is passed
    items, total = _items(SEGS, offs, hop, chunk, RANGE, two)
    rc, msg, out = rate_cut(eng._lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, RANGE, out_fmt, total, thr=0.01)
    assert rc == _ffi.VAD_OK, msg
    written = np.zeros(out.size, bool)
    for it in items:
        want = R.reference(block, kind, it, chunk, hop, RANGE, out_fmt, None)
        assert want.size == eng.cut_samples(it[2], hop, "range", sample_rate=sr)
        assert out[it[3]:it[3] + want.size].tobytes() == want.tobytes(), ("range", it)
        written[it[3]:it[3] + want.size] = True
    assert untouched(out[~written])


def test_both_instantiations_of_the_resample_kernel(engines):
    """one segment of 8 192 frames = 256 tiles of 32 rows, the last launch in which two workgroups share a tile, and one of 8 200 =
    257 tiles, the first of the other instantiation (the switch of vadk_scan_resample)"""
    eng, twin = engines
    sr, chunk, hop = 8000, 256, 128
    rng = np.random.default_rng(41)
    x = R.values(rng, "f32", (chunk + 8199 * hop,))
    frames = _frames(twin, x, sr, hop)
    for nf in (8192, 8200):
        rc, msg, out = rate_cut(eng._lib, eng, [(0, 0, nf, 0, 0)], x, 1, FMT["f32"], sr, hop, FRAMES, F32, nf * 512, thr=0.01)
        assert rc == _ffi.VAD_OK, msg
        assert out[:nf * 512].tobytes() == _payload(frames, 0, nf, 0.01, F32).tobytes(), nf
        assert untouched(out[nf * 512:])


def test_more_rows_than_one_window_holds(engines):
    """70 segments of 1 900 frames over the same recording: 133 000 rows, the engine's window holds 131 072 - two windows, and
    segment 68 (rows 129 200 .. 131 099) straddles them.  The twin is one resample of 1 900 chunks, 70 times."""
    eng, twin = engines
    sr, chunk, hop = 8000, 256, 128
    nseg, nf = 70, 1900
    assert nseg * nf > (256 << 20) // 2048 > 68 * nf and 69 * nf > (256 << 20) // 2048
    rng = np.random.default_rng(43)
    x = R.values(rng, "ulaw", (chunk + (nf - 1) * hop,))
    want = _payload(_frames(twin, R.heard(x, "ulaw", 0), sr, hop), 0, nf, 0.01, PCM16)
    total = nseg * nf * 512
    out = np.full(total + 8, SENT16, np.int16)
    rc, msg, out = rate_cut(eng._lib, eng, [(0, 0, nf, i * nf * 512, 0) for i in range(nseg)], x, 1, FMT["ulaw"], sr, hop, FRAMES, PCM16, total,
                            thr=0.01, out=out)
    assert rc == _ffi.VAD_OK, msg
    rows = out[:total].reshape(nseg, nf * 512)
    bad = [i for i in range(nseg) if rows[i].tobytes() != want.tobytes()]
    assert not bad, bad
    assert untouched(out[total:]) and want.any()


def test_device_form_equals_the_host_form(engines):
    import torch
    eng, _ = engines
    sr, kind, chunk = 24000, "i16_32767", 768
    hop = chunk // 2
    block, offs, lens = _block(kind, sr, hop, True, seed=47)
    for layout in (FRAMES, RANGE):
        items, total = _items(SEGS, offs, hop, chunk, layout, True)
        rc, msg, host = rate_cut(eng._lib, eng, items, block, 2, FMT[kind], sr, hop, layout, PCM16, total, thr=0.01)
        assert rc == _ffi.VAD_OK, msg
        d_audio = torch.from_numpy(block).cuda()
        d_out = torch.full((host.size,), int(SENT16), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        segs = [(it[0], it[1], it[2], {0: 0, 1: 1, MIX: "mix"}[it[4]]) for it in items]
        start = eng.cut_device(segs, d_audio.data_ptr(), block.shape[0], d_out.data_ptr(), total, hop=hop, fmt=FMT[kind], channels=2,
                               denoise=0.01, layout="frames" if layout == FRAMES else "range", out_start=[it[3] for it in items],
                               sample_rate=sr)
        eng.synchronize()
        got = d_out.cpu().numpy()
        assert got.tobytes() == host.tobytes() and untouched(got[total:]) and not untouched(got[:total])
        assert int(start[-1]) == sum(eng.cut_samples(it[2], hop, "frames" if layout == FRAMES else "range", sample_rate=sr) for it in items)


def _corpus(sr, hop):
    return _recordings("f32", sr, hop, seed=17, counts=[20, 0, 33, 7, 1, 40, 12, 3, 26])


@pytest.mark.parametrize("sr", [24000, 48000])
def test_the_table_is_the_per_frame_scans_and_the_block_stays_for_the_cut(engines, sr):
    eng, twin = engines
    lib = eng._lib
    chunk = CHUNK[sr]
    hop = chunk // 2
    recs = _corpus(sr, hop)
    n = len(recs)
    slots = _open(eng, n)
    try:
        probs, ev, seg = eng.scan(slots, recs, hop=hop, denoise=0.01, sample_rate=sr)
        states = [eng.save_stream(int(s)) for s in slots]
        assert eng.last_scan is None
        start = np.concatenate([[0], np.cumsum([p.size for p in probs])])
        want = seg_ref.table(np.concatenate(ev), np.concatenate(seg), np.concatenate(probs), start)
        assert want.size >= 2, "fewer than two segments: the comparison would show nothing"
        eng.reset(slots)
        eng.set_thresholds_many(slots, THR)
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01, sample_rate=sr)
        assert seg_ref.same(table, want)
        assert [eng.save_stream(int(s)) for s in slots] == states
        last = eng.last_scan
        assert last is not None and last["rate"] == sr
        offs = last["offsets"]
        # cut(audio=None) behind it equals the cut with the audio passed, and the twin
        segs = [(int(offs[r["item"]]), int(r["first_frame"]), int(r["nframes"])) for r in table]
        block = np.zeros(int(last["samples"]), np.float32)
        for r, o in zip(recs, offs):
            block[o:o + r.size] = r
        for layout in ("frames", "range"):
            got, gs = eng.cut(segs, hop=hop, denoise=0.01, layout=layout)
            for r, a, b in zip(table, gs[:-1], gs[1:]):
                x = _heard(recs[r["item"]], "f32")
                if layout == "frames":
                    w = _payload(_frames(twin, x, sr, hop), int(r["first_frame"]), int(r["nframes"]), 0.01, PCM16)
                else:
                    w = R.pcm16(x[r["first_frame"] * hop:(r["first_frame"] + r["nframes"] - 1) * hop + chunk])
                assert got[a:b].tobytes() == w.tobytes(), (layout, r)
            passed, ps = eng.cut(segs, hop=hop, denoise=0.01, layout=layout, audio=block, sample_rate=sr)
            assert passed.tobytes() == got.tobytes() and np.array_equal(ps, gs) and got.any()
            eng._scan_last = last                       # (the block passed is the scan's own: what the engine holds did not change)
        # seg_cap = 1: the true count, one record, and the rest from the table that stayed on the GPU
        eng.reset(slots)
        eng.set_thresholds_many(slots, THR)
        rc, msg, one, count = rate_segments(lib, eng, [(int(s), int(o), r.size) for s, o, r in zip(slots, offs, recs)], block, 1, FMT["f32"], sr,
                                            hop, cap=1, thr=0.01)
        assert rc == _ffi.VAD_OK and count == want.size and one.tobytes() == want[:1].tobytes(), msg
        rest = np.zeros(want.size - 1, _ffi.SEGMENT_DTYPE)
        assert lib.vad_scan_segments_read(eng.handle, 1, rest.size, rest.ctypes.data_as(C.POINTER(_ffi.Segment))) == _ffi.VAD_OK
        assert rest.tobytes() == want[1:].tobytes()
        assert [eng.save_stream(int(s)) for s in slots] == states
    finally:
        _close(eng, slots)


@pytest.mark.parametrize("sr", [24000, 48000])
def test_cut_recordings_delivers_the_twins_frames_and_the_recordings_own_ranges(engines, sr):
    from cutter_vad_amd import VADConfig, cut_recordings, scan_recordings
    from cutter_vad_amd.scan import _frame_stats
    from cutter_vad_amd.utils.wav_writer import WAVWriter
    eng, twin = engines
    chunk = CHUNK[sr]
    hop = chunk // 2
    recs = _corpus(sr, hop)
    cfg = VADConfig(vad_start_probability=THR[0], vad_end_probability=THR[1], voice_start_ratio=THR[2], voice_end_ratio=THR[3],
                    voice_start_frame_count=THR[4], voice_end_frame_count=THR[5], enable_denoising=True)
    ranges = scan_recordings(recs, cfg, engine=eng, sample_rate=sr)
    assert sum(len(r) for r in ranges) >= 2
    frames = cut_recordings(recs, cfg, engine=eng, sample_rate=sr)
    own = cut_recordings(recs, cfg, engine=eng, sample_rate=sr, layout="range")
    h16, hsr = WAVWriter(cfg.output_wav_sample_rate, 16, 1), WAVWriter(sr, 16, 1)
    for i, rec in enumerate(recs):
        assert [sg[:2] for sg in frames[i]] == [sg[:2] for sg in own[i]] == ranges[i]
        if not ranges[i]:
            continue
        x = _heard(rec, "f32")
        fr = _frames(twin, x, sr, hop)
        for (a, b, wav), (_, _, rng) in zip(frames[i], own[i]):
            raw = _payload(fr, a // hop, (b - a - chunk) // hop + 1, 0.01, PCM16).tobytes()
            assert wav == h16.header(len(raw)) + raw, (i, a, b)
            raw = R.pcm16(x[a:b]).tobytes()
            assert rng == hsr.header(len(raw)) + raw, (i, a, b)
    # stats=True: the table's statistics are the per-frame results', exactly
    stats = scan_recordings(recs, cfg, engine=eng, sample_rate=sr, stats=True)
    slots = _open(eng, len(recs))
    try:
        probs, ev, seg = eng.scan(slots, recs, hop=hop, denoise=0.01, sample_rate=sr)
    finally:
        _close(eng, slots)
    want = [[(a, b) + _frame_stats(p, e, (b - chunk) // hop, (b - a - chunk) // hop + 1) for a, b in one] for one, p, e in zip(ranges, probs, ev)]
    assert stats == want
