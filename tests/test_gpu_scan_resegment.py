"""Segment tables at other thresholds on the GPU (csrc/scan_resegment.hip: count, prefix, fill; vadk_seg_stats behind them;
vad_scan_resegment, vad_resegment_device).  The bar is BYTE equality: the table of every threshold set is what scan_segments returns
for the same recordings on a twin engine's freshly opened streams with that set - records, order, statistics - for int16 and
float32 corpora, a rejected frame inside speech, a 48 kHz rate scan whose resident block still cuts, the device form on a Silero V4
engine against the oracle's state machine, and sweep_recordings against scan_recordings."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import reseg_cases, reseg_ref, seg_ref
from tests.test_gpu_scan import GOLD, THR, _engine, _recordings

pytestmark = pytest.mark.gpu

DEFAULTS = (0.7, 0.7, 0.8, 0.95, 10, 50)
LONG_END = (0.5, 0.35, 0.6, 0.9, 4, 57)          # ends only behind 57 quiet frames: the 400-frame recording's silence
# THR first, the VADConfig defaults, and three that vary the probabilities, a ratio below 1 and the counts
SETS = [THR, (0.35, 0.25, 0.7, 0.9, 3, 4), LONG_END, (0.85, 0.6, 0.5, 0.75, 3, 8), DEFAULTS]
SCAN_THR = (0.45, 0.3, 0.75, 0.85, 5, 9)         # what the scan itself runs with: none of the sets
SENT = 0x5A


def sets64():
    """the five sets repeated with small changes in every field"""
    out = []
    for k in range(64):
        a, b, c, d, m, n = SETS[k % 5]
        j = k // 5
        out.append((a - 0.004 * j, b - 0.003 * j, c - 0.01 * j, d - 0.01 * j, m + j % 3, n + j % 4))
    return out


@pytest.fixture(scope="module")
def engines():
    eng, twin = _engine(16000, max_streams=128), _engine(16000, max_streams=128)
    yield eng, twin
    eng.close()
    twin.close()


def _long(kind, frame, hop):
    """400 frames: the clip's speech, then silence from frame 150 on"""
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float64) / 32768.0
    ns = frame + 399 * hop + 5
    x = np.resize(pcm, ns)
    x[150 * hop:] = 0.0
    return x.astype(np.float32) if kind == "f32" else np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)


def _corpus(kind, frame, hop):
    return _recordings("f32" if kind == "f32" else "i16_32767", frame, hop, 16000, seed=3) + [_long(kind, frame, hop)]


def _fresh(twin, sets, recs, hop, **kw):
    """scan_segments on freshly opened streams with each set"""
    out = []
    for s in sets:
        slots = twin.open_streams(len(recs))
        try:
            twin.set_thresholds_many(slots, s)
            out.append(twin.scan_segments(slots, recs, hop=hop, **kw))
        finally:
            for k in slots:
                twin.close_stream(int(k))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert seg_ref.same(np.ascontiguousarray(g), w), (k, len(g), len(w), g[:3], w[:3])


_cache = {}


def _reference(twin, kind, frame, hop):
    if kind not in _cache:
        recs = _corpus(kind, frame, hop)
        want = _fresh(twin, SETS, recs, hop, denoise=0.01)
        print(f"resegment [{kind}]: records per set {[len(w) for w in want]}")
        # not vacuous, by the fresh scans alone
        full = [w for w in want if len(w)]
        assert len(full) >= 2 and len({w.tobytes() for w in full}) == len(full)
        assert len(want[0]) >= 1 and (want[2]["item"] == len(recs) - 1).any()      # THR's END; the 57-frame END of the long recording
        _cache[kind] = (recs, want)
    return _cache[kind]


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_every_set_s_table_equals_the_scan_of_fresh_streams(engines, kind):
    eng, twin = engines
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs, want = _reference(twin, kind, frame, hop)
    assert len(recs) == 38 and eng.scan_frame_count(recs[-1].size, hop) == 400 > 2 * 192      # three launch windows
    slots = eng.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, SCAN_THR)
        with eng.scan_session():
            own = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
            saved = [eng.save_stream(int(s)) for s in slots]
            info = eng.info()
            _same(eng.resegment(SETS), want)
            _same(eng.resegment(SETS[:1]), want[:1])
            for k in (2, 4):
                _same(eng.resegment([SETS[k]]), [want[k]])
            # streams, counters and the scan's own table are where they were
            assert [eng.save_stream(int(s)) for s in slots] == saved
            assert (eng.info()["steps"], eng.info()["frames"]) == (info["steps"], info["frames"])
            again = np.zeros(len(own), _ffi.SEGMENT_DTYPE)
            if len(own):
                import ctypes as C
                assert eng._lib.vad_scan_segments_read(eng.handle, 0, len(own), again.ctypes.data_as(C.POINTER(_ffi.Segment))) == 0
            assert again.tobytes() == np.ascontiguousarray(own).tobytes()
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_sixty_four_sets_fill_a_wave_per_recording(engines):
    eng, twin = engines
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs, _ = _reference(twin, "f32", frame, hop)
    sets = sets64()
    want = _fresh(twin, sets, recs, hop, denoise=0.01)
    assert len({w.tobytes() for w in want if len(w)}) >= 10
    slots = eng.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, SCAN_THR)
        with eng.scan_session():
            eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
            _same(eng.resegment(sets), want)
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_a_rejected_frame_inside_speech_is_skipped(engines):
    eng, twin = engines
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    clean = _long("f32", frame, hop)
    # where speech is: the middle of the longest segment any set finds in the clean recording
    longest = max((r for w in _fresh(twin, SETS, [clean], hop, denoise=0.01) for r in w), key=lambda r: int(r["nframes"]))
    assert longest["nframes"] >= 9
    mid = int(longest["first_frame"]) + int(longest["nframes"]) // 2
    holed = clean.copy()
    holed[mid * hop + 100] = np.nan                 # frames mid - 1 and mid hold the sample: both rejected, inside speech
    recs = [clean, holed, clean[:40 * hop], holed[:(mid + 20) * hop]]
    want = _fresh(twin, SETS, recs, hop, denoise=0.01)
    both = [w for w in want if {0, 1} <= set(w["item"].tolist())]
    assert both, [len(w) for w in want]
    slots = eng.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, SCAN_THR)
        with eng.scan_session():
            eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
            _same(eng.resegment(SETS), want)
    finally:
        for s in slots:
            eng.close_stream(int(s))
    # the statistics leave the rejected frames out: some segment of the holed recording counts fewer frames than it spans
    assert any(((w["item"] == 1) & (w["counted"] < w["nframes"])).any() for w in want)


def test_a_48_khz_scan_replays_and_its_block_still_cuts(engines):
    from tests.test_gpu_scan_rate import _recordings as rate_recordings
    eng, twin = engines
    sr, chunk = 48000, 1536
    hop = chunk // 2
    recs = rate_recordings("f32", sr, hop, seed=17, counts=[20, 0, 33, 7, 40, 26])
    want = _fresh(twin, SETS, recs, hop, denoise=0.01, sample_rate=sr)
    assert len(want[0]) >= 1 and len(want[1]) >= 1 and want[0].tobytes() != want[1].tobytes(), [len(w) for w in want]
    slots, tslots = eng.open_streams(len(recs)), twin.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, SCAN_THR)
        twin.set_thresholds_many(tslots, SETS[1])
        with eng.scan_session(), twin.scan_session():
            eng.scan_segments(slots, recs, hop=hop, denoise=0.01, sample_rate=sr)
            got = eng.resegment(SETS)
            _same(got, want)
            # the resident block is still the rate block: the cut of set 1's table is the cut behind the twin's own scan with set 1
            assert eng.last_scan["rate"] == sr
            fresh = twin.scan_segments(tslots, recs, hop=hop, denoise=0.01, sample_rate=sr)
            assert seg_ref.same(fresh, want[1])
            segs = lambda e, t: [(int(e.last_scan["offsets"][r["item"]]), int(r["first_frame"]), int(r["nframes"])) for r in t]
            a, sa = eng.cut(segs(eng, got[1]), hop=hop, denoise=0.01, layout="frames")
            b, sb = twin.cut(segs(twin, fresh), hop=hop, denoise=0.01, layout="frames")
            assert a.size == 512 * int(got[1]["nframes"].sum()) and a.tobytes() == b.tobytes() and np.array_equal(sa, sb) and a.any()
    finally:
        for e, k in ((eng, slots), (twin, tslots)):
            for s in k:
                e.close_stream(int(s))


def test_the_device_form_on_a_v4_engine(engines):
    import torch
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(4, 16000), "rb") as f:
        v4 = Engine(f.read(), model_version=4, max_streams=64, sample_rate=16000)
    try:
        n, T, frame = 6, 48, v4.frame_samples
        pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float32) / np.float32(32768.0)
        frames = np.stack([np.resize(pcm[i * 7000:], T * frame).reshape(T, frame) for i in range(n)])
        frames[:, 30:] = 0.0                                    # speech, then silence
        slots = v4.open_streams(n)
        d_frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        d_slots = torch.from_numpy(np.asarray(slots, np.int32)).cuda()
        d_probs = torch.zeros(n * T, dtype=torch.float32, device="cuda")
        d_events = torch.zeros(n * T, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        v4.step_multi_device(n, T, d_frames.data_ptr(), d_probs.data_ptr(), d_slots.data_ptr(), d_events.data_ptr(), denoise=0.01)
        v4.synchronize()
        probs, events = d_probs.cpu().numpy(), d_events.cpu().numpy()
        sets = [THR, (0.2, 0.15, 0.6, 0.8, 1, 3), DEFAULTS, (0.5, 0.4, 0.7, 0.9, 3, 6)]
        for start in (np.arange(n + 1) * T, np.array([T + 5, 2 * T, 2 * T, 5 * T - 3])):      # the second: out_start[0] > 0, an empty item
            want = reseg_ref.tables(events, probs, start, sets)
            whole = np.concatenate(want)
            counts = np.concatenate([[0], np.cumsum([len(w) for w in want])])
            print(f"resegment_device [v4]: records per set {[len(w) for w in want]}")
            assert len(whole) >= 2
            for cap in (len(whole) + 2, len(whole) - 1, 0):
                tab = torch.full(((cap + 2) * 24,), SENT, dtype=torch.uint8, device="cuda")
                cnt = torch.full((len(sets) + 2,), -7, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                v4.resegment_device(d_events.data_ptr(), d_probs.data_ptr(), start, sets, tab.data_ptr(), cap, cnt.data_ptr())
                v4.synchronize()
                assert cnt.cpu().numpy().tolist() == counts.tolist() + [-7]
                raw, k = tab.cpu().numpy(), min(cap, len(whole))
                assert raw[:k * 24].tobytes() == whole[:k].tobytes() and (raw[k * 24:] == SENT).all(), cap
        for s in slots:
            v4.close_stream(int(s))
    finally:
        v4.close()


@pytest.mark.parametrize("n,nsets", [(n, 5) for n in reseg_cases.NS] + [(257, 1), (257, 64)])
def test_tables_past_a_wave_and_a_workgroup(engines, n, nsets):
    """vadk_reseg_prefix's sums across waves (n > 64), its second and third round (n > 256, n > 512) and the total carried from one
    set into the next between rounds, and reseg_replay's ENDs in the frames behind its last group of four - hand-built arrays
    (tests/reseg_cases.py, every condition asserted there on the reference), no model run: the records, set_start as a whole, the
    bytes around both outputs and the inputs, at caps above and below the total, 0, and inside the second set"""
    import torch
    eng, _ = engines
    ev, probs, start, sets, want, (counts, caps) = reseg_cases.built(n, nsets)
    whole = np.concatenate(want)
    print(f"resegment_device [n = {n}, {nsets} sets]: {len(probs)} frames, set_start {counts.tolist()[:9]}, caps {caps}")
    d_ev, d_p = torch.from_numpy(ev).cuda(), torch.from_numpy(probs).cuda()
    for cap in caps:
        tab = torch.full(((cap + 4) * 24,), SENT, dtype=torch.uint8, device="cuda")
        cnt = torch.full((len(sets) + 3,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.resegment_device(d_ev.data_ptr(), d_p.data_ptr(), start, sets, tab.data_ptr() + 48, cap, cnt.data_ptr() + 8)
        eng.synchronize()
        torch.cuda.synchronize()
        assert cnt.cpu().numpy().tolist() == [-7] + counts.tolist() + [-7], cap
        raw, k = tab.cpu().numpy(), min(cap, len(whole))
        assert (raw[:48] == SENT).all() and (raw[48 + k * 24:] == SENT).all(), cap
        got = raw[48:48 + k * 24].view(seg_ref.DTYPE)
        assert got.tobytes() == whole[:k].tobytes(), (cap, got[:3], whole[:3])
    assert d_ev.cpu().numpy().tobytes() == ev.tobytes() and d_p.cpu().numpy().tobytes() == probs.tobytes()


def test_sweep_recordings_is_scan_recordings_per_config():
    from cutter_vad_amd import VADConfig, scan_recordings, sweep_recordings
    frame = 512
    recs = _recordings("f32", frame, frame // 2, 16000, seed=3)[2:8]
    cfg = lambda s: VADConfig(vad_start_probability=s[0], vad_end_probability=s[1], voice_start_ratio=s[2], voice_end_ratio=s[3],
                              voice_start_frame_count=s[4], voice_end_frame_count=s[5])
    cfgs = [cfg(THR), cfg(SETS[1])]
    got = sweep_recordings(recs, cfgs, stats=True)
    want = [scan_recordings(recs, c, stats=True) for c in cfgs]
    assert got == want and sum(len(r) for r in want[0]) >= 1
