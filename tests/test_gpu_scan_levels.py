"""vad_scan_levels and vad_scan_cut_gain on the GPU (csrc/scan_levels.hip: vadk_seg_levels; csrc/scan_cut.hip: vadk_scan_cut_gain).
The bar is BYTE equality.  Levels: the records are tests/levels_ref.py applied to Engine.cut(layout="range", out="f32") of the same
table - the cut is read through its existing, unchanged path.  Gains: the payload is the existing cut's float32 times the factor in
numpy float32, then the existing conversion.  The geometry tests aim at the lanes behind a segment's last quad, which load like
the others and must contribute nothing: every segment there is fenced by the block's largest samples."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.scan import SegmentRefine, level_stats
from tests.cut_ref import FMT, MIX, decode, gate, heard, pcm16, values
from tests.levels_ref import levels_ref, of_cut, records
from tests.test_gpu_scan import GOLD, _engine

pytestmark = pytest.mark.gpu

KINDS = tuple(FMT)
THR = float(np.float32(0.01))


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(key):
        if key not in made:
            if key == "v4":
                from cutter_vad_amd.engine import Engine
                with open(weights_io.packaged_blob_path(4, 16000), "rb") as f:
                    made[key] = Engine(f.read(), model_version=4, max_streams=64, sample_rate=16000)
            else:
                made[key] = _engine(key)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _kw(kind, denoise=THR):
    return dict(law=kind if kind in ("ulaw", "alaw") else None, i16_scale=32768 if kind == "i16_32768" else 32767, denoise=denoise)


def _same(eng, segs, clip=0.95, **kw):
    """Engine.levels against the reference on the existing cut; both read the same block with the same arguments"""
    want = of_cut(eng, segs, clip, **kw)
    got = eng.levels(segs, clip=clip, **kw)
    assert got.dtype == _ffi.LEVEL_DTYPE and got.tobytes() == want.tobytes(), (got, want)
    return got


# ---- formats and channels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [None, 0.3], ids=["nogate", "gate"])
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", KINDS)
def test_formats_and_channels(engines, kind, channels, denoise):
    eng = engines(16000)
    frame, hop = eng.frame_samples, eng.frame_samples // 4 + 4
    rng = np.random.default_rng(len(kind) + 10 * channels)
    ns = 9000
    x = values(rng, kind, (ns, 2) if channels == 2 else ns)
    chans = (0, 1, "mix") if channels == 2 else (0,)
    segs = []
    for k in range(9):
        off = (0, 1028, 2000)[k % 3]
        room = (ns - off - frame) // hop + 1
        nf = int(rng.integers(1, room + 1))
        segs.append((off, int(rng.integers(0, room - nf + 1)), nf, chans[k % len(chans)]))
    got = _same(eng, segs, hop=hop, audio=x, **_kw(kind, denoise))
    # and against numpy alone, no cut in between
    for sg, rec in zip(segs, got):
        h = gate(heard(x, kind, MIX if sg[3] == "mix" else sg[3]), denoise)
        a = sg[0] + sg[1] * hop
        assert rec.tobytes() == records([h[a:a + (sg[2] - 1) * hop + frame]]).tobytes(), sg
    if kind == "f32":
        assert (got["peak"] > 1).any() and (got["energy_q32"] > 0).all()      # saturated samples entered
    if kind in ("i16_32768", "ulaw", "alaw") and channels == 1:
        # x = s / 32768: no term is rounded, the sum is 4 * sum(s^2) (the gate zeroes whole samples)
        for sg, rec in zip(segs, got):
            a = sg[0] + sg[1] * hop
            s = np.rint(gate(decode(x, kind), denoise)[a:a + (sg[2] - 1) * hop + frame].astype(np.float64) * 32768).astype(np.int64)
            assert int(rec["energy_q32"]) == 4 * int((s * s).sum())


# ---- geometry: waves, passes, workgroups; the lanes behind the last quad --------------------------------------------------
QUADS = [128, 255, 256, 257, 1023, 1024, 1025, 2049, 3 * 1024 + 17]


def _fenced(eng, quads, kind="f32"):
    """a mono block with one segment of `quads` quads at hop 4, quiet inside (|x| <= 0.5), the block's largest samples in the quad
    before its first sample and in the quad behind its last -> (block, segment, first sample, end)"""
    frame = eng.frame_samples
    nf = quads - frame // 4 + 1
    assert nf >= 1
    a, n = 2048, 4 * quads
    rng = np.random.default_rng(quads)
    x = rng.uniform(-0.5, 0.5, a + n + 8192).astype(np.float32)
    x[a - 4:a] = np.float32(0.99)
    x[a + n:a + n + 4] = np.float32(-0.99)
    if kind != "f32":
        x = np.rint(x * 32767).astype(np.int16)
    return x, (0, a // 4, nf), a, a + n


@pytest.mark.parametrize("kind", ["f32", "i16_32767"])
@pytest.mark.parametrize("quads", QUADS)
def test_segment_sizes_fenced_by_the_blocks_largest_samples(engines, quads, kind):
    eng = engines(16000)
    x, seg, a, b = _fenced(eng, quads, kind)
    assert eng.cut_samples(seg[2], 4, "range") == 4 * quads
    got = _same(eng, [seg], hop=4, audio=x, **_kw(kind, None))[0]
    assert got["peak"] <= 0.5 + 1e-4 and got["clipped"] == 0 and got["energy_q32"] > 0
    # the peak at the segment's very first and very last sample
    for pos in (a, b - 1):
        y = x.copy()
        y[pos] = np.float32(-0.75) if kind == "f32" else np.int16(-24575)
        got = _same(eng, [seg], hop=4, audio=y, clip=0.75 if kind == "f32" else 0.7, **_kw(kind, None))[0]
        assert got["peak"] == np.abs(decode(y[pos:pos + 1], kind))[0] and got["clipped"] == 1


def test_one_wave_of_pass_0_and_three_idle_waves(engines):
    """64 quads: a one-frame segment of the 8 kHz engine's 256-sample frames"""
    eng = engines(8000)
    assert eng.frame_samples == 256
    x, seg, a, b = _fenced(eng, 64)
    segs = [seg, (0, (a + 1024) // 4, 1), (0, (a + 4096) // 4, 1)]
    x[a + 1024 - 4:a + 1024] = np.float32(0.99)
    x[a + 1024 + 256:a + 1024 + 260] = np.float32(0.99)
    got = _same(eng, segs, hop=4, audio=x, denoise=None)
    assert (got["peak"][:2] <= 0.5).all() and (got["clipped"] == 0).all()
    zero = np.zeros_like(x)
    zero[a - 4:a] = 1
    zero[b:b + 4] = 1
    got = _same(eng, [seg], hop=4, audio=zero, denoise=None, clip=0.0)[0]
    assert (int(got["energy_q32"]), float(got["peak"]), int(got["clipped"])) == (0, 0.0, 256)


def test_clip_thresh_0_on_an_all_zero_segment_counts_exactly_its_samples(engines):
    eng = engines(16000)
    for quads in (128, 257, 1025, 3 * 1024 + 17):
        x, seg, a, b = _fenced(eng, quads)
        x[a:b] = 0
        got = _same(eng, [seg], hop=4, audio=x, denoise=None, clip=0.0)[0]
        assert (int(got["energy_q32"]), float(got["peak"]), int(got["clipped"])) == (0, 0.0, 4 * quads)
        got = _same(eng, [seg], hop=4, audio=x, denoise=THR, clip=0.0)[0]
        assert int(got["clipped"]) == 4 * quads


def test_300_one_frame_segments_and_items_that_share_samples(engines):
    eng = engines(16000)
    frame = eng.frame_samples
    rng = np.random.default_rng(300)
    x = values(rng, "i16_32767", 300 * 520 + frame)
    segs = [(0, 130 * k, 1) for k in range(300)]          # hop 4: frame k starts at sample 520 k
    got = _same(eng, segs, hop=4, audio=x, **_kw("i16_32767"))
    assert np.unique(got["energy_q32"]).size == 300
    twice = [(0, 7, 900), (0, 7, 900), (4, 6, 900), (0, 7, 900)]     # the same samples under three names, and once more
    got = _same(eng, twice, hop=4, audio=x, **_kw("i16_32767"))
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes() == got[3].tobytes()


# ---- values -----------------------------------------------------------------------------------------------------------
def test_probe_values_float32(engines):
    eng = engines(16000)
    frame = eng.frame_samples
    c = np.float32(0.95)
    t = np.float32(THR)
    probes = np.array([1.0, -1.0, 1.5, -3.0, c, -c, np.nextafter(c, np.float32(0)), t, -t, np.nextafter(t, np.float32(1)), 0.5, -0.0,
                       2.0 ** -16, 2.0 ** -17, 3.0 * 2.0 ** -17, 1e-30], np.float32)
    x = np.zeros(frame, np.float32)
    x[:probes.size] = probes
    for denoise in (None, THR):
        got = _same(eng, [(0, 0, 1)], hop=4, audio=x, denoise=denoise)[0]
        kept = probes if denoise is None else probes[np.abs(probes) > t]        # the gate is strict: |x| == thr is zeroed
        # the rule in Python's own arithmetic: float(v) ** 2 and the scaling are exact, round() rounds half to even
        q = sum(min(round(float(v) ** 2 * 2 ** 32), 2 ** 32) for v in kept)
        assert int(got["energy_q32"]) == q
        assert float(got["peak"]) == 3.0 and int(got["clipped"]) == 6           # +-1, 1.5, -3, +-0.95: |x| == clip_thresh counts
    on, off = eng.levels([(0, 0, 1)], hop=4, audio=x, denoise=THR), eng.levels([(0, 0, 1)], hop=4, audio=x, denoise=None)
    assert int(off["energy_q32"][0]) - int(on["energy_q32"][0]) >= 2 * round(float(t) ** 2 * 2 ** 32) > 0      # +-thr themselves were zeroed
    only = np.zeros(frame, np.float32)
    only[5], only[9] = t, -t
    got = _same(eng, [(0, 0, 1)], hop=4, audio=only, denoise=THR, clip=THR)[0]
    assert (int(got["energy_q32"]), float(got["peak"]), int(got["clipped"])) == (0, 0.0, 0)
    got = _same(eng, [(0, 0, 1)], hop=4, audio=only, denoise=None, clip=THR)[0]
    assert (float(got["peak"]), int(got["clipped"])) == (float(t), 2)
    one = np.zeros(frame, np.float32)
    one[[0, frame - 1]] = 1.0, -1.0
    got = _same(eng, [(0, 0, 1)], hop=4, audio=one, clip=1.0)[0]
    assert (int(got["energy_q32"]), float(got["peak"]), int(got["clipped"])) == (2 << 32, 1.0, 2)
    # 2^-17 squared is a quarter of 2^-32: rounds to 0; 3 * 2^-17 squared is 2.25: rounds to 2; half-way cases go to even
    half = np.zeros(frame, np.float32)
    half[:3] = np.sqrt(0.5) * 2.0 ** -16, np.sqrt(1.5) * 2.0 ** -16, np.sqrt(2.5) * 2.0 ** -16
    _same(eng, [(0, 0, 1)], hop=4, audio=half, denoise=None)


def test_int16_minus_32768_under_32767_saturates(engines):
    eng = engines(16000)
    x = np.zeros(eng.frame_samples, np.int16)
    x[3], x[4], x[5] = -32768, 32767, -32767
    got = _same(eng, [(0, 0, 1)], hop=4, audio=x, clip=1.0)[0]
    assert int(got["energy_q32"]) == 3 << 32 and got["peak"] == np.float32(32768) / np.float32(32767) and int(got["clipped"]) == 3
    got = _same(eng, [(0, 0, 1)], hop=4, audio=x, clip=1.0, i16_scale=32768)[0]
    assert int(got["energy_q32"]) == 4 * (32768 ** 2 + 2 * 32767 ** 2) and float(got["peak"]) == 1.0 and int(got["clipped"]) == 1


# ---- non-finite -------------------------------------------------------------------------------------------------------
def test_nan_and_inf_stay_in_their_own_segments(engines):
    eng = engines(16000)
    frame = eng.frame_samples
    x = values(np.random.default_rng(9), "f32", 8 * frame)
    segs = [(0, 0, 2), (0, 2, 2), (0, 4, 2), (0, 6, 2), (0, 3, 1)]          # at hop = frame: frames 0-1, 2-3, 4-5, 6-7, and 3 again
    y = x.copy()
    y[frame + 7] = np.nan
    y[5 * frame - 1] = -np.inf
    y[5 * frame - 2] = np.nan
    y[5 * frame - 3] = np.inf
    clean = eng.levels(segs, hop=frame, audio=x, denoise=None)
    got = eng.levels(segs, hop=frame, audio=y, denoise=None)
    assert np.isnan(got["peak"][0]) and np.isnan(got["peak"][2])            # a NaN's pattern beats Inf
    y[5 * frame - 2] = 0
    got2 = eng.levels(segs, hop=frame, audio=y, denoise=None)
    assert np.isinf(got2["peak"][2]) and np.isnan(got2["peak"][0])
    for g in (got, got2):
        assert g[[1, 3, 4]].tobytes() == clean[[1, 3, 4]].tobytes()
    assert clean.tobytes() == of_cut(eng, segs, hop=frame, audio=x, denoise=None).tobytes()


# ---- rate blocks and other engines ------------------------------------------------------------------------------------
def test_a_48_khz_stereo_block_is_measured_at_its_own_rate_and_never_gated(engines):
    eng = engines(16000)
    chunk, hop = 1536, 772
    x = values(np.random.default_rng(48), "i16_32767", (chunk + 14 * hop + 40, 2))
    segs = [(0, 0, 15, 0), (0, 3, 1, 1), (4, 2, 9, "mix"), (0, 14, 1, "mix")]
    got = _same(eng, segs, hop=hop, audio=x, sample_rate=48000, denoise=0.3)
    assert got.tobytes() == eng.levels(segs, hop=hop, audio=x, sample_rate=48000, denoise=None).tobytes()
    for sg, rec in zip(segs, got):
        h = heard(x, "i16_32767", MIX if sg[3] == "mix" else sg[3])
        a = sg[0] + sg[1] * hop
        assert rec.tobytes() == records([h[a:a + (sg[2] - 1) * hop + chunk]]).tobytes(), sg


@pytest.mark.parametrize("rate", [None, 48000], ids=["own", "48k"])
def test_the_resident_block_behind_scan_segments(engines, rate):
    eng = engines(16000)
    kw = {} if rate is None else {"sample_rate": rate}
    chunk = eng.scan_chunk_samples(rate)
    hop = chunk // 2
    rec = values(np.random.default_rng(5), "i16_32767", (chunk + 11 * hop + 9, 2))
    slots = eng.open_streams(1)
    try:
        with eng.scan_session():
            eng.scan_segments(slots, [rec], hop=hop, denoise=THR, **kw)
            last = eng.last_scan
            segs = [(int(last["offsets"][0]), 1, 9, 0), (int(last["offsets"][0]), 0, 12), (int(last["offsets"][0]), 11, 1, 1)]
            got = eng.levels(segs, hop=hop, denoise=THR)
            want = of_cut(eng, segs, hop=hop, denoise=THR)
        block = np.zeros((last["samples"], 2), np.int16)
        block[:rec.shape[0]] = rec
        given = eng.levels(segs, hop=hop, denoise=THR, audio=block, **kw)
        assert got.tobytes() == want.tobytes() == given.tobytes() and (got["peak"] > 0.5).all()
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_the_device_form_on_a_v4_engine(engines):
    import torch
    eng = engines("v4")
    frame, hop = eng.frame_samples, 260
    x = values(np.random.default_rng(4), "ulaw", (9000, 2))
    segs = [(0, 3, 9, 0), (1028, 0, 20, "mix"), (1028, 1, 1, 1)]
    want = _same(eng, segs, hop=hop, audio=x, law="ulaw")
    d_audio = torch.from_numpy(x).cuda()
    d_lv = torch.full((len(segs) * 2 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.levels_device(segs, d_audio.data_ptr(), 9000, d_lv.data_ptr(), hop=hop, fmt=FMT["ulaw"], channels=2, stream=stream.cuda_stream)
    stream.synchronize()
    out = d_lv.cpu().numpy()
    assert out[:len(segs) * 2].tobytes() == want.tobytes() and (out[len(segs) * 2:] == 0x5A5A5A5A5A5A5A5A).all()
    assert eng.levels(segs, hop=hop, audio=x, law="ulaw").tobytes() == want.tobytes()      # waits for the launch by itself


# ---- gain -------------------------------------------------------------------------------------------------------------
def _gain_cases(eng):
    frame = eng.frame_samples
    rng = np.random.default_rng(77)
    own = (dict(hop=frame // 4 + 4, audio=values(rng, "f32", (9000, 2)), denoise=0.3),
           [(0, 3, 9, 0), (1028, 0, 30, "mix"), (1028, 1, 1, 1), (0, 0, 5)])
    rate = (dict(hop=772, audio=values(rng, "i16_32767", (1536 + 40 * 772 + 40, 2)), denoise=THR, sample_rate=48000),
            [(0, 0, 15, 0), (0, 3, 1, 1), (4, 2, 39, "mix"), (0, 14, 20, "mix")])
    return {"own": own, "48k": rate}


@pytest.mark.parametrize("out", ["pcm16", "f32"])
@pytest.mark.parametrize("layout", ["frames", "range"])
@pytest.mark.parametrize("which", ["own", "48k"])
def test_gains(engines, which, layout, out):
    eng = engines(16000)
    kw, segs = _gain_cases(eng)[which]
    plain, start = eng.cut(segs, layout=layout, out=out, **kw)
    ones, start1 = eng.cut(segs, layout=layout, out=out, gains=np.ones(len(segs), np.float32), **kw)
    assert ones.tobytes() == plain.tobytes() and list(start) == list(start1)
    f32, _ = eng.cut(segs, layout=layout, out="f32", **kw)
    # random finite gains, a negative one, a tiny one, and one that drives samples past full scale
    gains = np.array([0.37, -1.25, 2.0 ** -20, 40.0], np.float32)
    got, _ = eng.cut(segs, layout=layout, out=out, gains=gains, **kw)
    want = np.concatenate([f32[start[i]:start[i + 1]] * gains[i] for i in range(len(segs))]).astype(np.float32)
    assert got.tobytes() == (want if out == "f32" else pcm16(want)).tobytes()
    if out == "pcm16":
        loud = got[start[3]:start[4]]
        assert loud.max() == 32767 and loud.min() == -32768                     # saturated, both ways


def test_a_rate_frames_cut_with_gains_over_several_windows(engines):
    eng = engines(16000)
    kw, segs = _gain_cases(eng)["48k"]
    gains = np.array([0.5, 3.0, -0.75, 1.0], np.float32)
    whole, start = eng.cut(segs, layout="frames", out="f32", **kw)
    want = np.concatenate([whole[start[i]:start[i + 1]] * gains[i] for i in range(len(segs))]).astype(np.float32)
    eng.set_scan_launch_frames(1)           # windows of 32 frames: 75 frames in three windows, two segments cross a boundary
    try:
        for out in ("f32", "pcm16"):
            got, _ = eng.cut(segs, layout="frames", out=out, gains=gains, **kw)
            assert got.tobytes() == (want if out == "f32" else pcm16(want)).tobytes()
    finally:
        eng.set_scan_launch_frames(0)


def test_the_gain_device_form(engines):
    import torch
    eng = engines("v4")
    kw, segs = _gain_cases(eng)["own"]
    gains = np.array([0.37, -1.25, 2.0 ** -20, 40.0], np.float32)
    want, start = eng.cut(segs, gains=gains, **kw)
    d_audio = torch.from_numpy(kw["audio"]).cuda()
    d_out = torch.full((want.size + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    eng.cut_device(segs, d_audio.data_ptr(), 9000, d_out.data_ptr(), want.size, hop=kw["hop"], channels=2, denoise=kw["denoise"], gains=gains)
    eng.synchronize()
    out = d_out.cpu().numpy()
    assert out[:want.size].tobytes() == want.tobytes() and (out[want.size:] == 0x5A5A).all()


# ---- the corpus faces -------------------------------------------------------------------------------------------------
def _corpus():
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float32) / np.float32(32767.0)
    delayed = np.concatenate([np.zeros(3 * 16000, np.float32), pcm[:-3 * 16000]])
    whole = np.ascontiguousarray(np.stack([pcm * np.float32(0.5), delayed], axis=1))
    return [pcm[:pcm.size // 2], np.zeros(20000, np.float32), whole, pcm[pcm.size // 3:] * np.float32(0.25)]


CLIENT = dict(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)


def test_cut_recordings_normalize(engines):
    from cutter_vad_amd import VADConfig, cut_recordings
    eng = engines(16000)
    cfg = VADConfig(**CLIENT)
    recs = _corpus()
    target = 0.9
    n = 0
    for layout in ("range", "frames"):
        plain = cut_recordings(recs, cfg, engine=eng, layout=layout, wav=False)
        got = cut_recordings(recs, cfg, engine=eng, layout=layout, wav=False, normalize=target)
        wavs = cut_recordings(recs, cfg, engine=eng, layout=layout, normalize=target)
        assert [[w[44:] for _, _, w in r] for r in wavs] == [[p.tobytes() for _, _, p in r] for r in got]
        assert [[(a, b) for a, b, _ in r] for r in got] == [[(a, b) for a, b, _ in r] for r in plain] and got[1] == []
        for x, segs in zip(recs, got):
            h = gate(x if x.ndim == 1 else np.mean(x, axis=1), 0.01)
            for a, b, payload in segs:
                peak = np.abs(h[a:b]).max()
                g = np.float32(np.float32(target) / peak) if peak > 0 else np.float32(1)
                frames = h[a:b] if layout == "range" else np.concatenate([h[s:s + 512] for s in range(a, b - 511, 256)])
                assert payload.tobytes() == pcm16(frames * g).tobytes(), (a, b)
                # 0.9 * 32767 = 29490.3, and three float32 roundings move the product by less than 0.01: the bytes say 29490
                assert int(np.abs(payload.astype(np.int32)).max()) == 29490
                n += 1
    assert n >= 4


def test_scan_recordings_levels_with_refine_and_open_end(engines):
    from cutter_vad_amd import VADConfig, scan_recordings, sweep_recordings
    eng = engines(16000)
    cfg = VADConfig(**CLIENT)
    recs = _corpus()
    recs[0] = recs[0][:recs[0].size - 37000]            # stops inside speech more likely: an open segment is listed if there is one
    frame, hop = 512, 256
    rule = SegmentRefine(pad_before=2, pad_after=3, merge_gap=4, min_frames=3, max_frames=60)
    kw = dict(engine=eng, open_end=True, refine=rule)
    bare = scan_recordings(recs, cfg, stats=True, **kw)
    got = scan_recordings(recs, cfg, stats=True, levels=True, **kw)
    short = scan_recordings(recs, cfg, levels=True, **kw)
    n = 0
    for x, rb, rg, rs in zip(recs, bare, got, short):
        assert [r[:4] for r in rg] == rb and [r[:2] + r[4:] for r in rg] == rs
        if not rg:
            continue
        segs = [(0, a // hop, (b - a - frame) // hop + 1) for a, b, *_ in rg]
        lv = eng.levels(segs, hop=hop, denoise=0.01, audio=x)
        _, rms = level_stats(lv, [b - a for a, b, *_ in rg])
        assert [r[4:] for r in rg] == list(zip(rms.tolist(), lv["peak"].tolist(), lv["clipped"].tolist()))
        h = gate(x if x.ndim == 1 else np.mean(x, axis=1), 0.01)
        for r in rg:
            a, b = r[:2]
            q, peak, clipped = levels_ref(h[a:b])
            assert r[4] == float(np.sqrt(q / 2.0 ** 32 / (b - a))) and r[5] == float(peak) and r[6] == clipped
            n += 1
    assert n >= 2
    swept = sweep_recordings(recs, [cfg, VADConfig()], stats=True, levels=True, **kw)
    assert swept[0] == got and swept[1] == scan_recordings(recs, VADConfig(), stats=True, levels=True, **kw)
