"""vad_mel_stats / vad_mel_batch on the GPU (csrc/mel_batch.hip: vadk_mel_stats, vadk_mel_batch), byte for byte against
tests/batch_ref.py - the rule was written so that no tolerance is needed.  Synthetic float32 matrices, no scan, except in the last two
cases.  The shapes are the smallest at which the kernels can go wrong: MELB_STATS_ROWS is 256 rows per workgroup (the 5 000-row
segment crosses it 19 times), a batch tile has 64 frames - T = 68 has a tile of 4 - or 32 where 128 bands with two orders of deltas
would not fit the LDS, and the deltas' halo is 2 or 4 rows: segments of 1 to 5 and 9 rows meet every clamp depth."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import batch_ref as B
from tests.test_gpu_scan import GOLD, _engine
from tests.test_mel_batch_host import batch_cases, matrix, special_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint16 if got.itemsize == 2 else np.uint32) != want.view(np.uint16 if want.itemsize == 2 else np.uint32))
        raise AssertionError(f"{len(bad)} cells differ, the first at {bad[:4].tolist()}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")


# ---- statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [1, 5, 80, 128])
def test_stats_byte_for_byte(eng, n_mels):
    rng = np.random.default_rng(n_mels)
    x, start = matrix(rng, [0, 1, 63, 64, 65, 5000, 0, 257], n_mels, -2100.0, 2100.0)      # +-2048 and beyond: the clamp is live
    special_values(x[1:])
    x[start[7]:] = -np.abs(x[start[7]:])                                                       # a segment whose maximum is negative
    want = B.stats(x, start)
    st = eng.mel_stats(x, start)
    assert st["max"].tobytes() == want[0].tobytes() and st["sum"].tobytes() == want[1].tobytes() and st["sumsq"].tobytes() == want[2].tobytes()
    assert st["max"][0] == -np.inf and st["max"][6] == -np.inf and st["max"][7] < 0
    again = eng.mel_stats(x, start)
    assert all(again[k].tobytes() == st[k].tobytes() for k in st)                              # two runs, the same bytes
    only = eng.mel_stats(x, start, moments=False)
    assert set(only) == {"max"} and only["max"].tobytes() == want[0].tobytes()


def test_stats_each_output_null_in_turn_and_the_zeros(eng):
    import ctypes as C
    x = np.array([[-0.0, -0.0], [-0.0, -0.0], [-0.0, 0.0], [0.0, -0.0], [-1.0, -2.0], [-2.0, -0.5], [3000.0, 0.0], [-3000.0, 0.0]], np.float32)
    start = np.array([0, 2, 4, 6, 8], np.int64)
    want = B.stats(x, start)
    assert want[0].view(np.uint32).tolist() == [0x80000000, 0, np.float32(-0.5).view(np.uint32), np.float32(3000).view(np.uint32)]
    for skip in range(3):
        mx, s, s2 = np.full(4, 7, np.float32), np.full((4, 2), 7, np.int64), np.full((4, 2), 7, np.uint64)
        ptrs = [mx.ctypes.data_as(C.POINTER(C.c_float)), s.ctypes.data_as(C.POINTER(C.c_int64)), s2.ctypes.data_as(C.POINTER(C.c_uint64))]
        ptrs[skip] = None
        eng._check(eng._lib.vad_mel_stats(eng._h, x.ctypes.data_as(C.POINTER(C.c_float)), 8, 2, start.ctypes.data_as(C.POINTER(C.c_int64)), 4, *ptrs))
        for k, (got, ref) in enumerate(zip((mx, s, s2), want)):
            assert (got == 7).all() if k == skip else got.tobytes() == ref.tobytes(), (skip, k)


def test_stats_refuses_a_segment_of_2_17_plus_1_rows_without_a_launch(eng):
    from cutter_vad_amd.core.exceptions import AudioProcessingError
    start = np.array([0, 3, 3 + (1 << 17) + 1], np.int64)
    x = np.zeros(((1 << 17) + 4, 1), np.float32)
    x[5, 0] = 3.0
    with pytest.raises(AudioProcessingError, match="segment 1 has 131073 rows, the sums take 131072"):
        eng.mel_stats(x, start)
    assert eng.mel_stats(x, start, moments=False)["max"].tolist() == [0.0, 3.0]      # the maximum alone has no such bound


# ---- batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 64, 68])
@pytest.mark.parametrize("deltas", [0, 1, 2])
def test_batch_byte_for_byte(eng, T, deltas):
    rng = np.random.default_rng(10 * T + deltas)
    for n_mels in (5, 80, 128) if T == 68 else (5,):          # 128 bands, two orders: the tile of 32 frames
        x, start, win = batch_cases(rng, n_mels, T)
        n = len(start) - 1
        lo_some = np.sort(x, axis=None)[[x.size // 3] * n].astype(np.float32)          # a finite lo that IS a feature value
        sh1, sc1 = rng.uniform(-2, 2, (1, n_mels)).astype(np.float32), rng.uniform(0.1, 3, (1, n_mels)).astype(np.float32)
        shn, scn = rng.uniform(-2, 2, (n, n_mels)).astype(np.float32), rng.uniform(0.1, 3, (n, n_mels)).astype(np.float32)
        for layout in ("channel", "time"):
            for dtype in ("f32", "f16", "bf16"):
                for pad, (lo, sh, sc) in (("value", (None, None, None)), ("feature", (lo_some, shn, scn)), ("feature", (None, sh1, sc1))):
                    rec = dict(frames=T, deltas=deltas, layout=layout, dtype=dtype, pad=pad, pad_value=-10.0)
                    want = B.batch(x, start, win, n_mels, T, deltas, _ffi.BATCH_LAYOUTS[layout], _ffi.BATCH_DTYPES[dtype], _ffi.BATCH_PADS[pad],
                                   -10.0, lo, sh, sc)
                    got = eng.mel_batch(win, rec, lo=lo, shift=sh, scale=sc, features=x, start=start)
                    _same(got, want)
        again = eng.mel_batch(win, rec, lo=lo, shift=sh, scale=sc, features=x, start=start)
        assert again.tobytes() == got.tobytes()                                        # two runs, the same bytes


def test_batch_rule_is_add_then_multiply_and_float16_overflows_to_inf(eng):
    rng = np.random.default_rng(5)
    x, start = matrix(rng, [64], 8, -1.0, 1.0)
    sh, sc = rng.uniform(0.5, 1.5, (1, 8)).astype(np.float32), rng.uniform(0.5, 3, (1, 8)).astype(np.float32)
    want = B.batch(x, start, [(0, 64, 0)], 8, 64, shift=sh, scale=sc)
    fused = (x.astype(np.float64) * sc.astype(np.float64) + (sh * sc).astype(np.float64)).astype(np.float32).T[None]
    assert (fused != want).sum() > 50
    _same(eng.mel_batch([(0, 64, 0)], dict(frames=64), shift=sh, scale=sc, features=x, start=start), want)
    big = np.array([[65519.0, 65520.0, -70000.0, 1e30]], np.float32)
    got = eng.mel_batch([(0, 1, 0)], dict(frames=4, dtype="f16"), features=big, start=[0, 1])
    assert got[0, :, 0].tolist() == [65504.0, np.inf, -np.inf, np.inf]
    # a difference that overflows float32 where a fused 2 * d + e would not
    v = np.array([[3e38], [3e38], [0.0], [-1e38], [-1e38]], np.float32)
    _same(eng.mel_batch([(0, 5, 0)], dict(frames=8, deltas=2), features=v, start=[0, 5]), B.batch(v, [0, 5], [(0, 5, 0)], 1, 8, 2))


def test_batch_device_form_and_alignment(eng):
    import torch
    from cutter_vad_amd.core.exceptions import AudioProcessingError
    rng = np.random.default_rng(9)
    x, start, win = batch_cases(rng, 5, 64)
    want = B.batch(x, start, win, 5, 64, 1, dtype=B.F16)
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros(want.size + 8, dtype=torch.float16, device="cuda")
    shape = eng.mel_batch_device(win, dict(frames=64, deltas=1, dtype="f16"), d_out.data_ptr(), want.nbytes, d_features=d_x.data_ptr(), rows=x.shape[0],
                                 n_mels=5, start=start)
    eng.synchronize()
    assert shape == want.shape
    host = d_out.cpu().numpy()
    assert host[:want.size].tobytes() == want.tobytes() and not host[want.size:].any()
    with pytest.raises(AudioProcessingError, match="the output must be 16-byte aligned"):
        eng.mel_batch_device(win, dict(frames=64, deltas=1, dtype="f16"), d_out.data_ptr() + 2, want.nbytes, d_features=d_x.data_ptr(), rows=x.shape[0],
                             n_mels=5, start=start)


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_keep_stats_batch_behind_a_scan(eng):
    from cutter_vad_amd.scan import MelSpec
    hop = 256
    rec = np.load(GOLD + "/speech16k_i16.npz")["pcm"][16000:16000 + 40 * 256 + 512]
    slots = eng.open_streams(1)
    spec = MelSpec(16000, n_mels=40)
    try:
        with eng.scan_session():
            eng.scan_segments(slots, [rec], hop=hop, denoise=0.01)
            off = int(eng.last_scan["offsets"][0])
            segs = [(off, 1, 9), (off, 0, 40), (off, 11, 1)]
            want, wstart = eng.mel(segs, spec, hop=hop, denoise=0.01)
            start = eng.mel_keep(segs, spec, hop=hop, denoise=0.01)
            assert start.tolist() == wstart.tolist() and eng.mel_resident() == (int(start[-1]), 40, 3)
            assert eng.mel_resident_read().tobytes() == want.tobytes()
            st = eng.mel_stats()
            ref = B.stats(want, wstart)
            assert st["max"].tobytes() == ref[0].tobytes() and st["sum"].tobytes() == ref[1].tobytes() and st["sumsq"].tobytes() == ref[2].tobytes()
            win = [(1, 32, 2), (0, 17, 0), (2, 4, 0), (1, 32, 33)]
            got = eng.mel_batch(win, dict(frames=32, deltas=2, dtype="f16", pad="feature", pad_value=-10.0), lo=st["max"] - np.float32(8), shift=4.0,
                                scale=0.25)
        _same(got, B.batch(want, wstart, win, 40, 32, 2, dtype=B.F16, pad_mode=B.PAD_FEATURE, pad_value=-10.0, lo=ref[0] - np.float32(8),
                           shift=np.full(40, 4, np.float32), scale=np.full(40, 0.25, np.float32)))
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_batch_recordings_whisper_setting_in_float16(eng):
    from cutter_vad_amd import FeatureBatch, MelSpec, VADConfig, batch_recordings, features_recordings
    pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"].astype(np.float32) / np.float32(32767.0)
    recs = [pcm[:pcm.size // 2], np.zeros(20000, np.float32), pcm[pcm.size // 2:]]
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    spec = MelSpec(16000)
    fb = FeatureBatch(frames=3000, norm="whisper", pad="feature", pad_value=-10.0, dtype="f16")
    got, index = batch_recordings(recs, spec, fb, cfg, engine=eng, open_end=True)
    feats = features_recordings(recs, spec, cfg, engine=eng, open_end=True)
    segs = [(i, a, b, f) for i, one in enumerate(feats) for a, b, f in one]
    assert len(segs) >= 2
    x = np.concatenate([f for *_, f in segs])
    start = np.concatenate([[0], np.cumsum([f.shape[0] for *_, f in segs])])
    win = [(k, min(3000, f.shape[0] - r), r) for k, (*_, f) in enumerate(segs) for r in range(0, f.shape[0], 3000)]
    lo = B.stats(x, start)[0] - np.float32(8)
    want = B.batch(x, start, win, 80, 3000, dtype=B.F16, pad_mode=B.PAD_FEATURE, pad_value=-10.0, lo=lo, shift=np.full(80, 4, np.float32),
                   scale=np.full(80, 0.25, np.float32))
    _same(got, want)
    assert index == [(segs[k][0], 0, segs[k][1], segs[k][2], r, nr) for k, nr, r in win]
    # Whisper's own two lines on a clip, then its padding: a frame of log10(1e-10) through the same lines
    k = 0
    clip = np.maximum(segs[k][3], segs[k][3].max() - np.float32(8.0))
    clip = ((clip + np.float32(4.0)) / np.float32(4.0)).astype(np.float16)
    assert got[0, :, :win[0][1]].tobytes() == np.ascontiguousarray(clip[:win[0][1]].T).tobytes()
