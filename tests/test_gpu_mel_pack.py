"""vad_mel_batch_packed / vad_mel_stats_grouped on the GPU (csrc/mel_batch.hip: vadk_mel_batch_packed, vadk_mel_stats), byte for byte
against tests/pack_ref.py - no tolerance anywhere.  Synthetic float32 matrices, no scan, except in the last two cases.  The shapes
are the smallest at which the kernel can go wrong: a workgroup serves 64 frames of a PIECE (32 where 128 bands with two orders of
deltas would not fit the LDS), so the 64- and 72-row pieces of the long segment cross a tile and every short piece ends in a tile of
4 or 8 frames; pieces of 1 to 5 and 9 rows meet every clamp depth of the deltas' halo, at offsets 0, 4, T - 8 and T - 4; T = 72
holds the piece of 9 rows at offset 60."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi
from tests import batch_ref as B
from tests import pack_ref as P
from tests.test_gpu_scan import GOLD, _engine
from tests.test_mel_batch_host import matrix, special_values
from tests.test_mel_pack_host import EXAMPLE_GROUPS, EXAMPLE_ROWS, PACK_SEGS, affines, pack_cases, piece_array

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


LAYOUTS, DTYPES, PADS = {v: k for k, v in _ffi.BATCH_LAYOUTS.items()}, {v: k for k, v in _ffi.BATCH_DTYPES.items()}, {v: k for k, v in _ffi.BATCH_PADS.items()}


# ---- packed batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 64, 68, 72])
@pytest.mark.parametrize("deltas", [0, 1, 2])
def test_packed_byte_for_byte(eng, T, deltas):
    rng = np.random.default_rng(10 * T + deltas)
    for n_mels in {4: (5,), 64: (1, 5), 68: (5, 80), 72: (5, 128)}[T]:      # 128 bands, two orders: the tile of 32 frames
        x, start, pieces, nw = pack_cases(rng, n_mels, T)
        for layout in (B.CHANNEL, B.TIME):
            for dtype in (B.F32, B.F16, B.BF16):
                for pad_mode, (lo, sh, sc, nss) in affines(rng, x, nw, n_mels):
                    rec = dict(frames=T, deltas=deltas, layout=LAYOUTS[layout], dtype=DTYPES[dtype], pad=PADS[pad_mode], pad_value=-10.0)
                    want = P.batch(x, start, pieces, nw, n_mels, T, deltas, layout, dtype, pad_mode, -10.0, lo, sh, sc)
                    got = eng.mel_batch_packed(pieces, nw, rec, lo=lo, shift=sh, scale=sc, features=x, start=start)
                    _same(got, want)
        again = eng.mel_batch_packed(pieces, nw, rec, lo=lo, shift=sh, scale=sc, features=x, start=start)
        assert again.tobytes() == got.tobytes()                                        # two runs, the same bytes


@pytest.mark.parametrize("gap", [0, 2])
def test_packed_planned_windows(eng, gap):
    """the planner's output for the header's worked example, with real rows: segments of 64 and 70 rows in windows of 68"""
    from cutter_vad_amd import batch_pack
    rng = np.random.default_rng(gap)
    x, start = matrix(rng, EXAMPLE_ROWS, 5)
    pieces, nw = batch_pack(start, 68, gap, EXAMPLE_GROUPS)
    assert (pieces.tolist(), nw) == (piece_array(P.plan(start, 68, gap, EXAMPLE_GROUPS)[0]).tolist(), 5)
    for deltas in (0, 2):
        for pad_mode, (lo, sh, sc, nss) in affines(rng, x, nw, 5):
            want = P.batch(x, start, pieces.tolist(), nw, 5, 68, deltas, B.CHANNEL, B.F16, pad_mode, -10.0, lo, sh, sc)
            _same(eng.mel_batch_packed(pieces, nw, dict(frames=68, deltas=deltas, dtype="f16", pad=PADS[pad_mode], pad_value=-10.0), lo=lo, shift=sh,
                                       scale=sc, features=x, start=start), want)


def test_single_piece_windows_are_vad_mel_batch(eng):
    rng = np.random.default_rng(21)
    x, start = matrix(rng, PACK_SEGS, 5)
    win = [(7, 64, 2), (0, 1, 0), (5, 9, 0), (7, 22, 128), (3, 2, 1), (7, 68, 80)]
    pieces = [(s, k, r, w, 0) for w, (s, k, r) in enumerate(win)]
    n, segs = len(start) - 1, [w[0] for w in win]
    lo_n, sh_n, sc_n = rng.uniform(-8, 0, n).astype(np.float32), rng.uniform(-2, 2, (n, 5)).astype(np.float32), rng.uniform(0.1, 3, (n, 5)).astype(np.float32)
    for deltas in (0, 1, 2):
        for layout in ("channel", "time"):
            for dtype in ("f32", "f16", "bf16"):
                rec = dict(frames=68, deltas=deltas, layout=layout, dtype=dtype, pad="feature", pad_value=-10.0)
                old = eng.mel_batch(win, rec, lo=lo_n, shift=sh_n, scale=sc_n, features=x, start=start)
                new = eng.mel_batch_packed(pieces, len(win), rec, lo=lo_n[segs], shift=sh_n[segs], scale=sc_n[segs], features=x, start=start)
                _same(new, old)


def test_packed_rule_is_add_then_multiply_and_float16_overflows_to_inf(eng):
    rng = np.random.default_rng(5)
    x, start = matrix(rng, [64], 8, -1.0, 1.0)
    sh, sc = rng.uniform(0.5, 1.5, (1, 8)).astype(np.float32), rng.uniform(0.5, 3, (1, 8)).astype(np.float32)
    pieces = [(0, 30, 0, 0, 0), (0, 30, 30, 0, 32)]
    want = P.batch(x, start, pieces, 1, 8, 64, shift=sh, scale=sc)
    fused = (x.astype(np.float64) * sc.astype(np.float64) + (sh * sc).astype(np.float64)).astype(np.float32)
    assert (fused[:30].T != want[0, :, :30]).sum() > 20
    _same(eng.mel_batch_packed(pieces, 1, dict(frames=64), shift=sh, scale=sc, features=x, start=start), want)
    big = np.array([[65519.0, 65520.0, -70000.0, 1e30]], np.float32)
    got = eng.mel_batch_packed([(0, 1, 0, 0, 4)], 1, dict(frames=8, dtype="f16"), features=big, start=[0, 1])
    assert got[0, :, 4].tolist() == [65504.0, np.inf, -np.inf, np.inf] and not got[0, :, :4].any() and not got[0, :, 5:].any()
    # a difference that overflows float32 where a fused 2 * d + e would not, in a piece behind another
    v = np.array([[3e38], [3e38], [0.0], [-1e38], [-1e38]], np.float32)
    pieces = [(0, 2, 0, 0, 0), (0, 3, 2, 0, 4)]
    _same(eng.mel_batch_packed(pieces, 1, dict(frames=8, deltas=2), features=v, start=[0, 5]), P.batch(v, [0, 5], pieces, 1, 1, 8, 2))


def test_packed_of_nothing_and_a_refusal(eng):
    from cutter_vad_amd.core.exceptions import AudioProcessingError
    x, start = matrix(np.random.default_rng(7), [5], 5)
    sh = np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 1]], np.float32)
    for pad in ("value", "feature"):
        got = eng.mel_batch_packed([], 2, dict(frames=8, deltas=2, dtype="bf16", pad=pad, pad_value=-3.0), lo=[-np.inf, 0.0], shift=sh, features=x, start=start)
        _same(got, P.batch(x, start, [], 2, 5, 8, 2, B.CHANNEL, B.BF16, _ffi.BATCH_PADS[pad], -3.0, [-np.inf, 0.0], sh))
    assert eng.mel_batch_packed([], 0, dict(frames=8), features=x, start=start).shape == (0, 5, 8)
    with pytest.raises(AudioProcessingError, match="pieces 0 and 1 overlap in window 0"):
        eng.mel_batch_packed([(0, 5, 0, 0, 0), (0, 1, 0, 0, 4)], 1, dict(frames=8), features=x, start=start)


def test_packed_device_form_and_alignment(eng):
    import torch
    from cutter_vad_amd.core.exceptions import AudioProcessingError
    rng = np.random.default_rng(9)
    x, start, pieces, nw = pack_cases(rng, 5, 72)
    want = P.batch(x, start, pieces, nw, 5, 72, 1, dtype=B.F16)
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros(want.size + 8, dtype=torch.float16, device="cuda")
    rec = dict(frames=72, deltas=1, dtype="f16")
    shape = eng.mel_batch_packed_device(pieces, nw, rec, d_out.data_ptr(), want.nbytes, d_features=d_x.data_ptr(), rows=x.shape[0], n_mels=5, start=start)
    eng.synchronize()
    assert shape == want.shape
    host = d_out.cpu().numpy()
    assert host[:want.size].tobytes() == want.tobytes() and not host[want.size:].any()
    with pytest.raises(AudioProcessingError, match="the output must be 16-byte aligned"):
        eng.mel_batch_packed_device(pieces, nw, rec, d_out.data_ptr() + 2, want.nbytes, d_features=d_x.data_ptr(), rows=x.shape[0], n_mels=5, start=start)


# ---- grouped statistics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [1, 80])
def test_grouped_stats_byte_for_byte(eng, n_mels):
    rng = np.random.default_rng(n_mels)
    x, start = matrix(rng, [0, 1, 257, 5000, 0, 257], n_mels, -2100.0, 2100.0)       # 5 000 rows cross the workgroup's 256 rows 19 times
    special_values(x[1:])
    x[start[5]:] = -np.abs(x[start[5]:])
    n = len(start) - 1
    plain = eng.mel_stats(x, start)
    for group, ng in (([0] * n, 1), ([0, 1, 0, 1, 0, 1], 2), ([1, 1, 0, 0, 2, 4], 5), (list(range(n)), n)):
        want = P.stats_grouped(x, start, group, ng)
        st = eng.mel_stats(x, start, group=(group, ng))
        assert st["max"].tobytes() == want[0].tobytes() and st["sum"].tobytes() == want[1].tobytes() and st["sumsq"].tobytes() == want[2].tobytes()
        again = eng.mel_stats(x, start, group=(group, ng))
        assert all(again[k].tobytes() == st[k].tobytes() for k in st)                  # two runs, the same bytes
    assert all(st[k].tobytes() == plain[k].tobytes() for k in st)                      # n groups of one segment: vad_mel_stats's bytes
    st = eng.mel_stats(x, start, group=([1, 1, 0, 0, 2, 4], 5), moments=False)
    assert set(st) == {"max"} and st["max"][3] == -np.inf and st["max"][2] == -np.inf and st["max"][4] < 0


def test_grouped_stats_refuse_a_group_of_2_17_plus_1_rows_without_a_launch(eng):
    from cutter_vad_amd.core.exceptions import AudioProcessingError
    half = 1 << 16
    start = np.array([0, half, 2 * half + 1, 2 * half + 2], np.int64)
    x = np.zeros((2 * half + 2, 1), np.float32)
    x[half + 5, 0] = 3.0
    with pytest.raises(AudioProcessingError, match="group 1 has 131073 rows, the sums take 131072"):
        eng.mel_stats(x, start, group=[1, 1, 0])
    assert eng.mel_stats(x, start, group=[1, 1, 0], moments=False)["max"].tolist() == [0.0, 3.0]
    st = eng.mel_stats(x, start, group=[1, 0, 1])
    assert st["max"].tolist() == [3.0, 0.0] and st["sum"].tolist() == [[3 * 4096], [0]]


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_keep_grouped_stats_packed_batch_behind_a_scan(eng):
    from cutter_vad_amd import batch_pack
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
            assert start.tolist() == wstart.tolist()
            pieces, nw = batch_pack(start, 32, 1)
            ref_pieces, ref_nw = P.plan(wstart, 32, 1)
            assert (pieces.tolist(), nw) == (piece_array(ref_pieces).tolist(), ref_nw) and nw < len(pieces)
            bounds = P.piece_bounds(wstart, ref_pieces)
            st = eng.mel_stats(start=bounds, group=(pieces["window"], nw))       # window scope: one call on the resident matrix
            ref = P.stats_grouped(want, bounds, pieces["window"], nw)
            assert st["max"].tobytes() == ref[0].tobytes() and st["sum"].tobytes() == ref[1].tobytes() and st["sumsq"].tobytes() == ref[2].tobytes()
            got = eng.mel_batch_packed(pieces, nw, dict(frames=32, deltas=2, dtype="f16", pad="feature", pad_value=-10.0), lo=st["max"] - np.float32(8),
                                       shift=4.0, scale=0.25)
        _same(got, P.batch(want, wstart, ref_pieces, nw, 40, 32, 2, dtype=B.F16, pad_mode=B.PAD_FEATURE, pad_value=-10.0, lo=ref[0] - np.float32(8),
                           shift=np.full(40, 4, np.float32), scale=np.full(40, 0.25, np.float32)))
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_batch_recordings_packed_whisper_setting_in_float16(eng):
    from cutter_vad_amd import FeatureBatch, MelSpec, VADConfig, batch_recordings, features_recordings
    pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"].astype(np.float32) / np.float32(32767.0)
    recs = [pcm[:pcm.size // 2], np.zeros(20000, np.float32), pcm[pcm.size // 2:]]
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    spec = MelSpec(16000)
    fb = FeatureBatch(frames=3000, norm="whisper", pad="feature", pad_value=-10.0, dtype="f16", pack=True)
    got, index = batch_recordings(recs, spec, fb, cfg, engine=eng, open_end=True)
    feats = features_recordings(recs, spec, cfg, engine=eng, open_end=True)
    segs = [(i, a, b, f) for i, one in enumerate(feats) for a, b, f in one]
    assert len(segs) >= 2
    x = np.concatenate([f for *_, f in segs])
    start = np.concatenate([[0], np.cumsum([f.shape[0] for *_, f in segs])])
    pieces, nw = P.plan(start, 3000, 0, [i for i, *_ in segs])
    parr = piece_array(pieces)
    lo = P.stats_grouped(x, P.piece_bounds(start, pieces), parr["window"], nw)[0] - np.float32(8)
    want = P.batch(x, start, pieces, nw, 80, 3000, dtype=B.F16, pad_mode=B.PAD_FEATURE, pad_value=-10.0, lo=lo, shift=np.full(80, 4, np.float32),
                   scale=np.full(80, 0.25, np.float32))
    _same(got, want)
    assert index == [(segs[s][0], 0, segs[s][1], segs[s][2], r, k, w, o) for s, k, r, w, o in pieces]
    assert nw == len({i for i, *_ in segs}) or nw < len(pieces)
    # Whisper's own two lines on the first window's first piece, under the WINDOW's maximum
    s, k, r, w, o = pieces[0]
    top = max(segs[p[0]][3][p[2]:p[2] + p[1]].max() for p in pieces if p[3] == 0)
    clip = np.maximum(segs[s][3][r:r + k], top - np.float32(8.0))
    clip = ((clip + np.float32(4.0)) / np.float32(4.0)).astype(np.float16)
    assert got[0, :, o:o + k].tobytes() == np.ascontiguousarray(clip.T).tobytes()
