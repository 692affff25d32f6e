"""vad_scan_moments / vad_scan_audio_batch on the GPU (csrc/scan_levels.hip: vadk_seg_moments, csrc/audio_batch.hip:
vadk_audio_batch), byte for byte against tests/audio_batch_ref.py - the rule was written so that no tolerance is needed.  Synthetic
blocks, no scan.  The shapes sit around the kernels' edges: a lane is one quad, a wave 64, a pass 256 and a workgroup 1024 quads.
A SEGMENT is a frame at the least - 128 quads on the 16 kHz engines, 64 on the 8 kHz one - so segments of 128, 129, 255 .. 257,
1023 .. 1025 and 2049 quads come from hop = 4 on the 16 kHz engine and 64 and 65 quads from the 8 kHz engine; spans of 1, 2, 63,
64 and 65 quads, which no segment can have, are shown as WINDOWS (nsamples of 4 .. 260), where the batch kernel meets the same edges."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import audio_batch_ref as AR
from tests.batch_ref import BF16, F16, F32, PAD_FEATURE, PAD_VALUE
from tests.cut_ref import FMT, MIX, values
from tests.test_gpu_scan import _engine

pytestmark = pytest.mark.gpu

KINDS = ("f32", "i16_32767", "i16_32768", "ulaw", "alaw")
QUADS = (128, 129, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 1)
DT = {F32: "f32", F16: "f16", BF16: "bf16"}
PAD = {PAD_VALUE: "value", PAD_FEATURE: "feature"}


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        u = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError(f"{len(bad)} cells differ, the first at {bad[:4].tolist()}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")


def _args(kind):
    return dict(law=kind if kind in ("ulaw", "alaw") else None, i16_scale=32768 if kind == "i16_32768" else 32767)


def _block(rng, kind, channels, ns):
    block = values(rng, kind, (ns, 2) if channels == 2 else ns)
    if kind == "f32":
        flat = block.reshape(-1)
        flat[8:20] = [0.0, -0.0, 1e-40, -1e-40, 0.01, -0.01, 1.0, -1.0, 1.2, -1.2, np.float32(0.01), 5e-39]   # +-0, denormals, the gate's threshold
    return block


def _table(quads, frame, hop, channel):
    """segments of `quads` quads each, every one in a recording of its own, the recordings back to back -> (table for the Engine,
    items for the reference, samples of the block)"""
    table, items, at = [], [], 0
    for q in quads:
        nf = (4 * q - frame) // hop + 1
        assert (nf - 1) * hop + frame == 4 * q
        table.append((at, 0, nf) if channel == "mono" else (at, 0, nf, "mix" if channel == MIX else channel))
        items.append((at, 0, nf, 0, 0 if channel == "mono" else channel))
        at += 4 * q
    return table, items, at


@pytest.fixture(scope="module")
def edge(eng):
    """the float32 block of the edge segments, its reference cut and its moments: computed once, shared, left unchanged"""
    rng = np.random.default_rng(1)
    table, items, ns = _table(QUADS, 512, 4, "mono")
    block = _block(rng, "f32", 1, ns)
    segs = {thr: [AR.segment(block, "f32", it, 512, 4, thr) for it in items] for thr in (None, 0.01)}
    return table, block, segs


def test_moments_at_the_edges_and_equal_to_the_levels_energy(eng, edge):
    table, block, segs = edge
    for thr in (None, 0.01):
        mo = eng.moments(table, hop=4, denoise=thr, audio=block)
        _same(mo, AR.moments_records(segs[thr]))
        lv = eng.levels(table, hop=4, denoise=thr, audio=block)
        assert lv["energy_q32"].tobytes() == mo["energy_q32"].tobytes()
        assert eng.moments(table, hop=4, denoise=thr, audio=block).tobytes() == mo.tobytes()          # two runs, the same bytes
    # segments that share samples, in another order
    again = [table[8], table[0], table[8], table[4]]
    _same(eng.moments(again, hop=4, denoise=None, audio=block), AR.moments_records([segs[None][i] for i in (8, 0, 8, 4)]))


@pytest.mark.parametrize("kind", KINDS)
def test_moments_every_format_and_channel(eng, kind):
    rng = np.random.default_rng(5)
    for channel in ("mono", 0, 1, MIX):
        table, items, ns = _table((128, 1025, 257), 512, 4, channel)
        block = _block(rng, kind, 1 if channel == "mono" else 2, ns)
        segs = [AR.segment(block, kind, it, 512, 4, 0.01) for it in items]
        mo = eng.moments(table, hop=4, audio=block, **_args(kind))
        _same(mo, AR.moments_records(segs))
        assert eng.levels(table, hop=4, audio=block, **_args(kind))["energy_q32"].tobytes() == mo["energy_q32"].tobytes()
        if kind in ("i16_32768", "ulaw", "alaw") and channel != MIX:
            from tests import g711_ref as G
            raw = block.astype(np.int64) if kind == "i16_32768" else G.table(kind)[block].astype(np.int64)
            raw = raw if channel == "mono" else raw[:, channel]
            mo = eng.moments(table, hop=4, denoise=None, audio=block, **_args(kind))
            assert int(mo["sum_q31"][1]) == 65536 * int(raw[512:512 + 4100].sum()) and int(mo["energy_q32"][1]) == 4 * int((raw[512:512 + 4100] ** 2).sum())


@pytest.mark.parametrize("T", [4, 4096, 4100, 8196])
def test_batch_window_lengths_and_positions(eng, edge, T):
    table, block, segs = edge
    S = [s.size for s in segs[None]]
    windows = []
    for ns in (0, 1, 3, 4, 5, T - 1, T):
        if ns <= T:                                                       # (T = 4 has no window of 5)
            windows += [(8, ns, 0), (8, ns, 8196 - ((ns + 3) & ~3))]           # sample0 = 0, and up to the segment's last quad
    windows += [(i, min(S[i], T), 0) for i in range(len(S))] + [(i, min(S[i], T), S[i] - ((min(S[i], T) + 3) & ~3)) for i in range(len(S))]
    windows += [(3, ns, 4 * 63) for ns in (4, 8, 252, 256, 260) if ns <= T] + [(0, min(T, 4), 508), (0, 1, 508)]
    shift = np.linspace(-0.5, 0.5, len(S)).astype(np.float32)
    scale = np.linspace(0.5, 3.0, len(S)).astype(np.float32)
    got, m = eng.audio_batch(table, windows, dict(samples=T, pad="feature"), shift=shift, scale=scale, mask=True, hop=4, audio=block)
    want, wm = AR.batch(segs[0.01], windows, T, F32, PAD_FEATURE, 0.0, shift, scale)
    _same(got, want)
    _same(m, wm)
    got2 = eng.audio_batch(table, windows, dict(samples=T, dtype="bf16", pad_value=-2.0), hop=4, denoise=None, audio=block)
    _same(got2, AR.batch(segs[None], windows, T, BF16, PAD_VALUE, -2.0)[0])
    assert eng.audio_batch(table, windows, dict(samples=T, dtype="bf16", pad_value=-2.0), hop=4, denoise=None, audio=block).tobytes() == got2.tobytes()


def _shuffled(S, T):
    """one window list that is reversed, overlapping and duplicated"""
    w = [(i, min(s, T), 0) for i, s in enumerate(S)] + [(i, min(s - 4, T), 4) for i, s in enumerate(S)]
    w += [(1, min(T, 260), 256), (1, min(T, 260), 256), (0, 0, 0), (2, 5, S[2] - 8)]
    return w[::-1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channel", ["mono", 0, 1, MIX])
def test_batch_every_format_channel_dtype_and_pad(eng, kind, channel):
    rng = np.random.default_rng(3)
    table, items, ns = _table((128, 1025, 257), 512, 4, channel)
    block = _block(rng, kind, 1 if channel == "mono" else 2, ns)
    segs = [AR.segment(block, kind, it, 512, 4, 0.01) for it in items]
    T = 1028
    windows = _shuffled([s.size for s in segs], T)
    shift, scale = np.array([0.25, -0.5, 0.015625], np.float32), np.array([3.0, 0.3, -1.7], np.float32)
    for dtype in (F32, F16, BF16):
        for pad_mode in (PAD_VALUE, PAD_FEATURE):
            for sh, sc in ((shift, scale), (shift[1:2], scale[1:2]), (None, None)):
                mask = (dtype + pad_mode) % 2 == 0
                got = eng.audio_batch(table, windows, dict(samples=T, dtype=DT[dtype], pad=PAD[pad_mode], pad_value=-3.5), shift=sh, scale=sc, mask=mask,
                                      hop=4, audio=block, **_args(kind))
                want, wm = AR.batch(segs, windows, T, dtype, pad_mode, -3.5, sh, sc)
                _same(got[0] if mask else got, want)
                if mask:
                    _same(got[1], wm)


def test_float16_overflows_to_inf(eng, edge):
    table, block, segs = edge
    got = eng.audio_batch(table[:1], [(0, 512, 0)], dict(samples=512, dtype="f16"), scale=[1e5], hop=4, denoise=None, audio=block)
    want = AR.batch(segs[None][:1], [(0, 512, 0)], 512, F16, scale=[1e5])[0]
    _same(got, want)
    assert np.isinf(got).any() and not np.isnan(got).any()


def test_device_forms_write_every_cell_and_nothing_else(eng, edge):
    import torch
    from cutter_vad_amd.core.exceptions import AudioProcessingError
    table, block, segs = edge
    T = 4100
    windows = _shuffled([s.size for s in segs[0.01]], T)
    nw = len(windows)
    d_audio = torch.from_numpy(block).cuda()
    where = dict(d_audio=d_audio.data_ptr(), audio_samples=block.size)
    for dtype, tdt in ((F16, torch.float16), (F32, torch.float32)):
        want, wm = AR.batch(segs[0.01], windows, T, dtype, PAD_FEATURE, 0.0, [0.125], [0.5])
        d_out = torch.full((nw * T + 16,), -7.0, dtype=tdt, device="cuda")
        d_mask = torch.full((nw * T + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        shape = eng.audio_batch_device(table, windows, dict(samples=T, dtype=DT[dtype], pad="feature"), d_out=d_out.data_ptr(), out_bytes=want.nbytes,
                                       d_mask=d_mask.data_ptr(), shift=[0.125], scale=[0.5], hop=4, **where)
        eng.synchronize()
        assert shape == want.shape
        host, hm = d_out.cpu().numpy(), d_mask.cpu().numpy()
        _same(host[:nw * T].reshape(nw, T), want)
        _same(hm[:nw * T].reshape(nw, T), wm)
        assert (host[nw * T:] == -7.0).all() and (hm[nw * T:] == 0x5A).all()
    d_mo = torch.full((2 * len(table) + 2,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    eng.moments_device(table, d_moments=d_mo.data_ptr(), hop=4, **where)
    eng.synchronize()
    mo = d_mo.cpu().numpy()
    assert mo[:2 * len(table)].tobytes() == AR.moments_records(segs[0.01]).tobytes() and (mo[2 * len(table):] == 0x5A5A5A5A).all()
    with pytest.raises(AudioProcessingError, match="the output must be 16-byte aligned"):
        eng.audio_batch_device(table, windows, dict(samples=T), d_out=d_out.data_ptr() + 4, out_bytes=nw * T * 4, hop=4, **where)
    with pytest.raises(AudioProcessingError, match="the mask must be 4-byte aligned"):
        eng.audio_batch_device(table, windows, dict(samples=T), d_out=d_out.data_ptr(), out_bytes=nw * T * 4, d_mask=d_mask.data_ptr() + 2, hop=4, **where)
    with pytest.raises(AudioProcessingError, match="the moments must be 8-byte aligned"):
        eng.moments_device(table, d_moments=d_mo.data_ptr() + 4, hop=4, **where)


def test_a_48_khz_rate_block_is_not_gated(eng):
    rng = np.random.default_rng(8)
    block = (values(rng, "i16_32767", 6 * 1536 + 768)).astype(np.int16)
    block[:64] = 100                                   # under the gate's threshold: a rate block keeps them
    table = [(0, 0, 3), (1536, 1, 2)]
    segs = [AR.segment(block, "i16_32767", (o, f, n, 0, 0), 1536, 768, None) for o, f, n in table]
    assert [s.size for s in segs] == [3072, 2304]
    mo = eng.moments(table, audio=block, sample_rate=48000)
    _same(mo, AR.moments_records(segs))
    assert eng.levels(table, audio=block, sample_rate=48000)["energy_q32"].tobytes() == mo["energy_q32"].tobytes()
    windows = [(1, 2304, 0), (0, 3072, 0), (0, 7, 3064)]
    got, m = eng.audio_batch(table, windows, dict(samples=3072, dtype="f16"), shift=[0.1, 0.2], mask=True, audio=block, sample_rate=48000)
    want, wm = AR.batch(segs, windows, 3072, F16, shift=[0.1, 0.2])
    _same(got, want)
    _same(m, wm)


def test_a_block_made_by_convert(eng):
    rng = np.random.default_rng(9)
    recs = [rng.uniform(-0.9, 0.9, n).astype(np.float32) for n in (7000, 3000)]
    data, start = eng.convert(recs, 44100)
    assert data.dtype == np.float32 and data.size >= 2 * 512
    nf = (int(start[1]) - 512) // 256 + 1
    table = [(0, 0, nf), (int(start[1]), 0, 1)]
    segs = [AR.segment(data, "f32", (o, f, n, 0, 0), 512, 256, 0.01) for o, f, n in table]
    _same(eng.moments(table, audio=data), AR.moments_records(segs))
    windows, T = [(0, segs[0].size, 0), (1, 512, 0)], (segs[0].size + 3) & ~3
    got = eng.audio_batch(table, windows, dict(samples=T, dtype="bf16"), audio=data)
    _same(got, AR.batch(segs, windows, T, BF16)[0])


def test_other_engines(eng):
    from cutter_vad_amd.engine import Engine
    rng = np.random.default_rng(10)
    with open(weights_io.packaged_blob_path(4, 16000), "rb") as f:
        v4 = Engine(f.read(), model_version=4, max_streams=16, sample_rate=16000)
    e8 = _engine(8000, max_streams=16)
    try:
        for e, frame, quads in ((v4, 512, (128, 257)), (e8, 256, (64, 65))):
            table, items, ns = _table(quads, frame, 4, "mono")
            block = _block(rng, "f32", 1, ns)
            segs = [AR.segment(block, "f32", it, frame, 4, 0.01) for it in items]
            _same(e.moments(table, hop=4, audio=block), AR.moments_records(segs))
            windows = [(1, segs[1].size, 0), (0, 4 * quads[0], 0), (1, 4, 4 * quads[1] - 4)]
            got, m = e.audio_batch(table, windows, dict(samples=1028, dtype="f16", pad="feature"), shift=[-0.25, 0.25], scale=[2.0, 0.5], mask=True, hop=4, audio=block)
            want, wm = AR.batch(segs, windows, 1028, F16, PAD_FEATURE, 0.0, [-0.25, 0.25], [2.0, 0.5])
            _same(got, want)
            _same(m, wm)
    finally:
        v4.close()
        e8.close()
