"""vad_mel_project on the GPU (csrc/mel_project.hip: vadk_mel_project) against tests/project_ref.py: byte-equal where float32 is exact
and to the header's fused-multiply-add chain, inside the derived bound (n_in + 2) u D on real operators.  Synthetic matrices, no scan,
except in the replace form's case.  The shapes are the smallest that reach every edge of the kernel, from its constants restated
here: a workgroup serves PROJ_ROWS = 64 rows, a wave a tile of 16 of them, a k-step has 4 columns of the input (the remainder is
zero-padded in LDS) and a column tile 16 of the output."""
import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests import batch_ref as B
from tests import project_ref as R
from tests.test_gpu_scan import GOLD, _engine

pytestmark = pytest.mark.gpu

PROJ_ROWS, TILE_ROWS, K_STEP, COL_TILE = 64, 16, 4, 16
ROWS = [0, 1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, PROJ_ROWS - 1, PROJ_ROWS, PROJ_ROWS + 1, 3 * PROJ_ROWS + 1]
N_IN = [1, K_STEP - 1, K_STEP, K_STEP + 1, 80, 127, 128]
N_OUT = [1, 13, COL_TILE - 1, COL_TILE, COL_TILE + 1, 128]
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000)
    yield e
    e.close()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{len(bad)} cells differ, the first at {bad[:4].tolist()}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")


def device_project(eng, d_x, x_offset_floats, rows, op, bias, guard=32):
    """vad_mel_project_device out of d_x (a float32 torch tensor) from element x_offset_floats, into sentinel-filled device memory
    -> [rows, n_out]; nothing outside the output may have been written"""
    import torch
    n_out = op.shape[1]
    d_out = torch.full((guard + rows * n_out + guard,), float(SENTINEL), dtype=torch.float32, device="cuda")
    got = eng.mel_project_device(op, bias, d_features=d_x.data_ptr() + 4 * x_offset_floats, rows=rows, d_out=d_out.data_ptr() + 4 * guard)
    eng.synchronize()
    assert got == (rows, n_out)
    host = d_out.cpu().numpy()
    assert (host[:guard] == SENTINEL).all() and (host[guard + rows * n_out:] == SENTINEL).all()
    return host[guard:guard + rows * n_out].reshape(rows, n_out)


@pytest.mark.parametrize("n_in", N_IN)
def test_integers_byte_equal_in_both_forms(eng, n_in):
    import torch
    rng = np.random.default_rng(n_in)
    for n_out in N_OUT:
        x, op, bias = R.integers(rng, max(ROWS), n_in, n_out)
        want = R.project(x, op, bias)
        assert (want.astype(np.float32).astype(np.float64) == want).all()
        want = want.astype(np.float32)
        d_x = torch.from_numpy(x).cuda()
        for rows in ROWS:
            _same(eng.mel_project(op, bias, features=x[:rows]), want[:rows])
            if rows:
                _same(device_project(eng, d_x, 0, rows, op, bias), want[:rows])
        _same(eng.mel_project(op, None, features=x), R.project(x, op).astype(np.float32))      # no bias: 0


def test_zero_rows_device_form_writes_nothing(eng):
    import torch
    x, op, bias = R.integers(np.random.default_rng(0), 4, 5, 3)
    assert device_project(eng, torch.from_numpy(x).cuda(), 0, 0, op, bias).shape == (0, 3)


@pytest.mark.parametrize("n_in,n_out", [(5, 13), (80, 13), (127, 17)])
def test_position_independence(eng, n_in, n_out):
    """the same rows at row offsets 0 .. 3 of a larger matrix - with an odd n_in a 4-byte-aligned, not 16-byte-aligned, input, and
    every row in another lane, wave and workgroup - give the same bytes row by row"""
    import torch
    rng = np.random.default_rng(100 + n_in)
    rows = 2 * PROJ_ROWS + 5
    x = R.logmel_like(rng, rows + 3, n_in)
    op = rng.normal(0, 0.3, (n_in, n_out)).astype(np.float32)
    bias = rng.normal(0, 2, n_out).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    whole = device_project(eng, d_x, 0, rows + 3, op, bias)
    _same(whole, R.fma_chain(x, op, bias))
    for off in range(4):
        _same(device_project(eng, d_x, off * n_in, rows, op, bias), whole[off:off + rows])
    _same(eng.mel_project(op, bias, features=x[3:7]), whole[3:7])                   # and on rows and the launch shape


@pytest.mark.parametrize("n_in,n_out", [(80, 13), (128, 128)])
def test_real_operators_inside_the_derived_bound(eng, n_in, n_out):
    from cutter_vad_amd import dct_operator
    rng = np.random.default_rng(200 + n_in)
    x = R.logmel_like(rng, 3 * PROJ_ROWS + 1, n_in)
    op = dct_operator(n_in, n_out)
    bias = rng.normal(0, 3, n_out).astype(np.float32)
    got = eng.mel_project(op, bias, features=x)
    ratio = R.ratio(got, x, op, bias)
    print(f"mel_project {n_in} -> {n_out} ortho DCT: worst |err| / (u D) = {ratio.max():.3f}, bound {n_in + 2}")
    assert (np.abs(got.astype(np.float64) - R.project(x, op, bias)) <= R.bound(x, op, bias)).all()
    _same(got, R.fma_chain(x, op, bias))                                           # the rule to the bit
    _same(eng.mel_project(op, bias, features=x), got)                              # two runs, the same bytes


def test_a_nan_row_leaves_every_other_row(eng):
    rng = np.random.default_rng(7)
    x = R.logmel_like(rng, PROJ_ROWS + 9, 80)
    op = rng.normal(0, 0.3, (80, 17)).astype(np.float32)
    clean = eng.mel_project(op, None, features=x)
    dirty = x.copy()
    dirty[20, 3], dirty[PROJ_ROWS + 2, 79], dirty[5, 0] = np.nan, np.inf, -np.inf
    got = eng.mel_project(op, None, features=dirty)
    others = np.setdiff1d(np.arange(x.shape[0]), [20, PROJ_ROWS + 2, 5])
    _same(got[others], clean[others])


def _keep_project_batch(e, spec, rec, hop, scan=True):
    """mel_keep behind a scan (or of the recording itself: only a V5 engine scans), the replace form, then mel_stats + mel_batch with
    deltas against batch_ref on the reference's projection"""
    from cutter_vad_amd import CepstralSpec
    op, bias = CepstralSpec(n_ceps=13, lifter=22).operator(spec.n_mels)
    bias = bias + np.float32(0.5)
    slots = e.open_streams(1)
    try:
        with e.scan_session():
            kw = {"denoise": 0.01}
            if scan:
                e.scan_segments(slots, [rec], hop=hop, denoise=0.01)
            else:
                kw["audio"] = rec.astype(np.float32) / np.float32(32768)
            off = int(e.last_scan["offsets"][0]) if scan else 0
            segs = [(off, 1, 9), (off, 0, 40), (off, 11, 1)]
            want, wstart = e.mel(segs, spec, hop=hop, **kw)
            start = e.mel_keep(segs, spec, hop=hop, **kw)
            rows = int(start[-1])
            assert start.tolist() == wstart.tolist() and e.mel_resident() == (rows, spec.n_mels, 3)
            y = R.fma_chain(want, op, bias)
            assert (np.abs(y.astype(np.float64) - R.project(want, op, bias)) <= R.bound(want, op, bias)).all()
            _same(e.mel_project(op, bias), y)                                       # with an out: the matrix stays
            assert e.mel_resident_read().tobytes() == want.tobytes()
            assert e.mel_project(op, bias, out=False) == (rows, 13) and e.mel_resident() == (rows, 13, 3)
            _same(e.mel_resident_read(), y)
            st = e.mel_stats()
            ref = B.stats(y, start)
            assert st["max"].tobytes() == ref[0].tobytes() and st["sum"].tobytes() == ref[1].tobytes() and st["sumsq"].tobytes() == ref[2].tobytes()
            win = [(1, 32, 2), (0, 17, 0), (2, 4, 0), (1, 32, 33)]
            sh = -(ref[1] / (4096.0 * np.maximum(np.diff(start), 1)[:, None])).astype(np.float32)
            got = e.mel_batch(win, dict(frames=32, deltas=2, dtype="f16"), shift=sh)
        _same(got, B.batch(y, start, win, 13, 32, 2, dtype=B.F16, shift=sh))
    finally:
        for s in slots:
            e.close_stream(int(s))


def test_replace_form_behind_a_keep_on_the_gold_recording(eng):
    from cutter_vad_amd.scan import MelSpec
    rec = np.load(GOLD + "/speech16k_i16.npz")["pcm"][16000:16000 + 40 * 256 + 512]
    _keep_project_batch(eng, MelSpec(16000, n_mels=40), rec, 256)


@pytest.mark.parametrize("kind", ["v4", "8k"])
def test_other_engines(kind):
    from cutter_vad_amd.engine import Engine
    from cutter_vad_amd.scan import MelSpec
    version, rate = (4, 16000) if kind == "v4" else (5, 8000)
    with open(weights_io.packaged_blob_path(version, rate), "rb") as f:
        e = Engine(f.read(), model_version=version, max_streams=16, sample_rate=rate)
    try:
        x, op, bias = R.integers(np.random.default_rng(11), PROJ_ROWS + 1, 5, 17)
        _same(e.mel_project(op, bias, features=x), R.project(x, op, bias).astype(np.float32))
        frame = e.frame_samples
        pcm = np.load(GOLD + "/speech16k_i16.npz")["pcm"]
        rec = pcm[16000:16000 + 40 * (frame // 2) + frame] if rate == 16000 else pcm[16000:16000 + 2 * (40 * (frame // 2) + frame):2]
        _keep_project_batch(e, MelSpec(rate, n_fft=256 if rate == 8000 else 400, hop=80 if rate == 8000 else 160, n_mels=40), np.ascontiguousarray(rec),
                            frame // 2, scan=False)
    finally:
        e.close()
