"""vad_mel_project on the host side: exports, every refusal with its message and an untouched, pre-filled output, the order of the
checks, the replace form behind a real keep with the calls that read the resident matrix, every kind of engine, host form against
device form, and the Python faces (dct_operator, CepstralSpec, Engine.mel_project, features_recordings / batch_recordings(project=))
- the real csrc/engine.cpp over the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp states the launch as the header's
fused-multiply-add chain), against tests/project_ref.py.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from cutter_vad_amd.core.exceptions import AudioProcessingError, ConfigurationError
from tests import batch_ref as B
from tests import project_ref as R
from tests import refusal_order as O
from tests.test_mel_batch_host import FILL, INV, ROOT, _cfg, _speech, eng, lib, make_engine  # noqa: F401

NEW = ["vad_mel_project", "vad_mel_project_device"]
_f32p = C.POINTER(C.c_float)


def raw_project(lib, eng, x, op, bias=None, device=False, rows=None, n_in=None, n_out=None, null_out=False, null_op=False, x_off=0, out_off=0,
                overlap=False, out_rows=None):
    """vad_mel_project (or _device) -> (rc, message, the output's bytes with 64 behind, the whole pre-filled buffer).  x = None names
    the resident matrix; x_off / out_off move the device pointers off a 64-byte boundary; overlap puts the output inside x"""
    w = None if op is None else np.ascontiguousarray(op, np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    nin = (w.shape[0] if w is not None else 1) if n_in is None else n_in
    nout = (w.shape[1] if w is not None else 1) if n_out is None else n_out
    xs = None
    if x is not None:
        xs = O.buf(max(np.asarray(x).size, 1) * 4, x_off).view(np.float32)
        xs[:np.asarray(x).size] = np.asarray(x, np.float32).reshape(-1)
    nrows = (0 if x is None else np.asarray(x).shape[0]) if rows is None else rows
    need = max(nrows if out_rows is None else out_rows, 0) * max(nout, 0) * 4
    need = need if need < (1 << 30) else 0
    whole = O.buf(need + 64, out_off)
    whole[:] = FILL
    optr = xs.ctypes.data + 4 if overlap else whole.ctypes.data
    if nrows > (1 << 30) and xs is not None and not overlap:
        optr = xs.ctypes.data + (1 << 42)                            # a claim of terabytes, refused unread: an output clear of it
    args = (eng.handle, None if xs is None else (xs.ctypes.data if device else xs.ctypes.data_as(_f32p)), nrows, nin,
            None if null_op or w is None else w.ctypes.data_as(_f32p), None if b is None else b.ctypes.data_as(_f32p), nout,
            None if null_out else (optr if device else C.cast(optr, _f32p)))
    if device:
        rc = lib.vad_mel_project_device(*args, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_mel_project(*args)
    return rc, lib.vad_last_error(eng.handle).decode(), whole[:need + 48], whole


def keep(eng, n_mels=6):
    """a real keep on the packaged speech -> (the matrix as Engine.mel returns it, start)"""
    from cutter_vad_amd.scan import MelSpec
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=n_mels)
    x = _speech(20000)
    hop = eng.frame_samples // 2
    segs = [(0, 0, 5), (eng.frame_samples * 2, 1, 9), (0, 3, 1)]
    want, wstart = eng.mel(segs, spec, hop=hop, audio=x)
    start = eng.mel_keep(segs, spec, hop=hop, audio=x)
    assert start.tolist() == wstart.tolist() and eng.mel_resident_read().tobytes() == want.tobytes()
    return want, start


def inside(got, x, op, bias=None):
    """every value inside the header's bound; -> the worst |err| / (u D)"""
    assert (np.abs(got.astype(np.float64) - R.project(x, op, bias)) <= R.bound(x, op, bias)).all()
    return float(R.ratio(got, x, op, bias).max(initial=0.0))


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    proto = lambda name: re.search(r"VAD_API\s+\w+\s+%s\((.*?)\);" % name, header, re.S).group(1)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
        assert len(proto(name).split(",")) == len(_ffi.SIGNATURES[name][1]), name
    assert "#define VAD_ABI_VERSION 5" in header
    from cutter_vad_amd import _build
    assert "mel_project.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    from cutter_vad_amd.engine import Engine
    for name in ("CepstralSpec", "dct_operator"):
        assert name in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, name)
    assert hasattr(Engine, "mel_project") and hasattr(Engine, "mel_project_device")


# ---- the value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (3, 13), (5, 17), (80, 13), (127, 15), (128, 128)])
def test_integers_are_exact_and_real_operators_inside_the_bound(lib, eng, n_in, n_out):
    rng = np.random.default_rng(1000 * n_in + n_out)
    for rows in (1, 17, 65):
        x, op, bias = R.integers(rng, rows, n_in, n_out)
        want = R.project(x, op, bias).astype(np.float32)
        assert (want.astype(np.float64) == R.project(x, op, bias)).all()
        for device in (False, True):
            rc, msg, got, _ = raw_project(lib, eng, x, op, bias, device=device)
            assert rc == 0, msg
            assert got[:want.nbytes].tobytes() == want.tobytes() and (got[want.nbytes:] == FILL).all(), (rows, device)
    x = R.logmel_like(rng, 33, n_in)
    op = rng.normal(0, 0.3, (n_in, n_out)).astype(np.float32)
    bias = rng.normal(0, 2, n_out).astype(np.float32)
    for b in (None, bias):
        rc, msg, got, _ = raw_project(lib, eng, x, op, b)
        assert rc == 0 and inside(got[:33 * n_out * 4].view(np.float32).reshape(33, n_out), x, op, b) <= n_in + 2, msg
        assert got[:33 * n_out * 4].tobytes() == R.fma_chain(x, op, b).tobytes()         # the rule to the bit: fmaf from the bias, k ascending
        rc, msg, dev, _ = raw_project(lib, eng, x, op, b, device=True, x_off=4, out_off=4)       # 4-byte aligned, no more
        assert rc == 0 and dev.tobytes() == got.tobytes(), msg


def test_zero_rows_and_the_operator_cache(lib, eng):
    rng = np.random.default_rng(2)
    x, op, bias = R.integers(rng, 5, 4, 3)
    for device in (False, True):
        rc, msg, got, whole = raw_project(lib, eng, x[:0], op, bias, device=device)
        assert rc == 0 and (whole == FILL).all(), msg
    # the same bytes neither pack nor upload again; other bytes do: a changed entry, a changed bias, NULL against zeros
    want = R.project(x, op, bias).astype(np.float32)
    for _ in range(2):
        rc, msg, got, _ = raw_project(lib, eng, x, op, bias)
        assert rc == 0 and got[:want.nbytes].tobytes() == want.tobytes(), msg
    op2 = op.copy()
    op2[3, 2] += 1
    for o, b in ((op2, bias), (op2, bias + 1), (op2, None), (op2, np.zeros(3, np.float32)), (op, bias)):
        rc, msg, got, _ = raw_project(lib, eng, x, o, b)
        assert rc == 0 and got[:want.nbytes].tobytes() == R.project(x, o, b).astype(np.float32).tobytes(), msg


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(lib, make_engine):
    eng = make_engine()                                               # an engine of its own: no resident matrix yet
    rng = np.random.default_rng(3)
    x, op, bias = R.integers(rng, 5, 4, 3)

    def refused(pattern, devices=(False, True), x=x, op=op, bias=bias, **kw):
        for device in devices:
            rc, msg, got, whole = raw_project(lib, eng, x, op, bias, device=device, **kw)
            assert rc == INV and re.search(pattern, msg), (rc, msg)
            assert msg.startswith("Model prediction failed: vad_mel_project_device: " if device else "Model prediction failed: vad_mel_project: "), msg
            assert (whole == FILL).all()

    refused("NULL names the resident matrix, and the engine holds none: no vad_scan_mel_keep has kept one", x=None)
    refused("NULL names the resident matrix, and the engine holds none", x=None, null_out=True)
    refused("rows = -1 is negative", rows=-1)
    refused("n_in = 0 must be 1 \\.\\. 128", n_in=0)
    refused("n_in = 129 must be 1 \\.\\. 128", n_in=129)
    refused("n_out = 0 must be 1 \\.\\. 128", n_out=0)
    refused("n_out = 129 must be 1 \\.\\. 128", n_out=129)
    refused("null op", null_op=True)
    bad = op.copy()
    bad[2, 1] = np.nan
    refused("op\\[2\\]\\[1\\] is NaN, an operator entry is a finite number", op=bad)
    bad[2, 1] = -np.inf
    refused("op\\[2\\]\\[1\\] is infinite", op=bad)
    refused("bias\\[2\\] is NaN, a bias is a finite number", bias=np.array([0, 0, np.nan]))
    refused("bias\\[0\\] is infinite", bias=np.array([np.inf, 0, 0]))
    refused("out = NULL replaces the resident matrix, which features = NULL names", null_out=True)
    refused("the features and the output must be 4-byte aligned", devices=(True,), x_off=2)
    refused("the features and the output must be 4-byte aligned", devices=(True,), out_off=1)
    refused("the output's 60 bytes overlap the 80 bytes of the features", devices=(True,), overlap=True)
    refused("more than 2\\^31 - 1 workgroups of 64 rows in one call", rows=(1 << 31) * 64 - 63)
    rc, msg, got, _ = raw_project(lib, eng, x, op, bias, device=True, x_off=4, out_off=12)
    assert rc == 0 and got[:60].tobytes() == R.project(x, op, bias).astype(np.float32).tobytes(), msg
    rc = lib.vad_mel_resident(eng.handle, None, None, None)
    assert rc == INV                                                  # none of this kept a matrix


def test_a_projection_with_several_faults_gets_the_first_refusal(lib, make_engine):
    """the header's order: the resident matrix, rows, n_in, n_out, op, its entries, the bias's, out == NULL with a features, the
    pointers' alignment, the overlap, the workgroups"""
    eng = make_engine()
    rng = np.random.default_rng(4)
    x, op, bias = R.integers(rng, 5, 4, 3)
    nan_op, nan_bias = op.copy(), bias.copy()
    nan_op[1, 2], nan_bias[1] = np.nan, np.inf

    def call(device, **kw):
        return raw_project(lib, eng, device=device, **kw)[0]

    # with a features: everything wrong at once but the resident matrix, which a features does not name
    faults = dict(x=x, rows=-3, n_in=0, n_out=200, op=nan_op, null_op=True, bias=nan_bias, null_out=True, x_off=2)
    steps = [(INV, "rows = -3 is negative", "rows", (1 << 31) * 64), (INV, "n_in = 0 must", "n_in", 4), (INV, "n_out = 200 must", "n_out", 3),
             (INV, "null op", "null_op", False), (INV, "op\\[1\\]\\[2\\] is NaN", "op", op), (INV, "bias\\[1\\] is infinite", "bias", bias),
             (INV, "out = NULL replaces", "null_out", False), (INV, "4-byte aligned", "x_off", 0, O.DEVICE),
             (INV, "more than 2\\^31 - 1 workgroups", "rows", None)]
    O.walk(lib, eng, call, faults, steps)
    # the overlap stands between the alignment and the workgroups
    O.walk_one(lib, eng, lambda **kw: call(True, **kw), dict(x=x, op=op, bias=bias, x_off=2, overlap=True, rows=(1 << 31) * 64),
               [(INV, "4-byte aligned", "x_off", 0), (INV, "overlap", "overlap", False), (INV, "more than 2\\^31 - 1 workgroups", "rows", None)])
    # naming the resident matrix: its absence is the first refusal, ahead of n_out, op and the bias
    O.walk_one(lib, eng, lambda **kw: call(False, **kw), dict(x=None, n_out=0, op=nan_op, bias=nan_bias, n_in=0, rows=-1),
               [(INV, "the engine holds none", "x", x), (INV, "rows = -1", "rows", None), (INV, "n_in = 0", "n_in", None), (INV, "n_out = 0", "n_out", None),
                (INV, "op\\[1\\]\\[2\\]", "op", op), (INV, "bias\\[1\\]", "bias", None)])


# ---- the replace form -------------------------------------------------------------------------------------------------
def test_replace_form_behind_a_keep(lib, eng):
    want, start = keep(eng)
    rows = int(start[-1])
    rng = np.random.default_rng(5)
    op, bias = rng.normal(0, 0.4, (6, 4)).astype(np.float32), rng.normal(0, 1, 4).astype(np.float32)
    # with an out the resident matrix is left alone: both forms, the same bytes
    y = eng.mel_project(op, bias)
    assert y.shape == (rows, 4) and y.dtype == np.float32 and inside(y, want, op, bias) <= 8
    assert eng.mel_resident() == (rows, 6, 3) and eng.mel_resident_read().tobytes() == want.tobytes()
    rc, msg, got, _ = raw_project(lib, eng, None, op, bias, device=True, out_rows=rows, n_in=77, rows=-5)     # rows and n_in are not read
    assert rc == 0 and got[:y.nbytes].tobytes() == y.tobytes() and (got[y.nbytes:] == FILL).all(), msg
    assert eng.mel_project(op, bias, features=want).tobytes() == y.tobytes()
    # a refused replace leaves the old matrix
    bad = op.copy()
    bad[0, 0] = np.nan
    with pytest.raises(AudioProcessingError, match="vad_mel_project: op\\[0\\]\\[0\\] is NaN"):
        eng.mel_project(bad, bias, out=False)
    with pytest.raises(AudioProcessingError, match="the resident matrix has 6 columns, op has n_in = 5"):
        eng.mel_project(op[:5], bias, out=False)
    rc, msg, _, _ = raw_project(lib, eng, None, op, bias, n_out=0, null_out=True)
    assert rc == INV and "n_out = 0" in msg
    assert eng.mel_resident() == (rows, 6, 3) and eng.mel_resident_read().tobytes() == want.tobytes()
    # the replace: n_mels = n_out, the starts stay, and everything that reads the resident matrix reads the projection
    assert eng.mel_project(op, bias, out=False) == (rows, 4)
    assert eng.mel_resident() == (rows, 4, 3)
    assert eng.mel_resident_read().tobytes() == y.tobytes()
    assert eng.mel_resident_read(int(start[1]), 3).tobytes() == y[start[1]:start[1] + 3].tobytes()
    st = eng.mel_stats()
    ref = B.stats(y, start)
    assert st["max"].tobytes() == ref[0].tobytes() and st["sum"].tobytes() == ref[1].tobytes() and st["sumsq"].tobytes() == ref[2].tobytes()
    grouped = eng.mel_stats(group=[0, 1, 0])
    from tests import pack_ref as P
    assert all(grouped[k].tobytes() == w.tobytes() for k, w in zip(("max", "sum", "sumsq"), P.stats_grouped(y, start, [0, 1, 0], 2)))
    win = [(1, 8, 2), (0, 4, 0), (2, 1, 0)]
    sh = -(ref[1] / (4096.0 * np.maximum(np.diff(start), 1)[:, None])).astype(np.float32)
    got = eng.mel_batch(win, dict(frames=8, deltas=2, dtype="f16"), shift=sh)
    assert got.shape == (3, 12, 8) and got.tobytes() == B.batch(y, start, win, 4, 8, 2, dtype=B.F16, shift=sh).tobytes()
    pieces = [(0, 5, 0, 0, 0), (1, 9, 0, 0, 8), (2, 1, 0, 1, 0)]
    got = eng.mel_batch_packed(pieces, 2, dict(frames=20, deltas=1))
    assert got.tobytes() == P.batch(y, start, pieces, 2, 4, 20, 1).tobytes()
    with pytest.raises(AudioProcessingError, match="n_mels = 6, the resident matrix has 4"):
        eng.mel_batch(win, dict(frames=8, n_mels=6))
    # a second projection works on the first one's result (the device form: the same swap), and the next keep replaces it
    op2 = rng.integers(-3, 4, (4, 7)).astype(np.float32)
    assert eng.mel_project_device(op2) == (rows, 7)
    eng.synchronize()
    z = eng.mel_resident_read()
    assert eng.mel_resident() == (rows, 7, 3) and inside(z, y, op2) <= 6
    again, start2 = keep(eng)
    assert eng.mel_resident() == (rows, 6, 3) and again.tobytes() == want.tobytes()
    # a keep of nothing: a matrix of no rows takes a projection
    from cutter_vad_amd.scan import MelSpec
    eng.mel_keep([], MelSpec(16000, n_fft=64, hop=32, n_mels=6), hop=256, audio=_speech(2048))
    assert eng.mel_project(op, out=False) == (0, 4) and eng.mel_resident() == (0, 4, 0) and eng.mel_project(op2[:, :2]).shape == (0, 2)


@pytest.mark.parametrize("kind", ["v4", "8k", "shared"])
def test_every_engine_is_served(lib, make_engine, kind):
    e = make_engine(**{"v4": dict(version=4), "8k": dict(rate=8000), "shared": dict(shared_gpu=True)}[kind])
    rng = np.random.default_rng(6)
    x, op, bias = R.integers(rng, 70, 5, 3)
    want = R.project(x, op, bias).astype(np.float32)
    for device in (False, True):
        rc, msg, got, _ = raw_project(lib, e, x, op, bias, device=device)
        assert rc == 0 and got[:want.nbytes].tobytes() == want.tobytes(), msg
    assert e.mel_project(op, bias, features=x).tobytes() == want.tobytes()
    if kind != "8k":
        kept, start = keep(e)
        op6 = rng.integers(-2, 3, (6, 2)).astype(np.float32)
        assert e.mel_project(op6, out=False) == (int(start[-1]), 2) and inside(e.mel_resident_read(), kept, op6) <= 8


# ---- the operators ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 1), (5, 5), (40, 13), (80, 13), (128, 128)])
def test_dct_operator(n, k):
    from cutter_vad_amd import dct_operator
    m, c = np.arange(n)[:, None], np.arange(k)[None, :]
    closed = np.cos(np.pi * c * (2 * m + 1) / (2.0 * n)) * np.where(c == 0, np.sqrt(1.0 / n), np.sqrt(2.0 / n))
    op = dct_operator(n, k)
    assert op.dtype == np.float32 and op.shape == (n, k)
    assert np.abs(op.astype(np.float64) - closed).max() <= 2.0 ** -24 * np.abs(closed).max() + 1e-15 * n
    assert np.abs(dct_operator(n, k, norm=None).astype(np.float64) - 2 * np.cos(np.pi * c * (2 * m + 1) / (2.0 * n))).max() <= 2.0 ** -23 + 1e-14 * n
    if k > 1:
        assert dct_operator(n, k - 1, first=1).tobytes() == np.ascontiguousarray(op[:, 1:]).tobytes()
    try:
        from scipy.fft import dct
    except ImportError:
        dct = None
    if dct is not None:
        eye = np.eye(n)
        assert np.abs(op - dct(eye, type=2, norm="ortho", axis=1)[:, :k]).max() <= 2.0 ** -24 + 1e-14
        assert np.abs(dct_operator(n, k, norm=None) - dct(eye, type=2, axis=1)[:, :k]).max() <= 2.0 ** -23 + 1e-13
    for bad in (dict(n_in=0, n_out=1), dict(n_in=4, n_out=5), dict(n_in=4, n_out=4, first=1), dict(n_in=4, n_out=2, norm="backward"),
                dict(n_in=4, n_out=2, first=-1)):
        with pytest.raises(ConfigurationError):
            dct_operator(**bad)


@pytest.mark.parametrize("n", [1, 2, 13, 80, 128])
def test_the_square_ortho_operator_is_orthogonal(n):
    from cutter_vad_amd.scan import _dct64
    w = _dct64(n, n, "ortho", 0)
    assert np.abs(w.T @ w - np.eye(n)).max() <= 4 * n * 2.0 ** -53        # to float64's rounding
    assert np.abs(w @ w.T - np.eye(n)).max() <= 4 * n * 2.0 ** -53


def test_cepstral_spec():
    from cutter_vad_amd import CepstralSpec, dct_operator
    from cutter_vad_amd.scan import _dct64
    op, bias = CepstralSpec().operator(80)
    assert op.tobytes() == dct_operator(80, 13).tobytes() and bias.dtype == np.float32 and bias.tolist() == [0.0] * 13
    c = np.arange(13)
    # HTK / Kaldi: 1 + 11 sin(pi c / 22), c0 untouched; librosa: the same at c + 1
    op, _ = CepstralSpec(lifter=22).operator(40)
    assert op.tobytes() == (_dct64(40, 13, "ortho", 0) * (1 + 11 * np.sin(np.pi * c / 22))[None, :]).astype(np.float32).tobytes()
    assert op[:, 0].tobytes() == dct_operator(40, 13)[:, 0].tobytes()
    op, _ = CepstralSpec(lifter=22, lifter_offset=1).operator(40)
    assert op.tobytes() == (_dct64(40, 13, "ortho", 0) * (1 + 11 * np.sin(np.pi * (c + 1) / 22))[None, :]).astype(np.float32).tobytes()
    # dropping c0 keeps each coefficient's own lifter weight; the scale is folded in before the one rounding
    op, _ = CepstralSpec(n_ceps=12, lifter=22, first=1, scale=10.0).operator(40)
    assert op.tobytes() == (_dct64(40, 12, "ortho", 1) * (10 * (1 + 11 * np.sin(np.pi * c[1:] / 22)))[None, :]).astype(np.float32).tobytes()
    assert CepstralSpec(n_ceps=20, norm=None).operator(20)[0].tobytes() == dct_operator(20, 20, norm=None).tobytes()
    for bad in (CepstralSpec(n_ceps=41), CepstralSpec(lifter=-1), CepstralSpec(scale=float("nan")), CepstralSpec(norm="x"), CepstralSpec(first=30)):
        with pytest.raises(ConfigurationError):
            bad.operator(40)


# ---- the corpus calls -------------------------------------------------------------------------------------------------
def test_features_and_batch_recordings_project(eng):
    from cutter_vad_amd import CepstralSpec, FeatureBatch, MelSpec, batch_affine, batch_recordings, features_recordings
    pcm = _speech(60000)
    recs = [pcm[:30000], np.zeros(4000, np.float32), pcm[30000:]]
    cfg = _cfg(eng.frame_samples)
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    ceps = CepstralSpec(n_ceps=4, lifter=22, scale=10.0)
    op, bias = ceps.operator(6)
    plain = features_recordings(recs, spec, cfg, engine=eng)
    # project=None takes today's path and returns today's bytes
    none = features_recordings(recs, spec, cfg, engine=eng, project=None)
    assert [[(a, b, f.tobytes()) for a, b, f in one] for one in none] == [[(a, b, f.tobytes()) for a, b, f in one] for one in plain]
    fb = FeatureBatch(frames=32, stride=24, norm="cmvn", deltas=1, pad="feature", pad_value=-10.0)
    b0, i0 = batch_recordings(recs, spec, fb, cfg, engine=eng)
    b1, i1 = batch_recordings(recs, spec, fb, cfg, engine=eng, project=None)
    assert b0.tobytes() == b1.tobytes() and i0 == i1
    # keep + the projection + the existing calls
    segs = [(i, a, b, f) for i, one in enumerate(plain) for a, b, f in one]
    assert len(segs) >= 3 and not plain[1]
    x = np.concatenate([f for *_, f in segs])
    start = np.concatenate([[0], np.cumsum([f.shape[0] for *_, f in segs])])
    y = eng.mel_project(op, bias, features=x)
    assert inside(y, x, op, bias) <= 8
    for project in (ceps, (op, bias), (op, None)):
        got = features_recordings(recs, spec, cfg, engine=eng, project=project)
        flat = [(i, a, b, f) for i, one in enumerate(got) for a, b, f in one]
        assert [s[:3] for s in flat] == [s[:3] for s in segs] and not got[1]
        assert np.concatenate([f for *_, f in flat]).tobytes() == y.tobytes() and all(f.shape[1] == 4 for *_, f in flat)
    got, index = batch_recordings(recs, spec, fb, cfg, engine=eng, project=ceps)
    lo, sh, sc = batch_affine(dict(zip(("max", "sum", "sumsq"), B.stats(y, start))), start, "cmvn")
    win = [(k, min(32, f.shape[0] - r), r) for k, (*_, f) in enumerate(segs) for r in range(0, f.shape[0], 24)]
    want = B.batch(y, start, win, 4, 32, 1, pad_mode=B.PAD_FEATURE, pad_value=-10.0, lo=lo, shift=sh, scale=sc)
    assert got.shape == want.shape == (len(win), 8, 32) and got.tobytes() == want.tobytes() and index == i0
    from tests import pack_ref as P
    saved, _ffi._lib = _ffi._lib, eng._lib
    try:
        packed, pindex = batch_recordings(recs, spec, FeatureBatch(frames=64, pack=True, dtype="bf16"), cfg, engine=eng, project=(op, bias))
    finally:
        _ffi._lib = saved
    pieces, nw = P.plan(start, 64, 0, [i for i, *_ in segs])
    assert packed.tobytes() == P.batch(y, start, pieces, nw, 4, 64, 0, dtype=B.BF16).tobytes() and len(pindex) == len(pieces)
    # no speech, no recordings: the empty batch has the projected width
    mono = np.zeros(4000, np.float32)
    assert batch_recordings([mono], spec, FeatureBatch(frames=8, deltas=2), cfg, engine=eng, project=ceps)[0].shape == (0, 12, 8)
    assert batch_recordings([], spec, FeatureBatch(frames=8), cfg, engine=eng, project=ceps)[0].shape == (0, 4, 8)
    assert features_recordings([mono], spec, cfg, engine=eng, project=ceps) == [[]]

    class NoProject:
        sample_rate, frame_samples = 16000, 512
        mel = mel_batch = mel_keep = None

    for call in (lambda **kw: features_recordings([mono], spec, cfg, **kw), lambda **kw: batch_recordings([mono], spec, fb, cfg, **kw)):
        with pytest.raises(ConfigurationError, match="project= needs an engine with mel_keep and mel_project"):
            call(engine=NoProject(), project=ceps)
        with pytest.raises(ConfigurationError, match="project's operator is \\[n_mels = 6, 1 \\.\\. 128\\], got \\(5, 4\\)"):
            call(engine=eng, project=(op[:5], None))
