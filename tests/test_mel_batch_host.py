"""vad_scan_mel_keep, vad_mel_stats and vad_mel_batch on the host side: exports, every refusal with its message and an untouched,
pre-filled output, n == 0 and nw == 0, every kind of engine, the resident matrix against Engine.mel's bytes on both paths, host
form against device form, and the Python faces (batch_windows, batch_affine, batch_recordings) - the real csrc/engine.cpp over
the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp states both launches in plain loops), byte for byte against
tests/batch_ref.py.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import AudioProcessingError, ConfigurationError
from tests import batch_ref as B
from tests import standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_mel_keep", "vad_scan_mel_keep_device", "vad_mel_resident", "vad_mel_resident_read", "vad_mel_stats", "vad_mel_stats_device",
       "vad_mel_batch", "vad_mel_batch_device"]
INV = _ffi.VAD_ERR_INVALID_ARG
FILL = 0xA5
_f32p, _i64p, _u64p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    handle = C.CDLL(standin.build(tmp_path_factory.mktemp("standin")))
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


@pytest.fixture(scope="module")
def make_engine(lib):
    from cutter_vad_amd.engine import Engine
    made = []

    def make(version=5, rate=16000, max_streams=128, shared_gpu=False):
        with open(weights_io.packaged_blob_path(version, rate), "rb") as f:
            blob = f.read()
        saved = _ffi._lib
        _ffi._lib = lib
        try:
            e = Engine(blob, model_version=version, max_streams=max_streams, sample_rate=rate, shared_gpu=shared_gpu)
        finally:
            _ffi._lib = saved
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


@pytest.fixture(scope="module")
def eng(make_engine):
    return make_engine()


# ---- shared cases (tests/test_gpu_mel_batch.py runs the same ones on the GPU) ------------------------------------------------
def matrix(rng, seg_rows, n_mels, lo=-12.0, hi=4.0):
    """a feature matrix with the listed rows per segment -> (x float32 [rows, n_mels], start int64 [n + 1])"""
    start = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int64)
    x = rng.uniform(lo, hi, (int(start[-1]), n_mels)).astype(np.float32)
    return x, start


def special_values(x):
    """values the statistics and the conversions have to get right, written over the first entries of x (in place)"""
    v = [2048.0, -2048.0, 2048.5, -3000.0, 1e30, -1e30,                     # the clamp
         0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.5 / 4096, -1.5 / 4096,     # ties of rint: to even
         -0.0, 0.0,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11),             # ties of float16
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8),           # ties of bfloat16
         65519.0, 65520.0, 70000.0, -70000.0, 2.0 ** -25, 3 * 2.0 ** -26]    # float16: the last finite, overflow, the subnormals' tie
    flat = x.reshape(-1)
    k = min(len(v), flat.size)
    flat[:k] = np.asarray(v[:k], np.float32)
    return x


def batch_struct(n_mels, frames, deltas=0, layout=B.CHANNEL, dtype=B.F32, pad_mode=B.PAD_VALUE, pad_value=0.0, reserved=0):
    return _ffi.Batch(n_mels, frames, deltas, layout, dtype, pad_mode, pad_value, reserved)


def window_array(windows):
    return np.array([tuple(map(int, w)) for w in windows], _ffi.BATCH_WINDOW_DTYPE).reshape(-1)


def np_dtype(dtype):
    return {B.F32: np.float32, B.F16: np.float16}.get(dtype, np.uint16)


def raw_stats(lib, eng, x, start, want=(True, True, True), device=False, rows=None, n_mels=None, n=None):
    """vad_mel_stats (or _device) -> (rc, message, max, sum, sumsq); the outputs are pre-filled with FILL bytes"""
    nm = (x.shape[1] if x is not None else 1) if n_mels is None else n_mels
    nn = (len(start) - 1 if start is not None else 4) if n is None else n
    mx = np.full(max(nn, 1), FILL, np.uint8).repeat(4).view(np.float32)
    s = np.full(max(nn, 1) * max(nm, 1) * 8, FILL, np.uint8).view(np.int64)
    s2 = np.full(max(nn, 1) * max(nm, 1) * 8, FILL, np.uint8).view(np.uint64)
    xs = None if x is None else np.ascontiguousarray(x, np.float32)
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    head = (eng.handle, None if xs is None else (xs.ctypes.data if device else xs.ctypes.data_as(_f32p)),
            (0 if xs is None else xs.shape[0]) if rows is None else rows, nm, None if st is None else st.ctypes.data_as(_i64p), nn)
    if device:
        rc = lib.vad_mel_stats_device(*head, mx.ctypes.data if want[0] else None, s.ctypes.data if want[1] else None,
                                      s2.ctypes.data if want[2] else None, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_mel_stats(*head, mx.ctypes.data_as(_f32p) if want[0] else None, s.ctypes.data_as(_i64p) if want[1] else None,
                               s2.ctypes.data_as(_u64p) if want[2] else None)
    return rc, lib.vad_last_error(eng.handle).decode(), mx, s, s2


def raw_batch(lib, eng, x, start, b, windows, lo=None, shift=None, scale=None, nss=1, device=False, out_bytes=None, rows=None, n=None,
              null_out=False, misalign=0):
    """vad_mel_batch (or _device) -> (rc, message, out as bytes with 64 bytes of room behind); pre-filled with FILL"""
    w = window_array(windows)
    elt = 4 if b is None or b.dtype == B.F32 else 2
    need = 0 if b is None else len(w) * b.n_mels * (b.deltas + 1) * b.frames * elt
    out = np.full(max(need, 0) + 64 + 16, FILL, np.uint8)
    base = out.ctypes.data + (-out.ctypes.data) % 16 + misalign
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (lo, shift, scale)]
    xs = None if x is None else np.ascontiguousarray(x, np.float32)
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    wp = (w if w.size else np.zeros(1, _ffi.BATCH_WINDOW_DTYPE)).ctypes.data_as(C.POINTER(_ffi.BatchWindow))
    args = (eng.handle, None if xs is None else (xs.ctypes.data if device else xs.ctypes.data_as(_f32p)),
            (0 if xs is None else xs.shape[0]) if rows is None else rows, None if st is None else st.ctypes.data_as(_i64p),
            (0 if st is None else st.size - 1) if n is None else n, None if b is None else C.byref(b), wp, len(w),
            *[None if a is None else a.ctypes.data_as(_f32p) for a in keep], nss, None if null_out else base, need if out_bytes is None else out_bytes)
    if device:
        rc = lib.vad_mel_batch_device(*args, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_mel_batch(*args)
    off = base - out.ctypes.data
    return rc, lib.vad_last_error(eng.handle).decode(), out[off:off + need + 48], out


def same(got_bytes, want):
    return got_bytes[:want.nbytes].tobytes() == want.tobytes() and bool((got_bytes[want.nbytes:] == FILL).all())


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header
    m = re.search(r"typedef struct vad_batch \{(.*?)\} vad_batch;", header, re.S)
    got = re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))
    assert [g[1] for g in got] == [f[0] for f in _ffi.Batch._fields_] == ["n_mels", "frames", "deltas", "layout", "dtype", "pad_mode", "pad_value",
                                                                           "reserved"]
    assert [g[0] for g in got] == ["int32_t"] * 6 + ["float", "int32_t"] and C.sizeof(_ffi.Batch) == 32
    m = re.search(r"typedef struct vad_batch_window \{(.*?)\} vad_batch_window;", header, re.S)
    assert re.findall(r"(int32_t|int64_t)\s+(\w+);", m.group(1)) == [("int32_t", "seg"), ("int32_t", "nrows"), ("int64_t", "row0")]
    assert C.sizeof(_ffi.BatchWindow) == 16 == _ffi.BATCH_WINDOW_DTYPE.itemsize
    for name, v in (("VAD_BATCH_F32", 0), ("VAD_BATCH_F16", 1), ("VAD_BATCH_BF16", 2), ("VAD_BATCH_CHANNEL_MAJOR", 0), ("VAD_BATCH_TIME_MAJOR", 1),
                    ("VAD_BATCH_PAD_VALUE", 0), ("VAD_BATCH_PAD_FEATURE", 1)):
        assert re.search(r"\b%s = %d\b" % (name, v), header) and getattr(_ffi, name) == v
    assert "#define VAD_STATS_MAX_ROWS 131072" in header and _ffi.VAD_STATS_MAX_ROWS == 1 << 17
    proto = lambda name: re.search(r"VAD_API\s+\w+\s+%s\((.*?)\);" % name, header, re.S).group(1)
    for name in NEW:
        assert len(proto(name).split(",")) == len(_ffi.SIGNATURES[name][1]), name
    from cutter_vad_amd import _build
    assert "mel_batch.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    for name in ("FeatureBatch", "batch_windows", "batch_affine", "batch_recordings"):
        assert name in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, name)


# ---- statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [1, 5, 80, 128])
def test_stats_byte_for_byte(lib, eng, n_mels):
    rng = np.random.default_rng(n_mels)
    x, start = matrix(rng, [0, 1, 63, 64, 65, 300, 0], n_mels, -2100.0, 2100.0)
    special_values(x[1:])
    want = B.stats(x, start)
    for device in (False, True):
        rc, msg, mx, s, s2 = raw_stats(lib, eng, x, start, device=device)
        assert rc == 0, msg
        assert mx.tobytes() == want[0].tobytes() and s.tobytes() == want[1].tobytes() and s2.tobytes() == want[2].tobytes()
        assert mx[0] == -np.inf and mx[6] == -np.inf and not s[:n_mels].any()
        for skip in range(3):                                   # each output NULL in turn: skipped, the others as before
            flags = tuple(k != skip for k in range(3))
            rc, msg, *outs = raw_stats(lib, eng, x, start, want=flags, device=device)
            assert rc == 0, msg
            for k in range(3):
                if flags[k]:
                    assert outs[k].tobytes() == want[k].tobytes()
                else:
                    assert (outs[k].view(np.uint8) == FILL).all()


def test_stats_order_of_the_zeros_and_the_clamp(lib, eng):
    x = np.array([[-0.0], [-0.0], [-0.0], [0.0], [-1.0], [-2.0], [3000.0], [-3000.0]], np.float32)
    start = np.array([0, 2, 4, 6, 8], np.int64)
    rc, msg, mx, s, s2 = raw_stats(lib, eng, x, start)
    assert rc == 0, msg
    assert mx.view(np.uint32).tolist() == [0x80000000, 0, 0xbf800000, np.float32(3000).view(np.uint32)]
    assert s.tolist() == [0, 0, -3 * 4096, 0] and s2.tolist() == [0, 0, 5 << 24, 2 << 46]
    assert mx.tobytes() == B.stats(x, start)[0].tobytes()


def test_stats_refusals(lib, eng):
    rng = np.random.default_rng(2)
    x, start = matrix(rng, [3, 4], 5)

    def refused(pattern, **kw):
        for device in (False, True):
            args = dict(x=x, start=start, device=device)
            args.update(kw)
            rc, msg, *outs = raw_stats(lib, eng, **args)
            assert rc == INV and re.search(pattern, msg), (rc, msg)
            assert msg.startswith("Model prediction failed: vad_mel_stats"), msg
            assert all((o.view(np.uint8) == FILL).all() for o in outs)

    refused("rows = -1 is negative", rows=-1)
    refused("n_mels = 0 must be 1 .. 128", n_mels=0)
    refused("n_mels = 129 must be 1 .. 128", n_mels=129)
    refused("n = -1 is negative", n=-1)
    refused("leaves the matrix of 6 rows", rows=6)
    refused("start\\[0\\] = -1", start=np.array([-1, 3, 7]))
    refused("segment 1: start = 5 is followed by 4", start=np.array([0, 5, 4, 7]))
    long = np.array([0, 3, 3 + (1 << 17) + 1], np.int64)
    refused("segment 1 has 131073 rows, the sums take 131072", start=long, rows=1 << 20)
    # ... the maximum alone takes it (the stand-in would read the rows: one row less on a real matrix is enough here)
    rc, msg, mx, s, s2 = raw_stats(lib, eng, x, start, n=0)
    assert rc == 0 and all((o.view(np.uint8) == FILL).all() for o in (mx, s, s2)), msg


def test_stats_without_a_resident_matrix(lib, make_engine):
    e = make_engine()
    x, start = matrix(np.random.default_rng(3), [3], 4)
    for kw in (dict(x=None, start=start, n_mels=4), dict(x=x, start=None)):
        rc, msg, *outs = raw_stats(lib, e, **{"x": x, "start": start, **kw})
        assert rc == INV and "holds none: no vad_scan_mel_keep has kept one" in msg, msg
    rows, nm, ns = C.c_int64(), C.c_int32(), C.c_int64()
    assert lib.vad_mel_resident(e.handle, C.byref(rows), C.byref(nm), C.byref(ns)) == INV
    assert "holds no resident matrix" in lib.vad_last_error(e.handle).decode()
    assert lib.vad_mel_resident_read(e.handle, 0, 0, None) == INV


# ---- batches ----------------------------------------------------------------------------------------------------------
SEGS = [1, 2, 3, 4, 5, 9, 0, 150]


def batch_cases(rng, n_mels, T):
    """(x, start, windows): windows of 0, 1, T - 1 and T rows where the segments allow, at a segment's start, middle and end, the
    same rows twice, in reverse order, one starting at row 2 of the long segment"""
    x, start = matrix(rng, SEGS, n_mels)
    special_values(x[int(start[7]):])
    win = []
    for seg, M in enumerate(SEGS):
        for nrows in sorted({0, 1, T - 1, T}):
            if nrows > M:
                continue
            for row0 in sorted({0, (M - nrows) // 2, M - nrows}):
                win.append((seg, nrows, row0))
    win += [(7, min(T, 64), 2), (7, min(T, 64), 2), (7, min(T, 148), 2), (6, 0, 0), (5, 4, 5)]
    return x, start, win[::-1]


@pytest.mark.parametrize("T", [4, 64, 68])
@pytest.mark.parametrize("deltas", [0, 1, 2])
def test_batch_byte_for_byte(lib, eng, T, deltas):
    rng = np.random.default_rng(10 * T + deltas)
    for n_mels in (5, 128) if T == 68 else (5,):
        x, start, win = batch_cases(rng, n_mels, T)
        n = len(start) - 1
        lo_some = np.sort(x, axis=None)[[x.size // 3] * n].astype(np.float32)          # a finite lo that IS a feature value
        sh1, sc1 = rng.uniform(-2, 2, (1, n_mels)).astype(np.float32), rng.uniform(0.1, 3, (1, n_mels)).astype(np.float32)
        shn, scn = rng.uniform(-2, 2, (n, n_mels)).astype(np.float32), rng.uniform(0.1, 3, (n, n_mels)).astype(np.float32)
        for layout in (B.CHANNEL, B.TIME):
            for dtype in (B.F32, B.F16, B.BF16):
                for pad_mode, (lo, sh, sc, nss) in ((B.PAD_VALUE, (None, None, None, 1)), (B.PAD_FEATURE, (lo_some, shn, scn, n)),
                                                    (B.PAD_FEATURE, (None, sh1, sc1, 1))):
                    b = batch_struct(n_mels, T, deltas, layout, dtype, pad_mode, -10.0)
                    want = B.batch(x, start, win, n_mels, T, deltas, layout, dtype, pad_mode, -10.0, lo, sh, sc)
                    assert want.shape == ((len(win), n_mels * (deltas + 1), T) if layout == B.CHANNEL else (len(win), T, n_mels * (deltas + 1)))
                    for device in (False, True):
                        rc, msg, got, _ = raw_batch(lib, eng, x, start, b, win, lo, sh, sc, nss, device=device)
                        assert rc == 0, msg
                        assert same(got, want), (n_mels, T, deltas, layout, dtype, pad_mode, device)


def test_batch_rule_is_add_then_multiply(lib, eng):
    """values where fmaf(x, scale, shift * scale) differs from (x + shift) * scale: a refactored formula is a wrong byte"""
    rng = np.random.default_rng(5)
    x, start = matrix(rng, [64], 8, -1.0, 1.0)
    sh, sc = rng.uniform(0.5, 1.5, (1, 8)).astype(np.float32), rng.uniform(0.5, 3, (1, 8)).astype(np.float32)
    want = B.batch(x, start, [(0, 64, 0)], 8, 64, shift=sh, scale=sc)
    fused = (x.astype(np.float64) * sc.astype(np.float64) + (sh * sc).astype(np.float64)).astype(np.float32).T[None]
    assert (fused != want).sum() > 50
    rc, msg, got, _ = raw_batch(lib, eng, x, start, batch_struct(8, 64), [(0, 64, 0)], None, sh, sc, 1)
    assert rc == 0 and same(got, want), msg


def test_batch_refusals(lib, eng):
    rng = np.random.default_rng(6)
    x, start = matrix(rng, [5, 9], 5)
    ok = [(0, 4, 1), (1, 8, 0)]
    good = dict(x=x, start=start, b=batch_struct(5, 8), windows=ok)

    def refused(pattern, devices=(False, True), **kw):
        for device in devices:
            rc, msg, got, whole = raw_batch(lib, eng, **{**good, **kw}, device=device)
            assert rc == INV and re.search(pattern, msg), (rc, msg)
            assert msg.startswith("Model prediction failed: vad_mel_batch"), msg
            assert (whole == FILL).all()

    rc, msg, got, _ = raw_batch(lib, eng, **good)
    assert rc == 0 and same(got, B.batch(x, start, ok, 5, 8)), msg
    refused("null vad_batch", b=None)
    for f, pat in ((dict(n_mels=0), "n_mels = 0 must be 1 .. 128"), (dict(n_mels=129), "n_mels = 129"), (dict(frames=0), "frames = 0 must be a multiple of 4"),
                   (dict(frames=6), "frames = 6"), (dict(frames=65540), "frames = 65540"), (dict(deltas=-1), "deltas = -1 must be 0 .. 2"),
                   (dict(deltas=3), "deltas = 3"), (dict(layout=2), "layout = 2 is neither"), (dict(dtype=3), "dtype = 3 is none of"),
                   (dict(pad_mode=2), "pad_mode = 2 is neither"), (dict(pad_value=float("nan")), "pad_value is NaN"),
                   (dict(pad_value=float("inf")), "pad_value is infinite"), (dict(reserved=1), "reserved = 1 must be 0")):
        refused(pat, b=batch_struct(**{**dict(n_mels=5, frames=8), **f}))
    refused("window 1 names segment 2 of 2", windows=[(0, 4, 1), (2, 1, 0)])
    refused("window 0 names segment -1", windows=[(-1, 1, 0)])
    refused("window 1: rows 0 \\.\\. \\+9 of segment 1, which has 9, in 8 frames", windows=[(0, 4, 1), (1, 9, 0)])
    refused("window 0: rows 2 \\.\\. \\+4 of segment 0, which has 5", windows=[(0, 4, 2)])
    refused("window 0: rows -1", windows=[(0, 1, -1)])
    refused("window 0: rows 0 \\.\\. \\+-1", windows=[(0, -1, 0)])
    refused("nss = 3: shift and scale have 1 row or n = 2", shift=np.zeros((3, 5)), nss=3)
    refused("shift\\[1\\]\\[2\\] is NaN", shift=np.array([[0] * 5, [0, 0, np.nan, 0, 0]]), nss=2)
    refused("scale\\[0\\]\\[4\\] is infinite", scale=np.array([[1, 1, 1, 1, np.inf]]), nss=1)
    refused("lo\\[1\\] is NaN", lo=np.array([0, np.nan]))
    refused("out_bytes = 319, the windows have 320 bytes", out_bytes=319)
    refused("null buffer", null_out=True)
    refused("the output must be 16-byte aligned", devices=(True,), misalign=4)
    refused("leaves the matrix of 13 rows", rows=13)
    # lo = -inf and +inf are values, not refusals
    rc, msg, got, _ = raw_batch(lib, eng, **good, lo=np.array([-np.inf, np.inf]))
    assert rc == 0 and same(got, B.batch(x, start, ok, 5, 8, lo=[-np.inf, np.inf])), msg


def test_batch_of_nothing(lib, eng):
    x, start = matrix(np.random.default_rng(7), [5], 5)
    rc, msg, got, whole = raw_batch(lib, eng, x, start, batch_struct(5, 8), [])
    assert rc == 0 and (whole == FILL).all(), msg
    rc, msg, got, whole = raw_batch(lib, eng, x, start, batch_struct(5, 8), [], null_out=True, out_bytes=0)
    assert rc == 0, msg
    rc, msg, got, whole = raw_batch(lib, eng, np.zeros((0, 5), np.float32), np.array([0]), batch_struct(5, 8), [])      # n == 0
    assert rc == 0, msg
    rc, msg, got, whole = raw_batch(lib, eng, np.zeros((0, 5), np.float32), np.array([0]), batch_struct(5, 8), [(0, 0, 0)])
    assert rc == INV and "names segment 0 of 0" in msg


@pytest.mark.parametrize("kind", ["v4", "8k", "shared"])
def test_every_engine_is_served(lib, make_engine, kind):
    e = make_engine(**{"v4": dict(version=4), "8k": dict(rate=8000), "shared": dict(shared_gpu=True)}[kind])
    rng = np.random.default_rng(8)
    x, start, win = batch_cases(rng, 5, 8)
    rc, msg, mx, s, s2 = raw_stats(lib, e, x, start)
    want = B.stats(x, start)
    assert rc == 0 and mx.tobytes() == want[0].tobytes() and s.tobytes() == want[1].tobytes() and s2.tobytes() == want[2].tobytes(), msg
    rc, msg, got, _ = raw_batch(lib, e, x, start, batch_struct(5, 8, 2, dtype=B.F16), win)
    assert rc == 0 and same(got, B.batch(x, start, win, 5, 8, 2, dtype=B.F16)), msg


# ---- the resident matrix ---------------------------------------------------------------------------------------------
def _speech(n=40000):
    return np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"][16000:16000 + n].astype(np.float32) / np.float32(32768)


@pytest.mark.parametrize("rate", [None, 48000])
def test_keep_is_mel_left_on_the_gpu(eng, rate):
    from cutter_vad_amd.scan import MelSpec
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    x = _speech(12000 if rate is None else 36000)
    chunk = eng.scan_chunk_samples(rate)
    hop = chunk // 2
    segs = [(0, 0, 5), (chunk * 2, 1, 9), (0, 3, 1)]
    kw = {"audio": x} if rate is None else {"audio": x, "sample_rate": rate}
    want, wstart = eng.mel(segs, spec, hop=hop, **kw)
    start = eng.mel_keep(segs, spec, hop=hop, **kw)
    assert start.tolist() == wstart.tolist() and eng.mel_resident() == (int(start[-1]), 6, 3)
    assert eng.mel_resident_read().tobytes() == want.tobytes()
    assert eng.mel_resident_read(int(start[1]), 3).tobytes() == want[start[1]:start[1] + 3].tobytes()
    # the matrix survives a cut and is read by the calls that name it with None
    again = eng.mel_keep(segs[:2], spec, hop=hop, **kw)
    assert again.tolist() == wstart[:3].tolist() and eng.mel_resident_read().tobytes() == want[:wstart[2]].tobytes()
    eng.cut(segs, hop=hop, layout="range", out="f32", **kw)
    assert eng.mel_resident_read().tobytes() == want[:wstart[2]].tobytes()
    st = eng.mel_stats()
    ref = B.stats(want[:wstart[2]], wstart[:3])
    assert st["max"].tobytes() == ref[0].tobytes() and st["sum"].tobytes() == ref[1].tobytes() and st["sumsq"].tobytes() == ref[2].tobytes()
    assert set(eng.mel_stats(moments=False)) == {"max"}
    win = [(1, 8, 2), (0, 4, 0)]
    got = eng.mel_batch(win, dict(frames=8, deltas=1, dtype="bf16"), lo=st["max"] - np.float32(8), shift=4.0, scale=0.25)
    assert got.dtype == np.uint16 and got.tobytes() == B.batch(want, wstart[:3], win, 6, 8, 1, dtype=B.BF16, lo=ref[0] - np.float32(8),
                                                              shift=np.full(6, 4, np.float32), scale=np.full(6, 0.25, np.float32)).tobytes()
    with pytest.raises(AudioProcessingError, match="n_mels = 5, the resident matrix has 6"):
        eng.mel_batch(win, dict(frames=8, n_mels=5))
    with pytest.raises(AudioProcessingError, match="rows %d .. \\+1 of a matrix of %d" % (wstart[2], wstart[2])):
        eng.mel_resident_read(int(wstart[2]), 1)
    # a refused keep leaves the matrix; the next keep replaces it; a keep of nothing keeps a matrix of no rows
    with pytest.raises(AudioProcessingError, match="vad_scan_mel_keep: segment 0: first_frame = -1"):
        eng.mel_keep([(0, -1, 3)], spec, hop=hop, **kw)
    assert eng.mel_resident_read().tobytes() == want[:wstart[2]].tobytes()
    eng.mel_keep(segs[2:], spec, hop=hop, **kw)
    assert eng.mel_resident_read().tobytes() == want[wstart[2]:].tobytes()
    assert eng.mel_keep([], spec, hop=hop, **kw).tolist() == [0] and eng.mel_resident() == (0, 6, 0)


def test_keep_device_form_and_its_refusals(lib, eng):
    from cutter_vad_amd.scan import MelSpec
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    m, a, b, w = eng._mel_arrays(spec)
    x = _speech(6000)
    segs = [(0, 1, 4), (1024, 0, 2)]
    want, wstart = eng.mel(segs, spec, hop=256, audio=x, denoise=None)
    items = (_ffi.CutItem * 2)(*[_ffi.CutItem(s[0], s[1], s[2], 0, 0, 0) for s in segs])
    rows = C.c_int64(-1)
    ops = [v.ctypes.data_as(_f32p) for v in (a, b, w)]
    rc = lib.vad_scan_mel_keep_device(eng.handle, items, 2, C.byref(m), *ops, None, 0, x.ctypes.data, x.size, 1, 0, 0, 256, -1.0, C.byref(rows), None)
    assert rc == 0 and rows.value == wstart[-1], lib.vad_last_error(eng.handle)
    assert eng.mel_resident_read().tobytes() == want.tobytes()
    rc = lib.vad_scan_mel_keep_device(eng.handle, items, 2, C.byref(m), *ops, None, 0, None, x.size, 1, 0, 0, 256, -1.0, C.byref(rows), None)
    assert rc == INV and "vad_scan_mel_keep_device: null buffer" in lib.vad_last_error(eng.handle).decode()
    rc = lib.vad_scan_mel_keep(eng.handle, items, 2, C.byref(m), *ops, None, 0, x.ctypes.data, x.size, 1, 0, 48000, 768, -1.0, None)
    assert rc == INV and "vad_scan_mel_keep: null taps" in lib.vad_last_error(eng.handle).decode()
    rc = lib.vad_scan_mel_keep(eng.handle, items, 2, C.byref(m), *ops, None, 0, x.ctypes.data, x.size, 1, 0, 44100, 768, -1.0, None)
    assert rc == _ffi.VAD_ERR_UNSUPPORTED and "supported input rates are 8000, 24000, 48000" in lib.vad_last_error(eng.handle).decode()
    assert eng.mel_resident_read().tobytes() == want.tobytes()


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_batch_windows():
    from cutter_vad_amd import batch_windows
    start = [0, 5, 5, 17, 18]
    w, T = batch_windows(start, 8)
    assert T == 8 and w.tolist() == [(0, 5, 0), (2, 8, 0), (2, 4, 8), (3, 1, 0)]
    w, T = batch_windows(start, 8, 4)
    assert T == 8 and w.tolist() == [(0, 5, 0), (0, 1, 4), (2, 8, 0), (2, 8, 4), (2, 4, 8), (3, 1, 0)]
    w, T = batch_windows(start)
    assert T == 12 and w.tolist() == [(0, 5, 0), (1, 0, 0), (2, 12, 0), (3, 1, 0)]
    assert batch_windows([0, 0])[1] == 4 and batch_windows([0])[0].size == 0 and batch_windows([0], 8)[0].size == 0
    for bad in (dict(frames=6), dict(frames=0), dict(frames=8, stride=0), dict(frames=65540)):
        with pytest.raises(ConfigurationError):
            batch_windows(start, **bad)
    with pytest.raises(ConfigurationError):
        batch_windows([0, 5, 4])
    with pytest.raises(ConfigurationError, match="give frames"):
        batch_windows([0, 70000])


def test_batch_affine():
    from cutter_vad_amd import batch_affine
    rng = np.random.default_rng(11)
    x, start = matrix(rng, [7, 0, 300], 5)
    mx, s, s2 = B.stats(x, start)
    st = {"max": mx, "sum": s, "sumsq": s2}
    assert batch_affine(None, start, "none") == (None, None, None)
    lo, sh, sc = batch_affine(st, start, "whisper")
    assert lo.dtype == np.float32 and lo.tobytes() == (mx - np.float32(8)).tobytes() and lo[1] == -np.inf and (sh, sc) == (4.0, 0.25)
    lo, sh, sc = batch_affine(st, start, "cmn")
    q = B.q_of(x).astype(np.float64) / 4096
    assert lo is None and sc is None and sh.dtype == np.float32 and sh.shape == (3, 5)
    assert sh[0].tobytes() == (-q[:7].mean(axis=0)).astype(np.float32).tobytes() or np.abs(sh[0] + q[:7].mean(axis=0)).max() < 1e-6
    assert not sh[1].any()
    lo, sh2, sc = batch_affine(st, start, "cmvn", eps=1e-5)
    assert sh2.tobytes() == sh.tobytes() and (sc[1] == 1).all()
    assert np.abs(sc[2] * q[7:].std(axis=0) - 1).max() < 1e-5
    const = {"max": np.zeros(1, np.float32), "sum": np.full((1, 2), 3 * 4096 * 4), "sumsq": np.full((1, 2), 9 * (1 << 24) * 4, np.uint64)}
    assert batch_affine(const, [0, 4], "cmvn", eps=0.5)[2].tolist() == [[2.0, 2.0]]      # no deviation: 1 / eps
    with pytest.raises(ConfigurationError):
        batch_affine(st, start, "l2")


def _cfg(frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.05, vad_end_probability=0.05, voice_start_frame_count=2,
                     voice_end_frame_count=3, **kw)


@pytest.mark.parametrize("norm", ["whisper", "cmn", "cmvn"])
def test_batch_recordings_on_speech(eng, norm):
    """against features_recordings and tests/batch_ref.py on the packaged speech (the stand-in's model is |first sample of a frame|)"""
    from cutter_vad_amd import FeatureBatch, MelSpec, batch_affine, batch_recordings, features_recordings
    pcm = _speech(60000)
    recs = [pcm[:30000], np.zeros(4000, np.float32), pcm[30000:]]
    cfg = _cfg(eng.frame_samples)
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    fb = FeatureBatch(frames=32, stride=24, norm=norm, deltas=1 if norm == "cmvn" else 0, dtype="f16" if norm == "whisper" else "f32",
                      layout="time" if norm == "cmn" else "channel", pad="feature", pad_value=-10.0)
    got, index = batch_recordings(recs, spec, fb, cfg, engine=eng)
    feats = features_recordings(recs, spec, cfg, engine=eng)
    segs = [(i, a, b, f) for i, one in enumerate(feats) for a, b, f in one]
    assert len(segs) >= 3 and not feats[1]
    x = np.concatenate([f for *_, f in segs])
    start = np.concatenate([[0], np.cumsum([f.shape[0] for *_, f in segs])])
    mx, s, s2 = B.stats(x, start)
    lo, sh, sc = batch_affine({"max": mx, "sum": s, "sumsq": s2}, start, norm)
    if norm == "whisper":
        sh, sc = np.full(6, 4, np.float32), np.full(6, 0.25, np.float32)
    win = [(k, min(32, f.shape[0] - r), r) for k, (*_, f) in enumerate(segs) for r in range(0, f.shape[0], 24)]
    want = B.batch(x, start, win, 6, 32, fb.deltas, _ffi.BATCH_LAYOUTS[fb.layout], _ffi.BATCH_DTYPES[fb.dtype], B.PAD_FEATURE, -10.0, lo, sh, sc)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert index == [(segs[k][0], 0, segs[k][1], segs[k][2], r, nr) for k, nr, r in win]
    # one window per segment, as long as the longest
    got1, index1 = batch_recordings(recs, spec, FeatureBatch(norm=norm), cfg, engine=eng)
    T = max(4, -(-max(f.shape[0] for *_, f in segs) // 4) * 4)
    assert got1.shape == (len(segs), 6, T) and [ix[4:] for ix in index1] == [(0, f.shape[0]) for *_, f in segs]
    assert got1.tobytes() == B.batch(x, start, [(k, f.shape[0], 0) for k, (*_, f) in enumerate(segs)], 6, T, lo=lo, shift=sh, scale=sc).tobytes()


def test_batch_recordings_refusals(eng):
    from cutter_vad_amd import FeatureBatch, MelSpec, batch_recordings
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    cfg = _cfg(eng.frame_samples)
    mono, stereo = np.zeros(4000, np.float32), np.zeros((4000, 2), np.float32)
    with pytest.raises(ConfigurationError, match="once for the 1-D and once for the two-channel"):
        batch_recordings([mono, stereo], spec, FeatureBatch(), cfg, engine=eng)

    class NoBatch:
        sample_rate, frame_samples = 16000, 512
        mel = None

    with pytest.raises(ConfigurationError, match="batch_recordings needs an engine with mel_batch .*NoBatch has none"):
        batch_recordings([mono], spec, FeatureBatch(), cfg, engine=NoBatch())
    for bad in (dict(norm="l2"), dict(frames=6), dict(deltas=3), dict(dtype="f64"), dict(layout="x"), dict(pad="zero"), dict(stride=0)):
        with pytest.raises(ConfigurationError):
            batch_recordings([mono], spec, FeatureBatch(**bad), cfg, engine=eng)
    got, index = batch_recordings([mono, mono], spec, FeatureBatch(frames=8, dtype="f16"), cfg, engine=eng)      # no speech anywhere
    assert got.shape == (0, 6, 8) and got.dtype == np.float16 and index == []
    assert batch_recordings([], spec, FeatureBatch(frames=8, layout="time", deltas=2), cfg, engine=eng)[0].shape == (0, 8, 18)


# ---- the order of the checks ------------------------------------------------------------------------------------------
def test_a_batch_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_mel_batch's checks is behaviour: vad_batch's fields, the matrix and its segments (the device form's
    feature alignment with them), the counts, nss, lo, shift, the windows, out_bytes, the output pointer, and last the device
    form's output alignment.  Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    nan, inf = float("nan"), float("inf")

    def call(device, n_mels, frames, deltas, layout, dtype, pad_mode, pad_value, rows, n, start, features, nw, nss, lo, shift, windows, out_bytes,
             out):
        b = _ffi.Batch(n_mels, frames, deltas, layout, dtype, pad_mode, pad_value, 0)
        st = np.array(start, np.int64)
        win = (_ffi.BatchWindow * len(windows))(*[_ffi.BatchWindow(*w) for w in windows])
        args = (rows, st.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(b), win, nw, RO.f32p(lo), RO.f32p(shift), None, nss, RO.addr(out),
                out_bytes)
        if device:
            return lib.vad_mel_batch_device(eng.handle, RO.addr(features), *args, None)
        return lib.vad_mel_batch(eng.handle, RO.f32p(features), *args)

    good = [(0, 3, 0), (1, 4, 1)]                                # (seg, nrows, row0): segments of 3 and 5 rows
    faults = dict(n_mels=0, frames=5, deltas=3, layout=2, dtype=3, pad_mode=2, pad_value=nan, rows=-1, n=-1, start=[0, 3, 9],
                  features=RO.buf(4 * 4 * 8, 2), nw=-1, nss=3, lo=RO.f32(nan, 0.0), shift=RO.f32(0.0, inf, 0.0, 0.0), windows=[(0, 3, 0), (5, 4, 1)],
                  out_bytes=0, out=None)
    RO.walk(lib, eng, call, faults, (
        (INV, "n_mels = 0 must be", "n_mels", 4),
        (INV, "frames = 5 must be", "frames", 4),
        (INV, "deltas = 3 must be", "deltas", 0),
        (INV, "layout = 2 is neither", "layout", 0),
        (INV, "dtype = 3 is none of", "dtype", 0),
        (INV, "pad_mode = 2 is neither", "pad_mode", 0),
        (INV, "pad_value is NaN", "pad_value", 0.0),
        (INV, "rows = -1 is negative", "rows", 8),
        (INV, "n = -1 is negative", "n", 2),
        (INV, r"start\[n\] = 9 leaves the matrix of 8 rows", "start", [0, 3, 8]),
        (INV, "the features must be 4-byte aligned", "features", RO.buf(4 * 4 * 8), RO.DEVICE),
        (INV, "null buffer or bad count", "nw", 2),
        (INV, "nss = 3: shift and scale have 1 row or n = 2", "nss", 1),
        (INV, r"lo\[0\] is NaN", "lo", None),
        (INV, r"shift\[0\]\[1\] is infinite", "shift", RO.f32(0.0, 0.0, 0.0, 0.0)),
        (INV, "window 1 names segment 5 of 2", "windows", good),
        (INV, "out_bytes = 0, the windows have 128 bytes", "out_bytes", 128),
        (INV, "vad_mel_batch(_device)?: null buffer$", "out", RO.buf(128, 4)),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(128), RO.DEVICE)))


@pytest.mark.parametrize("rate", [16000, 48000])
def test_a_keep_with_several_faults_gets_the_first_refusal(lib, eng, rate):
    """... and vad_scan_mel_keep's, which has no output to refuse.  At the engine's rate vad_mel's fields and the filters come
    before the block's and the segments' checks, as in vad_scan_mel; at 48 kHz the rate and the taps come first and vad_mel's
    fields behind the segments, as in vad_scan_rate_mel."""
    from tests import refusal_order as RO
    op_re, op_im, filters = RO.mel_ops()
    good, far = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 0, 0, 0)], [(0, 0, 1, 0, 0, 0), (0, 7, 2, 0, 0, 0)]
    rows_out = C.c_int64(-1)

    def call(device, sr_in, taps, ntaps, fmt, channels, hop, items, n_fft, floor, fil, audio):
        m = RO.mel(n_fft=n_fft, floor=floor)
        args = (eng.handle, RO.cut_items(items), len(items), C.byref(m), RO.f32p(op_re), RO.f32p(op_im), RO.f32p(fil), RO.f32p(taps), ntaps,
                RO.addr(audio), RO.NS, channels, fmt, sr_in, hop, -1.0, C.byref(rows_out))
        return lib.vad_scan_mel_keep_device(*args, None) if device else lib.vad_scan_mel_keep(*args)

    faults = dict(sr_in=44100 if rate == 48000 else 0, taps=None, ntaps=2, fmt=9, channels=3, hop=6, items=far, n_fft=100, floor=float("nan"),
                  fil=None, audio=RO.buf(4 * RO.NS, 2))
    first = ((RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 48000),
             (INV, "null taps", "taps", RO.f32(0.25, float("nan"), 0.25)),
             (INV, "ntaps = 2 must be odd", "ntaps", 3),
             (INV, r"taps\[1\] is NaN", "taps", RO.f32(0.25, 0.5, 0.25)))
    block = ((INV, "unknown frame format 9", "fmt", 0),
             (INV, "channels = 3, the block holds", "channels", 1),
             (INV, "hop = 6 must be", "hop", 256),
             (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", good))
    fields = ((INV, "n_fft = 100 must be", "n_fft", 64),
              (INV, "floor = -?nan: a logarithm needs", "floor", 1e-5),
              (INV, "null filters", "fil", filters))
    last = ((INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),)
    RO.walk(lib, eng, call, faults, first + block + fields + last if rate == 48000 else fields + block + last)
    assert rows_out.value == (63 if rate == 48000 else 74)


# ---- the whole order of the family's checks, on the smallest shapes that reach them ----------------------------------------
# A matrix of 3 rows x 2 columns, start = [0, 1, 3], frames = 4, one window or one piece - a caller's matrix and a resident one.
# tests/test_mel_pack_host.py walks vad_mel_batch_packed and vad_mel_stats_grouped with the same helpers
def keep_3x2(lib, eng):
    """a keep that leaves 3 rows x 2 columns resident, start = [0, 1, 3]: analysis frames of 512 samples at a hop of 256 over two
    segments of 512 and 768 samples"""
    from tests import refusal_order as RO
    m = RO.mel(n_fft=512, hop=256, n_bins=1, n_mels=2)
    op, fil, rows = np.zeros(512, np.float32), np.zeros(2, np.float32), C.c_int64(-1)
    rc = lib.vad_scan_mel_keep(eng.handle, RO.cut_items([(0, 0, 1, 0, 0, 0), (0, 1, 2, 0, 0, 0)]), 2, C.byref(m), RO.f32p(op), RO.f32p(op), RO.f32p(fil),
                               None, 0, RO.addr(RO.buf(4 * RO.NS)), RO.NS, 1, _ffi.VAD_FMT_F32, 0, 256, -1.0, C.byref(rows))
    assert rc == 0 and rows.value == 3, lib.vad_last_error(eng.handle).decode()


def batch_order_call(lib, eng, packed=False):
    """call(device, **kw) -> rc of vad_mel_batch, or of vad_mel_batch_packed, for refusal_order.walk.  kw names every argument; items
    are the windows (seg, nrows, row0) or the pieces (seg, nrows, row0, window, offset); kept = True keeps keep_3x2's matrix first"""
    from tests import refusal_order as RO
    rec, name = (_ffi.BatchPiece, "vad_mel_batch_packed") if packed else (_ffi.BatchWindow, "vad_mel_batch")

    def call(device, null_b, n_mels, frames, deltas, layout, dtype, pad_mode, pad_value, reserved, features, rows, start, n, items, nw, lo, shift, scale,
             nss, out, out_bytes, kept=False):
        if kept:
            keep_3x2(lib, eng)
        b = _ffi.Batch(n_mels, frames, deltas, layout, dtype, pad_mode, pad_value, reserved)
        st = None if start is None else np.array(start, np.int64)
        arr = (rec * max(len(items), 1))(*[rec(*i) for i in items])
        counts = (len(items), nw) if packed else (nw,)
        args = (rows, RO.i64p(st), n, None if null_b else C.byref(b), arr, *counts, RO.f32p(lo), RO.f32p(shift), RO.f32p(scale), nss, RO.addr(out),
                out_bytes)
        if device:
            return getattr(lib, name + "_device")(eng.handle, RO.addr(features), *args, None)
        return getattr(lib, name)(eng.handle, RO.f32p(features), *args)

    return call


def batch_order(packed, items, item_steps):
    """(faults, steps) of a batch call on a caller's matrix with every reachable fault at once.  lo is indexed over the n = 2 segments
    and nss is 1 or n, or both go over the nw = 1 windows (packed).  items: the call's windows or pieces with every fault of theirs;
    item_steps: (pattern, mended items) in the order of their checks"""
    from tests import refusal_order as RO
    nan, inf, per = float("nan"), float("inf"), 1 if packed else 2
    faults = dict(null_b=True, n_mels=0, frames=5, deltas=3, layout=2, dtype=3, pad_mode=2, pad_value=nan, reserved=1, features=RO.buf(24, 2), rows=-1,
                  start=[0, 2, 4], n=-1, items=items, nw=-1, lo=RO.f32(*[nan] * per), shift=RO.f32(0.0, inf, *[0.0] * (2 * per - 2)),
                  scale=RO.f32(*[1.0] * (2 * per - 1), nan), nss=3, out=None, out_bytes=0)
    steps = ((INV, "null vad_batch", "null_b", False),
             (INV, "n_mels = 0 must be", "n_mels", 2),
             (INV, "frames = 5 must be", "frames", 4),
             (INV, "deltas = 3 must be", "deltas", 0),
             (INV, "layout = 2 is neither", "layout", 0),
             (INV, "dtype = 3 is none of", "dtype", 0),
             (INV, "pad_mode = 2 is neither", "pad_mode", 0),
             (INV, "pad_value is NaN", "pad_value", 0.0),
             (INV, "vad_batch.reserved = 1 must be 0", "reserved", 0),
             (INV, "rows = -1 is negative", "rows", 3),
             (INV, "n = -1 is negative", "n", 2),
             (INV, r"start\[0\] = 0 \.\. start\[n\] = 4 leaves the matrix of 3 rows", "start", [0, 2, 1]),
             (INV, "segment 1: start = 2 is followed by 1", "start", [0, 1, 3]),
             (INV, "the features must be 4-byte aligned", "features", RO.buf(24), RO.DEVICE),
             (INV, "null buffer or bad count", "nw", 1),
             (INV, "nss = 3: shift and scale have 1 row or " + ("nw = 1" if packed else "n = 2"), "nss", per),
             (INV, r"lo\[0\] is NaN", "lo", RO.f32(*[-1.0] * per)),
             (INV, r"shift\[0\]\[1\] is infinite", "shift", RO.f32(*[0.5] * (2 * per))),
             (INV, r"scale\[%d\]\[1\] is NaN" % (per - 1), "scale", RO.f32(*[2.0] * (2 * per))))
    steps += tuple((INV, pattern, "items", mended) for pattern, mended in item_steps)
    steps += ((INV, "out_bytes = 0, the windows have 32 bytes", "out_bytes", 32),
              (INV, r"vad_mel_batch(_packed)?(_device)?: null buffer$", "out", RO.buf(32, 4)),
              (INV, "the output must be 16-byte aligned", "out", RO.buf(32), RO.DEVICE))
    return faults, steps


def batch_order_walks(lib, make_engine, packed, items, item_steps):
    """the three parts of a batch call's order: the walk on a caller's matrix, where nw == 0 stands, and the walk on a resident one"""
    from tests import refusal_order as RO
    faults, steps = batch_order(packed, items, item_steps)
    eng = make_engine()
    call = batch_order_call(lib, eng, packed)
    RO.walk(lib, eng, call, faults, steps)
    # nw == 0 is VAD_OK behind out_bytes and ahead of the output's checks: a null or misaligned out passes and nothing is written, while
    # an infinite shift (no window is read) and a negative out_bytes are still refused
    done = dict(faults)
    done.update({s[2]: s[3] for s in steps})
    for device in (False, True):
        for out in (None, RO.buf(32, 4)):
            if out is not None:
                out[:] = FILL
            assert call(device, **{**done, "nw": 0, "items": [], "out": out, "out_bytes": 0}) == 0
            assert out is None or (out == FILL).all()
        assert call(device, **{**done, "nw": 0, "items": [], "shift": faults["shift"]}) == INV and "shift[0][1] is infinite" in lib.vad_last_error(eng.handle).decode()
        assert call(device, **{**done, "nw": 0, "items": [], "out_bytes": -1}) == INV
    # the resident matrix under segments of the caller's, then under its own: its absence first, its width behind the segments
    for device in (False, True):
        eng = make_engine()
        call = batch_order_call(lib, eng, packed)
        RO.walk_one(lib, eng, lambda **kw: call(device, **kw),
                    {**done, "features": None, "rows": -1, "n_mels": 3, "start": [0, 1, 4], "nw": -1, "nss": 3, "out": RO.buf(32, 4 if device else 0)},
                    [(INV, "NULL names the resident matrix, and the engine holds none", "kept", True),
                     (INV, r"start\[n\] = 4 leaves the matrix of 3 rows", "start", None),
                     (INV, "n_mels = 3, the resident matrix has 2", "n_mels", 2),
                     (INV, "null buffer or bad count", "nw", 1),
                     (INV, "nss = 3: shift and scale have 1 row or " + ("nw = 1" if packed else "n = 2"), "nss", 1 if packed else 2)] +
                    ([(INV, "the output must be 16-byte aligned", "out", RO.buf(32))] if device else []))


def test_the_whole_order_of_a_batch_call(lib, make_engine):
    """vad_mel_batch / _device, every reachable check: vad_batch's fields in batch_check's order, the matrix and its segments (no
    resident matrix, rows, n, start[0] / start[n], ascending, the device form's feature alignment), n_mels against the resident
    matrix, the counts, nss, lo, shift, scale, per window its segment and its rows, out_bytes, nw == 0, the null out, the device
    form's output alignment.  Left out, as they need more than 2^31 - 1 elements: more than 2^31 - 1 segments, a segment of 2^31
    rows or more, more than 2^31 - 1 workgroups."""
    batch_order_walks(lib, make_engine, False, [(5, 3, 0)],
                      [("window 0 names segment 5 of 2", [(1, 3, 0)]),
                       (r"window 0: rows 0 \.\. \+3 of segment 1, which has 2, in 4 frames", [(1, 2, 0)])])


def stats_order_call(lib, eng, grouped=False):
    """call(device, **kw) -> rc of vad_mel_stats, or of vad_mel_stats_grouped, for refusal_order.walk; outs = (max, sum, sumsq)"""
    from tests import refusal_order as RO
    name = "vad_mel_stats_grouped" if grouped else "vad_mel_stats"

    def call(device, features, rows, n_mels, start, n, outs, group=None, ngroups=0, kept=False):
        if kept:
            keep_3x2(lib, eng)
        st = None if start is None else np.array(start, np.int64)
        gr = None if group is None else np.array(group, np.int32)
        head = (rows, n_mels, RO.i64p(st), n) + ((None if gr is None else gr.ctypes.data_as(C.POINTER(C.c_int32)), ngroups) if grouped else ())
        if device:
            return getattr(lib, name + "_device")(eng.handle, RO.addr(features), *head, *[RO.addr(o) for o in outs], None)
        mx, sm, sq = outs
        return getattr(lib, name)(eng.handle, RO.f32p(features), *head, RO.f32p(mx), RO.i64p(sm), None if sq is None else sq.ctypes.data_as(_u64p))

    return call


def stats_order_walks(lib, make_engine, grouped):
    """the parts of a statistics call's order: a caller's 3 x 2 matrix, the row bound of the sums on one segment of
    VAD_STATS_MAX_ROWS + 1 rows x 1 column, where the early VAD_OK stands, and a resident matrix"""
    from tests import refusal_order as RO
    eng = make_engine()
    call = stats_order_call(lib, eng, grouped)
    most = _ffi.VAD_STATS_MAX_ROWS
    aligned = lambda cols: (RO.buf(8), RO.buf(16 * cols), RO.buf(16 * cols))                      # noqa: E731
    askew = lambda cols: (RO.buf(8), RO.buf(16 * cols, 4), RO.buf(16 * cols))                     # noqa: E731
    groups = dict(group=[0, 5], ngroups=-1) if grouped else {}
    group_steps = ((INV, "ngroups = -1 must be", "ngroups", 2), (INV, "segment 1 names group 5 of 2", "group", [1, 0])) if grouped else ()
    faults = dict(features=RO.buf(24, 2), rows=-1, n_mels=0, start=[0, 2, 4], n=-1, outs=askew(2), **groups)
    steps = ((INV, "rows = -1 is negative", "rows", 3),
             (INV, "n_mels = 0 must be 1 .. 128", "n_mels", 2),
             (INV, "n = -1 is negative", "n", 2),
             (INV, r"start\[0\] = 0 \.\. start\[n\] = 4 leaves the matrix of 3 rows", "start", [0, 2, 1]),
             (INV, "segment 1: start = 2 is followed by 1", "start", [0, 1, 3]),
             (INV, "the features must be 4-byte aligned", "features", RO.buf(24), RO.DEVICE)) + group_steps + (
             (INV, "the sums must be 8-byte aligned, the maxima 4-byte", "outs", aligned(2), RO.DEVICE),)
    RO.walk(lib, eng, call, faults, steps)
    # the row bound stands behind the groups and ahead of the outputs' alignment
    one = dict(group=[0], ngroups=1) if grouped else {}
    RO.walk(lib, eng, call, dict(features=RO.buf(4 * (most + 1)), rows=most + 1, n_mels=1, start=[0, most + 1], n=1, outs=askew(1), **one),
            ((INV, "%s 0 has %d rows, the sums take %d at the most" % ("group" if grouped else "segment", most + 1, most), "start", [0, most]),
             (INV, "the sums must be 8-byte aligned, the maxima 4-byte", "outs", aligned(1), RO.DEVICE)))
    # no entry to write, or no output asked for, is VAD_OK behind the alignment, and nothing is written
    none = dict(features=RO.buf(24), rows=3, n_mels=2, start=[0], n=0, **(dict(group=[], ngroups=0) if grouped else {}))
    assert call(True, **none, outs=askew(2)) == INV and "8-byte aligned" in lib.vad_last_error(eng.handle).decode()
    for device in (False, True):
        outs = aligned(2)
        for o in outs:
            o[:] = FILL
        assert call(device, **none, outs=outs) == 0 and all((o == FILL).all() for o in outs)
        assert call(device, **{**none, "start": [0, 1, 3], "n": 2, **(dict(group=[1, 0], ngroups=2) if grouped else {})}, outs=(None, None, None)) == 0
    # the resident matrix under segments of the caller's: its absence first (n_mels is the resident one's: the argument is not read)
    for device in (False, True):
        eng = make_engine()
        call = stats_order_call(lib, eng, grouped)
        RO.walk_one(lib, eng, lambda **kw: call(device, **kw),
                    dict(features=None, rows=-1, n_mels=0, start=[0, 1, 4], n=2, outs=askew(2) if device else aligned(2), **groups),
                    [(INV, "NULL names the resident matrix, and the engine holds none", "kept", True),
                     (INV, r"start\[n\] = 4 leaves the matrix of 3 rows", "start", None)] + list(group_steps) +
                    ([(INV, "the sums must be 8-byte aligned, the maxima 4-byte", "outs", aligned(2))] if device else []))


def test_the_whole_order_of_a_stats_call(lib, make_engine):
    """vad_mel_stats / _device, every reachable check: the matrix and its segments (no resident matrix, rows, n_mels, n,
    start[0] / start[n], ascending, the device form's feature alignment), the row bound of the sums per segment, the device form's
    output alignment, then VAD_OK for n == 0 or no output.  Left out, as they need more than 2^31 - 1 elements: more than 2^31 - 1
    segments, a segment of 2^31 rows or more, more than 2^31 - 1 workgroups."""
    stats_order_walks(lib, make_engine, False)
