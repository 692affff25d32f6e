"""vad_mel_pack_plan, vad_mel_batch_packed and vad_mel_stats_grouped on the host side: exports, the planner against the header's
worked example and tests/pack_ref.py, every refusal with its message and an untouched, pre-filled output, np == 0 and nw == 0,
single-piece windows against vad_mel_batch, every kind of engine, host form against device form, and the Python faces (batch_pack,
FeatureBatch, batch_recordings(pack=True)) - the real csrc/engine.cpp over the HIP stand-in (tests/standin.py), byte for byte against
tests/pack_ref.py.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi
from cutter_vad_amd.core.exceptions import AudioProcessingError, ConfigurationError
from tests import batch_ref as B
from tests import pack_ref as P
from tests.test_mel_batch_host import (FILL, INV, ROOT, _cfg, _speech, batch_struct, eng, lib, make_engine, matrix, raw_batch, same,  # noqa: F401
                                       special_values)

NEW = ["vad_mel_pack_plan", "vad_mel_batch_packed", "vad_mel_batch_packed_device", "vad_mel_stats_grouped", "vad_mel_stats_grouped_device"]
_f32p, _i64p, _u64p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
EXAMPLE_ROWS, EXAMPLE_GROUPS = [5, 3, 0, 9, 64, 1, 70, 2, 2], [0, 0, 0, 0, 0, 1, 1, 1, 1]
# (seg, row0, nrows, window, offset), as the issue and the header's rule give them for T = 68, gap = 0
EXAMPLE = [(0, 0, 5, 0, 0), (1, 0, 3, 0, 8), (3, 0, 9, 0, 12), (4, 0, 64, 1, 0), (5, 0, 1, 2, 0), (6, 0, 68, 3, 0), (6, 68, 2, 4, 0), (7, 0, 2, 4, 4),
           (8, 0, 2, 4, 8)]


def piece_array(pieces):
    return np.array([tuple(map(int, p)) for p in pieces], _ffi.BATCH_PIECE_DTYPE).reshape(-1)


def raw_plan(lib, start, frames, gap=0, group=None, cap=None, count_only=False):
    """vad_mel_pack_plan -> (rc, pieces as tuples, npieces, nwindows, the whole pre-filled piece buffer as bytes)"""
    st = np.ascontiguousarray(start, np.int64)
    gr = None if group is None else np.ascontiguousarray(group, np.int32)
    room = 64 if cap is None else max(cap, 1)
    buf = np.full(room * 24, FILL, np.uint8)
    np_, nw = C.c_int64(-7), C.c_int64(-7)
    rc = lib.vad_mel_pack_plan(st.ctypes.data_as(_i64p), st.size - 1, None if gr is None else gr.ctypes.data_as(_i32p), frames, gap,
                               None if count_only else buf.ctypes.data_as(C.POINTER(_ffi.BatchPiece)), room if cap is None else cap, C.byref(np_),
                               C.byref(nw))
    got = buf.view(_ffi.BATCH_PIECE_DTYPE)[:max(np_.value, 0)] if rc == 0 and not count_only else buf.view(_ffi.BATCH_PIECE_DTYPE)[:0]
    return rc, [tuple(int(v) for v in p) for p in got.tolist()], np_.value, nw.value, buf


def raw_packed(lib, eng, x, start, b, pieces, nw, lo=None, shift=None, scale=None, nss=1, device=False, out_bytes=None, rows=None, n=None,
               null_out=False, misalign=0, np_=None):
    """vad_mel_batch_packed (or _device) -> (rc, message, out as bytes with room behind, the whole buffer); pre-filled with FILL"""
    p = piece_array(pieces)
    elt = 4 if b is None or b.dtype == B.F32 else 2
    need = 0 if b is None else max(nw, 0) * b.n_mels * (b.deltas + 1) * b.frames * elt
    out = np.full(need + 64 + 16, FILL, np.uint8)
    base = out.ctypes.data + (-out.ctypes.data) % 16 + misalign
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (lo, shift, scale)]
    xs = None if x is None else np.ascontiguousarray(x, np.float32)
    st = None if start is None else np.ascontiguousarray(start, np.int64)
    pp = (p if p.size else np.zeros(1, _ffi.BATCH_PIECE_DTYPE)).ctypes.data_as(C.POINTER(_ffi.BatchPiece))
    args = (eng.handle, None if xs is None else (xs.ctypes.data if device else xs.ctypes.data_as(_f32p)),
            (0 if xs is None else xs.shape[0]) if rows is None else rows, None if st is None else st.ctypes.data_as(_i64p),
            (0 if st is None else st.size - 1) if n is None else n, None if b is None else C.byref(b), pp, len(p) if np_ is None else np_, nw,
            *[None if a is None else a.ctypes.data_as(_f32p) for a in keep], nss, None if null_out else base, need if out_bytes is None else out_bytes)
    if device:
        rc = lib.vad_mel_batch_packed_device(*args, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_mel_batch_packed(*args)
    off = base - out.ctypes.data
    return rc, lib.vad_last_error(eng.handle).decode(), out[off:off + need + 48], out


def raw_grouped(lib, eng, x, start, group, ngroups, want=(True, True, True), device=False):
    nm = x.shape[1]
    room = max(ngroups if group is not None else len(start) - 1, 1)
    mx = np.full(room, FILL, np.uint8).repeat(4).view(np.float32)
    s = np.full(room * nm * 8, FILL, np.uint8).view(np.int64)
    s2 = np.full(room * nm * 8, FILL, np.uint8).view(np.uint64)
    xs, st = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(start, np.int64)
    gr = None if group is None else np.ascontiguousarray(group, np.int32)
    head = (eng.handle, xs.ctypes.data if device else xs.ctypes.data_as(_f32p), xs.shape[0], nm, st.ctypes.data_as(_i64p), st.size - 1,
            None if gr is None else gr.ctypes.data_as(_i32p), ngroups)
    if device:
        rc = lib.vad_mel_stats_grouped_device(*head, mx.ctypes.data if want[0] else None, s.ctypes.data if want[1] else None,
                                              s2.ctypes.data if want[2] else None, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_mel_stats_grouped(*head, mx.ctypes.data_as(_f32p) if want[0] else None, s.ctypes.data_as(_i64p) if want[1] else None,
                                       s2.ctypes.data_as(_u64p) if want[2] else None)
    return rc, lib.vad_last_error(eng.handle).decode(), mx, s, s2


# ---- shared cases (tests/test_gpu_mel_pack.py runs the same ones on the GPU) ------------------------------------------------
PACK_SEGS = [1, 2, 3, 4, 5, 9, 0, 150]


def pack_cases(rng, n_mels, T):
    """(x, start, pieces, nw): pieces of 1, 2, 3, 4, 5 and 9 rows at offsets 0, 4, T - 8 and T - 4 where they fit, two and three pieces
    inside one tile, a piece across the tile edge of 64 (offset 60, 9 rows: T = 72 and more), a split segment whose later piece
    needs the earlier one's rows as its delta halo, the same segment in two windows, the same rows twice, a window with no piece, a
    window covered exactly, and the whole list in reversed order"""
    x, start = matrix(rng, PACK_SEGS, n_mels)
    special_values(x[int(start[7]):])
    pieces, w = [], 0
    for seg, M in enumerate(PACK_SEGS[:6]):                       # window per short segment and offset
        for offset in sorted({0, 4, T - 8, T - 4}):
            if offset >= 0 and offset + M <= T:
                pieces.append((seg, M, 0, w, offset))
                w += 1
    if T >= 12:                                                   # three pieces inside one tile, gaps of 0 and of a quad
        pieces += [(0, 1, 0, w, 0), (2, 3, 0, w, 4), (4, 2, 3, w, T - 4)]
        w += 1
    if T >= 72:                                                   # across the edge of the 64-frame tile (and of the 32-frame one)
        pieces += [(5, 9, 0, w, 60), (3, 4, 0, w, 28)]
        w += 1
    w += 1                                                        # a window with no piece
    k = min(T, 64)
    pieces += [(7, k, 0, w, 0)]                                   # covered exactly (T <= 64), then the segment's next rows: a split
    pieces += [(7, min(T, 150 - k), k, w + 1, 0)]
    pieces += [(7, min(T, 60), 2, w + 2, 0), (7, min(T, 60), 2, w + 3, 0)]      # the same rows twice
    if T >= 16:
        pieces += [(7, 5, 77, w + 3, T - 8)] if T >= 72 else []
        pieces += [(7, 3, 147, w + 4, 0), (7, 4, 0, w + 4, 4), (7, 4, 4, w + 4, 8)]     # the segment's last rows ahead of its first
        w += 1
    return x, start, pieces[::-1], w + 4


def affines(rng, x, nw, n_mels):
    """(pad_mode, (lo, shift, scale, nss)): none, per window with a lo that IS a feature value (and one -inf), one row"""
    lo_some = np.sort(x, axis=None)[[x.size // 3] * nw].astype(np.float32)
    lo_some[::3] = -np.inf
    sh1, sc1 = rng.uniform(-2, 2, (1, n_mels)).astype(np.float32), rng.uniform(0.1, 3, (1, n_mels)).astype(np.float32)
    shn, scn = rng.uniform(-2, 2, (nw, n_mels)).astype(np.float32), rng.uniform(0.1, 3, (nw, n_mels)).astype(np.float32)
    return ((B.PAD_VALUE, (None, None, None, 1)), (B.PAD_FEATURE, (lo_some, shn, scn, nw)), (B.PAD_FEATURE, (None, sh1, sc1, 1)))


def random_rows(rng, n, T):
    return rng.choice([0, 1, 2, 3, 4, 5, 7, T - 1, T, T + 1, 2 * T, 2 * T + 3], n).astype(np.int64)


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
    m = re.search(r"typedef struct vad_batch_piece \{(.*?)\} vad_batch_piece;", header, re.S)
    fields = re.findall(r"(int32_t|int64_t)\s+(\w+);", m.group(1))
    assert fields == [("int32_t", "seg"), ("int32_t", "nrows"), ("int64_t", "row0"), ("int32_t", "window"), ("int32_t", "offset")]
    assert [f[0] for f in _ffi.BatchPiece._fields_] == [f[1] for f in fields] == list(_ffi.BATCH_PIECE_DTYPE.names)
    assert C.sizeof(_ffi.BatchPiece) == 24 == _ffi.BATCH_PIECE_DTYPE.itemsize
    assert [_ffi.BATCH_PIECE_DTYPE.fields[k][1] for k in _ffi.BATCH_PIECE_DTYPE.names] == [0, 4, 8, 16, 20]
    import cutter_vad_amd
    from cutter_vad_amd.engine import Engine
    assert "batch_pack" in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, "batch_pack")
    assert hasattr(Engine, "mel_batch_packed") and hasattr(Engine, "mel_batch_packed_device")
    fb = cutter_vad_amd.FeatureBatch()
    assert list(fb.__dataclass_fields__)[-3:] == ["pack", "gap", "scope"] and (fb.pack, fb.gap, fb.scope) == (False, 0, None)


# ---- the planner ------------------------------------------------------------------------------------------------------
def test_plan_worked_example(lib):
    start = np.concatenate([[0], np.cumsum(EXAMPLE_ROWS)])
    rc, got, np_, nw, _ = raw_plan(lib, start, 68, 0, EXAMPLE_GROUPS)
    assert rc == 0 and (np_, nw) == (9, 5)
    assert [(s, r, k, w, o) for s, k, r, w, o in got] == EXAMPLE
    assert P.plan(start, 68, 0, EXAMPLE_GROUPS) == (got, 5)
    rc, got2, np_, nw, _ = raw_plan(lib, start, 68, 2, EXAMPLE_GROUPS)
    assert rc == 0 and (np_, nw) == (9, 5) and [p[4] for p in got2 if p[3] == 0] == [0, 8, 16]
    assert P.plan(start, 68, 2, EXAMPLE_GROUPS) == (got2, 5)
    assert P.piece_bounds(start, got).tolist() == sorted(P.piece_bounds(start, got).tolist()) and P.piece_bounds(start, got)[-1] == start[-1]
    rc, none, np_, nw, buf = raw_plan(lib, start, 68, 0, EXAMPLE_GROUPS, count_only=True)
    assert rc == 0 and (np_, nw) == (9, 5) and (buf == FILL).all()


@pytest.mark.parametrize("case", ["T4", "all_longer", "all_empty", "n0", "one_group", "random0", "random1", "random2", "random3"])
def test_plan_against_the_reference(lib, case):
    rng = np.random.default_rng(sum(map(ord, case)))
    T, gap, group = 8, 0, None
    if case == "T4":
        T, rows, gap = 4, [1, 4, 5, 0, 3, 9, 2], 0
    elif case == "all_longer":
        rows, gap = [9, 17, 8 + 1, 24 + 7], 4
    elif case == "all_empty":
        rows = [0] * 5
    elif case == "n0":
        rows = []
    elif case == "one_group":
        T, rows = 64, random_rows(rng, 40, 64).tolist()
    else:
        T = int(rng.choice([4, 8, 64, 68]))
        rows = random_rows(rng, int(rng.integers(1, 60)), T).tolist()
        gap = int(rng.choice([0, 1, 2, 4, T]))
        group = np.sort(rng.integers(0, 6, len(rows))) if case != "random3" else rng.integers(0, 2, len(rows))
    start = np.concatenate([[3], 3 + np.cumsum(rows)]).astype(np.int64)
    want, wnw = P.plan(start, T, gap, group)
    rc, got, np_, nw, _ = raw_plan(lib, start, T, gap, group, cap=max(len(want), 1))
    assert rc == 0 and got == want and (np_, nw) == (len(want), wnw)
    # the properties the rule promises
    arr = piece_array(got)
    assert (arr["offset"] % 4 == 0).all() and (arr["offset"] + arr["nrows"] <= T).all() and (arr["nrows"] >= 1).all()
    assert arr["nrows"].sum() == start[-1] - start[0]
    if len(got):
        assert arr["window"][0] == 0 and set(np.diff(arr["window"]).tolist()) <= {0, 1} and arr["window"][-1] == nw - 1
        g = np.zeros(len(rows), np.int64) if group is None else np.asarray(group)
        for w in range(nw):
            assert len(set(g[arr["seg"][arr["window"] == w]].tolist())) == 1
    if case == "all_longer":
        assert [p[1] for p in got if p[2] == 0] == [8] * 4
    if case in ("all_empty", "n0"):
        assert (np_, nw) == (0, 0)


def test_plan_refusals(lib):
    start = np.array([0, 5, 9], np.int64)
    for kw in (dict(frames=0), dict(frames=6), dict(frames=65540), dict(frames=-4), dict(frames=8, gap=-1), dict(frames=8, gap=9),
               dict(frames=8, start=[0, 5, 4]), dict(frames=8, cap=1)):
        rc, got, np_, nw, buf = raw_plan(lib, kw.get("start", start), kw["frames"], kw.get("gap", 0), cap=kw.get("cap"))
        assert rc == INV and (buf == FILL).all(), kw
    rc, got, np_, nw, buf = raw_plan(lib, start, 8, cap=1)
    assert rc == INV and (np_, nw) == (2, 2)                      # too little room: the counts say how much
    rc, got, np_, nw, _ = raw_plan(lib, start, 8, gap=8)
    assert rc == 0 and [p[3:] for p in got] == [(0, 0), (1, 0)]    # gap = T: a window each
    rc, got, np_, nw, _ = raw_plan(lib, start, 65536)
    assert rc == 0 and [p[3:] for p in got] == [(0, 0), (0, 8)]


# ---- packed batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 64, 68, 72])
@pytest.mark.parametrize("deltas", [0, 1, 2])
def test_packed_byte_for_byte(lib, eng, T, deltas):
    rng = np.random.default_rng(10 * T + deltas)
    for n_mels in (5, 128) if T == 72 else (5,):
        x, start, pieces, nw = pack_cases(rng, n_mels, T)
        for layout in (B.CHANNEL, B.TIME):
            for dtype in (B.F32, B.F16, B.BF16):
                for pad_mode, (lo, sh, sc, nss) in affines(rng, x, nw, n_mels):
                    b = batch_struct(n_mels, T, deltas, layout, dtype, pad_mode, -10.0)
                    want = P.batch(x, start, pieces, nw, n_mels, T, deltas, layout, dtype, pad_mode, -10.0, lo, sh, sc)
                    for device in (False, True):
                        rc, msg, got, _ = raw_packed(lib, eng, x, start, b, pieces, nw, lo, sh, sc, nss, device=device)
                        assert rc == 0, msg
                        assert same(got, want), (n_mels, T, deltas, layout, dtype, pad_mode, device)


@pytest.mark.parametrize("gap", [0, 2])
def test_packed_planned_windows(lib, eng, gap):
    """the planner's own output - the worked example's segments with real rows - through the batch call"""
    rng = np.random.default_rng(gap)
    x, start = matrix(rng, EXAMPLE_ROWS, 5)
    rc, pieces, np_, nw, _ = raw_plan(lib, start, 68, gap, EXAMPLE_GROUPS)
    for deltas in (0, 2):
        for pad_mode, (lo, sh, sc, nss) in affines(rng, x, nw, 5):
            want = P.batch(x, start, pieces, nw, 5, 68, deltas, B.CHANNEL, B.F16, pad_mode, -10.0, lo, sh, sc)
            rc, msg, got, _ = raw_packed(lib, eng, x, start, batch_struct(5, 68, deltas, B.CHANNEL, B.F16, pad_mode, -10.0), pieces, nw, lo, sh, sc, nss)
            assert rc == 0 and same(got, want), msg


def test_single_piece_windows_are_vad_mel_batch(lib, eng):
    rng = np.random.default_rng(21)
    x, start = matrix(rng, PACK_SEGS, 5)
    win = [(7, 64, 2), (0, 1, 0), (5, 9, 0), (7, 22, 128), (3, 2, 1)]
    pieces = [(s, k, r, w, 0) for w, (s, k, r) in enumerate(win)]
    n = len(start) - 1
    lo_n, sh_n, sc_n = rng.uniform(-8, 0, n).astype(np.float32), rng.uniform(-2, 2, (n, 5)).astype(np.float32), rng.uniform(0.1, 3, (n, 5)).astype(np.float32)
    segs = [w[0] for w in win]
    for deltas in (0, 1, 2):
        for layout in (B.CHANNEL, B.TIME):
            for dtype in (B.F32, B.F16, B.BF16):
                b = batch_struct(5, 64, deltas, layout, dtype, B.PAD_FEATURE, -10.0)
                rc, msg, old, _ = raw_batch(lib, eng, x, start, b, win, lo_n, sh_n, sc_n, n)
                assert rc == 0, msg
                rc, msg, new, _ = raw_packed(lib, eng, x, start, b, pieces, len(win), lo_n[segs], sh_n[segs], sc_n[segs], len(win))
                assert rc == 0 and new.tobytes() == old.tobytes(), msg


def test_packed_rule_is_add_then_multiply(lib, eng):
    rng = np.random.default_rng(5)
    x, start = matrix(rng, [64], 8, -1.0, 1.0)
    sh, sc = rng.uniform(0.5, 1.5, (1, 8)).astype(np.float32), rng.uniform(0.5, 3, (1, 8)).astype(np.float32)
    pieces = [(0, 30, 0, 0, 0), (0, 30, 30, 0, 32)]
    want = P.batch(x, start, pieces, 1, 8, 64, shift=sh, scale=sc)
    fused = (x.astype(np.float64) * sc.astype(np.float64) + (sh * sc).astype(np.float64)).astype(np.float32)
    assert (fused[:30].T != want[0, :, :30]).sum() > 20
    rc, msg, got, _ = raw_packed(lib, eng, x, start, batch_struct(8, 64), pieces, 1, None, sh, sc, 1)
    assert rc == 0 and same(got, want), msg


def test_packed_refusals(lib, eng):
    rng = np.random.default_rng(6)
    x, start = matrix(rng, [5, 9], 5)
    ok = [(0, 4, 1, 0, 0), (1, 8, 0, 1, 0), (0, 2, 0, 0, 4)]
    good = dict(x=x, start=start, b=batch_struct(5, 8), pieces=ok, nw=2)

    def refused(pattern, devices=(False, True), **kw):
        for device in devices:
            rc, msg, got, whole = raw_packed(lib, eng, **{**good, **kw}, device=device)
            assert rc == INV and re.search(pattern, msg), (rc, msg)
            assert msg.startswith("Model prediction failed: vad_mel_batch_packed"), msg
            assert (whole == FILL).all()

    rc, msg, got, _ = raw_packed(lib, eng, **good)
    assert rc == 0 and same(got, P.batch(x, start, ok, 2, 5, 8)), msg
    refused("null vad_batch", b=None)
    for f, pat in ((dict(n_mels=0), "n_mels = 0 must be 1 .. 128"), (dict(frames=6), "frames = 6"), (dict(deltas=3), "deltas = 3"),
                   (dict(layout=2), "layout = 2 is neither"), (dict(dtype=3), "dtype = 3 is none of"), (dict(pad_mode=2), "pad_mode = 2 is neither"),
                   (dict(pad_value=float("nan")), "pad_value is NaN"), (dict(reserved=1), "reserved = 1 must be 0")):
        refused(pat, b=batch_struct(**{**dict(n_mels=5, frames=8), **f}))
    refused("leaves the matrix of 13 rows", rows=13)
    refused("null buffer or bad count", np_=-1)
    refused("null buffer or bad count", nw=-1)
    refused("nss = 3: shift and scale have 1 row or nw = 2", shift=np.zeros((3, 5)), nss=3)
    refused("shift\\[1\\]\\[2\\] is NaN", shift=np.array([[0] * 5, [0, 0, np.nan, 0, 0]]), nss=2)
    refused("scale\\[0\\]\\[4\\] is infinite", scale=np.array([[1, 1, 1, 1, np.inf]]), nss=1)
    refused("lo\\[1\\] is NaN", lo=np.array([0, np.nan]))
    refused("piece 1 names segment 2 of 2", pieces=[ok[0], (2, 1, 0, 1, 0)])
    refused("piece 0 names segment -1", pieces=[(-1, 1, 0, 0, 0)])
    refused("piece 1: rows 2 \\.\\. \\+8 of segment 1, which has 9", pieces=[ok[0], (1, 8, 2, 1, 0)])
    refused("piece 0: rows -1", pieces=[(0, 1, -1, 0, 0)])
    refused("piece 0: rows 0 \\.\\. \\+0 of segment 0", pieces=[(0, 0, 0, 0, 0)])
    refused("piece 0: rows 0 \\.\\. \\+-1", pieces=[(0, -1, 0, 0, 0)])
    refused("piece 2 names window 2 of 2", pieces=ok[:2] + [(0, 2, 0, 2, 4)])
    refused("piece 0 names window -1", pieces=[(0, 2, 0, -1, 4)])
    refused("piece 0: offset = -4 with 2 rows", pieces=[(0, 2, 0, 0, -4)])
    refused("piece 0: offset = 2 with 2 rows", pieces=[(0, 2, 0, 0, 2)])
    refused("piece 1: offset = 4 with 5 rows: a multiple of 4 from 0, offset \\+ nrows <= 8 frames", pieces=[ok[0], (1, 5, 0, 1, 4)])
    refused("piece 1: offset = 0 with 9 rows", pieces=[ok[0], (1, 9, 0, 1, 0)])
    refused("pieces 0 and 2 overlap in window 0: frames 0 \\.\\. 3 and 0 \\.\\. 3", pieces=ok[:2] + [(0, 2, 0, 0, 0)])
    # a piece of 5 rows owns the quad behind its last row as well
    refused("pieces 0 and 1 overlap in window 0: frames 0 \\.\\. 7 and 4 \\.\\. 7", pieces=[(0, 5, 0, 0, 0), (1, 1, 0, 0, 4)])
    refused("out_bytes = 319, the windows have 320 bytes", out_bytes=319)
    refused("null buffer$", null_out=True)
    refused("the output must be 16-byte aligned", devices=(True,), misalign=4)
    # the first of several faults: vad_batch, the matrix, the counts, nss, lo, shift, the pieces in their order, out_bytes, the output
    several = dict(b=batch_struct(5, 6), rows=13, nss=3, shift=np.zeros((3, 5)), lo=np.array([np.nan, 0]), pieces=[(2, 0, 0, 5, 2), (0, 5, 0, 0, 0), (1, 1, 0, 0, 4)],
                   out_bytes=0, null_out=True)
    order = (("frames = 6", dict(b=good["b"])), ("leaves the matrix of 13 rows", dict(rows=None)), ("nss = 3", dict(nss=1, shift=None)),
             ("lo\\[0\\] is NaN", dict(lo=None)), ("piece 0 names segment 2", dict(pieces=[(1, 0, 0, 5, 2)] + several["pieces"][1:])),
             ("piece 0: rows 0 \\.\\. \\+0", dict(pieces=[(1, 1, 0, 5, 2)] + several["pieces"][1:])),
             ("piece 0 names window 5", dict(pieces=[(1, 1, 0, 1, 2)] + several["pieces"][1:])),
             ("piece 0: offset = 2", dict(pieces=[(1, 1, 0, 1, 0)] + several["pieces"][1:])),
             ("pieces 1 and 2 overlap", dict(pieces=[(1, 1, 0, 1, 0), (0, 4, 0, 0, 0), (1, 1, 0, 0, 4)])),
             ("out_bytes = 0", dict(out_bytes=None)), ("null buffer$", dict(null_out=False)))
    for pattern, mend in order:
        refused(pattern, **several)
        several.update(mend)
    rc, msg, got, _ = raw_packed(lib, eng, **{**good, **several})
    assert rc == 0, msg


def test_packed_of_nothing(lib, eng):
    x, start = matrix(np.random.default_rng(7), [5], 5)
    sh = np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 1]], np.float32)
    for pad_mode in (B.PAD_VALUE, B.PAD_FEATURE):                 # np = 0 with nw > 0: pad windows
        for dtype in (B.F32, B.BF16):
            b = batch_struct(5, 8, 2, B.CHANNEL, dtype, pad_mode, -3.0)
            rc, msg, got, _ = raw_packed(lib, eng, x, start, b, [], 2, [-np.inf, 0.0], sh, None, 2)
            want = P.batch(x, start, [], 2, 5, 8, 2, B.CHANNEL, dtype, pad_mode, -3.0, [-np.inf, 0.0], sh)
            assert rc == 0 and same(got, want), msg
            assert B.convert(np.float32([-3.0 if pad_mode == B.PAD_VALUE else 1.0]), dtype)[0] == want[1, 4, 0] and not want[:, 5:].any()
    rc, msg, got, whole = raw_packed(lib, eng, x, start, batch_struct(5, 8), [], 0)
    assert rc == 0 and (whole == FILL).all(), msg
    rc, msg, got, whole = raw_packed(lib, eng, x, start, batch_struct(5, 8), [], 0, null_out=True, out_bytes=0)
    assert rc == 0, msg
    rc, msg, got, whole = raw_packed(lib, eng, np.zeros((0, 5), np.float32), np.array([0]), batch_struct(5, 8), [], 1)      # n == 0
    assert rc == 0 and same(got, np.zeros((1, 5, 8), np.float32)), msg
    rc, msg, got, whole = raw_packed(lib, eng, x, start, batch_struct(5, 8), [(0, 1, 0, 0, 0)], 0)
    assert rc == INV and "piece 0 names window 0 of 0" in msg


# ---- grouped statistics -----------------------------------------------------------------------------------------------
def test_grouped_stats(lib, eng):
    rng = np.random.default_rng(12)
    x, start = matrix(rng, [0, 1, 63, 300, 0, 65, 7], 5, -2100.0, 2100.0)
    special_values(x[1:])
    n = len(start) - 1
    plain = B.stats(x, start)
    for device in (False, True):
        # group = NULL is the identity: vad_mel_stats's bytes (ngroups is not read)
        rc, msg, *got = raw_grouped(lib, eng, x, start, None, -3, device=device)
        assert rc == 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, plain)), msg
        rc, msg, *got = raw_grouped(lib, eng, x, start, np.arange(n), n, device=device)
        assert rc == 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, plain)), msg
        for group, ng in (([0] * n, 1), ([2, 2, 0, 0, 4, 2, 4], 5), ([1, 0, 1, 0, 1, 0, 1], 2), ([3, 3, 3, 3, 3, 3, 3], 4)):
            want = P.stats_grouped(x, start, group, ng)
            rc, msg, *got = raw_grouped(lib, eng, x, start, group, ng, device=device)
            assert rc == 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (msg, group)
        rc, msg, mx, s, s2 = raw_grouped(lib, eng, x, start, [2, 2, 0, 0, 4, 2, 4], 5, device=device)
        assert mx[1] == -np.inf and mx[3] == -np.inf and not s[5:10].any() and not s2[15:20].any()       # groups without rows
        rc, msg, mx, s, s2 = raw_grouped(lib, eng, x, start, [0] * n, 1, want=(True, False, True), device=device)
        assert rc == 0 and (s.view(np.uint8) == FILL).all() and mx.tobytes() == P.stats_grouped(x, start, [0] * n, 1)[0].tobytes()


def test_grouped_stats_refusals(lib, eng):
    x, start = matrix(np.random.default_rng(13), [3, 4], 5)

    def refused(pattern, start=start, **kw):
        for device in (False, True):
            rc, msg, *outs = raw_grouped(lib, eng, x, start, device=device, **kw)
            assert rc == INV and re.search(pattern, msg), (rc, msg)
            assert msg.startswith("Model prediction failed: vad_mel_stats_grouped"), msg
            assert all((o.view(np.uint8) == FILL).all() for o in outs)

    refused("segment 1 names group 2 of 2", group=[0, 2], ngroups=2)
    refused("segment 0 names group -1 of 2", group=[-1, 0], ngroups=2)
    refused("ngroups = -1 must be", group=[0, 0], ngroups=-1)
    refused("segment 1: start = 5 is followed by 4", start=np.array([0, 5, 4, 7]), group=[0, 0, 0], ngroups=1)
    # the 2^17 rows bound a GROUP when a sum is asked for: two segments of 2^16 and 2^16 + 1 rows pass apart and are refused together
    half = 1 << 16
    long = np.array([0, half, 2 * half + 1, 2 * half + 2], np.int64)
    big = np.zeros((2 * half + 2, 1), np.float32)
    big[half + 5, 0] = 3.0
    for device in (False, True):
        rc, msg, mx, s, s2 = raw_grouped(lib, eng, big, long, [1, 1, 0], 2, device=device)
        assert rc == INV and "group 1 has 131073 rows, the sums take 131072 at the most" in msg
        assert all((o.view(np.uint8) == FILL).all() for o in (mx, s, s2))
        rc, msg, mx, s, s2 = raw_grouped(lib, eng, big, long, [1, 1, 0], 2, want=(True, False, False), device=device)
        assert rc == 0 and mx.tolist() == [0.0, 3.0], msg         # the maximum alone has no such bound
        rc, msg, mx, s, s2 = raw_grouped(lib, eng, big, long, [1, 0, 1], 2, device=device)
        assert rc == 0 and mx.tolist() == [3.0, 0.0], msg


# ---- every engine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v4", "8k", "shared"])
def test_every_engine_is_served(lib, make_engine, kind):
    e = make_engine(**{"v4": dict(version=4), "8k": dict(rate=8000), "shared": dict(shared_gpu=True)}[kind])
    rng = np.random.default_rng(8)
    x, start, pieces, nw = pack_cases(rng, 5, 8)
    group = [0, 1, 0, 1, 2, 2, 2, 0]
    rc, msg, *got = raw_grouped(lib, e, x, start, group, 3)
    assert rc == 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, P.stats_grouped(x, start, group, 3))), msg
    rc, msg, got, _ = raw_packed(lib, e, x, start, batch_struct(5, 8, 2, dtype=B.F16), pieces, nw)
    assert rc == 0 and same(got, P.batch(x, start, pieces, nw, 5, 8, 2, dtype=B.F16)), msg


# ---- the Python faces -------------------------------------------------------------------------------------------------
@pytest.fixture()
def standin_lib(lib):
    """batch_pack reaches the planner through _ffi.lib(): the stand-in library for the length of a test"""
    saved = _ffi._lib
    _ffi._lib = lib
    yield lib
    _ffi._lib = saved


def test_batch_pack(standin_lib):
    from cutter_vad_amd import batch_pack
    start = np.concatenate([[0], np.cumsum(EXAMPLE_ROWS)])
    pieces, nw = batch_pack(start, 68, group=EXAMPLE_GROUPS)
    assert pieces.dtype == _ffi.BATCH_PIECE_DTYPE and nw == 5
    assert [(int(p["seg"]), int(p["row0"]), int(p["nrows"]), int(p["window"]), int(p["offset"])) for p in pieces] == EXAMPLE
    pieces, nw = batch_pack(start, 68, 2, EXAMPLE_GROUPS)
    assert pieces["offset"][:3].tolist() == [0, 8, 16] and nw == 5
    pieces, nw = batch_pack(start, 68)                            # one group: segment 5 joins window 1
    assert (pieces.tolist(), nw) == (piece_array(P.plan(start, 68)[0]).tolist(), P.plan(start, 68)[1]) and pieces["window"][4] == 1
    assert batch_pack([0], 8)[0].size == 0 and batch_pack([0], 8)[1] == 0 and batch_pack([4, 4, 4], 8)[1] == 0
    for bad in (dict(frames=6), dict(frames=0), dict(frames=8, gap=9), dict(frames=8, gap=-1), dict(frames=65540)):
        with pytest.raises(ConfigurationError):
            batch_pack(start, **bad)
    with pytest.raises(ConfigurationError):
        batch_pack([0, 5, 4], 8)
    with pytest.raises(ConfigurationError):
        batch_pack(start, 8, group=[0, 1])


def test_feature_batch_refusals():
    from cutter_vad_amd import FeatureBatch
    for bad in (dict(pack=True, frames=8, scope="segment"), dict(frames=8, scope="window"), dict(pack=True, frames=8, stride=4), dict(pack=True),
                dict(pack=True, frames=8, gap=9), dict(pack=True, frames=8, gap=-1), dict(frames=8, scope="utterance")):
        with pytest.raises(ConfigurationError):
            FeatureBatch(**bad).check()
    for good in (dict(), dict(scope="segment"), dict(scope="recording"), dict(pack=True, frames=8), dict(pack=True, frames=8, scope="window", gap=8),
                 dict(pack=True, frames=8, scope="recording")):
        FeatureBatch(**good).check()


def test_engine_methods(eng):
    rng = np.random.default_rng(14)
    x, start, pieces, nw = pack_cases(rng, 5, 68)
    lo = rng.uniform(-8, 0, nw).astype(np.float32)
    got = eng.mel_batch_packed(pieces, nw, dict(frames=68, deltas=1, dtype="bf16", layout="time"), lo=lo, shift=4.0, scale=0.25, features=x, start=start)
    want = P.batch(x, start, pieces, nw, 5, 68, 1, B.TIME, B.BF16, lo=lo, shift=np.full(5, 4, np.float32), scale=np.full(5, 0.25, np.float32))
    assert got.dtype == np.uint16 and got.shape == want.shape and got.tobytes() == want.tobytes()
    again = eng.mel_batch_packed(piece_array(pieces), nw, dict(frames=68, deltas=1, dtype="bf16", layout="time"), lo=lo, shift=4.0, scale=0.25, features=x,
                                 start=start)
    assert again.tobytes() == got.tobytes()
    out = np.full(want.size + 8, 0x5A5A, np.uint16)
    base = out.ctypes.data + (-out.ctypes.data) % 16
    shape = eng.mel_batch_packed_device(pieces, nw, dict(frames=68, deltas=1, dtype="bf16", layout="time"), base, want.nbytes, lo=lo, shift=4.0, scale=0.25,
                                        d_features=x.ctypes.data, rows=x.shape[0], n_mels=5, start=start)
    eng.synchronize()
    off = (base - out.ctypes.data) // 2
    assert shape == want.shape and out[off:off + want.size].tobytes() == want.tobytes() and (out[off + want.size:] == 0x5A5A).all()
    group = [0, 1, 0, 1, 2, 2, 2, 0]
    st = eng.mel_stats(x, start, group=group)
    ref = P.stats_grouped(x, start, group, 3)
    assert st["max"].tobytes() == ref[0].tobytes() and st["sum"].tobytes() == ref[1].tobytes() and st["sumsq"].tobytes() == ref[2].tobytes()
    st = eng.mel_stats(x, start, group=(group, 5), moments=False)
    assert set(st) == {"max"} and st["max"].shape == (5,) and st["max"][3] == -np.inf
    with pytest.raises(AudioProcessingError, match="group has an entry per segment"):
        eng.mel_stats(x, start, group=[0, 1])
    with pytest.raises(AudioProcessingError, match="pieces 0 and 1 overlap"):
        eng.mel_batch_packed([(0, 1, 0, 0, 0), (1, 1, 0, 0, 0)], 1, dict(frames=8), features=x, start=start)


@pytest.mark.parametrize("norm", ["whisper", "cmn", "cmvn"])
@pytest.mark.parametrize("scope", [None, "recording"])
def test_batch_recordings_packed_on_speech(eng, standin_lib, norm, scope):
    """against features_recordings and tests/pack_ref.py on the packaged speech (the stand-in's model is |first sample of a frame|)"""
    from cutter_vad_amd import FeatureBatch, MelSpec, batch_affine, batch_recordings, features_recordings
    pcm = _speech(60000)
    recs = [pcm[:12000], np.zeros(4000, np.float32), pcm[12000:]]
    cfg = _cfg(eng.frame_samples)
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    # cmvn: windows of 64 frames split the long segments, and a short one joins a remainder; else 128 frames hold two segments
    T, gap = 64 if norm == "cmvn" else 128, 2 if norm == "cmn" else 0
    fb = FeatureBatch(frames=T, norm=norm, deltas=1 if norm == "cmvn" else 0, dtype="f16" if norm == "whisper" else "f32",
                      layout="time" if norm == "cmn" else "channel", pad="feature", pad_value=-10.0, pack=True, gap=gap, scope=scope)
    got, index = batch_recordings(recs, spec, fb, cfg, engine=eng)
    feats = features_recordings(recs, spec, cfg, engine=eng)
    segs = [(i, a, b, f) for i, one in enumerate(feats) for a, b, f in one]
    assert len(segs) >= 3 and not feats[1]
    x = np.concatenate([f for *_, f in segs])
    start = np.concatenate([[0], np.cumsum([f.shape[0] for *_, f in segs])])
    group = [i for i, *_ in segs]
    pieces, nw = P.plan(start, T, gap, group)
    assert nw < len(pieces) and len(set(group)) == 2              # something was packed, and two recordings have speech
    assert norm != "cmvn" or any(r > 0 for _, _, r, _, _ in pieces) and any(r > 0 and o == 0 and pieces[k + 1][3] == w
                                                                             for k, (_, _, r, w, o) in enumerate(pieces[:-1]))
    parr = piece_array(pieces)
    if scope is None:                                             # the window's statistics: its pieces' rows
        st = P.stats_grouped(x, P.piece_bounds(start, pieces), parr["window"], nw)
        rows = np.concatenate([[0], np.cumsum(np.bincount(parr["window"], weights=parr["nrows"], minlength=nw))]).astype(np.int64)
        lo, sh, sc = batch_affine(dict(zip(("max", "sum", "sumsq"), st)), rows, norm)
    else:                                                         # the recording's, for each of its windows
        st = P.stats_grouped(x, start, group, 3)
        rows = np.concatenate([[0], np.cumsum(np.bincount(group, weights=np.diff(start), minlength=3))]).astype(np.int64)
        wg = np.zeros(nw, np.int64)
        wg[parr["window"]] = np.asarray(group)[parr["seg"]]
        lo, sh, sc = [a if a is None or np.ndim(a) == 0 else a[wg] for a in batch_affine(dict(zip(("max", "sum", "sumsq"), st)), rows, norm)]
    if norm == "whisper":
        sh, sc = np.full(6, 4, np.float32), np.full(6, 0.25, np.float32)
    want = P.batch(x, start, pieces, nw, 6, T, fb.deltas, _ffi.BATCH_LAYOUTS[fb.layout], _ffi.BATCH_DTYPES[fb.dtype], B.PAD_FEATURE, -10.0, lo, sh, sc)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert index == [(segs[s][0], 0, segs[s][1], segs[s][2], r, k, w, o) for s, k, r, w, o in pieces]
    if norm == "whisper" and scope is None:                       # Whisper's clamp is the window's: max - 8 over everything the window shows
        w0 = [p for p in pieces if p[3] == 0]
        top = max(segs[s][3][r:r + k].max() for s, k, r, *_ in w0)
        assert lo[0] == np.float32(top) - np.float32(8)


def test_batch_recordings_unpacked_is_unchanged_and_recording_scope(eng, standin_lib):
    from cutter_vad_amd import FeatureBatch, MelSpec, batch_affine, batch_recordings, features_recordings
    pcm = _speech(60000)
    recs = [pcm[:12000], np.zeros(4000, np.float32), pcm[12000:]]
    cfg = _cfg(eng.frame_samples)
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6)
    feats = features_recordings(recs, spec, cfg, engine=eng)
    segs = [(i, a, b, f) for i, one in enumerate(feats) for a, b, f in one]
    x = np.concatenate([f for *_, f in segs])
    start = np.concatenate([[0], np.cumsum([f.shape[0] for *_, f in segs])])
    win = [(k, min(32, f.shape[0] - r), r) for k, (*_, f) in enumerate(segs) for r in range(0, f.shape[0], 24)]
    # the call of before: per segment, the index of six entries
    fb = FeatureBatch(frames=32, stride=24, norm="cmvn", deltas=1, pad="feature", pad_value=-10.0)
    got, index = batch_recordings(recs, spec, fb, cfg, engine=eng)
    lo, sh, sc = batch_affine(dict(zip(("max", "sum", "sumsq"), B.stats(x, start))), start, "cmvn")
    assert got.tobytes() == B.batch(x, start, win, 6, 32, 1, pad_mode=B.PAD_FEATURE, pad_value=-10.0, lo=lo, shift=sh, scale=sc).tobytes()
    assert index == [(segs[k][0], 0, segs[k][1], segs[k][2], r, nr) for k, nr, r in win]
    same_again, _ = batch_recordings(recs, spec, FeatureBatch(frames=32, stride=24, norm="cmvn", deltas=1, pad="feature", pad_value=-10.0, scope="segment"),
                                     cfg, engine=eng)
    assert same_again.tobytes() == got.tobytes()
    # per recording, unpacked: the same windows, the recording's statistics for each of its segments
    group = np.array([i for i, *_ in segs])
    rows = np.concatenate([[0], np.cumsum(np.bincount(group, weights=np.diff(start), minlength=3))]).astype(np.int64)
    lo, sh, sc = batch_affine(dict(zip(("max", "sum", "sumsq"), P.stats_grouped(x, start, group, 3))), rows, "cmvn")
    got, index2 = batch_recordings(recs, spec, FeatureBatch(frames=32, stride=24, norm="cmvn", deltas=1, pad="feature", pad_value=-10.0, scope="recording"),
                                   cfg, engine=eng)
    assert got.tobytes() == B.batch(x, start, win, 6, 32, 1, pad_mode=B.PAD_FEATURE, pad_value=-10.0, shift=sh[group], scale=sc[group]).tobytes()
    assert index2 == index
    # no speech anywhere, and no recordings
    mono = np.zeros(4000, np.float32)
    got, index = batch_recordings([mono, mono], spec, FeatureBatch(frames=8, dtype="f16", pack=True), cfg, engine=eng)
    assert got.shape == (0, 6, 8) and got.dtype == np.float16 and index == []
    assert batch_recordings([], spec, FeatureBatch(frames=8, layout="time", deltas=2, pack=True), cfg, engine=eng)[0].shape == (0, 8, 18)

    class NoPack:
        sample_rate, frame_samples = 16000, 512
        mel = mel_batch = None

    with pytest.raises(ConfigurationError, match="pack=True needs an engine with mel_batch_packed"):
        batch_recordings([mono], spec, FeatureBatch(frames=8, pack=True), cfg, engine=NoPack())
    for bad in (dict(frames=8, pack=True, scope="segment"), dict(pack=True), dict(frames=8, pack=True, stride=4), dict(frames=8, scope="window")):
        with pytest.raises(ConfigurationError):
            batch_recordings([mono], spec, FeatureBatch(**bad), cfg, engine=eng)


# ---- the whole order of the checks (the helpers and the shapes: tests/test_mel_batch_host.py) ---------------------------------
def test_the_whole_order_of_a_packed_call(lib, make_engine):
    """vad_mel_batch_packed / _device, every reachable check: vad_mel_batch's order with nss and lo over the nw windows, per piece its
    segment, rows, window and offset, and behind the pieces the overlap of two in a window.  Left out, as they need more than
    2^31 - 1 elements: more than 2^31 - 1 segments, a segment of 2^31 rows or more, more than 2^31 - 1 windows or workgroups."""
    from tests.test_mel_batch_host import batch_order_walks
    batch_order_walks(lib, make_engine, True, [(5, 3, 0, 1, 2)],
                      [("piece 0 names segment 5 of 2", [(1, 3, 0, 1, 2)]),
                       (r"piece 0: rows 0 \.\. \+3 of segment 1, which has 2", [(1, 2, 0, 1, 2)]),
                       ("piece 0 names window 1 of 1", [(1, 2, 0, 0, 2)]),
                       ("piece 0: offset = 2 with 2 rows", [(1, 2, 0, 0, 0), (0, 1, 0, 0, 0)]),
                       ("pieces 0 and 1 overlap in window 0: frames 0 .. 3 and 0 .. 3", [(1, 2, 0, 0, 0)])])


def test_the_whole_order_of_a_grouped_stats_call(lib, make_engine):
    """vad_mel_stats_grouped / _device: vad_mel_stats's order with ngroups and group[i] behind the segments and the row bound of the
    sums per group.  Left out: the same checks as there."""
    from tests.test_mel_batch_host import stats_order_walks
    stats_order_walks(lib, make_engine, True)
