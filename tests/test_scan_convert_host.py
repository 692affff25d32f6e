"""vad_convert, vad_convert_device, vad_scan_convert_segments and their Python faces on the host side: exports, vad_convert_samples,
every refusal with its message and an untouched output, n == 0, every kind of engine, the operator pack against h[m M - k L + C], the
taps cache, convert_taps against resample_taps, values against tests/convert_ref.py, the definitional equality with vad_convert +
vad_scan_segments, the corpus functions and their ConfigurationErrors, every accepted rate and the covering set of
tests/convert_cases.py (the bodies tests/test_gpu_scan_convert_family.py runs on the GPU) - the real csrc/engine.cpp (checks, plan, operator pack) over
the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp restates the rule in plain float32, k ascending, over the
unpacked view of the packed operators).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import convert_cases as CC
from tests import convert_ref as CR
from tests import standin
from tests.cut_ref import FMT, INV, MIX, SENT32, heard, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_convert_samples", "vad_convert", "vad_convert_device", "vad_scan_convert_segments"]
UNSUPPORTED = _ffi.VAD_ERR_UNSUPPORTED
RATES = (44100, 22050, 11025, 32000, 12000, 96000, 8000, 48000)
THR = (0.3, 0.2, 0.8, 0.95, 2, 2)
_f32p = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)


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

    def make(version=5, rate=16000, max_streams=64, shared_gpu=False):
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


def ch_items(items):
    """(slot, sample_offset, nsamples, channel[, reserved]) each"""
    return (_ffi.ScanChItem * max(1, len(items)))(*[_ffi.ScanChItem(*map(int, tuple(it) + (0,) * (5 - len(it)))) for it in items])


def conv(lib, eng, items, taps, audio, channels, fmt, sr, out_samples, ntaps=None, audio_samples=None, device=False, out=None, offsets=True):
    """vad_convert (or _device: the stand-in's device memory is host memory) -> (rc, message, out, out_offset); `out` and
    `out_offset` are pre-filled with sentinels"""
    if out is None:
        out = np.full(min(max(out_samples, 0), 1 << 22) + 8, SENT32, np.float32)
    h = None if taps is None else np.ascontiguousarray(taps, np.float32)
    off = np.full(len(items) + 1, -5, np.int64)
    ptr, ns = None, audio_samples
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    head = (eng.handle, ch_items(items), len(items), ptr, ns, channels, fmt, sr, None if h is None else h.ctypes.data_as(_f32p),
            (0 if h is None else h.size) if ntaps is None else ntaps)
    tail = (out_samples, off.ctypes.data_as(_i64p) if offsets else None)
    if device:
        rc = lib.vad_convert_device(*head, out.ctypes.data, *tail, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_convert(*head, out.ctypes.data_as(_f32p), *tail)
    return rc, lib.vad_last_error(eng.handle).decode(), out, off


def scan_conv(lib, eng, items, taps, audio, channels, fmt, sr, hop, seg_cap=64, thr=-1.0, ntaps=None, nsegs=True, audio_samples=0):
    """vad_scan_convert_segments -> (rc, message, table[:count], count, out_offset)"""
    h = None if taps is None else np.ascontiguousarray(taps, np.float32)
    table = np.zeros(max(seg_cap, 1), _ffi.SEGMENT_DTYPE)
    table["item"] = -9
    count = C.c_int64(-3)
    off = np.full(len(items) + 1, -5, np.int64)
    ptr, ns = None, audio_samples
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr, ns = audio.ctypes.data, audio.size // max(channels, 1)
    rc = lib.vad_scan_convert_segments(eng.handle, ch_items(items), len(items), ptr, ns, channels, fmt, sr,
                                       None if h is None else h.ctypes.data_as(_f32p), (0 if h is None else h.size) if ntaps is None else ntaps,
                                       hop, thr, table.ctypes.data_as(C.POINTER(_ffi.Segment)), seg_cap, C.byref(count) if nsegs else None,
                                       off.ctypes.data_as(_i64p))
    return rc, lib.vad_last_error(eng.handle).decode(), table, count.value, off


def scan_segs(lib, eng, items, audio, hop, seg_cap=64, thr=-1.0):
    """vad_scan_segments on a mono float32 block"""
    table = np.zeros(max(seg_cap, 1), _ffi.SEGMENT_DTYPE)
    count = C.c_int64(-3)
    audio = np.ascontiguousarray(audio, np.float32)
    rc = lib.vad_scan_segments(eng.handle, ch_items(items), len(items), audio.ctypes.data, audio.size, 1, _ffi.VAD_FMT_F32, hop, thr,
                               table.ctypes.data_as(C.POINTER(_ffi.Segment)), seg_cap, C.byref(count))
    return rc, lib.vad_last_error(eng.handle).decode(), table, count.value


def exact_taps(rng, n, lo=-2):
    h = rng.integers(lo, 3, n).astype(np.float32)
    h[0] = h[-1] = 2
    return h


def want_exact(block, kind, ch, off, S_in, taps, sr, R=16000):
    """the item's float32 output through the int64 reference: samples in units of 2^-16 - of 1 / 2 for float32 blocks, which hold
    integers - so that the mix of two channels is a whole number of units too"""
    unit = 2.0 if kind == "f32" else 65536.0
    x = heard(block, kind, ch)[off:off + S_in].astype(np.float64) * unit
    xi = np.rint(x).astype(np.int64)
    assert np.array_equal(xi.astype(np.float64), x)
    y = CR.convert_exact(xi, np.asarray(taps, np.float64).astype(np.int64), sr, R)
    return (y.astype(np.float64) / unit).astype(np.float32)


def _check(out, off, block, kind, items, lens, taps, sr, R=16000):
    for i, it in enumerate(items):
        y = want_exact(block, kind, it[3], it[1], lens[i], taps, sr, R)
        a, b = int(off[i]), int(off[i + 1])
        assert b - a == (y.size + 3) & ~3
        assert out[a:a + y.size].tobytes() == y.tobytes(), (sr, kind, taps.size, i, lens[i], np.flatnonzero(out[a:a + y.size] != y)[:8])
        assert out[a + y.size:b].tobytes() == bytes(4 * (b - a - y.size)), (sr, i)       # the padding is +0.0
    assert untouched(out[int(off[-1]):])                                                  # the sentinel behind the output


# ---- the bodies that run on the stand-in here and on the GPU in tests/test_gpu_scan_convert_family.py -------------------
def exact_items(lib, eng, sr, taps, block, items, R=16000):
    """mono int16 items byte for byte against the int64 reference: values, +0.0 padding, the sentinel, out_offset == CR.layout"""
    lens = [it[2] for it in items]
    want_off = CR.layout(lens, sr, R)
    rc, msg, out, off = conv(lib, eng, items, taps, block, 1, FMT["i16_32768"], sr, int(want_off[-1]))
    assert rc == _ffi.VAD_OK and off.tolist() == want_off.tolist(), (sr, msg)
    _check(out, off, block, "i16_32768", items, lens, taps, sr, R)
    return out[:int(want_off[-1])].tobytes()


def every_rate_body(lib, eng, rates, R=16000):
    """one item of PI + 1 samples - one whole period and a period with a single input - and 2 L + 1 taps at each rate"""
    for sr in rates:
        assert CR.accepted(sr, R)
        rng = np.random.default_rng(sr)
        n = CR.period_inputs(sr, R) + 1
        exact_items(lib, eng, sr, exact_taps(rng, 2 * CR.ratio(sr, R)[0] + 1), rng.integers(-64, 65, n).astype(np.int16), [(0, 0, n, 0)], R)


def depth_body(lib, eng, sr):
    """the body of tests/test_gpu_scan_convert.py::test_rates_tap_counts_and_lengths_byte_for_byte, with the largest tap count at
    every rate"""
    rng = np.random.default_rng(sr)
    L, _ = CR.ratio(sr)
    for N in (1, 3, 2 * L + 1, CR.MAX_REACH * L - 1):
        block, items = CC.depth_block(rng, CC.depth_lengths(N, sr))
        assert block.size < 90000
        exact_items(lib, eng, sr, exact_taps(rng, N), block, items)


RATES_8K = {44100: (80, 441), 16000: (1, 2), 11025: (320, 441), 48000: (1, 6)}


def engine_8k_body(lib, e8):
    for sr, LM in RATES_8K.items():
        assert CR.ratio(sr, 8000) == LM and CR.accepted(sr, 8000)
        rng = np.random.default_rng(sr)
        PI = CR.period_inputs(sr, 8000)
        block, items = CC.depth_block(rng, [1, PI + 1, 3 * PI + 2])
        exact_items(lib, e8, sr, exact_taps(rng, 2 * LM[0] + 1), block, items, 8000)


def cache_body(lib, eng):
    """the same taps' bytes at the same L and another M, and at the same M and another L: each call has its own operators"""
    rng = np.random.default_rng(321)
    h = exact_taps(rng, 321)
    x = rng.integers(-64, 65, 3001).astype(np.int16)
    for a, b in ((44100, 63900), (15975, 31950)):
        (La, Ma), (Lb, Mb) = CR.ratio(a), CR.ratio(b)
        assert (La == Lb) != (Ma == Mb) and h.size <= CR.MAX_REACH * min(La, Lb)
        first = exact_items(lib, eng, a, h, x, [(0, 0, x.size, 0)])
        other = exact_items(lib, eng, b, h, x, [(0, 0, x.size, 0)])
        assert exact_items(lib, eng, a, h, x, [(0, 0, x.size, 0)]) == first != other


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
    for name in ("VAD_CONVERT_MAX_REACH", "VAD_CONVERT_MIN_RATE", "VAD_CONVERT_MAX_RATE", "VAD_CONVERT_MAX_PERIOD", "VAD_CONVERT_WG_SAMPLES"):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == getattr(_ffi, name)
    assert (_ffi.VAD_CONVERT_MAX_REACH, _ffi.VAD_CONVERT_MIN_RATE, _ffi.VAD_CONVERT_MAX_RATE, _ffi.VAD_CONVERT_MAX_PERIOD) == \
        (CR.MAX_REACH, CR.MIN_RATE, CR.MAX_RATE, CR.MAX_PERIOD) == (128, 4000, 192000, 640)
    proto = lambda name: re.search(r"VAD_API\s+\w+\s+%s\((.*?)\);" % name, header, re.S).group(1)
    for name, k in (("vad_convert_samples", 3), ("vad_convert", 13), ("vad_convert_device", 14), ("vad_scan_convert_segments", 16)):
        assert len(proto(name).split(",")) == len(_ffi.SIGNATURES[name][1]) == k, name
    from cutter_vad_amd import _build
    assert "scan_convert.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    for name in ("convert_taps", "convert_ratio", "input_ranges"):
        assert name in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, name)


def test_sample_counts_and_accepted_rates(lib, eng, make_engine):
    for sr in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        assert CR.accepted(sr), sr
        for S in (0, 1, 3, 440, 441, 442, 44100, 1323000, (1 << 31) - 1):
            assert lib.vad_convert_samples(eng.handle, S, sr) == CR.samples(S, sr), (sr, S)
    assert lib.vad_convert_samples(eng.handle, 44100, 44100) == 16000
    for sr in (16000, 3999, 192001, 0, -44100, 16001, 44101, 43904, 128200, 15999):
        assert not CR.accepted(sr) and lib.vad_convert_samples(eng.handle, 1000, sr) == -1, sr
    assert lib.vad_convert_samples(eng.handle, -1, 44100) == -1 and lib.vad_convert_samples(eng.handle, 1 << 31, 44100) == -1
    assert lib.vad_convert_samples(None, 100, 44100) == -1
    # the engine's rate is R: an 8 kHz engine converts 16 kHz recordings, and refuses its own rate
    e8 = make_engine(rate=8000)
    assert lib.vad_convert_samples(e8.handle, 44100, 44100) == 8000 and lib.vad_convert_samples(e8.handle, 100, 16000) == 50
    assert lib.vad_convert_samples(e8.handle, 100, 8000) == -1


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_every_refusal_names_itself_and_writes_nothing(lib, eng):
    rng = np.random.default_rng(1)
    block = rng.integers(-64, 65, 4000).astype(np.int16)
    h = exact_taps(rng, 31)
    fmt = FMT["i16_32768"]
    good = [(0, 0, 1000, 0), (0, 1000, 3000, 0)]
    total = int(CR.layout([1000, 3000], 44100)[-1])

    def refused(code, *words, **kw):
        args = dict(items=good, taps=h, audio=block, channels=1, fmt=fmt, sr=44100, out_samples=total)
        args.update(kw)
        for device in (False, True):
            rc, msg, out, off = conv(lib, eng, device=device, **args)
            who = "vad_convert_device" if device else "vad_convert"
            assert rc == code and untouched(out) and (off == -5).all(), (rc, msg)
            assert all(w in msg for w in words), msg
            assert who + ":" in msg or "unknown frame format" in msg, msg

    # the rate
    refused(UNSUPPORTED, "44101Hz", "L / M = 16000 / 44101", "4000", "192000", "640", sr=44101)
    refused(UNSUPPORTED, "L / M = 1 / 1", sr=16000)
    refused(UNSUPPORTED, "3000Hz", sr=3000)
    refused(UNSUPPORTED, "L / M = 125 / 343", sr=43904)            # lcm(125, 16) = 2000 outputs
    refused(UNSUPPORTED, "L / M = 80 / 641", sr=128200)            # M above 640
    refused(UNSUPPORTED, "L / M = 2 / 25", sr=200000)
    # the taps
    refused(INV, "null taps", taps=None)
    refused(INV, "ntaps = 30 must be odd", taps=np.ones(30, np.float32))
    refused(INV, "ntaps = 0 must be odd", taps=np.ones(3, np.float32), ntaps=0)
    refused(INV, "ntaps = 20481", "20480", taps=np.ones(20481, np.float32))          # 128 * 160
    refused(INV, "ntaps = 129", "from 1 to 128", taps=np.ones(129, np.float32), sr=48000)
    bad = h.copy()
    bad[7], bad[20] = np.nan, np.inf
    refused(INV, "taps[7] is NaN", taps=bad.copy())
    bad[7] = 1
    refused(INV, "taps[20] is infinite", taps=bad)
    # block and items, in vad_scan_channels's words
    refused(INV, "null buffer or bad count", audio_samples=-1)
    refused(INV, "unknown frame format 9", fmt=9)
    refused(INV, "channels = 3, the block holds 1 or 2 interleaved channels", channels=3)
    refused(INV, "exceed the 2 GiB one call may address", audio_samples=1 << 30)
    refused(INV, "recording 1 starts at sample 1001, not a multiple of 4", items=[(0, 0, 1000, 0), (0, 1001, 100, 0)])
    refused(INV, "recording 0 starts at sample -4", items=[(0, -4, 100, 0)])
    refused(INV, "recording 1 (samples 1000 .. +3001) leaves the audio block of 4000 samples", items=[(0, 0, 1000, 0), (0, 1000, 3001, 0)])
    refused(INV, "recording 0 (samples 0 .. +-1)", items=[(0, 0, -1, 0)])
    refused(INV, "recording 0 names channel 1 of 1", items=[(0, 0, 1000, 1)])
    refused(INV, "recording 1: reserved = 7 must be 0", items=[(0, 0, 1000, 0), (0, 1000, 3000, 0, 7)])
    # the output
    refused(INV, "out_samples = %d, the converted block has %d samples" % (total - 1, total), out_samples=total - 1)
    refused(INV, "null buffer", audio=None, audio_samples=4000)
    # 2 GiB of float32: items that name the same samples again and again (8000 Hz doubles them)
    big = np.zeros(1 << 20, np.uint8)
    refused(INV, "the converted block reaches 2 GiB of float32 at recording 255", items=[(0, 0, 1 << 20, 0)] * 300, audio=big, fmt=FMT["ulaw"],
            sr=8000, taps=np.ones(3, np.float32), out_samples=1 << 40)
    # a null output, and misaligned device pointers
    rc = lib.vad_convert(eng.handle, ch_items(good), 2, block.ctypes.data, 4000, 1, fmt, 44100, h.ctypes.data_as(_f32p), h.size, None, total, None)
    assert rc == INV and "vad_convert: null buffer" in lib.vad_last_error(eng.handle).decode()
    out = np.full(total + 16, SENT32, np.float32)
    rc = lib.vad_convert_device(eng.handle, ch_items(good), 2, block.ctypes.data, 4000, 1, fmt, 44100, h.ctypes.data_as(_f32p), h.size,
                                out.ctypes.data + 4, total, None, None)
    assert rc == INV and "the output must be 16-byte aligned" in lib.vad_last_error(eng.handle).decode() and untouched(out)
    rc = lib.vad_convert_device(eng.handle, ch_items(good[:1]), 1, block.ctypes.data + 2, 3000, 1, fmt, 44100, h.ctypes.data_as(_f32p), h.size,
                                out.ctypes.data, total, None, None)
    assert rc == INV and "the audio block must be 4-byte aligned" in lib.vad_last_error(eng.handle).decode() and untouched(out)
    assert lib.vad_convert(None, None, 0, None, 0, 1, fmt, 44100, None, 0, None, 0, None) == INV


def test_scan_convert_refusals_then_those_of_scan_segments(lib, eng, make_engine):
    rng = np.random.default_rng(2)
    block = rng.integers(-64, 65, 8000).astype(np.int16)
    h = exact_taps(rng, 31)
    fmt = FMT["i16_32768"]
    slots = eng.open_streams(2)
    try:
        good = [(slots[0], 0, 4000, 0), (slots[1], 4000, 4000, 0)]

        def refused(code, *words, **kw):
            args = dict(items=good, taps=h, audio=block, channels=1, fmt=fmt, sr=44100, hop=256)
            args.update(kw)
            rc, msg, table, count, off = scan_conv(lib, eng, **args)
            assert rc == code and count == -3 and (table["item"] == -9).all() and (off == -5).all(), (rc, msg)
            assert all(w in msg for w in words), msg

        refused(UNSUPPORTED, "vad_scan_convert_segments", "L / M = 16000 / 44101", sr=44101)
        refused(INV, "vad_scan_convert_segments: null taps", taps=None)
        refused(INV, "vad_scan_convert_segments: ntaps = 30 must be odd", taps=np.ones(30, np.float32))
        refused(INV, "vad_scan_convert_segments: recording 1 starts at sample 4001", items=[good[0], (slots[1], 4001, 100, 0)])
        refused(INV, "vad_scan_convert_segments: recording 0 names channel 1 of 1", items=[(slots[0], 0, 4000, 1)])
        # vad_scan_segments's own, under this function's name
        refused(INV, "vad_scan_convert_segments: hop = 6 must be a positive multiple of 4", hop=6)
        refused(INV, "vad_scan_convert_segments: seg_cap = -1", seg_cap=-1)
        refused(_ffi.VAD_ERR_BAD_SLOT, items=[(slots[0], 0, 4000, 0), (slots[0], 4000, 4000, 0)])
        refused(_ffi.VAD_ERR_BAD_SLOT, items=[(63, 0, 4000, 0)])
        refused(INV, "vad_scan_convert_segments: null buffer", audio=None, audio_samples=8000)
        rc, msg, table, count, off = scan_conv(lib, eng, good, h, block, 1, fmt, 44100, 256, nsegs=False)
        assert rc == INV and "vad_scan_convert_segments: null buffer" in msg and (off == -5).all()
        small = make_engine(max_streams=1)
        s1 = small.open_streams(1)
        rc, msg, *_ = scan_conv(lib, small, [(s1[0], 0, 4000, 0), (s1[0], 4000, 4000, 0)], h, block, 1, fmt, 44100, 256)
        assert rc == INV and "vad_scan_convert_segments: 2 recordings, max_streams = 1" in msg
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_n_zero_and_items_without_output(lib, eng):
    h = np.ones(3, np.float32)
    rc, msg, out, off = conv(lib, eng, [], h, None, 1, FMT["f32"], 44100, 0, audio_samples=0)
    assert rc == _ffi.VAD_OK and untouched(out) and off.tolist() == [0]
    rc, msg, table, count, off = scan_conv(lib, eng, [], h, None, 1, FMT["f32"], 44100, 256)
    assert rc == _ffi.VAD_OK and count == 0 and off.tolist() == [0]
    # S_in = 1 and 2 at 44.1 kHz have no output at all, 3 has one: nothing is launched for the first two
    block = np.arange(12, dtype=np.float32) + 1
    rc, msg, out, off = conv(lib, eng, [(0, 0, 1, 0), (0, 4, 2, 0), (0, 8, 3, 0)], h, block, 1, FMT["f32"], 44100, 4)
    assert rc == _ffi.VAD_OK and off.tolist() == [0, 0, 0, 4], msg
    assert out[:4].tolist() == [9.0 + 0.0, 0.0, 0.0, 0.0] and untouched(out[4:])     # y[0] = x[0] h[C]
    rc, msg, out, off = conv(lib, eng, [(0, 0, 1, 0), (0, 4, 2, 0)], h, block, 1, FMT["f32"], 44100, 0, offsets=False)
    assert rc == _ffi.VAD_OK and untouched(out)


@pytest.mark.parametrize("kind", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)])
def test_every_kind_of_engine_converts_and_only_v5_tiles_scan(lib, make_engine, kind):
    e = make_engine(**kind)
    R = kind.get("rate", 16000)
    rng = np.random.default_rng(3)
    x = rng.integers(-64, 65, 3000).astype(np.float32)
    h = exact_taps(rng, 5)
    rc, msg, out, off = conv(lib, e, [(0, 0, 3000, 0)], h, x, 1, FMT["f32"], 44100, CR.samples(3000, 44100, R) + 3)
    want = CR.convert_exact(x.astype(np.int64), h.astype(np.int64), 44100, R).astype(np.float32)
    assert rc == _ffi.VAD_OK and out[:want.size].tobytes() == want.tobytes(), msg
    slot = e.open_streams(1)
    rc, msg, *_ = scan_conv(lib, e, [(slot[0], 0, 3000, 0)], h, x, 1, FMT["f32"], 44100, 128)
    if kind.get("rate") == 8000:
        assert rc == _ffi.VAD_OK, msg
    else:
        assert rc == UNSUPPORTED and "vad_scan_convert_segments" in msg, msg


# ---- the operator and the cache ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,sr,R", [(160, 441, 44100, 16000), (320, 441, 22050, 16000), (640, 441, 11025, 16000), (1, 2, 32000, 16000),
                                     (4, 3, 12000, 16000)])
def test_the_packed_operator_applies_h_of_m_M_minus_k_L_plus_C(lib, eng, L, M, sr, R):
    """unit impulses through the engine's pack: x = delta_k gives y[m] = h[m M - k L + C] wherever that index is a tap, with h = 1, 2,
    3, ..: every entry of every row-tile's operator is read back, at its place"""
    assert CR.ratio(sr, R) == (L, M)
    PI = CR.period_inputs(sr, R)
    for N in (1, 3, 2 * L + 1):
        h = (np.arange(N) % 251 + 1).astype(np.float32)
        C_ = (N - 1) // 2
        S_in = 2 * PI + 7
        S_out = CR.samples(S_in, sr, R)
        for k in (0, 1, PI - 1, PI, PI + 5, S_in - 1):
            x = np.zeros(S_in, np.float32)
            x[k] = 1.0
            rc, msg, out, off = conv(lib, eng, [(0, 0, S_in, 0)], h, x, 1, FMT["f32"], sr, S_out + 3)
            assert rc == _ffi.VAD_OK, msg
            t = np.arange(S_out) * M - k * L + C_
            want = np.where((t >= 0) & (t < N), h[np.clip(t, 0, N - 1)], 0).astype(np.float32)
            assert np.array_equal(out[:S_out], want), (sr, N, k, np.flatnonzero(out[:S_out] != want)[:8])


def test_the_taps_cache_follows_rate_and_bytes(lib, eng):
    rng = np.random.default_rng(4)
    x = rng.integers(-64, 65, 2000).astype(np.float32)
    a, b = exact_taps(rng, 31), exact_taps(rng, 31)
    assert a.tobytes() != b.tobytes()

    def run(h, sr):
        rc, msg, out, _ = conv(lib, eng, [(0, 0, 2000, 0)], h, x, 1, FMT["f32"], sr, CR.samples(2000, sr) + 3)
        assert rc == _ffi.VAD_OK, msg
        want = CR.convert_exact(x.astype(np.int64), h.astype(np.int64), sr).astype(np.float32)
        assert out[:want.size].tobytes() == want.tobytes(), sr
        return out[:want.size].tobytes()

    first = run(a, 44100)
    assert run(a, 44100) == first and run(b, 44100) != first and run(a, 44100) == first
    run(a, 22050)                  # the same bytes at another ratio: packed again
    run(a, 44100)
    run(a[:29].copy(), 44100)      # a prefix of the cached taps
    # a refused call leaves the cache alone
    assert conv(lib, eng, [(0, 0, 2000, 0)], a, x, 1, FMT["f32"], 44101, 4000)[0] == UNSUPPORTED
    assert run(a, 44100) == first


def test_convert_taps_is_resample_taps_at_the_old_rates_and_sums_to_L():
    from cutter_vad_amd.scan import convert_ratio, convert_taps, input_ranges, resample_taps
    for sr in (8000, 24000, 48000):
        for kw in ({}, dict(half_width=5, beta=6.0), dict(cutoff=3000.0)):
            assert convert_taps(sr, **kw).tobytes() == resample_taps(sr, **kw).tobytes()
    for sr, hw in ((44100, 16), (22050, 16), (11025, 16), (32000, 16), (12000, 16), (96000, 10), (88200, 11)):
        L, M = convert_ratio(sr)
        h = convert_taps(sr, half_width=hw)
        assert (L, M) == CR.ratio(sr) and h.dtype == np.float32 and h.size == 2 * hw * max(L, M) + 1 <= 128 * L
        assert abs(float(h.astype(np.float64).sum()) - L) < 1e-3 * L and np.array_equal(h, h[::-1])
    assert convert_taps(16000, engine_rate=8000).size == 2 * 16 * 2 + 1
    with pytest.raises(ConfigurationError, match="half_width"):
        convert_taps(96000)                 # 2 * 16 * 6 + 1 = 193 > 128
    with pytest.raises(ConfigurationError, match="cutoff"):
        convert_taps(44100, cutoff=9000.0)
    for sr in (16000, 3000, 44101, 200000):
        with pytest.raises(ConfigurationError, match="L / M"):
            convert_taps(sr)
    assert input_ranges([(0, 160), (160, 16000, 0.5, 0.9), (15999, 16000)], 44100, 16000, 44000) == [(0, 441), (441, 44000, 0.5, 0.9), (44097, 44000)]


# ---- values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_values_formats_channels_and_layout_against_the_int64_reference(lib, eng, sr):
    rng = np.random.default_rng(sr)
    L, M = CR.ratio(sr)
    PI = CR.period_inputs(sr)
    h = exact_taps(rng, 2 * L + 1)
    lens = [1, 3, PI - 1, PI, PI + 1, 3 * PI + 2]
    for kind in ("f32", "i16_32768", "ulaw", "alaw"):
        for two in (False, True):
            offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
            shape = (int(offs[-2]) + lens[-1], 2) if two else int(offs[-2]) + lens[-1]
            if kind == "f32":
                block = rng.integers(-64, 65, shape).astype(np.float32)
            elif kind == "i16_32768":
                block = rng.integers(-64, 65, shape).astype(np.int16)
            else:
                block = rng.integers(0, 256, shape).astype(np.uint8)
            taps = h if kind in ("f32", "i16_32768") else exact_taps(rng, 3, lo=-1)
            chans = [0] * len(lens) if not two else [0, 1, MIX, 1, MIX, MIX]
            items = [(0, int(offs[i]), lens[i], chans[i]) for i in range(len(lens))]
            want_off = CR.layout(lens, sr)
            for device in (False, True):
                rc, msg, out, off = conv(lib, eng, items, taps, block, 2 if two else 1, FMT[kind], sr, int(want_off[-1]), device=device)
                assert rc == _ffi.VAD_OK and off.tolist() == want_off.tolist(), msg
                for i, it in enumerate(items):
                    y = want_exact(block, kind, chans[i], it[1], lens[i], taps, sr)
                    a, b = int(want_off[i]), int(want_off[i + 1])
                    assert out[a:a + y.size].tobytes() == y.tobytes(), (sr, kind, two, i, np.flatnonzero(out[a:a + y.size] != y)[:8])
                    assert out[a + y.size:b].tobytes() == bytes(4 * (b - a - y.size))        # the padding is +0.0
                assert untouched(out[int(want_off[-1]):])


def test_real_taps_stay_inside_the_bound_on_the_stand_in(lib, eng):
    from cutter_vad_amd.scan import convert_taps
    rng = np.random.default_rng(7)
    x = rng.standard_normal(2500).astype(np.float32)
    for sr in (44100, 22050):
        L, _ = CR.ratio(sr)
        h = convert_taps(sr)
        rc, msg, out, off = conv(lib, eng, [(0, 0, x.size, 0)], h, x, 1, FMT["f32"], sr, CR.samples(x.size, sr) + 3)
        y, D = CR.convert_f64(x, h, sr), CR.convert_f64(x, h, sr, absolute=True)
        assert rc == _ffi.VAD_OK and (np.abs(out[:y.size] - y) <= CR.bound(h.size, L) * CR.U * D).all(), msg


# ---- the definitional equality ----------------------------------------------------------------------------------------
def test_scan_convert_segments_is_convert_then_scan_segments(lib, make_engine):
    """the stand-in's model is p = |first sample of the frame|: loud first samples start segments, quiet ones end them"""
    rng = np.random.default_rng(8)
    sr, hop = 44100, 256
    h = np.ones(321, np.float32)                                    # every output sums two or three inputs
    lens = [9000, 30000, 441, 14000]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in lens])])
    block = np.zeros((int(offs[-1]), 2), np.float32)
    for i, n in enumerate(lens):
        env = (np.arange(n) // 4000) % 2 == 0                       # bursts of 4000 input samples
        block[offs[i]:offs[i] + n, 0] = np.where(env, 0.25, 0.0) * rng.integers(1, 3, n)
        block[offs[i]:offs[i] + n, 1] = 0.05 * rng.standard_normal(n)
    a, b = make_engine(), make_engine()
    sa, sb = a.open_streams(4), b.open_streams(4)
    for e, s in ((a, sa), (b, sb)):
        e.set_thresholds_many(s, THR)
    items = [(0, int(offs[i]), lens[i], (0, MIX, 1, 0)[i]) for i in range(4)]
    rc, msg, table, count, off = scan_conv(lib, a, [(int(sa[i]),) + it[1:] for i, it in enumerate(items)], h, block, 2, FMT["f32"], sr, hop)
    assert rc == _ffi.VAD_OK and count >= 2, (msg, count)
    total = int(CR.layout(lens, sr)[-1])
    rc, msg, out, off2 = conv(lib, b, items, h, block, 2, FMT["f32"], sr, total)
    assert rc == _ffi.VAD_OK and off.tolist() == off2.tolist() == CR.layout(lens, sr).tolist()
    second = [(int(sb[i]), int(off[i]), CR.samples(lens[i], sr), 0) for i in range(4)]
    rc, msg, table2, count2 = scan_segs(lib, b, second, out[:total], hop)
    assert rc == _ffi.VAD_OK and count2 == count and table[:count].tobytes() == table2[:count].tobytes(), msg
    # the resident per-frame results and the resident block: tails, resegment and a cut of audio = NULL
    from tests.cut_ref import F32, RANGE, raw_cut
    for e in (a, b):
        e._tail_items = 4
    assert a.scan_tails().tobytes() == b.scan_tails().tobytes()
    ta, tb = a.resegment([THR, (0.5, 0.4, 0.8, 0.95, 1, 1)]), b.resegment([THR, (0.5, 0.4, 0.8, 0.95, 1, 1)])
    assert [t.tobytes() for t in ta] == [t.tobytes() for t in tb] and ta[0].tobytes() == table[:count].tobytes()
    cuts = [(int(off[i]), 1, 3, 8 * i * 512, 0) for i in (0, 1, 3)]
    ra = raw_cut(lib, a, cuts, None, 1, FMT["f32"], hop, RANGE, F32, 32 * 512, audio_samples=total)
    rb = raw_cut(lib, b, cuts, None, 1, FMT["f32"], hop, RANGE, F32, 32 * 512, audio_samples=total)
    assert ra[0] == rb[0] == _ffi.VAD_OK and ra[2].tobytes() == rb[2].tobytes(), (ra[1], rb[1])
    i0 = int(off[1])
    assert ra[2][8 * 512:8 * 512 + 2 * hop + 512].tobytes() == out[i0 + hop:i0 + 3 * hop + 512].tobytes()
    # the streams were stepped alike
    assert a.info()["frames"] == b.info()["frames"] and a.info()["steps"] == b.info()["steps"]


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_engine_convert_and_scan_segments_convert(lib, make_engine):
    from cutter_vad_amd.scan import convert_taps
    rng = np.random.default_rng(9)
    e = make_engine()
    sr = 44100
    recs = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (5000, 441, 12345)]
    data, start = e.convert(recs, sr)
    h = convert_taps(sr)
    assert start.tolist() == CR.layout([r.size for r in recs], sr).tolist() and data.size == start[-1]
    assert [e.convert_samples(r.size, sr) for r in recs] == [CR.samples(r.size, sr) for r in recs]
    for i, r in enumerate(recs):
        x = r.astype(np.float32) / np.float32(32767.0)
        y, D = CR.convert_f64(x, h, sr), CR.convert_f64(x, h, sr, absolute=True)
        assert (np.abs(data[start[i]:start[i] + y.size] - y) <= CR.bound(h.size, 160) * CR.U * D).all()
    # two-channel recordings, a channel per recording, explicit taps, G.711
    two = [np.ascontiguousarray(rng.integers(-64, 65, (n, 2)).astype(np.int16)) for n in (900, 1000)]
    t3 = np.array([1, 2, 1], np.float32)
    data, start = e.convert(two, 22050, taps=t3, channel=[1, "mix"], i16_scale=32768)
    for i, ch in enumerate((1, MIX)):
        y = want_exact(two[i], "i16_32768", ch, 0, two[i].shape[0], t3, 22050)
        assert data[start[i]:start[i] + y.size].tobytes() == y.tobytes()
    # 96 kHz: the default design is the widest the reach holds
    d96, s96 = e.convert([recs[0]], 96000)
    assert s96.tolist() == [0, (CR.samples(5000, 96000) + 3) & ~3] and np.isfinite(d96).all()
    # convert_device on host memory (the stand-in's device memory)
    x = np.ascontiguousarray(recs[2].astype(np.float32))
    out = np.full(8192, SENT32, np.float32)
    st = e.convert_device([0], [x.size], sr, x.ctypes.data, x.size, out.ctypes.data, 8192)
    e.synchronize()
    want, _ = e.convert([x], sr)
    assert st.tolist() == [0, want.size] and out[:want.size].tobytes() == want.tobytes() and untouched(out[want.size:])
    # scan_segments(convert=...)
    slots = e.open_streams(3)
    e.set_thresholds_many(slots, THR)
    loud = [np.where((np.arange(n) // 6000) % 2 == 0, 20000, 0).astype(np.int16) for n in (30000, 20000, 50000)]
    with e.scan_session():
        table = e.scan_segments(slots, loud, sample_rate=sr, convert=True)
        last = dict(e.last_scan)
        tails = e.scan_tails()
    conv_data, conv_start = e.convert(loud, sr)
    assert len(table) >= 3 and last["channels"] == 1 and last["fmt"] == _ffi.VAD_FMT_F32 and "rate" not in last
    assert last["offsets"].tolist() == conv_start[:-1].tolist() and last["samples"] == conv_start[-1] and len(tails) == 3
    b = make_engine()
    sb = b.open_streams(3)
    b.set_thresholds_many(sb, THR)
    pieces = [conv_data[conv_start[i]:conv_start[i] + CR.samples(loud[i].size, sr)] for i in range(3)]
    assert b.scan_segments(sb, pieces, denoise=0.01).tobytes() == table.tobytes()
    # the ConfigurationErrors of the method
    for kw in (dict(sample_rate=None), dict(sample_rate=16000)):
        with pytest.raises(ConfigurationError, match="sample_rate"):
            e.scan_segments(slots, loud, convert=True, **kw)
    with pytest.raises(ConfigurationError, match="mono"):
        e.scan_segments(np.zeros((1, 2), np.int64), two[:1], sample_rate=sr, convert=True, channel="split")
    with pytest.raises(ConfigurationError, match="sample_rate"):
        e.convert(loud, 16000)


def test_corpus_functions_take_convert_and_keep_refusing_without_it(lib, make_engine):
    from cutter_vad_amd import VADConfig, cut_recordings, features_recordings, batch_recordings, render_recordings, scan_recordings, sweep_recordings
    from cutter_vad_amd.scan import FeatureBatch, MelSpec, input_ranges
    e = make_engine()
    sr = 44100
    cfg = VADConfig(vad_start_probability=0.3, vad_end_probability=0.2, voice_start_frame_count=2, voice_end_frame_count=2)
    loud = [np.where((np.arange(n) // 9000) % 2 == 0, 20000, 0).astype(np.int16) for n in (60000, 441, 45000)]
    # WITHOUT convert= the rate is refused as it always was
    for fn in (scan_recordings, cut_recordings, render_recordings):
        with pytest.raises(ConfigurationError, match="8000, 16000, 24000 or 48000"):
            fn(loud, cfg, engine=e, sample_rate=sr)
    with pytest.raises(ConfigurationError, match="8000, 16000, 24000 or 48000"):
        sweep_recordings(loud, [cfg], engine=e, sample_rate=sr)
    got = scan_recordings(loud, cfg, engine=e, sample_rate=sr, convert=True)
    data, start = e.convert(loud, sr)
    pieces = [data[start[i]:start[i] + e.convert_samples(loud[i].size, sr)] for i in range(3)]
    assert got == scan_recordings(pieces, cfg, engine=e) and len(got[0]) >= 2 and got[1] == []
    assert all(b <= p.size for rc, p in zip(got, pieces) for _, b in rc)
    back = input_ranges(got[0], sr, 16000, loud[0].size)
    assert all(0 <= a < b <= loud[0].size for a, b in back)
    full = scan_recordings(loud, cfg, engine=e, sample_rate=sr, convert=True, stats=True, open_end=True, levels=True)
    assert full == scan_recordings(pieces, cfg, engine=e, stats=True, open_end=True, levels=True)
    assert sweep_recordings(loud, [cfg, cfg], engine=e, sample_rate=sr, convert=True) == [got, got]
    for layout in ("frames", "range"):
        cut = cut_recordings(loud, cfg, engine=e, sample_rate=sr, convert=True, layout=layout, wav=False)
        ref = cut_recordings(pieces, cfg, engine=e, layout=layout, wav=False)
        assert [[(a, b, p.tobytes()) for a, b, p in rc] for rc in cut] == [[(a, b, p.tobytes()) for a, b, p in rc] for rc in ref]
    wav = cut_recordings(loud, cfg, engine=e, sample_rate=sr, convert=True)[0][0][2]
    assert int.from_bytes(wav[24:28], "little") == cfg.output_wav_sample_rate
    for mode in ("join", "mask"):
        r1 = render_recordings(loud, cfg, engine=e, sample_rate=sr, convert=True, mode=mode, wav=False)
        r2 = render_recordings(pieces, cfg, engine=e, mode=mode, wav=False)
        assert [(p.tobytes(), t) for p, t in r1] == [(p.tobytes(), t) for p, t in r2]
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=8)
    f1 = features_recordings(loud, spec, cfg, engine=e, sample_rate=sr, convert=True)
    f2 = features_recordings(pieces, spec, cfg, engine=e)
    assert [[(a, b, f.tobytes()) for a, b, f in rc] for rc in f1] == [[(a, b, f.tobytes()) for a, b, f in rc] for rc in f2] and f1[0]
    b1, i1 = batch_recordings(loud, spec, FeatureBatch(frames=16), cfg, engine=e, sample_rate=sr, convert=True)
    b2, i2 = batch_recordings(pieces, spec, FeatureBatch(frames=16), cfg, engine=e)
    assert b1.tobytes() == b2.tobytes() and i1 == i2 and b1.shape[0] > 0
    # taps of the caller's, and a two-channel corpus scanned on channel 1
    taps = np.full(321, 0.5, np.float32)
    stereo = [np.ascontiguousarray(np.stack([np.zeros_like(x), x], axis=1)) for x in loud]
    assert scan_recordings(stereo, cfg, engine=e, sample_rate=sr, convert=taps, channel=1) == scan_recordings(loud, cfg, engine=e, sample_rate=sr, convert=taps)
    assert cut_recordings(stereo, cfg, engine=e, sample_rate=sr, convert=taps, channel=1, wav=False)[0][0][2].size > 0
    # ConfigurationErrors
    with pytest.raises(ConfigurationError, match="needs sample_rate"):
        scan_recordings(loud, cfg, engine=e, convert=True)
    with pytest.raises(ConfigurationError, match="needs sample_rate"):
        cut_recordings(loud, cfg, engine=e, sample_rate=16000, convert=True)
    with pytest.raises(ConfigurationError, match="keep_channels"):
        cut_recordings(stereo, cfg, engine=e, sample_rate=sr, convert=True, keep_channels=True)
    with pytest.raises(ConfigurationError, match="keep_channels"):
        render_recordings(stereo, cfg, engine=e, sample_rate=sr, convert=True, keep_channels=True)
    with pytest.raises(ConfigurationError, match="resample="):
        cut_recordings(loud, cfg, engine=e, sample_rate=48000, convert=True, resample=True, layout="range")
    with pytest.raises(ConfigurationError, match="split"):
        scan_recordings(stereo, cfg, engine=e, sample_rate=sr, convert=True, channel="split")
    with pytest.raises(ConfigurationError, match="L / M"):
        scan_recordings(loud, cfg, engine=e, sample_rate=44101, convert=True)

    class Bare:
        sample_rate, frame_samples = 16000, 512
    for fn in (scan_recordings, cut_recordings):
        with pytest.raises(ConfigurationError, match="needs an engine with convert"):
            fn(loud, cfg, engine=Bare(), sample_rate=sr, convert=True)


# ---- the whole family of accepted rates (tests/convert_cases.py) -------------------------------------------------------
@pytest.mark.parametrize("L", CC.CLASSES)
def test_every_accepted_rate_of_a_class_byte_for_byte(lib, eng, L):
    """all 3 440 rates the argument check takes on a 16 kHz engine, class of L by class"""
    c = CC.cover_census()
    rates = CC.family()[L]
    assert c["family_size"] == 3440 and L in c["family_classes"] and rates and all(CR.ratio(sr)[0] == L for sr in rates)
    every_rate_body(lib, eng, rates)


@pytest.mark.parametrize("L", CC.CLASSES)
def test_default_taps_and_sample_counts_at_every_accepted_rate(lib, eng, L):
    for sr in CC.family()[L]:
        h = eng._convert_taps(sr, None)
        assert h.dtype == np.float32 and h.size % 2 == 1 and 1 <= h.size <= CR.MAX_REACH * L and np.isfinite(h).all(), (sr, h.size)
        for S in (0, 1, CR.ratio(sr)[1] - 1, CR.ratio(sr)[1], 100003):
            assert eng.convert_samples(S, sr) == S * L // CR.ratio(sr)[1] == CR.samples(S, sr), (sr, S)


@pytest.mark.parametrize("sr", CC.COVER)
def test_the_covering_set_in_depth(lib, eng, sr):
    CC.cover_census()
    depth_body(lib, eng, sr)


def test_an_8k_engine_converts_against_its_own_rate(lib, make_engine):
    assert sorted(CC.family(8000)) == [1, 2, 4, 5, 8, 10, 16, 20, 25, 32, 40, 50, 64, 80, 100, 160, 200, 320, 400]
    engine_8k_body(lib, make_engine(rate=8000))


def test_the_operator_cache_keys_on_L_and_on_M(lib, eng):
    cache_body(lib, eng)


def test_a_sample_of_refused_rates_launches_nothing(lib, eng, make_engine):
    """just outside 4 000 .. 192 000 Hz, the engine's own rate, a period above 640 outputs (L = 125) and M = 641 - and their accepted
    neighbours"""
    rng = np.random.default_rng(5)
    block = rng.integers(-64, 65, 2000).astype(np.int16)
    h = exact_taps(rng, 3)
    for sr, words in ((3999, "L / M = 16000 / 3999"), (192001, "L / M = 16000 / 192001"), (16000, "L / M = 1 / 1"), (4096, "L / M = 125 / 32"),
                      (128200, "L / M = 80 / 641"), (64100, "L / M = 160 / 641"), (10256, "L / M = 1000 / 641")):
        assert not CR.accepted(sr)
        for device in (False, True):
            rc, msg, out, off = conv(lib, eng, [(0, 0, 2000, 0)], h, block, 1, FMT["i16_32768"], sr, 1 << 16, device=device)
            assert rc == UNSUPPORTED and untouched(out) and (off == -5).all() and words in msg, (sr, rc, msg)
        assert lib.vad_convert_samples(eng.handle, 1000, sr) == -1 and eng.convert_samples(1000, sr) == -1
    for sr in (4000, 192000, 127800, 15999 + 26):
        assert CR.accepted(sr) == (lib.vad_convert_samples(eng.handle, 1000, sr) >= 0), sr
    assert CR.accepted(4000) and CR.accepted(192000) and CR.accepted(127800)
    e8 = make_engine(rate=8000)
    rc, msg, out, off = conv(lib, e8, [(0, 0, 2000, 0)], h, block, 1, FMT["i16_32768"], 8000, 1 << 16)
    assert rc == UNSUPPORTED and untouched(out) and (off == -5).all() and "L / M = 1 / 1" in msg, msg


# ---- the LDS pitch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,N", [(44100, 14113), (22050, 14113), (11025, 20479), (88200, 9703), (176400, 5001), (32000, 65), (12000, 129),
                                 (96000, 121), (8000, 65), (48000, 97), (192000, 121)])
def test_the_lds_pitch_keeps_a_fragment_in_64_banks(sr, N):
    """csrc/vad_layout.h restated: local sample j lies at float j + skew (j / PI), skew = (4 - PI) mod 64, so column p's sample c is at
    p (PI + skew) + c + skew (c / PI).  The 16 periods x 4 k of every B fragment the kernel reads - every row-tile, k-step and shift -
    fall into 64 different banks, except where the four k cross a period's end: there two lanes share a bank, in under 1 % of the
    k-steps of the 44.1 kHz family and nowhere at the rates whose period has a multiple of 4 inputs."""
    L, M = CR.ratio(sr)
    P, PI, K, C = CR.period(L), CR.period_inputs(sr), CR.reach(N, sr), (N - 1) // 2
    lead, skew = -(-C // L), (4 - PI % 64) % 64
    assert (PI + skew) % 64 == 4
    steps = crossing = 0
    for shift in range(lead, lead + 4):
        for r in range(P // 16):
            base = (16 * r * M - C) // L
            assert shift + base >= 0
            for n0 in range(0, K, 4):
                c = shift + base + n0 + np.arange(4)
                addr = (np.arange(16)[:, None] * (PI + skew) + c[None, :] + skew * (c[None, :] // PI)).reshape(-1)
                worst = np.bincount(addr % 64, minlength=64).max()
                steps += 1
                if c[0] // PI == c[3] // PI:
                    assert worst == 1, (sr, r, n0)
                else:
                    assert worst <= 2, (sr, r, n0)
                    crossing += worst == 2
    assert crossing * 100 < steps and (PI % 4 or crossing == 0), (sr, crossing, steps)


# ---- the order of the checks ------------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_convert's checks is behaviour: the rate, the taps, frame format, channels, per recording its place in the
    block and its channel, out_samples against the converted block, the output pointer, and last the device form's two alignments.
    Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    far = [(0, 0, 512, 0, 0), (0, 512, 2048, 1, 0)]              # (slot, sample_offset, nsamples, channel, reserved)
    right = [(0, 0, 512, 0, 0), (0, 512, 1024, 1, 0)]
    good = [(0, 0, 512, 0, 0), (0, 512, 1024, 0, 0)]
    offsets = np.full(3, -1, np.int64)

    def call(device, sr_in, taps, ntaps, fmt, channels, items, out_samples, out, audio):
        arr = (_ffi.ScanChItem * len(items))(*[_ffi.ScanChItem(*it) for it in items])
        args = (eng.handle, arr, len(items), RO.addr(audio), RO.NS, channels, fmt, sr_in, RO.f32p(taps), ntaps)
        if device:
            return lib.vad_convert_device(*args, RO.addr(out), out_samples, offsets.ctypes.data_as(C.POINTER(C.c_int64)), None)
        return lib.vad_convert(*args, RO.f32p(out), out_samples, offsets.ctypes.data_as(C.POINTER(C.c_int64)))

    faults = dict(sr_in=16000, taps=None, ntaps=2, fmt=9, channels=3, items=far, out_samples=0, out=None, audio=RO.buf(4 * RO.NS, 2))
    RO.walk(lib, eng, call, faults, (
        (RO.UNS, "from 16000Hz to 16000Hz", "sr_in", 48000),
        (INV, "null taps", "taps", RO.f32(0.25, float("nan"), 0.25)),
        (INV, "ntaps = 2 must be odd", "ntaps", 3),
        (INV, r"taps\[1\] is NaN", "taps", RO.f32(0.25, 0.5, 0.25)),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "recording 1 .*leaves the audio block of 2048 samples", "items", right),
        (INV, "recording 1 names channel 1 of 1", "items", good),
        (INV, "out_samples = 0, the converted block has 516 samples", "out_samples", 2048),
        (INV, "vad_convert(_device)?: null buffer$", "out", RO.buf(4 * 2048, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(4 * 2048), RO.DEVICE)))
    assert offsets.tolist() == [0, 172, 516]
