"""vad_scan_resample_cut and vad_scan_rate_mel on the host side: exports, vad_resample_cut_samples, every refusal with its message and
an untouched output, the resident rate block, n == 0, every kind of engine, values against tests/resample_cut_ref.py, the host and
device forms, the taps cache, vad_scan_rate_mel against the composition the header names, resample_taps, and the Python faces - the
real csrc/engine.cpp (checks, tables, operator pack) over the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp restates
the rule in plain float32, k ascending, over the unpacked view of the packed operator).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import mel_ref as MR
from tests import resample_cut_ref as R
from tests import standin
from tests.cut_ref import F32, FMT, INV, MIX, PCM16, RANGE, SENT16, SENT32, heard, untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_resample_cut_samples", "vad_scan_resample_cut", "vad_scan_resample_cut_device", "vad_scan_rate_mel", "vad_scan_rate_mel_device"]
UNSUPPORTED = _ffi.VAD_ERR_UNSUPPORTED
CHUNK = R.CHUNK
W = _ffi.VAD_RESAMPLE_CUT_WG_SAMPLES
_f32p = C.POINTER(C.c_float)


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


def _items(items):
    return (_ffi.CutItem * max(1, len(items)))(*[_ffi.CutItem(*map(int, it)) for it in items])


def _fp(a):
    return None if a is None else a.ctypes.data_as(_f32p)


def rsc(lib, eng, items, taps, audio, channels, fmt, sr, hop, out_fmt, out_samples, gains=None, ntaps=None, audio_samples=None, device=False,
        out=None):
    """vad_scan_resample_cut (or _device) -> (rc, message, out); items as tests/cut_ref.py's raw_cut; `out` is pre-filled"""
    if out is None:
        out = np.full(max(out_samples, 0) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)
    h = None if taps is None else np.ascontiguousarray(taps, np.float32)
    g = None if gains is None else np.ascontiguousarray(gains, np.float32)
    ptr, ns = None, audio_samples
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    head = (eng.handle, _items(items), len(items), _fp(g), _fp(h), (0 if h is None else h.size) if ntaps is None else ntaps, ptr, ns, channels,
            fmt, sr, hop, out_fmt)
    if device:
        rc = lib.vad_scan_resample_cut_device(*head, out.ctypes.data, out_samples, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_resample_cut(*head, out.ctypes.data, out_samples)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def rate_cut(lib, eng, items, audio, channels, fmt, sr, hop, out_fmt, out_samples, audio_samples=None, device=False):
    out = np.full(max(out_samples, 0) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)
    ptr, ns = None, audio_samples
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    head = (eng.handle, _items(items), len(items), ptr, ns, channels, fmt, sr, hop, -1.0, RANGE, out_fmt)
    if device:
        rc = lib.vad_scan_rate_cut_device(*head, out.ctypes.data, out_samples, None)
    else:
        rc = lib.vad_scan_rate_cut(*head, out.ctypes.data, out_samples)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def rate_mel(lib, eng, items, f, ops, taps, audio, channels, fmt, sr, hop, out_rows, device=False, ntaps=None):
    out = np.full((max(out_rows, 0) + 2, max(f["n_mels"], 1)), np.float32(-7.0), np.float32)
    m = MR.mel_struct(f)
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in ops]
    h = None if taps is None else np.ascontiguousarray(taps, np.float32)
    ptr, ns = None, 0
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr, ns = audio.ctypes.data, audio.size // max(channels, 1)
    head = (eng.handle, _items(items), len(items), C.byref(m), *[_fp(a) for a in keep], _fp(h),
            (0 if h is None else h.size) if ntaps is None else ntaps, ptr, ns, channels, fmt, sr, hop)
    if device:
        rc = lib.vad_scan_rate_mel_device(*head, out.ctypes.data, out_rows, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_rate_mel(*head, out.ctypes.data_as(_f32p), out_rows)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def exact_block(rng, kind, shape):
    """samples for which float32 is exact (resample_cut_ref.assert_exact): |s| <= 8 of 32768, or the G.711 codes that decode so"""
    if kind == "f32":
        return (rng.integers(-8, 9, shape) / 32768.0).astype(np.float32)
    if kind == "i16_32768":
        return rng.integers(-8, 9, shape).astype(np.int16)
    from tests import g711_ref as G
    table = G.table(kind).astype(np.int64)
    small = np.flatnonzero(np.abs(table) <= (64 if kind == "ulaw" else 120)).astype(np.uint8)
    return rng.choice(small, size=shape)


def exact_taps(rng, n):
    return rng.integers(-2, 3, n).astype(np.float32)


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
    for name in ("VAD_RESAMPLE_CUT_MAX_TAPS", "VAD_RESAMPLE_CUT_WG_SAMPLES"):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == getattr(_ffi, name)
    assert _ffi.VAD_RESAMPLE_CUT_MAX_TAPS == 511 and W % 16 == 0
    proto = lambda name: re.search(r"VAD_API\s+\w+\s+%s\((.*?)\);" % name, header, re.S).group(1)
    for name, k in (("vad_resample_cut_samples", 4), ("vad_scan_resample_cut", 15), ("vad_scan_resample_cut_device", 16), ("vad_scan_rate_mel", 17),
                    ("vad_scan_rate_mel_device", 18)):
        assert len(proto(name).split(",")) == len(_ffi.SIGNATURES[name][1]) == k, name
    from cutter_vad_amd import _build
    assert "scan_resample_cut.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    assert "resample_taps" in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, "resample_taps")


def test_sample_counts(lib, eng):
    table = {(8000, 3, 128): 1024, (24000, 3, 384): 1024, (48000, 3, 768): 1024,       # three chunks at the default hop
             (8000, 1, 128): 512, (24000, 1, 384): 512, (48000, 1, 768): 512,
             (8000, 2, 4): 520, (24000, 2, 4): 512, (48000, 2, 4): 512,                # 260 * 2; 772 * 2 / 3 = 514.67; 1540 / 3 = 513.33
             (24000, 2, 8): 516, (48000, 5, 100): 644, (8000, 1000, 256): 512000}      # 776 * 2 / 3 = 517.33; 1936 / 3 = 645.33
    for (sr, nf, hop), want in table.items():
        assert lib.vad_resample_cut_samples(eng.handle, nf, sr, hop) == want == R.s16(R.s_in(nf, sr, hop), sr), (sr, nf, hop)
        assert eng.resample_cut_samples(nf, sr, hop) == want
    assert eng.resample_cut_samples(3, 48000) == 1024                                  # the default hop: half a chunk
    for bad in ((0, 8000, 128), (-1, 8000, 128), (3, 8000, 0), (3, 8000, 6), (3, 8000, -128), (3, 44100, 128), (3, 0, 128), (3, 16000, 256),
                (1 << 62, 48000, 768)):
        assert lib.vad_resample_cut_samples(eng.handle, *bad) == -1, bad
    assert lib.vad_resample_cut_samples(None, 3, 8000, 128) == -1


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_have_a_status_the_functions_name_and_write_nothing(lib, make_engine):
    eng = make_engine()
    sr, chunk, hop = 24000, 768, 384
    x = np.zeros(8192, np.float32)                      # room for 20 chunks
    taps = np.ones(3, np.float32)
    ok = [(0, 0, 3, 0, 0), (1536, 1, 4, 1024, 0)]       # 1536 and 1920 input samples: 1024 and 1280 at 16 kHz
    total = 1024 + 1280
    for device in (False, True):
        for of in (PCM16, F32):
            rc, msg, out = rsc(lib, eng, ok, taps, x, 1, FMT["f32"], sr, hop, of, total, device=device)
            assert rc == _ffi.VAD_OK and (out[:total] == 0).all() and untouched(out[total:]), msg

    def refused(code, pattern, items, audio=x, channels=1, fmt=FMT["f32"], rate=sr, h=hop, out_fmt=PCM16, out_samples=total, named=True,
                t=taps, same=True, **kw):
        for device in (False, True):
            rc, msg, out = rsc(lib, eng, items, t, audio, channels, fmt, rate, h, out_fmt, out_samples, device=device, **kw)
            assert rc == code, (rc, msg)
            assert re.search(pattern, msg), msg
            if named:
                assert "vad_scan_resample_cut_device" in msg if device else re.search(r"vad_scan_resample_cut\b(?!_)", msg), msg
            assert untouched(out)                       # a refused call writes nothing
            if same and "gains" not in kw:
                # the block and item refusals are vad_scan_rate_cut's, in the same words
                rc2, msg2, _ = rate_cut(lib, eng, items, audio, channels, fmt, rate, h, out_fmt, 1 << 20, device=device,
                                        audio_samples=kw.get("audio_samples"))
                assert rc2 == code and msg2.replace("vad_scan_rate_cut", "vad_scan_resample_cut") == msg, (msg, msg2)

    for h in (0, 2, 6, -384, 386):
        refused(INV, "hop", ok, h=h)
    refused(INV, "out_fmt", ok, out_fmt=2)
    refused(INV, "channels = 3", ok, channels=3)
    refused(INV, "multiple of 4", [(2, 0, 3, 0, 0)])
    refused(INV, "first_frame", [(0, -1, 3, 0, 0)])
    refused(INV, "nframes", [(0, 0, 0, 0, 0)])
    rc, msg, out = rsc(lib, eng, [(0, 0, 20, 0, 0)], taps, x, 1, FMT["f32"], sr, hop, PCM16, R.s16(19 * hop + chunk, sr))
    assert rc == _ffi.VAD_OK, msg
    refused(INV, "leaves the audio block", [(0, 0, 21, 0, 0)], out_samples=1 << 16)
    refused(INV, "leaves the audio block", [(0, 1, 20, 0, 0)], out_samples=1 << 16)
    refused(INV, "leaves the audio block", [(7428, 0, 1, 0, 0)])       # 7428 + 768 > 8192
    refused(INV, "names channel 1 of 1", [(0, 0, 3, 0, 1)])
    refused(INV, "reserved", [(0, 0, 3, 0, 0, 5)])
    refused(INV, "2 GiB", ok, audio_samples=1 << 29)
    refused(INV, "2 GiB", ok, channels=2, audio_samples=1 << 28)
    refused(INV, "unknown frame format 9", ok, fmt=9, named=False)
    # out_sample counts 16 kHz samples here: the second segment's 1280 end at 2304
    refused(INV, r"out_sample = 2 \(\+1024 samples\)", [(0, 0, 3, 2, 0)], same=False)
    refused(INV, "out_sample", [(0, 0, 3, -4, 0)], same=False)
    refused(INV, r"out_sample = 1024 \(\+1280 samples\)", ok, out_samples=total - 4, same=False)
    refused(INV, "the output ranges of segments 0 and 1 overlap", [(0, 0, 3, 0, 0), (1536, 1, 4, 1020, 0)], same=False)
    # a gain, in vad_scan_cut_gain's words
    for bad, word in ((np.nan, "NaN"), (np.inf, "infinite"), (-np.inf, "infinite")):
        refused(INV, "segment 1: its gain is %s, a gain is a finite number" % word, ok, gains=[1.0, bad])
        arr = _items(ok)
        g = np.asarray([1.0, bad], np.float32)
        out = np.full(total, SENT16, np.int16)
        assert lib.vad_scan_cut_gain(eng.handle, arr, 2, _fp(g), x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, -1.0, RANGE, PCM16, out.ctypes.data,
                                     1 << 20) == INV
        assert lib.vad_last_error(eng.handle).decode().split(": ", 2)[2] == rsc(lib, eng, ok, taps, x, 1, FMT["f32"], sr, hop, PCM16, total,
                                                                               gains=g)[1].split(": ", 2)[2]
    # its own: the taps
    refused(INV, "null taps", ok, t=None, ntaps=3, same=False)
    for n in (0, 2, 64, -1, 513, 512):
        refused(INV, "ntaps = %d must be odd, from 1 to 511" % n, ok, t=np.ones(600, np.float32), ntaps=n, same=False)
    for bad, word in ((np.nan, "NaN"), (np.inf, "infinite")):
        t = np.ones(31, np.float32)
        t[[7, 20]] = bad
        refused(INV, r"taps\[7\] is %s, a tap is a finite number" % word, ok, t=t, same=False)
    rc, msg, out = rsc(lib, eng, ok, np.ones(511, np.float32), x, 1, FMT["f32"], sr, hop, PCM16, total)
    assert rc == _ffi.VAD_OK, msg
    # the rate: 16000 has nothing to resample
    for rate in (44100, 32000, 0, -8000, 16001, 16000):
        refused(UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: .*supported input rates are 8000, 24000, 48000" % rate, ok, rate=rate,
                same=False)
    # null buffers
    arr = _items(ok[:1])
    assert lib.vad_scan_resample_cut(eng.handle, arr, 1, None, _fp(taps), 3, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, PCM16, None, 2048) == INV
    assert "vad_scan_resample_cut: null buffer" in lib.vad_last_error(eng.handle).decode()
    assert lib.vad_scan_resample_cut_device(eng.handle, arr, 1, None, _fp(taps), 3, None, 8192, 1, FMT["f32"], sr, hop, PCM16, x.ctypes.data, 2048,
                                            None) == INV
    assert "vad_scan_resample_cut_device: null buffer" in lib.vad_last_error(eng.handle).decode()
    assert lib.vad_scan_resample_cut(None, arr, 1, None, _fp(taps), 3, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, PCM16, x.ctypes.data, 2048) == INV
    assert lib.vad_scan_resample_cut(eng.handle, None, 1, None, _fp(taps), 3, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, PCM16, x.ctypes.data,
                                     2048) == INV
    buf = np.full(4096 + 16, SENT16, np.int16)
    mis = buf[((16 - buf.ctypes.data % 16) % 16) // 2 + 2:][:4096]
    rc, msg, out = rsc(lib, eng, ok[:1], taps, x, 1, FMT["f32"], sr, hop, PCM16, 1024, device=True, out=mis)
    assert rc == INV and "vad_scan_resample_cut_device: the output must be 16-byte aligned" in msg and untouched(mis), msg
    # n == 0 is VAD_OK and touches nothing - behind the checks of the call's own arguments
    rc, msg, out = rsc(lib, eng, [], taps, x, 1, FMT["f32"], sr, hop, PCM16, 64)
    assert rc == _ffi.VAD_OK and untouched(out)
    rc, msg, out = rsc(lib, eng, [], np.ones(4, np.float32), x, 1, FMT["f32"], sr, hop, PCM16, 64)
    assert rc == INV and "ntaps" in msg


def test_every_kind_of_engine(lib, make_engine):
    x = (np.arange(8192) % 17 - 8).astype(np.float32) / np.float32(32768.0)
    taps = np.asarray([1, 2, 1], np.float32)
    for rate in R.RATES:
        hop = CHUNK[rate] // 2
        want = R.assert_exact(x[hop:hop + CHUNK[rate] + 2 * hop], taps, rate)
        for kw in (dict(), dict(version=4), dict(shared_gpu=True)):
            e = make_engine(**kw)
            for device in (False, True):
                rc, msg, out = rsc(lib, e, [(0, 1, 3, 0, 0)], taps, x, 1, FMT["f32"], rate, hop, F32, 1024, device=device)
                assert rc == _ffi.VAD_OK and out[:1024].tobytes() == want.tobytes() and untouched(out[1024:]), (kw, rate, msg)
    other = make_engine(rate=8000)
    for device in (False, True):
        for rate in (8000, 16000, 24000, 48000):
            rc, msg, out = rsc(lib, other, [(0, 0, 2, 0, 0)], taps, x, 1, FMT["f32"], rate, CHUNK.get(rate, 512) // 2, PCM16, 4096, device=device)
            assert rc == UNSUPPORTED and "8 kHz sub-model" in msg and "vad_scan_resample_cut" in msg and untouched(out), (rate, rc, msg)


# ---- the resident rate block ------------------------------------------------------------------------------------------
def test_the_resident_rate_block(lib, make_engine):
    eng = make_engine()
    sr, chunk = 8000, 256
    hop = chunk // 2
    rng = np.random.default_rng(3)
    recs = [exact_block(rng, "i16_32768", 3000), exact_block(rng, "i16_32768", 1500)]
    taps = exact_taps(rng, 7)
    slots = np.asarray(eng.open_streams(2))
    try:
        with eng.scan_session():
            eng.scan_segments(slots, recs, hop=hop, denoise=None, sample_rate=sr, i16_scale=32768)
            last = eng.last_scan
            off1 = int(last["offsets"][1])
            n0, n1 = R.s16(R.s_in(5, sr, hop), sr), R.s16(R.s_in(3, sr, hop), sr)
            items = [(0, 2, 5, 0, 0), (off1, 0, 3, n0, 0)]
            fmt = last["fmt"]
            rc, msg, got = rsc(lib, eng, items, taps, None, 1, fmt, sr, hop, F32, n0 + n1, audio_samples=last["samples"])
            assert rc == _ffi.VAD_OK, msg
            dec = lambda r: r.astype(np.float32) / np.float32(32768.0)
            assert got[:n0].tobytes() == R.assert_exact(dec(recs[0])[2 * hop:2 * hop + 4 * hop + chunk], taps, sr).tobytes()
            assert got[n0:n0 + n1].tobytes() == R.assert_exact(dec(recs[1])[:2 * hop + chunk], taps, sr).tobytes()
            # the Python face on the same block, and what names another block
            data, start = eng.resample_cut([(0, 2, 5), (off1, 0, 3)], sr, taps, hop=hop, out="f32")
            assert start.tolist() == [0, n0, n0 + n1] and data.tobytes() == got[:n0 + n1].tobytes()
            for kw, word in ((dict(sr=24000, hop=384), "sample rate 8000, not 24000"), (dict(fmt=FMT["f32"]), "frame format"),
                             (dict(channels=2), "channels"), (dict(audio_samples=last["samples"] + 4), "bytes")):
                a = dict(sr=sr, hop=hop, fmt=fmt, channels=1, audio_samples=last["samples"])
                a.update(kw)
                rc, msg, out = rsc(lib, eng, [(0, 0, 1, 0, 0 if a["channels"] == 1 else MIX)], taps, None, a["channels"], a["fmt"], a["sr"], a["hop"],
                                   F32, n0 + n1, audio_samples=a["audio_samples"])
                assert rc == INV and "audio = NULL" in msg and word in msg and untouched(out), msg
            # a scan at the engine's own rate leaves no rate block: vad_scan_rate_cut's words
            eng.scan_segments(slots, [r[:2048] for r in recs], hop=256, denoise=None, i16_scale=32768)
            n16 = eng.last_scan["samples"]
            rc, msg, out = rsc(lib, eng, [(0, 0, 1, 0, 0)], taps, None, 1, fmt, sr, hop, F32, n0 + n1, audio_samples=n16)
            rc2, msg2, _ = rate_cut(lib, eng, [(0, 0, 1, 0, 0)], None, 1, fmt, sr, hop, F32, n0 + n1, audio_samples=n16)
            assert rc == rc2 == INV and "holds no resident rate block" in msg and untouched(out)
            assert msg == msg2.replace("vad_scan_rate_cut:", "vad_scan_resample_cut:")
            # with an audio the call uploads it, and it becomes the resident rate block
            block = np.concatenate([recs[0], recs[1]])
            rc, msg, a1 = rsc(lib, eng, [(0, 2, 5, 0, 0)], taps, block, 1, fmt, sr, hop, F32, n0)
            rc2, msg2, a2 = rsc(lib, eng, [(0, 2, 5, 0, 0)], taps, None, 1, fmt, sr, hop, F32, n0, audio_samples=block.size)
            rc3, msg3, a3 = rate_cut(lib, eng, [(0, 2, 5, 0, 0)], None, 1, fmt, sr, hop, F32, n0, audio_samples=block.size)
            assert rc == rc2 == rc3 == _ffi.VAD_OK and a1.tobytes() == a2.tobytes() and a1[:n0].tobytes() == got[:n0].tobytes() and untouched(a1[n0:]), (msg, msg2, msg3)
            assert a3[:4 * hop + chunk].tobytes() == dec(recs[0])[2 * hop:6 * hop + chunk].tobytes()
    finally:
        for s in slots:
            eng.close_stream(int(s))


# ---- values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("kind", ("f32", "i16_32768", "ulaw", "alaw"))
def test_exact_cases_are_byte_equal(lib, eng, sr, kind):
    rng = np.random.default_rng(sr + len(kind))
    chunk = CHUNK[sr]
    hop = chunk // 2
    for two in (False, True):
        block = exact_block(rng, kind, (12 * chunk, 2) if two else 12 * chunk)
        block[:4] = block[-4:] = exact_block(rng, kind, block[:4].shape)
        for ntaps in (1, 3, 31):
            taps = exact_taps(rng, ntaps)
            taps[0] = taps[-1] = 2
            # the block's first sample, its last, one chunk, and the same samples twice
            items, at = [], 0
            for off, first, nf, ch in ((0, 0, 3, 0), (4 * chunk, 2, 13, 1 if two else 0), (0, 0, 1, MIX if two else 0), (4 * chunk, 2, 13, MIX if two else 0),
                                       (11 * chunk, 0, 1, 0), (0, 0, 23, 0)):
                items.append((off, first, nf, at, ch))
                at += R.s16(R.s_in(nf, sr, hop), sr) + 8
            gains = [1.0, -2.0, 0.5, 4.0, -0.25, 1.0]
            for of in (F32, PCM16):
                for g in (None, gains):
                    rc, msg, out = rsc(lib, eng, items, taps, block, 2 if two else 1, FMT[kind], sr, hop, of, at, gains=g)
                    rc2, msg2, dev = rsc(lib, eng, items, taps, block, 2 if two else 1, FMT[kind], sr, hop, of, at, gains=g, device=True)
                    assert rc == rc2 == _ffi.VAD_OK and out.tobytes() == dev.tobytes(), (msg, msg2)
                    for i, (off, first, nf, o, ch) in enumerate(items):
                        x = heard(block, kind, ch)[off + first * hop:off + first * hop + R.s_in(nf, sr, hop)]
                        y = R.gained(R.assert_exact(x, taps, sr), None if g is None else g[i])
                        want = y if of == F32 else R.pcm16(y)
                        assert out[o:o + want.size].tobytes() == want.tobytes(), (two, ntaps, of, i)
                        assert untouched(out[o + want.size:o + want.size + 8])


def test_saturation_at_both_ends_of_pcm16(lib, eng):
    x = np.zeros(2048, np.float32)
    x[100:110] = 0.75
    x[300:310] = -0.75
    x[500] = 1.0
    x[600] = -1.0
    rc, msg, out = rsc(lib, eng, [(0, 0, 7, 0, 0)], np.asarray([2.0], np.float32), x, 1, FMT["f32"], 8000, 128, PCM16, 2048, gains=[1.0])
    assert rc == _ffi.VAD_OK, msg
    assert (out[200:220:2] == 32767).all() and (out[600:620:2] == -32768).all() and out[1000] == 32767 and out[1200] == -32768
    assert not out[201:221:2].any()
    rc, msg, out = rsc(lib, eng, [(0, 0, 7, 0, 0)], np.asarray([0.5], np.float32), x, 1, FMT["f32"], 8000, 128, PCM16, 2048)
    assert rc == _ffi.VAD_OK and out[1000] == 16383 and out[1200] == -16383, msg


@pytest.mark.parametrize("sr", R.RATES)
def test_real_taps_stay_within_the_bound_and_zero_extend(lib, eng, sr):
    from cutter_vad_amd.scan import resample_taps
    rng = np.random.default_rng(sr)
    chunk = CHUNK[sr]
    hop = chunk // 2
    n = 6 * chunk
    tone = np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)
    block = np.clip(rng.integers(-32768, 32768, n) * 0.5 + 16000 * tone, -32768, 32767).astype(np.int16)
    x = block.astype(np.float32) / np.float32(32767.0)
    L, M = R.ratio(sr)
    for taps in (resample_taps(sr), resample_taps(sr, half_width=255 // max(L, M))[:511], np.ones(511, np.float32) * np.float32(0.01)):
        taps = taps[:taps.size - 1 + taps.size % 2]
        # loud audio right outside the segment: the reference zero-extends
        items = [(chunk, 1, 3, 0, 0)]
        rc, msg, out = rsc(lib, eng, items, taps, block, 1, FMT["i16_32767"], sr, hop, F32, 1024)
        assert rc == _ffi.VAD_OK, msg
        y, D = R.evaluate(x[chunk + hop:chunk + hop + 2 * hop + chunk], taps, sr)
        err = np.abs(out[:1024].astype(np.float64) - y)
        assert (err <= R.bound(taps.size, sr) * D).all(), (sr, taps.size, (err / np.maximum(D, 1e-300)).max() / R.U)
        assert out[:1024].tobytes() == R.evaluate_f32(x[chunk + hop:chunk + hop + 2 * hop + chunk], taps, sr).tobytes()    # (the stand-in's order)


def test_workgroup_edges_and_odd_hops(lib, eng):
    """S16 of W - 4, W, W + 4 and 2 W + 4 (at 8 kHz, where S16 = 2 S_in is a multiple of 8: W - 8 .. 2 W + 8) at hop 4, each from
    the longest segment with that count, so that S_in L / M is no integer wherever M = 3"""
    rng = np.random.default_rng(9)
    for sr in R.RATES:
        hop = 4
        L, M = R.ratio(sr)
        taps = exact_taps(rng, 31)
        odd = 0
        for want in ((W - 8, W, W + 8, 2 * W + 8) if sr == 8000 else (W - 4, W, W + 4, 2 * W + 4)):
            nf = next(k for k in range(1, 1 << 16) if R.s16(R.s_in(k + 1, sr, hop), sr) > want)
            S = R.s_in(nf, sr, hop)
            assert R.s16(S, sr) == want
            odd += (S * L) % M != 0
            block = exact_block(rng, "i16_32768", S)
            rc, msg, out = rsc(lib, eng, [(0, 0, nf, 0, 0)], taps, block, 1, FMT["i16_32768"], sr, hop, F32, want)
            y = R.assert_exact(block.astype(np.float32) / np.float32(32768.0), taps, sr)
            assert rc == _ffi.VAD_OK and y.size == want and out[:want].tobytes() == y.tobytes() and untouched(out[want:]), (sr, want, msg)
        assert sr == 8000 or odd > 0


def test_the_taps_cache(lib, make_engine):
    eng = make_engine()
    rng = np.random.default_rng(21)
    x = exact_block(rng, "f32", 8192)
    ta, tb = exact_taps(rng, 31), exact_taps(rng, 31)
    tb[3] = ta[3] + 1
    items = [(0, 1, 4, 0, 0)]
    outs = {}
    for name, sr, t in (("a", 24000, ta), ("b", 24000, tb), ("a2", 24000, ta), ("a3", 24000, ta.copy()), ("a8", 8000, ta), ("a24", 24000, ta),
                        ("short", 24000, ta[:29]), ("a4", 24000, ta)):
        hop = CHUNK[sr] // 2
        n = R.s16(R.s_in(4, sr, hop), sr)
        rc, msg, out = rsc(lib, eng, items, t, x, 1, FMT["f32"], sr, hop, F32, n)
        assert rc == _ffi.VAD_OK and out[:n].tobytes() == R.assert_exact(x[hop:hop + R.s_in(4, sr, hop)], t, sr).tobytes(), (name, msg)
        outs[name] = out[:n].tobytes()
    assert outs["a"] == outs["a2"] == outs["a3"] == outs["a24"] == outs["a4"] != outs["b"]


# ---- vad_scan_rate_mel ------------------------------------------------------------------------------------------------
GEO = dict(n_fft=64, hop=16, n_bins=33, n_mels=5)


def _compose(lib, eng, items, f, ops, taps, block, channels, fmt, sr, hop):
    """the header's recipe: vad_scan_resample_cut(F32) into a mono block at offsets o_i, then vad_scan_mel on it with the items
    (o_i, 0, (S16 - 512) / 4 + 1, 0), hop = 4, gate off"""
    at, packed = 0, []
    for off, first, nf, _, ch in items:
        packed.append((off, first, nf, at, ch))
        at += R.s16(R.s_in(nf, sr, hop), sr)
    rc, msg, mid = rsc(lib, eng, packed, taps, block, channels, fmt, sr, hop, F32, at)
    assert rc == _ffi.VAD_OK, msg
    mid = np.ascontiguousarray(mid[:at])
    second = [(p[3], 0, (R.s16(R.s_in(p[2], sr, hop), sr) - 512) // 4 + 1, 0, 0) for p in packed]
    m = MR.mel_struct(f)
    rows = sum(MR.nframes(f, R.s16(R.s_in(p[2], sr, hop), sr)) for p in packed)
    out = np.full((rows + 2, f["n_mels"]), np.float32(-7.0), np.float32)
    keep = [np.ascontiguousarray(a, np.float32) for a in ops]
    rc = lib.vad_scan_mel(eng.handle, _items(second), len(second), C.byref(m), *[_fp(a) for a in keep], mid.ctypes.data, at, 1, FMT["f32"], 4, -1.0,
                          _fp(out), rows)
    assert rc == _ffi.VAD_OK, lib.vad_last_error(eng.handle).decode()
    return out, rows


@pytest.mark.parametrize("sr", R.RATES)
def test_rate_mel_is_the_composition_byte_for_byte(lib, make_engine, sr):
    eng = make_engine()
    rng = np.random.default_rng(sr + 1)
    chunk = CHUNK[sr]
    hop = chunk // 2
    block = exact_block(rng, "i16_32768", (10 * chunk, 2))
    items = [(0, 0, 3, 0, 0), (4 * chunk, 1, 7, 0, MIX), (0, 0, 3, 0, 0), (9 * chunk, 0, 1, 0, 1)]
    for taps, ops, pad in ((exact_taps(rng, 31), MR.exact_operators(rng, 64, 33, 5), MR.REFLECT),
                           (exact_taps(rng, 3), MR.exact_operators(rng, 64, 33, 5), MR.NONE)):
        f = MR.fields(**GEO, pad=pad)
        want, rows = _compose(lib, eng, items, f, ops, taps, block, 2, FMT["i16_32768"], sr, hop)
        for device in (False, True):
            rc, msg, got = rate_mel(lib, eng, items, f, ops, taps, block, 2, FMT["i16_32768"], sr, hop, rows, device=device)
            assert rc == _ffi.VAD_OK and got.tobytes() == want.tobytes(), msg
        # ... and the exact values of the rule
        at = 0
        for off, first, nf, _, ch in items:
            x = heard(block, "i16_32768", ch)[off + first * hop:off + first * hop + R.s_in(nf, sr, hop)]
            E = MR.assert_exact(R.assert_exact(x, taps, sr), f, *ops)
            assert got[at:at + E.shape[0]].tobytes() == E.astype(np.float32).tobytes()
            at += E.shape[0]
        assert at == rows


def test_rate_mel_refusals(lib, make_engine):
    eng = make_engine()
    sr, hop = 48000, 768
    rng = np.random.default_rng(2)
    x = exact_block(rng, "f32", 8192)
    taps = exact_taps(rng, 3)
    ops = MR.exact_operators(rng, 64, 33, 5)
    f = MR.fields(**GEO, pad=MR.REFLECT)
    items = [(0, 0, 3, 0, 0)]
    rows = MR.nframes(f, 1024)

    def refused(code, pattern, device_too=True, **kw):
        a = dict(items=items, f=f, ops=ops, taps=taps, audio=x, channels=1, fmt=FMT["f32"], sr=sr, hop=hop, out_rows=rows)
        a.update(kw)
        for device in ((False, True) if device_too else (False,)):
            rc, msg, out = rate_mel(lib, eng, device=device, **a)
            assert rc == code and re.search(pattern, msg), (rc, msg)
            assert "vad_scan_rate_mel_device" in msg if device else re.search(r"vad_scan_rate_mel\b(?!_)", msg) or "unknown frame format" in msg, msg
            assert (out == np.float32(-7.0)).all()

    rc, msg, out = rate_mel(lib, eng, items, f, ops, taps, x, 1, FMT["f32"], sr, hop, rows)
    assert rc == _ffi.VAD_OK and (out[rows:] == np.float32(-7.0)).all(), msg
    refused(UNSUPPORTED, "supported input rates are 8000, 24000, 48000", sr=16000)
    refused(INV, "null taps", taps=None, ntaps=3)
    refused(INV, "ntaps = 4", taps=np.ones(4, np.float32))
    refused(INV, "leaves the audio block", items=[(0, 0, 30, 0, 0)])
    refused(INV, "hop", hop=6)
    refused(INV, "n_fft = 60", f=dict(f, n_fft=60))
    refused(INV, "null operator", ops=(None, ops[1], ops[2]))
    refused(INV, "null filters", ops=(ops[0], ops[1], None))
    refused(INV, "out_rows = -1", out_rows=-1)
    refused(INV, "out_rows = %d, the segments have %d rows" % (rows - 1, rows), out_rows=rows - 1)
    refused(INV, "segment 0 has 512 samples: reflect padding needs more than n_fft / 2 = 512", items=[(0, 0, 1, 0, 0)],
            f=MR.fields(1024, 16, 33, 5, pad=MR.REFLECT), ops=MR.exact_operators(rng, 1024, 33, 5))
    # the taps and the block come before vad_mel
    refused(INV, "ntaps", taps=np.ones(4, np.float32), f=dict(f, n_fft=60))
    refused(INV, "leaves the audio block", items=[(0, 0, 30, 0, 0)], f=dict(f, n_fft=60))
    # no item's out_sample is read
    rc, msg, again = rate_mel(lib, eng, [(0, 0, 3, -3, 0)], f, ops, taps, x, 1, FMT["f32"], sr, hop, rows)
    assert rc == _ffi.VAD_OK and again.tobytes() == out.tobytes(), msg
    rc, msg, out = rate_mel(lib, eng, [], f, ops, taps, x, 1, FMT["f32"], sr, hop, 0)
    assert rc == _ffi.VAD_OK and (out == np.float32(-7.0)).all()
    other = make_engine(rate=8000)
    rc, msg, out = rate_mel(lib, other, items, f, ops, taps, x, 1, FMT["f32"], sr, hop, rows)
    assert rc == UNSUPPORTED and "8 kHz sub-model" in msg


# ---- resample_taps ----------------------------------------------------------------------------------------------------
def test_resample_taps_properties():
    from cutter_vad_amd.scan import resample_taps
    assert [resample_taps(sr).size for sr in R.RATES] == [65, 97, 97]
    for sr in R.RATES:
        L, M = R.ratio(sr)
        h = resample_taps(sr)
        assert h.dtype == np.float32 and h.size % 2 == 1 and np.array_equal(h, h[::-1]) and abs(float(h.astype(np.float64).sum()) - L) < 1e-6
        C_ = (h.size - 1) // 2
        if L == 2:
            # both phases of the L = 2 designs sum to 1
            for ph in (0, 1):
                assert abs(float(h.astype(np.float64)[(C_ + ph) % 2::2].sum()) - 1.0) < 2e-5, (sr, ph)
        n = 40 * CHUNK[sr]
        t = np.arange(n) / sr
        x = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
        y, _ = R.evaluate(x, h, sr)
        mid = slice(y.size // 4, 3 * y.size // 4)
        rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
        assert abs(rms(y[mid]) / rms(x.astype(np.float64)) - 1.0) < 1e-3, (sr, rms(y[mid]) / rms(x))
        # ... and it IS a 1 kHz tone at 16 kHz
        ref = np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / 16000.0)
        assert np.abs(y[mid] - ref[mid]).max() < 2e-3
    x = np.sin(2 * np.pi * 12000.0 * np.arange(40 * 1536) / 48000.0).astype(np.float32)
    y, _ = R.evaluate(x, resample_taps(48000), 48000)
    assert float(np.sqrt(np.mean(np.square(y[y.size // 4:3 * y.size // 4])))) < 1e-4 * float(np.sqrt(np.mean(np.square(x.astype(np.float64)))))
    assert resample_taps(48000, half_width=85).size == 511 and resample_taps(8000, half_width=4, cutoff=3000.0).size == 17
    for bad in (dict(sample_rate=16000), dict(sample_rate=44100), dict(sample_rate=48000, half_width=86), dict(sample_rate=8000, cutoff=5000.0),
                dict(sample_rate=8000, cutoff=0.0), dict(sample_rate=8000, half_width=-1)):
        with pytest.raises(ConfigurationError):
            resample_taps(**bad)


# ---- the Python faces -------------------------------------------------------------------------------------------------
def _script(frame, s, amp=1.0, fill=0.125):
    """the stand-in's p = |first sample of the frame|: a recording whose frames have the probabilities `s`"""
    s = list(s) + [0.0] * (15 - len(s))
    x = np.full(frame * len(s) + 3, np.float32(fill), np.float32)
    x[:len(s) * frame:frame] = np.asarray(s, np.float32) * np.float32(amp)
    return x


def _cfg(frame=512, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5, voice_start_frame_count=2,
                     voice_end_frame_count=2, output_wav_sample_rate=8000, **kw)


def test_engine_resample_cut_and_mel_at_a_rate(eng):
    from cutter_vad_amd.scan import resample_taps
    sr, chunk = 24000, 768
    hop = chunk // 2
    rng = np.random.default_rng(5)
    block = exact_block(rng, "f32", (9 * chunk, 2))
    segs = [(0, 1, 3), (4 * chunk, 0, 2, 1), (0, 0, 1, 0)]
    taps = exact_taps(rng, 5)
    data, start = eng.resample_cut(segs, sr, taps, hop=hop, out="f32", audio=block)
    assert eng.last_scan is None and data.dtype == np.float32 and start.tolist() == [0, 1024, 1792, 2304]
    chans = (MIX, 1, 0)
    for i, sg in enumerate(segs):
        x = heard(block, "f32", chans[i])[sg[0] + sg[1] * hop:sg[0] + sg[1] * hop + R.s_in(sg[2], sr, hop)]
        assert data[start[i]:start[i + 1]].tobytes() == R.assert_exact(x, taps, sr).tobytes()
    pcm, _ = eng.resample_cut(segs, sr, taps, hop=hop, audio=block, gains=[2.0, 1.0, -1.0])
    assert pcm.dtype == np.int16 and pcm[:1024].tobytes() == R.pcm16(R.gained(data[:1024], 2.0)).tobytes()
    # the defaults: resample_taps and half a chunk
    d2, s2 = eng.resample_cut(segs, sr, out="f32", audio=block)
    d3, _ = eng.resample_cut(segs, sr, resample_taps(sr), hop=hop, out="f32", audio=block)
    assert d2.tobytes() == d3.tobytes() and s2.tolist() == start.tolist()
    out = np.zeros(2304 + 8, np.float32)
    assert eng.resample_cut_device(segs, sr, block.ctypes.data, block.shape[0], out.ctypes.data, out.size, taps, hop=hop, channels=2,
                                   out="f32").tolist() == start.tolist()
    eng.synchronize()
    assert out[:2304].tobytes() == data.tobytes() and not out[2304:].any()
    # mel at a rate: the rows of the 16 kHz signal
    f = MR.fields(**GEO, pad=MR.REFLECT)
    ops = MR.exact_operators(rng, 64, 33, 5)
    spec = (dict(n_fft=64, hop=16, pad="reflect", log="linear"), *ops)
    got, rstart = eng.mel(segs, spec, hop=hop, audio=block, sample_rate=sr, taps=taps)
    rows, want_start = MR.rows_of([data[start[i]:start[i + 1]] for i in range(3)], f, *ops, exact=True)
    assert got.tobytes() == rows.astype(np.float32).tobytes() and rstart.tolist() == want_start.tolist()
    dev = np.zeros((int(rstart[-1]) + 1, 5), np.float32)
    assert eng.mel_device(segs, spec, block.ctypes.data, block.shape[0], dev.ctypes.data, dev.shape[0], hop=hop, channels=2, sample_rate=sr,
                          taps=taps).tolist() == rstart.tolist()
    eng.synchronize()
    assert dev[:-1].tobytes() == got.tobytes() and not dev[-1].any()
    # sample_rate = the engine's is today's path
    b16 = exact_block(rng, "f32", 4096)
    a, sa = eng.mel([(0, 0, 3)], spec, hop=256, audio=b16, denoise=None, sample_rate=16000)
    b, sb = eng.mel([(0, 0, 3)], spec, hop=256, audio=b16, denoise=None)
    assert a.tobytes() == b.tobytes() and sa.tolist() == sb.tolist()
    with pytest.raises(Exception, match="follows a scan"):
        eng.resample_cut(segs, sr, taps, hop=hop)
    with pytest.raises(Exception, match="supported input rates are 8000, 24000, 48000"):
        eng.resample_cut([(0, 0, 1)], 16000, taps, hop=256, audio=b16)
    with pytest.raises(Exception, match="ntaps = 4"):
        eng.resample_cut(segs, sr, np.ones(4), hop=hop, audio=block)
    with pytest.raises(Exception, match="gains has 2 entries for 3 segments"):
        eng.resample_cut(segs, sr, taps, hop=hop, audio=block, gains=[1.0, 1.0])


def _corpus(chunk):
    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
    none = [0.0] * 9
    st = lambda l, r: np.ascontiguousarray(np.stack([_script(chunk, l), _script(chunk, r)], axis=1))
    return [_script(chunk, one), st(two, none), _script(chunk, none), st(none, one), _script(chunk, two, fill=0.0)]


# the stand-in's probability is |first sample of the RESAMPLED frame|: recordings that are constant over a chunk keep it
def _flat(chunk, s, fill=0.0):
    s = list(s) + [0.0] * (15 - len(s))
    x = np.repeat(np.asarray(s, np.float32), chunk)
    return np.concatenate([x, np.full(3, np.float32(fill), np.float32)])


def test_cut_recordings_resample_and_features_at_a_rate(make_engine):
    from cutter_vad_amd import MelSpec, cut_recordings, features_recordings, resample_taps
    from cutter_vad_amd.utils.wav_writer import WAVWriter
    eng = make_engine()
    cfg = _cfg(enable_denoising=False)
    n = 0
    for sr in (48000, 8000):
        chunk = CHUNK[sr]
        hop = chunk
        one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
        two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
        corpus = [_flat(chunk, one), np.ascontiguousarray(np.stack([_flat(chunk, two), _flat(chunk, [0.0] * 9)], axis=1)), _flat(chunk, [0.0] * 9)]
        plain = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=0, layout="range", wav=False, sample_rate=sr)
        assert any(plain)
        taps = resample_taps(sr)
        for kw in (dict(resample=True), dict(resample=taps), dict(resample=np.asarray([1.0], np.float32))):
            t = taps if kw["resample"] is True else kw["resample"]
            got = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=0, layout="range", wav=False, sample_rate=sr, **kw)
            assert [[r[:2] for r in rc] for rc in got] == [[r[:2] for r in rc] for rc in plain]           # ranges stay input-rate samples
            for x, rc in zip(corpus, got):
                h = x if x.ndim == 1 else x[:, 0]
                for a, b, pcm in rc:
                    y, D = R.evaluate(h[a:b], t, sr)
                    assert pcm.dtype == np.int16 and pcm.size == R.s16(b - a, sr)
                    # within the bound of the rule, then one multiply and the truncation
                    assert (np.abs(pcm - np.clip(y * 32767, -32768, 32767)) <= 1.0 + 32767 * R.bound(t.size, sr) * D + 1e-3).all()
                    n += 1
        wavs = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=0, layout="range", sample_rate=sr, resample=True)
        raw = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=0, layout="range", wav=False, sample_rate=sr, resample=True)
        for rw, rr in zip(wavs, raw):
            for (a, b, w), (_, _, pcm) in zip(rw, rr):
                assert w == WAVWriter(16000, 16, 1).header(2 * pcm.size) + pcm.tobytes()
        # normalize: the input-rate peak
        norm = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=0, layout="range", wav=False, sample_rate=sr, resample=np.asarray([1.0], np.float32),
                              normalize=0.5)
        for rc in norm:
            for a, b, pcm in rc:
                assert abs(int(np.abs(pcm).max()) - 16383) <= 1
        # features: the rows of the same 16 kHz signal
        spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6, log="linear")
        flds, a_, b_, w_ = spec.operators()
        f = MR.fields(64, 32, 33, 6, MR.REFLECT, MR.LINEAR)
        feats = features_recordings(corpus, spec, cfg, engine=eng, hop=hop, channel=0, sample_rate=sr, taps=taps)
        assert [[r[:2] for r in rc] for rc in feats] == [[r[:2] for r in rc] for rc in plain]
        for x, rc in zip(corpus, feats):
            h = x if x.ndim == 1 else x[:, 0]
            for a, b, feat in rc:
                y32 = R.evaluate_f32(h[a:b], taps, sr)                     # the stand-in's own order: the 16 kHz signal bit for bit
                E, D = MR.energies(y32, f, a_, b_, w_)
                assert feat.dtype == np.float32 and feat.shape == E.shape and (np.abs(feat - E) <= MR.bound(f) * D).all()
                n += 1
    assert n >= 10
    corpus = [_flat(1536, [0.0] * 2 + [0.9] * 5)]
    for kw, word in ((dict(sample_rate=48000, layout="frames", resample=True), "layout=\"range\""), (dict(layout="range", resample=True), "sample_rate="),
                     (dict(sample_rate=16000, layout="range", resample=True), "sample_rate="),
                     (dict(sample_rate=48000, layout="range", resample=True, keep_channels=True), "keep_channels=True")):
        with pytest.raises(ConfigurationError, match=word):
            cut_recordings(corpus, cfg, engine=eng, **kw)
    with pytest.raises(ConfigurationError, match="the spec is for 48000 Hz, the engine's blocks are at 16000 Hz"):
        features_recordings(corpus, MelSpec(48000, n_fft=64, hop=32, n_mels=6), cfg, engine=eng, sample_rate=48000)
    with pytest.raises(ConfigurationError, match="recordings at 8000, 16000, 24000 or 48000 Hz"):
        features_recordings(corpus, MelSpec(16000, n_fft=64, hop=32, n_mels=6), cfg, engine=eng, sample_rate=44100)


class _NoResample:
    """an engine object of another make: everything a rate scan, a cut and mel need, no resample_cut"""
    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        if name.startswith("resample_cut"):
            raise AttributeError(name)
        return getattr(self._e, name)


def test_an_engine_object_without_resample_cut_is_a_configuration_error(make_engine):
    from cutter_vad_amd import MelSpec, cut_recordings, features_recordings
    eng = make_engine()
    cfg = _cfg(enable_denoising=False)
    corpus = [_flat(1536, [0.0] * 2 + [0.9] * 5 + [0.0] * 4)]
    bare = _NoResample(eng)
    assert cut_recordings(corpus, cfg, engine=bare, hop=1536, layout="range", wav=False, sample_rate=48000) != [[]]
    opened = eng.info()["open_streams"]
    with pytest.raises(ConfigurationError, match="cut_recordings: resample= needs an engine with resample_cut.*_NoResample has none"):
        cut_recordings(corpus, cfg, engine=bare, hop=1536, layout="range", sample_rate=48000, resample=True)
    with pytest.raises(ConfigurationError, match="features_recordings: sample_rate= needs an engine with resample_cut.*_NoResample has none"):
        features_recordings(corpus, MelSpec(16000), cfg, engine=bare, hop=1536, sample_rate=48000)
    assert eng.info()["open_streams"] == opened


# ---- the order of the checks ------------------------------------------------------------------------------------------
def test_a_resample_cut_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_scan_resample_cut's checks is behaviour: the rate, the taps, frame format, channels, out_fmt, hop, per
    segment its place in the block, its out_sample and its gain, the output pointer, and last the device form's two alignments.
    Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    far = [(0, 0, 1, 0, 0, 0), (0, 2, 2, 514, 0, 0)]
    odd = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 514, 0, 0)]
    good = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 512, 0, 0)]            # 1536 and 1792 samples at 48 kHz: 512 and 596 at 16 kHz

    def call(device, sr_in, taps, ntaps, fmt, channels, out_fmt, hop, items, gains, out, audio):
        args = (eng.handle, RO.cut_items(items), len(items), RO.f32p(gains), RO.f32p(taps), ntaps, RO.addr(audio), RO.NS, channels, fmt, sr_in,
                hop, out_fmt, RO.addr(out), 1108)
        return lib.vad_scan_resample_cut_device(*args, None) if device else lib.vad_scan_resample_cut(*args)

    faults = dict(sr_in=44100, taps=None, ntaps=2, fmt=9, channels=3, out_fmt=2, hop=6, items=far, gains=RO.f32(1.0, float("inf")), out=None,
                  audio=RO.buf(4 * RO.NS, 2))
    RO.walk(lib, eng, call, faults, (
        (RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 48000),
        (INV, "null taps", "taps", RO.f32(0.25, float("nan"), 0.25)),
        (INV, "ntaps = 2 must be odd", "ntaps", 3),
        (INV, r"taps\[1\] is NaN", "taps", RO.f32(0.25, 0.5, 0.25)),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "out_fmt = 2 is neither", "out_fmt", F32),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", odd),
        (INV, r"segment 1: out_sample = 514 \(\+596 samples\)", "items", good),
        (INV, "segment 1: its gain is infinite", "gains", RO.f32(1.0, 0.5)),
        (INV, "vad_scan_resample_cut(_device)?: null buffer$", "out", RO.buf(4 * 1108, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(4 * 1108), RO.DEVICE)))


def test_a_rate_mel_with_several_faults_gets_the_first_refusal(lib, eng):
    """... and vad_scan_rate_mel's: the rate, the taps, frame format, channels, hop and the segments come before vad_mel's fields,
    the filters and out_rows - the other way round from vad_scan_mel - then out_rows against the rows, the output pointer and the
    device form's two alignments."""
    from tests import refusal_order as RO
    op_re, op_im, filters = RO.mel_ops()
    good, far = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 0, 0, 0)], [(0, 0, 1, 0, 0, 0), (0, 2, 2, 0, 0, 0)]      # 29 + 34 rows

    def call(device, sr_in, taps, ntaps, fmt, channels, hop, items, n_fft, floor, fil, out_rows, out, audio):
        m = RO.mel(n_fft=n_fft, floor=floor)
        args = (eng.handle, RO.cut_items(items), len(items), C.byref(m), RO.f32p(op_re), RO.f32p(op_im), RO.f32p(fil), RO.f32p(taps), ntaps,
                RO.addr(audio), RO.NS, channels, fmt, sr_in, hop)
        if device:
            return lib.vad_scan_rate_mel_device(*args, RO.addr(out), out_rows, None)
        return lib.vad_scan_rate_mel(*args, RO.f32p(out), out_rows)

    faults = dict(sr_in=44100, taps=None, ntaps=2, fmt=9, channels=3, hop=6, items=far, n_fft=100, floor=float("nan"), fil=None, out_rows=-1,
                  out=None, audio=RO.buf(4 * RO.NS, 2))
    RO.walk(lib, eng, call, faults, (
        (RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 48000),
        (INV, "null taps", "taps", RO.f32(0.25, float("nan"), 0.25)),
        (INV, "ntaps = 2 must be odd", "ntaps", 3),
        (INV, r"taps\[1\] is NaN", "taps", RO.f32(0.25, 0.5, 0.25)),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", good),
        (INV, "n_fft = 100 must be", "n_fft", 64),
        (INV, "floor = -?nan: a logarithm needs", "floor", 1e-5),
        (INV, "null filters", "fil", filters),
        (INV, "out_rows = -1 is negative", "out_rows", 0),
        (INV, "out_rows = 0, the segments have 63 rows", "out_rows", 63),
        (INV, "vad_scan_rate_mel(_device)?: null buffer$", "out", RO.buf(4 * 4 * 63, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(4 * 4 * 63), RO.DEVICE)))
