"""vad_scan_mel on the host side: exports, every refusal with its message and an untouched output, the resident-block rules, n == 0,
every kind of engine, values against tests/mel_ref.py (exact cases byte-equal, real operators within the derived bound), the host
and device forms, vad_mel_frames, and the Python faces (Engine.mel, MelSpec, mel_filterbank, features_recordings) - the real
csrc/engine.cpp (checks, tables, operator pack) over the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp restates
the rule in plain float32 loops over the unpacked view of the packed tables).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import mel_ref as R
from tests import standin
from tests.cut_ref import F32, FMT, INV, MIX, RANGE, gate, heard, raw_cut, values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_mel_frames", "vad_scan_mel", "vad_scan_mel_device"]
SENT = np.float32(-7.0)
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


def _items(items):
    return (_ffi.CutItem * max(1, len(items)))(*[_ffi.CutItem(*map(int, it)) for it in items])


def raw_mel(lib, eng, items, f, ops, audio, channels, fmt, hop, thr=-1.0, out_rows=None, audio_samples=None, device=False, out="own",
            mel="own", reserved=0):
    """vad_scan_mel (or _device) -> (rc, message, out [rows + 2, n_mels]); items as tests/cut_ref.py's raw_cut; `out` is pre-filled"""
    rows = 64 if out_rows is None else out_rows
    if isinstance(out, str):
        out = np.full((max(rows, 0) + 2, max(f["n_mels"], 1)), SENT, np.float32)
    m = R.mel_struct(f, reserved) if isinstance(mel, str) else mel
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in ops]
    ptrs = [None if a is None else a.ctypes.data_as(_f32p) for a in keep]
    ptr, ns = None, audio_samples
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    head = (eng.handle, _items(items), len(items), None if m is None else C.byref(m), *ptrs, ptr, ns, channels, fmt, hop, thr)
    if device:
        rc = lib.vad_scan_mel_device(*head, None if out is None else out.ctypes.data, rows, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_mel(*head, None if out is None else out.ctypes.data_as(_f32p), rows)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def untouched(out):
    return bool((out == SENT).all())


def _exact_block(rng, kind, shape):
    """samples for which float32 is exact (tests/mel_ref.py: assert_exact): |s| <= 8 of 32768, or the G.711 codes that decode so"""
    if kind == "f32":
        return (rng.integers(-8, 9, shape) / 32768.0).astype(np.float32)
    if kind == "i16_32768":
        return rng.integers(-8, 9, shape).astype(np.int16)
    from tests import g711_ref as G
    table = G.table(kind).astype(np.int64)
    small = np.flatnonzero(np.abs(table) <= (64 if kind == "ulaw" else 120)).astype(np.uint8)
    return rng.choice(small, size=shape)


EXACT_KINDS = ("f32", "i16_32768", "ulaw", "alaw")
GEO = dict(n_fft=64, hop=16, n_bins=33, n_mels=5)


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
    m = re.search(r"typedef struct vad_mel \{(.*?)\} vad_mel;", header, re.S)
    got = re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))
    assert got == [("int32_t", "n_fft"), ("int32_t", "hop"), ("int32_t", "n_bins"), ("int32_t", "n_mels"), ("int32_t", "pad"),
                   ("int32_t", "log"), ("float", "floor"), ("int32_t", "reserved")]
    assert [f[0] for f in _ffi.Mel._fields_] == [f[1] for f in got] and C.sizeof(_ffi.Mel) == 32
    for name, v in (("VAD_MEL_PAD_NONE", 0), ("VAD_MEL_PAD_REFLECT", 1), ("VAD_MEL_LINEAR", 0), ("VAD_MEL_LN", 1), ("VAD_MEL_LOG10", 2)):
        assert re.search(r"\b%s = %d\b" % (name, v), header) and getattr(_ffi, name) == v
    proto = lambda name: re.search(r"VAD_API\s+\w+\s+%s\((.*?)\);" % name, header, re.S).group(1)
    assert len(proto("vad_scan_mel").split(",")) == len(_ffi.SIGNATURES["vad_scan_mel"][1]) == 15
    assert len(proto("vad_scan_mel_device").split(",")) == len(_ffi.SIGNATURES["vad_scan_mel_device"][1]) == 16
    from cutter_vad_amd import _build
    assert "scan_mel.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    for name in ("MelSpec", "mel_filterbank", "features_recordings"):
        assert name in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, name)


def test_mel_frames(lib):
    def M(S, **kw):
        f = R.fields(**{**GEO, **kw})
        return lib.vad_mel_frames(C.byref(R.mel_struct(f)), S), f

    for S in (0, 1, 63, 64, 79, 80, 81, 512, 544, 1 << 31):
        got, f = M(S)
        assert got == R.nframes(f, S) == (0 if S < 64 else (S - 64) // 16 + 1), S
    for S in (33, 34, 63, 64, 65, 512):
        got, f = M(S, pad=R.REFLECT)
        assert got == R.nframes(f, S) == S // 16 + 1, S
    for S in (0, 1, 32):                                    # reflect padding needs S > n_fft / 2
        assert M(S, pad=R.REFLECT)[0] == -1
    assert M(-1)[0] == -1
    assert M(512, hop=64)[0] == 8 and M(512, hop=4)[0] == 113
    assert M(1024, n_fft=1024, hop=1024, n_bins=513)[0] == 1 and M(1023, n_fft=1024, hop=1024, n_bins=513)[0] == 0
    for bad in (dict(n_fft=48), dict(n_fft=1040, n_bins=1), dict(n_fft=72), dict(hop=0), dict(hop=6), dict(hop=68), dict(n_bins=0),
                dict(n_bins=34), dict(n_mels=0), dict(n_mels=129), dict(pad=2), dict(log=3), dict(log=R.LN, floor=0.0),
                dict(log=R.LOG10, floor=float("inf")), dict(log=R.LOG10, floor=float("nan")), dict(log=R.LN, floor=-1.0)):
        assert M(512, **bad)[0] == -1, bad
    assert M(512, floor=float("nan"))[0] == 29              # LINEAR does not read the floor
    f = R.fields(**GEO)
    assert lib.vad_mel_frames(C.byref(R.mel_struct(f, reserved=1)), 512) == -1
    assert lib.vad_mel_frames(None, 512) == -1


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    rng = np.random.default_rng(1)
    x = _exact_block(rng, "f32", (4096, 2))
    hop = 256
    f = R.fields(**GEO)
    ops = R.exact_operators(rng, 64, 33, 5)
    ok = [(0, 0, 3, 0, 0), (1024, 2, 2, 0, MIX)]            # out_sample is not read: both say 0
    want, start = R.rows_of([heard(x, "f32", 0)[:1024], heard(x, "f32", MIX)[1536:2304]], f, *ops, exact=True)
    assert start.tolist() == [0, 61, 106]
    for device in (False, True):
        rc, msg, out = raw_mel(lib, eng, ok, f, ops, x, 2, FMT["f32"], hop, out_rows=106, device=device)
        assert rc == _ffi.VAD_OK, msg
        assert out[:106].tobytes() == want.astype(np.float32).tobytes() and untouched(out[106:])
        rc, msg, out = raw_mel(lib, eng, ok, f, ops, x, 2, FMT["f32"], hop, out_rows=200, device=device)
        assert rc == _ffi.VAD_OK and out[:106].tobytes() == want.astype(np.float32).tobytes() and untouched(out[106:]), msg

    def refused(pattern, items=ok, audio=x, channels=2, fmt=FMT["f32"], hop=hop, f=f, ops=ops, **kw):
        for device in (False, True):
            rc, msg, out = raw_mel(lib, eng, items, f, ops, audio, channels, fmt, hop, device=device, **{"out_rows": 200, **kw})
            assert rc == INV, (rc, msg)
            assert re.search(pattern, msg), msg
            assert msg.startswith("Model prediction failed: ") and ("vad_scan_mel" in msg or "format" in msg), msg
            if out is not None:
                assert untouched(out)

    # the block and the items, in the cut's words
    for fmt in (5, -1, 9):
        refused("unknown frame format", fmt=fmt)
    for channels in (0, 3, -1):
        refused(r"channels = -?\d", channels=channels, audio_samples=4096)
    for h in (0, 2, 6, -256, 258):
        refused("hop = -?\\d+ must be a positive multiple of 4", hop=h)
    refused("starts at sample 2, not a multiple of 4", [(2, 0, 3, 0, 0)])
    refused("first_frame = -1", [(0, -1, 3, 0, 0)])
    refused("nframes = 0", [(0, 0, 0, 0, 0)])
    refused("leaves the audio block of 4096 samples", [(1024, 2, 11, 0, 0)])
    rc, msg, _ = raw_mel(lib, eng, [(1024, 2, 9, 0, 0)], f, ops, x, 2, FMT["f32"], hop, out_rows=200)
    assert rc == _ffi.VAD_OK, msg                           # ends ON the block's last sample
    refused("leaves the audio block", [(1 << 40, 0, 1, 0, 0)])
    refused("channel 2 of 2", [(0, 0, 3, 0, 2)])
    refused("channel -2 of 2", [(0, 0, 3, 0, -2)])
    refused("channel 1 of 1", [(0, 0, 3, 0, 1)], audio=x.reshape(-1), channels=1)
    refused("reserved = 7 must be 0", [(0, 0, 3, 0, 0, 7)])
    refused("2 GiB", audio_samples=1 << 28)
    refused("null buffer or bad count", audio_samples=-1)
    # the call's own arguments
    refused("null vad_mel", mel=None)
    for bad, pat in ((dict(n_fft=48), "n_fft = 48 must be a multiple of 16 from 64 to 1024"), (dict(n_fft=72), "n_fft = 72"),
                     (dict(n_fft=1040), "n_fft = 1040"), (dict(hop=0), "hop = 0 must be a multiple of 4 from 4 to n_fft = 64"),
                     (dict(hop=18), "hop = 18"), (dict(hop=68), "hop = 68"), (dict(n_bins=0), r"n_bins = 0 must be 1 \.\. n_fft / 2 \+ 1 = 33"),
                     (dict(n_bins=34), "n_bins = 34"), (dict(n_mels=0), r"n_mels = 0 must be 1 \.\. 128"), (dict(n_mels=129), "n_mels = 129"),
                     (dict(pad=2), "pad = 2 is neither"), (dict(pad=-1), "pad = -1"), (dict(log=3), "log = 3 is none of"),
                     (dict(log=R.LN, floor=0.0), "floor = 0: a logarithm needs a finite floor > 0"),
                     (dict(log=R.LOG10, floor=-1.0), "floor = -1"), (dict(log=R.LOG10, floor=float("inf")), "floor = inf"),
                     (dict(log=R.LN, floor=float("nan")), "floor = nan")):
        refused(pat, f={**f, **bad})
    refused(r"vad_mel\.reserved = 3 must be 0", reserved=3)
    refused("null operator", ops=(None, ops[1], ops[2]))
    refused("null operator", ops=(ops[0], None, ops[2]))
    refused("null filters", ops=(ops[0], ops[1], None))
    refused("null buffer", out=None)
    refused("out_rows = -1 is negative", out_rows=-1)
    refused("out_rows = 105, the segments have 106 rows", out_rows=105)
    refused("out_rows = 0, the segments have 106 rows", out_rows=0)
    # reflect padding needs S > n_fft / 2: S = 512 here
    big = R.exact_operators(rng, 1024, 513, 5)
    fr = R.fields(1024, 1024, 513, 5, pad=R.REFLECT)
    refused("segment 1 has 512 samples: reflect padding needs more than n_fft / 2 = 512", [(0, 0, 3, 0, 0), (0, 1, 1, 0, 1)], f=fr, ops=big)
    rc, msg, out = raw_mel(lib, eng, [(0, 4, 2, 0, 1)], fr, big, x, 2, FMT["f32"], 4, out_rows=2)      # S = 516 = n_fft / 2 + 4
    assert rc == _ffi.VAD_OK and out[:1].tobytes() == R.rows_of([heard(x, "f32", 1)[16:532]], fr, *big, exact=True)[0].astype(np.float32).tobytes(), msg
    # what a cut says about out_sample is no refusal here: negative, odd, overlapping
    rc, msg, out = raw_mel(lib, eng, [(0, 0, 3, -4, 0), (0, 0, 3, 2, 0)], f, ops, x, 2, FMT["f32"], hop, out_rows=122)
    assert rc == _ffi.VAD_OK and out[:61].tobytes() == out[61:122].tobytes() == want[:61].astype(np.float32).tobytes(), msg
    # the device form's pointers
    for device, pat in ((True, "null buffer"), (False, "no resident block|resident block has")):
        rc, msg, out = raw_mel(lib, eng, ok, f, ops, None, 2, FMT["f32"], hop, audio_samples=4095, device=device, out_rows=200)
        assert rc == INV and re.search(pat, msg) and untouched(out), msg
    base = np.zeros(2 * 4096 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 4096]
    rc, msg, out = raw_mel(lib, eng, [(0, 0, 3, 0, 0)], f, ops, odd, 2, FMT["ulaw"], hop, audio_samples=4096, device=True, out_rows=200)
    assert rc == INV and "vad_scan_mel_device: the audio block must be 8-byte aligned" in msg and untouched(out), msg
    buf = np.zeros(61 * 5 * 4 + 32, np.uint8)
    mis = buf[(4 - buf.ctypes.data) % 16:][:61 * 5 * 4].view(np.float32).reshape(61, 5)
    assert mis.ctypes.data % 16 == 4
    rc, msg, _ = raw_mel(lib, eng, [(0, 0, 3, 0, 0)], f, ops, x, 2, FMT["f32"], hop, device=True, out=mis, out_rows=61)
    assert rc == INV and "the output must be 16-byte aligned" in msg and not buf.any(), msg
    rc, msg, _ = raw_mel(lib, eng, [(0, 0, 3, 0, 0)], f, ops, x, 2, FMT["f32"], hop, device=False, out=mis, out_rows=61)
    assert rc == _ffi.VAD_OK and mis.tobytes() == want[:61].astype(np.float32).tobytes(), msg
    # no segments: fine, and nothing is written - but the call's own arguments are still checked
    for device in (False, True):
        rc, msg, out = raw_mel(lib, eng, [], f, ops, x, 2, FMT["f32"], hop, device=device)
        assert rc == _ffi.VAD_OK and untouched(out), msg
        rc, msg, out = raw_mel(lib, eng, [], f, ops, None, 2, FMT["f32"], hop, audio_samples=0, device=device, out=None, out_rows=0)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = raw_mel(lib, eng, [], f, ops, x, 2, FMT["f32"], 6, device=device)
        assert rc == INV and "hop = 6" in msg
        rc, msg, out = raw_mel(lib, eng, [], {**f, "n_mels": 0}, ops, x, 2, FMT["f32"], hop, device=device)
        assert rc == INV and "n_mels = 0" in msg
    assert lib.vad_scan_mel(None, None, 0, None, None, None, None, None, 0, 1, 0, 256, -1.0, None, 0) == INV
    # a segment without a frame is legal without padding and writes nothing; its neighbours' rows close up
    rc, msg, out = raw_mel(lib, eng, [(0, 0, 1, 0, 0), (0, 0, 3, 0, 0), (0, 1, 1, 0, 1)], R.fields(1024, 512, 513, 5), big, x, 2, FMT["f32"], hop,
                           out_rows=1)
    assert rc == _ffi.VAD_OK and untouched(out[1:]), msg
    assert out[:1].tobytes() == R.rows_of([heard(x, "f32", 0)[:1024]], R.fields(1024, 512, 513, 5), *big, exact=True)[0].astype(np.float32).tobytes()
    rc, msg, out = raw_mel(lib, eng, [(0, 0, 1, 0, 0)], R.fields(1024, 512, 513, 5), big, x, 2, FMT["f32"], hop, out_rows=0, out=None)
    assert rc == _ffi.VAD_OK, msg                           # no row at all: no buffer needed


# ---- the resident block -----------------------------------------------------------------------------------------------
def test_null_audio_names_the_resident_block_of_the_right_kind(lib, make_engine):
    eng = make_engine()
    hop = 256
    rng = np.random.default_rng(7)
    x = _exact_block(rng, "i16_32768", (6000, 2))
    items = [(0, 1, 4, 0, 1), (1024, 3, 2, 0, MIX)]
    i16 = FMT["i16_32768"]
    f = R.fields(**GEO, pad=R.REFLECT)
    ops = R.exact_operators(rng, 64, 33, 5)

    def null(ns=6000, channels=2, fmt=i16, hop=hop, its=items):
        return raw_mel(lib, eng, its, f, ops, None, channels, fmt, hop, thr=0.0001, audio_samples=ns, out_rows=200)

    rc, msg, out = null()
    assert rc == INV and "no resident block" in msg and "vad_scan_mel" in msg and untouched(out), msg
    rc, msg, want = raw_mel(lib, eng, items, f, ops, x, 2, i16, hop, thr=0.0001, out_rows=200)
    assert rc == _ffi.VAD_OK, msg
    rc, msg, got = null()
    assert rc == _ffi.VAD_OK and got.tobytes() == want.tobytes(), msg
    rc, msg, out = null(fmt=FMT["i16_32767"])
    assert rc == INV and "resident block has frame format 2, not 1" in msg and untouched(out), msg
    rc, msg, out = null(channels=1, ns=12000, its=[(0, 1, 4, 0, 0)])
    assert rc == INV and "resident block has 2 channels, not 1" in msg and untouched(out), msg
    rc, msg, out = null(ns=6008)
    assert rc == INV and "resident block has 24000 bytes, not the 24032 of 6008 samples" in msg and untouched(out), msg
    # the cut behind it reads the same block, and the rows are the rule applied to what it cuts
    rc, msg, pay = raw_cut(lib, eng, [(0, 1, 4, 0, 1), (1024, 3, 2, 1280, MIX)], None, 2, i16, hop, RANGE, F32, 2048, thr=0.0001, audio_samples=6000)
    assert rc == _ffi.VAD_OK, msg
    rows, start = R.rows_of([pay[:1280], pay[1280:2048]], f, *ops, exact=True)
    assert want[:start[-1]].tobytes() == rows.astype(np.float32).tobytes() and untouched(want[start[-1]:])
    # a rate block is none of this call's: the cut's message for the wrong kind of block
    rc, msg, _ = raw_cut(lib, eng, [(0, 0, 3, 0, 0)], x, 2, i16, 772, RANGE, F32, 3080, audio_samples=6000)
    lv = np.zeros(1, _ffi.LEVEL_DTYPE)
    rc = lib.vad_scan_levels(eng.handle, _items([(0, 0, 3, 0, 0)]), 1, x.ctypes.data, 6000, 2, i16, 48000, 772, -1.0, 0.95,
                             lv.ctypes.data_as(C.POINTER(_ffi.Level)))
    assert rc == _ffi.VAD_OK
    rc, msg, out = null()
    assert rc == INV and "no resident block" in msg and "vad_scan_mel" in msg and untouched(out), msg


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_computes_features(lib, make_engine, kw):
    other = make_engine(**kw)
    frame = other.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(3)
    x = _exact_block(rng, "alaw", (4096, 2))
    items = [(4, 1, 3, 0, 1), (4, 0, 2, 0, MIX)]
    f = R.fields(**GEO, pad=R.REFLECT, log=R.LOG10, floor=2.0 ** -20)
    ops = R.exact_operators(rng, 64, 33, 5)
    thr = 16.5 / 32768
    want = [gate(heard(x, "alaw", 1), thr)[4 + hop:4 + 3 * hop + frame], gate(heard(x, "alaw", MIX), thr)[4:4 + hop + frame]]
    rows, start = R.rows_of(want, f, *ops, exact=True)
    for device in (False, True):
        rc, msg, out = raw_mel(lib, other, items, f, ops, x, 2, FMT["alaw"], hop, thr=thr, device=device, out_rows=int(start[-1]))
        assert rc == _ffi.VAD_OK, (kw, msg)
        assert (np.abs(out[:start[-1]] - rows) <= R.log_tolerance(rows)).all() and untouched(out[start[-1]:])


# ---- values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_exact_cases_are_byte_equal(eng, kind, channels):
    frame, hop = eng.frame_samples, 32
    rng = np.random.default_rng(len(kind) + 10 * channels)
    x = _exact_block(rng, kind, (3000, 2) if channels == 2 else 3000)
    chans = (0, 1, "mix") if channels == 2 else (0,)
    # M = 29 .. 61 at hop 16; with hop 32 and n_fft 64: 15, 16, 17 and 35 frames - one short of a tile, a tile, one more, two and three
    segs = [(0, 0, 1, chans[0]), (4, 1, 2, chans[1 % len(chans)]), (1028, 3, 3, chans[2 % len(chans)]), (0, 0, 21, chans[0])]
    kw = dict(hop=hop, audio=x, law=kind if kind in ("ulaw", "alaw") else None, i16_scale=32768)
    thr = 2.5 / 32768 if kind in ("f32", "i16_32768") else 16.5 / 32768
    for denoise in (None, thr):
        for f in (R.fields(**GEO), R.fields(**GEO, pad=R.REFLECT), R.fields(64, 32, 33, 5), R.fields(64, 64, 33, 5), R.fields(64, 4, 17, 20)):
            ops = R.exact_operators(rng, f["n_fft"], f["n_bins"], f["n_mels"])
            got, start = eng.mel(segs, (f, *ops), denoise=denoise, **kw)
            want = []
            for sg in segs:
                a = sg[0] + sg[1] * hop
                want.append(gate(heard(x, kind, MIX if sg[3] == "mix" else sg[3]), denoise)[a:a + (sg[2] - 1) * hop + frame])
            rows, rstart = R.rows_of(want, f, *ops, exact=True)
            assert start.tolist() == rstart.tolist() and got.shape == rows.shape
            assert got.tobytes() == rows.astype(np.float32).tobytes(), (kind, channels, denoise, f)
            if f["hop"] == 32 and f["pad"] == R.NONE:
                assert np.diff(start).tolist() == [15, 16, 17, 35]
            cut, cstart = eng.cut(segs, layout="range", out="f32", denoise=denoise, **kw)
            assert [cut[cstart[i]:cstart[i + 1]].tobytes() for i in range(4)] == [np.asarray(w, np.float32).tobytes() for w in want]
        # the gate is live: it zeroed samples that were not zero
        assert denoise is None or any((w == 0).sum() > (u == 0).sum() for w, u in zip(want, want_plain(x, kind, segs, hop, frame)))
    # logs on exact energies: the argument is the reference's, bit for bit
    for log in (R.LN, R.LOG10):
        ops = R.exact_operators(rng, 64, 33, 5)
        lin = R.rows_of(want_plain(x, kind, segs, hop, frame), R.fields(**GEO, pad=R.REFLECT), *ops, exact=True)[0]
        f = R.fields(**GEO, pad=R.REFLECT, log=log, floor=2.0 ** round(np.log2(np.median(lin[lin > 0]))))      # about half of them
        got, _ = eng.mel(segs, (f, *ops), denoise=None, **kw)
        rows, _ = R.rows_of(want_plain(x, kind, segs, hop, frame), f, *ops, exact=True)
        assert (np.abs(got - rows) <= R.log_tolerance(rows)).all()
        assert (rows == R.logged(np.zeros(1), f)[0]).any() and (rows > rows.min()).any()      # the floor is live


def want_plain(x, kind, segs, hop, frame):
    return [heard(x, kind, MIX if sg[3] == "mix" else sg[3])[sg[0] + sg[1] * hop:sg[0] + sg[1] * hop + (sg[2] - 1) * hop + frame] for sg in segs]


@pytest.mark.parametrize("geo", [(400, 160, 80), (512, 128, 40), (64, 16, 12), (1024, 1024, 128)], ids=lambda g: "%d_%d_%d" % g)
def test_real_operators_within_the_derived_bound(eng, geo):
    """LINEAR on a speech-like signal under the gate; the logarithms on tests/mel_ref.py's noise_and_tone, where at most a tenth of
    the entries may fall outside the condition E >= 16 bound D - by the float64 reference alone, which is what `mask` is made of"""
    from cutter_vad_amd.scan import MelSpec
    n_fft, mhop, n_mels = geo
    segs = [(0, 0, 3), (1000, 2, 9 if n_fft == 1024 else 2)]
    hop = 256
    for pad, log in (("reflect", "linear"), ("none", "linear"), ("reflect", "log10"), ("none", "ln")):
        rng = np.random.default_rng(n_fft)
        x, thr = (R.speechlike(rng, 6000), 0.01) if log == "linear" else (R.noise_and_tone(rng, 6000), None)
        spec = MelSpec(16000, n_fft=n_fft, hop=mhop, n_mels=n_mels, pad=pad, log=log)
        flds, a, b, w = spec.operators()
        f = R.fields(n_fft, mhop, n_fft // 2 + 1, n_mels, _ffi.MEL_PADS[pad], _ffi.MEL_LOGS[log], 1e-10)
        got, start = eng.mel(segs, spec, hop=hop, audio=x, denoise=thr)
        at, inside = 0, []
        for sg in segs:
            s0 = sg[0] + sg[1] * hop
            v = gate(x, thr)[s0:s0 + (sg[2] - 1) * hop + eng.frame_samples]
            E, D = R.energies(v, f, a, b, w)
            g = got[at:at + E.shape[0]].astype(np.float64)
            at += E.shape[0]
            assert E.shape[0] == R.nframes(f, v.size) > 0
            if log == "linear":
                assert (np.abs(g - E) <= R.bound(f) * D).all(), (geo, pad, float((np.abs(g - E) / (R.U * D)).max()))
            else:
                mask, diff, tol = R.log_of_bounded(g, E, D, f)
                inside.append(mask.ravel())
                assert (diff[mask] <= tol[mask]).all(), (geo, pad, log)
        assert at == got.shape[0] == start[-1]
        assert log == "linear" or np.concatenate(inside).mean() >= 0.9, (geo, pad, log, np.concatenate(inside).mean())


def test_host_and_device_forms_and_the_operator_cache(lib, make_engine):
    eng = make_engine()
    rng = np.random.default_rng(11)
    x = _exact_block(rng, "f32", 5000)
    items = [(0, 0, 5, 0, 0), (1000, 1, 2, 0, 0)]
    f = R.fields(**GEO, pad=R.REFLECT)
    ops_a, ops_b = R.exact_operators(rng, 64, 33, 5), R.exact_operators(rng, 64, 33, 5)
    outs = {}
    for name, ops in (("a", ops_a), ("b", ops_b), ("a2", ops_a), ("a3", tuple(o.copy() for o in ops_a))):
        rc, msg, host = raw_mel(lib, eng, items, f, ops, x, 1, FMT["f32"], 256, out_rows=200)
        rc2, msg2, dev = raw_mel(lib, eng, items, f, ops, x, 1, FMT["f32"], 256, out_rows=200, device=True)
        assert rc == rc2 == _ffi.VAD_OK and host.tobytes() == dev.tobytes(), (msg, msg2)
        outs[name] = host
    assert outs["a"].tobytes() == outs["a2"].tobytes() == outs["a3"].tobytes() != outs["b"].tobytes()
    # the same arrays under another geometry of the same size are another operator
    g = R.fields(64, 16, 33, 5, pad=R.NONE)
    rc, msg, other = raw_mel(lib, eng, items, g, ops_a, x, 1, FMT["f32"], 256, out_rows=200)
    rows, start = R.rows_of([x[:1536], x[1256:2024]], g, *ops_a, exact=True)
    assert rc == _ffi.VAD_OK and other[:start[-1]].tobytes() == rows.astype(np.float32).tobytes(), msg


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_engine_mel_and_its_argument_errors(eng):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(5)
    recs = [_exact_block(rng, "f32", (frame + 5 * hop + 3, 2)), _exact_block(rng, "f32", (frame, 2))]
    f = R.fields(**GEO, pad=R.REFLECT)
    ops = R.exact_operators(rng, 64, 33, 5)
    spec = (dict(n_fft=64, hop=16, pad="reflect", log="linear"), *ops)
    slots = np.asarray(eng.open_streams(2))
    try:
        with eng.scan_session():
            eng.scan(slots, recs, hop=hop, denoise=None)
            last = eng.last_scan
            segs = [(0, 1, 3), (int(last["offsets"][1]), 0, 1, 1), (0, 0, 2, 0)]
            got, start = eng.mel(segs, spec, hop=hop, denoise=None)
            cut, cstart = eng.cut(segs, hop=hop, denoise=None, layout="range", out="f32")
        rows, rstart = R.rows_of([cut[cstart[i]:cstart[i + 1]] for i in range(3)], f, *ops, exact=True)
        assert got.dtype == np.float32 and got.tobytes() == rows.astype(np.float32).tobytes() and start.tolist() == rstart.tolist()
        block = np.zeros((last["samples"], 2), np.float32)
        block[:recs[0].shape[0]] = recs[0]
        block[int(last["offsets"][1]):] = recs[1]
        assert eng.mel(segs, (f, *ops), hop=hop, denoise=None, audio=block)[0].tobytes() == got.tobytes()
        assert eng.last_scan is None
        empty, s0 = eng.mel([], spec, hop=hop, audio=block)
        assert empty.shape == (0, 5) and s0.tolist() == [0]
        out = np.zeros((int(start[-1]) + 1, 5), np.float32)
        assert eng.mel_device(segs, spec, block.ctypes.data, block.shape[0], out.ctypes.data, out.shape[0], hop=hop, channels=2,
                              denoise=None).tolist() == start.tolist()
        eng.synchronize()
        assert out[:-1].tobytes() == got.tobytes() and not out[-1].any()
        assert eng.mel_frames(spec, 512) == 33 and eng.mel_frames((dict(n_fft=64, hop=16, pad="none"), *ops), 512) == 29
        with pytest.raises(Exception, match="follows a scan"):
            eng.mel(segs, spec, hop=hop)
        with pytest.raises(Exception, match="a segment is"):
            eng.mel([(0, 1)], spec, hop=hop, audio=block)
        with pytest.raises(Exception, match="leaves the audio block"):
            eng.mel([(0, 40, 3)], spec, hop=hop, audio=block)
        with pytest.raises(Exception, match=r"op_re / op_im are \[n_fft, n_bins\]"):
            eng.mel(segs, (dict(n_fft=128, hop=16), *ops), hop=hop, audio=block)
        with pytest.raises(Exception, match="pad is one of"):
            eng.mel(segs, (dict(n_fft=64, hop=16, pad="zero"), *ops), hop=hop, audio=block)
        with pytest.raises(Exception, match="hop = 6 must be a multiple of 4"):
            eng.mel(segs, (dict(n_fft=64, hop=6), *ops), hop=hop, audio=block)
    finally:
        for s in slots:
            eng.close_stream(int(s))


def _script(frame, s, amp=1.0, fill=0.125):
    """the stand-in's p = |first sample of the frame|: a recording whose frames have the probabilities `s`"""
    s = list(s) + [0.0] * (15 - len(s))
    x = np.full(frame * len(s) + 3, np.float32(fill), np.float32)
    x[:len(s) * frame:frame] = np.asarray(s, np.float32) * np.float32(amp)
    return x


def _cfg(frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5, voice_start_frame_count=2,
                     voice_end_frame_count=2, output_wav_sample_rate=8000, **kw)


def test_features_recordings(make_engine):
    from cutter_vad_amd import MelSpec, SegmentRefine, cut_recordings, features_recordings
    eng = make_engine()
    frame = hop = eng.frame_samples
    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
    none = [0.0] * 9
    tail = [0.0] * 10 + [0.8] * 5                      # stops inside speech
    st = lambda l, r: np.ascontiguousarray(np.stack([_script(frame, l), _script(frame, r)], axis=1))
    corpus = [_script(frame, one), st(two, none), _script(frame, none), st(none, one), _script(frame, two, fill=0.0), _script(frame, tail)]
    spec = MelSpec(16000, n_fft=64, hop=32, n_mels=6, log="linear")
    flds, a, b, w = spec.operators()
    f = R.fields(64, 32, 33, 6, R.REFLECT, R.LINEAR)
    cfg = _cfg(frame, enable_denoising=True)
    n = 0
    for channel in (0, "mix", "split"):
        for kw in (dict(), dict(open_end=True), dict(open_end=True, refine=SegmentRefine(pad_before=1, pad_after=1, max_frames=3))):
            got = features_recordings(corpus, spec, cfg, engine=eng, hop=hop, channel=channel, **kw)
            cuts = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout="range", wav=False, **kw)
            assert len(got) == len(cuts) == len(corpus)
            for x, rg, rc in zip(corpus, got, cuts):
                per = [(c, rg[c], rc[c]) for c in range(len(rg))] if channel == "split" else [(channel, rg, rc)]
                assert len(per) == (x.ndim if channel == "split" else 1)
                for c, g_, c_ in per:
                    assert [r[:2] for r in g_] == [r[:2] for r in c_]
                    h = gate(x if x.ndim == 1 else heard(x, "f32", MIX if c == "mix" else c), 0.01)
                    for s0, s1, feat in g_:
                        E, D = R.energies(h[s0:s1], f, a, b, w)
                        assert feat.dtype == np.float32 and feat.shape == E.shape == ((s1 - s0) // 32 + 1, 6)
                        assert (np.abs(feat - E) <= R.bound(f) * D).all()
                        n += 1
            if kw.get("open_end"):
                assert len(got[5][0] if channel == "split" else got[5]) >= 1
    assert n >= 20 and features_recordings([], spec, cfg, engine=eng) == []
    assert features_recordings(corpus[2:3], spec, cfg, engine=eng, hop=hop) == [[]]
    with pytest.raises(ConfigurationError, match="the spec is for 8000 Hz, the engine's blocks are at 16000 Hz"):
        features_recordings(corpus, MelSpec(8000, n_fft=64, hop=32, n_mels=6), cfg, engine=eng, hop=hop)
    with pytest.raises(ConfigurationError, match="channel is 'mix', 0, 1 or 'split'"):
        features_recordings(corpus, spec, cfg, engine=eng, hop=hop, channel=2)


class _NoMel:
    """an engine object of another make: everything a scan needs, no mel"""
    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        if name == "mel":
            raise AttributeError(name)
        return getattr(self._e, name)


def test_an_engine_object_without_mel_is_a_configuration_error(make_engine):
    from cutter_vad_amd import MelSpec, features_recordings, scan_recordings
    eng = make_engine()
    frame = eng.frame_samples
    cfg = _cfg(frame, enable_denoising=False)
    corpus = [_script(frame, [0.0] * 2 + [0.9] * 5 + [0.0] * 4)]
    bare = _NoMel(eng)
    assert scan_recordings(corpus, cfg, engine=bare, hop=frame) == scan_recordings(corpus, cfg, engine=eng, hop=frame) != [[]]
    opened = eng.info()["open_streams"]
    with pytest.raises(ConfigurationError, match="features_recordings needs an engine with mel.*_NoMel has none"):
        features_recordings(corpus, MelSpec(16000), cfg, engine=bare, hop=frame)
    assert eng.info()["open_streams"] == opened


# ---- MelSpec and mel_filterbank ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", [(400, 160), (512, 128), (64, 16)], ids=lambda g: "%d_%d" % g)
def test_melspec_operators_against_torch_stft(geo):
    import torch
    from cutter_vad_amd.scan import MelSpec
    n_fft, hop = geo
    spec = MelSpec(16000, n_fft=n_fft, hop=hop, n_mels=8)
    flds, a, b, w = spec.operators()
    assert flds == dict(n_fft=n_fft, hop=hop, n_bins=n_fft // 2 + 1, n_mels=8, pad="reflect", log="log10", floor=1e-10)
    assert a.dtype == b.dtype == w.dtype == np.float32 and a.shape == b.shape == (n_fft, n_fft // 2 + 1) and w.shape == (8, n_fft // 2 + 1)
    # the float64 operators, before the one rounding: rebuilt here from the docstring's formula
    n = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
    ang = 2 * np.pi * ((n[:, None] * np.arange(n_fft // 2 + 1)[None, :]) % n_fft) / n_fft
    a64, b64 = win[:, None] * np.cos(ang), -win[:, None] * np.sin(ang)
    assert np.array_equal(a, a64.astype(np.float32)) and np.array_equal(b, b64.astype(np.float32))
    x = np.random.default_rng(n_fft).standard_normal(4000)
    z = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64), center=True,
                   pad_mode="reflect", return_complex=True).numpy().T
    fr = R.frames(x, R.fields(n_fft, hop, n_fft // 2 + 1, 8, R.REFLECT))
    assert fr.shape[0] == z.shape[0] == 4000 // hop + 1
    P = (fr @ a64) ** 2 + (fr @ b64) ** 2
    assert np.abs(P - np.abs(z) ** 2).max() <= 1e-12 * (np.abs(z) ** 2).max()
    rect = MelSpec(16000, n_fft=n_fft, hop=hop, n_mels=8, window="rect").operators()
    assert np.array_equal(rect[1][:, 0], np.ones(n_fft, np.float32)) and not rect[2][:, 0].any()
    with pytest.raises(ConfigurationError, match="window is 'hann' or 'rect'"):
        MelSpec(16000, window="hamming").operators()
    with pytest.raises(ConfigurationError, match="pad is one of"):
        MelSpec(16000, pad="zero").operators()


@pytest.mark.parametrize("args", [(16000, 400, 80, 0.0, None), (16000, 400, 128, 0.0, None), (16000, 512, 40, 20.0, 7600.0), (8000, 256, 23, 100.0, 3800.0)],
                         ids=lambda a: "%d_%d_%d" % a[:3])
def test_mel_filterbank_properties(args):
    from cutter_vad_amd.scan import _hz_to_mel, _mel_to_hz, mel_filterbank
    sr, n_fft, n_mels, fmin, fmax = args
    w = mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    assert w.dtype == np.float64 and w.shape == (n_mels, n_fft // 2 + 1) and (w >= 0).all() and np.isfinite(w).all()
    top = sr / 2.0 if fmax is None else fmax
    c = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(top), n_mels + 2))
    assert abs(c[0] - fmin) < 1e-9 and abs(c[-1] - top) < 1e-9 and (np.diff(c) > 0).all()
    assert abs(float(_hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(_hz_to_mel(200.0)) - 3.0) < 1e-12
    fk = np.arange(n_fft // 2 + 1) * sr / n_fft
    df = sr / n_fft
    for j in range(n_mels):
        nz = np.flatnonzero(w[j])
        # one triangle: the non-zeros are exactly the bins strictly inside (c_j, c_j+2), contiguous, rising to one peak and falling
        inside = np.flatnonzero((fk > c[j]) & (fk < c[j + 2]))
        assert nz.tolist() == inside.tolist(), j
        if nz.size:
            assert (np.diff(nz) == 1).all()
            d = np.sign(np.diff(w[j, nz]))
            assert (np.diff(d[d != 0]) <= 0).all(), j          # never falls and rises again
            assert w[j].max() <= 2.0 / (c[j + 2] - c[j]) * (1 + 1e-12)
        # the docstring's area: the continuous triangle has area 1, the sampled row sums to it over the bin spacing within what a
        # trapezoid sum of a triangle can miss - its three kinks, each by at most peak * df / 2 ... in units of 1 / df
        peak = 2.0 / (c[j + 2] - c[j])
        assert abs(w[j].sum() * df - 1.0) <= 1.5 * peak * df + 1e-12, (j, w[j].sum() * df)
    wide = [j for j in range(n_mels) if c[j + 2] - c[j] >= 8 * df]
    assert wide and all(abs(w[j].sum() * df - 1.0) < 0.05 for j in wide)
    with pytest.raises(ConfigurationError, match="0 <= fmin < fmax <= sample_rate / 2"):
        mel_filterbank(16000, 400, 80, 0.0, 9000.0)


# ---- the order of the checks ------------------------------------------------------------------------------------------
def test_a_call_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_scan_mel's checks is behaviour: vad_mel's fields, the filters, out_rows below 0, frame format, channels,
    hop, the segments, out_rows against the segments' rows, the output pointer, and last the device form's two alignments.  Every
    fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    op_re, op_im, filters = RO.mel_ops()
    good, far = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 0, 0, 0)], [(0, 0, 1, 0, 0, 0), (0, 7, 2, 0, 0, 0)]      # 29 + 45 rows

    def call(device, n_fft, floor, fil, out_rows, fmt, channels, hop, items, out, audio):
        m = RO.mel(n_fft=n_fft, floor=floor)
        args = (eng.handle, RO.cut_items(items), len(items), C.byref(m), RO.f32p(op_re), RO.f32p(op_im), RO.f32p(fil), RO.addr(audio), RO.NS,
                channels, fmt, hop, -1.0)
        if device:
            return lib.vad_scan_mel_device(*args, RO.addr(out), out_rows, None)
        return lib.vad_scan_mel(*args, RO.f32p(out), out_rows)

    faults = dict(n_fft=100, floor=float("nan"), fil=None, out_rows=-1, fmt=9, channels=3, hop=6, items=far, out=None, audio=RO.buf(4 * RO.NS, 2))
    RO.walk(lib, eng, call, faults, (
        (INV, "n_fft = 100 must be", "n_fft", 64),
        (INV, "floor = -?nan: a logarithm needs", "floor", 1e-5),
        (INV, "null filters", "fil", filters),
        (INV, "out_rows = -1 is negative", "out_rows", 0),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", good),
        (INV, "out_rows = 0, the segments have 74 rows", "out_rows", 74),
        (INV, "vad_scan_mel(_device)?: null buffer$", "out", RO.buf(4 * 4 * 74, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(4 * 4 * 74), RO.DEVICE)))
