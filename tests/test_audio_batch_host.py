"""vad_scan_moments and vad_scan_audio_batch on the host side: exports, every refusal with its message and untouched outputs, the
order of the checks, the resident-block rules, nw == 0 and n == 0, every kind of engine, values against tests/audio_batch_ref.py for
every wire format and channel mode, and the Python faces (Engine.moments, Engine.audio_batch, AudioBatch, audio_windows,
audio_affine, audio_recordings) - the real csrc/engine.cpp over the HIP stand-in (tests/standin.py: tools/san_tick/fake_kernels.cpp
restates the kernels' rule in plain C++).  Every comparison is of bytes.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import ConfigurationError
from tests import audio_batch_ref as AR
from tests import standin
from tests.batch_ref import BF16, F16, F32, PAD_FEATURE, PAD_VALUE
from tests.cut_ref import FMT, INV, MIX, gate, heard, values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_moments", "vad_scan_moments_device", "vad_scan_audio_batch", "vad_scan_audio_batch_device"]
SENT_MO = (0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C)
SENT8 = 0x5A
NP = {F32: np.float32, F16: np.float16, BF16: np.uint16}


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


def _block(audio, channels, audio_samples):
    if audio is None:
        return None, None, audio_samples
    audio = np.ascontiguousarray(audio)
    return audio, audio.ctypes.data, audio.size // max(channels, 1) if audio_samples is None else audio_samples


def raw_moments(lib, eng, items, audio, channels, fmt, hop, thr=-1.0, sr_in=0, audio_samples=None, device=False, out="own"):
    """vad_scan_moments (or _device) -> (rc, message, records); the records are pre-filled"""
    if isinstance(out, str):
        out = np.zeros(len(items) + 1, _ffi.MOMENTS_DTYPE)
        out[:] = SENT_MO
    keep, ptr, ns = _block(audio, channels, audio_samples)
    if device:
        rc = lib.vad_scan_moments_device(eng.handle, _items(items), len(items), ptr, ns, channels, fmt, sr_in, hop, thr,
                                         None if out is None else out.ctypes.data, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_moments(eng.handle, _items(items), len(items), ptr, ns, channels, fmt, sr_in, hop, thr,
                                  None if out is None else out.ctypes.data_as(C.POINTER(_ffi.Moments)))
    return rc, lib.vad_last_error(eng.handle).decode(), out


def mo_untouched(out):
    return all((out[name] == v).all() for name, v in zip(("sum_q31", "energy_q32"), SENT_MO))


def raw_batch(lib, eng, items, audio, channels, fmt, hop, T, windows, dtype=F32, pad_mode=PAD_VALUE, pad_value=0.0, shift=None, scale=None,
              nss=None, thr=-1.0, sr_in=0, audio_samples=None, device=False, mask=True, out="own", out_bytes=None, b="own", nw=None):
    """vad_scan_audio_batch (or _device) -> (rc, message, out bytes with 16 sentinel bytes behind nw * T cells, mask likewise)"""
    nwin = len(windows) if nw is None else nw
    cells = max(2 if windows is None else len(windows), 0) * max(T, 0)
    esize = 4 if dtype == F32 else 2
    if isinstance(out, str):
        out = np.full(cells * esize + 16, SENT8, np.uint8)
    m = np.full(cells + 16, SENT8, np.uint8) if mask is True else mask
    w = np.array([tuple(map(int, x)) for x in windows], _ffi.AUDIO_WINDOW_DTYPE).reshape(-1) if windows is not None else None
    wp = None if w is None else (w if w.size else np.zeros(1, _ffi.AUDIO_WINDOW_DTYPE)).ctypes.data_as(C.POINTER(_ffi.AudioWindow))
    rec = _ffi.AudioBatchRecord(int(T), int(dtype), int(pad_mode), float(pad_value)) if isinstance(b, str) else b
    sh = None if shift is None else np.ascontiguousarray(shift, np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
    f32p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    if nss is None:
        nss = max([a.size for a in (sh, sc) if a is not None] or [1])
    keep, ptr, ns = _block(audio, channels, audio_samples)
    args = (eng.handle, _items(items), len(items), ptr, ns, channels, fmt, sr_in, hop, thr, None if rec is None else C.byref(rec), wp, nwin,
            f32p(sh), f32p(sc), nss, None if out is None else out.ctypes.data, cells * esize if out_bytes is None else out_bytes,
            None if m is None or m is False else m.ctypes.data)
    if device:
        rc = lib.vad_scan_audio_batch_device(*args, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_audio_batch(*args)
    return rc, lib.vad_last_error(eng.handle).decode(), out, (None if m is None or m is False else m)


def untouched(a):
    return a is None or bool((a == SENT8).all())


def split(out, m, nw, T, dtype):
    """the call's outputs -> ([nw, T] in the dtype's numpy form, mask [nw, T]); the 16 bytes behind each are still the sentinel"""
    esize = 4 if dtype == F32 else 2
    assert (out[nw * T * esize:] == SENT8).all() and (m is None or (m[nw * T:] == SENT8).all())
    return out[:nw * T * esize].view(NP[dtype]).reshape(nw, T), None if m is None else m[:nw * T].reshape(nw, T)


def same(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes()


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
    for struct, cls, dt in (("vad_moments", _ffi.Moments, _ffi.MOMENTS_DTYPE), ("vad_audio_window", _ffi.AudioWindow, _ffi.AUDIO_WINDOW_DTYPE),
                            ("vad_audio_batch", _ffi.AudioBatchRecord, None)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S)
        fields = re.findall(r"(int64_t|int32_t|float)\s+(\w+);", m.group(1))
        assert [f[0] for f in cls._fields_] == [f[1] for f in fields]
        assert C.sizeof(cls) == 16
        if dt is not None:
            assert list(dt.names) == [f[1] for f in fields] and dt.itemsize == 16
            assert [dt.fields[n][1] for n in dt.names] == [getattr(cls, n).offset for n in dt.names]
    from cutter_vad_amd import _build
    assert "audio_batch.hip" in _build.HIP_SOURCES
    import cutter_vad_amd
    for name in ("AudioBatch", "audio_windows", "audio_affine", "audio_recordings"):
        assert name in cutter_vad_amd.__all__ and hasattr(cutter_vad_amd, name)


# ---- values -----------------------------------------------------------------------------------------------------------
def _case(rng, kind, channels, ns=4096):
    block = values(rng, kind, (ns, 2) if channels == 2 else ns)
    if kind == "f32":
        flat = block.reshape(-1)
        flat[:6] = [0.0, -0.0, 1e-40, -1e-40, 0.01, -0.01]       # zeros, denormals, the gate's threshold itself
    return block


@pytest.mark.parametrize("kind", ["f32", "i16_32767", "i16_32768", "ulaw", "alaw"])
@pytest.mark.parametrize("channel", ["mono", 0, 1, MIX])
def test_values_against_the_reference(lib, eng, kind, channel):
    rng = np.random.default_rng(7)
    channels = 1 if channel == "mono" else 2
    ch = 0 if channel == "mono" else channel
    frame, hop = eng.frame_samples, 256
    block = _case(rng, kind, channels)
    # (sample_offset, first_frame, nframes, out_sample, channel): three segments, two of which share samples
    items = [(0, 0, 1, 0, ch), (4, 1, 3, 0, ch), (0, 2, 13, 0, ch)]
    for thr in (-1.0, 0.01):
        segs = [AR.segment(block, kind, it, frame, hop, None if thr < 0 else thr) for it in items]
        S = [s.size for s in segs]
        assert S == [512, 1024, 3584]
        rc, msg, mo = raw_moments(lib, eng, items, block, channels, FMT[kind], hop, thr)
        assert rc == 0, msg
        assert same(mo[:3], AR.moments_records(segs)) and mo_untouched(mo[3:])
        lv = np.zeros(3, _ffi.LEVEL_DTYPE)
        rc = lib.vad_scan_levels(eng.handle, _items(items), 3, None, 4096, channels, FMT[kind], 0, hop, thr, 0.95, lv.ctypes.data_as(C.POINTER(_ffi.Level)))
        assert rc == 0 and lv["energy_q32"].tolist() == mo["energy_q32"][:3].tolist()
        if kind in ("i16_32768", "ulaw", "alaw") and thr < 0:
            from tests import g711_ref as G
            raw = block.astype(np.int64) if kind == "i16_32768" else G.table(kind)[block].astype(np.int64)
            if channels == 2 and ch != MIX:
                raw = raw[:, ch]
            if channels == 1 or ch != MIX:
                assert int(mo["sum_q31"][2]) == 65536 * int(raw[512:512 + 3584].sum())
                assert int(mo["energy_q32"][2]) == 4 * int((raw[512:512 + 3584] ** 2).sum())
        T = 1028
        windows = [(2, 1028, 0), (0, 512, 0), (1, 5, 1016), (2, 0, 3584), (2, 1028, 2556), (1, 1024, 0), (2, 1, 4), (0, 3, 508), (2, 1028, 0)]
        shift, scale = np.array([0.25, -0.5, 0.015625], np.float32), np.array([3.0, 0.3, -1.7], np.float32)
        for dtype, pad_mode, per_seg, device in ((F32, PAD_VALUE, True, False), (F16, PAD_FEATURE, True, True), (BF16, PAD_FEATURE, False, False),
                                                 (F32, PAD_FEATURE, False, True), (F16, PAD_VALUE, None, False)):
            sh, sc = (None, None) if per_seg is None else (shift, scale) if per_seg else (shift[1:2], scale[1:2])
            rc, msg, out, m = raw_batch(lib, eng, items, None if device is False else block, channels, FMT[kind], hop, T, windows, dtype, pad_mode,
                                        -3.5, sh, sc, thr=thr, audio_samples=4096, device=device)
            assert rc == 0, msg
            got, gm = split(out, m, len(windows), T, dtype)
            ref, rm = AR.batch(segs, windows, T, dtype, pad_mode, -3.5, sh, sc)
            assert same(got, ref) and same(gm, rm), (dtype, pad_mode, per_seg)


def test_f16_overflow_becomes_inf_and_no_mask_is_written(lib, eng):
    block = np.array([1.0, -1.0, 0.5, 0.0] * 128, np.float32)
    items = [(0, 0, 1, 0, 0)]
    rc, msg, out, m = raw_batch(lib, eng, items, block, 1, FMT["f32"], 256, 8, [(0, 8, 0)], F16, scale=[70000.0], mask=False)
    assert rc == 0 and m is None, msg
    got, _ = split(out, None, 1, 8, F16)
    assert got[0].tolist() == [np.inf, -np.inf, 35008.0, 0.0] * 2


def test_nw_zero_and_n_zero(lib, eng):
    block = np.zeros(2048, np.float32)
    rc, msg, out, m = raw_batch(lib, eng, [(0, 0, 1, 0, 0)], block, 1, FMT["f32"], 256, 8, [])
    assert rc == 0 and untouched(out) and untouched(m), msg
    rc, msg, out, m = raw_batch(lib, eng, [], block, 1, FMT["f32"], 256, 8, [], out=None, mask=None)
    assert rc == 0, msg
    rc, msg, out, m = raw_batch(lib, eng, [], block, 1, FMT["f32"], 256, 8, [(0, 0, 0)])
    assert rc == INV and "window 0 names segment 0 of 0" in msg and untouched(out) and untouched(m)
    rc, msg, mo = raw_moments(lib, eng, [], block, 1, FMT["f32"], 256, out=None)
    assert rc == 0, msg
    # a pad window
    rc, msg, out, m = raw_batch(lib, eng, [(0, 0, 1, 0, 0)], block + 1, 1, FMT["f32"], 256, 8, [(0, 0, 512), (0, 0, 0)], pad_value=2.5)
    got, gm = split(out, m, 2, 8, F32)
    assert rc == 0 and (got == 2.5).all() and (gm == 0).all()


# ---- the block ---------------------------------------------------------------------------------------------------------
def test_resident_block_rules(lib, make_engine):
    eng = make_engine()
    block = values(np.random.default_rng(3), "i16_32767", 2048)
    items, win = [(0, 1, 2, 0, 0)], [(0, 768, 0)]
    seg = [AR.segment(block, "i16_32767", items[0], 512, 256, None)]
    fmt = FMT["i16_32767"]
    # nothing resident
    rc, msg, mo = raw_moments(lib, eng, items, None, 1, fmt, 256, audio_samples=2048)
    assert rc == INV and "audio = NULL, and the engine holds no resident block" in msg and "vad_scan_moments:" in msg and mo_untouched(mo)
    rc, msg, out, m = raw_batch(lib, eng, items, None, 1, fmt, 256, 768, win, audio_samples=2048)
    assert rc == INV and "audio = NULL, and the engine holds no resident block" in msg and "vad_scan_audio_batch:" in msg
    assert untouched(out) and untouched(m)
    # an upload by the batch leaves the block resident for the moments, the levels and a cut
    rc, msg, out, m = raw_batch(lib, eng, items, block, 1, fmt, 256, 768, win)
    assert rc == 0 and same(split(out, m, 1, 768, F32)[0], AR.batch(seg, win, 768)[0]), msg
    rc, msg, mo = raw_moments(lib, eng, items, None, 1, fmt, 256, audio_samples=2048)
    assert rc == 0 and same(mo[:1], AR.moments_records(seg)), msg
    # ... and one by the moments for the batch
    other = values(np.random.default_rng(4), "i16_32767", 2048)
    seg2 = [AR.segment(other, "i16_32767", items[0], 512, 256, None)]
    assert raw_moments(lib, eng, items, other, 1, fmt, 256)[0] == 0
    rc, msg, out, m = raw_batch(lib, eng, items, None, 1, fmt, 256, 768, win, audio_samples=2048)
    assert rc == 0 and same(split(out, m, 1, 768, F32)[0], AR.batch(seg2, win, 768)[0]), msg
    # the resident block is what the call says it is
    for kw, text in ((dict(fmt=FMT["i16_32768"]), "has frame format"), (dict(channels=2), "has 1 channels, not 2"),
                     (dict(audio_samples=1024), "bytes, not the")):
        a = dict(fmt=fmt, channels=1, audio_samples=2048)
        a.update(kw)
        rc, msg, out, m = raw_batch(lib, eng, [(0, 0, 1, 0, 0)], None, a["channels"], a["fmt"], 256, 768, [(0, 4, 0)], audio_samples=a["audio_samples"])
        assert rc == INV and text in msg and untouched(out) and untouched(m), msg
    # a rate block is none of a plain call's
    rc, msg, mo = raw_moments(lib, eng, [(0, 0, 1, 0, 0)], None, 1, fmt, 768, sr_in=48000, audio_samples=2048)
    assert rc == INV and "holds no resident rate block" in msg


def test_a_rate_block_is_never_gated(lib, eng):
    block = values(np.random.default_rng(5), "f32", 8192) * np.float32(0.02)
    items = [(0, 1, 2, 0, 0)]                                            # chunks of 1536 samples at 48 kHz
    seg = [np.ascontiguousarray(block[768:768 + 768 + 1536])]
    rc, msg, mo = raw_moments(lib, eng, items, block, 1, FMT["f32"], 768, thr=0.01, sr_in=48000)
    assert rc == 0 and same(mo[:1], AR.moments_records(seg)), msg
    win = [(0, 2304, 0), (0, 4, 2300)]
    rc, msg, out, m = raw_batch(lib, eng, items, None, 1, FMT["f32"], 768, 2304, win, thr=0.01, sr_in=48000, audio_samples=8192)
    assert rc == 0 and same(split(out, m, 2, 2304, F32)[0], AR.batch(seg, win, 2304)[0]), msg
    rc, msg, out, m = raw_batch(lib, eng, items, None, 1, FMT["f32"], 768, 2304, [(0, 2304, 4)], sr_in=48000, audio_samples=8192)
    assert rc == INV and "window 0: samples 4 .. \\+2304".replace("\\", "") in msg and "which has 2304" in msg


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)])
def test_every_engine_is_served(lib, make_engine, kw):
    eng = make_engine(**kw)
    frame = eng.frame_samples
    block = values(np.random.default_rng(6), "f32", 8 * frame)
    items = [(0, 1, 3, 0, 0), (frame, 0, 1, 0, 0)]
    segs = [AR.segment(block, "f32", it, frame, frame // 2, 0.01) for it in items]
    rc, msg, mo = raw_moments(lib, eng, items, block, 1, FMT["f32"], frame // 2, 0.01)
    assert rc == 0 and same(mo[:2], AR.moments_records(segs)), msg
    T = 2 * frame
    win = [(1, frame, 0), (0, T, 0)]
    rc, msg, out, m = raw_batch(lib, eng, items, None, 1, FMT["f32"], frame // 2, T, win, F16, thr=0.01, audio_samples=8 * frame, shift=[0.5, -0.5])
    assert rc == 0, msg
    got, gm = split(out, m, 2, T, F16)
    ref, rm = AR.batch(segs, win, T, F16, shift=[0.5, -0.5])
    assert same(got, ref) and same(gm, rm)


# ---- refusals -----------------------------------------------------------------------------------------------------------
GOOD = dict(items=[(0, 0, 1, 0, 0), (0, 1, 2, 0, 0)], channels=1, fmt=FMT["f32"], hop=256, T=8, windows=[(0, 8, 0), (1, 4, 764)])


@pytest.mark.parametrize("kw, text", [
    (dict(sr_in=44100), "from 44100Hz to 16000Hz"),
    (dict(fmt=9), "unknown frame format 9"),
    (dict(channels=3), "channels = 3, the block holds"),
    (dict(hop=6), "hop = 6 must be"),
    (dict(items=[(2, 0, 1, 0, 0)]), "segment 0: its recording starts at sample 2"),
    (dict(items=[(0, 0, 0, 0, 0)]), "segment 0: first_frame = 0, nframes = 0"),
    (dict(items=[(0, 0, 1, 0, 0), (0, 7, 2, 0, 0)]), "segment 1 .*leaves the audio block of 2048 samples"),
    (dict(items=[(0, 0, 1, 0, 1)]), "segment 0 names channel 1 of 1"),
    (dict(items=[(0, 0, 1, 0, 0, 5)]), "reserved = 5 must be 0"),
    (dict(b=None), "null vad_audio_batch"),
    (dict(T=0), "samples = 0 must be a multiple of 4 from 4 to 2\\^24"),
    (dict(T=6), "samples = 6 must be a multiple of 4"),
    (dict(T=(1 << 24) + 4, out_bytes=0), "samples = 16777220 must be"),
    (dict(dtype=3), "dtype = 3 is none of"),
    (dict(pad_mode=2), "pad_mode = 2 is neither"),
    (dict(pad_value=float("inf")), "pad_value is infinite"),
    (dict(pad_value=float("nan")), "pad_value is NaN"),
    (dict(nw=-1), "null buffer or bad count"),
    (dict(windows=None, nw=2), "null buffer or bad count"),
    (dict(shift=[0.0] * 3), "nss = 3: shift and scale have 1 entry or n = 2"),
    (dict(shift=[0.0, float("nan")]), "shift\\[1\\] is NaN, a shift is a finite number"),
    (dict(scale=[float("-inf")]), "scale\\[0\\] is infinite, a scale is a finite number"),
    (dict(windows=[(0, 8, 0), (2, 4, 0)]), "window 1 names segment 2 of 2"),
    (dict(windows=[(-1, 4, 0)]), "window 0 names segment -1 of 2"),
    (dict(windows=[(0, 4, 2)]), "window 0: samples 2 .. \\+4 of segment 0, which has 512, in 8 samples"),
    (dict(windows=[(0, 4, -4)]), "window 0: samples -4 .. \\+4"),
    (dict(windows=[(0, 8, 0), (0, 9, 0)]), "window 1: samples 0 .. \\+9"),
    (dict(windows=[(0, -1, 0)]), "window 0: samples 0 .. \\+-1"),
    (dict(windows=[(1, 8, 764)]), "window 0: samples 764 .. \\+8 of segment 1, which has 768"),
    (dict(windows=[(0, 0, 516)]), "window 0: samples 516 .. \\+0 of segment 0, which has 512"),
    (dict(out_bytes=63), "out_bytes = 63, the windows have 64 bytes"),
    (dict(out=None), "vad_scan_audio_batch(_device)?: null buffer$"),
])
def test_every_refusal_names_the_function_and_writes_nothing(lib, eng, kw, text):
    block = np.zeros(2048, np.float32)
    for device in (False, True):
        a = dict(GOOD)
        a.update(kw)
        rc, msg, out, m = raw_batch(lib, eng, a.pop("items"), block, a.pop("channels"), a.pop("fmt"), a.pop("hop"), a.pop("T"), a.pop("windows"),
                                    device=device, **a)
        assert rc in (INV, _ffi.VAD_ERR_UNSUPPORTED) and re.search(text, msg), msg
        assert ("vad_scan_audio_batch_device:" if device else "vad_scan_audio_batch:") in msg or "unknown frame format" in msg or "Hz" in msg
        assert untouched(out) and untouched(m)
        if kw.keys() & {"sr_in", "fmt", "channels", "hop", "items"}:
            a = dict(GOOD)
            a.update(kw)
            rc, msg, mo = raw_moments(lib, eng, a["items"], block, a["channels"], a["fmt"], a["hop"], sr_in=a.get("sr_in", 0), device=device)
            assert rc in (INV, _ffi.VAD_ERR_UNSUPPORTED) and re.search(text, msg) and mo_untouched(mo), msg
    rc, msg, mo = raw_moments(lib, eng, GOOD["items"], block, 1, FMT["f32"], 256, out=None)
    assert rc == INV and msg.endswith("vad_scan_moments: null buffer")


def test_too_many_workgroups(lib, eng):
    block = np.zeros(2048, np.float32)
    w = np.zeros(1, _ffi.AUDIO_WINDOW_DTYPE)
    rec = _ffi.AudioBatchRecord(1 << 24, F32, PAD_VALUE, 0.0)
    # nw = 2^19 windows of 2^24 samples are 2^31 workgroups; the first window is looked at, the count refuses before the others
    # would be: the windows are checked first, so all of them must be there
    nw = 1 << 19
    wins = np.zeros(nw, _ffi.AUDIO_WINDOW_DTYPE)
    rc = lib.vad_scan_audio_batch(eng.handle, _items([(0, 0, 1, 0, 0)]), 1, block.ctypes.data, 2048, 1, FMT["f32"], 0, 256, -1.0, C.byref(rec),
                                  wins.ctypes.data_as(C.POINTER(_ffi.AudioWindow)), nw, None, None, 1, w.ctypes.data, (1 << 62), None)
    msg = lib.vad_last_error(eng.handle).decode()
    assert rc == INV and "vad_scan_audio_batch: more than 2^31 - 1 workgroups of 4096 samples in one call" in msg


def test_a_call_with_several_faults_gets_the_first_refusal(lib, eng):
    """The order of vad_scan_audio_batch's checks is behaviour: the rate, the block and the items as vad_scan_levels has them, the
    batch record, the counts, nss, shift and scale, the windows, out_bytes, the output pointer, and last the device form's
    alignments.  Every fault at once, then one mended at a time."""
    from tests import refusal_order as RO
    good, far = [(0, 0, 1, 0, 0, 0), (0, 1, 2, 0, 0, 0)], [(0, 0, 1, 0, 0, 0), (0, 7, 2, 0, 0, 0)]
    wgood = np.array([(0, 8, 0), (1, 4, 764)], _ffi.AUDIO_WINDOW_DTYPE)
    wbad = np.array([(0, 8, 0), (1, 4, 766)], _ffi.AUDIO_WINDOW_DTYPE)

    def call(device, sr_in, fmt, channels, hop, items, b, nw, shift, scale, windows, out_bytes, out, audio, mask):
        rec = None if b is None else _ffi.AudioBatchRecord(*b)
        args = (eng.handle, RO.cut_items(items), len(items), RO.addr(audio), RO.NS, channels, fmt, sr_in, hop, -1.0,
                None if rec is None else C.byref(rec), windows.ctypes.data_as(C.POINTER(_ffi.AudioWindow)), nw, RO.f32p(shift), RO.f32p(scale),
                3 if shift is not None and shift.size == 3 else 2, RO.addr(out), out_bytes, RO.addr(mask))
        if device:
            return lib.vad_scan_audio_batch_device(*args, None)
        return lib.vad_scan_audio_batch(*args)

    faults = dict(sr_in=44100, fmt=9, channels=3, hop=6, items=far, b=None, nw=-2, shift=RO.f32(0, 0, 0), scale=RO.f32(1, float("inf")),
                  windows=wbad, out_bytes=8, out=None, audio=RO.buf(4 * RO.NS, 2), mask=RO.buf(16, 2))
    RO.walk(lib, eng, call, faults, (
        (RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 0),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", good),
        (INV, "null vad_audio_batch", "b", (6, 7, 7, float("nan"))),
        (INV, "samples = 6 must be", "b", (8, 7, 7, float("nan"))),
        (INV, "dtype = 7 is none of", "b", (8, F32, 7, float("nan"))),
        (INV, "pad_mode = 7 is neither", "b", (8, F32, PAD_VALUE, float("nan"))),
        (INV, "pad_value is NaN", "b", (8, F32, PAD_VALUE, 0.0)),
        (INV, "null buffer or bad count", "nw", 2),
        (INV, "nss = 3: shift and scale", "shift", RO.f32(0, 0)),
        (INV, "scale\\[1\\] is infinite", "scale", RO.f32(1, 1)),
        (INV, "window 1: samples 766 .. \\+4 of segment 1", "windows", wgood),
        (INV, "out_bytes = 8, the windows have 64 bytes", "out_bytes", 64),
        (INV, "vad_scan_audio_batch(_device)?: null buffer$", "out", RO.buf(64, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the output must be 16-byte aligned", "out", RO.buf(64), RO.DEVICE),
        (INV, "the mask must be 4-byte aligned", "mask", RO.buf(16), RO.DEVICE)))

    def mcall(device, sr_in, fmt, channels, hop, items, out, audio):
        args = (eng.handle, RO.cut_items(items), len(items), RO.addr(audio), RO.NS, channels, fmt, sr_in, hop, -1.0)
        if device:
            return lib.vad_scan_moments_device(*args, RO.addr(out), None)
        return lib.vad_scan_moments(*args, None if out is None else C.cast(RO.addr(out), C.POINTER(_ffi.Moments)))

    RO.walk(lib, eng, mcall, dict(sr_in=44100, fmt=9, channels=3, hop=6, items=far, out=None, audio=RO.buf(4 * RO.NS, 2)), (
        (RO.UNS, "from 44100Hz to 16000Hz", "sr_in", 0),
        (INV, "unknown frame format 9", "fmt", FMT["f32"]),
        (INV, "channels = 3, the block holds", "channels", 1),
        (INV, "hop = 6 must be", "hop", 256),
        (INV, "segment 1 .*leaves the audio block of 2048 samples", "items", good),
        (INV, "vad_scan_moments(_device)?: null buffer$", "out", RO.buf(2 * 16, 4)),
        (INV, "the audio block must be 4-byte aligned", "audio", RO.buf(4 * RO.NS), RO.DEVICE),
        (INV, "the moments must be 8-byte aligned", "out", RO.buf(2 * 16), RO.DEVICE)))


# ---- the Python faces ----------------------------------------------------------------------------------------------------
def test_audio_windows():
    from cutter_vad_amd import audio_windows
    w, T = audio_windows([5, 0, 1030])
    assert T == 1032 and w.dtype == _ffi.AUDIO_WINDOW_DTYPE and w.tolist() == [(0, 5, 0), (1, 0, 0), (2, 1030, 0)]
    assert audio_windows([])[1] == 4 and audio_windows([0])[1] == 4 and audio_windows([4])[1] == 4
    w, T = audio_windows([10, 0, 8], samples=8)
    assert T == 8 and w.tolist() == [(0, 8, 0), (0, 2, 8), (2, 8, 0)]
    w, T = audio_windows([10, 3], samples=8, stride=4)
    assert T == 8 and w.tolist() == [(0, 8, 0), (0, 6, 4), (0, 2, 8), (1, 3, 0)]
    for bad in (dict(samples=6), dict(samples=0), dict(samples=8, stride=2), dict(samples=8, stride=0), dict(samples=(1 << 24) + 4)):
        with pytest.raises(ConfigurationError):
            audio_windows([10], **bad)
    with pytest.raises(ConfigurationError):
        audio_windows([-1])
    with pytest.raises(ConfigurationError, match="give samples"):
        audio_windows([(1 << 24) + 1])


def test_audio_batch_check():
    from cutter_vad_amd import AudioBatch
    AudioBatch().check()
    assert AudioBatch(samples=16, dtype="bf16", pad="feature", pad_value=1.0).record() == dict(samples=16, dtype="bf16", pad="feature", pad_value=1.0)
    for bad in (dict(norm="cmvn"), dict(dtype="f64"), dict(pad="zero"), dict(samples=6), dict(samples=0), dict(stride=6), dict(stride=0),
                dict(scope="window"), dict(eps=-1.0), dict(eps=float("nan")), dict(target=0.0), dict(target=float("inf")), dict(pad_value=float("nan"))):
        with pytest.raises(ConfigurationError):
            AudioBatch(**bad).check()
    with pytest.raises(ConfigurationError, match="samples=None"):
        AudioBatch().record()


def test_audio_affine_is_exact_on_int16_sums():
    from cutter_vad_amd import audio_affine
    rng = np.random.default_rng(11)
    segs = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (1, 7, 100000, 0)] + [np.full(50, 1234, np.int16), np.zeros(9, np.int16)]
    mo = np.zeros(len(segs), _ffi.MOMENTS_DTYPE)
    lv = np.zeros(len(segs), _ffi.LEVEL_DTYPE)
    for i, s in enumerate(segs):
        s64 = s.astype(np.int64)
        mo[i] = (65536 * int(s64.sum()), 4 * int((s64 ** 2).sum()))
        lv[i]["peak"] = np.abs(s.astype(np.float32) / np.float32(32768)).max(initial=0)
        assert s.size == 0 or tuple(mo[i]) == AR.moments(s.astype(np.float32) / np.float32(32768))
    ns = [s.size for s in segs]
    assert audio_affine(mo, lv, ns, "none") == (None, None)
    for norm in ("mean", "zscore"):
        shift, scale = audio_affine(mo, None, ns, norm, eps=1e-7)
        rs, rc = [], []
        for s in segs:
            x = s.astype(np.float64) / 32768.0
            mean = x.sum() / x.size if x.size else 0.0
            # the same formulas on the exact sums: sum s / (32768 N) and sum s^2 / (32768^2 N) - mean^2
            mean = float(int(s.astype(np.int64).sum())) * 65536.0 / (2147483648.0 * max(s.size, 1))
            var = float(4 * int((s.astype(np.int64) ** 2).sum())) / (4294967296.0 * max(s.size, 1)) - mean * mean
            rs.append(np.float32(-mean))
            rc.append(np.float32(1.0 / np.sqrt(max(var, 0.0) + 1e-7)) if s.size else np.float32(1))
        assert shift.dtype == np.float32 and shift.tobytes() == np.array(rs, np.float32).tobytes()
        if norm == "mean":
            assert scale is None
        else:
            assert scale.dtype == np.float32 and scale.tobytes() == np.array(rc, np.float32).tobytes()
            assert scale[4] == np.float32(1.0 / np.sqrt(1e-7))          # a constant segment: var 0, not negative
    shift, scale = audio_affine(None, lv, ns, "peak", target=0.9)
    ref = [np.float32(np.float32(0.9) / p) if p > 0 else np.float32(1) for p in lv["peak"]]
    assert shift is None and scale.tobytes() == np.array(ref, np.float32).tobytes() and scale[3] == 1 and scale[5] == 1
    with pytest.raises(ConfigurationError):
        audio_affine(mo, lv, ns, "cmvn")


def _script(frame, s, amp=1.0, fill=0.125, rng=None):
    """the stand-in's p = |first sample of the frame|: a recording whose frames have the probabilities `s`"""
    s = list(s) + [0.0] * (15 - len(s))
    x = np.full(frame * len(s) + 3, np.float32(fill), np.float32)
    if rng is not None:
        x = rng.uniform(-0.4, 0.6, x.size).astype(np.float32)
    x[:len(s) * frame:frame] = np.asarray(s, np.float32) * np.float32(amp)
    return x


def _cfg(frame, **kw):
    from cutter_vad_amd import VADConfig
    return VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5, voice_start_frame_count=2,
                     voice_end_frame_count=2, output_wav_sample_rate=8000, **kw)


def _numpy_batch(cut, batch, T, windows, groups):
    """cut: the float32 range cut of each segment, in the table's order -> what audio_recordings returns, in numpy: audio_affine's
    formulas on the reference's integer moments, then the rule"""
    from cutter_vad_amd import audio_affine
    mo = AR.moments_records(cut)
    lv = np.zeros(len(cut), _ffi.LEVEL_DTYPE)
    lv["peak"] = [np.abs(c).max() for c in cut]
    ns = np.array([c.size for c in cut], np.int64)
    if batch.scope == "recording":
        ids = sorted(set(groups))
        gm, gl, gn = np.zeros(len(ids), _ffi.MOMENTS_DTYPE), np.zeros(len(ids), _ffi.LEVEL_DTYPE), np.zeros(len(ids), np.int64)
        for k, g in enumerate(groups):
            j = ids.index(g)
            gm[j] = (int(gm[j]["sum_q31"]) + int(mo[k]["sum_q31"]), int(gm[j]["energy_q32"]) + int(mo[k]["energy_q32"]))
            gl[j]["peak"] = max(gl[j]["peak"], lv[k]["peak"])
            gn[j] += ns[k]
        pick = np.array([ids.index(g) for g in groups])
        shift, scale = (None if a is None else a[pick] for a in audio_affine(gm, gl, gn, batch.norm, batch.eps, batch.target))
    else:
        shift, scale = audio_affine(mo, lv, ns, batch.norm, batch.eps, batch.target)
    return AR.batch(cut, windows, T, _ffi.BATCH_DTYPES[batch.dtype], _ffi.BATCH_PADS[batch.pad], batch.pad_value, shift, scale)


def test_audio_recordings_against_the_range_cut_and_numpy(make_engine):
    from cutter_vad_amd import AudioBatch, audio_recordings, audio_windows, cut_recordings
    eng = make_engine()
    frame = hop = eng.frame_samples
    rng = np.random.default_rng(2)
    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.7] * 4 + [0.0] * 4 + [0.96] * 3 + [0.0] * 4
    none = [0.0] * 9
    st = lambda l, r: np.ascontiguousarray(np.stack([_script(frame, l, rng=rng), _script(frame, r, rng=rng)], axis=1))
    mono = [_script(frame, one, rng=rng), _script(frame, none), _script(frame, two, rng=rng)]
    stereo = [st(two, none), st(none, one)]
    seen = 0
    for corpus, channel in ((mono, "mix"), (stereo, 0), (stereo, "split")):
        for gate_on in (False, True):
            cfg = _cfg(frame, enable_denoising=gate_on)
            cuts = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout="range", wav=False)
            if channel != "split":
                cuts = [[c] for c in cuts]
            chans = (0, 1) if channel == "split" else (0 if corpus is mono else channel,)
            flat = [(i, chans[c], a, b, np.frombuffer(pcm, np.int16)) for i, rc in enumerate(cuts) for c, rg in enumerate(rc) for a, b, pcm in rg]
            # the float32 cut itself: the segment's samples as the recording has them, gated
            f32cut = []
            for i, ch, a, b, _ in flat:
                x = corpus[i] if corpus[i].ndim == 1 else heard(corpus[i], "f32", ch)
                f32cut.append(np.ascontiguousarray(gate(x, 0.01 if gate_on else None)[a:b], np.float32))
            groups = [(i, ch) for i, ch, *_ in flat]
            for batch in (AudioBatch(norm="zscore", dtype="f16"), AudioBatch(samples=1024, stride=512, norm="mean", pad="feature"),
                          AudioBatch(samples=2048, norm="peak", dtype="bf16", pad_value=-1.0), AudioBatch(norm="none"),
                          AudioBatch(norm="zscore", scope="recording"), AudioBatch(samples=1024, norm="peak", scope="recording", target=0.5)):
                got, index, gm = audio_recordings(corpus, batch, cfg, engine=eng, hop=hop, channel=channel, mask=True)
                windows, T = audio_windows([c.size for c in f32cut], batch.samples, batch.stride)
                ref, rm = _numpy_batch(f32cut, batch, T, windows, groups)
                assert same(got, ref) and same(gm, rm), (channel, gate_on, batch)
                assert index == [flat[int(w["seg"])][:4] + (int(w["sample0"]), int(w["nsamples"])) for w in windows]
                assert same(audio_recordings(corpus, batch, cfg, engine=eng, hop=hop, channel=channel)[0], ref)
                seen += len(index)
    assert seen > 50
    # nothing to show
    got, index, gm = audio_recordings([_script(frame, none)], AudioBatch(samples=64, dtype="f16"), _cfg(frame), engine=eng, hop=hop, mask=True)
    assert got.shape == (0, 64) and got.dtype == np.float16 and index == [] and gm.shape == (0, 64)
    assert audio_recordings([], AudioBatch(), _cfg(frame), engine=eng)[0].shape == (0, 4)
    # one scan, one moments, one batch
    calls = []
    names = ("scan_segments", "moments", "levels", "audio_batch", "cut", "scan")

    class Spy:
        def __getattr__(self, name):
            f = getattr(eng, name)
            if name not in names:
                return f

            def g(*a, **k):
                calls.append(name)
                return f(*a, **k)
            return g

    audio_recordings(mono, AudioBatch(norm="zscore"), _cfg(frame), engine=Spy(), hop=hop)
    assert calls == ["scan_segments", "moments", "audio_batch"]
    del calls[:]
    audio_recordings(mono, AudioBatch(norm="peak", scope="recording"), _cfg(frame), engine=Spy(), hop=hop)
    assert calls == ["scan_segments", "levels", "audio_batch"]
    del calls[:]
    audio_recordings(mono, AudioBatch(), _cfg(frame), engine=Spy(), hop=hop)
    assert calls == ["scan_segments", "audio_batch"]


def test_audio_recordings_refusals(make_engine):
    from cutter_vad_amd import AudioBatch, audio_recordings
    eng = make_engine()
    frame = eng.frame_samples
    x = _script(frame, [0.9] * 5)
    with pytest.raises(ConfigurationError, match="need convert="):
        audio_recordings([x], AudioBatch(), _cfg(frame), engine=eng, sample_rate=48000)
    with pytest.raises(ConfigurationError, match="one batch holds recordings of one kind"):
        audio_recordings([x, np.stack([x, x], axis=1)], AudioBatch(), _cfg(frame), engine=eng)
    with pytest.raises(ConfigurationError, match="norm is"):
        audio_recordings([x], AudioBatch(norm="cmn"), _cfg(frame), engine=eng)
    with pytest.raises(ConfigurationError, match="channel is"):
        audio_recordings([x], AudioBatch(), _cfg(frame), engine=eng, channel=2)

    class Bare:
        sample_rate, frame_samples = 16000, frame
    with pytest.raises(ConfigurationError, match="needs an engine with audio_batch"):
        audio_recordings([x], AudioBatch(), _cfg(frame), engine=Bare())


def test_engine_faces(make_engine):
    eng = make_engine()
    block = values(np.random.default_rng(9), "i16_32767", 4096)
    table = [(0, 1, 2), (512, 0, 5)]
    items = [(0, 1, 2, 0, 0), (512, 0, 5, 0, 0)]
    segs = [AR.segment(block, "i16_32768", it, 512, 256, 0.01) for it in items]
    mo = eng.moments(table, audio=block, i16_scale=32768)
    assert same(mo, AR.moments_records(segs))
    assert eng.levels(table, audio=block, i16_scale=32768)["energy_q32"].tolist() == mo["energy_q32"].tolist()
    win = [(1, 1536, 0), (0, 768, 0)]
    got, m = eng.audio_batch(table, win, dict(samples=1536, dtype="bf16", pad="feature"), shift=[0.5, -0.25], scale=2.0, mask=True, audio=block,
                             i16_scale=32768)
    ref, rm = AR.batch(segs, win, 1536, BF16, PAD_FEATURE, 0.0, [0.5, -0.25], [2.0])
    assert same(got, ref) and same(m, rm)
    out = np.full(2 * 1536 + 4, -7.0, np.float32)
    mk = np.full(2 * 1536 + 4, SENT8, np.uint8)
    dmo = np.zeros(2, _ffi.MOMENTS_DTYPE)
    assert eng.audio_batch_device(table, win, dict(samples=1536), block.ctypes.data, 4096, out.ctypes.data, 2 * 1536 * 4, mk.ctypes.data,
                                  fmt=FMT["i16_32768"]) == (2, 1536)
    eng.moments_device(table, block.ctypes.data, 4096, dmo.ctypes.data, fmt=FMT["i16_32768"])
    eng.synchronize()
    ref, rm = AR.batch(segs, win, 1536)
    assert same(out[:-4].reshape(2, 1536), ref) and (out[-4:] == -7.0).all() and same(mk[:-4].reshape(2, 1536), rm) and (mk[-4:] == SENT8).all()
    assert same(dmo, mo)
    with pytest.raises(Exception, match="shift and scale have the same number of entries"):
        eng.audio_batch(table, win, dict(samples=1536), shift=[0.0, 0.0], scale=[1.0, 1.0, 1.0], audio=block)
