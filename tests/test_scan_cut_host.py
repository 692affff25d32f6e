"""vad_scan_cut on the host side: exports, vad_cut_samples, every refusal with its message and an untouched output, the resident
block (audio = NULL), V4 and shared-GPU engines, ragged segments in every format x channel mode x layout x output format x gate
against a numpy reference written here, and the Python faces - the real csrc/engine.cpp over the HIP stand-in (tests/standin.py:
tools/san_tick/fake_kernels.cpp restates the cut kernel's arithmetic in plain C++).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests import standin
from tests.cut_ref import (F32, FMT, FRAMES, INV, MIX, PCM16, RANGE, SENT16, decode, heard, pcm16, raw_cut, reference, untouched,
                           values)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_cut_samples", "vad_scan_cut", "vad_scan_cut_device"]
# ---- fixtures ---------------------------------------------------------------------------------------------------------
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
    assert C.sizeof(_ffi.CutItem) == 40
    m = re.search(r"typedef struct vad_cut_item \{(.*?)\} vad_cut_item;", header, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    assert fields == [("int64_t", "sample_offset"), ("int64_t", "first_frame"), ("int64_t", "nframes"), ("int64_t", "out_sample"),
                      ("int32_t", "channel"), ("int32_t", "reserved")]
    assert [f[0] for f in _ffi.CutItem._fields_] == [f[1] for f in fields]
    assert re.search(r"enum \{ VAD_CUT_FRAMES = 0, VAD_CUT_RANGE = 1 \};", header) and (FRAMES, RANGE) == (0, 1)
    assert re.search(r"enum \{ VAD_CUT_PCM16 = 0, VAD_CUT_F32 = 1 \};", header) and (PCM16, F32) == (0, 1)
    w = int(re.search(r"#define\s+VAD_CUT_WG_SAMPLES\s+(\d+)", header).group(1))
    assert w == _ffi.VAD_CUT_WG_SAMPLES and w % 1024 == 0      # whole passes of 256 threads x one quad


@pytest.mark.parametrize("rate", [16000, 8000])
def test_cut_samples(lib, make_engine, rate):
    eng = make_engine(rate=rate)
    frame = eng.frame_samples
    assert frame == (512 if rate == 16000 else 256)
    for nf in (1, 2, 9, 1000):
        for hop in (4, frame // 4 + 4, frame // 2, frame, frame + 4):
            assert lib.vad_cut_samples(eng.handle, nf, hop, FRAMES) == nf * frame
            assert lib.vad_cut_samples(eng.handle, nf, hop, RANGE) == (nf - 1) * hop + frame
            assert eng.cut_samples(nf, hop, "range") == (nf - 1) * hop + frame
    for bad in ((0, 256, FRAMES), (-1, 256, RANGE), (3, 0, FRAMES), (3, 2, FRAMES), (3, 6, RANGE), (3, -256, RANGE), (3, 256, 2),
                (3, 256, -1)):
        assert lib.vad_cut_samples(eng.handle, *bad) == -1, bad
    assert lib.vad_cut_samples(None, 3, 256, FRAMES) == -1
    with pytest.raises(Exception, match="bad frame count, hop or layout"):
        eng.cut_samples(0, 256)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_write_nothing(lib, make_engine):
    eng = make_engine()
    x = np.zeros((4096, 2), np.float32) + np.float32(0.25)
    hop = 256
    ok = [(0, 0, 3, 0, 0), (1024, 2, 2, 1536, MIX)]          # FRAMES: 1 536 and 1 024 samples
    n_out = 2560
    for device in (False, True):
        rc, msg, out = raw_cut(lib, eng, ok, x, 2, FMT["f32"], hop, FRAMES, F32, n_out, device=device)
        assert rc == _ffi.VAD_OK, msg
        assert (out[:n_out] == np.float32(0.25)).all() and untouched(out[n_out:])

    def refused(pattern, items, audio=x, channels=2, fmt=FMT["f32"], hop=hop, layout=FRAMES, out_fmt=F32, out_samples=n_out, **kw):
        for device in (False, True):
            rc, msg, out = raw_cut(lib, eng, items, audio, channels, fmt, hop, layout, out_fmt, out_samples, device=device, **kw)
            assert rc == INV, (rc, msg)
            assert re.search(pattern, msg), msg
            assert msg.startswith("Model prediction failed: ") and ("vad_scan_cut" in msg or "format" in msg), msg
            assert untouched(out)

    for layout in (2, -1):
        refused(r"layout = -?\d", ok, layout=layout)
    for out_fmt in (2, -1):
        refused(r"out_fmt = -?\d", ok, out_fmt=out_fmt)
    for fmt in (5, -1, 9):
        refused("unknown frame format", ok, fmt=fmt)
    for channels in (0, 3, -1):
        refused(r"channels = -?\d", ok, channels=channels, audio_samples=4096)
    for h in (0, 2, 6, -256, 258):
        refused("hop = -?\\d+ must be a positive multiple of 4", ok, hop=h)
    refused("starts at sample 2, not a multiple of 4", [(2, 0, 3, 0, 0)])
    refused("starts at sample -4, not a multiple of 4", [(-4, 0, 3, 0, 0)])
    refused("first_frame = -1", [(0, -1, 3, 0, 0)])
    refused("nframes = 0", [(0, 0, 0, 0, 0)])
    refused("nframes = -2", [(0, 0, -2, 0, 0)])
    # the last sample frame: 1024 + (2 + 11 - 1) * 256 + 512 = 4 608 > 4 096; one frame less ends ON the block's last sample
    refused("leaves the audio block of 4096 samples", [(1024, 2, 11, 0, 0)], out_samples=11 * 512)
    rc, msg, _ = raw_cut(lib, eng, [(1024, 2, 9, 0, 0)], x, 2, FMT["f32"], hop, FRAMES, F32, 9 * 512)
    assert rc == _ffi.VAD_OK, msg
    refused("leaves the audio block", [(1 << 40, 0, 1, 0, 0)])
    refused("leaves the audio block", [(0, 1 << 40, 1, 0, 0)])
    refused("leaves the audio block", [(0, 0, 1 << 40, 0, 0)], out_samples=1 << 50)
    refused("channel 2 of 2", [(0, 0, 3, 0, 2)])
    refused("channel -2 of 2", [(0, 0, 3, 0, -2)])
    refused("channel 1 of 1", [(0, 0, 3, 0, 1)], audio=x.reshape(-1), channels=1)
    refused("reserved = 7 must be 0", [(0, 0, 3, 0, 0, 7)])
    refused("out_sample = -4", [(0, 0, 3, -4, 0)])
    refused("out_sample = 2 .* multiple of 4", [(0, 0, 3, 2, 0)])
    refused("out_sample = 1536 .*output of 2560 samples", [(0, 0, 3, 0, 0), (1024, 2, 3, 1536, MIX)])      # 1 536 + 1 536 > 2 560
    refused("output ranges of segments 0 and 1 overlap", [(0, 0, 3, 0, 0), (1024, 2, 2, 1532, MIX)])
    refused("output ranges of segments 1 and 0 overlap", [(0, 0, 3, 512, 0), (1024, 2, 2, 0, MIX)])
    # 2 GiB or more: sample frames x channels x bytes per sample
    refused("2 GiB", ok, audio_samples=1 << 28)
    refused("2 GiB", ok, fmt=FMT["i16_32768"], audio_samples=1 << 29)
    refused("2 GiB", ok, fmt=FMT["ulaw"], audio_samples=1 << 30)
    refused("2 GiB", ok, audio=x.reshape(-1), channels=1, fmt=FMT["ulaw"], audio_samples=1 << 31)
    refused("null buffer or bad count", ok, out_samples=-1)
    # the device form's pointers
    for device, pat in ((True, "null buffer"), (False, "no resident block|resident block has")):
        rc, msg, out = raw_cut(lib, eng, ok, None, 2, FMT["f32"], hop, FRAMES, F32, n_out, audio_samples=4095, device=device)
        assert rc == INV and re.search(pat, msg) and untouched(out), msg
    base = np.zeros(2 * 4096 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 4096]
    assert odd.ctypes.data % 8 == 4
    rc, msg, out = raw_cut(lib, eng, [(0, 0, 3, 0, 0)], odd, 2, FMT["ulaw"], hop, FRAMES, PCM16, 1536, audio_samples=4096, device=True)
    assert rc == INV and "vad_scan_cut_device: the audio block must be 8-byte aligned" in msg and untouched(out), msg
    rc, msg, out = raw_cut(lib, eng, [(0, 0, 3, 0, 0)], odd[2:], 1, FMT["ulaw"], hop, FRAMES, PCM16, 1536, audio_samples=4096, device=True)
    assert rc == INV and "must be 4-byte aligned" in msg and untouched(out), msg
    buf = np.full(1536 + 16, SENT16, np.int16)
    mis = buf[((16 - buf.ctypes.data % 16) % 16) // 2 + 4:]
    assert mis.ctypes.data % 16 == 8
    rc, msg, _ = raw_cut(lib, eng, [(0, 0, 3, 0, 0)], x, 2, FMT["f32"], hop, FRAMES, PCM16, 1536, device=True, out=mis)
    assert rc == INV and "the output must be 16-byte aligned" in msg and untouched(buf), msg
    rc, msg, _ = raw_cut(lib, eng, [(0, 0, 3, 0, 0)], x, 2, FMT["f32"], hop, FRAMES, PCM16, 1536, device=False, out=mis)
    assert rc == _ffi.VAD_OK, msg                       # host memory needs no alignment
    # no segments: fine, and nothing is written
    for device in (False, True):
        rc, msg, out = raw_cut(lib, eng, [], x, 2, FMT["f32"], hop, FRAMES, F32, n_out, device=device)
        assert rc == _ffi.VAD_OK and untouched(out), msg
    assert lib.vad_scan_cut(None, None, 0, None, 0, 1, 0, 256, -1.0, 0, 0, None, 0) == INV


def test_a_call_with_several_faults_gets_the_first_refusal(lib, make_engine):
    """The order of the checks is behaviour: frame format, channels, layout, out_fmt, hop, the 2 GiB limit, the segments, the
    output pointer, and last the device form's audio alignment.  Every fault at once, then one mended at a time."""
    eng = make_engine()
    base = np.zeros(2 * 512 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 512]          # one frame of two-channel G.711, 4 bytes off an 8-byte boundary
    faults = dict(fmt=9, channels=3, layout=2, out_fmt=2, hop=6, audio_samples=1 << 30, items=[(2, 0, 1, 0, 0)])
    mended = dict(fmt=FMT["ulaw"], channels=2, layout=RANGE, out_fmt=PCM16, hop=8, audio_samples=512, items=[(0, 0, 1, 0, 0)])
    order = (("fmt", "unknown frame format 9"), ("channels", "channels = 3"), ("layout", "layout = 2"), ("out_fmt", "out_fmt = 2"),
             ("hop", "hop = 6 must be"), ("audio_samples", "exceed the 2 GiB"), ("items", "starts at sample 2"),
             (None, "the audio block must be 8-byte aligned"))
    for device in (False, True):
        kw = dict(faults)
        for key, pattern in order:
            if key is None and not device:
                break                                           # host memory needs no alignment
            rc, msg, out = raw_cut(lib, eng, kw["items"], odd, kw["channels"], kw["fmt"], kw["hop"], kw["layout"], kw["out_fmt"], 512,
                                   audio_samples=kw["audio_samples"], device=device)
            assert rc == INV and re.search(pattern, msg) and untouched(out), (key, device, rc, msg)
            if key:
                kw[key] = mended[key]


# ---- the resident block -----------------------------------------------------------------------------------------------
def test_null_audio_cuts_the_block_the_last_scan_uploaded(lib, make_engine):
    eng = make_engine()
    frame, hop = eng.frame_samples, 256
    rng = np.random.default_rng(7)
    x = values(rng, "i16_32767", (6000, 2))
    items = [(0, 1, 4, 0, 1), (1024, 3, 2, 2048, MIX)]

    def null_cut(ns=6000, channels=2, fmt=FMT["i16_32767"]):
        return raw_cut(lib, eng, items, None, channels, fmt, hop, FRAMES, PCM16, 3072, thr=0.01, audio_samples=ns)

    rc, msg, out = null_cut()
    assert rc == INV and "no resident block" in msg and "vad_scan_cut" in msg and untouched(out), msg

    slots = eng.open_streams(2)
    nf = eng.scan_frame_count(6000, hop)
    start = np.array([0, nf, 2 * nf], np.int64)
    probs = np.zeros(2 * nf, np.float32)

    def scan(audio, channels, fmt):
        audio = np.ascontiguousarray(audio)
        ns = audio.shape[0]
        arr = (_ffi.ScanChItem * 2)(_ffi.ScanChItem(int(slots[0]), 0, 6000, 0, 0), _ffi.ScanChItem(int(slots[1]), 0, 6000, channels - 1, 0))
        rc = lib.vad_scan_channels(eng.handle, arr, 2, audio.ctypes.data, ns, channels, fmt, hop, 0.01, start.ctypes.data_as(C.POINTER(C.c_int64)),
                                   probs.ctypes.data_as(C.POINTER(C.c_float)), None, None)
        assert rc == _ffi.VAD_OK, lib.vad_last_error(eng.handle).decode()

    try:
        scan(x, 2, FMT["i16_32768"])
        rc, msg, out = null_cut()
        assert rc == INV and "resident block has frame format 2, not 1" in msg and untouched(out), msg
        scan(x.view(np.uint8).reshape(-1)[:6000].copy(), 1, FMT["ulaw"])
        rc, msg, out = null_cut(fmt=FMT["ulaw"])
        assert rc == INV and "resident block has 1 channels, not 2" in msg and untouched(out), msg
        scan(np.concatenate([x, x[:8]]), 2, FMT["i16_32767"])
        rc, msg, out = null_cut()
        assert rc == INV and "resident block has 24032 bytes, not the 24000 of 6000 samples" in msg and untouched(out), msg
        scan(x, 2, FMT["i16_32767"])
        rc, msg, got = null_cut()
        assert rc == _ffi.VAD_OK, msg
        rc, msg, explicit = raw_cut(lib, eng, items, x, 2, FMT["i16_32767"], hop, FRAMES, PCM16, 3072, thr=0.01)
        assert rc == _ffi.VAD_OK, msg
        assert got.tobytes() == explicit.tobytes() and untouched(got[3072:])
        want = np.concatenate([reference(x, "i16_32767", it, frame, hop, FRAMES, PCM16, 0.01) for it in items])
        assert np.array_equal(got[:3072], want) and np.abs(want).max() > 1000
        # an explicit block becomes the resident one
        y = values(rng, "f32", 5000)
        one = [(0, 0, 2, 0, 0)]
        rc, msg, a = raw_cut(lib, eng, one, y, 1, FMT["f32"], hop, RANGE, F32, 768)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, b = raw_cut(lib, eng, one, None, 1, FMT["f32"], hop, RANGE, F32, 768, audio_samples=5000)
        assert rc == _ffi.VAD_OK and a.tobytes() == b.tobytes() and np.array_equal(a[:768], y[:768]), msg
        rc, msg, out = null_cut()
        assert rc == INV and "resident block has frame format 0, not 1" in msg, msg
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("kw", [dict(version=4), dict(shared_gpu=True), dict(rate=8000)], ids=["v4", "shared_gpu", "v5_8k"])
def test_every_engine_cuts(lib, make_engine, kw):
    other = make_engine(**kw)
    frame = other.frame_samples
    hop = frame // 2
    rng = np.random.default_rng(3)
    x = values(rng, "alaw", (4096, 2))
    items = [(4, 1, 3, 0, 1), (4, 0, 2, 3 * frame + 4, MIX)]
    for device in (False, True):
        rc, msg, out = raw_cut(lib, other, items, x, 2, FMT["alaw"], hop, FRAMES, PCM16, 5 * frame + 4, thr=0.01, device=device)
        assert rc == _ffi.VAD_OK, (kw, msg)
        assert np.array_equal(out[:3 * frame], reference(x, "alaw", items[0], frame, hop, FRAMES, PCM16, 0.01))
        assert np.array_equal(out[3 * frame + 4:5 * frame + 4], reference(x, "alaw", items[1], frame, hop, FRAMES, PCM16, 0.01))
        assert untouched(out[3 * frame:3 * frame + 4]) and untouched(out[5 * frame + 4:])


# ---- values -----------------------------------------------------------------------------------------------------------
def _ragged(rng, frame, hop, nsamples, channels, layout):
    """segments of 1 .. 23 frames all over one block of several recordings, outputs in no order of input, gaps of 0, 4 and 8
    samples between them -> items, out_samples"""
    offs = [0, 1028, 5000]
    items, o = [], 0
    for k in range(12):
        off = offs[k % 3]
        room = (nsamples - off - frame) // hop + 1
        nf = int(rng.integers(1, min(24, room) + 1)) if k else 1
        first = int(rng.integers(0, room - nf + 1))
        ch = 0 if channels == 1 else (0, 1, MIX)[k % 3]
        items.append((off, first, nf, o, ch))
        o += (nf * frame if layout == FRAMES else (nf - 1) * hop + frame) + 4 * (k % 3)
    order = rng.permutation(len(items))
    return [items[i] for i in order], o


@pytest.mark.parametrize("gate_on", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("out_fmt", [PCM16, F32], ids=["pcm16", "f32"])
@pytest.mark.parametrize("layout", [FRAMES, RANGE], ids=["frames", "range"])
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", list(FMT))
def test_ragged_segments_against_numpy(lib, eng, kind, channels, layout, out_fmt, gate_on):
    frame = eng.frame_samples
    rng = np.random.default_rng(len(kind) * 100 + channels * 10 + layout * 4 + out_fmt * 2 + gate_on)
    hop = (frame // 2, frame // 4 + 4, frame + 4)[(layout + out_fmt + channels) % 3]
    ns = 20000
    x = values(rng, kind, (ns, 2) if channels == 2 else ns)
    thr = 0.3 if gate_on else None          # a gate that bites: about a third of uniform samples
    items, n_out = _ragged(rng, frame, hop, ns, channels, layout)
    got = {}
    for device in (False, True):
        rc, msg, out = raw_cut(lib, eng, items, x, channels, FMT[kind], hop, layout, out_fmt, n_out, thr=-1.0 if thr is None else thr,
                               device=device)
        assert rc == _ffi.VAD_OK, msg
        got[device] = out
    assert got[False].tobytes() == got[True].tobytes()
    out = got[False]
    covered = np.zeros(out.size, bool)
    for it in items:
        want = reference(x, kind, it, frame, hop, layout, out_fmt, thr)
        seg = out[it[3]:it[3] + want.size]
        assert seg.tobytes() == want.tobytes(), it
        covered[it[3]:it[3] + want.size] = True
    assert untouched(out[~covered]) and (~covered).sum() >= 8 + 12      # the gaps and the tail keep their sentinel
    if gate_on:
        assert (np.concatenate([reference(x, kind, it, frame, hop, layout, F32, thr) for it in items]) == 0).mean() > 0.1


def test_a_long_segment_spans_workgroups_in_the_stand_in_too(lib, eng):
    W, frame = _ffi.VAD_CUT_WG_SAMPLES, eng.frame_samples
    x = values(np.random.default_rng(1), "i16_32768", 3 * W + frame)
    for total in (W - 4, W, W + 4, 3 * W):
        hop = 4
        nf = (total - frame) // hop + 1
        rc, msg, out = raw_cut(lib, eng, [(0, 0, nf, 0, 0)], x, 1, FMT["i16_32768"], hop, RANGE, PCM16, total)
        assert rc == _ffi.VAD_OK, msg
        assert np.array_equal(out[:total], pcm16(decode(x[:total], "i16_32768"))) and untouched(out[total:])


# ---- the Python faces -------------------------------------------------------------------------------------------------
def test_engine_cut_and_its_argument_errors(lib, eng):
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    rng = np.random.default_rng(5)
    recs = [values(rng, "f32", (frame + 5 * hop + 3, 2)), values(rng, "f32", (frame, 2))]
    slots = np.asarray(eng.open_streams(2))
    try:
        with eng.scan_session():
            eng.scan(slots, recs, hop=hop, denoise=None)
            last = eng.last_scan
            assert last["channels"] == 2 and last["samples"] == int(last["offsets"][1]) + frame
            segs = [(0, 1, 3), (int(last["offsets"][1]), 0, 1, 1), (0, 0, 2, 0)]
            data, start = eng.cut(segs, hop=hop, denoise=0.3)
        assert data.dtype == np.int16 and list(start) == [0, 3 * frame, 4 * frame, 6 * frame]
        block = np.zeros((last["samples"], 2), np.float32)
        block[:recs[0].shape[0]] = recs[0]
        block[int(last["offsets"][1]):] = recs[1]
        want = [reference(block, "f32", (sg[0], sg[1], sg[2], 0, sg[3] if len(sg) == 4 else MIX), frame, hop, FRAMES, PCM16, 0.3) for sg in segs]
        assert np.array_equal(data, np.concatenate(want))
        # the same with the block handed over, as float32 and as the range
        data2, _ = eng.cut(segs, hop=hop, denoise=0.3, audio=block)
        assert np.array_equal(data2, data)
        assert eng.last_scan is None
        f, st = eng.cut(segs[:1], hop=hop, denoise=None, audio=block, layout="range", out="f32")
        assert f.dtype == np.float32 and np.array_equal(f, np.mean(block, axis=1)[hop:hop + 2 * hop + frame])
        mono = np.ascontiguousarray(block[:, 0])
        f, st = eng.cut([(0, 0, 1)], hop=hop, denoise=None, audio=mono, out="f32")
        assert np.array_equal(f, mono[:frame])
        u = values(rng, "ulaw", 2048)
        p, _ = eng.cut([(4, 0, 1)], hop=hop, denoise=None, audio=u, law="ulaw")
        assert np.array_equal(p, pcm16(decode(u[4:4 + frame], "ulaw")))
        # cut_device on host memory (the stand-in's device memory)
        outbuf = np.full(4 * frame + 64, SENT16, np.int16)
        al = outbuf[((16 - outbuf.ctypes.data % 16) % 16) // 2:]
        st = eng.cut_device(segs[:2], block.ctypes.data, block.shape[0], al.ctypes.data, 4 * frame + 8, hop=hop, channels=2, denoise=0.3,
                            out_start=[frame + 8, 0])
        eng.synchronize()
        assert list(st) == [0, 3 * frame, 4 * frame]
        assert np.array_equal(al[frame + 8:4 * frame + 8], want[0]) and np.array_equal(al[:frame], want[1]) and untouched(al[frame:frame + 8])
        with pytest.raises(Exception, match="layout is one of"):
            eng.cut(segs, hop=hop, audio=block, layout="both")
        with pytest.raises(Exception, match="out is one of"):
            eng.cut(segs, hop=hop, audio=block, out="wav")
        with pytest.raises(Exception, match="a segment is"):
            eng.cut([(0, 1)], hop=hop, audio=block)
        with pytest.raises(Exception, match="channel must be"):
            eng.cut([(0, 1, 2, "left")], hop=hop, audio=block)
        with pytest.raises(Exception, match="1-D or"):
            eng.cut(segs, hop=hop, audio=np.zeros((64, 3), np.float32))
        with pytest.raises(Exception, match="follows a scan"):
            eng.cut(segs, hop=hop)
        with pytest.raises(Exception, match="leaves the audio block"):
            eng.cut([(0, 40, 3)], hop=hop, audio=block)
        with pytest.raises(Exception, match="hop = 6"):
            eng.cut(segs, hop=6, audio=block)
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_cut_recordings_shape_on_a_corpus_of_both_kinds(lib, make_engine):
    from cutter_vad_amd import VADConfig, WAVWriter, cut_recordings
    from cutter_vad_amd.scan import scan_recordings
    eng = make_engine()
    frame = eng.frame_samples
    hop = frame

    def script(s, amp=1.0):
        s = list(s) + [0.0] * (15 - len(s))
        x = np.full(frame * len(s) + 3, np.float32(0.125), np.float32)      # the payloads are not silence
        x[:len(s) * hop:hop] = np.asarray(s, np.float32) * np.float32(amp)  # the stand-in's p = |first sample of the frame|
        return x

    one = [0.0] * 2 + [0.9] * 5 + [0.0] * 4
    two = [0.9] * 4 + [0.0] * 4 + [0.9] * 3 + [0.0] * 4
    none = [0.0] * 9
    st = lambda l, r: np.ascontiguousarray(np.stack([script(l), script(r)], axis=1))
    corpus = [script(one), st(two, none), script(none), st(none, one), np.zeros((0, 2), np.float32), script(two)]
    cfg = VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=0.5, vad_end_probability=0.5,
                    voice_start_frame_count=2, voice_end_frame_count=2, enable_denoising=False, output_wav_sample_rate=8000)
    opened = eng.info()["open_streams"]
    for channel in (0, 1, "mix", "split"):
        segs = scan_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel)
        for layout in ("frames", "range"):
            got = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout=layout, wav=False)
            wavs = cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=channel, layout=layout)
            assert len(got) == len(corpus)
            n = 0
            for x, s_i, g_i, w_i in zip(corpus, segs, got, wavs):
                per = [(c, s_i[c], g_i[c], w_i[c]) for c in range(len(s_i))] if channel == "split" else [(channel, s_i, g_i, w_i)]
                for c, s, g, w in per:
                    assert [(a, b) for a, b, _ in g] == s == [(a, b) for a, b, _ in w]
                    for (a, b, pcm), (_, _, wav) in zip(g, w):
                        assert isinstance(pcm, np.ndarray) and pcm.dtype == np.int16 and isinstance(wav, bytes)
                        h = x if x.ndim == 1 else heard(x, "f32", MIX if c == "mix" else c)
                        assert np.array_equal(pcm, pcm16(h[a:b]))           # hop = frame: both layouts are the range
                        assert wav == WAVWriter(8000, 16, 1).header(2 * pcm.size) + pcm.tobytes()
                        assert wav == WAVWriter(8000, 16, 1).write_wav_data(h[a:b])
                        n += 1
            assert n >= (3 if channel == "mix" else 4)      # (0.9 against silence mixes to 0.45, under the thresholds)
    assert eng.info()["open_streams"] == opened
    assert cut_recordings([], cfg, engine=eng) == []
    assert cut_recordings([script(none)], cfg, engine=eng, hop=hop) == [[]]
    for bad in ("left", 2, None):
        with pytest.raises(Exception, match="channel is 'mix', 0, 1 or 'split'"):
            cut_recordings(corpus, cfg, engine=eng, hop=hop, channel=bad)
    with pytest.raises(Exception, match="layout is 'frames' or 'range'"):
        cut_recordings(corpus, cfg, engine=eng, hop=hop, layout="both")


def test_the_kernel_file_compiles_without_scratch_or_spills(tmp_path):
    """all 16 instantiations {4 loaders} x {1, 2 channels} x {int16, float32 out} from the compiler's own metadata"""
    import shutil
    import subprocess
    from cutter_vad_amd import _build
    cc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("hipcc not found")
    assert "scan_cut.hip" in _build.HIP_SOURCES
    out = tmp_path / "scan_cut.s"
    subprocess.run([cc, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "cutter_vad_amd", "csrc", "scan_cut.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = re.findall(r"\.name:\s*(_Z13vadk_scan_cutILi(\d)ELi(\d)ELi(\d)EE\S*).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_spill_count:\s*(\d+)"
                      r".*?\.vgpr_spill_count:\s*(\d+)", text, re.S)
    assert sorted(m[1:4] for m in meta) == sorted((str(f), str(c), str(o)) for f in range(4) for c in (1, 2) for o in (0, 1)), meta
    for name, _, _, _, scratch, sspill, vspill in meta:
        assert (scratch, sspill, vspill) == ("0", "0", "0"), (name, scratch, sspill, vspill)
    # the loads and stores DESIGN 2.1h lists, per thread: one load per pass (two for two-channel float32), all of them requested
    # before the first wait - four requests in flight, not one - and one store per pass; at most 64 VGPRs = 8 waves per SIMD
    width = {("0", "1"): "dwordx4", ("1", "1"): "dwordx2", ("2", "1"): "dword", ("3", "1"): "dword",
             ("0", "2"): "dwordx4", ("1", "2"): "dwordx4", ("2", "2"): "dwordx2", ("3", "2"): "dwordx2"}
    vgprs = {n: int(v) for n, v in re.findall(r"\.name:\s*(_Z13vadk_scan_cut\S*).*?\.vgpr_count:\s*(\d+)", text, re.S)}
    for name, f, c, o, *_ in meta:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)
        ops = re.findall(r"\b(buffer_load_\w+|global_store_\w+|flat_store_\w+|s_waitcnt vmcnt)", body)
        nload = 8 if (f, c) == ("0", "2") else 4
        assert ops[:nload] == ["buffer_load_" + width[(f, c)]] * nload, (name, ops)
        assert ops[nload] == "s_waitcnt vmcnt" and not any(x.startswith("buffer_load") for x in ops[nload:]), (name, ops)
        assert [x for x in ops if "store" in x] == ["global_store_" + ("dwordx2" if o == "0" else "dwordx4")] * 4, (name, ops)
        assert vgprs[name] <= 64, (name, vgprs[name])
    assert len(vgprs) == 16
