"""vad_scan_rate_segments / vad_scan_rate_cut / vad_rate_cut_samples on the host side: exports, sample counts, refusals, the tables
of a cut of frames (rows, tiles, windows) and the bookkeeping of the two kinds of resident block - the real csrc/engine.cpp over the
HIP stand-in (tests/standin.py).  The stand-in's resample launches write frames of zeros whose first sample is the chunk's first
decoded sample, and its model makes p = |first sample of the frame|.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.core.exceptions import AudioProcessingError
from tests import cut_ref as R
from tests import standin
from tests.cut_ref import F32, FMT, FRAMES, INV, MIX, PCM16, RANGE, SENT16, raw_cut, untouched
from tests.rate_cut_ref import rate_cut, rate_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vad_scan_rate_segments", "vad_rate_cut_samples", "vad_scan_rate_cut", "vad_scan_rate_cut_device"]
CHUNK = {8000: 256, 24000: 768, 48000: 1536}
UNSUPPORTED = _ffi.VAD_ERR_UNSUPPORTED


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


def test_header_ctypes_table_and_library_agree_on_the_additions(lib):
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        header = f.read()
    declared = re.findall(r"VAD_API\s+[\w\s\*]+?\b(vad_\w+)\s*\(", header)
    for name in NEW:
        assert declared.count(name) == 1, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "#define VAD_ABI_VERSION 5" in header


def test_sample_counts(lib, make_engine):
    eng = make_engine()
    for sr, chunk in CHUNK.items():
        for hop in (chunk // 2, chunk, 4, chunk + 4):
            for nf in (1, 2, 33, 1000):
                assert lib.vad_rate_cut_samples(eng.handle, nf, sr, hop, FRAMES) == nf * 512
                assert lib.vad_rate_cut_samples(eng.handle, nf, sr, hop, RANGE) == (nf - 1) * hop + chunk
                assert eng.cut_samples(nf, hop, "frames", sample_rate=sr) == nf * 512
                assert eng.cut_samples(nf, hop, "range", sample_rate=sr) == (nf - 1) * hop + chunk
        assert eng.cut_samples(3, sample_rate=sr, layout="range") == 2 * chunk          # the default hop: half a chunk
    for nf, hop, lay in ((5, 256, FRAMES), (5, 256, RANGE), (1, 512, RANGE), (7, 4, FRAMES)):
        assert lib.vad_rate_cut_samples(eng.handle, nf, 16000, hop, lay) == lib.vad_cut_samples(eng.handle, nf, hop, lay) > 0
    for bad in ((0, 8000, 128, FRAMES), (-1, 8000, 128, RANGE), (3, 8000, 0, FRAMES), (3, 8000, 6, FRAMES), (3, 8000, -128, RANGE),
                (3, 8000, 128, 2), (3, 8000, 128, -1), (3, 44100, 128, FRAMES), (3, 0, 128, FRAMES), (3, 16000, 6, FRAMES),
                (1 << 62, 48000, 768, RANGE)):
        assert lib.vad_rate_cut_samples(eng.handle, *bad) == -1, bad
    assert lib.vad_rate_cut_samples(None, 3, 8000, 128, FRAMES) == -1
    with pytest.raises(AudioProcessingError):
        eng.cut_samples(0, sample_rate=8000)


def test_refusals_have_a_status_the_functions_name_and_write_nothing(lib, make_engine):
    eng = make_engine()
    sr, chunk, hop = 24000, 768, 384
    x = np.zeros(8192, np.float32)                      # room for 20 chunks
    ok = [(0, 0, 3, 0, 0), (1536, 1, 4, 1536, 0)]
    for device in (False, True):
        for lay, total in ((FRAMES, 3584), (RANGE, 1536 + 3 * hop + chunk)):
            rc, msg, out = rate_cut(lib, eng, ok, x, 1, FMT["f32"], sr, hop, lay, PCM16, total, device=device)
            assert rc == _ffi.VAD_OK and (out[:total] == 0).all() and untouched(out[total:]), msg

    def refused(code, pattern, items, audio=x, channels=1, fmt=FMT["f32"], rate=sr, h=hop, layout=FRAMES, out_fmt=PCM16, out_samples=3584,
                named=True, **kw):
        for device in (False, True):
            rc, msg, out = rate_cut(lib, eng, items, audio, channels, fmt, rate, h, layout, out_fmt, out_samples, device=device, **kw)
            assert rc == code, (rc, msg)
            assert re.search(pattern, msg), msg
            if named:
                assert "vad_scan_rate_cut_device" in msg if device else re.search(r"vad_scan_rate_cut\b(?!_)", msg), msg
            assert untouched(out)                       # a refused call writes nothing

    for h in (0, 2, 6, -384, 386):
        refused(INV, "hop", ok, h=h)
    refused(INV, "layout", ok, layout=2)
    refused(INV, "out_fmt", ok, out_fmt=2)
    refused(INV, "channels = 3", ok, channels=3)
    refused(INV, "multiple of 4", [(2, 0, 3, 0, 0)])
    refused(INV, "first_frame", [(0, -1, 3, 0, 0)])
    refused(INV, "nframes", [(0, 0, 0, 0, 0)])
    # the block-bounds check with the chunk as the frame: 20 chunks fit (19 * 384 + 768 = 8064), 21 do not
    rc, msg, out = rate_cut(lib, eng, [(0, 0, 20, 0, 0)], x, 1, FMT["f32"], sr, hop, FRAMES, PCM16, 20 * 512)
    assert rc == _ffi.VAD_OK, msg
    refused(INV, "leaves the audio block", [(0, 0, 21, 0, 0)], out_samples=21 * 512)
    refused(INV, "leaves the audio block", [(0, 1, 20, 0, 0)], out_samples=20 * 512)
    refused(INV, "leaves the audio block", [(7428, 0, 1, 0, 0)])       # 7428 + 768 > 8192
    refused(INV, "names channel 1 of 1", [(0, 0, 3, 0, 1)])
    refused(INV, "reserved", [(0, 0, 3, 0, 0, 5)])
    refused(INV, "out_sample", [(0, 0, 3, 2, 0)])
    refused(INV, "out_sample", [(0, 0, 3, -4, 0)])
    refused(INV, "out_sample", ok, out_samples=3580)                    # the second segment's 2048 samples end at 3584
    refused(INV, "out_sample", ok, layout=RANGE, out_samples=1536 + 3 * hop + chunk - 4)
    refused(INV, "overlap", [(0, 0, 3, 0, 0), (1536, 1, 4, 1532, 0)])
    refused(INV, "2 GiB", ok, audio_samples=1 << 29)
    refused(INV, "2 GiB", ok, channels=2, audio_samples=1 << 28)
    refused(INV, "unknown frame format 9", ok, fmt=9, named=False)       # (every entry point's message, as vad_scan_cut's)
    for rate in (44100, 32000, 0, -8000, 16001):
        refused(UNSUPPORTED, "supported input rates are 8000, 16000, 24000, 48000", ok, rate=rate)
    # null buffers
    arr = (_ffi.CutItem * 1)(_ffi.CutItem(0, 0, 3, 0, 0, 0))
    assert lib.vad_scan_rate_cut(eng.handle, arr, 1, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, -1.0, FRAMES, PCM16, None, 2048) == INV
    assert "vad_scan_rate_cut: null buffer" in lib.vad_last_error(eng.handle).decode()
    assert lib.vad_scan_rate_cut_device(eng.handle, arr, 1, None, 8192, 1, FMT["f32"], sr, hop, -1.0, FRAMES, PCM16, x.ctypes.data, 2048, None) == INV
    assert "vad_scan_rate_cut_device: null buffer" in lib.vad_last_error(eng.handle).decode()
    assert lib.vad_scan_rate_cut(None, arr, 1, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, -1.0, FRAMES, PCM16, x.ctypes.data, 2048) == INV
    # the device block's alignment: 4 bytes, 8 for two channels; the output's: 16
    base = np.zeros(2 * 8192 + 16, np.uint8)
    odd = base[(4 - base.ctypes.data) % 8:][:2 * 8192]
    rc, msg, out = rate_cut(lib, eng, [(0, 0, 3, 0, MIX)], odd, 2, FMT["ulaw"], sr, hop, FRAMES, PCM16, 1536, audio_samples=8192, device=True)
    assert rc == INV and "vad_scan_rate_cut_device: the audio block must be 8-byte aligned" in msg and untouched(out), msg
    rc, msg, out = rate_cut(lib, eng, [(0, 0, 3, 0, 0)], odd[2:], 1, FMT["ulaw"], sr, hop, FRAMES, PCM16, 1536, audio_samples=8192, device=True)
    assert rc == INV and "must be 4-byte aligned" in msg and untouched(out), msg
    buf = np.full(4096 + 16, SENT16, np.int16)
    mis = buf[((16 - buf.ctypes.data % 16) % 16) // 2 + 2:][:4096]
    rc, msg, out = rate_cut(lib, eng, [(0, 0, 3, 0, 0)], x, 1, FMT["f32"], sr, hop, FRAMES, PCM16, 1536, device=True, out=mis)
    assert rc == INV and "vad_scan_rate_cut_device: the output must be 16-byte aligned" in msg and untouched(mis), msg
    # n == 0 is VAD_OK and touches nothing
    rc, msg, out = rate_cut(lib, eng, [], x, 1, FMT["f32"], sr, hop, FRAMES, PCM16, 64)
    assert rc == _ffi.VAD_OK and untouched(out)

    # an engine of the 8 kHz sub-model has no 512-sample frames to deliver: every rate is refused, 16000 included
    other = make_engine(rate=8000)
    for device in (False, True):
        for rate in (8000, 16000, 24000, 48000):
            ch = CHUNK.get(rate, 512)
            for lay in (FRAMES, RANGE):
                rc, msg, out = rate_cut(lib, other, [(0, 0, 2, 0, 0)], x, 1, FMT["f32"], rate, ch // 2, lay, PCM16, 4096, device=device)
                assert rc == UNSUPPORTED and "8 kHz sub-model" in msg and "vad_scan_rate_cut" in msg and untouched(out), (rate, rc, msg)
    # Silero V4 and shared-GPU engines cut: no model runs
    for kw in (dict(version=4), dict(shared_gpu=True)):
        other = make_engine(**kw)
        y = np.arange(8192, dtype=np.float32) / np.float32(8192.0)
        for device in (False, True):
            rc, msg, out = rate_cut(lib, other, [(0, 1, 3, 0, 0)], y, 1, FMT["f32"], sr, hop, FRAMES, F32, 1536, device=device)
            assert rc == _ffi.VAD_OK, (kw, msg)
            assert np.array_equal(out[:1536:512], y[hop:4 * hop:hop]) and untouched(out[1536:])
            rc, msg, out = rate_cut(lib, other, [(0, 1, 3, 0, 0)], y, 1, FMT["f32"], sr, hop, RANGE, F32, 1536, device=device)
            assert rc == _ffi.VAD_OK and np.array_equal(out[:1536], y[hop:hop + 1536]), (kw, msg)


def test_segments_refusals_are_vad_scan_rates_under_the_new_name(lib, make_engine):
    eng = make_engine()
    a, b = (int(s) for s in eng.open_streams(2))
    sr, hop = 24000, 384
    x = np.zeros(8192, np.float32)
    ok = [(a, 0, 1536), (b, 1536, 2304)]
    rc, msg, table, count = rate_segments(lib, eng, ok, x, 1, FMT["f32"], sr, hop)
    assert rc == _ffi.VAD_OK and count == 0, msg

    def refused(code, pattern, items, audio=x, channels=1, fmt=FMT["f32"], rate=sr, h=hop, named=True):
        rc, msg, table, count = rate_segments(lib, eng, items, audio, channels, fmt, rate, h)
        assert rc == code and re.search(pattern, msg), (rc, msg)
        assert not named or "vad_scan_rate_segments" in msg, msg
        assert count == -5 and not table.size           # a refused call writes nothing

    for h in (0, 2, 6, -384, 386):
        refused(INV, "hop", ok, h=h)
    refused(INV, "multiple of 4", [(a, 2, 1536), (b, 1536, 2304)])
    refused(INV, "leaves the audio block", [(a, 0, 1536), (b, 6144, 2304)])
    refused(INV, "channels = 3", ok, channels=3)
    refused(INV, "names channel 1 of 1", [(a, 0, 1536, 1), (b, 1536, 2304)])
    refused(INV, "reserved", [(a, 0, 1536, 0, 5), (b, 1536, 2304)])
    refused(INV, "format", ok, fmt=9, named=False)
    refused(_ffi.VAD_ERR_BAD_SLOT, "twice", [(a, 0, 1536), (a, 1536, 2304)], named=False)
    for rate in (44100, 0, -8000, 16001):
        refused(UNSUPPORTED, "supported input rates are 8000, 16000, 24000, 48000", ok, rate=rate)
    arr = (_ffi.ScanChItem * 2)(*[_ffi.ScanChItem(*it, 0, 0) for it in ok])
    count = C.c_int64(-5)
    tab = np.zeros(4, _ffi.SEGMENT_DTYPE)
    tp = tab.ctypes.data_as(C.POINTER(_ffi.Segment))
    assert lib.vad_scan_rate_segments(eng.handle, arr, 2, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, -1.0, tp, -1, C.byref(count)) == INV
    assert "vad_scan_rate_segments: seg_cap" in lib.vad_last_error(eng.handle).decode()
    assert lib.vad_scan_rate_segments(eng.handle, arr, 2, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, -1.0, tp, 4, None) == INV
    assert lib.vad_scan_rate_segments(eng.handle, arr, 2, x.ctypes.data, 8192, 1, FMT["f32"], sr, hop, -1.0, None, 4, C.byref(count)) == INV
    assert lib.vad_scan_rate_segments(eng.handle, arr, 2, None, 8192, 1, FMT["f32"], sr, hop, -1.0, tp, 4, C.byref(count)) == INV
    assert "vad_scan_rate_segments: null buffer" in lib.vad_last_error(eng.handle).decode() and count.value == -5
    for kw, pattern in ((dict(version=4), "needs a Silero V5 engine"), (dict(shared_gpu=True), "VAD_ENGINE_SHARED_GPU"),
                        (dict(rate=8000), "8 kHz sub-model")):
        other = make_engine(**kw)
        s = [int(v) for v in other.open_streams(2)]
        for rate in (8000, 24000, 48000):
            ch = CHUNK[rate]
            rc, msg, table, count = rate_segments(lib, other, [(s[0], 0, 2 * ch), (s[1], 2 * ch, 3 * ch)], x, 1, FMT["f32"], rate, ch // 2)
            assert rc == UNSUPPORTED and re.search(pattern, msg) and "vad_scan_rate_segments" in msg and count == -5, (kw, rate, rc, msg)


def _block(rng, kind, ns, two):
    return R.values(rng, kind, (ns, 2) if two else (ns,))


@pytest.mark.parametrize("sr,kind,two,hop_name", [(8000, "f32", False, "half"), (24000, "i16_32767", True, "half"), (48000, "ulaw", False, "half"),
                                                  (24000, "alaw", True, "chunk"), (8000, "i16_32768", False, "hop4"), (48000, "f32", True, "half")])
@pytest.mark.parametrize("window", [0, 1])
def test_frames_start_with_their_chunks_first_sample_and_range_is_the_block_itself(lib, make_engine, sr, kind, two, hop_name, window):
    """FRAMES through the stand-in: frame j of segment i = zeros behind the decoded, channel-selected (and, resampled value that it
    stands for, gated) sample at offset + (first + j) * hop.  RANGE = cut_ref.reference with frame = chunk and NO gate, whatever
    threshold is passed.  Segments listed out of order, with gaps between their output ranges; window = 1: 32 rows per window, so the
    70-frame segment spans three windows and the tile table is walked across segments of one frame."""
    eng = make_engine()
    chunk = CHUNK[sr]
    hop = {"half": chunk // 2, "chunk": chunk, "hop4": 4}[hop_name]
    rng = np.random.default_rng(sr // 1000 + len(kind) + 7 * two)
    ns = 4096 + 72 * hop + chunk
    block = _block(rng, kind, ns, two)
    ch = (lambda k: (0, 1, MIX)[k % 3]) if two else (lambda k: 0)
    shapes = [(0, 0, 1), (4, 1, 2), (0, 3, 31), (1024, 0, 32), (8, 5, 33), (4096, 2, 70), (0, 3, 31), (4092, 7, 1), (16, 0, 64), (0, 9, 1), (0, 10, 1)]
    order = [5, 0, 9, 10, 3, 1, 7, 2, 8, 6, 4]           # not monotonic in the block, nor in length
    thr = 0.01
    lib.vad_debug_scan_launch_frames(eng.handle, window)
    try:
        for layout in (FRAMES, RANGE):
            for out_fmt in (PCM16, F32):
                items, pos = [], 0
                for k, idx in enumerate(order):
                    off, first, nf = shapes[idx]
                    count = nf * 512 if layout == FRAMES else (nf - 1) * hop + chunk
                    pos += 4 * (k % 3)                  # gaps of 0, 4 and 8 samples in front of the segments
                    items.append((off, first, nf, pos, ch(k)))
                    pos += (count + 3) & ~3
                total = pos + 12
                for device in (False, True):
                    rc, msg, out = rate_cut(lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, layout, out_fmt, total, thr=thr,
                                            device=device)
                    assert rc == _ffi.VAD_OK, msg
                    written = np.zeros(out.size, bool)
                    for it in items:
                        off, first, nf, o, c = it
                        if layout == RANGE:
                            want = R.reference(block, kind, it, chunk, hop, RANGE, out_fmt, None)
                        else:
                            x = R.heard(block, kind, c)
                            f = np.zeros((nf, 512), np.float32)
                            f[:, 0] = R.gate(x[off + first * hop:off + (first + nf) * hop:hop][:nf], thr)
                            want = f.reshape(-1) if out_fmt == F32 else R.pcm16(f.reshape(-1))
                        assert np.array_equal(out[o:o + want.size], want), (layout, out_fmt, device, it)
                        written[o:o + want.size] = True
                    assert untouched(out[~written]) and (~written).sum() > 20
    finally:
        lib.vad_debug_scan_launch_frames(eng.handle, 0)


@pytest.mark.parametrize("sr,kind,two,gate,out_fmt", [(24000, "i16_32767", False, 0.01, PCM16), (48000, "f32", True, None, F32)],
                         ids=["24000-i16-mono-gate-pcm16", "48000-f32-stereo-nogate-f32"])
def test_cut_windows_of_32_64_and_160_rows_change_no_byte(lib, make_engine, sr, kind, two, gate, out_fmt):
    """tests/test_gpu_scan_rate_cut.py's SEGS table (300 rows) over its block at hop = chunk / 2, under launch caps 1, 2 and 5: windows
    of 32, 64 and 160 rows, every boundary inside a segment, tiles that three segments share.  The stand-in's cut reads window row
    r - r0 through the per-window CutSeg {(lo - r0) * 128, (hi - lo) * 128, quad_out + (lo - row0) * 128}, and refuses a tile_seg entry
    that does not own its tile's first row: the payload is the uncapped call's, and frame j of a segment = zeros behind the gated
    first sample of its chunk."""
    from tests.test_gpu_scan_rate_cut import SEGS, _block, _items
    eng = make_engine()
    chunk = CHUNK[sr]
    hop = chunk // 2
    assert sum(nf for _, _, nf in SEGS) == 300
    block, offs, lens = _block(kind, sr, hop, two, seed=53)
    items, total = _items(SEGS, offs, hop, chunk, FRAMES, two)
    thr = -1.0 if gate is None else gate
    outs = {}
    try:
        for cap in (0, 1, 2, 5):
            lib.vad_debug_scan_launch_frames(eng.handle, cap)
            for device in (False, True):
                rc, msg, out = rate_cut(lib, eng, items, block, 2 if two else 1, FMT[kind], sr, hop, FRAMES, out_fmt, total, thr=thr, device=device)
                assert rc == _ffi.VAD_OK, (cap, msg)
                outs[cap, device] = out
    finally:
        lib.vad_debug_scan_launch_frames(eng.handle, 0)
    base = outs[0, False]
    written = np.zeros(base.size, bool)
    for off, first, nf, o, c in items:
        f = np.zeros((nf, 512), np.float32)
        f[:, 0] = R.gate(R.heard(block, kind, c)[off + first * hop:off + (first + nf) * hop:hop][:nf], gate)
        want = f.reshape(-1) if out_fmt == F32 else R.pcm16(f.reshape(-1))
        assert np.array_equal(base[o:o + want.size], want), (off, first, nf)
        written[o:o + want.size] = True
    assert untouched(base[~written]) and (~written).sum() >= 12 + 8 and base[written].any()
    for key, out in outs.items():
        assert out.tobytes() == base.tobytes(), key


def test_a_float_chunk_with_a_nan_completes(lib, make_engine):
    eng = make_engine()
    x = np.full(4 * 256, 0.25, np.float32)
    x[300] = np.nan
    rc, msg, out = rate_cut(lib, eng, [(0, 0, 4, 0, 0)], x, 1, FMT["f32"], 8000, 256, FRAMES, F32, 2048, thr=0.01)
    assert rc == _ffi.VAD_OK and np.array_equal(out[0:2048:512][[0, 2, 3]], np.full(3, 0.25, np.float32)), msg


def test_the_two_kinds_of_resident_block_exclude_each_other(lib, make_engine):
    eng = make_engine()
    slots = eng.open_streams(1)
    s = int(slots[0])
    sr, chunk, hop = 24000, 768, 384
    rng = np.random.default_rng(3)
    x = rng.integers(-3000, 3000, 6000).astype(np.int16)
    fmt = FMT["i16_32767"]
    items = [(0, 1, 4, 0, 0)]
    want = None
    try:
        # a rate scan to segments leaves a rate block: the rate cut of NULL gives the bytes of the cut with the audio
        rc, msg, table, count = rate_segments(lib, eng, [(s, 0, 6000)], x, 1, fmt, sr, hop)
        assert rc == _ffi.VAD_OK, msg
        for layout, n_out in ((FRAMES, 2048), (RANGE, 3 * hop + chunk)):
            rc, msg, want = rate_cut(lib, eng, items, x, 1, fmt, sr, hop, layout, PCM16, n_out)
            assert rc == _ffi.VAD_OK, msg
            rc, msg, table, count = rate_segments(lib, eng, [(s, 0, 6000)], x, 1, fmt, sr, hop)
            assert rc == _ffi.VAD_OK, msg
            rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, sr, hop, layout, PCM16, n_out, audio_samples=6000)
            assert rc == _ffi.VAD_OK and np.array_equal(out, want) and not untouched(out[:n_out]), msg
        # ... and names what differs
        for kw, pattern in ((dict(sr=48000), "sample rate 24000, not 48000"), (dict(sr=8000), "sample rate 24000, not 8000"),
                            (dict(fmt=FMT["i16_32768"]), "frame format"), (dict(channels=2, audio_samples=3000), "1 channels, not 2"),
                            (dict(audio_samples=5996), "12000 bytes, not the 11992")):
            a = dict(sr=sr, fmt=fmt, channels=1, audio_samples=6000)
            a.update(kw)
            ch = CHUNK[a["sr"]]
            rc, msg, out = rate_cut(lib, eng, [(0, 0, 1, 0, 0)], None, a["channels"], a["fmt"], a["sr"], ch // 2, FRAMES, PCM16, 512,
                                    audio_samples=a["audio_samples"])
            assert rc == INV and pattern in msg and "vad_scan_rate_cut" in msg and "audio = NULL" in msg and untouched(out), (kw, msg)
        # a rate block is none of vad_scan_cut's: today's message, also at sr_in = 16000 through the new entry point
        rc, msg, out = raw_cut(lib, eng, items, None, 1, fmt, 256, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == INV and "no resident block" in msg and re.search(r"vad_scan_cut\b", msg) and untouched(out), msg
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, 16000, 256, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == INV and "no resident block" in msg and untouched(out), msg
        # the refusals left the rate block where it was
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, sr, hop, RANGE, PCM16, 3 * hop + chunk, audio_samples=6000)
        assert rc == _ffi.VAD_OK and np.array_equal(out, want), msg
        # vad_scan_rate leaves nothing, for either cut
        eng.scan(slots, [x], denoise=None, sample_rate=sr)
        assert eng.last_scan is None
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, sr, hop, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == INV and "no resident rate block" in msg and "vad_scan_rate_cut" in msg and untouched(out), msg
        rc, msg, out = raw_cut(lib, eng, items, None, 1, fmt, 256, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == INV and "no resident block" in msg and untouched(out), msg
        # a rate cut with an audio uploads a rate block ...
        rc, msg, want = rate_cut(lib, eng, items, x, 1, fmt, sr, hop, FRAMES, F32, 2048)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, sr, hop, FRAMES, F32, 2048, audio_samples=6000)
        assert rc == _ffi.VAD_OK and np.array_equal(out, want), msg
        # ... a 16 kHz scan replaces it with a block of vad_scan_cut's, which the rate cut takes at sr_in = 16000 alone
        eng.scan(slots, [x], hop=256, denoise=None)
        rc, msg, want = raw_cut(lib, eng, items, None, 1, fmt, 256, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, 16000, 256, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == _ffi.VAD_OK and np.array_equal(out, want), msg
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, sr, hop, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == INV and "no resident rate block" in msg and untouched(out), msg
        # ... as does a vad_scan_cut with an audio, and vad_scan_rate_segments at 16 kHz IS vad_scan_segments
        rc, msg, out = rate_cut(lib, eng, items, x, 1, fmt, sr, hop, FRAMES, PCM16, 2048)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = raw_cut(lib, eng, items, x, 1, fmt, 256, FRAMES, PCM16, 2048)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = rate_cut(lib, eng, items, None, 1, fmt, sr, hop, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == INV and "no resident rate block" in msg, msg
        rc, msg, table, count = rate_segments(lib, eng, [(s, 0, 6000)], x, 1, fmt, 16000, 256)
        assert rc == _ffi.VAD_OK, msg
        rc, msg, out = raw_cut(lib, eng, items, None, 1, fmt, 256, FRAMES, PCM16, 2048, audio_samples=6000)
        assert rc == _ffi.VAD_OK and np.array_equal(out, want), msg
    finally:
        eng.close_stream(s)


def _scripted(chunk, hop, scripts):
    recs = []
    for k, s in enumerate(scripts):
        x = np.zeros(chunk + (s.size - 1) * hop + k if s.size else 9, np.float32)
        x[:s.size * hop:hop] = s
        recs.append(x)
    return recs


SCRIPTS = [np.array([0.0] * 3 + [0.9] * 6 + [0.0] * 5 + [0.8] * 4 + [0.0] * 4 + [0.9] * 2, np.float32),
           np.array([0.9] * 5, np.float32), np.zeros(0, np.float32), np.array([0.7] * 4 + [0.0] * 3, np.float32)]


@pytest.mark.parametrize("sr", [8000, 24000, 48000])
def test_the_table_is_the_per_frame_scans_and_the_engine_cuts_behind_it(lib, make_engine, sr):
    from tests import seg_ref
    eng = make_engine()
    chunk = CHUNK[sr]
    hop = chunk // 2
    recs = _scripted(chunk, hop, SCRIPTS)
    thresholds = (0.5, 0.5, 0.8, 0.95, 2, 2)
    slots = eng.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, thresholds)
        before = eng.info()
        probs, ev, seg = eng.scan(slots, recs, hop=hop, denoise=None, sample_rate=sr)
        per_frame = eng.info()
        states = [eng.save_stream(int(s)) for s in slots]
        eng.reset(slots)
        eng.set_thresholds_many(slots, thresholds)
        table = eng.scan_segments(slots, recs, hop=hop, denoise=None, sample_rate=sr)
        after = eng.info()
        assert [eng.save_stream(int(s)) for s in slots] == states
        assert after["steps"] - per_frame["steps"] == per_frame["steps"] - before["steps"] > 0
        assert after["frames"] - per_frame["frames"] == per_frame["frames"] - before["frames"] == sum(s.size for s in SCRIPTS)
        start = np.concatenate([[0], np.cumsum([p.size for p in probs])])
        want = seg_ref.table(np.concatenate(ev), np.concatenate(seg), np.concatenate(probs), start)
        assert table.tobytes() == want.tobytes() and table.size == 3
        last = eng.last_scan
        assert last is not None and last["rate"] == sr
        # seg_cap = 1: the count, one record, and the rest from the table that stayed
        eng.reset(slots)
        eng.set_thresholds_many(slots, thresholds)
        offs = last["offsets"]
        block = np.zeros(int(last["samples"]), np.float32)
        for r, o in zip(recs, offs):
            block[o:o + r.size] = r
        rc, msg, one, count = rate_segments(lib, eng, [(int(s), int(o), r.size) for s, o, r in zip(slots, offs, recs)], block, 1, FMT["f32"],
                                            sr, hop, cap=1)
        assert rc == _ffi.VAD_OK and count == 3 and one.tobytes() == want[:1].tobytes(), msg
        rest = np.zeros(2, _ffi.SEGMENT_DTYPE)
        assert lib.vad_scan_segments_read(eng.handle, 1, 2, rest.ctypes.data_as(C.POINTER(_ffi.Segment))) == _ffi.VAD_OK
        assert rest.tobytes() == want[1:].tobytes()
        # Engine.cut(audio=None) behind the rate scan = the cut with the audio passed
        eng._scan_last = last
        segs = [(int(offs[r["item"]]), int(r["first_frame"]), int(r["nframes"])) for r in table]
        for layout in ("frames", "range"):
            got, gs = eng.cut(segs, hop=hop, denoise=0.01, layout=layout)
            assert [int(b - a) for a, b in zip(gs[:-1], gs[1:])] == [eng.cut_samples(sg[2], hop, layout, sample_rate=sr) for sg in segs]
            eng._scan_last = last
            same, _ = eng.cut(segs, hop=hop, denoise=0.01, layout=layout, sample_rate=sr)
            assert np.array_equal(got, same)
            with pytest.raises(AudioProcessingError, match="sample_rate"):
                eng.cut(segs, hop=hop, layout=layout, sample_rate=8000 if sr != 8000 else 48000)
            with pytest.raises(AudioProcessingError, match="sample_rate"):
                eng.cut(segs, hop=hop, layout=layout, sample_rate=16000)
            passed, ps = eng.cut(segs, hop=hop, denoise=0.01, layout=layout, audio=block, sample_rate=sr)
            assert np.array_equal(passed, got) and np.array_equal(ps, gs) and got.any()
            assert eng.last_scan is None
            eng._scan_last = last                       # (the block passed IS the scan's: the engine's resident block did not change)
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_scan_and_cut_recordings_take_the_table_path(lib, make_engine):
    from cutter_vad_amd import VADConfig
    from cutter_vad_amd.scan import _frame_stats, cut_recordings, scan_recordings
    from cutter_vad_amd.utils.wav_writer import WAVWriter
    eng = make_engine()
    sr, chunk = 48000, 1536
    hop = chunk // 2
    recs = _scripted(chunk, hop, SCRIPTS)
    recs[3] = np.stack([recs[3], recs[3]], axis=1)       # a 2-D recording in a 1-D corpus
    cfg = VADConfig(sample_rate=16000, buffer_size=512, vad_start_probability=0.5, vad_end_probability=0.5,
                    voice_start_frame_count=2, voice_end_frame_count=2, enable_denoising=True)
    calls = []
    real = eng.scan_segments
    eng.scan_segments = lambda *a, **kw: (calls.append(kw.get("sample_rate")), real(*a, **kw))[1]
    try:
        ranges = scan_recordings(recs, cfg, engine=eng, sample_rate=sr)
        stats = scan_recordings(recs, cfg, engine=eng, sample_rate=sr, stats=True)
        assert calls == [sr] * 4 and [len(r) for r in ranges] == [2, 0, 0, 1]
        # the per-frame path's statistics, exactly
        slots = eng.open_streams(4)
        try:
            eng.set_thresholds_many(slots, (0.5, 0.5, 0.8, 0.95, 2, 2))
            for i in (0, 3):
                probs, ev, seg = eng.scan(slots[i:i + 1], [recs[i]], hop=hop, denoise=0.01, sample_rate=sr)
                want = [(a, b) + _frame_stats(probs[0], ev[0], (b - chunk) // hop, (b - a - chunk) // hop + 1) for a, b in ranges[i]]
                assert stats[i] == want and want
        finally:
            for s in slots:
                eng.close_stream(int(s))
        frames = cut_recordings(recs, cfg, engine=eng, sample_rate=sr)
        own = cut_recordings(recs, cfg, engine=eng, sample_rate=sr, layout="range")
        h16, hsr = WAVWriter(cfg.output_wav_sample_rate, 16, 1), WAVWriter(sr, 16, 1)
        for i, rec in enumerate(recs):
            x = R.heard(rec, "f32", MIX)
            assert [sg[:2] for sg in frames[i]] == [sg[:2] for sg in own[i]] == ranges[i]
            for (a, b, wav), (_, _, rng) in zip(frames[i], own[i]):
                nf = (b - a - chunk) // hop + 1
                f = np.zeros((nf, 512), np.float32)
                f[:, 0] = R.gate(x[a:a + nf * hop:hop], 0.01)
                raw = R.pcm16(f.reshape(-1)).tobytes()
                assert wav == h16.header(len(raw)) + raw
                raw = R.pcm16(x[a:b]).tobytes()
                assert rng == hsr.header(len(raw)) + raw and hsr.header(len(raw)) != h16.header(len(raw))
    finally:
        del eng.scan_segments
