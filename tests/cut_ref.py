"""The numpy reference and the call helpers of the vad_scan_cut tests (tests/test_scan_cut_host.py over the CPU stand-in,
tests/test_gpu_scan_cut.py on the GPU): the wire format decoded from utils/g711.py's tables and IEEE quotients, np.mean of a
two-channel pair, the strict gate, np.clip(x * 32767, -32768, 32767).astype(np.int16).  No test, no library: importing it loads
neither the stand-in nor the engine."""
import numpy as np

from cutter_vad_amd import _ffi
from tests import g711_ref as G

FMT = {"f32": _ffi.VAD_FMT_F32, "i16_32767": _ffi.VAD_FMT_I16_32767, "i16_32768": _ffi.VAD_FMT_I16_32768,
       "ulaw": _ffi.VAD_FMT_ULAW8, "alaw": _ffi.VAD_FMT_ALAW8}
MIX = _ffi.VAD_SCAN_MIX
FRAMES, RANGE = _ffi.VAD_CUT_FRAMES, _ffi.VAD_CUT_RANGE
PCM16, F32 = _ffi.VAD_CUT_PCM16, _ffi.VAD_CUT_F32
INV = _ffi.VAD_ERR_INVALID_ARG


def decode(x, kind):
    """the wire format -> the float32 the model reads"""
    if kind == "f32":
        return np.asarray(x, np.float32)
    if kind.startswith("i16"):
        return x.astype(np.float32) / np.float32(32767.0 if kind == "i16_32767" else 32768.0)
    return G.table(kind)[x].astype(np.float32) / np.float32(32768.0)


def heard(block, kind, channel):
    """a [ns] or [ns, 2] block -> the float32 stream of `channel` (0, 1 or MIX: np.mean of the decoded pair)"""
    d = decode(block, kind)
    if d.ndim == 1:
        return d
    return np.mean(d, axis=1) if channel == MIX else np.ascontiguousarray(d[:, channel])


def gate(x, thr):
    """utils/audio.py: np.where(np.abs(x) > thr, x, 0); None: no gate"""
    return x if thr is None else np.where(np.abs(x) > np.float32(thr), x, np.float32(0.0)).astype(np.float32)


def pcm16(x):
    """utils/wav_writer.py:41"""
    return np.clip(x * 32767, -32768, 32767).astype(np.int16)


def reference(block, kind, item, frame, hop, layout, out_fmt, thr):
    """item = (sample_offset, first_frame, nframes, out_sample, channel) -> the segment's samples"""
    off, first, nf, _, ch = item[:5]
    x = gate(heard(block, kind, ch), thr)
    a = off + first * hop
    if layout == RANGE:
        seg = x[a:a + (nf - 1) * hop + frame]
    else:
        seg = np.concatenate([x[a + j * hop:a + j * hop + frame] for j in range(nf)])
    return seg.astype(np.float32) if out_fmt == F32 else pcm16(seg)


def values(rng, kind, shape):
    if kind == "f32":
        return rng.uniform(-1.2, 1.2, shape).astype(np.float32)
    if kind.startswith("i16"):
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return rng.integers(0, 256, shape).astype(np.uint8)


SENT16, SENT32 = np.int16(0x5A5A), np.float32(-7.0)


def raw_cut(lib, eng, items, audio, channels, fmt, hop, layout, out_fmt, out_samples, thr=-1.0, audio_samples=None, device=False,
            out=None):
    """vad_scan_cut (or _device: the stand-in's device memory is host memory) -> (rc, message, out); items: (sample_offset,
    first_frame, nframes, out_sample, channel[, reserved]); `out` is pre-filled with a sentinel; audio None = the resident block"""
    arr = (_ffi.CutItem * max(1, len(items)))(*[_ffi.CutItem(*map(int, it)) for it in items])
    if out is None:
        out = np.full(min(max(out_samples, 0), 1 << 20) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)
    ptr = None
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    else:
        ns = audio_samples
    if device:
        rc = lib.vad_scan_cut_device(eng.handle, arr, len(items), ptr, ns, channels, fmt, hop, thr, layout, out_fmt, out.ctypes.data,
                                     out_samples, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_cut(eng.handle, arr, len(items), ptr, ns, channels, fmt, hop, thr, layout, out_fmt, out.ctypes.data, out_samples)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def untouched(out):
    return bool((out == (SENT32 if out.dtype == np.float32 else SENT16)).all())
