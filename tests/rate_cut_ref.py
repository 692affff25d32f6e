"""The call helpers of the vad_scan_rate_cut / vad_scan_rate_segments tests (tests/test_scan_rate_cut_host.py over the CPU stand-in,
tests/test_gpu_scan_rate_cut.py on the GPU), next to tests/cut_ref.py, whose numpy reference they share.  No test, no library:
importing it loads neither the stand-in nor the engine."""
import ctypes as C

import numpy as np

from cutter_vad_amd import _ffi
from tests.cut_ref import F32, SENT16, SENT32


def rate_cut(lib, eng, items, audio, channels, fmt, sr, hop, layout, out_fmt, out_samples, thr=-1.0, audio_samples=None, device=False,
             out=None):
    """vad_scan_rate_cut (or _device: the stand-in's device memory is host memory) -> (rc, message, out); items: (sample_offset,
    first_frame, nframes, out_sample, channel[, reserved]); `out` is pre-filled with a sentinel; audio None = the resident block"""
    arr = (_ffi.CutItem * max(1, len(items)))(*[_ffi.CutItem(*map(int, it)) for it in items])
    if out is None:
        # (a call that is expected to succeed writes out_samples samples: larger outputs are the caller's to allocate)
        assert out_samples <= 1 << 24, "pass an `out` of out_samples + 8 samples"
        out = np.full(max(out_samples, 0) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)
    ptr = None
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    else:
        ns = audio_samples
    if device:
        rc = lib.vad_scan_rate_cut_device(eng.handle, arr, len(items), ptr, ns, channels, fmt, sr, hop, thr, layout, out_fmt, out.ctypes.data,
                                          out_samples, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_rate_cut(eng.handle, arr, len(items), ptr, ns, channels, fmt, sr, hop, thr, layout, out_fmt, out.ctypes.data, out_samples)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def rate_segments(lib, eng, items, audio, channels, fmt, sr, hop, cap=64, thr=-1.0):
    """vad_scan_rate_segments -> (rc, message, table[:min(count, cap)], count)"""
    arr = (_ffi.ScanChItem * max(1, len(items)))(*[_ffi.ScanChItem(*map(int, (tuple(it) + (0, 0))[:5])) for it in items])
    audio = np.ascontiguousarray(audio)
    table = np.zeros(cap, _ffi.SEGMENT_DTYPE)
    count = C.c_int64(-5)
    rc = lib.vad_scan_rate_segments(eng.handle, arr, len(items), audio.ctypes.data, audio.shape[0], channels, fmt, sr, hop, thr,
                                    table.ctypes.data_as(C.POINTER(_ffi.Segment)), cap, C.byref(count))
    return rc, lib.vad_last_error(eng.handle).decode(), table[:max(0, min(cap, count.value))], count.value
