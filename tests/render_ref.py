"""The rule of vad_scan_render in numpy, and the call helper of its tests (tests/test_scan_render_host.py over the CPU stand-in,
tests/test_gpu_scan_render.py on the GPU).  A segment's starting values are the float32 that tests/cut_ref.reference(.., RANGE,
F32, ..) gives - the wire format decoded, the channel selected, the strict gate; from there float32 multiplies and adds only: the
gain, the fade-in entry, the fade-out entry, the sum of two segments, then the cut's conversion.  No test, no library."""
import numpy as np

from cutter_vad_amd import _ffi
from tests.cut_ref import F32, RANGE, SENT16, SENT32, pcm16, reference


def faded(v, ramp):
    """w[k] = (v[k] * a[k]) * b[k]: a = ramp[k] where k < nramp, b = ramp[S - 1 - k] where S - 1 - k < nramp, else 1.0f"""
    v = np.asarray(v, np.float32)
    ramp = np.zeros(0, np.float32) if ramp is None else np.asarray(ramp, np.float32)
    m = min(ramp.size, v.size)
    a = np.ones(v.size, np.float32)
    b = np.ones(v.size, np.float32)
    a[:m] = ramp[:m]
    b[v.size - m:] = ramp[:m][::-1]
    w = (v * a).astype(np.float32)
    return (w * b).astype(np.float32)


def render(block, kind, items, frame, hop, out_fmt, thr, out_samples, ramp=None, gains=None):
    """items = (sample_offset, first_frame, nframes, out_sample, channel) each -> out[0 .. out_samples): +0.0f where no segment
    covers a sample, w itself where one does (a -0.0f stays), w_i + w_j where two do; three are the caller's mistake.
    frame: the samples of a frame in the block (a chunk of a rate block, whose thr is None: never gated)"""
    acc = np.zeros(out_samples, np.float32)
    cover = np.zeros(out_samples, np.int32)
    for i, it in enumerate(items):
        v = reference(block, kind, it, frame, hop, RANGE, F32, thr)
        if gains is not None:
            v = (v * np.float32(gains[i])).astype(np.float32)
        w = faded(v, ramp)
        o = int(it[3])
        first = cover[o:o + w.size] == 0
        acc[o:o + w.size] = np.where(first, w, (acc[o:o + w.size] + w).astype(np.float32))
        cover[o:o + w.size] += 1
    assert cover.max(initial=0) <= 2
    return acc if out_fmt == F32 else pcm16(acc)


def raw_render(lib, eng, items, audio, channels, fmt, hop, out_fmt, out_samples, thr=-1.0, ramp=None, gains=None, sr_in=0,
               audio_samples=None, device=False, nramp=None, null_out=False, null_ramp=False):
    """vad_scan_render (or _device: the stand-in's device memory is host memory) -> (rc, message, out); `out` is pre-filled with a
    sentinel and has 8 samples more than the call may write; audio None = the resident block"""
    arr = (_ffi.CutItem * max(1, len(items)))(*[_ffi.CutItem(*map(int, it)) for it in items])
    out = np.full(min(max(out_samples, 0), 1 << 22) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)
    ptr = None
    if audio is not None:
        audio = np.ascontiguousarray(audio)
        ptr = audio.ctypes.data
        ns = audio.size // max(channels, 1) if audio_samples is None else audio_samples
    else:
        ns = audio_samples
    r = np.zeros(0, np.float32) if ramp is None else np.ascontiguousarray(ramp, np.float32)
    g = None if gains is None else np.ascontiguousarray(gains, np.float32)
    fp = _ffi.C.POINTER(_ffi.C.c_float)
    head = (eng.handle, arr, len(items), None if g is None else g.ctypes.data_as(fp), None if (null_ramp or r.size == 0) else r.ctypes.data_as(fp),
            r.size if nramp is None else nramp, ptr, ns, channels, fmt, sr_in, hop, thr, out_fmt, None if null_out else out.ctypes.data,
            out_samples)
    if device:
        rc = lib.vad_scan_render_device(*head, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_render(*head)
    return rc, lib.vad_last_error(eng.handle).decode(), out
