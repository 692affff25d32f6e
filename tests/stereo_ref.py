"""The rule of vad_scan_cut_stereo / vad_scan_render_stereo in numpy, and the call helpers of their tests
(tests/test_scan_stereo_host.py over the CPU stand-in, tests/test_gpu_scan_stereo.py on the GPU).  The rule IS the mono one per
channel: value (k, c) is what tests/cut_ref.reference / tests/render_ref.render give with every item's channel = c, so the
references call those once per channel and interleave.  No test, no library."""
import numpy as np

from cutter_vad_amd import _ffi
from tests.cut_ref import F32, SENT16, SENT32, reference
from tests.render_ref import render

BOTH = _ffi.VAD_SCAN_BOTH


def interleave(left, right):
    """two [k] arrays -> [k, 2]"""
    return np.ascontiguousarray(np.stack([left, right], axis=1))


def cut_stereo_ref(block, kind, item, frame, hop, layout, out_fmt, thr, gain=None):
    """item = (sample_offset, first_frame, nframes, out_sample[, ...]) -> the segment's sample frames [k, 2]; gain: one float32
    multiply of the gated float32, ahead of the conversion (None: no factor)"""
    cols = []
    for c in (0, 1):
        v = reference(block, kind, tuple(item[:4]) + (c,), frame, hop, layout, F32, thr)
        if gain is not None:
            v = (v * np.float32(gain)).astype(np.float32)
        cols.append(v if out_fmt == F32 else np.clip(v * 32767, -32768, 32767).astype(np.int16))
    return interleave(*cols)


def render_stereo_ref(block, kind, items, frame, hop, out_fmt, thr, out_samples, ramp=None, gains=None):
    """items = (sample_offset, first_frame, nframes, out_sample[, ...]) each -> [out_samples, 2]"""
    return interleave(*[render(block, kind, [tuple(it[:4]) + (c,) for it in items], frame, hop, out_fmt, thr, out_samples, ramp, gains)
                        for c in (0, 1)])


def _items(items):
    """(sample_offset, first_frame, nframes, out_sample[, channel[, reserved]]): the channel defaults to VAD_SCAN_BOTH"""
    rows = [tuple(map(int, it)) for it in items]
    rows = [it + (BOTH,) if len(it) == 4 else it for it in rows]
    return (_ffi.CutItem * max(1, len(rows)))(*[_ffi.CutItem(*it) for it in rows])


def _block(audio, channels, audio_samples):
    if audio is None:
        return None, audio_samples, None
    audio = np.ascontiguousarray(audio)
    return audio.ctypes.data, (audio.size // max(channels, 1) if audio_samples is None else audio_samples), audio


def sentinel_out(out_fmt, out_samples, cap=1 << 22):
    """room for out_samples sample frames and 8 values more, pre-filled with the sentinel of tests/cut_ref.untouched"""
    return np.full(2 * min(max(out_samples, 0), cap) + 8, SENT32 if out_fmt == F32 else SENT16, np.float32 if out_fmt == F32 else np.int16)


def raw_cut_stereo(lib, eng, items, audio, channels, fmt, hop, layout, out_fmt, out_samples, thr=-1.0, gains=None, sr_in=0,
                   audio_samples=None, device=False, out=None, null_out=False):
    """vad_scan_cut_stereo (or _device: the stand-in's device memory is host memory) -> (rc, message, out): `out` is flat,
    2 * out_samples values and 8 more, pre-filled with a sentinel; audio None = the resident block"""
    arr = _items(items)
    if out is None:
        out = sentinel_out(out_fmt, out_samples)
    ptr, ns, _keep = _block(audio, channels, audio_samples)
    g = None if gains is None else np.ascontiguousarray(gains, np.float32)
    fp = _ffi.C.POINTER(_ffi.C.c_float)
    head = (eng.handle, arr, len(items), None if g is None else g.ctypes.data_as(fp), ptr, ns, channels, fmt, sr_in, hop, thr, layout, out_fmt,
            None if null_out else out.ctypes.data, out_samples)
    if device:
        rc = lib.vad_scan_cut_stereo_device(*head, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_cut_stereo(*head)
    return rc, lib.vad_last_error(eng.handle).decode(), out


def raw_render_stereo(lib, eng, items, audio, channels, fmt, hop, out_fmt, out_samples, thr=-1.0, ramp=None, gains=None, sr_in=0,
                      audio_samples=None, device=False, nramp=None, null_out=False):
    """vad_scan_render_stereo (or _device) -> (rc, message, out), `out` as in raw_cut_stereo"""
    arr = _items(items)
    out = sentinel_out(out_fmt, out_samples)
    ptr, ns, _keep = _block(audio, channels, audio_samples)
    r = np.zeros(0, np.float32) if ramp is None else np.ascontiguousarray(ramp, np.float32)
    g = None if gains is None else np.ascontiguousarray(gains, np.float32)
    fp = _ffi.C.POINTER(_ffi.C.c_float)
    head = (eng.handle, arr, len(items), None if g is None else g.ctypes.data_as(fp), None if r.size == 0 else r.ctypes.data_as(fp),
            r.size if nramp is None else nramp, ptr, ns, channels, fmt, sr_in, hop, thr, out_fmt, None if null_out else out.ctypes.data,
            out_samples)
    if device:
        rc = lib.vad_scan_render_stereo_device(*head, None)
        if rc == 0:
            eng.synchronize()
    else:
        rc = lib.vad_scan_render_stereo(*head)
    return rc, lib.vad_last_error(eng.handle).decode(), out
