"""The rule of vad_scan_moments / vad_scan_audio_batch (include/vad_engine.h) in numpy over tests/cut_ref.py (heard, gate) and
tests/batch_ref.py (convert): a segment's samples are what the float32 range cut gives, the moments are Python integers, a cell is
one float32 add and one float32 multiply, each a numpy ufunc that rounds where it stands.  Nothing here has a tolerance: the tests
compare bytes.  No test, no library."""
import numpy as np

from tests.batch_ref import F32, PAD_FEATURE, PAD_VALUE, convert
from tests.cut_ref import gate, heard

f32 = np.float32


def segment(block, kind, item, frame, hop, thr):
    """item = (sample_offset, first_frame, nframes, out_sample, channel) -> the float32 samples of its range once"""
    off, first, nf, _, ch = item[:5]
    a = off + first * hop
    return np.ascontiguousarray(gate(heard(block, kind, ch), thr)[a:a + (nf - 1) * hop + frame], np.float32)


def moments(x):
    """-> (sum_q31, energy_q32) of finite float32 samples, as Python integers"""
    x = np.asarray(x, np.float32).astype(np.float64)
    s = np.rint(np.clip(x, -1.0, 1.0) * 2147483648.0)
    e = np.minimum(np.rint(x * x * 4294967296.0), 4294967296.0)
    return sum(int(v) for v in s), sum(int(v) for v in e)


def moments_records(segments):
    from cutter_vad_amd import _ffi
    out = np.zeros(len(segments), _ffi.MOMENTS_DTYPE)
    for i, x in enumerate(segments):
        out[i] = moments(x)
    return out


def batch(segments, windows, T, dtype=F32, pad_mode=PAD_VALUE, pad_value=0.0, shift=None, scale=None):
    """segments: the float32 samples of each; windows: (seg, nsamples, sample0) each -> ([B, T] in the dtype's numpy form - bfloat16:
    uint16 bits -, mask [B, T] uint8)"""
    sh = np.zeros(1, np.float32) if shift is None else np.asarray(shift, np.float32).reshape(-1)
    sc = np.ones(1, np.float32) if scale is None else np.asarray(scale, np.float32).reshape(-1)
    out = np.zeros((len(windows), T), np.float32)
    mask = np.zeros((len(windows), T), np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (seg, ns, s0) in enumerate(windows):
            seg, ns, s0 = int(seg), int(ns), int(s0)
            s_, c_ = sh[seg if sh.size > 1 else 0], sc[seg if sc.size > 1 else 0]
            out[k, :ns] = (segments[seg][s0:s0 + ns] + s_) * c_
            out[k, ns:] = (f32(0.0) + s_) * c_ if pad_mode == PAD_FEATURE else f32(pad_value)
            mask[k, :ns] = 1
    return convert(out, dtype), mask
