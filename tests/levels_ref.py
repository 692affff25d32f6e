"""The rule of vad_scan_levels (include/vad_engine.h: vad_level) in numpy, for tests/test_scan_levels_host.py (the CPU stand-in) and
tests/test_gpu_scan_levels.py (the GPU): the levels of a segment are statistics of exactly the float32 values a VAD_CUT_RANGE,
VAD_CUT_F32 cut writes for it.  No test, no library: importing it loads neither the stand-in nor the engine."""
import numpy as np

from cutter_vad_amd import _ffi


def levels_ref(x, thr=0.95):
    """float32 samples of one segment -> (energy_q32, peak, clipped)"""
    x = np.asarray(x, np.float32)
    q = np.minimum(np.rint(x.astype(np.float64) ** 2 * 2.0 ** 32), 2.0 ** 32).astype(np.int64).sum()
    peak = np.abs(x).max() if x.size else np.float32(0)
    clipped = (np.abs(x) >= np.float32(thr)).sum()
    return int(q), np.float32(peak), int(clipped)


def records(payloads, thr=0.95):
    """the float32 payloads of a call's segments -> the records vad_scan_levels writes for them (a structured array)"""
    out = np.zeros(len(payloads), _ffi.LEVEL_DTYPE)
    for i, p in enumerate(payloads):
        out[i] = levels_ref(p, thr)
    return out


def of_cut(eng, segments, clip=0.95, **kw):
    """the records of `segments` from the EXISTING cut: Engine.cut(layout="range", out="f32") with the same arguments, then numpy"""
    data, start = eng.cut(segments, layout="range", out="f32", **kw)
    return records([data[start[i]:start[i + 1]] for i in range(len(start) - 1)], clip)
