"""Which refusal a call with several faults gets is behaviour.  walk() runs one call with every fault at once, mends one fault per
step and asserts the refusal of each step, on the host form and on the _device form (the stand-in's device memory is host memory).
The smallest shapes that reach every check: one block of 2048 sample frames, two segments of one and two frames."""
import ctypes as C
import re

import numpy as np

from cutter_vad_amd import _ffi

INV, UNS = _ffi.VAD_ERR_INVALID_ARG, _ffi.VAD_ERR_UNSUPPORTED
DEVICE = "device"               # a step only the _device form takes: host memory needs no alignment
NS = 2048


def buf(nbytes, off=0):
    """nbytes of zeros that start `off` bytes behind a 64-byte boundary"""
    base = np.zeros(nbytes + 128, np.uint8)
    at = (-base.ctypes.data) % 64 + off
    return base[at:at + nbytes]


def addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def f32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def f32(*v):
    return np.array(v, np.float32)


def i64p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def segp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(_ffi.Segment))


def i64(*v):
    return np.array(v, np.int64)


def thr(sets):
    return None if sets is None else (_ffi.Thresholds * max(1, len(sets)))(*[_ffi.Thresholds(*t) for t in sets])


def scan_items(rows):
    return (_ffi.ScanChItem * max(1, len(rows)))(*[_ffi.ScanChItem(*map(int, r)) for r in rows])


def resident(lib, eng, slots, p=((0.0, 0.0, 0.0), ())):
    """vad_scan_segments of one recording per slot whose frame t has the stand-in's probability p[i][t], hop = frame: leaves the
    per-frame results, the positions (two items of 3 and 0 frames: [0, 3, 3]), the tails' snapshot and the table resident
    -> the table's count"""
    f = eng.frame_samples
    x = np.zeros(max(4, sum(len(q) for q in p) * f), np.float32)
    rows, at = [], 0
    for s, q in zip(slots, p):
        x[at + np.arange(len(q)) * f] = q
        rows.append((s, at, len(q) * f, 0, 0))
        at += len(q) * f
    count = np.full(1, -1, np.int64)
    rc = lib.vad_scan_segments(eng.handle, scan_items(rows), len(rows), addr(x), x.size, 1, _ffi.VAD_FMT_F32, f, -1.0, None, 0, i64p(count))
    assert rc == _ffi.VAD_OK, lib.vad_last_error(eng.handle).decode()
    return int(count[0])


def cut_items(rows):
    return (_ffi.CutItem * max(1, len(rows)))(*[_ffi.CutItem(*r) for r in rows])


def mel(**kw):
    m = dict(n_fft=64, hop=16, n_bins=33, n_mels=4, pad=_ffi.VAD_MEL_PAD_NONE, log=_ffi.VAD_MEL_LN, floor=1e-5, reserved=0)
    m.update(kw)
    return _ffi.Mel(**m)


def mel_ops():
    """op_re, op_im [64][33] and filters [4][33] of mel()"""
    return np.zeros(64 * 33, np.float32), np.zeros(64 * 33, np.float32), np.zeros(4 * 33, np.float32)


def walk(lib, eng, call, faults, steps):
    """call(device, **kw) -> rc.  steps: (code, pattern, key, mended value[, DEVICE]) in the order of the checks; behind the last
    step the call is in order and passes"""
    for device in (False, True):
        kw = dict(faults)
        for step in steps:
            code, pattern, key, value = step[:4]
            if device or DEVICE not in step[4:]:
                rc = call(device, **kw)
                msg = lib.vad_last_error(eng.handle).decode()
                assert rc == code and re.search(pattern, msg), (key, device, rc, msg)
            kw[key] = value
        rc = call(device, **kw)
        assert rc == _ffi.VAD_OK, (device, rc, lib.vad_last_error(eng.handle).decode())
        eng.synchronize()


def walk_one(lib, eng, call, faults, steps):
    """walk() for an entry point whose two forms take different arguments: call(**kw) -> rc is one form.
    steps: (code, pattern, key, mended value)"""
    kw = dict(faults)
    for code, pattern, key, value in steps:
        rc = call(**kw)
        msg = lib.vad_last_error(eng.handle).decode()
        assert rc == code and re.search(pattern, msg), (key, rc, msg)
        kw[key] = value
    rc = call(**kw)
    assert rc == _ffi.VAD_OK, (rc, lib.vad_last_error(eng.handle).decode())
    eng.synchronize()
