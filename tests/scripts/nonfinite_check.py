"""Run by tests/test_nonfinite_host.py in its own process: the rejection of non-finite frames (include/vad_engine.h,
VAD_EV_REJECTED) through the real csrc/engine.cpp over the HIP stand-in of tools/san_tick/ (tests/standin.py: p = |first sample|,
the real state machine, a NaN / Inf float32 frame rejected as the kernels reject it).  Prints one JSON object."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cutter_vad_amd import _ffi, weights_io  # noqa: E402
from tests import standin  # noqa: E402

_ffi.LIB_PATH = standin.build(os.path.join(ROOT, "build", "standin"))
from cutter_vad_amd.engine import Engine  # noqa: E402

out = {}
hdr = open(os.path.join(ROOT, "include", "vad_engine.h")).read()
out["abi"] = int(re.search(r"#define VAD_ABI_VERSION (\d+)", hdr).group(1))
out["ev_rejected"] = int(re.search(r"#define VAD_EV_REJECTED (0x[0-9a-fA-F]+|\d+)", hdr).group(1), 0) == _ffi.VAD_EV_REJECTED == 0x80
out["work_rejected"] = int(re.search(r"#define VAD_WORK_REJECTED (\d+)", hdr).group(1)) == _ffi.VAD_WORK_REJECTED == 32

with open(weights_io.packaged_blob_path(5), "rb") as f:
    blob = f.read()


def frame(p, seed):
    x = (np.random.default_rng(seed).standard_normal(512) * 0.001).astype(np.float32)
    x[0] = p
    return x


with Engine(blob, model_version=5, max_streams=16) as e:
    out["abi_info"] = e.info()["abi_version"]
    slots = e.open_streams(4)
    e.step(slots, np.stack([frame(0.5, k) for k in range(4)]))
    h0 = [float(e.get_state(int(s))[0]) for s in slots]
    saved = [e.save_stream(int(s)) for s in slots]
    x = np.stack([frame(0.5, 10 + k) for k in range(4)])
    x[1, 300], x[2, 0], x[3, 511] = np.nan, np.inf, -np.inf
    p, ev, seg = e.step_events(slots, x)
    out["step_nan"] = bool(np.isnan(p[1:]).all() and np.isfinite(p[0]))
    out["step_bits"] = ev.tolist()
    out["step_seg"] = seg.tolist()
    out["step_counter"] = [float(e.get_state(int(s))[0]) - h for s, h in zip(slots, h0)]
    out["step_blob_kept"] = all(e.save_stream(int(s)) == b for s, b in zip(slots[1:], saved[1:]))

    # tick path, segments on: slot a rejects a frame during pre-roll, slot b one inside its segment; slot c is the control that
    # never saw them
    e.tick_enable_segments(True)
    a, b, c = (int(s) for s in e.open_streams(3))
    for s in (a, b, c):
        e.set_thresholds(s, 0.5, 0.3, 0.5, 0.5, 2, 2)
    talk = [0.9, 0.9, 0.9, 0.9, 0.05, 0.05, 0.05]
    bad = frame(0.9, 99)
    bad[7] = np.nan
    n_work = 2
    last_prob = np.zeros(n_work + 16, np.float32)
    frames_done = np.zeros(n_work + 16, np.int64)
    active = np.zeros(n_work + 16, np.uint8)
    cont = np.zeros(n_work + 16, np.uint8)
    kinds, evs = [], {a: [], b: [], c: []}
    held_ok = True
    for t, pr in enumerate(talk):
        f = frame(pr, 200 + t)
        for s in (a, b, c):
            e.tick_push(s, f)
        if t == 0:
            e.tick_push(a, bad)                # during pre-roll (a is idle, one frame above start)
        if t == 2:
            e.tick_push(b, bad)                # inside b's segment
        while True:
            lp, fd, ac = last_prob.copy(), frames_done.copy(), active.copy()
            slots_, gs, frames_, nsamp, widx, wkind, wsamp = e.tick_run_work(0.01, last_prob, frames_done, active, cont, cont)
            if len(slots_) == 0:
                break
            for j, k in enumerate(widx):
                if wkind[j] & _ffi.VAD_WORK_REJECTED:
                    sl = int(slots_[k])
                    kinds.append((sl, int(wkind[j])))
                    held_ok &= last_prob[sl] == lp[sl] and frames_done[sl] == fd[sl] and active[sl] == ac[sl]
            r_slots = [int(v) for v in slots_]
            for s in (a, b, c):
                if s in r_slots:
                    evs[s].append(None)
    out["work_kinds"] = sorted(set(k for _, k in kinds))
    out["work_slots"] = sorted(s for s, _ in kinds)
    out["work_held"] = bool(held_ok)
    out["a_b_c"] = [a, b, c]
    wav = {s: e.tick_take_segment_wav16(s, 16000) for s in (a, b, c)}
    out["wav_lens"] = [len(wav[s]) for s in (a, b, c)]
    out["wav_same"] = wav[a] == wav[c] and wav[b] == wav[c] and len(wav[c]) > 44
    out["frames_done"] = [int(frames_done[s]) for s in (a, b, c)]
print(json.dumps(out))
