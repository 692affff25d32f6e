"""Rejected non-finite frames on the host side, without a GPU (include/vad_engine.h, VAD_EV_REJECTED; ABI 5): the constants of the
header and the bindings, vad_step_events through the real engine.cpp, and the tick's segment assembler and work list skipping a
rejected entry - tests/scripts/nonfinite_check.py over the stand-in kernels of tools/san_tick/, in its own process."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rejected_frames_through_the_host_engine():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scripts", "nonfinite_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["abi"] == r["abi_info"] == 5 and r["ev_rejected"] and r["work_rejected"], r
    # step: NaN, the bit alone, seg 0, the state counter not advanced, the blob unchanged
    assert r["step_nan"] and r["step_bits"][1:] == [0x80] * 3 and not r["step_bits"][0] & 0x80, r
    assert r["step_seg"][1:] == [0, 0, 0] and r["step_counter"] == [1.0, 0.0, 0.0, 0.0] and r["step_blob_kept"], r
    # tick: the rejected entries are listed as VAD_WORK_REJECTED only, with the per-slot arrays left alone ...
    a, b, c = r["a_b_c"]
    assert r["work_kinds"] == [32] and r["work_slots"] == sorted([a, b]) and r["work_held"], r
    assert r["frames_done"][0] == r["frames_done"][1] == r["frames_done"][2], r
    # ... and the segment audio equals that of a stream that never saw the bad frames (pre-roll kept, no NaN frame inside)
    assert r["wav_same"], r
