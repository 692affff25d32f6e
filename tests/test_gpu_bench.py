"""bench.py on the GPU, on a small pool (the plumbing, not the headline): a plain run prints the contract's line without the
CPU leg, and `--dump-outputs` writes what the timed path's last step computed - the same arrays in every run with the same
arguments, and what the oracle computes for those W + K ring frames from zero state."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cutter_vad_amd import weights_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS, STEPS, WARMUP = 512, 7, 2


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--streams", str(STREAMS), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip() == json.dumps(lines[0])
    return lines[0], {n[:-len(".npy")]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}


def test_plain_run_line_and_dumped_outputs_repeat_and_match_the_oracle(tmp_path):
    a, da = _bench(tmp_path / "a")
    b, db = _bench(tmp_path / "b")
    assert a["steps"] == STEPS and a["warmup"] == WARMUP and a["unit"] == "frames/s" and a["dtype"] == "f32"
    assert a["higher_is_better"] is True and a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(STREAMS / (a["ms_per_step"] * 1e-3))
    assert "cpu_baseline" not in a and "parity" not in a                       # the CPU leg runs with --full only
    assert sorted(da) == ["events", "probs"]
    for k in da:
        assert da[k].dtype == np.float32 and da[k].shape == (STREAMS,)
        assert np.array_equal(da[k], db[k]), k                                  # same arguments, same outputs
    # the last timed step is step W + K - 1 from zero state over ring frames 0, 1, ...: replay it in the f64 oracle
    import bench
    from oracle import oracle
    ring = bench.synth_ring(0, STREAMS)
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        om = oracle.OracleModel(f.read(), "f64")
    st = np.zeros((STREAMS, 256), np.float32)
    for i in range(WARMUP + STEPS):
        ref = om.step_batch(oracle.denoise(ring[i % bench.RING]).reshape(STREAMS, 512), st, nthreads=8)
    assert float(np.abs(da["probs"] - ref).max()) <= 1e-4
