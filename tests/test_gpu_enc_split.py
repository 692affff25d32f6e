"""The 16-stream kernel's encoder.0 as a direct 3-tap convolution on the exact three-piece bf16 split (S_ENC0_X3): the headline
shape (8 192 streams, one frame per call, two workgroups per CU) against the f64 oracle for the 16 kHz model and its 8 kHz
sub-model, and a ragged batch against the 32-stream tiles, whose encoder.0 is still the fp32 Toom-3 product."""

import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests.signals import make_streams

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sr", [16000, 8000])
def test_split_encoders_8192_streams_against_the_f64_oracle(sr):
    from cutter_vad_amd.engine import Engine
    from oracle import oracle
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    om = oracle.OracleModel(blob, "f64")
    L = om.frame_samples
    n, T = 8192, 6
    x = make_streams(n, T, seed=7300 + sr // 1000)
    if L != 512:
        x = np.ascontiguousarray(x.reshape(n, -1, L)[:, :T])
    with Engine(blob, model_version=5, max_streams=n, sample_rate=sr) as eng:
        eng.set_tile(16)
        slots = eng.open_streams(n)
        st = np.zeros((n, 256), np.float32)
        worst = 0.0
        for t in range(T):
            got = eng.step(slots, np.ascontiguousarray(x[:, t]))
            ref = om.step_batch(oracle.denoise(x[:, t]).reshape(n, L), st, nthreads=8)
            worst = max(worst, float(np.abs(got - ref).max()))
        dev = np.stack([eng.get_state(int(s)) for s in slots[:: 512]])
    assert worst <= 2e-6, worst
    assert np.abs(dev - st[:: 512]).max() <= 2e-5


def test_split_encoders_37_streams_against_the_32_stream_tiles():
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        blob = f.read()
    n, T = 37, 7
    x = make_streams(n, T, seed=7400)
    with Engine(blob, model_version=5, max_streams=256) as eng:
        slots = eng.open_streams(n)
        eng.set_tile(16)
        p16, ev16 = eng.step_multi(slots, x)                 # T frames in one launch
        eng.reset(slots)
        one = np.stack([eng.step(slots, x[:, t]) for t in range(T)], axis=1)   # the single-frame instantiation
        eng.set_tile(32)
        eng.reset(slots)
        p32, ev32 = eng.step_multi(slots, x)
    assert np.array_equal(one, p16)
    assert np.abs(p16 - p32).max() <= 2e-6
