"""The 16-stream kernel's LSTM on the exact three-piece bf16 split (S_LSTM_X3, v_mfma_f32_16x16x32_bf16): the headline shape
(8 192 streams, one frame per call, two workgroups per CU) against the f64 oracle, and a ragged batch against the 32-stream tiles,
whose LSTM still runs on fp32 MFMAs."""

import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests.signals import make_streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blob():
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        return f.read()


def test_split_lstm_8192_streams_against_the_f64_oracle(blob):
    from cutter_vad_amd.engine import Engine
    from oracle import oracle
    om = oracle.OracleModel(blob, "f64")
    n, T = 8192, 6
    x = make_streams(n, T, seed=7100)
    with Engine(blob, model_version=5, max_streams=n) as eng:
        eng.set_tile(16)
        slots = eng.open_streams(n)
        st = np.zeros((n, 256), np.float32)
        worst = 0.0
        for t in range(T):
            got = eng.step(slots, x[:, t])
            ref = om.step_batch(oracle.denoise(x[:, t]).reshape(n, 512), st, nthreads=8)
            worst = max(worst, float(np.abs(got - ref).max()))
        dev = np.stack([eng.get_state(int(s)) for s in slots[:: 512]])
    assert worst <= 2e-6, worst
    assert np.abs(dev - st[:: 512]).max() <= 2e-5


def test_split_lstm_45_streams_against_the_32_stream_tiles(blob):
    from cutter_vad_amd.engine import Engine
    n, T = 45, 8
    x = make_streams(n, T, seed=7200)
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
