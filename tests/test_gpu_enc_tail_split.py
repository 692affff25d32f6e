"""encoder.2 and encoder.3 of the 16-stream Silero V5 kernels on the bf16 split (silero_v5_t16_body.h: enc1's output and enc2's
output as activation planes, the weight ring running on from enc1 through both layers into the LSTM's input half): 37 streams -
three tiles, the last with five live streams, an odd tile count for pairing - of float32 and int16 frames at both rates.  Single
frames against the f64 oracle; the same frames as one multi-frame call (the frame loop re-uses rows 0..47 and the rows at T_ROW_E)
bit for bit, and against the 32-stream tiles; the paired entry against the unpaired one bit for bit."""
import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests.signals import make_streams

pytestmark = pytest.mark.gpu
N, T = 37, 6
PAIR, NO_PAIR = -3, -4


def _blob(sr):
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        return f.read()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def frames():
    """{(sr, kind): [N][T][frame]} of make_streams signals, computed once and left unchanged"""
    out = {}
    base = make_streams(N, T, seed=1137)
    for sr in (16000, 8000):
        x = base if sr == 16000 else np.ascontiguousarray(base.reshape(N, -1, 256)[:, :T])
        xi = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
        for kind, a in (("f32", x), ("i16", xi)):
            a.setflags(write=False)
            out[sr, kind] = a
    return out


@pytest.fixture(scope="module")
def single(frames):
    """(a)'s run, shared with (b): {(sr, kind): (probs [N][T], events [N][T], saved streams)} of T single-frame steps on 16-stream tiles"""
    from cutter_vad_amd.engine import Engine
    out = {}
    for sr in (16000, 8000):
        with Engine(_blob(sr), model_version=5, max_streams=64, sample_rate=sr) as eng:
            eng.set_tile(16)
            slots = eng.open_streams(N)
            for kind in ("f32", "i16"):
                x = frames[sr, kind]
                eng.reset(slots)
                pe = [eng.step_events(slots, np.ascontiguousarray(x[:, t])) for t in range(T)]
                p = np.stack([a[0] for a in pe], axis=1)
                ev = np.stack([a[1] for a in pe], axis=1)
                state = np.stack([eng.get_state(int(s)) for s in slots])
                out[sr, kind] = (p, ev, [eng.save_stream(int(s)) for s in slots], state)
    return out


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_single_frame_steps_against_the_f64_oracle(frames, single, sr, kind):
    from oracle import oracle
    om = oracle.OracleModel(_blob(sr), "f64")
    L = om.frame_samples
    x = frames[sr, kind]
    xf = x if kind == "f32" else (x.astype(np.float32) / np.float32(32767.0))
    p, _, _, state = single[sr, kind]
    st = np.zeros((N, 256), np.float32)
    worst = 0.0
    for t in range(T):
        ref = om.step_batch(oracle.denoise(np.ascontiguousarray(xf[:, t])).reshape(N, L), st, nthreads=4)
        worst = max(worst, float(np.abs(p[:, t] - ref).max()))
    ds = float(np.abs(state - st).max())
    print(f"{sr} Hz {kind}: max |dp| = {worst:.3e}, max |dstate| = {ds:.3e}")
    assert worst <= 2e-6, worst
    assert ds <= 2e-5, ds


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_one_multi_frame_call_leaves_the_bits_of_the_single_frames(frames, single, sr, kind):
    from cutter_vad_amd.engine import Engine
    x = frames[sr, kind]
    p1, ev1, saved1, _ = single[sr, kind]
    with Engine(_blob(sr), model_version=5, max_streams=64, sample_rate=sr) as eng:
        slots = eng.open_streams(N)
        eng.set_tile(16)
        p16, ev16 = eng.step_multi(slots, x)
        saved16 = [eng.save_stream(int(s)) for s in slots]
        eng.set_tile(32)
        eng.reset(slots)
        p32, _ = eng.step_multi(slots, x)
    assert np.array_equal(_bits(p16), _bits(p1))
    assert np.array_equal(ev16, ev1)
    assert saved16 == saved1
    d = float(np.abs(p16 - p32).max())
    print(f"{sr} Hz {kind}: max |p16 - p32| = {d:.3e}")
    assert d <= 2e-6, d


@pytest.mark.parametrize("n", [37, 16])
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_paired_at_every_size_equals_never_paired(frames, n, kind):
    from cutter_vad_amd.engine import Engine
    x = frames[16000, kind][:n]
    with Engine(_blob(16000), model_version=5, max_streams=64) as eng:
        slots = eng.open_streams(n)
        got = {}
        for mode in (NO_PAIR, PAIR):
            eng.reset(slots)
            eng.set_tile(mode)
            out = []
            for t in range(T):
                p, ev, seg = eng.step_events(slots, np.ascontiguousarray(x[:, t]))
                out += [_bits(p), ev, seg]
            out.append(np.stack([_bits(eng.get_state(int(s))) for s in slots]))
            out.append([eng.save_stream(int(s)) for s in slots])
            got[mode] = out
        eng.set_tile(0)
    for i, (u, v) in enumerate(zip(got[NO_PAIR], got[PAIR])):
        assert (u == v) if isinstance(u, list) else np.array_equal(u, v), i
    assert not np.array_equal(got[PAIR][0][: n // 2], got[PAIR][0][n - n // 2:])      # the streams do differ
