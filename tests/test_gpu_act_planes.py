"""The 16-stream kernel with its split activations as planes in LDS (silero_v5_t16.hip: the tensors that feed the bf16-split layers
- h, the |STFT| columns, the LSTM input - are cut once by the lane that produces them): the headline shape against the f64 oracle for
both sample rates, the single-frame and multi-frame instantiations against each other and against the 32-stream tiles, the
rejected-frame hold of a multi-frame float32 call (h_{t-1} is no longer in LDS as fp32: the lane keeps it), and the fused
resample -> step launch against the two-launch chain."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests.signals import make_streams

pytestmark = pytest.mark.gpu
REJ = _ffi.VAD_EV_REJECTED


def _blob(sr=16000):
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        return f.read()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("sr", [16000, 8000])
def test_planes_8192_streams_against_the_f64_oracle(sr):
    from cutter_vad_amd.engine import Engine
    from oracle import oracle
    blob = _blob(sr)
    om = oracle.OracleModel(blob, "f64")
    L = om.frame_samples
    n, T = 8192, 6
    x = make_streams(n, T, seed=8100 + sr // 1000)
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
    print(f"{sr} Hz: max |dp| = {worst:.3e}, max |dstate| = {np.abs(dev - st[:: 512]).max():.3e}")
    assert worst <= 2e-6, worst
    assert np.abs(dev - st[:: 512]).max() <= 2e-5


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("as_int16", [False, True])
def test_planes_ragged_batch_single_frame_equals_multi_frame_and_the_32_stream_tiles(sr, as_int16):
    from cutter_vad_amd.engine import Engine
    blob = _blob(sr)
    n, T = 37, 7
    x = make_streams(n, T, seed=8200)
    if sr == 8000:
        x = np.ascontiguousarray(x.reshape(n, -1, 256)[:, :T])
    if as_int16:
        x = np.round(x * 32767.0).astype(np.int16)
    with Engine(blob, model_version=5, max_streams=256, sample_rate=sr) as eng:
        slots = eng.open_streams(n)
        eng.set_tile(16)
        p16, ev16 = eng.step_multi(slots, x)                 # T frames in one launch
        s16 = [eng.save_stream(int(s)) for s in slots]
        eng.reset(slots)
        one = np.stack([eng.step(slots, np.ascontiguousarray(x[:, t])) for t in range(T)], axis=1)   # the single-frame instantiation
        s1 = [eng.save_stream(int(s)) for s in slots]
        eng.set_tile(32)
        eng.reset(slots)
        p32, ev32 = eng.step_multi(slots, x)
    assert np.array_equal(_bits(one), _bits(p16))
    assert s1 == s16
    print(f"{sr} Hz int16={as_int16}: max |p16 - p32| = {np.abs(p16 - p32).max():.3e}")
    assert np.abs(p16 - p32).max() <= 2e-6


@pytest.mark.parametrize("sr", [16000, 8000])
def test_planes_multi_frame_hold_of_a_rejected_frame_continues_bit_identically(sr):
    """float32, T frames per launch on 16-stream tiles: a stream with a non-finite frame in the MIDDLE of the call (and one each with
    it first and last) goes on exactly as the same stream stepped without that frame - probabilities, events and the saved state."""
    from cutter_vad_amd.engine import Engine
    F = 512 if sr == 16000 else 256
    n, T = 53, 5
    rng = np.random.default_rng(8300 + sr // 1000)
    with Engine(_blob(sr), model_version=5, max_streams=256, sample_rate=sr) as eng:
        eng.set_tile(16)
        slots = eng.open_streams(n)
        eng.step(slots, (rng.standard_normal((n, F)) * 0.3).astype(np.float32))
        before = [eng.save_stream(int(s)) for s in slots]
        x = (rng.standard_normal((n, T, F)) * 0.3).astype(np.float32)
        rej = {4: 2, 17: 2, 21: 0, 36: T - 1, 52: 1}          # stream -> rejected frame
        for k, (i, t) in enumerate(rej.items()):
            x[i, t, (97 * i) % F] = (np.nan, np.inf, -np.inf)[k % 3]
        p, ev = eng.step_multi(slots, x)
        after = [eng.save_stream(int(s)) for s in slots]
        one = np.array(sorted(rej))
        keep = np.array([[t for t in range(T) if t != rej[i]] for i in one])
        assert all(ev[i, rej[i]] == REJ and np.isnan(p[i, rej[i]]) for i in one)
        clean = np.setdiff1d(np.arange(n), one)
        assert np.isfinite(p[clean]).all() and not (ev[clean] & REJ).any()
        for s, b in zip(slots, before):
            eng.restore_stream(int(s), b)
        pc, evc = eng.step_multi(slots[one], x[one[:, None], keep])
        assert np.array_equal(_bits(p[one[:, None], keep]), _bits(pc)) and np.array_equal(ev[one[:, None], keep], evc)
        assert all(after[i] == b for i, b in zip(one, (eng.save_stream(int(s)) for s in slots[one])))
        # and the streams without a rejected frame do not depend on their neighbours' flags
        for s, b in zip(slots, before):
            eng.restore_stream(int(s), b)
        pk, evk = eng.step_multi(slots[clean], x[clean])
        assert np.array_equal(_bits(p[clean]), _bits(pk)) and np.array_equal(ev[clean], evk)


def test_planes_fused_rates_launch_against_the_two_launch_chain():
    from cutter_vad_amd.engine import Engine
    rates = ((8000, 256, 333), (24000, 768, 500), (48000, 1536, 411), (16000, 512, 90))
    B, T = sum(r[2] for r in rates), 4
    base = make_streams(B, T * 3, seed=8400).reshape(B, -1)
    starts = np.cumsum([0] + [r[2] for r in rates])
    with Engine(_blob(), model_version=5, max_streams=B) as eng, Engine(_blob(), model_version=5, max_streams=B) as two:
        slots, slots2 = eng.open_streams(B), two.open_streams(B)
        worst = 0.0
        for t in range(T):
            segs = [(np.ascontiguousarray(base[starts[k]:starts[k + 1], t * n_in:(t + 1) * n_in]), sr) for k, (sr, n_in, _) in enumerate(rates)]
            p, ev, _ = eng.step_rates(segs, slots)
            f16 = np.concatenate([two.resample(a, sr) if sr != 16000 else a for a, sr in segs])
            p2, ev2, _ = two.step_events(slots2, f16)
            worst = max(worst, float(np.abs(p - p2).max()))
            assert (ev == ev2).mean() > 0.999
    print(f"fused against two launches: max |dp| = {worst:.3e}")
    assert worst <= 5e-6, worst
