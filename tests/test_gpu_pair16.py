"""The paired form of the 16-stream Silero V5 kernel (csrc/silero_v5_t16.hip: silero_v5_pair16 - two tiles per workgroup, the bf16-split
LSTM halves and encoder.0 computed as one row tile for both tiles' streams) against the unpaired kernel it replaces in one-frame
calls with more tiles than CUs: the SAME BITS - probabilities, events, finished-segment lengths, every stream's h and c, the
state machine - from identical saved state, with pairing forced (vad_debug_set_tile(-3)) and forbidden (-4).  Every stream's
signal is different (tests.signals.make_streams), so a swap between the halves, or between row tiles in the hand-back, shows."""

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from tests.signals import make_streams

pytestmark = pytest.mark.gpu
PAIR, NO_PAIR = -3, -4
TOL_P = 2e-5      # the bar tests/test_gpu_v5_t16.py holds the unpaired kernel to against the f64 oracle
WARM, AFTER = 3, 2
THRESHOLDS = (0.5, 0.35, 0.8, 0.95, 2, 3)     # events within a handful of frames


@pytest.fixture(scope="module")
def blob():
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def eng(blob):
    from cutter_vad_amd.engine import Engine
    e = Engine(blob, model_version=5, max_streams=128)
    yield e
    e.set_tile(0)
    e.close()


@pytest.fixture(scope="module")
def signal():
    """[48 streams][WARM + 1 + AFTER frames][512], computed once and left unchanged"""
    x = make_streams(48, WARM + 1 + AFTER, seed=1610)
    x.setflags(write=False)
    return x


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(eng, mode, slots, frames, denoise, blobs):
    """the frames from the saved state under one pairing mode -> everything a call leaves behind"""
    for s, b in zip(slots, blobs):
        eng.restore_stream(int(s), b)
    eng.set_tile(mode)
    out = []
    for t in range(frames.shape[1]):
        p, ev, seg = eng.step_events(slots, np.ascontiguousarray(frames[:, t]), denoise=denoise)
        out += [_bits(p), ev, seg]
        if t == 0:
            out.append(np.stack([_bits(eng.get_state(int(s))) for s in slots]))
    out.append(np.stack([np.frombuffer(eng.save_stream(int(s)), np.uint8) for s in slots]))
    return out


def _prepare(eng, slots, warm, denoise):
    """non-zero h, c and state machines: three unpaired one-frame steps on the same slots, then saved"""
    eng.reset(slots)
    eng.set_thresholds_many(slots, THRESHOLDS)
    eng.set_tile(NO_PAIR)
    for t in range(WARM):
        eng.step(slots, np.ascontiguousarray(warm[:, t]), denoise=denoise)
    assert all(np.any(eng.get_state(int(s)) != 0) for s in slots[:2])
    return [eng.save_stream(int(s)) for s in slots]


def _as(x, kind):
    if kind == "f32":
        return x
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def _open(eng, n, scattered):
    if not scattered:
        return eng.open_streams(n), None
    pool = eng.open_streams(2 * n + 5)
    pick = np.random.default_rng(n).permutation(2 * n + 5)[:n]      # permuted and with gaps
    return pool[pick], pool


def _close(eng, slots, pool):
    eng.set_tile(0)
    for s in (pool if pool is not None else slots):
        eng.close_stream(int(s))


# 16: one workgroup, its second half dead; 17: one live stream in the second half; 32: one full pair; 33 / 48: two workgroups, the
# last one half dead / its second half whole
@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("denoise", [0.01, None])
@pytest.mark.parametrize("n,scattered", [(16, False), (17, False), (32, False), (33, False), (48, False), (33, True)])
def test_paired_call_leaves_the_bits_of_the_unpaired_one(eng, signal, n, scattered, denoise, kind):
    x = _as(signal[:n], kind)
    slots, pool = _open(eng, n, scattered)
    try:
        blobs = _prepare(eng, slots, x, denoise)
        a = _run(eng, NO_PAIR, slots, x[:, WARM:], denoise, blobs)
        b = _run(eng, PAIR, slots, x[:, WARM:], denoise, blobs)
        assert len(a) == len(b)
        for i, (u, v) in enumerate(zip(a, b)):
            assert np.array_equal(u, v), (i, np.argwhere(u != v)[:4])
        assert not np.array_equal(a[0][: n // 2], a[0][n - n // 2:])        # the streams do differ
    finally:
        _close(eng, slots, pool)


@pytest.mark.parametrize("bad", [5, 21])      # a NaN stream in half 0 only | in half 1 only
def test_rejected_frame_in_one_half_leaves_the_other_streams_and_its_own_state_alone(eng, signal, bad):
    n = 32
    x = signal[:n]
    slots, pool = _open(eng, n, False)
    try:
        blobs = _prepare(eng, slots, x, 0.01)
        clean = _run(eng, PAIR, slots, x[:, WARM:WARM + 1], 0.01, blobs)
        xb = x[:, WARM:WARM + 1].copy()
        xb[bad, 0, 300] = np.nan
        got = _run(eng, PAIR, slots, xb, 0.01, blobs)
        ref = _run(eng, NO_PAIR, slots, xb, 0.01, blobs)
        for u, v in zip(got, ref):
            assert np.array_equal(u, v)
        others = np.arange(n) != bad
        for u, v in zip(got, clean):
            assert np.array_equal(u[others], v[others])
        p, ev, seg, state, saved = got
        assert np.isnan(p.view(np.float32)[bad]) and ev[bad] == _ffi.VAD_EV_REJECTED and seg[bad] == 0
        assert np.array_equal(saved[bad], np.frombuffer(blobs[bad], np.uint8))      # h, c and the state machine as they were
    finally:
        _close(eng, slots, pool)


def test_paired_kernel_against_the_f64_oracle(eng, blob, signal):
    from oracle import oracle
    om = oracle.OracleModel(blob, "f64")
    n, T = 48, 4
    slots, pool = _open(eng, n, False)
    try:
        eng.reset(slots)
        eng.set_tile(PAIR)
        st = np.zeros((n, 256), np.float32)
        for t in range(T):
            got = eng.step(slots, np.ascontiguousarray(signal[:n, t]))
            ref = om.step_batch(oracle.denoise(signal[:n, t]).reshape(n, 512), st, nthreads=8)
            worst = float(np.abs(got - ref).max())
            print(f"frame {t}: max |dp| vs the f64 oracle = {worst:.3e}")
            assert worst <= TOL_P, t
    finally:
        _close(eng, slots, pool)
