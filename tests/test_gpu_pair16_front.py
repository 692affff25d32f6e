"""The launch front of the paired 16-stream Silero V5 kernel (csrc/silero_v5_t16_body.h, XFIRST): the frame is requested and folded
first, h_{t-1} reaches its planes behind barrier (4), and the recurrent gate half runs behind enc3 - against the unpaired kernel,
which keeps the recurrent half in front: the SAME BITS, since every accumulator sees the same MFMAs in the same order.

Every case makes FOUR consecutive one-frame calls from zero state: on the first call h and c are zero, so a recurrent half that
read stale or foreign planes (the partner half's, enc0's output left in the same rows, another stream's column) would go
unnoticed; from the second call on they are not.  Every stream has its own amplitude and its own samples."""

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io

pytestmark = pytest.mark.gpu
PAIR, NO_PAIR = -3, -4
TOL_P = 2e-5      # the bar tests/test_gpu_pair16_tail.py holds the paired kernel to against the f64 oracle
CALLS = 4
# events within the four calls: the f64 oracle puts a quarter of the probe streams above 0.16 on every call and half of them below 0.1
THRESHOLDS = (0.15, 0.1, 0.8, 0.95, 2, 3)


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
def probes():
    """[48 streams][CALLS frames][512]: noise under a per-stream tone, amplitudes from below the gate's 0.01 to 0.9, so that the
    gate matters, the probabilities spread and the state machines fire; computed once, unchanged"""
    rng = np.random.default_rng(1714)
    n = 48
    amp = np.geomspace(0.004, 0.9, n).astype(np.float32)[rng.permutation(n)]
    f0 = rng.uniform(90.0, 900.0, n)
    tt = np.arange(CALLS * 512, dtype=np.float64)
    tone = np.sin(2 * np.pi * f0[:, None] * tt[None, :] / 16000.0)
    x = (amp[:, None] * (0.6 * tone + 0.4 * rng.standard_normal((n, CALLS * 512)))).astype(np.float32)
    x = np.clip(x, -1.0, 1.0).reshape(n, CALLS, 512)
    x.setflags(write=False)
    return x


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _saved(eng, slots):
    """(h, c) and the state machine (SmSlot) of every listed stream, byte for byte"""
    return np.stack([np.frombuffer(eng.save_stream(int(s)), np.uint8) for s in slots])


def _run(eng, mode, slots, frames, denoise):
    """CALLS one-frame calls from zero state under one pairing mode -> everything every call leaves behind"""
    eng.reset(slots)
    eng.set_thresholds_many(slots, THRESHOLDS)
    eng.set_tile(mode)
    out = []
    for t in range(frames.shape[1]):
        p, ev, seg = eng.step_events(slots, np.ascontiguousarray(frames[:, t]), denoise=denoise)
        out += [_bits(p), ev, seg, np.stack([_bits(eng.get_state(int(s))) for s in slots]), _saved(eng, slots)]
    return out


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


def _same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (i, np.argwhere(u != v)[:4])


# 17: one live stream in the partner half; 32: one full pair; 33 / 48: two workgroups, the last one's second half-tile dead
@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("denoise", [0.0, 0.01])
@pytest.mark.parametrize("n,scattered", [(17, False), (32, False), (33, False), (48, False), (17, True), (33, True)])
def test_four_calls_from_zero_state_leave_the_bits_of_the_unpaired_kernel(eng, probes, n, scattered, denoise, kind):
    x = _as(probes[:n], kind)
    slots, pool = _open(eng, n, scattered)
    try:
        others = None if pool is None else np.setdiff1d(pool, slots)
        if others is not None:
            eng.reset(pool)
            eng.set_tile(NO_PAIR)
            eng.step(others, np.ascontiguousarray(_as(probes[np.arange(others.size) % 48, 0], kind)), denoise=denoise)
            before = _saved(eng, others)                                # bystanders with a state worth keeping
        a = _run(eng, NO_PAIR, slots, x, denoise)
        b = _run(eng, PAIR, slots, x, denoise)
        _same(a, b)
        h_c = a[5 + 3]                                                  # behind the second call
        assert np.all(np.any(h_c[:, :128] != 0, axis=1)) and np.all(np.any(h_c[:, 128:] != 0, axis=1))   # calls 2.. start from h, c != 0
        assert len({int(p) for p in a[-5]}) > n // 2                    # the streams do differ
        if others is not None:
            assert np.array_equal(_saved(eng, others), before)          # the slots in between: byte for byte what they were
    finally:
        _close(eng, slots, pool)


def test_events_fire_within_the_four_calls(eng, probes):
    """what the comparison above compares is not all zeros: some stream starts a segment, and seg_frames is written"""
    slots, pool = _open(eng, 48, False)
    try:
        a = _run(eng, PAIR, slots, probes, 0.01)
        ev = np.stack(a[1::5])
        assert np.any(ev != 0)
    finally:
        _close(eng, slots, pool)


def test_a_nan_frame_in_each_half_tile_is_held_and_its_neighbours_keep_their_bits(eng, probes):
    """48 streams = workgroup 0 with both half-tiles whole, workgroup 1 with its second half-tile dead.  On the third call one stream
    of each half-tile gets a NaN sample: rejected and held (NaN, VAD_EV_REJECTED alone, h, c and the state machine as they were) -
    its 15 neighbours and the partner tile, whose gate rows the same waves compute from the same weight units, bit for bit the
    unpaired run's"""
    n, bad_call, bad = 48, 2, (5, 21, 40)
    x = probes[:n].copy()
    for k, s in enumerate(bad):
        x[s, bad_call, 37 + 150 * k] = np.nan                           # a different STFT column each
    slots, pool = _open(eng, n, False)
    try:
        a = _run(eng, NO_PAIR, slots, x, 0.01)
        b = _run(eng, PAIR, slots, x, 0.01)
        _same(a, b)
        p, ev, seg, _, saved = b[5 * bad_call: 5 * bad_call + 5]
        held = b[5 * bad_call - 1]
        for s in bad:
            assert np.isnan(p.view(np.float32)[s]) and ev[s] == _ffi.VAD_EV_REJECTED and seg[s] == 0
            assert np.array_equal(saved[s], held[s])                    # state untouched by the rejected frame
        ok = np.setdiff1d(np.arange(n), bad)
        assert not np.any(np.isnan(p.view(np.float32)[ok])) and not np.any(ev[ok] & _ffi.VAD_EV_REJECTED)
        assert all(not np.array_equal(saved[s], held[s]) for s in ok)
        assert not np.any(np.isnan(b[5 * (bad_call + 1)].view(np.float32)))       # the next call: everybody steps again
    finally:
        _close(eng, slots, pool)


def test_four_calls_against_the_f64_oracle(eng, blob, probes):
    from oracle import oracle
    om = oracle.OracleModel(blob, "f64")
    n = 48
    slots, pool = _open(eng, n, False)
    try:
        eng.reset(slots)
        eng.set_tile(PAIR)
        st = np.zeros((n, 256), np.float32)
        for t in range(CALLS):
            got = eng.step(slots, np.ascontiguousarray(probes[:n, t]))
            ref = om.step_batch(oracle.denoise(probes[:n, t]).reshape(n, 512), st, nthreads=8)
            worst = float(np.abs(got - ref).max())
            print(f"call {t}: max |dp| vs the f64 oracle = {worst:.3e}")
            assert worst <= TOL_P, t
    finally:
        _close(eng, slots, pool)
