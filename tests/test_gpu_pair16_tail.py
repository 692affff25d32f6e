"""encoder.1 and encoder.3 of the paired 16-stream Silero V5 kernel (csrc/silero_v5_t16_body.h, PAIR: enc1 by output column, enc3 by
row tile, each weight unit feeding both half-tiles) against the unpaired kernel: the SAME BITS, since every accumulator sees the
same MFMAs in the same order.  The frames are column probes - energy in ONE of the three STFT columns only (samples 0..127,
192..319 or 384..511), every stream with its own amplitude and sign pattern and, frame by frame, its own column - so reading a wrong
input column, a wrong tap, a wrong row tile or the other half-tile's planes changes bits."""

import numpy as np
import pytest

from cutter_vad_amd import weights_io

pytestmark = pytest.mark.gpu
PAIR, NO_PAIR = -3, -4
TOL_P = 2e-5      # the bar tests/test_gpu_v5_t16.py holds the unpaired kernel to against the f64 oracle
WARM, AFTER = 3, 2
THRESHOLDS = (0.5, 0.35, 0.8, 0.95, 2, 3)     # events within a handful of frames
COLUMNS = ((0, 128), (192, 320), (384, 512))


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
    """[48 streams][WARM + AFTER frames][512]: stream i's frame t is non-zero in column (i + t) % 3 only; computed once, unchanged"""
    rng = np.random.default_rng(1613)
    n, T = 48, WARM + AFTER
    x = np.zeros((n, T, 512), np.float32)
    amp = rng.uniform(0.05, 0.9, n).astype(np.float32)
    for i in range(n):
        for t in range(T):
            a, b = COLUMNS[(i + t) % 3]
            sign = rng.integers(0, 2, b - a).astype(np.float32) * 2 - 1
            x[i, t, a:b] = amp[i] * sign * rng.uniform(0.5, 1.0, b - a).astype(np.float32)
    x.setflags(write=False)
    return x


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _saved(eng, slots):
    return np.stack([np.frombuffer(eng.save_stream(int(s)), np.uint8) for s in slots])


def _run(eng, mode, slots, frames, denoise, blobs):
    """the frames from the saved state under one pairing mode -> everything a call leaves behind"""
    for s, b in zip(slots, blobs):
        eng.restore_stream(int(s), b)
    eng.set_tile(mode)
    out = []
    for t in range(frames.shape[1]):
        p, ev, seg = eng.step_events(slots, np.ascontiguousarray(frames[:, t]), denoise=denoise)
        out += [_bits(p), ev, seg, np.stack([_bits(eng.get_state(int(s))) for s in slots])]      # h and c behind every frame
    out.append(_saved(eng, slots))
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


# 17: one live stream in the second half; 32: one full pair; 33 / 48: two workgroups, the last one half dead / its second half whole
@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("denoise", [0.01, None])
@pytest.mark.parametrize("n,scattered", [(17, False), (32, False), (33, False), (48, False), (33, True)])
def test_column_probes_leave_the_bits_of_the_unpaired_kernel(eng, probes, n, scattered, denoise, kind):
    x = _as(probes[:n], kind)
    slots, pool = _open(eng, n, scattered)
    try:
        blobs = _prepare(eng, slots, x, denoise)
        a = _run(eng, NO_PAIR, slots, x[:, WARM:], denoise, blobs)      # two consecutive frames from the non-zero saved state
        b = _run(eng, PAIR, slots, x[:, WARM:], denoise, blobs)
        assert len(a) == len(b)
        for i, (u, v) in enumerate(zip(a, b)):
            assert np.array_equal(u, v), (i, np.argwhere(u != v)[:4])
        assert len({int(p) for p in a[0]}) > n // 2                     # the streams do differ
    finally:
        _close(eng, slots, pool)


def test_bystanders_keep_their_state_and_slot_0_its_own_result(eng, probes):
    """17 of 40 open streams stepped paired: one live stream in the second half-tile, whose 15 dead streams - and the 16 of the
    partner-less tail - compute on slot 0's state; nothing of that may be stored"""
    n_open, n = 40, 17
    x = probes[:n_open]
    slots, pool = _open(eng, n_open, False)
    try:
        assert int(slots[0]) == 0
        blobs = _prepare(eng, slots, x, 0.01)
        before = _saved(eng, slots)
        ref = _run(eng, NO_PAIR, slots[:n], x[:n, WARM:], 0.01, blobs[:n])
        assert np.array_equal(_saved(eng, slots[n:]), before[n:])
        got = _run(eng, PAIR, slots[:n], x[:n, WARM:], 0.01, blobs[:n])
        after = _saved(eng, slots)
        assert np.array_equal(after[n:], before[n:])                    # the other 23 slots: byte for byte what they were
        for i, (u, v) in enumerate(zip(ref, got)):
            assert np.array_equal(u, v), (i, np.argwhere(u != v)[:4])
        assert np.array_equal(after[0], ref[-1][0]) and not np.array_equal(after[0], before[0])      # slot 0: stepped once, as unpaired
    finally:
        _close(eng, slots, pool)


def test_column_probes_against_the_f64_oracle(eng, blob, probes):
    from oracle import oracle
    om = oracle.OracleModel(blob, "f64")
    n, T = 48, 4
    slots, pool = _open(eng, n, False)
    try:
        eng.reset(slots)
        eng.set_tile(PAIR)
        st = np.zeros((n, 256), np.float32)
        for t in range(T):
            got = eng.step(slots, np.ascontiguousarray(probes[:n, t]))
            ref = om.step_batch(oracle.denoise(probes[:n, t]).reshape(n, 512), st, nthreads=8)
            worst = float(np.abs(got - ref).max())
            print(f"frame {t}: max |dp| vs the f64 oracle = {worst:.3e}")
            assert worst <= TOL_P, t
    finally:
        _close(eng, slots, pool)
