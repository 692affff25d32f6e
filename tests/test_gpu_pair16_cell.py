"""The launch end of the paired 16-stream Silero V5 kernel (csrc/silero_v5_t16_body.h, PAIR, "the cell in place"): wave (hf, w) runs
the LSTM cell of row tile hf for BOTH tiles of its workgroup the moment its own gate MFMAs end - no hand-back of gate quads through
LDS, no barrier (7) - and stores h' and c' of the partner tile's streams itself, by that tile's slot list and that tile's rejection
flags; only the head partial crosses row tiles, wave (0, w)'s fma(hw0, relu(h'), 0) travelling to wave (1, w) across barrier (8).
Against the unpaired kernel, whose waves own both row tiles of one tile: the SAME BITS in probabilities, events, seg_frames and
saved state, since gates, c', h' keep their arithmetic and the head partial keeps its fmas and the order of its sums.

Every case makes FOUR consecutive one-frame calls from zero state (from the second call on h and c are not zero), at the sizes at
which the partner tile is whole, has one live stream, or is absent.

The zero-input case (an all-zero first frame from zero state) compares like every other.  Measured on the GPU (MI355X, float32 and
int16 alike): behind that frame 54 of a stream's 128 h' are negative (1 782 of the 33 streams' 4 224), none is exactly zero - so
relu(h') WAS +0 for 54 units of every stream and the fma(.., +0, 0) cases of the head term were reached (how many of the 54 lie in
row tile 0, whose term is the exchanged one, and whether a -0 from a multiply in their place would have changed a probability bit was not measured)."""

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io

pytestmark = pytest.mark.gpu
PAIR, NO_PAIR = -3, -4
CALLS = 4
# events within the four calls (tests/test_gpu_pair16_front.py: the same probes, the same thresholds)
THRESHOLDS = (0.15, 0.1, 0.8, 0.95, 2, 3)
# n: 17 = the partner tile has one live stream; 32 = two full half-tiles; 33 = a second workgroup whose partner tile is absent;
# 48 = that workgroup with one whole live tile
SIZES = (17, 32, 33, 48)


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
    rng = np.random.default_rng(1815)
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
    """CALLS one-frame calls from zero state under one pairing mode -> what every call leaves behind: probabilities, events,
    seg_frames, h and c, the saved streams"""
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


@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("denoise", [0.0, 0.01])
@pytest.mark.parametrize("scattered", [False, True])
@pytest.mark.parametrize("n", SIZES)
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
    """what the comparison above compares is not all zeros: some stream starts a segment"""
    slots, pool = _open(eng, 48, False)
    try:
        a = _run(eng, PAIR, slots, probes, 0.01)
        assert np.any(np.stack(a[1::5]) != 0)
    finally:
        _close(eng, slots, pool)


@pytest.fixture(scope="module")
def clean48(eng, probes):
    """the paired run of the 48 probe streams with no NaN anywhere; computed once, unchanged"""
    slots, pool = _open(eng, 48, False)
    try:
        out = _run(eng, PAIR, slots, probes, 0.01)
    finally:
        _close(eng, slots, pool)
    for a in out:
        a.setflags(write=False)
    return out


# 48 streams = workgroup 0 with both half-tiles whole (streams 0..15 | 16..31), workgroup 1 with one live tile (32..47) and an absent
# partner: a NaN in each of the three half-tiles in turn
@pytest.mark.parametrize("bad", [5, 21, 40])
def test_a_nan_frame_in_one_half_tile_is_held_and_every_other_stream_keeps_its_bits(eng, probes, clean48, bad):
    """on the third call one stream gets a NaN sample: rejected (NaN, VAD_EV_REJECTED alone), its h, c and state machine as they
    were - stored by neither of the two waves that now hold its cell; the 15 other streams of its tile and the partner tile's, whose
    cells the same waves run under the OTHER half's flags, are bit for bit the clean run's on that call, and everything is the
    unpaired run's"""
    n, bad_call = 48, 2
    x = probes[:n].copy()
    x[bad, bad_call, 37 + 7 * bad] = np.nan
    slots, pool = _open(eng, n, False)
    try:
        a = _run(eng, NO_PAIR, slots, x, 0.01)
        b = _run(eng, PAIR, slots, x, 0.01)
        _same(a, b)
        p, ev, seg, hc, saved = b[5 * bad_call: 5 * bad_call + 5]
        assert np.isnan(p.view(np.float32)[bad]) and ev[bad] == _ffi.VAD_EV_REJECTED and seg[bad] == 0
        assert np.array_equal(saved[bad], b[5 * bad_call - 1][bad])     # state untouched by the rejected frame
        assert np.array_equal(hc[bad], b[5 * bad_call - 2][bad])
        ok = np.setdiff1d(np.arange(n), [bad])
        for u, v in zip(b[5 * bad_call: 5 * bad_call + 5], clean48[5 * bad_call: 5 * bad_call + 5]):
            assert np.array_equal(u[ok], v[ok])                         # the same tile's other streams and the other tiles': unaffected
        assert all(not np.array_equal(saved[s], b[5 * bad_call - 1][s]) for s in ok)
        assert not np.any(np.isnan(b[5 * (bad_call + 1)].view(np.float32)))       # the next call: everybody steps again
    finally:
        _close(eng, slots, pool)


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_a_zero_frame_from_zero_state_leaves_the_bits_of_the_unpaired_kernel(eng, probes, kind):
    """h' of an all-zero frame from zero state depends on the biases alone.  Where h' <= 0, relu(h') is +0 and the head partial's
    inner fma(hw0, +0, 0) must stay +0 under a negative weight - a multiply would hand -0 to the outer fma.  The count of such
    units is printed; the module docstring records what the GPU gave."""
    n = 33
    x = probes[:n].copy()
    x[:, 0] = 0.0
    x = _as(x, kind)
    slots, pool = _open(eng, n, False)
    try:
        a = _run(eng, NO_PAIR, slots, x, 0.01)
        b = _run(eng, PAIR, slots, x, 0.01)
        _same(a, b)
        h = b[3][:, :128].view(np.float32)                              # h' behind the zero frame
        print(f"zero frame from zero state ({kind}): {int((h <= 0).sum())} of {h.size} h' are <= 0 (relu gives +0), "
              f"{int((h == 0).sum())} are exactly 0; per stream {int((h[0] <= 0).sum())} of 128")
        assert np.all(h == h[0])                                        # every stream saw the same frame from the same state
    finally:
        _close(eng, slots, pool)
