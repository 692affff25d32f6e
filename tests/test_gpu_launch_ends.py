"""The two ends of a launch of the 16-stream Silero V5 kernel (csrc/silero_v5_t16_body.h): what a call leaves in the state arrays is
what the next call - on any tile, of either tile shape - and the host read; a rejected frame leaves them alone; and every raw
quad of a frame reaches the STFT column (and the position inside it) that it belongs to, although a loader thread fetches and
decodes the quads that two columns share only once.  Everything but the oracle comparisons is byte for byte."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.utils import g711_decode
from tests import g711_ref as G
from tests.signals import make_streams

pytestmark = pytest.mark.gpu
TOL_P = 2e-5                       # tests/test_gpu_v5_t16.py
TOL_TILES = 2e-6                   # the two tile shapes against each other (the same file)
THR = (0.3, 0.2, 0.8, 0.95, 2, 2)  # thresholds low enough for events inside three frames
REJ = _ffi.VAD_EV_REJECTED
KINDS = ("f32", "i16", "ulaw")


@pytest.fixture(scope="module")
def engines():
    from cutter_vad_amd.engine import Engine
    made = {}

    def get(rate):
        if rate not in made:
            with open(weights_io.packaged_blob_path(5, rate), "rb") as f:
                made[rate] = Engine(f.read(), model_version=5, max_streams=256, sample_rate=rate)
        return made[rate]

    yield get
    for e in made.values():
        e.set_tile(0)
        e.close()


@pytest.fixture(scope="module")
def blob16():
    with open(weights_io.packaged_blob_path(5), "rb") as f:
        return f.read()


def _wire(x, kind):
    """float frames -> (the frames in wire format `kind`, keyword arguments of the step calls, the float32 samples the model sees)"""
    if kind == "f32":
        x = np.ascontiguousarray(x, np.float32)
        return x, {}, x
    if kind == "i16":
        q = np.clip(np.round(np.asarray(x, np.float64) * 32767.0), -32768, 32767).astype(np.int16)
        return q, {}, (q.astype(np.float32) / np.float32(32767.0)).astype(np.float32)
    c = G.encode(np.asarray(x, np.float64), "ulaw")
    return c, {"law": "ulaw"}, (g711_decode(c, "ulaw").astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def _blobs(eng, slots):
    return [eng.get_state(int(s)).tobytes() + eng.save_stream(int(s)) for s in slots]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _Slots:
    """n fresh streams with the test's thresholds, closed on the way out"""

    def __init__(self, eng, n):
        self.eng, self.n = eng, n

    def __enter__(self):
        self.slots = self.eng.open_streams(self.n)
        self.eng.set_thresholds_many(self.slots, THR)
        return self.slots

    def __exit__(self, *exc):
        for s in self.slots:
            self.eng.close_stream(int(s))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 16, 17, 33])
@pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
def test_state_left_by_a_one_frame_call_is_what_the_next_call_and_the_host_see(engines, rate, n, kind):
    eng = engines(rate)
    fs = eng.frame_samples
    x, kw, _ = _wire(make_streams(n, 3, seed=7000 + n)[:, :, :fs], kind)
    eng.set_tile(16)
    try:
        with _Slots(eng, n) as slots:
            singles, states = [], []
            for t in range(3):
                p, ev, _ = eng.step_events(slots, x[:, t], **kw)
                singles.append((p, ev))
                states.append(_blobs(eng, slots))          # read after EVERY call: the host sees what the call stored
        assert states[0] != states[1] and states[1] != states[2]
        for T in (1, 2, 3):
            with _Slots(eng, n) as slots:
                p, ev = eng.step_multi(slots, x[:, :T], **kw)
                for t in range(T):
                    assert np.array_equal(_bits(p[:, t]), _bits(singles[t][0])), (T, t)
                    assert np.array_equal(ev[:, t], singles[t][1]), (T, t)
                assert _blobs(eng, slots) == states[T - 1], T
        assert np.isfinite(np.stack([s[0] for s in singles])).all()
    finally:
        eng.set_tile(0)


def test_the_next_launch_may_run_a_stream_on_another_tile_xcd_and_tile_shape(engines):
    eng = engines(16000)
    n = 145                                     # ten tiles, the last one partial: reversed, every stream lands on another tile
    x = make_streams(n, 3, seed=7145)
    rev = np.arange(n)[::-1].copy()
    eng.set_tile(16)
    try:
        with _Slots(eng, n) as slots:
            ref = [eng.step_events(slots, x[:, t])[:2] for t in range(2)]
            ref_state2 = _blobs(eng, slots)
            p3_16 = eng.step(slots, x[:, 2])
        with _Slots(eng, n) as slots:
            p1, e1, _ = eng.step_events(slots, x[:, 0])
            p2, e2, _ = eng.step_events(slots[rev], x[rev, 1])
            assert np.array_equal(_bits(p1), _bits(ref[0][0])) and np.array_equal(e1, ref[0][1])
            assert np.array_equal(_bits(p2[rev]), _bits(ref[1][0])) and np.array_equal(e2[rev], ref[1][1])
            assert _blobs(eng, slots) == ref_state2
            # the third frame on 32-stream tiles, which read the state with plain loads
            eng.set_tile(32)
            p3_32 = eng.step(slots, x[:, 2])
        assert np.abs(p3_32 - p3_16).max() <= TOL_TILES
    finally:
        eng.set_tile(0)


# A frame is 128 quads of samples; STFT column c reads the quads 32 c .. 32 c + 63, so two columns share the quads 32..63 and
# 64..95 (samples 128..255 and 256..383), and a loader thread holds each shared region as two quads (k = 2, 3 of the earlier
# column).  One poisoned quad in each of those four, and one in each unshared end of the frame.
_NAN_QUADS = (5, 32 + 3, 48 + 9, 64 + 14, 80 + 0, 127)


def test_a_rejected_frame_leaves_its_stream_untouched_wherever_the_bad_sample_lies(engines):
    """(tests/test_gpu_nonfinite.py rejects at every sample position of the 8 192-stream call; this is the small shape with a
    partial second tile, and it reads the state back through both host paths.)"""
    eng = engines(16000)
    n = 17                                      # tile 0 full, tile 1 a single stream
    rng = np.random.default_rng(717)
    eng.set_tile(16)
    try:
        with _Slots(eng, n) as slots:
            for _ in range(2):
                eng.step(slots, (rng.standard_normal((n, 512)) * 0.3).astype(np.float32))
            saved = [eng.save_stream(int(s)) for s in slots]
            before = _blobs(eng, slots)
            x = (rng.standard_normal((n, 512)) * 0.3).astype(np.float32)
            p0, e0, s0 = eng.step_events(slots, x)
            after0 = _blobs(eng, slots)
            assert np.isfinite(p0).all() and all(a != b for a, b in zip(before, after0))
            for i, quad in enumerate(_NAN_QUADS):
                bad = [(3 * i + 1) % 16, 16]    # one stream of each tile
                y = x.copy()
                for b in bad:
                    y[b, 4 * quad + (i + b) % 4] = np.nan
                for s, blob in zip(slots, saved):
                    eng.restore_stream(int(s), blob)
                p, ev, seg = eng.step_events(slots, y)
                after = _blobs(eng, slots)
                ok = np.setdiff1d(np.arange(n), bad)
                assert np.isnan(p[bad]).all() and (ev[bad] == REJ).all() and (seg[bad] == 0).all(), quad
                assert all(after[b] == before[b] for b in bad), quad
                assert np.array_equal(_bits(p[ok]), _bits(p0[ok])) and np.array_equal(ev[ok], e0[ok]) and np.array_equal(seg[ok], s0[ok]), quad
                assert all(after[k] == after0[k] for k in ok), quad
    finally:
        eng.set_tile(0)


def quad_probes():
    """[16 streams, 2 frames, 512]: each frame silent but for ONE quad of samples above the gate.  Loader thread q of a stream
    fetches the quads q + 16 j, j = 0..7, as the 12 (column, k) positions (c, k) -> j = 2 c + k: over the streams of a frame the
    live quad visits every j for thread q = 5, the frame's first and last quad, and thread 15's; the second frame moves every
    stream eight places on."""
    quads = [5 + 16 * j for j in range(8)] + [0, 127] + [15 + 16 * j for j in (1, 2, 3, 4, 5, 6)]
    assert len(quads) == 16
    vals = np.array([0.25, -0.5, 0.375, -0.125], np.float64)
    x = np.zeros((16, 2, 512), np.float64)
    for s in range(16):
        for t in range(2):
            qd = quads[(s + 8 * t) % 16]
            x[s, t, 4 * qd:4 * qd + 4] = vals * (1.0 + 0.0625 * s)
    return x


@pytest.mark.parametrize("kind", KINDS)
def test_each_quad_reaches_its_column(engines, blob16, kind):
    from oracle import oracle
    eng = engines(16000)
    x, kw, xf = _wire(quad_probes(), kind)
    assert (np.abs(xf[xf != 0]) > 0.01).all() and (np.count_nonzero(xf.reshape(32, 512), axis=1) == 4).all()
    om = oracle.OracleModel(blob16, "f64")
    st = np.zeros((16, 256), np.float32)
    ref = np.stack([om.step_batch(oracle.denoise(xf[:, t]).reshape(16, 512), st, nthreads=4) for t in range(2)], axis=1)
    got = {}
    try:
        for tile in (16, 32):
            eng.set_tile(tile)
            with _Slots(eng, 16) as slots:
                got[tile] = np.stack([eng.step(slots, x[:, t], **kw) for t in range(2)], axis=1)
    finally:
        eng.set_tile(0)
    err = np.abs(got[16] - ref).max()
    print(f"quad probes {kind}: max |p - f64 oracle| = {err:.3g}, max |p16 - p32| = {np.abs(got[16] - got[32]).max():.3g}")
    assert err <= TOL_P
    assert np.abs(got[16] - got[32]).max() <= TOL_TILES
