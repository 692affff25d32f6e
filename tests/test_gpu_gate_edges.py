"""The denoise gate at its threshold, on every kernel's loader.  README, DESIGN and include/vad_engine.h promise: the gate is strict
(x if |x| > thr else 0); an int16 sample is the IEEE quotient float32(s) / float32(32767) (csrc/vadk_device.h: i16_div, a
reciprocal multiply + a Newton correction - a plain multiply mis-rounds 768 magnitudes by one ulp); a G.711 frame gives bit for
bit what its decoded int16 samples / 32768 give.  Every sample of a probe frame is +-m (tests/gate_ladders.py), so one ulp in the
decode, in the threshold or in the comparison turns a whole frame: with thr = |decoded m| the frame must give the bytes of an
all-zero frame, with thr = nextafter(|decoded m|, 0) the bytes of the same call with the gate off - probability bits and the
stream's saved state.  The float64 oracle on the NumPy-decoded samples ties both answers to the truth.

Preconditions, asserted (never skipped): every probe stream's gate-off result differs from the silent one in its probability
bits; in the oracle leg the float64 probabilities of kept and silent frame differ by at least 10 x TOL_P."""
import numpy as np
import pytest

from cutter_vad_amd import weights_io
from cutter_vad_amd.utils.audio import AudioUtils
from tests import gate_ladders as L

pytestmark = pytest.mark.gpu

TOL_P = 2e-5                      # tests/test_gpu_v5.py, tests/test_gpu_v5_8k.py, tests/test_gpu_v4.py
MODELS = [(5, 16000), (5, 8000), (4, 16000), (4, 8000)]
MODEL_IDS = ["v5_16k", "v5_8k", "v4_16k", "v4_8k"]
LADDERS = L.by_name()
MAX_STREAMS = 160


def _blob(version, rate):
    with open(weights_io.packaged_blob_path(version, rate), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def engines():
    from cutter_vad_amd.engine import Engine
    made = {}

    def get(version, rate, twin=False):
        key = (version, rate, twin)
        if key not in made:
            made[key] = Engine(_blob(version, rate), model_version=version, max_streams=MAX_STREAMS, sample_rate=rate)
        return made[key]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def oracles():
    from oracle import oracle
    made = {}

    def get(version, rate):
        if (version, rate) not in made:
            made[(version, rate)] = oracle.OracleModel(_blob(version, rate), "f64")
        return made[(version, rate)]

    return get


class _Streams:
    """n fresh slots of an engine with its tile pinned; closed and unpinned on exit"""

    def __init__(self, eng, n, tile=0):
        self.eng, self.n, self.tile = eng, n, tile

    def __enter__(self):
        self.eng.set_tile(self.tile)
        self.slots = self.eng.open_streams(self.n)
        return self.slots

    def __exit__(self, *exc):
        for s in self.slots:
            self.eng.close_stream(int(s))
        self.eng.set_tile(0)


@pytest.mark.parametrize("name", list(LADDERS))
@pytest.mark.parametrize("tile", [16, 32], ids=["tile16", "tile32"])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_one_frame_calls(engines, model, tile, name):
    """the ONE instantiation of each loader; the 64- and 128-stream ladders span several tiles, the 21- and 33-stream ones end in a
    partial tile on either shape; the float32 ladder adds the special thresholds (+inf, +-0, negative)"""
    eng, lad = engines(*model), LADDERS[name]
    with _Streams(eng, lad.N, tile) as slots:
        L.check_step(eng, slots, lad, (model, tile))


@pytest.mark.parametrize("name", list(LADDERS))
@pytest.mark.parametrize("tile", [16, 32], ids=["tile16", "tile32"])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_multi_frame_calls(engines, model, tile, name):
    """T = 3, [zeros, probe, zeros]: the multi-frame instantiation of each loader"""
    eng, lad = engines(*model), LADDERS[name]
    with _Streams(eng, lad.N, tile) as slots:
        L.check_multi(eng, slots, lad, (model, tile))


@pytest.mark.parametrize("name", ["f32", "i16_32767_00", "ulaw", "alaw"])
@pytest.mark.parametrize("rate", [16000, 8000])
def test_scan(engines, rate, name):
    """whole recordings [zeros, probe, zeros] at hop = frame; at hop = frame / 2 the same bytes as step_multi (16-stream tiles, on
    a second engine) on AudioUtils.split_into_frames of the same samples at that threshold"""
    eng, twin, lad = engines(5, rate), engines(5, rate, twin=True), LADDERS[name]
    with _Streams(eng, lad.N) as slots, _Streams(twin, lad.N, 16) as tslots:
        L.check_scan(eng, slots, lad, rate)
        L.check_scan_half_hop(eng, slots, lad, AudioUtils.split_into_frames, twin, tslots, rate)


@pytest.mark.parametrize("name", ["f32", "i16_32767_00"])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_tick(engines, model, name):
    """even streams pushed with gate_on, odd ones without: tick_run(denoise=q_k) leaves the odd streams their frame"""
    eng, lad = engines(*model), LADDERS[name]
    with _Streams(eng, lad.N) as slots:
        L.check_tick(eng, slots, lad, model)


@pytest.mark.parametrize("tile", [0, 32], ids=["fused", "two_launches"])
def test_step_rates_pass_through_segment(engines, tile):
    """the float32 ladder as the 16 kHz pass-through segment of vad_step_rates, an 8 kHz segment of ordinary noise next to it:
    through the fused launch and, with 32-stream tiles pinned, through the two-launch form"""
    eng, lad = engines(5, 16000), LADDERS["f32"]
    noise = np.random.default_rng(5).normal(0.0, 0.1, (5, 256)).astype(np.float32)
    with _Streams(eng, lad.N + len(noise), tile) as slots:
        L.check_rates(eng, slots, lad, noise, tile)


@pytest.mark.parametrize("name", L.ORACLE_LEG)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_oracle_leg(engines, oracles, model, name):
    """the lowest, a middle and the highest threshold of one ladder per format: the kernel's probabilities against the float64
    oracle on oracle.denoise(xf, thr), xf decoded in NumPy"""
    from oracle import oracle
    eng, om, lad = engines(*model), oracles(*model), LADDERS[name]
    F = eng.frame_samples
    x, xf = lad.frames(F), lad.xf(F)

    def ref(frames):
        return om.step_batch(np.ascontiguousarray(frames, np.float32), np.zeros((lad.N, 256), np.float32), nthreads=8)

    kept64, silent64 = ref(xf), ref(np.zeros_like(xf))
    gap = np.abs(kept64.astype(np.float64) - silent64)[:lad.K]
    assert gap.min() >= 10 * TOL_P, (model, name, int(gap.argmin()), float(gap.min()))
    worst = 0.0
    with _Streams(eng, lad.N) as slots:
        for thr, kept, k in lad.pick3():
            want = ref(oracle.denoise(xf, float(thr)))
            assert np.array_equal(want, np.where(kept, kept64, silent64)), (model, name, k)
            eng.reset(slots)
            got = eng.step(slots, x, denoise=float(thr), **lad.kw)
            err = float(np.abs(got.astype(np.float64) - want).max())
            worst = max(worst, err)
            print(f"gate oracle leg {model} {name} thr={float(thr)!r} kept={int(kept.sum())}/{lad.N} max|p - f64 oracle| = {err:.3e}")
            assert err <= TOL_P, (model, name, k, err)
    print(f"gate oracle leg {model} {name} worst = {worst:.3e}")
