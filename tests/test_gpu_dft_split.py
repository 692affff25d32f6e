"""The STFT's odd-bin tile of the 16-stream Silero V5 kernels on the bf16 split (silero_v5_t16_body.h: the loader cuts po | qo into
planes, the even tile's operands stay fp32 behind them, the weight ring runs from the recurrent half through the DFT's four units into
encoder.0): 37 streams - three tiles, the last with five live streams, an odd tile count for pairing - of float32 and int16 frames
at 16 kHz.  Single frames against the f64 oracle; the same frames as one multi-frame call bit for bit, and against the 32-stream
tiles; the paired entry against the unpaired one bit for bit; G.711 frames and one scan call against the steps they decode to, bit
for bit; and the probes of tests/test_dft_split_pack.py, one stream each beside ordinary streams, against the f64 oracle."""
import numpy as np
import pytest

from cutter_vad_amd import weights_io
from cutter_vad_amd.utils import g711_decode
from tests import g711_ref as G
from tests.signals import make_streams
from tests.test_dft_split_pack import probe_frames

pytestmark = pytest.mark.gpu
N, T = 37, 6
PAIR, NO_PAIR = -3, -4


def _blob():
    with open(weights_io.packaged_blob_path(5, 16000), "rb") as f:
        return f.read()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def frames():
    """{kind: [N][T][512]} of make_streams signals, computed once and left unchanged"""
    x = make_streams(N, T, seed=5164)
    xi = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    out = {"f32": x, "i16": xi}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def engine():
    from cutter_vad_amd.engine import Engine
    with Engine(_blob(), model_version=5, max_streams=64) as eng:
        yield eng, eng.open_streams(N)


def _steps(eng, slots, x, **kw):
    """T single-frame steps -> (probs [n][T], events [n][T], seg [n][T], saved streams, states)"""
    eng.reset(slots)
    pe = [eng.step_events(slots, np.ascontiguousarray(x[:, t]), **kw) for t in range(x.shape[1])]
    return (np.stack([a[0] for a in pe], axis=1), np.stack([a[1] for a in pe], axis=1), np.stack([a[2] for a in pe], axis=1),
            [eng.save_stream(int(s)) for s in slots], np.stack([eng.get_state(int(s)) for s in slots]))


@pytest.fixture(scope="module")
def single(frames, engine):
    """{kind: _steps(...)} on 16-stream tiles, shared by the tests below"""
    eng, slots = engine
    eng.set_tile(16)
    out = {kind: _steps(eng, slots, frames[kind]) for kind in ("f32", "i16")}
    eng.set_tile(0)
    return out


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_single_frame_steps_against_the_f64_oracle(frames, single, kind):
    from oracle import oracle
    om = oracle.OracleModel(_blob(), "f64")
    x = frames[kind]
    xf = x if kind == "f32" else (x.astype(np.float32) / np.float32(32767.0))
    p, _, _, _, state = single[kind]
    st = np.zeros((N, 256), np.float32)
    worst = 0.0
    for t in range(T):
        ref = om.step_batch(oracle.denoise(np.ascontiguousarray(xf[:, t])).reshape(N, 512), st, nthreads=4)
        worst = max(worst, float(np.abs(p[:, t] - ref).max()))
    ds = float(np.abs(state - st).max())
    print(f"{kind}: max |dp| = {worst:.3e}, max |dstate| = {ds:.3e}")
    assert worst <= 2e-6, worst
    assert ds <= 2e-5, ds


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_one_multi_frame_call_leaves_the_bits_of_the_single_frames(frames, single, engine, kind):
    eng, slots = engine
    x = frames[kind]
    p1, ev1, _, saved1, _ = single[kind]
    eng.set_tile(16)
    eng.reset(slots)
    p16, ev16 = eng.step_multi(slots, x)
    saved16 = [eng.save_stream(int(s)) for s in slots]
    eng.set_tile(32)
    eng.reset(slots)
    p32, _ = eng.step_multi(slots, x)
    eng.set_tile(0)
    assert np.array_equal(_bits(p16), _bits(p1))
    assert np.array_equal(ev16, ev1)
    assert saved16 == saved1
    d = float(np.abs(p16 - p32).max())
    print(f"{kind}: max |p16 - p32| = {d:.3e}")
    assert d <= 2e-6, d


@pytest.mark.parametrize("n", [37, 16])
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_paired_at_every_size_equals_never_paired(frames, engine, n, kind):
    eng, slots = engine
    x = frames[kind][:n]
    got = {}
    for mode in (NO_PAIR, PAIR):
        eng.set_tile(mode)
        p, ev, seg, saved, state = _steps(eng, slots[:n], x)
        got[mode] = [_bits(p), ev, seg, _bits(state), saved]
    eng.set_tile(0)
    for i, (u, v) in enumerate(zip(got[NO_PAIR], got[PAIR])):
        assert (u == v) if isinstance(u, list) else np.array_equal(u, v), i
    assert not np.array_equal(got[PAIR][0][: n // 2], got[PAIR][0][n - n // 2:])      # the streams do differ


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_g711_frames_equal_the_int16_steps_they_decode_to(frames, engine, law):
    eng, slots = engine
    codes = G.encode(frames["f32"].astype(np.float64), law)
    pcm = g711_decode(codes, law)
    assert pcm.dtype == np.int16 and pcm.shape == codes.shape
    eng.set_tile(16)
    a = _steps(eng, slots, codes, law=law)
    b = _steps(eng, slots, pcm, i16_scale=32768)
    eng.set_tile(0)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3] and np.array_equal(_bits(a[4]), _bits(b[4]))
    assert float(np.nanmax(a[0])) > float(np.nanmin(a[0]))


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_one_scan_over_the_same_samples_equals_the_steps(frames, single, engine, kind):
    eng, slots = engine
    x = frames[kind]
    p1, ev1, _, saved1, state1 = single[kind]
    eng.reset(slots)
    probs, ev, _ = eng.scan(slots, [np.ascontiguousarray(x[i].reshape(-1)) for i in range(N)], hop=512)
    assert np.array_equal(_bits(np.stack(probs)), _bits(p1))
    assert np.array_equal(np.stack(ev), ev1)
    assert [eng.save_stream(int(s)) for s in slots] == saved1
    assert np.array_equal(_bits(np.stack([eng.get_state(int(s)) for s in slots])), _bits(state1))


def test_probes_beside_ordinary_streams_against_the_f64_oracle(frames, engine):
    """three frames of every probe (the same frame again: the state moves), stream k of a 16-stream batch whose other streams carry
    make_streams signals, once with the gate on and once with it off; a probe is judged in the run whose gate it names.  Bar per
    probe: max(2e-6, twice the distance of the oracle's own f32 build from its f64 build on that probe)."""
    from oracle import oracle
    eng, slots = engine
    o64, o32 = oracle.OracleModel(_blob(), "f64"), oracle.OracleModel(_blob(), "f32")
    probes = probe_frames()
    x = np.ascontiguousarray(frames["f32"][:16, :3]).copy()
    for k, (fr, _) in enumerate(probes.values()):
        x[2 * k + 1] = fr                                             # odd places: tiles' lanes between ordinary streams
    failed = []
    for mode in (NO_PAIR, PAIR):
        for thr in (0.01, None):
            eng.set_tile(mode)
            p = _steps(eng, slots[:16], x, denoise=thr)[0]
            for k, (name, (fr, want)) in enumerate(probes.items()):
                if want != thr:
                    continue
                xin = np.ascontiguousarray(np.tile(fr if thr is None else oracle.denoise(fr, thr), (3, 1)))
                p64, _ = o64.run_stream(xin)
                p32, _ = o32.run_stream(xin)
                d32 = float(np.abs(p32 - p64).max())
                d = float(np.abs(p[2 * k + 1] - p64).max())
                print(f"tile {mode} {name}: |gpu - f64| = {d:.3e}, |f32 - f64| = {d32:.3e}")
                if not d <= max(2e-6, 2 * d32):
                    failed.append((mode, name, d, d32))
    eng.set_tile(0)
    assert not failed, failed
