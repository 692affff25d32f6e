"""Non-finite frames are rejected per stream inside the step kernels (include/vad_engine.h, VAD_EV_REJECTED; ABI 5): probability
NaN, the event bit alone, seg 0, and the stream's (h, c) and state machine exactly as they were (byte-equal vad_stream_save blobs);
every other stream of the call bit-identical to the same call without the rejected streams.  The reference validates every frame
before the model (core/silero_model.py:779, utils/audio.py:227-228), and SileroVADModel.predict raises on the NaN probability before
it updates its state (core/silero_model.py:436-437)."""
import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io

pytestmark = pytest.mark.gpu
REJ = _ffi.VAD_EV_REJECTED


def _blob(version, rate=16000):
    with open(weights_io.packaged_blob_path(version, rate) if rate != 16000 else weights_io.packaged_blob_path(version), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def v5():
    from cutter_vad_amd.engine import Engine
    e = Engine(_blob(5), model_version=5, max_streams=8192)
    yield e
    e.set_tile(0)
    e.close()


def _saves(eng, slots):
    return [eng.save_stream(int(s)) for s in slots]


def _restore(eng, slots, blobs):
    for s, b in zip(slots, blobs):
        eng.restore_stream(int(s), b)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _poisoned_frame(n, F, rng):
    """A frame per stream: 3 blocks of F streams with one NaN / +Inf / -Inf at every position, four whole-NaN frames, then
    finite edge values that must pass (+-0.0, subnormals, +-1.0, magnitudes up to 1e4) and plain noise."""
    x = (rng.standard_normal((n, F)) * 0.1).astype(np.float32)
    bad, k = [], 0
    for val in (np.nan, np.inf, -np.inf):
        for i in range(F):
            x[k, i] = val
            bad.append(k)
            k += 1
    for _ in range(4):
        x[k] = np.nan
        bad.append(k)
        k += 1
    x[k] = 0.0
    x[k, 1::2] = -0.0
    x[k + 1] = np.float32(1e-40) * np.sign(rng.standard_normal(F)).astype(np.float32)
    x[k + 2] = np.where(rng.standard_normal(F) > 0, 1.0, -1.0).astype(np.float32)
    x[k + 3] = np.linspace(-1e4, 1e4, F, dtype=np.float32)
    assert k + 4 <= n
    return x, np.array(bad)


def _check_reject(eng, n, F, gate, seed, warm=3):
    rng = np.random.default_rng(seed)
    slots = eng.open_streams(n)
    try:
        for _ in range(warm):
            eng.step(slots, (rng.standard_normal((n, F)) * 0.3).astype(np.float32), denoise=gate)
        before = _saves(eng, slots)
        x, bad = _poisoned_frame(n, F, rng)
        ok = np.setdiff1d(np.arange(n), bad)
        p, ev, seg = eng.step_events(slots, x, denoise=gate)
        after = _saves(eng, slots)
        assert np.isnan(p[bad]).all() and (ev[bad] == REJ).all() and (seg[bad] == 0).all()
        assert all(after[i] == before[i] for i in bad)
        assert np.isfinite(p[ok]).all() and not (ev[ok] & REJ).any()
        # the same call with the rejected streams left out
        _restore(eng, slots, before)
        pc, evc, segc = eng.step_events(slots[ok], x[ok], denoise=gate)
        assert np.array_equal(_bits(p[ok]), _bits(pc)) and np.array_equal(ev[ok], evc) and np.array_equal(seg[ok], segc)
        assert all(a == b for a, b in zip((after[i] for i in ok), _saves(eng, slots[ok])))
        # one clean frame for all: the formerly rejected streams go on as streams that never saw the bad frame
        y = (rng.standard_normal((n, F)) * 0.3).astype(np.float32)
        _restore(eng, slots, after)
        q, qe, _ = eng.step_events(slots, y, denoise=gate)
        mixed = [before[i] if i in set(bad.tolist()) else after[i] for i in range(n)]
        _restore(eng, slots, mixed)
        qc, qec, _ = eng.step_events(slots, y, denoise=gate)
        assert np.array_equal(_bits(q), _bits(qc)) and np.array_equal(qe, qec)
        assert np.isfinite(q).all()
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("gate", [0.01, None])
def test_headline_rejects_nonfinite_streams_state_untouched(v5, gate):
    v5.set_tile(0)
    _check_reject(v5, 8192, 512, gate, seed=11 if gate else 12)


def test_v5_on_32_stream_tiles(v5):
    v5.set_tile(32)
    try:
        _check_reject(v5, 1600, 512, 0.01, seed=21)
    finally:
        v5.set_tile(0)


def test_v5_8k_sub_model():
    from cutter_vad_amd.engine import Engine
    with Engine(_blob(5, 8000), model_version=5, max_streams=2048, sample_rate=8000) as e:
        for tile in (16, 32):
            e.set_tile(tile)
            _check_reject(e, 832, 256, 0.01, seed=31 + tile)


@pytest.mark.parametrize("rate", [16000, 8000])
def test_v4_both_tile_shapes(rate):
    from cutter_vad_amd.engine import Engine
    with Engine(_blob(4, rate), model_version=4, max_streams=2048, sample_rate=rate) as e:
        for tile in (16, 32):
            e.set_tile(tile)
            _check_reject(e, 1600, 512, 0.01, seed=41 + tile + rate)


@pytest.mark.parametrize("n,tile", [(8192, 32), (1024, 16)])
def test_multi_frame_continues_from_the_last_accepted_frame(v5, n, tile):
    rng = np.random.default_rng(50 + n)
    T = 4
    slots = v5.open_streams(n)
    v5.set_tile(tile)
    try:
        v5.step(slots, (rng.standard_normal((n, 512)) * 0.3).astype(np.float32))
        before = _saves(v5, slots)
        x = (rng.standard_normal((n, T, 512)) * 0.3).astype(np.float32)
        rej = {}                                    # stream -> rejected frame
        for k, t in enumerate((0, 1, 3)):
            for i in range(k * 64, k * 64 + 64):
                rej[i] = t
                x[i, t, (i * 37) % 512] = (np.nan, np.inf, -np.inf)[i % 3]
        x[200, :, 5] = np.nan                       # every frame of one stream
        p, ev = v5.step_multi(slots, x)
        after = _saves(v5, slots)
        assert after[200] == before[200] and (ev[200] == REJ).all() and np.isnan(p[200]).all()
        one = np.array(sorted(rej))
        keep = np.array([[t for t in range(T) if t != rej[i]] for i in one])
        assert all(ev[i, rej[i]] == REJ and np.isnan(p[i, rej[i]]) for i in one)
        _restore(v5, slots, before)
        pc, evc = v5.step_multi(slots[one], x[one[:, None], keep])
        assert np.array_equal(_bits(p[one[:, None], keep]), _bits(pc)) and np.array_equal(ev[one[:, None], keep], evc)
        assert all(after[i] == b for i, b in zip(one, _saves(v5, slots[one])))
        clean = np.setdiff1d(np.arange(n), np.append(one, 200))
        assert np.isfinite(p[clean]).all() and not (ev[clean] & REJ).any()
    finally:
        v5.set_tile(0)
        for s in slots:
            v5.close_stream(int(s))


def test_device_and_pipelined_entry_points(v5):
    import torch
    n = 256
    rng = np.random.default_rng(60)
    slots = v5.open_streams(n)
    try:
        v5.step(slots, (rng.standard_normal((n, 512)) * 0.3).astype(np.float32))
        before = _saves(v5, slots)
        x = (rng.standard_normal((n, 512)) * 0.3).astype(np.float32)
        bad = np.array([3, 17, 100, 255])
        x[3, 0], x[17, 511], x[100, 200], x[255] = np.nan, np.inf, -np.inf, np.nan
        ref_p, ref_ev, ref_seg = v5.step_events(slots, x)
        ref_after = _saves(v5, slots)
        assert np.isnan(ref_p[bad]).all() and (ref_ev[bad] == REJ).all()
        assert all(ref_after[i] == before[i] for i in bad)
        # vad_step_device on torch tensors
        _restore(v5, slots, before)
        dx = torch.from_numpy(x).cuda()
        ds = torch.from_numpy(slots.astype(np.int32)).cuda()          # vad_step_device: int32 slots
        dp = torch.empty(n, dtype=torch.float32, device="cuda")
        de = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dg = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        v5.step_device(n, dx.data_ptr(), dp.data_ptr(), ds.data_ptr(), de.data_ptr(), dg.data_ptr())
        v5.synchronize()
        assert np.array_equal(_bits(dp.cpu().numpy()), _bits(ref_p)) and np.array_equal(de.cpu().numpy(), ref_ev)
        assert _saves(v5, slots) == ref_after
        # vad_step_submit / vad_step_collect
        _restore(v5, slots, before)
        p, ev, seg = v5.collect(v5.submit(slots, x))
        assert np.array_equal(_bits(p), _bits(ref_p)) and np.array_equal(ev, ref_ev) and np.array_equal(seg, ref_seg)
        assert _saves(v5, slots) == ref_after
    finally:
        for s in slots:
            v5.close_stream(int(s))


def test_fused_resample_rejects_a_bad_input_sample_at_every_rate(v5):
    rng = np.random.default_rng(70)
    segs, m = [], 48
    for sr, n_in in ((8000, 256), (24000, 768), (48000, 1536)):
        a = (rng.standard_normal((m, n_in)) * 0.3).astype(np.float32)
        for j, pos in enumerate((0, n_in // 2 + 1, n_in - 1)):
            a[5 + 7 * j, pos] = (np.nan, np.inf, -np.inf)[j]
        segs.append((a, sr))
    slots = v5.open_streams(3 * m)
    try:
        before = _saves(v5, slots)
        p, ev, seg = v5.step_rates(segs, slots)
        after = _saves(v5, slots)
        bad = np.array([k * m + 5 + 7 * j for k in range(3) for j in range(3)])
        ok = np.setdiff1d(np.arange(3 * m), bad)
        assert np.isnan(p[bad]).all() and (ev[bad] == REJ).all() and (seg[bad] == 0).all()
        assert all(after[i] == before[i] for i in bad)
        assert np.isfinite(p[ok]).all() and not (ev[ok] & REJ).any()
        _restore(v5, slots, before)
        keep = [np.setdiff1d(np.arange(m), [5, 12, 19]) for _ in range(3)]
        pc, evc, _ = v5.step_rates([(a[kp], sr) for (a, sr), kp in zip(segs, keep)], slots[ok])
        assert np.array_equal(_bits(p[ok]), _bits(pc)) and np.array_equal(ev[ok], evc)
        assert all(after[i] == b for i, b in zip(ok, _saves(v5, slots[ok])))
    finally:
        for s in slots:
            v5.close_stream(int(s))


@pytest.mark.parametrize("bad_value", [np.nan, np.inf])
def test_predict_raises_like_the_reference_and_keeps_its_state(bad_value):
    from cutter_vad_amd import AudioProcessingError, SileroModelVersion
    from cutter_vad_amd.core.silero_model import SileroVADModel
    rng = np.random.default_rng(80)
    clean = [(rng.standard_normal(512) * 0.3).astype(np.float32) for _ in range(4)]
    m = SileroVADModel(weights_io.packaged_blob_path(5), SileroModelVersion.V5)
    for c in clean[:3]:
        m.predict(c, 16000)
    st0, n0 = m.model_state.state.copy(), m.prediction_count
    bad = clean[3].copy()
    bad[100] = bad_value
    with pytest.raises(AudioProcessingError, match="Probability extraction failed"):
        m.predict(bad, 16000)
    assert m.prediction_count == n0 and np.array_equal(_bits(m.model_state.state), _bits(st0))
    fresh = SileroVADModel(weights_io.packaged_blob_path(5), SileroModelVersion.V5)
    for c in clean[:3]:
        fresh.predict(c, 16000)
    assert m.predict(clean[3], 16000) == fresh.predict(clean[3], 16000)
