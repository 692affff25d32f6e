"""The gate ladders of tests/gate_ladders.py without a GPU: the generator's own properties, and the expectation logic of
tests/test_gpu_gate_edges.py rehearsed on the real csrc/engine.cpp over the HIP stand-in (tests/standin.py), whose kernels decode
and gate with true division and return p = |first sample of the frame|."""
import ctypes as C

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.utils.audio import AudioUtils
from tests import g711_ref as G
from tests import gate_ladders as L
from tests import standin

LADDERS = L.by_name()
ONE_EACH = ["f32", "i16_32768", "ulaw", "alaw", "i16_32767_00", "i16_32767_12"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    handle = C.CDLL(standin.build(tmp_path_factory.mktemp("standin")))
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


@pytest.fixture(scope="module")
def engines(lib):
    """Engine objects over the stand-in library (the product's loader knows one library: it is swapped for the constructor only)"""
    from cutter_vad_amd.engine import Engine
    made = {}

    def get(rate):
        if rate not in made:
            with open(weights_io.packaged_blob_path(5, rate), "rb") as f:
                blob = f.read()
            saved = _ffi._lib
            _ffi._lib = lib
            try:
                made[rate] = Engine(blob, model_version=5, max_streams=160, sample_rate=rate)
            finally:
                _ffi._lib = saved
        return made[rate]

    yield get
    for e in made.values():
        e.close()


def test_the_ladders_are_what_the_issue_lists():
    lads = L.ladders()
    assert [l.name for l in lads[:4]] == ["f32", "i16_32768", "ulaw", "alaw"] and [(l.K, l.N) for l in lads[:4]] == [(21, 21), (33, 33), (127, 128), (128, 128)]
    # int16 / 32767: the 768 magnitudes a multiply by float32(1 / 32767) mis-rounds (by one ulp, never more), the named ones, -32768
    sweep = L.misrounded_i16()
    assert len(sweep) == L.I16_MISROUNDED == 768
    s = np.array(sweep, np.float32)
    assert (np.abs((s * (np.float32(1) / np.float32(32767))).view(np.int32) - (s / np.float32(32767)).view(np.int32)) == 1).all()
    i16 = lads[4:]
    mags = [m for l in i16 for m in l.mags]
    assert all(l.kind == "i16_32767" for l in i16) and all(l.K == 64 for l in i16[:-1]) and 2 <= i16[-1].K <= 64
    assert set(mags) == set(sweep) | set(L.I16_EXTRA) | {-32768} and len(mags) == len(set(mags)) and mags[-1] == -32768
    assert i16[-1].q[-1] > 1.0
    allq = np.concatenate([l.q for l in i16])
    assert (np.diff(allq) > 0).all()
    # float32: 8 below .. 7 above float32(0.01), consecutive; no subnormal anywhere
    f = lads[0]
    near = f.q[1:17]
    assert near[8] == np.float32(0.01) and (np.diff(near.view(np.int32)) == 1).all()
    assert f.q[0] == np.float32(2.0 ** -15) and f.q[17:].tolist() == [0.25, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 1e4]
    for l in lads:
        assert l.q.min() >= np.finfo(np.float32).tiny and np.nextafter(l.q[0], np.float32(0)) >= np.finfo(np.float32).tiny
    # G.711: every distinct non-zero decoded magnitude
    for l in lads[2:4]:
        tab = G.table(l.kind).astype(np.int64)
        assert l.mags == sorted(set(np.abs(tab[tab != 0]).tolist())) and 2 * l.K + (l.kind == "ulaw") == G.DISTINCT[l.kind]


@pytest.mark.parametrize("F", [512, 256])
@pytest.mark.parametrize("name", list(LADDERS))
def test_frames_decode_to_plus_minus_q_and_thresholds_split_them(name, F):
    lad = LADDERS[name]
    x, xf = lad.frames(F), lad.xf(F)
    assert x.shape == (lad.N, F) and xf.shape == (lad.N, F) and xf.dtype == np.float32
    assert x.dtype == {"f32": np.float32, "i16_32767": np.int16, "i16_32768": np.int16, "ulaw": np.uint8, "alaw": np.uint8}[lad.kind]
    if lad.kind in G.LAWS:
        from cutter_vad_amd.utils import g711_decode
        assert np.array_equal(g711_decode(x, lad.kind).astype(np.float32) / np.float32(32768), xf)
    for i in range(lad.K):                                   # both signs throughout the frame (-32768 has the negative one only)
        assert (xf[i] < 0).sum() > F // 4 and ((xf[i] > 0).sum() > F // 4 or lad.mags[i] == -32768)
    calls = lad.calls()
    assert len(calls) == 2 * lad.K + (lad.N - lad.K)
    for thr, kept, k in calls:
        assert thr.dtype == np.float32 and float(np.float32(float(thr))) == float(thr)
        gated = np.where(np.abs(xf) > thr, xf, np.float32(0))          # the rule itself, on the samples the model must see
        full = (gated == xf).all(axis=1) & (np.abs(xf).max(axis=1) > 0)
        none = (gated == 0).all(axis=1)
        assert np.array_equal(full, kept) and np.array_equal(none, ~kept), (name, k)
    assert [int(c[1].sum()) for c in lad.pick3()] == [lad.K, lad.K - 1 - lad.K // 2, 0]


@pytest.mark.parametrize("rate", [16000, 8000])
@pytest.mark.parametrize("name", ONE_EACH)
def test_step_multi_and_scan_on_the_stand_in(engines, name, rate):
    eng, lad = engines(rate), LADDERS[name]
    slots = eng.open_streams(lad.N)
    try:
        off, sil = L.check_step(eng, slots, lad, rate, model_state=False)
        # the stand-in's "model": p = |first sample| of what the gate left
        assert np.array_equal(off[0], np.minimum(np.abs(lad.xf(eng.frame_samples)[:, 0]), np.float32(1))) and not sil[0].any()
        L.check_multi(eng, slots, lad, rate, model_state=False)
        L.check_scan(eng, slots, lad, rate, model_state=False)
        L.check_scan_half_hop(eng, slots, lad, AudioUtils.split_into_frames, what=rate)
    finally:
        for s in slots:
            eng.close_stream(int(s))


@pytest.mark.parametrize("name", ["f32", "i16_32767_00"])
def test_tick_on_the_stand_in(engines, name):
    eng, lad = engines(16000), LADDERS[name]
    slots = eng.open_streams(lad.N)
    try:
        L.check_tick(eng, slots, lad, model_state=False)
    finally:
        for s in slots:
            eng.close_stream(int(s))


def test_the_checks_fail_on_a_wrong_gate(engines):
    """the expectation logic has teeth: an engine whose gate is `>=`, or whose threshold arrives one ulp low, fails check_step"""
    eng, lad = engines(16000), LADDERS["f32"]

    class Wrong:
        frame_samples = eng.frame_samples

        def __init__(self, bend):
            self.bend = bend

        def __getattr__(self, name):
            return getattr(eng, name)

        def step(self, slots, frames, denoise=0.01, **kw):
            return eng.step(slots, frames, denoise=None if denoise is None else self.bend(np.float32(denoise)), **kw)

    slots = eng.open_streams(lad.N)
    try:
        up = lambda t: float(np.nextafter(t, np.float32(np.inf))) if np.isfinite(t) and t > 0 else float(t)
        down = lambda t: float(np.nextafter(t, np.float32(0))) if np.isfinite(t) and t > 0 else float(t)        # = `>=` for `>`
        L.check_step(Wrong(float), slots, lad, model_state=False)
        for bend in (up, down):
            with pytest.raises(AssertionError):
                L.check_step(Wrong(bend), slots, lad, model_state=False)
    finally:
        for s in slots:
            eng.close_stream(int(s))
