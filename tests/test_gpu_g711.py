"""ITU-T G.711 frames on the GPU.  One statement, checked everywhere: a G.711 frame gives BIT FOR BIT what the same entry point
gives for the decoded int16 samples under VAD_FMT_I16_32768 - probabilities, event bits, segment lengths, recurrent state, state
machine (every code decodes to an int16, and s / 32768 is exact in float32).  Each case carries, per law, frames that hold all
256 codes.  The 16-stream Silero V5 kernel decodes in its loader; every other kernel sits behind the expansion kernel."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.utils import g711_decode
from tests import g711_ref as G

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_P = 2e-5                      # tests/test_gpu_v5.py
THR = (0.3, 0.2, 0.8, 0.95, 2, 2)  # thresholds low enough for START / END events inside a few frames


def _engine(version, rate, max_streams):
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(version, rate), "rb") as f:
        return Engine(f.read(), model_version=version, max_streams=max_streams, sample_rate=rate)


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(version, rate, max_streams=1024):
        key = (version, rate)
        if key not in made or made[key].max_streams < max_streams:
            if key in made:
                made.pop(key).close()
            made[key] = _engine(version, rate, max_streams)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _codes(n, T, fs, law, seed, rate=16000):
    """[n, T, fs] uint8: every third stream real speech - each from one of the clip's loudest stretches, so that START / END events
    fire within a few frames at either rate - the others Gaussian bursts; the LAST frame of every stream (and frame 0 of stream
    1, a Gaussian one) holds all 256 codes."""
    x = G.speechlike(n, T, fs, seed)
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"].astype(np.float64) / 32768.0
    if rate == 8000:
        pcm = pcm[::2]
    L = T * fs
    energy = (pcm[:pcm.size // L * L].reshape(-1, L) ** 2).mean(axis=1)
    loud = np.argsort(-energy, kind="stable")[:max(1, min(8, energy.size // 4))]
    for k in range(0, n, 3):
        o = int(loud[(k // 3) % loud.size]) * L
        x[k] = pcm[o:o + L].reshape(T, fs)
    c = G.encode(x, law)
    for k in range(n):
        c[k, T - 1] = G.all_codes_frame(fs, roll=k)
    if n > 1 and T > 1:
        c[1, 0] = G.all_codes_frame(fs)
    return c


def _blobs(eng, slots):
    return [eng.get_state(int(s)).tobytes() + eng.save_stream(int(s)) for s in slots]


def _both(eng, n, run):
    """run(slots, use_g711) on fresh slots, once per input form -> the two result lists (+ the streams' state blobs)"""
    out = []
    for g711 in (True, False):
        slots = eng.open_streams(n)
        try:
            eng.set_thresholds_many(slots, THR)
            res = list(run(slots, g711))
            out.append(res + [_blobs(eng, slots)])
        finally:
            for s in slots:
                eng.close_stream(int(s))
    return out


def _assert_same(a, b, what=""):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, list):
            assert x == y, (what, i)
        else:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, i)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, i, int((x != y).sum()))


MODELS = [(5, 16000), (5, 8000)]


@pytest.mark.parametrize("gate", [0.01, None], ids=["gate", "nogate"])
@pytest.mark.parametrize("n", [1, 16, 17, 33, 200])
@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("model", MODELS, ids=["v5_16k", "v5_8k"])
def test_single_frame_steps_equal_the_decoded_int16(engines, model, law, n, gate):
    eng = engines(*model)
    T = 8
    c = _codes(n, T, eng.frame_samples, law, seed=n, rate=model[1])
    pcm = g711_decode(c, law)
    assert np.array_equal(pcm, G.table(law)[c])

    def run(slots, g711):
        res = [eng.step_events(slots, c[:, t], denoise=gate, law=law) if g711
               else eng.step_events(slots, pcm[:, t], denoise=gate, i16_scale=32768) for t in range(T)]
        return [np.stack([r[k] for r in res]) for k in range(3)]

    a, b = _both(eng, n, run)
    _assert_same(a, b, (model, law, n, gate))
    assert np.isfinite(a[0]).all() and (a[0] >= 0).all() and (a[0] <= 1).all()
    if n >= 16:
        assert a[1].any(), "no event fired: the comparison of event bits would be empty"
    # vad_step (probabilities only) takes the format too
    s = eng.open_streams(n)
    try:
        assert np.array_equal(eng.step(s, c[:, 0], denoise=gate, law=law), a[0][0])
    finally:
        for k in s:
            eng.close_stream(int(k))


@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("model", MODELS, ids=["v5_16k", "v5_8k"])
@pytest.mark.parametrize("n,tile", [(200, 0), (4200, 0), (200, 32), (200, 16)], ids=["fused_loop", "tiles32_above_4096", "pinned32", "pinned16"])
def test_step_multi_equals_the_decoded_int16_on_every_tile_shape(engines, model, law, n, tile):
    eng = engines(*model, max_streams=8400)
    T = 4
    c = _codes(n, T, eng.frame_samples, law, seed=1000 + n + tile, rate=model[1])
    pcm = g711_decode(c, law)

    def run(slots, g711):
        return eng.step_multi(slots, c, denoise=0.01, law=law) if g711 else eng.step_multi(slots, pcm, denoise=0.01, i16_scale=32768)

    eng.set_tile(tile)
    try:
        a, b = _both(eng, n, run)
    finally:
        eng.set_tile(0)
    _assert_same(a, b, (model, law, n, tile))
    assert a[1].any()


@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("rate", [16000, 8000])
def test_silero_v4_takes_g711_through_the_expansion_kernel(engines, rate, law):
    eng = engines(4, rate)
    n, T = 33, 6
    c = _codes(n, T, eng.frame_samples, law, seed=77, rate=rate)
    pcm = g711_decode(c, law)

    def run(slots, g711):
        single = [eng.step_events(slots, c[:, t], law=law) if g711 else eng.step_events(slots, pcm[:, t], i16_scale=32768)
                  for t in range(T)]
        multi = eng.step_multi(slots, c, law=law) if g711 else eng.step_multi(slots, pcm, i16_scale=32768)
        return [np.stack([r[k] for r in single]) for k in range(3)] + list(multi)

    for tile in (0, 32):
        eng.set_tile(tile)
        try:
            a, b = _both(eng, n, run)
        finally:
            eng.set_tile(0)
        _assert_same(a, b, (rate, law, tile))


@pytest.mark.parametrize("law", G.LAWS)
def test_device_pointers_and_the_pipelined_path(engines, law):
    import torch
    eng = engines(5, 16000)
    n, T = 200, 6
    c = _codes(n, T, 512, law, seed=5)
    pcm = g711_decode(c, law)
    fmt = _ffi.G711_LAWS[law]

    def run_device(slots, g711):
        d_slots = torch.tensor(np.asarray(slots, np.int32), device="cuda")
        src = torch.from_numpy(c if g711 else pcm).cuda()
        f = fmt if g711 else _ffi.VAD_FMT_I16_32768
        d_p = torch.empty((n,), dtype=torch.float32, device="cuda")
        d_e = torch.empty((n,), dtype=torch.uint8, device="cuda")
        d_s = torch.empty((n,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        out = []
        for t in range(2):
            fr = src[:, t].contiguous()
            torch.cuda.synchronize()
            eng.step_device(n, fr.data_ptr(), d_p.data_ptr(), d_slots.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), fmt=f)
            eng.synchronize()
            out += [d_p.cpu().numpy(), d_e.cpu().numpy(), d_s.cpu().numpy()]
        d_pm = torch.empty((n, T - 2), dtype=torch.float32, device="cuda")
        d_em = torch.empty((n, T - 2), dtype=torch.uint8, device="cuda")
        rest = src[:, 2:].contiguous()
        torch.cuda.synchronize()
        eng.step_multi_device(n, T - 2, rest.data_ptr(), d_pm.data_ptr(), d_slots.data_ptr(), d_em.data_ptr(), d_s.data_ptr(), fmt=f)
        eng.synchronize()
        return out + [d_pm.cpu().numpy(), d_em.cpu().numpy(), d_s.cpu().numpy()]

    a, b = _both(eng, n, run_device)
    _assert_same(a, b, ("device", law))

    def run_pipe(slots, g711):
        bufs = [np.ascontiguousarray(c[:, t]) if g711 else np.ascontiguousarray(pcm[:, t]) for t in range(T)]
        out, tickets = [], []
        for t in range(T):
            tickets.append(eng.submit(slots, bufs[t], law=law) if g711 else eng.submit(slots, bufs[t], i16_scale=32768))
            if len(tickets) == 2:
                out += list(eng.collect(tickets.pop(0)))
        out += list(eng.collect(tickets.pop(0)))
        return out

    a2, b2 = _both(eng, n, run_pipe)
    _assert_same(a2, b2, ("pipelined", law))
    # the pipelined path, the device path and the plain calls agree with each other as well
    def run_plain(slots, g711):
        res = [eng.step_events(slots, c[:, t], law=law) for t in range(T)]
        return [x for r in res for x in r]
    p = _both(eng, n, run_plain)[0]
    _assert_same(a2, p, ("pipelined vs plain", law))


@pytest.mark.parametrize("law", G.LAWS)
def test_tick_pushes_of_g711_equal_pushes_of_the_decoded_int16(engines, law):
    eng = engines(5, 16000)
    n, T = 48, 14
    c = _codes(n, T + 1, 480, law, seed=9)
    c[:, 4:13] = G.encode(np.zeros((n, 9, 480)), law)                   # a quiet stretch so that segments end
    c8 = _codes(n, T, 256, law, seed=10, rate=8000)                      # 8 kHz chunks into the 16 kHz engine

    def frame(k, t):
        if k == 5:
            return np.concatenate([c[k, t], c[k, t + 1][:220]])          # over-long: 700 samples
        if k == 6:
            return c[k, t][:100]                                         # short
        if k == 7:
            return np.concatenate([c[k, t], c[k, t + 1][:32]])           # exactly the model's 512
        return c[k, t]

    def run(g711):
        slots = eng.open_streams(n)
        n_slots = int(max(slots)) + 1
        lastp, done, act = np.zeros(n_slots, np.float32), np.zeros(n_slots, np.int64), np.zeros(n_slots, bool)
        cont, contp = np.zeros(n_slots, bool), np.zeros(n_slots, bool)
        out, wavs = [], []
        try:
            eng.tick_enable_segments(True)
            eng.set_thresholds_many(slots, THR)
            for t in range(T):
                for k in range(n):
                    rate = 8000 if k >= 40 else None
                    f = c8[k, t] if rate else frame(k, t)
                    if g711:
                        eng.tick_push(int(slots[k]), f.tobytes() if k % 2 else f, gate_on=(k % 3 != 0), sample_rate=rate, law=law)
                    else:
                        eng.tick_push(int(slots[k]), g711_decode(f, law).tobytes(), gate_on=(k % 3 != 0), i16_scale=32768, sample_rate=rate)
                if t == 3:                                               # batched pushes: a second frame for streams 0..3 waits a tick
                    many = np.stack([c[k, t + 1] for k in range(4)])
                    if g711:
                        eng.tick_push_many(slots[:4], many, gate_on=False, law=law)
                    else:
                        eng.tick_push_many(slots[:4], g711_decode(many, law), gate_on=False, i16_scale=32768)
                if t == 5:
                    two = [c[k, t + 1].tobytes() for k in (8, 9)]
                    if g711:
                        st = eng.tick_push_gather(slots[8:10], two, 480, gate_on=True, law=law)
                    else:
                        st = eng.tick_push_gather(slots[8:10], [g711_decode(b, law).tobytes() for b in two], 480, gate_on=True, i16_scale=32768)
                    assert st.tolist() == [0, 0]
                    blob = np.concatenate([c[k, t + 1] for k in (10, 11)])
                    if g711:
                        st = eng.tick_push_status(slots[10:12], blob.tobytes(), 480, gate_on=True, law=law)
                    else:
                        st = eng.tick_push_status(slots[10:12], g711_decode(blob, law).tobytes(), 480, gate_on=True, i16_scale=32768)
                    assert st.tolist() == [0, 0]
                    chunks = [c8[k, t].tobytes() for k in (12, 13)]
                    eng.tick_cancel(int(slots[12])), eng.tick_cancel(int(slots[13]))
                    if g711:
                        st = eng.tick_push_rate_gather(slots[12:14], chunks, 8000, gate_on=True, law=law)
                    else:
                        st = eng.tick_push_rate_gather(slots[12:14], [g711_decode(b, law).tobytes() for b in chunks], 8000, gate_on=True, i16_scale=32768)
                    assert st.tolist() == [0, 0]
                for _ in range(2 if t in (3, 5) else 1):
                    s, gs, frames, ns, widx, wkind, wsamp = eng.tick_run_work(0.01, lastp, done, act, cont, contp)
                    rel = {int(v): i for i, v in enumerate(slots)}
                    out.append(np.array([rel[int(v)] for v in s], np.int64))
                    out += [np.asarray(gs).copy(), np.asarray(ns).copy(), np.asarray(widx).copy(), np.asarray(wkind).copy(),
                            np.asarray(wsamp).copy(), lastp[slots].copy(), done[slots].copy(), act[slots].copy()]
                    out += [np.asarray(f).copy() for f in frames if f is not None]
                    for j, kind in zip(np.asarray(widx), np.asarray(wkind)):
                        if kind & _ffi.VAD_WORK_END:
                            wavs.append(hashlib.sha256(eng.tick_take_segment_wav16(int(s[j]), 16000)).hexdigest())
            assert len(wavs) >= 4, "segments must end inside the run"
            return out + [wavs] + [_blobs(eng, slots)]
        finally:
            eng.tick_enable_segments(False)
            for s in slots:
                eng.close_stream(int(s))

    a, b = run(True), run(False)
    _assert_same(a, b, ("tick", law))


def test_full_size_call_equals_int16_and_the_oracle(engines):
    from oracle import oracle
    eng = engines(5, 16000, max_streams=8400)
    n, law = 8192, "ulaw"
    c = np.ascontiguousarray(_codes(n, 2, 512, law, seed=42)[:, 0])
    pcm = g711_decode(c, law)

    def run(slots, g711):
        return eng.step_events(slots, c, denoise=0.01, law=law) if g711 else eng.step_events(slots, pcm, denoise=0.01, i16_scale=32768)

    a, b = _both(eng, n, run)
    _assert_same(a, b, "8192 streams")
    with open(weights_io.packaged_blob_path(5, 16000), "rb") as f:
        om = oracle.OracleModel(f.read(), "f64")
    x = pcm.astype(np.float32) / np.float32(32768)
    st = np.zeros((n, 256), np.float32)
    ref = om.step_batch(oracle.denoise(x, 0.01).reshape(n, 512), st, nthreads=16)
    err = float(np.abs(a[0] - ref).max())
    print(f"8192 mu-law streams vs the f64 oracle: max |dp| = {err:.3g}")
    assert err <= TOL_P


def test_speech_through_the_shared_pool_g711_equals_pcm16():
    from cutter_vad_amd import VADConfig
    from cutter_vad_amd.server import SharedStreamPool
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"]
    assert pcm.dtype == np.int16 and pcm.size == 271360
    codes = G.encode(pcm.astype(np.float64) / 32768.0, "ulaw")
    dec = g711_decode(codes, "ulaw")
    logs = []
    for kind in ("g711", "pcm16"):
        pool = SharedStreamPool()
        log = []
        try:
            s = pool.open_session(VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6,
                                            voice_end_frame_count=12, buffer_size=480))
            s.set_callbacks(lambda: log.append(("S", s.frames_done)), lambda wav: log.append(("E", s.frames_done, hashlib.sha256(wav).hexdigest(), len(wav))),
                            None)
            for i in range(pcm.size // 480):
                if kind == "g711":
                    s.submit_g711(codes[i * 480:(i + 1) * 480].tobytes(), "ulaw")
                else:
                    s.submit_pcm16(dec[i * 480:(i + 1) * 480].astype("<i2").tobytes())
                pool.tick()
            pool.drain()
        finally:
            pool.close()
        logs.append(log)
    assert logs[0] == logs[1]
    assert sum(e[0] == "E" for e in logs[0]) >= 3 and sum(e[0] == "S" for e in logs[0]) >= 3


def test_raw_c_abi_refuses_bad_g711_arguments_and_keeps_working(engines):
    eng = engines(5, 16000)
    lib, h = eng._lib, eng.handle
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    s = eng.open_streams(2)
    sl = s.ctypes.data_as(i64p)
    c = _codes(2, 2, 512, "ulaw", seed=3)[:, 0].copy()
    cp = c.ctypes.data_as(C.c_void_p)
    p = np.zeros(2, np.float32)
    pp = p.ctypes.data_as(f32p)
    ev = np.zeros(2, np.uint8)
    tk = C.c_int64()
    try:
        bad = [
            lib.vad_step(h, sl, 2, None, _ffi.VAD_FMT_ULAW8, 0.01, pp),
            lib.vad_step(h, sl, 2, cp, 5, 0.01, pp),
            lib.vad_step(h, sl, 2, cp, -1, 0.01, pp),
            lib.vad_step_events(h, sl, 2, cp, _ffi.VAD_FMT_ALAW8, 0.01, pp, None, None),
            lib.vad_step_multi(h, sl, 2, 0, cp, _ffi.VAD_FMT_ULAW8, 0.01, pp, None),
            lib.vad_step_multi_device(h, None, 2, 1, None, _ffi.VAD_FMT_ULAW8, 0.01, pp, None, None, None),
            lib.vad_step_multi_device(h, None, 2, 1, cp, 5, 0.01, pp, None, None, None),
            lib.vad_step_submit(h, sl, 2, 1, None, _ffi.VAD_FMT_ALAW8, 0.01, C.byref(tk)),
            lib.vad_step_submit(h, sl, 2, 1, cp, 5, 0.01, C.byref(tk)),
            lib.vad_tick_push(h, int(s[0]), None, 512, _ffi.VAD_FMT_ULAW8, 1),
            lib.vad_tick_push(h, int(s[0]), cp, 0, _ffi.VAD_FMT_ULAW8, 1),
            lib.vad_tick_push(h, int(s[0]), cp, 512, 5, 1),
            lib.vad_tick_push_rate(h, int(s[0]), cp, 255, _ffi.VAD_FMT_ULAW8, 1, 8000),      # an 8 kHz chunk is 256 samples
            lib.vad_tick_push_many(h, sl, 2, cp, 0, _ffi.VAD_FMT_ALAW8, 1),
            lib.vad_g711_decode(_ffi.VAD_FMT_I16_32768, c.ctypes.data, 4, ev.ctypes.data),
        ]
        assert all(rc == _ffi.VAD_ERR_INVALID_ARG for rc in bad), bad
        assert lib.vad_last_error(h)
        assert lib.vad_step(h, sl, 0, cp, _ffi.VAD_FMT_ULAW8, 0.01, pp) == 0
        # the Python mirror refuses a frame of the wrong byte count before the call
        from cutter_vad_amd.core.exceptions import AudioProcessingError
        with pytest.raises(AudioProcessingError, match="expected"):
            eng.step(s, c[:, :500], law="ulaw")
        with pytest.raises(AudioProcessingError):
            eng.step_device(2, 0, 0, fmt=5)
        # and the engine serves a correct G.711 step afterwards
        got = eng.step(s, c, denoise=0.01, law="ulaw")
        r = eng.open_streams(2)
        want = eng.step(r, g711_decode(c, "ulaw"), denoise=0.01, i16_scale=32768)
        for k in r:
            eng.close_stream(int(k))
        assert np.array_equal(got, want) and np.isfinite(got).all()
    finally:
        for k in s:
            eng.close_stream(int(k))
