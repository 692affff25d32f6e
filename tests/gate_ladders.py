"""The denoise gate at its threshold (csrc/vadk_device.h: gate4, i16_div, g711_quad; csrc/vad_util.hip: vadk_g711_expand): the
frames, the thresholds and the expectation logic of tests/test_gpu_gate_edges.py and tests/test_gate_host.py.  NumPy only - no
GPU, no import of the engine; the check_* functions take the engine they drive.

Every sample of a probe frame is +-m with seeded random signs, so a decode that is one ulp off, or `>=` for `>`, changes a WHOLE
frame: with thr = q = |decoded m| the frame is gated to silence, with thr = nextafter(q, 0) it passes untouched.  A ladder is K
sorted distinct magnitudes, stream i holding +-m_i: a call with thr = q_k gives silence for the streams i <= k and the gate-off
result for i > k; with thr = nextafter(q_k, 0) the boundary is i < k / i >= k.  Both expected answers are the engine's own: the
bytes of an all-zero frame in the same format, and the bytes of the same call with the gate off (denoise=None).

`xf` - the float32 samples the model must see - is plain NumPy: s.astype(f32) / f32(32767), the same with 32768, the G.711 tables
of tests/g711_ref.py / 32768."""
import numpy as np

from tests import g711_ref as G

f32 = np.float32
I16_EXTRA = (1, 2, 327, 328, 16384, 32766, 32767)         # int16 / 32767: next to the magnitudes a reciprocal multiply mis-rounds
I16_32768 = (1, 2, 327, 328, 8192, 32767)                 # int16 / 32768 (exact division): with -32768 and 26 more, a ladder of 33
I16_MISROUNDED = 768                                      # how many of 1 .. 32767 differ between s * (1 / 32767) and s / 32767
SPECIAL_KEPT = (0.0, -0.0)                                # float32 ladder: every non-zero sample passes
SPECIAL_OFF = (-1.0, -1e-30)                              # ... the gate is off: the denoise=None result
SPECIAL_SILENT = (float("inf"),)                          # ... everything is silent
# Streams whose signs were drawn again (the third word of their seed) because the float64 oracle's probability of the kept frame
# came within 10 x 2e-5 of the silent frame's on one of the four packaged models: the oracle leg of tests/test_gpu_gate_edges.py
# asserts that distance for the ladders it uses.
RESEED = {("f32", 0): 1, ("f32", 3): 1, ("f32", 19): 1, ("alaw", 37): 1, ("alaw", 39): 1, ("alaw", 47): 1, ("alaw", 95): 1,
          ("i16_32767_00", 0): 1}
ORACLE_LEG = ("f32", "i16_32767_00", "i16_32768", "ulaw", "alaw")      # one ladder per format


def misrounded_i16():
    """the magnitudes s in 1 .. 32767 for which a multiply by float32(1 / 32767) is not the IEEE quotient"""
    s = np.arange(1, 32768).astype(f32)
    return (np.flatnonzero(s * (f32(1) / f32(32767)) != s / f32(32767)) + 1).tolist()


def kwargs(kind):
    """the engine's keyword arguments for a wire format"""
    return dict(law=kind if kind in G.LAWS else None, i16_scale=32768 if kind == "i16_32768" else 32767)


class Ladder:
    """K probe streams (+ `extra` streams that are silent at every threshold: the two mu-law zero codes).

    name, kind   : id and wire format
    q [K]        : float32 |decoded m_i|, ascending and distinct
    K, N         : probe streams, all streams
    """

    def __init__(self, name, kind, mags, seed):
        self.name, self.kind, self.seed = name, kind, seed
        self.kw = kwargs(kind)
        self.mags = list(mags)                      # float32 values | int16 magnitudes (-32768 = the negative-only one) | G.711 int16
        self.K = len(self.mags)
        self.N = self.K + (1 if kind == "ulaw" else 0)
        if kind == "f32":
            q = np.array(self.mags, f32)
        elif kind in ("i16_32767", "i16_32768"):
            q = np.abs(np.array(self.mags, np.int64)).astype(f32) / f32(32767 if kind == "i16_32767" else 32768)
        else:
            q = np.array(self.mags, np.int64).astype(f32) / f32(32768)
        self.q = q
        assert q.dtype == f32 and (np.diff(q) > 0).all() and q[0] > 0 and np.isfinite(q).all(), name
        self._cache = {}

    # ---------------------------------------------------------------- frames
    def frames(self, F):
        """-> wire frames [N, F]: stream i holds +-m_i"""
        if F not in self._cache:
            neg = np.stack([np.random.default_rng([self.seed, i, RESEED.get((self.name, i), 0)]).integers(0, 2, F).astype(bool)
                            for i in range(self.N)])
            if self.kind == "f32":
                x = np.where(neg[:self.K], -self.q[:, None], self.q[:, None]).astype(f32)
            elif self.kind.startswith("i16"):
                m = np.array(self.mags, np.int64)[:, None]
                only = (m == -32768)                 # exists with the negative sign only: 0 where the sign would be +
                neg[:self.K, 0] |= only[:, 0]        # ... and never at the frame's first sample
                x = np.where(only, np.where(neg, -32768, 0), np.where(neg, -m, m)).astype(np.int16)
            else:
                tab = G.table(self.kind).astype(np.int64)
                pos = np.array([int(np.flatnonzero(tab == m)[0]) for m in self.mags])
                ngc = np.array([int(np.flatnonzero(tab == -m)[0]) for m in self.mags])
                assert ((pos ^ ngc) == 0x80).all()   # the sign is bit 7 of the code
                x = np.where(neg[:self.K], ngc[:, None], pos[:, None])
                if self.kind == "ulaw":
                    zero = np.flatnonzero(tab == 0)
                    assert zero.tolist() == [0x7F, 0xFF]
                    x = np.concatenate([x, np.where(neg[self.K:], 0x7F, 0xFF)])
                x = x.astype(np.uint8)
            self._cache[F] = np.ascontiguousarray(x)
        return self._cache[F]

    def xf(self, F):
        """-> float32 [N, F]: what the model must see of frames(F) with the gate off"""
        x = self.frames(F)
        if self.kind == "f32":
            y = x
        elif self.kind.startswith("i16"):
            y = x.astype(f32) / f32(32767 if self.kind == "i16_32767" else 32768)
        else:
            y = G.table(self.kind)[x].astype(f32) / f32(32768)
        a = np.abs(y[:self.K])
        assert y.dtype == f32 and ((a == self.q[:, None]) | ((a == 0) & (np.array(self.mags)[:, None] == -32768))).all()
        assert (a[:, 0] > 0).all() and (y[self.K:] == 0).all()
        return y

    def silent(self, F, T=None):
        """-> (all-zero frames [N, F] or [N, T, F], the engine's keyword arguments for them).  A-law has no zero code: its silent
        frames are int16 zeros / 32768, which the engine promises to equal bit for bit."""
        shape = (self.N, F) if T is None else (self.N, T, F)
        if self.kind == "alaw":
            return np.zeros(shape, np.int16), kwargs("i16_32768")
        if self.kind == "ulaw":
            return np.full(shape, 0xFF, np.uint8), self.kw
        return np.zeros(shape, self.frames(F).dtype), self.kw

    def probe3(self, F):
        """-> [N, 3, F]: [zeros, probe, zeros] (zero frames are indifferent to the threshold); A-law, without a zero code:
        [probe, probe, probe] - all three gated or all three kept"""
        x = self.frames(F)
        if self.kind == "alaw":
            return np.ascontiguousarray(np.stack([x, x, x], axis=1))
        z = self.silent(F)[0]
        return np.ascontiguousarray(np.stack([z, x, z], axis=1))

    # ---------------------------------------------------------------- thresholds
    def calls(self):
        """-> [(thr float32, kept bool [N], k)]: thr = q_k keeps i > k, thr = nextafter(q_k, 0) keeps i >= k; mu-law (its zero
        stream) adds thr = 0, which keeps every probe stream"""
        out = []
        i = np.arange(self.N)
        probe = i < self.K
        for k in range(self.K):
            below = np.nextafter(self.q[k], f32(0))
            assert below.dtype == f32 and below < self.q[k] and (k == 0 or below >= self.q[k - 1])
            out.append((self.q[k], (i > k) & probe, k))
            out.append((below, (i >= k) & probe, k))
        if self.N > self.K:
            out.append((f32(0), probe.copy(), 0))
        return out

    def pick3(self):
        """the oracle leg's thresholds: the lowest (everything kept), a middle one, the highest (everything silent)"""
        c = self.calls()[:2 * self.K]
        return [c[1], c[2 * (self.K // 2)], c[2 * self.K - 2]]


def _cut(name, kind, mags, seed, size):
    return [Ladder(f"{name}_{j // size:02d}", kind, mags[j:j + size], seed + j // size) for j in range(0, len(mags), size)]


def ladders():
    """-> every ladder, in a fixed order: float32 (21), int16 / 32768 (33), mu-law (127 + the zero stream), A-law (128), and the
    int16 / 32767 magnitudes in ladders of 64"""
    c = f32(0.01)
    near = [c]
    for _ in range(8):
        near.insert(0, np.nextafter(near[0], f32(0)))
    for _ in range(7):
        near.append(np.nextafter(near[-1], f32(1)))
    f = [f32(2.0 ** -15)] + near + [f32(0.25), f32(1.0), np.nextafter(f32(1), f32(2)), f32(1e4)]
    assert len(f) == 21
    out = [Ladder("f32", "f32", f, 7)]
    rng = np.random.default_rng(32768)
    more = sorted(set(I16_32768) | set(int(v) for v in rng.choice(np.arange(3, 32767), 40, replace=False)[:26]))
    out.append(Ladder("i16_32768", "i16_32768", more[:32] + [-32768], 8))
    assert out[-1].K == 33 and set(I16_32768) <= set(out[-1].mags)
    for law, seed in (("ulaw", 9), ("alaw", 10)):
        tab = G.table(law).astype(np.int64)
        out.append(Ladder(law, law, sorted(set(np.abs(tab[tab != 0]).tolist())), seed))
    assert out[-2].K == 127 and out[-1].K == 128
    sweep = misrounded_i16()
    assert len(sweep) == I16_MISROUNDED
    out += _cut("i16_32767", "i16_32767", sorted(set(sweep) | set(I16_EXTRA)) + [-32768], 100, 64)
    return out


def by_name():
    return {l.name: l for l in ladders()}


# -------------------------------------------------------------------- expectation logic (the engine is the caller's)
def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    bad = np.flatnonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(a.shape[0], -1).any(axis=1)) if a.ndim else []
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, "streams", list(bad[:8]), len(bad))


def mix(kept, off, silent):
    """the expected result of a call: the gate-off result for the kept streams, the silent one for the others"""
    k = np.asarray(kept).reshape((-1,) + (1,) * (np.ndim(off) - 1))
    return np.where(k, off, silent)


def _blobs(eng, slots, which=None):
    return {int(i): eng.save_stream(int(slots[i])) for i in (range(len(slots)) if which is None else which)}


def _near(k, n):
    return [i for i in (k - 1, k, k + 1) if 0 <= i < n]


def _preconditions(lad, off, silent, b_off, b_sil, what, model_state):
    """no vacuous pass: every probe stream's gate-off result differs from the silent one (probability bits, and the saved state
    where a model stands behind it: model_state); the mu-law zero stream's does not"""
    off, silent = np.asarray(off, f32).reshape(lad.N, -1), np.asarray(silent, f32).reshape(lad.N, -1)
    for i in range(lad.K):
        assert (off[i].view(np.uint32) != silent[i].view(np.uint32)).any(), (what, "gate-off equals silence", i)
        assert b_off[i] != b_sil[i] or not model_state, (what, "saved state", i)
    for i in range(lad.K, lad.N):
        assert np.array_equal(off[i].view(np.uint32), silent[i].view(np.uint32)) and b_off[i] == b_sil[i], (what, "zero codes", i)


def _ladder_calls(lad, run, what, calls, model_state):
    """run(None for silence | True for the probe, denoise) -> (engine, tuple of result arrays [N, ...], slots): the two reference
    calls, the preconditions, then every (thr, kept, k) of `calls` against mix().  -> (gate-off results, silent results)"""
    eng, sil, slots = run(None, None)
    b_sil = _blobs(eng, slots)
    _, off, _ = run(True, None)
    b_off = _blobs(eng, slots)
    _preconditions(lad, off[0], sil[0], b_off, b_sil, what, model_state)
    for thr, kept, k in calls:
        _, got, _ = run(True, float(thr))
        for j, (g, o, s) in enumerate(zip(got, off, sil)):
            same_bytes(g, mix(kept, o, s), (what, float(thr).hex(), k, "result", j))
        for i in _near(k, lad.N):
            assert eng.save_stream(int(slots[i])) == (b_off[i] if kept[i] else b_sil[i]), (what, float(thr).hex(), k, "saved state", i)
    return off, sil


def calls_with_specials(lad):
    """lad.calls(); the float32 ladder adds its special thresholds"""
    if lad.kind != "f32":
        return lad.calls()
    all_, none = np.ones(lad.N, bool), np.zeros(lad.N, bool)
    return lad.calls() + [(t, all_, 0) for t in SPECIAL_KEPT + SPECIAL_OFF] + [(t, none, lad.K - 1) for t in SPECIAL_SILENT]


def check_step(eng, slots, lad, what="", model_state=True):
    """one-frame calls: reset, step, the probability bits of all streams + the saved state at the boundary"""
    F = eng.frame_samples
    x, (z, zkw) = lad.frames(F), lad.silent(F)

    def run(probe, thr):
        eng.reset(slots)
        if probe is None:
            return eng, (eng.step(slots, z, denoise=None, **zkw),), slots
        return eng, (eng.step(slots, x, denoise=thr, **lad.kw),), slots

    return _ladder_calls(lad, run, (what, lad.name, "step"), calls_with_specials(lad), model_state)


def check_multi(eng, slots, lad, what="", model_state=True):
    """T = 3 in one call: the multi-frame instantiation of each loader"""
    F = eng.frame_samples
    x, (z, zkw) = lad.probe3(F), lad.silent(F, 3)

    def run(probe, thr):
        eng.reset(slots)
        if probe is None:
            return eng, tuple(eng.step_multi(slots, z, denoise=None, **zkw)), slots
        return eng, tuple(eng.step_multi(slots, x, denoise=thr, **lad.kw)), slots

    return _ladder_calls(lad, run, (what, lad.name, "step_multi"), calls_with_specials(lad), model_state)


def check_scan(eng, slots, lad, what="", model_state=True):
    """whole recordings, hop = frame: probabilities, event bits, segment lengths"""
    F = eng.frame_samples
    x, (z, zkw) = lad.probe3(F).reshape(lad.N, -1), lad.silent(F, 3)
    z = z.reshape(lad.N, -1)

    def run(probe, thr):
        eng.reset(slots)
        res = eng.scan(slots, list(z), hop=F, denoise=None, **zkw) if probe is None else eng.scan(slots, list(x), hop=F, denoise=thr, **lad.kw)
        return eng, tuple(np.stack(r) for r in res), slots

    return _ladder_calls(lad, run, (what, lad.name, "scan"), lad.calls(), model_state)


def check_scan_half_hop(eng, slots, lad, split, multi=None, multi_slots=None, what=""):
    """hop = frame / 2: the same bytes as step_multi on split(samples, frame, hop) at that threshold (tests/test_gpu_scan.py);
    `multi` = the engine that runs step_multi (default: the scanning one)"""
    F = eng.frame_samples
    multi, multi_slots = (eng, slots) if multi is None else (multi, multi_slots)
    recs = lad.probe3(F).reshape(lad.N, -1)
    fr = np.ascontiguousarray(np.stack([split(r, F, F // 2) for r in recs]))
    assert fr.shape == (lad.N, 5, F)
    for thr, _, k in [(None, None, -1)] + lad.calls():
        thr = None if thr is None else float(thr)
        eng.reset(slots)
        p, ev, _ = eng.scan(slots, list(recs), hop=F // 2, denoise=thr, **lad.kw)
        b = _blobs(eng, slots, _near(max(k, 0), lad.N))
        multi.reset(multi_slots)
        mp, mev = multi.step_multi(multi_slots, fr, denoise=thr, **lad.kw)
        same_bytes(np.stack(p), mp, (what, lad.name, "half hop", thr, "probs"))
        same_bytes(np.stack(ev), mev, (what, lad.name, "half hop", thr, "events"))
        assert b == _blobs(multi, multi_slots, b.keys()), (what, lad.name, "half hop", thr, "saved state")


def check_tick(eng, slots, lad, what="", model_state=True):
    """the tick assembler: even streams pushed with gate_on, odd ones without - those keep their frame at every threshold"""
    F = eng.frame_samples
    x, z = lad.frames(F), lad.silent(F)[0]
    assert lad.kind in ("f32", "i16_32767")
    odd = np.arange(lad.N) % 2 == 1
    s = np.asarray(slots, np.int64)

    def tick(frames, gated, thr):
        eng.reset(slots)
        if gated.any():
            eng.tick_push_many(s[gated], frames[gated], gate_on=True)
        if (~gated).any():
            eng.tick_push_many(s[~gated], frames[~gated], gate_on=False)
        o_slots, p, ev, seg = [np.array(a) for a in eng.tick_run(denoise=thr)[:4]]
        at = {int(v): j for j, v in enumerate(o_slots)}
        assert sorted(at) == sorted(int(v) for v in s)
        j = np.array([at[int(v)] for v in s])
        return p[j], ev[j], seg[j]

    def run(probe, thr):
        if probe is None:
            return eng, tick(z, np.zeros(lad.N, bool), 0.01), slots
        if thr is None:
            return eng, tick(x, np.zeros(lad.N, bool), 0.01), slots
        return eng, tick(x, ~odd, thr), slots

    return _ladder_calls(lad, run, (what, lad.name, "tick"), [(t, kept | odd, k) for t, kept, k in lad.calls()], model_state)


def check_rates(eng, slots, lad, noise, what="", model_state=True):
    """step_rates: the float32 ladder as a 16 kHz pass-through segment next to an 8 kHz segment of ordinary noise (whose
    resampled samples are not under the test's control: its streams are stepped and not compared)"""
    assert lad.kind == "f32" and eng.frame_samples == 512 and len(slots) == lad.N + len(noise)
    x, z = lad.frames(512), lad.silent(512)[0]
    head = slots[:lad.N]

    def run(probe, thr):
        eng.reset(slots)
        res = eng.step_rates([(z if probe is None else x, 16000), (noise, 8000)], slots, denoise=thr)
        return eng, tuple(r[:lad.N] for r in res), head

    return _ladder_calls(lad, run, (what, lad.name, "step_rates"), calls_with_specials(lad), model_state)
