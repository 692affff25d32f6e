"""tests/resample_exact.py without a GPU: the two references against float64 scipy and each other on every parity of up-sampling,
down-sampling and equal lengths (which also measures scipy's own float64 error, from which SLACK is set), the tolerance on the
HOST half of the direct kernel (vad_debug_resample_generic_entries) with two mutations that it must catch, and the restated
launch splits on the shapes tests/test_gpu_resample_exact.py names."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import resample_exact as X

PARITY, tone_spec = X.PARITY, X.tone_spec


def nyquist_rule_is_live(n_in, n_out, spec):
    """the rule changes y only when the array grows: at 2 k == n_out < n_in the plain rule, cos(pi m + phi), is already (-1)^m cos(phi)"""
    return n_out > n_in and any(2 * k == n_in for k, _, _ in spec)


@pytest.fixture(scope="module")
def cases():
    """per shape: the tone input, the impulse input (both float64 here) and their references at every output, computed once"""
    out = {}
    for n_in, n_out in PARITY:
        spec = tone_spec(n_in, n_out)
        xt, yt = X.tones(n_in, n_out, spec)
        pos = X.impulse_positions(n_in, n_in * 7919 + n_out)
        xi, yi, ai = X.impulses(n_in, n_out, pos, np.arange(n_out))
        for a in (xt, yt, xi, yi):
            a.setflags(write=False)
        out[n_in, n_out] = dict(spec=spec, xt=xt, yt=yt, at=X.tone_amp(spec), pos=pos, xi=xi, yi=yi, ai=ai)
    return out


def test_references_agree_with_float64_scipy_and_slack_follows(cases):
    import scipy.signal
    worst = {"tones": (0.0, None), "entries": (0.0, None)}
    for (n_in, n_out), c in cases.items():
        for kind, x, y, amp in (("tones", c["xt"], c["yt"], c["at"]), ("entries", c["xi"].astype(np.float64), c["yi"], c["ai"])):
            dev = float(np.abs(scipy.signal.resample(x, n_out) - y).max()) / amp
            assert dev <= 1e-13, (kind, n_in, n_out, dev)             # the two rules are one function: far below any tolerance in use
            if dev > worst[kind][0]:
                worst[kind] = (dev, (n_in, n_out))
    dev = max(worst["tones"][0], worst["entries"][0])
    rule = 2.0 ** math.ceil(math.log2(X.MARGIN * dev))
    print(f"float64 scipy.signal.resample vs tones: {worst['tones'][0]:.2e} at {worst['tones'][1]}, vs entries: {worst['entries'][0]:.2e} "
          f"at {worst['entries'][1]} (relative to amp); 1024 x that, rounded up to a power of two = 2^{int(math.log2(rule))}; "
          f"SLACK = 2^{int(math.log2(X.SLACK))} = {X.SLACK:.2e}")
    assert dev > 0.0
    assert X.SLACK == 2.0 ** round(math.log2(X.SLACK))
    assert X.MARGIN * dev <= X.SLACK <= 4 * X.MARGIN * dev            # 1024 x scipy's float64 deviation, to the next power of two
    assert X.SLACK <= X.SLACK_LIMIT == 2.0 ** -34                     # 2^10 under the float32 half-ulp of a full-scale sample


def test_tones_and_entries_are_the_same_operator(cases):
    """the dense rule and the closed form never meet in the tests above: here the entries, as a matrix, are applied to the tones"""
    for (n_in, n_out), c in cases.items():
        if n_in * n_out > 1 << 19:
            continue
        R = X.entries(n_in, n_out, np.arange(n_out)[:, None], np.arange(n_in)[None, :])
        y = (R @ c["xt"].astype(np.longdouble)).astype(np.float64)
        assert np.abs(y - c["yt"]).max() <= 2.0 ** -40 * c["at"], (n_in, n_out)


def host_rows(n_in, n_out, m0, m1):
    from cutter_vad_amd import _ffi
    R = np.empty((m1 - m0, n_in), np.float64)
    assert _ffi.lib().vad_debug_resample_generic_entries(n_in, n_out, m0, m1, R.ctypes.data_as(C.POINTER(C.c_double)), R.size) == 0
    return R


def test_tolerance_on_the_host_half_and_its_teeth(cases):
    """the direct kernel's host half (float64 tables, the entry arithmetic) times x, cast to float32, is inside `tolerance` of both
    references; ONE entry off by 1e-6 of itself, or a reference without scipy's Nyquist rule, is outside.  The GPU tests make the
    same comparison, so this is what they can see."""
    inside = lambda got, y, amp: bool((np.abs(got.astype(np.float64) - y) <= X.tolerance(y, amp)).all())
    mutated = live = 0
    for (n_in, n_out), c in cases.items():
        # every output where the operator is small; three 64-output ranges (both ends and the middle) of the 3e8-entry one
        ranges = [(0, n_out)] if n_in * n_out <= 1 << 22 else [(0, 64), (n_out // 2 - 32, n_out // 2 + 32), (n_out - 64, n_out)]
        for m0, m1 in ranges:
            R = host_rows(n_in, n_out, m0, m1)
            for x, y, amp in ((c["xt"], c["yt"][m0:m1], c["at"]), (c["xi"].astype(np.float64), c["yi"][m0:m1], c["ai"])):
                assert inside((R @ x).astype(np.float32), y, amp), (n_in, n_out, m0)
                # the entry whose product with x[n] is the largest part of its output
                m, n = np.unravel_index(np.argmax(np.abs(R * x[None, :]) / X.tolerance(y, amp)[:, None]), R.shape)
                Rm = R.copy()
                Rm[m, n] *= 1.0 + 1e-6
                assert not inside((Rm @ x).astype(np.float32), y, amp), (n_in, n_out, m0, m, n)
                mutated += 1
            if nyquist_rule_is_live(n_in, n_out, c["spec"]):
                _, wrong = X.tones(n_in, n_out, c["spec"], nyquist=False)
                assert not inside((R @ c["xt"]).astype(np.float32), wrong[m0:m1], c["at"]), (n_in, n_out)
                live += 1
    print(f"{mutated} single-entry mutations and {live} references without the Nyquist rule: all outside the tolerance")
    assert mutated >= 2 * len(PARITY) and live == 4                  # (6, 8), (6, 9), (500, 1000), (512, 1411)


def test_split_helpers_on_the_named_shapes():
    L = X.direct_launches
    # past the FFT path's limit, by the size rule
    big = (1 << 25) + 1
    assert not X.by_size_fft(1, big, 1000) and not X.by_size_fft(1, 1000, big)
    assert [(l.m_end - l.m_begin, l.nslice) for l in L(1, big, 1000)] == [(448, 586), (448, 586), (104, 2048)]
    assert [l.m_begin for l in L(1, 1000, big)] == [0, 17179840] and L(1, 1000, big)[1].m_end == big
    # direct splits, pinned
    assert [(l.m_begin, l.m_end, l.nslice) for l in L(1, 131073, 131137)] == [(0, 131008, 3), (131008, 131137, 1366)]
    assert [(l.row0, l.rows, l.m_begin, l.m_end) for l in L(5, 65537, 65536)] == [(0, 3, 0, 65536), (3, 2, 0, 65536)]
    # row groups
    assert not X.by_size_fft(65537, 8, 5)
    assert [(l.row0, l.rows) for l in L(65537, 8, 5)] == [(0, 65535), (65535, 2)]
    assert X.by_size_fft(65537, 300, 512) and X.fft_groups(65537, 300, 512) == (10, 10, [(0, 65535), (65535, 2)])
    assert X.by_size_fft(16385, 1411, 512) and X.fft_groups(16385, 1411, 512) == (12, 10, [(0, 16384), (16384, 1)])
    # FFT stage mixes and the length limit: one group each
    for n_in, n_out, p1, p2 in ((40000, 20001, 17, 16), (70000, 140001, 18, 19), (600000, 1200001, 21, 22),
                                (1 << 25, 11184811, 26, 25), ((1 << 24) + 3, 1 << 25, 26, 26)):
        assert X.by_size_fft(1, n_in, n_out) and X.fft_groups(1, n_in, n_out) == (p1, p2, [(0, 1)])
    # every parity shape is one launch on either path
    for n_in, n_out in PARITY:
        assert len(L(1, n_in, n_out)) == 1 and len(X.fft_groups(1, n_in, n_out)[2]) == 1
