"""The accepted rates of vad_convert as a family, and the rates that stand for every branch of the kernel that depends on the ratio
(csrc/scan_convert.hip, csrc/vad_layout.h: the period P and its inputs PI, the row-tiles, cv_base, the LDS skew, cv_nper, the operator
pack), shared by tests/test_scan_convert_host.py (the stand-in) and tests/test_gpu_scan_convert_family.py.  Everything here is
computed from tests/convert_ref.py alone - never from the engine's code or its answers - and `hold` asserts, before a test touches
the engine, that its rates have the properties they were chosen for, so that no case is vacuous.  No test, no library."""
import numpy as np

from tests import convert_ref as CR

# the classes of L on a 16 kHz engine: every L = 16000 / gcd with lcm(L, 16) <= 640
CLASSES = (1, 2, 4, 5, 8, 10, 16, 20, 25, 32, 40, 50, 64, 80, 100, 128, 160, 200, 320, 400, 640)

# rate -> why it is here (16 kHz engine)
COVER = (4000,      # L 4, PI 4: skew 0, the smallest PI, x4 upsampling
         4500,      # L 32, PI 9: a quad of inputs spans two periods
         5000,      # L 16, PI 5
         5120,      # L 25, PI 128: a multiple of 64, 25 row-tiles
         5600,      # L 20, PI 28, 5 row-tiles
         6000,      # L 8, PI 6
         6400,      # L 5, PI 32, 5 row-tiles
         7000,      # L 16, PI 7
         4800,      # L 10, PI 24, 5 row-tiles
         12800,     # L 5, PI 64, 5 row-tiles
         13600,     # L 20, PI 68: skew 0, 5 row-tiles
         15625,     # L 128, M 125
         4025,      # L 640, M 161
         15975,     # L 640, M 639
         4040,      # L 400, 25 row-tiles
         25560,     # L 400, M 639
         4250,      # L 64
         159750,    # L 64, M 639
         31950,     # L 320, M 639
         63900,     # L 160, M 639: 44 100 Hz's L
         127800,    # L 80, M 639
         79875,     # L 128, M 639
         102240,    # L 100, M 639: runs of 6 periods
         51120,     # L 200, M 639: runs of 12 periods
         38640,     # L 200, M 483: runs of 15 periods
         88200,     # L 80, PI 441
         176400,    # L 40, PI 882: runs of exactly 16 periods
         161920,    # L 25, M 253: runs of 3 periods
         191680,    # L 50, M 599: the largest PI and K, runs of 3 periods
         186800,    # L 40, M 467: the largest K, 5 row-tiles
         190000,    # L 8, M 95
         184000,    # L 2, M 23
         192000)    # L 1, M 12


def family(R=16000):
    """L -> the accepted rates with that L, ascending: every rate the argument check takes on an engine at rate R"""
    out = {}
    for sr in range(CR.MIN_RATE, CR.MAX_RATE + 1):
        if CR.accepted(sr, R):
            out.setdefault(CR.ratio(sr, R)[0], []).append(sr)
    return dict(sorted(out.items()))


def facts(sr, R=16000):
    """what the kernel's ratio-dependent code sees at one rate, from the reference alone"""
    L, M = CR.ratio(sr, R)
    P, PI = CR.period(L), CR.period_inputs(sr, R)
    most = CR.MAX_REACH * L - 1
    return dict(sr=sr, L=L, M=M, P=P, PI=PI, tiles=P // 16, skew=(4 - PI % 64) % 64, K_max=CR.reach(most, sr, R),
                run=CR.run_periods(2 * L + 1, sr, R), run_most=CR.run_periods(most, sr, R))


def census(rates, R=16000):
    """property -> the rates of `rates` that have it (and "classes" / "tiles": the sets of L and of row-tile counts)"""
    fam = family(R)
    every = [facts(sr, R) for sr in sum(fam.values(), [])]
    top_PI, top_K = max(f["PI"] for f in every), max(f["K_max"] for f in every)
    fs = [facts(sr, R) for sr in rates]
    assert all(CR.accepted(sr, R) for sr in rates)
    pick = lambda cond: [f["sr"] for f in fs if cond(f)]
    return {"classes": {f["L"] for f in fs}, "tiles": {f["tiles"] for f in fs}, "family_classes": set(fam), "family_size": len(every),
            "skew0": pick(lambda f: f["skew"] == 0), "pi_mult64": pick(lambda f: f["PI"] % 64 == 0), "pi_not_mult4": pick(lambda f: f["PI"] % 4 != 0),
            "pi_below16": pick(lambda f: f["PI"] < 16), "pi_below_K": pick(lambda f: f["PI"] < f["K_max"]),
            "run_below16": pick(lambda f: f["run"] < 16), "run_16": pick(lambda f: f["run"] == 16), "run_above16": pick(lambda f: f["run"] > 16),
            "run_le3": pick(lambda f: f["run"] <= 3), "run_most_below16": pick(lambda f: f["run_most"] < 16),
            "top_PI": pick(lambda f: f["PI"] == top_PI), "top_K": pick(lambda f: f["K_max"] == top_K),
            "M_639_640": pick(lambda f: f["M"] in (639, 640)), "below_8000": pick(lambda f: f["sr"] < 8000),
            "upsampling_over2": pick(lambda f: f["L"] > 2 * f["M"]), "top_PI_value": top_PI, "top_K_value": top_K}


SINGLE = ("skew0", "pi_mult64", "pi_not_mult4", "pi_below16", "pi_below_K", "run_below16", "run_16", "run_above16", "run_le3", "top_PI", "top_K",
          "M_639_640", "below_8000", "upsampling_over2")


def hold(c, *names):
    """the named properties are met by at least one rate each; without names: everything the covering set stands for on a 16 kHz
    engine - all 21 classes of the family of 3 440 rates, periods of 5 and of 25 row-tiles, and every property of SINGLE"""
    if names:
        for name in names:
            assert c[name], name
        return
    assert c["family_size"] == 3440 and c["family_classes"] == set(CLASSES) == c["classes"], sorted(c["classes"])
    assert {1, 5, 25, 10, 20, 40} <= c["tiles"], sorted(c["tiles"])
    assert (c["top_PI_value"], c["top_K_value"]) == (4792, 320)
    for name in SINGLE:
        assert c[name], name


_census = {}


def cover_census():
    """census(COVER), held; computed once"""
    if "c" not in _census:
        c = census(COVER)
        hold(c)
        _census["c"] = c
    return _census["c"]


def depth_lengths(ntaps, sr, R=16000):
    """S_in around one period's inputs, around one workgroup's run of periods and two runs plus 5 (zero lengths dropped)"""
    PI = CR.period_inputs(sr, R)
    span = CR.run_periods(ntaps, sr, R) * PI
    assert span >= PI
    return [n for n in (1, 3, PI - 1, PI, PI + 1, span - 1, span, span + 1, 2 * span + 5) if n > 0]


def depth_block(rng, lens):
    """-> (int16 block, items): the first item on the block's first sample, the last on its last, every gap 8 .. 11 LOUD samples"""
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at = (at + n + 3 + 8) & ~3
    total = offs[-1] + lens[-1]
    block = np.where(np.arange(total) % 2 == 0, 16384, -16384).astype(np.int16)
    for o, n in zip(offs, lens):
        block[o:o + n] = rng.integers(-64, 65, n)
    return block, [(0, o, n, 0) for o, n in zip(offs, lens)]
