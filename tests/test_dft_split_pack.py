"""The STFT's odd-bin tile of the 16-stream Silero V5 kernels on the bf16 split (vad_layout.h, DFT_X3_BLOCKS): the packing's fifth
block range (vad_debug_pack_weights id 5164; the engine uploads it behind the fourth, in the third stream's buffer).  CPU only: its
pieces sum bit for bit to the odd-tile values of S_STFT in the first stream; the other streams and the section table keep every
byte (tests/golden/v5_t16_streams_before_dft_split.json, hashed before the range existed); a NumPy model of the kernel's order -
the rank-1 terms as the accumulator's start, the units in order, the six products of mfma_x3, one fp32 rounding per MFMA - is no
further from a float64 DFT than twice a model of the fp32 MFMA form it replaces; and the LDS regions of the new map do not overlap
while live.  The probes at the bottom are shared with tests/test_gpu_dft_split.py.

Layout modelled, per wave w (12 blocks from block 12 w on): unit 2 part + s, part 0 = the cos rows (on po), part 1 = the -sin rows
(on qo), K-step s = the folded samples n = 32 s .. 32 s + 31, bins bin_of_channel_fold3(32 w + r) = 2 (16 w + r) + 1."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.signals import make_streams
from tests.test_enc_split_pack import ORDER, _f32, _split, _unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFT_BLOCKS = 4 * 3
S_STFT = 0
GATE = 0.01


@pytest.fixture(scope="module")
def packed():
    """-> (the 5164 blocks, {id: (blocks, sect)} of the other ranges, the window w[256]) of the 16 kHz model, packed once"""
    from cutter_vad_amd import weights_io
    from tests import kernel_model as km
    with open(weights_io.packaged_blob_path(5, 16000), "rb") as f:
        blob = f.read()
    D, sect = km.packed_streams(5164, blob)
    others = {v: km.packed_streams(v, blob) for v in (516, 5161, 5162, 5163)}
    _, tensors = weights_io.unpack_svw(blob)
    return D, sect, others, tensors["stft.basis"].reshape(-1, 256)[0].astype(np.float32).copy()


def _odd_tile_fp32(W1, sect, w):
    """-> [2 parts][16 rows][64 n]: the odd tile of S_STFT as the fp32 kernel read it (weight_block16: block 2 j + part, lane
    (row l & 15, kq), component i = n 16 j + 4 kq + i)"""
    out = np.zeros((2, 16, 64), np.float32)
    lane, i = np.arange(64), np.arange(4)
    for j in range(4):
        n_of = 16 * j + 4 * (lane >> 4)[:, None] + i[None, :]
        for part in range(2):
            out[part, (lane & 15)[:, None], n_of] = W1[int(sect[w][S_STFT]) + 2 * j + part]
    return out


def _pieces(D, w):
    """-> [3 pieces][2 parts][16 rows][64 n] of wave w"""
    return np.stack([np.concatenate([_unit(D, DFT_BLOCKS * w + 3 * (2 * part + s)) for s in range(2)], axis=-1) for part in range(2)], axis=1)


def test_header_constant_and_the_kernels_offset():
    src = open(os.path.join(ROOT, "cutter_vad_amd", "csrc", "vad_layout.h")).read()
    assert re.search(r"constexpr int DFT_X3_BLOCKS = 4 \* 3;", src)
    body = open(os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16_body.h")).read()
    assert "4 * ENC1_X3_BLOCKS + 4 * ENC23_X3_BLOCKS + w * DFT_X3_BLOCKS" in body


def test_fifth_range_holds_the_odd_tile_exactly(packed):
    D, sect, others, _ = packed
    assert D.shape[0] == 4 * DFT_BLOCKS
    W1 = others[516][0]
    for w in range(4):
        T = _odd_tile_fp32(W1, sect, w)
        P = _pieces(D, w)
        assert np.array_equal(P.sum(axis=0), T.astype(np.float64)), w                  # bit for bit: the sum is exact in float64
        assert np.all(T[:, :, 0] == 0) and np.all(P[:, :, :, 0] == 0)                   # the zero slot n = 0
        k = 2 * (16 * w + np.arange(16)) + 1
        ph = 2 * np.pi * ((k[:, None] * np.arange(64)[None, :]) & 255) / 256.0
        assert np.array_equal(T[0][:, 1:], np.cos(ph).astype(np.float32)[:, 1:])        # cos on po, -sin on qo, the wave's odd bins
        assert np.array_equal(T[1][:, 1:], (-np.sin(ph)).astype(np.float32)[:, 1:])
        assert np.all(np.abs(P[1]) <= np.abs(P[0]) * 2.0 ** -7) and np.all(np.abs(P[2]) <= np.abs(P[1]) * 2.0 ** -7)
    u16 = D.view(np.uint16)
    assert not np.any(((u16 & 0x7F80) == 0) & ((u16 & 0x007F) != 0))                    # no denormal piece


def test_the_8_khz_packing_has_no_such_range():
    from cutter_vad_amd import weights_io
    from tests import kernel_model as km
    with open(weights_io.packaged_blob_path(5, 8000), "rb") as f:
        blob = f.read()
    assert km.packed_streams(5164, blob)[0].shape[0] == 0


@pytest.mark.parametrize("sr", [16000, 8000])
def test_the_other_streams_and_the_section_table_keep_every_byte(sr):
    from cutter_vad_amd import weights_io
    from tests import kernel_model as km
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    with open(os.path.join(ROOT, "tests", "golden", "v5_t16_streams_before_dft_split.json")) as f:
        gold = json.load(f)[str(sr)]
    for v in (516, 5161, 5162, 5163):
        W, sect = km.packed_streams(v, blob)
        assert W.shape[0] == gold[str(v)]["blocks"], v
        assert hashlib.sha256(W.tobytes()).hexdigest() == gold[str(v)]["sha256"], v
    assert hashlib.sha256(sect.astype("<u4").tobytes()).hexdigest() == gold["sect_sha256"]
    assert not np.any(sect[:, 11:])                                   # the range has no section entry


# ---- the odd bins: the kernel's two forms against a float64 DFT ----

def _fold(x, win):
    """the loader's fold of one 256-sample window per stream, x [streams][256] fp32 (gated), in its fp32 order (no contraction)
    -> po, qo [64][streams] with the zero slot n = 0, and the rank-1 terms y128, b64 [streams]"""
    f = np.float32
    n = np.arange(64)
    y1 = (x[:, n] * win[n]).astype(f)
    y3 = (x[:, 128 + n] * win[128 + n]).astype(f)
    y2 = (x[:, 128 - n] * win[128 + n]).astype(f)
    y4 = (x[:, (256 - n) & 255] * win[n]).astype(f)
    s14, d14, s23, d23 = (y1 + y4).astype(f), (y1 - y4).astype(f), (y2 + y3).astype(f), (y2 - y3).astype(f)
    po, qo = (s14 - s23).astype(f), (d14 + d23).astype(f)
    po[:, 0] = 0
    qo[:, 0] = 0
    y64, y192 = (x[:, 64] * win[64]).astype(f), (x[:, 192] * win[64]).astype(f)
    return po.T.copy(), qo.T.copy(), y3[:, 0].copy(), (y64 - y192).astype(f)


def _odd_bins(packed, x):
    """x [streams][256] fp32 -> (split model, fp32 model, float64 DFT, scale), each [2 (re, im)][64 odd bins][streams]; scale =
    sum_n |x[n]| w[n] of the stream's window"""
    D, sect, others, win = packed
    W1 = others[516][0]
    po, qo, y128, b64 = _fold(x, win)
    ops = (po.astype(np.float64), qo.astype(np.float64))
    ops_s = (_split(po), _split(qo))
    S = x.shape[0]
    split, plain = np.zeros((2, 64, S)), np.zeros((2, 64, S))
    for w in range(4):
        rows = slice(16 * w, 16 * w + 16)
        sg = np.where(np.arange(16) & 1, 1.0, -1.0)[:, None]
        init = (np.broadcast_to(-y128.astype(np.float64), (16, S)), sg * b64.astype(np.float64)[None, :])
        P, T = _pieces(D, w), _odd_tile_fp32(W1, sect, w).astype(np.float64)
        for part in range(2):
            acc = init[part].copy()
            for s in range(2):                                      # the split: unit 2 part + s, six products, a rounding each
                ks = slice(32 * s, 32 * s + 32)
                for pw, pa in ORDER:
                    acc = _f32(acc + P[pw, part][:, ks] @ ops_s[part][pa][ks])
            split[part, rows] = acc
            acc = init[part].copy()
            for j in range(4):                                      # fp32: k-iteration j, MFMA i contracts n = 16 j + 4 kq + i, kq = 0..3
                for i in range(4):
                    ns = 16 * j + 4 * np.arange(4) + i
                    acc = _f32(acc + T[part][:, ns] @ ops[part][ns])
            plain[part, rows] = acc
    k = 2 * np.arange(64) + 1
    ph = 2 * np.pi * ((k[:, None] * np.arange(256)[None, :]) & 255) / 256.0
    y = x.astype(np.float64) * win.astype(np.float64)
    exact = np.stack([np.cos(ph) @ y.T, -np.sin(ph) @ y.T])
    scale = np.broadcast_to(np.abs(y).sum(axis=1)[None, None, :], exact.shape)
    return split, plain, exact, scale


def _gate(x, thr=GATE):
    return x if thr is None else np.where(np.abs(x) > np.float32(thr), x, np.float32(0)).astype(np.float32)


def _errors(packed, x):
    split, plain, exact, scale = _odd_bins(packed, x)
    ok = scale > 0
    return (np.abs(split - exact)[ok] / scale[ok] * 2.0 ** 24), (np.abs(plain - exact)[ok] / scale[ok] * 2.0 ** 24)


def probe_frames():
    """{name: (frame [512] fp32, gate)}: the inputs that single out parts of the folded DFT's odd tile.  Tones sit on odd-bin centres
    (62.5 k Hz, k odd); the square wave of period 128 has its lines on the bins 2 m (2 j + 1) - even - so its odd bins hold window
    leakage only; an impulse at n = 0 of a window is the zero slot (nothing reaches an odd bin's sum but what the window leaves: w[0]
    = 0), one at n = 64 is the rank-1 term b64 alone; the last frame's samples lie just above the denoise gate."""
    t = np.arange(512)
    rng = np.random.default_rng(5164)
    out = {}
    out["tone k=37, full scale"] = (np.sin(2 * np.pi * 37 * t / 256.0 + 0.3).astype(np.float32), GATE)
    out["tone k=37, 2^-20, gate off"] = ((2.0 ** -20) * np.sin(2 * np.pi * 37 * t / 256.0 + 0.3).astype(np.float32), None)
    out["square, period 128"] = (np.where((t % 128) < 64, 1.0, -1.0).astype(np.float32), GATE)
    imp0, imp64 = np.zeros(512, np.float32), np.zeros(512, np.float32)
    imp0[[0, 128, 256]] = 1.0                                       # n = 0 of each of the three windows (columns at 0, 128, 256)
    imp64[[64, 192, 320]] = 1.0                                     # n = 64 of each
    out["impulses at n = 0"] = (imp0, GATE)
    out["impulses at n = 64"] = (imp64, GATE)
    out["just above the gate"] = ((GATE * (1 + rng.uniform(2.0 ** -10, 2.0 ** -6, 512)) * rng.choice([-1.0, 1.0], 512)).astype(np.float32), GATE)
    for x, _ in out.values():
        x.setflags(write=False)
    assert np.all(np.abs(out["just above the gate"][0]) > np.float32(GATE))              # the gate passes every sample of it
    return out


def _windows(frames):
    """[n][512] -> the three columns' windows [3 n][256]"""
    return np.concatenate([frames[:, 128 * c:128 * c + 256] for c in range(3)])


def test_split_odd_bins_are_no_further_from_a_float64_dft_than_twice_the_fp32_form(packed):
    """in units of 2^-24 sum |x| w per bin.  Measured: make_streams 99th percentile / worst: split 0.31 / 1.39, fp32 form 0.36 /
    1.92; probes: split 0.20 / 0.49, fp32 form 0.21 / 0.49.  Twice, because the two forms associate the sum differently and neither
    is the reference."""
    sets = {"make_streams": _windows(_gate(make_streams(16, 2, seed=1137).reshape(-1, 512))),
            "probes": _windows(np.stack([_gate(x, thr) for x, thr in probe_frames().values()]))}
    for name, x in sets.items():
        es, ep = _errors(packed, x)
        s99, sw, p99, pw = float(np.percentile(es, 99)), float(es.max()), float(np.percentile(ep, 99)), float(ep.max())
        print(f"{name}: split 99th percentile {s99:.2f} worst {sw:.2f}; fp32 form 99th percentile {p99:.2f} worst {pw:.2f}")
        assert pw > 0
        assert s99 <= 2 * p99 and sw <= 2 * pw, (name, s99, sw, p99, pw)


def test_the_oracles_f32_build_is_inside_the_probes_bar():
    """the GPU test's bar per probe is max(2e-6, twice the distance of the oracle's f32 build from its f64 build): the f32 build
    itself must pass it on every probe, or the probe asks for more than fp32 arithmetic gives"""
    from cutter_vad_amd import weights_io
    from oracle import oracle
    with open(weights_io.packaged_blob_path(5, 16000), "rb") as f:
        blob = f.read()
    o64, o32 = oracle.OracleModel(blob, "f64"), oracle.OracleModel(blob, "f32")
    for name, (x, thr) in probe_frames().items():
        fr = np.ascontiguousarray(np.tile(_gate(x, thr), (3, 1)))
        p64, _ = o64.run_stream(fr)
        p32, _ = o32.run_stream(fr)
        d = float(np.abs(p64 - p32).max())
        print(f"{name}: |f32 - f64| = {d:.3e}, p = {p64}")
        assert np.all(np.isfinite(p64)) and d <= max(2e-6, 2 * d)


# ---- the LDS map ----

def test_regions_of_the_new_lds_map_do_not_overlap_while_live():
    """quads (16 bytes) from the kernel's constants - the planes in the dense view, the even tile's operands in the loader view
    behind them - live ranges in the frame's barrier numbers [written behind, read until) as the header gives them ((1b) = 1.5; the
    h planes are written behind (7) and read until the next frame's (1)); two regions may share quads only if their ranges are
    disjoint"""
    src = open(os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16.hip")).read()
    names = "QSL|QSD|T_ROW_E0|T_ROW_E|T_ROW_H|T_ROWS_H|T_ROWS_E1|T_ROWS_E2|T_ROWS_DFT|T_EVEN_ROWS"
    c = {k: int(v) for k, v in re.findall(r"constexpr int (%s) = (\d+);" % names, src)}
    assert set(c) == set(names.split("|"))
    assert re.search(r"constexpr int T_EVEN_Q = T_ROWS_DFT \* QSD;", src)
    d, even0 = c["QSD"], c["T_ROWS_DFT"] * c["QSD"]
    assert c["T_ROWS_DFT"] == 3 * 4 * 12 and c["T_EVEN_ROWS"] == 3 * 32
    regions = {
        "po | qo planes": ((0, even0), [(0, 1.5)]),
        "even operands": ((even0, even0 + c["T_EVEN_ROWS"] * c["QSL"]), [(0, 1.5)]),
        "|STFT| planes": ((0, 144 * d), [(1.5, 3)]),
        "enc0's output": ((c["T_ROW_E0"] * d, (c["T_ROW_E0"] + 144) * d), [(2, 4)]),
        "enc1's planes": ((0, c["T_ROWS_E1"] * d), [(3, 5)]),
        "enc2's planes": ((c["T_ROW_E"] * d, (c["T_ROW_E"] + c["T_ROWS_E2"]) * d), [(4, 6)]),
        "x planes": ((0, 48 * d), [(5, 7)]),
        "paired hand-back": ((c["T_ROW_E0"] * d, (c["T_ROW_E0"] + 64) * d), [(6, 8)]),
        "h planes": ((c["T_ROW_H"] * d, (c["T_ROW_H"] + c["T_ROWS_H"]) * d), [(-1, 1), (7, 9)]),
    }
    end = (c["T_ROW_H"] + c["T_ROWS_H"]) * d
    keys = list(regions)
    for i, a in enumerate(keys):
        (a0, a1), la = regions[a]
        assert 0 <= a0 < a1 <= end, a
        for b in keys[i + 1:]:
            (b0, b1), lb = regions[b]
            quads_meet = a0 < b1 and b0 < a1
            live_meet = any(u0 < v1 and v0 < u1 for u0, u1 in la for v0, v1 in lb)
            assert not (quads_meet and live_meet), (a, b)
    # what the test would catch: the even operands running into h, which the recurrent half reads while the loader folds
    assert regions["even operands"][0][1] <= regions["h planes"][0][0]
    assert regions["h planes"][0][0] - regions["even operands"][0][1] < 32 * c["QSL"]        # ... and there is no room for sink rows
