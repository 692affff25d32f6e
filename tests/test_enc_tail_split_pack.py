"""encoder.2 and encoder.3 of the 16-stream kernel on the bf16 split (vad_layout.h, ENC23_X3_BLOCKS): the packing's fourth block
range (vad_debug_pack_weights id 5163; the engine uploads it behind the third stream, in the same buffer).  CPU only: its pieces sum
exactly to the centre / right taps the layers use, in natural channel order; the three existing streams and the section table keep
every byte (hashes of a packing made before the range existed, tests/golden/v5_t16_streams_before_enc_tail.json); a NumPy model of
the kernel's order - bias as the accumulator's start, the units in order, the six products of mfma_x3, one fp32 rounding per MFMA -
stays within the bound encoder.0 and encoder.1 are held to; and the LDS regions of the kernel's map do not overlap while live.

Layout modelled, per wave w (27 blocks from block 27 w on):
  enc2: 1 bias block (channels 16 w + r), then 4 units (input column c on tap 1 + c, K-step s), unit 2 c + s
  enc3: 2 bias blocks (channels 32 w + 16 rt + r), then 4 units (K-step s, rt), unit 2 s + rt, centre tap"""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.test_enc_split_pack import ORDER, _f32, _split, _unit, _vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC2_BLOCKS = 1 + 4 * 3
ENC3_BLOCKS = 2 + 4 * 3
ENC23_BLOCKS = ENC2_BLOCKS + ENC3_BLOCKS


def _layout_constants():
    src = open(os.path.join(ROOT, "cutter_vad_amd", "csrc", "vad_layout.h")).read()
    return {k: v for k, v in re.findall(r"constexpr int (ENC2_X3_BLOCKS|ENC3_X3_BLOCKS|ENC23_X3_BLOCKS|ENC1_X3_BLOCKS) = ([^;]+);", src)}


@pytest.fixture(scope="module", params=[16000, 8000])
def packed(request):
    """-> (sample rate, the 5163 blocks, the other three streams, the blob's tensors), packed once per rate"""
    from cutter_vad_amd import weights_io
    from tests import kernel_model as km
    sr = request.param
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    Z, sect = km.packed_streams(5163, blob)
    others = {v: km.packed_streams(v, blob) for v in (516, 5161, 5162)}
    _, tensors = weights_io.unpack_svw(blob)
    return sr, Z, sect, others, tensors


def _enc2_pieces(Z, w):
    """-> pieces [3][4 units][16 rows][32 K] of wave w"""
    return np.stack([_unit(Z, ENC23_BLOCKS * w + 1 + 3 * u) for u in range(4)], axis=1)


def _enc3_pieces(Z, w):
    """-> pieces [3][K-step s][rt][16 rows][32 K] of wave w"""
    base = ENC23_BLOCKS * w + ENC2_BLOCKS + 2
    return np.stack([np.stack([_unit(Z, base + 3 * (2 * s + rt)) for rt in range(2)], axis=1) for s in range(2)], axis=1)


def test_header_constants_are_the_ones_modelled_here():
    c = _layout_constants()
    assert c["ENC2_X3_BLOCKS"].replace(" ", "") == "1+4*3" and c["ENC3_X3_BLOCKS"].replace(" ", "") == "2+4*3"
    assert c["ENC23_X3_BLOCKS"].replace(" ", "") == "ENC2_X3_BLOCKS+ENC3_X3_BLOCKS"


def test_fourth_range_holds_enc2_and_enc3_exactly(packed):
    sr, Z, sect, others, T = packed
    assert Z.shape[0] == 4 * ENC23_BLOCKS
    w2, w3 = T["enc2.w"].astype(np.float64), T["enc3.w"].astype(np.float64)
    assert w2.shape == (64, 64, 3) and w3.shape == (128, 64, 3)
    for w in range(4):
        base = ENC23_BLOCKS * w
        r2 = slice(16 * w, 16 * w + 16)
        assert np.array_equal(Z[base].reshape(4, 16, 4)[:, 0, :].reshape(16), T["enc2.b"][r2])          # bit-equal fp32
        assert np.array_equal(Z[base], np.broadcast_to(T["enc2.b"][r2].reshape(4, 1, 4), (4, 16, 4)).reshape(64, 4))
        P2 = _enc2_pieces(Z, w)
        for col in range(2):
            for s in range(2):
                assert np.array_equal(P2[:, 2 * col + s].sum(axis=0), w2[r2, 32 * s:32 * s + 32, 1 + col]), (sr, w, col, s)
        P3 = _enc3_pieces(Z, w)
        for rt in range(2):
            r3 = slice(32 * w + 16 * rt, 32 * w + 16 * rt + 16)
            assert np.array_equal(_vec(Z, base + ENC2_BLOCKS + rt).astype(np.float32), T["enc3.b"][r3])
            for s in range(2):
                assert np.array_equal(P3[:, s, rt].sum(axis=0), w3[r3, 32 * s:32 * s + 32, 1]), (sr, w, rt, s)
        for P in (P2, P3):
            assert np.all(np.abs(P[1]) <= np.abs(P[0]) * 2.0 ** -7) and np.all(np.abs(P[2]) <= np.abs(P[1]) * 2.0 ** -7)
        for lo, hi in ((base + 1, base + ENC2_BLOCKS), (base + ENC2_BLOCKS + 2, base + ENC23_BLOCKS)):
            u16 = Z[lo:hi].view(np.uint16)
            assert not np.any(((u16 & 0x7F80) == 0) & ((u16 & 0x007F) != 0))                             # no denormal piece


def test_the_three_streams_and_the_section_table_keep_every_byte(packed):
    sr, Z, sect, others, T = packed
    with open(os.path.join(ROOT, "tests", "golden", "v5_t16_streams_before_enc_tail.json")) as f:
        gold = json.load(f)[str(sr)]
    for v, (W, s) in others.items():
        assert W.shape[0] == gold[str(v)]["blocks"], v
        assert hashlib.sha256(W.tobytes()).hexdigest() == gold[str(v)]["sha256"], v
        assert np.array_equal(s, sect)
    assert hashlib.sha256(sect.astype("<u4").tobytes()).hexdigest() == gold["sect_sha256"]
    assert not np.any(sect[:, 11:])                                   # the range has no section entry


def _inputs(seed):
    """the activations of tests/test_act_planes_pack.py's enc1 model - ReLU'd normals over a wide range of channel scales - in enc2's
    input shape [2 columns][64 channels][16 streams]"""
    rng = np.random.default_rng(seed)
    return (np.maximum(rng.standard_normal((2, 64, 16)), 0.0) * np.exp(rng.uniform(-6, 3, (2, 64, 1)))).astype(np.float32)


def _rel(acc, exact, scale):
    return (np.abs(acc - exact) / scale * 2.0 ** 24).ravel()


@pytest.mark.parametrize("seed", [100, 101, 102, 103, 104])
def test_split_enc2_and_enc3_over_the_packed_units_match_the_exact_sums(packed, seed):
    """relative to |b| + sum |w| |x| in units of 2^-24: 99th percentile <= 4, worst <= 8, the bar of encoder.0 and encoder.1.  enc2
    takes 24 roundings per output, enc3 12; enc3 is fed the ReLU of the model's own enc2.  A truncation-split model of the weights
    without the packer gives 1.75 - 2.44 / 2.69 - 3.89 (enc2) and 1.25 - 1.54 / 1.91 - 3.26 (enc3) over these seeds and both rates."""
    sr, Z, sect, others, T = packed
    x = _inputs(seed)
    xs = [_split(x[c]) for c in range(2)]
    xd = x.astype(np.float64)
    w2, b2 = T["enc2.w"].astype(np.float64), T["enc2.b"].astype(np.float64)
    w3, b3 = T["enc3.w"].astype(np.float64), T["enc3.b"].astype(np.float64)
    e2 = np.zeros((64, 16))
    rel2 = []
    for w in range(4):
        rows = slice(16 * w, 16 * w + 16)
        P = _enc2_pieces(Z, w)
        acc = np.broadcast_to(b2[rows][:, None], (16, 16)).copy()
        for u in range(4):
            col, ks = u >> 1, slice(32 * (u & 1), 32 * (u & 1) + 32)
            for pw, pa in ORDER:
                acc = _f32(acc + P[pw, u] @ xs[col][pa][ks])
        exact = b2[rows][:, None] + w2[rows, :, 1] @ xd[0] + w2[rows, :, 2] @ xd[1]
        scale = np.abs(b2[rows])[:, None] + np.abs(w2[rows, :, 1]) @ np.abs(xd[0]) + np.abs(w2[rows, :, 2]) @ np.abs(xd[1])
        rel2.append(_rel(acc, exact, scale))
        e2[rows] = np.maximum(acc, 0.0)
    y = e2.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), e2)                    # the model's enc2 IS fp32
    ys, yd = _split(y), e2
    rel3 = []
    for w in range(4):
        P = _enc3_pieces(Z, w)
        for rt in range(2):
            rows = slice(32 * w + 16 * rt, 32 * w + 16 * rt + 16)
            acc = np.broadcast_to(b3[rows][:, None], (16, 16)).copy()
            for s in range(2):
                ks = slice(32 * s, 32 * s + 32)
                for pw, pa in ORDER:
                    acc = _f32(acc + P[pw, s, rt] @ ys[pa][ks])
            exact = b3[rows][:, None] + w3[rows, :, 1] @ yd
            scale = np.abs(b3[rows])[:, None] + np.abs(w3[rows, :, 1]) @ np.abs(yd)
            rel3.append(_rel(acc, exact, scale))
    for name, rel in (("enc2", np.concatenate(rel2)), ("enc3", np.concatenate(rel3))):
        p99, worst = float(np.percentile(rel, 99)), float(rel.max())
        print(f"{sr} Hz seed {seed} {name}: 99th percentile {p99:.2f}, worst {worst:.2f}")
        assert worst > 0
        assert p99 <= 4 and worst <= 8, (name, p99, worst)


@pytest.mark.parametrize("sr", [16000, 8000])
def test_plane_regions_of_the_lds_map_do_not_overlap_while_live(sr):
    """rows from the kernel's constants, live ranges in the frame's barrier numbers [written behind, read until) as the header gives
    them ((1b) = 1.5; the h planes are written behind (7) and read until the next frame's (1)); two regions may share rows only if
    their ranges are disjoint"""
    src = open(os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16.hip")).read()
    names = "T_ROW_E0|T_ROW_E|T_ROW_H|T_ROWS_H|T_ROWS_E1|T_ROWS_E2"
    c = {k: int(v) for k, v in re.findall(r"constexpr int (%s) = (\d+);" % names, src)}
    assert set(c) == set(names.split("|"))
    body = open(os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16_body.h")).read()
    assert re.search(r"constexpr int PP = K8 \? 24 : 48;", body)
    pp = 48 if sr == 16000 else 24
    assert c["T_ROWS_E1"] == 2 * 2 * 12 and c["T_ROWS_E2"] == 2 * 12 and c["T_ROWS_H"] == 4 * 12
    regions = {
        "|STFT| planes": ((0, 3 * pp), [(1.5, 3)]),
        "enc0's output": ((c["T_ROW_E0"], c["T_ROW_E0"] + 3 * 48), [(2, 4)]),
        "enc1's planes": ((0, c["T_ROWS_E1"]), [(3, 5)]),
        "enc2's planes": ((c["T_ROW_E"], c["T_ROW_E"] + c["T_ROWS_E2"]), [(4, 6)]),
        "x planes": ((0, 48), [(5, 7)]),
        "paired hand-back": ((c["T_ROW_E0"], c["T_ROW_E0"] + 64), [(6, 8)]),
        "h planes": ((c["T_ROW_H"], c["T_ROW_H"] + c["T_ROWS_H"]), [(0, 1), (7, 9)]),
    }
    end = c["T_ROW_H"] + c["T_ROWS_H"]
    keys = list(regions)
    for i, a in enumerate(keys):
        (a0, a1), la = regions[a]
        assert 0 <= a0 < a1 <= end, a
        for b in keys[i + 1:]:
            (b0, b1), lb = regions[b]
            rows_meet = a0 < b1 and b0 < a1
            live_meet = any(u0 < v1 and v0 < u1 for u0, u1 in la for v0, v1 in lb)
            assert not (rows_meet and live_meet), (a, b)
    # what the test would catch: enc2's planes where enc1's are still read
    assert regions["enc1's planes"][0][1] <= regions["enc2's planes"][0][0]
