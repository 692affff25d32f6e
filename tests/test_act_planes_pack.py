"""Activation planes of the 16-stream kernel (cutter_vad_amd/csrc/silero_v5_t16.hip): an activation that feeds a bf16-split layer is
cut into its three pieces by the lane that produces it and lies in LDS as the consumer's B fragments.  A NumPy model of the data
movement - producer lane -> plane group -> consumer fragment - must hand every consumer lane, element for element, the dwords that
split3_pair gives it for the fp32 value it used to read back: the move cannot change a bit of any MFMA operand.  And the packing's
third weight stream (S_ENC1_X3: encoder.1 on the bf16 split, which reads enc0's output as such planes): its pieces sum exactly to
enc1.w, the first two streams and their section entries are untouched, and a NumPy model of enc1 over the packed units stays within
the bound encoder.0 is held to.  CPU only.

Layouts modelled (vad_layout.h, S_LSTM_X3 / S_ENC0_X3; the kernel's header):
  D tile of wave w, row tile rt, lane (stream n, rq): channels 32 w + 16 rt + 4 rq + i, i = 0..3
  B fragment of K-step s, lane (n, kq): element e = channel 32 s + 16 (e >> 2) + 4 kq + (e & 3); dword d = elements 2 d, 2 d + 1
  plane group: piece p of lane (n, kq)'s fragment of K-step s = dwords [12 s + 4 p + kq][n][0..3]"""
import numpy as np
import pytest


def _hi16(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _split3_pair(a, b):
    """vadk_device.h split3_pair on arrays: the three dwords (low half = a's piece, high half = b's)"""
    out = []
    ra, rb = np.asarray(a, np.float32), np.asarray(b, np.float32)
    for k in range(3):
        ha, hb = _hi16(ra), _hi16(rb)
        out.append((hb.view(np.uint32) & np.uint32(0xFFFF0000)) | (ha.view(np.uint32) >> np.uint32(16)))
        if k < 2:
            ra, rb = (ra - ha).astype(np.float32), (rb - hb).astype(np.float32)
        else:
            assert np.all(ra == ha) and np.all(rb == hb)          # the third piece is the whole remainder: the sum is exact
    return out


def _consumer_fragments_from_fp32(x):
    """what the kernel did before: lane (n, kq) reads its two fp32 quads of K-step s and cuts them.  x [channels][16 streams] ->
    dwords [K-steps][3 pieces][4 kq][16 n][4 d]"""
    ns = x.shape[0] // 32
    F = np.zeros((ns, 3, 4, 16, 4), np.uint32)
    for s in range(ns):
        for kq in range(4):
            for d in range(4):
                ch = 32 * s + 16 * (d >> 1) + 4 * kq + 2 * (d & 1)
                p = _split3_pair(x[ch], x[ch + 1])
                for k in range(3):
                    F[s, k, kq, :, d] = p[k]
    return F


def _planes_from_full_tiles(x):
    """producers that own both row tiles of a K-step (16 kHz |STFT|, enc3's output, the cell's h, the prologue's h): wave w, lane
    (n, rq) cuts its quads rt = 0, 1 and writes three 16-byte pieces.  -> LDS dwords [12 ns rows][16 n][4]"""
    ns = x.shape[0] // 32
    L = np.full((12 * ns, 16, 4), 0xDEADBEEF, np.uint32)
    for w in range(ns):
        for rq in range(4):
            quad = [x[32 * w + 16 * rt + 4 * rq: 32 * w + 16 * rt + 4 * rq + 4] for rt in range(2)]       # [rt][i][n]
            for d in range(4):
                q = quad[d >> 1]
                p = _split3_pair(q[2 * (d & 1)], q[2 * (d & 1) + 1])
                for k in range(3):
                    L[12 * w + 4 * k + rq, :, d] = p[k]
    return L


def _planes_from_half_tiles(x):
    """8 kHz |STFT|: wave w owns ONE row tile (channels 16 w + 4 rq + i) = half w & 1 of K-step w >> 1's fragments, written as
    8-byte halves"""
    nw = x.shape[0] // 16
    L = np.full((12 * (nw // 2), 16, 4), 0xDEADBEEF, np.uint32)
    for w in range(nw):
        for rq in range(4):
            q = x[16 * w + 4 * rq: 16 * w + 4 * rq + 4]
            for j in range(2):
                p = _split3_pair(q[2 * j], q[2 * j + 1])
                for k in range(3):
                    L[12 * (w >> 1) + 4 * k + rq, :, 2 * (w & 1) + j] = p[k]
    return L


def _consumer_fragments_from_planes(L):
    ns = L.shape[0] // 12
    F = np.zeros((ns, 3, 4, 16, 4), np.uint32)
    for s in range(ns):
        for k in range(3):
            for kq in range(4):
                F[s, k, kq] = L[12 * s + 4 * k + kq]
    return F


def _activations(rng, channels):
    x = (np.maximum(rng.standard_normal((channels, 16)), 0.0) * np.exp(rng.uniform(-6, 3, (channels, 1)))).astype(np.float32)
    x[3, 5] = np.float32(2.0 ** -120)            # small but normal, zero, and a value whose third piece is empty
    x[7, 0] = 0.0
    x[9, 2] = np.float32(1.5)
    return x


@pytest.mark.parametrize("seed", [100, 101, 102, 103, 104])
def test_planes_written_by_the_producer_are_the_fragments_the_consumer_used_to_cut(seed):
    rng = np.random.default_rng(seed)
    for channels in (128, 64):                   # LSTM halves, enc0's input at 16 kHz | enc0's input at 8 kHz
        x = _activations(rng, channels)
        want = _consumer_fragments_from_fp32(x)
        L = _planes_from_full_tiles(x)
        assert not np.any(L == 0xDEADBEEF)       # every dword of the group is written (the values are non-negative: no 0xDEAD.. piece)
        assert np.array_equal(_consumer_fragments_from_planes(L), want)
    x = _activations(rng, 64)
    assert np.array_equal(_consumer_fragments_from_planes(_planes_from_half_tiles(x)), _consumer_fragments_from_fp32(x))


def test_signed_values_split_alike():
    """h is signed (the |STFT| columns and the ReLU'd tensors are not): the pieces of the producer and of the consumer are the same
    function of the value, so the sign changes nothing - and the pieces still sum exactly."""
    rng = np.random.default_rng(7)
    x = np.tanh(rng.standard_normal((128, 16)) * 2).astype(np.float32)
    F = _consumer_fragments_from_planes(_planes_from_full_tiles(x))
    assert np.array_equal(F, _consumer_fragments_from_fp32(x))
    lo = (F << np.uint32(16)).view(np.float32).astype(np.float64)
    hi = (F & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    for s in range(4):
        for kq in range(4):
            for d in range(4):
                ch = 32 * s + 16 * (d >> 1) + 4 * kq + 2 * (d & 1)
                assert np.array_equal(lo[s, :, kq, :, d].sum(axis=0), x[ch].astype(np.float64))
                assert np.array_equal(hi[s, :, kq, :, d].sum(axis=0), x[ch + 1].astype(np.float64))


def test_lds_map_of_the_16_stream_kernel_keeps_its_regions_apart():
    """the constants of the kernel's LDS map, read from the source: the h planes start past the loader view and end with the
    activation region; enc0's output planes start past the |STFT| planes (which other waves still read) and end inside the region;
    the enc2 partials lie past enc1's fp32 output and the x planes"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cutter_vad_amd", "csrc", "silero_v5_t16.hip")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (QSL|QSD|T_ROW_E0|T_ROW_E|T_ROW_H|T_ROWS_H|T_FOLD_SINK) = (\d+);", src)}
    end = c["T_ROW_H"] + c["T_ROWS_H"]
    assert c["T_ROWS_H"] == 48                                                      # four K-steps of h
    assert c["T_ROW_H"] * c["QSD"] >= (c["T_FOLD_SINK"] + 32) * c["QSL"]            # the loader view ends before h
    assert c["T_ROW_E0"] >= 3 * 48 and c["T_ROW_E0"] + 3 * 48 <= end                # three columns of planes each
    assert c["T_ROW_E"] >= 48 and c["T_ROW_E"] + 32 <= end


# ---- the third weight stream: encoder.1 on the bf16 split (vad_layout.h, S_ENC1_X3) ----
S_ENC1_X3 = 10
ENC1_F32 = 1                        # fp32 blocks (the bias) in front of a wave's units
ENC1_BLOCKS = ENC1_F32 + 3 * 4 * 3  # + (4 K-steps x 3 taps) units of three pieces


def _pack3(sr):
    from cutter_vad_amd import weights_io
    from tests import kernel_model as km
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    streams = {v: km.packed_streams(v, blob) for v in (516, 5161, 5162)}
    _, tensors = weights_io.unpack_svw(blob)
    return streams, tensors


def _enc1_pieces(W, sect, w):
    """-> pieces [3 pieces][3 taps][16 rows of wave w][128 K] of the packed units"""
    from tests.test_enc_split_pack import _unit
    P = np.zeros((3, 3, 16, 128))
    for s in range(4):
        for t in range(3):
            P[:, t, :, 32 * s:32 * s + 32] = _unit(W, int(sect[w][S_ENC1_X3]) + ENC1_F32 + 3 * (s * 3 + t))
    return P


@pytest.mark.parametrize("sr", [16000, 8000])
def test_third_stream_holds_enc1_and_the_other_two_are_unchanged(sr):
    from tests.test_enc_split_pack import _vec
    streams, T = _pack3(sr)
    (W1, s1), (W2, s2), (W3, s3) = streams[516], streams[5161], streams[5162]
    assert np.array_equal(s1, s2) and np.array_equal(s1, s3)              # one section table for the three streams
    assert not np.any(s3[:, 11:])                                         # entries 0..9 as before, 10 is new, nothing behind it
    assert [int(s3[w][S_ENC1_X3]) for w in range(4)] == [ENC1_BLOCKS * w for w in range(4)]
    assert W3.shape[0] == 4 * ENC1_BLOCKS
    # (tests/test_enc_split_pack.py pins the first stream's length and section order and the second's length)
    assert W1.shape[0] > W2.shape[0] > W3.shape[0]
    w1 = T["enc1.w"].astype(np.float64)
    for w in range(4):
        rows = slice(16 * w, 16 * w + 16)
        assert np.array_equal(_vec(W3, int(s3[w][S_ENC1_X3])), T["enc1.b"][rows].astype(np.float64))
        P = _enc1_pieces(W3, s3, w)
        assert np.array_equal(P.sum(axis=0), np.transpose(w1[rows], (2, 0, 1))), (sr, w)     # exactly the fp32 weights, natural channel order
        assert np.all(np.abs(P[1]) <= np.abs(P[0]) * 2.0 ** -7) and np.all(np.abs(P[2]) <= np.abs(P[1]) * 2.0 ** -7)
        u16 = W3[int(s3[w][S_ENC1_X3]) + ENC1_F32: int(s3[w][S_ENC1_X3]) + ENC1_BLOCKS].view(np.uint16)
        assert not np.any(((u16 & 0x7F80) == 0) & ((u16 & 0x007F) != 0))                       # no denormal piece


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("seed", [100, 101, 102, 103, 104])
def test_split_enc1_over_the_packed_units_matches_the_exact_convolution(sr, seed):
    """enc1 as the kernel computes it - bias as the accumulators' start, per K-step and tap the six products of mfma_x3 in its order
    into every output column the tap reaches, one fp32 rounding per MFMA - against the exact float64 convolution, relative to
    |b| + sum |w| |x| in units of 2^-24.  The bound is the one tests/test_enc_split_pack.py holds enc0 to (99th percentile <= 4,
    worst <= 8): enc1 takes fewer roundings per output (2 taps x 4 K-steps x 6).  A truncation-split model of enc1.w without the
    packer gives 2.2 - 2.7 / 3.5 - 4.4 on these inputs."""
    from tests.test_enc_split_pack import _split_conv
    streams, T = _pack3(sr)
    W3, s3 = streams[5162]
    rng = np.random.default_rng(seed)
    x = (np.maximum(rng.standard_normal((3, 128, 16)), 0.0) * np.exp(rng.uniform(-6, 3, (3, 128, 1)))).astype(np.float32)
    w1, b1 = T["enc1.w"].astype(np.float64), T["enc1.b"].astype(np.float64)
    xd = x.astype(np.float64)
    rels = []
    for w in range(4):
        rows = slice(16 * w, 16 * w + 16)
        acc = np.broadcast_to(b1[rows][None, :, None], (2, 16, 16)).astype(np.float64).copy()
        acc = _split_conv(_enc1_pieces(W3, s3, w), x, acc, 2, 2)
        for o in range(2):
            exact = np.broadcast_to(b1[rows][:, None], (16, 16)).copy()
            scale = np.abs(exact)
            for t in range(3):
                c = 2 * o + t - 1
                if 0 <= c < 3:
                    exact = exact + w1[rows, :, t] @ xd[c]
                    scale = scale + np.abs(w1[rows, :, t]) @ np.abs(xd[c])
            rels.append(np.abs(acc[o] - exact) / scale * 2.0 ** 24)
    rel = np.concatenate([r.ravel() for r in rels])
    print(f"{sr} Hz seed {seed}: 99th percentile {np.percentile(rel, 99):.2f}, worst {rel.max():.2f}")
    assert rel.max() > 0
    assert np.percentile(rel, 99) <= 4 and rel.max() <= 8, (np.percentile(rel, 99), rel.max())
