"""The packer's S_LSTM_X3 section (vad_layout.h): the 16-stream kernel's LSTM weights as three exact bf16 pieces, laid out as the A
fragments of v_mfma_f32_16x16x32_bf16.  CPU only: the planes must sum to the blob's fp32 weights exactly, the section must sit behind
every other one, and a NumPy model of the kernel's six-product contraction must agree with the fp32 contraction of S_LSTM."""

import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests import kernel_model as km

S_LSTM_X3 = 8
HALF = 4 * 8 * 3          # blocks per half: 4 K-steps x 8 row tiles x 3 pieces


def _bf16_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _planes(W, base, half):
    """-> pieces [3][512 rows local to the wave's order: (gate q, unit 0..31)][128 K] as float64, read back from the blocks"""
    u16 = W.view(np.uint16).reshape(W.shape[0], 64, 8)
    P = np.zeros((3, 4, 32, 128))
    lane = np.arange(64)
    e = np.arange(8)
    k_of = 16 * (e >> 2)[None, :] + 4 * (lane >> 4)[:, None] + (e & 3)[None, :]        # [lane][element]
    for s in range(4):
        for q in range(4):
            for rt in range(2):
                for p in range(3):
                    blk = u16[base + half * HALF + (s * 8 + 2 * q + rt) * 3 + p]
                    P[p, q, (16 * rt + (lane & 15))[:, None], 32 * s + k_of] = _bf16_to_f64(blk)
    return P


def _pack(sr):
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    W, sect = km.packed_streams(516, blob)
    _, tensors = weights_io.unpack_svw(blob)
    return W, sect, tensors


@pytest.mark.parametrize("sr", [16000, 8000])
def test_planes_sum_exactly_to_the_fp32_weights(sr):
    W, sect, T = _pack(sr)
    old_end = int(sect[0][km.S_NYQ]) + 1                    # the fp32 stream ends with the window block
    assert sorted(int(sect[w][S_LSTM_X3]) for w in range(4)) == [old_end + 2 * HALF * w for w in range(4)]
    assert W.shape[0] == old_end + 4 * 2 * HALF
    for w in range(4):
        for half, name in enumerate(("lstm.w_ih", "lstm.w_hh")):
            M = T[name].reshape(4, 128, 128)[:, 32 * w:32 * w + 32, :].astype(np.float64)
            P = _planes(W, int(sect[w][S_LSTM_X3]), half)
            assert np.array_equal(P.sum(axis=0), M), (sr, w, name)
            # truncation pieces: |w2| < 2^-7 |w1|, |w3| < 2^-7 |w2| (each piece carries the next 8 significant bits)
            assert np.all(np.abs(P[1]) <= np.abs(P[0]) * 2.0 ** -7)
            assert np.all(np.abs(P[2]) <= np.abs(P[1]) * 2.0 ** -7)


def _split(x):
    """fp32 -> three float64 pieces as the kernel cuts them (vadk_device.h: split3_pair)"""
    x = np.asarray(x, np.float32)
    m = np.uint32(0xFFFF0000)
    x1 = (x.view(np.uint32) & m).view(np.float32)
    r = (x - x1).astype(np.float32)
    x2 = (r.view(np.uint32) & m).view(np.float32)
    x3 = (r - x2).astype(np.float32)
    assert np.all((x3.view(np.uint32) & np.uint32(0xFFFF)) == 0)
    return [v.astype(np.float64) for v in (x1, x2, x3)]


def test_six_product_contraction_matches_the_fp32_section():
    """relative to the condition scale |b| + sum |w| |a| of each gate output: 4 x 2^-24 is four fp32 roundings of that scale"""
    W, sect, T = _pack(16000)
    rng = np.random.default_rng(11)
    nstr = 16
    x = np.maximum(rng.standard_normal((128, nstr)), 0).astype(np.float32)        # enc3's ReLU output
    h = np.tanh(rng.standard_normal((128, nstr))).astype(np.float32)              # h_{t-1}
    xs, hs = _split(x), _split(h)
    # (weight piece, activation piece) in the kernel's order: mfma_x3
    order = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]
    worst = 0.0
    for w in range(4):
        # the fp32 weights S_LSTM holds (the blob's own; tests/kernel_model.py checks that section's layout), of the wave's units:
        # rows [gate q][unit 32 w + ..]
        wih = T["lstm.w_ih"].reshape(4, 128, 128)[:, 32 * w:32 * w + 32, :].astype(np.float64)
        whh = T["lstm.w_hh"].reshape(4, 128, 128)[:, 32 * w:32 * w + 32, :].astype(np.float64)
        b = (T["lstm.b_ih"] + T["lstm.b_hh"]).astype(np.float32).reshape(4, 128)[:, 32 * w:32 * w + 32].astype(np.float64)
        exact = b[..., None] + np.einsum("qrk,kn->qrn", whh, h.astype(np.float64)) + np.einsum("qrk,kn->qrn", wih, x.astype(np.float64))
        scale = np.abs(b)[..., None] + np.einsum("qrk,kn->qrn", np.abs(whh), np.abs(h)) + np.einsum("qrk,kn->qrn", np.abs(wih), np.abs(x))
        # the split form: recurrent half first, then the input half; per K-step one fp32 rounding per MFMA (products exact, the
        # MFMA's 32-term sum taken as exact)
        acc = np.broadcast_to(b[..., None], exact.shape).astype(np.float32)
        for half, act in ((1, hs), (0, xs)):
            P = _planes(W, int(sect[w][S_LSTM_X3]), half)
            for s in range(4):
                ks = slice(32 * s, 32 * s + 32)
                for pw, pa in order:
                    acc = (acc.astype(np.float64) + np.einsum("qrk,kn->qrn", P[pw][:, :, ks], act[pa][ks])).astype(np.float32)
        # the fp32 form (v_mfma_f32_16x16x4_f32 = an fmaf chain): sequential fp32 accumulation over K, recurrent half first
        ref = np.broadcast_to(b[..., None], exact.shape).astype(np.float32)
        for M, a in ((whh, h), (wih, x)):
            for k in range(128):
                ref = (ref.astype(np.float64) + M[:, :, k:k + 1] * a[k].astype(np.float64)).astype(np.float32)
        # the split form is within 4 ulp-of-scale of the exact sum, and apart from the fp32 form by no more than the fp32 form's own
        # rounding error (up to ~7 x 2^-24 of scale: 256 roundings against the split's 48) plus that
        err_split = np.abs(acc - exact) / scale
        err_f32 = np.abs(ref - exact) / scale
        assert float(err_split.max()) <= 4 * 2.0 ** -24
        assert np.all(np.abs(acc.astype(np.float64) - ref) / scale <= err_f32 + 4 * 2.0 ** -24)
        worst = max(worst, float(err_split.max()))
    assert worst > 0          # the model does round
