"""The packer's S_ENC0_X3 section (vad_layout.h): encoder.0 of the 16-stream kernel as a direct 3-tap convolution on three exact
bf16 pieces, laid out as the A fragments of v_mfma_f32_16x16x32_bf16.  CPU only: the planes must sum to the blob's fp32 weights
exactly, the section must fill the packing's second stream (the first keeps every byte it had), a NumPy model of the kernel's
enc0 -> enc1 dataflow over the packed blocks (enc0 split, enc1 in fp32) must stay within a few fp32 roundings of the exact
convolutions, and no instantiation of the kernel may spill registers."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests import kernel_model as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_LSTM_X3, S_ENC0_X3 = 8, 9          # vad_layout.h Section
LSTM_X3 = 2 * 4 * 8 * 3            # blocks per wave of S_LSTM_X3
ENC0_F32 = 8                        # fp32 blocks in front of the units
# (weight piece, activation piece) in the kernel's order: vadk_device.h mfma_x3
ORDER = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]


def _bf16_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _unit(W, blk):
    """-> pieces [3][16 rows][32 K] of the unit whose first block is blk (lane = (row l & 15, kq = l >> 4), element e = K
    16 (e >> 2) + 4 kq + (e & 3))"""
    u16 = W.view(np.uint16).reshape(W.shape[0], 64, 8)
    lane, e = np.arange(64), np.arange(8)
    k_of = 16 * (e >> 2)[None, :] + 4 * (lane >> 4)[:, None] + (e & 3)[None, :]
    P = np.zeros((3, 16, 32))
    for p in range(3):
        P[p, (lane & 15)[:, None], k_of] = _bf16_to_f64(u16[blk + p])
    return P


def _vec(W, blk):
    """a vector_block16: lane (n, kq) register i = channel 4 kq + i -> [16]"""
    return W[blk].reshape(4, 16, 4)[:, 0, :].reshape(16).astype(np.float64)


def _bin_fold3(ch):
    if ch & 16 == 0:
        return 2 * (16 * (ch >> 5) + (ch & 15)) + 1
    return 4 * (16 * (ch >> 5) + (ch & 15)) + 2 if (ch >> 5) < 2 else 4 * (16 * ((ch >> 5) - 2) + (ch & 15))


def _bin_8k(ch):
    return 2 * (ch & 31) + (ch >> 5)


def _pack(sr):
    """-> (the second stream of the 16-stream V5 packing, which holds S_ENC0_X3, section table, blob tensors)"""
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    W, sect = km.packed_streams(5161, blob)
    _, tensors = weights_io.unpack_svw(blob)
    return W, sect, tensors


def _enc0_planes(W, sect, w, ns):
    """-> pieces [3 pieces][3 taps][32 rows of wave w][32 ns K], K in the kernel's channel order"""
    P = np.zeros((3, 3, 32, 32 * ns))
    for s in range(ns):
        for t in range(3):
            for rt in range(2):
                P[:, t, 16 * rt:16 * rt + 16, 32 * s:32 * s + 32] = _unit(W, int(sect[w][S_ENC0_X3]) + ENC0_F32 + 3 * ((s * 3 + t) * 2 + rt))
    return P


@pytest.mark.parametrize("sr", [16000, 8000])
def test_second_stream_holds_the_split_encoders_and_the_first_is_unchanged(sr):
    with open(weights_io.packaged_blob_path(5, sr), "rb") as f:
        blob = f.read()
    W1, sect1 = km.packed_streams(516, blob)
    W, sect, _ = _pack(sr)
    assert np.array_equal(sect, sect1)                          # one section table for both streams
    old_end = int(sect[0][km.S_NYQ]) + 1                       # the fp32 sections end with the window block
    # the first stream: the fp32 sections in their old order, then S_LSTM_X3, and nothing behind it
    assert sorted(int(sect[w][S_LSTM_X3]) for w in range(4)) == [old_end + LSTM_X3 * w for w in range(4)]
    assert W1.shape[0] == old_end + 4 * LSTM_X3
    for w in range(4):
        offs = [int(sect[w][k]) for k in (km.S_STFT, km.S_ENC0, km.S_ENC1, km.S_ENC3, km.S_LSTM)]
        assert offs == sorted(offs) and offs[-1] < old_end
    # the second: S_ENC0_X3 of the four waves
    ns = 4 if sr == 16000 else 2
    e0 = ENC0_F32 + 3 * ns * 3 * 2
    assert [int(sect[w][S_ENC0_X3]) for w in range(4)] == [e0 * w for w in range(4)]
    assert W.shape[0] == 4 * e0


@pytest.mark.parametrize("sr", [16000, 8000])
def test_planes_sum_exactly_to_the_fp32_conv_weights(sr):
    W, sect, T = _pack(sr)
    ns = 4 if sr == 16000 else 2
    w0 = T["enc0.w"].astype(np.float64)
    nb = w0.shape[1]
    cin = [(_bin_fold3 if sr == 16000 else _bin_8k)(ch) for ch in range(32 * ns)]
    assert sorted(cin) == list(range(nb - 1))
    for w in range(4):
        base = int(sect[w][S_ENC0_X3])
        rows = slice(32 * w, 32 * w + 32)
        for rt in range(2):
            r = slice(32 * w + 16 * rt, 32 * w + 16 * rt + 16)
            assert np.array_equal(_vec(W, base + rt), T["enc0.b"][r].astype(np.float64))
            for t in range(3):
                assert np.array_equal(_vec(W, base + 2 + 2 * t + rt), w0[r, nb - 1, t])
        P = _enc0_planes(W, sect, w, ns)
        assert np.array_equal(P.sum(axis=0), np.transpose(w0[rows][:, cin, :], (2, 0, 1))), (sr, w)
        # truncation pieces: each carries the next 8 significant bits
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


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _split_conv(P, x, acc, stride, nout):
    """the kernel's X3_CONV: P pieces [3][3 taps][rows][K], x [3 columns][K][streams] fp32, acc [nout][rows][streams] fp32; per
    K-step and unit (tap) the tap's products into every output column it reaches, one fp32 rounding per MFMA (products exact, the
    MFMA's 32-term sum taken as exact)"""
    xs = [_split(xc) for xc in x]
    for s in range(P.shape[-1] // 32):
        ks = slice(32 * s, 32 * s + 32)
        for t in range(3):
            for o in range(nout):
                c = stride * o + t - 1
                if 0 <= c < 3:
                    for pw, pa in ORDER:
                        acc[o] = _f32(acc[o] + P[pw, t][:, ks] @ xs[c][pa][ks])
    return acc


@pytest.mark.parametrize("sr", [16000, 8000])
def test_split_dataflow_of_enc0_and_enc1_matches_the_exact_convolutions(sr):
    """relative to the condition scale |b| + sum |w| |x| of each output, in units of 2^-24 (one fp32 rounding of that scale): the
    99th percentile within 4, the worst within 8.  Up to 75 roundings go into an output (3 taps x 4 K-steps x 6 MFMAs + the Nyquist
    fmas); a sequential fp32 fma chain over the same 387 terms, as the fp32 form computes it, reaches 8 - 17 on these inputs."""
    W, sect, T = _pack(sr)
    ns = 4 if sr == 16000 else 2
    rng = np.random.default_rng(31 + ns)
    nstr = 16
    nb = T["enc0.w"].shape[1]
    # |STFT| of three columns, the kernel's channel order, with the Nyquist channel apart; a wide dynamic range, as real spectra have
    mags = (np.abs(rng.standard_normal((3, nb, nstr))) * np.exp(rng.uniform(-6, 3, (3, nb, 1)))).astype(np.float32)
    cin = [(_bin_fold3 if sr == 16000 else _bin_8k)(ch) for ch in range(32 * ns)]
    x = mags[:, cin, :]
    nyq = mags[:, nb - 1, :].astype(np.float64)
    w0 = T["enc0.w"].astype(np.float64)
    w1 = T["enc1.w"].astype(np.float64)
    xin = [mags[c].astype(np.float64) for c in range(3)]

    def conv(wt, b, cols, stride, nout):
        out, scale = [], []
        for o in range(nout):
            acc, sc = np.broadcast_to(b[:, None], (wt.shape[0], nstr)).copy(), np.abs(np.broadcast_to(b[:, None], (wt.shape[0], nstr)))
            for t in range(3):
                c = stride * o + t - 1
                if 0 <= c < 3:
                    acc = acc + wt[:, :, t] @ cols[c]
                    sc = sc + np.abs(wt[:, :, t]) @ np.abs(cols[c])
            out.append(acc)
            scale.append(sc)
        return np.array(out), np.array(scale)

    worst = 0.0
    e0 = np.zeros((3, 128, nstr))
    for w in range(4):
        base = int(sect[w][S_ENC0_X3])
        acc = np.zeros((3, 32, nstr))
        for rt in range(2):
            rows = slice(16 * rt, 16 * rt + 16)
            b = _vec(W, base + rt)[:, None]
            for o in range(3):
                a = np.broadcast_to(b, (16, nstr)).astype(np.float64)
                for t in range(3):
                    c = o + t - 1
                    if 0 <= c < 3:
                        a = _f32(a + _vec(W, base + 2 + 2 * t + rt)[:, None] * nyq[c][None, :])     # exact fmaf
                acc[o, rows] = a
        acc = _split_conv(_enc0_planes(W, sect, w, ns), x, acc, 1, 3)
        exact, scale = conv(w0[32 * w:32 * w + 32], T["enc0.b"][32 * w:32 * w + 32].astype(np.float64), xin, 1, 3)
        rel = np.abs(acc - exact) / scale * 2.0 ** 24
        assert np.percentile(rel, 99) <= 4 and rel.max() <= 8, (sr, w, np.percentile(rel, 99), rel.max())
        worst = max(worst, float(rel.max()))
        e0[:, 32 * w:32 * w + 32] = np.maximum(acc, 0)
    # enc1 (fp32, S_ENC1: one fmaf per term, taps 1, 2 for column 0 and 0, 1 for column 1, channels in order) on the model's own
    # enc0 output (fp32 values, ReLU): the split enc0 feeds it values the exact enc0 gives, to a few roundings
    cols = [e0[c].astype(np.float32) for c in range(3)]
    exact, scale = conv(w1, T["enc1.b"].astype(np.float64), [c.astype(np.float64) for c in cols], 2, 2)
    ex0, _ = conv(w0[:, cin + [nb - 1], :], T["enc0.b"].astype(np.float64),
                  [np.concatenate([x[c].astype(np.float64), nyq[c][None, :]]) for c in range(3)], 1, 3)
    exact_chain, _ = conv(w1, T["enc1.b"].astype(np.float64), [np.maximum(ex0[c], 0) for c in range(3)], 2, 2)
    for o in range(2):
        acc = np.broadcast_to(T["enc1.b"].astype(np.float64)[:, None], (64, nstr)).astype(np.float32)
        for t in range(3):
            c = 2 * o + t - 1
            if 0 <= c < 3:
                for k in range(128):
                    acc = (acc.astype(np.float64) + w1[:, k:k + 1, t] * cols[c][k][None, :].astype(np.float64)).astype(np.float32)
        rel = np.abs(acc - exact[o]) / scale[o] * 2.0 ** 24
        assert rel.max() <= 64, (sr, o, rel.max())                              # 257 sequential fp32 roundings
        assert float((np.abs(acc - exact_chain[o]) / scale[o]).max()) <= 2.0 ** -19
    assert worst > 0          # the model does round


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_no_instantiation_of_the_16_stream_kernel_spills(tmp_path):
    """compiled as tests/test_occupancy_contract.py compiles it: the product's flags, assembly for gfx950"""
    from cutter_vad_amd import _build
    out = tmp_path / "t16.s"
    flags = ["-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=8"]
    subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", *flags, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"\.name:\s*(\S+).*?\.sgpr_spill_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)", text, re.S):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    step16 = {k: v for k, v in kernels.items() if k.startswith("_Z16silero_v5_step16")}
    assert len(step16) == 9, sorted(kernels)
    for name, (sgpr_spills, vgpr_spills) in step16.items():
        assert vgpr_spills == 0, (name, vgpr_spills)
