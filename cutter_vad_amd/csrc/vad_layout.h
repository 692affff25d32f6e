// Shared host/device layout constants of the fused Silero kernels (gfx950).
//
// Geometry common to every model kernel:
//   * one workgroup = 4 wavefronts (256 threads) = one tile of MT = 32 streams;
//   * every contraction runs on v_mfma_f32_32x32x2_f32 with the WEIGHTS as the A operand
//     (32 output channels on the rows) and the ACTIVATIONS as the B operand (32 streams on
//     the columns), so the D tile has the stream on the lane (col = lane & 31) and 16 output
//     channels in the lane's registers: channel = 8*(r>>2) + 4*(lane>>5) + (r&3);
//   * activations live in LDS as "quads": row q holds channels 4q..4q+3 of all 32 streams
//     as 32 float4 (+1 float4 of padding, row stride QS = 33 float4 = 528 B, which makes both
//     the transposing ds_write_b128 of the loader and the row reads conflict-free);
//   * weights are pre-packed on the host into per-wave linear streams of 1 KiB blocks
//     (64 lanes x float4) in exactly the order the wave consumes them, so a wave's weight
//     traffic is one coalesced global_load_dwordx4 per 4 MFMAs, straight into VGPRs
//     (each wave owns different output channels, so LDS staging would not be shared).
//   One k-iteration j consumes quad 2j (lanes 0-31) and quad 2j+1 (lanes 32-63): MFMA
//   k-step i in 0..3 contracts channel 8j+i (lower half-wave) and 8j+4+i (upper half).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace vadk {

constexpr int MT = 32;        // streams per workgroup
constexpr int NWAVES = 4;     // wavefronts per workgroup
constexpr int NTHREADS = 256;
constexpr int QS = 33;        // float4 per LDS quad row
constexpr int BLK_F4 = 64;    // float4 per weight block (one per lane)
constexpr int BLK_FLOATS = 256;

// ---- Silero V5 (16 kHz branch) -------------------------------------------------------
namespace v5 {
// STFT as a 4-way folded DFT.  The stored basis is the windowed DFT w[n] cos/sin(2 pi k n / 256) (the packer
// verifies this to 2e-7 and takes w[n] from its k = 0 row), so with y = w * x and, for n = 1..63,
//   pe = y[n] + y[256-n] + y[128-n] + y[128+n]      po = y[n] + y[256-n] - y[128-n] - y[128+n]
//   qe = y[n] - y[256-n] - y[128-n] + y[128+n]      qo = y[n] - y[256-n] + y[128-n] - y[128+n]
//   re[k even] =  sum pe cos + y128 + a64 (-1)^(k/2)        re[k odd] =  sum po cos - y128
//   im[k even] = -sum qe sin                                im[k odd] = -sum qo sin - b64 (-1)^((k-1)/2)
// (y128 = y[128], a64 = y[64] + y[192], b64 = y[64] - y[192]): every contraction has K = 64 instead of 256.
// Wave w owns 32 bins: w = 0: k = 0,2..62   w = 1: k = 64..126   w = 2: k = 1,3..63   w = 3: k = 65..127,
// so |STFT| channel ch = 32 w + r holds bin  (w < 2 ? 64 w + 2 r : 64 (w - 2) + 2 r + 1); enc0's input
// channels are permuted accordingly by the packer.  Bin 128 (even) is an alternating sum on the VALU.
// weight-stream sections, in blocks, per wave
constexpr int STFT_BLOCKS = 16;            // 8 k-iterations x {cos, -sin}
constexpr int NYQ_BLOCKS = 1;              // shared table: floats 0..255 = w[n] (the Hann window of the stored basis)
constexpr int ENC0_BLOCKS = 4 + 16 * 5 + 2;  // bias, 16 k-iterations x 5 Toom-3 points, Nyquist channel (points 0,1,-1,2 | inf)
constexpr int ENC1_BLOCKS = 4 + 2 * 16;
constexpr int ENC2_BLOCKS = 4 + 2 * 8;     // packed for waves 0,1; waves 2,3 read the second K half of the same streams
constexpr int ENC3_BLOCKS = 4 + 8;
constexpr int LSTM_BLOCKS = 16 + 64 + 64 + 4;  // bias(4 gates), W_ih, W_hh, head weights
enum Section { S_STFT = 0, S_NYQ, S_ENC0, S_ENC1, S_ENC2, S_ENC3, S_LSTM, S_HEADB, S_LSTM_X3, S_ENC0_X3, S_ENC1_X3, S_COUNT };  // S_HEADB: 1 block, float 0 = head bias
// S_LSTM_X3 (16-stream kernel only, pack_silero_v5_t16): the wave's W_ih and W_hh rows once more, as three exact bf16 pieces
// w = w1 + w2 + w3 (w1 = hi16(w), w2 = hi16(w - w1), w3 = w - w1 - w2) for v_mfma_f32_16x16x32_bf16.  Per half (W_ih, then W_hh):
// 4 K-steps s x 8 row tiles (gate q, rt: tile 2 q + rt) x 3 pieces, block (s * 8 + tile) * 3 + piece.  A block is the tile's A
// fragment: lane (row l & 15, kq = l >> 4) holds 8 bf16, elements 0..3 = K 32 s + 4 kq + 0..3 and elements 4..7 = K 32 s + 16 +
// 4 kq + 0..3 - the two activation quads 8 s + kq and 8 s + 4 + kq that the lane reads as it does for the fp32 form.
constexpr int LSTM_X3_HALF_BLOCKS = 4 * 8 * 3;
// S_ENC0_X3 (16-stream kernel only): the SECOND weight stream (PackedWeights::data_x, StepParams::wstream_x; its sect entries are
// block offsets into it) - the first stream keeps every byte it had.  encoder.0 as a DIRECT 3-tap convolution, out(o) = sum_tap
// W[tap] x[o + tap - 1] (x[-1] = x[3] = 0).  Wave w = output channels 32 w + 16 rt + r: ENC0_X3_F32_BLOCKS fp32 blocks in the D
// layout of a row tile (vector_block16) - the bias (rt 0, 1), then the Nyquist input channel's taps 0, 1, 2 (rt 0, 1 each) - then
// one unit of three blocks per (K-step s < 4 (8 kHz: 2), tap, rt): block ENC0_X3_F32_BLOCKS + 3 ((s * 3 + tap) * 2 + rt) + piece,
// the pieces of the tile's A fragment as in S_LSTM_X3 (lane (row l & 15, kq), element e = K 32 s + 16 (e >> 2) + 4 kq + (e & 3)),
// piece 0 first; input channel K = the STFT's channel order (bin_of_channel_fold3 / bin_of_channel_8k).
constexpr int ENC0_X3_F32_BLOCKS = 2 + 3 * 2;
// S_ENC1_X3 (16-stream kernel only): the THIRD weight stream (PackedWeights::data_y, StepParams::wstream_y; sect entries are block
// offsets into it) - the first two streams keep every byte they had, S_ENC1 stays in the first, unread by the 16-stream kernel.
// encoder.1 (128 -> 64 channels, k3 s2 p1, 3 -> 2 columns) as a direct convolution on the bf16 split: wave w = output channels
// 16 w + r, ONE row tile, for both output columns.  ENC1_X3_F32_BLOCKS fp32 block (the bias, vector_block16), then one unit of three
// blocks per (K-step s < 4, tap): block ENC1_X3_F32_BLOCKS + 3 (s * 3 + tap) + piece, the tile's A fragment as in S_LSTM_X3 over
// the input channels 32 s .. 32 s + 31 in their natural order (enc0's output channel = the K index of its activation planes).
constexpr int ENC1_X3_F32_BLOCKS = 1;
constexpr int ENC1_X3_BLOCKS = ENC1_X3_F32_BLOCKS + 3 * 4 * 3;
// The FOURTH block range (16-stream kernel only; PackedWeights::data_z): encoder.2 and encoder.3 on the bf16 split.  It has no sect
// entry, no host vector among the first three and no field of StepParams: the engine uploads it BEHIND the third stream, in the same
// allocation (StepParams::wstream_y_bytes covers both), and wave w finds its ENC23_X3_BLOCKS blocks at block
// 4 * ENC1_X3_BLOCKS + w * ENC23_X3_BLOCKS of that buffer.  The first three streams keep every byte; S_ENC2 / S_ENC3 stay in the first,
// unread by the 16-stream kernels (the 32-stream packing and tests/kernel_model.py have their own).
//   encoder.2 (64 -> 64 channels, k3 s2 p1, 2 -> 1 column; tap 0 meets the padding only): wave w = output channels 16 w + r, ONE row
//   tile over the whole K = 128 - one fp32 block (the bias, vector_block16), then four units of three blocks, the tile's A fragment as
//   in S_LSTM_X3: (column 0, K-step 0), (column 0, K-step 1), (column 1, K-step 0), (column 1, K-step 1), column c on tap 1 + c;
//   encoder.3 (64 -> 128 channels, centre tap): wave w = channels 32 w + 16 rt + r - two fp32 blocks (the bias of rt 0, 1), then four
//   units (K-step s, rt): block 2 + 3 (2 s + rt) + piece of its part.
// Input channels in their natural order (enc1's and enc2's output channel = the K index of their activation planes).
constexpr int ENC2_X3_BLOCKS = 1 + 4 * 3;
constexpr int ENC3_X3_BLOCKS = 2 + 4 * 3;
constexpr int ENC23_X3_BLOCKS = ENC2_X3_BLOCKS + ENC3_X3_BLOCKS;
// The FIFTH block range (16-stream kernel, 16 kHz model only; PackedWeights::data_d): the odd-bin row tile of the STFT on the bf16
// split.  Like the fourth it has no sect entry and no field of StepParams: the engine uploads it behind the fourth, in the third
// stream's allocation, and wave w finds its DFT_X3_BLOCKS blocks at block 4 * ENC1_X3_BLOCKS + 4 * ENC23_X3_BLOCKS + w * DFT_X3_BLOCKS
// of that buffer.  S_STFT stays whole in the first stream; its odd-tile blocks (k-iterations 0..3) are no longer read by this kernel.
//   Wave w = the 16 odd bins bin_of_channel_fold3(32 w + r): four units of three blocks, unit 2 part + s - part 0 the cos rows
//   (contracted with po), part 1 the -sin rows (with qo), K-step s = the folded samples n = 32 s .. 32 s + 31 - each the tile's A
//   fragment as in S_LSTM_X3 (lane (row l & 15, kq), element e = n 32 s + 16 (e >> 2) + 4 kq + (e & 3)), the very fp32 table values of
//   S_STFT cut into three exact pieces; n = 0 is the zero slot it is there (the loader writes 0 into po[0] and qo[0]).
constexpr int DFT_X3_BLOCKS = 4 * 3;
__host__ __device__ constexpr int bin_of_channel(int ch) {
    return (ch >> 5) < 2 ? 64 * (ch >> 5) + 2 * (ch & 31) : 64 * ((ch >> 5) - 2) + 2 * (ch & 31) + 1;
}
// Channel order of the kernels whose STFT folds the EVEN bins once more (silero_v5.hip's 16 kHz instantiation, silero_v4_t16.hip):
// wave w owns the channels 32 w .. 32 w + 31 as two 16-row tiles of v_mfma_f32_16x16x4_f32.  Row tile 0: the odd bins
// 2 (16 w + r) + 1 against the 4-way folded operands po | qo (K = 64).  Row tile 1: even bins k = 2 m, whose operands fold again
// about n = 32 - cos(2 pi m (64 - n) / 128) = (-1)^m cos(2 pi m n / 128), the sine with the opposite sign - into K = 32, in two
// classes by the parity of m: waves 0, 1: k = 4 (16 w + r) + 2 (m odd: pe[n] - pe[64 - n] | qe[n] + qe[64 - n]), waves 2, 3:
// k = 4 (16 (w - 2) + r) (m even: pe[n] + pe[64 - n] | qe[n] - qe[64 - n]; bin 0 = wave 2, tile 1, row 0).  Per column a wave
// contracts 16 x (64 + 64) + 16 x (32 + 32) instead of 32 x (64 + 64): three quarters of the 4-way fold's MFMAs, the same on
// every wave.
//   loader (v5, 16 kHz): column c: po -> rows 64c + q, qo -> 64c + 16 + q (q = 0..15, n = 4q..4q+3), then n = 4q'..4q'+3, q' = 0..7:
//   pe+ -> 64c + 32 + q', pe- -> 64c + 40 + q', qe- -> 64c + 48 + q', qe+ -> 64c + 56 + q'; slot n = 0 of pe+ holds pe[32], of qe+ qe[32]
__host__ __device__ constexpr int bin_of_channel_fold3(int ch) {
    return (ch & 16) == 0 ? 2 * (16 * (ch >> 5) + (ch & 15)) + 1
                          : ((ch >> 5) < 2 ? 4 * (16 * (ch >> 5) + (ch & 15)) + 2 : 4 * (16 * ((ch >> 5) - 2) + (ch & 15)));
}
constexpr int ROW_FOLD_SINK = 192;         // 32 rows past the three columns: where the loader lanes q >= 8 drop their duplicate quads
// The graph's 8 kHz sub-model (If_0 else-branch) is the same dataflow at half the front-end size: 256-sample
// frames, window N = 128, hop 64 -> three columns at 0, 64, 128; 65 bins; 4-way fold with n = 1..31 (K = 32), unpaired samples
// n = 0, 32, 64; the 64 complex bins are two 32-row tiles - wave 0: even bins 2 r, wave 1: odd bins 2 r + 1 - and bin 64
// (even) is the alternating sum on the VALU; encoder.0 has 65 input channels.
//   loader : column c: pe -> rows 32c + q, po -> 32c + 8 + q, qe -> 32c + 16 + q, qo -> 32c + 24 + q   (q = 0..7, n = 4q..4q+3)
//   |STFT| : Toom-3 planes rows 16p + ch/4 (p = 0..4), rows 80/81 and 82/83 for |X64| as ROW_NYQ below
__host__ __device__ constexpr int bin_of_channel_8k(int ch) { return 2 * (ch & 31) + (ch >> 5); }
constexpr int ROW_NYQ_8K = 80;
constexpr int FRAME_8K = 256;

// LDS, in quad rows.  One activation region X, reused by every layer:
//   loader : column c: pe -> rows 64c + q, po -> 64c + 16 + q, qe -> 64c + 32 + q, qo -> 64c + 48 + q   (q = 0..15, n = 4q..4q+3)
//   |STFT| : the three columns x0, x1, x2 of a channel enter enc0 as the Toom-3 evaluations of x0 + x1 z + x2 z^2 at
//            z = 0, 1, -1, 2, inf: rows 32p + ch/4 (p = 0..4); rows 160/161 = (the same for |X128|, points 0,1,-1,2) / 0,
//            rows 162/163 = (|X128| at inf, 0, 0, 0) / 0
//   enc0   : rows 164 + 32c + ch/4         enc1 : rows 16c + ch/4
//   enc2   : rows 164 + ch/4 (two K halves) enc3 : rows ch/4 (LSTM input)
// enc0 as a Toom-3 product: out(c) = sum_tap w[tap] x[c + tap - 1] are the coefficients y1, y2, y3 of
// (w2 + w1 z + w0 z^2)(x0 + x1 z + x2 z^2); five point-wise products (one MFMA contraction over the channels each)
// replace the seven (tap, column) contractions: y0 = P(0), y4 = P(inf), y2 = (P(1) + P(-1))/2 - y0 - y4,
// b = (P(1) - P(-1))/2, y3 = ((P(2) - y0 - 4 y2 - 16 y4)/2 - b)/3, y1 = b - y3.  fp32 error 1.5-2.5 x that of the direct
// sums on real spectra (tools note in DESIGN.md), 28 % fewer MFMAs in the kernel's largest phase.
constexpr int ROWS_X = 260;
constexpr int ROW_E = 164;                 // first row of the upper part (enc0 / enc2 outputs)
constexpr int ROW_NYQ = 160;
constexpr int ROWS_H = 32;                 // h_{t-1}
constexpr int LDS_F4 = (ROWS_X + ROWS_H) * QS + 32 + 24 + 72 + 16 + 192 + 128;  // + head partials [4][32], |X128| [3][32], fold corrections [3][3][32], write sink [64], state machines [32] x 96 B, gate biases [4 waves][4 gates][32 units]
constexpr int LSTM_BIAS_BLOCK = 16 + 64 + 64 + 4;   // block of a wave's LSTM section that holds its gate biases compact: floats [gate][unit]
constexpr int LDS_BYTES = LDS_F4 * 16;
}  // namespace v5

// ---- Silero V4 (16 kHz branch) -------------------------------------------------------
// One launch per frame, two LDS layouts in sequence (the 258 x 8 first-layer input of 32 streams does not fit one CU's
// LDS next to the STFT operands, so the magnitudes wait in registers until those are dead):
//   STFT part : gate/int16 ingest, reflect pad 96+96, fold, 8-column STFT (MFMA), |.| -> registers
//   tail      : log-spectrum + adaptive normalisation, 4 separable blocks, 2 x LSTM(64), head, state machine
namespace v4 {
enum Section {
    S_STFT = 0, S_NYQ,            // as V5 (the DFT basis is identical): folded-DFT tables, window table
    S_DW0,                        // first-layer depthwise taps+bias per channel quad (VALU table)
    S_L0,                         // first layer: pw(relu(dw(x1))) + proj(x1), 16 outputs (rows 16..31 of the tile are zero)
    S_S0, S_L1, S_S1, S_L2, S_S2, S_L3, S_S3, S_LSTM0, S_LSTM1, S_HEADB, S_COUNT
};
// Channel order of the 16-STREAM kernel's STFT (silero_v4_t16.hip; the 32-stream kernel keeps v5::bin_of_channel): the order of
// the once-more-folded DFT, v5::bin_of_channel_fold3
__host__ __device__ constexpr int bin_of_channel_t16(int ch) { return v5::bin_of_channel_fold3(ch); }
constexpr int MAG_Q = 33;                      // quads per STFT column: 128 bins + Nyquist (+3 pad channels)
constexpr int MAG_ROWS = 8 * MAG_Q;            // 264 rows per tile, row = 33 t + q
// STFT part, LDS: reflect-padded frame [32][704] f32 + the 4-way fold of two columns (2 x 64 quad rows: pe, po, qe, qo as in
// V5) + window table w[256] + |X0|, |X128| of the two columns [2][2][32] + fold corrections [2][3][32].
// The two REAL bins (k = 0, k = 128) are summed in float64 from the samples: they are the graph's ill-conditioned
// inputs (log(1 + |X| 2^20) of a real sum that may cancel to ~1e-6 of its terms; a complex bin needs re AND im to
// cancel, which is ~100 x rarer) - DESIGN.md §3 "Numerics".
constexpr int K1_XP_QUADS = 176;               // reflect-padded frame: 704 samples per stream
constexpr int K1_XS_F4 = 32 * K1_XP_QUADS;
constexpr int K1_UV_ROWS = 128;
constexpr int K1_WT_F4 = 64;                   // w[n] as 64 quads, 256-byte aligned (the readers XOR-swizzle the quad index)
constexpr int K1_LDS_F4 = K1_XS_F4 + K1_UV_ROWS * QS + K1_WT_F4 + 32 + 48;
static_assert((K1_XS_F4 + K1_UV_ROWS * QS) % 16 == 0, "window table must start on a 16-quad boundary");
// tail, LDS rows
constexpr int R_A16 = MAG_ROWS;                // first-layer output: 264 + 4 t' + quad
constexpr int K2_ROWS = MAG_ROWS + 16;
constexpr int R_Y0 = 0, R_Y1 = 16, R_Y2 = 48, R_Y3 = 64, R_Y4 = 80, R_Y5 = 88, R_Y6 = 104;
constexpr int R_H0 = 120, R_H1 = 136, R_H0N = 152;   // h_{t-1} of LSTM layers 0 / 1, layer 0's new h
constexpr int K2_MISC_FLOATS = 32 + 8 * 32 + 256;  // mm[32], colmean[8][32], head partials [2 steps][4 waves][32]
// 8 kHz sub-model: two columns survive the third stride conv (stride 1); rows re-used from dead activations
constexpr int R8_Y4 = 80, R8_Y5 = 0, R8_Y6 = 32, R_H1N = 96;
constexpr int K2_LDS_F4 = K2_ROWS * QS + K2_MISC_FLOATS / 4 + 256;   // + partial log sums [4 waves][8 columns][32 streams]
constexpr int V4_SM_F4 = K1_LDS_F4 > K2_LDS_F4 ? K1_LDS_F4 : K2_LDS_F4;   // the tile's 32 state machines (96 B each) sit past both layouts
constexpr int V4_LDS_F4 = V4_SM_F4 + 192;
static_assert(V4_LDS_F4 * 16 <= 160 * 1024, "V4 LDS layout exceeds one CU");
}  // namespace v4

// per-slot hysteresis state (VADProcessor fields, core/silero_model.py:596-639), 96 bytes.
// Thresholds are doubles: the reference compares Python floats (float(np.float32 p) >= 0.7).
struct SmSlot {
    double start_prob, end_prob, start_ratio, end_ratio;
    int32_t start_count, end_count;
    int32_t active, n_start, n_end;
    int32_t start_len;       // len(recent_start_frames), deque maxlen 20
    uint32_t start_hist;     // its contents, newest in bit 0
    int32_t end_len;         // len(recent_end_frames), deque maxlen 100
    uint32_t end_hist[4];    // newest in bit 0 of word 0
    int32_t buffered;        // len(voice_buffer) in frames
    int32_t seg_frames;      // frames in current_voice_data (-1 = None)
    int32_t pad[2];
};
static_assert(sizeof(SmSlot) == 96, "SmSlot layout");

struct StepParams {
    const float *wstream;          // packed weight streams
    uint32_t wstream_bytes;
    uint32_t sect[NWAVES][16];     // block offset of each section, per wave
    // (the second and third streams' sizes sit where the compiler would pad: the struct is a by-value kernel argument and keeps the
    //  size it had with one stream.  16 bytes more put silero_v4_step16's last argument into a seventh 64-byte line of the kernarg
    //  segment: + 0.3 us per step of the V4 + V5 mix, measured - profiles/r08_planes_other_configs.jsonl)
    uint32_t wstream_y_bytes;
    float *state;                  // [max_streams][256]
    SmSlot *sm;                    // [max_streams]
    const int32_t *slots;          // [n] or nullptr (identity)
    const void *frames;            // [n][T][512]
    float *probs;                  // [n][T]
    uint8_t *events;               // [n][T] or nullptr
    int32_t *seg_frames;           // [n] or nullptr (last END of the call)
    int32_t n;
    int32_t T;                     // frames per stream in this call
    int32_t fmt;                   // vad_frame_format
    float thresh;                  // denoise gate, < 0 = off
    int32_t variant;               // 1 = the graph's 8 kHz sub-model (pack_weights.h): V4 two LSTM steps per frame, V5 256-sample frames
    uint32_t wstream_x_bytes;
    const float *wstream_x;        // second weight stream (PackedWeights::data_x), or nullptr
    const float *wstream_y;        // third weight stream (PackedWeights::data_y), or nullptr
#ifdef VADK_STAMPS
    unsigned long long *stamps;    // diagnostic builds only (tools/kbench.cpp): [block][wave][16] s_memtime stamps
#endif
};
#ifndef VADK_STAMPS
static_assert(sizeof(StepParams) == 368, "StepParams keeps its size (see above)");
#endif

// whole recordings, framed by the kernel's loader (csrc/silero_v5_t16.hip: silero_v5_scan16; vad_scan).  A launch reads one
// contiguous block of audio and a table of work items, one per stream, sorted by nframes (descending): frame t of an item are
// the samples from 4 (quad0 + t hopq) on, its results go to entry out0 + t of the call's probs / events / seg arrays.
struct ScanItem {
    int32_t slot;
    uint32_t quad0;           // sample_offset / 4; two-channel blocks: | the stream's channel mode << SCAN_MODE_SHIFT
    int32_t nframes;
    uint32_t out0;            // index of the recording's frame 0 in the outputs (CSR)
};
static_assert(sizeof(ScanItem) == 16, "ScanItem layout");
// Interleaved two-channel blocks (vad_scan_channels; silero_v5_stereo16): positions count sample frames (one sample of every
// channel), and each item says what its stream hears - the left channel, the right one, or the float32 mean of the decoded pair
// (AudioUtils.convert_to_mono).  A block is under 2 GiB, so quad0 < 2^29 and its two top bits are free; a mono item, and the left
// channel, encode as quad0 itself.
constexpr int SCAN_MODE_SHIFT = 30;
enum : uint32_t { SCAN_LEFT = 0, SCAN_RIGHT = 1, SCAN_MIX = 2 };
// a launch's arguments next to StepParams (which keeps its size): StepParams.n = items, .T = frames of the window, .frames = the
// audio block; probs / events / seg_frames = the CSR arrays (seg_frames: one entry per FRAME here)
struct ScanArgs {
    uint32_t audio_bytes;     // the buffer descriptor's range: the whole block; loads past it return 0
    uint32_t hopq;            // hop / 4
    int32_t t0;               // the launch covers frames t0 .. t0 + T - 1 of every item
    int32_t channels;         // interleaved channels of the block: 2, or 0 / 1 = mono
};

// finished segments cut out of a scanned block (csrc/scan_cut.hip: vadk_scan_cut, vadk_scan_cut_stereo; vad_scan_cut).  The unit is the loader's quad:
// output quad oq of a segment comes from input quad quad_in + (oq >> frame_shift) * hopq + (oq & (frame / 4 - 1)) - the segment's
// frames back to back (VAD_CUT_FRAMES) - or from quad_in + oq (VAD_CUT_RANGE: frame_shift = 31, hopq unused), and goes to quad
// quad_out + oq of the output.  A workgroup of CUT_THREADS threads serves CUT_WG_QUADS consecutive output quads of ONE segment in
// CUT_PASSES passes of one quad per thread; the host lists the workgroups (CutWork), so no thread searches the segment table.
constexpr int CUT_THREADS = 256;
constexpr int CUT_PASSES = 4;
constexpr int CUT_WG_QUADS = CUT_THREADS * CUT_PASSES;
struct CutSeg {
    uint32_t quad_in;         // (sample_offset + first_frame * hop) / 4 | the channel mode << SCAN_MODE_SHIFT, as ScanItem::quad0
    uint32_t nquads;          // output quads of the segment, < 2^31
    uint64_t quad_out;        // out_sample / 4
};
static_assert(sizeof(CutSeg) == 16, "CutSeg layout");
struct CutWork {
    uint32_t seg;             // index into the segment table
    uint32_t quad0;           // first output quad of this workgroup's share, a multiple of CUT_WG_QUADS
};
static_assert(sizeof(CutWork) == 8, "CutWork layout");
struct CutArgs {
    const void *audio;        // the block, in its wire format
    void *out;                // int16 or float32 samples
    const CutSeg *segs;
    const CutWork *work;      // [nwork]: one entry per workgroup
    uint32_t audio_bytes;     // the buffer descriptor's range
    uint32_t nwork;
    uint32_t hopq;            // hop / 4
    uint32_t frame_shift;     // log2(frame / 4), or 31: the sample range once
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
    int32_t out_fmt;          // 0 = int16 PCM, 1 = float32
    float thresh;             // denoise gate, < 0 = off
};

// normalised, padded waveform windows (csrc/audio_batch.hip: vadk_audio_batch; vad_scan_audio_batch).  Window w of T = 4 tq samples
// shows samples 4 quad0 .. 4 quad0 + nsamples - 1 of segment seg's range once (a CutSeg of it: quad_in + the mode bits; quad_out is
// not read); the cells behind nsamples are pad cells.  A workgroup of CUT_THREADS threads serves CUT_WG_QUADS consecutive quads of
// ONE window in CUT_PASSES passes; the host lists the workgroups (AudioWork), so no thread searches a table.
struct AudioWin {
    uint32_t seg;             // index into the segment table, and into shift / scale when per_seg
    uint32_t quad0;           // sample0 / 4, within the segment
    uint32_t nsamples;        // 0 .. T
    uint32_t reserved;
};
static_assert(sizeof(AudioWin) == 16, "AudioWin layout");
struct AudioWork {
    uint32_t window;
    uint32_t quad0;           // first quad of this workgroup's share of the window, a multiple of CUT_WG_QUADS, < tq
};
static_assert(sizeof(AudioWork) == 8, "AudioWork layout");
struct AudioBatchArgs {
    const void *audio;        // the block, in its wire format
    void *out;                // [nw][T] float32 / float16 / bfloat16
    uint8_t *mask;            // [nw][T] or nullptr
    const CutSeg *segs;
    const AudioWin *win;      // [nw]
    const AudioWork *work;    // [nwork]
    const float *shift;       // [1 or segments]
    const float *scale;
    uint32_t audio_bytes;     // the buffer descriptor's range
    uint32_t nwork;
    uint32_t tq;              // T / 4
    uint32_t per_seg;         // 1: shift / scale have an entry per segment, 0: one
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
    int32_t dtype, pad_mode;  // VAD_BATCH_*
    float pad_value;
    float thresh;             // denoise gate, < 0 = off
};
static_assert(sizeof(AudioBatchArgs) == 104, "AudioBatchArgs layout");

// log-mel features of finished segments (csrc/scan_mel.hip: vadk_seg_mel; vad_scan_mel).  A workgroup of MEL_THREADS threads
// serves MEL_TILE consecutive analysis frames of ONE segment; the host lists the workgroups (MelWork) next to the segments, which
// are CutSeg of the sample range once with quad_out = the segment's first ROW of the output.  Both matrix products run on
// v_mfma_f32_16x16x4_f32 and take one operand from a stream the host packed into fragment order (lane l of a 16 x 16 x 4 step
// holds row / column l & 15 and k = l >> 4), one float4 per lane and block of 64 lanes:
//   operator  [bin tile bt][pair of k-steps sp][lane]  {re, im}[n = 8 sp + kq][bin], {re, im}[n = 8 sp + 4 + kq][bin]
//   filters   [mel tile mt][four k-steps sp][lane]     filters[mel][k = 16 sp + 4 t + kq], t = 0 .. 3
// with bin = 16 bt + (l & 15), mel = 16 mt + (l & 15), kq = l >> 4; bins and mels past the caller's counts are zeros of the pack.
constexpr int MEL_THREADS = 256;
constexpr int MEL_TILE = 16;
struct MelWork {
    uint32_t seg;             // index into the segment table
    uint32_t frame0;          // first analysis frame of this workgroup's tile, a multiple of MEL_TILE
};
static_assert(sizeof(MelWork) == 8, "MelWork layout");
__host__ __device__ inline uint32_t mel_pad16(uint32_t v) { return (v + 15u) & ~15u; }
// float index of op_re[n][bin] in the packed operator (op_im: + 1)
__host__ __device__ inline size_t mel_op_index(uint32_t n, uint32_t bin, uint32_t n_fft) {
    const uint32_t lane = ((n & 3u) << 4) | (bin & 15u);
    return (((size_t)(bin >> 4) * (n_fft >> 3) + (n >> 3)) * 64u + lane) * 4u + ((n >> 2) & 1u) * 2u;
}
// float index of filters[mel][k] in the packed filters
__host__ __device__ inline size_t mel_filter_index(uint32_t mel, uint32_t k, uint32_t bins_pad) {
    const uint32_t lane = ((k & 3u) << 4) | (mel & 15u);
    return (((size_t)(mel >> 4) * (bins_pad >> 4) + (k >> 4)) * 64u + lane) * 4u + ((k >> 2) & 3u);
}
// The tile's samples in LDS: local sample i of the tile's span lies at float i + skew * (i / hop) with skew = (4 - hop) mod 64, so
// that frame j's sample n is j * (hop + skew) + n + skew * (n / hop) and the 16 frames x 4 k of one B fragment (stride hop + skew =
// 4 mod 64 between frames, 1 between k) fall into 64 different banks, whatever the hop; behind them P as [bin][MEL_TILE]
__host__ __device__ inline uint32_t mel_skew(uint32_t hop) { return (4u - (hop & 63u)) & 63u; }
__host__ __device__ inline uint32_t mel_lds_span_floats(uint32_t n_fft, uint32_t hop) {
    const uint32_t span = (MEL_TILE - 1) * hop + n_fft;
    return ((span + hop - 1) / hop) * (hop + mel_skew(hop));
}
struct MelArgs {
    const void *audio;        // the block, in its wire format
    float *out;               // [rows][n_mels]
    const CutSeg *segs;       // quad_out: the segment's first row
    const MelWork *work;      // [nwork]: one entry per workgroup
    const float *op;          // the packed operator: 2 n_fft bins_pad floats
    const float *filters;     // the packed filters: mels_pad bins_pad floats
    uint32_t audio_bytes;     // the buffer descriptor's range
    uint32_t nwork;
    uint32_t n_fft, hop;      // of the analysis (vad_mel), not the scan's
    uint32_t bins_pad;        // n_bins in whole tiles of 16
    uint32_t n_mels;
    int32_t pad, log;         // VAD_MEL_PAD_*, VAD_MEL_*
    float floor;
    float thresh;             // denoise gate, < 0 = off
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
};
static_assert(sizeof(MelArgs) == 96, "MelArgs layout");

// finished segments of a rate block as one continuous signal at 16 kHz (csrc/scan_resample_cut.hip: vadk_resample_cut;
// vad_scan_resample_cut).  L / M = 16000 / sr_in; A = 16 M / L input samples advance under 16 outputs.  A workgroup of RSC_THREADS
// threads serves RSC_WG_SAMPLES consecutive outputs of ONE segment - RSC_WG_SAMPLES / 256 tiles of 16 row-blocks x 16 outputs, two per
// wave; the host lists the workgroups as CutWork (quad0: the first OUTPUT quad) next to the segments, which are CutSeg with nquads =
// S16 / 4, and the segments' INPUT quads (inq).  Output o of row-block r of a tile is
//     D[o][r] = sum over n < K of T[o][n] * xs[A r + n],   T[o][n] = h[o M - (n - n0) L + C]  (0 outside the taps)
// where xs starts n0 samples ahead of the tile's first input sample: n0 = C / L rounded up to a multiple of 4 (so that the span
// starts on a quad), K = n0 + (15 M + C) / L + 1 in whole k-steps of 16.  T is the A operand of v_mfma_f32_16x16x4_f32, packed by the
// host in fragment order - one float4 per lane and four k-steps: [n >> 4][lane = (n & 3) << 4 | o]{n >> 2 & 3}.
// LDS: local sample j of the span at float j + RSC_SKEW * (j / A), so that row-block r's sample n is r (A + 4) + n + 4 (n / A) and
// the 16 row-blocks x 4 k of a B fragment (stride A + 4 = 4 * odd between row-blocks, 1 between k) fall into 64 different banks.
constexpr int RSC_THREADS = 256;
constexpr int RSC_WG_SAMPLES = 2048;
constexpr uint32_t RSC_SKEW = 4;
__host__ __device__ inline uint32_t rsc_L(int32_t sr_in) { return sr_in == 48000 ? 1u : 2u; }
__host__ __device__ inline uint32_t rsc_M(int32_t sr_in) { return sr_in == 8000 ? 1u : 3u; }
__host__ __device__ inline uint32_t rsc_A(int32_t sr_in) { return 16u * rsc_M(sr_in) / rsc_L(sr_in); }
__host__ __device__ inline uint32_t rsc_n0(uint32_t ntaps, uint32_t L) { return (((ntaps - 1u) / 2u) / L + 3u) & ~3u; }
__host__ __device__ inline uint32_t rsc_K(uint32_t ntaps, uint32_t L, uint32_t M) {
    return (rsc_n0(ntaps, L) + (15u * M + (ntaps - 1u) / 2u) / L + 1u + 15u) & ~15u;
}
// index into the taps of T[o][n], in [0, ntaps) or outside
__host__ __device__ inline int32_t rsc_tap(uint32_t o, uint32_t n, uint32_t ntaps, uint32_t L, uint32_t M) {
    return (int32_t)(o * M) - ((int32_t)n - (int32_t)rsc_n0(ntaps, L)) * (int32_t)L + (int32_t)((ntaps - 1u) / 2u);
}
// float index of T[o][n] in the packed operator
__host__ __device__ inline size_t rsc_pack_index(uint32_t o, uint32_t n) {
    return (((size_t)(n >> 4) * 64u) + (((n & 3u) << 4) | o)) * 4u + ((n >> 2) & 3u);
}
// floats of a workgroup's span in LDS
__host__ __device__ inline uint32_t rsc_lds_floats(uint32_t A, uint32_t K) {
    const uint32_t span = (RSC_WG_SAMPLES / 16) * A + K;
    return span + RSC_SKEW * ((span + A - 1u) / A);
}
struct ResampleCutArgs {
    const void *audio;        // the rate block, in its wire format
    void *out;                // int16 or float32 samples at 16 kHz
    const CutSeg *segs;       // quad_in: the segment's first input quad | mode; nquads: S16 / 4; quad_out: out_sample / 4
    const uint32_t *inq;      // [segments]: S_in / 4
    const CutWork *work;      // [nwork]: one entry per workgroup, quad0 a multiple of RSC_WG_SAMPLES / 4
    const float *gains;       // [segments], or nullptr
    const float *op;          // the packed T: 16 K floats
    uint32_t audio_bytes;     // of the block
    uint32_t nwork;
    uint32_t ksteps;          // K / 16
    uint32_t n0;
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
    int32_t out_fmt;          // 0 = int16 PCM, 1 = float32
    int32_t sr_in;            // 8000, 24000 or 48000
};
static_assert(sizeof(ResampleCutArgs) == 88, "ResampleCutArgs layout");

// whole recordings of a block at ANY rational rate as one continuous signal each at the engine's rate (csrc/scan_convert.hip:
// vadk_convert; vad_convert, vad_scan_convert_segments).  L / M = engine rate / sr_in in lowest terms.  16 outputs do not advance a
// whole number of inputs in general; a PERIOD of P = lcm(L, 16) outputs does: PI = P M / L inputs (441 for the 44.1 kHz family).  A
// period has NT = P / 16 row-tiles, each with a 16 x K operator and a first-input offset of its own: output 16 r + o of period p is
//     D_r[o][p] = sum over n < K of T_r[o][n] * x[p PI + base_r + n],   T_r[o][n] = h[(16 r + o) M - (base_r + n) L + C]  (0 outside)
// with base_r = floor((16 r M - C) / L), the first input the tile's first output reads, and K = (15 M + N - 1) / L + 2 in whole
// k-steps of 16 - the same for every tile.  T_r is the A operand of v_mfma_f32_16x16x4_f32, the samples are the B operand, column =
// period; the host packs the tiles back to back, each in the fragment order of the resample cut's T: [r][n >> 4][lane = (n & 3) << 4 |
// o]{n >> 2 & 3}.  A workgroup of CV_THREADS threads serves `nper` consecutive periods of ONE item (ConvertWork::run counts such
// runs): cv_nper() asks for CV_WG_SAMPLES outputs in whole column groups of 16 periods and cuts that to what CV_LDS_FLOATS hold.
// LDS: the run's input span starts `shift` samples ahead of its first period - shift = lead .. lead + 3, lead = ceil(C / L), so that
// the span starts on a quad of the item - and local sample j lies at float j + skew (j / PI) with skew = (4 - PI) mod 64: column p's
// sample c = shift + base_r + n is at p (PI + skew) + c + skew (c / PI), and the 16 periods x 4 k of a B fragment (stride PI + skew =
// 4 mod 64 between periods, 1 between k) fall into 64 different banks, except in the one k-step per PI samples that crosses a period's
// end, where two of a lane group's four k move by skew.
constexpr int CV_THREADS = 256;
constexpr uint32_t CV_WG_SAMPLES = 2048;
constexpr uint32_t CV_LDS_FLOATS = 16384;   // 64 KiB
__host__ __device__ inline uint32_t cv_gcd(uint32_t a, uint32_t b) {
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}
__host__ __device__ inline uint32_t cv_P(uint32_t L) { return L * 16u / cv_gcd(L, 16u); }
__host__ __device__ inline uint32_t cv_PI(uint32_t L, uint32_t M) { return 16u / cv_gcd(L, 16u) * M; }
__host__ __device__ inline uint32_t cv_K(uint32_t ntaps, uint32_t L, uint32_t M) { return ((15u * M + ntaps - 1u) / L + 2u + 15u) & ~15u; }
__host__ __device__ inline uint32_t cv_lead(uint32_t ntaps, uint32_t L) { return ((ntaps - 1u) / 2u + L - 1u) / L; }
// first input of row-tile r, relative to its period's first input (floor division: negative for the first tiles)
__host__ __device__ inline int32_t cv_base(uint32_t r, uint32_t ntaps, uint32_t L, uint32_t M) {
    const int32_t v = (int32_t)(16u * r * M) - (int32_t)((ntaps - 1u) / 2u), l = (int32_t)L;
    return v >= 0 ? v / l : -((-v + l - 1) / l);
}
// index into the taps of T_r[o][n], in [0, ntaps) or outside
__host__ __device__ inline int64_t cv_tap(uint32_t r, uint32_t o, uint32_t n, uint32_t ntaps, uint32_t L, uint32_t M) {
    return (int64_t)((16u * r + o) * M) - ((int64_t)cv_base(r, ntaps, L, M) + (int64_t)n) * (int64_t)L + (int64_t)((ntaps - 1u) / 2u);
}
// float index of T_r[o][n] in the packed operator of NT 16 K floats
__host__ __device__ inline size_t cv_pack_index(uint32_t r, uint32_t o, uint32_t n, uint32_t K) {
    return (size_t)r * 16u * K + (((size_t)(n >> 4) * 64u) + (((n & 3u) << 4) | o)) * 4u + ((n >> 2) & 3u);
}
__host__ __device__ inline uint32_t cv_skew(uint32_t PI) { return (4u - (PI & 63u)) & 63u; }
// floats of a run of nper periods in LDS, at the largest shift
__host__ __device__ inline uint32_t cv_lds_floats(uint32_t nper, uint32_t PI, uint32_t lead, int32_t bmax, uint32_t K) {
    const uint32_t span = (uint32_t)((int32_t)(lead + 3u + (nper - 1u) * PI + K) + bmax + 3) & ~3u;
    return span + cv_skew(PI) * (span / PI + 1u);
}
// periods of a workgroup's run; 0: not even one period fits
__host__ __device__ inline uint32_t cv_nper(uint32_t P, uint32_t PI, uint32_t lead, int32_t bmax, uint32_t K) {
    uint32_t nper = (((CV_WG_SAMPLES + P - 1u) / P) + 15u) & ~15u;
    while (nper > 0 && cv_lds_floats(nper, PI, lead, bmax, K) > CV_LDS_FLOATS) nper = nper > 16u ? nper - 16u : nper - 1u;
    return nper;
}
struct ConvertItem {
    uint32_t quad_in;         // sample_offset / 4 | the channel mode << SCAN_MODE_SHIFT, as ScanItem::quad0
    uint32_t s_in;            // input sample frames of the item: ANY count, the last quad may be partial
    uint32_t s_out;           // floor(s_in L / M)
    uint32_t quad_out;        // out_offset / 4; the item owns roundup4(s_out) floats from there
};
static_assert(sizeof(ConvertItem) == 16, "ConvertItem layout");
struct ConvertWork {
    uint32_t item;            // index into the item table
    uint32_t run;             // the workgroup serves periods run * nper .. of it
};
static_assert(sizeof(ConvertWork) == 8, "ConvertWork layout");
struct ConvertArgs {
    const void *audio;        // the block, in its wire format
    float *out;               // the converted block
    const ConvertItem *items;
    const ConvertWork *work;  // [nwork]: one entry per workgroup
    const float *op;          // the packed operators: ntiles 16 K floats
    uint32_t nwork;
    uint32_t L, M;
    uint32_t ntaps;
    uint32_t P, PI;           // outputs and inputs of a period
    uint32_t ntiles;          // P / 16
    uint32_t ksteps;          // K / 16
    uint32_t nper;            // periods of a workgroup's run
    int32_t bmax;             // cv_base(ntiles - 1)
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
};
static_assert(sizeof(ConvertArgs) == 88, "ConvertArgs layout");

// one finished piece of audio out of a scanned block (csrc/scan_render.hip: vadk_scan_render, vadk_scan_render_stereo; vad_scan_render).  The kernel is
// driven by the OUTPUT: the host sweeps the segments' output spans into regions - maximal runs of output quads covered by the same
// none, one or two segments - and lists a workgroup per CUT_WG_QUADS quads of a region, so the kind of a workgroup is uniform.
// The segments are CutSeg, the sample range once (input quad quad_in + k for local quad k = output quad - quad_out).  ramp holds
// nrampq quads of the caller's fade table: local quad k of a segment is multiplied by ramp quad k if k < nrampq (the fade-in) and
// then by ramp quad nquads - 1 - k with its four components reversed if that index is below nrampq (the fade-out).
constexpr uint32_t RENDER_NONE = 0xffffffffu;
struct RenderWork {
    uint32_t seg_a, seg_b;    // the segments that cover this share: both RENDER_NONE = a gap (zeros), seg_b RENDER_NONE = one
    uint64_t quad_out;        // first output quad of this workgroup's share
    uint32_t nquads;          // 1 .. CUT_WG_QUADS
    uint32_t reserved;
};
static_assert(sizeof(RenderWork) == 24, "RenderWork layout");
struct RenderArgs {
    const void *audio;        // the block, in its wire format
    void *out;                // int16 or float32 samples: every quad of it is in exactly one workgroup's share
    const CutSeg *segs;
    const RenderWork *work;   // [nwork]: one entry per workgroup
    const float *gains;       // [segments] or nullptr: no factor
    const float *ramp;        // [4 nrampq], or nullptr with nrampq = 0
    uint32_t audio_bytes;     // the buffer descriptor's range
    uint32_t nwork;
    uint32_t nrampq;          // nramp / 4
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
    int32_t out_fmt;          // 0 = int16 PCM, 1 = float32
    float thresh;             // denoise gate, < 0 = off
    uint32_t reserved;
};
static_assert(sizeof(RenderArgs) == 80, "RenderArgs layout");

// the segment table of a scan (csrc/scan_segments.hip; vad_segments_device, vad_scan_segments).  Flat index k of the scan's CSR
// arrays is an END iff (events[k] & SEG_EV_MASK) == SEG_EV_END; every END becomes one SegRecord (the header's vad_segment), in
// ascending k.  Three passes fix that order: a workgroup of SEG_THREADS threads counts the ENDs of SEG_WG_FRAMES consecutive frames
// (16 event bytes per thread, one load), one workgroup turns the chunk counts into their exclusive prefix (SEG_THREADS chunks per
// round) and writes the grand total, and the fill pass reads each chunk again and writes its records from the chunk's prefix on.
// A fourth kernel, one wave per written record, adds the statistics.
constexpr int SEG_THREADS = 256;
constexpr int SEG_WG_FRAMES = 16 * SEG_THREADS;
constexpr int SEG_PROB_SHIFT = 30;            // a probability enters the mean as (int64) rint((double)p * 2^30): the sum is exact in any order
constexpr uint32_t SEG_EV_MASK = 0x82, SEG_EV_END = 0x02;     // VAD_EV_END set, VAD_EV_REJECTED clear
struct SegRecord {
    int32_t item, first_frame, nframes, counted;
    float mean_prob, max_prob;
};
static_assert(sizeof(SegRecord) == 24, "SegRecord layout");
struct SegArgs {
    const uint8_t *events;    // [total], 16-byte aligned
    const int32_t *seg_frames;
    const float *probs;
    const int32_t *out_start; // [n + 1] on the device: item i owns the flat indices out_start[i] .. out_start[i + 1] - 1
    uint32_t *chunk;          // [nchunks]: the count pass's counts, then their exclusive prefix
    SegRecord *segs;          // [seg_cap]
    long long *nsegs;         // the true count
    uint32_t first;           // out_start[0]: flat indices below it belong to no item and are not looked at
    uint32_t total;           // out_start[n] <= 2^31 - 1
    uint32_t nchunks;         // ceil(total / SEG_WG_FRAMES)
    uint32_t seg_cap;         // records at positions >= seg_cap are dropped (the host clamps a larger capacity to 2^31 - 1)
    int32_t n;                // items
};

// segment tables at other thresholds from a scan's per-frame results (csrc/scan_resegment.hip; vad_resegment_device,
// vad_scan_resegment).  Thread (item i, set k) replays the accepted frames of item i through a state machine that starts as
// sm0[k] - what a stream just opened and given the set's thresholds holds - and every END becomes one SegRecord; the records are
// ordered by set, then item, then frame.  Sets run along the lanes, padded to the power of two 1 << set_shift, so the lanes of a
// wave that share an item read the same addresses.  Two replays around a prefix fix the order: the first counts the ENDs of
// (item, set) into cnt[k n + i], one workgroup turns cnt into its exclusive prefix in that order and writes set_start[0 .. nt]
// (the records of the sets before k; [nt] = all), the second writes record j of (item, set) at cnt[k n + i] + j.
constexpr int RESEG_THREADS = 256;
constexpr int RESEG_MAX_SETS = 64;            // one wave holds a recording's sets
struct ResegArgs {
    const uint8_t *events;    // [out_start[n]]: VAD_EV_REJECTED alone is read
    const float *probs;
    const int32_t *out_start; // [n + 1] on the device, as SegArgs::out_start
    const SmSlot *sm0;        // [nt]
    uint32_t *cnt;            // [nt n]: counts, then their exclusive prefix (saturated at 2^32 - 1: no position below seg_cap)
    SegRecord *segs;          // [seg_cap]
    long long *set_start;     // [nt + 1]: the true counts
    uint32_t seg_cap;         // records at positions >= seg_cap are dropped (<= 2^31 - 1)
    int32_t n;                // items; n nt <= 2^31 - 1
    int32_t nt;               // sets, 1 .. RESEG_MAX_SETS
    int32_t set_shift;        // log2 of the lanes one item takes
};

// the segment still open at a recording's last frame (csrc/scan_tails.hip; vad_scan_tails, vad_scan_resegment_tails and the two
// device forms).  tail_len[k n + i] is the seg_frames of the state machine of (set k, item i) behind the item's last frame where it
// is inside a segment, else 0: vadk_tail_snapshot reads it out of the streams' slots (nt = 1; slots in the caller's item order),
// csrc/scan_resegment.hip's vadk_tails_reseg_count out of its threads' registers.  vadk_seg_tails, one wave per entry, turns every
// entry into one SegRecord - all zero where tail_len is 0 - with the statistics of vadk_seg_stats.
constexpr int TAIL_THREADS = 256;
struct TailArgs {
    const uint8_t *events;    // [out_start[n]]: VAD_EV_REJECTED alone is read
    const float *probs;
    const int32_t *out_start; // [n + 1] on the device, as SegArgs::out_start
    const SmSlot *sm;         // the engine's slots (vadk_tail_snapshot)
    const int32_t *slots;     // [n]: item i's stream (vadk_tail_snapshot)
    uint32_t *tail_len;       // [nt n]
    SegRecord *tails;         // [nt n] (vadk_seg_tails)
    int32_t n;                // items; n nt <= 2^31 - 1
    int32_t nt;               // sets; 1 on the scan path
};

// a segment table refined - clipped, merged, dropped, padded, split - by the rule of include/vad_engine.h's vad_refine
// (csrc/scan_refine.hip; vad_refine_device, vad_scan_refine).  The input is the first min(*nsegs_in, in_cap) records of segs_in and,
// where tails is given, the tail of each item as its last record.  first[i] is the table position of the first record that names
// item i behind a record that does not (the head of the item's first run; REFINE_NONE: no record names it): a thread per item walks
// that run twice around a prefix - cnt[i] = the item's output records, then their exclusive prefix, the total in *nsegs_out - and
// the second walk writes the records; a piece of a split carries its window in the fields the statistics overwrite later
// (counted = the half width h, the bits of mean_prob = REFINE_CUT_FIRST | REFINE_CUT_END: which of its two ends is searched), and
// one wave per written record then moves those ends to the quietest accepted frame of their windows.
constexpr int REFINE_THREADS = 256;
constexpr uint32_t REFINE_NONE = 0xffffffffu;
constexpr int REFINE_CUT_FIRST = 1, REFINE_CUT_END = 2;
struct RefineArgs {
    const SegRecord *segs_in; // [in_cap]
    const long long *nsegs_in;
    const SegRecord *tails;   // [n], or nullptr
    const uint8_t *events;    // [out_start[n]]: VAD_EV_REJECTED alone is read
    const float *probs;
    const int32_t *out_start; // [n + 1] on the device, as SegArgs::out_start
    uint32_t *first;          // [n]
    unsigned long long *cnt;  // [n]
    SegRecord *segs_out;      // [seg_cap]
    long long *nsegs_out;     // the true count
    uint32_t in_cap;          // <= 2^31 - 1
    uint32_t seg_cap;         // records at positions >= seg_cap are dropped (<= 2^31 - 1)
    int32_t n;                // items
    int32_t pad_before, pad_after, merge_gap, min_frames, max_frames;      // vad_refine, checked by the host
};

// resampler launch parameters (csrc/resample.hip)
struct ResampleSeg {
    const float *wstream;     // folded operator (pack_weights.cpp: pack_resample_operator)
    uint32_t wstream_bytes;
    uint32_t tile_blocks;     // blocks per 32-row tile = 8 + (n_in / 32) * 4
    uint32_t row128_block;    // first block of the VALU row's coefficients (outputs 128 / 384)
    const float *in;          // [n][n_in]
    float *out;               // [n][512]
    int32_t n;
    int32_t n_in;             // multiple of 256
};
// one launch resamples up to 4 segments (e.g. the 8 / 24 / 48 kHz clients of a tick): workgroups
// tile_start[s] .. tile_start[s+1]-1 serve segment s
constexpr int RESAMPLE_MAX_SEGS = 4;
struct ResampleParams {
    ResampleSeg seg[RESAMPLE_MAX_SEGS];
    int32_t nseg;
    int32_t tile_start[RESAMPLE_MAX_SEGS + 1];
};

// whole recordings at 8 / 24 / 48 kHz (csrc/scan_resample.hip: vadk_scan_resample; vad_scan_rate).  One launch serves one window
// of W frames of the `live` first items of the scan's sorted table: row i W + tt = chunk t0 + tt of item i - the n_in sample
// frames from 4 (quad0_i + (t0 + tt) hopq) on, decoded and channel-selected as the scans' loaders do - resampled to 512 samples at
// win + 512 (i W + tt); rows past an item's last chunk are not written.  The same launch writes the window's item table,
// items_win[i] = {slot_i, i W 128, clamp(nframes_i - t0, 0, W), out0_i + t0}: the model launch behind it (silero_v5_scan16,
// unchanged) scans `win` as a mono float32 block with hop = frame = 512.
struct ScanResampleArgs {
    const float *wstream;     // folded operator (pack_resample_operator), as ResampleSeg
    uint32_t wstream_bytes, tile_blocks, row128_block;
    uint32_t audio_bytes;     // the buffer descriptor's range: the whole block
    const void *audio;        // the block, in its wire format
    const ScanItem *items;    // the scan's sorted table
    ScanItem *items_win;      // [live]
    float *win;               // [live][W][512]
    int32_t live, W, t0;
    int32_t n_in;             // chunk length: 256 / 768 / 1536
    uint32_t hopq;            // hop / 4, in input sample frames
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
};

// the frames of finished segments of a block at 8 / 24 / 48 kHz (csrc/scan_cut_resample.hip: vadk_cut_resample;
// vad_scan_rate_cut, VAD_CUT_FRAMES).  The rows of a call are the frames of its segments in listing order, packed: segment s owns
// the rows row0_s .. row0_{s+1} - 1 (segs has one record more than the call has segments, its row0 the total), and row r of it is
// the n_in sample frames from 4 ((quad_in_s & mask) + (r - row0_s) hopq) on.  A launch serves the rows r0 .. rows_end - 1 - one
// window of the engine's buffer, r0 a multiple of the tile's 32 rows - and writes row r resampled to 512 samples at
// win + 512 (r - r0).  tile_seg[r / 32] is the segment that owns row 32 (r / 32): every segment has a row, so a thread finds its
// row's segment at most 31 records further on.  vadk_scan_cut (unchanged) then cuts `win` as a mono float32 block with
// hop = frame = 512, which is where the gate and the conversion to PCM16 happen.
struct CutResampleSeg {
    uint32_t quad_in;         // (sample_offset + first_frame * hop) / 4 | the channel mode << SCAN_MODE_SHIFT, as CutSeg::quad_in
    uint32_t row0;            // rows of the segments listed before this one
};
static_assert(sizeof(CutResampleSeg) == 8, "CutResampleSeg layout");
struct CutResampleArgs {
    const float *wstream;     // folded operator (pack_resample_operator), as ResampleSeg
    uint32_t wstream_bytes, tile_blocks, row128_block;
    uint32_t audio_bytes;     // the buffer descriptor's range: the whole block
    const void *audio;        // the block, in its wire format
    const CutResampleSeg *segs;   // [segments + 1]
    const uint32_t *tile_seg; // [ceil(rows / 32)], indexed by the row's tile in the whole call
    float *win;               // [rows_end - r0][512]
    uint32_t r0, rows_end;
    int32_t n_in;             // chunk length: 256 / 768 / 1536
    uint32_t hopq;            // hop / 4, in input sample frames
    int32_t fmt;              // vad_frame_format
    int32_t channels;         // 1 or 2
};
static_assert(sizeof(CutResampleArgs) == 80, "CutResampleArgs layout");

// fused resample -> Silero V5 step on 16-stream tiles (csrc/silero_v5_t16.hip, RS instantiation): one launch for a tick whose
// streams arrive at different rates.  Segment k = n streams of one input rate; stream0 = index of its first stream in the
// call's slots / probs / events arrays.  The tiles walk the segments back to back in the order given here: tile b carries the
// "virtual" streams 16 b .. 16 b + 15 of that concatenation (vstart = where the segment begins in it), so a tile may hold the
// last streams of one segment and the first of the next - it then resamples each part with its own operator - and 4 096
// streams in three uneven thirds are exactly 256 tiles, one per CU.
struct RateSeg {
    const float *wstream;     // pack_resample_operator_t16; nullptr: the segment is 16 kHz already (`in` holds 512-sample frames)
    uint32_t wstream_bytes;
    uint32_t wave_blocks;     // operator blocks per wave
    uint32_t row128_block;
    int32_t n, n_in, stream0, vstart;
    const float *in;          // [n][n_in]
};
constexpr int RATE_MAX_SEGS = 8;
struct RateParams {
    RateSeg seg[RATE_MAX_SEGS];
    int32_t nseg;
    int32_t total;            // streams of all segments
};

// statistics and model-ready batches of a feature matrix [rows][n_mels] (csrc/mel_batch.hip; vad_mel_stats, vad_mel_batch).
// vadk_mel_stats: a workgroup of MELB_THREADS threads reduces MELB_STATS_ROWS consecutive rows of ONE segment (MelStatsWork, listed
// by the host) and adds its partial results to the segment's with integer atomics; the caller has set max to -inf and the sums to 0.
constexpr int MELB_THREADS = 256;
constexpr int MELB_STATS_ROWS = 256;
struct MelStatsWork {
    uint32_t seg;             // the segment whose outputs take this workgroup's part
    uint32_t nrows;           // 1 .. MELB_STATS_ROWS
    uint64_t row0;            // first row of the part in the matrix
};
static_assert(sizeof(MelStatsWork) == 16, "MelStatsWork layout");
struct MelStatsArgs {
    const float *x;           // [rows][n_mels]
    const MelStatsWork *work; // [nwork]
    float *max_out;           // [n] or nullptr
    long long *sum_out;       // [n][n_mels] or nullptr
    unsigned long long *sumsq_out;   // [n][n_mels] or nullptr
    uint32_t nwork, n_mels;
};
static_assert(sizeof(MelStatsArgs) == 48, "MelStatsArgs layout");
// the fixed-point value of a feature (include/vad_engine.h: vad_mel_stats): exact in float32 up to the conversion
__host__ __device__ inline int32_t melb_q(float x) {
    const float c = x < -2048.0f ? -2048.0f : x > 2048.0f ? 2048.0f : x;
    return (int32_t)rintf(c * 4096.0f);
}

// vadk_mel_batch: a workgroup serves `tile` consecutive frames of ONE window (workgroup b: window b / tiles, tile b % tiles with
// tiles = ceil(frames / tile)).  tile is 64, or 32 where the rows of 64 frames with their halo (2 deltas rows on either side), as
// normalised values and - deltas == 2 - as first differences, would not fit 64 KiB of LDS at the odd pitch n_mels | 1.
struct MelBatchWin {
    uint64_t seg_row;         // first row of the window's segment in the matrix
    uint32_t M;               // rows of the segment
    uint32_t row0, nrows;     // the window: rows row0 .. row0 + nrows - 1 of the segment, nrows <= frames
    uint32_t seg;
};
static_assert(sizeof(MelBatchWin) == 24, "MelBatchWin layout");
struct MelBatchArgs {
    const float *x;           // [rows][n_mels]
    void *out;                // [nw][C][frames] or [nw][frames][C], C = n_mels (deltas + 1)
    const MelBatchWin *win;   // [nw]
    const float *lo;          // [n]
    const float *shift;       // [nss][n_mels]
    const float *scale;       // [nss][n_mels]
    uint32_t nw, n_mels, frames, deltas;
    int32_t layout, dtype, pad_mode;   // VAD_BATCH_*
    float pad_value;
    uint32_t per_seg;         // 1: shift / scale have a row per segment, 0: one row
    uint32_t tile;            // 64 or 32
};
static_assert(sizeof(MelBatchArgs) == 88, "MelBatchArgs layout");
__host__ __device__ inline uint32_t melb_pitch(uint32_t n_mels) { return n_mels | 1u; }
__host__ __device__ inline uint32_t melb_lds_floats(uint32_t n_mels, uint32_t deltas, uint32_t tile) {
    const uint32_t L = tile + 4u * deltas;
    return (deltas == 2u ? 2u * L - 4u : L) * melb_pitch(n_mels);
}
__host__ __device__ inline uint32_t melb_tile(uint32_t n_mels, uint32_t deltas) {
    return melb_lds_floats(n_mels, deltas, 64u) * 4u <= 65536u ? 64u : 32u;
}
// vadk_mel_batch_packed (vad_mel_batch_packed): several pieces of segments per window.  The host lists one workgroup per (piece,
// tile of `tile` frames of the piece) and one per pad run of at most `tile` frames, a span of whole quads of a window that no piece
// owns.  A workgroup owns frames t0 .. t0 + nt - 1 of its window - t0 and nt multiples of 4: the packed two-frame 16-bit store and a
// float32 quad never hold cells of two owners - of which the first nv show segment rows row0 .. row0 + nv - 1 and the rest are pad
// cells.  MelBatchArgs as above with win unused, lo [nw] and shift / scale [1 or nw][n_mels] indexed by WINDOW.
struct MelPackWork {
    uint64_t seg_row;         // first row of the piece's segment in the matrix
    uint32_t M;               // rows of the segment (a pad run: 0)
    uint32_t row0;            // the segment row at frame t0
    uint32_t window, t0;
    uint32_t nt;              // 4 .. tile, a multiple of 4, t0 + nt <= frames
    uint32_t nv;              // 0 .. nt (a pad run: 0), row0 + nv <= M
};
static_assert(sizeof(MelPackWork) == 32, "MelPackWork layout");
struct MelPackArgs {
    MelBatchArgs b;
    const MelPackWork *work;  // [nwork]
    uint32_t nwork;
};
static_assert(sizeof(MelPackArgs) == 104, "MelPackArgs layout");
// float32 -> bfloat16 bits, round to nearest even; overflow becomes inf, a NaN stays one
__host__ __device__ inline uint16_t melb_bf16(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((bits >> 16) | 0x40u);
    return (uint16_t)((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
}

// a projection of a feature matrix, y [rows][n_out] = bias + x [rows][n_in] * op [n_in][n_out] (csrc/mel_project.hip:
// vadk_mel_project; vad_mel_project).  A workgroup of PROJ_THREADS threads serves PROJ_ROWS consecutive rows (workgroup b: rows
// PROJ_ROWS b ..), each wave a tile of 16 of them over all column tiles, on v_mfma_f32_16x16x4_f32.  The host packs the operator
// into the B fragments' order, zero-padded to K4 = up4(n_in) rows and N16 = up16(n_out) columns - entry (k, c) at proj_pack_index:
// the 64 floats of (column tile c / 16, k-step k / 4) lie together, lane (k % 4) * 16 + c % 16 - followed by the bias, N16 floats,
// zero-padded.  At most 128 * 128 + 128 floats: it stays in L2.
constexpr int PROJ_THREADS = 256;
constexpr int PROJ_ROWS = 64;
constexpr int PROJ_MAX = 128;                 // n_in and n_out at the most
constexpr int PROJ_LOADS = 8;                 // loads a thread has in flight: of the matrix into LDS, and of the k-steps' fragments
__host__ __device__ inline uint32_t proj_up4(uint32_t n) { return (n + 3u) & ~3u; }
__host__ __device__ inline uint32_t proj_up16(uint32_t n) { return (n + 15u) & ~15u; }
__host__ __device__ inline uint32_t proj_pack_index(uint32_t k, uint32_t c, uint32_t K4) {
    return ((c >> 4) * (K4 >> 2) + (k >> 2)) * 64u + (k & 3u) * 16u + (c & 15u);
}
__host__ __device__ inline uint32_t proj_pack_floats(uint32_t n_in, uint32_t n_out) { return (proj_up4(n_in) + 1u) * proj_up16(n_out); }
// the x tile in LDS: PROJ_ROWS rows of K4 floats at an odd pitch
__host__ __device__ inline uint32_t proj_pitch(uint32_t n_in) { return proj_up4(n_in) | 1u; }
struct ProjArgs {
    const float *x;           // [rows][n_in], 4-byte aligned
    float *out;               // [rows][n_out], 4-byte aligned, apart from x
    const float *op;          // packed operator, then the bias: proj_pack_floats(n_in, n_out) floats
    uint64_t rows;
    uint32_t n_in, n_out;     // 1 .. PROJ_MAX
};
static_assert(sizeof(ProjArgs) == 40, "ProjArgs layout");

}  // namespace vadk
