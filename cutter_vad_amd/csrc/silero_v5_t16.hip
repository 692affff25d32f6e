// Silero-VAD V5 (16 kHz) step kernel on 16-STREAM tiles, for small and medium batches (gfx950).
//
// silero_v5.hip carries 32 streams per workgroup, so a launch of n streams occupies n / 32 of the 256 CUs: 1 024 streams
// (BASELINE.json configs[1]) use 32 CUs, 4 096 (configs[3]) half the chip - and a tile takes the same ~47 us however few
// there are.  This kernel is the same network, much of the same algebra (frame ingest under the recurrent gate half, 4-way folded
// DFT) and the same per-stream results, re-expressed on v_mfma_f32_16x16x4_f32: a workgroup (4 waves) carries 16
// streams, so the same batch spreads over twice as many CUs and every MFMA / VALU phase is half as long.
// The LSTM's two halves and the four encoder layers run on v_mfma_f32_16x16x32_bf16 instead, with weights and activations as exact
// three-piece bf16 splits (X3_HALF, X3_CONV below; vad_layout.h S_LSTM_X3, S_ENC0_X3, S_ENC1_X3, ENC23_X3_BLOCKS); the encoders as
// direct convolutions, not the Toom-3 product of silero_v5.hip, enc2 over its whole K in one wave, not split-K - and so does the
// odd-bin tile of the 16 kHz model's STFT (DFT_X3_BLOCKS); its even-bin tile and the 8 kHz sub-model's STFT alone are fp32.  An
// activation that feeds such a layer is cut into its pieces ONCE, by the lane that produces it, and lies in LDS as the consumers'
// B fragments ("activation planes", at QSD below).
// The engine runs it for every one-frame call and for multi-frame calls of at most T16_MAX_STREAMS streams (engine.cpp: launch()).
//
// Fragment convention (v_mfma_f32_16x16x4_f32, D = A[16 x 4] B[4 x 16] + C): lane l = (n = l & 15, kq = l >> 4).
//   A: lane (row n, kq) holds W[row][k = kq]       B: lane (stream n, kq) holds X[k = kq][n]
//   D: lane (stream n, rq = kq) holds rows 4 rq .. 4 rq + 3 of the 16-row tile  ->  exactly one LDS quad.
// One k-iteration j contracts 16 channels: lane (n, kq) reads activation quad row 4 j + kq of stream n (ONE ds_read_b128, the B
// operands of 4 MFMAs: component i = channel 16 j + 4 kq + i) and a 1 KiB weight block gives it W[row n][16 j + 4 kq + i].
// A wave owns 32 output channels = two row tiles rt = 0, 1: channel 32 w + 16 rt + 4 rq + i lives in quad row 8 w + 4 rt + rq.
// LDS quad row: 16 streams x float4.  The folded STFT operands are written TRANSPOSED by the loader (16 lanes of a stream write
// 16 different rows), so that view of the memory has a padded row stride (QSL = 17 float4); every other tensor is written and
// read in the D / B fragment layout (a group of 16 lanes = 256 contiguous bytes) and uses the dense stride QSD = 16.  With the
// two views overlaid the workgroup needs 78.6 KB of LDS - under half a CU's 160 KB.
// Two workgroups per CU were measured (__launch_bounds__(256, 2): 256 registers, 14 spilled; 8 192 streams = 512 tiles):
// 51.8 us against 53.6 us for the two tiles of a CU one after the other and 49.5 us for the 32-stream tile kernel, and
// +1.2 us on every batch of <= 4 096 streams - the second wave of a SIMD only hides waits; fp32 MFMAs and VALU work share the
// vector datapath on this chip, also across waves.  That was the fp32 kernel of round 3.  What the engine does today: the
// single-frame instantiations (ONE) fit a CU twice (<= 256 registers, <= 80 KB of LDS: tests/test_occupancy_contract.py), and every
// one-frame call runs on 16-stream tiles - up to one tile per CU (4 096 streams on 256 CUs) as silero_v5_step16, the tiles spread
// out; with more tiles than CUs (16 kHz model, float32 / int16) as silero_v5_pair16 below: the two tiles a CU gets anyway as ONE
// workgroup of eight waves that fetches every bf16 weight fragment once for both (G.711 and the 8 kHz sub-model: two workgroups of
// silero_v5_step16 per CU, as before).  Multi-frame calls use this kernel up to 4 096 streams, one workgroup per CU with all 512
// registers, and the 32-stream tiles above that.
// Weight stream: pack_silero_v5_t16.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>
#include "vad_layout.h"
#include "sm_device.h"
#include "vadk_device.h"

using namespace vadk;

#ifdef VADK_STAMPS      // tools/kbench.sh -DKB_TILE16 -DVADK_STAMPS: the same phase indices as silero_v5.hip
#define STAMP(k)                                                                                   \
    do {                                                                                           \
        if (lane == 0) P.stamps[((size_t)tilei * NWAVES + w) * 32 + (k)] = clock64();          \
    } while (0)
template <class V>
__device__ __forceinline__ void stamp_wait(V v) {
    if constexpr (sizeof(V) == 4) asm volatile("" ::"v"(v) : "memory");
    else if constexpr (sizeof(V) == 32) asm volatile("" ::"v"(v.b.x) : "memory");      // a two-channel float32 quad: its second load
    else asm volatile("" ::"v"(v.x) : "memory");
}
// in front of the stamp, v has arrived in its registers | every memory operation of the wave is acknowledged
// (not in the fused resampler's entry: its build with these stamps does not get through the register allocator)
#define STAMP_ON(k, v)                                                                             \
    do {                                                                                           \
        if constexpr (!RS) {                                                                       \
            stamp_wait(v);                                                                         \
            STAMP(k);                                                                              \
        }                                                                                          \
    } while (0)
#define STAMP_DRAIN(k)                                                                             \
    do {                                                                                           \
        if constexpr (!RS) {                                                                       \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                       \
            STAMP(k);                                                                              \
        }                                                                                          \
    } while (0)
#else
#define STAMP(k) do { } while (0)
#define STAMP_ON(k, v) do { } while (0)
#define STAMP_DRAIN(k) do { } while (0)
#endif
using namespace vadk::dev;

namespace {

constexpr int MT16 = 16;
constexpr int QSL = 17;                   // loader view (padded stride): the transposed stores of the fold - 16 kHz: the even tile's operands (T_EVEN_Q below), 8 kHz: all four
constexpr int QSD = 16;                   // dense view of the same memory, used by everything else:
//   rows 0..143 the |STFT| columns as activation planes (below; 48 c + 12 s + 4 p + kq; 8 kHz: 24 c + ..; the Nyquist channel is in
//   nyqv); rows 0..47 later enc1's output as planes (24 c + 12 s + ..: the four K-steps of enc2), then the LSTM input as planes; rows
//   144..287 = enc0's output as planes (144 + 48 c + ..), then rows 168..191 enc2's output as planes (168 + 12 s + ..); rows 248..295 =
//   h_{t-1} as planes.
// Activation planes: a tensor that feeds a bf16-split layer is cut into its three bf16 pieces by the lane that PRODUCES it, once,
// and lies in LDS as the consumers' B fragments: a plane group = one K-step s (32 channels) of the 16 streams = 12 quad rows, piece p
// of lane (n, kq)'s fragment = the 16 bytes at quad row 12 s + 4 p + kq, stream n - one ds_read_b128 per piece for each of the four
// waves that consume it, no VALU work (before: every wave cut every activation it read, 11 instructions per pair of values).
// Live ranges: the h planes are read in the recurrent half only (barrier (0) .. (1)) and written by the prologue and by the cell
// behind barrier (7), so they may lie under enc0's output (written behind (2), last read before (4)), in every instantiation (the
// rejected-frame hold keeps h_{t-1} in registers; silero_v5_pair16: written behind (4), read between (5) and (6)), and lie past the folded operands (T_ROWS_DFT, T_EVEN_Q below, live (0) .. (1b)); the |STFT| planes are
// written behind (1b) and read until (3); enc1's planes are written behind (3) and read until (5), enc2's planes behind (4)
// until (6); the x planes are written behind (5), when enc1's planes and the |STFT| planes are dead, and read until (7).
constexpr int T_ROW_E0 = 144;
constexpr int T_ROW_E = 168;
constexpr int T_ROW_H = 248;
constexpr int T_ROWS_H = 48;
constexpr int T_ROWS = T_ROW_H + T_ROWS_H;
constexpr int T_ROWS_E1 = 48;             // enc1's output: 2 columns x 2 K-steps of planes, rows 0..47
constexpr int T_ROWS_E2 = 24;             // enc2's output: 2 K-steps of planes at T_ROW_E
static_assert(T_ROW_E0 + 144 <= T_ROWS && T_ROW_E + 32 <= T_ROWS, "enc0's output and enc2's output end inside the activation region");
static_assert(T_ROWS_E1 <= T_ROW_E0, "enc1's planes are written while other waves still read enc0's output");
static_assert(T_ROW_E >= T_ROWS_E1 && T_ROW_E >= 48, "enc2's planes are written while enc1's are read, and read while the x planes are written");
static_assert(T_ROW_E >= T_ROW_E0 && T_ROW_E + T_ROWS_E2 <= T_ROW_H, "enc2's planes lie in enc0's dead output and stay clear of h");
// silero_v5_pair16 (the body's XFIRST order) writes the h planes behind barrier (4) and reads them behind (5), in front of (6): enc0's
// output above them is dead by then, and what is written or read between (4) and (7) - enc2's planes, the x planes (rows 0 ..
// T_ROWS_H - 1, the input half's) and the paired head exchange rows (T_ROW_E0 .. T_ROW_E0 + 31) - lies below them
// The head exchange (the body's cell in place): half 0's rows T_ROW_E0 + 8 w + 4 half + kq carry wave (0, w)'s row tile 0 terms of both
// tiles' head partials to wave (1, w) across barrier (8).  They are written with NO barrier since (6), while other waves are still in
// the input half: those read the x planes (rows 0 .. T_ROWS_H - 1) and nothing else in LDS, enc0's output here has been dead since
// barrier (4) and enc2's planes (T_ROW_E ..) since (6), whose enc3 and recurrent half are their and the h planes' last readers.
constexpr int T_ROWS_HEADX = 32;          // PAIR: 4 waves x 2 tiles x 4 quad rows from T_ROW_E0 on, across barrier (8)
static_assert(T_ROWS_H <= T_ROW_E0 && T_ROW_E0 + T_ROWS_HEADX <= T_ROW_H,
              "the head exchange rows lie above the x planes, which the input half of other waves is still reading, and below the h planes");
static_assert(T_ROW_E0 + T_ROWS_HEADX <= T_ROW_H && T_ROWS_H <= T_ROW_E0 && T_ROW_E + T_ROWS_E2 <= T_ROW_H,
              "frames first: the h planes, written behind barrier (4), stay clear of the x planes, enc2's planes and the head exchange rows");
static_assert(T_ROW_H >= T_ROW_E0 && T_ROW_H + T_ROWS_H <= T_ROWS, "frames first: the h planes take the place of enc0's output, dead behind barrier (4)");
// The folded STFT operands, live (0) .. (1b).  8 kHz sub-model: the loader view from row 0 on (96 rows).  16 kHz model: the odd tile
// runs on the bf16 split (vad_layout.h, DFT_X3_BLOCKS), so the loader cuts po | qo into planes, DENSE view: column c = rows 48 c ..
// 48 c + 47 = four plane groups 2 part + s (part 0 po, 1 qo; K-step s = the folded samples n = 32 s .. 32 s + 31), where the |STFT|
// planes of the same column follow them behind (1b).  Inside a row of such a group the stream is XOR-swizzled, stream n of lane
// (n, kq)'s fragment of K-step s at quad n ^ (kq | 4 s): the 16 loader lanes of a stream hold the 8 (kq, s) x 2 halves of ONE stream
// and would otherwise write 8 bytes each into the same 16-byte column of banks (an 8-way conflict of ds_write_b64's 16-lane
// groups); swizzled they cover all 32 banks, and a reader's 16-lane groups of ds_read_b128 (kq pairs 0 | 1 and 2 | 3 on
// complementary streams) still cover a whole row each.  The even tile's operands stay fp32 in the LOADER view behind the planes:
// T_EVEN_ROWS rows of QSL quads from quad T_EVEN_Q on, column c: pe+ 32 c + q', qe- 32 c + 8 + q', pe- 32 c + 16 + q', qe+ 32 c + 24 + q'
// (q' = 0..7, n = 4 q' .. 4 q' + 3; slot n = 0 of pe+ holds pe[32], of qe+ qe[32]).
constexpr int T_ROWS_DFT = 144;           // dense rows of the po | qo planes
constexpr int T_EVEN_Q = T_ROWS_DFT * QSD;
constexpr int T_EVEN_ROWS = 96;
static_assert(T_ROWS_DFT == 3 * 4 * 12, "three columns of four plane groups");
static_assert(T_EVEN_Q + T_EVEN_ROWS * QSL <= T_ROW_H * QSD, "the planes and the even operands behind them must end before h");
// The loader view proper - rows of QSL quads from row 0 on: the 8 kHz sub-model's folded operands (96 rows) and the resampler's
// staging (128 rows) - ends at this row.  (The name is from the layout in which the 16 kHz fold dropped duplicate quads into 32 sink
// rows from here on; the fold has none any more, and tests/test_act_planes_pack.py still holds the 32 rows behind it clear of h.)
constexpr int T_FOLD_SINK = 192;
static_assert(96 <= T_FOLD_SINK && T_FOLD_SINK * QSL <= T_ROW_H * QSD, "the 8 kHz sub-model's loader view must end before h");
static_assert(T_ROWS_DFT <= T_ROW_E0 && T_EVEN_Q >= T_ROW_E0 * QSD,
              "the magnitudes (rows 0..143, behind (1b)) take the planes' place; enc0's output (behind (2)) starts where the even operands did");
constexpr int T_LDS_F4 = T_ROWS * QSD + 16 + 12 + 36 + 16 + 96 + 128;   // + head partials [4][16], |X128| [3][16], fold corrections [3][3][16], sink [64], state machines [16] x 96 B, gate biases [4 waves][4 gates][32 units]
constexpr int T_LSTM_BIAS_BLOCK = 8 + 64 + 64 + 2;   // block of a wave's LSTM section that holds its gate biases compact: floats [gate][unit]
static_assert(T_LDS_F4 * 16 <= 80 * 1024, "stays under half a CU's LDS");
// float32 instantiations: + the frame's rejection flags (VAD_EV_REJECTED), one byte per (loader column half, stream), behind
// everything else
constexpr int T_FLAG_F4 = 2;
static_assert((T_LDS_F4 + T_FLAG_F4) * 16 <= 80 * 1024, "the flags stay under half a CU's LDS");
// RS instantiation (fused resample -> step).  The resampler's folded input chunks (2 buffers x {ue, ve, uo, vo} x 16 quad rows,
// loader stride) are staged in the activation region, which is idle until the frame loop starts; the tile's 16 kHz frames
// F [16 streams][129 quads] (128 + 1 of padding: the recombination stores scalars down a column of streams) have 33 KB of their
// own behind the common layout (111.6 KB in all; the launch is one workgroup per CU anyway) - so a tile whose 16 streams come
// from TWO segments (the last streams of one input rate and the first of the next) can resample one part after the other, each
// with its own operator, without the second part's staging running over the first part's frames.
constexpr int FQ = 129;
constexpr int RS_CH_ROWS = 16;
constexpr int RS_BUF = 4 * RS_CH_ROWS * QSL;
static_assert(2 * RS_BUF <= T_FOLD_SINK * QSL, "resampler staging must fit the loader view");
static_assert((T_LDS_F4 + MT16 * FQ) * 16 <= 160 * 1024, "RS: common layout + F must fit one CU");

__device__ __forceinline__ f32x4 mfma16(f32x4 w, f32x4 a, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, a.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, a.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, a.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, a.w, acc, 0, 0, 0);
    return acc;
}

// A wave's two D quads (row tiles 0, 1) of a lane -> the three pieces of K-step s = w's fragment, into the plane group at grp (= the
// group's first row + the lane's nq); a single D quad (8 kHz |STFT|: a wave owns one row tile) -> half of each piece
__device__ __forceinline__ void st_planes(f32x4 *grp, f32x4 xa, f32x4 xb) {
    u32x4 F[3];
    split3_frag(xa, xb, F);
#pragma unroll
    for (int p = 0; p < 3; ++p) grp[4 * p * QSD] = __builtin_bit_cast(f32x4, F[p]);
}
__device__ __forceinline__ void st_planes_half(f32x4 *grp, int half, f32x4 x) {
    u32x2 H[3];
    split3_half(x, H);
#pragma unroll
    for (int p = 0; p < 3; ++p) reinterpret_cast<f32x2 *>(grp + 4 * p * QSD)[half] = __builtin_bit_cast(f32x2, H[p]);
}
// piece p of the lane's fragment of K-step s
#define PL_RD(SRC, s, p) __builtin_bit_cast(u32x4, (SRC)[(12 * (s) + 4 * (p)) * QSD + nq])

// the weight ring of the bf16-split layers (S_LSTM_X3, S_ENC0_X3): units requested ahead, slots
constexpr int X3_D = 4;
constexpr int X3_NR = X3_D + 1;

// f(integral_constant<int, i>) for i = 0 .. N - 1, in order: every unit of a split layer is its own code, with constant indices
template <class F, int... I>
__device__ __forceinline__ void x3_units(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

}  // namespace

// A k-iteration's MFMAs with the NEXT iteration's requests issued in their shadow: ND LDS reads first, then one weight-block
// request behind every four MFMAs, NV times.  On this kernel's 32-cycle MFMAs a burst of 8 - 10 requests between two groups of 32
// costs ~10 % of the group (the 32-stream kernel's MFMAs are twice as long and were left alone, but for its STFT).
#define T16_IL(NV, ND)                                                                                          \
    __builtin_amdgcn_sched_group_barrier(0x100, (ND), 0);                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < (NV); ++i_) {                                                       \
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                                      \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                      \
    }
// One half of the LSTM (W_ih . x or W_hh . h) on the bf16 split: 32 units u = 8 s + tile, unit u = the six MFMAs of tile u & 7 at
// K-step s (vadk_device.h: mfma_x3) into G[tile].  Requests run X3_D units ahead through the ring xw, unit u in slot (U0 + u) % X3_NR
// (U0: where the layer in front left the ring - the input half follows enc3's units).  The activations: lane (n, kq)
// reads its fragment's three pieces of K-step s from the plane groups at SRC (quad rows 12 s + 4 p + kq), ready made; K-step s + 1's
// are read in unit (s, 0), under K-step s's MFMAs.
// EXTRA(u): work placed in unit u; FOLD(u): unit u is fenced together with the next one (a longer region for the caller's
// interleave hints).
#define X3_UNIT(u, U0, B, SRC, EXTRA, FOLD)                                                                     \
    {                                                                                                           \
        constexpr int s_ = (u) >> 3, k_ = (u) & 7;                                                              \
        if constexpr ((u) + X3_D < 32) { X3_LD(B, (u) + X3_D, U0) }                                             \
        if constexpr (k_ == 0 && s_ < 3) { _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) N_[p_] = PL_RD(SRC, s_ + 1, p_); } \
        EXTRA(u)                                                                                                \
        G[k_] = mfma_x3(xw[((U0) + (u)) % X3_NR], F_, G[k_]);                                                   \
        if constexpr (k_ == 7) { F_[0] = N_[0]; F_[1] = N_[1]; F_[2] = N_[2]; }                                 \
        if constexpr (!(FOLD(u)) || k_ == 7) SB();                                                              \
    }
#define X3_STEP(s, U0, B, SRC, EXTRA, FOLD)                                                                     \
    X3_UNIT(8 * (s) + 0, U0, B, SRC, EXTRA, FOLD) X3_UNIT(8 * (s) + 1, U0, B, SRC, EXTRA, FOLD)                 \
    X3_UNIT(8 * (s) + 2, U0, B, SRC, EXTRA, FOLD) X3_UNIT(8 * (s) + 3, U0, B, SRC, EXTRA, FOLD)                 \
    X3_UNIT(8 * (s) + 4, U0, B, SRC, EXTRA, FOLD) X3_UNIT(8 * (s) + 5, U0, B, SRC, EXTRA, FOLD)                 \
    X3_UNIT(8 * (s) + 6, U0, B, SRC, EXTRA, FOLD) X3_UNIT(8 * (s) + 7, U0, B, SRC, EXTRA, FOLD)
#define X3_HALF(U0, B, SRC, EXTRA, FOLD)                                                                        \
    {                                                                                                           \
        u32x4 F_[3], N_[3];                                                                                     \
        _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) F_[p_] = PL_RD(SRC, 0, p_);                            \
        SB();                                                                                                   \
        X3_STEP(0, U0, B, SRC, EXTRA, FOLD) X3_STEP(1, U0, B, SRC, EXTRA, FOLD)                                 \
        X3_STEP(2, U0, B, SRC, EXTRA, FOLD) X3_STEP(3, U0, B, SRC, EXTRA, FOLD)                                 \
    }
// The paired form (silero_v5_pair16): wave (hf, w) computes row tile rt = hf of the four gates for BOTH half-tiles' streams - 16 units
// v = 4 s + q per half, unit v = the existing unit 8 s + 2 q + hf of S_LSTM_X3 (X3_LDP), its three blocks feeding two mfma_x3: on the
// wave's own tile's B fragments (SRC0, into Gp[q][0]) and on the partner half's (SRC1, Gp[q][1]).  An accumulator sees what it saw.
#define X3P_UNIT(v, U0, B, SRC0, SRC1, EXTRA, FOLD)                                                             \
    {                                                                                                           \
        constexpr int s_ = (v) >> 2, q_ = (v) & 3;                                                              \
        if constexpr ((v) + X3_D < 16) { X3_LDP(B, (v) + X3_D, U0) }                                            \
        if constexpr (q_ == 0 && s_ < 3) {                                                                      \
            _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) { N0_[p_] = PL_RD(SRC0, s_ + 1, p_); N1_[p_] = PL_RD(SRC1, s_ + 1, p_); } \
        }                                                                                                       \
        EXTRA(v)                                                                                                \
        Gp[q_][0] = mfma_x3(xw[((U0) + (v)) % X3_NR], F0_, Gp[q_][0]);                                          \
        Gp[q_][1] = mfma_x3(xw[((U0) + (v)) % X3_NR], F1_, Gp[q_][1]);                                          \
        if constexpr (q_ == 3) { _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) { F0_[p_] = N0_[p_]; F1_[p_] = N1_[p_]; } } \
        if constexpr (!(FOLD(v)) || q_ == 3) SB();                                                              \
    }
#define X3P_STEP(s, U0, B, SRC0, SRC1, EXTRA, FOLD)                                                             \
    X3P_UNIT(4 * (s) + 0, U0, B, SRC0, SRC1, EXTRA, FOLD) X3P_UNIT(4 * (s) + 1, U0, B, SRC0, SRC1, EXTRA, FOLD) \
    X3P_UNIT(4 * (s) + 2, U0, B, SRC0, SRC1, EXTRA, FOLD) X3P_UNIT(4 * (s) + 3, U0, B, SRC0, SRC1, EXTRA, FOLD)
#define X3P_HALF(U0, B, SRC0, SRC1, EXTRA, FOLD)                                                                \
    {                                                                                                           \
        u32x4 F0_[3], F1_[3], N0_[3], N1_[3];                                                                   \
        _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) { F0_[p_] = PL_RD(SRC0, 0, p_); F1_[p_] = PL_RD(SRC1, 0, p_); } \
        SB();                                                                                                   \
        X3P_STEP(0, U0, B, SRC0, SRC1, EXTRA, FOLD) X3P_STEP(1, U0, B, SRC0, SRC1, EXTRA, FOLD)                 \
        X3P_STEP(2, U0, B, SRC0, SRC1, EXTRA, FOLD) X3P_STEP(3, U0, B, SRC0, SRC1, EXTRA, FOLD)                 \
    }
// A direct 3-tap convolution on the bf16 split (encoder.0: vad_layout.h S_ENC0_X3, in the second weight stream - block offset B
// into it; LDM = the stream's unit loader, X3_LDX / X3_LDY): NO output columns
// out(o) = sum_tap W[tap] x[STR o + tap - 1] over the three input columns x[c], plane groups at SRC(c), NT row tiles per
// wave, NS K-steps of 32 channels.  Unit u = (K-step s, tap, tile) = (s * 3 + tap) * NT + tile: the tap's A fragment (3 blocks at
// B + 3 u, ring slot (U0 + u) % X3_NR) feeds every output column that the tap reaches, mfma_x3 into ACC[o][tile] - the unit is
// loaded once and used up to three times.  K-step s + 1's nine pieces (three columns) are read in K-step s's first unit.  Requests
// run X3_D units ahead.  EXTRA(u): work placed in unit u.
#define X3_CONV(NS, NT, STR, NO, LDM, B, U0, SRC, ACC, EXTRA)                                         \
    {                                                                                                           \
        constexpr int NU_ = (NS) * 3 * (NT);                                                                    \
        u32x4 F_[3][3], N_[3][3];                                                                               \
        _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_)                                                        \
            _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) F_[c_][p_] = PL_RD(SRC(c_), 0, p_);                \
        SB();                                                                                                   \
        x3_units([&](auto uc_) {                                                                                \
            constexpr int u_ = decltype(uc_)::value, s_ = u_ / (3 * (NT)), r_ = u_ % (3 * (NT));                \
            constexpr int t_ = r_ / (NT), tl_ = r_ % (NT);                                                      \
            if constexpr (u_ + X3_D < NU_) { LDM((B) + 3 * (u_ + X3_D), (U0) + u_ + X3_D) }                     \
            if constexpr (r_ == 0 && s_ + 1 < (NS)) {                                                           \
                _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_)                                                \
                    _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) N_[c_][p_] = PL_RD(SRC(c_), s_ + 1, p_);   \
            }                                                                                                   \
            EXTRA(u_)                                                                                           \
            _Pragma("unroll") for (int o_ = 0; o_ < (NO); ++o_) {                                               \
                const int c_ = (STR) * o_ + t_ - 1;                                                             \
                if (c_ >= 0 && c_ < 3) ACC[o_][tl_] = mfma_x3(xw[((U0) + u_) % X3_NR], F_[c_], ACC[o_][tl_]);    \
            }                                                                                                   \
            if constexpr (s_ + 1 < (NS)) {                                                                      \
                if constexpr (r_ == 3 * (NT) - 1) {                                                             \
                    _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_)                                            \
                        _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) F_[c_][p_] = N_[c_][p_];               \
                }                                                                                               \
            }                                                                                                   \
            SB();                                                                                               \
        }, std::make_integer_sequence<int, NU_>{});                                                             \
    }

// RS: one tick for streams at other input rates (vad_step_rates): the tile first resamples its 16 chunks to 16 kHz into LDS -
// AudioUtils.resample_audio's Fourier method as the folded operator of resample.hip, on 16 x 16 x 4 tiles - and the frame loop
// ingests them from there: no second launch, no HBM round trip of the 16 kHz frames.  T = 1, float32 input.
// K8: the graph's 8 kHz sub-model on native 8 kHz audio in 256-sample frames (silero_v5.hip has the algebra: window 128, hop 64, three
// columns, 4-way fold with n = 1..31, 64 complex bins as four 16-row tiles - one per wave - bin 64 on the VALU, encoder.0 with 65
// input channels; from enc1 on the instantiations are the same): pools of at most 4 096 native-8 kHz sessions get one tile per CU
// like the 16 kHz model's (the 32-stream K8 kernel runs n / 32 CUs: 37 us whatever the size).  Loader: 8 lanes per stream, so a
// fold call covers TWO columns of the tile's 16 streams (threads 0..127 / 128..255).
// ONE: one frame per stream in the call (k_T == 1), instantiated without the frame loop (silero_v5.hip has the reasons); the fused
// resample -> step launch is always one frame.
// FMT: the wire format of the frames - 0 float32, 1 int16 (either scale), 2 / 3 ITU-T G.711 mu-law / A-law, one byte per sample.
// SCAN (silero_v5_scan16): whole recordings.  The frame loop reads contiguous audio and a table of work items (vad_layout.h:
// ScanItem) instead of [n][T][frame]: frame t of the loader's stream is addressed at quad quad0 + t hop / 4, so overlapping frames
// (hop < frame) are never materialised, and the streams of a tile may have different frame counts - the items arrive sorted by
// count (descending), the tile's loop runs to its first item's count, and a stream whose recording has ended is HELD exactly as a
// rejected float32 frame holds one (h, c selected from the previous values, no sm_step), in every format, and writes no result.
// Results go to out0 + t (CSR); the finished segment's length is written on every END, 0 on the recording's other frames.
// CH = 2 (silero_v5_stereo16): the same scan over interleaved two-channel recordings L0 R0 L1 R1 ..  All positions count sample
// frames; a quad of four sample frames is twice the mono quad's bytes (float32: two b128 loads, int16: the b128 the mono loader
// issues anyway, G.711: a b64), both channels are decoded and the item's mode - in the top bits of its quad0, vad_layout.h -
// selects the left one, the right one or their mean (dL + dR) * 0.5f = AudioUtils.convert_to_mono, in front of the non-finite
// check and the gate.  The VALU instructions this adds (178 per wave in the int16 body) lie in the fold's slot under the recurrent
// MFMAs but do not all hide there: + 1.8 % per frame at 4 096 streams, within the spread at 1 024; everything behind
// the decode is the scan's.  The channel count belongs to the call, the mode to the item: two items may name the same samples.
// The kernel's body is silero_v5_t16_body.h, shared by the four __global__ entries below.
// One workgroup per CU also here.  Built for two (a tick's segments are padded to whole tiles, so it can have a few more tiles
// than CUs), the dispatcher packs consecutive workgroups onto the same CU: 258 tiles ran on ~130 CUs, 69.9 us per tick against
// 55.6 for the two-launch form - so the engine uses this launch only when the tick has at most one tile per CU.
// (the eight leading arguments: the fields of P the kernel needs first, preloaded into SGPRs - see silero_v5.hip; KP(f) = that copy)
#define STEP16_PARAMS const float *k_wstream, float *k_state, SmSlot *k_sm, const int32_t *k_slots, const void *k_frames, const int k_n, \
                      const uint32_t k_wstream_bytes, const int k_T, const StepParams P, const RateParams R
// float32 / int16 frames (and the fused resampler); tests/test_occupancy_contract.py knows these by name
// (entries that are no scan: the body's SCAN branches are discarded, these two names only have to exist)
#define STEP16_NO_SCAN                                  \
    constexpr bool SCAN = false;                        \
    constexpr int CH = 1;                               \
    constexpr const ScanItem *k_items = nullptr;        \
    constexpr ScanArgs S{};
#define STEP16_NO_PAIR                                  \
    constexpr bool PAIR = false;                        \
    constexpr bool XFIRST = false;
template <bool F32IN_, bool RS, bool K8 = false, bool ONE = false>
__global__ void __launch_bounds__(NTHREADS, 1) silero_v5_step16(STEP16_PARAMS) {
    constexpr int FMT = F32IN_ ? 0 : 1;
    STEP16_NO_SCAN
    STEP16_NO_PAIR
#include "silero_v5_t16_body.h"
}
// One-frame calls with more tiles than CUs (16 kHz model, float32 / int16): the TWO tiles of a CU as one workgroup of eight waves.
// Wave (hf, w) is wave w of half-tile hf = tile 2 blockIdx.x + hf, with its own half of the LDS, and runs the body as it is, behind
// barriers the halves share - but for the bf16-split LSTM halves and encoder.0, where it computes ONE row tile (rt = hf) for BOTH
// half-tiles' streams: every weight fragment that reaches the CU's registers feeds two stream tiles, and the bytes those layers
// stream per wave halve - and for encoder.1 (one output column, hf, for both half-tiles: two thirds of its units) and encoder.3 (row
// tile hf for both: half of them).  The body's PAIR branches; results bit for bit those of silero_v5_step16<., false, false, true>.
template <bool F32IN_>
__global__ void __launch_bounds__(2 * NTHREADS, 1) silero_v5_pair16(STEP16_PARAMS) {
    constexpr int FMT = F32IN_ ? 0 : 1;
    constexpr bool RS = false, K8 = false, ONE = true, PAIR = true;
    constexpr bool XFIRST = true;      // frames first, the recurrent half behind enc3 (silero_v5_t16_body.h)
    STEP16_NO_SCAN
#include "silero_v5_t16_body.h"
}
// ITU-T G.711 frames (VAD_FMT_ULAW8 / VAD_FMT_ALAW8), decoded in the loader
template <bool ALAW, bool K8, bool ONE>
__global__ void __launch_bounds__(NTHREADS, 1) silero_v5_step16_g711(STEP16_PARAMS) {
    constexpr int FMT = ALAW ? 3 : 2;
    constexpr bool RS = false;
    STEP16_NO_SCAN
    STEP16_NO_PAIR
#include "silero_v5_t16_body.h"
}
// whole recordings (vad_scan): k_items [k_n] work items, k_frames the audio block, k_T the frames of the launch's window
template <int FMT_, bool K8>
__global__ void __launch_bounds__(NTHREADS, 1) silero_v5_scan16(const float *k_wstream, float *k_state, SmSlot *k_sm, const ScanItem *k_items,
                                                                const void *k_frames, const int k_n, const uint32_t k_wstream_bytes,
                                                                const int k_T, const StepParams P, const ScanArgs S) {
    constexpr int FMT = FMT_;
    constexpr bool RS = false, ONE = false, SCAN = true;
    constexpr int CH = 1;
    constexpr const int32_t *k_slots = nullptr;
    const RateParams R{};
    STEP16_NO_PAIR
#include "silero_v5_t16_body.h"
}
// whole two-channel recordings, interleaved (vad_scan_channels): the scan with every position counted in sample frames
template <int FMT_, bool K8>
__global__ void __launch_bounds__(NTHREADS, 1) silero_v5_stereo16(const float *k_wstream, float *k_state, SmSlot *k_sm, const ScanItem *k_items,
                                                                  const void *k_frames, const int k_n, const uint32_t k_wstream_bytes,
                                                                  const int k_T, const StepParams P, const ScanArgs S) {
    constexpr int FMT = FMT_;
    constexpr bool RS = false, ONE = false, SCAN = true;
    constexpr int CH = 2;
    constexpr const int32_t *k_slots = nullptr;
    const RateParams R{};
    STEP16_NO_PAIR
#include "silero_v5_t16_body.h"
}
#undef STEP16_NO_PAIR
#undef STEP16_NO_SCAN
#undef STEP16_PARAMS
#undef X3_CONV
#undef X3P_HALF
#undef X3P_STEP
#undef X3P_UNIT
#undef X3_HALF
#undef X3_STEP
#undef X3_UNIT
#undef PL_RD


#define V5_ARGS p->wstream, p->state, p->sm, p->slots, p->frames, (int)p->n, p->wstream_bytes, (int)p->T, *p
extern "C" hipError_t vadk_launch_silero_v5_t16(const vadk::StepParams *p, hipStream_t stream) {
    (void)hipGetLastError();
    const int tiles = (p->n + MT16 - 1) / MT16;
    if (tiles <= 0) return hipSuccess;
    const vadk::RateParams none{};
#define T16_LAUNCH(F, K, O) hipLaunchKernelGGL((silero_v5_step16<F, false, K, O>), dim3(tiles), dim3(vadk::NTHREADS), 0, stream, V5_ARGS, none)
    if (p->T < 1) return hipErrorInvalidValue;     // the frame loop tests its count at the bottom
    const bool k8 = p->variant != 0;               // the 8 kHz sub-model's blob (256-sample frames)
#define T16_LAUNCH_G711(A, K, O) hipLaunchKernelGGL((silero_v5_step16_g711<A, K, O>), dim3(tiles), dim3(vadk::NTHREADS), 0, stream, V5_ARGS, none)
    const bool one = p->T == 1;
    if (p->fmt == 3 || p->fmt == 4) {                  // vad_frame_format: G.711 mu-law | A-law
        if (reinterpret_cast<uintptr_t>(p->frames) & 3) return hipErrorInvalidValue;     // a quad of samples is one dword
        const bool al = p->fmt == 4;
        if (k8) {
            if (al) { if (one) T16_LAUNCH_G711(true, true, true); else T16_LAUNCH_G711(true, true, false); }
            else { if (one) T16_LAUNCH_G711(false, true, true); else T16_LAUNCH_G711(false, true, false); }
        } else {
            if (al) { if (one) T16_LAUNCH_G711(true, false, true); else T16_LAUNCH_G711(true, false, false); }
            else { if (one) T16_LAUNCH_G711(false, false, true); else T16_LAUNCH_G711(false, false, false); }
        }
        return hipGetLastError();
    }
    if (p->fmt < 0 || p->fmt > 2) return hipErrorInvalidValue;     // float32 | int16 / 32767 | int16 / 32768
    const bool f32 = p->fmt == 0;
    if (k8) {
        if (f32) { if (one) T16_LAUNCH(true, true, true); else T16_LAUNCH(true, true, false); }
        else { if (one) T16_LAUNCH(false, true, true); else T16_LAUNCH(false, true, false); }
    } else {
        if (f32) { if (one) T16_LAUNCH(true, false, true); else T16_LAUNCH(true, false, false); }
        else { if (one) T16_LAUNCH(false, false, true); else T16_LAUNCH(false, false, false); }
    }
#undef T16_LAUNCH_G711
#undef T16_LAUNCH
    return hipGetLastError();
}

// the paired form of a one-frame call on the 16 kHz model, float32 or int16 frames: tiles 2 b and 2 b + 1 in workgroup b
extern "C" hipError_t vadk_launch_silero_v5_t16_pair(const vadk::StepParams *p, hipStream_t stream) {
    (void)hipGetLastError();
    const int tiles = (p->n + MT16 - 1) / MT16;
    if (tiles <= 0) return hipSuccess;
    if (p->T != 1 || p->variant != 0 || p->fmt < 0 || p->fmt > 2) return hipErrorInvalidValue;
    const vadk::RateParams none{};
    if (p->fmt == 0) hipLaunchKernelGGL((silero_v5_pair16<true>), dim3((tiles + 1) / 2), dim3(2 * vadk::NTHREADS), 0, stream, V5_ARGS, none);
    else hipLaunchKernelGGL((silero_v5_pair16<false>), dim3((tiles + 1) / 2), dim3(2 * vadk::NTHREADS), 0, stream, V5_ARGS, none);
    return hipGetLastError();
}

// whole recordings: p->n items (sorted by frame count, descending), p->frames = the audio block, p->T = frames of this launch's window
// [a->t0, a->t0 + p->T), p->probs / events / seg_frames = the CSR arrays; p->fmt as in vadk_launch_silero_v5_t16
// a->channels = 2: the block is interleaved two-channel audio (silero_v5_stereo16; 8-byte aligned: G.711's quad of sample frames)
extern "C" hipError_t vadk_launch_silero_v5_scan16(const vadk::StepParams *p, const vadk::ScanItem *items, const vadk::ScanArgs *a,
                                                   hipStream_t stream) {
    (void)hipGetLastError();
    const int tiles = (p->n + MT16 - 1) / MT16;
    if (tiles <= 0) return hipSuccess;
    if (p->T < 1 || p->fmt < 0 || p->fmt > 4 || a->hopq < 1 || a->t0 < 0 || (a->audio_bytes >> 31)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p->frames) & 3) || (reinterpret_cast<uintptr_t>(items) & 15)) return hipErrorInvalidValue;
    if (a->channels < 0 || a->channels > 2 || (a->channels == 2 && (reinterpret_cast<uintptr_t>(p->frames) & 7))) return hipErrorInvalidValue;
#define SCAN16_LAUNCH(F, K)                                                                                                    \
    hipLaunchKernelGGL((silero_v5_scan16<F, K>), dim3(tiles), dim3(vadk::NTHREADS), 0, stream, p->wstream, p->state, p->sm, items, \
                       p->frames, (int)p->n, p->wstream_bytes, (int)p->T, *p, *a)
#define STEREO16_LAUNCH(F, K)                                                                                                  \
    hipLaunchKernelGGL((silero_v5_stereo16<F, K>), dim3(tiles), dim3(vadk::NTHREADS), 0, stream, p->wstream, p->state, p->sm, items, \
                       p->frames, (int)p->n, p->wstream_bytes, (int)p->T, *p, *a)
    const int f = p->fmt == 0 ? 0 : p->fmt <= 2 ? 1 : p->fmt - 1;      // vad_frame_format -> FMT
    if (a->channels == 2) {
        if (p->variant != 0) {
            if (f == 0) STEREO16_LAUNCH(0, true); else if (f == 1) STEREO16_LAUNCH(1, true); else if (f == 2) STEREO16_LAUNCH(2, true); else STEREO16_LAUNCH(3, true);
        } else {
            if (f == 0) STEREO16_LAUNCH(0, false); else if (f == 1) STEREO16_LAUNCH(1, false); else if (f == 2) STEREO16_LAUNCH(2, false); else STEREO16_LAUNCH(3, false);
        }
    } else if (p->variant != 0) {
        if (f == 0) SCAN16_LAUNCH(0, true); else if (f == 1) SCAN16_LAUNCH(1, true); else if (f == 2) SCAN16_LAUNCH(2, true); else SCAN16_LAUNCH(3, true);
    } else {
        if (f == 0) SCAN16_LAUNCH(0, false); else if (f == 1) SCAN16_LAUNCH(1, false); else if (f == 2) SCAN16_LAUNCH(2, false); else SCAN16_LAUNCH(3, false);
    }
#undef STEREO16_LAUNCH
#undef SCAN16_LAUNCH
    return hipGetLastError();
}

// one tick for streams at several input rates: resample + step fused, one launch (p->T must be 1, p->n = all streams)
extern "C" hipError_t vadk_launch_silero_v5_t16_rates(const vadk::StepParams *p, const vadk::RateParams *r, hipStream_t stream) {
    (void)hipGetLastError();
    const int tiles = (r->total + MT16 - 1) / MT16;
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL((silero_v5_step16<true, true>), dim3(tiles), dim3(vadk::NTHREADS), 0, stream, V5_ARGS, *r);
    return hipGetLastError();
}
