// Device helpers shared by the fused model kernels (gfx950): MFMA fragment convention, quad stores,
// fenced scheduling, buffer-descriptor weight loads, fast activation functions.  See vad_layout.h.
// Behind them what the scan kernels share: a block's wire quads (WireQuad), the gate, the PCM16 conversion and the packed store of
// segment audio (pcm16, store_quad), and the launchers' choice of an instantiation (wire_fmt, launch_variant).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>
#include "../../include/vad_engine.h"
#include "vad_layout.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

namespace vadk { namespace dev {

__device__ __forceinline__ f32x16 mfma4(f32x4 w, f32x4 a, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, a.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, a.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, a.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, a.w, acc, 0, 0, 0);
    return acc;
}

// accumulator initialised from 4 "lane-expanded" bias blocks (regs 4g..4g+3 <- block g)
__device__ __forceinline__ f32x16 acc_from(const f32x4 *ws) {
    f32x4 b0 = ws[0], b1 = ws[BLK_F4], b2 = ws[2 * BLK_F4], b3 = ws[3 * BLK_F4];
    f32x16 a;
    a.s0 = b0.x; a.s1 = b0.y; a.s2 = b0.z; a.s3 = b0.w;
    a.s4 = b1.x; a.s5 = b1.y; a.s6 = b1.z; a.s7 = b1.w;
    a.s8 = b2.x; a.s9 = b2.y; a.sa = b2.z; a.sb = b2.w;
    a.sc = b3.x; a.sd = b3.y; a.se = b3.z; a.sf = b3.w;
    return a;
}

// A quad stored as two 8-byte halves: values that come out of packed (pair) arithmetic or of scalar ops need not be copied
// into four consecutive registers first (the compiler merges the two halves into one ds_write2_b64)
__device__ __forceinline__ void st2(f32x4 *dst, f32x4 v) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 *d = reinterpret_cast<f32x2 *>(dst);
    d[0] = f32x2{v.x, v.y};
    d[1] = f32x2{v.z, v.w};
}

// ReLU as ONE instruction: max of the BIT PATTERN, as a signed integer, with 0 - a float with its sign bit clear is a non-negative
// integer and is kept, one with the sign bit set (negative values, -0) is a negative integer and becomes +0.  fmaxf(v, 0) and
// v_med3_f32(v, 0, +inf) - which the compiler folds back into fmaxf - cost two v_max_f32 each, the first (v, v) only to quiet a
// signalling NaN the hardware would quiet anyway.  (Inline asm `v_max_f32 %0, 0, %1` is NOT an option: inline asm is opaque to the
// hazard recogniser, which then leaves out the wait states between an MFMA and a VALU read of its result - tried, Silero V4's
// probabilities came out wrong by 0.5.)
__device__ __forceinline__ float relu1(float v) {
    const int b = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, b > 0 ? b : 0);
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)}; }

__device__ __forceinline__ f32x4 quad_of(const f32x16 &a, int g) {
    switch (g) {
        case 0: return f32x4{a.s0, a.s1, a.s2, a.s3};
        case 1: return f32x4{a.s4, a.s5, a.s6, a.s7};
        case 2: return f32x4{a.s8, a.s9, a.sa, a.sb};
        default: return f32x4{a.sc, a.sd, a.se, a.sf};
    }
}

// write a 32-channel output tile (relu'd) as 8 quad rows starting at row `row0`;
// lane (m,h) owns quads row0 + 2g + h
__device__ __forceinline__ void store_tile_relu(f32x4 *region, int row0, int m, int h, const f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) region[(row0 + 2 * g + h) * QS + m] = relu4(quad_of(acc, g));
}

// v_exp_f32 / v_rcp_f32 / v_sqrt_f32 are 1-ulp hardware ops: |error| of sigmoid/tanh below 5e-7 absolute
__device__ __forceinline__ float sigmoidf_(float v) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * v));
}
__device__ __forceinline__ float tanhf_(float v) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008177792681f * v));
}
// one v_mul + one v_fma (written as an explicit fma: left as re*re + im*im the vectoriser pairs the two products into a
// v_pk_mul_f32 and pays three register copies per magnitude to line the operands up)
__device__ __forceinline__ float mag_(float re, float im) { return __builtin_amdgcn_sqrtf(__builtin_fmaf(re, re, im * im)); }

__device__ __forceinline__ f32x16 acc_of(f32x4 b0, f32x4 b1, f32x4 b2, f32x4 b3) {
    f32x16 a;
    a.s0 = b0.x; a.s1 = b0.y; a.s2 = b0.z; a.s3 = b0.w;
    a.s4 = b1.x; a.s5 = b1.y; a.s6 = b1.z; a.s7 = b1.w;
    a.s8 = b2.x; a.s9 = b2.y; a.sa = b2.z; a.sb = b2.w;
    a.sc = b3.x; a.sd = b3.y; a.se = b3.z; a.sf = b3.w;
    return a;
}

// ---- quad / tile arithmetic as PACKED fp32 (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: two lanes of a register pair per
// instruction, the scalar forms' rounding).  fp32 MFMAs and VALU instructions share the vector pipe on this chip, so every VALU
// instruction not issued is time; left to itself the compiler packs about a fifth of such code and scalarises every subtraction
// (the backend has no packed subtract: the packed add with its negate modifier is written out).  The add / mul helpers are
// compiled WITHOUT contraction: where a caller keeps a product and a sum apart (the loaders' folds: the int16 and float32
// instantiations must round alike) they stay apart after inlining.
typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma clang fp contract(off)
namespace pk {
__device__ __forceinline__ f32x4 cat(f32x2 lo, f32x2 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3); }
// a - b as ONE packed instruction.  The backend has no packed subtract (an fsub of a <2 x float> is split into two v_sub_f32, and
// fma(b, -1, a) is folded back into that fsub), so the -1 is made opaque: v_pk_fma_f32(b, k, a) with k = -1 from an empty asm - the
// product is exact, the one rounding is that of a - b.  NOT written as inline asm (`v_pk_add_f32 ... neg_lo:[0,1] neg_hi:[0,1]`, as
// it was): inline asm is opaque to the hazard recogniser, which then does not insert the wait states an MFMA result needs before a
// VALU instruction reads it - and this helper is applied to accumulators (enc0's Toom-3 interpolation).
__device__ __forceinline__ f32x2 sub2(f32x2 a, f32x2 b) {
    float k = -1.0f;
    asm("" : "+v"(k));
    return __builtin_elementwise_fma(b, f32x2{k, k}, a);
}
__device__ __forceinline__ f32x4 add(f32x4 a, f32x4 b) { return cat(a.lo + b.lo, a.hi + b.hi); }
__device__ __forceinline__ f32x4 sub(f32x4 a, f32x4 b) { return cat(sub2(a.lo, b.lo), sub2(a.hi, b.hi)); }
__device__ __forceinline__ f32x4 mul(f32x4 a, f32x4 b) { return cat(a.lo * b.lo, a.hi * b.hi); }
__device__ __forceinline__ f32x4 fma(f32x4 a, f32x4 b, f32x4 c) {
    return cat(__builtin_elementwise_fma(a.lo, b.lo, c.lo), __builtin_elementwise_fma(a.hi, b.hi, c.hi));
}
__device__ __forceinline__ f32x4 splat(float v) { return f32x4{v, v, v, v}; }
// |re + i im| of a quad: fma(re, re, im * im) as in mag_(), packed, then the four square roots
__device__ __forceinline__ f32x4 mag(f32x4 re, f32x4 im) {
    const f32x4 q = fma(re, re, mul(im, im));
    return f32x4{__builtin_amdgcn_sqrtf(q.x), __builtin_amdgcn_sqrtf(q.y), __builtin_amdgcn_sqrtf(q.z), __builtin_amdgcn_sqrtf(q.w)};
}
// the same on a 32 x 32 tile's 16 accumulator registers, quad by quad
#define VADK_PK16(expr)                                                                                            \
    {                                                                                                              \
        f32x16 r_;                                                                                                 \
        _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) {                                                         \
            const f32x4 q_ = (expr);                                                                               \
            switch (g_) {                                                                                          \
                case 0: r_.s0 = q_.x; r_.s1 = q_.y; r_.s2 = q_.z; r_.s3 = q_.w; break;                             \
                case 1: r_.s4 = q_.x; r_.s5 = q_.y; r_.s6 = q_.z; r_.s7 = q_.w; break;                             \
                case 2: r_.s8 = q_.x; r_.s9 = q_.y; r_.sa = q_.z; r_.sb = q_.w; break;                             \
                default: r_.sc = q_.x; r_.sd = q_.y; r_.se = q_.z; r_.sf = q_.w; break;                            \
            }                                                                                                      \
        }                                                                                                          \
        return r_;                                                                                                 \
    }
// sigmoidf_ / tanhf_ on a quad: the same operations per component (scale, v_exp_f32, 1 +, v_rcp_f32, and tanh's 1 - 2 r as one fma),
// the full-rate ones as packed instructions: half the issue slots of the LSTM cell's non-transcendental part
__device__ __forceinline__ f32x4 exp2_4(f32x4 v) {
    return f32x4{__builtin_amdgcn_exp2f(v.x), __builtin_amdgcn_exp2f(v.y), __builtin_amdgcn_exp2f(v.z), __builtin_amdgcn_exp2f(v.w)};
}
__device__ __forceinline__ f32x4 rcp4(f32x4 v) {
    return f32x4{__builtin_amdgcn_rcpf(v.x), __builtin_amdgcn_rcpf(v.y), __builtin_amdgcn_rcpf(v.z), __builtin_amdgcn_rcpf(v.w)};
}
__device__ __forceinline__ f32x4 sigmoid4(f32x4 v) { return rcp4(add(exp2_4(mul(v, splat(-1.44269504088896341f))), splat(1.0f))); }
__device__ __forceinline__ f32x4 tanh4(f32x4 v) {
    return fma(rcp4(add(exp2_4(mul(v, splat(2.88539008177792681f))), splat(1.0f))), splat(-2.0f), splat(1.0f));
}
__device__ __forceinline__ f32x4 q16(const f32x16 &a, int g) {
    return g == 0 ? f32x4{a.s0, a.s1, a.s2, a.s3} : g == 1 ? f32x4{a.s4, a.s5, a.s6, a.s7}
         : g == 2 ? f32x4{a.s8, a.s9, a.sa, a.sb} : f32x4{a.sc, a.sd, a.se, a.sf};
}
__device__ __forceinline__ f32x16 add16(const f32x16 &a, const f32x16 &b) VADK_PK16(add(q16(a, g_), q16(b, g_)))
__device__ __forceinline__ f32x16 sub16(const f32x16 &a, const f32x16 &b) VADK_PK16(sub(q16(a, g_), q16(b, g_)))
__device__ __forceinline__ f32x16 fma16(const f32x16 &a, float k, const f32x16 &c) VADK_PK16(fma(q16(a, g_), splat(k), q16(c, g_)))
__device__ __forceinline__ f32x16 mul16(const f32x16 &a, float k) VADK_PK16(mul(q16(a, g_), splat(k)))
#undef VADK_PK16
}  // namespace pk
#pragma clang fp contract(fast)

// No instruction may be moved across this point by the compiler's scheduler.  The kernel's
// software pipelining (weights for iteration i+1 are requested before the MFMAs of iteration i
// are issued) only survives hipcc's machine scheduler when it is fenced like this.
#define SB() __builtin_amdgcn_sched_barrier(0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// one 1 KiB weight block: 16 bytes per lane at byte offset voff = lane*16, block index in SGPRs
__device__ __forceinline__ f32x4 ldw(__amdgpu_buffer_rsrc_t rs, int voff, int blk) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, blk * 1024, 0));
}

// ---- fp32-exact products on bf16 MFMAs (the 16-stream kernel's LSTM: vad_layout.h, S_LSTM_X3) ----
// A float x with 24 significant bits is x1 + x2 + x3, each the high half of an fp32 bit pattern: x1 = hi16(x), x2 = hi16(x - x1),
// x3 = x - x1 - x2 (both subtractions are exact, x3 has at most 8 significant bits).  With the weights split the same way on the host,
// the six products x_i w_j with i + j <= 4 on v_mfma_f32_16x16x32_bf16 (products exact, fp32 accumulation) leave out terms of at most
// ~2^-24 |x w|: fp32's own rounding, at 6 x 16 cycles per 16 x 16 x 32 tile instead of 8 x 32 for v_mfma_f32_16x16x4_f32.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// dword of the three B fragments from two consecutive K values a (low half) and b (high half): 4 v_and + 4 v_sub_f32 + 3 v_perm_b32
// = 11 instructions per pair of values, 44 per fragment.  The 16-stream kernel therefore splits an activation ONCE,
// where it is produced (split3_frag / split3_half below), and its consumers read finished pieces from LDS (silero_v5_t16.hip:
// activation planes).
__device__ __forceinline__ void split3_pair(float a, float b, unsigned &p1, unsigned &p2, unsigned &p3) {
    const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
    const float ra = a - __builtin_bit_cast(float, ua & 0xffff0000u), rb = b - __builtin_bit_cast(float, ub & 0xffff0000u);
    const unsigned va = __builtin_bit_cast(unsigned, ra), vb = __builtin_bit_cast(unsigned, rb);
    const float sa = ra - __builtin_bit_cast(float, va & 0xffff0000u), sb = rb - __builtin_bit_cast(float, vb & 0xffff0000u);
    p1 = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
    p2 = __builtin_amdgcn_perm(vb, va, 0x07060302u);
    p3 = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, sb), __builtin_bit_cast(unsigned, sa), 0x07060302u);
}
// dword d (0..3) of the fragments of quads xa (K elements 0..3) and xb (4..7)
__device__ __forceinline__ void split3_dword(f32x4 xa, f32x4 xb, int d, u32x4 *F) {
    const f32x4 x = d < 2 ? xa : xb;
    const float a = (d & 1) ? x.z : x.x, b = (d & 1) ? x.w : x.y;
    unsigned p1, p2, p3;
    split3_pair(a, b, p1, p2, p3);
    F[0][d] = p1; F[1][d] = p2; F[2][d] = p3;
}
// The producer's side of the split.  A wave's two D quads of a lane (stream n, rq) - row tiles rt = 0, 1: channels 32 w + 16 rt +
// 4 rq + i - ARE the K elements 0..3 and 4..7 of lane (n, kq = rq)'s B fragment of K-step s = w, so the lane that computed the
// values cuts them: the three pieces F[0..2] of that fragment, the same numbers split3_dword gives a consumer that reads the fp32
// quads back.
__device__ __forceinline__ void split3_frag(f32x4 xa, f32x4 xb, u32x4 *F) {
#pragma unroll
    for (int d = 0; d < 4; ++d) split3_dword(xa, xb, d, F);
}
// half a fragment (one D quad = K elements 0..3 or 4..7): dwords 0, 1 or 2, 3 of the three pieces
__device__ __forceinline__ void split3_half(f32x4 x, u32x2 *H) {
    unsigned lo[3], hi[3];
    split3_pair(x.x, x.y, lo[0], lo[1], lo[2]);
    split3_pair(x.z, x.w, hi[0], hi[1], hi[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) H[p] = u32x2{lo[p], hi[p]};
}
// one 16 x 16 x 32 tile: A pieces W[0..2], B pieces X[0..2], the six leading products, smallest first
__device__ __forceinline__ f32x4 mfma_x3(const f32x4 *W, const u32x4 *X, f32x4 acc) {
#define VADK_BF(v) __builtin_bit_cast(bf16x8, v)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VADK_BF(W[2]), VADK_BF(X[0]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VADK_BF(W[1]), VADK_BF(X[1]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VADK_BF(W[0]), VADK_BF(X[2]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VADK_BF(W[1]), VADK_BF(X[0]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VADK_BF(W[0]), VADK_BF(X[1]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VADK_BF(W[0]), VADK_BF(X[0]), acc, 0, 0, 0);
#undef VADK_BF
    return acc;
}

// (float) s / d for an int16 s and d = 32767 or 32768, bit for bit the IEEE quotient that numpy's true division gives
// (vad_websocket_server.py:341): q = s * r with r = float(1 / d), then one Newton correction in two fmas.  The FORMULA is
// exhaustively equal over all 65 536 values of s (tools/i16_division_check.py, tests/test_host_logic.py: exact rationals on the
// CPU); the COMPILED code of every loader is held to it by tests/test_gpu_gate_edges.py, which gates at |s / d| itself for the 768
// magnitudes that q alone mis-rounds for d = 32767.  3 instructions instead of the ~10 of the v_div_scale / v_rcp / v_div_fmas /
// v_div_fixup sequence - 64 samples per thread in the V5 kernel.
__device__ __forceinline__ float i16_div(int s, float d, float r) {
    const float x = (float)s;
    const float q = x * r;
    const float e = __builtin_fmaf(-q, d, x);
    return __builtin_fmaf(e, r, q);
}

// ITU-T G.711 in a loader: the four codes of one dword -> decode(code) / 32768 as float32, exactly (every code decodes to an
// int16, and s / 32768 is exact), branch-free, without building the integer: a code IS a small float - sign, 3 exponent bits, 4
// mantissa bits - so its 7 low bits, shifted to bits 19..25, land on a float32's exponent and mantissa fields.
//   mu-law (u = ~b): |s| + 132 = (2 m + 33) << (e + 2) = 1.mmmm1b x 2^(e + 7): fields e | mmmm1 under the exponent base 112 give
//     (|s| + 132) / 2^22; minus 132 / 2^22, times +-128 (the sign from bit 7, u & 0x80 = negative).  The product goes through an
//     fma with +0.0f: both zero codes (0x7F, 0xFF) give +0.0f, as (float)(short)0 does on the int16 path, never -0.0f.
//   A-law (a = b ^ 0x55): |s| = (2 m + 1) << 3 for e = 0, (2 m + 33) << (e + 2) above: fields e | mmmm1 under the exponent base
//     0 are that very number x 2^-134, the e = 0 codes as float32 denormals (the kernels run with float32 denormals on - the
//     compiler's default for gfx9, .amdhsa_float_denorm_mode_32 3); times +-2^119 (a & 0x80 = positive).  No zero code.
// About 6 (mu-law) / 5 (A-law) VALU instructions per sample; tests/test_gpu_g711.py feeds all 256 codes of both laws.
template <bool ALAW>
__device__ __forceinline__ f32x4 g711_quad(uint32_t b) {
    const uint32_t w = b ^ (ALAW ? 0xD5D5D5D5u : 0xFFFFFFFFu);      // low 7 bits: the fields; bit 7 set = negative, for both laws
    auto one = [&](auto kc) -> float {
        constexpr int k = decltype(kc)::value;
        uint32_t x;                                                 // byte k's fields at bits 19..25
        if constexpr (k < 3) x = w << (19 - 8 * k);
        else x = w >> 5;
        const uint32_t sx = w << (24 - 8 * k);                      // byte k's sign at bit 31
        const uint32_t fb = (x & (0x7Fu << 19)) | (ALAW ? 1u << 18 : (112u << 23) | (1u << 18));
        const float f = __builtin_bit_cast(float, fb);
        const float sg = __builtin_bit_cast(float, (sx & 0x80000000u) | (ALAW ? 0x7B000000u : 0x43000000u));   // +-2^119 | +-128
        if constexpr (ALAW) return f * sg;
        else return __builtin_fmaf(sg, f - 0x1.08p-15f, 0.0f);      // 132 / 2^22
    };
    return f32x4{one(std::integral_constant<int, 0>{}), one(std::integral_constant<int, 1>{}),
                 one(std::integral_constant<int, 2>{}), one(std::integral_constant<int, 3>{})};
}

__device__ __forceinline__ f32x4 gate4(f32x4 v, float thr) {
    // utils/audio.py:117-118: np.where(np.abs(x) > thr, x, 0.0); thr < 0 disables the gate
    // branch-free (a uniform branch here would split the caller's basic block and defeat its instruction interleave)
    const bool off = !(thr >= 0.f);
    v.x = ((fabsf(v.x) > thr) | off) ? v.x : 0.f;
    v.y = ((fabsf(v.y) > thr) | off) ? v.y : 0.f;
    v.z = ((fabsf(v.z) > thr) | off) ? v.z : 0.f;
    v.w = ((fabsf(v.w) > thr) | off) ? v.w : 0.f;
    return v;
}

// One aligned quad of sample frames of a scanned block in its wire format, outside the model kernels (scan_cut.hip,
// scan_resample.hip): the loads, the decoders and the channel selection of silero_v5_t16_body.h's loader, restated - the
// instantiations of that file stay the code they were.  FMT: 0 float32, 1 int16 (the divisor is an argument), 2 mu-law, 3 A-law -
// the numbering of silero_v5_t16.hip's loaders (a launcher gets it from wire_fmt, below); CH: interleaved channels of the block.
// No gate: that is the caller's.
template <int FMT, int CH>
struct WireQuad {
    static constexpr bool f32in = FMT == 0, G711 = FMT >= 2;
    static constexpr int qsh = (f32in ? 4 : G711 ? 2 : 3) + (CH == 2 ? 1 : 0);   // a quad of sample frames: 16 / 8 / 4 bytes per channel
    struct XQ2F { u32x4 a, b; };
    // mono: b128 float32, b64 int16, b32 G.711; two channels: two b128, one b128, one b64
    using XQ = std::conditional_t<CH == 2, std::conditional_t<f32in, XQ2F, std::conditional_t<G711, u32x2, u32x4>>,
                                  std::conditional_t<f32in, u32x4, std::conditional_t<G711, uint32_t, u32x2>>>;
    static __device__ __forceinline__ XQ load(__amdgpu_buffer_rsrc_t rs, int off) {
        if constexpr (CH == 2 && f32in)
            return XQ2F{__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0), __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0)};
        else if constexpr ((CH == 2 && G711) || (CH == 1 && !f32in && !G711)) return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
        else if constexpr (G711) return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
        else return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
    }
    // the loader's decode: both channels through the mono decoders, then left | right | (dL + dR) * 0.5f (an add, then a multiply:
    // np.mean(x, axis=1) of the decoded float32 pair)
    static __device__ __forceinline__ f32x4 decode(XQ b, uint32_t mode, float sc, float rsc) {
#pragma clang fp contract(off)
        f32x4 v;
        if constexpr (CH == 2) {
            f32x4 dl, dr;
            if constexpr (G711) {
                dl = g711_quad<FMT == 3>(__builtin_amdgcn_perm(b.y, b.x, 0x06040200u));    // codes L0 L1 L2 L3
                dr = g711_quad<FMT == 3>(__builtin_amdgcn_perm(b.y, b.x, 0x07050301u));
            } else if constexpr (!f32in) {
                dl = f32x4{i16_div((int)(short)(b.x & 0xffffu), sc, rsc), i16_div((int)(short)(b.y & 0xffffu), sc, rsc),
                           i16_div((int)(short)(b.z & 0xffffu), sc, rsc), i16_div((int)(short)(b.w & 0xffffu), sc, rsc)};
                dr = f32x4{i16_div((int)(short)(b.x >> 16), sc, rsc), i16_div((int)(short)(b.y >> 16), sc, rsc),
                           i16_div((int)(short)(b.z >> 16), sc, rsc), i16_div((int)(short)(b.w >> 16), sc, rsc)};
            } else {
                dl = __builtin_bit_cast(f32x4, u32x4{b.a.x, b.a.z, b.b.x, b.b.z});
                dr = __builtin_bit_cast(f32x4, u32x4{b.a.y, b.a.w, b.b.y, b.b.w});
            }
            const bool right = mode == SCAN_RIGHT, mix = mode >= SCAN_MIX;
            const f32x4 mx = pk::mul(pk::add(dl, dr), f32x4{0.5f, 0.5f, 0.5f, 0.5f});
            v.x = mix ? mx.x : right ? dr.x : dl.x;
            v.y = mix ? mx.y : right ? dr.y : dl.y;
            v.z = mix ? mx.z : right ? dr.z : dl.z;
            v.w = mix ? mx.w : right ? dr.w : dl.w;
        } else if constexpr (G711) {
            v = g711_quad<FMT == 3>(b);
        } else if constexpr (!f32in) {
            const int s0 = (int)(short)(b.x & 0xffffu), s1 = (int)(short)(b.x >> 16);
            const int s2 = (int)(short)(b.y & 0xffffu), s3 = (int)(short)(b.y >> 16);
            v = f32x4{i16_div(s0, sc, rsc), i16_div(s1, sc, rsc), i16_div(s2, sc, rsc), i16_div(s3, sc, rsc)};
        } else {
            v = __builtin_bit_cast(f32x4, b);
        }
        return v;
    }
};

// The segment-audio kernels' conversion to int16 PCM.  utils/wav_writer.py:41: np.clip(x * 32767, -32768, 32767).astype(np.int16) -
// one float32 multiply, the clamp, the conversion toward zero (a NaN's result is unspecified there and here)
__device__ __forceinline__ uint32_t pcm16(float x) {
#pragma clang fp contract(off)
    const float v = x * 32767.0f;
    return (uint32_t)(int)fminf(fmaxf(v, -32768.0f), 32767.0f) & 0xffffu;
}

// Output quad o of packed segment audio.  One channel (l): 8 bytes of int16 PCM (OUT 0) or 16 of float32 (OUT 1).  BOTH channels
// kept (l, r): interleaved L0 R0 L1 R1 L2 R2 L3 R3 and twice as wide - one 16-byte store or two.
template <int OUT, bool BOTH>
__device__ __forceinline__ void store_quad(void *out, uint64_t o, f32x4 l, [[maybe_unused]] f32x4 r) {
    if constexpr (!BOTH) {
        if constexpr (OUT == 0)
            static_cast<u32x2 *>(out)[o] = u32x2{pcm16(l.x) | (pcm16(l.y) << 16), pcm16(l.z) | (pcm16(l.w) << 16)};
        else
            static_cast<f32x4 *>(out)[o] = l;
    } else if constexpr (OUT == 0) {
        static_cast<u32x4 *>(out)[o] = u32x4{pcm16(l.x) | (pcm16(r.x) << 16), pcm16(l.y) | (pcm16(r.y) << 16),
                                             pcm16(l.z) | (pcm16(r.z) << 16), pcm16(l.w) | (pcm16(r.w) << 16)};
    } else {
        static_cast<f32x4 *>(out)[2 * o] = f32x4{l.x, r.x, l.y, r.y};
        static_cast<f32x4 *>(out)[2 * o + 1] = f32x4{l.z, r.z, l.w, r.w};
    }
}

// Non-finite input (include/vad_engine.h, VAD_EV_REJECTED): a running maximum of |x| over the raw samples, before the gate, with
// IEEE maximum semantics - a NaN operand makes the result NaN (v_maximum3_f32, the |.| as source modifiers; fmaxf would drop it).
// The frame is rejected when the maximum of its samples is NaN or +Inf: nonfinite(m).
__device__ __forceinline__ float absmax4(float m, f32x4 v) {
    const float a = __builtin_elementwise_maximum(m, __builtin_elementwise_maximum(fabsf(v.x), fabsf(v.y)));
    return __builtin_elementwise_maximum(a, __builtin_elementwise_maximum(fabsf(v.z), fabsf(v.w)));
}
__device__ __forceinline__ bool nonfinite(float m) { return !(m <= 3.40282347e+38f); }

// ---- host side: the launchers' choice of an instantiation ----
// VAD_FMT_* -> WireQuad's FMT (the int16 divisor is an argument of the kernel, not a kernel of its own)
inline int wire_fmt(int fmt) { return fmt == VAD_FMT_F32 ? 0 : fmt == VAD_FMT_ULAW8 ? 2 : fmt == VAD_FMT_ALAW8 ? 3 : 1; }

// launch_variant<N0, N1, ...>(fn, i0, i1, ...): run-time indices i_k in [0, N_k) as compile-time constants - fn(c0, c1, ...) with
// c_k a std::integral_constant<int, i_k>, usable as a template argument; fn launches and returns hipGetLastError().  An index out
// of its range launches nothing: hipErrorInvalidValue.  fn is instantiated for every combination, and for nothing else.
template <class Fn>
hipError_t launch_variant(Fn &&fn) { return fn(); }
template <int N, int... Ns, class Fn, class... Is>
hipError_t launch_variant(Fn &&fn, int i, Is... is);
template <int... Ns, int... K, class Fn, class... Is>
hipError_t launch_variant_(std::integer_sequence<int, K...>, Fn &fn, int i, Is... is) {
    hipError_t r = hipErrorInvalidValue;
    (void)((i == K && (r = launch_variant<Ns...>([&](auto... c) { return fn(std::integral_constant<int, K>{}, c...); }, is...), true)) || ...);
    return r;
}
template <int N, int... Ns, class Fn, class... Is>
hipError_t launch_variant(Fn &&fn, int i, Is... is) { return launch_variant_<Ns...>(std::make_integer_sequence<int, N>{}, fn, i, is...); }

} }  // namespace vadk::dev

