// vad_scan_levels: energy, peak and clipped samples of finished segments, reduced out of a scanned block in its wire format
// (include/vad_engine.h: vad_level).  The levels of a segment are statistics of exactly the float32 values that vadk_scan_cut with
// the sample range once (VAD_CUT_RANGE) and float32 output would write for it: the same tables (vad_layout.h: CutSeg / CutWork /
// CutArgs - one workgroup per CUT_WG_QUADS quads of ONE segment), the same loads, decoders, channel selection and gate (vadk_device.h:
// WireQuad, gate4).  Where that kernel stores a quad, this one folds it into three integers per thread:
//   energy  sum of rint(min(|x|, 1)^2 * 2^32) - the header's min(rint(x * x * 2^32), 2^32): the clamp commutes with the monotone
//           square and rounding, and |x| >= 1 gives 2^32 exactly.  y = min(|x|, 1) * 65536 is exact in float32 (a power of two), y * y
//           is exact in float64 (48 bits), v_rndne_f64 rounds to nearest-even.  A thread adds its <= 16 terms (each <= 2^32) in
//           float64 - integers below 2^53, so that sum is exact too - and converts ONCE to uint64; everything after is integer adds.
//   peak    the maximum of the bit patterns of |x|: for finite values that is max |x|; +Inf beats them, a NaN pattern beats +Inf.
//   clipped |x| >= clip_thresh, compared in float32.
// Integers, so the record does not depend on the order in which lanes, waves and workgroups arrive: two runs give the same bytes.
// Registers -> wave (xor shuffles) -> the workgroup's waves through LDS -> one atomic per field and workgroup on the segment's
// record, which the host zeroed (hipMemsetAsync) ahead of the launch.  No float atomics.
// vad_scan_moments (vadk_seg_moments, below the levels' kernel): a segment's sum and energy by the same skeleton, for its mean and variance.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

static_assert(sizeof(vad_level) == 16, "vad_level layout");

namespace {

struct Lv {
    unsigned long long e;
    uint32_t peak, clipped;
};

__device__ __forceinline__ void level1(float x, float clip, double &e, uint32_t &peak, uint32_t &clipped) {
#pragma clang fp contract(off)
    const float ax = fabsf(x);
    const uint32_t bits = __builtin_bit_cast(uint32_t, ax);
    peak = bits > peak ? bits : peak;
    clipped += ax >= clip ? 1u : 0u;
    const double y = (double)(fminf(ax, 1.0f) * 65536.0f);
    e += __builtin_rint(y * y);
}

__device__ __forceinline__ Lv wave_sum(Lv v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v.e, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v.e >> 32), m);
        const uint32_t pk = (uint32_t)__shfl_xor((int)v.peak, m), cl = (uint32_t)__shfl_xor((int)v.clipped, m);
        v.e += ((unsigned long long)hi << 32) | lo;
        v.peak = pk > v.peak ? pk : v.peak;
        v.clipped += cl;
    }
    return v;
}

}  // namespace

// a.out: vad_level[segments of a.segs], zeroed.  a.frame_shift is 31 (the range once), a.out_fmt and CutSeg::quad_out are not read.
// The loads are the cut's - all CUT_PASSES of a thread requested before the first is decoded, UNCONDITIONALLY: a lane behind its
// segment's last quad reads some quad of the block (a neighbour's samples, or 0 past the descriptor's range) and must fold NOTHING
// of it - the guard sits in front of the fold as it sits in front of the cut's store.  A wave without a quad of the segment (a
// segment's last workgroup is mostly such waves) carries zeros, the identity of all three reductions, into LDS.
template <int FMT, int CH>
__global__ void __launch_bounds__(CUT_THREADS) vadk_seg_levels(const CutArgs a, const float clip) {
    using In = WireQuad<FMT, CH>;
    constexpr int NW = CUT_THREADS / 64;
    __shared__ Lv part[NW];
    const CutWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
    typename In::XQ x[CUT_PASSES];
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t oq = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        // unsigned 32-bit: the argument check keeps every quad of a segment inside the block, which is under 2 GiB
        x[p] = In::load(rs, (int)((qin + oq) << In::qsh));
    }
    double e = 0.0;
    Lv t{0ull, 0u, 0u};
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t oq = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        if (oq >= sg.nquads) continue;
        const f32x4 v = gate4(In::decode(x[p], mode, sc, rsc), a.thresh);
        level1(v.x, clip, e, t.peak, t.clipped);
        level1(v.y, clip, e, t.peak, t.clipped);
        level1(v.z, clip, e, t.peak, t.clipped);
        level1(v.w, clip, e, t.peak, t.clipped);
    }
    t.e = (unsigned long long)e;          // an integer <= 16 * 2^32, exact
    t = wave_sum(t);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) part[wave] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 1; k < NW; ++k) {
        t.e += part[k].e;
        t.peak = part[k].peak > t.peak ? part[k].peak : t.peak;
        t.clipped += part[k].clipped;
    }
    vad_level *rec = static_cast<vad_level *>(a.out) + w.seg;
    atomicAdd(reinterpret_cast<unsigned long long *>(&rec->energy_q32), t.e);
    atomicMax(reinterpret_cast<unsigned int *>(&rec->peak), t.peak);
    atomicAdd(reinterpret_cast<unsigned int *>(&rec->clipped), t.clipped);
}

// vad_scan_moments: the sum and the energy of the same values, for a mean and a variance (include/vad_engine.h: vad_moments).
//   sum     sum of rint(clamp(x, -1, 1) * 2^31): the product is exact in float64, v_rndne_f64 rounds to nearest-even; a thread's <= 16
//           terms (each |.| <= 2^31) add up exactly in float64 and are converted ONCE to int64.
//   energy  vad_level's energy_q32, by level1's own expression: the two calls agree on it byte for byte.
// a.out: vad_moments[segments of a.segs], zeroed.  The loads, the guard in front of the fold and the reduction are vadk_seg_levels':
// registers -> wave -> LDS -> one 64-bit integer atomic per field and workgroup (the signed sum as its two's complement).
static_assert(sizeof(vad_moments) == 16, "vad_moments layout");

template <int FMT, int CH>
__global__ void __launch_bounds__(CUT_THREADS) vadk_seg_moments(const CutArgs a) {
    using In = WireQuad<FMT, CH>;
    constexpr int NW = CUT_THREADS / 64;
    __shared__ unsigned long long part[NW][2];
    const CutWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
    typename In::XQ x[CUT_PASSES];
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t oq = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        x[p] = In::load(rs, (int)((qin + oq) << In::qsh));
    }
    double s = 0.0, e = 0.0;
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t oq = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        if (oq >= sg.nquads) continue;
        const f32x4 v = gate4(In::decode(x[p], mode, sc, rsc), a.thresh);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
            const float xk = v[k];
            s += __builtin_rint((double)fminf(fmaxf(xk, -1.0f), 1.0f) * 2147483648.0);
            const double y = (double)(fminf(fabsf(xk), 1.0f) * 65536.0f);
            e += __builtin_rint(y * y);
        }
    }
    unsigned long long ts = (unsigned long long)(long long)s, te = (unsigned long long)e;      // integers, exact
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t slo = (uint32_t)__shfl_xor((int)(uint32_t)ts, m), shi = (uint32_t)__shfl_xor((int)(uint32_t)(ts >> 32), m);
        const uint32_t elo = (uint32_t)__shfl_xor((int)(uint32_t)te, m), ehi = (uint32_t)__shfl_xor((int)(uint32_t)(te >> 32), m);
        ts += ((unsigned long long)shi << 32) | slo;
        te += ((unsigned long long)ehi << 32) | elo;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = ts;
        part[wave][1] = te;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 1; k < NW; ++k) {
        ts += part[k][0];
        te += part[k][1];
    }
    vad_moments *rec = static_cast<vad_moments *>(a.out) + w.seg;
    atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum_q31), ts);
    atomicAdd(reinterpret_cast<unsigned long long *>(&rec->energy_q32), te);
}

extern "C" hipError_t vadk_launch_seg_moments(const CutArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2>([&](auto F, auto C) {
        hipLaunchKernelGGL((vadk_seg_moments<F, C + 1>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1);
}

extern "C" hipError_t vadk_launch_seg_levels(const CutArgs *a, float clip, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2>([&](auto F, auto C) {
        hipLaunchKernelGGL((vadk_seg_levels<F, C + 1>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a, clip);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1);
}
