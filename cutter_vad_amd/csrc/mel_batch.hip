// vad_mel_stats / vad_mel_batch: per-segment statistics of a feature matrix [rows][n_mels] and model-ready batches cut out of it
// (include/vad_engine.h: vad_batch; vad_layout.h: MelStatsArgs, MelBatchArgs).  Neither kernel reads audio: the matrix is what
// vadk_seg_mel wrote, resident on the GPU (vad_scan_mel_keep), or the caller's.
//
// vadk_mel_stats.  One workgroup per MELB_STATS_ROWS consecutive rows of one segment, so a long segment is spread over many
// workgroups.  With P = the power of two >= n_mels, thread t owns band t % P and the rows t / P, t / P + 256 / P, ... of the part:
// the loads of a wave run along mel.  It folds the maximum by the bit patterns (melb_max_bits: -0.0 below +0.0) and q = rint(clamp(x,
// -2048, 2048) * 4096) and q * q in 64-bit integers; the threads of a band are summed through LDS, and one thread per band adds the
// part to the segment's sums with 64-bit integer atomics.  The maximum is reduced across the wave, then through LDS, and goes into
// the segment's by the bits: a value with the sign bit clear by a signed integer maximum, one with the sign bit set by an unsigned
// integer minimum - on the float32 bit patterns both move toward the larger value from the -inf the caller stored.  Integer sums
// and a maximum do not depend on the order.
//
// vadk_mel_batch.  One workgroup per (window, tile of 64 or 32 frames), in melb_tile_body:
//   1. the rows of the tile and a halo of 2 deltas rows on either side, with the row index clamped to the SEGMENT, are loaded with
//      the lanes along mel and normalised into LDS - v = (max(x, lo) + shift) * scale - at the odd pitch n_mels | 1.
//   2. deltas == 2: the first differences of all but the outermost two rows on either side go to a second LDS array, each taken at
//      the clamped row's own index, so that a row past the segment's edge repeats the edge's difference.
//   3. the cells: statics out of the first array, first differences out of it as well (deltas == 1) or out of the second, second
//      differences out of the second; pad cells for frames past the window's rows.  Channel-major output runs the lanes along
//      time - float32 one frame per lane, 16-bit types two frames per lane as one packed 4-byte store and two channels per wave -
//      and time-major output runs them along the channels.
// Every cell of every window is written by exactly one lane, nothing is accumulated: two runs give the same bytes.
//
// vadk_mel_batch_packed.  Several pieces of segments per window (vad_mel_batch_packed): one workgroup per entry of the host's work
// list (vad_layout.h: MelPackWork) - a tile of a piece, stored at the piece's offset in its window, or a pad run of whole quads that
// no piece owns - through the same body (melb_tile_body) with the WINDOW's lo, shift and scale.  A piece's workgroups own the cells
// up to the next multiple of 4 behind its last row, so a packed 16-bit pair or a float32 quad never holds cells of two workgroups.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"

// the header's rule is a sequence of float32 operations, each rounded on its own
#pragma clang fp contract(off)

using namespace vadk;

namespace {

__device__ __forceinline__ float melb_delta(float m2, float m1, float p1, float p2) { return ((p1 - m1) + 2.0f * (p2 - m2)) * 0.1f; }

// the larger of two float32 by their bits, -0.0 below +0.0: among patterns with the sign clear the larger one, among those with it
// set the smaller one
__device__ __forceinline__ uint32_t melb_max_bits(uint32_t x, uint32_t y) {
    const bool xn = x >> 31, yn = y >> 31;
    return (xn != yn ? xn : xn ? y < x : y > x) ? y : x;
}

__device__ __forceinline__ uint16_t melb_f16(float v) { return __half_as_ushort(__float2half_rn(v)); }

}  // namespace

__global__ void __launch_bounds__(MELB_THREADS) vadk_mel_stats(const MelStatsArgs a) {
    __shared__ long long s_sum[MELB_THREADS];
    __shared__ unsigned long long s_sq[MELB_THREADS];
    __shared__ uint32_t s_max[MELB_THREADS / 64];
    const MelStatsWork w = a.work[blockIdx.x];
    uint32_t P = 1;
    while (P < a.n_mels) P <<= 1;
    const uint32_t j = threadIdx.x & (P - 1u), r0 = threadIdx.x / P, R = MELB_THREADS / P;
    long long sum = 0;
    unsigned long long sq = 0;
    uint32_t mx = 0xff800000u;                                         // -inf
    if (j < a.n_mels) {
        const float *x = a.x + (size_t)w.row0 * a.n_mels + j;
        for (uint32_t r = r0; r < w.nrows; r += R) {
            const float v = x[(size_t)r * a.n_mels];
            mx = melb_max_bits(mx, __float_as_uint(v));
            const long long q = melb_q(v);
            sum += q;
            sq += (unsigned long long)(q * q);
        }
    }
    for (int off = 32; off > 0; off >>= 1) mx = melb_max_bits(mx, (uint32_t)__shfl_xor((int)mx, off));
    s_sum[threadIdx.x] = sum;
    s_sq[threadIdx.x] = sq;
    if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x < P && j < a.n_mels) {
        for (uint32_t k = 1; k < R; ++k) {
            sum += s_sum[threadIdx.x + k * P];
            sq += s_sq[threadIdx.x + k * P];
        }
        if (a.sum_out) atomicAdd(reinterpret_cast<unsigned long long *>(a.sum_out) + (size_t)w.seg * a.n_mels + j, (unsigned long long)sum);
        if (a.sumsq_out) atomicAdd(a.sumsq_out + (size_t)w.seg * a.n_mels + j, sq);
    }
    if (a.max_out && threadIdx.x == 0) {
        for (uint32_t k = 1; k < MELB_THREADS / 64; ++k) mx = melb_max_bits(mx, s_max[k]);
        // toward the larger value on the patterns themselves, from the -inf the caller stored
        if (mx >> 31) atomicMin(reinterpret_cast<unsigned int *>(a.max_out) + w.seg, mx);
        else atomicMax(reinterpret_cast<int *>(a.max_out) + w.seg, (int)mx);
    }
}

// The one body of both batch kernels.  A workgroup owns frames t0 .. t0 + nt - 1 of window wi: the first nv of them show rows
// row0 .. row0 + nv - 1 of the segment of M rows whose first row in the matrix is seg_row, the rest are pad cells; lo, shift and
// scale are taken at index aff (vadk_mel_batch: the segment; vadk_mel_batch_packed: the window).
// DT: VAD_BATCH_F32 / F16 / BF16.  Dynamic LDS: melb_lds_floats(n_mels, deltas, tile) floats
template <int DT>
__device__ __forceinline__ void melb_tile_body(const MelBatchArgs &a, float *melb_lds, uint32_t wi, uint32_t t0, uint32_t nt, uint32_t nv,
                                               uint64_t seg_row0, uint32_t M, uint32_t row0, uint32_t aff) {
    const uint32_t nm = a.n_mels, pitch = melb_pitch(nm), H = 2u * a.deltas, L = a.tile + 2u * H, C = nm * (a.deltas + 1u);
    const float lo = a.lo[aff];
    const float *shift = a.shift + (size_t)(a.per_seg ? aff : 0u) * nm, *scale = a.scale + (size_t)(a.per_seg ? aff : 0u) * nm;
    float *V = melb_lds, *D = melb_lds + (size_t)L * pitch - 2u * pitch;          // D's row l lies at D + l * pitch, l = 2 .. L - 3
    // LDS row l holds segment row clamp(base + l, 0, M - 1); a tile with a row has base + H <= M - 1 and base >= -H
    const int64_t base = (int64_t)row0 - H, last = (int64_t)M - 1;
    auto seg_row = [&](int64_t s) -> int64_t { return s < 0 ? 0 : s > last ? last : s; };

    if (nv) {
        // 1. rows l = 0 .. nv + 2 H - 1 (the rest of the tile is pad cells)
        const uint32_t nl = nv + 2u * H, step_r = MELB_THREADS / nm, step_j = MELB_THREADS % nm;
        uint32_t l = threadIdx.x / nm, j = threadIdx.x % nm;
        while (l < nl) {
            const float x = a.x[((size_t)seg_row0 + (size_t)seg_row(base + l)) * nm + j];
            V[l * pitch + j] = (fmaxf(x, lo) + shift[j]) * scale[j];
            l += step_r;
            j += step_j;
            if (j >= nm) { j -= nm; ++l; }
        }
        __syncthreads();
        // 2. first differences of rows l = 2 .. nl - 3 at the clamped row's own index u: V's row of segment row p is p - base
        if (a.deltas == 2u) {
            l = 2u + threadIdx.x / nm;
            j = threadIdx.x % nm;
            while (l < nl - 2u) {
                const int64_t u = seg_row(base + l);
                const float *c = V + j;
                D[l * pitch + j] = melb_delta(c[(seg_row(u - 2) - base) * pitch], c[(seg_row(u - 1) - base) * pitch],
                                              c[(seg_row(u + 1) - base) * pitch], c[(seg_row(u + 2) - base) * pitch]);
                l += step_r;
                j += step_j;
                if (j >= nm) { j -= nm; ++l; }
            }
            __syncthreads();
        }
    }

    // 3. the value of cell (channel ch, frame t0 + tt)
    auto cell = [&](uint32_t ch, uint32_t tt) -> float {
        const uint32_t k = ch / nm, j = ch - k * nm;
        if (tt >= nv) {
            if (k) return 0.0f;
            return a.pad_mode == VAD_BATCH_PAD_FEATURE ? (fmaxf(a.pad_value, lo) + shift[j]) * scale[j] : a.pad_value;
        }
        const int64_t u = (int64_t)row0 + tt;
        if (k == 0u) return V[(H + tt) * pitch + j];
        const float *c = (a.deltas == 2u ? D : V) + j;
        if (k == 1u && a.deltas == 2u) return c[(H + tt) * pitch];
        return melb_delta(c[(seg_row(u - 2) - base) * pitch], c[(seg_row(u - 1) - base) * pitch], c[(seg_row(u + 1) - base) * pitch],
                          c[(seg_row(u + 2) - base) * pitch]);
    };
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (a.layout == VAD_BATCH_TIME_MAJOR) {
        // [w][t][C]: the lanes along the channels
        for (uint32_t tt = wave; tt < nt; tt += MELB_THREADS / 64) {
            const size_t o = ((size_t)wi * a.frames + t0 + tt) * C;
            for (uint32_t ch = lane; ch < C; ch += 64u) {
                const float v = cell(ch, tt);
                if (DT == VAD_BATCH_F32) static_cast<float *>(a.out)[o + ch] = v;
                else static_cast<uint16_t *>(a.out)[o + ch] = DT == VAD_BATCH_F16 ? melb_f16(v) : melb_bf16(__float_as_uint(v));
            }
        }
        return;
    }
    // [w][C][t]: the lanes along time
    if (DT == VAD_BATCH_F32) {
        for (uint32_t ch = wave; ch < C; ch += MELB_THREADS / 64) {
            if (lane >= nt) continue;
            static_cast<float *>(a.out)[((size_t)wi * C + ch) * a.frames + t0 + lane] = cell(ch, lane);
        }
        return;
    }
    // frames 2 (lane & 31) and + 1 of channel ch + (lane >> 5): frames and tile are multiples of 4, so a pair is whole and aligned
    const uint32_t tt = 2u * (lane & 31u);
    for (uint32_t ch = 2u * wave + (lane >> 5); ch < C; ch += 2u * (MELB_THREADS / 64)) {
        if (tt >= nt) continue;
        const float v0 = cell(ch, tt), v1 = cell(ch, tt + 1u);
        const uint32_t b0 = DT == VAD_BATCH_F16 ? melb_f16(v0) : melb_bf16(__float_as_uint(v0));
        const uint32_t b1 = DT == VAD_BATCH_F16 ? melb_f16(v1) : melb_bf16(__float_as_uint(v1));
        *reinterpret_cast<uint32_t *>(static_cast<uint16_t *>(a.out) + ((size_t)wi * C + ch) * a.frames + t0 + tt) = b0 | (b1 << 16);
    }
}

template <int DT>
__global__ void __launch_bounds__(MELB_THREADS) vadk_mel_batch(const MelBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) float melb_lds[];
    const uint32_t tiles = (a.frames + a.tile - 1u) / a.tile;
    const uint32_t wi = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * a.tile;
    const MelBatchWin w = a.win[wi];
    const uint32_t nt = a.frames - t0 < a.tile ? a.frames - t0 : a.tile;          // frames of this tile
    const uint32_t nv = w.nrows > t0 ? (w.nrows - t0 < nt ? w.nrows - t0 : nt) : 0u;   // ... that hold a row of the window
    melb_tile_body<DT>(a, melb_lds, wi, t0, nt, nv, w.seg_row, w.M, w.row0 + t0, w.seg);
}

// one workgroup per entry of the host's work list: a tile of a piece, or a pad run
template <int DT>
__global__ void __launch_bounds__(MELB_THREADS) vadk_mel_batch_packed(const MelPackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float melb_lds[];
    const MelPackWork w = a.work[blockIdx.x];
    melb_tile_body<DT>(a.b, melb_lds, w.window, w.t0, w.nt, w.nv, w.seg_row, w.M, w.row0, w.window);
}

extern "C" hipError_t vadk_launch_mel_stats(const MelStatsArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    hipLaunchKernelGGL(vadk_mel_stats, dim3(a->nwork), dim3(MELB_THREADS), 0, stream, *a);
    return hipGetLastError();
}

extern "C" hipError_t vadk_launch_mel_batch(const MelBatchArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nw == 0) return hipSuccess;
    if (a->tile != melb_tile(a->n_mels, a->deltas)) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (size_t)melb_lds_floats(a->n_mels, a->deltas, a->tile);
    const uint32_t tiles = (a->frames + a->tile - 1u) / a->tile;
#define VADK_MELB(DT)                                                                                                               \
    if (a->dtype == DT) {                                                                                                           \
        if (lds > 48u * 1024u) {                                                                                                    \
            const hipError_t r = hipFuncSetAttribute(reinterpret_cast<const void *>(&vadk_mel_batch<DT>),                           \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                         \
            if (r != hipSuccess) return r;                                                                                          \
        }                                                                                                                           \
        hipLaunchKernelGGL((vadk_mel_batch<DT>), dim3(a->nw * tiles), dim3(MELB_THREADS), lds, stream, *a);                         \
        return hipGetLastError();                                                                                                   \
    }
    VADK_MELB(VAD_BATCH_F32) VADK_MELB(VAD_BATCH_F16) VADK_MELB(VAD_BATCH_BF16)
#undef VADK_MELB
    return hipErrorInvalidValue;
}

extern "C" hipError_t vadk_launch_mel_batch_packed(const MelPackArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    if (a->b.tile != melb_tile(a->b.n_mels, a->b.deltas)) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (size_t)melb_lds_floats(a->b.n_mels, a->b.deltas, a->b.tile);
#define VADK_MELP(DT)                                                                                                               \
    if (a->b.dtype == DT) {                                                                                                         \
        if (lds > 48u * 1024u) {                                                                                                    \
            const hipError_t r = hipFuncSetAttribute(reinterpret_cast<const void *>(&vadk_mel_batch_packed<DT>),                    \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                         \
            if (r != hipSuccess) return r;                                                                                          \
        }                                                                                                                           \
        hipLaunchKernelGGL((vadk_mel_batch_packed<DT>), dim3(a->nwork), dim3(MELB_THREADS), lds, stream, *a);                       \
        return hipGetLastError();                                                                                                   \
    }
    VADK_MELP(VAD_BATCH_F32) VADK_MELP(VAD_BATCH_F16) VADK_MELP(VAD_BATCH_BF16)
#undef VADK_MELP
    return hipErrorInvalidValue;
}
