// vad_segments_device / vad_scan_segments: the CSR event arrays a scan left in device memory, turned into a packed, ordered table of
// finished segments (vad_layout.h: SegRecord / SegArgs; include/vad_engine.h: vad_segment).  Flat index k is an END iff
// (events[k] & 0x82) == 0x02; the records come in ascending k, and that order does not depend on which workgroup runs when:
//   count  - a workgroup counts the ENDs of SEG_WG_FRAMES consecutive frames (16 event bytes per thread, one 16-byte load through a
//            buffer descriptor whose range ends with the 16-byte line of index total - 1: loads behind it read as 0, and the bytes
//            of that line behind `total` are masked by index);
//   prefix - ONE workgroup turns the chunk counts into their exclusive prefix, SEG_THREADS chunks per round, and writes the total;
//   fill   - the count pass again, then every END takes the position (chunk prefix) + (ENDs of the waves below, through LDS) +
//            (ENDs of the lanes below: one wave64 ballot per byte position, counted below the lane) + (ENDs of its own bytes below);
//   stats  - one wave per written record strides over the segment's frames; the mean's sum is fixed point, so it is exact in any order.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"

using namespace vadk;

static_assert(sizeof(vad_segment) == sizeof(SegRecord) && offsetof(vad_segment, item) == offsetof(SegRecord, item) &&
              offsetof(vad_segment, first_frame) == offsetof(SegRecord, first_frame) && offsetof(vad_segment, nframes) == offsetof(SegRecord, nframes) &&
              offsetof(vad_segment, counted) == offsetof(SegRecord, counted) && offsetof(vad_segment, mean_prob) == offsetof(SegRecord, mean_prob) &&
              offsetof(vad_segment, max_prob) == offsetof(SegRecord, max_prob), "the header's record is the kernel's");
static_assert((SEG_EV_MASK == (VAD_EV_END | VAD_EV_REJECTED)) && SEG_EV_END == VAD_EV_END, "the END rule is the header's");

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int SEG_WAVES = SEG_THREADS / 64;

// four event bytes -> bit i = byte i is an END
__device__ __forceinline__ uint32_t end_nibble(uint32_t w) {
    const uint32_t y = (w & (SEG_EV_MASK * 0x01010101u)) ^ (SEG_EV_END * 0x01010101u);     // a byte is 0 iff it is an END
    const uint32_t e = ~((y >> 7) | (y >> 1)) & 0x01010101u;
    return (e * 0x01020408u) >> 24;             // bits 0, 8, 16, 24 -> bits 24 .. 27: no two partial products meet
}

// the ENDs among this thread's 16 frames, from flat index f0 on: bit j = frame f0 + j
__device__ __forceinline__ uint32_t end_mask(const SegArgs &a, uint32_t f0) {
    // the range ends with the 16-byte line that holds the last event (the array is 16-byte aligned, so that line lies in its pages;
    // a load is inside the range or outside it as a whole, whatever the hardware checks per dword): lines behind it read as 0
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.events), 0, (int)((a.total + 15u) & ~15u), 0x00020000);
    const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)f0, 0, 0);
    uint32_t m = end_nibble(x.x) | (end_nibble(x.y) << 4) | (end_nibble(x.z) << 8) | (end_nibble(x.w) << 12);
    // frames of no item: behind the last one (the bytes that share the tail's last dword) and before the first
    const uint32_t valid = a.total > f0 ? min(a.total - f0, 16u) : 0u;
    m &= (1u << valid) - 1u;
    const uint32_t skip = a.first > f0 ? min(a.first - f0, 16u) : 0u;
    return m & ~((1u << skip) - 1u);
}

}  // namespace

template <bool FILL>
__global__ void __launch_bounds__(SEG_THREADS) vadk_seg_pass(const SegArgs a) {
    __shared__ uint32_t wave_ends[SEG_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t f0 = blockIdx.x * (uint32_t)SEG_WG_FRAMES + tid * 16u;      // nchunks <= 2^19: below 2^31 + SEG_WG_FRAMES
    const uint32_t m = end_mask(a, f0);
    uint32_t below = 0, inwave = 0;
    if (__ballot(m != 0u) != 0ull) {            // most waves of a recording see no END
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long b = __ballot(((m >> j) & 1u) != 0u);
            below += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            inwave += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0) wave_ends[wave] = inwave;
    __syncthreads();
    if constexpr (!FILL) {
        if (tid == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int w = 0; w < SEG_WAVES; ++w) all += wave_ends[w];
            a.chunk[blockIdx.x] = all;
        }
    } else {
        uint32_t pos = a.chunk[blockIdx.x] + below;
#pragma unroll
        for (int w = 0; w < SEG_WAVES; ++w) pos += (uint32_t)w < wave ? wave_ends[w] : 0u;
        for (uint32_t mm = m; mm != 0u; mm &= mm - 1u, ++pos) {
            if (pos >= a.seg_cap) break;
            const uint32_t k = f0 + (uint32_t)__builtin_ctz(mm);
            // the last item with out_start[i] <= k: first <= k < total, so the answer lies in 0 .. n - 1 and owns frame k
            int32_t lo = 0, hi = a.n;
            while (hi - lo > 1) {
                const int32_t mid = lo + ((hi - lo) >> 1);
                if ((uint32_t)a.out_start[mid] <= k) lo = mid; else hi = mid;
            }
            const uint32_t e = k - (uint32_t)a.out_start[lo], L = (uint32_t)a.seg_frames[k];
            SegRecord *r = a.segs + pos;
            r->item = lo;
            r->first_frame = (int32_t)(e - L + 1u);
            r->nframes = (int32_t)L;
        }
    }
}

__global__ void __launch_bounds__(SEG_THREADS) vadk_seg_prefix(const SegArgs a) {
    __shared__ uint32_t wave_sum[SEG_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;                         // at most `total` ENDs: below 2^31
    for (uint32_t c0 = 0; c0 < a.nchunks; c0 += SEG_THREADS) {
        const uint32_t i = c0 + tid;
        const uint32_t v = i < a.nchunks ? a.chunk[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(inc, d);
            if ((int)lane >= d) inc += u;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t under = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SEG_WAVES; ++w) {
            const uint32_t s = wave_sum[w];
            under += (uint32_t)w < wave ? s : 0u;
            all += s;
        }
        if (i < a.nchunks) a.chunk[i] = carry + under + inc - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *a.nsegs = (long long)carry;
}

// the frames max(first_frame, 0) .. e of the record's item whose events have VAD_EV_REJECTED clear: their number, their maximum and
// (float)((double)S / ((double)counted * 2^30)) with S = the sum of (int64) rint((double)p * 2^30).  Every index lies in the item:
// 0 <= t <= e, whatever seg_frames held.
__global__ void __launch_bounds__(SEG_THREADS) vadk_seg_stats(const SegArgs a) {
    const long long all = *a.nsegs;
    const uint32_t nrec = all < (long long)a.seg_cap ? (uint32_t)all : a.seg_cap;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x * (uint32_t)SEG_WAVES + wave; r < nrec; r += gridDim.x * (uint32_t)SEG_WAVES) {
        const int32_t first = a.segs[r].first_frame;
        const uint32_t base = (uint32_t)a.out_start[a.segs[r].item];
        const uint32_t e = (uint32_t)first + (uint32_t)a.segs[r].nframes - 1u;
        int32_t c = 0;
        long long S = 0;
        float mx = -INFINITY;
        for (uint32_t t = (first > 0 ? (uint32_t)first : 0u) + lane; t <= e; t += 64u) {
            const float p = a.probs[base + t];
            if ((a.events[base + t] & VAD_EV_REJECTED) == 0) {
                c += 1;
                S += (long long)rint((double)p * (double)(1ll << SEG_PROB_SHIFT));
                mx = fmaxf(mx, p);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            c += __shfl_xor(c, d);
            S += __shfl_xor(S, d);
            mx = fmaxf(mx, __shfl_xor(mx, d));
        }
        if (lane == 0) {
            a.segs[r].counted = c;
            a.segs[r].mean_prob = c > 0 ? (float)((double)S / ((double)c * (double)(1ll << SEG_PROB_SHIFT))) : 0.0f;
            a.segs[r].max_prob = c > 0 ? mx : 0.0f;
        }
    }
}

extern "C" hipError_t vadk_launch_scan_segments(const SegArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    hipError_t r = hipSuccess;
    if (a->nchunks) {
        hipLaunchKernelGGL((vadk_seg_pass<false>), dim3(a->nchunks), dim3(SEG_THREADS), 0, stream, *a);
        if ((r = hipGetLastError()) != hipSuccess) return r;
    }
    hipLaunchKernelGGL(vadk_seg_prefix, dim3(1), dim3(SEG_THREADS), 0, stream, *a);      // no chunk: the total, 0
    if ((r = hipGetLastError()) != hipSuccess) return r;
    if (a->nchunks == 0 || a->seg_cap == 0) return hipSuccess;
    hipLaunchKernelGGL((vadk_seg_pass<true>), dim3(a->nchunks), dim3(SEG_THREADS), 0, stream, *a);
    if ((r = hipGetLastError()) != hipSuccess) return r;
    const uint32_t most = a->seg_cap < a->total ? a->seg_cap : a->total;
    const uint32_t blocks = (most + SEG_WAVES - 1) / SEG_WAVES;
    hipLaunchKernelGGL(vadk_seg_stats, dim3(blocks < 2048u ? blocks : 2048u), dim3(SEG_THREADS), 0, stream, *a);
    return hipGetLastError();
}

// the statistics alone, for a table whose item, first_frame and nframes another file's kernels wrote (csrc/scan_resegment.hip): the
// first min(*a->nsegs, a->seg_cap) records of a->segs, from a->events, a->probs and a->out_start; `most` bounds that number on the
// host (the grid; the kernel strides over whatever the count turns out to be)
extern "C" hipError_t vadk_launch_seg_stats(const SegArgs *a, uint32_t most, hipStream_t stream) {
    (void)hipGetLastError();
    if (most == 0 || a->seg_cap == 0) return hipSuccess;
    const uint32_t blocks = (most + SEG_WAVES - 1) / SEG_WAVES;
    hipLaunchKernelGGL(vadk_seg_stats, dim3(blocks < 2048u ? blocks : 2048u), dim3(SEG_THREADS), 0, stream, *a);
    return hipGetLastError();
}
