// vad_refine_device / vad_scan_refine: a segment table refined on the GPU by the rule of include/vad_engine.h's vad_refine - clip,
// merge, drop, pad, split - with the per-frame probabilities that a scan left in device memory deciding where a long segment is cut
// (vad_layout.h: RefineArgs).  The records come in item order, then frame order, whatever the GPU's scheduling: count, prefix, fill.
//   heads  - first[i] = the position of the first record that names item i behind one that does not: a thread per table position,
//            atomicMin on the item's word (the minimum does not depend on who comes first; no position of the output is an atomic's);
//   count  - a thread per item walks the item's run of records, and its tail, through steps 1 - 4 of the rule with one group of
//            look-ahead (a group's padding needs its neighbour), counting the pieces of step 5 into cnt[i];
//   prefix - ONE workgroup turns cnt into its exclusive prefix and writes the total;
//   fill   - the walk again, writing piece j of item i at cnt[i] + j, dropped at seg_cap or above, with the NOMINAL cuts of step 5;
//   cuts   - one wave per written record: an end that is a boundary of step 5 moves to the frame of its window with the smallest
//            probability among those whose event byte has VAD_EV_REJECTED clear - a 64-bit key of the probability's bits (probabilities
//            are not negative: their bit patterns order as integers) above the frame number, min-reduced over the wave, so ties go to
//            the lowest frame; a rejected frame's key is all ones, and a window of nothing else leaves the nominal cut.  A record
//            searches both of its ends itself: the window of a boundary is read twice, and no record waits for another;
//   stats  - csrc/scan_segments.hip's vadk_seg_stats over the written records (vadk_launch_seg_stats), from the engine.
// Nothing read from device memory is trusted: a record's frames are clipped into its item before anything is computed from them, a
// run ends where the item column changes, every grid comes from in_cap, n and seg_cap, and counts are 64 bits wide.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "sm_device.h"
#include "vad_layout.h"

using namespace vadk;

static_assert(EV_REJECTED == VAD_EV_REJECTED, "the frames a cut avoids are the header's");

namespace {

constexpr int REFINE_WAVES = REFINE_THREADS / 64;

__device__ __forceinline__ uint32_t refine_rows(const RefineArgs &a) {
    const long long m = *a.nsegs_in;
    return m < 0 ? 0u : m < (long long)a.in_cap ? (uint32_t)m : a.in_cap;
}

// one item's walk.  `cur` = the group that records still join, `held` = the last group that survived the drop: it is written when
// the next survivor (or the end of the item) has settled the padding behind it.
template <bool FILL>
struct RefineWalk {
    const RefineArgs &a;
    int32_t item, nf;
    unsigned long long at;          // FILL: the position of the next piece; else: the pieces so far
    bool have_cur = false, have_held = false;
    int32_t cs = 0, ce = 0;         // cur, clipped
    int32_t he = 0, hps = 0;        // held: its end and its padded start

    __device__ __forceinline__ RefineWalk(const RefineArgs &a_, int32_t item_, int32_t nf_, unsigned long long at_) : a(a_), item(item_), nf(nf_), at(at_) {}

    // step 5: the padded group [s, e), 0 <= s < e <= nf
    __device__ __forceinline__ void emit(int32_t s, int32_t e) {
        const int32_t len = e - s;
        if (a.max_frames <= 0 || len <= a.max_frames) {
            if constexpr (FILL) {
                if (at < (unsigned long long)a.seg_cap) a.segs_out[at] = SegRecord{item, s, len, 0, __int_as_float(0), 0.0f};
            }
            at += 1ull;
            return;
        }
        const int32_t k = (int32_t)(((long long)len + a.max_frames - 1) / a.max_frames);      // >= 2
        if constexpr (FILL) {
            const int32_t sz = (int32_t)(((long long)len + k - 1) / k), h = (a.max_frames - sz) / 2;
            int32_t c0 = s;
            for (int32_t j = 0; j < k && at + (unsigned long long)j < (unsigned long long)a.seg_cap; ++j) {
                const int32_t c1 = j == k - 1 ? e : s + (int32_t)(((long long)(j + 1) * (long long)len) / (long long)k);
                const int flags = (j > 0 ? REFINE_CUT_FIRST : 0) | (j < k - 1 ? REFINE_CUT_END : 0);
                a.segs_out[at + (unsigned long long)j] = SegRecord{item, c0, c1 - c0, h, __int_as_float(flags), 0.0f};
                c0 = c1;
            }
            // (the loop starts at the group's first piece whatever seg_cap cuts off: c0 of piece j is the c1 of piece j - 1)
        }
        at += (unsigned long long)k;
    }

    // step 4: a group that survived step 3
    __device__ __forceinline__ void survivor(int32_t s, int32_t e) {
        int32_t left = a.pad_before;
        if (have_held) {
            int32_t right = a.pad_after;
            const long long g = (long long)s - (long long)he, both = (long long)a.pad_before + (long long)a.pad_after;
            if (g < both) {
                if (g <= 0) {
                    right = 0;
                    left = 0;
                } else {
                    right = (int32_t)((g * (long long)a.pad_after) / both);
                    left = (int32_t)g - right;
                }
            }
            const long long pe = (long long)he + (long long)right;
            emit(hps, pe < (long long)nf ? (int32_t)pe : nf);
        }
        he = e;
        hps = s > left ? s - left : 0;
        have_held = true;
    }

    // step 3
    __device__ __forceinline__ void close() {
        if (!have_cur) return;
        have_cur = false;
        const int32_t len = ce - cs;                // below 1: an item's records out of frame order
        if (len >= 1 && len >= a.min_frames) survivor(cs, ce);
    }

    // steps 1 and 2
    __device__ __forceinline__ void record(int32_t first_frame, int32_t nframes) {
        if (nframes < 1) return;
        const long long e64 = (long long)first_frame + (long long)nframes;
        const int32_t s = first_frame > 0 ? first_frame : 0, e = e64 < (long long)nf ? (int32_t)e64 : nf;
        if (s >= e) return;
        if (have_cur && a.merge_gap >= 0 && (long long)s - (long long)ce <= (long long)a.merge_gap) {
            ce = e;
            return;
        }
        close();
        cs = s;
        ce = e;
        have_cur = true;
    }

    __device__ __forceinline__ void finish() {
        close();
        if (have_held) {
            const long long pe = (long long)he + (long long)a.pad_after;
            emit(hps, pe < (long long)nf ? (int32_t)pe : nf);
        }
    }
};

template <bool FILL>
__device__ __forceinline__ unsigned long long refine_item(const RefineArgs &a, int32_t item, unsigned long long base) {
    const int32_t k0 = a.out_start[item], k1 = a.out_start[item + 1];
    RefineWalk<FILL> w(a, item, k1 > k0 ? k1 - k0 : 0, base);
    const uint32_t m = refine_rows(a);
    for (uint32_t r = a.first[item]; r < m; ++r) {          // REFINE_NONE: no round
        const SegRecord x = a.segs_in[r];
        if (x.item != item) break;
        w.record(x.first_frame, x.nframes);
    }
    if (a.tails) {
        const SegRecord x = a.tails[item];
        w.record(x.first_frame, x.nframes);
    }
    w.finish();
    return w.at;
}

// the frame of [c - h, c + h], clipped to the item's 0 .. nf - 1, with the smallest accepted probability, the lowest of equals; none: c
__device__ __forceinline__ int32_t refine_cut(const RefineArgs &a, uint32_t base, int32_t nf, int32_t c, int32_t h, uint32_t lane) {
    const long long lo64 = (long long)c - (long long)h, hi64 = (long long)c + (long long)h;
    const int32_t lo = lo64 > 0 ? (int32_t)lo64 : 0, hi = hi64 < (long long)nf - 1 ? (int32_t)hi64 : nf - 1;
    unsigned long long key = ~0ull;
    for (long long t = (long long)lo + lane; t <= (long long)hi; t += 64) {
        const uint32_t k = base + (uint32_t)t;
        const float p = a.probs[k];
        if ((a.events[k] & (uint32_t)EV_REJECTED) == 0u) {
            const unsigned long long mine = ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(uint32_t)t;
            key = mine < key ? mine : key;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long other = __shfl_xor(key, d);
        key = other < key ? other : key;
    }
    return key == ~0ull ? c : (int32_t)(uint32_t)key;
}

}  // namespace

__global__ void __launch_bounds__(REFINE_THREADS) vadk_refine_init(const RefineArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (i < (unsigned long long)a.n) a.first[i] = REFINE_NONE;
}

__global__ void __launch_bounds__(REFINE_THREADS) vadk_refine_heads(const RefineArgs a) {
    const unsigned long long r = (unsigned long long)blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (r >= (unsigned long long)refine_rows(a)) return;
    const int32_t it = a.segs_in[r].item;
    if (it < 0 || it >= a.n) return;
    if (r == 0 || a.segs_in[r - 1].item != it) atomicMin(a.first + it, (uint32_t)r);
}

__global__ void __launch_bounds__(REFINE_THREADS) vadk_refine_count(const RefineArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (i < (unsigned long long)a.n) a.cnt[i] = refine_item<false>(a, (int32_t)i, 0ull);
}

__global__ void __launch_bounds__(REFINE_THREADS) vadk_refine_fill(const RefineArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (i >= (unsigned long long)a.n) return;
    const unsigned long long base = a.cnt[i];
    if (base >= (unsigned long long)a.seg_cap) return;       // every record of this item would be dropped
    (void)refine_item<true>(a, (int32_t)i, base);
}

// cnt -> its exclusive prefix in item order, after the pattern of vadk_seg_prefix, 64 bits wide throughout
__global__ void __launch_bounds__(REFINE_THREADS) vadk_refine_prefix(const RefineArgs a) {
    __shared__ unsigned long long wave_sum[REFINE_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n = (uint32_t)a.n;
    unsigned long long carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += REFINE_THREADS) {
        const uint32_t i = c0 + tid;
        const unsigned long long v = i < n ? a.cnt[i] : 0ull;
        unsigned long long inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long u = __shfl_up(inc, d);
            if ((int)lane >= d) inc += u;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        unsigned long long under = 0, all = 0;
#pragma unroll
        for (int w = 0; w < REFINE_WAVES; ++w) {
            const unsigned long long s = wave_sum[w];
            under += (uint32_t)w < wave ? s : 0ull;
            all += s;
        }
        if (i < n) a.cnt[i] = carry + under + inc - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *a.nsegs_out = carry > 0x7fffffffffffffffull ? 0x7fffffffffffffffll : (long long)carry;
}

// the fill pass wrote every record: item in 0 .. n - 1, 0 <= first_frame, first_frame + nframes <= nf, nominal cuts strictly inside
__global__ void __launch_bounds__(REFINE_THREADS) vadk_refine_cuts(const RefineArgs a) {
    const long long all = *a.nsegs_out;
    const uint32_t nrec = all < (long long)a.seg_cap ? (uint32_t)all : a.seg_cap;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x * (uint32_t)REFINE_WAVES + wave; r < nrec; r += gridDim.x * (uint32_t)REFINE_WAVES) {
        const SegRecord x = a.segs_out[r];
        const int flags = __float_as_int(x.mean_prob);
        if (flags == 0) continue;               // the wave's lanes agree: no piece of a split
        const uint32_t base = (uint32_t)a.out_start[x.item];
        const int32_t nf = a.out_start[x.item + 1] - a.out_start[x.item];
        int32_t s = x.first_frame, e = x.first_frame + x.nframes;
        if (flags & REFINE_CUT_FIRST) s = refine_cut(a, base, nf, s, x.counted, lane);
        if (flags & REFINE_CUT_END) e = refine_cut(a, base, nf, e, x.counted, lane);
        if (lane == 0) {
            a.segs_out[r].first_frame = s;
            a.segs_out[r].nframes = e - s;
        }
    }
}

static unsigned refine_blocks(unsigned long long threads) { return (unsigned)((threads + REFINE_THREADS - 1) / REFINE_THREADS); }

// heads, count and prefix: *a->nsegs_out holds the true count behind them (no item: 0)
extern "C" hipError_t vadk_launch_refine_count(const RefineArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    hipError_t r = hipSuccess;
    if (a->n > 0) {
        hipLaunchKernelGGL(vadk_refine_init, dim3(refine_blocks((unsigned long long)a->n)), dim3(REFINE_THREADS), 0, stream, *a);
        if ((r = hipGetLastError()) != hipSuccess) return r;
        if (a->in_cap) {
            hipLaunchKernelGGL(vadk_refine_heads, dim3(refine_blocks(a->in_cap)), dim3(REFINE_THREADS), 0, stream, *a);
            if ((r = hipGetLastError()) != hipSuccess) return r;
        }
        hipLaunchKernelGGL(vadk_refine_count, dim3(refine_blocks((unsigned long long)a->n)), dim3(REFINE_THREADS), 0, stream, *a);
        if ((r = hipGetLastError()) != hipSuccess) return r;
    }
    hipLaunchKernelGGL(vadk_refine_prefix, dim3(1), dim3(REFINE_THREADS), 0, stream, *a);
    return hipGetLastError();
}

// the records and their cuts, behind vadk_launch_refine_count on the same stream; vadk_launch_seg_stats completes them
extern "C" hipError_t vadk_launch_refine_fill(const RefineArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->n <= 0 || a->seg_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(vadk_refine_fill, dim3(refine_blocks((unsigned long long)a->n)), dim3(REFINE_THREADS), 0, stream, *a);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess || a->max_frames <= 0) return r;
    const uint32_t blocks = (a->seg_cap + REFINE_WAVES - 1) / REFINE_WAVES;
    hipLaunchKernelGGL(vadk_refine_cuts, dim3(blocks < 2048u ? blocks : 2048u), dim3(REFINE_THREADS), 0, stream, *a);
    return hipGetLastError();
}
