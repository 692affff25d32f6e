// vad_resegment_device / vad_scan_resegment: the per-frame results a scan left in device memory, replayed through the state machine
// under up to RESEG_MAX_SETS threshold sets at once (vad_layout.h: ResegArgs; include/vad_engine.h).  The model's output does not
// depend on the thresholds - sm_step runs behind the probability head and never feeds back into (h, c) - so the probabilities answer
// every other setting.  One thread per (item, set) keeps its SmSlot in registers and walks the item's frames in order; a frame whose
// event byte has VAD_EV_REJECTED set is skipped as the model kernels skip it, and nothing else of the old events is read.  The
// records are ordered by set, then item, then frame, whatever the GPU's scheduling, so there are no atomics:
//   count  - the replay, counting ENDs into cnt[set n + item];
//   prefix - ONE workgroup turns cnt into its exclusive prefix in (set, item) order, RESEG_THREADS items per round, and writes
//            set_start[0 .. nt] as it passes each set's first item;
//   fill   - the replay again: the j-th END of (item, set) goes to position cnt[set n + item] + j, dropped at seg_cap or above;
//   stats  - csrc/scan_segments.hip's vadk_seg_stats over the written records (vadk_launch_seg_stats): the item index of a record
//            addresses the same out_start in every set.
// Sets run along the lanes, 1 << set_shift of them per item: the lanes of a wave that share an item load the same probability and
// event addresses (one request each), and with 64 sets a wave is one recording.  Lanes whose items differ in length run to the
// longest.  Four frames are loaded ahead of their four steps, so a thread waits for memory once per four frames.
//   tails  - vadk_tails_reseg_count (vad_scan_resegment_tails, vad_resegment_tails_device): the count replay once more, which also
//            keeps the state machine it ends with - inside a segment: its seg_frames, else 0, into tail_len[set n + item] - for
//            csrc/scan_tails.hip's vadk_seg_tails.  A kernel of its own: the three above compile to what they were without it.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "sm_device.h"
#include "vad_layout.h"

using namespace vadk;

static_assert(EV_REJECTED == VAD_EV_REJECTED, "the skipped frames are the header's");
static_assert(RESEG_MAX_SETS == 64, "a recording's sets fit one wave");

namespace {

constexpr int RESEG_WAVES = RESEG_THREADS / 64;
constexpr int RESEG_AHEAD = 4;                // frames loaded before the first of them is stepped

// the accepted frames of `item` through `s`; FILL: END number j is written at base + j -> the number of ENDs; `last`: where the
// state machine behind the item's last frame goes (the tails)
template <bool FILL>
__device__ __forceinline__ uint32_t reseg_replay(const ResegArgs &a, int32_t item, SmSlot s, unsigned long long base, SmSlot *last = nullptr) {
    const uint32_t k0 = (uint32_t)a.out_start[item], k1 = (uint32_t)a.out_start[item + 1];      // k0 <= k1 <= 2^31 - 1
    uint32_t j = 0;
    auto step = [&](uint32_t k, uint32_t ev, float p) {
        if (ev & (uint32_t)EV_REJECTED) return;
        int L = 0;
        if (sm_step(s, p, &L) & 2) {
            if constexpr (FILL) {
                const unsigned long long pos = base + j;
                if (pos < (unsigned long long)a.seg_cap) {
                    SegRecord *r = a.segs + pos;
                    r->item = item;
                    r->first_frame = (int32_t)(k - k0) - L + 1;
                    r->nframes = L;
                }
            }
            ++j;
        }
    };
    uint32_t k = k0;
    for (; k1 - k >= (uint32_t)RESEG_AHEAD; k += (uint32_t)RESEG_AHEAD) {
        float p[RESEG_AHEAD];
        uint32_t ev[RESEG_AHEAD];
#pragma unroll
        for (int u = 0; u < RESEG_AHEAD; ++u) {
            p[u] = a.probs[k + (uint32_t)u];
            ev[u] = a.events[k + (uint32_t)u];
        }
#pragma unroll
        for (int u = 0; u < RESEG_AHEAD; ++u) step(k + (uint32_t)u, ev[u], p[u]);
    }
    for (; k < k1; ++k) step(k, a.events[k], a.probs[k]);
    if (last) *last = s;
    return j;
}

// thread -> (item, set); false: a lane of the padding, or behind the last item
__device__ __forceinline__ bool reseg_thread(const ResegArgs &a, int32_t *item, int32_t *set) {
    const unsigned long long g = (unsigned long long)blockIdx.x * (unsigned long long)RESEG_THREADS + threadIdx.x;
    const unsigned long long i = g >> a.set_shift;
    *set = (int32_t)(g & ((1ull << a.set_shift) - 1ull));
    *item = (int32_t)i;
    return i < (unsigned long long)a.n && *set < a.nt;
}

}  // namespace

__global__ void __launch_bounds__(RESEG_THREADS) vadk_reseg_count(const ResegArgs a) {
    int32_t item, set;
    if (!reseg_thread(a, &item, &set)) return;
    a.cnt[(size_t)set * (size_t)a.n + (size_t)item] = reseg_replay<false>(a, item, a.sm0[set], 0ull);
}

// the count replay that also keeps what vadk_tail_snapshot reads out of a stream's slot (csrc/scan_tails.hip): the seg_frames of a
// state machine that ends the item inside a segment, else 0.  A fresh state machine is not active before its first frame, so an
// item without frames has no tail.
__global__ void __launch_bounds__(RESEG_THREADS) vadk_tails_reseg_count(const ResegArgs a, uint32_t *tail_len) {
    int32_t item, set;
    if (!reseg_thread(a, &item, &set)) return;
    SmSlot s;
    a.cnt[(size_t)set * (size_t)a.n + (size_t)item] = reseg_replay<false>(a, item, a.sm0[set], 0ull, &s);
    const bool any = a.out_start[item + 1] > a.out_start[item];
    tail_len[(size_t)set * (size_t)a.n + (size_t)item] = any && s.active != 0 && s.seg_frames >= 1 ? (uint32_t)s.seg_frames : 0u;
}

__global__ void __launch_bounds__(RESEG_THREADS) vadk_reseg_fill(const ResegArgs a) {
    int32_t item, set;
    if (!reseg_thread(a, &item, &set)) return;
    const unsigned long long base = a.cnt[(size_t)set * (size_t)a.n + (size_t)item];
    if (base >= (unsigned long long)a.seg_cap) return;         // every record of this thread would be dropped
    (void)reseg_replay<true>(a, item, a.sm0[set], base);
}

// cnt -> its exclusive prefix in (set, item) order, after the pattern of vadk_seg_prefix; a round's 256 counts sum to at most the
// frames of 256 items, below 2^31, and the running total is 64 bits wide
__global__ void __launch_bounds__(RESEG_THREADS) vadk_reseg_prefix(const ResegArgs a) {
    __shared__ uint32_t wave_sum[RESEG_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n = (uint32_t)a.n;
    unsigned long long carry = 0;
    for (int32_t set = 0; set < a.nt; ++set) {
        if (tid == 0) a.set_start[set] = (long long)carry;
        uint32_t *cnt = a.cnt + (size_t)set * (size_t)n;
        for (uint32_t c0 = 0; c0 < n; c0 += RESEG_THREADS) {
            const uint32_t i = c0 + tid;
            const uint32_t v = i < n ? cnt[i] : 0u;
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
            for (int w = 0; w < RESEG_WAVES; ++w) {
                const uint32_t s = wave_sum[w];
                under += (uint32_t)w < wave ? s : 0u;
                all += s;
            }
            if (i < n) {
                const unsigned long long at = carry + under + inc - v;
                cnt[i] = at > 0xffffffffull ? 0xffffffffu : (uint32_t)at;
            }
            carry += all;
            __syncthreads();
        }
    }
    if (tid == 0) a.set_start[a.nt] = (long long)carry;
}

static unsigned reseg_blocks(const ResegArgs *a) {
    const unsigned long long threads = (unsigned long long)a->n << a->set_shift;      // n nt <= 2^31 - 1: below 2^32
    return (unsigned)((threads + RESEG_THREADS - 1) / RESEG_THREADS);
}

// count and prefix: set_start holds the true counts behind them (no item: all zero)
extern "C" hipError_t vadk_launch_reseg_count(const ResegArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    hipError_t r = hipSuccess;
    const unsigned blocks = reseg_blocks(a);
    if (blocks) {
        hipLaunchKernelGGL(vadk_reseg_count, dim3(blocks), dim3(RESEG_THREADS), 0, stream, *a);
        if ((r = hipGetLastError()) != hipSuccess) return r;
    }
    hipLaunchKernelGGL(vadk_reseg_prefix, dim3(1), dim3(RESEG_THREADS), 0, stream, *a);
    return hipGetLastError();
}

// the count replay alone, with the tails' lengths: tail_len[set n + item] (no prefix: a->set_start is not written)
extern "C" hipError_t vadk_launch_reseg_tails(const ResegArgs *a, uint32_t *tail_len, hipStream_t stream) {
    (void)hipGetLastError();
    const unsigned blocks = reseg_blocks(a);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(vadk_tails_reseg_count, dim3(blocks), dim3(RESEG_THREADS), 0, stream, *a, tail_len);
    return hipGetLastError();
}

// the records, behind vadk_launch_reseg_count on the same stream; vadk_launch_seg_stats completes them
extern "C" hipError_t vadk_launch_reseg_fill(const ResegArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    const unsigned blocks = reseg_blocks(a);
    if (blocks == 0 || a->seg_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(vadk_reseg_fill, dim3(blocks), dim3(RESEG_THREADS), 0, stream, *a);
    return hipGetLastError();
}
