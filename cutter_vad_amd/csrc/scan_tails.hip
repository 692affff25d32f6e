// vad_scan_tails / vad_scan_resegment_tails and their device forms: the segment still open at a recording's last frame, which has no
// END and therefore no record in a segment table (vad_layout.h: TailArgs; include/vad_engine.h).  The length of such a segment
// includes the frames buffered before its START, so only the state machine knows it:
//   snapshot - one thread per item reads active and seg_frames of the item's stream out of its SmSlot, behind the scan's model
//              launches, and keeps the length (0: no tail) in the caller's item order; a replay gets the same number out of the
//              registers of its threads (csrc/scan_resegment.hip: vadk_tails_reseg_count);
//   tails    - one wave per entry of tail_len[nt n] writes the record {item, nf - L, L} and strides over the segment's frames for
//              the statistics of vadk_seg_stats (csrc/scan_segments.hip), the mean's sum in fixed point: exact in any order.  With 64
//              sets the waves of one item read the same lines.  An entry of 0 becomes 24 zero bytes and reads nothing else.
// vadk_seg_stats itself must not see these records: its last frame first_frame + nframes - 1 wraps for an all-zero record.  Here
// every frame index lies in 0 .. nf - 1 whatever tail_len holds - a restored slot may hold any seg_frames.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"

using namespace vadk;

namespace {
constexpr int TAIL_WAVES = TAIL_THREADS / 64;
}

__global__ void __launch_bounds__(TAIL_THREADS) vadk_tail_snapshot(const TailArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)TAIL_THREADS + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const int32_t nf = a.out_start[i + 1] - a.out_start[i];
    const SmSlot *s = a.sm + a.slots[i];
    const int32_t active = s->active, L = s->seg_frames;
    a.tail_len[i] = nf >= 1 && active != 0 && L >= 1 ? (uint32_t)L : 0u;
}

__global__ void __launch_bounds__(TAIL_THREADS) vadk_seg_tails(const TailArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = (uint32_t)a.n, entries = n * (uint32_t)a.nt;            // n nt <= 2^31 - 1
    for (uint32_t q = blockIdx.x * (uint32_t)TAIL_WAVES + wave; q < entries; q += gridDim.x * (uint32_t)TAIL_WAVES) {
        const uint32_t L = a.tail_len[q];
        SegRecord *r = a.tails + q;
        if (L == 0u) {
            if (lane == 0) *r = SegRecord{0, 0, 0, 0, 0.0f, 0.0f};
            continue;
        }
        const uint32_t item = q % n;
        const uint32_t base = (uint32_t)a.out_start[item], nf = (uint32_t)a.out_start[item + 1] - base;      // nf <= 2^31 - 1
        if (nf == 0u || L > 0x7fffffffu) {       // no frame, no tail; a length that is no seg_frames
            if (lane == 0) *r = SegRecord{0, 0, 0, 0, 0.0f, 0.0f};
            continue;
        }
        int32_t c = 0;
        long long S = 0;
        float mx = -INFINITY;
        // frames max(nf - L, 0) .. nf - 1 of the item
        for (uint32_t t = (L < nf ? nf - L : 0u) + lane; t < nf; t += 64u) {
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
            r->item = (int32_t)item;
            r->first_frame = (int32_t)nf - (int32_t)L;
            r->nframes = (int32_t)L;
            r->counted = c;
            r->mean_prob = c > 0 ? (float)((double)S / ((double)c * (double)(1ll << SEG_PROB_SHIFT))) : 0.0f;
            r->max_prob = c > 0 ? mx : 0.0f;
        }
    }
}

// tail_len[0 .. n - 1] from the slots, behind the model launches of the scan on the same stream
extern "C" hipError_t vadk_launch_tail_snapshot(const TailArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->n <= 0) return hipSuccess;
    const unsigned blocks = ((unsigned)a->n + TAIL_THREADS - 1) / TAIL_THREADS;
    hipLaunchKernelGGL(vadk_tail_snapshot, dim3(blocks), dim3(TAIL_THREADS), 0, stream, *a);
    return hipGetLastError();
}

// the records of tail_len[0 .. nt n - 1], behind whatever wrote them on the same stream
extern "C" hipError_t vadk_launch_seg_tails(const TailArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    const unsigned long long entries = (unsigned long long)(a->n > 0 ? a->n : 0) * (unsigned long long)(a->nt > 0 ? a->nt : 0);
    if (entries == 0) return hipSuccess;
    const unsigned long long blocks = (entries + TAIL_WAVES - 1) / TAIL_WAVES;
    hipLaunchKernelGGL(vadk_seg_tails, dim3((unsigned)(blocks < 2048ull ? blocks : 2048ull)), dim3(TAIL_THREADS), 0, stream, *a);
    return hipGetLastError();
}
