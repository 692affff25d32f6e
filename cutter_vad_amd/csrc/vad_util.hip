// Small utility kernels of the engine: batched slot control (open / reset / thresholds for many slots in ONE launch) and the
// state-machine replay (diagnostic).
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "sm_device.h"
#include "vad_layout.h"

using namespace vadk;

// One 64-thread block per listed slot.  op bits: 1 = zero (h, c); 2 = state machine := `def` (stream open); 4 = reset the
// dynamic part of the state machine, thresholds kept (VADProcessor.reset, core/silero_model.py:951-968); 8 = thresholds :=
// thr[nthr == 1 ? 0 : i] (VADWrapper.set_thresholds, core/vad_wrapper.py:367-419: values only).
extern "C" __global__ void vadk_slot_control(SmSlot *sm, float *state, const int32_t *slots, int n, int op, SmSlot def,
                                             const vad_thresholds *thr, int nthr) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (op & 1) reinterpret_cast<float4 *>(state + (size_t)s * 256)[threadIdx.x] = float4{0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x != 0) return;
    SmSlot cur = sm[s];
    if (op & 2) cur = def;
    if (op & 4) {
        SmSlot fresh = def;
        fresh.start_prob = cur.start_prob; fresh.end_prob = cur.end_prob;
        fresh.start_ratio = cur.start_ratio; fresh.end_ratio = cur.end_ratio;
        fresh.start_count = cur.start_count; fresh.end_count = cur.end_count;
        cur = fresh;
    }
    if (op & 8) {
        const vad_thresholds t = thr[nthr == 1 ? 0 : i];
        cur.start_prob = t.start_probability; cur.end_prob = t.end_probability;
        cur.start_ratio = t.start_ratio; cur.end_ratio = t.end_ratio;
        cur.start_count = t.start_frame_count; cur.end_count = t.end_frame_count;
    }
    sm[s] = cur;
}

extern "C" hipError_t vadk_launch_slot_control(SmSlot *sm, float *state, const int32_t *d_slots, int n, int op, const SmSlot *def,
                                               const vad_thresholds *d_thr, int nthr, hipStream_t stream) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(vadk_slot_control, dim3(n), dim3(64), 0, stream, sm, state, d_slots, n, op, *def, d_thr, nthr);
    return hipGetLastError();
}

// one thread replays a scripted probability sequence through one slot's state machine
extern "C" __global__ void vadk_sm_replay(SmSlot *sm, int slot, const float *probs, int n, uint8_t *events, int32_t *seg) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SmSlot s = sm[slot];
    for (int i = 0; i < n; ++i) {
        int sg = 0;
        const int ev = sm_step(s, probs[i], &sg);
        events[i] = (uint8_t)ev;
        seg[i] = (ev & 2) ? sg : 0;
    }
    sm[slot] = s;
}

extern "C" hipError_t vadk_launch_sm_replay(SmSlot *sm, int slot, const float *probs, int n, uint8_t *events, int32_t *seg,
                                            hipStream_t stream) {
    (void)hipGetLastError();   // HIP's last-error slot is sticky and process-wide: a stale failure from anywhere else must not become ours
    hipLaunchKernelGGL(vadk_sm_replay, dim3(1), dim3(64), 0, stream, sm, slot, probs, n, events, seg);
    return hipGetLastError();
}

// ITU-T G.711 codes -> 16-bit linear PCM in front of the step kernels whose loaders do not decode them (engine.cpp: launch()):
// 16 codes per thread in (four dwords: the caller's pointer is only promised 4-byte alignment), two 16-byte stores out (the
// engine's own buffer).  nbytes is a multiple of 16 (whole frames of 256 / 512 codes).
__device__ __forceinline__ uint32_t g711_pcm(uint32_t b, bool alaw) {
    const uint32_t u = ~b & 0xFFu, tu = (((u & 0x0Fu) << 3) + 0x84u) << ((u & 0x70u) >> 4);
    const int su = (u & 0x80u) ? 0x84 - (int)tu : (int)tu - 0x84;
    const uint32_t a = b ^ 0x55u, seg = (a & 0x70u) >> 4, m = (a & 0x0Fu) << 4;
    const int ta = (int)(seg == 0 ? m + 8u : (m + 0x108u) << (seg == 0 ? 0u : seg - 1u));
    const int sa = (a & 0x80u) ? ta : -ta;
    return (uint32_t)(alaw ? sa : su) & 0xFFFFu;
}

extern "C" __global__ void __launch_bounds__(256) vadk_g711_expand(const uint32_t *in, uint4 *out, int64_t n16, int alaw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const bool al = alaw != 0;
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = in[4 * i + k];
        o[2 * k] = g711_pcm(w & 0xFFu, al) | (g711_pcm((w >> 8) & 0xFFu, al) << 16);
        o[2 * k + 1] = g711_pcm((w >> 16) & 0xFFu, al) | (g711_pcm(w >> 24, al) << 16);
    }
    out[2 * i] = uint4{o[0], o[1], o[2], o[3]};
    out[2 * i + 1] = uint4{o[4], o[5], o[6], o[7]};
}

extern "C" hipError_t vadk_launch_g711_expand(const void *d_in, int16_t *d_out, int64_t nbytes, int alaw, hipStream_t stream) {
    (void)hipGetLastError();
    if (nbytes <= 0) return hipSuccess;
    if ((nbytes & 15) || (reinterpret_cast<uintptr_t>(d_in) & 3)) return hipErrorInvalidValue;
    const int64_t n16 = nbytes / 16;
    hipLaunchKernelGGL(vadk_g711_expand, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const uint32_t *>(d_in), reinterpret_cast<uint4 *>(d_out), n16, alaw);
    return hipGetLastError();
}
