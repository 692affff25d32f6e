// vad_scan_cut: the audio of finished segments, gathered out of a scanned block in its wire format and written packed, as int16 PCM
// (a WAV payload) or as float32 (vad_layout.h: CutSeg / CutWork / CutArgs).  A sample of the payload is bit for bit the float32 the
// model's loader read: the same loads (one aligned quad per thread), the same decoders (vadk_device.h: i16_div, g711_quad), the same
// channel selection ((dL + dR) * 0.5f for the mix) and the same gate (gate4) as silero_v5_t16_body.h's decode - restated in
// vadk_device.h (WireQuad), not shared with it: the 33 instantiations of that file stay the code they were.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// utils/wav_writer.py:41: np.clip(x * 32767, -32768, 32767).astype(np.int16) - one float32 multiply, the clamp, the conversion
// toward zero (a NaN's result is unspecified there and here)
__device__ __forceinline__ uint32_t pcm16(float x) {
#pragma clang fp contract(off)
    const float v = x * 32767.0f;
    return (uint32_t)(int)fminf(fmaxf(v, -32768.0f), 32767.0f) & 0xffffu;
}

}  // namespace

// OUT: 0 = int16 PCM (one 8-byte store per thread and pass), 1 = float32, the gated value itself (one 16-byte store).
// The CUT_PASSES loads of a thread are requested back to back, before the first is decoded, and UNCONDITIONALLY: a lane behind its
// segment's last quad reads some quad of the block or, past the descriptor's range, gets 0 - harmless either way, only the store
// is guarded.  (Guarded loads compile to one exec-mask block each with a full wait behind it: one request in flight, not four.)
// GAIN (vad_scan_cut_gain): the gated value times gains[segment] - one float32 multiply of its own, never fused - ahead of the
// conversion or the store; the segment's gain is one uniform load next to its CutSeg.
template <int FMT, int CH, int OUT, bool GAIN>
__device__ __forceinline__ void cut_body(const CutArgs &a, const float *gains) {
    using In = WireQuad<FMT, CH>;
    const CutWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const uint32_t fmask = a.frame_shift >= 31u ? 0x7fffffffu : (1u << a.frame_shift) - 1u;
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
    float g = 1.0f;
    if constexpr (GAIN) g = gains[w.seg];
    typename In::XQ x[CUT_PASSES];
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t oq = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        // unsigned 32-bit: the argument check keeps every quad of a segment inside the block, which is under 2 GiB
        const uint32_t iq = qin + (oq >> a.frame_shift) * a.hopq + (oq & fmask);
        x[p] = In::load(rs, (int)(iq << In::qsh));
    }
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t oq = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        if (oq >= sg.nquads) continue;
        f32x4 v = gate4(In::decode(x[p], mode, sc, rsc), a.thresh);
        if constexpr (GAIN) {
#pragma clang fp contract(off)
            v = f32x4{v.x * g, v.y * g, v.z * g, v.w * g};
        }
        const uint64_t o = sg.quad_out + oq;
        if constexpr (OUT == 0)
            static_cast<u32x2 *>(a.out)[o] = u32x2{pcm16(v.x) | (pcm16(v.y) << 16), pcm16(v.z) | (pcm16(v.w) << 16)};
        else
            static_cast<f32x4 *>(a.out)[o] = v;
    }
}

template <int FMT, int CH, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut(const CutArgs a) {
    cut_body<FMT, CH, OUT, false>(a, nullptr);
}

// gains: [segments of a.segs], one per CutSeg (a window of a rate cut's frames lists its own segments, each with its call
// segment's gain)
template <int FMT, int CH, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut_gain(const CutArgs a, const float *gains) {
    cut_body<FMT, CH, OUT, true>(a, gains);
}

extern "C" hipError_t vadk_launch_scan_cut(const CutArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    const int f = a->fmt == VAD_FMT_F32 ? 0 : a->fmt == VAD_FMT_ULAW8 ? 2 : a->fmt == VAD_FMT_ALAW8 ? 3 : 1;
#define VADK_CUT(F, C, O)                                                                                               \
    if (f == F && a->channels == C && a->out_fmt == O) {                                                                \
        hipLaunchKernelGGL((vadk_scan_cut<F, C, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);                 \
        return hipGetLastError();                                                                                       \
    }
#define VADK_CUT4(C, O) VADK_CUT(0, C, O) VADK_CUT(1, C, O) VADK_CUT(2, C, O) VADK_CUT(3, C, O)
    VADK_CUT4(1, 0) VADK_CUT4(1, 1) VADK_CUT4(2, 0) VADK_CUT4(2, 1)
#undef VADK_CUT4
#undef VADK_CUT
    return hipErrorInvalidValue;
}

extern "C" hipError_t vadk_launch_scan_cut_gain(const CutArgs *a, const float *gains, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    const int f = a->fmt == VAD_FMT_F32 ? 0 : a->fmt == VAD_FMT_ULAW8 ? 2 : a->fmt == VAD_FMT_ALAW8 ? 3 : 1;
#define VADK_CUT(F, C, O)                                                                                               \
    if (f == F && a->channels == C && a->out_fmt == O) {                                                                \
        hipLaunchKernelGGL((vadk_scan_cut_gain<F, C, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a, gains);     \
        return hipGetLastError();                                                                                       \
    }
#define VADK_CUT4(C, O) VADK_CUT(0, C, O) VADK_CUT(1, C, O) VADK_CUT(2, C, O) VADK_CUT(3, C, O)
    VADK_CUT4(1, 0) VADK_CUT4(1, 1) VADK_CUT4(2, 0) VADK_CUT4(2, 1)
#undef VADK_CUT4
#undef VADK_CUT
    return hipErrorInvalidValue;
}
