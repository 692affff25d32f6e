// vad_scan_cut: the audio of finished segments, gathered out of a scanned block in its wire format and written packed, as int16 PCM
// (a WAV payload) or as float32 (vad_layout.h: CutSeg / CutWork / CutArgs).  A sample of the payload is bit for bit the float32 the
// model's loader read: the same loads (one aligned quad per thread), the same decoders (vadk_device.h: i16_div, g711_quad), the same
// channel selection ((dL + dR) * 0.5f for the mix) and the same gate (gate4) as silero_v5_t16_body.h's decode - restated in
// vadk_device.h (WireQuad), not shared with it: the 33 instantiations of that file stay the code they were.
// vad_scan_cut_stereo: the same out of a TWO-CHANNEL block with both channels kept - the work list, the unit (a quad = 4 sample
// frames) and the loads of the mono cut, each quad decoded twice, the channel a compile-time constant, and stored interleaved,
// L0 R0 L1 R1 L2 R2 L3 R3, twice as wide.  Value (k, c) is bit for bit what the mono cut writes for sample k of a segment that
// names channel c.  One body (cut_body) serves all three kernels.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

// OUT: 0 = int16 PCM, 1 = float32, the gated value itself (vadk_device.h: store_quad - 8 / 16 bytes per thread and pass, twice that
// with both channels).
// The CUT_PASSES loads of a thread are requested back to back, before the first is decoded, and UNCONDITIONALLY: a lane behind its
// segment's last quad reads some quad of the block or, past the descriptor's range, gets 0 - harmless either way, only the store
// is guarded.  (Guarded loads compile to one exec-mask block each with a full wait behind it: one request in flight, not four.)
// GAIN (vad_scan_cut_gain): the gated value times gains[segment] - one float32 multiply of its own, never fused - ahead of the
// conversion or the store; the segment's gain is one uniform load next to its CutSeg.
// BOTH (CH == 2 only): both channels are written, whatever the mode bits of CutSeg::quad_in say.
template <int FMT, int CH, int OUT, bool GAIN, bool BOTH>
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
        [[maybe_unused]] f32x4 l, r;
        l = gate4(In::decode(x[p], BOTH ? SCAN_LEFT : mode, sc, rsc), a.thresh);
        if constexpr (BOTH) r = gate4(In::decode(x[p], SCAN_RIGHT, sc, rsc), a.thresh);
        if constexpr (GAIN) {
#pragma clang fp contract(off)
            l = f32x4{l.x * g, l.y * g, l.z * g, l.w * g};
            if constexpr (BOTH) r = f32x4{r.x * g, r.y * g, r.z * g, r.w * g};
        }
        store_quad<OUT, BOTH>(a.out, sg.quad_out + oq, l, BOTH ? r : l);
    }
}

template <int FMT, int CH, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut(const CutArgs a) {
    cut_body<FMT, CH, OUT, false, false>(a, nullptr);
}

// gains: [segments of a.segs], one per CutSeg (a window of a rate cut's frames lists its own segments, each with its call
// segment's gain)
template <int FMT, int CH, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut_gain(const CutArgs a, const float *gains) {
    cut_body<FMT, CH, OUT, true, false>(a, gains);
}

template <int FMT, int OUT, bool GAIN>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut_stereo(const CutArgs a, const float *gains) {
    cut_body<FMT, 2, OUT, GAIN, true>(a, gains);
}

extern "C" hipError_t vadk_launch_scan_cut(const CutArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2, 2>([&](auto F, auto C, auto O) {
        hipLaunchKernelGGL((vadk_scan_cut<F, C + 1, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1, (int)a->out_fmt);
}

extern "C" hipError_t vadk_launch_scan_cut_gain(const CutArgs *a, const float *gains, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2, 2>([&](auto F, auto C, auto O) {
        hipLaunchKernelGGL((vadk_scan_cut_gain<F, C + 1, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a, gains);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1, (int)a->out_fmt);
}

// gains: [segments of a.segs] on the device, or nullptr: no factor (the ungained instantiation)
extern "C" hipError_t vadk_launch_scan_cut_stereo(const CutArgs *a, const float *gains, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->channels != 2) return hipErrorInvalidValue;
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2, 2>([&](auto F, auto O, auto G) {
        hipLaunchKernelGGL((vadk_scan_cut_stereo<F, O, (G != 0)>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a, gains);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->out_fmt, gains != nullptr ? 1 : 0);
}
