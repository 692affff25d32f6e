// vad_scan_cut_stereo: the audio of finished segments out of a TWO-CHANNEL block with both channels kept - the work list, the unit
// (a quad = 4 sample frames) and the loads of vadk_scan_cut (scan_cut.hip), each quad of sample frames decoded twice and stored
// interleaved, L0 R0 L1 R1 L2 R2 L3 R3, twice as wide.  Value (k, c) is bit for bit what vadk_scan_cut / vadk_scan_cut_gain writes
// for sample k of a segment that names channel c: the same request (WireQuad<FMT, 2>::load), the same decoder with the channel a
// compile-time constant, the same gate per value (gate4), the same lone multiply by the segment's gain, the same conversion.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// scan_cut.hip's pcm16, restated (that file stays byte for byte): np.clip(x * 32767, -32768, 32767).astype(np.int16)
__device__ __forceinline__ uint32_t pcm16(float x) {
#pragma clang fp contract(off)
    const float v = x * 32767.0f;
    return (uint32_t)(int)fminf(fmaxf(v, -32768.0f), 32767.0f) & 0xffffu;
}

}  // namespace

// OUT: 0 = int16 PCM (one 16-byte store per thread and pass: eight values), 1 = float32 (two 16-byte stores).  As in the mono cut
// the CUT_PASSES loads of a thread are requested back to back and UNCONDITIONALLY before the first decode; only the stores are
// guarded.  The mode bits of CutSeg::quad_in are masked off: both channels are written whatever they say.
template <int FMT, int OUT, bool GAIN>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut_stereo(const CutArgs a, const float *gains) {
    using In = WireQuad<FMT, 2>;
    const CutWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
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
        f32x4 l = gate4(In::decode(x[p], SCAN_LEFT, sc, rsc), a.thresh);
        f32x4 r = gate4(In::decode(x[p], SCAN_RIGHT, sc, rsc), a.thresh);
        if constexpr (GAIN) {
#pragma clang fp contract(off)
            l = f32x4{l.x * g, l.y * g, l.z * g, l.w * g};
            r = f32x4{r.x * g, r.y * g, r.z * g, r.w * g};
        }
        const uint64_t o = sg.quad_out + oq;
        if constexpr (OUT == 0) {
            static_cast<u32x4 *>(a.out)[o] = u32x4{pcm16(l.x) | (pcm16(r.x) << 16), pcm16(l.y) | (pcm16(r.y) << 16),
                                                   pcm16(l.z) | (pcm16(r.z) << 16), pcm16(l.w) | (pcm16(r.w) << 16)};
        } else {
            static_cast<f32x4 *>(a.out)[2 * o] = f32x4{l.x, r.x, l.y, r.y};
            static_cast<f32x4 *>(a.out)[2 * o + 1] = f32x4{l.z, r.z, l.w, r.w};
        }
    }
}

// gains: [segments of a.segs] on the device, or nullptr: no factor (the ungained instantiation)
extern "C" hipError_t vadk_launch_scan_cut_stereo(const CutArgs *a, const float *gains, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->channels != 2) return hipErrorInvalidValue;
    if (a->nwork == 0) return hipSuccess;
    const int f = a->fmt == VAD_FMT_F32 ? 0 : a->fmt == VAD_FMT_ULAW8 ? 2 : a->fmt == VAD_FMT_ALAW8 ? 3 : 1;
    const bool gain = gains != nullptr;
#define VADK_CUT(F, O, G)                                                                                                  \
    if (f == F && a->out_fmt == O && gain == G) {                                                                          \
        hipLaunchKernelGGL((vadk_scan_cut_stereo<F, O, G>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a, gains);      \
        return hipGetLastError();                                                                                          \
    }
#define VADK_CUT4(O, G) VADK_CUT(0, O, G) VADK_CUT(1, O, G) VADK_CUT(2, O, G) VADK_CUT(3, O, G)
    VADK_CUT4(0, false) VADK_CUT4(1, false) VADK_CUT4(0, true) VADK_CUT4(1, true)
#undef VADK_CUT4
#undef VADK_CUT
    return hipErrorInvalidValue;
}
