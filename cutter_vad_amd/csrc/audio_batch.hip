// vad_scan_audio_batch: normalised, zero-padded windows of segment audio, [nw][T] in float32, float16 or bfloat16, with an
// attention mask (include/vad_engine.h: vad_audio_batch; vad_layout.h: AudioWin / AudioWork / AudioBatchArgs).  A sample of a window
// is exactly the float32 that vadk_scan_cut with the sample range once and float32 output would write for the segment - the same
// loads, decoders, channel selection and gate (vadk_device.h: WireQuad, gate4) - then (x + shift) * scale, an add and a multiply that
// are each rounded on their own, then the conversion, round to nearest even.
// One workgroup of CUT_THREADS threads serves CUT_WG_QUADS consecutive quads of ONE window; the host lists the workgroups.  A
// workgroup that lies wholly behind the window's nsamples is a block-uniform case: it requests no audio and stores pad cells.
// Otherwise the CUT_PASSES loads of a thread are requested back to back before the first is decoded, and UNCONDITIONALLY, as in the
// cut: a lane behind the window's samples reads some quad of the block or, past the descriptor's range, gets 0, and every component
// at or behind nsamples is replaced by the pad cell.  One b128 (float32) or b64 (16-bit types) store per quad, one b32 of mask.
// Every cell is written by exactly one lane and nothing is accumulated: two runs give the same bytes.  No LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

// the header's rule is a sequence of float32 operations, each rounded on its own
#pragma clang fp contract(off)

using namespace vadk;
using namespace vadk::dev;

namespace {

// mel_batch.hip's converters: v_cvt_f16_f32 under the default rounding mode, and vad_layout.h's melb_bf16
template <int DT>
__device__ __forceinline__ uint32_t ab_bits16(float v) {
    if constexpr (DT == VAD_BATCH_F16) return __half_as_ushort(__float2half_rn(v));
    else return melb_bf16(__float_as_uint(v));
}

template <int DT>
__device__ __forceinline__ void ab_store(void *out, uint64_t oq, f32x4 v) {
    if constexpr (DT == VAD_BATCH_F32) static_cast<f32x4 *>(out)[oq] = v;
    else static_cast<u32x2 *>(out)[oq] = u32x2{ab_bits16<DT>(v.x) | (ab_bits16<DT>(v.y) << 16), ab_bits16<DT>(v.z) | (ab_bits16<DT>(v.w) << 16)};
}

}  // namespace

template <int FMT, int CH, int DT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_audio_batch(const AudioBatchArgs a) {
    using In = WireQuad<FMT, CH>;
    const AudioWork w = a.work[blockIdx.x];
    const AudioWin win = a.win[w.window];
    const uint32_t aff = a.per_seg ? win.seg : 0u;
    const float shift = a.shift[aff], scale = a.scale[aff];
    const float pad = a.pad_mode == VAD_BATCH_PAD_FEATURE ? (0.0f + shift) * scale : a.pad_value;
    const uint64_t out0 = (uint64_t)w.window * a.tq;                 // the window's first quad of the output
    if (4u * w.quad0 >= win.nsamples) {                                // uniform: nothing of the segment is shown here
#pragma unroll
        for (int p = 0; p < CUT_PASSES; ++p) {
            const uint32_t q = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
            if (q >= a.tq) continue;
            ab_store<DT>(a.out, out0 + q, f32x4{pad, pad, pad, pad});
            if (a.mask) reinterpret_cast<uint32_t *>(a.mask)[out0 + q] = 0u;
        }
        return;
    }
    const CutSeg sg = a.segs[win.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = (sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u)) + win.quad0;
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
    typename In::XQ x[CUT_PASSES];
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t q = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        // unsigned 32-bit: the block is under 2 GiB and a window under 2^24 samples; past the descriptor's range a load gives 0
        x[p] = In::load(rs, (int)((qin + q) << In::qsh));
    }
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const uint32_t q = w.quad0 + (uint32_t)(p * CUT_THREADS) + threadIdx.x;
        if (q >= a.tq) continue;
        f32x4 v = gate4(In::decode(x[p], mode, sc, rsc), a.thresh);
        v = f32x4{(v.x + shift) * scale, (v.y + shift) * scale, (v.z + shift) * scale, (v.w + shift) * scale};
        const uint32_t t = 4u * q, n = win.nsamples;
        const bool m0 = t < n, m1 = t + 1u < n, m2 = t + 2u < n, m3 = t + 3u < n;
        v = f32x4{m0 ? v.x : pad, m1 ? v.y : pad, m2 ? v.z : pad, m3 ? v.w : pad};
        ab_store<DT>(a.out, out0 + q, v);
        if (a.mask)
            reinterpret_cast<uint32_t *>(a.mask)[out0 + q] = (m0 ? 1u : 0u) | (m1 ? 1u << 8 : 0u) | (m2 ? 1u << 16 : 0u) | (m3 ? 1u << 24 : 0u);
    }
}

extern "C" hipError_t vadk_launch_audio_batch(const AudioBatchArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2, 3>([&](auto F, auto C, auto D) {
        hipLaunchKernelGGL((vadk_audio_batch<F, C + 1, D>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1, (int)a->dtype);
}
