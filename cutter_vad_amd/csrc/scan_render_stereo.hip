// vad_scan_render_stereo: vadk_scan_render (scan_render.hip) on a TWO-CHANNEL block with both channels kept: the same work list
// and the same uniform bodies - gap, one source, two sources, each with or without ramp - with every quad of sample frames decoded
// twice and stored interleaved, L0 R0 L1 R1 L2 R2 L3 R3, twice as wide.  Value (s, c) is bit for bit what vadk_scan_render writes
// for sample s when every item names channel c: the same request (WireQuad<FMT, 2>::load), the decoder with the channel a
// compile-time constant, the gate per value, then the gain and the two ramp factors - the same for both channels of a sample
// frame, each a float32 multiply of its own - then one add per channel where two segments meet, then the conversion.
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

// NSRC, RAMP: as scan_render.hip's render_body.  All loads of a round are requested before the first decode and UNCONDITIONALLY;
// only the store is guarded.  A round holds, per pass, twice the accumulators of the mono kernel and - for a float32 block - two
// 16-byte requests per source, so it is ROUND passes long: two where two sources meet, all CUT_PASSES otherwise (DESIGN 2.1r lists
// the registers of every instantiation; none uses scratch).
template <int FMT, int OUT, int NSRC, bool RAMP>
__device__ __forceinline__ void render_body(const RenderArgs &a, const RenderWork &w, const CutSeg *sg) {
#pragma clang fp contract(off)
    using In = WireQuad<FMT, 2>;
    constexpr int ROUND = NSRC == 2 ? 2 : CUT_PASSES;
    [[maybe_unused]] const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rr =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.ramp), 0, (int)(a.nrampq * 16u), 0x00020000);
    [[maybe_unused]] float g[NSRC > 0 ? NSRC : 1];
    [[maybe_unused]] uint32_t k0[NSRC > 0 ? NSRC : 1];
#pragma unroll
    for (int s = 0; s < NSRC; ++s) {
        g[s] = a.gains ? a.gains[s == 0 ? w.seg_a : w.seg_b] : 1.0f;
        k0[s] = (uint32_t)(w.quad_out - sg[s].quad_out);         // the share lies inside the segment's span: k0 < nquads < 2^31
    }
#pragma unroll
    for (int p0 = 0; p0 < CUT_PASSES; p0 += ROUND) {
        f32x4 accl[ROUND], accr[ROUND];
#pragma unroll
        for (int p = 0; p < ROUND; ++p) accl[p] = accr[p] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (NSRC > 0) {
            typename In::XQ x[NSRC][ROUND];
            [[maybe_unused]] u32x4 fin[NSRC][ROUND], fout[NSRC][ROUND];
#pragma unroll
            for (int s = 0; s < NSRC; ++s) {
                const uint32_t qin = sg[s].quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
#pragma unroll
                for (int p = 0; p < ROUND; ++p) {
                    const uint32_t k = k0[s] + (uint32_t)((p0 + p) * CUT_THREADS) + threadIdx.x;
                    // unsigned 32-bit: the argument check keeps every quad of a segment inside the block, which is under 2 GiB
                    x[s][p] = In::load(rs, (int)((qin + k) << In::qsh));
                    if constexpr (RAMP) {
                        fin[s][p] = __builtin_amdgcn_raw_buffer_load_b128(rr, (int)(k << 4), 0, 0);
                        fout[s][p] = __builtin_amdgcn_raw_buffer_load_b128(rr, (int)((sg[s].nquads - 1u - k) << 4), 0, 0);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < NSRC; ++s) {
#pragma unroll
                for (int p = 0; p < ROUND; ++p) {
                    f32x4 l = gate4(In::decode(x[s][p], SCAN_LEFT, sc, rsc), a.thresh);
                    f32x4 r = gate4(In::decode(x[s][p], SCAN_RIGHT, sc, rsc), a.thresh);
                    if (a.gains) {
                        l = f32x4{l.x * g[s], l.y * g[s], l.z * g[s], l.w * g[s]};
                        r = f32x4{r.x * g[s], r.y * g[s], r.z * g[s], r.w * g[s]};
                    }
                    if constexpr (RAMP) {
                        const uint32_t k = k0[s] + (uint32_t)((p0 + p) * CUT_THREADS) + threadIdx.x, j = sg[s].nquads - 1u - k;
                        const f32x4 one{1.0f, 1.0f, 1.0f, 1.0f};
                        const f32x4 fi = k < a.nrampq ? __builtin_bit_cast(f32x4, fin[s][p]) : one;
                        const f32x4 fo = j < a.nrampq ? __builtin_bit_cast(f32x4, fout[s][p]) : one;
                        // sample frame 4 k + c is S - 1 - (4 j + 3 - c): the fade-out reads the table forwards from the last frame
                        l = f32x4{(l.x * fi.x) * fo.w, (l.y * fi.y) * fo.z, (l.z * fi.z) * fo.y, (l.w * fi.w) * fo.x};
                        r = f32x4{(r.x * fi.x) * fo.w, (r.y * fi.y) * fo.z, (r.z * fi.z) * fo.y, (r.w * fi.w) * fo.x};
                    }
                    if (s == 0) {
                        accl[p] = l;
                        accr[p] = r;
                    } else {
                        accl[p] = f32x4{accl[p].x + l.x, accl[p].y + l.y, accl[p].z + l.z, accl[p].w + l.w};
                        accr[p] = f32x4{accr[p].x + r.x, accr[p].y + r.y, accr[p].z + r.z, accr[p].w + r.w};
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < ROUND; ++p) {
            const uint32_t t = (uint32_t)((p0 + p) * CUT_THREADS) + threadIdx.x;
            if (t >= w.nquads) continue;
            const uint64_t o = w.quad_out + t;
            const f32x4 l = accl[p], r = accr[p];
            if constexpr (OUT == 0) {
                static_cast<u32x4 *>(a.out)[o] = u32x4{pcm16(l.x) | (pcm16(r.x) << 16), pcm16(l.y) | (pcm16(r.y) << 16),
                                                       pcm16(l.z) | (pcm16(r.z) << 16), pcm16(l.w) | (pcm16(r.w) << 16)};
            } else {
                static_cast<f32x4 *>(a.out)[2 * o] = f32x4{l.x, r.x, l.y, r.y};
                static_cast<f32x4 *>(a.out)[2 * o + 1] = f32x4{l.z, r.z, l.w, r.w};
            }
        }
    }
}

// local quads [k0, k0 + n) of a segment: does one of them lie in its fade-in (k < nrampq) or its fade-out (nquads - 1 - k < nrampq)
__device__ __forceinline__ bool in_a_fade(const CutSeg &sg, uint64_t quad_out, uint32_t n, uint32_t nrampq) {
    const uint32_t k0 = (uint32_t)(quad_out - sg.quad_out);
    return k0 < nrampq || sg.nquads - k0 - n < nrampq;
}

}  // namespace

// OUT: 0 = int16 PCM (one 16-byte store per thread and pass: eight values), 1 = float32 (two 16-byte stores).  The kinds of a
// share are bodies behind uniform branches on the work entry, as in vadk_scan_render: a gap requests nothing and stores zeros for
// both channels.
template <int FMT, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_render_stereo(const RenderArgs a) {
    const RenderWork w = a.work[blockIdx.x];
    if (w.seg_a == RENDER_NONE) {
        render_body<FMT, OUT, 0, false>(a, w, nullptr);
    } else if (w.seg_b == RENDER_NONE) {
        const CutSeg sg[1] = {a.segs[w.seg_a]};
        if (in_a_fade(sg[0], w.quad_out, w.nquads, a.nrampq)) render_body<FMT, OUT, 1, true>(a, w, sg);
        else render_body<FMT, OUT, 1, false>(a, w, sg);
    } else {
        const CutSeg sg[2] = {a.segs[w.seg_a], a.segs[w.seg_b]};
        if (in_a_fade(sg[0], w.quad_out, w.nquads, a.nrampq) || in_a_fade(sg[1], w.quad_out, w.nquads, a.nrampq))
            render_body<FMT, OUT, 2, true>(a, w, sg);
        else
            render_body<FMT, OUT, 2, false>(a, w, sg);
    }
}

extern "C" hipError_t vadk_launch_scan_render_stereo(const RenderArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->channels != 2) return hipErrorInvalidValue;
    if (a->nwork == 0) return hipSuccess;
    const int f = a->fmt == VAD_FMT_F32 ? 0 : a->fmt == VAD_FMT_ULAW8 ? 2 : a->fmt == VAD_FMT_ALAW8 ? 3 : 1;
#define VADK_RENDER(F, O)                                                                                               \
    if (f == F && a->out_fmt == O) {                                                                                    \
        hipLaunchKernelGGL((vadk_scan_render_stereo<F, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);          \
        return hipGetLastError();                                                                                       \
    }
#define VADK_RENDER4(O) VADK_RENDER(0, O) VADK_RENDER(1, O) VADK_RENDER(2, O) VADK_RENDER(3, O)
    VADK_RENDER4(0) VADK_RENDER4(1)
#undef VADK_RENDER4
#undef VADK_RENDER
    return hipErrorInvalidValue;
}
