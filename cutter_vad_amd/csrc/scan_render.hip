// vad_scan_render: one finished piece of audio per call - the segments of a scanned block faded by the caller's ramp, crossfaded
// where two of them share output samples, joined, and every other output sample zero (vad_layout.h: RenderWork / RenderArgs).
// The kernel is driven by the OUTPUT: a workgroup serves up to CUT_WG_QUADS consecutive output quads that the same none, one or two
// segments cover (the host lists them), so the kind of a workgroup is uniform and no lane diverges on it.  A source sample is bit
// for bit what vadk_scan_cut_gain writes as float32 for the sample range once: the same loads, decoders, channel selection and gate
// (vadk_device.h: WireQuad, gate4), then the gain, then the two ramp factors - each a float32 multiply of its own - then one add
// where two segments meet, then the cut's conversion and one store (vadk_device.h: store_quad).  No transcendental, no division:
// the ramp is a table.
// vad_scan_render_stereo: the same on a TWO-CHANNEL block with both channels kept: the same work list and the same uniform bodies,
// every quad of sample frames decoded twice, the channel a compile-time constant, and stored interleaved, L0 R0 L1 R1 L2 R2 L3 R3,
// twice as wide.  Value (s, c) is bit for bit what vadk_scan_render writes for sample s when every item names channel c; the gain
// and the two ramp factors are the same for both channels of a sample frame.  One body (render_body) serves both kernels.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// NSRC: the segments that cover the workgroup's share; RAMP: some quad of the share lies in a fade of one of them (uniform per
// workgroup: the bulk of a long segment touches neither end and then requests and multiplies nothing of the table - its samples
// times 1.0f are themselves).  All loads of a round - per source and pass one block quad and, with RAMP, two ramp quads - are
// requested before the first decode and UNCONDITIONALLY, as in the cut: a lane behind its share's last quad reads some quad of the
// block or gets 0 past the descriptor's range, and a ramp quad outside the table reads 0 and is replaced by ones - harmless either
// way, only the store is guarded.  A round is all CUT_PASSES passes, or two of them where two faded sources would otherwise hold
// 24 requests per thread in registers: the kernel's register count is that of its largest body.
// BOTH (CH == 2 only): both channels are written, whatever the mode bits say.  A round then holds, per pass, twice the accumulators
// and - for a float32 block - two 16-byte requests per source, so it is two passes long wherever two sources meet, faded or not
// (DESIGN 2.1q / 2.1r list the registers of every instantiation; none uses scratch).
template <int FMT, int CH, int OUT, int NSRC, bool RAMP, bool BOTH>
__device__ __forceinline__ void render_body(const RenderArgs &a, const RenderWork &w, const CutSeg *sg) {
#pragma clang fp contract(off)
    using In = WireQuad<FMT, CH>;
    constexpr int NV = BOTH ? 2 : 1, ROUND = (NSRC == 2 && (RAMP || BOTH)) ? 2 : CUT_PASSES;
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
        f32x4 acc[NV][ROUND];                                    // [0]: the one channel, or left; [1]: right
#pragma unroll
        for (int p = 0; p < ROUND; ++p) acc[0][p] = acc[NV - 1][p] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
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
                const uint32_t mode = sg[s].quad_in >> SCAN_MODE_SHIFT;
#pragma unroll
                for (int p = 0; p < ROUND; ++p) {
                    [[maybe_unused]] f32x4 l, r;
                    l = gate4(In::decode(x[s][p], BOTH ? SCAN_LEFT : mode, sc, rsc), a.thresh);
                    if constexpr (BOTH) r = gate4(In::decode(x[s][p], SCAN_RIGHT, sc, rsc), a.thresh);
                    if (a.gains) {
                        l = f32x4{l.x * g[s], l.y * g[s], l.z * g[s], l.w * g[s]};
                        if constexpr (BOTH) r = f32x4{r.x * g[s], r.y * g[s], r.z * g[s], r.w * g[s]};
                    }
                    if constexpr (RAMP) {
                        const uint32_t k = k0[s] + (uint32_t)((p0 + p) * CUT_THREADS) + threadIdx.x, j = sg[s].nquads - 1u - k;
                        const f32x4 one{1.0f, 1.0f, 1.0f, 1.0f};
                        const f32x4 fi = k < a.nrampq ? __builtin_bit_cast(f32x4, fin[s][p]) : one;
                        const f32x4 fo = j < a.nrampq ? __builtin_bit_cast(f32x4, fout[s][p]) : one;
                        // sample frame 4 k + c is S - 1 - (4 j + 3 - c): the fade-out reads the table forwards from the last frame
                        l = f32x4{(l.x * fi.x) * fo.w, (l.y * fi.y) * fo.z, (l.z * fi.z) * fo.y, (l.w * fi.w) * fo.x};
                        if constexpr (BOTH) r = f32x4{(r.x * fi.x) * fo.w, (r.y * fi.y) * fo.z, (r.z * fi.z) * fo.y, (r.w * fi.w) * fo.x};
                    }
                    if (s == 0) {
                        acc[0][p] = l;
                        if constexpr (BOTH) acc[1][p] = r;
                    } else {
                        acc[0][p] = f32x4{acc[0][p].x + l.x, acc[0][p].y + l.y, acc[0][p].z + l.z, acc[0][p].w + l.w};
                        if constexpr (BOTH) acc[1][p] = f32x4{acc[1][p].x + r.x, acc[1][p].y + r.y, acc[1][p].z + r.z, acc[1][p].w + r.w};
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < ROUND; ++p) {
            const uint32_t t = (uint32_t)((p0 + p) * CUT_THREADS) + threadIdx.x;
            if (t >= w.nquads) continue;
            store_quad<OUT, BOTH>(a.out, w.quad_out + t, acc[0][p], acc[NV - 1][p]);
        }
    }
}

// local quads [k0, k0 + n) of a segment: does one of them lie in its fade-in (k < nrampq) or its fade-out (nquads - 1 - k < nrampq)
__device__ __forceinline__ bool in_a_fade(const CutSeg &sg, uint64_t quad_out, uint32_t n, uint32_t nrampq) {
    const uint32_t k0 = (uint32_t)(quad_out - sg.quad_out);
    return k0 < nrampq || sg.nquads - k0 - n < nrampq;
}

}  // namespace

// OUT: 0 = int16 PCM, 1 = float32 (vadk_device.h: store_quad).  The kinds of a share are bodies behind uniform branches on the work
// entry and the segments it names: a gap requests nothing and stores zeros.  (The branches stand in both kernels: behind a shared
// function of their own the mono kernels no longer compile to the instructions they were.)

template <int FMT, int CH, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_render(const RenderArgs a) {
    const RenderWork w = a.work[blockIdx.x];
    if (w.seg_a == RENDER_NONE) {
        render_body<FMT, CH, OUT, 0, false, false>(a, w, nullptr);
    } else if (w.seg_b == RENDER_NONE) {
        const CutSeg sg[1] = {a.segs[w.seg_a]};
        if (in_a_fade(sg[0], w.quad_out, w.nquads, a.nrampq)) render_body<FMT, CH, OUT, 1, true, false>(a, w, sg);
        else render_body<FMT, CH, OUT, 1, false, false>(a, w, sg);
    } else {
        const CutSeg sg[2] = {a.segs[w.seg_a], a.segs[w.seg_b]};
        if (in_a_fade(sg[0], w.quad_out, w.nquads, a.nrampq) || in_a_fade(sg[1], w.quad_out, w.nquads, a.nrampq))
            render_body<FMT, CH, OUT, 2, true, false>(a, w, sg);
        else
            render_body<FMT, CH, OUT, 2, false, false>(a, w, sg);
    }
}

template <int FMT, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_render_stereo(const RenderArgs a) {
    const RenderWork w = a.work[blockIdx.x];
    if (w.seg_a == RENDER_NONE) {
        render_body<FMT, 2, OUT, 0, false, true>(a, w, nullptr);
    } else if (w.seg_b == RENDER_NONE) {
        const CutSeg sg[1] = {a.segs[w.seg_a]};
        if (in_a_fade(sg[0], w.quad_out, w.nquads, a.nrampq)) render_body<FMT, 2, OUT, 1, true, true>(a, w, sg);
        else render_body<FMT, 2, OUT, 1, false, true>(a, w, sg);
    } else {
        const CutSeg sg[2] = {a.segs[w.seg_a], a.segs[w.seg_b]};
        if (in_a_fade(sg[0], w.quad_out, w.nquads, a.nrampq) || in_a_fade(sg[1], w.quad_out, w.nquads, a.nrampq))
            render_body<FMT, 2, OUT, 2, true, true>(a, w, sg);
        else
            render_body<FMT, 2, OUT, 2, false, true>(a, w, sg);
    }
}

extern "C" hipError_t vadk_launch_scan_render(const RenderArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2, 2>([&](auto F, auto C, auto O) {
        hipLaunchKernelGGL((vadk_scan_render<F, C + 1, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1, (int)a->out_fmt);
}

extern "C" hipError_t vadk_launch_scan_render_stereo(const RenderArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->channels != 2) return hipErrorInvalidValue;
    if (a->nwork == 0) return hipSuccess;
    return launch_variant<4, 2>([&](auto F, auto O) {
        hipLaunchKernelGGL((vadk_scan_render_stereo<F, O>), dim3(a->nwork), dim3(CUT_THREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->out_fmt);
}
