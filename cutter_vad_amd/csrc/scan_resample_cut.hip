// vad_scan_resample_cut: finished segments of a rate block (8 / 24 / 48 kHz) as ONE continuous signal each at 16 kHz, by a polyphase
// FIR whose taps are the caller's (include/vad_engine.h: the rule; vad_layout.h: ResampleCutArgs and the packed operator).  A
// segment's input samples are exactly the float32 values vadk_scan_cut with the sample range once and float32 output writes for it
// on such a block: the same loads, decoders and channel selection (vadk_device.h: WireQuad), no gate.  One workgroup serves
// RSC_WG_SAMPLES consecutive outputs of ONE segment:
//   1. its input span - the outputs' own inputs and the taps' reach on either side - is loaded ONCE, quad by quad, decoded and put
//      into LDS as float32.  A quad outside the segment's sample range [0, S_in) is a zero and NO LOAD: the rule zero-extends the
//      segment, whatever the block holds there, and a segment may start on the block's first sample and end on its last.  The
//      buffer descriptor covers the segment's own bytes and nothing else, so the hardware holds the same line.
//   2. the banded Toeplitz product on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain along n): T, packed by the host in fragment
//      order, is the A operand - one coalesced 1 KiB load per wave and four k-steps, shared by the wave's two tiles - and the span
//      is the B operand out of LDS, column = row-block, in the skew that keeps a fragment's 64 reads in 64 banks.
//   3. D has four consecutive outputs of one row-block on a lane: one quad, gained (a multiply of its own) and stored as the cut
//      stores it - 16 bytes of float32 or 8 of int16 PCM (vadk_device.h: pcm16).
// Every sum has a fixed order and nothing is accumulated across workgroups: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

static_assert(VAD_RESAMPLE_CUT_WG_SAMPLES == RSC_WG_SAMPLES, "the header's workgroup share is the kernel's");
static_assert(RSC_WG_SAMPLES == 2 * 256 * (RSC_THREADS / 64), "two tiles of 256 outputs per wave");

namespace {

__device__ __forceinline__ float pick(f32x4 v, uint32_t k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

constexpr int RSC_LOADS = 4;      // quads a thread requests back to back

}  // namespace

// RATE: 0 = 8000 (L / M = 2 / 1), 1 = 24000 (2 / 3), 2 = 48000 (1 / 3).  Dynamic LDS: rsc_lds_floats(A, K) floats.  Row-blocks past
// the segment's last output read LDS nobody wrote: a row-block is a column of D of its own, and the store leaves those quads out.
template <int FMT, int CH, int RATE>
__global__ void __launch_bounds__(RSC_THREADS) vadk_resample_cut(const ResampleCutArgs a) {
    using In = WireQuad<FMT, CH>;
    constexpr uint32_t A = RATE == 0 ? 8u : RATE == 1 ? 24u : 48u, ST = A + RSC_SKEW;
    extern __shared__ __attribute__((aligned(16))) float rsc_lds[];
    const CutWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const uint32_t inq = a.inq[w.seg];                                // S_in / 4
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    // the segment's own bytes: the argument check keeps them inside the block, which is under 2 GiB
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(static_cast<const char *>(a.audio)) + ((size_t)qin << In::qsh), 0, (int)(inq << In::qsh), 0x00020000);
    const uint32_t left = sg.nquads - w.quad0, nq = left < (uint32_t)(RSC_WG_SAMPLES / 4) ? left : (uint32_t)(RSC_WG_SAMPLES / 4);
    const uint32_t K = a.ksteps << 4;
    // 1. the span: ceil(nq / 4) row-blocks of A samples and the K - A more that the last one reads, from input quad q0 (signed)
    const uint32_t spanq = (((nq + 3u) >> 2) * A + K) >> 2;
    const int32_t q0 = (int32_t)((w.quad0 >> 2) * (A >> 2)) - (int32_t)(a.n0 >> 2);
    for (uint32_t base = 0; base < spanq; base += RSC_LOADS * RSC_THREADS) {
        typename In::XQ x[RSC_LOADS] = {};
        bool in[RSC_LOADS];
#pragma unroll
        for (int p = 0; p < RSC_LOADS; ++p) {
            const uint32_t lq = base + (uint32_t)(p * RSC_THREADS) + threadIdx.x;
            const int32_t q = q0 + (int32_t)lq;
            in[p] = lq < spanq && q >= 0 && (uint32_t)q < inq;
            if (in[p]) x[p] = In::load(rs, (int)((uint32_t)q << In::qsh));
        }
#pragma unroll
        for (int p = 0; p < RSC_LOADS; ++p) {
            const uint32_t lq = base + (uint32_t)(p * RSC_THREADS) + threadIdx.x;
            if (lq >= spanq) continue;
            const f32x4 d = In::decode(x[p], mode, sc, rsc);
            const uint32_t j = lq << 2;
            *reinterpret_cast<f32x4 *>(rsc_lds + j + RSC_SKEW * (j / A)) = in[p] ? d : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();

    // 2. tiles 2 wave and 2 wave + 1 of the workgroup: 64 output quads each
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, col = lane & 15u, kq = lane >> 4;
    if (wave * 128u >= nq) return;                                    // (no barrier follows)
    const float *xb0 = rsc_lds + (32u * wave + col) * ST + kq, *xb1 = xb0 + 16u * ST;
    const f32x4 *ts = reinterpret_cast<const f32x4 *>(a.op) + lane;
    f32x4 d0{0.f, 0.f, 0.f, 0.f}, d1{0.f, 0.f, 0.f, 0.f};
    for (uint32_t sp = 0; sp < a.ksteps; ++sp) {
        const f32x4 tv = ts[(size_t)sp * 64u];
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            const uint32_t n = 16u * sp + 4u * t, off = n + RSC_SKEW * (n / A);
            const float tk = pick(tv, t);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(tk, xb0[off], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(tk, xb1[off], d1, 0, 0, 0);
        }
    }

    // 3. D: column = row-block `col`, rows = outputs 4 kq + r of it - output quad 4 col + kq of the tile
    float g = 1.0f;
    if (a.gains) g = a.gains[w.seg];
#pragma unroll
    for (uint32_t t = 0; t < 2u; ++t) {
        const uint32_t oq = (2u * wave + t) * 64u + 4u * col + kq;
        if (oq >= nq) continue;
        f32x4 v = t ? d1 : d0;
        if (a.gains) {
#pragma clang fp contract(off)
            v = f32x4{v.x * g, v.y * g, v.z * g, v.w * g};
        }
        const uint64_t o = sg.quad_out + w.quad0 + oq;
        if (a.out_fmt == 0)
            static_cast<u32x2 *>(a.out)[o] = u32x2{pcm16(v.x) | (pcm16(v.y) << 16), pcm16(v.z) | (pcm16(v.w) << 16)};
        else
            static_cast<f32x4 *>(a.out)[o] = v;
    }
}

extern "C" hipError_t vadk_launch_resample_cut(const ResampleCutArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    const int rate = a->sr_in == 8000 ? 0 : a->sr_in == 24000 ? 1 : a->sr_in == 48000 ? 2 : -1;
    if (rate < 0) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (size_t)rsc_lds_floats(rsc_A(a->sr_in), a->ksteps << 4);
    if (lds > 48u * 1024u) return hipErrorInvalidValue;               // (511 taps at 48 kHz: 29 KiB)
    return launch_variant<4, 2, 3>([&](auto F, auto C, auto R) {
        hipLaunchKernelGGL((vadk_resample_cut<F, C + 1, R>), dim3(a->nwork), dim3(RSC_THREADS), lds, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1, rate);
}
