// vad_scan_mel: log-mel frames of finished segments, computed out of a scanned block in its wire format (include/vad_engine.h:
// vad_mel).  A segment's samples are exactly the float32 values that vadk_scan_cut with the sample range once (VAD_CUT_RANGE) and
// float32 output would write for it: the same loads, decoders, channel selection and gate (vadk_device.h: WireQuad, gate4).  One
// workgroup serves MEL_TILE consecutive analysis frames of ONE segment (vad_layout.h: MelWork / MelArgs):
//   1. the tile's contiguous span, (frames - 1) hop + n_fft samples, is loaded ONCE and put into LDS as float32 - overlapping
//      frames are neither fetched twice nor written out anywhere.  Reflect padding is an index at load time: a quad that lies
//      inside the segment is one load, a quad that touches an edge picks its four samples from the quads that hold them.
//   2. re / im = operator x frames on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain along n): the operator is the A operand
//      out of the host's packed stream - one coalesced 1 KiB load per wave and four MFMAs - the frames are the B operand out of
//      LDS, whose skewed layout (vad_layout.h: mel_skew) keeps the 64 reads of a fragment in 64 banks at any hop.  The waves split
//      the bin tiles.
//   3. P = fma(re, re, im * im) into LDS as [bin][frame].
//   4. E = P^T x filters on the same MFMA: P is the A operand (row = frame; 64 consecutive floats per fragment), the packed filters
//      the B operand, so D has the mel on the lane.  The waves split the mel tiles; two accumulators (even / odd k-steps) are added
//      at the end.
//   5. floor and log: v_log_f32 times a constant.
//   6. rows [frame][mel] with the lanes along mel.
// Every sum has a fixed order, nothing is accumulated across workgroups: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

static_assert(MEL_TILE == 16, "one 16 x 16 x 4 tile of frames per workgroup");

namespace {

// ln / log10 of max(v, floor) as v_log_f32 times a constant.  v_log_f32 takes no denormal: below 2^-100 the argument is scaled
// by 2^64 (exact) and 64 is taken off the logarithm.  (A NaN comes out as the floor's logarithm: unspecified rows.)
__device__ __forceinline__ float mel_log(float v, float floor, float k) {
    const float m = fmaxf(v, floor);
    const bool tiny = m < 0x1p-100f;
    const float l = __builtin_amdgcn_logf(tiny ? m * 0x1p64f : m);
    return (tiny ? l - 64.0f : l) * k;
}

__device__ __forceinline__ float pick(f32x4 v, uint32_t k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

}  // namespace

// Dynamic LDS: mel_lds_span_floats(n_fft, hop) floats of samples, then bins_pad * MEL_TILE floats of P.  Frames of the tile past
// the segment's last (a segment's last tile) read LDS nobody wrote: every product keeps a frame in its own column (step 2) or row
// (step 4) of D, and the store leaves those rows out.
template <int FMT, int CH>
__global__ void __launch_bounds__(MEL_THREADS) vadk_seg_mel(const MelArgs a) {
    using In = WireQuad<FMT, CH>;
    extern __shared__ __attribute__((aligned(16))) float mel_lds[];
    const MelWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
    // a block is under 2 GiB, so a segment's samples, with the padding, stay below 2^32
    const uint32_t S = sg.nquads << 2, half = a.pad == VAD_MEL_PAD_REFLECT ? a.n_fft >> 1 : 0u, plen = S + 2u * half;
    const uint32_t M = (plen - a.n_fft) / a.hop + 1u;                 // the host lists no tile of a segment without a frame
    const uint32_t nf = M - w.frame0 < (uint32_t)MEL_TILE ? M - w.frame0 : (uint32_t)MEL_TILE;
    const uint32_t spanq = ((nf - 1u) * a.hop + a.n_fft) >> 2, p0 = w.frame0 * a.hop, skew = mel_skew(a.hop);
    float *P = mel_lds + mel_lds_span_floats(a.n_fft, a.hop);

    // 1. the span.  unsigned 32-bit offsets: the argument check keeps every quad of a segment inside the block
    auto quad = [&](uint32_t q) -> f32x4 { return gate4(In::decode(In::load(rs, (int)((qin + q) << In::qsh)), mode, sc, rsc), a.thresh); };
    for (uint32_t lq = threadIdx.x; lq < spanq; lq += MEL_THREADS) {
        const uint32_t li = lq << 2;
        const int32_t i = (int32_t)(p0 + li) - (int32_t)half;         // the segment's sample behind padded sample p0 + li
        f32x4 v;
        if (i >= 0 && (uint32_t)i + 4u <= S) {
            v = quad((uint32_t)i >> 2);
        } else {
            // S > n_fft / 2 (the argument check): one reflection lands inside the segment
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t r0 = i + k, r = r0 < 0 ? -r0 : r0 >= (int32_t)S ? 2 * ((int32_t)S - 1) - r0 : r0;
                t[k] = pick(quad((uint32_t)r >> 2), (uint32_t)r & 3u);
            }
            v = f32x4{t[0], t[1], t[2], t[3]};
        }
        *reinterpret_cast<f32x4 *>(mel_lds + li + skew * (li / a.hop)) = v;
    }
    __syncthreads();

    // 2. and 3.
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, col = lane & 15u, kq = lane >> 4;
    const uint32_t nbt = a.bins_pad >> 4, nsp = a.n_fft >> 3;
    const float *xb = mel_lds + col * (a.hop + skew) + kq;
    for (uint32_t bt = wave; bt < nbt; bt += MEL_THREADS / 64) {
        const f32x4 *ws = reinterpret_cast<const f32x4 *>(a.op) + (size_t)bt * nsp * 64u + lane;
        f32x4 re{0.f, 0.f, 0.f, 0.f}, im{0.f, 0.f, 0.f, 0.f};
        uint32_t off = 0, rem = 0;                                    // n + skew * (n / hop) and n % hop of the k-step's first n
        auto next = [&]() {
            const float x = xb[off];
            off += 4u;
            rem += 4u;
            if (rem == a.hop) { rem = 0; off += skew; }
            return x;
        };
        // two float4 of the stream and four samples in flight per trip (n_fft is a multiple of 16: nsp is even)
        for (uint32_t sp = 0; sp < nsp; sp += 2u) {
            const f32x4 wa = ws[(size_t)sp * 64u], wb = ws[(size_t)sp * 64u + 64u];
            const float x0 = next(), x1 = next(), x2 = next(), x3 = next();
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.x, x0, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.y, x0, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.z, x1, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.w, x1, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.x, x2, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.y, x2, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.z, x3, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.w, x3, im, 0, 0, 0);
        }
        // D: column = frame `col`, rows = bins 16 bt + 4 kq + r
        float *pw = P + (bt * 16u + 4u * kq) * MEL_TILE + col;
        pw[0] = __builtin_fmaf(re.x, re.x, im.x * im.x);
        pw[MEL_TILE] = __builtin_fmaf(re.y, re.y, im.y * im.y);
        pw[2 * MEL_TILE] = __builtin_fmaf(re.z, re.z, im.z * im.z);
        pw[3 * MEL_TILE] = __builtin_fmaf(re.w, re.w, im.w * im.w);
    }
    __syncthreads();

    // 4. to 6.
    const uint32_t nmt = mel_pad16(a.n_mels) >> 4, nks = a.bins_pad >> 4;
    const float klog = a.log == VAD_MEL_LN ? 0.69314718055994531f : 0.30102999566398120f;
    const float *pa = P + kq * MEL_TILE + col;
    for (uint32_t mt = wave; mt < nmt; mt += MEL_THREADS / 64) {
        const f32x4 *fs = reinterpret_cast<const f32x4 *>(a.filters) + (size_t)mt * nks * 64u + lane;
        f32x4 e0{0.f, 0.f, 0.f, 0.f}, e1{0.f, 0.f, 0.f, 0.f};
        for (uint32_t sp = 0; sp < nks; ++sp) {
            const f32x4 fv = fs[(size_t)sp * 64u];
            const float *pp = pa + sp * (16u * MEL_TILE);
            e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pp[0], fv.x, e0, 0, 0, 0);
            e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pp[4 * MEL_TILE], fv.y, e1, 0, 0, 0);
            e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pp[8 * MEL_TILE], fv.z, e0, 0, 0, 0);
            e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pp[12 * MEL_TILE], fv.w, e1, 0, 0, 0);
        }
        const f32x4 ev = e0 + e1;
        // D: column = mel 16 mt + col, rows = frames 4 kq + r
        const uint32_t mel = mt * 16u + col;
        float *o = a.out + ((size_t)sg.quad_out + w.frame0 + 4u * kq) * a.n_mels + mel;
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {
            if (mel >= a.n_mels || 4u * kq + r >= nf) continue;   // (no lane leaves the loop: the next tile's MFMAs want them all)
            const float v = pick(ev, r);
            o[(size_t)r * a.n_mels] = a.log == VAD_MEL_LINEAR ? v : mel_log(v, a.floor, klog);
        }
    }
}

extern "C" hipError_t vadk_launch_seg_mel(const MelArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    const size_t lds = sizeof(float) * ((size_t)mel_lds_span_floats(a->n_fft, a->hop) + (size_t)a->bins_pad * MEL_TILE);
    return launch_variant<4, 2>([&](auto F, auto C) {
        if (lds > 48u * 1024u) {
            const hipError_t r = hipFuncSetAttribute(reinterpret_cast<const void *>(&vadk_seg_mel<F, C + 1>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (r != hipSuccess) return r;
        }
        hipLaunchKernelGGL((vadk_seg_mel<F, C + 1>), dim3(a->nwork), dim3(MEL_THREADS), lds, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1);
}
