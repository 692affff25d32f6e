// vad_scan_cut: the audio of finished segments, gathered out of a scanned block in its wire format and written packed, as int16 PCM
// (a WAV payload) or as float32 (vad_layout.h: CutSeg / CutWork / CutArgs).  A sample of the payload is bit for bit the float32 the
// model's loader read: the same loads (one aligned quad per thread), the same decoders (vadk_device.h: i16_div, g711_quad), the same
// channel selection ((dL + dR) * 0.5f for the mix) and the same gate (gate4) as silero_v5_t16_body.h's decode - restated here, not
// shared: the 33 instantiations of that file stay the code they were.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// FMT: 0 float32, 1 int16 (the divisor is an argument), 2 mu-law, 3 A-law - the numbering of silero_v5_t16.hip's loaders
template <int FMT, int CH>
struct CutIn {
    static constexpr bool f32in = FMT == 0, G711 = FMT >= 2;
    static constexpr int qsh = (f32in ? 4 : G711 ? 2 : 3) + (CH == 2 ? 1 : 0);   // a quad of sample frames: 16 / 8 / 4 bytes per channel
    struct XQ2F { u32x4 a, b; };
    // mono: b128 float32, b64 int16, b32 G.711; two channels: two b128, one b128, one b64
    using XQ = std::conditional_t<CH == 2, std::conditional_t<f32in, XQ2F, std::conditional_t<G711, u32x2, u32x4>>,
                                  std::conditional_t<f32in, u32x4, std::conditional_t<G711, uint32_t, u32x2>>>;
    static __device__ __forceinline__ XQ load(__amdgpu_buffer_rsrc_t rs, int off) {
        if constexpr (CH == 2 && f32in)
            return XQ2F{__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0), __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0)};
        else if constexpr ((CH == 2 && G711) || (CH == 1 && !f32in && !G711)) return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
        else if constexpr (G711) return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
        else return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
    }
    // the loader's decode: both channels through the mono decoders, then left | right | (dL + dR) * 0.5f (an add, then a multiply:
    // np.mean(x, axis=1) of the decoded float32 pair), then the gate on the selected value
    static __device__ __forceinline__ f32x4 decode(XQ b, uint32_t mode, float sc, float rsc, float thr) {
#pragma clang fp contract(off)
        f32x4 v;
        if constexpr (CH == 2) {
            f32x4 dl, dr;
            if constexpr (G711) {
                dl = g711_quad<FMT == 3>(__builtin_amdgcn_perm(b.y, b.x, 0x06040200u));    // codes L0 L1 L2 L3
                dr = g711_quad<FMT == 3>(__builtin_amdgcn_perm(b.y, b.x, 0x07050301u));
            } else if constexpr (!f32in) {
                dl = f32x4{i16_div((int)(short)(b.x & 0xffffu), sc, rsc), i16_div((int)(short)(b.y & 0xffffu), sc, rsc),
                           i16_div((int)(short)(b.z & 0xffffu), sc, rsc), i16_div((int)(short)(b.w & 0xffffu), sc, rsc)};
                dr = f32x4{i16_div((int)(short)(b.x >> 16), sc, rsc), i16_div((int)(short)(b.y >> 16), sc, rsc),
                           i16_div((int)(short)(b.z >> 16), sc, rsc), i16_div((int)(short)(b.w >> 16), sc, rsc)};
            } else {
                dl = __builtin_bit_cast(f32x4, u32x4{b.a.x, b.a.z, b.b.x, b.b.z});
                dr = __builtin_bit_cast(f32x4, u32x4{b.a.y, b.a.w, b.b.y, b.b.w});
            }
            const bool right = mode == SCAN_RIGHT, mix = mode >= SCAN_MIX;
            const f32x4 mx = pk::mul(pk::add(dl, dr), f32x4{0.5f, 0.5f, 0.5f, 0.5f});
            v.x = mix ? mx.x : right ? dr.x : dl.x;
            v.y = mix ? mx.y : right ? dr.y : dl.y;
            v.z = mix ? mx.z : right ? dr.z : dl.z;
            v.w = mix ? mx.w : right ? dr.w : dl.w;
        } else if constexpr (G711) {
            v = g711_quad<FMT == 3>(b);
        } else if constexpr (!f32in) {
            const int s0 = (int)(short)(b.x & 0xffffu), s1 = (int)(short)(b.x >> 16);
            const int s2 = (int)(short)(b.y & 0xffffu), s3 = (int)(short)(b.y >> 16);
            v = f32x4{i16_div(s0, sc, rsc), i16_div(s1, sc, rsc), i16_div(s2, sc, rsc), i16_div(s3, sc, rsc)};
        } else {
            v = __builtin_bit_cast(f32x4, b);
        }
        return gate4(v, thr);
    }
};

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
template <int FMT, int CH, int OUT>
__global__ void __launch_bounds__(CUT_THREADS) vadk_scan_cut(const CutArgs a) {
    using In = CutIn<FMT, CH>;
    const CutWork w = a.work[blockIdx.x];
    const CutSeg sg = a.segs[w.seg];
    const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const uint32_t fmask = a.frame_shift >= 31u ? 0x7fffffffu : (1u << a.frame_shift) - 1u;
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.audio), 0, (int)a.audio_bytes, 0x00020000);
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
        const f32x4 v = In::decode(x[p], mode, sc, rsc, a.thresh);
        const uint64_t o = sg.quad_out + oq;
        if constexpr (OUT == 0)
            static_cast<u32x2 *>(a.out)[o] = u32x2{pcm16(v.x) | (pcm16(v.y) << 16), pcm16(v.z) | (pcm16(v.w) << 16)};
        else
            static_cast<f32x4 *>(a.out)[o] = v;
    }
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
