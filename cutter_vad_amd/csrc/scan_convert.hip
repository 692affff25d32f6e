// vad_convert / vad_scan_convert_segments: whole recordings of a block at any accepted rate (44.1 kHz and its family, 32, 12, 96 kHz ..)
// as ONE continuous signal each at the engine's rate, by a polyphase FIR whose taps are the caller's (include/vad_engine.h: the
// rule; vad_layout.h: ConvertArgs, the periods, the packed operators and the LDS pitch).  An item's input samples are the float32
// values the scans' loader hears before the gate: the same loads, decoders and channel selection (vadk_device.h: WireQuad), no
// gate.  One workgroup serves a run of `nper` consecutive periods of ONE item:
//   1. the run's input span - its periods' own inputs and the taps' reach on either side - is loaded ONCE, quad by quad, decoded and
//      put into LDS as float32.  A sample outside the item's range [0, S_in) is a zero and NO LOAD: the rule zero-extends the item,
//      whatever the block holds there.  The buffer descriptor covers the item's own bytes and nothing else.  S_in is any count: the
//      one quad that holds the item's end is fetched byte by byte, each byte inside the item, and its samples past the end are zeros.
//   2. per row-tile r of the period a banded product on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain along n): T_r, packed by
//      the host in fragment order, is the A operand - one coalesced 1 KiB load per wave and four k-steps, applied to TWO column groups
//      of 16 periods where the run has them - and the span is the B operand out of LDS, column = period.
//   3. D has four consecutive outputs of one period on a lane: one float32 quad.  The quad that holds the item's last output carries
//      +0.0 behind it: the padding to the next item's start comes from the same launch.
// Every sum has a fixed order and nothing is accumulated across workgroups: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

__device__ __forceinline__ float pick(f32x4 v, uint32_t k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

constexpr int CV_LOADS = 4;       // quads a thread requests back to back

// the first nb bytes of a quad, byte by byte (every load inside the descriptor's range), the rest zeros
template <class XQ>
__device__ __forceinline__ XQ load_bytes(__amdgpu_buffer_rsrc_t rs, int off, uint32_t nb) {
    constexpr int W = (int)(sizeof(XQ) / 4);
    uint32_t w[W] = {};
#pragma unroll
    for (int b = 0; b < 4 * W; ++b)
        if ((uint32_t)b < nb) w[b >> 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, off + b, 0, 0) << (8 * (b & 3));
    XQ x;
    __builtin_memcpy(&x, w, sizeof(XQ));
    return x;
}

// one unit of a wave: row-tile r on column group ga and - TWO - on gb.  xa / xb: the columns' first floats in LDS; c: the lane's
// first sample of the column (shift + base_r + kq)
template <bool TWO>
__device__ __forceinline__ void product(const f32x4 *ts, uint32_t ksteps, const float *xa, const float *xb, uint32_t c, uint32_t PI, uint32_t skew,
                                        f32x4 &d0, f32x4 &d1) {
    const uint32_t qd = c / PI;
    uint32_t rem = c - qd * PI, off = c + skew * qd;
    for (uint32_t sp = 0; sp < ksteps; ++sp) {
        const f32x4 tv = ts[(size_t)sp * 64u];
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            const float tk = pick(tv, t);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(tk, xa[off], d0, 0, 0, 0);
            if (TWO) d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(tk, xb[off], d1, 0, 0, 0);
            rem += 4u;
            off += 4u;
            while (rem >= PI) {
                rem -= PI;
                off += skew;
            }
        }
    }
}

}  // namespace

static_assert(VAD_CONVERT_WG_SAMPLES == CV_WG_SAMPLES, "the header's workgroup share is the kernel's");

// Dynamic LDS: cv_lds_floats(nper, ..) floats.  Columns past the run's last period read the last period's samples (the address is
// clamped into the span) and are not stored.
template <int FMT, int CH>
__global__ void __launch_bounds__(CV_THREADS) vadk_convert(const ConvertArgs a) {
    using In = WireQuad<FMT, CH>;
    using XQ = typename In::XQ;
    extern __shared__ __attribute__((aligned(16))) float cv_lds[];
    const ConvertWork w = a.work[blockIdx.x];
    const ConvertItem it = a.items[w.item];
    const uint32_t mode = it.quad_in >> SCAN_MODE_SHIFT, qin = it.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
    const uint32_t S_in = it.s_in, S_out = it.s_out, PI = a.PI, P = a.P, skew = cv_skew(PI), pitch = PI + skew;
    const float sc = a.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    constexpr uint32_t fsh = In::qsh - 2;                              // log2 of a sample frame's bytes
    // the item's own bytes: the argument check keeps them inside the block, which is under 2 GiB
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(static_cast<const char *>(a.audio)) + ((size_t)qin << In::qsh), 0, (int)(S_in << fsh), 0x00020000);
    const uint32_t nperiods = (S_out + P - 1u) / P, p0 = w.run * a.nper;
    if (p0 >= nperiods) return;                                        // (the host lists no such run; no barrier was passed)
    const uint32_t np = nperiods - p0 < a.nper ? nperiods - p0 : a.nper;
    const uint32_t K = a.ksteps << 4, lead = cv_lead(a.ntaps, a.L);
    // 1. the span, from input quad q0 (signed): `shift` samples ahead of the run's first period
    const int32_t q0 = ((int32_t)(p0 * PI) - (int32_t)lead) >> 2;
    const uint32_t shift = (uint32_t)((int32_t)(p0 * PI) - 4 * q0);
    const uint32_t spanq = (uint32_t)((int32_t)(shift + (np - 1u) * PI + K) + a.bmax + 3) >> 2;
    for (uint32_t base = 0; base < spanq; base += CV_LOADS * CV_THREADS) {
        XQ x[CV_LOADS] = {};
        bool in[CV_LOADS];
#pragma unroll
        for (int p = 0; p < CV_LOADS; ++p) {
            const uint32_t lq = base + (uint32_t)(p * CV_THREADS) + threadIdx.x;
            const int32_t q = q0 + (int32_t)lq;
            in[p] = lq < spanq && q >= 0 && ((uint32_t)q << 2) < S_in;
            if (in[p]) {
                const uint32_t k = (uint32_t)q << 2;
                if (k + 4u <= S_in) x[p] = In::load(rs, (int)((uint32_t)q << In::qsh));
                else x[p] = load_bytes<XQ>(rs, (int)((uint32_t)q << In::qsh), (S_in - k) << fsh);
            }
        }
#pragma unroll
        for (int p = 0; p < CV_LOADS; ++p) {
            const uint32_t lq = base + (uint32_t)(p * CV_THREADS) + threadIdx.x;
            if (lq >= spanq) continue;
            f32x4 d{0.f, 0.f, 0.f, 0.f};
            if (in[p]) {
                d = In::decode(x[p], mode, sc, rsc);
                const uint32_t k = (uint32_t)(q0 + (int32_t)lq) << 2;       // (a zero code of G.711 or the mix of zeros is no zero sample)
                d.y = k + 1u < S_in ? d.y : 0.f;
                d.z = k + 2u < S_in ? d.z : 0.f;
                d.w = k + 3u < S_in ? d.w : 0.f;
            }
            const uint32_t j = lq << 2;
            uint32_t qd = j / PI, rem = j - qd * PI;
#pragma unroll
            for (uint32_t t = 0; t < 4u; ++t) {
                cv_lds[j + t + skew * qd] = pick(d, t);
                if (++rem == PI) {
                    rem = 0;
                    ++qd;
                }
            }
        }
    }
    __syncthreads();

    // 2. units of the workgroup: row-tile r on a pair of column groups (the last pair of an odd count is a single group)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, col = lane & 15u, kq = lane >> 4;
    const uint32_t G = (np + 15u) >> 4, GH = (G + 1u) >> 1, units = a.ntiles * GH;
    for (uint32_t u = wave; u < units; u += CV_THREADS / 64) {
        const uint32_t r = u / GH, ga = 2u * (u - r * GH), gb = ga + 1u;
        const bool two = gb < G;
        const uint32_t ca = 16u * ga + col, cb = 16u * gb + col;
        const float *xa = cv_lds + (ca < np ? ca : np - 1u) * pitch, *xb = cv_lds + (cb < np ? cb : np - 1u) * pitch;
        const uint32_t c = (uint32_t)((int32_t)shift + cv_base(r, a.ntaps, a.L, a.M)) + kq;
        const f32x4 *ts = reinterpret_cast<const f32x4 *>(a.op) + (size_t)r * a.ksteps * 64u + lane;
        f32x4 d0{0.f, 0.f, 0.f, 0.f}, d1{0.f, 0.f, 0.f, 0.f};
        if (two) product<true>(ts, a.ksteps, xa, xb, c, PI, skew, d0, d1);
        else product<false>(ts, a.ksteps, xa, xb, c, PI, skew, d0, d1);

        // 3. D: column = period, rows = outputs 16 r + 4 kq + i of it
#pragma unroll
        for (uint32_t t = 0; t < 2u; ++t) {
            const uint32_t cc = t ? cb : ca;
            if ((t && !two) || cc >= np) continue;
            const uint32_t m = (p0 + cc) * P + 16u * r + 4u * kq;
            if (m >= S_out) continue;                                  // (the item's last quad starts below S_out)
            f32x4 v = t ? d1 : d0;
            v.y = m + 1u < S_out ? v.y : 0.f;
            v.z = m + 2u < S_out ? v.z : 0.f;
            v.w = m + 3u < S_out ? v.w : 0.f;
            reinterpret_cast<f32x4 *>(a.out)[(size_t)it.quad_out + (m >> 2)] = v;
        }
    }
}

extern "C" hipError_t vadk_launch_convert(const ConvertArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->nwork == 0) return hipSuccess;
    if (a->nper == 0 || a->ntiles * 16u != a->P) return hipErrorInvalidValue;
    const uint32_t floats = cv_lds_floats(a->nper, a->PI, cv_lead(a->ntaps, a->L), a->bmax, a->ksteps << 4);
    if (floats > CV_LDS_FLOATS) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (size_t)floats;
    return launch_variant<4, 2>([&](auto F, auto C) {
        hipLaunchKernelGGL((vadk_convert<F, C + 1>), dim3(a->nwork), dim3(CV_THREADS), lds, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1);
}
