// The contraction of vadk_resample_512 (resample.hip has the kernel, pack_weights.cpp the operator): one workgroup resamples a tile
// of 32 rows of n_in samples to 512 samples each.  Where a row's samples come from, and where its 512 go, is the LOADER's business:
// resample.hip reads dense float32 chunks [n][n_in], scan_resample.hip frames, decodes and channel-selects them out of a scanned
// block in its wire format.  Everything behind the loader - the fold, the order of the MFMAs, the VALU rows, the recombination - is
// this one body, so two kernels over it give the same bytes for the same float32 chunk.
//
// A loader has:  XQ (a raw quad as loaded), load(it, q) - quad q (samples 4q .. 4q + 3 of the chunk) of the thread's loader row
// `it` (0 / 1: tile row (it * NTHREADS + tid) >> 4), decode(it, XQ) -> f32x4, mid(j) / tail(j) - sample j (a multiple of 4) of tile
// row tid & 31, mid from any thread (zeros for a row that does not exist), tail only where live(); live() - tile row tid & 31 exists;
// out() - where that row's 512 samples go.
#pragma once
#include <hip/hip_runtime.h>
#include "vad_layout.h"
#include "vadk_device.h"

namespace vadk { namespace dev {

// the operator's side of a launch: what ResampleSeg says about the packed stream
struct ResampleOpArgs {
    const float *wstream;
    uint32_t wstream_bytes, tile_blocks, row128_block;
    int32_t n_in;
};

// The operator has a half-period shift symmetry and a mirror symmetry (pack_weights.cpp: pack_resample_operator spells
// out the algebra), so the kernel contracts four folded inputs of length Q = n_in / 4
//   ue / ve = (x[j] + x[j+H]) +/- (x[H-j] + x[n-j]),   uo / vo = (x[j] - x[j+H]) +/- (x[H-j] - x[n-j])      (H = n_in / 2)
// against four 128-row operators (se, ae, so, ao) and recombines
//   y[o] = se+ae+so+ao, y[o+256] = se+ae-so-ao, y[256-o] = se-ae+so-ao, y[512-o] = se-ae-so+ao   (o < 128; 128, 384 on the VALU)
// - a quarter of the dense product's MFMAs.
// NT = 2: one workgroup per chunk tile, wave w = row tile w (o = 32w..32w+31) with all four parts.
// NT = 1: two workgroups (blockIdx.y) share a chunk tile: wave (y, w) = row tile 2y + (w >> 1), parts (se, ae) or (so, ao)
// by w & 1, partner waves swap their sums through LDS at the end - used when the call has too few chunk tiles to fill the
// 256 CUs (the input is read twice, from L2).
template <int NT, class Loader>
__device__ __forceinline__ void resample_512_tile(const ResampleOpArgs P, const Loader &L) {
    constexpr int CH_ROWS = 16;                       // one K chunk = 64 folded samples = 16 quad rows of each of ue, ve, uo, vo
    constexpr int NP = 2 * NT;                        // accumulators per wave
    constexpr int BUF = 4 * CH_ROWS * QS;
    __shared__ f32x4 lds[2 * BUF + 64];
    float *const red = reinterpret_cast<float *>(lds + 2 * BUF);                    // [8 parts][32 streams]: rows 128 / 384
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 31, h = lane >> 5;
    const int hq = h * QS + m;
    const int Q = P.n_in >> 2;                        // folded length in samples = quads per input chunk
    const int nchunks = Q >> 6;
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.wstream), 0, (int)P.wstream_bytes, 0x00020000);
    const int lane16 = lane * 16;
    const int rt = NT == 2 ? w : 2 * (int)blockIdx.y + (w >> 1);     // this wave's 32-row output tile (0..3)
    const int po = NT == 2 ? 0 : (w & 1);                            // NT = 1: 0 = the (se, ae) pair, 1 = (so, ao)
    const int wbase = rt * (int)P.tile_blocks;

    // the one sample each half-size product cannot pair, x[Q] +/- x[Q + H], enters as a rank-1 term: accumulator init
    f32x16 acc[NP];
    {
        const float xa_ = L.mid(Q), xb_ = L.mid(3 * Q);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int tb = wbase + 4 * (NT == 2 ? t : po);
            const float xmid = (NT == 2 ? t : po) == 0 ? xa_ + xb_ : xa_ - xb_;
            const f32x4 r0 = ldw(wrs, lane16, tb), r1 = ldw(wrs, lane16, tb + 1), r2 = ldw(wrs, lane16, tb + 2), r3 = ldw(wrs, lane16, tb + 3);
            acc[2 * t] = f32x16{r0.x * xmid, r0.y * xmid, r0.z * xmid, r0.w * xmid, r1.x * xmid, r1.y * xmid, r1.z * xmid, r1.w * xmid,
                                r2.x * xmid, r2.y * xmid, r2.z * xmid, r2.w * xmid, r3.x * xmid, r3.y * xmid, r3.z * xmid, r3.w * xmid};
            acc[2 * t + 1] = (f32x16)(0.f);
        }
    }

    // chunk loader: 32 streams x 16 folded quads, 2 per thread.  Folded quad q (j = 4q..4q+3) needs x[j] (quad q), x[j+H]
    // (quad q + Q/2), x[H-j] (quad Q/2 - q element 0, quad Q/2 - q - 1 elements 3, 2, 1) and x[n-j] (likewise from Q - q)
    // (the loader's row `it` = tile row (it * NTHREADS + tid) >> 4; a row the call does not have answers zeros)
    typename Loader::XQ xl[2][6];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int q = ((it * NTHREADS + tid) & 15) + 16 * c;
            xl[it][0] = L.load(it, q);
            xl[it][1] = L.load(it, q + (Q >> 1));
            xl[it][2] = L.load(it, (Q >> 1) - q);
            xl[it][3] = L.load(it, (Q >> 1) - q - 1);
            xl[it][4] = L.load(it, q == 0 ? 0 : Q - q);
            xl[it][5] = L.load(it, Q - q - 1);
        }
    };
    auto store_chunk = [&](int c, int buf) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = it * NTHREADS + tid;
            const int ms = idx >> 4, ql = idx & 15;
            const f32x4 a = L.decode(it, xl[it][0]), cc = L.decode(it, xl[it][1]);
            const f32x4 b0 = L.decode(it, xl[it][2]), b1 = L.decode(it, xl[it][3]);
            const f32x4 d0 = L.decode(it, xl[it][4]), d1 = L.decode(it, xl[it][5]);
            const f32x4 b = f32x4{b0.x, b1.w, b1.z, b1.y}, d = f32x4{d0.x, d1.w, d1.z, d1.y};
            const f32x4 pe = a + cc, me = a - cc, qe = b + d, qo = b - d;
            f32x4 ue = pe + qe, ve = pe - qe, uo = me + qo, vo = me - qo;
            if (ql + 16 * c == 0) { ue.x = pe.x; ve.x = 0.f; uo.x = 0.f; vo.x = me.x; }     // j = 0 has no partner
            f32x4 *dst = lds + buf * BUF + ql * QS + ms;
            dst[0] = ue;
            dst[CH_ROWS * QS] = ve;
            dst[2 * CH_ROWS * QS] = uo;
            dst[3 * CH_ROWS * QS] = vo;
        }
    };

    // output rows 128 / 384 on the VALU: thread = (stream tid & 31, part tid >> 5); parts 0..3 dot ue with GSE[128], 4..7 uo
    // with GSO[128], four quads of every chunk each
    float r128 = 0.f;
    const bool do128 = NT == 2 || blockIdx.y == 0;
    const int part = tid >> 5, pr = part & 3, psel = part >> 2;

    // The operator stream does not depend on LDS, so its loads run D k-iterations (about 4 k cycles of MFMA) ahead,
    // across chunk boundaries.  That depth is what hides the next chunk's input loads: loads complete in order, so the
    // first operator block issued after them cannot be consumed before they have come back from HBM.
    constexpr int D = NT == 1 ? 8 : 4;
    f32x4 wq[D][NP], xq[2][NP];
    int ws = wbase + 8 + (NT == 2 ? 0 : 2 * po);           // 8 k-iterations x {SE, AE, SO, AO} per chunk
    const int xrow0 = (NT == 2 ? 0 : 2 * po) * CH_ROWS * QS + hq;
#define R_LDW(slot, j)                                                                          \
    _Pragma("unroll") for (int k = 0; k < NP; ++k) wq[slot][k] = ldw(wrs, lane16, ws + 4 * (j) + k);
#define R_LDX(slot, j)                                                                          \
    _Pragma("unroll") for (int k = 0; k < NP; ++k) xq[slot][k] = X[xrow0 + (k * CH_ROWS + 2 * (j)) * QS];
#pragma unroll
    for (int d = 0; d < D - 1; ++d) { R_LDW(d, d) }
    load_chunk(0);
    store_chunk(0, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const f32x4 *X = lds + (c & 1) * BUF;
        asm volatile("" : "+s"(ws));
        R_LDX(0, 0)
        f32x4 g128[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            R_LDW((j + D - 1) % D, j + D - 1)            // past j = 7: the next chunk's blocks (the stream is contiguous)
            if (j == 0) {
                if (c + 1 < nchunks) load_chunk(c + 1);  // global loads in flight under the MFMAs
                if (do128) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        g128[i] = ldw(wrs, (psel * (Q >> 2) + 16 * c + 4 * pr + i) * 16, (int)P.row128_block);
                }
            }
            if (j + 1 < 8) { R_LDX((j + 1) & 1, j + 1) }
            SB();
#pragma unroll
            for (int k = 0; k < NP; ++k) acc[k] = mfma4(wq[j % D][k], xq[j & 1][k], acc[k]);
            SB();
        }
        ws += 32;
        if (do128) {
            const int ms = tid & 31;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 uu = X[(psel * 2 * CH_ROWS + 4 * pr + i) * QS + ms];
                r128 += g128[i].x * uu.x + g128[i].y * uu.y + g128[i].z * uu.z + g128[i].w * uu.w;
            }
        }
        if (c + 1 < nchunks) store_chunk(c + 1, (c + 1) & 1);   // the other buffer: last read two chunks ago
        __syncthreads();
    }
#undef R_LDW
#undef R_LDX
    // epilogue: lane (m, h) holds rows o = 32 rt + 8g + 4h + i of its parts
    const bool row_live = L.live();           // the row of lane m (= tid & 31) exists: its results are stored
    float *const o = L.out();
    if constexpr (NT == 2) {
        if (row_live) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = 32 * rt + 8 * g + 4 * h;
                const f32x4 se = quad_of(acc[0], g), ae = quad_of(acc[1], g), so = quad_of(acc[2], g), ao = quad_of(acc[3], g);
                const f32x4 pe = se + ae, me = se - ae, pO = so + ao, mO = so - ao;
                *reinterpret_cast<f32x4 *>(o + row) = pe + pO;
                *reinterpret_cast<f32x4 *>(o + 256 + row) = pe - pO;
                const f32x4 lo = me + mO, hi = me - mO;
                if (row != 0) { o[256 - row] = lo.x; o[512 - row] = hi.x; }     // o = 0: rows 256 and 512 = 0 are written above
                o[255 - row] = lo.y; o[511 - row] = hi.y;
                o[254 - row] = lo.z; o[510 - row] = hi.z;
                o[253 - row] = lo.w; o[509 - row] = hi.w;
            }
        }
    } else {
        // partner waves (w ^ 1: the other pair of the same row tile) swap s + a and s - a through the now idle staging area
        f32x4 *const ex = lds;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 s_ = quad_of(acc[0], g), a_ = quad_of(acc[1], g);
            ex[(w * 8 + g) * 64 + lane] = s_ + a_;
            ex[(w * 8 + 4 + g) * 64 + lane] = s_ - a_;
        }
        __syncthreads();
        if (row_live) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = 32 * rt + 8 * g + 4 * h;
                const f32x4 s_ = quad_of(acc[0], g), a_ = quad_of(acc[1], g);
                const f32x4 pp = ex[((w ^ 1) * 8 + g) * 64 + lane], pm = ex[((w ^ 1) * 8 + 4 + g) * 64 + lane];
                if (po == 0) {          // this wave: (se, ae); partner: (so, ao) -> y[o], y[256 - o]
                    *reinterpret_cast<f32x4 *>(o + row) = (s_ + a_) + pp;
                    const f32x4 lo = (s_ - a_) + pm;
                    if (row != 0) o[256 - row] = lo.x;
                    o[255 - row] = lo.y; o[254 - row] = lo.z; o[253 - row] = lo.w;
                } else {                // this wave: (so, ao); partner: (se, ae) -> y[o + 256], y[512 - o]
                    *reinterpret_cast<f32x4 *>(o + 256 + row) = pp - (s_ + a_);
                    const f32x4 hi = pm - (s_ - a_);
                    if (row != 0) o[512 - row] = hi.x;
                    o[511 - row] = hi.y; o[510 - row] = hi.z; o[509 - row] = hi.w;
                }
            }
        }
    }
    if (do128) {
        const int ms = tid & 31;
        red[part * 32 + ms] = r128;
        __syncthreads();
        if (tid < 32 && row_live) {
            float e = 0.f, od = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) { e += red[k * 32 + tid]; od += red[(4 + k) * 32 + tid]; }
            const f32x4 mid = ldw(wrs, (Q >> 1) * 16, (int)P.row128_block);       // floats 2Q, 2Q + 1: RE[128][Q] / 2, RO[128][Q] / 2
            e += mid.x * (L.tail(Q) + L.tail(3 * Q));
            od += mid.y * (L.tail(Q) - L.tail(3 * Q));
            o[128] = e + od;
            o[384] = e - od;
        }
    }
}

} }  // namespace vadk::dev
