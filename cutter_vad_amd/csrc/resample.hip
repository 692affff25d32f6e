// Batched Fourier resampler to 16 kHz for MI355X / gfx950.
//
// Replaces AudioUtils.resample_audio (/root/reference/src/real_time_vad/utils/audio.py:19-55 ->
// scipy.signal.resample, Fourier method, window=None) for chunks that yield exactly 512 output
// samples: 256 (8 kHz) / 768 (24 kHz) / 1536 (48 kHz) input samples per chunk.
//
// For a fixed (n_in, 512) the Fourier method is a fixed linear operator R[512][n_in]
// (SURVEY §8 a11); the host builds it in double precision from the closed form of scipy's
// spectrum copy (pack_weights.cpp: build_resample_operator) and packs it like every other weight
// stream.  The kernel is the same MFMA skeleton as the model kernels: one workgroup = 32 streams,
// weights (operator rows) on the A operand, the stream tile on the B operand, v_mfma_f32_32x32x2_f32.
// The input is folded about its midpoint on the way into LDS (chunks of 128 folded samples, double
// buffered), which halves the contraction length - see the body's comment (resample_512.h: the kernel's body, shared with
// scan_resample.hip through a loader).
#include <hip/hip_runtime.h>
#include "resample_512.h"
#include "vad_layout.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// dense float32 chunks [n][n_in] through a buffer descriptor: rows past n are out of range and answer zeros
struct DenseRows {
    using XQ = u32x4;
    __amdgpu_buffer_rsrc_t xrs;
    const float *in;
    float *outp;
    int n, n_in, Q, tile0, tid;
    __device__ __forceinline__ XQ load(int it, int q) const {
        const int ms = (it * NTHREADS + tid) >> 4;
        return __builtin_amdgcn_raw_buffer_load_b128(xrs, ((tile0 + ms) * Q + q) * 16, 0, 0);
    }
    __device__ __forceinline__ f32x4 decode(int, XQ v) const { return __builtin_bit_cast(f32x4, v); }
    __device__ __forceinline__ float mid(int j) const {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, ((tile0 + (tid & 31)) * n_in + j) * 4, 0, 0));
    }
    __device__ __forceinline__ float tail(int j) const { return in[(size_t)(tile0 + (tid & 31)) * n_in + j]; }
    __device__ __forceinline__ bool live() const { return tile0 + (tid & 31) < n; }
    __device__ __forceinline__ float *out() const { return outp + (size_t)(tile0 + (tid & 31)) * 512; }
};

}  // namespace

// the body is resample_512.h's (resample_512_tile); here: which segment a workgroup serves, and its dense loader
template <int NT>
__global__ void __launch_bounds__(NTHREADS, 1) vadk_resample_512(const vadk::ResampleParams PP) {
    // which segment does this workgroup serve?  (block-uniform: scalar compares on kernel arguments)
    int sidx = 0;
#pragma unroll
    for (int k = 1; k < RESAMPLE_MAX_SEGS; ++k)
        if (k < PP.nseg && (int)blockIdx.x >= PP.tile_start[k]) sidx = k;
    const vadk::ResampleSeg P = PP.seg[sidx];
    const int tile_in_seg = (int)blockIdx.x - PP.tile_start[sidx];
    const DenseRows L{__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.in), 0, (int)((unsigned)P.n * (unsigned)P.n_in * 4u), 0x00020000),
                      P.in, P.out, P.n, P.n_in, P.n_in >> 2, tile_in_seg * MT, (int)threadIdx.x};
    resample_512_tile<NT>(ResampleOpArgs{P.wstream, P.wstream_bytes, P.tile_blocks, P.row128_block, P.n_in}, L);
}

extern "C" hipError_t vadk_launch_resample(const vadk::ResampleParams *p, hipStream_t stream) {
    (void)hipGetLastError();   // HIP's last-error slot is sticky and process-wide: a stale failure from anywhere else must not become ours
    const int tiles = p->tile_start[p->nseg];
    if (tiles <= 0) return hipSuccess;
    // up to 256 chunk tiles: two workgroups per tile (finer grain also evens out mixed-rate launches, whose 48 kHz tiles run
    // six times longer than their 8 kHz ones)
    if (tiles <= 256)
        hipLaunchKernelGGL(vadk_resample_512<1>, dim3(tiles, 2), dim3(vadk::NTHREADS), 0, stream, *p);
    else
        hipLaunchKernelGGL(vadk_resample_512<2>, dim3(tiles), dim3(vadk::NTHREADS), 0, stream, *p);
    return hipGetLastError();
}
