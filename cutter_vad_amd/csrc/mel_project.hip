// vad_mel_project: a projection of a feature matrix, y [rows][n_out] = bias + x [rows][n_in] * op [n_in][n_out] in float32
// (include/vad_engine.h: vad_mel_project; vad_layout.h: ProjArgs, proj_pack_index) - the DCT of MFCC and LFCC, or any learned linear
// front end, over the rows vadk_seg_mel left on the GPU.  No audio is read.
//
// vadk_mel_project.  One workgroup per PROJ_ROWS consecutive rows:
//   1. the rows of the tile - one contiguous run of the matrix - are loaded with the lanes along the row, plain dwords (the matrix
//      is 4-byte aligned, no more), into LDS at the odd pitch up4(n_in) | 1.  Columns n_in .. up4(n_in) - 1 of all PROJ_ROWS rows are
//      written with +0.0: a pad lane of the last k-step would else read whatever LDS held, and NaN * 0 is NaN.  Rows past the matrix
//      are not written: what they hold reaches only accumulator rows that are never stored.
//   2. each wave owns 16 rows and walks the column tiles: v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain along k ascending, from
//      the bias the accumulators start with) with the rows as the A operand out of LDS - row on lane % 16, k on lane / 16 - and the
//      operator as the B operand out of the host's packed stream, one coalesced 256-byte load per k-step, which stays in L2.
//   3. D has the column on lane % 16 and rows 4 (lane / 16) + r: each of the four stores of a lane is part of a 64-byte run along
//      the output row.  Columns past n_out and rows past the matrix are not stored.
// A row's value depends on that row, the operator and the bias alone: not on where the row lies in its tile, in the matrix or in
// the launch.  Every output cell is written by exactly one lane, nothing is accumulated across lanes' stores: two runs give the
// same bytes.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "vad_layout.h"

using namespace vadk;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(PROJ_THREADS) vadk_mel_project(const ProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) float proj_lds[];
    const uint32_t n_in = a.n_in, n_out = a.n_out, K4 = proj_up4(n_in), pitch = proj_pitch(n_in), nks = K4 >> 2, nct = proj_up16(n_out) >> 4;
    const uint64_t row0 = (uint64_t)blockIdx.x * PROJ_ROWS;
    const uint32_t nr = a.rows - row0 < (uint64_t)PROJ_ROWS ? (uint32_t)(a.rows - row0) : (uint32_t)PROJ_ROWS;

    // 1. nr * n_in consecutive floats of the matrix
    {
        const float *x = a.x + (size_t)row0 * n_in;
        const uint32_t total = nr * n_in, step_r = PROJ_THREADS / n_in, step_j = PROJ_THREADS % n_in;
        uint32_t r = threadIdx.x / n_in, j = threadIdx.x % n_in;
        // PROJ_LOADS loads of a thread go out before the first of them is waited for and put into LDS
        for (uint32_t i0 = threadIdx.x; i0 < total; i0 += PROJ_LOADS * PROJ_THREADS) {
            float v[PROJ_LOADS];
#pragma unroll
            for (uint32_t u = 0; u < PROJ_LOADS; ++u) {
                const uint32_t i = i0 + u * PROJ_THREADS;
                v[u] = i < total ? x[i] : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < PROJ_LOADS; ++u) {
                if (i0 + u * PROJ_THREADS < total) proj_lds[r * pitch + j] = v[u];
                r += step_r;
                j += step_j;
                if (j >= n_in) { j -= n_in; ++r; }
            }
        }
        const uint32_t npad = K4 - n_in;
        for (uint32_t i = threadIdx.x; i < PROJ_ROWS * npad; i += PROJ_THREADS) proj_lds[(i / npad) * pitch + n_in + i % npad] = 0.0f;
    }
    __syncthreads();

    // 2. rows 16 wave .. + 15 of the tile
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, col = lane & 15u, kq = lane >> 4;
    if (16u * wave >= nr) return;
    const float *ap = proj_lds + (16u * wave + col) * pitch + kq;
    const float *bias = a.op + (size_t)K4 * (nct * 16u);
    for (uint32_t ct = 0; ct < nct; ++ct) {
        const float *bp = a.op + (size_t)ct * nks * 64u + lane;
        const float b0 = bias[ct * 16u + col];
        f32x4 acc{b0, b0, b0, b0};
        // PROJ_LOADS k-steps' fragments are requested - A out of LDS, B out of L2 - before the first of their MFMAs, which stay one
        // chain in the order of k
        for (uint32_t ks0 = 0; ks0 < nks; ks0 += PROJ_LOADS) {
            float av[PROJ_LOADS], bv[PROJ_LOADS];
#pragma unroll
            for (uint32_t u = 0; u < PROJ_LOADS; ++u) {
                const uint32_t ks = ks0 + u;
                av[u] = ks < nks ? ap[4u * ks] : 0.0f;
                bv[u] = ks < nks ? bp[(size_t)ks * 64u] : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < PROJ_LOADS; ++u)
                if (ks0 + u < nks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
        }
        // 3. D: column 16 ct + col, rows 16 wave + 4 kq + r
        const uint32_t c = ct * 16u + col, r0 = 16u * wave + 4u * kq;
        if (c >= n_out) continue;
        float *o = a.out + ((size_t)row0 + r0) * n_out + c;
        if (r0 < nr) o[0] = acc.x;
        if (r0 + 1u < nr) o[n_out] = acc.y;
        if (r0 + 2u < nr) o[2u * n_out] = acc.z;
        if (r0 + 3u < nr) o[3u * n_out] = acc.w;
    }
}

extern "C" hipError_t vadk_launch_mel_project(const ProjArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->rows == 0) return hipSuccess;
    if (a->n_in < 1 || a->n_in > (uint32_t)PROJ_MAX || a->n_out < 1 || a->n_out > (uint32_t)PROJ_MAX) return hipErrorInvalidValue;
    const uint64_t groups = (a->rows + PROJ_ROWS - 1) / PROJ_ROWS;
    if (groups > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (size_t)PROJ_ROWS * proj_pitch(a->n_in);
    hipLaunchKernelGGL(vadk_mel_project, dim3((uint32_t)groups), dim3(PROJ_THREADS), lds, stream, *a);
    return hipGetLastError();
}
