// vad_scan_rate_cut (VAD_CUT_FRAMES): the frames the model read of finished segments of a block at 8 / 24 / 48 kHz (vad_layout.h:
// CutResampleArgs).  The rows of a call are the chunks of the listed segments, in listing order; a chunk is framed out of the block
// in its wire format, decoded and channel-selected by the scans' loader arithmetic (vadk_device.h: WireQuad; NO gate here) and
// contracted by vadk_resample_512's body (resample_512.h) - the loader of scan_resample.hip with another map from row to chunk, so
// a row is byte for byte what vad_resample writes for the decoded float32 chunk, and what the rate scan's model launch read.  The
// rows land in the engine's window buffer; vadk_scan_cut (scan_cut.hip) gates them and writes the payload.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "resample_512.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// tile row k = row r = tile0 + k of the call.  A thread serves three rows - its two loader rows and row tid & 31 - and keeps each
// one's byte offset in the block and channel mode.  A row past the launch's last one is addressed past every block: the
// descriptor answers 0.
template <int FMT, int CH>
struct CutRows {
    using In = WireQuad<FMT, CH>;
    using XQ = typename In::XQ;
    static constexpr uint32_t DEAD = 0x80000000u;     // a block is under 2 GiB
    __amdgpu_buffer_rsrc_t rs;
    uint32_t off[3], mode[3];
    float sc, rsc;
    float *outp;
    bool live_;
    __device__ __forceinline__ CutRows(const CutResampleArgs &A, uint32_t tile0, int tid) {
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(A.audio), 0, (int)A.audio_bytes, 0x00020000);
        sc = A.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f;
        rsc = 1.0f / sc;
        const uint32_t first = A.tile_seg[tile0 / (uint32_t)MT];
        const int rows[3] = {tid >> 4, (NTHREADS + tid) >> 4, tid & 31};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t r = tile0 + (uint32_t)rows[k];
            off[k] = DEAD;
            mode[k] = 0;
            const bool ok = r < A.rows_end;
            if (ok) {
                // segs ends with a record whose row0 is the call's row count (> r): the walk stops inside the table, and after at
                // most 31 steps - `first` owns the tile's first row and every segment has a row
                uint32_t s = first;
                while (A.segs[s + 1].row0 <= r) ++s;
                const CutResampleSeg sg = A.segs[s];
                // the argument check keeps every chunk of a segment inside the block: the byte offset is under 2^31
                const uint32_t quad = (sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u)) + (r - sg.row0) * A.hopq;
                off[k] = quad << In::qsh;
                mode[k] = sg.quad_in >> SCAN_MODE_SHIFT;
            }
            if (k == 2) {
                live_ = ok;
                outp = A.win + (size_t)(r - A.r0) * 512;
            }
        }
    }
    __device__ __forceinline__ XQ load(int it, int q) const { return In::load(rs, (int)(off[it] + ((uint32_t)q << In::qsh))); }
    __device__ __forceinline__ f32x4 decode(int it, XQ v) const { return In::decode(v, mode[it], sc, rsc); }
    __device__ __forceinline__ float mid(int j) const {
        return In::decode(In::load(rs, (int)(off[2] + ((uint32_t)(j >> 2) << In::qsh))), mode[2], sc, rsc).x;
    }
    __device__ __forceinline__ float tail(int j) const { return mid(j); }
    __device__ __forceinline__ bool live() const { return live_; }
    __device__ __forceinline__ float *out() const { return outp; }
};

}  // namespace

// NT as vadk_scan_resample: 2 = one workgroup per tile of 32 rows, 1 = two (blockIdx.y) when the launch has few tiles.  Every tile
// of the grid has a row (the grid is ceil((rows_end - r0) / 32) tiles).
template <int NT, int FMT, int CH>
__global__ void __launch_bounds__(NTHREADS, 1) vadk_cut_resample(const CutResampleArgs A) {
    const CutRows<FMT, CH> L(A, A.r0 + (uint32_t)blockIdx.x * (uint32_t)MT, (int)threadIdx.x);
    resample_512_tile<NT>(ResampleOpArgs{A.wstream, A.wstream_bytes, A.tile_blocks, A.row128_block, A.n_in}, L);
}

extern "C" hipError_t vadk_launch_cut_resample(const CutResampleArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a->rows_end <= a->r0) return hipSuccess;
    if (a->r0 % (uint32_t)MT) return hipErrorInvalidValue;
    const int tiles = (int)((a->rows_end - a->r0 + (uint32_t)MT - 1u) / (uint32_t)MT);
    return launch_variant<4, 2>([&](auto F, auto C) {
        if (tiles <= 256) hipLaunchKernelGGL((vadk_cut_resample<1, F, C + 1>), dim3(tiles, 2), dim3(NTHREADS), 0, stream, *a);
        else hipLaunchKernelGGL((vadk_cut_resample<2, F, C + 1>), dim3(tiles), dim3(NTHREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1);
}
