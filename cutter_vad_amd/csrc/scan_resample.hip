// vad_scan_rate: whole recordings at 8 / 24 / 48 kHz, framed at their own rate and resampled to the model's 512-sample frames on
// the GPU (vad_layout.h: ScanResampleArgs).  The block stays in its wire format; a chunk is framed out of it as the scans frame a
// frame (nothing is copied when chunks overlap), decoded and channel-selected by the scans' loader arithmetic (vadk_device.h:
// WireQuad - i16_div, g711_quad, (dL + dR) * 0.5f for the mix; NO gate: the gate and the non-finite check act on the resampled
// frame, in the model kernel), and contracted by vadk_resample_512's body (resample_512.h): for the same float32 chunk the row
// is byte for byte what vad_resample writes.
#include <hip/hip_runtime.h>
#include "../../include/vad_engine.h"
#include "resample_512.h"
#include "vad_layout.h"
#include "vadk_device.h"

using namespace vadk;
using namespace vadk::dev;

namespace {

// rows framed out of the block: tile row r = row g = tile0 + r of the window = (item g / W, chunk t0 + g % W).  A thread serves
// three rows - its two loader rows and row tid & 31 - and keeps each one's byte offset in the block and channel mode.  A row that
// does not exist (past the live items, or past its item's last chunk) is addressed past every block: the descriptor answers 0.
template <int FMT, int CH>
struct ScanRows {
    using In = WireQuad<FMT, CH>;
    using XQ = typename In::XQ;
    static constexpr uint32_t DEAD = 0x80000000u;     // a block is under 2 GiB
    __amdgpu_buffer_rsrc_t rs;
    uint32_t off[3], mode[3];
    float sc, rsc;
    float *outp;
    bool live_;
    __device__ __forceinline__ ScanRows(const ScanResampleArgs &A, int tile0, int tid) {
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(A.audio), 0, (int)A.audio_bytes, 0x00020000);
        sc = A.fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f;
        rsc = 1.0f / sc;
        const int rows[3] = {tid >> 4, (NTHREADS + tid) >> 4, tid & 31};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int g = tile0 + rows[k], i = g / A.W, tt = g - i * A.W;
            off[k] = DEAD;
            mode[k] = 0;
            bool ok = false;
            if (i < A.live) {
                const ScanItem it = A.items[i];
                if (A.t0 + tt < it.nframes) {
                    // the argument check keeps every chunk of an item inside the block: the byte offset is under 2^31
                    const uint32_t quad = (it.quad0 & ((1u << SCAN_MODE_SHIFT) - 1u)) + (uint32_t)(A.t0 + tt) * A.hopq;
                    off[k] = quad << In::qsh;
                    mode[k] = it.quad0 >> SCAN_MODE_SHIFT;
                    ok = true;
                }
            }
            if (k == 2) {
                live_ = ok;
                outp = A.win + (size_t)g * 512;
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

// NT as vadk_resample_512: 2 = one workgroup per tile of 32 rows, 1 = two (blockIdx.y) when the window has few tiles.
template <int NT, int FMT, int CH>
__global__ void __launch_bounds__(NTHREADS, 1) vadk_scan_resample(const ScanResampleArgs A) {
    // the window's item table, for the model launch behind this one: entry i by thread i of the grid's first workgroups (a window
    // has at least live / 32 tiles); the order is the sorted table's, so the counts stay non-increasing
    if (blockIdx.y == 0) {
        const int i = (int)blockIdx.x * NTHREADS + (int)threadIdx.x;
        if (i < A.live) {
            const ScanItem it = A.items[i];
            const int left = it.nframes - A.t0;
            A.items_win[i] = ScanItem{it.slot, (uint32_t)i * (uint32_t)A.W * 128u, left < 0 ? 0 : left > A.W ? A.W : left, it.out0 + (uint32_t)A.t0};
        }
    }
    // a tile without a row to store ends here (block-uniform).  The table is sorted by frame count, descending, and the live items
    // all have a chunk in the window: the tile has a row iff its first row has one (the item's chunks t0 + tt go on that far) or a
    // second live item begins inside it
    const int tile0 = (int)blockIdx.x * MT, i0 = tile0 / A.W;
    bool any = false;
    if (i0 < A.live) {
        any = A.t0 + (tile0 - i0 * A.W) < A.items[i0].nframes;
        if (!any && (tile0 + MT - 1) / A.W > i0) any = i0 + 1 < A.live;
    }
    if (!any) return;
    const ScanRows<FMT, CH> L(A, tile0, (int)threadIdx.x);
    resample_512_tile<NT>(ResampleOpArgs{A.wstream, A.wstream_bytes, A.tile_blocks, A.row128_block, A.n_in}, L);
}

extern "C" hipError_t vadk_launch_scan_resample(const ScanResampleArgs *a, hipStream_t stream) {
    (void)hipGetLastError();
    const long long rows = (long long)a->live * a->W;
    if (rows <= 0) return hipSuccess;
    const int tiles = (int)((rows + MT - 1) / MT);
    return launch_variant<4, 2>([&](auto F, auto C) {
        if (tiles <= 256) hipLaunchKernelGGL((vadk_scan_resample<1, F, C + 1>), dim3(tiles, 2), dim3(NTHREADS), 0, stream, *a);
        else hipLaunchKernelGGL((vadk_scan_resample<2, F, C + 1>), dim3(tiles), dim3(NTHREADS), 0, stream, *a);
        return hipGetLastError();
    }, wire_fmt(a->fmt), (int)a->channels - 1);
}
