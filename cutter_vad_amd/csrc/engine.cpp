// C ABI of the batched Silero-VAD engine (include/vad_engine.h): stream pool, device state,
// host<->device staging and kernel launches.  Plain C++ over the HIP runtime API; the kernels
// live in silero_v5.hip / silero_v4.hip / resample.hip and are reached through
// vadk_launch_* so that this file never needs device compilation.
//
// Reference behaviour mirrored here (paths under /root/reference/src/real_time_vad/):
//   core/silero_model.py:276-334  model load            -> vad_engine_create
//   core/silero_model.py:384-401  zero-initialised state -> vad_stream_open / vad_stream_reset
//   core/silero_model.py:403-447  predict               -> vad_step*
//   core/silero_model.py:548-566  get_model_info        -> vad_engine_info
// There is deliberately no CPU execution path in this file.
#include "../../include/vad_engine.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdlib>
#include <new>
#include <chrono>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <array>
#include <vector>

#include "pack_weights.h"
#include "resample_generic.h"
#include "vad_layout.h"

extern "C" hipError_t vadk_launch_silero_v5(const vadk::StepParams *p, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v4(const vadk::StepParams *p, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v5_t16(const vadk::StepParams *p, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v5_t16_pair(const vadk::StepParams *p, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v4_t16(const vadk::StepParams *p, int one_per_cu, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v5_t16_rates(const vadk::StepParams *p, const vadk::RateParams *r, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v5_scan16(const vadk::StepParams *p, const vadk::ScanItem *items, const vadk::ScanArgs *a,
                                                   hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_cut(const vadk::CutArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_cut_gain(const vadk::CutArgs *a, const float *gains, hipStream_t stream);
extern "C" hipError_t vadk_launch_seg_levels(const vadk::CutArgs *a, float clip, hipStream_t stream);
extern "C" hipError_t vadk_launch_seg_moments(const vadk::CutArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_audio_batch(const vadk::AudioBatchArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_seg_mel(const vadk::MelArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_resample_cut(const vadk::ResampleCutArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_convert(const vadk::ConvertArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_mel_stats(const vadk::MelStatsArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_mel_project(const vadk::ProjArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_mel_batch(const vadk::MelBatchArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_mel_batch_packed(const vadk::MelPackArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_render(const vadk::RenderArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_cut_stereo(const vadk::CutArgs *a, const float *gains, hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_render_stereo(const vadk::RenderArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_segments(const vadk::SegArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_seg_stats(const vadk::SegArgs *a, uint32_t most, hipStream_t stream);
extern "C" hipError_t vadk_launch_reseg_count(const vadk::ResegArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_reseg_fill(const vadk::ResegArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_reseg_tails(const vadk::ResegArgs *a, uint32_t *tail_len, hipStream_t stream);
extern "C" hipError_t vadk_launch_tail_snapshot(const vadk::TailArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_seg_tails(const vadk::TailArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_refine_count(const vadk::RefineArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_refine_fill(const vadk::RefineArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_scan_resample(const vadk::ScanResampleArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_cut_resample(const vadk::CutResampleArgs *a, hipStream_t stream);
extern "C" hipError_t vadk_launch_resample(const vadk::ResampleParams *p, hipStream_t stream);
extern "C" hipError_t vadk_launch_slot_control(vadk::SmSlot *sm, float *state, const int32_t *d_slots, int n, int op,
                                               const vadk::SmSlot *def, const vad_thresholds *d_thr, int nthr, hipStream_t stream);
extern "C" hipError_t vadk_launch_sm_replay(vadk::SmSlot *sm, int slot, const float *probs, int n, uint8_t *events,
                                            int32_t *seg, hipStream_t stream);
extern "C" hipError_t vadk_launch_g711_expand(const void *d_in, int16_t *d_out, int64_t nbytes, int alaw, hipStream_t stream);

namespace {

thread_local std::string g_create_error;
thread_local std::string g_error_copy;      // vad_last_error hands out a copy taken under the engine's mutex

const vadk::SmSlot kDefaultSm = [] {
    vadk::SmSlot s;
    std::memset(&s, 0, sizeof s);
    // VADConfig defaults, core/config.py:54-94
    s.start_prob = 0.7; s.end_prob = 0.7; s.start_ratio = 0.8; s.end_ratio = 0.95;
    s.start_count = 10; s.end_count = 50;
    s.seg_frames = -1;
    return s;
}();

}  // namespace

// Packed weight streams on a device, shared by every engine of the process that was created from the same bytes on that device
// (a sharded pool with several engines per GPU, two pools side by side: one copy in HBM - and in the L2s, which the engines' launches
// then share: two pools of 4 096 streams on one GPU step in 41.0 us with one copy, 41.9 with two).  Immutable after the upload;
// reference counted; freed with the last engine.
struct DeviceWeights {
    int device = 0;
    std::vector<float> host;          // the key: the packed stream itself
    float *dev = nullptr;
    int refs = 0;
};
static std::mutex g_weights_mu;
static std::vector<DeviceWeights *> g_weights;

// the device copy of `data` on `device` (the caller has made it the current device); +1 reference
static hipError_t weights_acquire(int device, const std::vector<float> &data, float **out) {
    std::lock_guard<std::mutex> lk(g_weights_mu);
    for (DeviceWeights *w : g_weights)
        if (w->device == device && w->host.size() == data.size() && std::memcmp(w->host.data(), data.data(), data.size() * sizeof(float)) == 0) {
            w->refs += 1;
            *out = w->dev;
            return hipSuccess;
        }
    DeviceWeights *w = new DeviceWeights;
    w->device = device;
    w->host = data;
    hipError_t r = hipMalloc((void **)&w->dev, data.size() * sizeof(float));
    if (r == hipSuccess) r = hipMemcpy(w->dev, data.data(), data.size() * sizeof(float), hipMemcpyHostToDevice);
    if (r != hipSuccess) {
        if (w->dev) (void)hipFree(w->dev);
        delete w;
        return r;
    }
    w->refs = 1;
    g_weights.push_back(w);
    *out = w->dev;
    return hipSuccess;
}

static void weights_release(float *dev) {
    if (!dev) return;
    std::lock_guard<std::mutex> lk(g_weights_mu);
    for (size_t i = 0; i < g_weights.size(); ++i)
        if (g_weights[i]->dev == dev) {
            if (--g_weights[i]->refs == 0) {
                (void)hipFree(dev);
                delete g_weights[i];
                g_weights.erase(g_weights.begin() + (long)i);
            }
            return;
        }
}

struct vad_engine {
    int version = 5;
    int device = 0;
    int max_streams = 0;
    hipStream_t stream = nullptr;
    float *d_wstream = nullptr;
    size_t wbytes = 0;
    float *d_state = nullptr;
    vadk::SmSlot *d_sm = nullptr;
    // staging for the host-pointer entry points (grown on demand)
    void *d_frames = nullptr;  size_t d_frames_cap = 0;
    float *d_probs = nullptr;  size_t d_probs_cap = 0;
    uint8_t *d_events = nullptr; size_t d_events_cap = 0;
    int32_t *d_seg = nullptr;  size_t d_seg_cap = 0;
    int32_t *d_slots = nullptr; size_t d_slots_cap = 0;
    // whole recordings (vad_scan): the audio block and the work items on the device; the item table as it was uploaded (it must
    // outlive the copy).  One launch covers at most scan_launch_frames frames of every recording: 0 = SCAN_LAUNCH_FRAMES, chosen
    // with the aim that a launch with one tile per CU stays of the order of 10 ms on a GPU that others share.  An expectation, not
    // a measurement: the one figure at hand is the single-frame form's 25.5 us per frame of 4 096 streams (README, "other configs"),
    // the frame loop's own per-frame time is what tools/bench_configs.py scan_ingest (b) measures
    static constexpr int SCAN_LAUNCH_FRAMES = 192;
    int scan_launch_frames = 0;
    void *d_audio = nullptr; size_t d_audio_cap = 0;
    vadk::ScanItem *d_items = nullptr; size_t d_items_cap = 0;
    // vad_scan_rate: one launch window's resampled frames [live][W][512] f32 and its item table, written by vadk_scan_resample and
    // read by the model launch behind it.  live * W * 2 KiB stays within SCAN_RATE_WIN_BYTES (which the window size W is cut to):
    // far under the 2 GiB a buffer descriptor addresses.
    static constexpr size_t SCAN_RATE_WIN_BYTES = size_t(256) << 20;
    float *d_win = nullptr; size_t d_win_cap = 0;
    vadk::ScanItem *d_items_win = nullptr; size_t d_items_win_cap = 0;
    std::vector<vadk::ScanItem> scan_items;
    hipEvent_t scan_done = nullptr;          // vad_scan_device: recorded behind its last launch, which may still read d_items
    bool scan_pending = false;               // (an event, not the caller's stream: the caller may destroy that once its work is done)
    // vad_scan_cut: what d_audio holds - the block the last vad_scan / vad_scan_channels / vad_scan_cut of host audio uploaded
    // (d_audio is written by the scans' uploads and cut_run alone) - and the cut's tables as they were uploaded, segments then
    // workgroups.  audio_rate: 0 = a block at the engine's own rate (vad_scan_cut's), else the input rate of a RATE block
    // (vad_scan_rate_segments, vad_scan_rate_cut with an audio), which vad_scan_rate_cut alone accepts: whatever uploads into
    // d_audio says which of the two it left (set_resident).  cut_rows / cut_tiles: vad_scan_rate_cut's tables for vadk_cut_resample.
    bool audio_resident = false;
    size_t audio_bytes = 0; int32_t audio_channels = 0; int audio_fmt = 0; int32_t audio_rate = 0;
    std::vector<vadk::CutResampleSeg> cut_rows;
    std::vector<uint32_t> cut_tiles;
    std::vector<float> cut_gains;            // vad_scan_cut_gain: one factor per entry of cut_segs
    uint8_t *d_cut = nullptr; size_t d_cut_cap = 0;
    void *d_cut_out = nullptr; size_t d_cut_out_cap = 0;
    std::vector<vadk::CutSeg> cut_segs;
    std::vector<vadk::CutWork> cut_work;
    // vad_scan_render: the workgroups of its output regions and its copy of the caller's ramp, as they were uploaded
    std::vector<vadk::RenderWork> render_work;
    std::vector<float> render_ramp;
    // vad_scan_mel: the workgroups of its tiles, and the packed operator and filters (vad_layout.h: mel_op_index, mel_filter_index)
    // in d_mel, operator first.  The pack is CACHED: mel_key / mel_src are the vad_mel and the caller's three arrays (op_re, op_im,
    // filters, back to back) it was made from, and a call that brings the same bytes neither packs nor uploads again
    std::vector<vadk::MelWork> mel_work;
    std::vector<float> mel_src, mel_pack;
    vad_mel mel_key{};
    bool mel_packed = false;
    float *d_mel = nullptr; size_t d_mel_cap = 0;
    // vad_scan_resample_cut: the segments' input quads, and the packed operator T (vad_layout.h: rsc_pack_index) in d_rsc, CACHED as
    // the mel operator is: rsc_src are the caller's taps of the previous pack, rsc_rate its sr_in.  vad_scan_rate_mel: the 16 kHz
    // signals of its segments in d_rsc_mid (float32, back to back) and the mel kernel's segments over them
    std::vector<uint32_t> rsc_inq;
    std::vector<float> rsc_src, rsc_pack;
    int32_t rsc_rate = 0;
    bool rsc_packed = false;
    float *d_rsc = nullptr; size_t d_rsc_cap = 0;
    float *d_rsc_mid = nullptr; size_t d_rsc_mid_cap = 0;
    std::vector<vadk::CutSeg> rsc_mel_segs;
    // vad_convert / vad_scan_convert_segments: the packed operators of all row-tiles (vad_layout.h: cv_pack_index) in d_cv_op, CACHED
    // by (L, M, the taps' bytes) as the resample cut's operator is; the block in its wire format (d_cv_in: the staging of the host
    // forms), vad_convert's converted block (d_cv_out; vad_scan_convert_segments converts into d_audio), and the item and workgroup
    // tables as they were uploaded (d_cv_tab)
    std::vector<float> cv_src, cv_pack;
    uint32_t cv_L = 0, cv_M = 0;
    bool cv_packed = false;
    float *d_cv_op = nullptr; size_t d_cv_op_cap = 0;
    uint8_t *d_cv_in = nullptr; size_t d_cv_in_cap = 0;
    float *d_cv_out = nullptr; size_t d_cv_out_cap = 0;
    uint8_t *d_cv_tab = nullptr; size_t d_cv_tab_cap = 0;
    std::vector<vadk::ConvertItem> cv_items;
    std::vector<vadk::ConvertWork> cv_work;
    std::vector<int64_t> cv_offset;
    std::vector<vad_scan_ch_item> cv_scan_items;
    // vad_scan_mel_keep: the RESIDENT MATRIX d_melk [melk_start.back()][melk_n_mels] and its segments' first rows (n + 1 entries;
    // empty: none kept).  vad_mel_stats / vad_mel_batch: a host matrix uploaded to d_melb_in, the tables in d_melb (stats:
    // workgroups, the maxima's -inf; batch: windows, lo, shift, scale), the host forms' outputs in d_melb_out
    float *d_melk = nullptr; size_t d_melk_cap = 0;
    int32_t melk_n_mels = 0;
    std::vector<int64_t> melk_start;
    float *d_melb_in = nullptr; size_t d_melb_in_cap = 0;
    uint8_t *d_melb = nullptr; size_t d_melb_cap = 0;
    uint8_t *d_melb_out = nullptr; size_t d_melb_out_cap = 0;
    std::vector<vadk::MelStatsWork> melb_work;
    std::vector<vadk::MelBatchWin> melb_win;
    std::vector<vadk::MelPackWork> melb_pack;      // vad_mel_batch_packed: the work list, and the pieces' order by (window, offset)
    std::vector<int64_t> melb_order;
    std::vector<int64_t> melb_rows;                // vad_mel_stats_grouped: a group's rows
    std::vector<float> melb_f;
    // vad_mel_project: the packed operator and bias (vad_layout.h: proj_pack_index) in d_proj, CACHED as the mel operator is - proj_src
    // are the caller's op and bias (zeros for NULL) of the previous pack, back to back - and the buffer the replace form projects
    // into, which then changes places with d_melk
    std::vector<float> proj_src, proj_pack;
    int32_t proj_n_in = 0, proj_n_out = 0;
    bool proj_packed = false;
    float *d_proj = nullptr; size_t d_proj_cap = 0;
    float *d_melk_alt = nullptr; size_t d_melk_alt_cap = 0;
    // vad_scan_audio_batch: the windows, the work list, and shift and scale back to back, which lie in d_cut behind the segments
    std::vector<vadk::AudioWin> ab_win;
    std::vector<vadk::AudioWork> ab_work;
    std::vector<float> ab_f;
    // The calls that make or rewrite segment tables.  Each work area is laid out by one DevTables in the function
    // named, and has one staging block: what was uploaded, as it was, until the stream has passed the copy.
    // d_segwork (seg_launches): out_start as int32 [n + 1], the chunk counts; staged in seg_start.  For vad_scan_segments also the
    // items' CSR positions, the count and the retained table
    uint8_t *d_segwork = nullptr; size_t d_segwork_cap = 0;
    std::vector<int32_t> seg_start;
    std::vector<int64_t> seg_out_start;
    long long *d_nsegs = nullptr; size_t d_nsegs_cap = 0;
    vadk::SegRecord *d_segtab = nullptr; size_t d_segtab_cap = 0;
    int64_t segtab_count = -1;               // records of the table in d_segtab; -1: none
    // d_reseg (reseg_setup): out_start as int32, the sets' lane numbers, the sets - staged in reseg_up, one copy - then the scratch
    // state machines, the sets' counts, the items' counts and, for the tails, the lengths.  vad_scan_resegment's own table, and the
    // mark that d_probs / d_events / seg_out_start hold the results of a vad_scan_segments / vad_scan_rate_segments:
    // scan_segments_run sets it, whatever writes or reallocates the two arrays clears it
    uint8_t *d_reseg = nullptr; size_t d_reseg_cap = 0;
    std::vector<int32_t> reseg_up;
    vadk::SegRecord *d_resegtab = nullptr; size_t d_resegtab_cap = 0;
    bool scan_results = false;
    // the tails (vad_scan_tails and its kin): d_tail_len = the snapshot scan_segments_run takes of its streams' state machines, one
    // length per item of seg_out_start, written by nothing else.  d_tailwork (tail_setup): out_start as int32 with the items' slots
    // behind it - staged in tail_up - then the lengths [nt n] and the records [nt n]
    uint32_t *d_tail_len = nullptr; size_t d_tail_len_cap = 0;
    uint8_t *d_tailwork = nullptr; size_t d_tailwork_cap = 0;
    std::vector<int32_t> tail_up;
    // d_refine (refine_count): out_start as int32 - staged in refine_up - the items' first records, their counts.  vad_scan_refine's
    // input in d_refine_in (laid out there: the two counts, the caller's table, the caller's tails) and its output in d_refine_out
    uint8_t *d_refine = nullptr; size_t d_refine_cap = 0;
    std::vector<int32_t> refine_up;
    uint8_t *d_refine_in = nullptr; size_t d_refine_in_cap = 0;
    vadk::SegRecord *d_refine_out = nullptr; size_t d_refine_out_cap = 0;
    // G.711 frames expanded to int16 for the kernels whose loaders do not decode them (launch())
    int16_t *d_g711 = nullptr; size_t d_g711_cap = 0;
    // small calls (a few streams: the one-wrapper-per-client pattern): ONE pinned block in, ONE pinned block out
    static constexpr size_t SMALL_BYTES = 256u << 10;
    uint8_t *h_small_in = nullptr, *h_small_out = nullptr;   // hipHostMalloc
    std::vector<void *> host_blocks;                         // vad_host_alloc: freed with the engine
    uint8_t *d_small_in = nullptr, *d_small_out = nullptr;
    vadk::StepParams base{};
    // Silero V5: the same weights packed for the 16-stream tile kernel (csrc/silero_v5_t16.hip).  It serves
    //   - every ONE-frame call (T == 1: the serving tick, vad_step, the bench): its single-frame instantiation needs 220 registers
    //     and 80.6 KB of LDS, so TWO workgroups share a CU and fill each other's waits - 8 192 streams 44.1 us against 45.4 on
    //     32-stream tiles, 12 288 streams 65.9 against 87.9 (three tiles on a CU instead of two rounds of one);
    //   - multi-frame calls of at most T16_MAX_STREAMS streams: half-size tiles put a small batch on twice as many CUs (its
    //     multi-frame instantiation has 256 - 265 registers: one workgroup per CU, so a larger batch would run in two rounds).
    static constexpr int T16_MAX_STREAMS = 4096;
    float *d_wstream16 = nullptr;
    size_t wbytes16 = 0;
    float *d_wstream16x = nullptr;   // the 16-stream packing's second stream (V5: encoder.0 on bf16 splits), or nullptr
    size_t wbytes16x = 0;
    float *d_wstream16y = nullptr;   // ... and its third (V5: encoder.1 on bf16 splits), or nullptr
    size_t wbytes16y = 0;
    uint32_t sect16[vadk::NWAVES][16] = {};
    int tile_policy = 0;                     // 0 = by batch size, 16 / 32 = forced (vad_debug_set_tile)
    int pair_policy = 0;                     // paired 16-stream tiles: 0 = when a one-frame call has more tiles than CUs, 1 = at every size,
                                             // -1 = never (vad_debug_set_tile(-3 / -4); 0 / 16 / 32 reset it)
    bool rates_fused = true;                 // vad_debug_set_tile(-1 / -2): two-launch / fused form of vad_step_rates (benchmarks)
    bool shared_gpu = false;                 // VAD_ENGINE_SHARED_GPU: keep to 32-stream tiles (n / 32 CUs), leave the rest to the co-tenant
    int sample_rate = 16000;
    int frame_samples = VAD_FRAME_SAMPLES;   // samples per model step (512; Silero V5's 8 kHz sub-model: 256)
    std::vector<int32_t> work_index;         // vad_tick_run_work: the tick's entries the caller has work for
    std::vector<uint8_t> work_kind;
    std::vector<int64_t> work_samples;
    // batched slot control (open / reset / thresholds): one pinned block up, one kernel
    uint8_t *h_ctl = nullptr, *d_ctl = nullptr; size_t ctl_cap = 0;
    // pipelined host ingest (vad_step_submit / vad_step_collect): H2D of ticket t+1 on `copy_in` while the kernel of
    // ticket t runs on `stream`; results come back on `copy_out` into a pinned block
    static constexpr int PIPE_DEPTH = 2;
    struct PipeBuf {
        void *d_frames = nullptr; size_t d_frames_cap = 0;
        uint8_t *d_io = nullptr, *h_io = nullptr; size_t io_cap = 0;   // [slots i32 n | probs f32 n T | seg i32 n | events u8 n T]
        hipEvent_t copied = nullptr, done = nullptr, out = nullptr;
        int64_t ticket = -1; int64_t n = 0; int32_t T = 0; bool busy = false, collecting = false;
    } pipe[PIPE_DEPTH];
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    int64_t next_ticket = 0;
    // tick assembler (vad_tick_push / vad_tick_run): producers write a slot's next frame straight into the page-locked
    // staging row of the coming tick, grouped by (frame format, gate on/off) = the launches of that tick; double-buffered so
    // that frames keep arriving while a tick runs.  A slot's further frames wait in `tick_overflow` (one frame per slot and tick).
    // groups 0..5 = frame_fmt * 2 + gate_on: frames at the engine's own rate, staged in their wire format;
    // groups 6..11 = 6 + 3 * gate_on + {0: 8 kHz, 1: 24 kHz, 2: 48 kHz}: chunks at another input rate (vad_tick_push_rate), staged
    // as float32 [n_in] and resampled on the GPU inside the tick (vad_step_rates' path)
    static constexpr int TICK_GROUPS = VAD_TICK_GROUPS;
    static int tick_group_len(int group, int frame_samples) {
        static const int rate_len[3] = {256, 768, 1536};
        return group < 6 ? frame_samples : rate_len[(group - 6) % 3];
    }
    static int tick_group_rate(int group) {
        static const int rate[3] = {8000, 24000, 48000};
        return rate[(group - 6) % 3];
    }
    static size_t tick_sample_bytes(int group) { return (group >= 2 && group < 6) ? 2 : 4; }
    struct TickBuf {
        uint8_t *h = nullptr;                        // pinned: [cap] rows of frame bytes, then [cap] int32 slots, [cap] int32 lengths, [cap] uint32 epochs
        int64_t cap = 0, count = 0;
        size_t row_bytes = 0;
        uint8_t *row(int64_t r) const { return h + (size_t)r * row_bytes; }
        int32_t *slots() const { return reinterpret_cast<int32_t *>(h + (size_t)cap * row_bytes); }
        int32_t *lens() const { return slots() + cap; }   // samples the caller pushed (before padding / truncation)
        uint32_t *epochs() const { return reinterpret_cast<uint32_t *>(lens() + cap); }   // slot_epoch at push time: a row of a slot closed (and reopened) since is stale
        void drop_row(int64_t r) {                   // the last row fills the hole
            const int64_t last = count - 1;
            if (r != last) {
                std::memcpy(row(r), row(last), row_bytes);
                slots()[r] = slots()[last];
                lens()[r] = lens()[last];
                epochs()[r] = epochs()[last];
            }
            count = last;
        }
    };
    struct TickPending { std::vector<uint8_t> data; int32_t nsamples; int group; };   // the whole frame as pushed
    std::mutex tick_mu;                              // lock order: mu, then tick_mu
    int tick_cur = 0;
    TickBuf tick_buf[2][TICK_GROUPS];
    std::vector<uint32_t> tick_gen;                  // per slot: == tick_generation <=> the slot has a frame in the coming tick
    uint32_t tick_generation = 1;
    std::vector<uint32_t> slot_epoch;                // per slot: bumped by every open (written under mu + tick_mu)
    std::unordered_map<int64_t, std::deque<TickPending>> tick_overflow;
    std::vector<int64_t> tick_overflow_order;        // the slots of tick_overflow in the order they started waiting: their frames are placed in this order
    std::unordered_map<int64_t, std::deque<std::vector<uint8_t>>> tick_tails;   // samples past the model's frame of over-long frames, push order
    // segment assembly on the host side of the tick (vad_tick_enable_segments): what SegmentAssembler / VADProcessor keep per
    // stream (core/silero_model.py:838-869, 891-895, 925-949) - pre-roll, the open segment, the finished one until taken
    // The audio stays in its wire format (int16 stays int16: half the bytes, a memcpy per frame) as runs of (group, samples,
    // gate threshold); it becomes float32 - scaled with a true division and gated - when the finished segment is taken.
    // Storage: fixed 32 KB blocks from an arena (a free list over 8 MB chunks that were touched when they were allocated), so
    // that the tick never reallocates and never page-faults while 8 192 talking streams append a frame each; the tick's
    // assembly pass only PLANS the copies (destination block, offset, bytes) and a few threads then carry them out.
    struct SegArena {
        static constexpr size_t BLOCK = 32768, CHUNK_BLOCKS = 256;
        std::vector<uint8_t *> chunks, free_blocks;
        ~SegArena() { for (uint8_t *c : chunks) std::free(c); }
        void grow() {
            uint8_t *c = static_cast<uint8_t *>(std::malloc(BLOCK * CHUNK_BLOCKS));
            if (!c) throw std::bad_alloc();
            std::memset(c, 0, BLOCK * CHUNK_BLOCKS);          // fault the pages in now, not inside a tick
            chunks.push_back(c);
            for (size_t k = CHUNK_BLOCKS; k-- > 0;) free_blocks.push_back(c + k * BLOCK);
        }
        void reserve_blocks(size_t n) { while (free_blocks.size() < n) grow(); }
        uint8_t *get() {
            if (free_blocks.empty()) grow();
            uint8_t *b = free_blocks.back();
            free_blocks.pop_back();
            return b;
        }
        void put(uint8_t *b) { free_blocks.push_back(b); }
    };
    // one planned copy.  kind 0: `bytes` bytes as they are; 1 / 2: `bytes` bytes of int16 -> float32 / 32767 | / 32768 (dst holds
    // 2 x bytes): the resampled groups' chunks, converted by whoever carries the plan out
    struct SegCopy {
        uint8_t *dst; const uint8_t *src; uint32_t bytes; uint32_t kind = 0;
        void carry_out() const {
            if (kind == 0) { std::memcpy(dst, src, bytes); return; }
            const float sc = kind == 1 ? 32767.0f : 32768.0f;
            const int16_t *q = reinterpret_cast<const int16_t *>(src);
            float *o = reinterpret_cast<float *>(dst);
            for (uint32_t k = 0; k < bytes / 2; ++k) o[k] = (float)q[k] / sc;       // numpy's true division
        }
    };
    struct SegAudio {
        struct Run { int32_t group; float thr; int64_t samples; };      // group as in the tick: tells sample type, int16 scale, gate
        std::vector<uint8_t *> blocks;
        size_t tail = SegArena::BLOCK;                                  // bytes used in the last block (BLOCK: none / full)
        std::vector<Run> runs;
        int64_t samples = 0;
        static bool is_i16(int group) { return group >= 2 && group < 6; }
        static bool gated(int group) { return group < 6 ? (group & 1) : (group >= 9); }
        bool empty() const { return samples == 0; }
        void clear(SegArena &a) {
            for (uint8_t *b : blocks) a.put(b);
            blocks.clear();
            runs.clear();
            tail = SegArena::BLOCK;
            samples = 0;
        }
        void swap(SegAudio &o) { blocks.swap(o.blocks); runs.swap(o.runs); std::swap(samples, o.samples); std::swap(tail, o.tail); }
        // appends cnt samples of `group`: plans the byte copies into `out` (or does them, out == nullptr)
        void append(SegArena &a, int group, float thr, const uint8_t *src, size_t cnt, std::vector<SegCopy> *out) {
            if (!cnt) return;
            const size_t ss = is_i16(group) ? 2 : 4;
            const bool same = !runs.empty() && runs.back().group == group && runs.back().thr == thr;
            if (!same && ss == 4 && !blocks.empty()) tail = (tail + 3) & ~(size_t)3;     // a float32 run starts 4-aligned (the reader applies the same rule)
            size_t bytes = cnt * ss;
            while (bytes) {
                if (tail >= SegArena::BLOCK) {
                    blocks.push_back(a.get());
                    tail = 0;
                }
                const size_t k = std::min(bytes, SegArena::BLOCK - tail);
                if (out) out->push_back(SegCopy{blocks.back() + tail, src, (uint32_t)k});
                else std::memcpy(blocks.back() + tail, src, k);
                tail += k;
                src += k;
                bytes -= k;
            }
            if (same) runs.back().samples += (int64_t)cnt;
            else runs.push_back(Run{group, thr, (int64_t)cnt});
            samples += (int64_t)cnt;
        }
        // the stored bytes of every run in order: fn(run, pointer, samples in this piece); pieces never split a sample
        template <class F>
        void for_each_piece(F fn) const {
            size_t bi = 0, off = 0;
            for (const Run &r : runs) {
                const size_t ss = is_i16(r.group) ? 2 : 4;
                if (ss == 4) off = (off + 3) & ~(size_t)3;
                size_t left = (size_t)r.samples;
                while (left) {
                    if (off >= SegArena::BLOCK) { ++bi; off = 0; }
                    const size_t k = std::min(left, (SegArena::BLOCK - off) / ss);
                    fn(r, blocks[bi] + off, k);
                    off += k * ss;
                    left -= k;
                }
            }
        }
        void to_float(float *o) const {
            for_each_piece([&](const Run &r, const uint8_t *src, size_t cnt) {
                if (!is_i16(r.group)) std::memcpy(o, src, cnt * 4);
                else {
                    const float sc = r.group < 4 ? 32767.0f : 32768.0f;     // np.int16 -> float32 / 32767.0 (true division)
                    const int16_t *q = reinterpret_cast<const int16_t *>(src);
                    for (size_t k = 0; k < cnt; ++k) o[k] = (float)q[k] / sc;
                }
                if (gated(r.group))                                        // the group's gate: utils/audio.py:117-118
                    for (size_t k = 0; k < cnt; ++k) o[k] = std::fabs(o[k]) > r.thr ? o[k] : 0.f;
                o += cnt;
            });
        }
        size_t stored_bytes() const {
            size_t b = 0;
            for (const Run &r : runs) b += (size_t)r.samples * (is_i16(r.group) ? 2 : 4);
            return b;
        }
    };
    struct SegState {
        bool active = false;
        SegAudio pre, seg, done;
        void clear(SegArena &a) { active = false; pre.clear(a); seg.clear(a); done.clear(a); }
    };
    SegArena seg_arena;
    std::vector<SegCopy> seg_copies;                 // the copies one tick planned
    std::vector<SegCopy> push_copies;                // ... and the conversions a batched rate push planned (both under tick_mu)
    // the threads that carry out a tick's planned copies next to the calling one
    struct CopyCrew {
        std::vector<std::thread> th;
        std::mutex m;
        std::condition_variable cv_go, cv_done;
        const SegCopy *items = nullptr;
        size_t n = 0;
        std::atomic<size_t> next{0};
        uint64_t job = 0;
        int busy = 0;
        bool stop = false;
        static void work(const SegCopy *it, size_t n, std::atomic<size_t> &next) {
            for (;;) {
                const size_t a = next.fetch_add(128, std::memory_order_relaxed);
                if (a >= n) return;
                const size_t b = std::min(n, a + 128);
                for (size_t k = a; k < b; ++k) it[k].carry_out();
            }
        }
        void start(int threads) {
            for (int t = 0; t < threads; ++t)
                th.emplace_back([this] {
                    uint64_t seen = 0;
                    std::unique_lock<std::mutex> lk(m);
                    for (;;) {
                        cv_go.wait(lk, [&] { return stop || job != seen; });
                        if (stop) return;
                        seen = job;
                        const SegCopy *it = items;
                        const size_t cnt = n;
                        lk.unlock();
                        work(it, cnt, next);
                        lk.lock();
                        if (--busy == 0) cv_done.notify_one();
                    }
                });
        }
        void run(const SegCopy *it, size_t cnt) {
            size_t bytes = 0;
            for (size_t k = 0; k < cnt; ++k) bytes += it[k].bytes;
            if (th.empty() || bytes < (256u << 10)) {
                for (size_t k = 0; k < cnt; ++k) it[k].carry_out();
                return;
            }
            {
                std::lock_guard<std::mutex> lk(m);
                items = it;
                n = cnt;
                next.store(0, std::memory_order_relaxed);
                busy = (int)th.size();
                ++job;
            }
            cv_go.notify_all();
            work(it, cnt, next);
            std::unique_lock<std::mutex> lk(m);
            cv_done.wait(lk, [&] { return busy == 0; });
        }
        ~CopyCrew() {
            {
                std::lock_guard<std::mutex> lk(m);
                stop = true;
            }
            cv_go.notify_all();
            for (auto &t : th) t.join();
        }
    } copy_crew;
    bool tick_segments = false;
    std::vector<SegState> seg_state;
    std::vector<double> h_start_prob;                // host copy of each slot's vad_start_probability (pre-roll rule :832-839)
    uint8_t *h_tick_out = nullptr, *d_tick_out = nullptr; size_t tick_out_cap = 0;   // [slots i64 | probs f32 | seg i32 | events u8] x max n
    void *d_tick_frames = nullptr; size_t d_tick_frames_cap = 0;
    struct ResampleOp {
        int n_in = 0;
        float *d_w = nullptr;
        size_t bytes = 0;
        uint32_t tile_blocks = 0;
        uint32_t row128_block = 0;
    };
    std::vector<ResampleOp> resample_ops;   // built lazily, one per input rate
    std::vector<ResampleOp> resample_ops16; // the same operators packed for the fused resample -> step kernel (16-stream tiles)
    float *d_rs_in = nullptr;  size_t d_rs_in_cap = 0;
    float *d_rs_out = nullptr; size_t d_rs_out_cap = 0;
    // generic whole-array resampler (vad_resample_generic): the float64 tables of the last few (n_in, n_out) shapes, on the device
    struct RsgEntry {
        int64_t n_in = 0, n_out = 0, a = 0, b = 0, L = 0, P = 0;
        int32_t corrected = 0;
        double *d_tn = nullptr, *d_tm = nullptr;
        size_t bytes = 0;
        uint64_t used = 0;
    };
    static constexpr size_t RSG_CACHE_ENTRIES = 8;
    static constexpr size_t RSG_CACHE_BYTES = 512u << 20;
    std::vector<RsgEntry> rsg_cache;
    uint64_t rsg_clock = 0;
    // long arrays: chirp-z / FFT path (csrc/resample_fft.hip): tables of the last (n_in, n_out), work buffers
    struct RsfPlan {
        int64_t n_in = 0, n_out = 0, P1 = 0, P2 = 0;
        void *W1 = nullptr, *W2 = nullptr, *B1 = nullptr, *B2 = nullptr;
    } rsf_plan;
    void *d_rsf_a = nullptr, *d_rsf_b = nullptr; size_t d_rsf_cap = 0;
    int rsg_path = 0;                                // 0 = by size, 1 = direct kernel, 2 = FFT path (vad_debug_resample_path)
    double *d_rsg_partial = nullptr; size_t d_rsg_partial_cap = 0;
    void *d_rsg_in = nullptr;  size_t d_rsg_in_cap = 0;
    float *d_rsg_out = nullptr; size_t d_rsg_out_cap = 0;
    std::vector<uint8_t> open;
    std::vector<int64_t> free_list;
    std::vector<uint32_t> stamp;   // duplicate detection per step
    uint32_t stamp_gen = 0;
    int open_count = 0;
    int64_t steps = 0, frames = 0;
    hipDeviceProp_t prop{};
    mutable std::mutex mu;
    mutable std::mutex err_mu;        // `err` is written under `mu` by most entry points and under `tick_mu` by vad_tick_push
    mutable std::string err;

    int fail(int code, const char *fmt, ...) const {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        std::lock_guard<std::mutex> lk(err_mu);
        err = buf;
        return code;
    }
    int hip_fail(hipError_t e, const char *what) const {
        (void)hipGetLastError();      // reported here; do not leave it in HIP's process-wide last-error slot
        return fail(VAD_ERR_HIP, "Model prediction failed: %s: %s", what, hipGetErrorString(e));
    }
};

#define HIP_TRY(e, call)                                         \
    do {                                                         \
        hipError_t _r = (call);                                  \
        if (_r != hipSuccess) return (e)->hip_fail(_r, #call);   \
    } while (0)

namespace {

template <class T>
int ensure(vad_engine *e, T *&ptr, size_t &cap, size_t need) {
    if (need <= cap) return VAD_OK;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    void *p = nullptr;
    hipError_t r = hipMalloc(&p, need);
    if (r != hipSuccess) return e->hip_fail(r, "hipMalloc(staging)");
    ptr = static_cast<T *>(p);
    cap = need;
    return VAD_OK;
}

bool is_g711(int fmt) { return fmt == VAD_FMT_ULAW8 || fmt == VAD_FMT_ALAW8; }
size_t sample_bytes(int fmt) { return fmt == VAD_FMT_F32 ? 4u : is_g711(fmt) ? 1u : 2u; }
size_t frame_bytes(const vad_engine *e, int fmt) { return sample_bytes(fmt) * (size_t)e->frame_samples; }

// ITU-T G.711: code -> 16-bit linear PCM, the two laws as tables [law][code] (include/vad_engine.h: VAD_FMT_ULAW8 / VAD_FMT_ALAW8)
const int16_t *g711_table(int fmt) {
    static const std::array<std::array<int16_t, 256>, 2> tab = [] {
        std::array<std::array<int16_t, 256>, 2> t{};
        for (int b = 0; b < 256; ++b) {
            const int u = ~b & 0xFF;
            const int m = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
            t[0][(size_t)b] = (int16_t)((u & 0x80) ? 0x84 - m : m - 0x84);
            const int a = b ^ 0x55, seg = (a & 0x70) >> 4;
            int v = (a & 0x0F) << 4;
            v = seg == 0 ? v + 8 : seg == 1 ? v + 0x108 : (v + 0x108) << (seg - 1);
            t[1][(size_t)b] = (int16_t)((a & 0x80) ? v : -v);
        }
        return t;
    }();
    return tab[fmt == VAD_FMT_ALAW8 ? 1 : 0].data();
}
void g711_to_i16(int fmt, const uint8_t *in, size_t n, int16_t *out) {
    const int16_t *t = g711_table(fmt);
    for (size_t i = 0; i < n; ++i) out[i] = t[in[i]];
}

// The kernels address frames through a 32-bit buffer descriptor with signed 32-bit offset arithmetic: one call may not
// span 2 GiB of frames (1 M float32 frames).  Rejected here instead of wrapping silently.
int check_call_size(vad_engine *e, int64_t n, int32_t T, int fmt) {
    if (n < 0 || T < 1 || n > e->max_streams)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: bad stream or frame count (n = %lld, T = %d, max_streams = %d)",
                       (long long)n, T, e->max_streams);
    // (G.711: sized as the int16 frames the expansion in launch() may turn them into)
    const uint64_t fb = is_g711(fmt) ? frame_bytes(e, VAD_FMT_I16_32768) : frame_bytes(e, fmt);
    if ((uint64_t)n * (uint64_t)T * fb >= (1ull << 31))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: n * T * frame bytes = %llu exceeds the 2 GiB one call may address",
                       (unsigned long long)((uint64_t)n * (uint64_t)T * fb));
    return VAD_OK;
}

int check_slots(vad_engine *e, const int64_t *slots, int64_t n) {
    if (++e->stamp_gen == 0) {
        std::fill(e->stamp.begin(), e->stamp.end(), 0u);
        e->stamp_gen = 1;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t s = slots[i];
        if (s < 0 || s >= e->max_streams || !e->open[(size_t)s])
            return e->fail(VAD_ERR_BAD_SLOT, "Model prediction failed: slot %lld is not an open stream", (long long)s);
        if (e->stamp[(size_t)s] == e->stamp_gen)
            return e->fail(VAD_ERR_BAD_SLOT, "Model prediction failed: slot %lld appears twice in one step", (long long)s);
        e->stamp[(size_t)s] = e->stamp_gen;
    }
    return VAD_OK;
}

// `p` as the 16-stream kernels read it: their weight streams and section table in place of the 32-stream kernels'
vadk::StepParams params16(const vad_engine *e, const vadk::StepParams &p) {
    vadk::StepParams p16 = p;
    p16.wstream = e->d_wstream16;
    p16.wstream_bytes = (uint32_t)e->wbytes16;
    p16.wstream_x = e->d_wstream16x;
    p16.wstream_x_bytes = (uint32_t)e->wbytes16x;
    p16.wstream_y = e->d_wstream16y;
    p16.wstream_y_bytes = (uint32_t)e->wbytes16y;
    std::memcpy(p16.sect, e->sect16, sizeof p16.sect);
    return p16;
}

int launch(vad_engine *e, const vadk::StepParams &p_in, hipStream_t s) {
    hipError_t r = hipErrorInvalidValue;
    vadk::StepParams p = p_in;
    const bool t16 = e->d_wstream16 && (e->tile_policy == 16 || (e->tile_policy == 0 && !e->shared_gpu && (p.T == 1 || p.n <= vad_engine::T16_MAX_STREAMS)));
    if (is_g711(p.fmt) && !(e->version == 5 && t16)) {
        // only the 16-stream V5 kernel decodes G.711 in its loader: every other kernel gets the frames expanded to int16 in HBM by
        // a small kernel in front of it on the same stream (the link still carried one byte per sample) and runs as I16_32768
        const size_t nb = (size_t)p.n * (size_t)p.T * (size_t)e->frame_samples;
        if (int rc = ensure(e, e->d_g711, e->d_g711_cap, 2 * nb)) return rc;
        r = vadk_launch_g711_expand(p.frames, e->d_g711, (int64_t)nb, p.fmt == VAD_FMT_ALAW8 ? 1 : 0, s);
        if (r != hipSuccess) return e->hip_fail(r, "kernel launch (G.711 expansion)");
        p.frames = e->d_g711;
        p.fmt = VAD_FMT_I16_32768;
        r = hipErrorInvalidValue;
    }
    if (e->version == 4 && e->d_wstream16 && e->tile_policy != 32) {
        // Silero V4: 16-stream tiles, two workgroups per CU (each fills the other's waits) - one per CU while the call has no
        // more tiles than the GPU has CUs, so that a small batch spreads out instead of pairing up
        const vadk::StepParams p16 = params16(e, p);
        const int tiles16 = (p.n + 15) / 16;
        r = vadk_launch_silero_v4_t16(&p16, (!e->shared_gpu && tiles16 <= e->prop.multiProcessorCount) ? 1 : 0, s);
    } else if (e->version == 5 && t16) {
        const vadk::StepParams p16 = params16(e, p);
        // One frame per stream of the 16 kHz model, float32 or int16, and more tiles than CUs - so that a CU gets two anyway: the two
        // as ONE workgroup that shares every bf16 weight fragment between them (silero_v5_pair16).  Up to one tile per CU the tiles
        // spread out, as before.
        const int tiles16 = (int)((p.n + 15) / 16);
        const bool pairable = p.T == 1 && p.variant == 0 && p.fmt >= 0 && p.fmt <= 2;
        if (pairable && (e->pair_policy > 0 || (e->pair_policy == 0 && tiles16 > e->prop.multiProcessorCount)))
            r = vadk_launch_silero_v5_t16_pair(&p16, s);
        else
        r = vadk_launch_silero_v5_t16(&p16, s);
    } else if (e->version == 5) r = vadk_launch_silero_v5(&p, s);
    else if (e->version == 4) r = vadk_launch_silero_v4(&p, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch");
    e->steps += 1;
    e->frames += (int64_t)p.n * p.T;
    return VAD_OK;
}

// shared body of vad_step / vad_step_events / vad_step_multi
int step_host(vad_engine *e, const int64_t *slots, int64_t n, int32_t T, const void *frames, int fmt, float thr,
              float *probs, uint8_t *events, int32_t *seg) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n < 0 || T < 1 || (n > 0 && (!slots || !frames || !probs)))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: null buffer or bad count");
    if (fmt < VAD_FMT_F32 || fmt > VAD_FMT_ALAW8)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: unknown frame format %d", fmt);
    if (n == 0) return VAD_OK;
    if (int rc = check_call_size(e, n, T, fmt)) return rc;
    if (int rc = check_slots(e, slots, n)) return rc;
    HIP_TRY(e, hipSetDevice(e->device));
    e->scan_results = false;
    const size_t fb = frame_bytes(e, fmt) * (size_t)n * T;
    // ---- small calls: frames + slots travel as one pinned block, probs + seg + events come back as one; one
    //      synchronisation.  (The general path below issues 2 pageable H2D copies, waits, launches, 3 D2H copies, waits.)
    {
        auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        const size_t o_slots = up16(fb), in_bytes = o_slots + sizeof(int32_t) * n;
        const size_t o_seg = up16(sizeof(float) * n * T), o_ev = o_seg + up16(sizeof(int32_t) * n), out_bytes = o_ev + (size_t)n * T;
        if (in_bytes <= vad_engine::SMALL_BYTES && out_bytes <= vad_engine::SMALL_BYTES) {
            // allocated on first use, each buffer on its own so that a failed attempt can be repeated
            if (!e->h_small_in) HIP_TRY(e, hipHostMalloc((void **)&e->h_small_in, vad_engine::SMALL_BYTES, hipHostMallocDefault));
            if (!e->h_small_out) HIP_TRY(e, hipHostMalloc((void **)&e->h_small_out, vad_engine::SMALL_BYTES, hipHostMallocDefault));
            if (!e->d_small_in) HIP_TRY(e, hipMalloc((void **)&e->d_small_in, vad_engine::SMALL_BYTES));
            if (!e->d_small_out) HIP_TRY(e, hipMalloc((void **)&e->d_small_out, vad_engine::SMALL_BYTES));
            std::memcpy(e->h_small_in, frames, fb);
            int32_t *hs = reinterpret_cast<int32_t *>(e->h_small_in + o_slots);
            for (int64_t i = 0; i < n; ++i) hs[i] = (int32_t)slots[i];
            HIP_TRY(e, hipMemcpyAsync(e->d_small_in, e->h_small_in, in_bytes, hipMemcpyHostToDevice, e->stream));
            vadk::StepParams p = e->base;
            p.slots = reinterpret_cast<const int32_t *>(e->d_small_in + o_slots);
            p.frames = e->d_small_in;
            p.probs = reinterpret_cast<float *>(e->d_small_out);
            p.seg_frames = reinterpret_cast<int32_t *>(e->d_small_out + o_seg);
            p.events = e->d_small_out + o_ev;
            p.n = (int32_t)n;
            p.T = T;
            p.fmt = fmt;
            p.thresh = thr;
            if (int rc = launch(e, p, e->stream)) return rc;
            HIP_TRY(e, hipMemcpyAsync(e->h_small_out, e->d_small_out, out_bytes, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(e, hipStreamSynchronize(e->stream));
            std::memcpy(probs, e->h_small_out, sizeof(float) * n * T);
            if (seg) std::memcpy(seg, e->h_small_out + o_seg, sizeof(int32_t) * n);
            if (events) std::memcpy(events, e->h_small_out + o_ev, (size_t)n * T);
            return VAD_OK;
        }
    }
    if (int rc = ensure(e, e->d_frames, e->d_frames_cap, fb)) return rc;
    if (int rc = ensure(e, e->d_probs, e->d_probs_cap, sizeof(float) * n * T)) return rc;
    if (int rc = ensure(e, e->d_events, e->d_events_cap, (size_t)n * T)) return rc;
    if (int rc = ensure(e, e->d_seg, e->d_seg_cap, sizeof(int32_t) * n)) return rc;
    if (int rc = ensure(e, e->d_slots, e->d_slots_cap, sizeof(int32_t) * n)) return rc;
    std::vector<int32_t> s32((size_t)n);
    for (int64_t i = 0; i < n; ++i) s32[(size_t)i] = (int32_t)slots[i];
    HIP_TRY(e, hipMemcpyAsync(e->d_slots, s32.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->d_frames, frames, fb, hipMemcpyHostToDevice, e->stream));
    vadk::StepParams p = e->base;
    p.slots = e->d_slots;
    p.frames = e->d_frames;
    p.probs = e->d_probs;
    p.events = e->d_events;
    p.seg_frames = e->d_seg;
    p.n = (int32_t)n;
    p.T = T;
    p.fmt = fmt;
    p.thresh = thr;
    // the pageable-memory H2D copies above must not be overwritten before they are consumed
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (int rc = launch(e, p, e->stream)) return rc;
    HIP_TRY(e, hipMemcpyAsync(probs, e->d_probs, sizeof(float) * n * T, hipMemcpyDeviceToHost, e->stream));
    if (events) HIP_TRY(e, hipMemcpyAsync(events, e->d_events, (size_t)n * T, hipMemcpyDeviceToHost, e->stream));
    if (seg) HIP_TRY(e, hipMemcpyAsync(seg, e->d_seg, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

}  // namespace

extern "C" {

const char *vad_last_create_error(void) { return g_create_error.c_str(); }
const char *vad_last_error(const vad_engine *e) {
    if (!e) return "null engine";
    std::lock_guard<std::mutex> lk(e->err_mu);  // other threads may be writing e->err: hand out a thread-local copy
    g_error_copy = e->err;
    return g_error_copy.c_str();
}

int vad_engine_create(const vad_engine_desc *desc, vad_engine **out) {
    g_create_error.clear();
    if (!desc || !out || desc->struct_size < sizeof(vad_engine_desc)) {
        g_create_error = "Failed to load model: bad vad_engine_desc";
        return VAD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (desc->model_version != 4 && desc->model_version != 5) {
        g_create_error = "Failed to load model: model_version must be 4 or 5";
        return VAD_ERR_INVALID_ARG;
    }
    // `sample_rate` is the graph's `sr` input (core/silero_model.py:491): 16000 selects the 16 kHz sub-model, every other
    // value the graph's else-branch = the 8 kHz sub-model, which needs the blob that holds ITS weights (meta.variant = 8000).
    // V4's takes the same 512-sample frames at 8 / 24 / 48 kHz.  V5's is built for native 8 kHz audio in
    // 256-sample frames (with 512-sample frames a 3-D tensor reaches its LSTM and onnxruntime refuses): sample_rate 8000
    // creates that engine (vad_info.frame_samples = 256); 24 / 48 kHz audio has to be resampled first.
    const bool want_8k = desc->sample_rate != 16000;
    if (want_8k && desc->model_version == 5 && desc->sample_rate != 8000) {
        g_create_error = "Failed to load model: Silero V5 takes 16 kHz audio (512-sample frames) or native 8 kHz audio (256-sample frames); resample other rates first";
        return VAD_ERR_UNSUPPORTED;
    }
    if (desc->max_streams < 1) {
        g_create_error = "Failed to load model: max_streams must be >= 1";
        return VAD_ERR_INVALID_ARG;
    }
    vadk::PackedWeights pw;
    std::string perr;
    const bool ok = desc->model_version == 5 ? vadk::pack_silero_v5(desc->weights, desc->weights_len, pw, perr)
                                             : vadk::pack_silero_v4(desc->weights, desc->weights_len, pw, perr);
    if (!ok) {
        g_create_error = perr;
        return VAD_ERR_BAD_WEIGHTS;
    }
    if (want_8k != (pw.variant == 1)) {
        g_create_error = want_8k ? "Failed to load model: sample_rate selects the graph's 8 kHz sub-model but the weight blob holds the 16 kHz one"
                                 : "Failed to load model: sample_rate 16000 but the weight blob holds the graph's 8 kHz sub-model";
        return VAD_ERR_BAD_WEIGHTS;
    }
    int ndev = 0;
    hipError_t r = hipGetDeviceCount(&ndev);
    if (r != hipSuccess || ndev < 1) {
        g_create_error = "Failed to load model: no HIP device available (this engine has no CPU fallback)";
        return VAD_ERR_NO_DEVICE;
    }
    if (desc->device_id < 0 || desc->device_id >= ndev) {
        g_create_error = "Failed to load model: device_id out of range";
        return VAD_ERR_INVALID_ARG;
    }
    vad_engine *e = new vad_engine();
    e->version = desc->model_version;
    e->device = desc->device_id;
    e->max_streams = desc->max_streams;
    e->sample_rate = desc->sample_rate;
    e->shared_gpu = (desc->flags & VAD_ENGINE_SHARED_GPU) != 0;
    e->frame_samples = (desc->model_version == 5 && want_8k) ? vadk::v5::FRAME_8K : VAD_FRAME_SAMPLES;
    auto bail = [&](hipError_t hr, const char *what) {
        g_create_error = std::string("Failed to load model: ") + what + ": " + hipGetErrorString(hr);
        (void)hipGetLastError();      // consumed here: HIP keeps the failure in a process-wide slot otherwise
        vad_engine_destroy(e);
        return VAD_ERR_HIP;
    };
    if ((r = hipSetDevice(e->device)) != hipSuccess) return bail(r, "hipSetDevice");
    if ((r = hipGetDeviceProperties(&e->prop, e->device)) != hipSuccess) return bail(r, "hipGetDeviceProperties");
    if (std::strncmp(e->prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("Failed to load model: kernels are built for gfx950 only, device is ") + e->prop.gcnArchName;
        vad_engine_destroy(e);
        return VAD_ERR_NO_DEVICE;
    }
    if ((r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail(r, "hipStreamCreate");
    if ((r = hipStreamCreateWithFlags(&e->copy_in, hipStreamNonBlocking)) != hipSuccess) return bail(r, "hipStreamCreate");
    if ((r = hipStreamCreateWithFlags(&e->copy_out, hipStreamNonBlocking)) != hipSuccess) return bail(r, "hipStreamCreate");
    e->wbytes = pw.data.size() * sizeof(float);
    if ((r = weights_acquire(e->device, pw.data, &e->d_wstream)) != hipSuccess) return bail(r, "hipMalloc / hipMemcpy(weights)");
    {                                                    // every model has a 16-stream tile kernel for small calls
        vadk::PackedWeights pw16;
        const bool ok16 = desc->model_version == 4 ? vadk::pack_silero_v4_t16(desc->weights, desc->weights_len, pw16, perr)
                                                   : vadk::pack_silero_v5_t16(desc->weights, desc->weights_len, pw16, perr);
        if (!ok16) {
            g_create_error = perr;
            vad_engine_destroy(e);
            return VAD_ERR_BAD_WEIGHTS;
        }
        e->wbytes16 = pw16.data.size() * sizeof(float);
        if ((r = weights_acquire(e->device, pw16.data, &e->d_wstream16)) != hipSuccess)
            return bail(r, "hipMalloc / hipMemcpy(weights, 16-stream tiles)");
        e->wbytes16x = pw16.data_x.size() * sizeof(float);
        if (!pw16.data_x.empty() && (r = weights_acquire(e->device, pw16.data_x, &e->d_wstream16x)) != hipSuccess)
            return bail(r, "hipMalloc / hipMemcpy(weights, 16-stream tiles, second stream)");
        // the third stream and, behind it in the same buffer, the fourth block range (vad_layout.h, ENC23_X3_BLOCKS; V5 only): one
        // allocation, one descriptor in the kernel, shared between engines on the concatenated bytes
        pw16.data_y.insert(pw16.data_y.end(), pw16.data_z.begin(), pw16.data_z.end());
        pw16.data_y.insert(pw16.data_y.end(), pw16.data_d.begin(), pw16.data_d.end());      // the fifth (DFT_X3_BLOCKS) behind the fourth
        e->wbytes16y = pw16.data_y.size() * sizeof(float);
        if (!pw16.data_y.empty() && (r = weights_acquire(e->device, pw16.data_y, &e->d_wstream16y)) != hipSuccess)
            return bail(r, "hipMalloc / hipMemcpy(weights, 16-stream tiles, third stream)");
        std::memcpy(e->sect16, pw16.sect, sizeof pw16.sect);
    }
    const size_t sb = sizeof(float) * VAD_STATE_FLOATS * (size_t)e->max_streams;
    if ((r = hipMalloc((void **)&e->d_state, sb)) != hipSuccess) return bail(r, "hipMalloc(state)");
    if ((r = hipMemset(e->d_state, 0, sb)) != hipSuccess) return bail(r, "hipMemset(state)");
    if ((r = hipMalloc((void **)&e->d_sm, sizeof(vadk::SmSlot) * (size_t)e->max_streams)) != hipSuccess)
        return bail(r, "hipMalloc(sm)");
    {
        std::vector<vadk::SmSlot> init((size_t)e->max_streams, kDefaultSm);
        if ((r = hipMemcpy(e->d_sm, init.data(), sizeof(vadk::SmSlot) * init.size(), hipMemcpyHostToDevice)) != hipSuccess)
            return bail(r, "hipMemcpy(sm)");
    }
    e->base.wstream = e->d_wstream;
    e->base.wstream_bytes = (uint32_t)e->wbytes;
    std::memcpy(e->base.sect, pw.sect, sizeof pw.sect);
    e->base.variant = pw.variant;
    e->base.state = e->d_state;
    e->base.sm = e->d_sm;
    e->open.assign((size_t)e->max_streams, 0);
    e->stamp.assign((size_t)e->max_streams, 0);
    e->tick_gen.assign((size_t)e->max_streams, 0);
    e->slot_epoch.assign((size_t)e->max_streams, 0);
    e->h_start_prob.assign((size_t)e->max_streams, kDefaultSm.start_prob);
    e->free_list.reserve((size_t)e->max_streams);
    for (int64_t s = e->max_streams - 1; s >= 0; --s) e->free_list.push_back(s);
    *out = e;
    return VAD_OK;
}

void vad_engine_destroy(vad_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    for (hipStream_t st : {e->copy_in, e->stream, e->copy_out})
        if (st) (void)hipStreamSynchronize(st);
    weights_release(e->d_wstream);
    weights_release(e->d_wstream16);
    weights_release(e->d_wstream16x);
    weights_release(e->d_wstream16y);
    void *bufs[] = {e->d_refine, e->d_refine_in, e->d_refine_out, e->d_tail_len, e->d_tailwork, e->d_reseg, e->d_resegtab, e->d_state, e->d_sm, e->d_frames, e->d_probs, e->d_events, e->d_seg, e->d_slots, e->d_g711,
                    e->d_audio, e->d_items, e->d_win, e->d_items_win, e->d_cut, e->d_cut_out, e->d_mel, e->d_rsc, e->d_rsc_mid, e->d_cv_op, e->d_cv_in, e->d_cv_out, e->d_cv_tab, e->d_melk, e->d_melk_alt, e->d_proj, e->d_melb_in, e->d_melb, e->d_melb_out, e->d_segwork, e->d_nsegs, e->d_segtab, e->d_rs_in, e->d_rs_out, e->d_small_in, e->d_small_out, e->d_ctl};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (e->scan_done) (void)hipEventDestroy(e->scan_done);
    for (auto &pb : e->pipe) {
        if (pb.d_frames) (void)hipFree(pb.d_frames);
        if (pb.d_io) (void)hipFree(pb.d_io);
        if (pb.h_io) (void)hipHostFree(pb.h_io);
        for (hipEvent_t ev : {pb.copied, pb.done, pb.out})
            if (ev) (void)hipEventDestroy(ev);
    }
    if (e->copy_in) (void)hipStreamDestroy(e->copy_in);
    if (e->copy_out) (void)hipStreamDestroy(e->copy_out);
    if (e->h_ctl) (void)hipHostFree(e->h_ctl);
    for (auto &bb : e->tick_buf)
        for (auto &tb : bb)
            if (tb.h) (void)hipHostFree(tb.h);
    if (e->h_tick_out) (void)hipHostFree(e->h_tick_out);
    if (e->d_tick_out) (void)hipFree(e->d_tick_out);
    if (e->d_tick_frames) (void)hipFree(e->d_tick_frames);
    if (e->h_small_in) (void)hipHostFree(e->h_small_in);
    if (e->h_small_out) (void)hipHostFree(e->h_small_out);
    for (void *b : e->host_blocks) (void)hipHostFree(b);
    for (auto &op : e->resample_ops)
        if (op.d_w) (void)hipFree(op.d_w);
    for (auto &op : e->resample_ops16)
        if (op.d_w) (void)hipFree(op.d_w);
    for (auto &c : e->rsg_cache) {
        if (c.d_tn) (void)hipFree(c.d_tn);
        if (c.d_tm) (void)hipFree(c.d_tm);
    }
    for (void *q : {e->rsf_plan.W1, e->rsf_plan.W2, e->rsf_plan.B1, e->rsf_plan.B2, e->d_rsf_a, e->d_rsf_b})
        if (q) (void)hipFree(q);
    if (e->d_rsg_partial) (void)hipFree(e->d_rsg_partial);
    if (e->d_rsg_in) (void)hipFree(e->d_rsg_in);
    if (e->d_rsg_out) (void)hipFree(e->d_rsg_out);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int vad_engine_info(const vad_engine *e, vad_info *info) {
    if (!e || !info || info->struct_size < sizeof(vad_info)) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    const uint32_t sz = info->struct_size;
    std::memset(info, 0, sizeof *info);
    info->struct_size = sz;
    info->abi_version = VAD_ABI_VERSION;
    info->model_version = e->version;
    info->device_id = e->device;
    info->max_streams = e->max_streams;
    info->open_streams = e->open_count;
    info->compute_units = e->prop.multiProcessorCount;
    info->streams_per_workgroup = vadk::MT;
    info->weight_bytes_device = (int64_t)(e->wbytes + e->wbytes16 + e->wbytes16x + e->wbytes16y);
    info->state_bytes_device = (int64_t)(sizeof(float) * VAD_STATE_FLOATS + sizeof(vadk::SmSlot)) * e->max_streams;
    info->steps = e->steps;
    info->frames = e->frames;
    std::strncpy(info->device_name, e->prop.name, sizeof info->device_name - 1);
    std::strncpy(info->arch, e->prop.gcnArchName, sizeof info->arch - 1);
    info->frame_samples = e->frame_samples;
    info->sample_rate = e->sample_rate;
    return VAD_OK;
}

// One pinned block up (slots, optionally thresholds), ONE kernel for every listed slot, one synchronisation: open, reset and
// threshold updates cost the same for 1 slot and for 8 192 (the per-slot form was 2 round trips per slot).
static int slot_control(vad_engine *e, const int64_t *slots, int64_t n, int op, const vad_thresholds *thr, int64_t nthr) {
    if (n == 0) return VAD_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    const size_t o_thr = ((sizeof(int32_t) * (size_t)n) + 15) & ~(size_t)15;
    const size_t need = o_thr + sizeof(vad_thresholds) * (size_t)nthr;
    if (need > e->ctl_cap) {
        const size_t cap = std::max(need, (size_t)(sizeof(int32_t) + sizeof(vad_thresholds)) * (size_t)e->max_streams + 16);
        if (e->h_ctl) (void)hipHostFree(e->h_ctl);
        if (e->d_ctl) (void)hipFree(e->d_ctl);
        e->h_ctl = e->d_ctl = nullptr;
        e->ctl_cap = 0;
        HIP_TRY(e, hipHostMalloc((void **)&e->h_ctl, cap, hipHostMallocDefault));
        HIP_TRY(e, hipMalloc((void **)&e->d_ctl, cap));
        e->ctl_cap = cap;
    }
    int32_t *hs = reinterpret_cast<int32_t *>(e->h_ctl);
    for (int64_t i = 0; i < n; ++i) hs[i] = (int32_t)slots[i];
    if (nthr) std::memcpy(e->h_ctl + o_thr, thr, sizeof(vad_thresholds) * (size_t)nthr);
    {   // host mirrors used by the tick's segment assembly
        std::lock_guard<std::mutex> tl(e->tick_mu);
        for (int64_t i = 0; i < n; ++i) {
            const size_t sl = (size_t)slots[i];
            if (op & 2) e->h_start_prob[sl] = kDefaultSm.start_prob;
            if (op & 8) e->h_start_prob[sl] = thr[nthr == 1 ? 0 : i].start_probability;
            if ((op & (2 | 4)) && sl < e->seg_state.size()) e->seg_state[sl].clear(e->seg_arena);
        }
    }
    HIP_TRY(e, hipMemcpyAsync(e->d_ctl, e->h_ctl, need, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, vadk_launch_slot_control(e->d_sm, e->d_state, reinterpret_cast<const int32_t *>(e->d_ctl), (int)n, op, &kDefaultSm,
                                        reinterpret_cast<const vad_thresholds *>(e->d_ctl + o_thr), (int)nthr, e->stream));
    // callers may step on their own HIP stream next (vad_step_device): the slots must be ready when this returns
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}
enum { CTL_ZERO_STATE = 1, CTL_DEFAULT_SM = 2, CTL_RESET_DYNAMIC = 4, CTL_SET_THRESHOLDS = 8 };

int vad_stream_open(vad_engine *e, int64_t *slot) { return vad_stream_open_many(e, 1, slot); }

// everything the tick assembler holds for a slot: staged row, waiting frames, tails, segment audio (tick_mu held)
static void tick_forget(vad_engine *e, int64_t slot) {
    if (e->tick_overflow.erase(slot))
        e->tick_overflow_order.erase(std::remove(e->tick_overflow_order.begin(), e->tick_overflow_order.end(), slot), e->tick_overflow_order.end());
    e->tick_tails.erase(slot);
    if ((size_t)slot < e->seg_state.size()) e->seg_state[(size_t)slot].clear(e->seg_arena);
    if (e->tick_gen[(size_t)slot] == e->tick_generation) {
        for (auto &tb : e->tick_buf[e->tick_cur])
            for (int64_t r = 0; r < tb.count; ++r)
                if (tb.slots()[r] == (int32_t)slot) {
                    tb.drop_row(r);
                    break;
                }
        e->tick_gen[(size_t)slot] = 0;
    }
}

int vad_stream_open_many(vad_engine *e, int64_t n, int64_t *slots_out) {
    if (!e || n < 0 || (n > 0 && !slots_out)) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if ((int64_t)e->free_list.size() < n)
        return e->fail(VAD_ERR_NO_SLOT, "stream pool exhausted (%d slots, %d open, %lld requested)", e->max_streams,
                       e->open_count, (long long)n);
    for (int64_t i = 0; i < n; ++i) slots_out[i] = e->free_list[e->free_list.size() - 1 - (size_t)i];
    if (int rc = slot_control(e, slots_out, n, CTL_ZERO_STATE | CTL_DEFAULT_SM, nullptr, 0)) return rc;
    {   // `open` is read by the tick's producers under tick_mu alone: written under both locks.  A recycled slot starts with
        // nothing waiting, and a row it still has in a tick that is being run right now is recognised as stale by its epoch.
        std::lock_guard<std::mutex> tl(e->tick_mu);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t sl = e->free_list.back();
            tick_forget(e, sl);
            e->slot_epoch[(size_t)sl] += 1;
            e->open[(size_t)sl] = 1;
            e->free_list.pop_back();
        }
    }
    e->open_count += (int)n;
    return VAD_OK;
}

int vad_stream_close(vad_engine *e, int64_t slot) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    {
        std::lock_guard<std::mutex> tl(e->tick_mu);
        e->open[(size_t)slot] = 0;
        tick_forget(e, slot);              // frames the client had waiting die with its stream
    }
    e->open_count -= 1;
    e->free_list.push_back(slot);
    return VAD_OK;
}

int vad_stream_reset(vad_engine *e, const int64_t *slots, int64_t n) {
    if (!e || (n > 0 && !slots) || n < 0) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = check_slots(e, slots, n)) return rc;
    // keep the slots' thresholds, reset the dynamic part + (h, c) (VADProcessor.reset, silero_model.py:951-968)
    return slot_control(e, slots, n, CTL_ZERO_STATE | CTL_RESET_DYNAMIC, nullptr, 0);
}

int vad_stream_get_state(vad_engine *e, int64_t slot, float *hc) {
    if (!e || !hc) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpyAsync(hc, e->d_state + (size_t)slot * VAD_STATE_FLOATS, sizeof(float) * VAD_STATE_FLOATS,
                              hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

int vad_stream_set_state(vad_engine *e, int64_t slot, const float *hc) {
    if (!e || !hc) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpyAsync(e->d_state + (size_t)slot * VAD_STATE_FLOATS, hc, sizeof(float) * VAD_STATE_FLOATS,
                              hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

static_assert(VAD_STREAM_SAVE_BYTES == sizeof(float) * VAD_STATE_FLOATS + sizeof(vadk::SmSlot), "save blob layout");

int vad_stream_save(vad_engine *e, int64_t slot, void *buf, int64_t cap) {
    if (!e || !buf) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    if (cap < VAD_STREAM_SAVE_BYTES) return e->fail(VAD_ERR_INVALID_ARG, "save buffer too small (%lld < %d)", (long long)cap, VAD_STREAM_SAVE_BYTES);
    HIP_TRY(e, hipSetDevice(e->device));
    char *b = static_cast<char *>(buf);
    HIP_TRY(e, hipMemcpyAsync(b, e->d_state + (size_t)slot * VAD_STATE_FLOATS, sizeof(float) * VAD_STATE_FLOATS,
                              hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(b + sizeof(float) * VAD_STATE_FLOATS, e->d_sm + slot, sizeof(vadk::SmSlot),
                              hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

int vad_stream_restore(vad_engine *e, int64_t slot, const void *buf, int64_t nbytes) {
    if (!e || !buf) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    if (nbytes != VAD_STREAM_SAVE_BYTES) return e->fail(VAD_ERR_INVALID_ARG, "not a stream save blob (%lld bytes)", (long long)nbytes);
    vadk::SmSlot s;
    memcpy(&s, static_cast<const char *>(buf) + sizeof(float) * VAD_STATE_FLOATS, sizeof s);
    if (s.start_count < 1 || s.end_count < 1 || s.start_len < 0 || s.start_len > 20 || s.end_len < 0 || s.end_len > 100)
        return e->fail(VAD_ERR_INVALID_ARG, "corrupt stream save blob");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpyAsync(e->d_state + (size_t)slot * VAD_STATE_FLOATS, buf, sizeof(float) * VAD_STATE_FLOATS,
                              hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->d_sm + slot, &s, sizeof s, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    {   // the tick's pre-roll rule reads the host copy of vad_start_probability
        std::lock_guard<std::mutex> tl(e->tick_mu);
        e->h_start_prob[(size_t)slot] = s.start_prob;
    }
    return VAD_OK;
}

int vad_stream_set_thresholds(vad_engine *e, int64_t slot, const vad_thresholds *t) {
    return vad_stream_set_thresholds_many(e, &slot, 1, t, 1);
}

int vad_stream_set_thresholds_many(vad_engine *e, const int64_t *slots, int64_t n, const vad_thresholds *t, int64_t nt) {
    if (!e || n < 0 || (n > 0 && (!slots || !t))) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n == 0) return VAD_OK;
    if (nt != 1 && nt != n) return e->fail(VAD_ERR_INVALID_ARG, "thresholds: pass 1 (shared) or n (one per slot) entries, got %lld for %lld slots", (long long)nt, (long long)n);
    if (int rc = check_slots(e, slots, n)) return rc;
    for (int64_t i = 0; i < nt; ++i)
        if (t[i].start_frame_count < 1 || t[i].end_frame_count < 1) return e->fail(VAD_ERR_INVALID_ARG, "frame counts must be >= 1");
    // values only: the dynamic part (counters, history) is untouched.  VADWrapper.set_thresholds resets the
    // processor afterwards (vad_wrapper.py:412-413) through vad_stream_reset.
    return slot_control(e, slots, n, CTL_SET_THRESHOLDS, t, nt);
}

int vad_g711_decode(int frame_fmt, const uint8_t *in, int64_t n, int16_t *out) {
    if (!is_g711(frame_fmt) || n < 0 || (n > 0 && (!in || !out))) return VAD_ERR_INVALID_ARG;
    g711_to_i16(frame_fmt, in, (size_t)n, out);
    return VAD_OK;
}

int vad_step(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int frame_fmt, float denoise_thresh,
             float *probs_out) {
    return step_host(e, slots, n, 1, frames, frame_fmt, denoise_thresh, probs_out, nullptr, nullptr);
}

int vad_step_events(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int frame_fmt,
                    float denoise_thresh, float *probs_out, uint8_t *events_out, int32_t *seg_frames_out) {
    if (e && n > 0 && !events_out) {
        std::lock_guard<std::mutex> lk(e->mu);
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: events_out is null");
    }
    return step_host(e, slots, n, 1, frames, frame_fmt, denoise_thresh, probs_out, events_out, seg_frames_out);
}

int vad_step_multi(vad_engine *e, const int64_t *slots, int64_t n, int32_t T, const void *frames, int frame_fmt,
                   float denoise_thresh, float *probs_out, uint8_t *events_out) {
    return step_host(e, slots, n, T, frames, frame_fmt, denoise_thresh, probs_out, events_out, nullptr);
}

int vad_step_device(vad_engine *e, const int32_t *d_slots, int64_t n, const void *d_frames, int frame_fmt,
                    float denoise_thresh, float *d_probs, uint8_t *d_events, int32_t *d_seg_frames, void *stream) {
    return vad_step_multi_device(e, d_slots, n, 1, d_frames, frame_fmt, denoise_thresh, d_probs, d_events, d_seg_frames, stream);
}

int vad_step_multi_device(vad_engine *e, const int32_t *d_slots, int64_t n, int32_t T, const void *d_frames, int frame_fmt,
                          float denoise_thresh, float *d_probs, uint8_t *d_events, int32_t *d_seg_frames, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_ALAW8)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: unknown frame format %d", frame_fmt);
    if (int rc = check_call_size(e, n, T, frame_fmt)) return rc;
    if (n > 0 && (!d_frames || !d_probs)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: null buffer");
    if (is_g711(frame_fmt) && (reinterpret_cast<uintptr_t>(d_frames) & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: G.711 frames on the device must be 4-byte aligned");
    if (n == 0) return VAD_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    vadk::StepParams p = e->base;
    p.slots = d_slots;
    p.frames = d_frames;
    p.probs = d_probs;
    p.events = d_events;
    p.seg_frames = d_seg_frames;
    p.n = (int32_t)n;
    p.T = T;
    p.fmt = frame_fmt;
    p.thresh = denoise_thresh;
    return launch(e, p, stream ? static_cast<hipStream_t>(stream) : e->stream);
}

}  // extern "C"

// ---- whole recordings (vad_scan, vad_scan_channels, vad_scan_rate) -------------------------------------------------
// One host body and one device body serve every entry point.  The input rate is data: `chunk`, the sample frames of one frame in
// the block (0 = the engine's own frames, a block at the engine's rate), and sr_in.  The entry points take e->mu, once, settle the
// rate (scan_rate_check) and call the body.
namespace {

int64_t scan_frames(int64_t nsamples, int64_t frame, int64_t hop) { return nsamples < frame ? 0 : (nsamples - frame) / hop + 1; }

// chunk length that yields 512 samples at 16 kHz (AudioUtils.resample_audio: int(len * 16000 / sr), audio.py:46)
int resample_chunk_len(int sr_in) {
    switch (sr_in) {
        case 8000: return 256;
        case 24000: return 768;
        case 48000: return 1536;
        default: return 0;
    }
}

// the operator that resamples chunks of n_in samples, packed and uploaded when it is first asked for: the rate scans', the rate
// cuts' and the resampler's (t16: in the layout of the 16-stream rates kernel)
int get_resample_op(vad_engine *e, int n_in, vad_engine::ResampleOp **out, bool t16 = false) {
    auto &ops = t16 ? e->resample_ops16 : e->resample_ops;
    for (auto &op : ops)
        if (op.n_in == n_in) {
            *out = &op;
            return VAD_OK;
        }
    std::vector<float> packed;
    std::string perr;
    vad_engine::ResampleOp op;
    op.n_in = n_in;
    op.tile_blocks = t16 ? vadk::pack_resample_operator_t16(n_in, packed, &op.row128_block, perr)
                         : vadk::pack_resample_operator(n_in, packed, &op.row128_block, perr);
    if (op.tile_blocks == 0) return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: %s", perr.c_str());
    op.bytes = packed.size() * sizeof(float);
    hipError_t r = hipMalloc((void **)&op.d_w, op.bytes);
    if (r != hipSuccess) return e->hip_fail(r, "hipMalloc(resample operator)");
    r = hipMemcpy(op.d_w, packed.data(), op.bytes, hipMemcpyHostToDevice);
    if (r != hipSuccess) {
        (void)hipFree(op.d_w);
        return e->hip_fail(r, "hipMemcpy(resample operator)");
    }
    ops.push_back(op);
    *out = &ops.back();
    return VAD_OK;
}

// the tables of an earlier device call (vad_scan_device, vad_scan_cut_device, vad_segments_device) may still be read by its
// launches: they finish before a table is rebuilt
int scan_wait(vad_engine *e) {
    if (e->scan_pending) {
        HIP_TRY(e, hipEventSynchronize(e->scan_done));
        e->scan_pending = false;
    }
    return VAD_OK;
}

// ... and the device call's side of it: an event behind its last launch on `s` (an event, not the caller's stream: the caller may
// destroy that once its work is done)
int scan_mark_pending(vad_engine *e, hipStream_t s) {
    if (!e->scan_done) HIP_TRY(e, hipEventCreateWithFlags(&e->scan_done, hipEventDisableTiming));
    HIP_TRY(e, hipEventRecord(e->scan_done, s));
    e->scan_pending = true;
    return VAD_OK;
}

// The way into a call that rebuilds tables of the engine's, with e->mu held and the call's rate settled: a device call works on the
// caller's stream (NULL: the engine's), a host call on the engine's, and the launches of an earlier device call are waited for
int call_begin(vad_engine *e, bool dev, void *stream, hipStream_t *s) {
    *s = (dev && stream) ? static_cast<hipStream_t>(stream) : e->stream;
    HIP_TRY(e, hipSetDevice(e->device));
    return scan_wait(e);
}

// ... and the way out behind its launches, whose status is `launched`.  A device call: the launches read the engine's tables and
// buffers, so the next scan or cut waits for them, as behind vad_scan_device - after a failed launch too, whose status it returns
// unless the marking itself fails.  A host call: the status first; behind VAD_OK its caller copies back and synchronises
int call_end(vad_engine *e, bool dev, hipStream_t s, int launched) {
    if (!dev) return launched;
    if (int rc = scan_mark_pending(e, s)) return rc;
    return launched;
}

// The tables one call keeps in one of the engine's device buffers, laid out once.  add() appends a table - host pointer, bytes - in
// the order they lie, each at a multiple of 16 bytes (CutSeg and RenderWork hold 64-bit fields); reserve() is the buffer's one
// ensure, copy() the uploads on `s`, and at<T>() a table's device pointer, so that the kernel arguments sum no bytes.  An empty
// table is not copied and is nullptr; a table without a host pointer is room only.  Nothing is allocated: a call has few tables
// (the replay's work area has the most: seven)
struct DevTables {
    static constexpr int MAX = 7;
    uint8_t *&buf; size_t &cap;
    const void *host[MAX]; size_t bytes[MAX], off[MAX]; int n = 0; size_t total = 0;
    int add(const void *p, size_t b) {
        host[n] = p; bytes[n] = b; off[n] = total;
        total += (b + 15) & ~(size_t)15;
        return n++;
    }
    template <class T> int add(const std::vector<T> &v, size_t count) { return add(v.data(), sizeof(T) * count); }
    int reserve(vad_engine *e) { return ensure(e, buf, cap, total); }
    int copy(vad_engine *e, hipStream_t s) const {
        for (int i = 0; i < n; ++i)
            if (bytes[i] && host[i]) HIP_TRY(e, hipMemcpyAsync(buf + off[i], host[i], bytes[i], hipMemcpyHostToDevice, s));
        return VAD_OK;
    }
    template <class T> T *at(int i) const { return bytes[i] ? reinterpret_cast<T *>(buf + off[i]) : nullptr; }
};

// the block in e->d_audio stays for a following cut with audio = NULL.  rate: 0 = a block at the engine's own rate (vad_scan_cut's),
// else a RATE block of that input rate (vad_scan_rate_cut's: its positions and hop count samples at that rate)
void set_resident(vad_engine *e, size_t bytes, int32_t channels, int fmt, int32_t rate) {
    e->audio_resident = true;
    e->audio_bytes = bytes; e->audio_channels = channels; e->audio_fmt = fmt; e->audio_rate = rate;
}

// What a scan and a cut check about their block, in one wording.  Two functions, not one: each caller has checks of its own between
// them (scan_plan: max_streams; cut_check: layout and out_fmt), and which refusal a call with several faults gets is behaviour.
int check_block_format(vad_engine *e, const char *who, int fmt, int32_t channels) {
    if (fmt < VAD_FMT_F32 || fmt > VAD_FMT_ALAW8)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: unknown frame format %d", fmt);
    if (channels != 1 && channels != 2)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: channels = %d, the block holds 1 or 2 interleaved channels", who, channels);
    return VAD_OK;
}

int check_block_extent(vad_engine *e, const char *who, int32_t hop, int64_t audio_samples, int32_t channels, int fmt) {
    if (hop < 4 || (hop & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: hop = %d must be a positive multiple of 4 samples", who, hop);
    // the kernel addresses the block through a 32-bit buffer descriptor
    const uint64_t fbytes = (uint64_t)channels * sample_bytes(fmt);
    if ((uint64_t)audio_samples >= (1ull << 31) || (uint64_t)audio_samples * fbytes >= (1ull << 31))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %llu bytes of audio exceed the 2 GiB one call may address", who,
                       (unsigned long long)((uint64_t)audio_samples * fbytes));
    return VAD_OK;
}

// a block in device memory is read in quads of sample frames: 4 bytes of G.711, 8 of a two-channel block
int check_device_audio(vad_engine *e, const char *who, const void *d_audio, int32_t channels) {
    const uintptr_t align = channels == 2 ? 8 : 4;
    if (reinterpret_cast<uintptr_t>(d_audio) & (align - 1))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the audio block must be %d-byte aligned", who, (int)align);
    return VAD_OK;
}

// what an item of either entry point asks for: vad_scan's items are the channel-0 case
int32_t scan_item_channel(const vad_scan_item &) { return 0; }
int32_t scan_item_reserved(const vad_scan_item &) { return 0; }
int32_t scan_item_channel(const vad_scan_ch_item &it) { return it.channel; }
int32_t scan_item_reserved(const vad_scan_ch_item &it) { return it.reserved; }

// argument checks and the plan of a scan: e->scan_items = one work item per recording, sorted by frame count (stable, descending) so
// that the 16 streams of a tile end together; out0 = out_start[i] - out_base.  *total = frames of all recordings.
// `who` = the entry point's name in the messages; channels: the block's interleaved channels (vad_scan: 1) - offsets, lengths
// and hop count sample frames, and an item's channel (or VAD_SCAN_MIX) travels in the top bits of its quad0 (vad_layout.h).
// own_start (vad_scan_segments, which has no out_start argument): the plan lays the results out itself - the items in the order
// given, packed from 0 - and leaves the positions [n + 1] there; out_start is not looked at.
// frame (vad_scan_rate): the samples of one frame in the block - a chunk at the input rate; 0 = the engine's own frames.
template <class Item>
int scan_plan(vad_engine *e, const char *who, const Item *items, int64_t n, int64_t audio_samples, int32_t channels, int fmt, int32_t hop,
              const int64_t *out_start, int64_t out_base, int64_t *total, std::vector<int64_t> *own_start = nullptr, int64_t frame = 0) {
    if (e->version != 5)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s needs a Silero V5 engine; frame the recordings on the host and use vad_step_multi", who);
    if (e->shared_gpu)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s runs on 16-stream tiles, which a VAD_ENGINE_SHARED_GPU engine "
                                            "does not use; frame the recordings on the host and use vad_step_multi", who);
    if (!e->d_wstream16) return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s: the engine has no 16-stream kernel; use vad_step_multi", who);
    if (n < 0 || audio_samples < 0 || (n > 0 && (!items || (!out_start && !own_start))))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer or bad count", who);
    if (int rc = check_block_format(e, who, fmt, channels)) return rc;
    if (n > e->max_streams)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %lld recordings, max_streams = %d", who, (long long)n, e->max_streams);
    if (int rc = check_block_extent(e, who, hop, audio_samples, channels, fmt)) return rc;
    e->scan_items.resize((size_t)n);
    if (own_start) own_start->assign((size_t)n + 1, 0);
    std::vector<int64_t> slots((size_t)n);
    int64_t sum = 0;
    for (int64_t i = 0; i < n; ++i) {
        const Item &it = items[i];
        if (it.sample_offset < 0 || (it.sample_offset & 3))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld starts at sample %lld, not a multiple of 4", who,
                           (long long)i, (long long)it.sample_offset);
        if (it.nsamples < 0 || it.sample_offset > audio_samples || it.nsamples > audio_samples - it.sample_offset)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld (samples %lld .. +%lld) leaves the audio block of %lld samples", who,
                           (long long)i, (long long)it.sample_offset, (long long)it.nsamples, (long long)audio_samples);
        const int32_t ch = scan_item_channel(it);
        if (ch != VAD_SCAN_MIX && (ch < 0 || ch >= channels))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld names channel %d of %d (0 .. channels - 1, or VAD_SCAN_MIX)", who,
                           (long long)i, ch, channels);
        if (scan_item_reserved(it) != 0)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld: reserved = %d must be 0", who, (long long)i,
                           scan_item_reserved(it));
        const int64_t nf = scan_frames(it.nsamples, frame > 0 ? frame : e->frame_samples, hop);
        if (own_start) (*own_start)[(size_t)i + 1] = (*own_start)[(size_t)i] + nf;
        else if (out_start[i] < out_base || out_start[i + 1] - out_start[i] != nf)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_start gives recording %lld %lld entries, it has %lld frames", who,
                           (long long)i, (long long)(out_start[i + 1] - out_start[i]), (long long)nf);
        const int64_t pos = own_start ? (*own_start)[(size_t)i] : out_start[i] - out_base;
        if (pos + nf > INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 frames in one call", who);
        slots[(size_t)i] = it.slot;
        const uint32_t mode = channels == 1 ? vadk::SCAN_LEFT : ch == VAD_SCAN_MIX ? vadk::SCAN_MIX : (uint32_t)ch;
        e->scan_items[(size_t)i] = vadk::ScanItem{(int32_t)it.slot, (uint32_t)(it.sample_offset >> 2) | (mode << vadk::SCAN_MODE_SHIFT), (int32_t)nf,
                                                  (uint32_t)pos};
        sum += nf;
    }
    if (int rc = check_slots(e, slots.data(), n)) return rc;
    std::stable_sort(e->scan_items.begin(), e->scan_items.end(),
                     [](const vadk::ScanItem &a, const vadk::ScanItem &b) { return a.nframes > b.nframes; });
    *total = sum;
    return VAD_OK;
}

// the launches of a planned scan at the engine's rate (e->d_items holds e->scan_items): windows of at most scan_launch_frames
// frames, each over the items that still have frames in it - a prefix of the sorted table.  State travels through HBM between
// them, as between two vad_step_multi calls.
int scan_launches(vad_engine *e, const void *d_audio, int64_t audio_samples, int32_t channels, int fmt, int32_t hop, float thr, float *d_probs,
                  uint8_t *d_events, int32_t *d_seg, int64_t total, hipStream_t s) {
    const std::vector<vadk::ScanItem> &it = e->scan_items;
    const int maxf = it.empty() ? 0 : it.front().nframes;
    const int cap = e->scan_launch_frames > 0 ? e->scan_launch_frames : vad_engine::SCAN_LAUNCH_FRAMES;
    vadk::StepParams p = params16(e, e->base);
    p.slots = nullptr;
    p.frames = d_audio;
    p.probs = d_probs;
    p.events = d_events;
    p.seg_frames = d_seg;
    p.fmt = fmt;
    p.thresh = thr;
    vadk::ScanArgs a{};
    a.audio_bytes = (uint32_t)((uint64_t)audio_samples * (uint64_t)channels * sample_bytes(fmt));
    a.hopq = (uint32_t)hop >> 2;
    a.channels = channels;
    size_t live = it.size();
    for (int t0 = 0; t0 < maxf; t0 += cap) {
        while (live > 0 && it[live - 1].nframes <= t0) --live;
        p.n = (int32_t)live;
        p.T = std::min(cap, maxf - t0);
        a.t0 = t0;
        const hipError_t r = vadk_launch_silero_v5_scan16(&p, e->d_items, &a, s);
        if (r != hipSuccess) return e->hip_fail(r, "kernel launch (scan)");
        e->steps += 1;
    }
    e->frames += total;
    return VAD_OK;
}

// what comes before the plan's checks in a call that names its input rate: the engine's model rate and the input rate.  *chunk =
// sample frames of one chunk at sr_in, or 0: the recordings are at 16 kHz already and the call is vad_scan_channels under another
// name (AudioUtils.resample_audio returns its input).
int scan_rate_check(vad_engine *e, const char *who, int32_t sr_in, int *chunk) {
    if (e->version == 5 && e->frame_samples != VAD_FRAME_SAMPLES)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s: this engine runs an 8 kHz sub-model on %d-sample frames; "
                       "resampled recordings need the 16 kHz one", who, e->frame_samples);
    *chunk = sr_in == 16000 ? 0 : resample_chunk_len(sr_in);
    if (sr_in != 16000 && *chunk == 0)
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: %s: supported input rates are 8000, 16000, 24000, 48000", sr_in, who);
    return VAD_OK;
}

// the launches of a planned rate scan (e->d_items holds e->scan_items, planned on chunks of `chunk` sample frames): per window of W
// chunks one vadk_scan_resample - the window's chunks of the live items -> 512-sample frames in d_win, and the window's item table
// - and behind it, on the same stream, the scan kernel over d_win as a mono float32 block whose frames lie back to back.  State
// travels through HBM between the windows, as in scan_launches; the gate and the non-finite check act on the resampled frame.
int scan_rate_launches(vad_engine *e, const void *d_audio, int64_t audio_samples, int32_t channels, int fmt, int chunk, int32_t hop, float thr,
                       float *d_probs, uint8_t *d_events, int32_t *d_seg, int64_t total, hipStream_t s) {
    const std::vector<vadk::ScanItem> &it = e->scan_items;
    const int maxf = it.empty() ? 0 : it.front().nframes;
    size_t live = it.size();
    while (live > 0 && it[live - 1].nframes <= 0) --live;
    if (live == 0) return VAD_OK;
    const int cap = e->scan_launch_frames > 0 ? e->scan_launch_frames : vad_engine::SCAN_LAUNCH_FRAMES;
    const size_t fit = vad_engine::SCAN_RATE_WIN_BYTES / (live * 2048u);
    const int W = std::max(1, (int)std::min<size_t>((size_t)std::min(cap, maxf), fit));
    const size_t win_bytes = live * (size_t)W * 2048u;
    if (win_bytes >= (size_t(1) << 31))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %zu recordings with chunks in one call: one frame of each exceeds the 2 GiB a launch may address", live);
    vad_engine::ResampleOp *op = nullptr;
    if (int rc = get_resample_op(e, chunk, &op)) return rc;
    if (int rc = ensure(e, e->d_win, e->d_win_cap, win_bytes)) return rc;
    if (int rc = ensure(e, e->d_items_win, e->d_items_win_cap, sizeof(vadk::ScanItem) * live)) return rc;
    vadk::ScanResampleArgs r{};
    r.wstream = op->d_w;
    r.wstream_bytes = (uint32_t)op->bytes;
    r.tile_blocks = op->tile_blocks;
    r.row128_block = op->row128_block;
    r.audio_bytes = (uint32_t)((uint64_t)audio_samples * (uint64_t)channels * sample_bytes(fmt));
    r.audio = d_audio;
    r.items = e->d_items;
    r.items_win = e->d_items_win;
    r.win = e->d_win;
    r.W = W;
    r.n_in = chunk;
    r.hopq = (uint32_t)hop >> 2;
    r.fmt = fmt;
    r.channels = channels;
    vadk::StepParams p = params16(e, e->base);
    p.slots = nullptr;
    p.frames = e->d_win;
    p.probs = d_probs;
    p.events = d_events;
    p.seg_frames = d_seg;
    p.fmt = VAD_FMT_F32;
    p.thresh = thr;
    vadk::ScanArgs a{};
    a.hopq = VAD_FRAME_SAMPLES / 4;
    a.t0 = 0;
    a.channels = 1;
    for (int t0 = 0; t0 < maxf; t0 += W) {
        while (live > 0 && it[live - 1].nframes <= t0) --live;
        r.live = (int32_t)live;
        r.t0 = t0;
        hipError_t rr = vadk_launch_scan_resample(&r, s);
        if (rr != hipSuccess) return e->hip_fail(rr, "kernel launch (scan resample)");
        p.n = (int32_t)live;
        p.T = std::min(W, maxf - t0);
        a.audio_bytes = (uint32_t)(live * (size_t)W * 2048u);
        rr = vadk_launch_silero_v5_scan16(&p, e->d_items_win, &a, s);
        if (rr != hipSuccess) return e->hip_fail(rr, "kernel launch (scan)");
        e->steps += 1;
    }
    e->frames += total;
    return VAD_OK;
}

// the launches of a planned scan on `s`, by the rate of its block: two loops that share nothing but params16
int scan_enqueue(vad_engine *e, const void *d_audio, int64_t audio_samples, int32_t channels, int fmt, int chunk, int32_t hop, float thr,
                 float *d_probs, uint8_t *d_events, int32_t *d_seg, int64_t total, hipStream_t s) {
    if (chunk > 0) return scan_rate_launches(e, d_audio, audio_samples, channels, fmt, chunk, hop, thr, d_probs, d_events, d_seg, total, s);
    return scan_launches(e, d_audio, audio_samples, channels, fmt, hop, thr, d_probs, d_events, d_seg, total, s);
}

// a planned scan of host audio (scan_host, scan_segments_run): the block crosses the link once, in its wire format, interleaved as
// it is; the launches write the engine's own d_probs / d_events / d_seg.  resident: the block stays for a cut with audio = NULL,
// as a block at the engine's rate (chunk == 0) or as a rate block of sr_in - whatever becomes of the launches
int scan_upload_launch(vad_engine *e, int64_t n, const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt, int chunk,
                       int32_t sr_in, int32_t hop, float denoise_thresh, int64_t total, bool resident,
                       const std::function<int()> *fill = nullptr) {
    const size_t ab = (size_t)audio_samples * (size_t)channels * sample_bytes(frame_fmt);
    e->audio_resident = false;
    e->scan_results = false;
    if (int rc = ensure(e, e->d_audio, e->d_audio_cap, ab + 16)) return rc;
    if (int rc = ensure(e, e->d_items, e->d_items_cap, sizeof(vadk::ScanItem) * (size_t)n)) return rc;
    if (int rc = ensure(e, e->d_probs, e->d_probs_cap, sizeof(float) * (size_t)total)) return rc;
    if (int rc = ensure(e, e->d_events, e->d_events_cap, (size_t)total)) return rc;
    if (int rc = ensure(e, e->d_seg, e->d_seg_cap, sizeof(int32_t) * (size_t)total)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_items, e->scan_items.data(), sizeof(vadk::ScanItem) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    // fill (vad_scan_convert_segments): the block is made on the device, by launches on the engine's stream
    if (fill) {
        if (int rc = (*fill)()) return rc;
    } else {
        HIP_TRY(e, hipMemcpyAsync(e->d_audio, audio, ab, hipMemcpyHostToDevice, e->stream));
    }
    if (resident) set_resident(e, ab, channels, frame_fmt, chunk > 0 ? sr_in : 0);
    return scan_enqueue(e, e->d_audio, audio_samples, channels, frame_fmt, chunk, hop, denoise_thresh, e->d_probs, e->d_events, e->d_seg, total,
                        e->stream);
}

// vad_scan, vad_scan_channels and vad_scan_rate, with e->mu held.  A block at the engine's rate becomes the resident one;
// vad_scan_rate at another rate leaves nothing to cut, and no block stays
template <class Item>
int scan_host(vad_engine *e, const char *who, const Item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
              int frame_fmt, int chunk, int32_t sr_in, int32_t hop, float denoise_thresh, const int64_t *out_start, float *probs_out,
              uint8_t *events_out, int32_t *seg_frames_out) {
    HIP_TRY(e, hipSetDevice(e->device));
    if (int rc = scan_wait(e)) return rc;
    int64_t total = 0;
    const int64_t base = (n > 0 && out_start) ? out_start[0] : 0;
    if (base < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_start[0] is negative", who);
    if (int rc = scan_plan(e, who, items, n, audio_samples, channels, frame_fmt, hop, out_start, base, &total, nullptr, chunk)) return rc;
    if (total == 0) return VAD_OK;
    if (!audio || !probs_out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (int rc = scan_upload_launch(e, n, audio, audio_samples, channels, frame_fmt, chunk, sr_in, hop, denoise_thresh, total, chunk == 0)) return rc;
    HIP_TRY(e, hipMemcpyAsync(probs_out + base, e->d_probs, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, e->stream));
    if (events_out) HIP_TRY(e, hipMemcpyAsync(events_out + base, e->d_events, (size_t)total, hipMemcpyDeviceToHost, e->stream));
    if (seg_frames_out) HIP_TRY(e, hipMemcpyAsync(seg_frames_out + base, e->d_seg, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

// vad_scan_device, vad_scan_channels_device and vad_scan_rate_device, with e->mu held.  The plan's refusals carry `plan_who` - for
// the first two the host entry point's name, as they did before there were two.  Returns after enqueueing: the next call that
// rebuilds the tables waits (scan_mark_pending)
template <class Item>
int scan_dev(vad_engine *e, const char *who, const char *plan_who, const Item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
             int frame_fmt, int chunk, int32_t hop, float denoise_thresh, const int64_t *out_start, float *d_probs, uint8_t *d_events,
             int32_t *d_seg_frames, void *stream) {
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    HIP_TRY(e, hipSetDevice(e->device));
    if (int rc = scan_wait(e)) return rc;
    int64_t total = 0;
    if (int rc = scan_plan(e, plan_who, items, n, audio_samples, channels, frame_fmt, hop, out_start, 0, &total, nullptr, chunk)) return rc;
    if (total == 0) return VAD_OK;
    if (!d_audio || !d_probs) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (int rc = check_device_audio(e, who, d_audio, channels)) return rc;
    if (int rc = ensure(e, e->d_items, e->d_items_cap, sizeof(vadk::ScanItem) * (size_t)n)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_items, e->scan_items.data(), sizeof(vadk::ScanItem) * (size_t)n, hipMemcpyHostToDevice, s));
    const int rc = scan_enqueue(e, d_audio, audio_samples, channels, frame_fmt, chunk, hop, denoise_thresh, d_probs, d_events, d_seg_frames, total, s);
    // (also behind a failed launch: the copy of the table and the launches before it are on the stream)
    if (int rc2 = scan_mark_pending(e, s)) return rc2;
    return rc;
}

}  // namespace

extern "C" {

int64_t vad_scan_frame_count(const vad_engine *e, int64_t nsamples, int32_t hop) {
    if (!e || hop < 1 || nsamples < 0) return -1;
    return scan_frames(nsamples, e->frame_samples, hop);
}

int64_t vad_scan_rate_frame_count(const vad_engine *e, int64_t nsamples, int32_t sr_in, int32_t hop) {
    if (!e || hop < 1 || nsamples < 0) return -1;
    const int chunk = sr_in == 16000 ? e->frame_samples : resample_chunk_len(sr_in);
    if (chunk == 0) return -1;
    return scan_frames(nsamples, chunk, hop);
}

int vad_debug_scan_launch_frames(vad_engine *e, int32_t frames) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (frames < 0) return e->fail(VAD_ERR_INVALID_ARG, "vad_debug_scan_launch_frames: frames per launch >= 1, or 0 for the default");
    e->scan_launch_frames = frames;
    return VAD_OK;
}

int vad_scan(vad_engine *e, const vad_scan_item *items, int64_t n, const void *audio, int64_t audio_samples, int frame_fmt,
             int32_t hop, float denoise_thresh, const int64_t *out_start, float *probs_out, uint8_t *events_out,
             int32_t *seg_frames_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_host(e, "vad_scan", items, n, audio, audio_samples, 1, frame_fmt, 0, 0, hop, denoise_thresh, out_start, probs_out, events_out,
                     seg_frames_out);
}

int vad_scan_device(vad_engine *e, const vad_scan_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int frame_fmt,
                    int32_t hop, float denoise_thresh, const int64_t *out_start, float *d_probs, uint8_t *d_events,
                    int32_t *d_seg_frames, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_dev(e, "vad_scan_device", "vad_scan", items, n, d_audio, audio_samples, 1, frame_fmt, 0, hop, denoise_thresh, out_start, d_probs,
                    d_events, d_seg_frames, stream);
}

int vad_scan_channels(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                      int frame_fmt, int32_t hop, float denoise_thresh, const int64_t *out_start, float *probs_out, uint8_t *events_out,
                      int32_t *seg_frames_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_host(e, "vad_scan_channels", items, n, audio, audio_samples, channels, frame_fmt, 0, 0, hop, denoise_thresh, out_start, probs_out,
                     events_out, seg_frames_out);
}

int vad_scan_channels_device(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                             int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh, const int64_t *out_start, float *d_probs,
                             uint8_t *d_events, int32_t *d_seg_frames, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_dev(e, "vad_scan_channels_device", "vad_scan_channels", items, n, d_audio, audio_samples, channels, frame_fmt, 0, hop, denoise_thresh,
                    out_start, d_probs, d_events, d_seg_frames, stream);
}

// recordings at 8 / 24 / 48 kHz: framed at the input rate, resampled chunk by chunk, then scanned (sr_in = 16000: vad_scan_channels
// and vad_scan_channels_device under these names)
int vad_scan_rate(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                  int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, const int64_t *out_start, float *probs_out,
                  uint8_t *events_out, int32_t *seg_frames_out) {
    static const char *who = "vad_scan_rate";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    int chunk = 0;
    if (int rc = scan_rate_check(e, who, sr_in, &chunk)) return rc;
    return scan_host(e, who, items, n, audio, audio_samples, channels, frame_fmt, chunk, sr_in, hop, denoise_thresh, out_start, probs_out, events_out,
                     seg_frames_out);
}

int vad_scan_rate_device(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                         int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, const int64_t *out_start, float *d_probs,
                         uint8_t *d_events, int32_t *d_seg_frames, void *stream) {
    static const char *who = "vad_scan_rate_device";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    int chunk = 0;
    if (int rc = scan_rate_check(e, who, sr_in, &chunk)) return rc;
    return scan_dev(e, who, who, items, n, d_audio, audio_samples, channels, frame_fmt, chunk, hop, denoise_thresh, out_start, d_probs, d_events,
                    d_seg_frames, stream);
}

}  // extern "C"

// ---- finished segments cut out of a scanned block (vad_scan_cut, vad_scan_rate_cut) --------------------------------------
namespace {

static_assert(VAD_CUT_WG_SAMPLES == 4 * vadk::CUT_WG_QUADS && VAD_RESAMPLE_CUT_WG_SAMPLES == vadk::RSC_WG_SAMPLES,
              "the header's workgroup shares are the kernels'");

// frame: the samples of one frame in the block; out_frame: the samples a frame has in a VAD_CUT_FRAMES payload
int64_t cut_samples(int64_t frame, int64_t nframes, int64_t hop, int32_t layout, int64_t out_frame) {
    return layout == VAD_CUT_FRAMES ? nframes * out_frame : (nframes - 1) * hop + frame;
}

// rows of one window of vad_scan_rate_cut's frames: what the engine's window buffer holds, in whole tiles; the launch-frames knob
// of the scans (vad_debug_scan_launch_frames) cuts it to that many tiles, so that a test reaches the window loop with a small call
uint32_t cut_window_rows(const vad_engine *e) {
    const size_t full = vad_engine::SCAN_RATE_WIN_BYTES / 2048u;
    return (uint32_t)(e->scan_launch_frames > 0 ? std::min<size_t>(full, (size_t)e->scan_launch_frames * vadk::MT) : full);
}

// what comes before cut_run's checks in a rate cut: the engine's frames and the input rate.  No model runs, so Silero V4 and
// VAD_ENGINE_SHARED_GPU engines pass (every engine can hold a resample operator: get_resample_op); an engine whose frames are not
// the 512 samples the operator writes - an 8 kHz sub-model - does not.  *chunk = 0: 16 kHz, the call is vad_scan_cut.
int rate_cut_check(vad_engine *e, const char *who, int32_t sr_in, int *chunk) {
    if (e->frame_samples != VAD_FRAME_SAMPLES || e->sample_rate != 16000)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s: this engine runs an 8 kHz sub-model on %d-sample frames; "
                       "resampled recordings need the 16 kHz one", who, e->frame_samples);
    return scan_rate_check(e, who, sr_in, chunk);
}

struct CutSpan { int64_t lo, hi, i; };                           // the output samples [lo, hi) of segment i
struct CutWin { uint32_t r0, r1; size_t seg0, work0, nwork; };   // rows [r0, r1) of a rate cut's frames: their part of the tables

static_assert(sizeof(vad_level) == 16 && sizeof(vad_moments) == 16, "the records of the LEVELS and MOMENTS kinds have one size");

// what a call of this family makes of its segments
enum class CutKind {
    PAYLOAD,        // vad_scan_cut, _rate_cut, _cut_gain, _cut_stereo: each segment's samples at its out_sample
    LEVELS,         // vad_scan_levels: a vad_level record per segment, reduced where a cut stores
    MOMENTS,        // vad_scan_moments: a vad_moments record per segment, the levels' runner with another launcher
    AUDIO_BATCH,    // vad_scan_audio_batch: normalised, padded windows of the segments' ranges; the work follows the output
    RENDER,         // vad_scan_render, _render_stereo: every output sample written; the ranges of two segments may overlap, three not
    MEL,            // vad_scan_mel, vad_scan_mel_keep at the engine's rate: log-mel rows, the segments back to back
    RESAMPLE,       // vad_scan_resample_cut: a rate block's segments at 16 kHz, at their out_sample
    RESAMPLE_MEL    // vad_scan_rate_mel, vad_scan_mel_keep of a rate block: the rows of the segments resampled to 16 kHz
};

// The call as its entry point received it: cut_call fills the block arguments every call has, the entry point sets its own few
// fields by name.  Nothing in it is derived; what the phases test is named below the fields.
struct CutCall {
    const char *who; const vad_cut_item *items; int64_t n, audio_samples; int32_t channels; int fmt; int32_t hop; float thr;
    CutKind kind = CutKind::PAYLOAD;
    // the block's rate, settled on the way in (cut_enter; the resampling kinds: resample_cut_check): chunk > 0 - the block is
    // at sr_in and a frame in it is a chunk of `chunk` sample frames; chunk = 0 - a block at the engine's rate, and sr_in is 0
    int32_t sr_in = 0; int chunk = 0;
    // every kind but PAYLOAD reads or writes the sample range once, as float32 where it has no out_fmt of its own
    int32_t layout = VAD_CUT_RANGE, out_fmt = VAD_CUT_F32; int64_t out_samples = 0;
    // a factor per segment (host array [n]) or nullptr; vad_scan_cut_gain refuses nullptr
    const float *gains = nullptr; bool gains_required = false;
    float clip = 0.0f;                                   // LEVELS
    const float *ramp = nullptr; int32_t nramp = 0;      // RENDER: a sample is faded by `ramp` (host, nramp entries) from both ends of its segment
    // both channels of a two-channel block, interleaved.  Positions and counts stay sample FRAMES, so the tables are the mono
    // call's: an output frame has twice the bytes (CutPlan::ob), and the launcher is another
    bool stereo = false;
    const float *taps = nullptr; int32_t ntaps = 0;      // the resampling kinds
    // the mel kinds.  keep (vad_scan_mel_keep): the rows stay in e->d_melk, the call has no output and no out_rows
    const vad_mel *m = nullptr; const float *op_re = nullptr, *op_im = nullptr, *filters = nullptr; int64_t out_rows = 0;
    bool keep = false; int64_t *rows_out = nullptr;
    // AUDIO_BATCH: the windows (host), shift and scale (host [nss] or nullptr), the output's bytes and the mask
    const vad_audio_batch *ab = nullptr; const vad_audio_window *awin = nullptr; int64_t nw = 0;
    const float *shift = nullptr, *scale = nullptr; int64_t nss = 1, out_bytes = 0; uint8_t *mask = nullptr;

    bool rate() const { return chunk > 0; }
    // a rate block's frames resampled window by window into e->d_win (vadk_cut_resample), each window cut as a mono float32 block of
    // back-to-back frames, which gates.  The range once of a rate block is the same kernel on the input-rate block with the gate off
    bool rate_frames() const { return rate() && layout == VAD_CUT_FRAMES; }
    bool resamples() const { return kind == CutKind::RESAMPLE || kind == CutKind::RESAMPLE_MEL; }
    bool mel() const { return kind == CutKind::MEL || kind == CutKind::RESAMPLE_MEL; }
    // the segments' samples go to the caller at each item's out_sample; without a payload no out_sample is read and segments may
    // share samples
    bool has_payload() const { return kind == CutKind::PAYLOAD || kind == CutKind::RENDER || kind == CutKind::RESAMPLE; }
    // its workgroups follow the output, not the segments: render_regions lists them (mel: mel_tiles)
    bool work_follows_output() const { return kind == CutKind::RENDER || kind == CutKind::MEL || kind == CutKind::AUDIO_BATCH; }
    // the output is records of 16 bytes (vad_level, vad_moments), 8-byte aligned; else 16 bytes
    bool records_out() const { return kind == CutKind::LEVELS || kind == CutKind::MOMENTS; }
    float gate() const { return rate() && !rate_frames() ? -1.0f : thr; }    // no input-rate sample was ever gated
};

CutCall cut_call(const char *who, const vad_cut_item *items, int64_t n, int64_t audio_samples, int32_t channels, int fmt, int32_t hop, float thr) {
    return CutCall{who, items, n, audio_samples, channels, fmt, hop, thr};
}

// What the phases of a call derive and carry from one to the next; each phase is a function below, in the order it runs.  The tables
// themselves are the engine's (e->cut_segs, e->cut_work: one entry per workgroup; e->cut_rows, e->cut_tiles: a rate cut's frames).
struct CutPlan {
    const CutCall &k;
    // a. cut_check
    uint32_t fshift = 0;                     // log2 of the quads of a payload frame
    int64_t rows = 0;                        // rate_frames: the frames of all segments
    size_t ab = 0, ob = 0;                   // bytes of the block, and of one output sample (stereo: sample frame)
    std::vector<CutSpan> spans;              // by lo
    // b. cut_block: the block the kernels read, and where they write
    const void *d_audio = nullptr; void *d_out = nullptr;
    // c. cut_windows
    vad_engine::ResampleOp *op = nullptr; std::vector<CutWin> wins;
    // the mel kinds: the rows of all segments (mel_tiles) and their bytes (mel_output)
    int64_t mel_rows = 0; size_t mel_bytes = 0;
};

// vad_scan_render's own arguments, between the block's checks and the items': the output's length and the ramp
int render_check(vad_engine *e, const CutCall &c) {
    const char *who = c.who;
    if (c.out_samples & 3)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_samples = %lld must be a multiple of 4", who, (long long)c.out_samples);
    if (c.nramp < 0 || c.nramp > VAD_RENDER_MAX_RAMP || (c.nramp & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: nramp = %d must be a multiple of 4 from 0 to %d", who, c.nramp,
                       VAD_RENDER_MAX_RAMP);
    if (c.nramp > 0 && !c.ramp) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null ramp", who);
    for (int32_t k = 0; k < c.nramp; ++k)
        if (!std::isfinite(c.ramp[k]))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: ramp[%d] is %s, a ramp entry is a finite number", who, k,
                           std::isnan(c.ramp[k]) ? "NaN" : "infinite");
    return VAD_OK;
}

// a. every refusal that needs no device pointer, and the tables: e->cut_segs, e->cut_work (rate_frames: e->cut_rows - the work is
// listed per window, by cut_windows) and the output spans.  Writes nothing to the device.  A call without segments (n == 0) is
// done behind the checks of its own arguments
int cut_check(vad_engine *e, CutPlan &c) {
    const CutCall &k = c.k;
    const char *who = k.who;
    const int64_t n = k.n, audio_samples = k.audio_samples, hop = k.hop;
    if (n < 0 || audio_samples < 0 || k.out_samples < 0 || (n > 0 && !k.items))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer or bad count", who);
    if (int rc = check_block_format(e, who, k.fmt, k.channels)) return rc;
    if (k.stereo && k.channels != 2)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: channels = %d: two-channel blocks only", who, k.channels);
    if (k.layout != VAD_CUT_FRAMES && k.layout != VAD_CUT_RANGE)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: layout = %d is neither VAD_CUT_FRAMES nor VAD_CUT_RANGE", who, k.layout);
    // two resampled rows per chunk would have to pass vadk_cut_resample's window: not built
    if (k.stereo && k.chunk > 0 && k.layout == VAD_CUT_FRAMES)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s: VAD_CUT_FRAMES on a block at %d Hz: both channels of resampled frames "
                       "are not supported, VAD_CUT_RANGE is", who, k.sr_in);
    if (k.out_fmt != VAD_CUT_PCM16 && k.out_fmt != VAD_CUT_F32)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_fmt = %d is neither VAD_CUT_PCM16 nor VAD_CUT_F32", who, k.out_fmt);
    if (int rc = check_block_extent(e, who, k.hop, audio_samples, k.channels, k.fmt)) return rc;
    if (k.kind == CutKind::LEVELS && k.clip != k.clip)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: clip_thresh is NaN", who);
    if (k.kind == CutKind::RENDER)
        if (int rc = render_check(e, k)) return rc;
    c.ab = (size_t)audio_samples * (size_t)k.channels * sample_bytes(k.fmt);
    c.ob = (size_t)(k.out_fmt == VAD_CUT_PCM16 ? 2 : 4) * (k.stereo ? 2 : 1);
    if (n == 0) return VAD_OK;
    const bool resamples = k.resamples(), has_payload = k.has_payload(), rate_frames = k.rate_frames();
    const uint32_t wg_quads = resamples ? VAD_RESAMPLE_CUT_WG_SAMPLES / 4 : vadk::CUT_WG_QUADS;      // the output quads of a workgroup
    const int64_t frame = k.rate() ? k.chunk : e->frame_samples, out_frame = k.rate() ? VAD_FRAME_SAMPLES : frame;
    const uint32_t frameq = (uint32_t)out_frame >> 2;
    while ((1u << c.fshift) < frameq) ++c.fshift;
    // the kernel finds a quad's frame with a shift and a mask: 512 and 256 samples today (the sample range once needs neither:
    // chunks of 768 and 1536 samples pass)
    if (k.layout == VAD_CUT_FRAMES && ((out_frame & 3) || (1u << c.fshift) != frameq))
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s: frames of %lld samples: the cut kernel needs a power of two", who, (long long)out_frame);
    c.spans.resize((size_t)n);
    e->cut_segs.resize((size_t)n);
    e->cut_work.clear();
    e->cut_rows.clear();
    if (resamples) e->rsc_inq.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const vad_cut_item &it = k.items[i];
        if (it.sample_offset < 0 || (it.sample_offset & 3))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld: its recording starts at sample %lld, not a multiple of 4", who,
                           (long long)i, (long long)it.sample_offset);
        if (it.first_frame < 0 || it.nframes < 1)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld: first_frame = %lld, nframes = %lld (>= 0 and >= 1)", who,
                           (long long)i, (long long)it.first_frame, (long long)it.nframes);
        // (all of it below 2^31 before it is multiplied: a segment that fits the block has fewer frames than the block has samples)
        if (it.sample_offset > audio_samples || it.first_frame > audio_samples || it.nframes > audio_samples ||
            it.sample_offset + (it.first_frame + it.nframes - 1) * hop + frame > audio_samples)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld (recording at %lld, frames %lld .. +%lld) leaves the audio block of %lld samples",
                           who, (long long)i, (long long)it.sample_offset, (long long)it.first_frame, (long long)it.nframes, (long long)audio_samples);
        if (k.stereo && it.channel != VAD_SCAN_BOTH)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld names channel %d: both channels are written, "
                           "an item's channel is VAD_SCAN_BOTH", who, (long long)i, it.channel);
        if (!k.stereo && it.channel != VAD_SCAN_MIX && (it.channel < 0 || it.channel >= k.channels))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld names channel %d of %d (0 .. channels - 1, or VAD_SCAN_MIX)", who,
                           (long long)i, it.channel, k.channels);
        if (it.reserved != 0)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld: reserved = %d must be 0", who, (long long)i, it.reserved);
        const int64_t s_in = cut_samples(frame, it.nframes, hop, k.layout, out_frame);
        const int64_t count = resamples ? (s_in * vadk::rsc_L(k.sr_in) / vadk::rsc_M(k.sr_in)) & ~(int64_t)3 : s_in;
        if (has_payload && (it.out_sample < 0 || (it.out_sample & 3) || it.out_sample > k.out_samples || count > k.out_samples - it.out_sample))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld: out_sample = %lld (+%lld samples) must be a multiple of 4 inside "
                           "the output of %lld samples", who, (long long)i, (long long)it.out_sample, (long long)count, (long long)k.out_samples);
        if (count >= (int64_t)4 << 31)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld has %lld output samples, a segment may have less than 2^33", who,
                           (long long)i, (long long)count);
        if (k.gains && !std::isfinite(k.gains[i]))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld: its gain is %s, a gain is a finite number", who, (long long)i,
                           std::isnan(k.gains[i]) ? "NaN" : "infinite");
        c.spans[(size_t)i] = CutSpan{it.out_sample, it.out_sample + count, i};
        const uint32_t mode = k.channels == 1 || k.stereo ? vadk::SCAN_LEFT : it.channel == VAD_SCAN_MIX ? vadk::SCAN_MIX : (uint32_t)it.channel;
        const uint32_t nq = (uint32_t)(count >> 2);
        e->cut_segs[(size_t)i] = vadk::CutSeg{(uint32_t)((it.sample_offset + it.first_frame * hop) >> 2) | (mode << vadk::SCAN_MODE_SHIFT), nq,
                                              has_payload ? (uint64_t)it.out_sample >> 2 : 0u};
        if (rate_frames) {
            e->cut_rows.push_back(vadk::CutResampleSeg{e->cut_segs[(size_t)i].quad_in, (uint32_t)c.rows});
            c.rows += it.nframes;
            if (c.rows > INT32_MAX)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 frames in one call", who);
            continue;
        }
        if (resamples) e->rsc_inq[(size_t)i] = (uint32_t)(s_in >> 2);
        if (k.work_follows_output()) continue;
        for (uint32_t q = 0; q < nq; q += wg_quads) e->cut_work.push_back(vadk::CutWork{(uint32_t)i, q});
        if (e->cut_work.size() > (size_t)INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %d samples in one call", who,
                           (int)(4 * wg_quads));
    }
    if (k.gains) e->cut_gains.assign(k.gains, k.gains + n);
    if (!has_payload) c.spans.clear();       // segments may share samples
    std::sort(c.spans.begin(), c.spans.end(), [](const CutSpan &a, const CutSpan &b) { return a.lo < b.lo; });
    for (size_t j = 1; j < c.spans.size() && k.kind != CutKind::RENDER; ++j)     // a render: render_regions refuses three
        if (c.spans[j].lo < c.spans[j - 1].hi)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the output ranges of segments %lld and %lld overlap", who,
                           (long long)c.spans[j - 1].i, (long long)c.spans[j].i);
    return VAD_OK;
}

// b. the block the call reads and the output it writes.  A device call: the caller's two pointers.  A host call: e->d_audio - the
// resident block (audio = NULL: what the last scan or cut uploaded is still in device memory and crosses the link once; a rate block
// is none of vad_scan_cut's, and the other way round), or room for the upload - and e->d_cut_out
int cut_block(vad_engine *e, CutPlan &c, bool dev, const void *audio, void *out) {
    const CutCall &k = c.k;
    const char *who = k.who;
    if (dev) {
        if (!audio) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
        if (int rc = check_device_audio(e, who, audio, k.channels)) return rc;
        if (k.records_out() && (reinterpret_cast<uintptr_t>(out) & 7))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the %s must be 8-byte aligned", who,
                           k.kind == CutKind::MOMENTS ? "moments" : "levels");
        if (!k.records_out() && (reinterpret_cast<uintptr_t>(out) & 15))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the output must be 16-byte aligned", who);
        c.d_audio = audio;
        c.d_out = out;
        return VAD_OK;
    }
    if (!audio) {
        if (!k.rate() && (!e->audio_resident || e->audio_rate != 0))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: audio = NULL, and the engine holds no resident block: no vad_scan or "
                           "vad_scan_channels has uploaded one", who);
        if (k.rate() && (!e->audio_resident || e->audio_rate == 0))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: audio = NULL, and the engine holds no resident rate block: no "
                           "vad_scan_rate_segments or vad_scan_rate_cut has uploaded one", who);
        if (k.rate() && e->audio_rate != k.sr_in)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: audio = NULL, and the resident block has sample rate %d, not %d", who,
                           e->audio_rate, k.sr_in);
        if (e->audio_fmt != k.fmt)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: audio = NULL, and the resident block has frame format %d, not %d", who,
                           e->audio_fmt, k.fmt);
        if (e->audio_channels != k.channels)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: audio = NULL, and the resident block has %d channels, not %d", who,
                           e->audio_channels, k.channels);
        if (e->audio_bytes != c.ab)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: audio = NULL, and the resident block has %llu bytes, not the %llu of "
                           "%lld samples", who, (unsigned long long)e->audio_bytes, (unsigned long long)c.ab, (long long)k.audio_samples);
    } else {
        e->audio_resident = false;
        if (int rc = ensure(e, e->d_audio, e->d_audio_cap, c.ab + 16)) return rc;
    }
    c.d_audio = e->d_audio;
    if (k.mel()) return VAD_OK;              // the rows of all segments: mel_output sizes them
    if (k.records_out()) {
        if (int rc = ensure(e, e->d_cut_out, e->d_cut_out_cap, (size_t)k.n * sizeof(vad_level))) return rc;
        c.d_out = e->d_cut_out;
        return VAD_OK;
    }
    // the whole output, from sample 0: render_run / audio_batch_run sizes it
    if (k.kind == CutKind::RENDER || k.kind == CutKind::AUDIO_BATCH) return VAD_OK;
    const int64_t out_lo = c.spans.front().lo, out_hi = c.spans.back().hi;
    if (int rc = ensure(e, e->d_cut_out, e->d_cut_out_cap, (size_t)(out_hi - out_lo) * c.ob)) return rc;
    c.d_out = e->d_cut_out;
    // on the device the output starts at the first segment's first sample
    for (vadk::CutSeg &sg : e->cut_segs) sg.quad_out -= (uint64_t)out_lo >> 2;
    return VAD_OK;
}

// c. rate_frames: one window of rows at a time goes through e->d_win.  Per window the cut kernel's segments - one per (segment of
// the call, window), with its place in the window and in the output - and workgroups; per tile of the call the segment that owns
// its first row (vad_layout.h: CutResampleArgs)
int cut_windows(vad_engine *e, CutPlan &c) {
    if (int rc = get_resample_op(e, c.k.chunk, &c.op)) return rc;
    const uint32_t total = (uint32_t)c.rows, wr = cut_window_rows(e);
    std::vector<vadk::CutSeg> wsegs;
    std::vector<float> wgains;               // a window's segment carries its call segment's gain
    e->cut_rows.push_back(vadk::CutResampleSeg{0u, total});
    const std::vector<vadk::CutResampleSeg> &cr = e->cut_rows;
    size_t si = 0;
    for (uint32_t r0 = 0; r0 < total; r0 += wr) {
        const uint32_t r1 = (uint32_t)std::min<uint64_t>(total, (uint64_t)r0 + wr);
        CutWin w{r0, r1, wsegs.size(), e->cut_work.size(), 0};
        while (si < (size_t)c.k.n && cr[si].row0 < r1) {
            const uint32_t lo = std::max(cr[si].row0, r0), hi = std::min(cr[si + 1].row0, r1), nq = (hi - lo) * 128u;
            const uint32_t local = (uint32_t)(wsegs.size() - w.seg0);
            wsegs.push_back(vadk::CutSeg{(lo - r0) * 128u, nq, e->cut_segs[si].quad_out + (uint64_t)(lo - cr[si].row0) * 128u});
            if (c.k.gains) wgains.push_back(e->cut_gains[si]);
            for (uint32_t q = 0; q < nq; q += vadk::CUT_WG_QUADS) e->cut_work.push_back(vadk::CutWork{local, q});
            if (cr[si + 1].row0 > r1) break;     // the segment goes on in the next window
            ++si;
        }
        w.nwork = e->cut_work.size() - w.work0;
        c.wins.push_back(w);
    }
    e->cut_tiles.resize(((size_t)total + vadk::MT - 1) / vadk::MT);
    si = 0;
    for (size_t t = 0; t < e->cut_tiles.size(); ++t) {
        while (cr[si + 1].row0 <= (uint32_t)(t * vadk::MT)) ++si;
        e->cut_tiles[t] = (uint32_t)si;
    }
    e->cut_segs.swap(wsegs);
    if (c.k.gains) e->cut_gains.swap(wgains);
    return ensure(e, e->d_win, e->d_win_cap, (size_t)std::min(total, wr) * 2048u);
}

// The one place that says what e->d_audio holds: a host call's audio goes up on `s` and becomes the resident block, of the call's
// rate.  Every ensure and every refusal of the call lies before it
int cut_upload_audio(vad_engine *e, const CutPlan &c, bool dev, const void *audio, hipStream_t s) {
    if (dev || !audio || c.k.n == 0) return VAD_OK;
    HIP_TRY(e, hipMemcpyAsync(e->d_audio, audio, c.ab, hipMemcpyHostToDevice, s));
    set_resident(e, c.ab, c.k.channels, c.k.fmt, c.k.sr_in);
    return VAD_OK;
}

// d. the first writes, on `s`: host audio and the tables, which lie in e->d_cut (`t`) in the order of the names ...
enum { CUT_SEGS, CUT_WORK, CUT_ROWS, CUT_TILES, CUT_GAINS };
int cut_upload(vad_engine *e, const CutPlan &c, DevTables &t, bool dev, const void *audio, hipStream_t s) {
    const CutCall &k = c.k;
    t.add(e->cut_segs, e->cut_segs.size());
    t.add(e->cut_work, e->cut_work.size());
    t.add(e->cut_rows, k.rate_frames() ? e->cut_rows.size() : 0);
    t.add(e->cut_tiles, k.rate_frames() ? e->cut_tiles.size() : 0);
    t.add(e->cut_gains, k.gains ? e->cut_gains.size() : 0);
    if (int rc = t.reserve(e)) return rc;
    if (int rc = cut_upload_audio(e, c, dev, audio, s)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    if (k.records_out()) HIP_TRY(e, hipMemsetAsync(c.d_out, 0, (size_t)k.n * sizeof(vad_level), s));
    return VAD_OK;
}

// ... and the launches: one cut, or per window of a rate cut's frames the resampler and the cut of what it wrote
int cut_launches(vad_engine *e, const CutPlan &c, const DevTables &t, hipStream_t s) {
    const CutCall &k = c.k;
    const float *d_gains = t.at<const float>(CUT_GAINS);
    vadk::CutArgs a{};
    a.audio = c.d_audio;
    a.out = c.d_out;
    a.segs = t.at<const vadk::CutSeg>(CUT_SEGS);
    a.work = t.at<const vadk::CutWork>(CUT_WORK);
    a.audio_bytes = (uint32_t)c.ab;
    a.nwork = (uint32_t)e->cut_work.size();
    a.hopq = (uint32_t)k.hop >> 2;
    a.frame_shift = k.layout == VAD_CUT_FRAMES ? c.fshift : 31u;
    a.fmt = k.fmt;
    a.channels = k.channels;
    a.out_fmt = k.out_fmt;
    a.thresh = k.gate();
    if (!k.rate_frames()) {
        const bool levels = k.records_out();
        const hipError_t r = k.kind == CutKind::MOMENTS ? vadk_launch_seg_moments(&a, s)
                             : levels   ? vadk_launch_seg_levels(&a, k.clip, s)
                             : k.stereo ? vadk_launch_scan_cut_stereo(&a, d_gains, s)
                             : d_gains  ? vadk_launch_scan_cut_gain(&a, d_gains, s)
                                        : vadk_launch_scan_cut(&a, s);
        return r != hipSuccess ? e->hip_fail(r, k.kind == CutKind::MOMENTS ? "kernel launch (segment moments)"
                                              : levels ? "kernel launch (segment levels)" : "kernel launch (scan cut)") : VAD_OK;
    }
    vadk::CutResampleArgs ra{};
    ra.wstream = c.op->d_w;
    ra.wstream_bytes = (uint32_t)c.op->bytes;
    ra.tile_blocks = c.op->tile_blocks;
    ra.row128_block = c.op->row128_block;
    ra.audio_bytes = (uint32_t)c.ab;
    ra.audio = c.d_audio;
    ra.segs = t.at<const vadk::CutResampleSeg>(CUT_ROWS);
    ra.tile_seg = t.at<const uint32_t>(CUT_TILES);
    ra.win = e->d_win;
    ra.n_in = k.chunk;
    ra.hopq = (uint32_t)k.hop >> 2;
    ra.fmt = k.fmt;
    ra.channels = k.channels;
    // the window as the cut kernel sees it: mono float32 frames of 512 samples, back to back
    a.audio = e->d_win;
    a.hopq = VAD_FRAME_SAMPLES / 4;
    a.fmt = VAD_FMT_F32;
    a.channels = 1;
    for (const CutWin &w : c.wins) {
        ra.r0 = w.r0;
        ra.rows_end = w.r1;
        hipError_t r = vadk_launch_cut_resample(&ra, s);
        if (r != hipSuccess) return e->hip_fail(r, "kernel launch (cut resample)");
        // the window's slices of the same tables
        a.segs = t.at<const vadk::CutSeg>(CUT_SEGS) + w.seg0;
        a.work = t.at<const vadk::CutWork>(CUT_WORK) + w.work0;
        a.nwork = (uint32_t)w.nwork;
        a.audio_bytes = (w.r1 - w.r0) * 2048u;
        r = d_gains ? vadk_launch_scan_cut_gain(&a, d_gains + w.seg0, s) : vadk_launch_scan_cut(&a, s);
        if (r != hipSuccess) return e->hip_fail(r, "kernel launch (scan cut)");
    }
    return VAD_OK;
}

// e. a host call: only speech crosses the link back - one copy per run of adjoining segments (packed payloads: one), the gaps stay
// the caller's
int cut_copy_back(vad_engine *e, const CutPlan &c, void *out, hipStream_t s) {
    if (c.k.records_out()) {
        HIP_TRY(e, hipMemcpyAsync(out, c.d_out, (size_t)c.k.n * sizeof(vad_level), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        return VAD_OK;
    }
    const std::vector<CutSpan> &spans = c.spans;
    const int64_t out_lo = spans.front().lo;
    for (size_t k = 0; k < spans.size();) {
        size_t m = k + 1;
        while (m < spans.size() && spans[m].lo == spans[m - 1].hi) ++m;
        HIP_TRY(e, hipMemcpyAsync(static_cast<uint8_t *>(out) + (size_t)spans[k].lo * c.ob, static_cast<uint8_t *>(c.d_out) + (size_t)(spans[k].lo - out_lo) * c.ob,
                                  (size_t)(spans[m - 1].hi - spans[k].lo) * c.ob, hipMemcpyDeviceToHost, s));
        k = m;
    }
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// The PAYLOAD, LEVELS and MOMENTS kinds (dev = false: host audio, or NULL = the resident block, and a host `out`; dev: two device pointers),
// with e->mu held.  Every check comes before the first write: phases a to c refuse or size buffers, cut_upload writes first.  A
// gained cut's kernel applies the factors; the levels' (moments') `out` is n vad_level (vad_moments) records, cleared on the stream ahead of the reducing kernel
int cut_run(vad_engine *e, bool dev, const CutCall &k, const void *audio, void *out, hipStream_t s) {
    CutPlan c{k};
    if (k.gains_required && k.n > 0 && !k.gains) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null gains", k.who);
    if (int rc = cut_check(e, c)) return rc;
    if (k.n == 0) return VAD_OK;
    if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", k.who);
    if (int rc = cut_block(e, c, dev, audio, out)) return rc;
    if (k.rate_frames())
        if (int rc = cut_windows(e, c)) return rc;
    DevTables t{e->d_cut, e->d_cut_cap};
    if (int rc = cut_upload(e, c, t, dev, audio, s)) return rc;
    const int rc = call_end(e, dev, s, cut_launches(e, c, t, s));
    if (rc || dev) return rc;
    return cut_copy_back(e, c, out, s);
}

// vad_scan_render: the output [0, out_samples) swept into REGIONS - maximal intervals that the same none, one or two segments
// cover - and each region into workgroups of CUT_WG_QUADS output quads (e->render_work).  c.spans is sorted by lo; the ends of the
// spans are a second sorted list, and the sweep merges the two, ends first where they meet a start: a segment that ends where
// another begins does not overlap it.  A start that finds two segments open is the triple cover the call refuses.
int render_regions(vad_engine *e, const CutPlan &c) {
    std::vector<CutSpan> ends(c.spans);
    std::sort(ends.begin(), ends.end(), [](const CutSpan &a, const CutSpan &b) { return a.hi < b.hi; });
    e->render_work.clear();
    int64_t open[2] = {-1, -1}, at = 0;
    int nopen = 0;
    // the region [at, hi) under the segments now open; false: more workgroups than a launch has (checked before any is listed - a
    // gap may be as long as the caller's out_samples says)
    auto emit = [&](int64_t hi) {
        const int64_t q0 = at >> 2, q1 = hi >> 2;
        if (q1 <= q0) return true;
        if ((q1 - q0 + vadk::CUT_WG_QUADS - 1) / vadk::CUT_WG_QUADS + (int64_t)e->render_work.size() > (int64_t)INT32_MAX) return false;
        const uint32_t a = nopen > 0 ? (uint32_t)open[0] : vadk::RENDER_NONE, b = nopen > 1 ? (uint32_t)open[1] : vadk::RENDER_NONE;
        for (int64_t q = q0; q < q1; q += vadk::CUT_WG_QUADS)
            e->render_work.push_back(vadk::RenderWork{a, b, (uint64_t)q, (uint32_t)std::min<int64_t>(vadk::CUT_WG_QUADS, q1 - q), 0u});
        at = hi;
        return true;
    };
    auto too_many = [&]() {
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %d samples in one call", c.k.who, VAD_CUT_WG_SAMPLES);
    };
    size_t is = 0, ie = 0;
    while (ie < ends.size()) {
        if (is < c.spans.size() && c.spans[is].lo < ends[ie].hi) {
            const CutSpan &sp = c.spans[is++];
            if (!emit(sp.lo)) return too_many();
            if (nopen == 2)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: output sample %lld is covered by the segments %lld, %lld and %lld, "
                               "at most two may overlap", c.k.who, (long long)sp.lo, (long long)open[0], (long long)open[1], (long long)sp.i);
            open[nopen++] = sp.i;
        } else {
            const CutSpan &sp = ends[ie++];
            if (!emit(sp.hi)) return too_many();
            if (open[0] == sp.i) open[0] = open[1];
            --nopen;
        }
    }
    if (!emit(c.k.out_samples)) return too_many();
    return VAD_OK;
}

// The RENDER kind with e->mu held: cut_check's refusals under this name (without the overlap of two), the regions, then the block
// and the output as the cuts find them, one upload of the tables - segments, ramp, workgroups, gains, in this order in e->d_cut -
// and one launch, which writes every quad of the output: the gaps are zeroed by workgroups of the same launch (no memset per gap,
// and no second pass over the samples a memset of the whole output would cost).
int render_run(vad_engine *e, bool dev, const CutCall &k, const void *audio, void *out, hipStream_t s) {
    CutPlan c{k};
    if (int rc = cut_check(e, c)) return rc;
    if (k.n == 0) e->cut_segs.clear();
    if (int rc = render_regions(e, c)) return rc;
    if (k.out_samples == 0) return VAD_OK;
    if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", k.who);
    // a render without segments reads no block: only its output is looked at
    if (k.n > 0) {
        if (int rc = cut_block(e, c, dev, audio, out)) return rc;
    } else if (dev && (reinterpret_cast<uintptr_t>(out) & 15)) {
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the output must be 16-byte aligned", k.who);
    }
    c.d_out = out;
    if (!dev) {
        if (int rc = ensure(e, e->d_cut_out, e->d_cut_out_cap, (size_t)k.out_samples * c.ob)) return rc;
        c.d_out = e->d_cut_out;
    }
    e->render_ramp.assign(k.ramp, k.ramp + k.nramp);
    DevTables t{e->d_cut, e->d_cut_cap};
    const int segs = t.add(e->cut_segs, e->cut_segs.size()), ramp = t.add(e->render_ramp, (size_t)k.nramp);
    const int work = t.add(e->render_work, e->render_work.size()), gains = t.add(e->cut_gains, k.gains ? (size_t)k.n : 0);
    if (int rc = t.reserve(e)) return rc;
    if (int rc = cut_upload_audio(e, c, dev, audio, s)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    vadk::RenderArgs a{};
    a.audio = k.n > 0 ? c.d_audio : nullptr;
    a.out = c.d_out;
    a.segs = t.at<const vadk::CutSeg>(segs);
    a.work = t.at<const vadk::RenderWork>(work);
    a.gains = t.at<const float>(gains);
    a.ramp = t.at<const float>(ramp);
    a.audio_bytes = k.n > 0 ? (uint32_t)c.ab : 0u;
    a.nwork = (uint32_t)e->render_work.size();
    a.nrampq = (uint32_t)k.nramp >> 2;
    a.fmt = k.fmt;
    a.channels = k.channels;
    a.out_fmt = k.out_fmt;
    a.thresh = k.gate();
    const hipError_t r = k.stereo ? vadk_launch_scan_render_stereo(&a, s) : vadk_launch_scan_render(&a, s);
    const int rc = call_end(e, dev, s, r != hipSuccess ? e->hip_fail(r, "kernel launch (scan render)") : VAD_OK);
    if (rc || dev) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, c.d_out, (size_t)k.out_samples * c.ob, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// The number format of a batch's cells, which vad_batch and vad_audio_batch name alike: dtype, pad_mode, pad_value, in this order
int batch_format_check(vad_engine *e, const char *who, int32_t dtype, int32_t pad_mode, float pad_value) {
    if (dtype != VAD_BATCH_F32 && dtype != VAD_BATCH_F16 && dtype != VAD_BATCH_BF16)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: dtype = %d is none of VAD_BATCH_F32, VAD_BATCH_F16, VAD_BATCH_BF16", who, dtype);
    if (pad_mode != VAD_BATCH_PAD_VALUE && pad_mode != VAD_BATCH_PAD_FEATURE)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: pad_mode = %d is neither VAD_BATCH_PAD_VALUE nor VAD_BATCH_PAD_FEATURE", who, pad_mode);
    if (!std::isfinite(pad_value))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: pad_value is %s, a pad value is a finite number", who,
                       std::isnan(pad_value) ? "NaN" : "infinite");
    return VAD_OK;
}

// The nss rule: without shift and scale nss is not read and is 1; else they have one `row` ("row", "entry") or one per `over` ("n",
// "nw"), of which the call has `count`
int batch_nss(vad_engine *e, const char *who, const float *shift, const float *scale, int64_t *nss, const char *row, const char *over, int64_t count) {
    if (!shift && !scale) *nss = 1;
    if (*nss != 1 && *nss != count)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: nss = %lld: shift and scale have 1 %s or %s = %lld", who, (long long)*nss, row,
                       over, (long long)count);
    return VAD_OK;
}

// ... and their table as it goes up: shift, else zeros, in hs [count] and scale, else ones, in hc [count]
void affine_fill(float *hs, float *hc, const float *shift, const float *scale, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        hs[i] = shift ? shift[i] : 0.0f;
        hc[i] = scale ? scale[i] : 1.0f;
    }
}

// The AUDIO_BATCH kind with e->mu held: cut_check's refusals under this name, then the batch's own in the header's order, then the
// block as the levels find it.  Its work follows the output: a workgroup per CUT_WG_QUADS quads of a window, listed here.  One
// upload of the tables - segments, windows, workgroups, shift and scale, in this order in e->d_cut - and one launch, which writes
// every cell of the output and of the mask.  A host call's output and mask lie in e->d_cut_out, the mask behind the windows
int audio_batch_run(vad_engine *e, bool dev, const CutCall &k, const void *audio, void *out, hipStream_t s) {
    const char *who = k.who;
    CutPlan c{k};
    if (int rc = cut_check(e, c)) return rc;
    const vad_audio_batch *b = k.ab;
    if (!b) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null vad_audio_batch", who);
    if (b->samples < 4 || b->samples > (1 << 24) || (b->samples & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: samples = %d must be a multiple of 4 from 4 to 2^24", who, b->samples);
    if (int rc = batch_format_check(e, who, b->dtype, b->pad_mode, b->pad_value)) return rc;
    const int64_t nw = k.nw, n = k.n, T = b->samples;
    if (nw < 0 || k.out_bytes < 0 || (nw > 0 && !k.awin)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer or bad count", who);
    int64_t nss = k.nss;
    if (int rc = batch_nss(e, who, k.shift, k.scale, &nss, "entry", "n", n)) return rc;
    for (int which = 0; which < 2; ++which) {
        const float *v = which ? k.scale : k.shift;
        for (int64_t i = 0; v && i < nss; ++i)
            if (!std::isfinite(v[i]))
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %s[%lld] is %s, a %s is a finite number", who, which ? "scale" : "shift",
                               (long long)i, std::isnan(v[i]) ? "NaN" : "infinite", which ? "scale" : "shift");
    }
    e->ab_win.resize((size_t)nw);
    for (int64_t j = 0; j < nw; ++j) {
        const vad_audio_window &w = k.awin[j];
        if (w.seg < 0 || (int64_t)w.seg >= n)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: window %lld names segment %d of %lld", who, (long long)j, w.seg, (long long)n);
        const int64_t S = (int64_t)e->cut_segs[(size_t)w.seg].nquads * 4;
        if (w.sample0 < 0 || (w.sample0 & 3) || w.nsamples < 0 || w.nsamples > T || w.sample0 > S || w.nsamples > S - w.sample0)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: window %lld: samples %lld .. +%d of segment %d, which has %lld, in %lld "
                           "samples (sample0 a multiple of 4)", who, (long long)j, (long long)w.sample0, w.nsamples, w.seg, (long long)S, (long long)T);
        e->ab_win[(size_t)j] = vadk::AudioWin{(uint32_t)w.seg, (uint32_t)(w.sample0 >> 2), (uint32_t)w.nsamples, 0u};
    }
    const size_t esize = b->dtype == VAD_BATCH_F32 ? 4u : 2u, cells = (size_t)nw * (size_t)T, need = cells * esize;
    if (need > (size_t)k.out_bytes)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_bytes = %lld, the windows have %llu bytes", who, (long long)k.out_bytes,
                       (unsigned long long)need);
    const uint32_t tq = (uint32_t)T >> 2, per_win = (tq + vadk::CUT_WG_QUADS - 1u) / vadk::CUT_WG_QUADS;
    if ((uint64_t)nw * per_win > (uint64_t)INT32_MAX)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %d samples in one call", who, VAD_CUT_WG_SAMPLES);
    if (nw == 0) return VAD_OK;
    if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (int rc = cut_block(e, c, dev, audio, out)) return rc;
    if (dev && (reinterpret_cast<uintptr_t>(k.mask) & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the mask must be 4-byte aligned", who);
    e->ab_work.clear();
    e->ab_work.reserve((size_t)nw * per_win);
    for (int64_t j = 0; j < nw; ++j)
        for (uint32_t q = 0; q < tq; q += vadk::CUT_WG_QUADS) e->ab_work.push_back(vadk::AudioWork{(uint32_t)j, q});
    e->ab_f.resize(2 * (size_t)nss);
    affine_fill(e->ab_f.data(), e->ab_f.data() + nss, k.shift, k.scale, (size_t)nss);
    DevTables t{e->d_cut, e->d_cut_cap};
    const int segs = t.add(e->cut_segs, e->cut_segs.size()), win = t.add(e->ab_win, e->ab_win.size());
    const int work = t.add(e->ab_work, e->ab_work.size()), floats = t.add(e->ab_f, e->ab_f.size());
    if (int rc = t.reserve(e)) return rc;
    const size_t mask_off = (need + 15) & ~(size_t)15;
    c.d_out = out;
    uint8_t *d_mask = k.mask;
    if (!dev) {
        if (int rc = ensure(e, e->d_cut_out, e->d_cut_out_cap, mask_off + (k.mask ? cells : 0))) return rc;
        c.d_out = e->d_cut_out;
        d_mask = k.mask ? static_cast<uint8_t *>(c.d_out) + mask_off : nullptr;
    }
    if (int rc = cut_upload_audio(e, c, dev, audio, s)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    vadk::AudioBatchArgs a{};
    a.audio = c.d_audio;
    a.out = c.d_out;
    a.mask = d_mask;
    a.segs = t.at<const vadk::CutSeg>(segs);
    a.win = t.at<const vadk::AudioWin>(win);
    a.work = t.at<const vadk::AudioWork>(work);
    a.shift = t.at<const float>(floats);
    a.scale = a.shift + nss;
    a.audio_bytes = (uint32_t)c.ab;
    a.nwork = (uint32_t)e->ab_work.size();
    a.tq = tq;
    a.per_seg = nss == 1 ? 0u : 1u;
    a.fmt = k.fmt;
    a.channels = k.channels;
    a.dtype = b->dtype;
    a.pad_mode = b->pad_mode;
    a.pad_value = b->pad_value;
    a.thresh = k.gate();
    const hipError_t r = vadk_launch_audio_batch(&a, s);
    const int rc = call_end(e, dev, s, r != hipSuccess ? e->hip_fail(r, "kernel launch (audio batch)") : VAD_OK);
    if (rc || dev) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, c.d_out, need, hipMemcpyDeviceToHost, s));
    if (k.mask) HIP_TRY(e, hipMemcpyAsync(k.mask, d_mask, cells, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// vad_mel's fields: 0 = all in range, else the number of the first that is not (1 n_fft .. 8 reserved)
int mel_bad_field(const vad_mel *m) {
    if (m->n_fft < 64 || m->n_fft > 1024 || (m->n_fft & 15)) return 1;
    if (m->hop < 4 || m->hop > m->n_fft || (m->hop & 3)) return 2;
    if (m->n_bins < 1 || m->n_bins > m->n_fft / 2 + 1) return 3;
    if (m->n_mels < 1 || m->n_mels > 128) return 4;
    if (m->pad != VAD_MEL_PAD_NONE && m->pad != VAD_MEL_PAD_REFLECT) return 5;
    if (m->log != VAD_MEL_LINEAR && m->log != VAD_MEL_LN && m->log != VAD_MEL_LOG10) return 6;
    if (m->log != VAD_MEL_LINEAR && !(std::isfinite(m->floor) && m->floor > 0.0f)) return 7;
    if (m->reserved != 0) return 8;
    return 0;
}

// the analysis frames of a segment of S samples (the header's M); the reflect rule S > n_fft / 2 is the caller's to check
int64_t mel_frames(const vad_mel *m, int64_t S) {
    const int64_t len = S + (m->pad == VAD_MEL_PAD_REFLECT ? m->n_fft : 0);
    return len < m->n_fft ? 0 : (len - m->n_fft) / m->hop + 1;
}

// vad_scan_mel's own arguments, ahead of the block's and the items' checks
int mel_check(vad_engine *e, const CutCall &k) {
    const char *who = k.who;
    const vad_mel *m = k.m;
    if (!m) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null vad_mel", who);
    switch (mel_bad_field(m)) {
        case 1: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n_fft = %d must be a multiple of 16 from 64 to 1024", who, m->n_fft);
        case 2: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: hop = %d must be a multiple of 4 from 4 to n_fft = %d", who, m->hop, m->n_fft);
        case 3: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n_bins = %d must be 1 .. n_fft / 2 + 1 = %d", who, m->n_bins, m->n_fft / 2 + 1);
        case 4: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n_mels = %d must be 1 .. 128", who, m->n_mels);
        case 5: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: pad = %d is neither VAD_MEL_PAD_NONE nor VAD_MEL_PAD_REFLECT", who, m->pad);
        case 6: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: log = %d is none of VAD_MEL_LINEAR, VAD_MEL_LN, VAD_MEL_LOG10", who, m->log);
        case 7: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: floor = %g: a logarithm needs a finite floor > 0", who, (double)m->floor);
        case 8: return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: vad_mel.reserved = %d must be 0", who, m->reserved);
        default: break;
    }
    if (!k.op_re || !k.op_im) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null operator", who);
    if (!k.filters) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null filters", who);
    if (k.out_rows < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_rows = %lld is negative", who, (long long)k.out_rows);
    return VAD_OK;
}

// the operator and the filters in fragment order in e->d_mel (vad_layout.h), zero-padded to whole tiles of 16 bins and 16 mels.
// Cached against the bytes of the previous call: the same vad_mel and the same three arrays neither pack nor upload again (the
// compare reads what a pack would read, and writes nothing)
int mel_operator(vad_engine *e, const vad_mel *m, const float *op_re, const float *op_im, const float *filters, hipStream_t s) {
    const size_t nb = (size_t)m->n_bins, no = (size_t)m->n_fft * nb, nf = (size_t)m->n_mels * nb;
    const uint32_t bins_pad = vadk::mel_pad16((uint32_t)m->n_bins), mels_pad = vadk::mel_pad16((uint32_t)m->n_mels);
    const bool same = e->mel_packed && e->mel_key.n_fft == m->n_fft && e->mel_key.n_bins == m->n_bins && e->mel_key.n_mels == m->n_mels &&
                      e->mel_src.size() == 2 * no + nf && !std::memcmp(e->mel_src.data(), op_re, no * sizeof(float)) &&
                      !std::memcmp(e->mel_src.data() + no, op_im, no * sizeof(float)) &&
                      !std::memcmp(e->mel_src.data() + 2 * no, filters, nf * sizeof(float));
    if (same) return VAD_OK;
    e->mel_packed = false;
    const size_t po = 2 * (size_t)m->n_fft * bins_pad, pf = (size_t)mels_pad * bins_pad;
    if (int rc = ensure(e, e->d_mel, e->d_mel_cap, (po + pf) * sizeof(float))) return rc;
    e->mel_src.resize(2 * no + nf);
    std::memcpy(e->mel_src.data(), op_re, no * sizeof(float));
    std::memcpy(e->mel_src.data() + no, op_im, no * sizeof(float));
    std::memcpy(e->mel_src.data() + 2 * no, filters, nf * sizeof(float));
    e->mel_pack.assign(po + pf, 0.0f);
    for (uint32_t n = 0; n < (uint32_t)m->n_fft; ++n)
        for (uint32_t k = 0; k < (uint32_t)m->n_bins; ++k) {
            const size_t at = vadk::mel_op_index(n, k, (uint32_t)m->n_fft);
            e->mel_pack[at] = op_re[(size_t)n * nb + k];
            e->mel_pack[at + 1] = op_im[(size_t)n * nb + k];
        }
    for (uint32_t j = 0; j < (uint32_t)m->n_mels; ++j)
        for (uint32_t k = 0; k < (uint32_t)m->n_bins; ++k) e->mel_pack[po + vadk::mel_filter_index(j, k, bins_pad)] = filters[(size_t)j * nb + k];
    HIP_TRY(e, hipMemcpyAsync(e->d_mel, e->mel_pack.data(), (po + pf) * sizeof(float), hipMemcpyHostToDevice, s));
    e->mel_key = *m;
    e->mel_packed = true;
    return VAD_OK;
}

// the frames and rows of every segment of `segs` (nquads: its samples / 4; quad_out becomes its first row) and one workgroup per
// tile of MEL_TILE frames in e->mel_work; *rows: the total
int mel_tiles(vad_engine *e, const char *who, const vad_mel *m, std::vector<vadk::CutSeg> &segs, int64_t *rows_out) {
    e->mel_work.clear();
    int64_t rows = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        vadk::CutSeg &sg = segs[i];
        const int64_t S = (int64_t)sg.nquads << 2;
        if (m->pad == VAD_MEL_PAD_REFLECT && S <= m->n_fft / 2)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld has %lld samples: reflect padding needs more than n_fft / 2 = %d",
                           who, (long long)i, (long long)S, m->n_fft / 2);
        const int64_t M = mel_frames(m, S);
        sg.quad_out = (uint64_t)rows;
        rows += M;
        if ((int64_t)e->mel_work.size() + (M + vadk::MEL_TILE - 1) / vadk::MEL_TILE > (int64_t)INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %d frames in one call", who, vadk::MEL_TILE);
        for (int64_t f = 0; f < M; f += vadk::MEL_TILE) e->mel_work.push_back(vadk::MelWork{(uint32_t)i, (uint32_t)f});
    }
    *rows_out = rows;
    return VAD_OK;
}

// the launch of vadk_seg_mel over a block on the device, its tables (device pointers) and the packed operator in e->d_mel
int mel_launch(vad_engine *e, const vad_mel *m, const void *d_audio, size_t audio_bytes, int fmt, int32_t channels, float thr, float *d_out,
               const vadk::CutSeg *d_segs, const vadk::MelWork *d_work, hipStream_t s) {
    vadk::MelArgs a{};
    a.audio = d_audio;
    a.out = d_out;
    a.segs = d_segs;
    a.work = d_work;
    a.bins_pad = vadk::mel_pad16((uint32_t)m->n_bins);
    a.op = e->d_mel;
    a.filters = e->d_mel + 2 * (size_t)m->n_fft * a.bins_pad;
    a.audio_bytes = (uint32_t)audio_bytes;
    a.nwork = (uint32_t)e->mel_work.size();
    a.n_fft = (uint32_t)m->n_fft;
    a.hop = (uint32_t)m->hop;
    a.n_mels = (uint32_t)m->n_mels;
    a.pad = m->pad;
    a.log = m->log;
    a.floor = m->floor;
    a.thresh = thr;
    a.fmt = fmt;
    a.channels = channels;
    const hipError_t r = vadk_launch_seg_mel(&a, s);
    return r != hipSuccess ? e->hip_fail(r, "kernel launch (segment mel)") : VAD_OK;
}

// vad_scan_mel_keep: the segments' first rows (quad_out of the first n of `segs`), the total and n_mels of the resident matrix
void melk_remember(vad_engine *e, const std::vector<vadk::CutSeg> &segs, size_t n, int64_t rows, int32_t n_mels, int64_t *rows_out) {
    e->melk_start.resize(n + 1);
    for (size_t i = 0; i < n; ++i) e->melk_start[i] = (int64_t)segs[i].quad_out;
    e->melk_start[n] = rows;
    e->melk_n_mels = n_mels;
    if (rows_out) *rows_out = rows;
}

// The output rules of the mel kinds, once for vad_scan_mel and vad_scan_rate_mel (c.mel_rows: the rows of all segments).  Ahead of
// the first write: the refusals of rows and pointer, the block as the cuts find it, then where the rows go - the caller's device
// pointer, e->d_cut_out for a host call, e->d_melk for a keep
int mel_output(vad_engine *e, CutPlan &c, bool dev, const void *audio, void *out) {
    const CutCall &k = c.k;
    if (!k.keep && c.mel_rows > k.out_rows)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_rows = %lld, the segments have %lld rows", k.who, (long long)k.out_rows,
                       (long long)c.mel_rows);
    if (!k.keep && c.mel_rows > 0 && !out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", k.who);
    if (int rc = cut_block(e, c, dev, audio, out)) return rc;
    c.mel_bytes = (size_t)c.mel_rows * (size_t)k.m->n_mels * sizeof(float);
    if (k.keep) {
        // every refusal lies behind: the previous matrix ends here
        e->melk_start.clear();
        if (int rc = ensure(e, e->d_melk, e->d_melk_cap, c.mel_bytes)) return rc;
        c.d_out = e->d_melk;
    } else if (!dev) {
        if (int rc = ensure(e, e->d_cut_out, e->d_cut_out_cap, c.mel_bytes)) return rc;
        c.d_out = e->d_cut_out;
    }
    return VAD_OK;
}

// ... and behind the launches, whose status is `launched`: a keep remembers its matrix (`segs`: the table vadk_seg_mel read), then
// the way out, and a host call's rows cross the link back
int mel_finish(vad_engine *e, const CutPlan &c, bool dev, const std::vector<vadk::CutSeg> &segs, int launched, void *out, hipStream_t s) {
    const CutCall &k = c.k;
    if (k.keep && !launched) melk_remember(e, segs, (size_t)k.n, c.mel_rows, k.m->n_mels, k.rows_out);
    const int rc = call_end(e, dev, s, launched);
    if (rc || dev) return rc;
    if (c.mel_bytes && !k.keep) HIP_TRY(e, hipMemcpyAsync(out, c.d_out, c.mel_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// The MEL kind with e->mu held: the call's own checks, cut_check's refusals under this name (the sample range once, no out_sample),
// the frames and rows of every segment and one workgroup per tile of MEL_TILE frames, then the block and the output (mel_output),
// the operator (mel_operator), one upload of the tables - segments, workgroups, in this order in e->d_cut - and one launch.
int mel_run(vad_engine *e, bool dev, const CutCall &k, const void *audio, void *out, hipStream_t s) {
    if (int rc = mel_check(e, k)) return rc;
    CutPlan c{k};
    if (int rc = cut_check(e, c)) return rc;
    if (k.n == 0) {
        if (k.keep) melk_remember(e, e->cut_segs, 0, 0, k.m->n_mels, k.rows_out);
        return VAD_OK;
    }
    if (int rc = mel_tiles(e, k.who, k.m, e->cut_segs, &c.mel_rows)) return rc;
    if (int rc = mel_output(e, c, dev, audio, out)) return rc;
    DevTables t{e->d_cut, e->d_cut_cap};
    const int segs = t.add(e->cut_segs, e->cut_segs.size()), work = t.add(e->mel_work, e->mel_work.size());
    if (int rc = t.reserve(e)) return rc;
    if (int rc = mel_operator(e, k.m, k.op_re, k.op_im, k.filters, s)) return rc;
    if (int rc = cut_upload_audio(e, c, dev, audio, s)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    const int rc = mel_launch(e, k.m, c.d_audio, c.ab, k.fmt, k.channels, k.thr, static_cast<float *>(c.d_out), t.at<const vadk::CutSeg>(segs),
                              t.at<const vadk::MelWork>(work), s);
    return mel_finish(e, c, dev, e->cut_segs, rc, out, s);
}

// what comes before the block's and the items' checks in vad_scan_resample_cut / vad_scan_rate_mel: the engine's frames, the input
// rate (16000 has nothing to resample) and the taps
int resample_cut_check(vad_engine *e, const char *who, int32_t sr_in, const float *taps, int32_t ntaps, int *chunk) {
    if (e->frame_samples != VAD_FRAME_SAMPLES || e->sample_rate != 16000)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: %s: this engine runs an 8 kHz sub-model on %d-sample frames; "
                       "resampled recordings need the 16 kHz one", who, e->frame_samples);
    *chunk = sr_in == 16000 ? 0 : resample_chunk_len(sr_in);
    if (*chunk == 0)
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: %s: supported input rates are 8000, 24000, 48000", sr_in, who);
    if (!taps) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null taps", who);
    if (ntaps < 1 || ntaps > VAD_RESAMPLE_CUT_MAX_TAPS || !(ntaps & 1))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: ntaps = %d must be odd, from 1 to %d", who, ntaps, VAD_RESAMPLE_CUT_MAX_TAPS);
    for (int32_t k = 0; k < ntaps; ++k)
        if (!std::isfinite(taps[k]))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: taps[%d] is %s, a tap is a finite number", who, k,
                           std::isnan(taps[k]) ? "NaN" : "infinite");
    return VAD_OK;
}

// T of the taps in fragment order in e->d_rsc (vad_layout.h: rsc_pack_index), zeros outside the taps.  Cached against the bytes of
// the previous call, as mel_operator is: the same rate and the same taps neither pack nor upload again
int resample_cut_operator(vad_engine *e, int32_t sr_in, const float *taps, int32_t ntaps, hipStream_t s) {
    const uint32_t L = vadk::rsc_L(sr_in), M = vadk::rsc_M(sr_in), K = vadk::rsc_K((uint32_t)ntaps, L, M);
    if (e->rsc_packed && e->rsc_rate == sr_in && e->rsc_src.size() == (size_t)ntaps && !std::memcmp(e->rsc_src.data(), taps, sizeof(float) * (size_t)ntaps))
        return VAD_OK;
    e->rsc_packed = false;
    if (int rc = ensure(e, e->d_rsc, e->d_rsc_cap, sizeof(float) * 16u * K)) return rc;
    e->rsc_src.assign(taps, taps + ntaps);
    e->rsc_pack.assign((size_t)16u * K, 0.0f);
    for (uint32_t o = 0; o < 16u; ++o)
        for (uint32_t n = 0; n < K; ++n) {
            const int32_t t = vadk::rsc_tap(o, n, (uint32_t)ntaps, L, M);
            if (t >= 0 && t < ntaps) e->rsc_pack[vadk::rsc_pack_index(o, n)] = taps[t];
        }
    HIP_TRY(e, hipMemcpyAsync(e->d_rsc, e->rsc_pack.data(), sizeof(float) * 16u * K, hipMemcpyHostToDevice, s));
    e->rsc_rate = sr_in;
    e->rsc_packed = true;
    return VAD_OK;
}

// The RESAMPLE and RESAMPLE_MEL kinds with e->mu held (k by value: the check settles its chunk).  The rate cut's plan: its block and
// item refusals, segment table, block rules and output spans, with S16 samples per segment - its samples at 16 kHz, in the out_sample
// check, the spans and CutSeg::nquads - its input quads in e->rsc_inq and one workgroup per RSC_WG_SAMPLES outputs.  RESAMPLE_MEL:
// the resample kernel writes the segments back to back into e->d_rsc_mid, and vadk_seg_mel runs behind it on the same stream over
// that buffer as a mono float32 block - the header's recipe - with its own segment table and tiles.  In e->d_cut: segments, mel
// segments, workgroups, mel tiles, input quads, gains.
int resample_cut_run(vad_engine *e, bool dev, CutCall k, const void *audio, void *out, hipStream_t s) {
    if (int rc = resample_cut_check(e, k.who, k.sr_in, k.taps, k.ntaps, &k.chunk)) return rc;
    CutPlan c{k};
    if (int rc = cut_check(e, c)) return rc;
    const bool mel = k.mel();
    if (mel)
        if (int rc = mel_check(e, k)) return rc;
    if (k.n == 0) {
        if (k.keep) melk_remember(e, e->rsc_mel_segs, 0, 0, k.m->n_mels, k.rows_out);
        return VAD_OK;
    }
    int64_t mid = 0;
    if (mel) {
        e->rsc_mel_segs.resize((size_t)k.n);
        for (int64_t i = 0; i < k.n; ++i) {
            vadk::CutSeg &sg = e->cut_segs[(size_t)i];
            sg.quad_out = (uint64_t)mid >> 2;
            e->rsc_mel_segs[(size_t)i] = vadk::CutSeg{(uint32_t)(mid >> 2) | (vadk::SCAN_LEFT << vadk::SCAN_MODE_SHIFT), sg.nquads, 0};
            mid += (int64_t)sg.nquads << 2;
            if (mid >= (int64_t)1 << 29)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the segments have 2^29 or more samples at 16 kHz in one call", k.who);
        }
        if (int rc = mel_tiles(e, k.who, k.m, e->rsc_mel_segs, &c.mel_rows)) return rc;
        if (int rc = mel_output(e, c, dev, audio, out)) return rc;
        if (int rc = ensure(e, e->d_rsc_mid, e->d_rsc_mid_cap, (size_t)mid * sizeof(float))) return rc;
    } else {
        if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", k.who);
        if (int rc = cut_block(e, c, dev, audio, out)) return rc;
    }
    DevTables t{e->d_cut, e->d_cut_cap};
    const int segs = t.add(e->cut_segs, e->cut_segs.size()), msegs = t.add(e->rsc_mel_segs, mel ? (size_t)k.n : 0);
    const int work = t.add(e->cut_work, e->cut_work.size()), mwork = t.add(e->mel_work, mel ? e->mel_work.size() : 0);
    const int inq = t.add(e->rsc_inq, e->rsc_inq.size()), gains = t.add(e->cut_gains, k.gains ? e->cut_gains.size() : 0);
    if (int rc = t.reserve(e)) return rc;
    if (int rc = resample_cut_operator(e, k.sr_in, k.taps, k.ntaps, s)) return rc;
    if (mel)
        if (int rc = mel_operator(e, k.m, k.op_re, k.op_im, k.filters, s)) return rc;
    if (int rc = cut_upload_audio(e, c, dev, audio, s)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    const uint32_t L = vadk::rsc_L(k.sr_in), M = vadk::rsc_M(k.sr_in);
    vadk::ResampleCutArgs a{};
    a.audio = c.d_audio;
    a.out = mel ? static_cast<void *>(e->d_rsc_mid) : c.d_out;
    a.segs = t.at<const vadk::CutSeg>(segs);
    a.inq = t.at<const uint32_t>(inq);
    a.work = t.at<const vadk::CutWork>(work);
    a.gains = t.at<const float>(gains);
    a.op = e->d_rsc;
    a.audio_bytes = (uint32_t)c.ab;
    a.nwork = (uint32_t)e->cut_work.size();
    a.ksteps = vadk::rsc_K((uint32_t)k.ntaps, L, M) >> 4;
    a.n0 = vadk::rsc_n0((uint32_t)k.ntaps, L);
    a.fmt = k.fmt;
    a.channels = k.channels;
    a.out_fmt = mel ? VAD_CUT_F32 : k.out_fmt;
    a.sr_in = k.sr_in;
    const hipError_t r = vadk_launch_resample_cut(&a, s);
    int rc = r != hipSuccess ? e->hip_fail(r, "kernel launch (resample cut)") : VAD_OK;
    if (!mel) {
        rc = call_end(e, dev, s, rc);
        if (rc || dev) return rc;
        return cut_copy_back(e, c, out, s);
    }
    if (!rc)
        rc = mel_launch(e, k.m, e->d_rsc_mid, (size_t)mid * sizeof(float), VAD_FMT_F32, 1, -1.0f, static_cast<float *>(c.d_out),
                        t.at<const vadk::CutSeg>(msegs), t.at<const vadk::MelWork>(mwork), s);
    return mel_finish(e, c, dev, e->rsc_mel_segs, rc, out, s);
}


// ---- vad_mel_stats / vad_mel_batch: statistics and batches of a feature matrix
// The family's host path: melb_matrix (and melb_source behind it) for the checks of what a call reads, melb_out / melb_outs for where its
// results lie on the device, melb_upload for a host matrix once every refusal lies behind, melb_finish for the way out.  The two
// batch calls are mel_batch_body around what each supplies

// The matrix and the segments a call names: the caller's, or the resident ones of vad_scan_mel_keep.  Checks only; x is the device
// matrix where there is one already (a host matrix is uploaded by melb_upload once every refusal lies behind)
struct MelbSrc { const float *x; int64_t rows; int32_t n_mels; const int64_t *start; int64_t n; };

// The matrix half.  resident: the call names something resident (NULL features; NULL start too, where it has segments).  For
// features == NULL the resident matrix's rows and width replace the arguments; `noun` names the width in the refusal
int melb_matrix(vad_engine *e, const char *who, bool dev, bool resident, const float *features, int64_t rows, int32_t width, const char *noun,
                MelbSrc *src) {
    if (resident && e->melk_start.empty())
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: NULL names the resident matrix, and the engine holds none: no "
                       "vad_scan_mel_keep has kept one", who);
    if (!features) {
        rows = e->melk_start.back();
        width = e->melk_n_mels;
    } else if (rows < 0) {
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: rows = %lld is negative", who, (long long)rows);
    }
    if (width < 1 || width > 128) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %s = %d must be 1 .. 128", who, noun, width);
    src->x = features ? (dev ? features : nullptr) : e->d_melk;
    src->rows = rows;
    src->n_mels = width;
    return VAD_OK;
}

// ... and the segments behind it, with the device form's alignment of the features last
int melb_source(vad_engine *e, const char *who, bool dev, const float *features, int64_t rows, int32_t n_mels, const int64_t *start, int64_t n,
                MelbSrc *src) {
    if (int rc = melb_matrix(e, who, dev, !features || !start, features, rows, n_mels, "n_mels", src)) return rc;
    rows = src->rows;
    if (!start) {
        start = e->melk_start.data();
        n = (int64_t)e->melk_start.size() - 1;
    } else if (n < 0) {
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n = %lld is negative", who, (long long)n);
    }
    if (n > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 segments in one call", who);
    if (start[0] < 0 || start[n] > rows)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: start[0] = %lld .. start[n] = %lld leaves the matrix of %lld rows", who,
                       (long long)start[0], (long long)start[n], (long long)rows);
    for (int64_t i = 0; i < n; ++i) {
        if (start[i + 1] < start[i])
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld: start = %lld is followed by %lld, the first rows ascend", who,
                           (long long)i, (long long)start[i], (long long)start[i + 1]);
        if (start[i + 1] - start[i] > (int64_t)INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld has %lld rows, a segment may have less than 2^31", who,
                           (long long)i, (long long)(start[i + 1] - start[i]));
    }
    if (dev && features && (reinterpret_cast<uintptr_t>(features) & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the features must be 4-byte aligned", who);
    src->start = start;
    src->n = n;
    return VAD_OK;
}

int melb_upload(vad_engine *e, bool dev, const float *features, MelbSrc *src, hipStream_t s) {
    if (!features || dev) return VAD_OK;
    const size_t bytes = (size_t)src->rows * (size_t)src->n_mels * sizeof(float);
    if (int rc = ensure(e, e->d_melb_in, e->d_melb_in_cap, bytes)) return rc;
    if (bytes) HIP_TRY(e, hipMemcpyAsync(e->d_melb_in, features, bytes, hipMemcpyHostToDevice, s));
    src->x = e->d_melb_in;
    return VAD_OK;
}

// One output of a call: the caller's pointer (nullptr: not asked for), its bytes, and where it lies on the device
struct MelbOut { void *host; size_t bytes; void *dev; };

// The way out, first half: a device call writes where the caller says, a host call's one output is staged in e->d_melb_out ...
int melb_out(vad_engine *e, bool dev, void *host, size_t bytes, MelbOut *o) {
    o->host = o->dev = host;
    o->bytes = bytes;
    if (dev) return VAD_OK;
    if (int rc = ensure(e, e->d_melb_out, e->d_melb_out_cap, o->bytes)) return rc;
    o->dev = e->d_melb_out;
    return VAD_OK;
}

// ... and its several outputs in room-only slots there, for those the caller asked for
int melb_outs(vad_engine *e, bool dev, MelbOut *o, int count) {
    for (int i = 0; i < count; ++i) o[i].dev = o[i].host;
    if (dev) return VAD_OK;
    DevTables t{e->d_melb_out, e->d_melb_out_cap};
    int slot[DevTables::MAX];
    for (int i = 0; i < count; ++i) slot[i] = t.add(nullptr, o[i].host ? o[i].bytes : 0);
    if (int rc = t.reserve(e)) return rc;
    for (int i = 0; i < count; ++i) o[i].dev = t.at<uint8_t>(slot[i]);
    return VAD_OK;
}

// Second half, behind the launch whose status is `launched`: call_end, and for a host call the outputs in the order listed and one
// synchronise
int melb_finish(vad_engine *e, bool dev, hipStream_t s, int launched, const MelbOut *o, int count) {
    const int rc = call_end(e, dev, s, launched);
    if (rc || dev) return rc;
    for (int i = 0; i < count; ++i)
        if (o[i].host) HIP_TRY(e, hipMemcpyAsync(o[i].host, o[i].dev, o[i].bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// vad_mel_stats / _device with e->mu held
// group == nullptr: the outputs have an entry per segment (vad_mel_stats); else per group, ngroups of them (vad_mel_stats_grouped)
int mel_stats_run(vad_engine *e, bool dev, const char *who, const float *features, int64_t rows, int32_t n_mels, const int64_t *start, int64_t n,
                  const int32_t *group, int64_t ngroups, float *max_out, int64_t *sum_out, uint64_t *sumsq_out, void *stream) {
    hipStream_t s;
    if (int rc = call_begin(e, dev, stream, &s)) return rc;
    MelbSrc src{};
    if (int rc = melb_source(e, who, dev, features, rows, n_mels, start, n, &src)) return rc;
    if (group) {
        if (ngroups < 0 || ngroups > (int64_t)INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: ngroups = %lld must be 0 .. 2^31 - 1", who, (long long)ngroups);
        for (int64_t i = 0; i < src.n; ++i)
            if (group[i] < 0 || (int64_t)group[i] >= ngroups)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld names group %d of %lld", who, (long long)i, group[i],
                               (long long)ngroups);
    }
    if ((sum_out || sumsq_out) && !group)
        for (int64_t i = 0; i < src.n; ++i)
            if (src.start[i + 1] - src.start[i] > (int64_t)VAD_STATS_MAX_ROWS)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: segment %lld has %lld rows, the sums take %d at the most", who,
                               (long long)i, (long long)(src.start[i + 1] - src.start[i]), VAD_STATS_MAX_ROWS);
    if ((sum_out || sumsq_out) && group) {
        e->melb_rows.assign((size_t)ngroups, 0);
        for (int64_t i = 0; i < src.n; ++i) e->melb_rows[(size_t)group[i]] += src.start[i + 1] - src.start[i];
        for (int64_t g = 0; g < ngroups; ++g)
            if (e->melb_rows[(size_t)g] > (int64_t)VAD_STATS_MAX_ROWS)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: group %lld has %lld rows, the sums take %d at the most", who,
                               (long long)g, (long long)e->melb_rows[(size_t)g], VAD_STATS_MAX_ROWS);
    }
    if (dev && ((reinterpret_cast<uintptr_t>(max_out) & 3) || (reinterpret_cast<uintptr_t>(sum_out) & 7) || (reinterpret_cast<uintptr_t>(sumsq_out) & 7)))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the sums must be 8-byte aligned, the maxima 4-byte", who);
    const int64_t nout = group ? ngroups : src.n;
    if (nout == 0 || (!max_out && !sum_out && !sumsq_out)) return VAD_OK;
    e->melb_work.clear();
    for (int64_t i = 0; i < src.n; ++i)
        for (int64_t r = src.start[i]; r < src.start[i + 1]; r += vadk::MELB_STATS_ROWS)
            e->melb_work.push_back(vadk::MelStatsWork{(uint32_t)(group ? group[i] : i), (uint32_t)std::min<int64_t>(vadk::MELB_STATS_ROWS, src.start[i + 1] - r),
                                                      (uint64_t)r});
    if (e->melb_work.size() > (size_t)INT32_MAX)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %d rows in one call", who, vadk::MELB_STATS_ROWS);
    const size_t nn = (size_t)nout, sumb = nn * (size_t)src.n_mels * 8u, maxb = nn * sizeof(float);
    DevTables t{e->d_melb, e->d_melb_cap};
    const int work = t.add(e->melb_work, e->melb_work.size());
    if (int rc = t.reserve(e)) return rc;
    // the outputs in the order they lie in e->d_melb_out and come back: the sums, their squares, the maxima
    enum { SUM, SUMSQ, MAXIMA, OUTS };
    MelbOut o[OUTS] = {};
    o[SUM].host = sum_out;
    o[SUMSQ].host = sumsq_out;
    o[SUM].bytes = o[SUMSQ].bytes = sumb;
    o[MAXIMA].host = max_out;
    o[MAXIMA].bytes = maxb;
    if (int rc = melb_outs(e, dev, o, OUTS)) return rc;
    vadk::MelStatsArgs a{};
    a.sum_out = static_cast<long long *>(o[SUM].dev);
    a.sumsq_out = static_cast<unsigned long long *>(o[SUMSQ].dev);
    a.max_out = static_cast<float *>(o[MAXIMA].dev);
    if (int rc = melb_upload(e, dev, features, &src, s)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    // the call's own start values: -inf and zeros
    if (a.max_out) {
        e->melb_f.assign(nn, -INFINITY);
        HIP_TRY(e, hipMemcpyAsync(a.max_out, e->melb_f.data(), maxb, hipMemcpyHostToDevice, s));
    }
    if (a.sum_out) HIP_TRY(e, hipMemsetAsync(a.sum_out, 0, sumb, s));
    if (a.sumsq_out) HIP_TRY(e, hipMemsetAsync(a.sumsq_out, 0, sumb, s));
    a.x = src.x;
    a.work = t.at<const vadk::MelStatsWork>(work);
    a.nwork = (uint32_t)e->melb_work.size();
    a.n_mels = (uint32_t)src.n_mels;
    const hipError_t r = vadk_launch_mel_stats(&a, s);
    return melb_finish(e, dev, s, r != hipSuccess ? e->hip_fail(r, "kernel launch (mel stats)") : VAD_OK, o, OUTS);
}

// op [n_in][n_out] and bias [n_out] (nullptr: zeros) in fragment order in e->d_proj (vad_layout.h: proj_pack_index), the bias behind
// the operator, zeros in the padding.  Cached against the bytes of the previous call, as mel_operator is
int project_operator(vad_engine *e, int32_t n_in, int32_t n_out, const float *op, const float *bias, hipStream_t s) {
    const size_t no = (size_t)n_in * (size_t)n_out, nb = (size_t)n_out;
    const uint32_t K4 = vadk::proj_up4((uint32_t)n_in), N16 = vadk::proj_up16((uint32_t)n_out);
    bool same = e->proj_packed && e->proj_n_in == n_in && e->proj_n_out == n_out && e->proj_src.size() == no + nb &&
                !std::memcmp(e->proj_src.data(), op, no * sizeof(float));
    for (size_t c = 0; same && c < nb; ++c) {
        const float b = bias ? bias[c] : 0.0f;
        same = !std::memcmp(&e->proj_src[no + c], &b, sizeof(float));
    }
    if (same) return VAD_OK;
    e->proj_packed = false;
    const size_t pf = vadk::proj_pack_floats((uint32_t)n_in, (uint32_t)n_out);
    if (int rc = ensure(e, e->d_proj, e->d_proj_cap, pf * sizeof(float))) return rc;
    e->proj_src.assign(op, op + no);
    e->proj_src.resize(no + nb, 0.0f);
    if (bias) std::memcpy(e->proj_src.data() + no, bias, nb * sizeof(float));
    e->proj_pack.assign(pf, 0.0f);
    for (uint32_t k = 0; k < (uint32_t)n_in; ++k)
        for (uint32_t c = 0; c < (uint32_t)n_out; ++c) e->proj_pack[vadk::proj_pack_index(k, c, K4)] = op[(size_t)k * nb + c];
    for (uint32_t c = 0; c < (uint32_t)n_out; ++c) e->proj_pack[(size_t)K4 * N16 + c] = e->proj_src[no + c];
    HIP_TRY(e, hipMemcpyAsync(e->d_proj, e->proj_pack.data(), pf * sizeof(float), hipMemcpyHostToDevice, s));
    e->proj_n_in = n_in;
    e->proj_n_out = n_out;
    e->proj_packed = true;
    return VAD_OK;
}

// vad_mel_project / _device with e->mu held.  out == nullptr: the projection goes to e->d_melk_alt, which then becomes the resident
// matrix; a host call's out is staged in e->d_melb_out
int mel_project_run(vad_engine *e, bool dev, const char *who, const float *features, int64_t rows, int32_t n_in, const float *op, const float *bias,
                    int32_t n_out, float *out, void *stream) {
    hipStream_t s;
    if (int rc = call_begin(e, dev, stream, &s)) return rc;
    MelbSrc src{};
    if (int rc = melb_matrix(e, who, dev, !features, features, rows, n_in, "n_in", &src)) return rc;
    rows = src.rows;
    n_in = src.n_mels;
    if (n_out < 1 || n_out > vadk::PROJ_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n_out = %d must be 1 .. 128", who, n_out);
    if (!op) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null op", who);
    for (int32_t k = 0; k < n_in; ++k)
        for (int32_t c = 0; c < n_out; ++c)
            if (const float v = op[(size_t)k * (size_t)n_out + (size_t)c]; !std::isfinite(v))
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: op[%d][%d] is %s, an operator entry is a finite number", who, k, c,
                               std::isnan(v) ? "NaN" : "infinite");
    for (int32_t c = 0; bias && c < n_out; ++c)
        if (!std::isfinite(bias[c]))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: bias[%d] is %s, a bias is a finite number", who, c,
                           std::isnan(bias[c]) ? "NaN" : "infinite");
    if (!out && features)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out = NULL replaces the resident matrix, which features = NULL names: a "
                       "matrix of the caller's takes an out", who);
    if (dev && ((reinterpret_cast<uintptr_t>(features) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the features and the output must be 4-byte aligned", who);
    const size_t ib = (size_t)rows * (size_t)n_in * sizeof(float), ob = (size_t)rows * (size_t)n_out * sizeof(float);
    if (dev && out && rows) {
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(src.x), y0 = reinterpret_cast<uintptr_t>(out);
        if (x0 < y0 + ob && y0 < x0 + ib)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the output's %llu bytes overlap the %llu bytes of the features", who,
                           (unsigned long long)ob, (unsigned long long)ib);
    }
    if (((uint64_t)rows + vadk::PROJ_ROWS - 1) / vadk::PROJ_ROWS > (uint64_t)INT32_MAX)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %d rows in one call", who, vadk::PROJ_ROWS);
    if (rows == 0) {
        if (!out) e->melk_n_mels = n_out;
        return VAD_OK;
    }
    MelbOut o{};
    if (!out) {
        if (int rc = ensure(e, e->d_melk_alt, e->d_melk_alt_cap, ob)) return rc;
        o.dev = e->d_melk_alt;
    } else if (int rc = melb_out(e, dev, out, ob, &o)) {
        return rc;
    }
    if (int rc = project_operator(e, n_in, n_out, op, bias, s)) return rc;
    if (int rc = melb_upload(e, dev, features, &src, s)) return rc;
    vadk::ProjArgs a{};
    a.x = src.x;
    a.out = static_cast<float *>(o.dev);
    a.op = e->d_proj;
    a.rows = (uint64_t)rows;
    a.n_in = (uint32_t)n_in;
    a.n_out = (uint32_t)n_out;
    const hipError_t r = vadk_launch_mel_project(&a, s);
    const int launched = r != hipSuccess ? e->hip_fail(r, "kernel launch (mel project)") : VAD_OK;
    if (!launched && !out) {
        // the projection is the resident matrix from here on: the calls behind this one wait for the launch (call_begin)
        std::swap(e->d_melk, e->d_melk_alt);
        std::swap(e->d_melk_cap, e->d_melk_alt_cap);
        e->melk_n_mels = n_out;
    }
    return melb_finish(e, dev, s, launched, &o, 1);
}

// vad_batch's fields, ahead of everything else
int batch_check(vad_engine *e, const char *who, const vad_batch *b) {
    if (!b) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null vad_batch", who);
    if (b->n_mels < 1 || b->n_mels > 128) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n_mels = %d must be 1 .. 128", who, b->n_mels);
    if (b->frames < 4 || b->frames > 65536 || (b->frames & 3))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: frames = %d must be a multiple of 4 from 4 to 65536", who, b->frames);
    if (b->deltas < 0 || b->deltas > 2) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: deltas = %d must be 0 .. 2", who, b->deltas);
    if (b->layout != VAD_BATCH_CHANNEL_MAJOR && b->layout != VAD_BATCH_TIME_MAJOR)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: layout = %d is neither VAD_BATCH_CHANNEL_MAJOR nor VAD_BATCH_TIME_MAJOR", who, b->layout);
    if (int rc = batch_format_check(e, who, b->dtype, b->pad_mode, b->pad_value)) return rc;
    if (b->reserved != 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: vad_batch.reserved = %d must be 0", who, b->reserved);
    return VAD_OK;
}

// lo [nlo] without a NaN, shift and scale [nss][nm] finite (each may be null)
int batch_affine_check(vad_engine *e, const char *who, const float *lo, size_t nlo, const float *shift, const float *scale, size_t nss, size_t nm) {
    for (size_t i = 0; lo && i < nlo; ++i)
        if (std::isnan(lo[i])) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: lo[%lld] is NaN", who, (long long)i);
    for (int which = 0; which < 2; ++which) {
        const float *v = which ? scale : shift;
        for (size_t k = 0; v && k < nss * nm; ++k)
            if (!std::isfinite(v[k]))
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %s[%lld][%lld] is %s, a %s is a finite number", who, which ? "scale" : "shift",
                               (long long)(k / nm), (long long)(k % nm), std::isnan(v[k]) ? "NaN" : "infinite", which ? "scale" : "shift");
    }
    return VAD_OK;
}

// What a kind of batch is to mel_batch_body besides its three callables
struct BatchKind {
    bool bad_count;       // its part of the count check: a count or a buffer of its own is wrong
    bool per_window;      // lo, shift and scale go by window - lo [nw], nss is 1 or nw - else by segment: lo [n], nss is 1 or n
    const char *what;     // its launch, named for a failed one
};

// What the two batch calls share, around a kind and its three callables: check(src, tile, &groups) refuses its windows or pieces in
// its order and counts the workgroups; table(src, tile, groups, t), behind every refusal, adds its table to e->d_melb;
// launch(a, t, its table, s).  In e->d_melb: the kind's table, then lo [n or nw], shift and scale [nss][n_mels]
template <class Check, class Table, class Launch>
int mel_batch_body(vad_engine *e, bool dev, const char *who, const float *features, int64_t rows, const int64_t *start, int64_t n, const vad_batch *b,
                   int64_t nw, const float *lo, const float *shift, const float *scale, int64_t nss, void *out, int64_t out_bytes, void *stream,
                   const BatchKind &kind, Check check, Table table, Launch launch) {
    hipStream_t s;
    if (int rc = call_begin(e, dev, stream, &s)) return rc;
    if (int rc = batch_check(e, who, b)) return rc;
    MelbSrc src{};
    if (int rc = melb_source(e, who, dev, features, rows, b->n_mels, start, n, &src)) return rc;
    if (src.n_mels != b->n_mels)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n_mels = %d, the resident matrix has %d", who, b->n_mels, src.n_mels);
    if (nw < 0 || out_bytes < 0 || kind.bad_count) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer or bad count", who);
    const int64_t over = kind.per_window ? nw : src.n;
    if (int rc = batch_nss(e, who, shift, scale, &nss, "row", kind.per_window ? "nw" : "n", over)) return rc;
    const size_t nm = (size_t)b->n_mels;
    if (int rc = batch_affine_check(e, who, lo, (size_t)over, shift, scale, (size_t)nss, nm)) return rc;
    const uint32_t tile = vadk::melb_tile((uint32_t)b->n_mels, (uint32_t)b->deltas);
    uint64_t groups = 0;
    if (int rc = check(src, tile, &groups)) return rc;
    const size_t C = nm * (size_t)(b->deltas + 1), need = (size_t)nw * C * (size_t)b->frames * (b->dtype == VAD_BATCH_F32 ? 4u : 2u);
    if (need > (size_t)out_bytes)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_bytes = %lld, the windows have %llu bytes", who, (long long)out_bytes,
                       (unsigned long long)need);
    if (nw > (int64_t)INT32_MAX || groups > (uint64_t)INT32_MAX)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 workgroups of %u frames in one call", who, tile);
    if (nw == 0) return VAD_OK;
    if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (dev && (reinterpret_cast<uintptr_t>(out) & 15))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the output must be 16-byte aligned", who);
    DevTables t{e->d_melb, e->d_melb_cap};
    const int mine = table(src, tile, groups, t);
    // lo, shift and scale go up as one table of floats, in this order
    const size_t nlo = std::max<size_t>((size_t)over, 1), nsc = (size_t)nss * nm;
    e->melb_f.assign(nlo + 2 * nsc, 0.0f);
    const int floats = t.add(e->melb_f, e->melb_f.size());
    if (int rc = t.reserve(e)) return rc;
    MelbOut o{};
    if (int rc = melb_out(e, dev, out, need, &o)) return rc;
    if (int rc = melb_upload(e, dev, features, &src, s)) return rc;
    float *hl = e->melb_f.data();
    for (size_t i = 0; i < (size_t)over; ++i) hl[i] = lo ? lo[i] : -INFINITY;
    affine_fill(hl + nlo, hl + nlo + nsc, shift, scale, nsc);
    if (int rc = t.copy(e, s)) return rc;
    vadk::MelBatchArgs a{};
    a.x = src.x;
    a.out = o.dev;
    a.lo = t.at<const float>(floats);
    a.shift = a.lo + nlo;
    a.scale = a.shift + nsc;
    a.nw = (uint32_t)nw;
    a.n_mels = (uint32_t)b->n_mels;
    a.frames = (uint32_t)b->frames;
    a.deltas = (uint32_t)b->deltas;
    a.layout = b->layout;
    a.dtype = b->dtype;
    a.pad_mode = b->pad_mode;
    a.pad_value = b->pad_value;
    a.per_seg = nss == 1 ? 0u : 1u;
    a.tile = tile;
    const hipError_t r = launch(a, t, mine, s);
    return melb_finish(e, dev, s, r != hipSuccess ? e->hip_fail(r, kind.what) : VAD_OK, &o, 1);
}

// vad_mel_batch / _device with e->mu held: a window is rows of one segment, under the segment's lo, shift and scale.  Its table:
// MelBatchWin [nw]
int mel_batch_run(vad_engine *e, bool dev, const char *who, const float *features, int64_t rows, const int64_t *start, int64_t n, const vad_batch *b,
                  const vad_batch_window *windows, int64_t nw, const float *lo, const float *shift, const float *scale, int64_t nss, void *out,
                  int64_t out_bytes, void *stream) {
    auto check = [&](const MelbSrc &src, uint32_t tile, uint64_t *groups) -> int {
        e->melb_win.resize((size_t)nw);
        for (int64_t k = 0; k < nw; ++k) {
            const vad_batch_window &w = windows[k];
            if (w.seg < 0 || (int64_t)w.seg >= src.n)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: window %lld names segment %d of %lld", who, (long long)k, w.seg, (long long)src.n);
            const int64_t M = src.start[w.seg + 1] - src.start[w.seg];
            if (w.row0 < 0 || w.nrows < 0 || w.nrows > b->frames || w.row0 > M || w.nrows > M - w.row0)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: window %lld: rows %lld .. +%d of segment %d, which has %lld, in %d frames", who,
                               (long long)k, (long long)w.row0, w.nrows, w.seg, (long long)M, b->frames);
            e->melb_win[(size_t)k] = vadk::MelBatchWin{(uint64_t)src.start[w.seg], (uint32_t)M, (uint32_t)w.row0, (uint32_t)w.nrows, (uint32_t)w.seg};
        }
        *groups = (uint64_t)nw * (((uint32_t)b->frames + tile - 1u) / tile);
        return VAD_OK;
    };
    auto table = [&](const MelbSrc &, uint32_t, uint64_t, DevTables &t) { return t.add(e->melb_win, (size_t)nw); };
    auto launch = [&](vadk::MelBatchArgs &a, const DevTables &t, int win, hipStream_t s) {
        a.win = t.at<const vadk::MelBatchWin>(win);
        return vadk_launch_mel_batch(&a, s);
    };
    BatchKind kind{};
    kind.bad_count = nw > 0 && !windows;
    kind.per_window = false;
    kind.what = "kernel launch (mel batch)";
    return mel_batch_body(e, dev, who, features, rows, start, n, b, nw, lo, shift, scale, nss, out, out_bytes, stream, kind, check, table, launch);
}

// vad_mel_batch_packed / _device with e->mu held: pieces of segments side by side in a window, under the window's lo, shift and scale.
// Its table: the work list, a MelPackWork per workgroup
int mel_batch_packed_run(vad_engine *e, bool dev, const char *who, const float *features, int64_t rows, const int64_t *start, int64_t n,
                         const vad_batch *b, const vad_batch_piece *pieces, int64_t np, int64_t nw, const float *lo, const float *shift,
                         const float *scale, int64_t nss, void *out, int64_t out_bytes, void *stream) {
    auto check = [&](const MelbSrc &src, uint32_t tile, uint64_t *groups) -> int {
        const int64_t T = b->frames;
        for (int64_t k = 0; k < np; ++k) {
            const vad_batch_piece &p = pieces[k];
            if (p.seg < 0 || (int64_t)p.seg >= src.n)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: piece %lld names segment %d of %lld", who, (long long)k, p.seg, (long long)src.n);
            const int64_t M = src.start[p.seg + 1] - src.start[p.seg];
            if (p.row0 < 0 || p.nrows < 1 || p.row0 > M || p.nrows > M - p.row0)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: piece %lld: rows %lld .. +%d of segment %d, which has %lld", who, (long long)k,
                               (long long)p.row0, p.nrows, p.seg, (long long)M);
            if (p.window < 0 || (int64_t)p.window >= nw)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: piece %lld names window %d of %lld", who, (long long)k, p.window, (long long)nw);
            if (p.offset < 0 || (p.offset & 3) || (int64_t)p.offset + p.nrows > T)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: piece %lld: offset = %d with %d rows: a multiple of 4 from 0, offset + nrows <= %d "
                               "frames", who, (long long)k, p.offset, p.nrows, b->frames);
        }
        // the pieces by (window, offset); a piece owns [offset, up4(offset + nrows)) of its window
        auto groups_of = [tile](int64_t frames) -> int64_t { return (frames + tile - 1) / tile; };
        e->melb_order.resize((size_t)np);
        for (int64_t k = 0; k < np; ++k) e->melb_order[(size_t)k] = k;
        std::sort(e->melb_order.begin(), e->melb_order.end(), [pieces](int64_t x, int64_t y) {
            const vad_batch_piece &p = pieces[x], &q = pieces[y];
            return p.window != q.window ? p.window < q.window : p.offset != q.offset ? p.offset < q.offset : x < y;
        });
        int64_t nwork = 0, with_pieces = 0;           // workgroups of the windows that have a piece, and those windows
        for (int64_t k = 0, used = 0; k < np; ++k) {
            const int64_t pk = e->melb_order[(size_t)k];
            const vad_batch_piece &p = pieces[pk];
            const bool first = k == 0 || pieces[e->melb_order[(size_t)k - 1]].window != p.window;
            if (first) {
                if (k) nwork += groups_of(T - used);
                used = 0;
                ++with_pieces;
            } else if (p.offset < used) {
                const int64_t qk = e->melb_order[(size_t)k - 1];
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: pieces %lld and %lld overlap in window %d: frames %d .. %lld and %d .. %lld",
                               who, (long long)std::min(pk, qk), (long long)std::max(pk, qk), p.window, pieces[qk].offset, (long long)used - 1, p.offset,
                               (long long)(((int64_t)p.offset + p.nrows + 3) & ~(int64_t)3) - 1);
            }
            nwork += groups_of(p.offset - used) + groups_of(p.nrows);
            used = ((int64_t)p.offset + p.nrows + 3) & ~(int64_t)3;
            if (k == np - 1) nwork += groups_of(T - used);
        }
        *groups = (uint64_t)nwork + (uint64_t)(nw - with_pieces) * (uint64_t)groups_of(T);
        return VAD_OK;
    };
    // the work list, window by window: pad runs before, between and behind the pieces, each piece tile by tile
    auto table = [&](const MelbSrc &src, uint32_t tile, uint64_t groups, DevTables &t) {
        const int64_t T = b->frames;
        e->melb_pack.clear();
        e->melb_pack.reserve((size_t)groups);
        auto pad_run = [&](int64_t w, int64_t from, int64_t to) {
            for (int64_t f = from; f < to; f += tile)
                e->melb_pack.push_back(vadk::MelPackWork{0u, 0u, 0u, (uint32_t)w, (uint32_t)f, (uint32_t)std::min<int64_t>(tile, to - f), 0u});
        };
        int64_t k = 0;
        for (int64_t w = 0; w < nw; ++w) {
            int64_t used = 0;
            for (; k < np && pieces[e->melb_order[(size_t)k]].window == w; ++k) {
                const vad_batch_piece &p = pieces[e->melb_order[(size_t)k]];
                pad_run(w, used, p.offset);
                const int64_t M = src.start[p.seg + 1] - src.start[p.seg];
                for (int64_t r = 0; r < p.nrows; r += tile) {
                    const int64_t nv = std::min<int64_t>(tile, p.nrows - r);
                    e->melb_pack.push_back(vadk::MelPackWork{(uint64_t)src.start[p.seg], (uint32_t)M, (uint32_t)(p.row0 + r), (uint32_t)w,
                                                             (uint32_t)(p.offset + r), (uint32_t)((nv + 3) & ~(int64_t)3), (uint32_t)nv});
                }
                used = ((int64_t)p.offset + p.nrows + 3) & ~(int64_t)3;
            }
            pad_run(w, used, T);
        }
        return t.add(e->melb_pack, e->melb_pack.size());
    };
    auto launch = [&](const vadk::MelBatchArgs &args, const DevTables &t, int work, hipStream_t s) {
        vadk::MelPackArgs a{};
        a.b = args;
        a.work = t.at<const vadk::MelPackWork>(work);
        a.nwork = (uint32_t)e->melb_pack.size();
        return vadk_launch_mel_batch_packed(&a, s);
    };
    BatchKind kind{};
    kind.bad_count = np < 0 || (np > 0 && !pieces);
    kind.per_window = true;
    kind.what = "kernel launch (mel batch packed)";
    return mel_batch_body(e, dev, who, features, rows, start, n, b, nw, lo, shift, scale, nss, out, out_bytes, stream, kind, check, table, launch);
}

// ---- the entry points of the family: each host / _device pair fills the record in one function that takes `dev`

// what an entry point's sr_in may be: the call has none (a block at the engine's rate); an input rate (16000: the call is
// vad_scan_cut); or, in the calls that take both kinds of block, 0 or the engine's own rate too
enum class RateArg { NONE, GIVEN, EITHER };

// Around every record: the lock, the rate - ahead of the way in; the resampling kinds check theirs with the taps, behind it - the
// way in, and the kind's runner on the call's stream
int cut_enter(vad_engine *e, bool dev, CutCall &k, RateArg arg, int32_t sr_in, const void *audio, void *out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (arg == RateArg::GIVEN || (arg == RateArg::EITHER && sr_in != 0 && sr_in != e->sample_rate)) {
        if (int rc = rate_cut_check(e, k.who, sr_in, &k.chunk)) return rc;
        k.sr_in = k.chunk ? sr_in : 0;
    }
    hipStream_t s;
    if (int rc = call_begin(e, dev, stream, &s)) return rc;
    switch (k.kind) {
        case CutKind::RENDER: return render_run(e, dev, k, audio, out, s);
        case CutKind::MEL: return mel_run(e, dev, k, audio, out, s);
        case CutKind::AUDIO_BATCH: return audio_batch_run(e, dev, k, audio, out, s);
        case CutKind::RESAMPLE:
        case CutKind::RESAMPLE_MEL: return resample_cut_run(e, dev, k, audio, out, s);
        default: return cut_run(e, dev, k, audio, out, s);
    }
}

// The four PAYLOAD calls: vad_scan_cut has no sr_in and vad_scan_rate_cut no other; only these two have no gains.  vad_scan_cut_gain's
// `gains` is the host array [n], never nullptr; vad_scan_cut_stereo's may be
enum class Cut { PLAIN, RATE, GAIN, STEREO };
int payload_entry(vad_engine *e, bool dev, const char *who, Cut call, const vad_cut_item *items, int64_t n, const float *gains, const void *audio,
                  int64_t audio_samples, int32_t channels, int fmt, int32_t sr_in, int32_t hop, float thr, int32_t layout, int32_t out_fmt, void *out,
                  int64_t out_samples, void *stream) {
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, thr);
    k.layout = layout;
    k.out_fmt = out_fmt;
    k.out_samples = out_samples;
    k.gains = gains;
    k.gains_required = call == Cut::GAIN;
    k.stereo = call == Cut::STEREO;
    return cut_enter(e, dev, k, call == Cut::PLAIN ? RateArg::NONE : call == Cut::RATE ? RateArg::GIVEN : RateArg::EITHER, sr_in, audio, out, stream);
}

// vad_scan_levels: `out` is n vad_level records
int levels_entry(vad_engine *e, bool dev, const char *who, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples,
                 int32_t channels, int fmt, int32_t sr_in, int32_t hop, float thr, float clip, void *out, void *stream) {
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, thr);
    k.kind = CutKind::LEVELS;
    k.clip = clip;
    return cut_enter(e, dev, k, RateArg::EITHER, sr_in, audio, out, stream);
}

// vad_scan_moments: `out` is n vad_moments records
int moments_entry(vad_engine *e, bool dev, const char *who, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples,
                  int32_t channels, int fmt, int32_t sr_in, int32_t hop, float thr, void *out, void *stream) {
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, thr);
    k.kind = CutKind::MOMENTS;
    return cut_enter(e, dev, k, RateArg::EITHER, sr_in, audio, out, stream);
}

// vad_scan_audio_batch: windows, shift and scale are host arrays in both forms
int audio_batch_entry(vad_engine *e, bool dev, const char *who, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples,
                      int32_t channels, int fmt, int32_t sr_in, int32_t hop, float thr, const vad_audio_batch *b, const vad_audio_window *windows,
                      int64_t nw, const float *shift, const float *scale, int64_t nss, void *out, int64_t out_bytes, uint8_t *mask, void *stream) {
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, thr);
    k.kind = CutKind::AUDIO_BATCH;
    k.ab = b;
    k.awin = windows;
    k.nw = nw;
    k.shift = shift;
    k.scale = scale;
    k.nss = nss;
    k.out_bytes = out_bytes;
    k.mask = mask;
    return cut_enter(e, dev, k, RateArg::EITHER, sr_in, audio, out, stream);
}

// vad_scan_render and vad_scan_render_stereo (stereo)
int render_entry(vad_engine *e, bool dev, const char *who, bool stereo, const vad_cut_item *items, int64_t n, const float *gains, const float *ramp,
                 int32_t nramp, const void *audio, int64_t audio_samples, int32_t channels, int fmt, int32_t sr_in, int32_t hop, float thr,
                 int32_t out_fmt, void *out, int64_t out_samples, void *stream) {
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, thr);
    k.kind = CutKind::RENDER;
    k.out_fmt = out_fmt;
    k.out_samples = out_samples;
    k.gains = gains;
    k.ramp = ramp;
    k.nramp = nramp;
    k.stereo = stereo;
    return cut_enter(e, dev, k, RateArg::EITHER, sr_in, audio, out, stream);
}

// The mel calls.  vad_scan_mel: MEL, without taps and sr_in.  vad_scan_rate_mel: RESAMPLE_MEL.  vad_scan_mel_keep (keep: no `out`,
// no out_rows) is the plain call or the rate call under its own name, by sr_in: 0 or the engine's rate, which never changes, is MEL
int mel_entry(vad_engine *e, bool dev, const char *who, CutKind kind, bool keep, const vad_cut_item *items, int64_t n, const vad_mel *m,
              const float *op_re, const float *op_im, const float *filters, const float *taps, int32_t ntaps, const void *audio, int64_t audio_samples,
              int32_t channels, int fmt, int32_t sr_in, int32_t hop, float thr, void *out, int64_t out_rows, int64_t *rows_out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, thr);
    k.kind = keep && (sr_in == 0 || sr_in == e->sample_rate) ? CutKind::MEL : kind;
    k.sr_in = k.kind == CutKind::MEL ? 0 : sr_in;
    k.taps = taps;
    k.ntaps = ntaps;
    k.m = m;
    k.op_re = op_re;
    k.op_im = op_im;
    k.filters = filters;
    k.out_rows = out_rows;
    k.keep = keep;
    k.rows_out = rows_out;
    return cut_enter(e, dev, k, RateArg::NONE, 0, audio, out, stream);
}

// vad_scan_resample_cut.  A resampled sample was never gated
int resample_entry(vad_engine *e, bool dev, const char *who, const vad_cut_item *items, int64_t n, const float *gains, const float *taps, int32_t ntaps,
                   const void *audio, int64_t audio_samples, int32_t channels, int fmt, int32_t sr_in, int32_t hop, int32_t out_fmt, void *out,
                   int64_t out_samples, void *stream) {
    CutCall k = cut_call(who, items, n, audio_samples, channels, fmt, hop, -1.0f);
    k.kind = CutKind::RESAMPLE;
    k.sr_in = sr_in;
    k.out_fmt = out_fmt;
    k.out_samples = out_samples;
    k.gains = gains;
    k.taps = taps;
    k.ntaps = ntaps;
    return cut_enter(e, dev, k, RateArg::NONE, 0, audio, out, stream);
}

}  // namespace

extern "C" {

int vad_scan_mel_keep(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re, const float *op_im,
                      const float *filters, const float *taps, int32_t ntaps, const void *audio, int64_t audio_samples, int32_t channels,
                      int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int64_t *rows_out) {
    return mel_entry(e, false, "vad_scan_mel_keep", CutKind::RESAMPLE_MEL, true, items, n, m, op_re, op_im, filters, taps, ntaps, audio, audio_samples, channels, frame_fmt,
                     sr_in, hop, denoise_thresh, nullptr, 0, rows_out, nullptr);
}

int vad_scan_mel_keep_device(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re, const float *op_im,
                             const float *filters, const float *taps, int32_t ntaps, const void *d_audio, int64_t audio_samples,
                             int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int64_t *rows_out, void *stream) {
    return mel_entry(e, true, "vad_scan_mel_keep_device", CutKind::RESAMPLE_MEL, true, items, n, m, op_re, op_im, filters, taps, ntaps, d_audio, audio_samples, channels,
                     frame_fmt, sr_in, hop, denoise_thresh, nullptr, 0, rows_out, stream);
}

int vad_mel_resident(vad_engine *e, int64_t *rows, int32_t *n_mels, int64_t *nsegs) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->melk_start.empty())
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: vad_mel_resident: the engine holds no resident matrix: no vad_scan_mel_keep has kept one");
    if (rows) *rows = e->melk_start.back();
    if (n_mels) *n_mels = e->melk_n_mels;
    if (nsegs) *nsegs = (int64_t)e->melk_start.size() - 1;
    return VAD_OK;
}

int vad_mel_resident_read(vad_engine *e, int64_t first_row, int64_t count, float *out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    const char *who = "vad_mel_resident_read";
    if (e->melk_start.empty())
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the engine holds no resident matrix: no vad_scan_mel_keep has kept one", who);
    const int64_t rows = e->melk_start.back();
    if (first_row < 0 || count < 0 || first_row > rows || count > rows - first_row)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: rows %lld .. +%lld of a matrix of %lld", who, (long long)first_row,
                       (long long)count, (long long)rows);
    if (count == 0) return VAD_OK;
    if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    HIP_TRY(e, hipSetDevice(e->device));
    if (int rc = scan_wait(e)) return rc;
    const size_t nm = (size_t)e->melk_n_mels;
    HIP_TRY(e, hipMemcpyAsync(out, e->d_melk + (size_t)first_row * nm, (size_t)count * nm * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

int vad_mel_stats(vad_engine *e, const float *features, int64_t rows, int32_t n_mels, const int64_t *start, int64_t n, float *max_out,
                  int64_t *sum_out, uint64_t *sumsq_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_stats_run(e, false, "vad_mel_stats", features, rows, n_mels, start, n, nullptr, 0, max_out, sum_out, sumsq_out, nullptr);
}

int vad_mel_stats_device(vad_engine *e, const float *d_features, int64_t rows, int32_t n_mels, const int64_t *start, int64_t n, float *d_max_out,
                         int64_t *d_sum_out, uint64_t *d_sumsq_out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_stats_run(e, true, "vad_mel_stats_device", d_features, rows, n_mels, start, n, nullptr, 0, d_max_out, d_sum_out, d_sumsq_out, stream);
}

int vad_mel_batch(vad_engine *e, const float *features, int64_t rows, const int64_t *start, int64_t n, const vad_batch *b,
                  const vad_batch_window *windows, int64_t nw, const float *lo, const float *shift, const float *scale, int64_t nss, void *out,
                  int64_t out_bytes) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_batch_run(e, false, "vad_mel_batch", features, rows, start, n, b, windows, nw, lo, shift, scale, nss, out, out_bytes, nullptr);
}

int vad_mel_batch_device(vad_engine *e, const float *d_features, int64_t rows, const int64_t *start, int64_t n, const vad_batch *b,
                         const vad_batch_window *windows, int64_t nw, const float *lo, const float *shift, const float *scale, int64_t nss,
                         void *d_out, int64_t out_bytes, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_batch_run(e, true, "vad_mel_batch_device", d_features, rows, start, n, b, windows, nw, lo, shift, scale, nss, d_out, out_bytes, stream);
}

int vad_mel_stats_grouped(vad_engine *e, const float *features, int64_t rows, int32_t n_mels, const int64_t *start, int64_t n, const int32_t *group,
                          int64_t ngroups, float *max_out, int64_t *sum_out, uint64_t *sumsq_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_stats_run(e, false, "vad_mel_stats_grouped", features, rows, n_mels, start, n, group, ngroups, max_out, sum_out, sumsq_out, nullptr);
}

int vad_mel_stats_grouped_device(vad_engine *e, const float *d_features, int64_t rows, int32_t n_mels, const int64_t *start, int64_t n,
                                 const int32_t *group, int64_t ngroups, float *d_max_out, int64_t *d_sum_out, uint64_t *d_sumsq_out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_stats_run(e, true, "vad_mel_stats_grouped_device", d_features, rows, n_mels, start, n, group, ngroups, d_max_out, d_sum_out, d_sumsq_out,
                         stream);
}

int vad_mel_batch_packed(vad_engine *e, const float *features, int64_t rows, const int64_t *start, int64_t n, const vad_batch *b,
                         const vad_batch_piece *pieces, int64_t np, int64_t nw, const float *lo, const float *shift, const float *scale, int64_t nss,
                         void *out, int64_t out_bytes) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_batch_packed_run(e, false, "vad_mel_batch_packed", features, rows, start, n, b, pieces, np, nw, lo, shift, scale, nss, out, out_bytes,
                                nullptr);
}

int vad_mel_batch_packed_device(vad_engine *e, const float *d_features, int64_t rows, const int64_t *start, int64_t n, const vad_batch *b,
                                const vad_batch_piece *pieces, int64_t np, int64_t nw, const float *lo, const float *shift, const float *scale,
                                int64_t nss, void *d_out, int64_t out_bytes, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_batch_packed_run(e, true, "vad_mel_batch_packed_device", d_features, rows, start, n, b, pieces, np, nw, lo, shift, scale, nss, d_out,
                                out_bytes, stream);
}

int vad_mel_project(vad_engine *e, const float *features, int64_t rows, int32_t n_in, const float *op, const float *bias, int32_t n_out,
                    float *out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_project_run(e, false, "vad_mel_project", features, rows, n_in, op, bias, n_out, out, nullptr);
}

int vad_mel_project_device(vad_engine *e, const float *d_features, int64_t rows, int32_t n_in, const float *op, const float *bias, int32_t n_out,
                           float *d_out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return mel_project_run(e, true, "vad_mel_project_device", d_features, rows, n_in, op, bias, n_out, d_out, stream);
}

// the packing rule of include/vad_engine.h: host code only, no engine.  Twice over the segments: the counts, then the pieces
int vad_mel_pack_plan(const int64_t *start, int64_t n, const int32_t *group, int32_t frames, int32_t gap, vad_batch_piece *pieces_out, int64_t cap,
                      int64_t *npieces, int64_t *nwindows) {
    if (!start || n < 0 || n > (int64_t)INT32_MAX || frames < 4 || frames > 65536 || (frames & 3) || gap < 0 || gap > frames) return VAD_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (start[i + 1] < start[i]) return VAD_ERR_INVALID_ARG;
    const int64_t T = frames;
    int64_t np = 0, nw = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int64_t used = 0;
        int32_t cur = 0;
        np = nw = 0;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t M = start[i + 1] - start[i];
            const int32_t g = group ? group[i] : 0;
            for (int64_t r = 0; r < M; r += T) {
                const int64_t k = std::min(T, M - r);
                int64_t offset = (used + gap + 3) & ~(int64_t)3;
                if (nw == 0 || g != cur || offset + k > T) {
                    ++nw;
                    cur = g;
                    offset = 0;
                }
                if (pass) pieces_out[np] = vad_batch_piece{(int32_t)i, (int32_t)k, r, (int32_t)(nw - 1), (int32_t)offset};
                ++np;
                used = offset + k;
            }
        }
        if (pass == 0) {
            if (nw > (int64_t)INT32_MAX) return VAD_ERR_INVALID_ARG;
            if (npieces) *npieces = np;
            if (nwindows) *nwindows = nw;
            if (!pieces_out) return VAD_OK;
            if (cap < np) return VAD_ERR_INVALID_ARG;
        }
    }
    return VAD_OK;
}

int64_t vad_resample_cut_samples(const vad_engine *e, int64_t nframes, int32_t sr_in, int32_t hop) {
    if (sr_in == 16000) return -1;
    const int64_t s_in = vad_rate_cut_samples(e, nframes, sr_in, hop, VAD_CUT_RANGE);
    if (s_in < 0) return -1;
    return (s_in * vadk::rsc_L(sr_in) / vadk::rsc_M(sr_in)) & ~(int64_t)3;
}

int vad_scan_resample_cut(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const float *taps, int32_t ntaps, const void *audio,
                          int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, int32_t out_fmt, void *out,
                          int64_t out_samples) {
    return resample_entry(e, false, "vad_scan_resample_cut", items, n, gains, taps, ntaps, audio, audio_samples, channels, frame_fmt, sr_in, hop,
                          out_fmt, out, out_samples, nullptr);
}

int vad_scan_resample_cut_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const float *taps, int32_t ntaps,
                                 const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                                 int32_t out_fmt, void *d_out, int64_t out_samples, void *stream) {
    return resample_entry(e, true, "vad_scan_resample_cut_device", items, n, gains, taps, ntaps, d_audio, audio_samples, channels, frame_fmt, sr_in,
                          hop, out_fmt, d_out, out_samples, stream);
}

int vad_scan_rate_mel(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re, const float *op_im,
                      const float *filters, const float *taps, int32_t ntaps, const void *audio, int64_t audio_samples, int32_t channels,
                      int frame_fmt, int32_t sr_in, int32_t hop, float *out, int64_t out_rows) {
    return mel_entry(e, false, "vad_scan_rate_mel", CutKind::RESAMPLE_MEL, false, items, n, m, op_re, op_im, filters, taps, ntaps, audio,
                     audio_samples, channels, frame_fmt, sr_in, hop, -1.0f, out, out_rows, nullptr, nullptr);
}

int vad_scan_rate_mel_device(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re, const float *op_im,
                             const float *filters, const float *taps, int32_t ntaps, const void *d_audio, int64_t audio_samples,
                             int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float *d_out, int64_t out_rows, void *stream) {
    return mel_entry(e, true, "vad_scan_rate_mel_device", CutKind::RESAMPLE_MEL, false, items, n, m, op_re, op_im, filters, taps, ntaps, d_audio,
                     audio_samples, channels, frame_fmt, sr_in, hop, -1.0f, d_out, out_rows, nullptr, stream);
}

int64_t vad_mel_frames(const vad_mel *m, int64_t nsamples) {
    if (!m || mel_bad_field(m) || nsamples < 0 || nsamples > (INT64_MAX >> 1)) return -1;
    if (m->pad == VAD_MEL_PAD_REFLECT && nsamples <= m->n_fft / 2) return -1;
    return mel_frames(m, nsamples);
}

int vad_scan_mel(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re, const float *op_im, const float *filters,
                 const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh, float *out,
                 int64_t out_rows) {
    return mel_entry(e, false, "vad_scan_mel", CutKind::MEL, false, items, n, m, op_re, op_im, filters, nullptr, 0, audio, audio_samples, channels, frame_fmt, 0,
                     hop, denoise_thresh, out, out_rows, nullptr, nullptr);
}

int vad_scan_mel_device(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re, const float *op_im,
                        const float *filters, const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t hop,
                        float denoise_thresh, float *d_out, int64_t out_rows, void *stream) {
    return mel_entry(e, true, "vad_scan_mel_device", CutKind::MEL, false, items, n, m, op_re, op_im, filters, nullptr, 0, d_audio, audio_samples, channels,
                     frame_fmt, 0, hop, denoise_thresh, d_out, out_rows, nullptr, stream);
}

int64_t vad_cut_samples(const vad_engine *e, int64_t nframes, int32_t hop, int32_t layout) {
    if (!e || nframes < 1 || hop < 4 || (hop & 3) || (layout != VAD_CUT_FRAMES && layout != VAD_CUT_RANGE)) return -1;
    if (nframes > (INT64_MAX >> 1) / std::max<int64_t>(hop, e->frame_samples)) return -1;
    return cut_samples(e->frame_samples, nframes, hop, layout, e->frame_samples);
}

int64_t vad_rate_cut_samples(const vad_engine *e, int64_t nframes, int32_t sr_in, int32_t hop, int32_t layout) {
    if (sr_in == 16000) return vad_cut_samples(e, nframes, hop, layout);
    const int chunk = resample_chunk_len(sr_in);
    if (!e || chunk == 0 || nframes < 1 || hop < 4 || (hop & 3) || (layout != VAD_CUT_FRAMES && layout != VAD_CUT_RANGE)) return -1;
    if (nframes > (INT64_MAX >> 1) / std::max<int64_t>(hop, chunk)) return -1;
    return cut_samples(chunk, nframes, hop, layout, VAD_FRAME_SAMPLES);
}

int vad_scan_cut(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                 int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *out, int64_t out_samples) {
    return payload_entry(e, false, "vad_scan_cut", Cut::PLAIN, items, n, nullptr, audio, audio_samples, channels, frame_fmt, 0, hop, denoise_thresh,
                         layout, out_fmt, out, out_samples, nullptr);
}

int vad_scan_cut_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                        int frame_fmt, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *d_out, int64_t out_samples,
                        void *stream) {
    return payload_entry(e, true, "vad_scan_cut_device", Cut::PLAIN, items, n, nullptr, d_audio, audio_samples, channels, frame_fmt, 0, hop,
                         denoise_thresh, layout, out_fmt, d_out, out_samples, stream);
}

int vad_scan_rate_cut(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                      int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *out, int64_t out_samples) {
    return payload_entry(e, false, "vad_scan_rate_cut", Cut::RATE, items, n, nullptr, audio, audio_samples, channels, frame_fmt, sr_in, hop,
                         denoise_thresh, layout, out_fmt, out, out_samples, nullptr);
}

int vad_scan_rate_cut_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                             int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *d_out,
                             int64_t out_samples, void *stream) {
    return payload_entry(e, true, "vad_scan_rate_cut_device", Cut::RATE, items, n, nullptr, d_audio, audio_samples, channels, frame_fmt, sr_in, hop,
                         denoise_thresh, layout, out_fmt, d_out, out_samples, stream);
}

int vad_scan_levels(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                    int32_t sr_in, int32_t hop, float denoise_thresh, float clip_thresh, vad_level *levels_out) {
    return levels_entry(e, false, "vad_scan_levels", items, n, audio, audio_samples, channels, frame_fmt, sr_in, hop, denoise_thresh, clip_thresh,
                        levels_out, nullptr);
}

int vad_scan_levels_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                           int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, float clip_thresh, vad_level *d_levels, void *stream) {
    return levels_entry(e, true, "vad_scan_levels_device", items, n, d_audio, audio_samples, channels, frame_fmt, sr_in, hop, denoise_thresh,
                        clip_thresh, d_levels, stream);
}

int vad_scan_cut_gain(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const void *audio, int64_t audio_samples,
                      int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *out,
                      int64_t out_samples) {
    return payload_entry(e, false, "vad_scan_cut_gain", Cut::GAIN, items, n, gains, audio, audio_samples, channels, frame_fmt, sr_in, hop,
                         denoise_thresh, layout, out_fmt, out, out_samples, nullptr);
}

int vad_scan_cut_gain_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const void *d_audio, int64_t audio_samples,
                             int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt,
                             void *d_out, int64_t out_samples, void *stream) {
    return payload_entry(e, true, "vad_scan_cut_gain_device", Cut::GAIN, items, n, gains, d_audio, audio_samples, channels, frame_fmt, sr_in, hop,
                         denoise_thresh, layout, out_fmt, d_out, out_samples, stream);
}

int vad_scan_moments(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                     int32_t sr_in, int32_t hop, float denoise_thresh, vad_moments *out) {
    return moments_entry(e, false, "vad_scan_moments", items, n, audio, audio_samples, channels, frame_fmt, sr_in, hop, denoise_thresh, out, nullptr);
}

int vad_scan_moments_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                            int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, vad_moments *d_out, void *stream) {
    return moments_entry(e, true, "vad_scan_moments_device", items, n, d_audio, audio_samples, channels, frame_fmt, sr_in, hop, denoise_thresh,
                         d_out, stream);
}

int vad_scan_audio_batch(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                         int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, const vad_audio_batch *b, const vad_audio_window *windows,
                         int64_t nw, const float *shift, const float *scale, int64_t nss, void *out, int64_t out_bytes, uint8_t *mask) {
    return audio_batch_entry(e, false, "vad_scan_audio_batch", items, n, audio, audio_samples, channels, frame_fmt, sr_in, hop, denoise_thresh, b,
                             windows, nw, shift, scale, nss, out, out_bytes, mask, nullptr);
}

int vad_scan_audio_batch_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                                int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, const vad_audio_batch *b,
                                const vad_audio_window *windows, int64_t nw, const float *shift, const float *scale, int64_t nss, void *d_out,
                                int64_t out_bytes, uint8_t *d_mask, void *stream) {
    return audio_batch_entry(e, true, "vad_scan_audio_batch_device", items, n, d_audio, audio_samples, channels, frame_fmt, sr_in, hop,
                             denoise_thresh, b, windows, nw, shift, scale, nss, d_out, out_bytes, d_mask, stream);
}

int vad_scan_render(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const float *ramp, int32_t nramp, const void *audio,
                    int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t out_fmt,
                    void *out, int64_t out_samples) {
    return render_entry(e, false, "vad_scan_render", false, items, n, gains, ramp, nramp, audio, audio_samples, channels, frame_fmt, sr_in, hop,
                        denoise_thresh, out_fmt, out, out_samples, nullptr);
}

int vad_scan_render_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const float *ramp, int32_t nramp,
                           const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                           float denoise_thresh, int32_t out_fmt, void *d_out, int64_t out_samples, void *stream) {
    return render_entry(e, true, "vad_scan_render_device", false, items, n, gains, ramp, nramp, d_audio, audio_samples, channels, frame_fmt, sr_in, hop,
                        denoise_thresh, out_fmt, d_out, out_samples, stream);
}

// both channels of a two-channel block, interleaved (csrc/scan_cut.hip, csrc/scan_render.hip): the mono calls'
// plans, tables and checks under these names, sample FRAMES where those count samples
int vad_scan_cut_stereo(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const void *audio, int64_t audio_samples,
                        int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt,
                        void *out, int64_t out_samples) {
    return payload_entry(e, false, "vad_scan_cut_stereo", Cut::STEREO, items, n, gains, audio, audio_samples, channels, frame_fmt, sr_in, hop,
                         denoise_thresh, layout, out_fmt, out, out_samples, nullptr);
}

int vad_scan_cut_stereo_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const void *d_audio, int64_t audio_samples,
                               int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt,
                               void *d_out, int64_t out_samples, void *stream) {
    return payload_entry(e, true, "vad_scan_cut_stereo_device", Cut::STEREO, items, n, gains, d_audio, audio_samples, channels, frame_fmt, sr_in,
                         hop, denoise_thresh, layout, out_fmt, d_out, out_samples, stream);
}

int vad_scan_render_stereo(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const float *ramp, int32_t nramp,
                           const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                           float denoise_thresh, int32_t out_fmt, void *out, int64_t out_samples) {
    return render_entry(e, false, "vad_scan_render_stereo", true, items, n, gains, ramp, nramp, audio, audio_samples, channels, frame_fmt, sr_in, hop,
                        denoise_thresh, out_fmt, out, out_samples, nullptr);
}

int vad_scan_render_stereo_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains, const float *ramp, int32_t nramp,
                                  const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                                  float denoise_thresh, int32_t out_fmt, void *d_out, int64_t out_samples, void *stream) {
    return render_entry(e, true, "vad_scan_render_stereo_device", true, items, n, gains, ramp, nramp, d_audio, audio_samples, channels, frame_fmt,
                        sr_in, hop, denoise_thresh, out_fmt, d_out, out_samples, stream);
}

}  // extern "C"

// ---- the segment table of a scan (vad_segments_device, vad_scan_segments, vad_scan_rate_segments) ---------------------------
// This section and the three behind vad_scan_convert_segments - the replay, the tails, the refinement - are one family: the calls
// that make or rewrite segment tables from per-frame results.  Every one enters through call_begin and leaves through
// call_end, keeps its work area in one DevTables, and shares the checks and the small launches below.
namespace {

static_assert(sizeof(vad_segment) == sizeof(vadk::SegRecord), "the header's record is the kernel's");

// what a call that is given positions checks about them: the first not negative, never decreasing, at most 2^31 - 1 frames
// -> *total = out_start[n]
int check_positions(vad_engine *e, const char *who, const int64_t *out_start, int64_t n, int64_t *total) {
    if (n > 0 && out_start[0] < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_start[0] is negative", who);
    for (int64_t i = 0; i < n; ++i)
        if (out_start[i + 1] < out_start[i])
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_start decreases at item %lld (%lld after %lld)", who, (long long)i,
                           (long long)out_start[i + 1], (long long)out_start[i]);
    *total = n > 0 ? out_start[n] : 0;
    if (*total > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 frames in one call", who);
    return VAD_OK;
}

// what a host form that works on the last scan's per-frame results checks: the mark (scan_segments_run sets it)
int check_resident(vad_engine *e, const char *who) {
    if (!e->scan_results || e->seg_out_start.empty())
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: no scan results are resident: the engine's last vad_scan_segments or "
                                            "vad_scan_rate_segments failed, or a later call has reused its per-frame arrays", who);
    return VAD_OK;
}

// What a device form checks about the caller's arrays, behind the positions: the per-frame arrays - the events and `by4` - are
// there when there is a frame; then the alignments, each list under the entry point's own noun: the events and `by16`, `by4`, `by8`
struct Ptrs { std::initializer_list<const void *> p; const char *noun; };

bool misaligned(const Ptrs &q, uintptr_t mask) {
    for (const void *p : q.p)
        if (reinterpret_cast<uintptr_t>(p) & mask) return true;
    return false;
}

int check_device_arrays(vad_engine *e, const char *who, int64_t total, const uint8_t *d_events, const Ptrs &by16, const Ptrs &by4, const Ptrs &by8) {
    bool missing = !d_events;
    for (const void *p : by4.p) missing = missing || !p;
    if (total > 0 && missing) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if ((reinterpret_cast<uintptr_t>(d_events) & 15) || misaligned(by16, 15))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %s must be 16-byte aligned", who, by16.noun);
    if (misaligned(by4, 3)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %s must be 4-byte aligned", who, by4.noun);
    if (misaligned(by8, 7)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %s must be 8-byte aligned", who, by8.noun);
    return VAD_OK;
}

// the positions as the kernels read them: int32 [n + 1] (no item: one 0) at the front of `up`, a work area's staging block of `ints`
// entries - what lies behind the positions is the caller's to write.  One block per work area: it is the source of an asynchronous
// copy, the copy's until the stream has passed it
void narrow_positions(std::vector<int32_t> &up, size_t ints, const int64_t *out_start, int64_t n) {
    up.resize(ints);
    up[0] = 0;
    for (int64_t i = 0; n > 0 && i <= n; ++i) up[(size_t)i] = (int32_t)out_start[i];
}

// counts that the launches on `s` left on the device, behind them
int read_back(vad_engine *e, long long *out, const long long *d, size_t count, hipStream_t s) {
    HIP_TRY(e, hipMemcpyAsync(out, d, sizeof(long long) * count, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// `take` records of a table of the engine's to the caller, behind the launches on `s`
int download_records(vad_engine *e, vad_segment *out, const vadk::SegRecord *d, int64_t take, hipStream_t s) {
    HIP_TRY(e, hipMemcpyAsync(out, d, sizeof(vad_segment) * (size_t)take, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

// the statistics of the records that a replay or a refinement has written into d_segs; `most` bounds the records there are
int seg_stats(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int32_t *d_start, int32_t n, vadk::SegRecord *d_segs,
              uint32_t seg_cap, long long *d_nsegs, int64_t most, hipStream_t s) {
    vadk::SegArgs st{};
    st.events = d_events;
    st.probs = d_probs;
    st.out_start = d_start;
    st.segs = d_segs;
    st.nsegs = d_nsegs;
    st.seg_cap = seg_cap;
    st.n = n;
    const hipError_t r = vadk_launch_seg_stats(&st, (uint32_t)std::min<int64_t>(most, (int64_t)seg_cap), s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (segment statistics)");
    return VAD_OK;
}

// the launches of an extraction on `s`: out_start (checked: check_positions) goes to the device as int32 next to the chunk counts;
// seg_cap >= 0, the table at d_segs has room for it
int seg_launches(vad_engine *e, const uint8_t *d_events, const int32_t *d_seg, const float *d_probs, const int64_t *out_start, int64_t n,
                 vadk::SegRecord *d_segs, int64_t seg_cap, long long *d_nsegs, hipStream_t s) {
    const int64_t total = n > 0 ? out_start[n] : 0;
    vadk::SegArgs a{};
    a.first = n > 0 ? (uint32_t)out_start[0] : 0u;
    a.total = (uint32_t)total;
    a.nchunks = (uint32_t)((total + vadk::SEG_WG_FRAMES - 1) / vadk::SEG_WG_FRAMES);
    a.seg_cap = (uint32_t)std::min<int64_t>(seg_cap, INT32_MAX);
    a.n = (int32_t)n;
    a.events = d_events;
    a.seg_frames = d_seg;
    a.probs = d_probs;
    a.segs = d_segs;
    a.nsegs = d_nsegs;
    if (a.nchunks) {
        DevTables t{e->d_segwork, e->d_segwork_cap};
        narrow_positions(e->seg_start, (size_t)n + 1, out_start, n);
        const int k_start = t.add(e->seg_start, (size_t)n + 1), k_chunk = t.add(nullptr, sizeof(uint32_t) * (size_t)a.nchunks);
        if (int rc = t.reserve(e)) return rc;
        if (int rc = t.copy(e, s)) return rc;
        a.out_start = t.at<const int32_t>(k_start);
        a.chunk = t.at<uint32_t>(k_chunk);
    }
    const hipError_t r = vadk_launch_scan_segments(&a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (scan segments)");
    return VAD_OK;
}

// The first half of a tails call on `s`: the work area for n > 0 items under nt sets - out_start (checked: check_positions) with,
// slots != nullptr, the items' slots behind it, as int32 in one block; the lengths; the records.  a->tail_len and a->tails point
// into the work area; a caller with arrays of its own for either replaces them.
int tail_setup(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n, int64_t nt, const int64_t *slots,
               hipStream_t s, vadk::TailArgs *a) {
    DevTables t{e->d_tailwork, e->d_tailwork_cap};
    const size_t ints = (size_t)(n + 1) + (slots ? (size_t)n : 0), each = (size_t)nt * (size_t)n;
    narrow_positions(e->tail_up, ints, out_start, n);
    for (int64_t i = 0; slots && i < n; ++i) e->tail_up[(size_t)(n + 1 + i)] = (int32_t)slots[i];
    const int k_start = t.add(e->tail_up, ints), k_len = t.add(nullptr, sizeof(uint32_t) * each), k_rec = t.add(nullptr, sizeof(vadk::SegRecord) * each);
    if (int rc = t.reserve(e)) return rc;
    if (int rc = t.copy(e, s)) return rc;
    *a = vadk::TailArgs{};
    a->events = d_events;
    a->probs = d_probs;
    a->out_start = t.at<const int32_t>(k_start);
    a->sm = e->d_sm;
    a->slots = slots ? a->out_start + (n + 1) : nullptr;
    a->tail_len = t.at<uint32_t>(k_len);
    a->tails = t.at<vadk::SegRecord>(k_rec);
    a->n = (int32_t)n;
    a->nt = (int32_t)nt;
    return VAD_OK;
}

// the lengths of the segments open in the items' slots, out of the streams' state machines, into a->tail_len
int tail_snapshot(vad_engine *e, const vadk::TailArgs *a, hipStream_t s) {
    const hipError_t r = vadk_launch_tail_snapshot(a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (tail snapshot)");
    return VAD_OK;
}

// the tails' lengths of a scan, out of the streams' state machines as the model launches leave them (vad_scan_tails): one small
// launch on the same stream, no model launch - vad_info.steps and .frames do not move; whatever a later call does to the slots
// comes behind it
int scan_tail_lengths(vad_engine *e, const vad_scan_ch_item *items, int64_t n, hipStream_t s) {
    std::vector<int64_t> slots((size_t)n);
    for (int64_t i = 0; i < n; ++i) slots[(size_t)i] = items[i].slot;
    if (int rc = ensure(e, e->d_tail_len, e->d_tail_len_cap, sizeof(uint32_t) * (size_t)n)) return rc;
    vadk::TailArgs ta;
    if (int rc = tail_setup(e, e->d_events, e->d_probs, e->seg_out_start.data(), n, 1, slots.data(), s, &ta)) return rc;
    ta.tail_len = e->d_tail_len;
    return tail_snapshot(e, &ta, s);
}

// vad_scan_segments and vad_scan_rate_segments (chunk > 0: the recordings are at sr_in), with e->mu held: the scan of host audio
// into the engine's own arrays - the block stays resident, of its rate - then the extraction.  fill: nullptr, or
// (vad_scan_convert_segments) there is no host audio and the block is written into e->d_audio by fill's launches
int scan_segments_run(vad_engine *e, const char *who, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                      int32_t channels, int frame_fmt, int chunk, int32_t sr_in, int32_t hop, float denoise_thresh, vad_segment *segs_out,
                      int64_t seg_cap, int64_t *nsegs_out, const std::function<int()> *fill) {
    hipStream_t s;
    if (int rc = call_begin(e, false, nullptr, &s)) return rc;
    // the CSR positions the caller of vad_scan_channels would have passed are the plan's to make: the items packed in their order
    std::vector<int64_t> &start = e->seg_out_start;
    e->scan_results = false;                 // the plan rewrites the positions
    int64_t total = 0;
    if (int rc = scan_plan(e, who, items, n, audio_samples, channels, frame_fmt, hop, (const int64_t *)nullptr, 0, &total, &start, chunk)) return rc;
    if (seg_cap < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: seg_cap = %lld: bad count", who, (long long)seg_cap);
    if (!nsegs_out || (seg_cap > 0 && !segs_out) || (total > 0 && !audio && !fill))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    e->segtab_count = -1;
    if (total == 0) {                        // nothing to scan: an empty table
        e->segtab_count = 0;
        e->scan_results = true;
        *nsegs_out = 0;
        return VAD_OK;
    }
    int launched = scan_upload_launch(e, n, audio, audio_samples, channels, frame_fmt, chunk, sr_in, hop, denoise_thresh, total, true, fill);
    if (launched == VAD_OK) launched = scan_tail_lengths(e, items, n, s);
    if (int rc = call_end(e, false, s, launched)) return rc;
    if (int rc = ensure(e, e->d_nsegs, e->d_nsegs_cap, sizeof(long long))) return rc;
    // the table's size is known only behind the count: room for the caller's capacity and for a segment per 16 frames first, and
    // the extraction once more (the per-frame arrays are still there) in the rare case that the table is larger
    int64_t room = std::min(total, std::max<int64_t>({seg_cap, total / 16 + 256, (int64_t)(e->d_segtab_cap / sizeof(vadk::SegRecord))}));
    long long count = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (int rc = ensure(e, e->d_segtab, e->d_segtab_cap, sizeof(vadk::SegRecord) * (size_t)room)) return rc;
        if (int rc = seg_launches(e, e->d_events, e->d_seg, e->d_probs, start.data(), n, e->d_segtab, room, e->d_nsegs, s)) return rc;
        if (int rc = read_back(e, &count, e->d_nsegs, 1, s)) return rc;
        if (count <= room) break;
        room = count;
    }
    const int64_t take = std::min<int64_t>(count, seg_cap);
    if (take > 0)
        if (int rc = download_records(e, segs_out, e->d_segtab, take, s)) return rc;
    e->segtab_count = count;
    e->scan_results = true;
    *nsegs_out = count;
    return VAD_OK;
}

}  // namespace

extern "C" {

int vad_segments_device(vad_engine *e, const uint8_t *d_events, const int32_t *d_seg_frames, const float *d_probs, const int64_t *out_start,
                        int64_t n, vad_segment *d_segs, int64_t seg_cap, int64_t *d_nsegs, void *stream) {
    static const char *who = "vad_segments_device";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s;
    if (int rc = call_begin(e, true, stream, &s)) return rc;
    if (n < 0 || seg_cap < 0)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n = %lld, seg_cap = %lld: bad count", who, (long long)n, (long long)seg_cap);
    if (n > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 items", who);
    if ((n > 0 && !out_start) || !d_nsegs || (seg_cap > 0 && !d_segs))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    int64_t total = 0;
    if (int rc = check_positions(e, who, out_start, n, &total)) return rc;
    if (int rc = check_device_arrays(e, who, total, d_events, {{d_segs}, "the events and the segment table"},
                                     {{d_seg_frames, d_probs}, "seg_frames and probs"}, {{d_nsegs}, "the count"}))
        return rc;
    return call_end(e, true, s, seg_launches(e, d_events, d_seg_frames, d_probs, out_start, n, reinterpret_cast<vadk::SegRecord *>(d_segs), seg_cap,
                                             reinterpret_cast<long long *>(d_nsegs), s));
}

int vad_scan_segments(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                      int frame_fmt, int32_t hop, float denoise_thresh, vad_segment *segs_out, int64_t seg_cap, int64_t *nsegs_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_segments_run(e, "vad_scan_segments", items, n, audio, audio_samples, channels, frame_fmt, 0, 0, hop, denoise_thresh, segs_out, seg_cap,
                             nsegs_out, nullptr);
}

// (sr_in == 16000: scan_rate_check answers chunk = 0, and the call is vad_scan_segments under this name)
int vad_scan_rate_segments(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                           int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, vad_segment *segs_out, int64_t seg_cap,
                           int64_t *nsegs_out) {
    static const char *who = "vad_scan_rate_segments";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    int chunk = 0;
    if (int rc = scan_rate_check(e, who, sr_in, &chunk)) return rc;
    return scan_segments_run(e, who, items, n, audio, audio_samples, channels, frame_fmt, chunk, sr_in, hop, denoise_thresh, segs_out, seg_cap,
                             nsegs_out, nullptr);
}

// No call_begin: nothing is launched and no table is rebuilt.  d_segtab is written by scan_segments_run alone, on the engine's stream,
// which this copy is on too, and no device call reads or writes it: there is no earlier launch to wait for
int vad_scan_segments_read(vad_engine *e, int64_t first, int64_t count, vad_segment *out) {
    static const char *who = "vad_scan_segments_read";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->segtab_count < 0)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the engine holds no segment table: no vad_scan_segments has built one", who);
    if (first < 0 || count < 0 || first > e->segtab_count || count > e->segtab_count - first)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: records %lld .. +%lld leave the table of %lld", who, (long long)first,
                       (long long)count, (long long)e->segtab_count);
    if (count == 0) return VAD_OK;
    if (!out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    HIP_TRY(e, hipSetDevice(e->device));
    return download_records(e, out, e->d_segtab + first, count, e->stream);
}

}  // extern "C"

// ---- vad_convert / vad_scan_convert_segments: whole recordings at any accepted rate, converted once to the engine's rate -------
namespace {

// everything about a conversion that follows from the two rates and the tap count (vad_layout.h: the periods)
struct ConvertPlan {
    uint32_t L = 0, M = 0, P = 0, PI = 0, ntiles = 0, K = 0, lead = 0, nper = 0;
    int32_t bmax = 0;
};

// L / M of the header's rule; false: sr_in is not an accepted rate (L and M are set where they exist, for the message)
bool convert_ratio(int32_t R, int32_t sr_in, uint32_t *L, uint32_t *M) {
    *L = *M = 0;
    if (R < 1 || sr_in < 1) return false;
    const uint32_t g = vadk::cv_gcd((uint32_t)R, (uint32_t)sr_in);
    *L = (uint32_t)R / g;
    *M = (uint32_t)sr_in / g;
    if (sr_in < VAD_CONVERT_MIN_RATE || sr_in > VAD_CONVERT_MAX_RATE || sr_in == R) return false;
    return *L / vadk::cv_gcd(*L, 16u) * 16u <= (uint32_t)VAD_CONVERT_MAX_PERIOD && *M <= (uint32_t)VAD_CONVERT_MAX_PERIOD;
}

// what comes before the block's and the items' checks: the rate, then the taps
int convert_check(vad_engine *e, const char *who, int32_t sr_in, const float *taps, int32_t ntaps, ConvertPlan *c) {
    uint32_t L = 0, M = 0;
    if (!convert_ratio(e->sample_rate, sr_in, &L, &M))
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to %dHz: %s: L / M = %u / %u; accepted are rates from %d to %d Hz other "
                       "than the engine's whose period lcm(L, 16) is at most %d outputs and whose M is at most %d", sr_in, e->sample_rate, who, L, M,
                       VAD_CONVERT_MIN_RATE, VAD_CONVERT_MAX_RATE, VAD_CONVERT_MAX_PERIOD, VAD_CONVERT_MAX_PERIOD);
    if (!taps) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null taps", who);
    const int64_t most = (int64_t)VAD_CONVERT_MAX_REACH * (int64_t)L;
    if (ntaps < 1 || (int64_t)ntaps > most || !(ntaps & 1))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: ntaps = %d must be odd, from 1 to %lld (VAD_CONVERT_MAX_REACH * L, L = %u)", who,
                       ntaps, (long long)most, L);
    for (int32_t k = 0; k < ntaps; ++k)
        if (!std::isfinite(taps[k]))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: taps[%d] is %s, a tap is a finite number", who, k,
                           std::isnan(taps[k]) ? "NaN" : "infinite");
    c->L = L;
    c->M = M;
    c->P = vadk::cv_P(L);
    c->PI = vadk::cv_PI(L, M);
    c->ntiles = c->P / 16u;
    c->K = vadk::cv_K((uint32_t)ntaps, L, M);
    c->lead = vadk::cv_lead((uint32_t)ntaps, L);
    c->bmax = vadk::cv_base(c->ntiles - 1u, (uint32_t)ntaps, L, M);
    c->nper = vadk::cv_nper(c->P, c->PI, c->lead, c->bmax, c->K);
    if (c->nper == 0)
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to %dHz: %s: L / M = %u / %u: one period of %u inputs and %d taps "
                       "does not fit a workgroup's local memory", sr_in, e->sample_rate, who, L, M, c->PI, ntaps);
    return VAD_OK;
}

// The block's and the items' refusals, in vad_scan_channels's words (scan_plan's; no hop, no slot and no stream count enter a
// conversion), and the plan: e->cv_items, e->cv_work, and e->cv_offset [n + 1] = the items' first samples in the converted block
int convert_plan(vad_engine *e, const char *who, const ConvertPlan &c, const vad_scan_ch_item *items, int64_t n, int64_t audio_samples,
                 int32_t channels, int fmt) {
    if (n < 0 || audio_samples < 0 || (n > 0 && !items)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer or bad count", who);
    if (int rc = check_block_format(e, who, fmt, channels)) return rc;
    if (int rc = check_block_extent(e, who, 4, audio_samples, channels, fmt)) return rc;
    if (n > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 items", who);
    e->cv_items.resize((size_t)n);
    e->cv_work.clear();
    e->cv_offset.assign((size_t)n + 1, 0);
    const uint64_t run = (uint64_t)c.nper * c.P;
    for (int64_t i = 0; i < n; ++i) {
        const vad_scan_ch_item &it = items[i];
        if (it.sample_offset < 0 || (it.sample_offset & 3))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld starts at sample %lld, not a multiple of 4", who,
                           (long long)i, (long long)it.sample_offset);
        if (it.nsamples < 0 || it.sample_offset > audio_samples || it.nsamples > audio_samples - it.sample_offset)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld (samples %lld .. +%lld) leaves the audio block of %lld samples", who,
                           (long long)i, (long long)it.sample_offset, (long long)it.nsamples, (long long)audio_samples);
        if (it.channel != VAD_SCAN_MIX && (it.channel < 0 || it.channel >= channels))
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld names channel %d of %d (0 .. channels - 1, or VAD_SCAN_MIX)", who,
                           (long long)i, it.channel, channels);
        if (it.reserved != 0)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: recording %lld: reserved = %d must be 0", who, (long long)i, it.reserved);
        const uint64_t s_out = (uint64_t)it.nsamples * c.L / c.M;        // (nsamples < 2^31, L <= 640)
        const int64_t at = e->cv_offset[(size_t)i];
        e->cv_offset[(size_t)i + 1] = at + (int64_t)((s_out + 3u) & ~(uint64_t)3);
        if (e->cv_offset[(size_t)i + 1] >= (int64_t)1 << 29)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the converted block reaches 2 GiB of float32 at recording %lld; one call "
                           "may address less", who, (long long)i);
        const uint32_t mode = channels == 1 ? vadk::SCAN_LEFT : it.channel == VAD_SCAN_MIX ? vadk::SCAN_MIX : (uint32_t)it.channel;
        e->cv_items[(size_t)i] = vadk::ConvertItem{(uint32_t)(it.sample_offset >> 2) | (mode << vadk::SCAN_MODE_SHIFT), (uint32_t)it.nsamples,
                                                   (uint32_t)s_out, (uint32_t)(at >> 2)};
        for (uint64_t r = 0; r * run < s_out; ++r) e->cv_work.push_back(vadk::ConvertWork{(uint32_t)i, (uint32_t)r});
    }
    return VAD_OK;
}

// the operators of all row-tiles in fragment order in e->d_cv_op, zeros outside the taps; cached against the previous call's bytes
int convert_operator(vad_engine *e, const ConvertPlan &c, const float *taps, int32_t ntaps, hipStream_t s) {
    if (e->cv_packed && e->cv_L == c.L && e->cv_M == c.M && e->cv_src.size() == (size_t)ntaps &&
        !std::memcmp(e->cv_src.data(), taps, sizeof(float) * (size_t)ntaps))
        return VAD_OK;
    e->cv_packed = false;
    const size_t floats = (size_t)c.ntiles * 16u * c.K;
    if (int rc = ensure(e, e->d_cv_op, e->d_cv_op_cap, sizeof(float) * floats)) return rc;
    e->cv_src.assign(taps, taps + ntaps);
    e->cv_pack.assign(floats, 0.0f);
    for (uint32_t r = 0; r < c.ntiles; ++r)
        for (uint32_t o = 0; o < 16u; ++o)
            for (uint32_t n = 0; n < c.K; ++n) {
                const int64_t t = vadk::cv_tap(r, o, n, (uint32_t)ntaps, c.L, c.M);
                if (t >= 0 && t < ntaps) e->cv_pack[vadk::cv_pack_index(r, o, n, c.K)] = taps[t];
            }
    HIP_TRY(e, hipMemcpyAsync(e->d_cv_op, e->cv_pack.data(), sizeof(float) * floats, hipMemcpyHostToDevice, s));
    e->cv_L = c.L;
    e->cv_M = c.M;
    e->cv_packed = true;
    return VAD_OK;
}

// the planned conversion on `s`: the operators, the tables, the launch.  d_audio: the block in its wire format; d_out: room for
// e->cv_offset.back() floats
int convert_enqueue(vad_engine *e, const ConvertPlan &c, const float *taps, int32_t ntaps, const void *d_audio, int32_t channels, int fmt,
                    float *d_out, hipStream_t s) {
    if (e->cv_work.empty()) return VAD_OK;
    if (int rc = convert_operator(e, c, taps, ntaps, s)) return rc;
    const size_t ib = sizeof(vadk::ConvertItem) * e->cv_items.size(), wb = sizeof(vadk::ConvertWork) * e->cv_work.size();
    if (int rc = ensure(e, e->d_cv_tab, e->d_cv_tab_cap, ib + wb)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_cv_tab, e->cv_items.data(), ib, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemcpyAsync(e->d_cv_tab + ib, e->cv_work.data(), wb, hipMemcpyHostToDevice, s));
    vadk::ConvertArgs a{};
    a.audio = d_audio;
    a.out = d_out;
    a.items = reinterpret_cast<const vadk::ConvertItem *>(e->d_cv_tab);
    a.work = reinterpret_cast<const vadk::ConvertWork *>(e->d_cv_tab + ib);
    a.op = e->d_cv_op;
    a.nwork = (uint32_t)e->cv_work.size();
    a.L = c.L;
    a.M = c.M;
    a.ntaps = (uint32_t)ntaps;
    a.P = c.P;
    a.PI = c.PI;
    a.ntiles = c.ntiles;
    a.ksteps = c.K >> 4;
    a.nper = c.nper;
    a.bmax = c.bmax;
    a.fmt = fmt;
    a.channels = channels;
    const hipError_t r = vadk_launch_convert(&a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (convert)");
    return VAD_OK;
}

// vad_convert and vad_convert_device with e->mu held
int convert_run(vad_engine *e, bool dev, const char *who, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                int32_t channels, int fmt, int32_t sr_in, const float *taps, int32_t ntaps, float *out, int64_t out_samples, int64_t *out_offset,
                void *stream) {
    hipStream_t s;
    if (int rc = call_begin(e, dev, stream, &s)) return rc;
    ConvertPlan c;
    if (int rc = convert_check(e, who, sr_in, taps, ntaps, &c)) return rc;
    if (int rc = convert_plan(e, who, c, items, n, audio_samples, channels, fmt)) return rc;
    const int64_t total = e->cv_offset.back();
    if (out_samples < total)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: out_samples = %lld, the converted block has %lld samples", who,
                       (long long)out_samples, (long long)total);
    if (total > 0 && (!audio || !out)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (dev && total > 0) {
        if (int rc = check_device_audio(e, who, audio, channels)) return rc;
        if (reinterpret_cast<uintptr_t>(out) & 15)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the output must be 16-byte aligned", who);
    }
    if (out_offset) std::copy(e->cv_offset.begin(), e->cv_offset.end(), out_offset);
    if (total == 0) return VAD_OK;
    const void *d_in = audio;
    float *d_out = out;
    if (!dev) {
        const size_t ab = (size_t)audio_samples * (size_t)channels * sample_bytes(fmt);
        if (int rc = ensure(e, e->d_cv_in, e->d_cv_in_cap, ab + 16)) return rc;
        if (int rc = ensure(e, e->d_cv_out, e->d_cv_out_cap, sizeof(float) * (size_t)total)) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->d_cv_in, audio, ab, hipMemcpyHostToDevice, s));
        d_in = e->d_cv_in;
        d_out = e->d_cv_out;
    }
    const int rc = call_end(e, dev, s, convert_enqueue(e, c, taps, ntaps, d_in, channels, fmt, d_out, s));
    if (rc || dev) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, e->d_cv_out, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return VAD_OK;
}

}  // namespace

extern "C" {

int64_t vad_convert_samples(const vad_engine *e, int64_t nsamples, int32_t sr_in) {
    uint32_t L = 0, M = 0;
    if (!e || nsamples < 0 || nsamples >= ((int64_t)1 << 31) || !convert_ratio(e->sample_rate, sr_in, &L, &M)) return -1;
    return nsamples * (int64_t)L / (int64_t)M;
}

int vad_convert(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                int32_t sr_in, const float *taps, int32_t ntaps, float *out, int64_t out_samples, int64_t *out_offset) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return convert_run(e, false, "vad_convert", items, n, audio, audio_samples, channels, frame_fmt, sr_in, taps, ntaps, out, out_samples, out_offset,
                       nullptr);
}

int vad_convert_device(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *d_audio, int64_t audio_samples, int32_t channels,
                       int frame_fmt, int32_t sr_in, const float *taps, int32_t ntaps, float *d_out, int64_t out_samples, int64_t *out_offset,
                       void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return convert_run(e, true, "vad_convert_device", items, n, d_audio, audio_samples, channels, frame_fmt, sr_in, taps, ntaps, d_out, out_samples,
                       out_offset, stream);
}

// the conversion into e->d_audio, then vad_scan_segments' own path over that block: the items {slot, out_offset[i], S_out_i, 0} of a
// mono float32 block of out_offset[n] samples
int vad_scan_convert_segments(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                              int frame_fmt, int32_t sr_in, const float *taps, int32_t ntaps, int32_t hop, float denoise_thresh,
                              vad_segment *segs_out, int64_t seg_cap, int64_t *nsegs_out, int64_t *out_offset) {
    static const char *who = "vad_scan_convert_segments";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(e, hipSetDevice(e->device));
    if (int rc = scan_wait(e)) return rc;
    ConvertPlan c;
    if (int rc = convert_check(e, who, sr_in, taps, ntaps, &c)) return rc;
    if (int rc = convert_plan(e, who, c, items, n, audio_samples, channels, frame_fmt)) return rc;
    const int64_t total = e->cv_offset.back();
    e->cv_scan_items.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        e->cv_scan_items[(size_t)i] = vad_scan_ch_item{items[i].slot, e->cv_offset[(size_t)i], (int64_t)e->cv_items[(size_t)i].s_out, 0, 0};
    if (!audio && !e->cv_work.empty()) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    const std::function<int()> fill = [&]() -> int {
        const size_t ab = (size_t)audio_samples * (size_t)channels * sample_bytes(frame_fmt);
        if (int rc = ensure(e, e->d_cv_in, e->d_cv_in_cap, ab + 16)) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->d_cv_in, audio, ab, hipMemcpyHostToDevice, e->stream));
        return convert_enqueue(e, c, taps, ntaps, e->d_cv_in, channels, frame_fmt, static_cast<float *>(e->d_audio), e->stream);
    };
    // (vad_scan_segments' refusals follow under this function's name; a refused call has written nothing)
    if (int rc = scan_segments_run(e, who, e->cv_scan_items.data(), n, nullptr, total, 1, VAD_FMT_F32, 0, 0, hop, denoise_thresh, segs_out, seg_cap,
                                   nsegs_out, &fill))
        return rc;
    if (out_offset) std::copy(e->cv_offset.begin(), e->cv_offset.end(), out_offset);
    return VAD_OK;
}

}  // extern "C"

// ---- segment tables at other thresholds, from a scan's per-frame results (vad_resegment_device, vad_scan_resegment) -----------
namespace {

static_assert(VAD_RESEGMENT_MAX_SETS == vadk::RESEG_MAX_SETS, "the header's limit is the kernel's");
static_assert(sizeof(vad_thresholds) % sizeof(int32_t) == 0, "the sets lie in the replay's int32 staging block");

// what the replays check about the sets and the capacity
int reseg_check_sets(vad_engine *e, const char *who, const vad_thresholds *t, int64_t nt, int64_t seg_cap) {
    if (nt < 1 || nt > vadk::RESEG_MAX_SETS)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: nt = %lld: 1 .. %d threshold sets in one call", who, (long long)nt,
                       vadk::RESEG_MAX_SETS);
    if (seg_cap < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: seg_cap = %lld: bad count", who, (long long)seg_cap);
    if (!t) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    return VAD_OK;
}

// ... and the device forms about their counts, behind the sets
int reseg_check_counts(vad_engine *e, const char *who, int64_t n, int64_t nt) {
    if (n < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n = %lld: bad count", who, (long long)n);
    if (n * nt > INT32_MAX)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %lld items x %lld sets: more than 2^31 - 1 replays in one call", who,
                       (long long)n, (long long)nt);
    return VAD_OK;
}

// The work area of a replay on `s`, before its launch.  out_start (checked: check_positions), the sets' lane numbers and the sets
// are three adjoining tables and go up as ONE copy, out of one staging block laid out as they lie; behind them room for the nt
// scratch state machines, the sets' counts, the items' counts and - tails - the lengths [nt n] of the segments open behind each
// item's last frame (*tail_len; nullptr without).  The initial state machines are built by the kernel that serves vad_stream_open
// and vad_stream_set_thresholds - default, then the set's thresholds - on the scratch records (no stream's slot, no (h, c)).
// d_set_start == nullptr: the sets' counts go to the work area (a->set_start says where).
int reseg_setup(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n, const vad_thresholds *t,
                int64_t nt, bool tails, long long *d_set_start, hipStream_t s, vadk::ResegArgs *a, uint32_t **tail_len) {
    DevTables w{e->d_reseg, e->d_reseg_cap};
    const size_t each = (size_t)nt * (size_t)n;
    const int k_start = w.add(nullptr, sizeof(int32_t) * (size_t)(n + 1)), k_lane = w.add(nullptr, sizeof(int32_t) * (size_t)nt),
              k_thr = w.add(nullptr, sizeof(vad_thresholds) * (size_t)nt);
    const size_t up_bytes = w.total;
    const int k_sm = w.add(nullptr, sizeof(vadk::SmSlot) * (size_t)nt), k_set = w.add(nullptr, sizeof(long long) * (size_t)(nt + 1)),
              k_cnt = w.add(nullptr, sizeof(uint32_t) * each), k_tail = w.add(nullptr, tails ? sizeof(uint32_t) * each : 0);
    if (int rc = w.reserve(e)) return rc;
    narrow_positions(e->reseg_up, up_bytes / sizeof(int32_t), out_start, n);
    int32_t *up = e->reseg_up.data();
    for (int64_t k = 0; k < nt; ++k) up[w.off[k_lane] / sizeof(int32_t) + (size_t)k] = (int32_t)k;
    std::memcpy(up + w.off[k_thr] / sizeof(int32_t), t, sizeof(vad_thresholds) * (size_t)nt);
    HIP_TRY(e, hipMemcpyAsync(w.at<int32_t>(k_start), up, up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(e, vadk_launch_slot_control(w.at<vadk::SmSlot>(k_sm), nullptr, w.at<const int32_t>(k_lane), (int)nt, CTL_DEFAULT_SM | CTL_SET_THRESHOLDS,
                                        &kDefaultSm, w.at<const vad_thresholds>(k_thr), (int)nt, s));
    int shift = 0;
    while ((int64_t(1) << shift) < nt) ++shift;
    *a = vadk::ResegArgs{};
    a->events = d_events;
    a->probs = d_probs;
    a->out_start = w.at<const int32_t>(k_start);
    a->sm0 = w.at<vadk::SmSlot>(k_sm);
    a->cnt = w.at<uint32_t>(k_cnt);
    a->set_start = d_set_start ? d_set_start : w.at<long long>(k_set);
    a->n = (int32_t)n;
    a->nt = (int32_t)nt;
    a->set_shift = shift;
    *tail_len = w.at<uint32_t>(k_tail);
    return VAD_OK;
}

// the first half of a replay: the items' counts and their prefix, the sets' counts in a->set_start
int reseg_count(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n, const vad_thresholds *t,
                int64_t nt, long long *d_set_start, hipStream_t s, vadk::ResegArgs *a) {
    uint32_t *none;
    if (int rc = reseg_setup(e, d_events, d_probs, out_start, n, t, nt, false, d_set_start, s, a, &none)) return rc;
    const hipError_t r = vadk_launch_reseg_count(a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (resegment count)");
    return VAD_OK;
}

// the tails' replay: the count replay alone, in the form that also keeps the length of the segment open behind each item's last
// frame - *tail_len = those lengths [nt n], in the work area; no prefix, no set counts
int reseg_tail_lengths(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n, const vad_thresholds *t,
                       int64_t nt, hipStream_t s, uint32_t **tail_len) {
    vadk::ResegArgs a;
    if (int rc = reseg_setup(e, d_events, d_probs, out_start, n, t, nt, true, nullptr, s, &a, tail_len)) return rc;
    const hipError_t r = vadk_launch_reseg_tails(&a, *tail_len, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (resegment count)");
    return VAD_OK;
}

// ... and the second half behind reseg_count: the records into d_segs (room for seg_cap of them), then their statistics; `most`
// bounds the records written
int reseg_fill(vad_engine *e, vadk::ResegArgs *a, vadk::SegRecord *d_segs, int64_t seg_cap, int64_t most, hipStream_t s) {
    a->segs = d_segs;
    a->seg_cap = (uint32_t)std::min<int64_t>(seg_cap, INT32_MAX);
    const hipError_t r = vadk_launch_reseg_fill(a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (resegment fill)");
    return seg_stats(e, a->events, a->probs, a->out_start, a->n, d_segs, a->seg_cap, a->set_start + a->nt, most, s);
}

}  // namespace

extern "C" {

int vad_resegment_device(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n,
                         const vad_thresholds *t, int64_t nt, vad_segment *d_segs, int64_t seg_cap, int64_t *d_set_start, void *stream) {
    static const char *who = "vad_resegment_device";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s;
    if (int rc = call_begin(e, true, stream, &s)) return rc;
    if (int rc = reseg_check_sets(e, who, t, nt, seg_cap)) return rc;
    if (int rc = reseg_check_counts(e, who, n, nt)) return rc;
    if ((n > 0 && !out_start) || !d_set_start || (seg_cap > 0 && !d_segs))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    int64_t total = 0;
    if (int rc = check_positions(e, who, out_start, n, &total)) return rc;
    if (int rc = check_device_arrays(e, who, total, d_events, {{d_segs}, "the events and the segment table"}, {{d_probs}, "probs"},
                                     {{d_set_start}, "the set counts"}))
        return rc;
    vadk::ResegArgs a;
    int launched = reseg_count(e, d_events, d_probs, out_start, n, t, nt, reinterpret_cast<long long *>(d_set_start), s, &a);
    // a segment has a frame that starts it and a later one that ends it: at most total / 2 records per set
    if (launched == VAD_OK && seg_cap > 0)
        launched = reseg_fill(e, &a, reinterpret_cast<vadk::SegRecord *>(d_segs), seg_cap, (total / 2 + 1) * nt, s);
    return call_end(e, true, s, launched);
}

int vad_scan_resegment(vad_engine *e, const vad_thresholds *t, int64_t nt, vad_segment *segs_out, int64_t seg_cap, int64_t *set_start_out) {
    static const char *who = "vad_scan_resegment";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s;
    if (int rc = call_begin(e, false, nullptr, &s)) return rc;
    if (int rc = reseg_check_sets(e, who, t, nt, seg_cap)) return rc;
    if (!set_start_out || (seg_cap > 0 && !segs_out)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (int rc = check_resident(e, who)) return rc;
    const int64_t n = (int64_t)e->seg_out_start.size() - 1;
    std::vector<long long> counts((size_t)nt + 1, 0);
    if (e->seg_out_start[(size_t)n] > 0) {
        vadk::ResegArgs a;
        if (int rc = call_end(e, false, s, reseg_count(e, e->d_events, e->d_probs, e->seg_out_start.data(), n, t, nt, nullptr, s, &a))) return rc;
        if (int rc = read_back(e, counts.data(), a.set_start, counts.size(), s)) return rc;
        if (counts[(size_t)nt] > INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %lld records: more than 2^31 - 1 in one call", who, counts[(size_t)nt]);
        // the table is sized by the count that came back: exactly the records the caller takes
        const int64_t take = std::min<int64_t>(counts[(size_t)nt], seg_cap);
        if (take > 0) {
            if (int rc = ensure(e, e->d_resegtab, e->d_resegtab_cap, sizeof(vadk::SegRecord) * (size_t)take)) return rc;
            if (int rc = reseg_fill(e, &a, e->d_resegtab, take, take, s)) return rc;
            if (int rc = download_records(e, segs_out, e->d_resegtab, take, s)) return rc;
        }
    }
    for (int64_t k = 0; k <= nt; ++k) set_start_out[k] = counts[(size_t)k];
    return VAD_OK;
}

}  // extern "C"

// ---- the segment still open at a recording's last frame (vad_scan_tails, vad_scan_resegment_tails, the two device forms) ------
namespace {

int tail_records(vad_engine *e, const vadk::TailArgs *a, hipStream_t s) {
    const hipError_t r = vadk_launch_seg_tails(a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (segment tails)");
    return VAD_OK;
}

// vad_scan_tails and - replay: under the nt sets at t - vad_scan_resegment_tails, with e->mu held: the tails of the resident scan,
// whose item count the caller's n must be.  The lengths are the scan's own snapshot, or the replay's
int scan_tails_run(vad_engine *e, const char *who, bool replay, const vad_thresholds *t, int64_t nt, vad_segment *tails_out, int64_t n) {
    hipStream_t s;
    if (int rc = call_begin(e, false, nullptr, &s)) return rc;
    if (replay)
        if (int rc = reseg_check_sets(e, who, t, nt, 0)) return rc;
    if (int rc = check_resident(e, who)) return rc;
    const int64_t have = (int64_t)e->seg_out_start.size() - 1;
    if (n != have)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n = %lld: the scan had %lld items", who, (long long)n, (long long)have);
    if (n > 0 && !tails_out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (n == 0) return VAD_OK;
    if (e->seg_out_start[(size_t)n] == 0) {  // no frame, no tail (and no snapshot was taken)
        std::memset(tails_out, 0, sizeof(vad_segment) * (size_t)n * (size_t)nt);
        return VAD_OK;
    }
    vadk::TailArgs a;
    // (a replay's positions go up twice, once per work area and out of that area's own staging block: a few bytes per item)
    int launched = tail_setup(e, e->d_events, e->d_probs, e->seg_out_start.data(), n, nt, nullptr, s, &a);
    if (!replay) a.tail_len = e->d_tail_len;
    else if (launched == VAD_OK) launched = reseg_tail_lengths(e, e->d_events, e->d_probs, e->seg_out_start.data(), n, t, nt, s, &a.tail_len);
    if (launched == VAD_OK) launched = tail_records(e, &a, s);
    if (int rc = call_end(e, false, s, launched)) return rc;
    return download_records(e, tails_out, a.tails, n * nt, s);
}

// vad_tails_device and - replay: under the nt sets at t, no slots - vad_resegment_tails_device, with e->mu held: the same on the
// caller's per-frame arrays, the records into d_tails.  The lengths come out of the slots' state machines, or out of the replay
int tails_device_run(vad_engine *e, const char *who, bool replay, const int64_t *slots, const uint8_t *d_events, const float *d_probs,
                     const int64_t *out_start, int64_t n, const vad_thresholds *t, int64_t nt, vad_segment *d_tails, void *stream) {
    hipStream_t s;
    if (int rc = call_begin(e, true, stream, &s)) return rc;
    if (replay) {
        if (int rc = reseg_check_sets(e, who, t, nt, 0)) return rc;
        if (int rc = reseg_check_counts(e, who, n, nt)) return rc;
    } else {
        if (n < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n = %lld: bad count", who, (long long)n);
        if (n > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 items", who);
    }
    if (n > 0 && ((!replay && !slots) || !out_start || !d_tails)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    int64_t total = 0;
    if (int rc = check_positions(e, who, out_start, n, &total)) return rc;
    if (int rc = check_device_arrays(e, who, total, d_events, {{d_tails}, "the events and the tails"}, {{d_probs}, "probs"}, {{}, nullptr})) return rc;
    if (!replay)
        if (int rc = check_slots(e, slots, n)) return rc;
    if (n == 0) return VAD_OK;               // nothing was launched: nothing to mark
    vadk::TailArgs a;
    int launched = tail_setup(e, d_events, d_probs, out_start, n, nt, replay ? nullptr : slots, s, &a);
    a.tails = reinterpret_cast<vadk::SegRecord *>(d_tails);
    if (launched == VAD_OK) launched = replay ? reseg_tail_lengths(e, d_events, d_probs, out_start, n, t, nt, s, &a.tail_len) : tail_snapshot(e, &a, s);
    if (launched == VAD_OK) launched = tail_records(e, &a, s);
    return call_end(e, true, s, launched);
}

}  // namespace

extern "C" {

int vad_scan_tails(vad_engine *e, vad_segment *tails_out, int64_t n) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_tails_run(e, "vad_scan_tails", false, nullptr, 1, tails_out, n);
}

int vad_scan_resegment_tails(vad_engine *e, const vad_thresholds *t, int64_t nt, vad_segment *tails_out, int64_t n) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return scan_tails_run(e, "vad_scan_resegment_tails", true, t, nt, tails_out, n);
}

int vad_tails_device(vad_engine *e, const int64_t *slots, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n,
                     vad_segment *d_tails, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return tails_device_run(e, "vad_tails_device", false, slots, d_events, d_probs, out_start, n, nullptr, 1, d_tails, stream);
}

int vad_resegment_tails_device(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n,
                               const vad_thresholds *t, int64_t nt, vad_segment *d_tails, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return tails_device_run(e, "vad_resegment_tails_device", true, nullptr, d_events, d_probs, out_start, n, t, nt, d_tails, stream);
}

}  // extern "C"

// ---- segment tables refined: padded, merged, thinned, split (vad_refine_device, vad_scan_refine) ------------------------------
namespace {

static_assert(sizeof(vad_refine) == 24, "vad_refine layout");

// what both entry points check about the rule and the capacity
int refine_check_rule(vad_engine *e, const char *who, const vad_refine *r, int64_t seg_cap) {
    if (!r) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null rule", who);
    if (r->pad_before < 0 || r->pad_after < 0)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: pad_before = %d, pad_after = %d: a pad is 0 or more frames", who,
                       (int)r->pad_before, (int)r->pad_after);
    if (r->merge_gap < -1)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: merge_gap = %d: -1 (never join) or a gap of 0 or more frames", who,
                       (int)r->merge_gap);
    if (r->max_frames < 0 || r->max_frames == 1)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: max_frames = %d: 0 (no limit) or at least 2 frames", who, (int)r->max_frames);
    if (r->reserved != 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: reserved = %d: must be 0", who, (int)r->reserved);
    if (seg_cap < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: seg_cap = %lld: bad count", who, (long long)seg_cap);
    return VAD_OK;
}

// The first half of a refinement on `s`: out_start (checked: check_positions) goes up as int32 next to the items' first records and
// their counts; then heads, count and prefix - the true count is in *d_nsegs_out behind them.
int refine_count(vad_engine *e, const vadk::SegRecord *d_segs_in, const long long *d_nsegs_in, int64_t in_cap, const vadk::SegRecord *d_tails,
                 const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n, const vad_refine *r, long long *d_nsegs_out,
                 hipStream_t s, vadk::RefineArgs *a) {
    DevTables w{e->d_refine, e->d_refine_cap};
    narrow_positions(e->refine_up, (size_t)n + 1, out_start, n);
    const int k_start = w.add(e->refine_up, (size_t)n + 1), k_first = w.add(nullptr, sizeof(uint32_t) * (size_t)n),
              k_cnt = w.add(nullptr, sizeof(unsigned long long) * (size_t)n);
    if (int rc = w.reserve(e)) return rc;
    if (int rc = w.copy(e, s)) return rc;
    *a = vadk::RefineArgs{};
    a->segs_in = d_segs_in;
    a->nsegs_in = d_nsegs_in;
    a->tails = d_tails;
    a->events = d_events;
    a->probs = d_probs;
    a->out_start = w.at<const int32_t>(k_start);
    a->first = w.at<uint32_t>(k_first);
    a->cnt = w.at<unsigned long long>(k_cnt);
    a->nsegs_out = d_nsegs_out;
    a->in_cap = (uint32_t)in_cap;
    a->n = (int32_t)n;
    a->pad_before = r->pad_before;
    a->pad_after = r->pad_after;
    a->merge_gap = r->merge_gap;
    a->min_frames = r->min_frames;
    a->max_frames = r->max_frames;
    const hipError_t rr = vadk_launch_refine_count(a, s);
    if (rr != hipSuccess) return e->hip_fail(rr, "kernel launch (refine count)");
    return VAD_OK;
}

// ... and the second: the records into d_segs (room for seg_cap of them), their cuts, then - with items - their statistics
int refine_fill(vad_engine *e, vadk::RefineArgs *a, vadk::SegRecord *d_segs, int64_t seg_cap, hipStream_t s) {
    a->segs_out = d_segs;
    a->seg_cap = (uint32_t)std::min<int64_t>(seg_cap, INT32_MAX);
    const hipError_t r = vadk_launch_refine_fill(a, s);
    if (r != hipSuccess) return e->hip_fail(r, "kernel launch (refine fill)");
    if (a->n <= 0) return VAD_OK;
    return seg_stats(e, a->events, a->probs, a->out_start, a->n, d_segs, a->seg_cap, a->nsegs_out, a->seg_cap, s);
}

}  // namespace

extern "C" {

int vad_refine_device(vad_engine *e, const vad_segment *d_segs_in, const int64_t *d_nsegs_in, int64_t in_cap, const vad_segment *d_tails,
                      const uint8_t *d_events, const float *d_probs, const int64_t *out_start, int64_t n, const vad_refine *r,
                      vad_segment *d_segs_out, int64_t seg_cap, int64_t *d_nsegs_out, void *stream) {
    static const char *who = "vad_refine_device";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s;
    if (int rc = call_begin(e, true, stream, &s)) return rc;
    if (int rc = refine_check_rule(e, who, r, seg_cap)) return rc;
    if (n < 0 || in_cap < 0)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: n = %lld, in_cap = %lld: bad count", who, (long long)n, (long long)in_cap);
    if (n > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 items", who);
    if (in_cap > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: more than 2^31 - 1 input records", who);
    if ((n > 0 && !out_start) || !d_nsegs_in || !d_nsegs_out || (in_cap > 0 && !d_segs_in) || (seg_cap > 0 && !d_segs_out))
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    int64_t total = 0;
    if (int rc = check_positions(e, who, out_start, n, &total)) return rc;
    if (int rc = check_device_arrays(e, who, total, d_events, {{d_segs_in, d_tails, d_segs_out}, "the events, the segment tables and the tails"},
                                     {{d_probs}, "probs"}, {{d_nsegs_in, d_nsegs_out}, "the counts"}))
        return rc;
    vadk::RefineArgs a;
    int launched = refine_count(e, reinterpret_cast<const vadk::SegRecord *>(d_segs_in), reinterpret_cast<const long long *>(d_nsegs_in), in_cap,
                                reinterpret_cast<const vadk::SegRecord *>(d_tails), d_events, d_probs, out_start, n, r,
                                reinterpret_cast<long long *>(d_nsegs_out), s, &a);
    if (launched == VAD_OK && seg_cap > 0) launched = refine_fill(e, &a, reinterpret_cast<vadk::SegRecord *>(d_segs_out), seg_cap, s);
    return call_end(e, true, s, launched);
}

int vad_scan_refine(vad_engine *e, const vad_segment *segs_in, int64_t nsegs_in, const vad_segment *tails_in, const vad_refine *r,
                    vad_segment *segs_out, int64_t seg_cap, int64_t *nsegs_out) {
    static const char *who = "vad_scan_refine";
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s;
    if (int rc = call_begin(e, false, nullptr, &s)) return rc;
    if (int rc = refine_check_rule(e, who, r, seg_cap)) return rc;
    if (!nsegs_out || (seg_cap > 0 && !segs_out)) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: null buffer", who);
    if (int rc = check_resident(e, who)) return rc;
    const int64_t n = (int64_t)e->seg_out_start.size() - 1;
    if (segs_in) {
        if (nsegs_in < 0 || nsegs_in > INT32_MAX)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: nsegs_in = %lld: bad count", who, (long long)nsegs_in);
        for (int64_t k = 0; k < nsegs_in; ++k) {
            if (segs_in[k].item < 0 || segs_in[k].item >= n)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: record %lld names item %d: the scan had %lld items", who, (long long)k,
                               (int)segs_in[k].item, (long long)n);
            if (k > 0 && segs_in[k].item < segs_in[k - 1].item)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the items decrease at record %lld (%d after %d)", who, (long long)k,
                               (int)segs_in[k].item, (int)segs_in[k - 1].item);
            if (segs_in[k].nframes < 1)
                return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: record %lld has nframes = %d", who, (long long)k, (int)segs_in[k].nframes);
        }
    } else {
        if (e->segtab_count < 0)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: the engine holds no segment table: no vad_scan_segments has built one", who);
        nsegs_in = e->segtab_count;
    }
    if (n == 0 || e->seg_out_start[(size_t)n] == 0) {       // no frame: every record is clipped away
        *nsegs_out = 0;
        return VAD_OK;
    }
    // the input count and the output count, the table and the tails of a host input, in one engine-owned block
    const long long head[2] = {(long long)nsegs_in, 0};
    DevTables in{e->d_refine_in, e->d_refine_in_cap};
    const int k_head = in.add(head, sizeof head), k_tab = in.add(segs_in, sizeof(vad_segment) * (size_t)(segs_in ? nsegs_in : 0)),
              k_tails = in.add(tails_in, tails_in ? sizeof(vad_segment) * (size_t)n : 0);
    if (int rc = in.reserve(e)) return rc;
    if (int rc = in.copy(e, s)) return rc;
    HIP_TRY(e, hipStreamSynchronize(s));                     // `head` is this frame's, the rest the caller's
    long long *d_count = in.at<long long>(k_head);
    vadk::RefineArgs a;
    if (int rc = call_end(e, false, s, refine_count(e, segs_in ? in.at<const vadk::SegRecord>(k_tab) : e->d_segtab, d_count, nsegs_in,
                                                    in.at<const vadk::SegRecord>(k_tails), e->d_events, e->d_probs, e->seg_out_start.data(), n, r,
                                                    d_count + 1, s, &a)))
        return rc;
    long long count = 0;
    if (int rc = read_back(e, &count, d_count + 1, 1, s)) return rc;
    if (count > INT32_MAX) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: %s: %lld records: more than 2^31 - 1 in one call", who, count);
    // the table is sized by the count that came back, as the replay's is - but there is one count, not one per set
    const int64_t take = std::min<int64_t>(count, seg_cap);
    if (take > 0) {
        if (int rc = ensure(e, e->d_refine_out, e->d_refine_out_cap, sizeof(vadk::SegRecord) * (size_t)take)) return rc;
        if (int rc = refine_fill(e, &a, e->d_refine_out, take, s)) return rc;
        if (int rc = download_records(e, segs_out, e->d_refine_out, take, s)) return rc;
    }
    *nsegs_out = count;
    return VAD_OK;
}

// ---- pipelined host ingest ---------------------------------------------------------------------------------------
int vad_step_submit(vad_engine *e, const int64_t *slots, int64_t n, int32_t T, const void *frames, int fmt, float thr,
                    int64_t *ticket) {
    if (!e || !ticket) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (fmt < VAD_FMT_F32 || fmt > VAD_FMT_ALAW8)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: unknown frame format %d", fmt);
    if (int rc = check_call_size(e, n, T, fmt)) return rc;
    if (n < 1 || !slots || !frames) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: null buffer or bad count");
    vad_engine::PipeBuf &pb = e->pipe[e->next_ticket % vad_engine::PIPE_DEPTH];
    if (pb.busy)
        return e->fail(VAD_ERR_BUSY, "Model prediction failed: %d tickets are outstanding - collect ticket %lld first",
                       vad_engine::PIPE_DEPTH, (long long)pb.ticket);
    if (int rc = check_slots(e, slots, n)) return rc;
    HIP_TRY(e, hipSetDevice(e->device));
    e->scan_results = false;
    if (!pb.copied) {
        HIP_TRY(e, hipEventCreateWithFlags(&pb.copied, hipEventDisableTiming));
        HIP_TRY(e, hipEventCreateWithFlags(&pb.done, hipEventDisableTiming));
        HIP_TRY(e, hipEventCreateWithFlags(&pb.out, hipEventDisableTiming));
    }
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t fb = frame_bytes(e, fmt) * (size_t)n * T;
    const size_t o_probs = up16(sizeof(int32_t) * (size_t)n), o_seg = o_probs + up16(sizeof(float) * (size_t)n * T);
    const size_t o_ev = o_seg + up16(sizeof(int32_t) * (size_t)n), io_bytes = o_ev + up16((size_t)n * T);
    if (int rc = ensure(e, pb.d_frames, pb.d_frames_cap, fb)) return rc;
    if (io_bytes > pb.io_cap) {
        if (pb.d_io) (void)hipFree(pb.d_io);
        if (pb.h_io) (void)hipHostFree(pb.h_io);
        pb.d_io = pb.h_io = nullptr;
        pb.io_cap = 0;
        HIP_TRY(e, hipMalloc((void **)&pb.d_io, io_bytes));
        HIP_TRY(e, hipHostMalloc((void **)&pb.h_io, io_bytes, hipHostMallocDefault));
        pb.io_cap = io_bytes;
    }
    int32_t *hs = reinterpret_cast<int32_t *>(pb.h_io);
    for (int64_t i = 0; i < n; ++i) hs[i] = (int32_t)slots[i];
    // in: slots + frames on the copy-in stream (true DMA when `frames` is page-locked: vad_host_alloc)
    // from the first enqueued copy on, a failure must not leave `copy_in` reading the caller's frames (or this buffer) after
    // the call returned: the error path waits for the copy stream before it reports
    auto fail_after_copy = [&](int rc) {
        (void)hipStreamSynchronize(e->copy_in);
        (void)hipStreamSynchronize(e->stream);
        return rc;
    };
#define HIP_TRY_PIPE(call)                                                          \
    do {                                                                            \
        hipError_t _r = (call);                                                     \
        if (_r != hipSuccess) return fail_after_copy(e->hip_fail(_r, #call));       \
    } while (0)
    HIP_TRY_PIPE(hipMemcpyAsync(pb.d_io, pb.h_io, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, e->copy_in));
    HIP_TRY_PIPE(hipMemcpyAsync(pb.d_frames, frames, fb, hipMemcpyHostToDevice, e->copy_in));
    HIP_TRY_PIPE(hipEventRecord(pb.copied, e->copy_in));
    // compute: after the copy; kernels of successive tickets run in submission order on the engine's stream
    HIP_TRY_PIPE(hipStreamWaitEvent(e->stream, pb.copied, 0));
    vadk::StepParams p = e->base;
    p.slots = reinterpret_cast<const int32_t *>(pb.d_io);
    p.frames = pb.d_frames;
    p.probs = reinterpret_cast<float *>(pb.d_io + o_probs);
    p.seg_frames = reinterpret_cast<int32_t *>(pb.d_io + o_seg);
    p.events = pb.d_io + o_ev;
    p.n = (int32_t)n;
    p.T = T;
    p.fmt = fmt;
    p.thresh = thr;
    if (int rc = launch(e, p, e->stream)) return fail_after_copy(rc);
    HIP_TRY_PIPE(hipEventRecord(pb.done, e->stream));
    // out: probs | seg | events as one block on the copy-out stream
    HIP_TRY_PIPE(hipStreamWaitEvent(e->copy_out, pb.done, 0));
    HIP_TRY_PIPE(hipMemcpyAsync(pb.h_io + o_probs, pb.d_io + o_probs, io_bytes - o_probs, hipMemcpyDeviceToHost, e->copy_out));
    HIP_TRY_PIPE(hipEventRecord(pb.out, e->copy_out));
#undef HIP_TRY_PIPE
    pb.busy = true;
    pb.collecting = false;
    pb.ticket = e->next_ticket;
    pb.n = n;
    pb.T = T;
    *ticket = e->next_ticket++;
    return VAD_OK;
}

int vad_step_collect(vad_engine *e, int64_t ticket, float *probs_out, uint8_t *events_out, int32_t *seg_frames_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    hipEvent_t out_ev = nullptr;
    vad_engine::PipeBuf *pb = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (ticket < 0) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: bad ticket");
        pb = &e->pipe[ticket % vad_engine::PIPE_DEPTH];
        if (!pb->busy || pb->ticket != ticket || pb->collecting)
            return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: ticket %lld is not outstanding", (long long)ticket);
        if (!probs_out) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: probs_out is null");
        pb->collecting = true;         // a second collect of this ticket from another thread is refused, not raced
        out_ev = pb->out;
    }
    // wait WITHOUT the engine's mutex: another thread may submit the next ticket meanwhile (that is the overlap)
    hipError_t r = hipEventSynchronize(out_ev);
    std::lock_guard<std::mutex> lk(e->mu);
    pb->busy = false;
    pb->collecting = false;
    if (r != hipSuccess) return e->hip_fail(r, "hipEventSynchronize(ticket)");
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t n = (size_t)pb->n, T = (size_t)pb->T;
    const size_t o_probs = up16(sizeof(int32_t) * n), o_seg = o_probs + up16(sizeof(float) * n * T), o_ev = o_seg + up16(sizeof(int32_t) * n);
    std::memcpy(probs_out, pb->h_io + o_probs, sizeof(float) * n * T);
    if (seg_frames_out) std::memcpy(seg_frames_out, pb->h_io + o_seg, sizeof(int32_t) * n);
    if (events_out) std::memcpy(events_out, pb->h_io + o_ev, n * T);
    return VAD_OK;
}

}  // extern "C"

// ---- chunks of 8 / 24 / 48 kHz audio resampled to 512 samples at 16 kHz (vad_resample) --------------------------------------
namespace {

// fills one segment descriptor (validates the chunk convention, builds / finds the operator)
int resample_segment(vad_engine *e, const float *d_in, int64_t n, int32_t n_in, int32_t sr_in, float *d_out, vadk::ResampleSeg &sg) {
    const int want = resample_chunk_len(sr_in);
    if (want == 0)
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: supported input rates are 8000, 24000, 48000", sr_in);
    if (n_in != want)
        return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio from %dHz to 16000Hz: a chunk must hold %d samples, got %d", sr_in, want, n_in);
    vad_engine::ResampleOp *op = nullptr;
    if (int rc = get_resample_op(e, n_in, &op)) return rc;
    sg.wstream = op->d_w;
    sg.wstream_bytes = (uint32_t)op->bytes;
    sg.tile_blocks = op->tile_blocks;
    sg.row128_block = op->row128_block;
    sg.in = d_in;
    sg.out = d_out;
    sg.n = (int32_t)n;
    sg.n_in = n_in;
    return VAD_OK;
}

int resample_launch(vad_engine *e, const float *d_in, int64_t n, int32_t n_in, int32_t sr_in, float *d_out, hipStream_t s) {
    vadk::ResampleParams p{};
    if (int rc = resample_segment(e, d_in, n, n_in, sr_in, d_out, p.seg[0])) return rc;
    p.nseg = 1;
    p.tile_start[0] = 0;
    p.tile_start[1] = (int32_t)((n + vadk::MT - 1) / vadk::MT);
    hipError_t r = vadk_launch_resample(&p, s);
    if (r != hipSuccess) return e->hip_fail(r, "resample kernel launch");
    return VAD_OK;
}

}  // namespace

extern "C" {

int vad_resample(vad_engine *e, const float *in, int64_t n, int32_t n_in, int32_t sr_in, float *out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n < 0 || (n > 0 && (!in || !out))) return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: null buffer or bad count");
    if (n == 0) return VAD_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    const size_t ib = sizeof(float) * (size_t)n * n_in, ob = sizeof(float) * (size_t)n * VAD_FRAME_SAMPLES;
    if (resample_chunk_len(sr_in) != n_in)
        return resample_launch(e, nullptr, n, n_in, sr_in, nullptr, e->stream);   // reports the precise error
    if (int rc = ensure(e, e->d_rs_in, e->d_rs_in_cap, ib)) return rc;
    if (int rc = ensure(e, e->d_rs_out, e->d_rs_out_cap, ob)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_rs_in, in, ib, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (int rc = resample_launch(e, e->d_rs_in, n, n_in, sr_in, e->d_rs_out, e->stream)) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, e->d_rs_out, ob, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

int vad_resample_device(vad_engine *e, const float *d_in, int64_t n, int32_t n_in, int32_t sr_in, float *d_out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n < 0 || (n > 0 && (!d_in || !d_out))) return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: null buffer or bad count");
    if (n == 0) return VAD_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    return resample_launch(e, d_in, n, n_in, sr_in, d_out, stream ? static_cast<hipStream_t>(stream) : e->stream);
}

int vad_resample_multi_device(vad_engine *e, int32_t nseg, const float *const *d_in, const int64_t *n, const int32_t *n_in,
                              const int32_t *sr_in, float *const *d_out, void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (nseg < 1 || nseg > vadk::RESAMPLE_MAX_SEGS || !d_in || !n || !n_in || !sr_in || !d_out)
        return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: 1..%d segments, non-null tables", vadk::RESAMPLE_MAX_SEGS);
    HIP_TRY(e, hipSetDevice(e->device));
    vadk::ResampleParams p{};
    int32_t tiles = 0;
    for (int k = 0; k < nseg; ++k) {
        if (n[k] < 0 || (n[k] > 0 && (!d_in[k] || !d_out[k])))
            return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: null buffer or bad count in segment %d", k);
        if (int rc = resample_segment(e, d_in[k], n[k], n_in[k], sr_in[k], d_out[k], p.seg[k])) return rc;
        p.tile_start[k] = tiles;
        tiles += (int32_t)((n[k] + vadk::MT - 1) / vadk::MT);
    }
    p.nseg = nseg;
    p.tile_start[nseg] = tiles;
    hipError_t r = vadk_launch_resample(&p, stream ? static_cast<hipStream_t>(stream) : e->stream);
    if (r != hipSuccess) return e->hip_fail(r, "resample kernel launch");
    return VAD_OK;
}

}  // extern "C"

// ---- AudioUtils.resample_audio for any (length, rates): whole-array Fourier resampling, operator evaluated on the fly -----
namespace {

// which kernel serves a call: the direct one (every operator entry evaluated, O(n_in n_out), lowest latency) below 2^25 entries,
// the chirp-z / FFT one (O(n log n), ~100 launches: 0.2 ms at least) from there - when its lengths allow - which is where the two
// were measured to cross (profiles/r03_resample_generic.jsonl); vad_debug_resample_path pins one
bool rsf_fits(int64_t n_in, int64_t n_out) { return n_in <= vadk::RSF_MAX_LEN && n_out <= vadk::RSF_MAX_LEN; }
bool rsg_use_fft(const vad_engine *e, int64_t rows, int64_t n_in, int64_t n_out) {
    if (e->rsg_path == 1 || !rsf_fits(n_in, n_out)) return false;
    if (e->rsg_path == 2) return true;
    return (unsigned __int128)(rows ? rows : 1) * (unsigned __int128)n_in * (unsigned __int128)n_out >= ((unsigned __int128)1 << 25);
}

int rsg_check(vad_engine *e, int64_t rows, int64_t n_in, int64_t n_out) {
    if (rows < 0 || n_in < 1 || n_out < 1 || n_in > vadk::RSG_MAX_LEN || n_out > vadk::RSG_MAX_LEN)
        return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: rows >= 0 and 1 <= n_in, n_out < 2^31 (rows = %lld, n_in = %lld, n_out = %lld)",
                       (long long)rows, (long long)n_in, (long long)n_out);
    if (rsg_use_fft(e, rows, n_in, n_out)) return VAD_OK;
    const unsigned __int128 entries = (unsigned __int128)(rows ? rows : 1) * (unsigned __int128)n_in * (unsigned __int128)n_out;
    if (entries > (unsigned __int128)vadk::RSG_MAX_ENTRIES)
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio: %lld arrays of %lld -> %lld samples: longer than the FFT path takes (2^25 samples) and "
                       "more than the 2^42 operator entries the direct kernel evaluates per call", (long long)rows, (long long)n_in, (long long)n_out);
    return VAD_OK;
}

// chirp-z / FFT path: tables of the last shape stay on the device; rows are processed in groups that keep a work buffer <= 1 GB
int rsf_run(vad_engine *e, const void *d_in, int in_f64, int64_t rows, int64_t n_in, int64_t n_out, float *d_out, hipStream_t s) {
    auto pow2 = [](int64_t v) { int64_t q = 1; while (q < v) q <<= 1; return q; };
    vad_engine::RsfPlan &pl = e->rsf_plan;
    const int64_t P1 = pow2(2 * n_in), P2 = pow2(2 * n_out), Pmax = std::max(P1, P2);
    const int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>({rows, 65535, (1ll << 26) / Pmax}));
    const size_t need = (size_t)rows_per * (size_t)Pmax * 16;
    if (need > e->d_rsf_cap) {
        HIP_TRY(e, hipStreamSynchronize(s));
        if (e->d_rsf_a) (void)hipFree(e->d_rsf_a);
        if (e->d_rsf_b) (void)hipFree(e->d_rsf_b);
        e->d_rsf_a = e->d_rsf_b = nullptr;
        e->d_rsf_cap = 0;
        HIP_TRY(e, hipMalloc(&e->d_rsf_a, need));
        HIP_TRY(e, hipMalloc(&e->d_rsf_b, need));
        e->d_rsf_cap = need;
    }
    vadk::RsfParams p{};
    p.n_in = n_in; p.n_out = n_out; p.K = std::min(n_in, n_out) / 2;
    p.P1 = P1; p.P2 = P2; p.Pmax = Pmax;
    p.a = e->d_rsf_a; p.b = e->d_rsf_b;
    p.x_f64 = in_f64 ? 1 : 0;
    if (pl.n_in != n_in || pl.n_out != n_out) {
        HIP_TRY(e, hipStreamSynchronize(s));
        for (void **q : {&pl.W1, &pl.W2, &pl.B1, &pl.B2}) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        pl.n_in = pl.n_out = 0;
        HIP_TRY(e, hipMalloc(&pl.W1, (size_t)P1 / 2 * 16));
        HIP_TRY(e, hipMalloc(&pl.W2, (size_t)P2 / 2 * 16));
        HIP_TRY(e, hipMalloc(&pl.B1, (size_t)P1 * 16));
        HIP_TRY(e, hipMalloc(&pl.B2, (size_t)P2 * 16));
        p.W1 = pl.W1; p.W2 = pl.W2; p.B1 = pl.B1; p.B2 = pl.B2;
        p.rows = 1;
        hipError_t r = vadk_rsf_build_tables(&p, s);
        if (r != hipSuccess) return e->hip_fail(r, "resample kernel launch (tables)");
        pl.n_in = n_in; pl.n_out = n_out; pl.P1 = P1; pl.P2 = P2;
    }
    p.W1 = pl.W1; p.W2 = pl.W2; p.B1 = pl.B1; p.B2 = pl.B2;
    const size_t esz = in_f64 ? 8 : 4;
    for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
        p.rows = (int32_t)std::min(rows_per, rows - r0);
        p.x = static_cast<const uint8_t *>(d_in) + (size_t)r0 * (size_t)n_in * esz;
        p.y = d_out + (size_t)r0 * (size_t)n_out;
        hipError_t r = vadk_rsf_run(&p, s);
        if (r != hipSuccess) return e->hip_fail(r, "resample kernel launch");
    }
    return VAD_OK;
}

int rsg_tables(vad_engine *e, int64_t n_in, int64_t n_out, vad_engine::RsgEntry **out) {
    for (auto &c : e->rsg_cache)
        if (c.n_in == n_in && c.n_out == n_out) {
            c.used = ++e->rsg_clock;
            *out = &c;
            return VAD_OK;
        }
    vadk::RsgTables t;
    std::string perr;
    if (!vadk::build_rsg_tables(n_in, n_out, t, perr)) return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: %s", perr.c_str());
    vad_engine::RsgEntry c;
    c.n_in = n_in; c.n_out = n_out; c.a = t.a; c.b = t.b; c.L = t.L; c.P = t.P; c.corrected = t.corrected;
    const size_t bn = t.tn.size() * sizeof(double), bm = t.tm.size() * sizeof(double);
    c.bytes = bn + bm;
    // make room: the least recently used shapes go first
    auto total = [&] { size_t b = 0; for (auto &x : e->rsg_cache) b += x.bytes; return b; };
    while (!e->rsg_cache.empty() && (e->rsg_cache.size() >= vad_engine::RSG_CACHE_ENTRIES || total() + c.bytes > vad_engine::RSG_CACHE_BYTES)) {
        auto lru = std::min_element(e->rsg_cache.begin(), e->rsg_cache.end(), [](const auto &x, const auto &y) { return x.used < y.used; });
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        (void)hipFree(lru->d_tn);
        (void)hipFree(lru->d_tm);
        e->rsg_cache.erase(lru);
    }
    hipError_t r = hipMalloc((void **)&c.d_tn, bn);
    if (r != hipSuccess) return e->hip_fail(r, "hipMalloc(resample tables)");
    r = hipMalloc((void **)&c.d_tm, bm);
    if (r == hipSuccess) r = hipMemcpy(c.d_tn, t.tn.data(), bn, hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(c.d_tm, t.tm.data(), bm, hipMemcpyHostToDevice);
    if (r != hipSuccess) {
        (void)hipFree(c.d_tn);
        if (c.d_tm) (void)hipFree(c.d_tm);
        return e->hip_fail(r, "hipMalloc / hipMemcpy(resample tables)");
    }
    c.used = ++e->rsg_clock;
    e->rsg_cache.push_back(c);
    *out = &e->rsg_cache.back();
    return VAD_OK;
}

// device buffers in, device buffer out; launches cover (rows chunk) x (output range) pieces of at most 2^34 entries each
int rsg_run(vad_engine *e, const void *d_in, int in_f64, int64_t rows, int64_t n_in, int64_t n_out, float *d_out, hipStream_t s) {
    if (rsg_use_fft(e, rows, n_in, n_out)) return rsf_run(e, d_in, in_f64, rows, n_in, n_out, d_out, s);
    vad_engine::RsgEntry *c = nullptr;
    if (int rc = rsg_tables(e, n_in, n_out, &c)) return rc;
    constexpr int64_t BUDGET = 1ll << 34;
    const int64_t tiles_all = (n_out + 63) / 64;
    const int64_t per_tile = n_in * 64;                              // entries of one 64-output tile of one array
    int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>({rows, 65535, BUDGET / std::max<int64_t>(1, per_tile * tiles_all)}));
    int64_t tiles_per = rows_per > 1 ? tiles_all : std::max<int64_t>(1, std::min<int64_t>(tiles_all, BUDGET / per_tile));
    const size_t esz = in_f64 ? 8 : 4;
    for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
        const int64_t rc = std::min(rows_per, rows - r0);
        for (int64_t t0 = 0; t0 < tiles_all; t0 += tiles_per) {
            const int64_t tc = std::min(tiles_per, tiles_all - t0);
            vadk::RsgParams p{};
            p.x = static_cast<const uint8_t *>(d_in) + (size_t)r0 * (size_t)n_in * esz;
            p.y = d_out + (size_t)r0 * (size_t)n_out;
            p.tn = c->d_tn; p.tm = c->d_tm;
            p.n_in = n_in; p.n_out = n_out; p.a = c->a; p.b = c->b; p.L = c->L;
            p.m_begin = t0 * 64;
            p.m_end = std::min(n_out, (t0 + tc) * 64);
            p.rows = (int32_t)rc;
            // enough waves to fill the chip: slices of n per output tile, at least 64 samples each
            int64_t ns = std::max<int64_t>(1, std::min<int64_t>((4096 + tc * rc - 1) / (tc * rc), std::max<int64_t>(1, n_in / 64)));
            const int64_t sl = (n_in + ns - 1) / ns;
            ns = (n_in + sl - 1) / sl;
            p.nslice = (int32_t)ns;
            p.slice_len = (int32_t)sl;
            p.x_f64 = in_f64 ? 1 : 0;
            p.corrected = c->corrected;
            p.peak = (double)(c->P - c->corrected);
            p.inv_n_in = 1.0 / (double)n_in;
            if (int rc2 = ensure(e, e->d_rsg_partial, e->d_rsg_partial_cap, sizeof(double) * (size_t)ns * (size_t)rc * (size_t)(p.m_end - p.m_begin))) {
                return rc2;
            }
            p.partial = e->d_rsg_partial;
            hipError_t r = vadk_launch_rsg_partial(&p, s);
            if (r == hipSuccess) r = vadk_launch_rsg_finish(&p, s);
            if (r != hipSuccess) return e->hip_fail(r, "resample kernel launch");
        }
    }
    return VAD_OK;
}

}  // namespace

extern "C" {

int vad_resample_generic(vad_engine *e, const void *in, int in_f64, int64_t rows, int64_t n_in, int64_t n_out, float *out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = rsg_check(e, rows, n_in, n_out)) return rc;
    if (rows > 0 && (!in || !out)) return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: null buffer");
    if (rows == 0) return VAD_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    const size_t ib = (in_f64 ? 8u : 4u) * (size_t)rows * (size_t)n_in, ob = sizeof(float) * (size_t)rows * (size_t)n_out;
    HIP_TRY(e, hipStreamSynchronize(e->stream));          // the shared partial / staging buffers may still be in use by an earlier call
    if (int rc = ensure(e, e->d_rsg_in, e->d_rsg_in_cap, ib)) return rc;
    if (int rc = ensure(e, e->d_rsg_out, e->d_rsg_out_cap, ob)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_rsg_in, in, ib, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (int rc = rsg_run(e, e->d_rsg_in, in_f64, rows, n_in, n_out, e->d_rsg_out, e->stream)) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, e->d_rsg_out, ob, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

int vad_resample_generic_device(vad_engine *e, const void *d_in, int in_f64, int64_t rows, int64_t n_in, int64_t n_out, float *d_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = rsg_check(e, rows, n_in, n_out)) return rc;
    if (rows > 0 && (!d_in || !d_out)) return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio: null buffer");
    if (rows == 0) return VAD_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (int rc = rsg_run(e, d_in, in_f64, rows, n_in, n_out, d_out, e->stream)) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));          // synchronous: d_out is complete on return
    return VAD_OK;
}

int vad_debug_resample_path(vad_engine *e, int mode) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (mode < 0 || mode > 2) return e->fail(VAD_ERR_INVALID_ARG, "vad_debug_resample_path: 0 = by size, 1 = direct kernel, 2 = FFT path");
    e->rsg_path = mode;
    return VAD_OK;
}

int vad_debug_resample_generic_entries(int64_t n_in, int64_t n_out, int64_t m0, int64_t m1, double *R, size_t r_doubles) {
    g_create_error.clear();
    if (m0 < 0 || m1 < m0 || m1 > n_out || !R || r_doubles < (size_t)(m1 - m0) * (size_t)n_in) {
        g_create_error = "vad_debug_resample_generic_entries: 0 <= m0 <= m1 <= n_out and R must hold (m1 - m0) * n_in doubles";
        return VAD_ERR_INVALID_ARG;
    }
    vadk::RsgTables t;
    std::string perr;
    if (!vadk::build_rsg_tables(n_in, n_out, t, perr)) {
        g_create_error = "vad_debug_resample_generic_entries: " + perr;
        return VAD_ERR_INVALID_ARG;
    }
    for (int64_t m = m0; m < m1; ++m)
        for (int64_t n = 0; n < n_in; ++n) R[(size_t)(m - m0) * (size_t)n_in + (size_t)n] = vadk::rsg_entry(t, m, n);
    return VAD_OK;
}

}  // extern "C"

// ---- one tick for streams at other input rates: resample on the GPU -> model step, chained on the device -----------------
namespace {
int step_rates_enqueue(vad_engine *e, int32_t nseg, const float *const *d_in, const int64_t *n, const int32_t *sr_in,
                       const int32_t *d_slots, float thr, float *d_probs, uint8_t *d_events, int32_t *d_seg, hipStream_t s) {
    if (e->frame_samples != VAD_FRAME_SAMPLES)
        return e->fail(VAD_ERR_UNSUPPORTED, "Model prediction failed: this engine runs an 8 kHz sub-model on %d-sample frames; "
                       "resampled streams need the 16 kHz one", e->frame_samples);
    int64_t total = 0;
    for (int k = 0; k < nseg; ++k) {
        if (n[k] < 0 || (n[k] > 0 && !d_in[k])) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: null buffer or bad count in segment %d", k);
        total += n[k];
    }
    if (int rc = check_call_size(e, total, 1, VAD_FMT_F32)) return rc;
    if (total == 0) return VAD_OK;
    if (!d_probs) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: null buffer");
    // Silero V5, at most 4 096 streams: ONE launch - every 16-stream tile resamples its own chunks into LDS and steps the
    // model from there (silero_v5_t16.hip, RS instantiation); the 16 kHz frames never exist in HBM
    // The tiles walk the segments laid end to end, so a tile may hold the tail of one input rate and the head of the next
    // (it resamples the two parts one after the other): no padding per segment, 4 096 streams in uneven thirds are 256 tiles.
    // The walk order pairs the most expensive prologue (48 kHz, ~20 us) with the cheapest (8 kHz, ~2 us) in the tiles that
    // straddle a boundary: 48 k | 8 k | 24 k | 16 k.
    const int64_t tiles16 = (total + 15) / 16;
    if (e->version == 5 && e->d_wstream16 && !e->shared_gpu && e->tile_policy != 32 && nseg <= vadk::RATE_MAX_SEGS && e->rates_fused &&
        tiles16 <= e->prop.multiProcessorCount) {      // at most one tile per CU: a second round of tiles would cost a whole tile time
        vadk::RateParams rp{};
        int32_t stream0[vadk::RATE_MAX_SEGS], order[vadk::RATE_MAX_SEGS];
        int32_t at = 0, ns = 0;
        for (int k = 0; k < nseg; ++k) {
            stream0[k] = at;
            at += (int32_t)n[k];
            if (n[k] > 0) order[ns++] = k;
        }
        auto rank = [&](int k) { return sr_in[k] == 48000 ? 0 : sr_in[k] == 8000 ? 1 : sr_in[k] == 24000 ? 2 : 3; };
        std::stable_sort(order, order + ns, [&](int a, int b) { return rank(a) < rank(b); });
        int32_t vstart = 0;
        for (int i = 0; i < ns; ++i) {
            const int k = order[i];
            vadk::RateSeg &sg = rp.seg[i];
            if (sr_in[k] == 16000) {
                sg.wstream = nullptr;
                sg.n_in = VAD_FRAME_SAMPLES;
            } else {
                const int want = resample_chunk_len(sr_in[k]);
                if (want == 0)
                    return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: supported input rates are 8000, 16000, 24000, 48000", sr_in[k]);
                vad_engine::ResampleOp *op = nullptr;
                if (int rc = get_resample_op(e, want, &op, true)) return rc;
                sg.wstream = op->d_w;
                sg.wstream_bytes = (uint32_t)op->bytes;
                sg.wave_blocks = op->tile_blocks;
                sg.row128_block = op->row128_block;
                sg.n_in = want;
            }
            sg.in = d_in[k];
            sg.n = (int32_t)n[k];
            sg.stream0 = stream0[k];
            sg.vstart = vstart;
            vstart += (int32_t)n[k];
        }
        rp.nseg = ns;
        rp.total = vstart;
        vadk::StepParams p = params16(e, e->base);
        p.slots = d_slots;
        p.frames = nullptr;
        p.probs = d_probs;
        p.events = d_events;
        p.seg_frames = d_seg;
        p.n = (int32_t)total;
        p.T = 1;
        p.fmt = VAD_FMT_F32;
        p.thresh = thr;
        hipError_t r = vadk_launch_silero_v5_t16_rates(&p, &rp, s);
        if (r != hipSuccess) return e->hip_fail(r, "kernel launch");
        e->steps += 1;
        e->frames += total;
        return VAD_OK;
    }
    // the 16 kHz frames of the tick: [total][512] f32, engine-owned, written by the resampler and read by the model launch
    // right behind it on the same HIP stream - they never leave the GPU
    if (int rc = ensure(e, e->d_rs_out, e->d_rs_out_cap, sizeof(float) * VAD_FRAME_SAMPLES * (size_t)total)) return rc;
    vadk::ResampleParams rp{};
    int32_t tiles = 0, nrs = 0;
    int64_t row = 0;
    for (int k = 0; k < nseg; ++k) {
        float *dst = e->d_rs_out + (size_t)row * VAD_FRAME_SAMPLES;
        row += n[k];
        if (n[k] == 0) continue;
        if (sr_in[k] == 16000) {      // already 16 kHz (AudioUtils.resample_audio returns its input: utils/audio.py:39-40)
            HIP_TRY(e, hipMemcpyAsync(dst, d_in[k], sizeof(float) * VAD_FRAME_SAMPLES * (size_t)n[k], hipMemcpyDeviceToDevice, s));
            continue;
        }
        if (nrs == vadk::RESAMPLE_MAX_SEGS) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: at most %d resampled segments per call", vadk::RESAMPLE_MAX_SEGS);
        if (int rc = resample_segment(e, d_in[k], n[k], resample_chunk_len(sr_in[k]), sr_in[k], dst, rp.seg[nrs])) return rc;
        rp.tile_start[nrs++] = tiles;
        tiles += (int32_t)((n[k] + vadk::MT - 1) / vadk::MT);
    }
    if (nrs) {
        rp.nseg = nrs;
        rp.tile_start[nrs] = tiles;
        hipError_t r = vadk_launch_resample(&rp, s);
        if (r != hipSuccess) return e->hip_fail(r, "resample kernel launch");
    }
    vadk::StepParams p = e->base;
    p.slots = d_slots;
    p.frames = e->d_rs_out;
    p.probs = d_probs;
    p.events = d_events;
    p.seg_frames = d_seg;
    p.n = (int32_t)total;
    p.T = 1;
    p.fmt = VAD_FMT_F32;
    p.thresh = thr;
    return launch(e, p, s);
}
}  // namespace

extern "C" {

int vad_step_rates_device(vad_engine *e, int32_t nseg, const float *const *d_in, const int64_t *n, const int32_t *sr_in,
                          const int32_t *d_slots, float denoise_thresh, float *d_probs, uint8_t *d_events, int32_t *d_seg_frames,
                          void *stream) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (nseg < 1 || nseg > 8 || !d_in || !n || !sr_in) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: 1..8 segments, non-null tables");
    HIP_TRY(e, hipSetDevice(e->device));
    return step_rates_enqueue(e, nseg, d_in, n, sr_in, d_slots, denoise_thresh, d_probs, d_events, d_seg_frames,
                              stream ? static_cast<hipStream_t>(stream) : e->stream);
}

int vad_step_rates(vad_engine *e, int32_t nseg, const float *const *in, const int64_t *n, const int32_t *sr_in, const int64_t *slots,
                   float denoise_thresh, float *probs_out, uint8_t *events_out, int32_t *seg_frames_out) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (nseg < 1 || nseg > 8 || !in || !n || !sr_in || !slots || !probs_out)
        return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: 1..8 segments, non-null tables");
    int64_t total = 0;
    size_t in_floats = 0;
    for (int k = 0; k < nseg; ++k) {
        const int len = sr_in[k] == 16000 ? VAD_FRAME_SAMPLES : resample_chunk_len(sr_in[k]);
        if (len == 0)
            return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: supported input rates are 8000, 16000, 24000, 48000", sr_in[k]);
        if (n[k] < 0 || (n[k] > 0 && !in[k])) return e->fail(VAD_ERR_INVALID_ARG, "Model prediction failed: null buffer or bad count in segment %d", k);
        total += n[k];
        in_floats += (size_t)n[k] * len;
    }
    if (int rc = check_call_size(e, total, 1, VAD_FMT_F32)) return rc;
    if (total == 0) return VAD_OK;
    if (int rc = check_slots(e, slots, total)) return rc;
    HIP_TRY(e, hipSetDevice(e->device));
    e->scan_results = false;
    if (int rc = ensure(e, e->d_rs_in, e->d_rs_in_cap, sizeof(float) * in_floats)) return rc;
    if (int rc = ensure(e, e->d_probs, e->d_probs_cap, sizeof(float) * total)) return rc;
    if (int rc = ensure(e, e->d_events, e->d_events_cap, (size_t)total)) return rc;
    if (int rc = ensure(e, e->d_seg, e->d_seg_cap, sizeof(int32_t) * total)) return rc;
    if (int rc = ensure(e, e->d_slots, e->d_slots_cap, sizeof(int32_t) * total)) return rc;
    std::vector<int32_t> s32((size_t)total);
    for (int64_t i = 0; i < total; ++i) s32[(size_t)i] = (int32_t)slots[i];
    HIP_TRY(e, hipMemcpyAsync(e->d_slots, s32.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice, e->stream));
    const float *d_in[8];
    size_t off = 0;
    for (int k = 0; k < nseg; ++k) {
        const size_t len = sr_in[k] == 16000 ? VAD_FRAME_SAMPLES : (size_t)resample_chunk_len(sr_in[k]);
        d_in[k] = e->d_rs_in + off;
        if (n[k]) HIP_TRY(e, hipMemcpyAsync(e->d_rs_in + off, in[k], sizeof(float) * len * (size_t)n[k], hipMemcpyHostToDevice, e->stream));
        off += len * (size_t)n[k];
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));       // pageable sources must not change under the copies
    if (int rc = step_rates_enqueue(e, nseg, d_in, n, sr_in, e->d_slots, denoise_thresh, e->d_probs, e->d_events, e->d_seg, e->stream)) return rc;
    HIP_TRY(e, hipMemcpyAsync(probs_out, e->d_probs, sizeof(float) * total, hipMemcpyDeviceToHost, e->stream));
    if (events_out) HIP_TRY(e, hipMemcpyAsync(events_out, e->d_events, (size_t)total, hipMemcpyDeviceToHost, e->stream));
    if (seg_frames_out) HIP_TRY(e, hipMemcpyAsync(seg_frames_out, e->d_seg, sizeof(int32_t) * total, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

}  // extern "C"

// ---- tick assembler: the multi-stream caller's side of vad_step_events, in C ---------------------------------------------
namespace {
// per-frame pointers to G.711 codes -> the same frames as int16 in `pcm`, `ptr` pointing at them (a null frame stays null)
void g711_gather_decode(int fmt, const void *const *frames, int64_t n, int32_t nsamples, std::vector<int16_t> &pcm,
                        std::vector<const void *> &ptr) {
    pcm.resize((size_t)n * (size_t)nsamples);
    ptr.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        int16_t *row = pcm.data() + (size_t)i * (size_t)nsamples;
        if (frames[i]) g711_to_i16(fmt, static_cast<const uint8_t *>(frames[i]), (size_t)nsamples, row);
        ptr[(size_t)i] = frames[i] ? row : nullptr;
    }
}

// one frame of `slot` into the staging of the coming tick (tick_mu held).  With `defer` the row is assigned and its address handed
// back in defer->dst, the samples are NOT copied: the caller carries that out later (a batch converting int16 chunks on the copy
// crew); `pending` is then the caller's plan so far - it points into this buffer and is carried out before the buffer moves.
int tick_place(vad_engine *e, int64_t slot, const void *samples, int32_t nsamples, int group, vad_engine::SegCopy *defer = nullptr,
               std::vector<vad_engine::SegCopy> *pending = nullptr) {
    vad_engine::TickBuf &tb = e->tick_buf[e->tick_cur][group];
    const size_t ss = vad_engine::tick_sample_bytes(group);
    const int flen = vad_engine::tick_group_len(group, e->frame_samples);
    const size_t rb = ss * (size_t)flen;
    if (tb.count == tb.cap) {
        const int64_t cap = std::min<int64_t>(e->max_streams, std::max<int64_t>(256, 2 * tb.cap));
        if (cap <= tb.cap) return e->fail(VAD_ERR_INVALID_ARG, "tick: more pending frames than slots");
        if (pending && !pending->empty()) {
            e->copy_crew.run(pending->data(), pending->size());
            pending->clear();
        }
        uint8_t *nh = nullptr;
        hipError_t r = hipSetDevice(e->device);
        if (r == hipSuccess) r = hipHostMalloc((void **)&nh, (size_t)cap * (rb + 3 * sizeof(int32_t)), hipHostMallocDefault);
        if (r != hipSuccess) return e->hip_fail(r, "hipHostMalloc(tick staging)");
        if (tb.count) {
            std::memcpy(nh, tb.h, (size_t)tb.count * rb);
            std::memcpy(nh + (size_t)cap * rb, tb.slots(), sizeof(int32_t) * (size_t)tb.count);
            std::memcpy(nh + (size_t)cap * (rb + sizeof(int32_t)), tb.lens(), sizeof(int32_t) * (size_t)tb.count);
            std::memcpy(nh + (size_t)cap * (rb + 2 * sizeof(int32_t)), tb.epochs(), sizeof(int32_t) * (size_t)tb.count);
        }
        if (tb.h) (void)hipHostFree(tb.h);
        tb.h = nh;
        tb.cap = cap;
        tb.row_bytes = rb;
    }
    // SileroVADModel._prepare_audio_input (core/silero_model.py:464-468): right-zero-pad short frames, truncate long ones
    const size_t take = std::min<size_t>((size_t)nsamples, (size_t)flen) * ss;
    uint8_t *dst = tb.row(tb.count);
    if (defer) defer->dst = dst;
    else std::memcpy(dst, samples, take);
    if (take < rb) std::memset(dst + take, 0, rb - take);
    if (e->tick_segments && nsamples > flen) {                  // the model sees the head; a segment keeps the whole frame
        const uint8_t *src = static_cast<const uint8_t *>(samples);
        e->tick_tails[slot].emplace_back(src + take, src + ss * (size_t)nsamples);
    }
    tb.slots()[tb.count] = (int32_t)slot;
    tb.lens()[tb.count] = nsamples;
    tb.epochs()[tb.count] = e->slot_epoch[(size_t)slot];
    tb.count += 1;
    e->tick_gen[(size_t)slot] = e->tick_generation;
    return VAD_OK;
}

// a frame at the engine's own rate (tick_mu held, arguments checked)
int tick_push_locked(vad_engine *e, int64_t slot, const void *samples, int32_t nsamples, int frame_fmt, int group) {
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    if (e->tick_gen[(size_t)slot] != e->tick_generation) return tick_place(e, slot, samples, nsamples, group);
    // the slot already has its frame of the coming tick: later frames wait their turn (one per tick, submission order)
    auto it = e->tick_overflow.find(slot);
    if (it == e->tick_overflow.end()) {
        it = e->tick_overflow.emplace(slot, std::deque<vad_engine::TickPending>()).first;
        e->tick_overflow_order.push_back(slot);
    }
    auto &q = it->second;
    if (q.size() >= 256) return e->fail(VAD_ERR_BUSY, "tick: slot %lld has 256 frames waiting - is vad_tick_run being called?", (long long)slot);
    const size_t ss = vad_engine::tick_sample_bytes(group);
    const int flen = vad_engine::tick_group_len(group, e->frame_samples);
    const int32_t keep = e->tick_segments ? nsamples : std::min<int32_t>(nsamples, flen);
    const uint8_t *src = static_cast<const uint8_t *>(samples);
    q.push_back(vad_engine::TickPending{std::vector<uint8_t>(src, src + ss * (size_t)keep), nsamples, group});
    return VAD_OK;
}
}  // namespace

extern "C" {

// G.711 frames are decoded here, on the host, on push: they join the VAD_FMT_I16_32768 groups, so the tick's groups, its result
// layout, the segment arena and the WAV payload are what they are for a client that sent the decoded PCM16 itself
int vad_tick_push(vad_engine *e, int64_t slot, const void *samples, int32_t nsamples, int frame_fmt, int gate_on) {
    if (!e) return VAD_ERR_INVALID_ARG;
    if (is_g711(frame_fmt) && samples && nsamples >= 1) {
        thread_local std::vector<int16_t> pcm;
        pcm.resize((size_t)nsamples);
        g711_to_i16(frame_fmt, static_cast<const uint8_t *>(samples), (size_t)nsamples, pcm.data());
        return vad_tick_push(e, slot, pcm.data(), nsamples, VAD_FMT_I16_32768, gate_on);
    }
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (!samples || nsamples < 1 || frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_I16_32768)
        return e->fail(VAD_ERR_INVALID_ARG, "tick: null frame, empty frame or unknown format");
    return tick_push_locked(e, slot, samples, nsamples, frame_fmt, frame_fmt * 2 + (gate_on ? 1 : 0));
}

int vad_tick_push_rate(vad_engine *e, int64_t slot, const void *samples, int32_t nsamples, int frame_fmt, int gate_on, int32_t sr_in) {
    if (!e) return VAD_ERR_INVALID_ARG;
    if (sr_in == e->sample_rate) return vad_tick_push(e, slot, samples, nsamples, frame_fmt, gate_on);
    if (!samples || nsamples < 1 || frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_ALAW8) {
        std::lock_guard<std::mutex> lk(e->tick_mu);
        return e->fail(VAD_ERR_INVALID_ARG, "tick: null frame, empty frame or unknown format");
    }
    if (e->frame_samples != VAD_FRAME_SAMPLES || e->sample_rate != 16000) {
        std::lock_guard<std::mutex> lk(e->tick_mu);
        return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio: resampled streams need a 16 kHz engine");
    }
    const int ri = sr_in == 8000 ? 0 : sr_in == 24000 ? 1 : sr_in == 48000 ? 2 : -1;
    const int group = 6 + 3 * (gate_on ? 1 : 0) + (ri < 0 ? 0 : ri);
    const int want = vad_engine::tick_group_len(group, e->frame_samples);
    if (ri < 0 || nsamples != want) {
        std::lock_guard<std::mutex> lk(e->tick_mu);
        if (ri < 0)
            return e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: supported input rates are 8000, 24000, 48000", sr_in);
        return e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio from %dHz to 16000Hz: a chunk must hold %d samples, got %d", sr_in, want, nsamples);
    }
    // staged as float32 (the resampler's input type): int16 wire frames are scaled here - before the lock - with numpy's true division
    thread_local std::vector<float> cvt;
    const float *src = static_cast<const float *>(samples);
    if (is_g711(frame_fmt)) {
        cvt.resize((size_t)nsamples);
        const int16_t *t = g711_table(frame_fmt);
        const uint8_t *q = static_cast<const uint8_t *>(samples);
        for (int32_t k = 0; k < nsamples; ++k) cvt[(size_t)k] = (float)t[q[k]] / 32768.0f;
        src = cvt.data();
    } else if (frame_fmt != VAD_FMT_F32) {
        cvt.resize((size_t)nsamples);
        const float sc = frame_fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f;
        const int16_t *q = static_cast<const int16_t *>(samples);
        for (int32_t k = 0; k < nsamples; ++k) cvt[(size_t)k] = (float)q[k] / sc;
        src = cvt.data();
    }
    std::lock_guard<std::mutex> lk(e->tick_mu);
    return tick_push_locked(e, slot, src, nsamples, VAD_FMT_F32, group);
}

int vad_tick_enable_segments(vad_engine *e, int on) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    e->tick_segments = on != 0;
    if (e->tick_segments) {
        if (e->seg_state.size() < (size_t)e->max_streams) e->seg_state.resize((size_t)e->max_streams);
        // one block per stream up to 64 MB, touched now; the arena grows by 8 MB chunks after that
        try {
            e->seg_arena.reserve_blocks(std::min<size_t>((size_t)e->max_streams, 2048));
        } catch (const std::bad_alloc &) {
            return e->fail(VAD_ERR_INVALID_ARG, "tick: out of host memory for the segment arena");
        }
        if (e->copy_crew.th.empty()) {
            int want = 3;
            if (const char *v = std::getenv("VAD_TICK_COPY_THREADS")) want = std::max(0, std::min(16, std::atoi(v)));
            const unsigned hw = std::thread::hardware_concurrency();
            if (hw && (int)hw / 2 < want + 1) want = std::max(0, (int)hw / 2 - 1);
            e->copy_crew.start(want);
        }
    }
    return VAD_OK;
}

int vad_tick_take_segment(vad_engine *e, int64_t slot, float *out, int64_t cap, int64_t *nsamples) {
    if (!e || !nsamples) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (slot < 0 || (size_t)slot >= e->seg_state.size()) return e->fail(VAD_ERR_BAD_SLOT, "slot %lld has no segment state", (long long)slot);
    vad_engine::SegAudio &d = e->seg_state[(size_t)slot].done;
    *nsamples = d.samples;
    if (!out) return VAD_OK;                       // size query
    if (cap < d.samples) return e->fail(VAD_ERR_INVALID_ARG, "segment buffer too small (%lld < %lld samples)", (long long)cap, (long long)d.samples);
    d.to_float(out);
    d.clear(e->seg_arena);
    return VAD_OK;
}

int vad_tick_push_many(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int32_t nsamples, int frame_fmt, int gate_on) {
    if (!e || n < 0 || (n > 0 && (!slots || !frames))) return VAD_ERR_INVALID_ARG;
    if (is_g711(frame_fmt) && n > 0 && nsamples >= 1) {
        std::vector<int16_t> pcm((size_t)n * (size_t)nsamples);
        g711_to_i16(frame_fmt, static_cast<const uint8_t *>(frames), pcm.size(), pcm.data());
        return vad_tick_push_many(e, slots, n, pcm.data(), nsamples, VAD_FMT_I16_32768, gate_on);
    }
    std::lock_guard<std::mutex> lk(e->tick_mu);             // one lock for the batch
    if (n > 0 && (nsamples < 1 || frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_I16_32768))
        return e->fail(VAD_ERR_INVALID_ARG, "tick: empty frame or unknown format");
    const size_t stride = (frame_fmt == VAD_FMT_F32 ? 4 : 2) * (size_t)(nsamples > 0 ? nsamples : 0);
    const int group = frame_fmt * 2 + (gate_on ? 1 : 0);
    for (int64_t i = 0; i < n; ++i)
        if (int rc = tick_push_locked(e, slots[i], static_cast<const uint8_t *>(frames) + (size_t)i * stride, nsamples, frame_fmt, group)) return rc;
    return VAD_OK;
}

int vad_tick_push_status(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int32_t nsamples, int frame_fmt, int gate_on,
                         int32_t *status) {
    if (!e || n < 0 || (n > 0 && (!slots || !frames || !status))) return VAD_ERR_INVALID_ARG;
    if (is_g711(frame_fmt) && n > 0 && nsamples >= 1) {
        std::vector<int16_t> pcm((size_t)n * (size_t)nsamples);
        g711_to_i16(frame_fmt, static_cast<const uint8_t *>(frames), pcm.size(), pcm.data());
        return vad_tick_push_status(e, slots, n, pcm.data(), nsamples, VAD_FMT_I16_32768, gate_on, status);
    }
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (n > 0 && (nsamples < 1 || frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_I16_32768))
        return e->fail(VAD_ERR_INVALID_ARG, "tick: empty frame or unknown format");
    const size_t stride = (frame_fmt == VAD_FMT_F32 ? 4 : 2) * (size_t)(nsamples > 0 ? nsamples : 0);
    const int group = frame_fmt * 2 + (gate_on ? 1 : 0);
    int first = VAD_OK;
    for (int64_t i = 0; i < n; ++i) {           // every frame is tried: one full queue or one closed stream does not hold the others back
        status[i] = tick_push_locked(e, slots[i], static_cast<const uint8_t *>(frames) + (size_t)i * stride, nsamples, frame_fmt, group);
        if (status[i] != VAD_OK && first == VAD_OK) first = status[i];
    }
    return first;
}

int vad_tick_push_gather(vad_engine *e, const int64_t *slots, int64_t n, const void *const *frames, int32_t nsamples, int frame_fmt,
                         int gate_on, int32_t *status) {
    if (!e || n < 0 || (n > 0 && (!slots || !frames || !status))) return VAD_ERR_INVALID_ARG;
    if (is_g711(frame_fmt) && n > 0 && nsamples >= 1) {
        std::vector<int16_t> pcm;
        std::vector<const void *> ptr;
        g711_gather_decode(frame_fmt, frames, n, nsamples, pcm, ptr);
        return vad_tick_push_gather(e, slots, n, ptr.data(), nsamples, VAD_FMT_I16_32768, gate_on, status);
    }
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (n > 0 && (nsamples < 1 || frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_I16_32768))
        return e->fail(VAD_ERR_INVALID_ARG, "tick: empty frame or unknown format");
    const int group = frame_fmt * 2 + (gate_on ? 1 : 0);
    int first = VAD_OK;
    for (int64_t i = 0; i < n; ++i) {
        status[i] = frames[i] ? tick_push_locked(e, slots[i], frames[i], nsamples, frame_fmt, group)
                              : e->fail(VAD_ERR_INVALID_ARG, "tick: null frame");
        if (status[i] != VAD_OK && first == VAD_OK) first = status[i];
    }
    return first;
}

int vad_tick_push_rate_gather(vad_engine *e, const int64_t *slots, int64_t n, const void *const *frames, int32_t nsamples, int frame_fmt,
                              int gate_on, int32_t sr_in, int32_t *status) {
    if (!e || n < 0 || (n > 0 && (!slots || !frames || !status))) return VAD_ERR_INVALID_ARG;
    if (sr_in == e->sample_rate) return vad_tick_push_gather(e, slots, n, frames, nsamples, frame_fmt, gate_on, status);
    if (is_g711(frame_fmt) && n > 0 && nsamples >= 1) {     // decoded first, then scaled to float32 like a client's own PCM16
        std::vector<int16_t> pcm;
        std::vector<const void *> ptr;
        g711_gather_decode(frame_fmt, frames, n, nsamples, pcm, ptr);
        return vad_tick_push_rate_gather(e, slots, n, ptr.data(), nsamples, VAD_FMT_I16_32768, gate_on, sr_in, status);
    }
    std::lock_guard<std::mutex> lk(e->tick_mu);             // one lock for the batch
    auto all = [&](int rc) {
        for (int64_t i = 0; i < n; ++i) status[i] = rc;
        return rc;
    };
    if (n == 0) return VAD_OK;
    if (nsamples < 1 || frame_fmt < VAD_FMT_F32 || frame_fmt > VAD_FMT_I16_32768)
        return all(e->fail(VAD_ERR_INVALID_ARG, "tick: empty frame or unknown format"));
    if (e->frame_samples != VAD_FRAME_SAMPLES || e->sample_rate != 16000)
        return all(e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio: resampled streams need a 16 kHz engine"));
    const int ri = sr_in == 8000 ? 0 : sr_in == 24000 ? 1 : sr_in == 48000 ? 2 : -1;
    if (ri < 0)
        return all(e->fail(VAD_ERR_UNSUPPORTED, "Failed to resample audio from %dHz to 16000Hz: supported input rates are 8000, 24000, 48000", sr_in));
    const int group = 6 + 3 * (gate_on ? 1 : 0) + ri;
    const int want = vad_engine::tick_group_len(group, e->frame_samples);
    if (nsamples != want)
        return all(e->fail(VAD_ERR_INVALID_ARG, "Failed to resample audio from %dHz to 16000Hz: a chunk must hold %d samples, got %d", sr_in, want, nsamples));
    // rows are assigned here, under the lock; the chunks themselves - int16 -> float32 is most of this call's time - are converted
    // into their rows by the copy crew once the batch is placed.  A chunk that has to WAIT (its stream already has one in this
    // tick) is converted on the spot into the stream's queue.
    std::vector<float> cvt;
    std::vector<vad_engine::SegCopy> &plan = e->push_copies;
    plan.clear();
    const uint32_t kind = frame_fmt == VAD_FMT_F32 ? 0u : frame_fmt == VAD_FMT_I16_32767 ? 1u : 2u;
    const uint32_t src_bytes = (uint32_t)nsamples * (kind ? 2u : 4u);
    int first = VAD_OK;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t slot = slots[i];
        if (!frames[i]) {
            status[i] = e->fail(VAD_ERR_INVALID_ARG, "tick: null frame");
        } else if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot]) {
            status[i] = e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
        } else if (e->tick_gen[(size_t)slot] != e->tick_generation) {
            vad_engine::SegCopy cp{nullptr, static_cast<const uint8_t *>(frames[i]), src_bytes, kind};
            status[i] = tick_place(e, slot, frames[i], nsamples, group, &cp, &plan);
            if (status[i] == VAD_OK) plan.push_back(cp);
        } else {
            const float *src = static_cast<const float *>(frames[i]);
            if (kind) {
                cvt.resize((size_t)nsamples);
                vad_engine::SegCopy{reinterpret_cast<uint8_t *>(cvt.data()), static_cast<const uint8_t *>(frames[i]), src_bytes, kind}.carry_out();
                src = cvt.data();
            }
            status[i] = tick_push_locked(e, slot, src, nsamples, VAD_FMT_F32, group);
        }
        if (status[i] != VAD_OK && first == VAD_OK) first = status[i];
    }
    e->copy_crew.run(plan.data(), plan.size());
    plan.clear();
    return first;
}

int vad_tick_cancel(vad_engine *e, int64_t slot) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (slot < 0 || slot >= e->max_streams) return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is out of range", (long long)slot);
    tick_forget(e, slot);
    return VAD_OK;
}

int vad_tick_pending(vad_engine *e, int64_t slot, int64_t *frames) {
    if (!e || !frames) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (slot < 0 || slot >= e->max_streams) return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is out of range", (long long)slot);
    auto it = e->tick_overflow.find(slot);
    *frames = (e->tick_gen[(size_t)slot] == e->tick_generation ? 1 : 0) + (it == e->tick_overflow.end() ? 0 : (int64_t)it->second.size());
    return VAD_OK;
}

}  // extern "C"

// ---- a stream's segment audio as bytes: what moves with vad_stream_save when a session changes engines ------------------------
namespace {
struct SegBlobHeader { uint32_t magic, active; uint32_t nruns[3]; uint32_t pad; uint64_t bytes[3]; };
constexpr uint32_t SEG_BLOB_MAGIC = 0x31474553u;       // "SEG1"
}  // namespace

extern "C" {

int vad_tick_segment_save(vad_engine *e, int64_t slot, void *buf, int64_t cap, int64_t *nbytes) {
    if (!e || !nbytes) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (slot < 0 || slot >= e->max_streams) return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is out of range", (long long)slot);
    static const vad_engine::SegState none;
    const vad_engine::SegState &st = (size_t)slot < e->seg_state.size() ? e->seg_state[(size_t)slot] : none;
    const vad_engine::SegAudio *parts[3] = {&st.pre, &st.seg, &st.done};
    SegBlobHeader h{};
    h.magic = SEG_BLOB_MAGIC;
    h.active = st.active ? 1u : 0u;
    size_t total = sizeof h;
    for (int k = 0; k < 3; ++k) {
        h.nruns[k] = (uint32_t)parts[k]->runs.size();
        h.bytes[k] = parts[k]->stored_bytes();
        total += parts[k]->runs.size() * sizeof(vad_engine::SegAudio::Run) + (size_t)h.bytes[k];
    }
    *nbytes = (int64_t)total;
    if (!buf) return VAD_OK;                       // size query
    if (cap < (int64_t)total) return e->fail(VAD_ERR_INVALID_ARG, "segment save buffer too small (%lld < %lld bytes)", (long long)cap, (long long)total);
    uint8_t *o = static_cast<uint8_t *>(buf);
    std::memcpy(o, &h, sizeof h);
    o += sizeof h;
    for (int k = 0; k < 3; ++k) {
        if (!parts[k]->runs.empty()) std::memcpy(o, parts[k]->runs.data(), parts[k]->runs.size() * sizeof(vad_engine::SegAudio::Run));
        o += parts[k]->runs.size() * sizeof(vad_engine::SegAudio::Run);
        parts[k]->for_each_piece([&](const vad_engine::SegAudio::Run &r, const uint8_t *src, size_t cnt) {
            const size_t b = cnt * (vad_engine::SegAudio::is_i16(r.group) ? 2 : 4);
            std::memcpy(o, src, b);
            o += b;
        });
    }
    return VAD_OK;
}

int vad_tick_segment_restore(vad_engine *e, int64_t slot, const void *buf, int64_t nbytes) {
    if (!e || !buf) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    SegBlobHeader h;
    if (nbytes < (int64_t)sizeof h) return e->fail(VAD_ERR_INVALID_ARG, "not a segment save blob (%lld bytes)", (long long)nbytes);
    std::memcpy(&h, buf, sizeof h);
    size_t total = sizeof h;
    for (int k = 0; k < 3; ++k) total += (size_t)h.nruns[k] * sizeof(vad_engine::SegAudio::Run) + (size_t)h.bytes[k];
    if (h.magic != SEG_BLOB_MAGIC || h.active > 1 || (int64_t)total != nbytes) return e->fail(VAD_ERR_INVALID_ARG, "corrupt segment save blob");
    // check the runs against the byte counts before touching the slot
    const uint8_t *p = static_cast<const uint8_t *>(buf) + sizeof h;
    for (int k = 0; k < 3; ++k) {
        size_t want = 0;
        for (uint32_t r = 0; r < h.nruns[k]; ++r) {
            vad_engine::SegAudio::Run run;
            std::memcpy(&run, p + (size_t)r * sizeof run, sizeof run);
            if (run.group < 0 || run.group >= vad_engine::TICK_GROUPS || run.samples < 1) return e->fail(VAD_ERR_INVALID_ARG, "corrupt segment save blob");
            want += (size_t)run.samples * (vad_engine::SegAudio::is_i16(run.group) ? 2 : 4);
        }
        if (want != (size_t)h.bytes[k]) return e->fail(VAD_ERR_INVALID_ARG, "corrupt segment save blob");
        p += (size_t)h.nruns[k] * sizeof(vad_engine::SegAudio::Run) + (size_t)h.bytes[k];
    }
    if (e->seg_state.size() < (size_t)e->max_streams) e->seg_state.resize((size_t)e->max_streams);
    vad_engine::SegState &st = e->seg_state[(size_t)slot];
    st.clear(e->seg_arena);
    st.active = h.active != 0;
    vad_engine::SegAudio *parts[3] = {&st.pre, &st.seg, &st.done};
    p = static_cast<const uint8_t *>(buf) + sizeof h;
    try {
        for (int k = 0; k < 3; ++k) {
            const uint8_t *runs = p, *data = p + (size_t)h.nruns[k] * sizeof(vad_engine::SegAudio::Run);
            for (uint32_t r = 0; r < h.nruns[k]; ++r) {
                vad_engine::SegAudio::Run run;
                std::memcpy(&run, runs + (size_t)r * sizeof run, sizeof run);
                parts[k]->append(e->seg_arena, run.group, run.thr, data, (size_t)run.samples, nullptr);
                data += (size_t)run.samples * (vad_engine::SegAudio::is_i16(run.group) ? 2 : 4);
            }
            p = data;
        }
    } catch (const std::bad_alloc &) {
        st.clear(e->seg_arena);
        return e->fail(VAD_ERR_INVALID_ARG, "tick: out of host memory for the segment arena");
    }
    return VAD_OK;
}

}  // extern "C"

namespace {
// the HIP half of a tick: copies in, launches, results back (mu held).  Fills the result pointers on success.
int tick_execute(vad_engine *e, vad_engine::TickBuf *tbs, float denoise_thresh, vad_tick_result *out, int64_t total, size_t frame_total,
                 size_t o_probs, size_t o_seg, size_t o_ev, size_t o_s32) {
    if (int rc = ensure(e, e->d_tick_frames, e->d_tick_frames_cap, frame_total)) return rc;
    const int32_t *h_s32 = reinterpret_cast<const int32_t *>(e->h_tick_out + o_s32);
    HIP_TRY(e, hipMemcpyAsync(e->d_tick_out + o_s32, h_s32, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, e->stream));
    size_t foff = 0;
    const float *d_rate_in[vad_engine::TICK_GROUPS] = {};
    for (int g = 0; g < vad_engine::TICK_GROUPS; ++g) {        // one launch per (format, gate) group: one in practice
        const int64_t cnt = tbs[g].count;
        if (!cnt) continue;
        const size_t fbytes = (size_t)cnt * tbs[g].row_bytes;
        uint8_t *d_fr = static_cast<uint8_t *>(e->d_tick_frames) + foff;
        HIP_TRY(e, hipMemcpyAsync(d_fr, tbs[g].h, fbytes, hipMemcpyHostToDevice, e->stream));
        foff += (fbytes + 255) & ~(size_t)255;
        if (g >= 6) {               // chunks at another rate: stepped below, all rates of a gate value in one vad_step_rates tick
            d_rate_in[g] = reinterpret_cast<const float *>(d_fr);
            continue;
        }
        vadk::StepParams p = e->base;
        p.slots = reinterpret_cast<const int32_t *>(e->d_tick_out + o_s32) + out->group_start[g];
        p.frames = d_fr;
        p.probs = reinterpret_cast<float *>(e->d_tick_out + o_probs) + out->group_start[g];
        p.seg_frames = reinterpret_cast<int32_t *>(e->d_tick_out + o_seg) + out->group_start[g];
        p.events = e->d_tick_out + o_ev + out->group_start[g];
        p.n = (int32_t)cnt;
        p.T = 1;
        p.fmt = g / 2;
        p.thresh = (g & 1) ? denoise_thresh : -1.0f;
        if (int rc = launch(e, p, e->stream)) return rc;
    }
    for (int gate = 0; gate < 2; ++gate) {
        const int g0 = 6 + 3 * gate;
        const float *seg_in[3];
        int64_t seg_n[3];
        int32_t seg_sr[3];
        int ns = 0;
        for (int ri = 0; ri < 3; ++ri)
            if (tbs[g0 + ri].count) {
                seg_in[ns] = d_rate_in[g0 + ri];
                seg_n[ns] = tbs[g0 + ri].count;
                seg_sr[ns++] = vad_engine::tick_group_rate(g0 + ri);
            }
        if (!ns) continue;
        const int64_t at = out->group_start[g0];               // the gate's rate groups are adjacent in the result arrays
        if (int rc = step_rates_enqueue(e, ns, seg_in, seg_n, seg_sr, reinterpret_cast<const int32_t *>(e->d_tick_out + o_s32) + at,
                                        gate ? denoise_thresh : -1.0f, reinterpret_cast<float *>(e->d_tick_out + o_probs) + at,
                                        e->d_tick_out + o_ev + at, reinterpret_cast<int32_t *>(e->d_tick_out + o_seg) + at, e->stream))
            return rc;
    }
    HIP_TRY(e, hipMemcpyAsync(e->h_tick_out + o_probs, e->d_tick_out + o_probs, o_s32 - o_probs, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}
}  // namespace

extern "C" {

int vad_tick_run(vad_engine *e, float denoise_thresh, vad_tick_result *out) {
    if (!e || !out || out->struct_size < sizeof(vad_tick_result)) return VAD_ERR_INVALID_ARG;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b2) {
        return (float)std::chrono::duration<double, std::micro>(b2 - a).count();
    };
    const auto t0 = now();
    out->host_us[0] = out->host_us[1] = out->host_us[2] = 0.f;
    out->n = 0;
    out->dropped = 0;
    out->staged_next = 0;
    out->slots = nullptr; out->probs = nullptr; out->events = nullptr; out->seg_frames = nullptr; out->nsamples = nullptr;
    for (int g = 0; g < vad_engine::TICK_GROUPS; ++g) { out->group_start[g] = 0; out->group_frames[g] = nullptr; }
    out->group_start[vad_engine::TICK_GROUPS] = 0;
    // `mu` first (lock order), for the whole tick: slots cannot be opened or closed under it
    std::lock_guard<std::mutex> lk(e->mu);
    e->scan_results = false;
    int b;
    vad_engine::TickBuf *tbs;
    {   // swap the staging buffers; every slot that has more frames waiting gets its next one into the new buffer, in the order
        // the slots started waiting; rows whose stream was closed (or closed and reopened) since the push are dropped
        std::lock_guard<std::mutex> tl(e->tick_mu);
        b = e->tick_cur;
        tbs = e->tick_buf[b];
        for (int g = 0; g < vad_engine::TICK_GROUPS; ++g)
            for (int64_t r = 0; r < tbs[g].count;) {
                const int32_t sl = tbs[g].slots()[r];
                if (sl >= 0 && sl < e->max_streams && e->open[(size_t)sl] && tbs[g].epochs()[r] == e->slot_epoch[(size_t)sl]) { ++r; continue; }
                tbs[g].drop_row(r);                            // (close and open forget the slot's tick state, so this is belt and braces)
                out->dropped += 1;
            }
        e->tick_cur ^= 1;
        for (auto &tb : e->tick_buf[e->tick_cur]) tb.count = 0;
        if (++e->tick_generation == 0) {
            std::fill(e->tick_gen.begin(), e->tick_gen.end(), 0u);
            e->tick_generation = 1;
        }
        size_t keep = 0;
        for (size_t k = 0; k < e->tick_overflow_order.size(); ++k) {
            const int64_t sl = e->tick_overflow_order[k];
            auto it = e->tick_overflow.find(sl);
            if (it == e->tick_overflow.end() || it->second.empty()) {
                if (it != e->tick_overflow.end()) e->tick_overflow.erase(it);
                continue;
            }
            vad_engine::TickPending &p = it->second.front();
            if (tick_place(e, sl, p.data.data(), (int32_t)(p.data.size() / vad_engine::tick_sample_bytes(p.group)), p.group) == VAD_OK) {
                vad_engine::TickBuf &nb = e->tick_buf[e->tick_cur][p.group];
                nb.lens()[nb.count - 1] = p.nsamples;
                it->second.pop_front();
                out->staged_next += 1;
            }                                                   // (a failed placement - pinned memory exhausted - leaves the frame waiting)
            if (it->second.empty()) e->tick_overflow.erase(it);
            else e->tick_overflow_order[keep++] = sl;
        }
        e->tick_overflow_order.resize(keep);
    }
    const auto t1 = now();
    out->host_us[0] = us(t0, t1);
    int64_t total = 0;
    size_t frame_total = 0;
    for (int g = 0; g < vad_engine::TICK_GROUPS; ++g) {
        out->group_start[g] = total;
        out->group_frames[g] = tbs[g].count ? tbs[g].h : nullptr;
        total += tbs[g].count;
        frame_total += ((size_t)tbs[g].count * tbs[g].row_bytes + 255) & ~(size_t)255;
    }
    out->group_start[vad_engine::TICK_GROUPS] = total;
    if (total == 0) return VAD_OK;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_probs = up16(sizeof(int64_t) * (size_t)total), o_seg = o_probs + up16(sizeof(float) * (size_t)total);
    const size_t o_ev = o_seg + up16(sizeof(int32_t) * (size_t)total), o_s32 = o_ev + up16((size_t)total);
    const size_t o_len = o_s32 + up16(sizeof(int32_t) * (size_t)total);
    const size_t out_bytes = o_len + up16(sizeof(int32_t) * (size_t)total);
    // a tick that fails from here on has consumed its frames: the tails that belong to them go too, so that the slots' queues
    // stay aligned, and the caller is told which streams lost a frame (slots / nsamples / n are valid on failure, probs is NULL)
    auto lost = [&](int rc) {
        std::lock_guard<std::mutex> tl(e->tick_mu);
        for (int g = 0; g < vad_engine::TICK_GROUPS; ++g) {
            const int flen = vad_engine::tick_group_len(g, e->frame_samples);
            for (int64_t r = 0; r < tbs[g].count; ++r)
                if (tbs[g].lens()[r] > flen) {
                    auto it = e->tick_tails.find(tbs[g].slots()[r]);
                    if (it != e->tick_tails.end() && !it->second.empty()) it->second.pop_front();
                }
        }
        out->probs = nullptr; out->events = nullptr; out->seg_frames = nullptr;
        return rc;
    };
    hipError_t hr = hipSetDevice(e->device);
    if (hr == hipSuccess && out_bytes > e->tick_out_cap) {
        const size_t cap = std::max(out_bytes, (size_t)e->max_streams * 28 + 128);
        if (e->h_tick_out) (void)hipHostFree(e->h_tick_out);
        if (e->d_tick_out) (void)hipFree(e->d_tick_out);
        e->h_tick_out = e->d_tick_out = nullptr;
        e->tick_out_cap = 0;
        hr = hipHostMalloc((void **)&e->h_tick_out, cap, hipHostMallocDefault);
        if (hr == hipSuccess) hr = hipMalloc((void **)&e->d_tick_out, cap);
        if (hr == hipSuccess) e->tick_out_cap = cap;
    }
    if (hr != hipSuccess) return lost(e->hip_fail(hr, "tick: result buffers"));
    int64_t *h_slots = reinterpret_cast<int64_t *>(e->h_tick_out);
    int32_t *h_s32 = reinterpret_cast<int32_t *>(e->h_tick_out + o_s32);
    int32_t *h_len = reinterpret_cast<int32_t *>(e->h_tick_out + o_len);
    for (int g = 0; g < vad_engine::TICK_GROUPS; ++g)
        for (int64_t r = 0; r < tbs[g].count; ++r) {
            const int32_t sl = tbs[g].slots()[r];
            h_slots[out->group_start[g] + r] = sl;
            h_s32[out->group_start[g] + r] = sl;
            h_len[out->group_start[g] + r] = tbs[g].lens()[r];
        }
    out->n = total;
    out->slots = h_slots;
    out->nsamples = h_len;
    if (int rc = tick_execute(e, tbs, denoise_thresh, out, total, frame_total, o_probs, o_seg, o_ev, o_s32)) return lost(rc);
    out->probs = reinterpret_cast<const float *>(e->h_tick_out + o_probs);
    out->seg_frames = reinterpret_cast<const int32_t *>(e->h_tick_out + o_seg);
    out->events = e->h_tick_out + o_ev;
    const auto t2 = now();
    out->host_us[1] = us(t1, t2);
    if (e->tick_segments) {
        // the host half of _process_voice_state, per stepped stream, on the staged audio (kept in its wire format; float32 and
        // the gate of utils/audio.py:117-118 are applied when the finished segment is taken).  This pass decides and PLANS -
        // which buffer a frame goes to, which block and offset - and the copies themselves then run on the copy crew.
        std::lock_guard<std::mutex> tl(e->tick_mu);
        if (e->seg_state.size() < (size_t)e->max_streams) e->seg_state.resize((size_t)e->max_streams);
        std::vector<vad_engine::SegCopy> &plan = e->seg_copies;
        plan.clear();
        std::vector<std::vector<uint8_t>> spent;               // tails whose bytes the plan still points into
        try {
            for (int g = 0; g < vad_engine::TICK_GROUPS; ++g) {
                const int flen = vad_engine::tick_group_len(g, e->frame_samples);
                const size_t ss = vad_engine::tick_sample_bytes(g);
                for (int64_t r = 0; r < tbs[g].count; ++r) {
                    const int64_t i = out->group_start[g] + r;
                    const size_t sl = (size_t)h_slots[i];
                    vad_engine::SegState &st = e->seg_state[sl];
                    const int ev = out->events[i];
                    const bool above = (double)out->probs[i] >= e->h_start_prob[sl];
                    const int32_t L = tbs[g].lens()[r];
                    std::deque<std::vector<uint8_t>> *tails = nullptr;
                    if (L > flen) {
                        auto it = e->tick_tails.find((int64_t)sl);
                        if (it != e->tick_tails.end() && !it->second.empty()) tails = &it->second;
                    }
                    if (ev & VAD_EV_REJECTED) {            // a non-finite frame: as if never pushed (its staged tail is spent)
                        if (tails) tails->pop_front();
                        continue;
                    }
                    if (!st.active && !above) {                                            // idle stream: nothing is kept (:873-874)
                        if (!st.pre.empty()) st.pre.clear(e->seg_arena);
                        if (tails) tails->pop_front();
                        continue;
                    }
                    vad_engine::SegAudio &dst = st.active ? st.seg : st.pre;               // :891 / :838-839
                    dst.append(e->seg_arena, g, denoise_thresh, tbs[g].row(r), (size_t)std::min<int32_t>(L, flen), &plan);
                    if (tails) {
                        spent.push_back(std::move(tails->front()));
                        tails->pop_front();
                        dst.append(e->seg_arena, g, denoise_thresh, spent.back().data(), spent.back().size() / ss, &plan);
                    }
                    if (!st.active) {
                        if (ev & VAD_EV_START) {                                           // :860-869
                            st.active = true;
                            st.seg.swap(st.pre);
                            st.pre.clear(e->seg_arena);
                        }
                    } else if (ev & VAD_EV_END) {                                          // :932-949
                        st.done.clear(e->seg_arena);
                        st.done.swap(st.seg);
                        st.active = false;
                    }
                }
            }
        } catch (const std::bad_alloc &) {
            e->copy_crew.run(plan.data(), plan.size());        // what was planned is consistent; the rest of this tick's audio is lost
            return e->fail(VAD_ERR_INVALID_ARG, "tick: out of host memory for the segment arena");
        }
        e->copy_crew.run(plan.data(), plan.size());
        out->host_us[2] = us(t2, now());
    }
    return VAD_OK;
}

int vad_tick_run_work(vad_engine *e, float denoise_thresh, vad_tick_result *out, vad_tick_work *work) {
    if (!e || !work || work->struct_size < sizeof(vad_tick_work)) return VAD_ERR_INVALID_ARG;
    work->n_work = 0;
    work->work_index = nullptr;
    work->work_kind = nullptr;
    if (work->n_slots < 0 || (work->n_slots > 0 && (!work->last_prob || !work->frames_done || !work->active || !work->continue_cb ||
                                                    !work->continue_payload)))
        return e->fail(VAD_ERR_INVALID_ARG, "vad_tick_run_work: the per-slot arrays are missing");
    if (const int rc = vad_tick_run(e, denoise_thresh, out)) return rc;
    const int64_t n = out->n;
    // one tick at a time per engine (the caller's rule for vad_tick_run): the two vectors belong to this call until the next one
    e->work_index.clear();
    e->work_kind.clear();
    e->work_samples.clear();
    const int64_t first_rate_entry = out->group_start[6];       // chunks at another rate always have their exact length
    for (int64_t k = 0; k < n; ++k) {
        const int64_t sl = out->slots[k];
        if (sl < 0 || sl >= work->n_slots) return e->fail(VAD_ERR_INVALID_ARG, "vad_tick_run_work: slot %lld beyond the caller's arrays (%lld)", (long long)sl, (long long)work->n_slots);
        const uint8_t ev = out->events[k];
        const bool long_frame = k < first_rate_entry && out->nsamples[k] > e->frame_samples;
        if (ev & VAD_EV_REJECTED) {                             // the slot's last_prob / frames_done / active stay as they were
            e->work_index.push_back((int32_t)k);
            e->work_kind.push_back((uint8_t)(VAD_WORK_REJECTED | (long_frame ? VAD_WORK_LONG : 0)));
            e->work_samples.push_back(0);
            continue;
        }
        const bool was = work->active[sl] != 0, started = (ev & VAD_EV_START) != 0, ended = (ev & VAD_EV_END) != 0;
        work->last_prob[sl] = out->probs[k];
        work->frames_done[sl] += 1;
        work->active[sl] = (uint8_t)((was || started) && !ended);
        uint8_t kind = (uint8_t)((started ? VAD_WORK_START : 0) | (ended ? VAD_WORK_END : 0));
        if (was && work->continue_cb[sl]) kind |= (uint8_t)(VAD_WORK_CONTINUE | (work->continue_payload[sl] ? VAD_WORK_PAYLOAD : 0));
        if (long_frame) kind |= VAD_WORK_LONG;
        if (kind) {
            e->work_index.push_back((int32_t)k);
            e->work_kind.push_back(kind);
            e->work_samples.push_back(0);
        }
    }
    {   // the finished segments' lengths (segment assembly on): the caller sizes its payload buffers without a second call
        std::lock_guard<std::mutex> tl(e->tick_mu);
        for (size_t j = 0; j < e->work_kind.size(); ++j)
            if (e->work_kind[j] & VAD_WORK_END) {
                const size_t sl = (size_t)out->slots[e->work_index[j]];
                e->work_samples[j] = sl < e->seg_state.size() ? e->seg_state[sl].done.samples : 0;
            }
    }
    work->n_work = (int64_t)e->work_index.size();
    work->work_index = e->work_index.data();
    work->work_kind = e->work_kind.data();
    work->work_samples = e->work_samples.data();
    return VAD_OK;
}

int vad_tick_take_segment_wav16(vad_engine *e, int64_t slot, int32_t sample_rate, void *out, int64_t cap, int64_t *nbytes) {
    if (!e || !nbytes || sample_rate < 1) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->tick_mu);
    if (slot < 0 || (size_t)slot >= e->seg_state.size()) return e->fail(VAD_ERR_BAD_SLOT, "slot %lld has no segment state", (long long)slot);
    vad_engine::SegAudio &d = e->seg_state[(size_t)slot].done;
    const int64_t ns = d.samples, total = 44 + 2 * ns;
    *nbytes = total;
    if (!out) return VAD_OK;                       // size query
    if (cap < total) return e->fail(VAD_ERR_INVALID_ARG, "WAV buffer too small (%lld < %lld bytes)", (long long)cap, (long long)total);
    uint8_t *o = static_cast<uint8_t *>(out);
    auto put32 = [&](size_t at, uint32_t v) { std::memcpy(o + at, &v, 4); };       // (little-endian host, as everywhere in this file)
    auto put16 = [&](size_t at, uint16_t v) { std::memcpy(o + at, &v, 2); };
    std::memcpy(o, "RIFF", 4); put32(4, (uint32_t)(36 + 2 * ns)); std::memcpy(o + 8, "WAVEfmt ", 8);
    put32(16, 16); put16(20, 1); put16(22, 1); put32(24, (uint32_t)sample_rate); put32(28, (uint32_t)sample_rate * 2u); put16(32, 2); put16(34, 16);
    std::memcpy(o + 36, "data", 4); put32(40, (uint32_t)(2 * ns));
    // every stored run as vad_tick_take_segment hands it over (int16 / its scale as a float32 division, the run's gate), then
    // WAVWriter's conversion - float32 product, clip, truncation toward zero - in ONE pass, no float copy of the segment in between
    int16_t *q = reinterpret_cast<int16_t *>(o + 44);
    auto wav = [](float x) -> int16_t {
        float y = x * 32767.0f;
        y = y < -32768.0f ? -32768.0f : (y > 32767.0f ? 32767.0f : y);
        return (int16_t)y;
    };
    d.for_each_piece([&](const vad_engine::SegAudio::Run &r, const uint8_t *src, size_t cnt) {
        const bool g = vad_engine::SegAudio::gated(r.group);
        const float thr = r.thr;
        if (!vad_engine::SegAudio::is_i16(r.group)) {
            const float *x = reinterpret_cast<const float *>(src);
            if (g) for (size_t k = 0; k < cnt; ++k) q[k] = wav(std::fabs(x[k]) > thr ? x[k] : 0.f);
            else for (size_t k = 0; k < cnt; ++k) q[k] = wav(x[k]);
        } else {
            const float sc = r.group < 4 ? 32767.0f : 32768.0f;
            const int16_t *p16 = reinterpret_cast<const int16_t *>(src);
            if (g) for (size_t k = 0; k < cnt; ++k) { const float x = (float)p16[k] / sc; q[k] = wav(std::fabs(x) > thr ? x : 0.f); }
            else for (size_t k = 0; k < cnt; ++k) q[k] = wav((float)p16[k] / sc);
        }
        q += cnt;
    });
    d.clear(e->seg_arena);
    return VAD_OK;
}

int vad_debug_resample_operator(int32_t n_in, float *R, size_t r_floats) {
    g_create_error.clear();
    if (n_in < 8 || n_in % 8 || !R || r_floats < (size_t)n_in * VAD_FRAME_SAMPLES) {
        g_create_error = "vad_debug_resample_operator: n_in must be a positive multiple of 8 and R must hold 512*n_in floats";
        return VAD_ERR_INVALID_ARG;
    }
    std::vector<float> op;
    vadk::build_resample_operator(n_in, op);
    std::memcpy(R, op.data(), op.size() * sizeof(float));
    return VAD_OK;
}

int vad_debug_pack_resample(int32_t n_in, float *out, size_t out_floats, size_t *n_floats, uint32_t *tile_blocks,
                            uint32_t *row128_block) {
    g_create_error.clear();
    if (n_in < 256 || n_in % 256 || !n_floats || !tile_blocks || !row128_block) {
        g_create_error = "vad_debug_pack_resample: n_in must be a positive multiple of 256";
        return VAD_ERR_INVALID_ARG;
    }
    std::vector<float> packed;
    std::string perr;
    *tile_blocks = vadk::pack_resample_operator(n_in, packed, row128_block, perr);
    if (*tile_blocks == 0) {
        g_create_error = perr;
        return VAD_ERR_INVALID_ARG;
    }
    *n_floats = packed.size();
    if (out) {
        if (out_floats < packed.size()) {
            g_create_error = "vad_debug_pack_resample: output buffer too small";
            return VAD_ERR_INVALID_ARG;
        }
        std::memcpy(out, packed.data(), packed.size() * sizeof(float));
    }
    return VAD_OK;
}

int vad_debug_pack_resample_t16(int32_t n_in, float *out, size_t out_floats, size_t *n_floats, uint32_t *wave_blocks,
                                uint32_t *row128_block) {
    g_create_error.clear();
    if (n_in < 256 || n_in % 256 || !n_floats || !wave_blocks || !row128_block) {
        g_create_error = "vad_debug_pack_resample_t16: n_in must be a positive multiple of 256";
        return VAD_ERR_INVALID_ARG;
    }
    std::vector<float> packed;
    std::string perr;
    *wave_blocks = vadk::pack_resample_operator_t16(n_in, packed, row128_block, perr);
    if (*wave_blocks == 0) {
        g_create_error = perr;
        return VAD_ERR_INVALID_ARG;
    }
    *n_floats = packed.size();
    if (out) {
        if (out_floats < packed.size()) {
            g_create_error = "vad_debug_pack_resample_t16: output buffer too small";
            return VAD_ERR_INVALID_ARG;
        }
        std::memcpy(out, packed.data(), packed.size() * sizeof(float));
    }
    return VAD_OK;
}

int vad_debug_pack_weights(int32_t model_version, const void *weights, size_t weights_len, float *out,
                           size_t out_floats, size_t *n_floats, uint32_t *sect_out) {
    g_create_error.clear();
    vadk::PackedWeights pw;
    std::string perr;
    // model_version 516 / 416: Silero V5 / V4 packed for the 16-stream tile kernels (tests/kernel_model.py models both packings);
    // 5161: the second stream of the 516 packing (PackedWeights::data_x: encoder.0 on bf16 splits), with the same section table;
    // 5162: its third (PackedWeights::data_y: encoder.1 on bf16 splits); 5163: the block range uploaded behind the third
    // (PackedWeights::data_z: encoder.2 and encoder.3 on bf16 splits); 5164: the one behind that (PackedWeights::data_d: the STFT's
    // odd-bin tile on bf16 splits, 16 kHz model only)
    const bool t16 = model_version == 516 || (model_version >= 5161 && model_version <= 5164);
    const bool ok = model_version == 5     ? vadk::pack_silero_v5(weights, weights_len, pw, perr)
                    : t16                  ? vadk::pack_silero_v5_t16(weights, weights_len, pw, perr)
                    : model_version == 4   ? vadk::pack_silero_v4(weights, weights_len, pw, perr)
                    : model_version == 416 ? vadk::pack_silero_v4_t16(weights, weights_len, pw, perr)
                                           : false;
    if (!ok) {
        g_create_error = perr.empty() ? "Failed to load model: model_version must be 4 or 5" : perr;
        return VAD_ERR_BAD_WEIGHTS;
    }
    if (model_version == 5161) pw.data = std::move(pw.data_x);
    if (model_version == 5162) pw.data = std::move(pw.data_y);
    if (model_version == 5163) pw.data = std::move(pw.data_z);
    if (model_version == 5164) pw.data = std::move(pw.data_d);
    if (n_floats) *n_floats = pw.data.size();
    if (sect_out) std::memcpy(sect_out, pw.sect, sizeof pw.sect);
    if (out) {
        if (out_floats < pw.data.size()) {
            g_create_error = "vad_debug_pack_weights: output buffer too small";
            return VAD_ERR_INVALID_ARG;
        }
        std::memcpy(out, pw.data.data(), pw.data.size() * sizeof(float));
    }
    return VAD_OK;
}

int vad_debug_set_tile(vad_engine *e, int32_t streams_per_tile) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (streams_per_tile == -1 || streams_per_tile == -2) {       // vad_step_rates: -1 = resample launch + model launch, -2 = fused (default)
        e->rates_fused = streams_per_tile == -2;
        return VAD_OK;
    }
    if (streams_per_tile == -3 || streams_per_tile == -4) {       // paired 16-stream tiles: -3 = at every size, -4 = never
        e->pair_policy = streams_per_tile == -3 ? 1 : -1;
        return VAD_OK;
    }
    if (streams_per_tile != 0 && streams_per_tile != 16 && streams_per_tile != 32)
        return e->fail(VAD_ERR_INVALID_ARG, "tile: 0 (by batch size), 16 or 32");
    if (streams_per_tile == 16 && !e->d_wstream16)
        return e->fail(VAD_ERR_UNSUPPORTED, "Silero V5's 8 kHz sub-model has no 16-stream tile kernel");
    e->tile_policy = streams_per_tile;
    e->pair_policy = 0;
    return VAD_OK;
}

int vad_debug_sm_replay(vad_engine *e, int64_t slot, const float *probs, int64_t n, uint8_t *events_out,
                        int32_t *seg_frames_out) {
    if (!e || !probs || !events_out || !seg_frames_out || n < 1) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (slot < 0 || slot >= e->max_streams || !e->open[(size_t)slot])
        return e->fail(VAD_ERR_BAD_SLOT, "slot %lld is not an open stream", (long long)slot);
    HIP_TRY(e, hipSetDevice(e->device));
    e->scan_results = false;
    if (int rc = ensure(e, e->d_probs, e->d_probs_cap, sizeof(float) * n)) return rc;
    if (int rc = ensure(e, e->d_events, e->d_events_cap, (size_t)n)) return rc;
    if (int rc = ensure(e, e->d_seg, e->d_seg_cap, sizeof(int32_t) * n)) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_probs, probs, sizeof(float) * n, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, vadk_launch_sm_replay(e->d_sm, (int)slot, e->d_probs, (int)n, e->d_events, e->d_seg, e->stream));
    HIP_TRY(e, hipMemcpyAsync(events_out, e->d_events, (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(seg_frames_out, e->d_seg, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

int vad_host_alloc(vad_engine *e, size_t bytes, void **out) {
    if (!e || !out || bytes == 0) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(e, hipSetDevice(e->device));
    void *p = nullptr;
    HIP_TRY(e, hipHostMalloc(&p, bytes, hipHostMallocDefault));
    e->host_blocks.push_back(p);
    *out = p;
    return VAD_OK;
}

int vad_host_free(vad_engine *e, void *p) {
    if (!e || !p) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    auto it = std::find(e->host_blocks.begin(), e->host_blocks.end(), p);
    if (it == e->host_blocks.end()) return e->fail(VAD_ERR_INVALID_ARG, "vad_host_free: not a block of this engine");
    e->host_blocks.erase(it);
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));      // no copy of ours may still be reading it
    HIP_TRY(e, hipHostFree(p));
    return VAD_OK;
}

int vad_engine_synchronize(vad_engine *e) {
    if (!e) return VAD_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return VAD_OK;
}

}  // extern "C"
