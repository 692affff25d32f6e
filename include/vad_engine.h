/*
 * vad_engine.h — C ABI of the MI355X-native batched Silero-VAD engine.
 *
 * This is the drop-in boundary for ONE hot path of Picurit/cutter-vad: the per-frame model
 * operator and its pre/post steps.  Every entry point cites the reference interface it
 * replaces (paths relative to /root/reference/src/real_time_vad/).  The reference is pure
 * Python over onnxruntime; what it binds today is
 *
 *     ort.InferenceSession(path, sess_options, providers)          core/silero_model.py:321-325
 *     session.run(None, {'input','state','sr'} | {'input','h','c','sr'})   core/silero_model.py:433
 *
 * one 512-sample frame, one stream, batch 1.  The engine keeps that contract per stream and
 * adds the stream-batch axis: n independent streams advance one frame in one launch.
 *
 * Conventions
 *   - plain C, no C++/torch types; all sizes explicit; pointers are host pointers unless
 *     the parameter name starts with d_ (device pointer, same GPU as the engine).
 *   - return value: 0 = VAD_OK, negative = vad_status; the message for the last failure on
 *     an engine is vad_last_error(e); for a failed vad_engine_create it is
 *     vad_last_create_error() (thread-local).
 *   - there is NO CPU fallback: if no HIP device is usable, vad_engine_create fails with
 *     VAD_ERR_NO_DEVICE.
 *   - ownership: the engine owns per-slot recurrent state (h,c) in device HBM and a private
 *     copy of the weights; callers own every buffer they pass, for the duration of the call.
 *   - threading: calls on one engine are serialised by an internal mutex; a slot may appear
 *     at most once per step call (the same rule the reference's per-wrapper lock gives,
 *     core/vad_wrapper.py:560).
 */
#ifndef VAD_ENGINE_H
#define VAD_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VAD_API __attribute__((visibility("default")))
#else
#define VAD_API
#endif

#define VAD_ABI_VERSION 5
#define VAD_FRAME_SAMPLES 512   /* core/silero_model.py:464-468: frames are padded/truncated to 512 (Silero V5 8 kHz engines: 256, see vad_info) */
#define VAD_STATE_FLOATS 256    /* V5: state[2][1][128]; V4: h[2][1][64] then c[2][1][64]  (silero_model.py:391-401) */

typedef enum vad_status {
    VAD_OK = 0,
    VAD_ERR_INVALID_ARG = -1,   /* -> AudioProcessingError / ConfigurationError on the Python side */
    VAD_ERR_NO_DEVICE = -2,     /* no usable HIP device: the product has no CPU path */
    VAD_ERR_BAD_WEIGHTS = -3,   /* -> ModelInitializationError("Failed to load model ...") silero_model.py:330-334 */
    VAD_ERR_HIP = -4,           /* a HIP runtime call failed -> AudioProcessingError("Model prediction failed: ...") :444-447 */
    VAD_ERR_NO_SLOT = -5,       /* stream pool exhausted */
    VAD_ERR_BAD_SLOT = -6,      /* slot not open / out of range / duplicated within one step */
    VAD_ERR_UNSUPPORTED = -7,   /* e.g. an input rate the resampler has no operator for */
    VAD_ERR_BUSY = -8           /* vad_step_submit: every pipeline buffer holds an uncollected ticket */
} vad_status;

typedef enum vad_frame_format {
    VAD_FMT_F32 = 0,            /* float32 in [-1,1]: what VADWrapper.process_audio_data hands down (vad_wrapper.py:598) */
    VAD_FMT_I16_32767 = 1,      /* int16 PCM scaled by 1/32767 (websocket server convention, vad_websocket_server.py:341) */
    VAD_FMT_I16_32768 = 2,      /* int16 PCM scaled by 1/32768 (AudioUtils.pcm_to_float32, utils/audio.py:308) */
    VAD_FMT_ULAW8 = 3,          /* ITU-T G.711 mu-law (RTP PCMU), 1 byte per sample, value = decode(b) / 32768 */
    VAD_FMT_ALAW8 = 4           /* ITU-T G.711 A-law  (RTP PCMA), 1 byte per sample, value = decode(b) / 32768 */
} vad_frame_format;
/* G.711 frames (the wire format of 8 kHz telephony; no reference counterpart - its server takes PCM16 / float32 only,
 * vad_websocket_server.py:326-382): a frame row is frame_samples BYTES.  Every entry point that takes a frame_fmt accepts the two
 * formats, and gives bit for bit what it gives for the decoded int16 samples under VAD_FMT_I16_32768 (every code decodes to an
 * int16, and s / 32768 is exact in float32).  Silero V5's 16-stream kernel decodes in its loader; the other kernels are fed
 * through a small expansion kernel into engine-owned HBM, so the link carries one byte per sample either way.  Device pointers
 * to G.711 frames must be 4-byte aligned (the loader reads four samples as one dword).  The tick assembler decodes on push:
 * G.711 frames join the VAD_FMT_I16_32768 groups (4 / 5) of vad_tick_result, as 16-bit PCM.  The presence of vad_g711_decode is
 * how a caller detects the feature (VAD_ABI_VERSION is unchanged: nothing existing moved).
 * vad_g711_decode: the decoder itself, on the host: in [n] codes -> out [n] int16; VAD_ERR_INVALID_ARG for any other format. */
VAD_API int vad_g711_decode(int frame_fmt, const uint8_t *in, int64_t n, int16_t *out);

/* event bits produced by the per-stream hysteresis state machine (core/silero_model.py:790-949) */
enum { VAD_EV_START = 1, VAD_EV_END = 2, VAD_EV_CONTINUE = 4 };

/* ABI 5: non-finite frames are rejected per stream, inside the step kernels (core/silero_model.py:779 validates every frame
 * before the model; utils/audio.py:227-228).  Applies to every float32 entry point: vad_step*, vad_step_device, vad_step_submit,
 * vad_step_rates*, and float32 frames of vad_tick_push*.  int16 samples are always finite.
 *   - A stream's frame is REJECTED when any sample the model reads is NaN or +-Inf: the 512 samples (Silero V5 8 kHz: 256) after
 *     pad / truncate; vad_step_rates*: any sample of the input chunk (each one reaches the resampled frame).  The check comes
 *     before the denoise gate, so gate on and off give the same verdict.
 *   - A rejected frame gives probs = quiet NaN, events = VAD_EV_REJECTED and no other bit, seg_frames = 0 (for that frame).  The
 *     stream's (h, c) and state machine stay exactly as they were (a byte-equal vad_stream_save blob); in a multi-frame call the
 *     next frame continues from the state after the previous one, as if the rejected frame had not been submitted.
 *   - Other streams of the call are unaffected; the call still returns VAD_OK.
 *   - vad_tick_run reports the entry the same way; the segment assembler skips it entirely (no pre-roll or segment audio, no
 *     state-machine bookkeeping; a long frame's staged tail is dropped); vad_tick_run_work lists it as VAD_WORK_REJECTED.
 *   - Not covered: finite samples so large (|x| above ~1e18) that the model's own arithmetic overflows.  Those give a NaN
 *     probability and DO advance the state; the serving layer's host checks (utils/audio.py) still apply.
 */
#define VAD_EV_REJECTED 0x80

typedef struct vad_engine vad_engine;

/* Replaces SileroVADModel.__init__/_load_model (core/silero_model.py:276-334). */
typedef struct vad_engine_desc {
    uint32_t struct_size;       /* sizeof(vad_engine_desc) */
    int32_t model_version;      /* 4 | 5  (core/config.py:23-26) */
    const void *weights;        /* SVW blob: the tensors of the .onnx file's 16 kHz branch (tools/extract_weights.py) */
    size_t weights_len;
    int32_t device_id;          /* HIP device ordinal; one engine drives one GPU */
    int32_t max_streams;        /* capacity of the per-GPU stream pool (slots) */
    int32_t sample_rate;        /* the graph's `sr` input (core/silero_model.py:491): 16000, or - with the blob of the graph's 8 kHz
                                   sub-model - V4: 8000 / 24000 / 48000 (same 512-sample frames), V5: 8000 (native 8 kHz audio in
                                   256-sample frames: every [512] below reads [vad_info.frame_samples]) */
    uint32_t flags;             /* VAD_ENGINE_* bits */
} vad_engine_desc;
/* Another engine's kernels run on this GPU at the same time (e.g. a Silero V4 and a V5 pool side by side: BASELINE configs[4]).
 * A Silero V5 engine normally serves one-frame calls (and multi-frame calls of <= 4 096 streams) on 16-stream tiles, which spreads
 * them over up to all 256 CUs, two workgroups per CU above 4 096 streams (24.5 us per step for 1 024 streams, 44.5 for 8 192, instead
 * of 44 - 46 us on 32-stream tiles) - and leaves no CU to a co-tenant.  With this flag it keeps to 32-stream tiles: a call of n
 * streams occupies n / 32 CUs and the other engine's workgroups run beside it.  A Silero V4 engine (16-stream tiles) then always
 * places two workgroups on a CU instead of spreading a small call over one CU per tile: n / 32 CUs as well. */
#define VAD_ENGINE_SHARED_GPU 1u

typedef struct vad_info {
    uint32_t struct_size;
    int32_t abi_version;
    int32_t model_version;
    int32_t device_id;
    int32_t max_streams;
    int32_t open_streams;
    int32_t compute_units;
    int32_t streams_per_workgroup;
    int64_t weight_bytes_device;   /* packed weight streams resident in HBM */
    int64_t state_bytes_device;
    int64_t steps;                 /* launches so far (SileroVADModel.prediction_count analogue, silero_model.py:440) */
    int64_t frames;                /* frames processed so far */
    char device_name[64];
    char arch[32];                 /* "gfx950..." */
    int32_t frame_samples;         /* samples per model step: 512 (core/silero_model.py:464-468); 256 for Silero V5's 8 kHz sub-model */
    int32_t sample_rate;           /* the `sr` the engine was created for */
} vad_info;

/* thresholds of one stream's state machine: VADConfig fields core/config.py:54-94 */
typedef struct vad_thresholds {
    double start_probability;   /* vad_start_probability (Python float: compared as double, like the reference) */
    double end_probability;     /* vad_end_probability   */
    double start_ratio;         /* voice_start_ratio (dead logic in the reference, kept: SURVEY a10) */
    double end_ratio;           /* voice_end_ratio */
    int32_t start_frame_count;  /* voice_start_frame_count */
    int32_t end_frame_count;    /* voice_end_frame_count */
} vad_thresholds;

/* ---- lifetime ----------------------------------------------------------------------- */

/* SileroVADModel(model_path, model_version)  core/silero_model.py:276-301 */
VAD_API int vad_engine_create(const vad_engine_desc *desc, vad_engine **out);
/* session release (the reference lets the GC drop the ORT session; vad_wrapper.py:747-762 cleanup) */
VAD_API void vad_engine_destroy(vad_engine *e);
VAD_API const char *vad_last_error(const vad_engine *e);
VAD_API const char *vad_last_create_error(void);
/* SileroVADModel.get_model_info  core/silero_model.py:548-566 */
VAD_API int vad_engine_info(const vad_engine *e, vad_info *info);

/* ---- per-stream recurrent state (ModelState, core/silero_model.py:33-83) ------------- */

/* one VADWrapper/VADProcessor/SileroVADModel per client in the reference
 * (websocket_service/server/vad_websocket_server.py:277) == one slot here */
VAD_API int vad_stream_open(vad_engine *e, int64_t *slot);
/* n streams at once (one device synchronisation for the lot); slots_out [n] */
VAD_API int vad_stream_open_many(vad_engine *e, int64_t n, int64_t *slots_out);
VAD_API int vad_stream_close(vad_engine *e, int64_t slot);
/* SileroVADModel.reset / _reset_states  core/silero_model.py:384-401, 539-546 (also resets the slot's state machine) */
VAD_API int vad_stream_reset(vad_engine *e, const int64_t *slots, int64_t n);
/* ModelState.state / hidden_state+cell_state as ONNX lays them out: 256 floats */
VAD_API int vad_stream_get_state(vad_engine *e, int64_t slot, float *hc);
VAD_API int vad_stream_set_state(vad_engine *e, int64_t slot, const float *hc);
/* VADWrapper.set_thresholds  core/vad_wrapper.py:367-419: values only (validation lives in the host mirror);
 * the counters/history of the slot are NOT reset here - the wrapper calls vad_stream_reset next, as :412-413 does */
VAD_API int vad_stream_set_thresholds(vad_engine *e, int64_t slot, const vad_thresholds *t);
/* the same for n slots in ONE launch: t holds nt = 1 (shared by all) or nt = n (one per slot) entries.  vad_stream_reset,
 * vad_stream_open_many and this call cost one small copy + one kernel + one synchronisation whatever n is (a shared-pool
 * server resets / reconfigures thousands of sessions per tick: websocket_service/server/vad_websocket_server.py:277, 420-470) */
VAD_API int vad_stream_set_thresholds_many(vad_engine *e, const int64_t *slots, int64_t n, const vad_thresholds *t, int64_t nt);
/* Everything a stream is between two frames, as one opaque blob: (h, c) + the state machine's thresholds,
 * counters and history (VAD_STREAM_SAVE_BYTES).  No reference counterpart: the reference processes a chunk's frames
 * one by one and a callback that raises leaves the later frames unprocessed (core/vad_wrapper.py:638-647); the host
 * mirror runs a chunk's frames in ONE launch and uses save / restore to step back to that point.  Also what slot
 * migration between engines / GPUs moves (1 120 B per stream). */
#define VAD_STREAM_SAVE_BYTES 1120
VAD_API int vad_stream_save(vad_engine *e, int64_t slot, void *buf, int64_t cap);
VAD_API int vad_stream_restore(vad_engine *e, int64_t slot, const void *buf, int64_t nbytes);

/* ---- the hot path ------------------------------------------------------------------- */

/*
 * SileroVADModel.predict for n streams at once (core/silero_model.py:403-447):
 *   frames  [n][512] in `frame_fmt`; short frames must be right-zero-padded by the caller
 *           exactly as _prepare_audio_input does (:464-468);
 *   denoise_thresh >= 0 applies AudioUtils.denoise_audio's gate  x if |x| > thresh else 0
 *           (utils/audio.py:117-118; VADProcessor._preprocess_audio_frame core/silero_model.py:782-783);
 *           a negative value disables it (VADConfig.enable_denoising = False);
 *   probs_out [n]: float(outputs[0][0][0]) per stream (:515); state is advanced in place (:533-537).
 * Steps on one slot are applied in call order.
 */
VAD_API int vad_step(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int frame_fmt,
             float denoise_thresh, float *probs_out);

/*
 * Same, plus VADProcessor._process_voice_state (core/silero_model.py:790-949) on the device:
 * events_out[n] receives VAD_EV_* bits per stream for this frame; seg_frames_out[n] (may be NULL)
 * receives, on VAD_EV_END, the finished segment's length in frames (pre-roll included), else 0.
 */
VAD_API int vad_step_events(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int frame_fmt,
                    float denoise_thresh, float *probs_out, uint8_t *events_out, int32_t *seg_frames_out);

/*
 * T consecutive frames per stream in one call (VADWrapper._process_audio_frames' inner loop,
 * core/vad_wrapper.py:632-644): frames [n][T][512], probs_out [n][T], events_out [n][T] or NULL.
 */
VAD_API int vad_step_multi(vad_engine *e, const int64_t *slots, int64_t n, int32_t T, const void *frames, int frame_fmt,
                   float denoise_thresh, float *probs_out, uint8_t *events_out);

/*
 * Device-resident variant of vad_step_events for callers that already hold audio in HBM
 * (bench.py, GPU decode pipelines): every d_* pointer is device memory on the engine's GPU;
 * d_slots may be NULL (= slots 0..n-1); d_events / d_seg_frames may be NULL; `stream` is a
 * hipStream_t (NULL = the engine's own stream).  Asynchronous: returns after enqueueing.
 */
VAD_API int vad_step_device(vad_engine *e, const int32_t *d_slots, int64_t n, const void *d_frames, int frame_fmt,
                    float denoise_thresh, float *d_probs, uint8_t *d_events, int32_t *d_seg_frames, void *stream);
/*
 * The same with T consecutive frames per stream (vad_step_multi on device pointers): d_frames [n][T][frame], d_probs [n][T],
 * d_events [n][T] or NULL, d_seg_frames [n] or NULL (length of the LAST segment that ended inside the call, else 0).
 * Rules for both device entry points:
 *   - d_slots is trusted (it lives on the GPU, the host cannot validate it): every entry must be an OPEN slot of this engine
 *     and must appear AT MOST ONCE per call - a duplicate makes two workgroups read-modify-write the same (h, c) and state
 *     machine, and the result is undefined (the host-pointer entry points check this and return VAD_ERR_BAD_SLOT);
 *   - calls that touch the same slot must be ordered by the caller (same HIP stream, or events between streams);
 *   - one call may address at most 2 GiB of frames (n * T * frame bytes), else VAD_ERR_INVALID_ARG.
 */
VAD_API int vad_step_multi_device(vad_engine *e, const int32_t *d_slots, int64_t n, int32_t T, const void *d_frames,
                                  int frame_fmt, float denoise_thresh, float *d_probs, uint8_t *d_events,
                                  int32_t *d_seg_frames, void *stream);

/*
 * Whole recordings (Silero V5).  n recordings of different lengths lie in ONE block of audio (`audio`, audio_samples samples in
 * `frame_fmt`); recording i is the nsamples samples from sample_offset on and runs on stream `slot`, continuing from that
 * stream's state.  The kernel's loader frames them itself: frame t of a recording = its samples t * hop .. t * hop + frame - 1
 * (frame = vad_info.frame_samples), a trailing part shorter than a frame is dropped (AudioUtils.split_into_frames,
 * utils/audio.py:183).  hop = frame / 2 is that function's framing, hop = frame Silero's own back-to-back one.  Nothing is
 * framed or converted on the host, the block crosses the link once in its wire format, and recordings of different lengths
 * share launches: a stream whose recording has ended is held (its (h, c) and state machine stay exactly as its last frame left
 * them) while the longer ones go on.
 *   Results are CSR: recording i owns the entries out_start[i] .. out_start[i + 1] - 1 of probs_out / events_out /
 * seg_frames_out, and out_start[i + 1] - out_start[i] must equal vad_scan_frame_count(e, nsamples_i, hop), else
 * VAD_ERR_INVALID_ARG.  probs / events mean what they mean in vad_step_multi (a float32 frame with a NaN / Inf sample:
 * VAD_EV_REJECTED, NaN, state untouched); seg_frames_out[k] is the finished segment's length in frames on a VAD_EV_END frame
 * and 0 on every other one - every segment of a recording, not only the last.  Entries outside out_start[0] .. out_start[n]
 * are not written.
 *   VAD_ERR_INVALID_ARG, with a message: hop < 4 or not a multiple of 4; a sample_offset that is not a multiple of 4; a
 * recording that leaves the block; 2 GiB or more of audio in one call (the kernel addresses the block through a 32-bit buffer
 * descriptor); n > max_streams.  VAD_ERR_BAD_SLOT: a slot that is not open, or listed twice.
 *   One launch covers at most a fixed number of frames of every recording (so that no launch occupies a shared GPU for
 * seconds); state travels through device memory between launches as between two vad_step_multi calls, so the results do not
 * depend on that number.  vad_info.steps grows by the number of launches, vad_info.frames by the number of frames.
 *   Silero V4 engines and VAD_ENGINE_SHARED_GPU engines return VAD_ERR_UNSUPPORTED: there is no fallback kernel behind this
 * entry point; frame such recordings on the host and use vad_step_multi.
 *   VAD_ABI_VERSION is unchanged (nothing existing moved): the presence of vad_scan is how a caller detects the feature.
 */
typedef struct vad_scan_item {
    int64_t slot;
    int64_t sample_offset;   /* first sample of the recording in the block; a multiple of 4 */
    int64_t nsamples;
} vad_scan_item;
/* frames of a recording of nsamples samples: nsamples < frame ? 0 : (nsamples - frame) / hop + 1; -1 for a bad argument */
VAD_API int64_t vad_scan_frame_count(const vad_engine *e, int64_t nsamples, int32_t hop);
VAD_API int vad_scan(vad_engine *e, const vad_scan_item *items, int64_t n, const void *audio, int64_t audio_samples, int frame_fmt,
                     int32_t hop, float denoise_thresh, const int64_t *out_start /*[n + 1]*/, float *probs_out,
                     uint8_t *events_out /*or NULL*/, int32_t *seg_frames_out /*or NULL*/);
/*
 * The same on device memory: d_audio (4-byte aligned), d_probs, d_events (or NULL) and d_seg_frames (or NULL) live on the engine's
 * GPU; items and out_start are host arrays (the slots are checked).  Enqueues on `stream` (NULL = the engine's own) and returns;
 * a following vad_scan / vad_scan_device first waits for these launches (they read the engine's item table) - on an event the
 * engine recorded behind them, not on `stream`, which the caller may destroy once its own work has finished.
 */
VAD_API int vad_scan_device(vad_engine *e, const vad_scan_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                            int frame_fmt, int32_t hop, float denoise_thresh, const int64_t *out_start /*[n + 1]*/, float *d_probs,
                            uint8_t *d_events, int32_t *d_seg_frames, void *stream);
/*
 * Whole recordings with interleaved channels (Silero V5): the two-channel call recording - agent left, customer right, samples
 * L0 R0 L1 R1 .. as every WAV reader hands them over ([nsamples, 2]) - scanned as it is, de-interleaved by the kernel's loader.
 * `channels` is 1 or 2 and belongs to the call: the block holds audio_samples SAMPLE FRAMES (one sample of every channel), and
 * sample_offset, nsamples and hop count sample frames too, under vad_scan's rules (offset and hop multiples of 4).  What a stream
 * hears belongs to the item: `channel` = 0 .. channels - 1, or VAD_SCAN_MIX = the mean of the two channels, computed on the decoded
 * float32 values as (L + R) * 0.5f - bit for bit AudioUtils.convert_to_mono's np.mean(x, axis=1) on the decoded array, which is what
 * VADWrapper.process_audio_data makes of such a recording.  The denoise gate and the non-finite check (float32) follow the
 * selection: a NaN in the other channel does not reject a channel-selected stream, +Inf left with -Inf right rejects a mixed one.
 * With channels == 1 either accepted value means the mono samples, and the call is vad_scan.  `reserved` must be 0.
 *   Two items may name the same samples with different channels and different slots: that is how both speakers of a call are
 * scanned - the block crosses the link once, and the two streams sit side by side in a tile, on the same cache lines.
 *   Everything else is vad_scan's: CSR results, held streams, launches, statuses.  VAD_ERR_INVALID_ARG, with a message, also for
 * channels outside {1, 2}, a channel out of range, a non-zero reserved, and 2 GiB or more in audio_samples * channels * bytes
 * per sample.  A refused call writes nothing.  Silero V4 and VAD_ENGINE_SHARED_GPU engines: VAD_ERR_UNSUPPORTED.
 *   vad_scan_channels_device: a block of two channels must be 8-byte aligned (the loader reads a quad of G.711 sample frames as
 * one 8-byte word, wider ones in other formats), else VAD_ERR_INVALID_ARG; one channel: 4 bytes, as vad_scan_device.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_channels is how a caller detects the feature.
 */
#define VAD_SCAN_MIX (-1)
typedef struct vad_scan_ch_item {
    int64_t slot;
    int64_t sample_offset;   /* first sample frame of the recording in the block; a multiple of 4 */
    int64_t nsamples;        /* sample frames */
    int32_t channel;         /* 0 .. channels - 1, or VAD_SCAN_MIX */
    int32_t reserved;        /* 0 */
} vad_scan_ch_item;
VAD_API int vad_scan_channels(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                              int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh, const int64_t *out_start /*[n + 1]*/,
                              float *probs_out, uint8_t *events_out /*or NULL*/, int32_t *seg_frames_out /*or NULL*/);
VAD_API int vad_scan_channels_device(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                     int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh,
                                     const int64_t *out_start /*[n + 1]*/, float *d_probs, uint8_t *d_events, int32_t *d_seg_frames,
                                     void *stream);
/* Diagnostic: frames one launch of vad_scan covers at most; 0 = the default.  Results do not depend on it. */
VAD_API int vad_debug_scan_launch_frames(vad_engine *e, int32_t frames);
/*
 * Whole recordings at another rate than the model's (Silero V5, 16 kHz engine): sr_in = 8000, 24000 or 48000, the rates of
 * vad_step_rates and of the reference's SampleRate.  The block is vad_scan_channels's, in its wire format and AT THE INPUT RATE:
 * nothing is resampled or mixed on the host.  A recording is framed at the input rate, as vad_step_rates' callers frame a stream:
 * chunk t = its sample frames t * hop .. t * hop + chunk - 1 with chunk = 512 * sr_in / 16000 (256 / 768 / 1536) and hop in input
 * sample frames (a positive multiple of 4; AudioUtils.split_into_frames(x, chunk, chunk / 2) is hop = chunk / 2); a tail shorter
 * than a chunk is dropped - vad_scan_rate_frame_count(e, nsamples, sr_in, hop) chunks, -1 for bad arguments.  A kernel decodes and
 * channel-selects each chunk as the scans' loader does (s / 32767 or s / 32768, G.711, (L + R) * 0.5f for VAD_SCAN_MIX) and
 * resamples it to one 512-sample frame with the operator vad_resample applies - byte for byte the frame vad_resample gives for the
 * decoded float32 chunk - and the scan kernel steps the model over those frames.  The denoise gate and the non-finite check
 * (VAD_EV_REJECTED) act on the RESAMPLED frame, where the two-launch form of vad_step_rates has them: a NaN or Inf sample anywhere
 * in a chunk rejects that chunk's frame, state untouched.
 *   Everything that is not about the rate is vad_scan_channels's, under this function's name: items, CSR results (one entry per
 * chunk, seg_frames on every END), the 2 GiB limit, offsets and hops that are multiples of 4, the device block's alignment, slot
 * checks, a refused call writes nothing, the wait for an earlier *_device call's launches.  Results do not depend on
 * vad_debug_scan_launch_frames; the frames of one launch window live in an engine-owned buffer of at most 256 MiB, which may cut
 * the window shorter.  vad_info.steps grows by the model launches, frames by the chunks.
 *   sr_in == 16000 IS vad_scan_channels (AudioUtils.resample_audio returns its input).  Any other rate: VAD_ERR_UNSUPPORTED
 * ("supported input rates are ..").  VAD_ERR_UNSUPPORTED also for engines of the 8 kHz sub-model, Silero V4 and
 * VAD_ENGINE_SHARED_GPU engines.
 *   vad_scan_rate leaves NO block resident: vad_scan_cut(audio = NULL) behind it is refused (positions and hop of a cut count
 * samples at the engine's rate), and so is vad_scan_rate_cut(audio = NULL) - the scan that keeps its block for a cut is
 * vad_scan_rate_segments, below.  (sr_in == 16000: vad_scan_channels's block, as there.)
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_rate is how a caller detects the feature.
 */
VAD_API int64_t vad_scan_rate_frame_count(const vad_engine *e, int64_t nsamples, int32_t sr_in, int32_t hop);
VAD_API int vad_scan_rate(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                          int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                          const int64_t *out_start /*[n + 1]*/, float *probs_out, uint8_t *events_out /*or NULL*/,
                          int32_t *seg_frames_out /*or NULL*/);
VAD_API int vad_scan_rate_device(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                 int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                                 const int64_t *out_start /*[n + 1]*/, float *d_probs, uint8_t *d_events, int32_t *d_seg_frames,
                                 void *stream);

/*
 * The audio of finished segments, cut out of a scanned block: the second pass behind vad_scan / vad_scan_channels.  The
 * reference's product is a segment's audio - VADProcessor._finalize_voice_segment concatenates the segment's processed frames and
 * hands WAVWriter.write_wav_data(...) to voice_end_callback (core/silero_model.py, utils/wav_writer.py:41); the streaming side
 * delivers that through vad_tick_take_segment*, this is the corpus side.  A kernel gathers each listed segment's samples from the
 * block in its wire format, decodes, channel-selects and gates them exactly as the model's loader did - a sample of the payload is
 * bit for bit the float32 the model read: s / 32767 or s / 32768, the G.711 value, (L + R) * 0.5f for VAD_SCAN_MIX, then
 * |x| > denoise_thresh ? x : 0 (denoise_thresh < 0: no gate) - and writes them packed.  Only speech crosses the link back.
 *   A segment: an END event at frame e of a recording with seg_frames L covers the frames first_frame = e - L + 1 .. e; frame t of
 * a recording starts at sample frame sample_offset + t * hop of the block (sample_offset: the RECORDING's, as in its scan item).
 *   layout: VAD_CUT_FRAMES - the L frames back to back, L * frame samples, a sample once per frame that holds it: the bytes of the
 * reference's voice_end payload.  VAD_CUT_RANGE - the sample range once, (L - 1) * hop + frame samples.  vad_cut_samples gives
 * either count (-1: nframes < 1, hop < 4 or not a multiple of 4, an unknown layout).
 *   out_fmt: VAD_CUT_PCM16 - int16, np.clip(x * 32767, -32768, 32767).astype(np.int16): one float32 multiply, the clamp, the
 * conversion toward zero (a WAV payload behind a 44-byte header).  VAD_CUT_F32 - the gated value itself, what
 * vad_tick_take_segment keeps.  Segment i's samples go to out[out_sample .. out_sample + vad_cut_samples(..) - 1]; out holds
 * out_samples samples, and samples outside every segment's range are not written.
 *   audio: the block, as vad_scan_channels takes it (channels = 1: vad_scan's).  vad_scan_cut with audio == NULL cuts the block that
 * this engine's last vad_scan / vad_scan_channels (or vad_scan_cut with an audio) uploaded and that is still in device memory -
 * this is how a corpus crosses the link once.  The engine remembers that block's size in bytes, channel count and frame format;
 * audio_samples, channels and frame_fmt must name them, else - or with no such block - VAD_ERR_INVALID_ARG with a message that says
 * which it was.  With an audio the call uploads it, and it becomes the resident block.
 *   Works on every engine, Silero V4 and VAD_ENGINE_SHARED_GPU included: only vad_info.frame_samples enters, no model kernel
 * runs and no stream is touched.  Like the scans, a call first waits for the launches of an earlier vad_scan*_device /
 * vad_scan_cut_device (they read the engine's tables).
 *   VAD_ERR_INVALID_ARG, each with a message, and nothing is written: layout, out_fmt or frame_fmt out of range; channels outside
 * {1, 2}; hop < 4 or not a multiple of 4; a sample_offset that is negative or not a multiple of 4; first_frame < 0 or nframes < 1; a
 * segment whose last sample frame sample_offset + (first_frame + nframes - 1) * hop + frame exceeds audio_samples; a channel out of
 * range; a non-zero reserved; an out_sample that is negative, not a multiple of 4, or with its segment's samples past
 * out_samples; two segments whose output ranges overlap; a block of 2 GiB or more (a segment of 2^33 samples or more).  n == 0:
 * VAD_OK.  A float32 block with non-finite samples: what VAD_CUT_PCM16 writes for such a sample is unspecified, the call completes
 * normally - the segment table is the caller's.
 *   vad_scan_cut_device: d_audio (4-byte aligned, 8 for two channels) and d_out (16-byte aligned) live on the engine's GPU; enqueues
 * on `stream` (NULL = the engine's own) and returns.
 *   A workgroup of the kernel serves VAD_CUT_WG_SAMPLES consecutive output samples of one segment.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_cut is how a caller detects the feature.
 */
enum { VAD_CUT_FRAMES = 0, VAD_CUT_RANGE = 1 };
enum { VAD_CUT_PCM16 = 0, VAD_CUT_F32 = 1 };
#define VAD_CUT_WG_SAMPLES 4096
typedef struct vad_cut_item {
    int64_t sample_offset;   /* the RECORDING's first sample frame in the block (the scan item's); a multiple of 4 */
    int64_t first_frame;     /* e - L + 1 for an END at frame e with seg_frames L */
    int64_t nframes;         /* L >= 1 */
    int64_t out_sample;      /* first output sample of this segment in out; a multiple of 4 */
    int32_t channel;         /* 0 .. channels - 1, or VAD_SCAN_MIX, as vad_scan_ch_item */
    int32_t reserved;        /* 0 */
} vad_cut_item;
VAD_API int64_t vad_cut_samples(const vad_engine *e, int64_t nframes, int32_t hop, int32_t layout);
VAD_API int vad_scan_cut(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio /*or NULL*/, int64_t audio_samples,
                         int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt,
                         void *out, int64_t out_samples);
VAD_API int vad_scan_cut_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt,
                                void *d_out, int64_t out_samples, void *stream);

/*
 * The segment table of a scan, built on the GPU: what a corpus caller wants of vad_scan / vad_scan_channels is a few segments per
 * recording, not three values per frame.  Kernels read the CSR arrays a scan left in device memory and write one vad_segment per
 * finished segment, packed; only that table crosses the link back.
 *   END rule: flat index k of the CSR arrays is an END iff (events[k] & 0x82) == 0x02 - VAD_EV_END set, VAD_EV_REJECTED clear.  Its
 * item is the last i with out_start[i] <= k (items without frames own no index); with e = k - out_start[i] and L = seg_frames[k] the
 * record holds item = i, first_frame = e - L + 1, nframes = L.  first_frame is negative when the stream entered the recording inside
 * a segment (a slot continued from an earlier call), as cutter_vad_amd.scan.speech_segments reports such a segment.  A segment still
 * open at a recording's last frame has no END and no record in this table; vad_scan_tails (below) reports it, in an array of its own.
 *   Order: ascending k - the caller's item order, then frame order - whatever the GPU's scheduling.
 *   Statistics: over the frames t = max(first_frame, 0) .. e of the item whose events have VAD_EV_REJECTED clear: `counted` is their
 * number, max_prob their maximum, and mean_prob = (float)((double)S / ((double)counted * 0x1p30)) with
 * S = sum of (int64) rint((double)p * 0x1p30) - a fixed-point sum, exact in any order, so the value does not depend on how the
 * kernel strides over a segment.  (counted == 0 needs nframes < 1, which no scan writes: both statistics are 0 then.  An accepted
 * frame whose probability is NaN - see VAD_EV_REJECTED, "not covered" - leaves both unspecified.)
 *   Truncation: the first min(count, seg_cap) records are written, in that order; the true count always.
 *
 * vad_segments_device: the extraction alone.  d_events (16-byte aligned), d_seg_frames and d_probs (4-byte aligned) are the flat CSR
 * arrays on the engine's GPU, as vad_scan_device / vad_scan_channels_device wrote them (all three are needed; the events are read in
 * aligned 16-byte lines, so up to 15 bytes behind the last event are loaded - from the array's own last page - and ignored); out_start is the
 * host array [n + 1] of that call; d_segs (16-byte aligned, room for seg_cap records) and d_nsegs (an int64, 8-byte aligned) live on
 * the GPU too.  Enqueues on `stream` (NULL = the engine's own) and returns.  Works on every engine, Silero V4 and
 * VAD_ENGINE_SHARED_GPU included: no model kernel runs and no stream (slot) is touched.  Like the scans, the call first waits for
 * earlier *_device launches that read the engine's tables (its own copy of out_start is one).
 *   VAD_ERR_INVALID_ARG, each with a message, and nothing is written: n < 0 or seg_cap < 0; a null out_start with n > 0; a null
 * d_nsegs; a null d_events, d_seg_frames or d_probs when there are frames; a null d_segs with seg_cap > 0; an out_start that starts
 * below 0 or decreases; out_start[n] > 2^31 - 1; a misaligned pointer.  out_start[n] == 0 (or n == 0): VAD_OK, *d_nsegs = 0.
 *
 * vad_scan_segments: vad_scan_channels (channels = 1: vad_scan) without its per-frame results.  Every check, refusal and message of
 * vad_scan_channels applies, under this function's name; Silero V4 and VAD_ENGINE_SHARED_GPU engines: VAD_ERR_UNSUPPORTED.  Further
 * VAD_ERR_INVALID_ARG: seg_cap < 0, a null nsegs_out, a null segs_out with seg_cap > 0.  The call uploads the block, runs the scan's
 * launches, then the extraction on the engine's own arrays (items in the order given, out_start = the running sum of
 * vad_scan_frame_count), and copies back the count and the first min(count, seg_cap) records: no per-frame array reaches the host.
 * Streams are left as the scan leaves them, vad_info counts the same launches and frames, and the block stays resident:
 * vad_scan_cut(audio = NULL) works behind it.
 *   Lifetime of the table: the WHOLE table (all `count` records, not seg_cap) stays in device memory until this engine's next
 * vad_scan_segments that passes its checks; vad_scan_segments_read copies the records [first, first + count) of it - a caller whose
 * seg_cap was too small reads the rest without scanning again.  VAD_ERR_INVALID_ARG with a message when the engine holds no table,
 * for a negative first or count, a range that leaves the table, or a null out with count > 0.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_segments is how a caller detects the feature.
 */
typedef struct vad_segment {
    int32_t item;        /* index into the call's items */
    int32_t first_frame; /* e - L + 1; may be negative when the stream entered the recording inside a segment */
    int32_t nframes;     /* L */
    int32_t counted;     /* frames that entered the two statistics */
    float   mean_prob;
    float   max_prob;
} vad_segment;
VAD_API int vad_segments_device(vad_engine *e, const uint8_t *d_events, const int32_t *d_seg_frames, const float *d_probs,
                                const int64_t *out_start /*host [n + 1]*/, int64_t n, vad_segment *d_segs, int64_t seg_cap,
                                int64_t *d_nsegs /*on the GPU*/, void *stream);
VAD_API int vad_scan_segments(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                              int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh, vad_segment *segs_out, int64_t seg_cap,
                              int64_t *nsegs_out);
VAD_API int vad_scan_segments_read(vad_engine *e, int64_t first, int64_t count, vad_segment *out);

/*
 * Segment tables and segment audio for recordings at 8 / 24 / 48 kHz: vad_scan_segments and vad_scan_cut behind vad_scan_rate.
 * Positions, lengths and hop count sample frames at sr_in throughout; a frame of a recording is a chunk of 512 * sr_in / 16000
 * sample frames (256 / 768 / 1536), chunk t of a recording the sample frames sample_offset + t * hop .. + chunk - 1.
 *
 * vad_scan_rate_segments: vad_scan_rate without its per-frame results, exactly as vad_scan_segments is to vad_scan_channels.  Every
 * check, refusal and message of vad_scan_rate applies, under this function's name, and vad_scan_segments's further ones (seg_cap
 * < 0, a null nsegs_out, a null segs_out with seg_cap > 0).  The call uploads the block, runs the rate scan's launches into the
 * engine's own arrays, then the extraction (items in the order given, out_start = the running sum of vad_scan_rate_frame_count),
 * and copies back the count and the first min(count, seg_cap) records; first_frame and nframes count chunks, the statistics
 * follow the vad_segment rule, and the whole table stays in device memory for vad_scan_segments_read.  Streams, vad_info.steps and
 * vad_info.frames are left as vad_scan_rate leaves them.  sr_in == 16000 IS vad_scan_segments.
 *   The block stays resident AS A RATE BLOCK: the engine remembers its size in bytes, channel count, frame format and sr_in, and
 * only vad_scan_rate_cut(audio = NULL) naming the same four accepts it; vad_scan_cut(audio = NULL) behind it is refused as with
 * no resident block.  The two kinds of resident block share one buffer and exclude each other: whatever uploads a block (any
 * scan or cut of host audio) replaces the other kind - or, as vad_scan_rate does, leaves none.
 *
 * vad_scan_rate_cut / vad_scan_rate_cut_device: vad_scan_cut / vad_scan_cut_device for such a block.  vad_cut_item is unchanged;
 * first_frame and nframes count chunks.
 *   VAD_CUT_FRAMES: the frames the model read - the reference's voice_end payload for such a recording.  Each of the segment's
 * nframes chunks is decoded and channel-selected as the scans' loader does, resampled to 512 samples by the operator vad_resample
 * applies (byte for byte vad_resample of the decoded float32 chunk, as in vad_scan_rate), then gated on the RESAMPLED value
 * (|x| > denoise_thresh ? x : 0; denoise_thresh < 0: no gate) where the rate scan's model launch gates; the frames are written
 * back to back, nframes * 512 samples at 16 kHz.
 *   VAD_CUT_RANGE: the segment's own audio at the INPUT rate, once: (nframes - 1) * hop + chunk samples, decoded and
 * channel-selected, and NOT gated, whatever denoise_thresh says - the model gated resampled frames, no input-rate sample was ever
 * gated.
 *   vad_rate_cut_samples gives either count (-1: nframes < 1, hop < 4 or not a multiple of 4, an unknown layout or rate;
 * sr_in == 16000: vad_cut_samples).  out_fmt, out_sample, the non-overlap of the output ranges, the alignment rules, audio == NULL
 * (the resident RATE block; a refusal says which of rate, format, channels and size differs), "with an audio the call uploads
 * it, and it becomes the resident (rate) block", "a refused call writes nothing", non-finite float32 input (an unspecified
 * payload, the call completes) and the wait for earlier *_device launches are vad_scan_cut's; so are the checks, each before the
 * first write, with the chunk as the frame in the block-bounds check.  VAD_ERR_UNSUPPORTED: a rate outside 8000 / 16000 / 24000 /
 * 48000, and an engine of an 8 kHz sub-model (whose frames are not the 512 samples the operator writes), with vad_scan_rate's
 * messages.  sr_in == 16000 IS vad_scan_cut / vad_scan_cut_device.
 *   Works on Silero V4 and VAD_ENGINE_SHARED_GPU engines (at 16 kHz) as well: no model kernel runs, no stream is touched, and
 * every engine holds the resample operators vad_resample uses.
 *   VAD_CUT_FRAMES goes through an engine-owned window of at most 256 MiB of resampled frames (131 072 of them); a larger call is
 * served window by window, with the same bytes.  vad_debug_scan_launch_frames(f > 0) cuts the window to 32 * f frames (tests).
 *   vad_scan_rate_cut_device enqueues on `stream` (NULL = the engine's own) and returns, like vad_scan_cut_device; its launches
 * read the engine's tables and window buffer, so the next scan, cut or extraction waits for them.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_rate_segments / vad_scan_rate_cut is how a caller detects the feature.
 */
VAD_API int vad_scan_rate_segments(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                                   int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                                   vad_segment *segs_out, int64_t seg_cap, int64_t *nsegs_out);
VAD_API int64_t vad_rate_cut_samples(const vad_engine *e, int64_t nframes, int32_t sr_in, int32_t hop, int32_t layout);
VAD_API int vad_scan_rate_cut(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio /*or NULL*/, int64_t audio_samples,
                              int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout,
                              int32_t out_fmt, void *out, int64_t out_samples);
VAD_API int vad_scan_rate_cut_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                     int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, int32_t layout,
                                     int32_t out_fmt, void *d_out, int64_t out_samples, void *stream);

/*
 * Segment tables at other thresholds, without running the model again.  The model's output does not depend on the six values of
 * vad_thresholds: the state machine runs behind the probability head and never feeds back into (h, c).  The per-frame probabilities
 * a scan left in device memory therefore answer every other setting, and these calls replay them through the state machine under
 * up to VAD_RESEGMENT_MAX_SETS sets at once, on the GPU: nothing is uploaded but the sets, no model kernel runs, no stream (slot)
 * is touched.  A threshold sweep over an archive is one scan plus one replay.
 *   Replay rule, the same for every set k in 0 .. nt - 1 and every item i: start from the state machine of a stream that was just
 * opened and then given t[k] (vad_stream_open, vad_stream_set_thresholds: the defaults with the six values written into them);
 * walk the item's flat indices out_start[i] .. out_start[i + 1] - 1 in order; a frame whose event byte has VAD_EV_REJECTED set is
 * skipped as the model kernels skip it (no step of the state machine), every other frame is one step on probs[index].  Of the
 * events only the REJECTED bit is read - the START / END / CONTINUE bits of the scan's own thresholds are ignored, and seg_frames
 * is not needed.  Each END at frame e with length L gives one vad_segment {item = i, first_frame = e - L + 1, nframes = L} whose
 * counted, mean_prob and max_prob follow the vad_segment rule to the bit.
 *   Every recording starts from a FRESH state machine here, also where the scan itself continued its slots from an earlier call:
 * the table of set k is, byte for byte, what vad_scan_segments (or vad_scan_rate_segments) returns for the same items on freshly
 * reset streams whose thresholds are t[k] - same records, same order, same statistics - so first_frame is never negative.
 *   Order: by set, then item, then frame.  set_start[k] is the number of records of the sets before k and set_start[nt] the total:
 * always the true counts.  The first min(total, seg_cap) records of that order are written; a caller that wants exact room calls
 * once with seg_cap = 0 and again with the total (the replay is cheap: no second resident table is kept, and
 * vad_scan_segments_read's table is not touched).
 *   Left alone: the streams and their (h, c), vad_info.steps and vad_info.frames, the resident block of either kind
 * (vad_scan_cut / vad_scan_rate_cut with audio = NULL work on any of the new tables), the resident segment table.
 *
 * vad_resegment_device: the replay on device pointers - d_events (16-byte aligned) and d_probs (4-byte aligned) as a *_device scan
 * wrote them, out_start the host array [n + 1] of that call, d_segs (16-byte aligned, room for seg_cap records) and d_set_start
 * (int64 [nt + 1], 8-byte aligned) on the GPU.  Enqueues on `stream` (NULL = the engine's own) and returns.  Works on every engine,
 * Silero V4, VAD_ENGINE_SHARED_GPU and the 8 kHz sub-models included.  Like the scans, the call first waits for earlier *_device
 * launches that read the engine's tables, and the next such call waits for this one's.
 *   VAD_ERR_INVALID_ARG, each with a message, and nothing is written: nt < 1 or nt > VAD_RESEGMENT_MAX_SETS (the kernel puts a
 * recording's sets in one wave); seg_cap < 0; a null t; n < 0; n * nt > 2^31 - 1; a null out_start with n > 0; a null d_set_start;
 * a null d_segs with seg_cap > 0; an out_start that starts below 0 or decreases; out_start[n] > 2^31 - 1; a null d_events or
 * d_probs when there are frames; a misaligned pointer.  (A total above 2^31 - 1 records cannot be known before the launches here:
 * set_start is true all the same, and no record at a position of 2^31 - 1 or above is written.)
 *
 * vad_scan_resegment: the same on the per-frame results that this engine's last vad_scan_segments / vad_scan_rate_segments left in
 * its own arrays, for the items of that call in their order; segs_out, seg_cap and set_start_out [nt + 1] are host memory.  The
 * engine marks those arrays as a scan's results when such a call succeeds (one without frames included: every count is 0) and
 * drops the mark in whatever writes or reallocates them - vad_step and its kin, vad_scan / vad_scan_channels / vad_scan_rate,
 * vad_step_rates, vad_tick_run, vad_step_submit, vad_debug_sm_replay, a failed vad_scan_segments.  Without the mark:
 * VAD_ERR_INVALID_ARG, "vad_scan_resegment: no scan results are resident".  Further VAD_ERR_INVALID_ARG, each with a message and
 * nothing written: nt, seg_cap and t as above, a null set_start_out, a null segs_out with seg_cap > 0, a total above 2^31 - 1 records.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_resegment is how a caller detects the feature.
 */
#define VAD_RESEGMENT_MAX_SETS 64
VAD_API int vad_resegment_device(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start /*host [n + 1]*/,
                                 int64_t n, const vad_thresholds *t, int64_t nt, vad_segment *d_segs, int64_t seg_cap,
                                 int64_t *d_set_start /*on the GPU, [nt + 1]*/, void *stream);
VAD_API int vad_scan_resegment(vad_engine *e, const vad_thresholds *t, int64_t nt, vad_segment *segs_out, int64_t seg_cap,
                               int64_t *set_start_out /*[nt + 1]*/);

/*
 * Tails: the segment still open at a recording's last frame.  An END needs voice_end_frame_count low frames (50 by default: 0.8 s at
 * a hop of 256 samples), so a recording that stops sooner behind its last word has no END for it and the tables above do not list
 * it.  That is right for a stream, which may go on; a scan is handed finished recordings.  The length of an open segment includes
 * the frames buffered before its START, which only the state machine knows - so the engine reports it: one vad_segment per item, in
 * an array of its own.  Tails never enter a segment table: no table of the calls above changes by a byte.
 *   Definition.  Item i has nf frames; S is its stream's state machine behind the last of them.  The item has a tail iff nf >= 1,
 * S.active is set and L = S.seg_frames >= 1.  The record is then {item = i, first_frame = nf - L, nframes = L} - the END formula
 * e - L + 1 with e = nf - 1; first_frame is negative when the slot entered the recording inside a segment - and counted, mean_prob
 * and max_prob follow the vad_segment rule over the frames max(first_frame, 0) .. nf - 1: the fixed-point sum, rejected frames left
 * out, both statistics 0 when counted == 0.  No tail: all 24 bytes of the record are zero (nframes == 0 says so).
 *   In a replay S is the fresh state machine of set k stepped over the item's accepted frames (vad_scan_resegment's rule), and
 * entry [k * n + i] is the tail of set k, item i.
 *
 * vad_scan_tails: the tails of this engine's last vad_scan_segments / vad_scan_rate_segments, tails_out [n] in host memory, n = that
 * call's item count.  The scan itself saves each item's length in an engine-owned array - one small launch behind its model
 * launches, which is no model launch: vad_info.steps and vad_info.frames count what they counted - so vad_stream_reset, _close,
 * _restore or _set_thresholds behind the scan do not change the answer.  Needs the mark of vad_scan_resegment (without it:
 * VAD_ERR_INVALID_ARG, "vad_scan_tails: no scan results are resident"); further VAD_ERR_INVALID_ARG, nothing written: n is not the
 * scan's item count; a null tails_out with n > 0.  Touches no stream, not the table of vad_scan_segments_read, not
 * vad_scan_resegment's, not the resident block: vad_scan_cut(audio = NULL) cuts a tail like any other record.
 *
 * vad_scan_resegment_tails: the tails under nt other threshold sets, tails_out [nt * n]; the mark, n and tails_out as above, t and
 * nt as vad_scan_resegment checks them.
 *
 * vad_tails_device: the tails of the items a *_device scan ran on `slots` (host [n], the items' streams in item order; checked as
 * the scans check them: open, none twice - VAD_ERR_BAD_SLOT).  d_events (16-byte aligned) and d_probs as that scan wrote them,
 * out_start its host array [n + 1], d_tails (16-byte aligned, [n]) on the GPU.  The launch reads the slots' state machines when it
 * runs on `stream` (NULL = the engine's own): enqueue it behind the scan and before anything else that steps those streams.
 * vad_resegment_tails_device: the replay form, d_tails [nt * n]; its checks are vad_resegment_device's (no seg_cap, d_segs or
 * d_set_start here; a null d_tails with n > 0 is refused).  Both work on every engine - Silero V4, VAD_ENGINE_SHARED_GPU and the
 * 8 kHz sub-models included: no model kernel runs - both wait for earlier *_device launches as the scans do, and the next such call
 * waits for theirs.  A refused call writes nothing.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_tails is how a caller detects the feature.
 */
VAD_API int vad_scan_tails(vad_engine *e, vad_segment *tails_out /*[n]*/, int64_t n);
VAD_API int vad_scan_resegment_tails(vad_engine *e, const vad_thresholds *t, int64_t nt, vad_segment *tails_out /*[nt * n]*/, int64_t n);
VAD_API int vad_tails_device(vad_engine *e, const int64_t *slots /*host [n]*/, const uint8_t *d_events, const float *d_probs,
                             const int64_t *out_start /*host [n + 1]*/, int64_t n, vad_segment *d_tails /*on the GPU, [n]*/, void *stream);
VAD_API int vad_resegment_tails_device(vad_engine *e, const uint8_t *d_events, const float *d_probs, const int64_t *out_start /*host [n + 1]*/,
                                       int64_t n, const vad_thresholds *t, int64_t nt, vad_segment *d_tails /*on the GPU, [nt * n]*/,
                                       void *stream);

/*
 * Refinement: a segment table padded, merged, thinned and split for what reads it - an ASR model, a dataset cutter - on the GPU,
 * where the per-frame probabilities that decide a split still are.  The tables above are the raw output of the reference's hysteresis
 * state machine; this pass is what Silero's get_speech_timestamps has as speech_pad_ms, min_silence_duration_ms,
 * min_speech_duration_ms and max_speech_duration_s.  No model kernel runs and no stream (slot) is touched; only the refined table
 * crosses the link.
 *   All counts are frames, as in every table; hop and frame length turn them into samples.  Per item i with
 * nf = out_start[i + 1] - out_start[i] frames, take the item's input records in table order; if tails are given and
 * tails[i].nframes > 0, the item's tail (its first_frame and nframes; entry i belongs to item i) follows as its last record.
 *   1. Clip.  [s, e) = [max(first_frame, 0), min(first_frame + nframes, nf)).  A record with item outside 0 .. n - 1, nframes < 1 or
 *      s >= e is treated as absent.
 *   2. Merge.  Record b joins its predecessor a of the same item iff merge_gap >= 0 and s_b - e_a <= merge_gap.  The rule is pairwise
 *      and local, so chains join transitively and - with merge_gap >= 0 - overlapping records always join.  A group is
 *      [s of its first record, e of its last record).
 *   3. Drop.  A group with e - s < min_frames is removed - and one with e - s < 1, which needs records of an item out of frame order.
 *   4. Pad.  For a surviving group s' = max(s - pad_before, 0) and e' = min(e + pad_after, nf), except between a neighbouring pair of
 *      surviving groups of one item whose gap g = s_next - e_cur < pad_before + pad_after: g <= 0 gives no padding on that side of
 *      either; otherwise the earlier group gets a = floor(g * pad_after / (pad_before + pad_after)) frames behind it and the later one
 *      g - a in front (the product in 64 bits).  Then a <= pad_after, g - a <= pad_before, and the two records touch and never overlap.
 *   5. Split, when max_frames > 0 and len = e' - s' > max_frames: k = ceil(len / max_frames) pieces, sz = ceil(len / k),
 *      h = (max_frames - sz) / 2 rounded down; for j = 1 .. k - 1 the nominal cut is c_j = s' + floor(j * len / k), and boundary b_j is
 *      the frame t of [c_j - h, c_j + h] with the smallest probability among the frames whose event byte has VAD_EV_REJECTED clear,
 *      the lowest t of equals; b_j = c_j where every frame of the window is rejected.  The probabilities of accepted frames are taken
 *      to have the sign bit clear, as every kernel of this engine writes them; a caller's own d_probs with negative values or -0.0
 *      orders them by bit pattern, that is above every non-negative value.  Piece j is [b_j, b_{j+1}) with b_0 = s' and
 *      b_k = e'.  Every piece has 1 .. max_frames frames and the windows of neighbouring boundaries never meet (checked by brute
 *      force for max_frames 2 .. 79 and every len up to 8 * max_frames + 2, every boundary at either end of its window; the
 *      test-suite repeats it).
 *   6. Output.  One vad_segment {item, first_frame, nframes} per piece, in item order, then in the order the groups were formed;
 *      counted, mean_prob and max_prob follow the vad_segment rule over the new range, the fixed-point sum included.  Truncation as
 *      everywhere: the first min(count, seg_cap) records are written, the true count always.
 * The neutral rule {0, 0, -1, 0, 0, 0} returns a table that is byte-equal to its input, for tables whose records lie inside their items.
 *   "The item's records": in a table sorted by item - every table of the calls above, and every table vad_scan_refine accepts - all
 * records that name the item.  The device form cannot look at a table that lives on the GPU before it launches, so it takes the
 * item's FIRST RUN: the records from the first one that names the item and follows one that does not (or opens the table) up to
 * the next record of another item value, in range or not.  Later records that name the item again are treated as absent.  No
 * table content makes a kernel read or write outside the arrays it was given.
 *
 * vad_refine_device: on device pointers.  d_segs_in (16-byte aligned, in_cap records) and d_nsegs_in (an int64, 8-byte aligned) as
 * vad_segments_device wrote them: the first min(*d_nsegs_in, in_cap) records are read.  d_tails: NULL, or n records (16-byte aligned)
 * as vad_tails_device wrote them.  d_events (16-byte aligned) and d_probs (4-byte aligned) as a *_device scan wrote them, out_start
 * its host array [n + 1].  d_segs_out (16-byte aligned, room for seg_cap records, no part of an input) and d_nsegs_out (int64,
 * 8-byte aligned) on the GPU.  Enqueues on `stream` (NULL = the engine's own) and returns.  Works on every engine - Silero V4,
 * VAD_ENGINE_SHARED_GPU and the 8 kHz sub-models included; waits for earlier *_device launches as the scans do, and the next such
 * call waits for this one's.
 *   VAD_ERR_INVALID_ARG, each with a message, and nothing is written: a null r; a negative pad_before or pad_after; merge_gap < -1;
 * max_frames of 1 or negative; reserved != 0; n < 0, in_cap < 0 or seg_cap < 0; n or in_cap above 2^31 - 1; a null out_start with
 * n > 0; a null d_nsegs_in or d_nsegs_out; a null d_segs_in with in_cap > 0; a null d_segs_out with seg_cap > 0; an out_start that
 * starts below 0 or decreases; out_start[n] > 2^31 - 1; a null d_events or d_probs when there are frames; a misaligned pointer.
 * n == 0: VAD_OK, *d_nsegs_out = 0.
 *
 * vad_scan_refine: the same on the per-frame results that this engine's last vad_scan_segments / vad_scan_rate_segments left in its
 * own arrays, for the items of that call.  segs_in: a host table of nsegs_in records - a set of vad_scan_resegment's, one set per
 * call, or any other - or NULL: the resident table of that scan (nsegs_in is then not read).  tails_in: NULL, or the host array
 * [n] of vad_scan_tails / one set of vad_scan_resegment_tails.  segs_out (room for seg_cap records) and nsegs_out are host memory.
 * Needs the mark of vad_scan_resegment; without it VAD_ERR_INVALID_ARG, "vad_scan_refine: no scan results are resident".  A host
 * table is checked before anything is written: nsegs_in >= 0 and at most 2^31 - 1, items in 0 .. n - 1 and not decreasing,
 * nframes >= 1.  Further VAD_ERR_INVALID_ARG, each with a message and nothing written: the rule as above; seg_cap < 0; a null
 * nsegs_out; a null segs_out with seg_cap > 0; a null segs_in with nsegs_in > 0 is the resident table, never an error; more than
 * 2^31 - 1 output records.  Touches no stream, not the resident table, not the tails, not vad_scan_resegment's table and not the
 * resident block: vad_scan_cut(audio = NULL) cuts refined records like any others.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_refine is how a caller detects the feature.
 */
typedef struct vad_refine {
    int32_t pad_before;  /* frames added in front of a segment, >= 0 */
    int32_t pad_after;   /* frames added behind it, >= 0 */
    int32_t merge_gap;   /* join neighbours of an item whose gap is <= this many frames; -1: never join */
    int32_t min_frames;  /* drop joined segments shorter than this (before padding); <= 1: keep all */
    int32_t max_frames;  /* 0: no limit; otherwise >= 2: no output record is longer */
    int32_t reserved;    /* 0 */
} vad_refine;
VAD_API int vad_refine_device(vad_engine *e, const vad_segment *d_segs_in, const int64_t *d_nsegs_in /*on the GPU*/, int64_t in_cap,
                              const vad_segment *d_tails /*on the GPU, [n], or NULL*/, const uint8_t *d_events, const float *d_probs,
                              const int64_t *out_start /*host [n + 1]*/, int64_t n, const vad_refine *r, vad_segment *d_segs_out,
                              int64_t seg_cap, int64_t *d_nsegs_out /*on the GPU*/, void *stream);
VAD_API int vad_scan_refine(vad_engine *e, const vad_segment *segs_in /*host, or NULL: the resident table*/, int64_t nsegs_in,
                            const vad_segment *tails_in /*host [n], or NULL*/, const vad_refine *r, vad_segment *segs_out,
                            int64_t seg_cap, int64_t *nsegs_out);

/*
 * Segment levels and gained cuts: how loud a segment is, and its audio times a factor, without the samples crossing the link.
 * The reference has AudioUtils.calculate_rms, calculate_energy, detect_clipping(threshold = 0.95) and
 * normalize_audio(target_level = 0.9) for this, on a host array (utils/audio.py); a corpus caller filters on RMS, peak and clipping
 * right behind the VAD and often peak-normalises what it cuts.
 *
 * vad_scan_levels: one vad_level per listed segment.  THE RULE: the levels of a segment are statistics of exactly the float32
 * values that vad_scan_cut / vad_scan_rate_cut with VAD_CUT_RANGE, VAD_CUT_F32 and the same arguments would write for it - decoded,
 * channel-selected and gated; on a rate block input-rate samples, never gated, as there.  A kernel reads the block in its wire
 * format and reduces where the cut stores; 16 bytes per segment cross the link back.
 *   energy_q32 = sum over the samples of min(rint(x * x * 2^32), 2^32), with x * x and the scaling in float64 (both exact for a
 * float32 x) and rint to nearest-even: a fixed-point sum, exact in any order.  A sample with |x| >= 1 counts as 1.  For int16 / 32768
 * and G.711 blocks (x = s / 32768) no term is rounded at all: energy_q32 = 4 * sum of s^2.  energy = energy_q32 / 2^32
 * (calculate_energy), rms = sqrt(energy / samples) (calculate_rms).  A block is under 2^31 samples: the sum cannot overflow.
 *   peak = max |x|, taken as the maximum of the bit patterns of |x| (0 for an all-zero segment).
 *   clipped = the samples with |x| >= clip_thresh, compared in float32 (detect_clipping's >=).  clip_thresh <= 0 counts every
 * sample; +Inf none.
 *   All three are integer reductions: the records do not depend on the GPU's scheduling, and two calls give the same bytes.
 *   A float32 block with non-finite samples: the peak of a segment that holds one is not finite (a NaN's pattern beats +Inf, +Inf
 * beats every finite value), its other two fields are unspecified; other segments are unaffected, the call completes normally.
 *   sr_in: 0 or the engine's own rate - a block at the engine's rate, every rule of vad_scan_cut applies; 8000 / 24000 / 48000 on a
 * 16 kHz engine - a rate block, every rule of vad_scan_rate_cut applies (first_frame and nframes count chunks), including which
 * resident block audio == NULL may name.  The items are vad_cut_item; out_sample is NOT read, so two items may name the same
 * samples.  A segment has vad_cut_samples / vad_rate_cut_samples(.., VAD_CUT_RANGE) samples.
 *   audio == NULL: the resident block, as in the cuts; with an audio the call uploads it, and it becomes the resident block.
 * Works on every engine, Silero V4 and VAD_ENGINE_SHARED_GPU included: no model kernel runs, no stream is touched.  The call first
 * waits for earlier *_device launches that read the engine's tables.
 *   VAD_ERR_INVALID_ARG, each with a message and nothing written: every refusal of vad_scan_cut / vad_scan_rate_cut that concerns
 * the block and the items, in the same words under this function's name; a NaN clip_thresh; a null levels_out with n > 0.
 * n == 0: VAD_OK.
 *   vad_scan_levels_device: d_audio as vad_scan_cut_device takes it, d_levels (8-byte aligned, n records) on the engine's GPU;
 * enqueues a clear of the records and the kernel on `stream` (NULL = the engine's own) and returns.
 *
 * vad_scan_cut_gain / vad_scan_cut_gain_device: vad_scan_cut / vad_scan_rate_cut (sr_in as above) with a factor per segment: a
 * sample of segment i is the gated value times gains[i] - one float32 multiply of its own - and then the float32 itself or
 * clip(. * 32767, -32768, 32767) toward zero, as there.  gains is a HOST array [n] in both forms.  On a rate block the factor
 * applies to the input-rate samples of VAD_CUT_RANGE and, for VAD_CUT_FRAMES, to the resampled and gated frames.  gains[i] == 1.0f
 * for all i gives the bytes of the call without gains.  gain = (float) target / peak, with the peak of vad_scan_levels on the same
 * table, is AudioUtils.normalize_audio per segment.  Every rule and refusal of the cut applies under the new names; further
 * VAD_ERR_INVALID_ARG: a null gains with n > 0, and a gain that is NaN or infinite, with a message that names the segment.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_levels / vad_scan_cut_gain is how a caller detects the feature.
 */
typedef struct vad_level {
    int64_t energy_q32;  /* sum of min(rint(x * x * 2^32), 2^32) over the segment's samples */
    float   peak;        /* max |x| */
    int32_t clipped;     /* samples with |x| >= clip_thresh */
} vad_level;
VAD_API int vad_scan_levels(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio /*or NULL*/, int64_t audio_samples,
                            int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, float clip_thresh,
                            vad_level *levels_out /*[n]*/);
VAD_API int vad_scan_levels_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                   int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, float clip_thresh,
                                   vad_level *d_levels /*on the GPU, [n]*/, void *stream);
VAD_API int vad_scan_cut_gain(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n]*/,
                              const void *audio /*or NULL*/, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in,
                              int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *out, int64_t out_samples);
VAD_API int vad_scan_cut_gain_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n]*/,
                                     const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in,
                                     int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *d_out,
                                     int64_t out_samples, void *stream);

/*
 * Log-mel features: what an ASR front end, a speaker-embedding model or a classifier takes instead of PCM, computed from the block
 * a scan left on the GPU.  Whisper's front end is n_fft = 400, hop = 160, a Hann window, reflect padding, 80 or 128 mel bins and
 * log10 with a floor; Kaldi-style recipes are other geometries of the same shape.  Without this call the samples cross the link as
 * float32 (vad_scan_cut, VAD_CUT_RANGE, VAD_CUT_F32) and the host runs an STFT.
 *
 * vad_scan_mel: a packed float32 matrix out[rows][n_mels] holding the frames of every listed segment.  THE RULE: segment i's values
 * v[0 .. S - 1] are exactly the float32 values that vad_scan_cut with VAD_CUT_RANGE, VAD_CUT_F32 and the same arguments would write
 * for the item - decoded, channel-selected and gated; S = vad_cut_samples(e, nframes, hop, VAD_CUT_RANGE), where `hop` is the
 * SCAN's hop (the last hop argument), not m->hop.  out_sample is NOT read, so two items may name the same samples.
 *   Padding.  VAD_MEL_PAD_NONE: p = v.  VAD_MEL_PAD_REFLECT: p has S + n_fft samples, p[j] = v[r(j - n_fft / 2)] with r(i) = -i for
 * i < 0 and 2 (S - 1) - i for i >= S - numpy's 'reflect', torch.stft's center = True.  It needs S > n_fft / 2; otherwise the call
 * returns VAD_ERR_INVALID_ARG and names the segment.
 *   Frames.  M = len(p) < n_fft ? 0 : (len(p) - n_fft) / m->hop + 1 (vad_mel_frames).  A segment with M = 0 is legal under
 * VAD_MEL_PAD_NONE and writes nothing.
 *   The transform.  re[f][k] = sum over n of p[f * m->hop + n] * op_re[n][k], im the same with op_im; P = re^2 + im^2;
 * E[f][j] = sum over k of filters[j][k] * P[f][k]; out = E (VAD_MEL_LINEAR), ln(max(E, floor)) (VAD_MEL_LN) or
 * log10(max(E, floor)) (VAD_MEL_LOG10).  Everything is float32; the order of the sums is the kernel's own.  With u = 2^-24,
 *     |E - E_exact| <= (2 n_fft + n_bins + 8) u D,   D[f][j] = sum_k filters[j][k] (sum_n |p op_re| + sum_n |p op_im|)^2
 * - the forward error of two chained float32 dot products around a square in ANY order of summation - and where every intermediate
 * value is an integer multiple of a power of two below 2^24 in magnitude the result is exact.  The logarithm is the hardware's
 * log2 (1 ulp) times a constant.
 *   Window and DFT basis are the caller's: they are folded into op_re / op_im ([n_fft][n_bins], row-major), so n_fft = 400 costs
 * what it is and not what 512 would.  filters is [n_mels][n_bins].  All three are HOST arrays in both forms, as gains is.
 *   Rows are packed in item order: segment i's first row is the sum of M_j over j < i, a row is n_mels floats.  out_rows smaller
 * than the total is refused; rows past the total are not written.
 *   Blocks at the engine's own rate only (there is no sr_in); audio == NULL names the resident block as in vad_scan_cut - a
 * resident rate block is refused in the cut's words - and with an audio the call uploads it, and it becomes the resident block.
 * Works on every engine, Silero V4 and VAD_ENGINE_SHARED_GPU included: no model kernel runs, no stream is touched.  The call first
 * waits for earlier *_device launches that read the engine's tables.
 *   A float32 block with non-finite samples: the rows whose frames hold one are unspecified, other rows are unaffected.
 *   No float atomics, every sum in a fixed order: two calls with the same arguments give the same bytes.
 *   VAD_ERR_INVALID_ARG, each with a message and nothing written: every refusal of vad_scan_cut that concerns the block and the
 * items, in the same words under this function's name; a null m; each field of vad_mel out of its range; a floor that is not
 * finite or not > 0 with a log; a null op_re, op_im or filters; a reflect-padded segment with S <= n_fft / 2; out_rows < 0 or
 * below the total; a null out with rows to write.  n == 0: VAD_OK.
 *   vad_scan_mel_device: d_audio as vad_scan_cut_device takes it, d_out (16-byte aligned, out_rows rows) on the engine's GPU;
 * enqueues the kernel on `stream` (NULL = the engine's own) and returns.
 *   vad_mel_frames: M for a segment of nsamples samples; -1 for a bad vad_mel, a negative nsamples, or reflect padding with
 * nsamples <= n_fft / 2.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_mel is how a caller detects the feature.
 */
enum { VAD_MEL_PAD_NONE = 0, VAD_MEL_PAD_REFLECT = 1 };
enum { VAD_MEL_LINEAR = 0, VAD_MEL_LN = 1, VAD_MEL_LOG10 = 2 };
typedef struct vad_mel {
    int32_t n_fft;     /* samples of one analysis frame: 64 .. 1024, a multiple of 16 */
    int32_t hop;       /* samples between analysis frames: 4 .. n_fft, a multiple of 4 */
    int32_t n_bins;    /* columns of op_re / op_im / filters: 1 .. n_fft / 2 + 1 */
    int32_t n_mels;    /* 1 .. 128 */
    int32_t pad;       /* VAD_MEL_PAD_* */
    int32_t log;       /* VAD_MEL_* */
    float   floor;     /* log != VAD_MEL_LINEAR: finite and > 0; VAD_MEL_LINEAR: not read */
    int32_t reserved;  /* 0 */
} vad_mel;
VAD_API int64_t vad_mel_frames(const vad_mel *m, int64_t nsamples);
VAD_API int vad_scan_mel(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re /*[n_fft][n_bins]*/,
                         const float *op_im /*[n_fft][n_bins]*/, const float *filters /*[n_mels][n_bins]*/,
                         const void *audio /*or NULL*/, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t hop,
                         float denoise_thresh, float *out /*[out_rows][n_mels]*/, int64_t out_rows);
VAD_API int vad_scan_mel_device(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re /*host*/,
                                const float *op_im /*host*/, const float *filters /*host*/, const void *d_audio,
                                int64_t audio_samples, int32_t channels, int frame_fmt, int32_t hop, float denoise_thresh,
                                float *d_out /*on the GPU: [out_rows][n_mels]*/, int64_t out_rows, void *stream);

/*
 * Segment audio and log-mel features at 16 kHz from a rate block: what comes after a VAD - mel front ends, waveform models, speaker
 * embedders - runs at 16 kHz, and vad_scan_rate_cut(VAD_CUT_RANGE) returns a segment at the INPUT rate (VAD_CUT_FRAMES: overlapping
 * frames, each resampled on its own - no continuous signal).  vad_scan_resample_cut writes the segment as ONE continuous signal at
 * 16 kHz, by a polyphase FIR whose taps are the caller's; vad_scan_rate_mel computes vad_scan_mel's rows from that signal.
 *
 * THE RULE.  For item i of a rate block at sr_in (8000, 24000 or 48000):
 *   - L / M = 16000 / sr_in in lowest terms: 2 / 1, 2 / 3, 1 / 3.
 *   - x[k], k = 0 .. S_in - 1, are exactly the float32 values vad_scan_rate_cut(VAD_CUT_RANGE, VAD_CUT_F32) writes for the item:
 *     decoded and channel-selected, never gated; S_in = (nframes - 1) * hop + chunk.
 *   - x[k] = 0 outside that range, EVEN WHERE THE BLOCK HOLDS AUDIO THERE: zero extension at the segment's edges, as
 *     scipy.signal.resample_poly does on a cut.  The result depends on the item alone.
 *   - taps is a host float32 array h[0 .. N - 1], the prototype low-pass at rate L * sr_in: N odd, 1 <= N <=
 *     VAD_RESAMPLE_CUT_MAX_TAPS, every entry finite; C = (N - 1) / 2.
 *   - S16 = floor(S_in * L / M) rounded down to a multiple of 4 (vad_resample_cut_samples; -1 on the conditions of
 *     vad_rate_cut_samples, and for sr_in == 16000).
 *   - For m = 0 .. S16 - 1:  y[m] = sum over k of x[k] * h[m * M - k * L + C], over the k in [0, S_in) whose tap index lies in
 *     [0, N).  All arithmetic is float32; the order of the sum is the kernel's own.  A sample is then y[m], or y[m] * gains[i] as one
 *     float32 multiply of its own when gains != NULL.  The cut's conversion follows: VAD_CUT_F32 stores the value, VAD_CUT_PCM16 is
 *     clip(. * 32767, -32768, 32767) toward zero.
 *   With u = 2^-24 and D[m] = sum over k of |x[k]| |h[.]|:  |y - y_exact| <= (ceil(N / L) + 4) u D in ANY order of summation - at most
 * ceil(N / L) terms are non-zero, and the structural zeros of a padded operator add no error.  Where every product and partial sum is
 * an integer multiple of a power of two below 2^24 in magnitude the result is exact.
 *
 * vad_scan_resample_cut: items are vad_cut_item, frames count chunks; segment i owns out[out_sample .. out_sample + S16), out_sample
 * a multiple of 4; overlapping output ranges are refused as in the cut, samples outside every range are not written.  audio == NULL
 * names the resident RATE block exactly as vad_scan_rate_cut does; with an audio the call uploads it, and it becomes the resident
 * rate block.  Works on every 16 kHz engine, Silero V4 and VAD_ENGINE_SHARED_GPU included; waits for earlier *_device launches.  No
 * float atomics, every sum in a fixed order: two calls give the same bytes.
 *   Refusals, each with a message under this function's name and nothing written: VAD_ERR_UNSUPPORTED for an engine of an 8 kHz
 * sub-model and for any sr_in outside 8000 / 24000 / 48000 (16000: there is nothing to resample); a null taps, ntaps even or outside
 * 1 .. VAD_RESAMPLE_CUT_MAX_TAPS, a tap that is NaN or infinite (the message names the lowest index); every block and item refusal of
 * vad_scan_rate_cut, in the same words; a non-finite gain, in vad_scan_cut_gain's words.  n == 0: VAD_OK.
 *   A workgroup of the kernel serves VAD_RESAMPLE_CUT_WG_SAMPLES consecutive output samples of one segment, loads its input span
 * once and never issues a load outside the segment's own sample range.
 *
 * vad_scan_rate_mel: rows byte for byte what vad_scan_mel computes under this recipe - a mono float32 block at the engine's rate
 * holds segment i's y[0 .. S16) (no gain) at a multiple-of-4 offset o_i; items are (o_i, 0, (S16 - 512) / 4 + 1, 0), hop = 4, gate
 * off.  That is also how the engine runs it: the resample kernel writes into an engine-owned float32 buffer and vad_scan_mel's
 * kernel runs behind it on the same stream.  Refusals: those of vad_scan_resample_cut that concern block, items and taps (no item's
 * out_sample is read), then vad_scan_mel's for m, the operators and out_rows; a reflect-padded segment with S16 <= n_fft / 2; an
 * intermediate of 2^29 samples or more.  The operator cache is vad_scan_mel's.
 *   The _device forms take d_audio / d_out as the cuts' and vad_scan_mel_device's do, enqueue on `stream` (NULL = the engine's own)
 * and return; gains, taps and the operators stay HOST arrays, read before the call returns.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_resample_cut is how a caller detects the feature.
 */
#define VAD_RESAMPLE_CUT_MAX_TAPS 511
#define VAD_RESAMPLE_CUT_WG_SAMPLES 2048
VAD_API int64_t vad_resample_cut_samples(const vad_engine *e, int64_t nframes, int32_t sr_in, int32_t hop);
VAD_API int vad_scan_resample_cut(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                  const float *taps /*host [ntaps]*/, int32_t ntaps, const void *audio /*or NULL*/, int64_t audio_samples,
                                  int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, int32_t out_fmt, void *out,
                                  int64_t out_samples);
VAD_API int vad_scan_resample_cut_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                         const float *taps /*host [ntaps]*/, int32_t ntaps, const void *d_audio, int64_t audio_samples,
                                         int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, int32_t out_fmt, void *d_out,
                                         int64_t out_samples, void *stream);
VAD_API int vad_scan_rate_mel(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re /*[n_fft][n_bins]*/,
                              const float *op_im /*[n_fft][n_bins]*/, const float *filters /*[n_mels][n_bins]*/,
                              const float *taps /*host [ntaps]*/, int32_t ntaps, const void *audio /*or NULL*/, int64_t audio_samples,
                              int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float *out /*[out_rows][n_mels]*/,
                              int64_t out_rows);
VAD_API int vad_scan_rate_mel_device(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re /*host*/,
                                     const float *op_im /*host*/, const float *filters /*host*/, const float *taps /*host [ntaps]*/,
                                     int32_t ntaps, const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                                     int32_t sr_in, int32_t hop, float *d_out /*on the GPU: [out_rows][n_mels]*/, int64_t out_rows,
                                     void *stream);

/*
 * Recordings at 44.1 kHz and any other rational rate: a whole recording converted ONCE to the engine's rate, into an engine-owned
 * mono float32 block.  That block is an ordinary resident block at the engine's own rate: vad_scan_cut(audio = NULL), the levels,
 * renders, mel features and batches, vad_scan_resegment, the tails and vad_scan_refine work behind it unchanged, and none of them
 * needs a rate variant.  (The chunk route of vad_scan_rate cannot be stretched: a 512-sample frame is 1411.2 samples at 44.1 kHz.)
 *
 * THE RULE.  For item i (vad_scan_ch_item: slot, sample_offset - a multiple of 4 -, nsamples = S_in - ANY count -, channel) of a
 * block at sr_in, in any wire format, with 1 or 2 interleaved channels:
 *   - R is the engine's rate (vad_info.sample_rate), g = gcd(R, sr_in), L = R / g, M = sr_in / g.
 *   - Accepted: VAD_CONVERT_MIN_RATE <= sr_in <= VAD_CONVERT_MAX_RATE, sr_in != R, a period P = lcm(L, 16) of at most
 *     VAD_CONVERT_MAX_PERIOD outputs and M <= VAD_CONVERT_MAX_PERIOD: 8, 11.025, 12, 22.05, 24, 32, 44.1, 48, 88.2, 96, 176.4 and
 *     192 kHz on a 16 kHz engine, among others.  Anything else: VAD_ERR_UNSUPPORTED with a message that names L, M and the limits;
 *     sr_in == R is refused too, there is nothing to convert.
 *   - x[k], k = 0 .. S_in - 1, are the float32 values the scans' loader hears BEFORE THE GATE: decoded (s / 32767 or s / 32768,
 *     G.711) and channel-selected, (L + R) * 0.5f for VAD_SCAN_MIX.  Never gated: a scan gates the converted signal.
 *   - x[k] = 0 outside [0, S_in), EVEN WHERE THE BLOCK HOLDS AUDIO THERE.  The result depends on the item alone.
 *   - taps is a host float32 array h[0 .. N - 1], the prototype low-pass at rate L * sr_in: N odd, 1 <= N <= VAD_CONVERT_MAX_REACH * L,
 *     every entry finite; C = (N - 1) / 2.
 *   - S_out = floor(S_in * L / M): vad_convert_samples(e, nsamples, sr_in); -1 for a null engine, a negative or 2^31-or-larger count
 *     and a rate that is not accepted.
 *   - For m = 0 .. S_out - 1:  y[m] = sum over k of x[k] * h[m * M - k * L + C], over the k in [0, S_in) whose tap index lies in
 *     [0, N).  All arithmetic is float32; the order of the sum is the kernel's own and fixed: two calls give the same bytes.
 *   - With u = 2^-24 and D[m] = sum over k of |x[k]| |h[.]|:  |y - y_exact| <= (ceil(N / L) + 4) u D - vad_scan_resample_cut's bound,
 *     which holds in any order of summation.  Where every product and partial sum is an integer multiple of a power of two below
 *     2^24 in magnitude the result is exact.
 *   - Layout: item i sits at out_offset[i] = sum over j < i of roundup4(S_out_j); the 0 .. 3 samples between two items are written
 *     as +0.0, so EVERY sample of the converted block of out_offset[n] samples is written.  A block of 2 GiB of float32 or more
 *     (2^29 samples) is refused.
 *   - Non-finite float32 input.  The kernel computes output m from the K inputs that start at floor(m / P) * P * M / L + base_r,
 *     r = (m mod P) / 16, base_r = floor((16 r M - C) / L), K = (15 M + N - 1) / L + 2 rounded up to a multiple of 16: a window that
 *     holds the taps of the 16 outputs of m's row-tile, padded with structural zeros of the operator.  Every output whose TAP
 *     window holds the bad sample is non-finite (which NaN is not specified); an output m with |k - m M / L| >= K for the bad sample
 *     k is byte for byte what it is with x[k] = 0; an output in between is either (0 * NaN).
 *
 * vad_convert: the conversion alone, host to host: the block is uploaded, converted, and out[0 .. out_offset[n]) is copied back;
 * out_offset (host, [n + 1], or NULL) receives the layout.  Slots are not read, no stream is touched, no model runs and the resident
 * block stays what it was; works on every engine, Silero V4 and VAD_ENGINE_SHARED_GPU included.  Waits for earlier *_device launches.
 * vad_convert_device: d_audio -> d_out (16-byte aligned) on `stream` (NULL = the engine's own), returns after enqueueing; d_audio is
 * aligned as vad_scan_channels_device wants it (4 bytes, 8 for two channels); taps and out_offset are HOST arrays.
 *   Refusals, each with a message under the function's name and nothing written: the rate (above); a null taps, ntaps even or
 * outside 1 .. VAD_CONVERT_MAX_REACH * L, a tap that is NaN or infinite (the message names the lowest index); every block and item
 * refusal of vad_scan_channels, in its words (counts, format, channels, 2 GiB of input, an offset that is not a multiple of 4, an
 * item that leaves the block, a channel out of range, a non-zero reserved - not hop, slots or max_streams, which no conversion
 * reads); a converted block of 2 GiB or more; out_samples < out_offset[n]; a null audio or out when there is anything to convert; a
 * misaligned device pointer.  n == 0: VAD_OK.
 *
 * vad_scan_convert_segments: upload the block into a staging buffer, convert it into the engine's audio buffer, and run exactly what
 * vad_scan_segments runs - the model launches, the tail snapshot, the extraction - on that buffer as a mono VAD_FMT_F32 block at the
 * engine's rate, with the items {slot, out_offset[i], S_out_i, channel 0}; hop and every position downstream count samples at the
 * ENGINE's rate.  BY DEFINITION the call is byte-equal to vad_convert followed by vad_scan_segments on the float32 block it
 * returned: the table, the resident per-frame results (vad_scan_resegment, vad_scan_tails) and the resident block
 * (vad_scan_cut(audio = NULL, audio_samples = out_offset[n], channels = 1, VAD_FMT_F32)).  Refusals: those of vad_convert for rate,
 * taps, block and items, then vad_scan_segments's own (hop, max_streams, slots, seg_cap, null buffers; Silero V4 and
 * VAD_ENGINE_SHARED_GPU engines: VAD_ERR_UNSUPPORTED - only the conversion itself runs there).
 *   A workgroup of the kernel serves a run of whole periods of one item - VAD_CONVERT_WG_SAMPLES outputs or more where the item has
 * them and local memory holds their inputs -, loads the run's input span once and never issues a load outside the item's own samples.
 *   vad_scan_rate*, vad_scan_resample_cut and every other entry point accept the rates they accepted before.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_convert is how a caller detects the feature.
 */
#define VAD_CONVERT_MAX_REACH 128
#define VAD_CONVERT_MIN_RATE 4000
#define VAD_CONVERT_MAX_RATE 192000
#define VAD_CONVERT_MAX_PERIOD 640
#define VAD_CONVERT_WG_SAMPLES 2048
VAD_API int64_t vad_convert_samples(const vad_engine *e, int64_t nsamples, int32_t sr_in);
VAD_API int vad_convert(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples, int32_t channels,
                        int frame_fmt, int32_t sr_in, const float *taps /*host [ntaps]*/, int32_t ntaps, float *out, int64_t out_samples,
                        int64_t *out_offset /*[n + 1] host or NULL*/);
VAD_API int vad_convert_device(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                               int32_t channels, int frame_fmt, int32_t sr_in, const float *taps /*host [ntaps]*/, int32_t ntaps,
                               float *d_out, int64_t out_samples, int64_t *out_offset /*[n + 1] host or NULL*/, void *stream);
VAD_API int vad_scan_convert_segments(vad_engine *e, const vad_scan_ch_item *items, int64_t n, const void *audio, int64_t audio_samples,
                                      int32_t channels, int frame_fmt, int32_t sr_in, const float *taps /*host [ntaps]*/, int32_t ntaps,
                                      int32_t hop, float denoise_thresh, vad_segment *segs_out, int64_t seg_cap, int64_t *nsegs_out,
                                      int64_t *out_offset /*[n + 1] or NULL*/);

/*
 * Model-ready feature batches: what an ASR front end, a speaker model or a classifier takes is not the packed matrix of
 * vad_scan_mel but normalised, padded windows [B][n_mels][T] in its own number format.  Three steps, all on the GPU:
 *
 * vad_scan_mel_keep / _device: vad_scan_mel (sr_in = 0 or the engine's rate; taps / ntaps are not read) or vad_scan_rate_mel (sr_in
 * = 8000, 24000, 48000; denoise_thresh is not read) with the rows left in an engine-owned float32 buffer, the RESIDENT MATRIX,
 * instead of an `out`: the same kernels, the same refusals in the same words under this function's name, rows byte for byte
 * those.  The engine remembers n, n_mels and the segments' first rows start[n + 1]; *rows_out (may be NULL) gets start[n].  The
 * next keep replaces the matrix, a refused keep leaves the previous one, the engine's end frees it; the resident audio block and
 * the resident segment table are left as the plain calls leave them.  n = 0 keeps a matrix of no rows.  The _device form takes
 * d_audio as vad_scan_mel_device does and enqueues on `stream`; the calls below wait for it.
 *   vad_mel_resident: its size (each pointer may be NULL); VAD_ERR_INVALID_ARG with a message when no matrix is kept.
 *   vad_mel_resident_read: rows first_row .. first_row + count - 1 copied to the host.
 *
 * vad_mel_stats / _device: per segment of a matrix features[rows][n_mels] - a host array (_device: on the GPU), or NULL for the
 * resident matrix, whose rows and n_mels then stand for the arguments - with the segments' first rows start[n + 1] (host in both
 * forms; 0 <= start[0], ascending, start[n] <= rows), or start = NULL for the resident starts, whose n then stands for the argument.
 * Each output may be NULL and is then skipped (host arrays; _device: on the GPU, 8-byte aligned):
 *   max_out[n], float32: the maximum over all values of the segment, by the order of the bit patterns (-0.0 below +0.0); a
 *     segment without rows has -inf.
 *   sum_out[n][n_mels], int64, and sumsq_out[n][n_mels], uint64: with q = (int64) rintf(clamp(x, -2048, 2048) * 4096), the sums of q
 *     and of q * q over the segment's rows.  x * 4096 is exact in float32 and the sums are integers: the result is exact in any
 *     order.  mean = sum / (4096 M), E[x^2] = sumsq / (2^24 M).  With either requested a segment of more than VAD_STATS_MAX_ROWS =
 *     2^17 rows is refused by index (2^46 * 2^17 stays inside 64 bits).
 * The call initialises its outputs itself.  Two runs give the same bytes.  Rows that hold a NaN give unspecified values.
 *
 * vad_mel_batch / _device: nw windows of b->frames = T frames each, out[nw][C][T] (VAD_BATCH_CHANNEL_MAJOR) or out[nw][T][C]
 * (VAD_BATCH_TIME_MAJOR), C = n_mels * (deltas + 1), in float32, float16 or bfloat16.  features, rows, start, n as above (n_mels is
 * b->n_mels and must be the resident matrix's when that is named).  windows[nw] (host): window w shows rows row0 .. row0 + nrows - 1
 * of segment seg, 0 <= row0, 0 <= nrows <= T, row0 + nrows <= M (the segment's rows); in any order, overlapping, the same rows twice.
 * lo[n] (host, or NULL = -inf; no NaN), shift and scale [nss][n_mels] (host, finite; nss = 1: one row for all segments, nss = n: a
 * row per segment; NULL = 0 and 1, nss is then not read).
 * THE RULE, all of it float32, each operation rounded on its own.  For segment i, band j, row t in 0 .. M - 1:
 *     v[t][j] = (fmaxf(x[t][j], lo[i]) + shift[i][j]) * scale[i][j]
 *   (an add followed by a multiply: nothing to contract into a fused multiply-add).  With c(s) = min(max(s, 0), M - 1):
 *     d1[t] = ((v[c(t + 1)] - v[c(t - 1)]) + 2 * (v[c(t + 2)] - v[c(t - 2)])) * 0.1f
 *     d2[t] = ((d1[c(t + 1)] - d1[c(t - 1)]) + 2 * (d1[c(t + 2)] - d1[c(t - 2)])) * 0.1f
 *   c clamps to the SEGMENT, not to the window: a window inside a segment sees its neighbours' rows.  Channel k * n_mels + j holds
 *   v for k = 0, d1 for k = 1, d2 for k = 2.  Cell (w, channel, t), t < nrows: the value at segment row row0 + t.  t >= nrows, a
 *   pad cell: 0 in a delta channel; in a static channel pad_value as it is (VAD_BATCH_PAD_VALUE) or (fmaxf(pad_value, lo[i]) +
 *   shift[i][j]) * scale[i][j] (VAD_BATCH_PAD_FEATURE: a frame of silence through the same normalisation, as Whisper pads).  Then
 *   the conversion, round to nearest even; overflow becomes inf.  Every cell of every window is written by the one launch.
 * Whisper: lo[i] = max_i - 8, shift = 4, scale = 0.25, PAD_FEATURE with pad_value = -10 (log10 of the floor 1e-10), T = 3000.
 * Refusals (VAD_ERR_INVALID_ARG, a message, the output untouched): a field of vad_batch out of range; n_mels that is not the resident
 * matrix's; a bad start; a bad window, by index; nss neither 1 nor n; a non-finite scale, shift or pad_value; a NaN lo; out_bytes
 * below nw * C * T elements; more than 2^31 - 1 workgroups; a device `out` that is not 16-byte aligned; NULL features or start with
 * no resident matrix.  nw = 0 is VAD_OK.
 *   The _device forms enqueue on `stream` (NULL = the engine's own) and return; start, windows, lo, shift and scale stay HOST arrays,
 * read before the call returns.  Every engine is served - V4, 8 kHz, VAD_ENGINE_SHARED_GPU: no model kernel runs.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_mel_batch is how a caller detects the feature.
 */
#define VAD_STATS_MAX_ROWS 131072
enum { VAD_BATCH_F32 = 0, VAD_BATCH_F16 = 1, VAD_BATCH_BF16 = 2 };
enum { VAD_BATCH_CHANNEL_MAJOR = 0 /* [B][C][T] */, VAD_BATCH_TIME_MAJOR = 1 /* [B][T][C] */ };
enum { VAD_BATCH_PAD_VALUE = 0, VAD_BATCH_PAD_FEATURE = 1 };
typedef struct vad_batch {
    int32_t n_mels;    /* 1 .. 128 */
    int32_t frames;    /* T: 4 .. 65536, a multiple of 4 */
    int32_t deltas;    /* 0 .. 2 */
    int32_t layout;    /* VAD_BATCH_CHANNEL_MAJOR / VAD_BATCH_TIME_MAJOR */
    int32_t dtype;     /* VAD_BATCH_F32 / VAD_BATCH_F16 / VAD_BATCH_BF16 */
    int32_t pad_mode;  /* VAD_BATCH_PAD_VALUE / VAD_BATCH_PAD_FEATURE */
    float pad_value;   /* finite */
    int32_t reserved;  /* 0 */
} vad_batch;
typedef struct vad_batch_window {
    int32_t seg;       /* index into the segments */
    int32_t nrows;     /* 0 .. T */
    int64_t row0;      /* first row, within the segment */
} vad_batch_window;
VAD_API int vad_scan_mel_keep(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re /*[n_fft][n_bins]*/,
                              const float *op_im /*[n_fft][n_bins]*/, const float *filters /*[n_mels][n_bins]*/,
                              const float *taps /*host [ntaps]: a rate block*/, int32_t ntaps, const void *audio /*or NULL*/,
                              int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                              int64_t *rows_out);
VAD_API int vad_scan_mel_keep_device(vad_engine *e, const vad_cut_item *items, int64_t n, const vad_mel *m, const float *op_re /*host*/,
                                     const float *op_im /*host*/, const float *filters /*host*/, const float *taps /*host [ntaps]*/,
                                     int32_t ntaps, const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt,
                                     int32_t sr_in, int32_t hop, float denoise_thresh, int64_t *rows_out, void *stream);
VAD_API int vad_mel_resident(vad_engine *e, int64_t *rows, int32_t *n_mels, int64_t *nsegs);
VAD_API int vad_mel_resident_read(vad_engine *e, int64_t first_row, int64_t count, float *out /*[count][n_mels]*/);
VAD_API int vad_mel_stats(vad_engine *e, const float *features /*[rows][n_mels] or NULL*/, int64_t rows, int32_t n_mels,
                          const int64_t *start /*[n + 1] or NULL*/, int64_t n, float *max_out /*[n] or NULL*/,
                          int64_t *sum_out /*[n][n_mels] or NULL*/, uint64_t *sumsq_out /*[n][n_mels] or NULL*/);
VAD_API int vad_mel_stats_device(vad_engine *e, const float *d_features /*on the GPU or NULL*/, int64_t rows, int32_t n_mels,
                                 const int64_t *start /*host [n + 1] or NULL*/, int64_t n, float *d_max_out, int64_t *d_sum_out,
                                 uint64_t *d_sumsq_out, void *stream);
VAD_API int vad_mel_batch(vad_engine *e, const float *features /*[rows][n_mels] or NULL*/, int64_t rows,
                          const int64_t *start /*[n + 1] or NULL*/, int64_t n, const vad_batch *b, const vad_batch_window *windows,
                          int64_t nw, const float *lo /*[n] or NULL*/, const float *shift /*[nss][n_mels] or NULL*/,
                          const float *scale /*[nss][n_mels] or NULL*/, int64_t nss, void *out, int64_t out_bytes);
VAD_API int vad_mel_batch_device(vad_engine *e, const float *d_features /*on the GPU or NULL*/, int64_t rows,
                                 const int64_t *start /*host [n + 1] or NULL*/, int64_t n, const vad_batch *b,
                                 const vad_batch_window *windows /*host*/, int64_t nw, const float *lo /*host*/,
                                 const float *shift /*host*/, const float *scale /*host*/, int64_t nss, void *d_out, int64_t out_bytes,
                                 void *stream);

/*
 * Packed feature batches: several segments per window.  A fixed-window model pays for every frame of a window; with one segment per
 * window most frames of a corpus of short segments are padding.  Here the segments of a group (a recording, say) lie back to back
 * in as few windows as hold them, each PIECE at a frame offset, with an index that restores where it came from.
 *
 * vad_mel_pack_plan: the packing rule.  Host code only: no engine, no GPU.  start[n + 1] are the segments' first rows (ascending),
 * group[n] their groups (NULL: one group), frames = T, gap the frames of silence between the pieces of a window.  THE RULE, greedy
 * and in order, with up4(x) = x rounded up to a multiple of 4:
 *   1. Walk the segments i = 0 .. n - 1.
 *   2. Skip a segment without rows.
 *   3. A segment of M rows is taken in pieces of k = min(T, M - r) rows, at r = 0, T, 2T, ...
 *   4. A piece goes to the current window at offset = up4(used + gap), where used is the end of the window's last piece.
 *   5. A piece starts a new window at offset 0 in three cases: there is no window yet, the piece's group differs from the
 *      window's, or offset + k > T.
 * So windows never mix groups, a segment longer than T fills whole windows, and its remainder opens a window that later segments
 * may join.  The pieces tile [start[0], start[n]) in order: their bounds are themselves an ascending start array of npieces + 1
 * entries.  *npieces and *nwindows (each may be NULL) get the counts; pieces_out = NULL counts only, else it takes the pieces and
 * cap is its room.  Refusals (VAD_ERR_INVALID_ARG, pieces_out untouched): T not a multiple of 4 in 4 .. 65536; gap outside 0 .. T;
 * a start that does not ascend; n outside 0 .. 2^31 - 1; cap smaller than the count (the counts are still stored).
 *
 * vad_mel_batch_packed / _device: nw windows of b->frames = T frames holding np pieces.  The sources, layouts, number formats,
 * vad_batch fields and their checks are those of vad_mel_batch.  THE RULE: it is vad_mel_batch's rule, with lo[nw], shift and scale
 * [nss][n_mels] (nss = 1 or nw) indexed by WINDOW.  For a piece of window w at `offset`, cell (w, channel, offset + t) with t <
 * nrows is v, d1 or d2 of segment row row0 + t, with v = (fmaxf(x, lo[w]) + shift[w][j]) * scale[w][j]; the deltas are clamped to the
 * SEGMENT: a later piece of a split segment sees the earlier piece's rows.  Every cell that no piece covers is a pad cell - the
 * cells between pieces, behind the last piece, a whole window without pieces: 0 in the delta channels, in the static channels
 * pad_value, or pad_value through the window's normalisation.  Every cell of every window is written exactly once, by ONE launch.
 * Two runs give the same bytes: no atomics, no float accumulation.  The pieces may come in any order; a segment, or the same rows,
 * may be shown twice.
 * Refusals (VAD_ERR_INVALID_ARG, a message, by index, the output untouched), in this order: those of vad_mel_batch up to its
 * windows, with nss = 1 or nw and lo[nw]; a piece with seg, row0 or nrows outside its segment, or nrows < 1; window outside 0 ..
 * nw - 1; offset negative, not a multiple of 4, or with offset + nrows > T; two pieces of one window whose spans [offset,
 * up4(offset + nrows)) overlap; out_bytes below nw * C * T elements; more than 2^31 - 1 workgroups; then the output pointer as in
 * vad_mel_batch.  np = 0 with nw > 0 writes pad windows.  nw = 0 is VAD_OK.
 *
 * vad_mel_stats_grouped / _device: vad_mel_stats with group[n] (host; 0 .. ngroups - 1) and outputs of ngroups entries: group g's
 * maximum and sums are the reduction over every segment i with group[i] == g; a group without rows gets -inf and 0; the
 * VAD_STATS_MAX_ROWS bound applies to a group's total rows when a sum is asked for.  group = NULL is the identity (ngroups is not
 * read): vad_mel_stats's bytes.  Window scope is one call: start = the piece bounds, group = the pieces' windows.
 *   Every engine is served.  VAD_ABI_VERSION is unchanged: the presence of vad_mel_batch_packed is how a caller detects the feature.
 */
typedef struct vad_batch_piece {
    int32_t seg;       /* index into the segments */
    int32_t nrows;     /* 1 .. T */
    int64_t row0;      /* first row, within the segment */
    int32_t window;    /* 0 .. nw - 1 */
    int32_t offset;    /* first frame of the piece in its window: a multiple of 4, offset + nrows <= T */
} vad_batch_piece;     /* 24 bytes */
VAD_API int vad_mel_pack_plan(const int64_t *start /*[n + 1]*/, int64_t n, const int32_t *group /*[n] or NULL: one group*/, int32_t frames /*T*/,
                              int32_t gap, vad_batch_piece *pieces_out /*or NULL: count only*/, int64_t cap, int64_t *npieces,
                              int64_t *nwindows);
VAD_API int vad_mel_batch_packed(vad_engine *e, const float *features /*or NULL: resident*/, int64_t rows, const int64_t *start /*or NULL*/,
                                 int64_t n, const vad_batch *b, const vad_batch_piece *pieces /*host*/, int64_t np, int64_t nw,
                                 const float *lo /*[nw] or NULL*/, const float *shift /*[nss][n_mels] or NULL*/,
                                 const float *scale /*[nss][n_mels] or NULL*/, int64_t nss /*1 or nw*/, void *out, int64_t out_bytes);
VAD_API int vad_mel_batch_packed_device(vad_engine *e, const float *d_features /*on the GPU or NULL*/, int64_t rows,
                                        const int64_t *start /*host [n + 1] or NULL*/, int64_t n, const vad_batch *b,
                                        const vad_batch_piece *pieces /*host*/, int64_t np, int64_t nw, const float *lo /*host*/,
                                        const float *shift /*host*/, const float *scale /*host*/, int64_t nss, void *d_out, int64_t out_bytes,
                                        void *stream);
VAD_API int vad_mel_stats_grouped(vad_engine *e, const float *features /*[rows][n_mels] or NULL*/, int64_t rows, int32_t n_mels,
                                  const int64_t *start /*[n + 1] or NULL*/, int64_t n, const int32_t *group /*host [n] or NULL*/,
                                  int64_t ngroups, float *max_out /*[ngroups] or NULL*/, int64_t *sum_out /*[ngroups][n_mels] or NULL*/,
                                  uint64_t *sumsq_out /*[ngroups][n_mels] or NULL*/);
VAD_API int vad_mel_stats_grouped_device(vad_engine *e, const float *d_features /*on the GPU or NULL*/, int64_t rows, int32_t n_mels,
                                         const int64_t *start /*host [n + 1] or NULL*/, int64_t n, const int32_t *group /*host [n] or NULL*/,
                                         int64_t ngroups, float *d_max_out, int64_t *d_sum_out, uint64_t *d_sumsq_out, void *stream);

/*
 * Cepstral features and other linear front ends: MFCC and LFCC (a DCT of the log-mel or log-linear bands, a lifter, a scale), PCA /
 * LDA, global-CMVN whitening, band selection - one small matrix product per row of a feature matrix, done where the rows are.
 *
 * vad_mel_project / _device: out[rows][n_out] from features[rows][n_in] - a host array (_device: on the GPU), or NULL for the
 * resident matrix of vad_scan_mel_keep, whose rows and n_mels then stand for rows and n_in, which are not read - with the operator
 * op[n_in][n_out] and bias[n_out] (HOST arrays in both forms, finite; bias = NULL is 0), n_in and n_out in 1 .. 128.
 * THE RULE, in float32:
 *     y[r][c] = bias[c] + sum over k of x[r][k] * op[k][c]
 *   as a chain of fused multiply-adds that starts at bias[c] and takes k ascending: acc = fmaf(x[r][k], op[k][c], acc), one rounding
 *   per term (v_mfma_f32_16x16x4_f32 is this chain, bit for bit).  So with D[r][c] = |bias[c]| + sum over k of |x[r][k]| |op[k][c]| and
 *   u = 2^-24:
 *     |y - exact| <= (n_in + 2) u D[r][c]
 *   - the standard bound of an n_in-term fused-multiply-add sum in any order with the bias (derived, not measured; it holds while no
 *   term or partial sum is subnormal).  Where float32 is exact - integer x, op and bias with every partial sum below 2^24 - y is the
 *   exact integer (the sign of a zero result is unspecified: where n_in is no multiple of 4 the chain ends in fmaf(+0, +0, acc) for the
 *   padded k, and -0.0 becomes +0.0).  A row's value depends on that row, op and bias alone: not on the row's position in the matrix, on rows, or on
 *   the launch.  Nothing is accumulated across workgroups, there are no atomics: two runs give the same bytes.  A row that holds a NaN
 *   or an infinity gives unspecified values in that row only.
 * out == NULL REPLACES the resident matrix by its projection, and requires features == NULL: the matrix becomes [rows][n_out],
 * vad_mel_resident reports n_mels = n_out, the segments' first rows stay, and vad_mel_stats, vad_mel_stats_grouped, vad_mel_batch,
 * vad_mel_batch_packed and vad_mel_resident_read work on it as on any resident matrix (the engine projects into a second buffer of
 * its own and swaps the two).  With an `out` the resident matrix is left alone.  The resident audio block and the resident segment
 * table are left as vad_mel_stats leaves them.
 *   Refusals, each VAD_ERR_INVALID_ARG with a message under the function's name, nothing written and the resident matrix as it was,
 * in this order: features == NULL with no resident matrix; rows < 0; n_in outside 1 .. 128; n_out outside 1 .. 128; a null op; a
 * non-finite op entry, by index, then a non-finite bias entry, by index; out == NULL with a features; (_device) d_features or d_out
 * not 4-byte aligned; (_device) a d_out range that overlaps the input's; more than 2^31 - 1 workgroups (of 64 rows).  rows == 0 is
 * VAD_OK.
 *   The _device form enqueues on `stream` (NULL = the engine's own) and returns; op and bias are read before the call returns; the
 * calls that read the resident matrix wait for it.  Every engine is served - V4, 8 kHz, VAD_ENGINE_SHARED_GPU: no model kernel runs.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_mel_project is how a caller detects the feature.
 */
VAD_API int vad_mel_project(vad_engine *e, const float *features /*[rows][n_in] or NULL*/, int64_t rows, int32_t n_in,
                            const float *op /*host [n_in][n_out]*/, const float *bias /*host [n_out] or NULL = 0*/, int32_t n_out,
                            float *out /*[rows][n_out] or NULL: replace the resident matrix*/);
VAD_API int vad_mel_project_device(vad_engine *e, const float *d_features /*on the GPU or NULL*/, int64_t rows, int32_t n_in,
                                   const float *op /*host [n_in][n_out]*/, const float *bias /*host [n_out] or NULL*/, int32_t n_out,
                                   float *d_out /*on the GPU or NULL*/, void *stream);

/*
 * Audio batches: what a model that takes the waveform itself is fed - wav2vec 2.0, HuBERT, WavLM, speaker embedders: [B][T] windows
 * of samples in the model's number format, mean-removed, z-scored or peak-normalised per utterance, zero-padded, with an attention
 * mask - made from the block a scan left on the GPU, without the samples crossing the link as float32 and coming back.
 *
 * THE RULE of both calls: they work on exactly the float32 values that vad_scan_cut / vad_scan_rate_cut would write for each item
 * with VAD_CUT_RANGE, VAD_CUT_F32 and the same block arguments - decoded, channel-selected and gated; on a rate block (sr_in 8000 /
 * 24000 / 48000) input-rate samples, never gated.  Every word of vad_scan_levels about the block, the items, sr_in, audio == NULL,
 * the resident block and which engines are served applies: out_sample is NOT read, items may share samples, no model kernel runs.
 *
 * vad_scan_moments: one vad_moments per listed segment, for its mean and variance.
 *   sum_q31 = sum over the samples of rint((double) clamp(x, -1, 1) * 2^31), rounded to nearest-even.  The product is exact in
 * float64, so the sum is an integer, exact in any order, and below 2^62 for a block under 2^31 samples.
 *   energy_q32 is vad_level's field by the same definition: the two calls agree on it byte for byte.
 *   For int16 / 32768 and G.711 blocks nothing is rounded: sum_q31 = 65536 * sum of s.
 *   mean = sum_q31 / (2^31 N), var = energy_q32 / (2^32 N) - mean^2, with N the segment's samples.
 *   All reductions are integer, no float atomics: two calls give the same bytes.  A segment that holds a NaN gets an unspecified
 * record; other segments are unaffected.
 *   VAD_ERR_INVALID_ARG / VAD_ERR_UNSUPPORTED, each with a message and nothing written: every refusal of vad_scan_levels about the
 * rate, the block and the items, in the same words under this function's name; then a null out with n > 0.  n == 0: VAD_OK.
 *   vad_scan_moments_device: d_audio as vad_scan_cut_device takes it, d_out (8-byte aligned, n records) on the engine's GPU;
 * enqueues a clear of the records and the kernel on `stream` (NULL = the engine's own) and returns.
 *
 * vad_scan_audio_batch / _device: nw windows of b->samples = T samples each, out[nw][T] in float32, float16 or bfloat16 (dtype and
 * pad_mode are vad_batch's: VAD_BATCH_F32 / F16 / BF16, VAD_BATCH_PAD_VALUE / PAD_FEATURE), and mask[nw][T] bytes when asked.
 *   Window w shows samples sample0 .. sample0 + nsamples - 1 of segment seg's range: sample0 >= 0 and a multiple of 4, 0 <= nsamples
 * <= T, sample0 + nsamples <= S = the segment's vad_cut_samples / vad_rate_cut_samples(.., VAD_CUT_RANGE).  T is a multiple of 4 in
 * 4 .. 2^24.
 *   cell (w, t), t < nsamples: (x + shift[i]) * scale[i] with i = seg, or 0 when nss == 1 - float32, an add, then a multiply, each
 * rounded on its own.  shift == NULL is 0, scale == NULL is 1; both are HOST arrays [nss] in both forms.
 *   cell (w, t), t >= nsamples, a pad cell: pad_value as it is (VAD_BATCH_PAD_VALUE) or (0 + shift[i]) * scale[i]
 * (VAD_BATCH_PAD_FEATURE: silence through the normalisation).
 *   Then the conversion, round to nearest even; overflow becomes inf.
 *   mask[w][t] = 1 for t < nsamples, 0 otherwise.
 *   Every cell of out and of mask is written exactly once, by ONE launch; nothing is accumulated: two calls give the same bytes.
 * Windows may come in any order and overlap, the same samples may be shown twice, nsamples == 0 writes a pad window.  nw == 0 is
 * VAD_OK.
 *   Refusals, each VAD_ERR_INVALID_ARG or VAD_ERR_UNSUPPORTED with a message that names the function and the output untouched, in
 * this order: every refusal of vad_scan_levels about the rate, the block and the items; a null b, T out of range, an unknown dtype
 * or pad_mode, a non-finite pad_value; a negative nw or out_bytes, null windows with nw > 0; nss neither 1 nor n when shift or
 * scale is given; a non-finite shift or scale, by index; a bad window, by index; out_bytes below nw * T elements; more than 2^31 - 1
 * workgroups (of VAD_CUT_WG_SAMPLES samples of a window); a null out with nw > 0; then what vad_scan_levels says about the block's
 * pointer and residency, d_out not 16-byte aligned, d_mask not 4-byte aligned.
 *   Every engine is served.  VAD_ABI_VERSION is unchanged: the presence of vad_scan_audio_batch is how a caller detects the feature.
 */
typedef struct vad_moments {
    int64_t sum_q31;     /* sum of rint(clamp(x, -1, 1) * 2^31) over the segment's samples */
    int64_t energy_q32;  /* vad_level's field */
} vad_moments;           /* 16 bytes */
typedef struct vad_audio_batch {
    int32_t samples;   /* T: samples of a window, a multiple of 4 in 4 .. 2^24 */
    int32_t dtype;     /* VAD_BATCH_F32 / VAD_BATCH_F16 / VAD_BATCH_BF16 */
    int32_t pad_mode;  /* VAD_BATCH_PAD_VALUE / VAD_BATCH_PAD_FEATURE */
    float pad_value;
} vad_audio_batch;
typedef struct vad_audio_window {
    int32_t seg;       /* index into the items */
    int32_t nsamples;  /* 0 .. T */
    int64_t sample0;   /* first sample, within the segment's range: a multiple of 4 */
} vad_audio_window;    /* 16 bytes */
VAD_API int vad_scan_moments(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio /*or NULL*/, int64_t audio_samples,
                             int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, vad_moments *out /*[n]*/);
VAD_API int vad_scan_moments_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                    int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                                    vad_moments *d_out /*on the GPU, [n]*/, void *stream);
VAD_API int vad_scan_audio_batch(vad_engine *e, const vad_cut_item *items, int64_t n, const void *audio /*or NULL*/, int64_t audio_samples,
                                 int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh, const vad_audio_batch *b,
                                 const vad_audio_window *windows /*host*/, int64_t nw, const float *shift /*[nss] or NULL*/,
                                 const float *scale /*[nss] or NULL*/, int64_t nss /*1 or n*/, void *out, int64_t out_bytes,
                                 uint8_t *mask /*[nw][T] or NULL*/);
VAD_API int vad_scan_audio_batch_device(vad_engine *e, const vad_cut_item *items, int64_t n, const void *d_audio, int64_t audio_samples,
                                        int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                                        const vad_audio_batch *b, const vad_audio_window *windows /*host*/, int64_t nw,
                                        const float *shift /*host*/, const float *scale /*host*/, int64_t nss, void *d_out, int64_t out_bytes,
                                        uint8_t *d_mask /*on the GPU or NULL*/, void *stream);

/*
 * Rendered audio: one finished piece of audio per call - the segments of a block faded at their edges, crossfaded where two of
 * them share output samples, joined, everything else silence.  The two standard products of a VAD come out of it by where the caller
 * places the segments: silence removal (the segments back to back, neighbours overlapping by the ramp or a fixed pause apart) and
 * a VAD-driven noise gate (each segment at first_frame * hop of an output as long as the recording).  vad_scan_cut writes hard
 * edges, refuses two segments that share an output sample and leaves every sample outside a segment unwritten; this call is driven
 * by the OUTPUT instead.
 *
 * vad_scan_render.  The items are vad_cut_item, always in the VAD_CUT_RANGE layout: segment i has
 * S_i = vad_cut_samples / vad_rate_cut_samples(nframes, .., VAD_CUT_RANGE) samples and covers out[out_sample .. out_sample + S_i).
 * THE RULE:
 *   1. v_i[k] is the float32 that vad_scan_cut_gain with VAD_CUT_RANGE, VAD_CUT_F32 and the same arguments writes for sample k of
 * segment i: decoded, channel-selected and gated - on a rate block (sr_in as in vad_scan_levels) the input-rate sample, never
 * gated - times gains[i] (a host array [n]; gains == NULL: no factor).
 *   2. w_i[k] = (v_i[k] * a) * b, two float32 multiplies of their own, never fused, in that order: a = ramp[k] if k < nramp, else
 * 1.0f; b = ramp[S_i - 1 - k] if S_i - 1 - k < nramp, else 1.0f.  The one table (host, nramp entries) serves the fade-in, read
 * forwards from the segment's first sample, and the fade-out, read forwards from its last sample; in a segment shorter than
 * 2 * nramp both act on the samples where they meet.  nramp == 0: no ramp.  The shape of the ramp is the caller's: the kernel never
 * computes one, there is no transcendental and no division in the rule.
 *   3. Output sample s is +0.0f where no segment covers it, w itself where one does, and the float32 sum w_i + w_j - one add,
 * commutative: the bytes depend neither on the order of the items nor on scheduling - where two do.  Three or more: refused.  Then
 * the cut's conversion: VAD_CUT_F32 stores the value, VAD_CUT_PCM16 clip(x * 32767, -32768, 32767) toward zero.
 *   4. EVERY sample of out[0 .. out_samples) is written, gaps as zeros: the host form copies the whole range back, the device form
 * needs no memset by the caller.  A pause between joined segments is the caller placing them apart.
 *   audio == NULL: the resident block, as in the cuts; with an audio the call uploads it and it becomes the resident block (n == 0
 * uploads nothing).  Works on every engine, Silero V4 and VAD_ENGINE_SHARED_GPU included: no model kernel runs.  The call first
 * waits for earlier *_device launches that read the engine's tables.
 *   VAD_ERR_INVALID_ARG, each with a message under this function's name and nothing written, in THIS ORDER (a call with several
 * faults gets the first): sr_in (vad_scan_levels'); a negative n, audio_samples or out_samples, null items with n > 0; the frame
 * format and channels; out_fmt; hop and the block's extent; out_samples not a multiple of 4; nramp < 0, above
 * VAD_RENDER_MAX_RAMP or not a multiple of 4; a null ramp with nramp > 0; a ramp entry that is NaN or infinite (the message names
 * the lowest index); then per item in listing order every refusal of vad_scan_cut_gain that concerns the item (its recording's
 * offset, frames, extent in the block, channel, reserved, out_sample and length inside the output, a non-finite gain); an output
 * sample covered by three segments (the message names the sample and all three) or an output of more than 2^31 - 1 workgroups,
 * whichever the sweep over the output meets first; a null out with out_samples > 0; and last what
 * concerns the pointers: with audio == NULL the resident block's refusals, in the device form the alignment of d_audio and d_out.
 * The overlap of TWO segments, which the cuts refuse, is accepted here.  n == 0 with out_samples > 0: VAD_OK, all zeros.
 *   vad_scan_render_device: d_audio and d_out (16-byte aligned, out_samples samples) as vad_scan_cut_device takes them; gains and
 * ramp stay HOST arrays, read before the call returns; enqueues on `stream` (NULL = the engine's own) and returns.
 *   A workgroup of the kernel serves up to VAD_CUT_WG_SAMPLES consecutive output samples with one cover set; gaps are zeroed by
 * workgroups of the same launch.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_render is how a caller detects the feature.
 */
#define VAD_RENDER_MAX_RAMP 65536      /* samples: 1.36 s at 48 kHz, a 256 KiB table */
VAD_API int vad_scan_render(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                            const float *ramp /*host [nramp] or NULL*/, int32_t nramp, const void *audio /*or NULL*/,
                            int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop, float denoise_thresh,
                            int32_t out_fmt, void *out, int64_t out_samples);
VAD_API int vad_scan_render_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                   const float *ramp /*host [nramp] or NULL*/, int32_t nramp, const void *d_audio,
                                   int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                                   float denoise_thresh, int32_t out_fmt, void *d_out, int64_t out_samples, void *stream);

/*
 * Two-channel segment audio: the cut and the render of a TWO-CHANNEL block with both channels kept.  The VAD decides on the mix or
 * on one speaker (the scan's channel); the audio delivered is the recording's.  The argument lists are those of
 * vad_scan_cut_gain / _device and vad_scan_render / _device.  THE RULE:
 *   - out_sample, out_samples and vad_cut_samples / vad_rate_cut_samples count sample FRAMES; the output holds 2 * out_samples
 * values, interleaved L R L R (a two-channel WAV payload for VAD_CUT_PCM16).
 *   - Value (k, c) of vad_scan_cut_stereo is bit for bit what vad_scan_cut_gain writes for sample k with the same arguments and
 * every item's channel = c; gains == NULL means no factor: the bytes of vad_scan_cut.  The gate acts per value, so it may zero one
 * channel of a sample frame and keep the other.
 *   - Value (s, c) of vad_scan_render_stereo is bit for bit what vad_scan_render writes for sample s with every item's
 * channel = c: gain and ramp factors are the same for both channels of a sample frame, the sum where two segments meet is one
 * float32 add per channel, gaps are zeros in both.
 *   Every rule and refusal of the mono calls applies under these names, in the same order: block, hop, offsets and extents,
 * out_sample's alignment to 4 (sample frames), overlapping outputs (cut) and three covers (render), the ramp, non-finite gains, the
 * resident block with audio == NULL, sr_in, the wait for earlier *_device launches.  Refusals of their own, each
 * VAD_ERR_INVALID_ARG with a message and nothing written: channels != 2 ("two-channel blocks only", behind the frame format's
 * check) and an item whose channel is not VAD_SCAN_BOTH (where the mono calls check the channel).  VAD_CUT_FRAMES on a rate block
 * (sr_in 8000 / 24000 / 48000) is VAD_ERR_UNSUPPORTED with a message, behind the layout's check: it would need two resampled rows
 * per chunk; VAD_CUT_RANGE on rate blocks works - input-rate sample frames, never gated, as in mono.  The mono entry points keep
 * refusing channel = VAD_SCAN_BOTH in their present words.
 *   Works on every engine, Silero V4 and VAD_ENGINE_SHARED_GPU included: no model kernel runs.  Device forms: d_audio is 8-byte
 * aligned, d_out 16-byte aligned and holds 2 * out_samples values; gains and ramp stay HOST arrays.
 *   VAD_ABI_VERSION is unchanged: the presence of vad_scan_cut_stereo is how a caller detects the feature.
 */
#define VAD_SCAN_BOTH (-2)
VAD_API int vad_scan_cut_stereo(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                const void *audio /*or NULL*/, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in,
                                int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *out, int64_t out_samples);
VAD_API int vad_scan_cut_stereo_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                       const void *d_audio, int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in,
                                       int32_t hop, float denoise_thresh, int32_t layout, int32_t out_fmt, void *d_out,
                                       int64_t out_samples, void *stream);
VAD_API int vad_scan_render_stereo(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                   const float *ramp /*host [nramp] or NULL*/, int32_t nramp, const void *audio /*or NULL*/,
                                   int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                                   float denoise_thresh, int32_t out_fmt, void *out, int64_t out_samples);
VAD_API int vad_scan_render_stereo_device(vad_engine *e, const vad_cut_item *items, int64_t n, const float *gains /*host [n] or NULL*/,
                                          const float *ramp /*host [nramp] or NULL*/, int32_t nramp, const void *d_audio,
                                          int64_t audio_samples, int32_t channels, int frame_fmt, int32_t sr_in, int32_t hop,
                                          float denoise_thresh, int32_t out_fmt, void *d_out, int64_t out_samples, void *stream);

/*
 * Pipelined host ingest.  vad_step* on host pointers are copy -> kernel -> copy -> wait; at 8 192 streams the PCIe copy is
 * 5-8 x the kernel, so a serving loop should overlap the copy of tick t+1 with the kernel of tick t:
 *
 *     vad_step_submit(e, slots, n, T, frames_t1, fmt, thr, &ticket1);     // enqueues H2D -> kernel -> D2H, returns at once
 *     vad_step_collect(e, ticket0, probs, events, seg);                   // blocks until tick t's results are on the host
 *
 * Up to 2 tickets may be outstanding (a third submit returns VAD_ERR_BUSY); each ticket is collected exactly once, in any
 * order.  `frames` must stay valid and unchanged until its ticket is collected; allocate it
 * with vad_host_alloc for a true asynchronous DMA (a pageable buffer works, but the runtime then stages it synchronously).
 * Kernels of successive tickets run in submission order on the engine's stream, so a slot may appear in consecutive
 * tickets.  Results are identical, bit for bit, to vad_step_multi on the same inputs.
 * The reference has no counterpart: it calls session.run synchronously per frame (core/silero_model.py:433, 471-499).
 */
VAD_API int vad_step_submit(vad_engine *e, const int64_t *slots, int64_t n, int32_t T, const void *frames, int frame_fmt,
                            float denoise_thresh, int64_t *ticket);
VAD_API int vad_step_collect(vad_engine *e, int64_t ticket, float *probs_out /*[n][T]*/, uint8_t *events_out /*[n][T] or NULL*/,
                             int32_t *seg_frames_out /*[n] or NULL*/);

/*
 * AudioUtils.resample_audio (utils/audio.py:19-55 -> scipy.signal.resample, Fourier method)
 * for n streams: in [n][n_in] float32 at sr_in -> out [n][512] float32 at 16 kHz, one
 * 512-sample output chunk per call (n_in = 512 * sr_in / 16000: 256 / 768 / 1536).
 */
VAD_API int vad_resample(vad_engine *e, const float *in, int64_t n, int32_t n_in, int32_t sr_in, float *out);
VAD_API int vad_resample_device(vad_engine *e, const float *d_in, int64_t n, int32_t n_in, int32_t sr_in, float *d_out,
                        void *stream);
/* the same for up to 4 segments of different input rates in ONE launch (a tick's 8 / 24 / 48 kHz clients): segment k is
 * d_in[k] [n[k]][n_in[k]] at sr_in[k] -> d_out[k] [n[k]][512]; the tables are host arrays, the buffers device pointers */
#define VAD_RESAMPLE_MAX_SEGMENTS 4
VAD_API int vad_resample_multi_device(vad_engine *e, int32_t nseg, const float *const *d_in, const int64_t *n,
                                      const int32_t *n_in, const int32_t *sr_in, float *const *d_out, void *stream);

/*
 * AudioUtils.resample_audio for EVERY input the reference function accepts (utils/audio.py:39-49): the whole array goes through
 * scipy.signal.resample(x, int(len(x) * target_rate / original_rate)) - any length, any pair of rates.  The caller computes
 * n_out exactly as the reference does (Python float arithmetic, utils/audio.py:43-46); only the two lengths enter the maths.
 * in [rows][n_in] float32 (in_f64 = 0) or float64 (in_f64 = 1: scipy transforms float64 / integer arrays in double precision)
 * -> out [rows][n_out] float32 (the reference's .astype(np.float32), :49); rows = independent arrays of one length (the
 * columns of an [N, C] array: scipy resamples along axis 0).  Two kernels behind it, chosen by size: below 2^25 operator
 * entries (rows * n_in * n_out) every entry is evaluated where it is used, in float64, never stored (csrc/resample_generic.hip:
 * lowest latency, 70 us for 100 -> 50, 80 us for three 48 kHz chunks); from there the same function runs as two chirp-z
 * transforms on power-of-two float64 FFTs (csrc/resample_fft.hip: O(n log n) for any pair of lengths, up to 2^25 samples = 11
 * minutes of 48 kHz audio; host buffers in and out: 0.14 ms for one second of 48 kHz audio, 0.33 ms for ten, 18.5 ms for ten
 * minutes of 44.1 kHz - 2 x, 9 x and 22 x scipy on the box's host).  Beyond both (n > 2^25 and rows * n_in * n_out > 2^42): VAD_ERR_UNSUPPORTED - never cut into pieces,
 * the result of a cut array is NOT the reference's.
 * The _device form takes device pointers and is synchronous as well (the result is complete on return).
 */
VAD_API int vad_resample_generic(vad_engine *e, const void *in, int in_f64, int64_t rows, int64_t n_in, int64_t n_out, float *out);
VAD_API int vad_resample_generic_device(vad_engine *e, const void *d_in, int in_f64, int64_t rows, int64_t n_in, int64_t n_out,
                                        float *d_out);

/*
 * Tick assembler: the serving loop's side of vad_step_events, in C.  The reference runs the model inside every websocket's
 * receive loop, one client and one frame at a time (websocket_service/server/vad_websocket_server.py:326-382); a shared-pool
 * server instead collects the frames that arrived since the last tick and advances all those streams together:
 *
 *   vad_tick_push(e, slot, samples, nsamples, fmt, gate_on)   from any thread, as frames arrive: the frame is written straight
 *       into the page-locked staging row of the coming tick, right-zero-padded / truncated to the engine's frame length exactly
 *       as _prepare_audio_input does (core/silero_model.py:464-468).  One frame per slot and tick: a slot's further frames
 *       queue up and are fed in submission order, one per later tick (at most 256 waiting: VAD_ERR_BUSY).
 *   vad_tick_run(e, thr, &res)   advances every slot that has a frame by ONE frame - one launch per (frame format, gate)
 *       group, i.e. one launch when all clients speak one format - and returns compact arrays: res.slots[i], res.probs[i],
 *       res.events[i] (VAD_EV_* bits), res.seg_frames[i]; entries group_start[g] .. group_start[g+1]-1 belong to group
 *       g = frame_fmt * 2 + gate_on, in push order, and group_frames[g] is that group's staged audio [count][frame] in frame_fmt
 *       (what segment assembly keeps).  All pointers are engine-owned and stay valid until the next vad_tick_run.
 *       Pushes may continue while a tick runs (double-buffered staging).  `thr` is the gate threshold of the gate_on groups.
 *       Frames that waited are placed first, in the order their slots started waiting, then the frames pushed since, in push order.
 *       A tick that FAILS (a HIP error) has consumed its frames: res.n / res.slots / res.nsamples then list the streams that lost
 *       one (res.probs is NULL), everything queued behind them is intact and the next tick carries on.
 *   vad_tick_cancel(e, slot)   drops the slot's pending frames and segment audio.  vad_stream_close and vad_stream_open do the same
 *       for their slot, so a recycled slot never sees its predecessor's frames.
 *   vad_tick_pending(e, slot, &frames)   frames of `slot` that have not been stepped yet (staged + waiting).
 *   vad_tick_push_rate(e, slot, samples, nsamples, fmt, gate_on, sr_in)   the same for a client whose audio arrives at 8 / 24 /
 *       48 kHz (VADConfig.auto_convert_sample_rate; nsamples must be the chunk that yields one 16 kHz frame: 256 / 768 / 1536):
 *       the chunk is staged as float32 in group 6 + 3 * gate_on + {0, 1, 2}; vad_tick_run resamples those groups on the GPU and
 *       steps them like vad_step_rates (one fused launch when it fits); group_frames[g] then holds the chunks at their own rate
 *       [count][nsamples] float32 - what the segment keeps.  16 kHz engines only.
 */
#define VAD_TICK_GROUPS 12
typedef struct vad_tick_result {
    uint32_t struct_size;          /* sizeof(vad_tick_result) */
    int64_t n;
    const int64_t *slots;
    const float *probs;
    const uint8_t *events;
    const int32_t *seg_frames;
    int64_t group_start[VAD_TICK_GROUPS + 1];
    const void *group_frames[VAD_TICK_GROUPS];
    const int32_t *nsamples;       /* samples the caller pushed for entry i (before padding / truncation to the frame length) */
    float host_us[3];              /* where this tick's wall time went: buffer swap + queued frames | copies + launches + wait | segment assembly */
    int64_t dropped;               /* ABI 3: staged frames left out because their stream was closed (or closed and reopened) after the push */
    int64_t staged_next;           /* ABI 3: frames that had been waiting and are already staged for the NEXT tick - a ticker that sees
                                      > 0 runs again at once instead of sleeping (a client that sends faster than real time) */
} vad_tick_result;
VAD_API int vad_tick_push(vad_engine *e, int64_t slot, const void *samples, int32_t nsamples, int frame_fmt, int gate_on);
VAD_API int vad_tick_push_rate(vad_engine *e, int64_t slot, const void *samples, int32_t nsamples, int frame_fmt, int gate_on,
                               int32_t sr_in);
/* the same frame length / format / gate for n slots: frames [n][nsamples] (a front end that batches its sockets' frames) */
VAD_API int vad_tick_push_many(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int32_t nsamples,
                               int frame_fmt, int gate_on);
/* the same, but every frame is tried and status[i] receives its own result (VAD_OK, VAD_ERR_BAD_SLOT, VAD_ERR_BUSY ...): a
 * front end that coalesces the frames its sockets received during one tick window into ONE call learns which of them to
 * report to which client; returns the first failure (the last-error text belongs to the LAST one) */
VAD_API int vad_tick_push_status(vad_engine *e, const int64_t *slots, int64_t n, const void *frames, int32_t nsamples,
                                 int frame_fmt, int gate_on, int32_t *status);
/* the same with one pointer per frame (frames[i] -> nsamples samples): the sockets' receive buffers are copied straight into the
 * tick's staging rows, without being gathered into one array first */
VAD_API int vad_tick_push_gather(vad_engine *e, const int64_t *slots, int64_t n, const void *const *frames, int32_t nsamples,
                                 int frame_fmt, int gate_on, int32_t *status);
/* vad_tick_push_rate for n clients at ONE input rate, one pointer per chunk, a result per chunk: what vad_tick_push_gather is for
 * frames at the engine's rate (the reference declares this conversion and leaves it empty, vad_wrapper.py:621-624; its server
 * would call it once per message, vad_websocket_server.py:326-382).  int16 chunks are scaled to float32 on the way in. */
VAD_API int vad_tick_push_rate_gather(vad_engine *e, const int64_t *slots, int64_t n, const void *const *frames, int32_t nsamples,
                                      int frame_fmt, int gate_on, int32_t sr_in, int32_t *status);
VAD_API int vad_tick_cancel(vad_engine *e, int64_t slot);
VAD_API int vad_tick_pending(vad_engine *e, int64_t slot, int64_t *frames);
/*
 * Segment assembly inside the tick (off by default).  When on, vad_tick_run also does the host half of
 * VADProcessor._process_voice_state (core/silero_model.py:838-869, 891-895, 925-949) for every stepped stream, on the staged
 * audio converted to float32 and gated like the model input (utils/audio.py:117-118): frames at or above the slot's
 * vad_start_probability collect as pre-roll, START turns the pre-roll into the segment, frames of an open segment are appended
 * (whole frames, also beyond the model's 512 samples), END closes it.  vad_tick_take_segment then hands over the finished
 * segment's samples (out = NULL: size query; taking clears it) - the payload of voice_end_callback before WAV encoding.
 * A serving loop then touches a stream in its own language only on START / END.
 */
VAD_API int vad_tick_enable_segments(vad_engine *e, int on);
VAD_API int vad_tick_take_segment(vad_engine *e, int64_t slot, float *out, int64_t cap, int64_t *nsamples);
/* A stream's segment audio (pre-roll, open segment, finished segment not yet taken) as an opaque blob: with vad_stream_save /
 * vad_stream_restore this is everything a session needs to continue on ANOTHER engine (another GPU) in the middle of an
 * utterance.  buf = NULL: size query.  Restore replaces what the slot holds; blobs are checked before anything is touched. */
VAD_API int vad_tick_segment_save(vad_engine *e, int64_t slot, void *buf, int64_t cap, int64_t *nbytes);
VAD_API int vad_tick_segment_restore(vad_engine *e, int64_t slot, const void *buf, int64_t nbytes);
VAD_API int vad_tick_run(vad_engine *e, float denoise_thresh, vad_tick_result *out);

/*
 * ABI 4: vad_tick_run + the per-session bookkeeping a serving front end does with its result, in the same call - so that a
 * front end whose callbacks live in an interpreter touches only the sessions that HAVE something to hear (the reference does all
 * of this per frame and client in Python: VADProcessor.process_frame / VADWrapper._handle_callbacks,
 * core/silero_model.py:723-762, core/vad_wrapper.py:478-522).
 *   in  (caller-owned, one entry per slot, n_slots entries; updated for every stepped slot i = slots[k]):
 *         last_prob[i] = probs[k];  frames_done[i] += 1;  active[i] = (active[i] | START) & !END   ("inside a segment")
 *       continue_cb[i] / continue_payload[i]: the session registered a voice_continue callback / wants the frame's bytes with it
 *   out (engine-owned, valid until the next tick): the entries k of the tick's arrays the caller has work for, in order, with
 *       work_kind[j] = VAD_WORK_START | VAD_WORK_END (the tick's event bits) | VAD_WORK_CONTINUE (the session was inside a segment
 *       before this frame and has a voice_continue callback: vad_wrapper.py:513-519) | VAD_WORK_PAYLOAD (... which wants the bytes)
 *       | VAD_WORK_LONG (the pushed frame was longer than the model's frame: the caller kept the whole frame, vad_tick_push)
 * Entries without any of these (idle sessions, sessions talking without a continue callback) are not listed.
 */
#define VAD_WORK_START 1
#define VAD_WORK_END 2
#define VAD_WORK_CONTINUE 4
#define VAD_WORK_PAYLOAD 8
#define VAD_WORK_LONG 16
#define VAD_WORK_REJECTED 32   /* ABI 5: the entry's frame was rejected (VAD_EV_REJECTED): the slot's last_prob / frames_done / active are
                                  left as they were; LONG keeps its meaning */
typedef struct vad_tick_work {
    uint32_t struct_size;          /* sizeof(vad_tick_work) */
    int64_t n_slots;               /* length of the five arrays below */
    float *last_prob;
    int64_t *frames_done;
    uint8_t *active;
    const uint8_t *continue_cb;
    const uint8_t *continue_payload;
    int64_t n_work;                /* out */
    const int32_t *work_index;     /* out: k into vad_tick_result's arrays */
    const uint8_t *work_kind;      /* out */
    const int64_t *work_samples;   /* out: VAD_WORK_END entries: samples of the finished segment (vad_tick_take_segment*), else 0 */
} vad_tick_work;
VAD_API int vad_tick_run_work(vad_engine *e, float denoise_thresh, vad_tick_result *out, vad_tick_work *work);

/*
 * ABI 4: vad_tick_take_segment as the finished payload of voice_end_callback: 44-byte RIFF/WAVE header + int16 PCM, byte for
 * byte what WAVWriter.write_wav_data makes of the segment (utils/wav_writer.py:40-136: clip(x * 32767, -32768, 32767) truncated
 * to int16, mono).  out == NULL: size query (*nbytes = 44 + 2 * samples; vad_tick_work.work_samples has the count already).
 * The segment is released when it has been written.
 */
VAD_API int vad_tick_take_segment_wav16(vad_engine *e, int64_t slot, int32_t sample_rate, void *out, int64_t cap, int64_t *nbytes);

/*
 * One tick for streams whose audio arrives at another rate: VADConfig.auto_convert_sample_rate.  The reference's hook for it
 * is core/vad_wrapper.py:621-624 - a `pass` - and the function it was meant to call is AudioUtils.resample_audio
 * (utils/audio.py:19-55); this entry point is that path, on the GPU: segment k holds n[k] chunks of one tick at sr_in[k]
 * (256 samples @ 8 kHz, 768 @ 24 kHz, 1536 @ 48 kHz - one 512-sample 16 kHz frame each; 512 @ 16 kHz passes through, as
 * resample_audio does at :39-40); all segments are resampled in ONE launch into engine-owned HBM and every stream advances one
 * frame in ONE model launch right behind it on the same HIP stream - the 16 kHz frames never travel.  A Silero V5 engine serves
 * ticks that fit one 16-stream tile per CU (each segment padded to whole tiles: at most 256 tiles, ~4 000 streams) with ONE
 * fused launch instead: every tile resamples its own chunks into LDS and steps the model from there (results equal the
 * two-launch form to rounding).  slots / probs / events / seg_frames are the
 * concatenation of the segments, in order.  16 kHz engines only (Silero V5, or V4's 16 kHz sub-model).
 * The device form is asynchronous like vad_step_device and follows its slot rules; calls on one engine must use one stream.
 */
VAD_API int vad_step_rates_device(vad_engine *e, int32_t nseg, const float *const *d_in, const int64_t *n, const int32_t *sr_in,
                                  const int32_t *d_slots, float denoise_thresh, float *d_probs, uint8_t *d_events,
                                  int32_t *d_seg_frames, void *stream);
VAD_API int vad_step_rates(vad_engine *e, int32_t nseg, const float *const *in, const int64_t *n, const int32_t *sr_in,
                           const int64_t *slots, float denoise_thresh, float *probs_out, uint8_t *events_out,
                           int32_t *seg_frames_out);

/*
 * Diagnostic (no GPU needed): run the host-side weight packer and return the per-wave MFMA
 * weight streams exactly as vad_engine_create uploads them.  out may be NULL to query the size.
 * sect_out receives [4 waves][16 sections] block offsets (1 block = 256 floats).  Used by the
 * CPU test-suite to check the packed layout against a NumPy model of the kernel's dataflow.
 * model_version 4, 5; 416, 516 = the packings of the 16-stream tile kernels; 5161 = the second
 * stream of the 516 packing (encoder.0 on bf16 splits, uploaded as a buffer of its own); 5162 =
 * its third stream (encoder.1 on bf16 splits), with the same section table; 5163 = the blocks
 * uploaded behind the third stream (encoder.2 and encoder.3 on bf16 splits, no section entry).
 */
VAD_API int vad_debug_pack_weights(int32_t model_version, const void *weights, size_t weights_len, float *out,
                                   size_t out_floats, size_t *n_floats, uint32_t *sect_out);

/*
 * Diagnostic (no GPU needed): the dense operator R[512][n_in] (row-major) the resampler kernel
 * applies for chunks of n_in samples; the CPU test-suite checks R @ x against scipy.signal.resample.
 */
VAD_API int vad_debug_resample_operator(int32_t n_in, float *R, size_t r_floats);
/* rows m0 .. m1-1 of the operator vad_resample_generic applies, R[(m - m0) * n_in + n] in float64, evaluated on the HOST with the
 * arithmetic of the kernel (same tables, same small-angle rule): the CPU test-suite checks R @ x against scipy for awkward shapes */
/* which kernel vad_resample_generic uses: 0 = chosen by size (default), 1 = the direct kernel, 2 = the chirp-z / FFT path (tests, benchmarks) */
VAD_API int vad_debug_resample_path(vad_engine *e, int mode);
VAD_API int vad_debug_resample_generic_entries(int64_t n_in, int64_t n_out, int64_t m0, int64_t m1, double *R, size_t r_doubles);

/*
 * Diagnostic (no GPU needed): the folded, MFMA-packed form of that operator exactly as the kernel
 * streams it (csrc/pack_weights.cpp: pack_resample_operator).  out may be NULL to query n_floats.
 * tile_blocks = 1 KiB blocks per 32-row tile, row128_block = first block of the VALU row.
 */
VAD_API int vad_debug_pack_resample(int32_t n_in, float *out, size_t out_floats, size_t *n_floats,
                                    uint32_t *tile_blocks, uint32_t *row128_block);

/* the same operator as the fused resample -> step kernel streams it (16 x 16 x 4 tiles: pack_resample_operator_t16);
 * wave_blocks = 1 KiB blocks per wave, which also tells the kernel the stream's shape: 4 vector blocks + 8 per k-iteration of 16
 * folded samples - over n_in / 4 samples per part (every sample contracted), or over n_in / 6 for n_in = 768 / 1536 (24 / 48 kHz:
 * every third input sample sits on an output instant and is copied) - or, for n_in = 256 (8 kHz: the even outputs are the input
 * samples), 2 vector blocks + 4 per k-iteration: only the odd output rows */
VAD_API int vad_debug_pack_resample_t16(int32_t n_in, float *out, size_t out_floats, size_t *n_floats,
                                        uint32_t *wave_blocks, uint32_t *row128_block);

/*
 * Diagnostic: replay a scripted probability sequence through ONE slot's device-side state
 * machine (the code path vad_step_events runs after the model).  probs [n] -> events_out [n],
 * seg_frames_out [n] (segment length in frames on END, else 0).  Lets the GPU test-suite check
 * the hysteresis logic against the reference's own traces without needing audio that produces
 * a given probability sequence.
 */
VAD_API int vad_debug_sm_replay(vad_engine *e, int64_t slot, const float *probs, int64_t n, uint8_t *events_out,
                                int32_t *seg_frames_out);

/*
 * Diagnostic: which kernel shape serves the step calls.  0 (default) = the engine's choice - Silero V5 (both sub-models): one-frame
 * calls run on 16-stream tiles whatever their size (the single-frame instantiation of that kernel fits two workgroups on a CU),
 * multi-frame calls on 16-stream tiles up to 4 096 streams and on 32-stream tiles above; Silero V4 (both sub-models): always
 * 16-stream tiles, two workgroups per CU.  16 / 32 force one shape (the test-suite checks that both give the same results to
 * rounding; tools/bench_configs.py times them).
 * -1 / -2: vad_step_rates as two launches (resample, then model) / as the fused launch (default), for the same comparison.
 * Paired tiles: a one-frame call of Silero V5's 16 kHz model on 16-stream tiles, float32 or int16 frames, with MORE tiles than the
 * device has compute units runs two tiles per workgroup (512 threads; the tiles share every bf16 weight fragment the CU fetches) -
 * the same results bit for bit; up to one tile per CU nothing changes.  -3 pairs at every size (the test-suite), -4 never pairs (A/B
 * runs on one build); they leave the tile shape as it is, and 0, 16 and 32 set the pairing back to this default.
 */
VAD_API int vad_debug_set_tile(vad_engine *e, int32_t streams_per_tile);

/* block until everything enqueued on the engine's own stream has finished */
VAD_API int vad_engine_synchronize(vad_engine *e);

/*
 * Page-locked host memory for the caller's frame / result buffers.  The host-pointer entry points
 * (vad_step, vad_step_events, vad_step_multi, vad_resample) accept ANY host pointer; buffers from
 * this allocator are DMA'd directly (no runtime staging copy), which is what bounds a large batch:
 * 8 192 f32 frames are 16.8 MB per step.  The reference has no counterpart (numpy arrays handed to
 * onnxruntime, silero_model.py:471-499); the Python mirror exposes it as Engine.pinned_array().
 * Memory stays valid until vad_host_free or vad_engine_destroy.
 */
VAD_API int vad_host_alloc(vad_engine *e, size_t bytes, void **out);
VAD_API int vad_host_free(vad_engine *e, void *p);

#ifdef __cplusplus
}
#endif
#endif /* VAD_ENGINE_H */
