"""ctypes binding of ``include/vad_engine.h`` (the C ABI of the HIP engine).

Loading fails loudly when ``libvad_engine.so`` is missing — there is no Python or CPU
substitute for it.  The library itself loads without a GPU (so the CPU test-suite can check
its exports and the host-side weight packer); creating an engine without a usable gfx950
device fails with ``VAD_ERR_NO_DEVICE``.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvad_engine.so")

VAD_OK = 0
VAD_ERR_INVALID_ARG = -1
VAD_ERR_NO_DEVICE = -2
VAD_ERR_BAD_WEIGHTS = -3
VAD_ERR_HIP = -4
VAD_ERR_NO_SLOT = -5
VAD_ERR_BAD_SLOT = -6
VAD_ERR_UNSUPPORTED = -7
VAD_ERR_BUSY = -8

VAD_FMT_F32, VAD_FMT_I16_32767, VAD_FMT_I16_32768 = 0, 1, 2
VAD_FMT_ULAW8, VAD_FMT_ALAW8 = 3, 4         # ITU-T G.711, one byte per sample (include/vad_engine.h)
G711_LAWS = {"ulaw": VAD_FMT_ULAW8, "alaw": VAD_FMT_ALAW8}
VAD_EV_START, VAD_EV_END, VAD_EV_CONTINUE = 1, 2, 4
VAD_EV_REJECTED = 0x80          # ABI 5: the frame held a NaN / Inf sample (include/vad_engine.h); probability NaN, state untouched
VAD_FRAME_SAMPLES = 512
VAD_STATE_FLOATS = 256
VAD_STREAM_SAVE_BYTES = 1120


class EngineDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("model_version", C.c_int32),
        ("weights", C.c_void_p),
        ("weights_len", C.c_size_t),
        ("device_id", C.c_int32),
        ("max_streams", C.c_int32),
        ("sample_rate", C.c_int32),
        ("flags", C.c_uint32),
    ]


class EngineInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("abi_version", C.c_int32),
        ("model_version", C.c_int32),
        ("device_id", C.c_int32),
        ("max_streams", C.c_int32),
        ("open_streams", C.c_int32),
        ("compute_units", C.c_int32),
        ("streams_per_workgroup", C.c_int32),
        ("weight_bytes_device", C.c_int64),
        ("state_bytes_device", C.c_int64),
        ("steps", C.c_int64),
        ("frames", C.c_int64),
        ("device_name", C.c_char * 64),
        ("arch", C.c_char * 32),
        ("frame_samples", C.c_int32),
        ("sample_rate", C.c_int32),
    ]


class Thresholds(C.Structure):
    _fields_ = [
        ("start_probability", C.c_double),
        ("end_probability", C.c_double),
        ("start_ratio", C.c_double),
        ("end_ratio", C.c_double),
        ("start_frame_count", C.c_int32),
        ("end_frame_count", C.c_int32),
    ]


class TickResult(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n", C.c_int64),
        ("slots", C.POINTER(C.c_int64)),
        ("probs", C.POINTER(C.c_float)),
        ("events", C.POINTER(C.c_uint8)),
        ("seg_frames", C.POINTER(C.c_int32)),
        ("group_start", C.c_int64 * 13),
        ("group_frames", C.c_void_p * 12),
        ("nsamples", C.POINTER(C.c_int32)),
        ("host_us", C.c_float * 3),
        ("dropped", C.c_int64),
        ("staged_next", C.c_int64),
    ]


class TickWork(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_slots", C.c_int64),
        ("last_prob", C.POINTER(C.c_float)),
        ("frames_done", C.POINTER(C.c_int64)),
        ("active", C.POINTER(C.c_uint8)),
        ("continue_cb", C.POINTER(C.c_uint8)),
        ("continue_payload", C.POINTER(C.c_uint8)),
        ("n_work", C.c_int64),
        ("work_index", C.POINTER(C.c_int32)),
        ("work_kind", C.POINTER(C.c_uint8)),
        ("work_samples", C.POINTER(C.c_int64)),
    ]


class ScanItem(C.Structure):
    _fields_ = [("slot", C.c_int64), ("sample_offset", C.c_int64), ("nsamples", C.c_int64)]


class ScanChItem(C.Structure):
    _fields_ = [("slot", C.c_int64), ("sample_offset", C.c_int64), ("nsamples", C.c_int64), ("channel", C.c_int32),
                ("reserved", C.c_int32)]


VAD_SCAN_MIX = -1
VAD_SCAN_BOTH = -2     # vad_scan_cut_stereo / vad_scan_render_stereo: both channels are written


class CutItem(C.Structure):
    _fields_ = [("sample_offset", C.c_int64), ("first_frame", C.c_int64), ("nframes", C.c_int64), ("out_sample", C.c_int64),
                ("channel", C.c_int32), ("reserved", C.c_int32)]


VAD_CUT_FRAMES, VAD_CUT_RANGE = 0, 1
VAD_CUT_PCM16, VAD_CUT_F32 = 0, 1
VAD_CUT_WG_SAMPLES = 4096
VAD_RENDER_MAX_RAMP = 65536
VAD_RESAMPLE_CUT_MAX_TAPS = 511
VAD_RESAMPLE_CUT_WG_SAMPLES = 2048
VAD_CONVERT_MAX_REACH = 128
VAD_CONVERT_MIN_RATE, VAD_CONVERT_MAX_RATE, VAD_CONVERT_MAX_PERIOD = 4000, 192000, 640
VAD_CONVERT_WG_SAMPLES = 2048
CUT_LAYOUTS = {"frames": VAD_CUT_FRAMES, "range": VAD_CUT_RANGE}
CUT_OUTPUTS = {"pcm16": VAD_CUT_PCM16, "f32": VAD_CUT_F32}


class Level(C.Structure):
    _fields_ = [("energy_q32", C.c_int64), ("peak", C.c_float), ("clipped", C.c_int32)]


# the same record as a numpy structured dtype: the levels of n segments are np.ndarray(n, LEVEL_DTYPE)
LEVEL_DTYPE = np.dtype([("energy_q32", np.int64), ("peak", np.float32), ("clipped", np.int32)])


class Mel(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("n_bins", C.c_int32), ("n_mels", C.c_int32), ("pad", C.c_int32),
                ("log", C.c_int32), ("floor", C.c_float), ("reserved", C.c_int32)]


VAD_MEL_PAD_NONE, VAD_MEL_PAD_REFLECT = 0, 1
VAD_MEL_LINEAR, VAD_MEL_LN, VAD_MEL_LOG10 = 0, 1, 2
MEL_PADS = {"none": VAD_MEL_PAD_NONE, "reflect": VAD_MEL_PAD_REFLECT}
MEL_LOGS = {"linear": VAD_MEL_LINEAR, "ln": VAD_MEL_LN, "log10": VAD_MEL_LOG10}


class Batch(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("frames", C.c_int32), ("deltas", C.c_int32), ("layout", C.c_int32), ("dtype", C.c_int32),
                ("pad_mode", C.c_int32), ("pad_value", C.c_float), ("reserved", C.c_int32)]


class BatchWindow(C.Structure):
    _fields_ = [("seg", C.c_int32), ("nrows", C.c_int32), ("row0", C.c_int64)]


# the same record as a numpy structured dtype: the windows of a batch are np.ndarray(nw, BATCH_WINDOW_DTYPE)
BATCH_WINDOW_DTYPE = np.dtype([("seg", np.int32), ("nrows", np.int32), ("row0", np.int64)])


class BatchPiece(C.Structure):
    _fields_ = [("seg", C.c_int32), ("nrows", C.c_int32), ("row0", C.c_int64), ("window", C.c_int32), ("offset", C.c_int32)]


# the pieces of a packed batch are np.ndarray(np, BATCH_PIECE_DTYPE)
BATCH_PIECE_DTYPE = np.dtype([("seg", np.int32), ("nrows", np.int32), ("row0", np.int64), ("window", np.int32), ("offset", np.int32)])

VAD_STATS_MAX_ROWS = 131072
VAD_BATCH_F32, VAD_BATCH_F16, VAD_BATCH_BF16 = 0, 1, 2
VAD_BATCH_CHANNEL_MAJOR, VAD_BATCH_TIME_MAJOR = 0, 1
VAD_BATCH_PAD_VALUE, VAD_BATCH_PAD_FEATURE = 0, 1
BATCH_DTYPES = {"f32": VAD_BATCH_F32, "f16": VAD_BATCH_F16, "bf16": VAD_BATCH_BF16}
BATCH_LAYOUTS = {"channel": VAD_BATCH_CHANNEL_MAJOR, "time": VAD_BATCH_TIME_MAJOR}
BATCH_PADS = {"value": VAD_BATCH_PAD_VALUE, "feature": VAD_BATCH_PAD_FEATURE}


class Moments(C.Structure):
    _fields_ = [("sum_q31", C.c_int64), ("energy_q32", C.c_int64)]


# the moments of n segments are np.ndarray(n, MOMENTS_DTYPE)
MOMENTS_DTYPE = np.dtype([("sum_q31", np.int64), ("energy_q32", np.int64)])


class AudioBatchRecord(C.Structure):
    _fields_ = [("samples", C.c_int32), ("dtype", C.c_int32), ("pad_mode", C.c_int32), ("pad_value", C.c_float)]


class AudioWindow(C.Structure):
    _fields_ = [("seg", C.c_int32), ("nsamples", C.c_int32), ("sample0", C.c_int64)]


# the windows of an audio batch are np.ndarray(nw, AUDIO_WINDOW_DTYPE)
AUDIO_WINDOW_DTYPE = np.dtype([("seg", np.int32), ("nsamples", np.int32), ("sample0", np.int64)])


class Segment(C.Structure):
    _fields_ = [("item", C.c_int32), ("first_frame", C.c_int32), ("nframes", C.c_int32), ("counted", C.c_int32),
                ("mean_prob", C.c_float), ("max_prob", C.c_float)]


# the same record as a numpy structured dtype: a table of vad_segment is np.ndarray(count, SEGMENT_DTYPE)
SEGMENT_DTYPE = np.dtype([("item", np.int32), ("first_frame", np.int32), ("nframes", np.int32), ("counted", np.int32),
                          ("mean_prob", np.float32), ("max_prob", np.float32)])

class Refine(C.Structure):
    _fields_ = [("pad_before", C.c_int32), ("pad_after", C.c_int32), ("merge_gap", C.c_int32), ("min_frames", C.c_int32),
                ("max_frames", C.c_int32), ("reserved", C.c_int32)]


# a host table of no records still needs an address: a null segs_in names vad_scan_refine's resident table
EMPTY_TABLE = np.zeros(1, SEGMENT_DTYPE)

VAD_WORK_START, VAD_WORK_END, VAD_WORK_CONTINUE, VAD_WORK_PAYLOAD, VAD_WORK_LONG = 1, 2, 4, 8, 16
VAD_WORK_REJECTED = 32

# name -> (restype, argtypes); mirrors include/vad_engine.h one-to-one
_vp, _i64p, _f32p, _u8p, _i32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
SIGNATURES = {
    "vad_engine_create": (C.c_int, [C.POINTER(EngineDesc), C.POINTER(_vp)]),
    "vad_engine_destroy": (None, [_vp]),
    "vad_last_error": (C.c_char_p, [_vp]),
    "vad_last_create_error": (C.c_char_p, []),
    "vad_engine_info": (C.c_int, [_vp, C.POINTER(EngineInfo)]),
    "vad_stream_open": (C.c_int, [_vp, _i64p]),
    "vad_stream_open_many": (C.c_int, [_vp, C.c_int64, _i64p]),
    "vad_stream_close": (C.c_int, [_vp, C.c_int64]),
    "vad_stream_reset": (C.c_int, [_vp, _i64p, C.c_int64]),
    "vad_stream_get_state": (C.c_int, [_vp, C.c_int64, _f32p]),
    "vad_stream_set_state": (C.c_int, [_vp, C.c_int64, _f32p]),
    "vad_stream_set_thresholds": (C.c_int, [_vp, C.c_int64, C.POINTER(Thresholds)]),
    "vad_stream_set_thresholds_many": (C.c_int, [_vp, _i64p, C.c_int64, C.POINTER(Thresholds), C.c_int64]),
    "vad_stream_save": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64]),
    "vad_stream_restore": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64]),
    "vad_step": (C.c_int, [_vp, _i64p, C.c_int64, _vp, C.c_int, C.c_float, _f32p]),
    "vad_step_events": (C.c_int, [_vp, _i64p, C.c_int64, _vp, C.c_int, C.c_float, _f32p, _u8p, _i32p]),
    "vad_step_multi": (C.c_int, [_vp, _i64p, C.c_int64, C.c_int32, _vp, C.c_int, C.c_float, _f32p, _u8p]),
    "vad_step_device": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int, C.c_float, _vp, _vp, _vp, _vp]),
    "vad_step_multi_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int, C.c_float, _vp, _vp, _vp, _vp]),
    "vad_step_submit": (C.c_int, [_vp, _i64p, C.c_int64, C.c_int32, _vp, C.c_int, C.c_float, _i64p]),
    "vad_step_collect": (C.c_int, [_vp, C.c_int64, _f32p, _u8p, _i32p]),
    "vad_tick_push": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.c_int, C.c_int]),
    "vad_tick_push_rate": (C.c_int, [_vp, C.c_int64, _vp, C.c_int32, C.c_int, C.c_int, C.c_int32]),
    "vad_tick_push_rate_gather": (C.c_int, [_vp, _i64p, C.c_int64, C.POINTER(C.c_char_p), C.c_int32, C.c_int, C.c_int, C.c_int32, _i32p]),
    "vad_tick_cancel": (C.c_int, [_vp, C.c_int64]),
    "vad_tick_push_many": (C.c_int, [_vp, _i64p, C.c_int64, _vp, C.c_int32, C.c_int, C.c_int]),
    "vad_tick_enable_segments": (C.c_int, [_vp, C.c_int]),
    "vad_tick_take_segment": (C.c_int, [_vp, C.c_int64, _f32p, C.c_int64, _i64p]),
    "vad_tick_run": (C.c_int, [_vp, C.c_float, C.POINTER(TickResult)]),
    "vad_tick_run_work": (C.c_int, [_vp, C.c_float, C.POINTER(TickResult), C.POINTER(TickWork)]),
    "vad_tick_take_segment_wav16": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, _i64p]),
    "vad_step_rates_device": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_void_p), _i64p, C.POINTER(C.c_int32), _vp, C.c_float,
                                        _vp, _vp, _vp, _vp]),
    "vad_step_rates": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_void_p), _i64p, C.POINTER(C.c_int32), _i64p, C.c_float,
                                 _f32p, _u8p, _i32p]),
    "vad_resample": (C.c_int, [_vp, _f32p, C.c_int64, C.c_int32, C.c_int32, _f32p]),
    "vad_resample_multi_device": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_void_p), _i64p, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_void_p), _vp]),
    "vad_resample_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "vad_debug_pack_weights": (C.c_int, [C.c_int32, _vp, C.c_size_t, _f32p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_uint32)]),
    "vad_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "vad_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vad_g711_decode": (C.c_int, [C.c_int, _vp, C.c_int64, _vp]),
    "vad_tick_pending": (C.c_int, [_vp, C.c_int64, _i64p]),
    "vad_tick_push_gather": (C.c_int, [_vp, _i64p, C.c_int64, C.POINTER(C.c_char_p), C.c_int32, C.c_int, C.c_int, _i32p]),
    "vad_tick_push_status": (C.c_int, [_vp, _i64p, C.c_int64, _vp, C.c_int32, C.c_int, C.c_int, _i32p]),
    "vad_tick_segment_save": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _i64p]),
    "vad_tick_segment_restore": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64]),
    "vad_resample_generic": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, _f32p]),
    "vad_resample_generic_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, _vp]),
    "vad_debug_resample_operator": (C.c_int, [C.c_int32, _f32p, C.c_size_t]),
    "vad_debug_resample_path": (C.c_int, [_vp, C.c_int]),
    "vad_debug_resample_generic_entries": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_size_t]),
    "vad_debug_pack_resample": (C.c_int, [C.c_int32, _f32p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]),
    "vad_debug_pack_resample_t16": (C.c_int, [C.c_int32, _f32p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint32)]),
    "vad_debug_sm_replay": (C.c_int, [_vp, C.c_int64, _f32p, C.c_int64, _u8p, _i32p]),
    "vad_engine_synchronize": (C.c_int, [_vp]),
    "vad_debug_set_tile": (C.c_int, [_vp, C.c_int32]),
    "vad_scan_frame_count": (C.c_int64, [_vp, C.c_int64, C.c_int32]),
    "vad_scan": (C.c_int, [_vp, C.POINTER(ScanItem), C.c_int64, _vp, C.c_int64, C.c_int, C.c_int32, C.c_float, _i64p,
                           _f32p, _u8p, _i32p]),
    "vad_scan_device": (C.c_int, [_vp, C.POINTER(ScanItem), C.c_int64, _vp, C.c_int64, C.c_int, C.c_int32, C.c_float, _i64p,
                                  _vp, _vp, _vp, _vp]),
    "vad_scan_channels": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_float,
                                    _i64p, _f32p, _u8p, _i32p]),
    "vad_scan_channels_device": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32,
                                           C.c_float, _i64p, _vp, _vp, _vp, _vp]),
    "vad_debug_scan_launch_frames": (C.c_int, [_vp, C.c_int32]),
    "vad_scan_rate_frame_count": (C.c_int64, [_vp, C.c_int64, C.c_int32, C.c_int32]),
    "vad_scan_rate": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float,
                                _i64p, _f32p, _u8p, _i32p]),
    "vad_scan_rate_device": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                       C.c_float, _i64p, _vp, _vp, _vp, _vp]),
    "vad_cut_samples": (C.c_int64, [_vp, C.c_int64, C.c_int32, C.c_int32]),
    "vad_scan_cut": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_float, C.c_int32,
                               C.c_int32, _vp, C.c_int64]),
    "vad_scan_cut_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_float,
                                      C.c_int32, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_segments_device": (C.c_int, [_vp, _vp, _vp, _vp, _i64p, C.c_int64, _vp, C.c_int64, _vp, _vp]),
    "vad_scan_segments": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_float,
                                    C.POINTER(Segment), C.c_int64, _i64p]),
    "vad_scan_segments_read": (C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(Segment)]),
    "vad_resegment_device": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int64, C.POINTER(Thresholds), C.c_int64, _vp, C.c_int64, _vp, _vp]),
    "vad_scan_resegment": (C.c_int, [_vp, C.POINTER(Thresholds), C.c_int64, C.POINTER(Segment), C.c_int64, _i64p]),
    "vad_scan_tails": (C.c_int, [_vp, C.POINTER(Segment), C.c_int64]),
    "vad_scan_resegment_tails": (C.c_int, [_vp, C.POINTER(Thresholds), C.c_int64, C.POINTER(Segment), C.c_int64]),
    "vad_tails_device": (C.c_int, [_vp, _i64p, _vp, _vp, _i64p, C.c_int64, _vp, _vp]),
    "vad_resegment_tails_device": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int64, C.POINTER(Thresholds), C.c_int64, _vp, _vp]),
    "vad_refine_device": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _i64p, C.c_int64, C.POINTER(Refine), _vp, C.c_int64, _vp, _vp]),
    "vad_scan_refine": (C.c_int, [_vp, C.POINTER(Segment), C.c_int64, C.POINTER(Segment), C.POINTER(Refine), C.POINTER(Segment), C.c_int64,
                                  _i64p]),
    "vad_scan_rate_segments": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                         C.c_float, C.POINTER(Segment), C.c_int64, _i64p]),
    "vad_rate_cut_samples": (C.c_int64, [_vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "vad_scan_rate_cut": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float,
                                    C.c_int32, C.c_int32, _vp, C.c_int64]),
    "vad_scan_rate_cut_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                           C.c_float, C.c_int32, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_scan_levels": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float,
                                  C.c_float, C.POINTER(Level)]),
    "vad_scan_levels_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                         C.c_float, C.c_float, _vp, _vp]),
    "vad_scan_cut_gain": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                    C.c_float, C.c_int32, C.c_int32, _vp, C.c_int64]),
    "vad_scan_cut_gain_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32,
                                           C.c_int32, C.c_float, C.c_int32, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_mel_frames": (C.c_int64, [C.POINTER(Mel), C.c_int64]),
    "vad_scan_mel": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, C.POINTER(Mel), _f32p, _f32p, _f32p, _vp, C.c_int64, C.c_int32, C.c_int,
                               C.c_int32, C.c_float, _f32p, C.c_int64]),
    "vad_scan_mel_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, C.POINTER(Mel), _f32p, _f32p, _f32p, _vp, C.c_int64, C.c_int32,
                                      C.c_int, C.c_int32, C.c_float, _vp, C.c_int64, _vp]),
    "vad_resample_cut_samples": (C.c_int64, [_vp, C.c_int64, C.c_int32, C.c_int32]),
    "vad_scan_resample_cut": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _f32p, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int,
                                        C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int64]),
    "vad_scan_resample_cut_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _f32p, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int,
                                               C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_scan_rate_mel": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, C.POINTER(Mel), _f32p, _f32p, _f32p, _f32p, C.c_int32, _vp, C.c_int64,
                                    C.c_int32, C.c_int, C.c_int32, C.c_int32, _f32p, C.c_int64]),
    "vad_scan_rate_mel_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, C.POINTER(Mel), _f32p, _f32p, _f32p, _f32p, C.c_int32, _vp,
                                           C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_scan_mel_keep": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, C.POINTER(Mel), _f32p, _f32p, _f32p, _f32p, C.c_int32, _vp, C.c_int64,
                                    C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float, _i64p]),
    "vad_scan_mel_keep_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, C.POINTER(Mel), _f32p, _f32p, _f32p, _f32p, C.c_int32, _vp,
                                           C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float, _i64p, _vp]),
    "vad_mel_resident": (C.c_int, [_vp, _i64p, _i32p, _i64p]),
    "vad_mel_resident_read": (C.c_int, [_vp, C.c_int64, C.c_int64, _f32p]),
    "vad_mel_stats": (C.c_int, [_vp, _f32p, C.c_int64, C.c_int32, _i64p, C.c_int64, _f32p, _i64p, C.POINTER(C.c_uint64)]),
    "vad_mel_stats_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _i64p, C.c_int64, _vp, _vp, _vp, _vp]),
    "vad_mel_batch": (C.c_int, [_vp, _f32p, C.c_int64, _i64p, C.c_int64, C.POINTER(Batch), C.POINTER(BatchWindow), C.c_int64, _f32p, _f32p,
                                _f32p, C.c_int64, _vp, C.c_int64]),
    "vad_mel_batch_device": (C.c_int, [_vp, _vp, C.c_int64, _i64p, C.c_int64, C.POINTER(Batch), C.POINTER(BatchWindow), C.c_int64, _f32p,
                                       _f32p, _f32p, C.c_int64, _vp, C.c_int64, _vp]),
    "vad_mel_pack_plan": (C.c_int, [_i64p, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(BatchPiece), C.c_int64, _i64p, _i64p]),
    "vad_mel_batch_packed": (C.c_int, [_vp, _f32p, C.c_int64, _i64p, C.c_int64, C.POINTER(Batch), C.POINTER(BatchPiece), C.c_int64, C.c_int64,
                                       _f32p, _f32p, _f32p, C.c_int64, _vp, C.c_int64]),
    "vad_mel_batch_packed_device": (C.c_int, [_vp, _vp, C.c_int64, _i64p, C.c_int64, C.POINTER(Batch), C.POINTER(BatchPiece), C.c_int64, C.c_int64,
                                              _f32p, _f32p, _f32p, C.c_int64, _vp, C.c_int64, _vp]),
    "vad_mel_stats_grouped": (C.c_int, [_vp, _f32p, C.c_int64, C.c_int32, _i64p, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _f32p, _i64p,
                                        C.POINTER(C.c_uint64)]),
    "vad_mel_stats_grouped_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _i64p, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _vp, _vp, _vp,
                                               _vp]),
    "vad_mel_project": (C.c_int, [_vp, _f32p, C.c_int64, C.c_int32, _f32p, _f32p, C.c_int32, _f32p]),
    "vad_mel_project_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _f32p, _f32p, C.c_int32, _vp, _vp]),
    "vad_scan_moments": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float,
                                   C.POINTER(Moments)]),
    "vad_scan_moments_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                          C.c_float, _vp, _vp]),
    "vad_scan_audio_batch": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_float,
                                       C.POINTER(AudioBatchRecord), C.POINTER(AudioWindow), C.c_int64, _f32p, _f32p, C.c_int64, _vp, C.c_int64,
                                       _vp]),
    "vad_scan_audio_batch_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                              C.c_float, C.POINTER(AudioBatchRecord), C.POINTER(AudioWindow), C.c_int64, _f32p, _f32p, C.c_int64,
                                              _vp, C.c_int64, _vp, _vp]),
    "vad_scan_render": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _f32p, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32,
                                  C.c_int32, C.c_float, C.c_int32, _vp, C.c_int64]),
    "vad_scan_render_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _f32p, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int,
                                         C.c_int32, C.c_int32, C.c_float, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_scan_cut_stereo": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_int32,
                                      C.c_float, C.c_int32, C.c_int32, _vp, C.c_int64]),
    "vad_scan_cut_stereo_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32,
                                             C.c_int32, C.c_float, C.c_int32, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_scan_render_stereo": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _f32p, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int,
                                         C.c_int32, C.c_int32, C.c_float, C.c_int32, _vp, C.c_int64]),
    "vad_scan_render_stereo_device": (C.c_int, [_vp, C.POINTER(CutItem), C.c_int64, _f32p, _f32p, C.c_int32, _vp, C.c_int64, C.c_int32,
                                                C.c_int, C.c_int32, C.c_int32, C.c_float, C.c_int32, _vp, C.c_int64, _vp]),
    "vad_convert_samples": (C.c_int64, [_vp, C.c_int64, C.c_int32]),
    "vad_convert": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, _f32p, C.c_int32, _f32p,
                              C.c_int64, _i64p]),
    "vad_convert_device": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, _f32p, C.c_int32,
                                     _vp, C.c_int64, _i64p, _vp]),
    "vad_scan_convert_segments": (C.c_int, [_vp, C.POINTER(ScanChItem), C.c_int64, _vp, C.c_int64, C.c_int32, C.c_int, C.c_int32, _f32p,
                                            C.c_int32, C.c_int32, C.c_float, C.POINTER(Segment), C.c_int64, _i64p, _i64p]),
}

_lib = None


def lib() -> C.CDLL:
    """Load the in-tree HIP engine library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m cutter_vad_amd._build` "
                "(hipcc, gfx950). The engine has no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib
