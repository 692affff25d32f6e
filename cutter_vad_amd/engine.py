"""Python face of the C ABI (``include/vad_engine.h``): one :class:`Engine` = one GPU's stream pool.

This is the multi-stream operator the reference lacks.  The reference owns one
``SileroVADModel`` (one ORT session + one ``(h, c)``) per client
(/root/reference/websocket_service/server/vad_websocket_server.py:277,
/root/reference/src/real_time_vad/core/silero_model.py:238-566); here many streams share one
engine and advance together in one kernel launch.  Errors are mapped onto the reference's
exception classes with the same message prefixes (SURVEY §8 b).
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .core.exceptions import AudioProcessingError, ConfigurationError, ModelInitializationError, VADError

_FMT = {np.dtype(np.float32): _ffi.VAD_FMT_F32, np.dtype(np.int16): _ffi.VAD_FMT_I16_32767}
TICK_GROUPS = 12                      # include/vad_engine.h VAD_TICK_GROUPS
TICK_RATES = (8000, 24000, 48000)     # tick groups 6.. : 6 + 3 * gate_on + index into this
TICK_RATE_CHUNK = (256, 768, 1536)    # samples of such a chunk = one 16 kHz frame's worth


def _law_format(law: Optional[str], frames=None) -> Optional[int]:
    """``law`` = None: no G.711 (-> None).  "ulaw" / "alaw": the frame format for ITU-T G.711 codes, one byte per sample;
    ``frames`` (an array) must then be uint8.  Without ``law`` a uint8 array keeps its old meaning (numbers, converted to float32)."""
    if law is None:
        return None
    if law not in _ffi.G711_LAWS:
        raise AudioProcessingError(f"Model prediction failed: unknown G.711 law {law!r} (expected 'ulaw' or 'alaw')")
    if frames is not None and not isinstance(frames, (bytes, bytearray, memoryview)) and np.asarray(frames).dtype != np.uint8:
        raise AudioProcessingError(f"Model prediction failed: G.711 frames must be uint8 codes, got {np.asarray(frames).dtype}")
    return _ffi.G711_LAWS[law]


def _ptr(a: np.ndarray, ty):
    return a.ctypes.data_as(C.POINTER(ty))


class Engine:
    """Stream pool + fused Silero kernels on one MI355X.

    ``weights`` is an SVW blob (``weights_io.load_weight_blob``).  ``denoise`` is the gate
    threshold of ``AudioUtils.denoise_audio`` (0.01) or ``None`` to disable it.

    Rejected frames (ABI 5, ``include/vad_engine.h``): a float32 frame with a NaN / Inf sample the model would read gives
    that stream probability NaN, event ``_ffi.VAD_EV_REJECTED`` alone and seg 0, and leaves its (h, c) and state machine
    exactly as they were; the other streams of the call are unaffected and the call does not raise.  This holds for every
    ``step*``, ``submit`` / ``collect``, ``step_rates*`` and the tick entries (``tick_run_work`` lists such an entry as
    ``_ffi.VAD_WORK_REJECTED`` and leaves the slot's ``last_prob`` / ``frames_done`` / ``active``).
    """

    def __init__(self, weights: bytes, model_version: int = 5, device_id: int = 0, max_streams: int = 8192,
                 sample_rate: int = 16000, shared_gpu: bool = False):
        self._lib = _ffi.lib()
        self._gather_fn = int(C.cast(self._lib.vad_tick_push_gather, C.c_void_p).value)
        self._rate_gather_fn = int(C.cast(self._lib.vad_tick_push_rate_gather, C.c_void_p).value)
        self._h = C.c_void_p()
        self._pid = os.getpid()             # the process that owns the handle: see close()
        self._tickets = {}                  # ticket -> the buffers a pipelined call still reads (submit / collect)
        self._scan_block = None             # scan(): the page-locked block the recordings are packed into ...
        self._scan_lock = threading.RLock()  # ... held from the packing to the return of vad_scan: engines are shared between threads
        self._scan_last = None              # what scan() packed last (cut(audio=None) cuts that block): see scan_session()
        self._tail_items = None             # items of the last scan_segments (scan_tails asks for as many records)
        self.last_tick_us = (0.0, 0.0, 0.0)
        self.last_tick_dropped = 0
        self.last_tick_staged_next = 0
        self.last_tick_lost = None
        self._weights = weights  # keep alive during create
        desc = _ffi.EngineDesc(C.sizeof(_ffi.EngineDesc), model_version, C.cast(C.c_char_p(weights), C.c_void_p),
                               len(weights), device_id, max_streams, sample_rate, 1 if shared_gpu else 0)  # VAD_ENGINE_SHARED_GPU
        rc = self._lib.vad_engine_create(C.byref(desc), C.byref(self._h))
        if rc != _ffi.VAD_OK:
            self._h = C.c_void_p()
            msg = self._lib.vad_last_create_error().decode() or f"vad_engine_create failed ({rc})"
            raise ModelInitializationError(f"v{model_version}", msg)
        self.model_version = model_version
        self.max_streams = max_streams
        self.device_id = device_id
        self.sample_rate = sample_rate
        self.frame_samples = 256 if (model_version == 5 and sample_rate != 16000) else 512   # vad_info.frame_samples

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        h, self._h = self._h, C.c_void_p()
        self._scan_block = None             # the engine releases its page-locked blocks
        # An engine inherited through fork is the parent's: its streams, events and device memory mean nothing in the child, and
        # destroying them there crashed whenever the child's garbage collector found such an engine.  The child only drops the handle.
        if h and getattr(self, "_pid", None) == os.getpid():
            self._lib.vad_engine_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, exc=AudioProcessingError) -> None:
        if rc != _ffi.VAD_OK:
            msg = self._lib.vad_last_error(self._h).decode() or f"engine call failed ({rc})"
            raise exc(msg)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> dict:
        inf = _ffi.EngineInfo()
        inf.struct_size = C.sizeof(_ffi.EngineInfo)
        self._check(self._lib.vad_engine_info(self._h, C.byref(inf)), VADError)
        out = {k: getattr(inf, k) for k, _ in _ffi.EngineInfo._fields_ if k != "struct_size"}
        out["device_name"] = inf.device_name.decode()
        out["arch"] = inf.arch.decode()
        return out

    def set_tile(self, streams_per_tile: int = 0) -> None:
        """Diagnostic (``vad_debug_set_tile``): 0 = pick the kernel shape by batch size, 16 / 32 = force it (each also sets the
        pairing of 16-stream tiles back to its default: one-frame V5 calls with more tiles than CUs); -3 = pair at every size,
        -4 = never pair; -1 / -2 = ``vad_step_rates`` as two launches / fused."""
        self._check(self._lib.vad_debug_set_tile(self._h, int(streams_per_tile)), VADError)

    def synchronize(self) -> None:
        self._check(self._lib.vad_engine_synchronize(self._h))

    def pinned_array(self, shape, dtype=np.float32) -> np.ndarray:
        """A numpy array over page-locked host memory (``vad_host_alloc``): frame and result buffers handed to the
        host-pointer entry points from it are DMA'd without a staging copy.  The memory belongs to the engine and is
        released by ``close()``: do not use the array after that."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        p = C.c_void_p()
        self._check(self._lib.vad_host_alloc(self._h, max(1, n * dt.itemsize), C.byref(p)))
        buf = (C.c_char * (n * dt.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    # ------------------------------------------------------------------ streams
    def open_stream(self) -> int:
        s = C.c_int64()
        self._check(self._lib.vad_stream_open(self._h, C.byref(s)), VADError)
        return int(s.value)

    def open_streams(self, n: int) -> np.ndarray:
        out = np.empty(int(n), np.int64)
        self._check(self._lib.vad_stream_open_many(self._h, int(n), _ptr(out, C.c_int64)), VADError)
        return out

    def close_stream(self, slot: int) -> None:
        self._check(self._lib.vad_stream_close(self._h, int(slot)), VADError)

    def reset(self, slots: Sequence[int]) -> None:
        s = np.ascontiguousarray(slots, dtype=np.int64)
        self._check(self._lib.vad_stream_reset(self._h, _ptr(s, C.c_int64), s.size), VADError)

    def get_state(self, slot: int) -> np.ndarray:
        out = np.empty(_ffi.VAD_STATE_FLOATS, np.float32)
        self._check(self._lib.vad_stream_get_state(self._h, int(slot), _ptr(out, C.c_float)), VADError)
        return out

    def set_state(self, slot: int, hc: np.ndarray) -> None:
        hc = np.ascontiguousarray(hc, np.float32).reshape(_ffi.VAD_STATE_FLOATS)
        self._check(self._lib.vad_stream_set_state(self._h, int(slot), _ptr(hc, C.c_float)), VADError)

    def save_stream(self, slot: int) -> bytes:
        """(h, c) + state machine of one stream as an opaque blob (``vad_stream_save``)."""
        buf = C.create_string_buffer(_ffi.VAD_STREAM_SAVE_BYTES)
        self._check(self._lib.vad_stream_save(self._h, int(slot), buf, _ffi.VAD_STREAM_SAVE_BYTES), VADError)
        return buf.raw

    def restore_stream(self, slot: int, blob: bytes) -> None:
        self._check(self._lib.vad_stream_restore(self._h, int(slot), blob, len(blob)), VADError)

    def set_thresholds(self, slot: int, start_probability=0.7, end_probability=0.7, start_ratio=0.8, end_ratio=0.95,
                       start_frame_count=10, end_frame_count=50) -> None:
        t = _ffi.Thresholds(start_probability, end_probability, start_ratio, end_ratio, start_frame_count,
                            end_frame_count)
        self._check(self._lib.vad_stream_set_thresholds(self._h, int(slot), C.byref(t)), VADError)

    def set_thresholds_many(self, slots, thresholds) -> None:
        """``thresholds``: one 6-tuple (shared by all slots) or one per slot, in the order of ``set_thresholds``' arguments
        (``vad_stream_set_thresholds_many``: one launch for the lot)."""
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        rows = [thresholds] if np.isscalar(thresholds[0]) else list(thresholds)
        arr = (_ffi.Thresholds * len(rows))(*[_ffi.Thresholds(*r) for r in rows])
        self._check(self._lib.vad_stream_set_thresholds_many(self._h, _ptr(s, C.c_int64), s.size, arr, len(rows)), VADError)

    def debug_sm_replay(self, slot: int, probs) -> Tuple[np.ndarray, np.ndarray]:
        """Diagnostic: run scripted probabilities through one slot's device state machine."""
        p = np.ascontiguousarray(probs, np.float32)
        ev = np.zeros(p.size, np.uint8)
        seg = np.zeros(p.size, np.int32)
        self._check(self._lib.vad_debug_sm_replay(self._h, int(slot), _ptr(p, C.c_float), p.size, _ptr(ev, C.c_uint8),
                                                  _ptr(seg, C.c_int32)), VADError)
        return ev, seg

    # ------------------------------------------------------------------ hot path
    def _prep(self, slots, frames, T: Optional[int], law: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, int]:
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        f = np.asarray(frames)
        g711 = _law_format(law, f)
        if g711 is None and f.dtype not in _FMT:
            f = f.astype(np.float32)
        f = np.ascontiguousarray(f)
        want = (s.size, self.frame_samples) if T is None else (s.size, T, self.frame_samples)
        if f.shape != want:
            raise AudioProcessingError(f"Model prediction failed: frames have shape {f.shape}, expected {want}")
        return s, f, (_FMT[f.dtype] if g711 is None else g711)

    def step(self, slots, frames, denoise: Optional[float] = 0.01, i16_scale: int = 32767, law: Optional[str] = None) -> np.ndarray:
        """One 512-sample frame per listed stream -> probabilities [n] (NaN for a rejected non-finite frame).
        ``law`` = "ulaw" / "alaw": ``frames`` are uint8 ITU-T G.711 codes, decoded on the GPU (``VAD_FMT_ULAW8 / ALAW8``); the
        results equal those of the decoded int16 samples with ``i16_scale=32768``.  The same on every entry point that takes it."""
        s, f, fmt = self._prep(slots, frames, None, law)
        if fmt == _ffi.VAD_FMT_I16_32767 and i16_scale == 32768:
            fmt = _ffi.VAD_FMT_I16_32768
        probs = np.empty(s.size, np.float32)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step(self._h, _ptr(s, C.c_int64), s.size, f.ctypes.data_as(C.c_void_p), fmt, thr,
                                       _ptr(probs, C.c_float)))
        return probs

    def step_events(self, slots, frames, denoise: Optional[float] = 0.01, i16_scale: int = 32767, law: Optional[str] = None):
        """-> (probs [n], event bits [n] uint8, finished-segment frames [n] int32); a rejected non-finite frame: NaN,
        ``VAD_EV_REJECTED``, 0."""
        s, f, fmt = self._prep(slots, frames, None, law)
        if fmt == _ffi.VAD_FMT_I16_32767 and i16_scale == 32768:
            fmt = _ffi.VAD_FMT_I16_32768
        probs = np.empty(s.size, np.float32)
        ev = np.zeros(s.size, np.uint8)
        seg = np.zeros(s.size, np.int32)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step_events(self._h, _ptr(s, C.c_int64), s.size, f.ctypes.data_as(C.c_void_p), fmt,
                                              thr, _ptr(probs, C.c_float), _ptr(ev, C.c_uint8), _ptr(seg, C.c_int32)))
        return probs, ev, seg

    def step_multi(self, slots, frames, denoise: Optional[float] = 0.01, i16_scale: int = 32767, law: Optional[str] = None):
        """frames [n, T, 512]: T consecutive frames per stream -> (probs [n,T], events [n,T]).  A rejected non-finite frame
        (NaN, ``VAD_EV_REJECTED``) is skipped: the stream's next frame continues from the state before it."""
        f0 = np.asarray(frames)
        if f0.ndim != 3:
            raise AudioProcessingError(f"Model prediction failed: frames must be [n, T, 512], got {f0.shape}")
        T = int(f0.shape[1])
        s, f, fmt = self._prep(slots, f0, T, law)
        if fmt == _ffi.VAD_FMT_I16_32767 and i16_scale == 32768:
            fmt = _ffi.VAD_FMT_I16_32768
        probs = np.empty((s.size, T), np.float32)
        ev = np.zeros((s.size, T), np.uint8)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step_multi(self._h, _ptr(s, C.c_int64), s.size, T, f.ctypes.data_as(C.c_void_p), fmt,
                                             thr, _ptr(probs, C.c_float), _ptr(ev, C.c_uint8)))
        return probs, ev

    def step_device(self, n: int, d_frames: int, d_probs: int, d_slots: int = 0, d_events: int = 0, d_seg: int = 0,
                    fmt: int = _ffi.VAD_FMT_F32, denoise: Optional[float] = 0.01, stream: int = 0) -> None:
        """Asynchronous launch on device pointers (integers, e.g. ``tensor.data_ptr()``)."""
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step_device(self._h, d_slots or None, n, d_frames, fmt, thr, d_probs,
                                              d_events or None, d_seg or None, stream or None))

    def step_multi_device(self, n: int, T: int, d_frames: int, d_probs: int, d_slots: int = 0, d_events: int = 0,
                          d_seg: int = 0, fmt: int = _ffi.VAD_FMT_F32, denoise: Optional[float] = 0.01, stream: int = 0) -> None:
        """``step_device`` with T frames per stream: d_frames [n, T, frame], d_probs [n, T] (``vad_step_multi_device``)."""
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step_multi_device(self._h, d_slots or None, n, T, d_frames, fmt, thr, d_probs,
                                                    d_events or None, d_seg or None, stream or None))

    # ------------------------------------------------------------------ whole recordings
    def _scan_rate(self, sample_rate: Optional[int]) -> Optional[int]:
        """``sample_rate`` of ``scan`` / ``scan_frame_count``: None for the engine's own rate (today's path), else the input rate"""
        return None if sample_rate is None or int(sample_rate) == int(self.sample_rate) else int(sample_rate)

    def scan_chunk_samples(self, sample_rate: Optional[int] = None) -> int:
        """Samples of one frame as ``scan`` frames a recording at ``sample_rate``: ``frame_samples`` at the engine's own rate,
        ``512 * sample_rate / 16000`` (256 / 768 / 1536) at 8 / 24 / 48 kHz."""
        sr = self._scan_rate(sample_rate)
        if sr is None or sr == 16000:
            return self.frame_samples
        if sr not in (8000, 24000, 48000):
            raise AudioProcessingError(f"Failed to resample audio from {sr}Hz to 16000Hz: supported input rates are 8000, 16000, 24000, 48000")
        return 512 * sr // 16000

    def scan_frame_count(self, nsamples: int, hop: Optional[int] = None, sample_rate: Optional[int] = None) -> int:
        """Frames of a recording of ``nsamples`` samples at ``hop`` (``vad_scan_frame_count``; the tail is dropped).
        ``sample_rate``: the recording's rate (``vad_scan_rate_frame_count``: chunks of ``scan_chunk_samples(sample_rate)``, ``hop`` in
        input samples); None or the engine's own rate: the engine's frames."""
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        if sr is None:
            n = int(self._lib.vad_scan_frame_count(self._h, int(nsamples), hop))
        else:
            n = int(self._lib.vad_scan_rate_frame_count(self._h, int(nsamples), sr, hop))
        if n < 0:
            raise AudioProcessingError(f"Model prediction failed: bad sample count, hop or rate ({nsamples}, {hop}, {sample_rate})")
        return n

    def set_scan_launch_frames(self, frames: int = 0) -> None:
        """Diagnostic (``vad_debug_scan_launch_frames``): frames per launch of ``scan``; 0 = the default.  Results do not depend on it."""
        self._check(self._lib.vad_debug_scan_launch_frames(self._h, int(frames)), VADError)

    def _scan_pack(self, recordings, law: Optional[str]):
        """The recordings (1-D arrays of one dtype, or C-contiguous [nsamples, 2] arrays of one dtype: interleaved channels,
        copied as they are) packed into the engine's page-locked block, each starting on a multiple of 4 sample frames
        -> (block, sample frames, frame format, offsets, lengths, channels)."""
        recs = [np.asarray(r) for r in recordings]
        ch = 2 if recs and all(r.ndim == 2 for r in recs) else 1
        if ch == 1 and any(r.ndim == 2 for r in recs):
            raise AudioProcessingError("Model prediction failed: one call takes recordings that are all 1-D or all [nsamples, 2]; "
                                       "scan the two kinds in two calls (scan_recordings does)")
        g711 = _law_format(law, recs[0] if recs else None)
        if g711 is None:
            recs = [r if r.dtype in _FMT else r.astype(np.float32) for r in recs]
        dt = recs[0].dtype if recs else np.dtype(np.float32)
        for r in recs:
            if ch == 1 and (r.ndim != 1 or r.dtype != dt):
                raise AudioProcessingError(f"Model prediction failed: recordings must be 1-D arrays of one dtype, got {r.shape} {r.dtype} next to {dt}")
            if ch == 2 and (r.shape[1] != 2 or r.dtype != dt or not r.flags.c_contiguous):
                raise AudioProcessingError(f"Model prediction failed: two-channel recordings must be C-contiguous [nsamples, 2] arrays of one "
                                           f"dtype, got {r.shape} {r.dtype} next to {dt}")
        lens = np.array([r.shape[0] for r in recs], np.int64)
        offs = np.zeros(len(recs), np.int64)
        if len(recs) > 1:
            offs[1:] = np.cumsum((lens[:-1] + 3) & ~3)
        total = int(offs[-1] + lens[-1]) if recs else 0
        need = max(total, 1) * ch * dt.itemsize
        if self._scan_block is None or self._scan_block.size < need:      # grown on demand, kept: pinning is the slow part
            if self._scan_block is not None:
                self._check(self._lib.vad_host_free(self._h, self._scan_block.ctypes.data_as(C.c_void_p)), VADError)
                self._scan_block = None
            self._scan_block = self.pinned_array(need + need // 4, np.uint8)
        block = self._scan_block[:need].view(dt)
        if ch == 2:
            block = block.reshape(-1, 2)
        for i, (r, o) in enumerate(zip(recs, offs)):
            block[o:o + lens[i]] = r
            block[o + lens[i]:(offs[i + 1] if i + 1 < len(recs) else o + lens[i])] = 0      # the padding to a multiple of 4
        return block, total, (_FMT[dt] if g711 is None else g711), offs, lens, ch

    @staticmethod
    def _scan_channel(c) -> int:
        if isinstance(c, str):
            if c == "mix":
                return _ffi.VAD_SCAN_MIX
        elif int(c) in (0, 1):
            return int(c)
        raise AudioProcessingError(f"Model prediction failed: channel must be 'mix', 0, 1, a sequence of these, or 'split', got {c!r}")

    def scan(self, slots, recordings, hop: Optional[int] = None, law: Optional[str] = None, i16_scale: int = 32767,
             denoise: Optional[float] = 0.01, channel="mix", sample_rate: Optional[int] = None):
        """Whole recordings of different lengths, framed on the GPU (``vad_scan``): ``recordings`` is a list of 1-D arrays
        (float32, int16, or uint8 G.711 codes with ``law``), recording i continues stream ``slots[i]``.  Frame t of a recording
        = its samples ``t * hop .. t * hop + frame_samples - 1``; ``hop`` defaults to ``frame_samples // 2``
        (``AudioUtils.split_into_frames`` as ``VADWrapper`` calls it), ``hop = frame_samples`` is Silero's back-to-back framing.
        -> (probs, events, seg_frames): three lists with one array per recording (views of the call's CSR arrays), one entry per
        frame; ``seg_frames`` holds the finished segment's length on every ``VAD_EV_END`` frame and 0 elsewhere
        (``cutter_vad_amd.scan.speech_segments`` turns the two into sample ranges).
        Two-channel recordings (``vad_scan_channels``): every recording a C-contiguous ``[nsamples, 2]`` array, interleaved as WAV
        readers deliver it and scanned as it is.  ``channel`` says what a stream hears: ``"mix"`` (the default: the float32 mean
        of the decoded pair, what ``VADWrapper`` makes of such an array), ``0``, ``1``, a sequence of these per recording, or
        ``"split"``: both channels of every recording, each on its own stream - ``slots`` is ``[n, 2]``, a recording is packed
        once and every returned array gets a leading axis of 2.  1-D recordings ignore ``channel``.
        ``sample_rate``: the recordings' rate when it is not the engine's - 8000, 24000 or 48000 on a 16 kHz Silero V5 engine
        (``vad_scan_rate``): the recordings are packed and uploaded at that rate, framed in chunks of ``scan_chunk_samples(sample_rate)``
        at ``hop`` INPUT samples (default half a chunk), and each chunk is resampled on the GPU to the frame the model steps -
        ``Engine.resample`` of the decoded chunk, byte for byte.  One result per chunk; no block stays for ``cut(audio=None)``
        (``scan_segments(sample_rate=...)`` is the scan that keeps it).  None, or the engine's own rate: the path above."""
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        thr = -1.0 if denoise is None else float(denoise)
        with self._scan_lock:
            n, per, two, split, block, total, fmt, offs, lens, items, start = self._scan_plan(slots, recordings, hop, law, i16_scale, channel, sr)
            nf = int(start[-1])
            probs = np.empty(nf, np.float32)
            ev = np.zeros(nf, np.uint8)
            seg = np.zeros(nf, np.int32)
            out = (_ptr(start, C.c_int64), _ptr(probs, C.c_float), _ptr(ev, C.c_uint8), _ptr(seg, C.c_int32))
            self._scan_last = None
            if sr is not None:
                self._check(self._lib.vad_scan_rate(self._h, items, n * per, block.ctypes.data_as(C.c_void_p), total, 2 if two else 1, fmt, sr,
                                                    hop, thr, *out))
            elif two:
                self._check(self._lib.vad_scan_channels(self._h, items, n * per, block.ctypes.data_as(C.c_void_p), total, 2, fmt, hop, thr, *out))
            else:
                self._check(self._lib.vad_scan(self._h, items, n, block.ctypes.data_as(C.c_void_p), total, fmt, hop, thr, *out))
            if nf and sr is None:           # (a scan without a frame uploads nothing, a rate scan leaves nothing to cut)
                self._scan_last = {"samples": total, "channels": 2 if two else 1, "fmt": fmt, "offsets": offs, "lengths": lens}
        if split:
            cut = lambda a: [a[start[2 * i]:start[2 * i + 2]].reshape(2, -1) for i in range(n)]
        else:
            cut = lambda a: [a[start[i]:start[i + 1]] for i in range(n)]
        return cut(probs), cut(ev), cut(seg)

    def _scan_plan(self, slots, recordings, hop: int, law: Optional[str], i16_scale: int, channel, rate: Optional[int] = None):
        """What ``scan`` and ``scan_segments`` share, under ``_scan_lock``: the slots and channels checked, the recordings packed
        (``_scan_pack``), one item per (recording, channel listed for it) and the items' CSR positions; ``rate`` (``scan`` at another
        sample rate): frames are counted in chunks at that rate, and the items are channel items whatever the recordings' shape
        -> (n, per, two, split, block, sample frames, frame format, offsets, lengths, items, start [n * per + 1])."""
        recordings = [np.asarray(r) for r in recordings]
        n = len(recordings)
        two = any(r.ndim == 2 for r in recordings)
        split = two and isinstance(channel, str) and channel == "split"
        s = np.ascontiguousarray(slots, dtype=np.int64)
        if split:
            if s.shape != (n, 2):
                raise AudioProcessingError(f"Model prediction failed: channel='split' takes slots of shape ({n}, 2), got {s.shape}")
            chans = [(0, 1)] * n
        else:
            s = s.reshape(-1)
            if s.size != n:
                raise AudioProcessingError(f"Model prediction failed: {s.size} slots for {n} recordings")
            if not two:
                chans = [(0,)] * n
            elif isinstance(channel, (str, int, np.integer)):
                chans = [(self._scan_channel(channel),)] * n
            else:
                chans = [(self._scan_channel(c),) for c in channel]
                if len(chans) != n:
                    raise AudioProcessingError(f"Model prediction failed: {len(chans)} channels for {n} recordings")
        per = 2 if split else 1
        s = s.reshape(n, per)
        block, total, fmt, offs, lens, _ = self._scan_pack(recordings, law)
        if fmt == _ffi.VAD_FMT_I16_32767 and i16_scale == 32768:
            fmt = _ffi.VAD_FMT_I16_32768
        # one item per (recording, channel listed for it); a 1-D corpus goes through vad_scan as it always did
        ch_items = two or rate is not None
        items = ((_ffi.ScanChItem if ch_items else _ffi.ScanItem) * max(1, n * per))()
        start = np.zeros(n * per + 1, np.int64)
        for i in range(n):
            nf = self.scan_frame_count(int(lens[i]), hop, rate) if hop >= 1 else 0
            for k, c in enumerate(chans[i]):
                j = i * per + k
                where = (int(s[i, k]), int(offs[i]), int(lens[i]))
                items[j] = _ffi.ScanChItem(*where, c, 0) if ch_items else _ffi.ScanItem(*where)
                start[j + 1] = start[j] + nf
        return n, per, two, split, block, total, fmt, offs, lens, items, start

    def scan_segments(self, slots, recordings, hop: Optional[int] = None, law: Optional[str] = None, i16_scale: int = 32767,
                      denoise: Optional[float] = 0.01, channel="mix", sample_rate: Optional[int] = None, convert=None) -> np.ndarray:
        """``scan`` that answers with the finished segments alone (``vad_scan_segments``): the same arguments, packing, streams
        and resident block (``cut(audio=None)`` works behind it), but the per-frame results stay on the GPU, where kernels turn
        them into one record per ``VAD_EV_END`` -> a structured array (``_ffi.SEGMENT_DTYPE``) in item order, then frame order:
        ``item`` (recording i, or ``2 * i + channel`` for ``"split"``), ``first_frame`` and ``nframes`` (``segment_ranges`` gives
        the sample ranges ``speech_segments`` would), ``counted``, ``mean_prob`` and ``max_prob`` - the number, the mean and the
        maximum of the segment's accepted probabilities from the recording's frame 0 on.
        ``sample_rate`` as in ``scan`` (``vad_scan_rate_segments``): frames are chunks at that rate, ``hop`` counts input samples,
        and the block stays on the GPU as a block of that rate - ``cut(audio=None)`` behind it cuts at that rate.
        ``convert`` (``vad_scan_convert_segments``): ``True`` or a taps array (``convert``'s ``taps``) - the recordings are at ANY rate
        ``convert_samples`` accepts (44100, 22050, 32000, 96000 ..): each is converted once on the GPU to the engine's rate, and the
        scan, the table and everything behind it (``cut(audio=None)``, ``levels``, ``render``, ``mel``, ``resegment``, ``scan_tails``,
        ``refine``) see an ordinary mono float32 block at the engine's rate: ``hop``, frames and ranges count samples of the CONVERTED
        signal, ``last_scan["offsets"]`` are its items' first samples, and no ``sample_rate=`` is passed downstream."""
        if convert is not None and convert is not False:
            return self._scan_convert_segments(slots, recordings, hop, law, i16_scale, denoise, channel, sample_rate, convert)
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        thr = -1.0 if denoise is None else float(denoise)
        with self._scan_lock:
            n, per, two, split, block, total, fmt, offs, lens, items, start = self._scan_plan(slots, recordings, hop, law, i16_scale, channel, sr)
            if not two and sr is None:      # the entry point takes channel items; of a one-channel block every item hears channel 0
                mono = items
                items = (_ffi.ScanChItem * max(1, n))()
                for i in range(n):
                    items[i] = _ffi.ScanChItem(mono[i].slot, mono[i].sample_offset, mono[i].nsamples, 0, 0)
            # a guess first - a segment per 64 frames - then vad_scan_segments_read for what did not fit: the table stays on the GPU
            table = np.zeros(int(start[-1]) // 64 + 16, _ffi.SEGMENT_DTYPE)
            count = C.c_int64(0)
            self._scan_last = None
            self._tail_items = None
            where = (self._h, items, n * per, block.ctypes.data_as(C.c_void_p), total, 2 if two else 1, fmt)
            res = (thr, table.ctypes.data_as(C.POINTER(_ffi.Segment)), table.size, C.byref(count))
            if sr is not None:
                self._check(self._lib.vad_scan_rate_segments(*where, sr, hop, *res))
            else:
                self._check(self._lib.vad_scan_segments(*where, hop, *res))
            self._tail_items = n * per           # what scan_tails asks for
            if int(start[-1]):
                self._scan_last = {"samples": total, "channels": 2 if two else 1, "fmt": fmt, "offsets": offs, "lengths": lens}
                if sr is not None:
                    self._scan_last["rate"] = sr
            if count.value > table.size:
                rest = np.zeros(count.value - table.size, _ffi.SEGMENT_DTYPE)
                self._check(self._lib.vad_scan_segments_read(self._h, table.size, rest.size, rest.ctypes.data_as(C.POINTER(_ffi.Segment))))
                table = np.concatenate([table, rest])
        return table[:count.value]

    # ------------------------------------------------------------------ recordings at any rational rate
    def _convert_taps(self, rate: int, taps) -> np.ndarray:
        if taps is None or taps is True:
            from .scan import convert_taps, convert_ratio
            L, M = convert_ratio(rate, int(self.sample_rate))
            # the widest default the reach allows: 16 zero crossings where VAD_CONVERT_MAX_REACH * L taps hold them
            return convert_taps(rate, int(self.sample_rate), half_width=max(0, min(16, (_ffi.VAD_CONVERT_MAX_REACH * L - 1) // (2 * max(L, M)))))
        return np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))

    def convert_samples(self, nsamples: int, sample_rate: int) -> int:
        """Samples at the engine's rate of a recording of ``nsamples`` samples at ``sample_rate`` (``vad_convert_samples``):
        ``floor(nsamples * L / M)``; -1: a bad count or a rate the conversion does not accept."""
        return int(self._lib.vad_convert_samples(self._h, int(nsamples), int(sample_rate)))

    def _convert_plan(self, who: str, slots, recordings, law, i16_scale: int, channel, sample_rate):
        """What ``convert`` and ``scan_segments(convert=...)`` share, under ``_scan_lock``: the recordings packed as ``scan`` packs
        them and one channel item per recording -> (n, two, block, sample frames, fmt, lens, items)."""
        if sample_rate is None or self._scan_rate(sample_rate) is None:
            raise ConfigurationError("sample_rate", repr(sample_rate), f"{who}: a conversion needs the recordings' sample_rate, other than the "
                                     f"engine's {self.sample_rate} Hz")
        if isinstance(channel, str) and channel == "split":
            raise ConfigurationError("channel", repr(channel), f"{who}: a converted block is mono: channel is 'mix', 0, 1 or a sequence of these")
        n, per, two, _split, block, total, fmt, _offs, lens, items, _start = self._scan_plan(slots, recordings, 0, law, i16_scale, channel, None)
        if not two:
            mono = items
            items = (_ffi.ScanChItem * max(1, n))()
            for i in range(n):
                items[i] = _ffi.ScanChItem(mono[i].slot, mono[i].sample_offset, mono[i].nsamples, 0, 0)
        return n, two, block, total, fmt, lens, items

    def convert(self, recordings, sample_rate: int, taps=None, channel="mix", law: Optional[str] = None, i16_scale: int = 32767):
        """Whole recordings at ``sample_rate`` as continuous signals at the engine's rate (``vad_convert``): ``recordings`` as ``scan``
        takes them (1-D or ``[nsamples, 2]``, float32, int16, or uint8 codes with ``law``; ``channel``: ``"mix"``, 0, 1 or one per
        recording), decoded and channel-selected as the scans' loader does, never gated, zero-extended at their edges and filtered by
        the polyphase FIR of ``taps`` (odd, at most ``128 * L`` float32 at rate ``L * sample_rate``; default:
        ``cutter_vad_amd.scan.convert_taps``) as ``scipy.signal.resample_poly(x, L, M, window=taps / L)`` filters.  No stream is read and no
        model runs.  -> (data, start): one float32 array, recording i = ``data[start[i]:start[i] + convert_samples(len_i,
        sample_rate)]``; ``start[i]`` are multiples of 4, the samples between two recordings are +0.0, ``start[n]`` is the block's size."""
        rate = int(sample_rate)
        with self._scan_lock:
            n, two, block, total, fmt, lens, items = self._convert_plan("convert", np.zeros(len(recordings), np.int64), recordings, law, i16_scale,
                                                                        channel, sample_rate)
            h = self._convert_taps(rate, taps)
            start = np.zeros(n + 1, np.int64)
            for i in range(n):
                start[i + 1] = start[i] + ((max(self.convert_samples(int(lens[i]), rate), 0) + 3) & ~3)
            data = np.empty(int(start[-1]), np.float32)
            self._check(self._lib.vad_convert(self._h, items, n, block.ctypes.data_as(C.c_void_p), total, 2 if two else 1, fmt, rate,
                                              _ptr(h, C.c_float), h.size, _ptr(data, C.c_float), data.size, _ptr(start, C.c_int64)))
        return data, start

    def convert_device(self, offsets, lengths, sample_rate: int, d_audio: int, audio_samples: int, d_out: int, out_samples: int, taps=None,
                       fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, channel="mix", stream: int = 0) -> np.ndarray:
        """``convert`` on device pointers (integers; ``vad_convert_device``): recording i is the ``lengths[i]`` sample frames from
        ``offsets[i]`` (a multiple of 4) of the block at ``d_audio`` (4-byte aligned, 8 for two channels); the converted block goes to
        ``d_out`` (16-byte aligned, room for ``out_samples`` float32).  ``taps`` is a host array, read before the call returns.
        Asynchronous on ``stream``.  -> start [n + 1] as ``convert``."""
        rate = int(sample_rate)
        offs, lens = np.asarray(offsets, np.int64).reshape(-1), np.asarray(lengths, np.int64).reshape(-1)
        n = int(offs.size)
        if lens.size != n:
            raise AudioProcessingError(f"Model prediction failed: {lens.size} lengths for {n} offsets")
        chans = [self._scan_channel(channel)] * n if isinstance(channel, (str, int, np.integer)) else [self._scan_channel(c) for c in channel]
        if len(chans) != n:
            raise AudioProcessingError(f"Model prediction failed: {len(chans)} channels for {n} recordings")
        items = (_ffi.ScanChItem * max(1, n))()
        for i in range(n):
            items[i] = _ffi.ScanChItem(0, int(offs[i]), int(lens[i]), chans[i] if int(channels) == 2 else 0, 0)
        h = self._convert_taps(rate, taps)
        start = np.zeros(n + 1, np.int64)
        self._check(self._lib.vad_convert_device(self._h, items, n, d_audio or None, int(audio_samples), int(channels), int(fmt), rate,
                                                 _ptr(h, C.c_float), h.size, d_out or None, int(out_samples), _ptr(start, C.c_int64), stream or None))
        return start

    def _scan_convert_segments(self, slots, recordings, hop, law, i16_scale, denoise, channel, sample_rate, convert) -> np.ndarray:
        """``scan_segments(convert=...)``: ``vad_scan_convert_segments``"""
        hop = self.frame_samples // 2 if hop is None else int(hop)
        thr = -1.0 if denoise is None else float(denoise)
        with self._scan_lock:
            n, two, block, total, fmt, lens, items = self._convert_plan("scan_segments", slots, recordings, law, i16_scale, channel, sample_rate)
            rate = int(sample_rate)
            h = self._convert_taps(rate, convert)
            outs = np.array([max(self.convert_samples(int(v), rate), 0) for v in lens], np.int64)
            frames = sum(max(self.scan_frame_count(int(v), hop), 0) for v in outs) if hop >= 1 else 0
            table = np.zeros(frames // 64 + 16, _ffi.SEGMENT_DTYPE)
            count = C.c_int64(0)
            start = np.zeros(n + 1, np.int64)
            self._scan_last = None
            self._tail_items = None
            self._check(self._lib.vad_scan_convert_segments(self._h, items, n, block.ctypes.data_as(C.c_void_p), total, 2 if two else 1, fmt, rate,
                                                            _ptr(h, C.c_float), h.size, hop, thr, table.ctypes.data_as(C.POINTER(_ffi.Segment)),
                                                            table.size, C.byref(count), _ptr(start, C.c_int64)))
            self._tail_items = n
            if frames:
                # the resident block is the CONVERTED one: mono float32 at the engine's rate
                self._scan_last = {"samples": int(start[-1]), "channels": 1, "fmt": _ffi.VAD_FMT_F32, "offsets": start[:-1].copy(), "lengths": outs,
                                   "converted_from": rate}
            if count.value > table.size:
                rest = np.zeros(count.value - table.size, _ffi.SEGMENT_DTYPE)
                self._check(self._lib.vad_scan_segments_read(self._h, table.size, rest.size, rest.ctypes.data_as(C.POINTER(_ffi.Segment))))
                table = np.concatenate([table, rest])
        return table[:count.value]

    def segments_device(self, d_events: int, d_seg: int, d_probs: int, out_start, d_segs: int, seg_cap: int, d_nsegs: int,
                        stream: int = 0) -> None:
        """The segment table of a scan on device pointers (integers; ``vad_segments_device``): ``d_events`` (16-byte aligned),
        ``d_seg`` and ``d_probs`` as ``scan_device`` wrote them, ``out_start`` the positions it returned; the first
        ``min(count, seg_cap)`` records go to ``d_segs`` (16-byte aligned, 24 bytes each: ``_ffi.SEGMENT_DTYPE``), the true count
        to the int64 at ``d_nsegs``.  Asynchronous on ``stream``; every engine has it."""
        start = np.ascontiguousarray(out_start, dtype=np.int64).reshape(-1)
        self._check(self._lib.vad_segments_device(self._h, d_events or None, d_seg or None, d_probs or None, _ptr(start, C.c_int64),
                                                  max(start.size - 1, 0), d_segs or None, int(seg_cap), d_nsegs or None, stream or None))

    @staticmethod
    def _threshold_sets(thresholds):
        rows = [tuple(r) for r in thresholds]
        return (_ffi.Thresholds * max(1, len(rows)))(*[_ffi.Thresholds(*r) for r in rows]), len(rows)

    def resegment(self, thresholds) -> List[np.ndarray]:
        """Segment tables at other thresholds from the per-frame results the last ``scan_segments`` left on the GPU
        (``vad_scan_resegment``): no upload, no model launch, no stream touched.  ``thresholds``: a sequence of up to 64 6-tuples in
        ``set_thresholds_many``'s order -> one table (``_ffi.SEGMENT_DTYPE``) per set, each what ``scan_segments`` returns for the
        same recordings on freshly opened streams with that set.  The resident block stays: ``cut(audio=None)`` works on any of
        the tables.  Call it inside ``scan_session()``, behind the ``scan_segments``: another thread's scan, or any step on this
        engine, replaces the results (the call then raises)."""
        sets, nt = self._threshold_sets(thresholds)
        start = np.zeros(nt + 1, np.int64)
        with self._scan_lock:
            self._check(self._lib.vad_scan_resegment(self._h, sets, nt, None, 0, _ptr(start, C.c_int64)))
            table = np.zeros(int(start[-1]), _ffi.SEGMENT_DTYPE)
            if table.size:
                self._check(self._lib.vad_scan_resegment(self._h, sets, nt, table.ctypes.data_as(C.POINTER(_ffi.Segment)), table.size,
                                                         _ptr(start, C.c_int64)))
        return [table[int(start[k]):int(start[k + 1])] for k in range(nt)]

    def resegment_device(self, d_events: int, d_probs: int, out_start, thresholds, d_segs: int, seg_cap: int, d_set_start: int,
                         stream: int = 0) -> None:
        """``resegment`` on device pointers (integers; ``vad_resegment_device``): ``d_events`` (16-byte aligned) and ``d_probs`` as
        ``scan_device`` wrote them, ``out_start`` the positions it returned; the first ``min(total, seg_cap)`` records - by set,
        then item, then frame - go to ``d_segs`` (16-byte aligned, ``_ffi.SEGMENT_DTYPE``), the running counts per set to the
        int64 ``[len(thresholds) + 1]`` at ``d_set_start``.  Asynchronous on ``stream``; every engine has it."""
        sets, nt = self._threshold_sets(thresholds)
        start = np.ascontiguousarray(out_start, dtype=np.int64).reshape(-1)
        self._check(self._lib.vad_resegment_device(self._h, d_events or None, d_probs or None, _ptr(start, C.c_int64), max(start.size - 1, 0),
                                                   sets, nt, d_segs or None, int(seg_cap), d_set_start or None, stream or None))

    def scan_tails(self) -> np.ndarray:
        """The segment still open at the last frame of each item of the last ``scan_segments`` (``vad_scan_tails``) -> one record
        (``_ffi.SEGMENT_DTYPE``) per item, in item order: ``first_frame = frames - nframes`` (negative when the slot entered the
        recording inside a segment) and the statistics of a table's record; ``nframes == 0`` - the whole record is zero - where the
        recording ended outside speech.  The scan saved the lengths itself: resetting, closing or retuning its streams behind it
        does not change the answer.  No model launch, no stream touched, the tables and the resident block left alone.  Call it
        inside ``scan_session()``, behind the ``scan_segments``."""
        with self._scan_lock:
            n = 0 if self._tail_items is None else self._tail_items
            tails = np.zeros(n, _ffi.SEGMENT_DTYPE)
            self._check(self._lib.vad_scan_tails(self._h, tails.ctypes.data_as(C.POINTER(_ffi.Segment)) if n else None, n))
        return tails

    def resegment_tails(self, thresholds) -> List[np.ndarray]:
        """``scan_tails`` at other thresholds (``vad_scan_resegment_tails``): per set of ``thresholds`` (as ``resegment`` takes
        them) the tails of fresh state machines with that set, replayed over the per-frame results the last ``scan_segments`` left
        on the GPU -> one array of ``scan_tails``' shape per set."""
        sets, nt = self._threshold_sets(thresholds)
        with self._scan_lock:
            n = 0 if self._tail_items is None else self._tail_items
            tails = np.zeros(nt * n, _ffi.SEGMENT_DTYPE)
            self._check(self._lib.vad_scan_resegment_tails(self._h, sets, nt, tails.ctypes.data_as(C.POINTER(_ffi.Segment)) if tails.size else None, n))
        return [tails[k * n:(k + 1) * n] for k in range(nt)]

    def tails_device(self, slots, d_events: int, d_probs: int, out_start, d_tails: int, stream: int = 0) -> None:
        """``scan_tails`` on device pointers (integers; ``vad_tails_device``): ``slots`` the streams of the items in item order,
        ``d_events`` (16-byte aligned) and ``d_probs`` as ``scan_device`` wrote them, ``out_start`` the positions it returned; one
        record per item goes to ``d_tails`` (16-byte aligned, ``_ffi.SEGMENT_DTYPE``).  The launch reads the slots' state machines
        when it runs: enqueue it on ``stream`` behind the scan.  Every engine has it."""
        sl = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        start = np.ascontiguousarray(out_start, dtype=np.int64).reshape(-1)
        self._check(self._lib.vad_tails_device(self._h, _ptr(sl, C.c_int64), d_events or None, d_probs or None, _ptr(start, C.c_int64),
                                               max(start.size - 1, 0), d_tails or None, stream or None))

    def resegment_tails_device(self, d_events: int, d_probs: int, out_start, thresholds, d_tails: int, stream: int = 0) -> None:
        """``resegment_tails`` on device pointers (``vad_resegment_tails_device``): entry ``k * n + i`` of ``d_tails`` (16-byte
        aligned, ``len(thresholds) * n`` records) is the tail of set ``k``, item ``i``.  Asynchronous on ``stream``; every engine
        has it."""
        sets, nt = self._threshold_sets(thresholds)
        start = np.ascontiguousarray(out_start, dtype=np.int64).reshape(-1)
        self._check(self._lib.vad_resegment_tails_device(self._h, d_events or None, d_probs or None, _ptr(start, C.c_int64),
                                                         max(start.size - 1, 0), sets, nt, d_tails or None, stream or None))

    @staticmethod
    def _refine_rule(rule) -> _ffi.Refine:
        """``SegmentRefine``, any object with its six fields, or a 6-sequence in the struct's order -> ``vad_refine``"""
        names = ("pad_before", "pad_after", "merge_gap", "min_frames", "max_frames", "reserved")
        vals = [getattr(rule, k) for k in names] if hasattr(rule, "pad_before") else list(rule)
        if len(vals) != 6:
            raise AudioProcessingError(f"Model prediction failed: a refine rule has six fields, got {len(vals)}")
        return _ffi.Refine(*[int(v) for v in vals])

    def refine(self, rule, table: Optional[np.ndarray] = None, tails: Optional[np.ndarray] = None) -> np.ndarray:
        """A segment table padded, merged, thinned and split on the GPU (``vad_scan_refine``; the rule is ``vad_refine``'s in
        include/vad_engine.h, ``rule`` a :class:`~cutter_vad_amd.scan.SegmentRefine`), against the per-frame results the last
        ``scan_segments`` left there: a long segment is cut at the quietest frame near the cut point, and ``counted``,
        ``mean_prob`` and ``max_prob`` are those of the new ranges.  ``table``: what ``scan_segments`` returned or one table of
        ``resegment`` (sorted by item); None: the scan's own table, which never left the GPU.  ``tails``: ``scan_tails()`` or one
        array of ``resegment_tails`` - each item's open segment joins its records as the last one.  No upload but these, no model
        launch, no stream touched; the resident block stays, and ``cut(audio=None)`` cuts the refined records like any others.  Call
        it inside ``scan_session()``, behind the ``scan_segments``."""
        rl = self._refine_rule(rule)
        seg_p = C.POINTER(_ffi.Segment)
        tab = None if table is None else np.ascontiguousarray(table, dtype=_ffi.SEGMENT_DTYPE).reshape(-1)
        tl = None if tails is None else np.ascontiguousarray(tails, dtype=_ffi.SEGMENT_DTYPE).reshape(-1)
        with self._scan_lock:
            if tl is not None and tl.size != (self._tail_items or 0):
                raise AudioProcessingError(f"Model prediction failed: refine: {tl.size} tails for the {self._tail_items or 0} items of the scan")
            src = None if tab is None else tab if tab.size else _ffi.EMPTY_TABLE      # a null table names the resident one
            where = (self._h, None if src is None else src.ctypes.data_as(seg_p), 0 if tab is None else tab.size,
                     None if tl is None or tl.size == 0 else tl.ctypes.data_as(seg_p), C.byref(rl))
            count = C.c_int64(0)
            self._check(self._lib.vad_scan_refine(*where, None, 0, C.byref(count)))
            out = np.zeros(count.value, _ffi.SEGMENT_DTYPE)
            if out.size:
                self._check(self._lib.vad_scan_refine(*where, out.ctypes.data_as(seg_p), out.size, C.byref(count)))
        return out[:count.value]

    def refine_device(self, d_segs_in: int, d_nsegs_in: int, in_cap: int, d_tails: int, d_events: int, d_probs: int, out_start, rule,
                      d_segs_out: int, seg_cap: int, d_nsegs_out: int, stream: int = 0) -> None:
        """``refine`` on device pointers (integers; ``vad_refine_device``): the first ``min(*d_nsegs_in, in_cap)`` records at
        ``d_segs_in`` as ``segments_device`` wrote them, ``d_tails`` 0 or the ``n`` records of ``tails_device``, ``d_events`` and
        ``d_probs`` as ``scan_device`` wrote them, ``out_start`` the positions it returned; the first ``min(count, seg_cap)``
        refined records go to ``d_segs_out``, the true count to the int64 at ``d_nsegs_out``.  Tables, tails and events 16-byte
        aligned, the counts 8-byte.  Asynchronous on ``stream``; every engine has it."""
        rl = self._refine_rule(rule)
        start = np.ascontiguousarray(out_start, dtype=np.int64).reshape(-1)
        self._check(self._lib.vad_refine_device(self._h, d_segs_in or None, d_nsegs_in or None, int(in_cap), d_tails or None, d_events or None,
                                                d_probs or None, _ptr(start, C.c_int64), max(start.size - 1, 0), C.byref(rl), d_segs_out or None,
                                                int(seg_cap), d_nsegs_out or None, stream or None))

    def scan_device(self, slots, offsets, lengths, d_audio: int, audio_samples: int, d_probs: int, d_events: int = 0, d_seg: int = 0,
                    hop: Optional[int] = None, fmt: int = _ffi.VAD_FMT_F32, denoise: Optional[float] = 0.01, stream: int = 0,
                    channels: int = 1, channel=None, sample_rate: Optional[int] = None) -> np.ndarray:
        """``scan`` on device pointers (integers): recording i = ``lengths[i]`` samples from sample ``offsets[i]`` (a multiple
        of 4) of the block at ``d_audio``; results go to the CSR positions this returns (``out_start`` [n + 1]).  Asynchronous.
        ``channels = 2`` (``vad_scan_channels_device``): the block is interleaved two-channel audio (8-byte aligned), offsets,
        lengths and ``audio_samples`` count sample frames, and ``channel`` is ``"mix"`` (the default), ``0``, ``1`` or one of these
        per item - list a recording twice, with two slots, to scan both of its channels.
        ``sample_rate`` as in ``scan`` (``vad_scan_rate_device``): the block is at that rate, offsets, lengths and ``hop`` count input samples."""
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        if channels != 1 or channel is not None or sr is not None:
            channel = "mix" if channel is None else channel
            if isinstance(channel, (str, int, np.integer)):
                chans = [_ffi.VAD_SCAN_MIX if channels == 1 and channel == "mix" else self._scan_channel(channel)] * s.size
            else:
                chans = [self._scan_channel(c) for c in channel]
                if len(chans) != s.size:
                    raise AudioProcessingError(f"Model prediction failed: {len(chans)} channels for {s.size} recordings")
            citems = (_ffi.ScanChItem * max(1, s.size))()
            start = np.zeros(s.size + 1, np.int64)
            for i in range(s.size):
                citems[i] = _ffi.ScanChItem(int(s[i]), int(offsets[i]), int(lengths[i]), chans[i], 0)
                start[i + 1] = start[i] + self.scan_frame_count(int(lengths[i]), hop, sr)
            thr = -1.0 if denoise is None else float(denoise)
            if sr is not None:
                self._check(self._lib.vad_scan_rate_device(self._h, citems, s.size, d_audio, int(audio_samples), int(channels), fmt, sr, hop, thr,
                                                           _ptr(start, C.c_int64), d_probs, d_events or None, d_seg or None, stream or None))
                return start
            self._check(self._lib.vad_scan_channels_device(self._h, citems, s.size, d_audio, int(audio_samples), int(channels), fmt, hop, thr,
                                                           _ptr(start, C.c_int64), d_probs, d_events or None, d_seg or None, stream or None))
            return start
        items = (_ffi.ScanItem * max(1, s.size))()
        start = np.zeros(s.size + 1, np.int64)
        for i in range(s.size):
            items[i] = _ffi.ScanItem(int(s[i]), int(offsets[i]), int(lengths[i]))
            start[i + 1] = start[i] + self.scan_frame_count(int(lengths[i]), hop)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_scan_device(self._h, items, s.size, d_audio, int(audio_samples), fmt, hop, thr, _ptr(start, C.c_int64),
                                              d_probs, d_events or None, d_seg or None, stream or None))
        return start

    # ------------------------------------------------------------------ finished segments' audio
    def scan_session(self):
        """The lock that makes packing + scanning one critical section, re-entrant: ``with engine.scan_session():`` around a
        ``scan`` and the ``cut(audio=None)`` behind it keeps another thread's scan from replacing the block in between."""
        return self._scan_lock

    @property
    def last_scan(self) -> Optional[dict]:
        """What ``scan`` packed last - ``samples``, ``channels``, ``fmt``, ``offsets``, ``lengths`` (sample frames of the block), and
        ``rate`` when it is a block at another rate than the engine's (``scan_segments(sample_rate=...)``) - or None; meaningful
        inside ``scan_session()``."""
        return self._scan_last

    def cut_samples(self, nframes: int, hop: Optional[int] = None, layout="frames", sample_rate: Optional[int] = None) -> int:
        """Samples of a segment of ``nframes`` frames (``vad_cut_samples``): ``nframes * frame_samples`` for ``"frames"``,
        ``(nframes - 1) * hop + frame_samples`` for ``"range"``.  ``sample_rate`` (``vad_rate_cut_samples``): a segment of a block at
        that rate - ``nframes * 512`` samples at 16 kHz for ``"frames"``, ``(nframes - 1) * hop + scan_chunk_samples(sample_rate)``
        input samples for ``"range"``."""
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        lay = self._cut_enum(_ffi.CUT_LAYOUTS, "layout", layout)
        if sr is None:
            n = int(self._lib.vad_cut_samples(self._h, int(nframes), hop, lay))
        else:
            n = int(self._lib.vad_rate_cut_samples(self._h, int(nframes), sr, hop, lay))
        if n < 0:
            raise AudioProcessingError(f"Model prediction failed: bad frame count, hop or layout ({nframes}, {hop}, {layout!r})")
        return n

    @staticmethod
    def _cut_enum(table, what, v) -> int:
        if isinstance(v, str) and v in table:
            return table[v]
        raise AudioProcessingError(f"Model prediction failed: {what} is one of {sorted(table)}, got {v!r}")

    def _cut_items(self, segments, hop: int, layout: int, channels: int, out_samples=None, rate: Optional[int] = None):
        """segments: (sample_offset, first_frame, nframes[, channel]) each -> (items, out_start [n + 1]): payloads packed in the
        order listed, unless ``out_samples`` gives every segment's first output sample; ``rate``: a block at that rate - a frame
        is a chunk in the block and 512 samples in a ``"frames"`` payload"""
        segs = [tuple(sg) for sg in segments]
        n = len(segs)
        items = (_ffi.CutItem * max(1, n))()
        start = np.zeros(n + 1, np.int64)
        frame = self.frame_samples if rate is None else self.scan_chunk_samples(rate)
        out_frame = self.frame_samples if rate is None else 512
        for i, sg in enumerate(segs):
            if len(sg) not in (3, 4):
                raise AudioProcessingError(f"Model prediction failed: a segment is (sample_offset, first_frame, nframes[, channel]), got {sg!r}")
            ch = (_ffi.VAD_SCAN_MIX if channels == 2 else 0) if len(sg) == 3 else self._scan_channel(sg[3])
            nf = int(sg[2])
            count = nf * out_frame if layout == _ffi.VAD_CUT_FRAMES else (nf - 1) * hop + frame
            o = int(start[i]) if out_samples is None else int(out_samples[i])
            items[i] = _ffi.CutItem(int(sg[0]), int(sg[1]), nf, o, ch, 0)
            start[i + 1] = start[i] + max(count, 0)
        return items, start

    def _cut_block(self, who: str, audio, law: Optional[str], i16_scale: int, sample_rate: Optional[int]):
        """The block a cut or a levels call names, with ``_scan_lock`` held -> (rate or None, sample frames, channels, fmt,
        pointer or None, the array that owns the pointer): ``audio=None`` is the block the last scan packed."""
        sr = self._scan_rate(sample_rate)
        if audio is None:
            last = self._scan_last
            if last is None:
                raise AudioProcessingError(f"Model prediction failed: {who}(audio=None) follows a scan() of this engine that uploaded a block")
            if sample_rate is not None and sr != last.get("rate"):
                raise AudioProcessingError(f"Model prediction failed: {who}(audio=None, sample_rate={sample_rate}): the block of the last scan "
                                           f"is at {last.get('rate', self.sample_rate)} Hz")
            return last.get("rate"), last["samples"], last["channels"], last["fmt"], None, None
        block = np.asarray(audio)
        g711 = _law_format(law, block)
        if g711 is None and block.dtype not in _FMT:
            block = block.astype(np.float32)
        if block.ndim not in (1, 2) or (block.ndim == 2 and block.shape[1] != 2):
            raise AudioProcessingError(f"Model prediction failed: the audio block is 1-D or [nsamples, 2], got {block.shape}")
        block = np.ascontiguousarray(block)
        fmt = g711 if g711 is not None else _FMT[block.dtype]
        if fmt == _ffi.VAD_FMT_I16_32767 and i16_scale == 32768:
            fmt = _ffi.VAD_FMT_I16_32768
        self._scan_last = None      # the engine's resident block is this one now, not the last scan's
        return sr, int(block.shape[0]), block.ndim, fmt, block.ctypes.data_as(C.c_void_p), block

    @staticmethod
    def _cut_gains(gains, n: int) -> np.ndarray:
        g = np.ascontiguousarray(np.asarray(gains, np.float32).reshape(-1))
        if g.size != n:
            raise AudioProcessingError(f"Model prediction failed: gains has {g.size} entries for {n} segments")
        return g

    def cut(self, segments, hop: Optional[int] = None, law: Optional[str] = None, i16_scale: int = 32767, denoise: Optional[float] = 0.01,
            layout="frames", out="pcm16", audio=None, sample_rate: Optional[int] = None, gains=None):
        """The audio of finished segments (``vad_scan_cut``): ``segments`` lists ``(sample_offset, first_frame, nframes[, channel])``
        - the recording's first sample frame in the block, the segment's first frame (``e - L + 1`` for an END at frame ``e`` with
        ``seg_frames`` ``L``) and its length in frames; ``channel`` as in ``scan`` (default: ``"mix"`` of a two-channel block).
        ``layout="frames"``: the frames back to back (the reference's ``voice_end`` payload), ``"range"``: the sample range once.
        ``out="pcm16"``: int16, ``clip(x * 32767)`` toward zero - a WAV payload; ``"f32"``: the gated float32 the model read.
        -> (data, start): the payloads packed in one array, segment i = ``data[start[i]:start[i + 1]]``.
        ``audio=None``: the block ``scan`` packed last, which is still on the GPU - nothing is uploaded; format, channels and
        size are that scan's (``law`` / ``i16_scale`` are ignored).  Another thread's ``scan`` would replace the block: hold
        ``scan_session()`` around the scan and the cut.  ``audio``: a block of its own, a 1-D array or a C-contiguous
        ``[nsamples, 2]`` array (float32, int16, or uint8 codes with ``law``); it is uploaded and becomes the resident block.
        ``sample_rate`` (``vad_scan_rate_cut``): the block is at 8000, 24000 or 48000 Hz - ``first_frame`` / ``nframes`` count chunks of
        ``scan_chunk_samples(sample_rate)`` at ``hop`` input samples.  ``"frames"``: each chunk resampled on the GPU to the 512 samples
        the model read (``Engine.resample`` of the decoded chunk, byte for byte), then gated; ``"range"``: the segment's own samples at
        the input rate, NOT gated.  With ``audio=None`` behind ``scan_segments(sample_rate=...)`` the rate is that scan's; another
        ``sample_rate`` given then is an error.  With an ``audio``, ``sample_rate`` names its rate.
        ``gains`` (``vad_scan_cut_gain``): one finite float32 factor per segment; a sample is the gated value times its segment's
        factor (one float32 multiply) ahead of the conversion.  All ones: the bytes of the call without it."""
        lay, of = self._cut_enum(_ffi.CUT_LAYOUTS, "layout", layout), self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("cut", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._cut_items(segments, hop, lay, channels, rate=sr)
            n = len(start) - 1
            data = np.empty(int(start[-1]), np.int16 if of == _ffi.VAD_CUT_PCM16 else np.float32)
            thr = -1.0 if denoise is None else float(denoise)
            res = (thr, lay, of, data.ctypes.data_as(C.c_void_p), data.size)
            if gains is not None:
                g = self._cut_gains(gains, n)
                self._check(self._lib.vad_scan_cut_gain(self._h, items, n, _ptr(g, C.c_float), ptr, total, channels, fmt, sr or 0, hop, *res))
            elif sr is not None:
                self._check(self._lib.vad_scan_rate_cut(self._h, items, n, ptr, total, channels, fmt, sr, hop, *res))
            else:
                self._check(self._lib.vad_scan_cut(self._h, items, n, ptr, total, channels, fmt, hop, *res))
        return data, start

    def cut_device(self, segments, d_audio: int, audio_samples: int, d_out: int, out_samples: int, hop: Optional[int] = None,
                   fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, denoise: Optional[float] = 0.01, layout="frames", out="pcm16",
                   stream: int = 0, out_start=None, sample_rate: Optional[int] = None, gains=None) -> np.ndarray:
        """``cut`` on device pointers (integers; ``vad_scan_cut_device``): the block at ``d_audio`` (4-byte aligned, 8 for two
        channels), the payloads to ``d_out`` (16-byte aligned, room for ``out_samples`` samples), packed in the order listed
        or at ``out_start[i]`` (multiples of 4).  Asynchronous on ``stream``.  -> start [n + 1] of the packed order.
        ``sample_rate`` as in ``cut`` (``vad_scan_rate_cut_device``): the block is at that rate.  ``gains`` as in ``cut``
        (``vad_scan_cut_gain_device``): a host array, read before the call returns."""
        lay, of = self._cut_enum(_ffi.CUT_LAYOUTS, "layout", layout), self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._cut_items(segments, hop, lay, int(channels), out_start, rate=sr)
        thr = -1.0 if denoise is None else float(denoise)
        n = len(start) - 1
        where = (d_audio or None, int(audio_samples), int(channels), int(fmt))
        res = (thr, lay, of, d_out or None, int(out_samples), stream or None)
        if gains is not None:
            g = self._cut_gains(gains, n)
            self._check(self._lib.vad_scan_cut_gain_device(self._h, items, n, _ptr(g, C.c_float), *where, sr or 0, hop, *res))
        elif sr is not None:
            self._check(self._lib.vad_scan_rate_cut_device(self._h, items, n, *where, sr, hop, *res))
        else:
            self._check(self._lib.vad_scan_cut_device(self._h, items, n, *where, hop, *res))
        return start

    # ------------------------------------------------------------------ segment audio at 16 kHz from a rate block
    @staticmethod
    def _resample_taps(rate: int, taps) -> np.ndarray:
        if taps is None:
            from .scan import resample_taps
            return resample_taps(rate)
        return np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))

    def resample_cut_samples(self, nframes: int, sample_rate: int, hop: Optional[int] = None) -> int:
        """Samples at 16 kHz of a segment of ``nframes`` chunks of a block at ``sample_rate`` (``vad_resample_cut_samples``): ``(nframes
        - 1) * hop + chunk`` input samples times 16000 / ``sample_rate``, rounded down to a multiple of 4; -1: bad arguments."""
        hop = self.scan_chunk_samples(sample_rate) // 2 if hop is None else int(hop)
        return int(self._lib.vad_resample_cut_samples(self._h, int(nframes), int(sample_rate), hop))

    def _resample_items(self, segments, rate: int, hop: int, channels: int, out_samples=None):
        """``_cut_items`` for ``resample_cut``: a segment's count is ``resample_cut_samples`` of its frames"""
        segs = [tuple(sg) for sg in segments]
        items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, channels, None, rate=rate)
        start = np.zeros(len(segs) + 1, np.int64)
        for i, sg in enumerate(segs):
            items[i].out_sample = int(start[i]) if out_samples is None else int(out_samples[i])
            start[i + 1] = start[i] + max(int(self._lib.vad_resample_cut_samples(self._h, int(sg[2]), rate, hop)), 0)
        return items, start

    def resample_cut(self, segments, sample_rate: int, taps=None, hop: Optional[int] = None, out="pcm16", audio=None,
                     law: Optional[str] = None, i16_scale: int = 32767, gains=None):
        """The audio of finished segments of a block at ``sample_rate`` (8000, 24000 or 48000 Hz) as one continuous signal each at
        16 kHz (``vad_scan_resample_cut``): the samples ``cut(segments, layout="range", out="f32", sample_rate=...)`` gives - decoded,
        channel-selected, never gated - zero-extended at the segment's edges and filtered by the polyphase FIR of ``taps`` (odd, at most
        511 float32 at rate ``L * sample_rate``; default: ``cutter_vad_amd.scan.resample_taps(sample_rate)``), as
        ``scipy.signal.resample_poly(x, L, M, window=taps)`` does on the cut.  -> (data, start) as ``cut``; a segment has
        ``resample_cut_samples`` samples.  ``audio``, ``law``, ``i16_scale``, ``gains`` and the ``scan_session()`` rule as in ``cut``:
        ``audio=None`` is the block ``scan_segments(sample_rate=...)`` left on the GPU."""
        of = self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        rate = int(sample_rate)
        h = self._resample_taps(rate, taps)
        with self._scan_lock:
            _sr, total, channels, fmt, ptr, _keep = self._cut_block("resample_cut", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(rate) // 2 if hop is None else int(hop)
            items, start = self._resample_items(segments, rate, hop, channels)
            n = len(start) - 1
            data = np.empty(int(start[-1]), np.int16 if of == _ffi.VAD_CUT_PCM16 else np.float32)
            g = None if gains is None else self._cut_gains(gains, n)
            self._check(self._lib.vad_scan_resample_cut(self._h, items, n, None if g is None else _ptr(g, C.c_float), _ptr(h, C.c_float), h.size,
                                                        ptr, total, channels, fmt, rate, hop, of, data.ctypes.data_as(C.c_void_p), data.size))
        return data, start

    def resample_cut_device(self, segments, sample_rate: int, d_audio: int, audio_samples: int, d_out: int, out_samples: int, taps=None,
                            hop: Optional[int] = None, fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, out="pcm16", stream: int = 0,
                            out_start=None, gains=None) -> np.ndarray:
        """``resample_cut`` on device pointers (integers; ``vad_scan_resample_cut_device``): the block at ``d_audio`` as ``cut_device``
        takes it, the payloads to ``d_out`` (16-byte aligned, room for ``out_samples`` samples), packed in the order listed or at
        ``out_start[i]`` (multiples of 4).  ``taps`` and ``gains`` are host arrays, read before the call returns.  Asynchronous on
        ``stream``.  -> start [n + 1] of the packed order."""
        of = self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        rate = int(sample_rate)
        h = self._resample_taps(rate, taps)
        hop = self.scan_chunk_samples(rate) // 2 if hop is None else int(hop)
        items, start = self._resample_items(segments, rate, hop, int(channels), out_start)
        n = len(start) - 1
        g = None if gains is None else self._cut_gains(gains, n)
        self._check(self._lib.vad_scan_resample_cut_device(self._h, items, n, None if g is None else _ptr(g, C.c_float), _ptr(h, C.c_float), h.size,
                                                           d_audio or None, int(audio_samples), int(channels), int(fmt), rate, hop, of,
                                                           d_out or None, int(out_samples), stream or None))
        return start

    # ------------------------------------------------------------------ segment levels
    def levels(self, segments, hop: Optional[int] = None, denoise: Optional[float] = 0.01, clip: float = 0.95, audio=None,
               law: Optional[str] = None, i16_scale: int = 32767, sample_rate: Optional[int] = None) -> np.ndarray:
        """Energy, peak and clipped samples of finished segments (``vad_scan_levels``), reduced on the GPU: ``segments`` as in
        ``cut``.  -> a structured array ``(energy_q32, peak, clipped)``, one record per segment: statistics of exactly the float32
        values ``cut(segments, layout="range", out="f32")`` with the same arguments gives - ``energy_q32`` the fixed-point sum of
        ``min(rint(x * x * 2^32), 2^32)`` (``cutter_vad_amd.scan.level_stats`` turns it into energy and RMS), ``peak`` ``max |x|``,
        ``clipped`` the samples with ``|x| >= clip`` (``AudioUtils.detect_clipping``'s threshold).  ``audio``, ``law``, ``i16_scale``,
        ``sample_rate`` and the ``scan_session()`` rule as in ``cut``; on a block at another rate the samples are input-rate samples
        and never gated.  Segments may share samples.  16 bytes per segment cross the link back."""
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("levels", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, channels, rate=sr)
            n = len(start) - 1
            out = np.zeros(n, _ffi.LEVEL_DTYPE)
            thr = -1.0 if denoise is None else float(denoise)
            self._check(self._lib.vad_scan_levels(self._h, items, n, ptr, total, channels, fmt, sr or 0, hop, thr, float(clip),
                                                  out.ctypes.data_as(C.POINTER(_ffi.Level))))
        return out

    def levels_device(self, segments, d_audio: int, audio_samples: int, d_levels: int, hop: Optional[int] = None,
                      fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, denoise: Optional[float] = 0.01, clip: float = 0.95, stream: int = 0,
                      sample_rate: Optional[int] = None) -> None:
        """``levels`` on device pointers (integers; ``vad_scan_levels_device``): the block at ``d_audio`` as ``cut_device`` takes it,
        one 16-byte record per segment to ``d_levels`` (8-byte aligned).  Asynchronous on ``stream``."""
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, int(channels), rate=sr)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_scan_levels_device(self._h, items, len(start) - 1, d_audio or None, int(audio_samples), int(channels), int(fmt),
                                                     sr or 0, hop, thr, float(clip), d_levels or None, stream or None))

    # ------------------------------------------------------------------ segment moments and audio batches
    def moments(self, segments, hop: Optional[int] = None, denoise: Optional[float] = 0.01, audio=None, law: Optional[str] = None,
                i16_scale: int = 32767, sample_rate: Optional[int] = None) -> np.ndarray:
        """Sum and energy of finished segments (``vad_scan_moments``), reduced on the GPU: ``segments`` and every other argument as
        in ``levels``.  -> a structured array ``(sum_q31, energy_q32)``, one record per segment, over exactly the float32 values
        ``cut(segments, layout="range", out="f32")`` gives: ``sum_q31`` the sum of ``rint(clip(x, -1, 1) * 2^31)``, ``energy_q32``
        the field of ``levels``, byte for byte.  ``mean = sum_q31 / (2^31 N)``, ``var = energy_q32 / (2^32 N) - mean^2``
        (``cutter_vad_amd.scan.audio_affine``).  Integer reductions: two calls give the same bytes."""
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("moments", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, channels, rate=sr)
            n = len(start) - 1
            out = np.zeros(n, _ffi.MOMENTS_DTYPE)
            thr = -1.0 if denoise is None else float(denoise)
            self._check(self._lib.vad_scan_moments(self._h, items, n, ptr, total, channels, fmt, sr or 0, hop, thr,
                                                   out.ctypes.data_as(C.POINTER(_ffi.Moments))))
        return out

    def moments_device(self, segments, d_audio: int, audio_samples: int, d_moments: int, hop: Optional[int] = None,
                       fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, denoise: Optional[float] = 0.01, stream: int = 0,
                       sample_rate: Optional[int] = None) -> None:
        """``moments`` on device pointers (integers; ``vad_scan_moments_device``): the block at ``d_audio`` as ``cut_device`` takes it,
        one 16-byte record per segment to ``d_moments`` (8-byte aligned).  Asynchronous on ``stream``."""
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, int(channels), rate=sr)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_scan_moments_device(self._h, items, len(start) - 1, d_audio or None, int(audio_samples), int(channels), int(fmt),
                                                      sr or 0, hop, thr, d_moments or None, stream or None))

    @staticmethod
    def _audio_batch_record(batch) -> _ffi.AudioBatchRecord:
        """``batch``: a ``_ffi.AudioBatchRecord``, an object with ``record()`` (``cutter_vad_amd.scan.AudioBatch``) or a dict of
        ``vad_audio_batch``'s fields - ``samples``, and optionally ``dtype`` / ``pad`` (names or numbers) and ``pad_value``"""
        if isinstance(batch, _ffi.AudioBatchRecord):
            return batch
        f = dict(batch.record() if hasattr(batch, "record") else batch)
        enum = lambda table, what, v: Engine._cut_enum(table, what, v) if isinstance(v, str) else int(v)
        return _ffi.AudioBatchRecord(int(f["samples"]), enum(_ffi.BATCH_DTYPES, "dtype", f.get("dtype", "f32")),
                                     enum(_ffi.BATCH_PADS, "pad", f.get("pad", "value")), float(f.get("pad_value", 0.0)))

    @staticmethod
    def _audio_windows(windows):
        w = np.ascontiguousarray(np.asarray(windows, _ffi.AUDIO_WINDOW_DTYPE).reshape(-1)) if not (
            isinstance(windows, np.ndarray) and windows.dtype == _ffi.AUDIO_WINDOW_DTYPE) else np.ascontiguousarray(windows.reshape(-1))
        return w, (w if w.size else np.zeros(1, _ffi.AUDIO_WINDOW_DTYPE)).ctypes.data_as(C.POINTER(_ffi.AudioWindow))

    @staticmethod
    def _audio_affine(shift, scale):
        """-> (the float32 arrays or None, their pointers, nss); one entry next to an entry per segment is repeated"""
        two = [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in (shift, scale)]
        most = max([a.size for a in two if a is not None] or [1])
        two = [np.full(most, a[0], np.float32) if a is not None and a.size == 1 else a for a in two]
        sizes = {a.size for a in two if a is not None}
        if len(sizes) > 1:
            raise AudioProcessingError(f"Model prediction failed: shift and scale have the same number of entries, got {sorted(sizes)}")
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        return two, (ptr(two[0]), ptr(two[1])), (sizes.pop() if sizes else 1)

    def audio_batch(self, segments, windows, batch, shift=None, scale=None, mask: bool = False, hop: Optional[int] = None,
                    denoise: Optional[float] = 0.01, audio=None, law: Optional[str] = None, i16_scale: int = 32767,
                    sample_rate: Optional[int] = None):
        """Normalised, zero-padded windows of segment audio in a model's number format (``vad_scan_audio_batch``), one launch:
        ``segments`` as in ``cut``, ``windows`` lists ``(seg, nsamples, sample0)`` - samples ``sample0 .. sample0 + nsamples - 1`` of
        segment ``seg``'s range (``cutter_vad_amd.scan.audio_windows``; ``sample0`` a multiple of 4) - ``batch`` is a
        ``cutter_vad_amd.scan.AudioBatch`` with ``samples`` set, or a dict of ``vad_audio_batch``'s fields.  A value is
        ``(x + shift[seg]) * scale[seg]`` in float32 over exactly the samples ``cut(segments, layout="range", out="f32")`` gives
        (``shift`` / ``scale``: one entry or one per segment, ``None`` for 0 and 1); the cells behind ``nsamples`` are pad cells.
        ``audio``, ``law``, ``i16_scale``, ``sample_rate`` and the ``scan_session()`` rule as in ``cut``.  -> [B, T]: float32,
        ``np.float16``, or the bfloat16 bit patterns as ``np.uint16``; with ``mask=True`` -> (batch, mask [B, T] uint8)."""
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("audio_batch", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, channels, rate=sr)
            b = self._audio_batch_record(batch)
            w, wp = self._audio_windows(windows)
            _own, ptrs, nss = self._audio_affine(shift, scale)
            out = np.empty((w.size, b.samples), {_ffi.VAD_BATCH_F32: np.float32, _ffi.VAD_BATCH_F16: np.float16}.get(b.dtype, np.uint16))
            m = np.empty((w.size, b.samples), np.uint8) if mask else None
            thr = -1.0 if denoise is None else float(denoise)
            self._check(self._lib.vad_scan_audio_batch(self._h, items, len(start) - 1, ptr, total, channels, fmt, sr or 0, hop, thr, C.byref(b),
                                                       wp, w.size, *ptrs, nss, out.ctypes.data_as(C.c_void_p), out.nbytes,
                                                       None if m is None else m.ctypes.data_as(C.c_void_p)))
        return (out, m) if mask else out

    def audio_batch_device(self, segments, windows, batch, d_audio: int, audio_samples: int, d_out: int, out_bytes: int, d_mask: int = 0,
                           shift=None, scale=None, hop: Optional[int] = None, fmt: int = _ffi.VAD_FMT_F32, channels: int = 1,
                           denoise: Optional[float] = 0.01, stream: int = 0, sample_rate: Optional[int] = None) -> Tuple[int, int]:
        """``audio_batch`` on device pointers (integers; ``vad_scan_audio_batch_device``): the block at ``d_audio`` as ``cut_device``
        takes it, the windows to ``d_out`` (16-byte aligned, room for ``out_bytes``) and the mask to ``d_mask`` (4-byte aligned, or 0:
        none), where a model on the same GPU reads them.  ``windows``, ``shift`` and ``scale`` are host arrays, read before the call
        returns.  Asynchronous on ``stream``.  -> the shape of the batch."""
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, int(channels), rate=sr)
        b = self._audio_batch_record(batch)
        w, wp = self._audio_windows(windows)
        _own, ptrs, nss = self._audio_affine(shift, scale)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_scan_audio_batch_device(self._h, items, len(start) - 1, d_audio or None, int(audio_samples), int(channels),
                                                          int(fmt), sr or 0, hop, thr, C.byref(b), wp, w.size, *ptrs, nss, d_out or None,
                                                          int(out_bytes), d_mask or None, stream or None))
        return (w.size, b.samples)

    # ------------------------------------------------------------------ log-mel features
    @staticmethod
    def _mel_arrays(spec):
        """``spec``: an object with ``operators()`` (``cutter_vad_amd.scan.MelSpec``) or the tuple that returns -
        ``(fields, op_re [n_fft, n_bins], op_im, filters [n_mels, n_bins])`` with ``fields`` a dict of ``vad_mel``'s fields (``pad`` /
        ``log`` as names or numbers) -> (_ffi.Mel, op_re, op_im, filters) as contiguous float32"""
        fields, op_re, op_im, filters = spec.operators() if hasattr(spec, "operators") else spec
        op_re, op_im, filters = (np.ascontiguousarray(np.asarray(a, np.float32)) for a in (op_re, op_im, filters))
        if isinstance(fields, _ffi.Mel):
            m = fields
        else:
            f = dict(fields)
            pad, log = f.get("pad", "reflect"), f.get("log", "log10")
            pad = Engine._cut_enum(_ffi.MEL_PADS, "pad", pad) if isinstance(pad, str) else int(pad)
            log = Engine._cut_enum(_ffi.MEL_LOGS, "log", log) if isinstance(log, str) else int(log)
            m = _ffi.Mel(int(f["n_fft"]), int(f["hop"]), int(f.get("n_bins", op_re.shape[-1])), int(f.get("n_mels", filters.shape[0])),
                         pad, log, float(f.get("floor", 1e-10)), 0)
        if op_re.shape != (m.n_fft, m.n_bins) or op_im.shape != op_re.shape or filters.shape != (m.n_mels, m.n_bins):
            raise AudioProcessingError(f"Model prediction failed: mel: op_re / op_im are [n_fft, n_bins] = [{m.n_fft}, {m.n_bins}] and filters "
                                       f"[n_mels, n_bins] = [{m.n_mels}, {m.n_bins}], got {op_re.shape}, {op_im.shape}, {filters.shape}")
        return m, op_re, op_im, filters

    def mel_frames(self, spec, nsamples: int) -> int:
        """Analysis frames of a segment of ``nsamples`` samples under ``spec`` (``vad_mel_frames``); -1: bad arguments."""
        m = self._mel_arrays(spec)[0]
        return int(self._lib.vad_mel_frames(C.byref(m), int(nsamples)))

    def _mel_rows(self, m, segments, hop: int) -> np.ndarray:
        start = np.zeros(len(segments) + 1, np.int64)
        for i, sg in enumerate(segments):
            rows = int(self._lib.vad_mel_frames(C.byref(m), max(0, (int(sg[2]) - 1) * hop + self.frame_samples))) if len(sg) > 2 else 0
            start[i + 1] = start[i] + max(rows, 0)      # (-1: the call itself refuses the segment, by name)
        return start

    def _mel_rows_16k(self, m, segments, hop: int, rate: int) -> np.ndarray:
        start = np.zeros(len(segments) + 1, np.int64)
        for i, sg in enumerate(segments):
            s16 = int(self._lib.vad_resample_cut_samples(self._h, int(sg[2]), rate, hop)) if len(sg) > 2 else -1
            rows = int(self._lib.vad_mel_frames(C.byref(m), s16)) if s16 >= 0 else 0
            start[i + 1] = start[i] + max(rows, 0)      # (-1: the call itself refuses the segment, by name)
        return start

    def mel(self, segments, spec, hop: Optional[int] = None, denoise: Optional[float] = 0.01, audio=None, law: Optional[str] = None,
            i16_scale: int = 32767, sample_rate: Optional[int] = None, taps=None):
        """Log-mel frames of finished segments (``vad_scan_mel``), computed on the GPU from the block: ``segments`` as in ``cut``,
        ``spec`` a ``cutter_vad_amd.scan.MelSpec`` or ``(fields, op_re, op_im, filters)`` (``_mel_arrays``).  -> ``(features
        [rows, n_mels] float32, start [n + 1])``: segment i's frames are ``features[start[i]:start[i + 1]]``, computed from exactly
        the float32 values ``cut(segments, layout="range", out="f32")`` with the same arguments gives.  ``hop`` is the SCAN's hop
        (the segments' frames), not the analysis hop, which is the spec's.  ``audio``, ``law``, ``i16_scale`` and the
        ``scan_session()`` rule as in ``cut``.  Segments may share samples.
        ``sample_rate`` (``vad_scan_rate_mel``), given and not the engine's: the block is at 8000, 24000 or 48000 Hz, and the
        features are those of each segment's 16 kHz signal as ``resample_cut(segments, sample_rate, taps, out="f32")`` gives it -
        never gated (``denoise`` is not read), computed on the GPU without the signal crossing the link.  ``taps`` as there."""
        m, op_re, op_im, filters = self._mel_arrays(spec)
        rate = self._scan_rate(sample_rate)
        if rate is not None:
            h = self._resample_taps(rate, taps)
            with self._scan_lock:
                sr, total, channels, fmt, ptr, _keep = self._cut_block("mel", audio, law, i16_scale, sample_rate)
                hop = self.scan_chunk_samples(rate) // 2 if hop is None else int(hop)
                segs = [tuple(sg) for sg in segments]
                items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, channels, rate=rate)
                start = self._mel_rows_16k(m, segs, hop, rate)
                out = np.empty((int(start[-1]), m.n_mels), np.float32)
                self._check(self._lib.vad_scan_rate_mel(self._h, items, len(segs), C.byref(m), _ptr(op_re, C.c_float), _ptr(op_im, C.c_float),
                                                        _ptr(filters, C.c_float), _ptr(h, C.c_float), h.size, ptr, total, channels, fmt, rate,
                                                        hop, out.ctypes.data_as(C.POINTER(C.c_float)), int(start[-1])))
            return out, start
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("mel", audio, law, i16_scale, None)
            if sr is not None:
                raise AudioProcessingError(f"Model prediction failed: mel(audio=None): the block of the last scan is at {sr} Hz; features are "
                                           "computed from blocks at the engine's own rate")
            hop = self.frame_samples // 2 if hop is None else int(hop)
            segs = [tuple(sg) for sg in segments]
            items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, channels)
            start = self._mel_rows(m, segs, hop)
            out = np.empty((int(start[-1]), m.n_mels), np.float32)
            thr = -1.0 if denoise is None else float(denoise)
            self._check(self._lib.vad_scan_mel(self._h, items, len(segs), C.byref(m), _ptr(op_re, C.c_float), _ptr(op_im, C.c_float),
                                               _ptr(filters, C.c_float), ptr, total, channels, fmt, hop, thr,
                                               out.ctypes.data_as(C.POINTER(C.c_float)), int(start[-1])))
        return out, start

    def mel_device(self, segments, spec, d_audio: int, audio_samples: int, d_out: int, out_rows: int, hop: Optional[int] = None,
                   fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, denoise: Optional[float] = 0.01, stream: int = 0,
                   sample_rate: Optional[int] = None, taps=None) -> np.ndarray:
        """``mel`` on device pointers (integers; ``vad_scan_mel_device``): the block at ``d_audio`` as ``cut_device`` takes it, the
        rows to ``d_out`` (16-byte aligned, room for ``out_rows`` rows of ``n_mels`` float32).  The operators stay host arrays, read
        before the call returns.  Asynchronous on ``stream``.  -> start [n + 1], the segments' first rows.  ``sample_rate`` and
        ``taps`` as in ``mel`` (``vad_scan_rate_mel_device``)."""
        m, op_re, op_im, filters = self._mel_arrays(spec)
        rate = self._scan_rate(sample_rate)
        if rate is not None:
            h = self._resample_taps(rate, taps)
            hop = self.scan_chunk_samples(rate) // 2 if hop is None else int(hop)
            segs = [tuple(sg) for sg in segments]
            items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, int(channels), rate=rate)
            start = self._mel_rows_16k(m, segs, hop, rate)
            self._check(self._lib.vad_scan_rate_mel_device(self._h, items, len(segs), C.byref(m), _ptr(op_re, C.c_float), _ptr(op_im, C.c_float),
                                                           _ptr(filters, C.c_float), _ptr(h, C.c_float), h.size, d_audio or None,
                                                           int(audio_samples), int(channels), int(fmt), rate, hop, d_out or None,
                                                           int(out_rows), stream or None))
            return start
        hop = self.frame_samples // 2 if hop is None else int(hop)
        segs = [tuple(sg) for sg in segments]
        items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, int(channels))
        start = self._mel_rows(m, segs, hop)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_scan_mel_device(self._h, items, len(segs), C.byref(m), _ptr(op_re, C.c_float), _ptr(op_im, C.c_float),
                                                  _ptr(filters, C.c_float), d_audio or None, int(audio_samples), int(channels), int(fmt), hop,
                                                  thr, d_out or None, int(out_rows), stream or None))
        return start

    # ------------------------------------------------------------------ model-ready feature batches
    def mel_keep(self, segments, spec, hop: Optional[int] = None, denoise: Optional[float] = 0.01, audio=None, law: Optional[str] = None,
                 i16_scale: int = 32767, sample_rate: Optional[int] = None, taps=None) -> np.ndarray:
        """``mel`` with the rows left on the GPU (``vad_scan_mel_keep``): the same arguments, the same rows byte for byte, in an
        engine-owned matrix - the RESIDENT MATRIX - that ``mel_stats`` and ``mel_batch`` read with ``features=None``; nothing comes
        back but -> start [n + 1], the segments' first rows.  The next ``mel_keep`` replaces the matrix; another thread's would too:
        hold ``scan_session()`` around the scan, the keep and the batch."""
        m, op_re, op_im, filters = self._mel_arrays(spec)
        rate = self._scan_rate(sample_rate)
        h = self._resample_taps(rate, taps) if rate is not None else None
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("mel_keep", audio, law, i16_scale, sample_rate if rate is not None else None)
            if rate is None and sr is not None:
                raise AudioProcessingError(f"Model prediction failed: mel_keep(audio=None): the block of the last scan is at {sr} Hz; give "
                                           "sample_rate")
            segs = [tuple(sg) for sg in segments]
            if rate is not None:
                hop = self.scan_chunk_samples(rate) // 2 if hop is None else int(hop)
                items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, channels, rate=rate)
                start = self._mel_rows_16k(m, segs, hop, rate)
            else:
                hop = self.frame_samples // 2 if hop is None else int(hop)
                items, _ = self._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, channels)
                start = self._mel_rows(m, segs, hop)
            rows = C.c_int64(-1)
            thr = -1.0 if denoise is None else float(denoise)
            self._check(self._lib.vad_scan_mel_keep(self._h, items, len(segs), C.byref(m), _ptr(op_re, C.c_float), _ptr(op_im, C.c_float),
                                                    _ptr(filters, C.c_float), None if h is None else _ptr(h, C.c_float),
                                                    0 if h is None else h.size, ptr, total, channels, fmt, rate or 0, hop, thr, C.byref(rows)))
            if rows.value != int(start[-1]):
                raise AudioProcessingError(f"Model prediction failed: mel_keep: the engine kept {rows.value} rows, {int(start[-1])} were expected")
        return start

    def mel_resident(self) -> Tuple[int, int, int]:
        """-> (rows, n_mels, segments) of the resident matrix (``vad_mel_resident``); an error when none is kept."""
        rows, nm, ns = C.c_int64(), C.c_int32(), C.c_int64()
        self._check(self._lib.vad_mel_resident(self._h, C.byref(rows), C.byref(nm), C.byref(ns)))
        return rows.value, nm.value, ns.value

    def mel_resident_read(self, first_row: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Rows of the resident matrix copied to the host (``vad_mel_resident_read``) -> float32 [count, n_mels]; default: all."""
        rows, nm, _ = self.mel_resident()
        count = rows - int(first_row) if count is None else int(count)
        out = np.empty((max(count, 0), nm), np.float32)
        self._check(self._lib.vad_mel_resident_read(self._h, int(first_row), count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    @staticmethod
    def _project_operator(op, bias):
        """-> (op float32 [n_in, n_out], bias float32 [n_out] or None, their pointers)"""
        f32p = C.POINTER(C.c_float)
        w = np.ascontiguousarray(np.asarray(op, np.float32))
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1:
            raise AudioProcessingError(f"Model prediction failed: mel_project: op is [n_in, n_out], got {w.shape}")
        b = None if bias is None else np.ascontiguousarray(np.asarray(bias, np.float32).reshape(-1))
        if b is not None and b.size != w.shape[1]:
            raise AudioProcessingError(f"Model prediction failed: mel_project: bias has n_out = {w.shape[1]} entries, got {b.size}")
        return w, b, w.ctypes.data_as(f32p), None if b is None else b.ctypes.data_as(f32p)

    def _project_resident(self, who: str, n_in: int) -> int:
        """-> the rows of the resident matrix, which has op's ``n_in`` columns"""
        rows, nm, _ = self.mel_resident()
        if nm != n_in:
            raise AudioProcessingError(f"Model prediction failed: {who}: the resident matrix has {nm} columns, op has n_in = {n_in} rows")
        return rows

    def mel_project(self, op, bias=None, features=None, out: bool = True):
        """A linear stage over a feature matrix on the GPU (``vad_mel_project``): ``y = bias + x @ op`` in float32, a fused
        multiply-add chain along ``k`` from the bias, with ``op`` [n_in, n_out] and ``bias`` [n_out] (``None``: 0), both 1 .. 128
        wide - the DCT of MFCC / LFCC (``cutter_vad_amd.scan.CepstralSpec.operator``), PCA / LDA, whitening, band selection.
        ``features`` [rows, n_in] float32, or ``None`` for the resident matrix of ``mel_keep``.  -> float32 [rows, n_out].
        ``out=False`` (with ``features=None``): the projection REPLACES the resident matrix - ``mel_stats``, ``mel_batch``,
        ``mel_batch_packed`` and ``mel_resident_read`` then work on it, the segments' first rows stay - and nothing comes back but
        -> (rows, n_out)."""
        w, b, wp, bp = self._project_operator(op, bias)
        x = None if features is None else np.ascontiguousarray(np.asarray(features, np.float32))
        if x is not None and x.ndim != 2:
            raise AudioProcessingError(f"Model prediction failed: features are [rows, n_in], got {x.shape}")
        if x is not None and x.shape[1] != w.shape[0]:
            raise AudioProcessingError(f"Model prediction failed: mel_project: the features have {x.shape[1]} columns, op has n_in = {w.shape[0]} rows")
        with self._scan_lock:
            rows, n_in = (self._project_resident("mel_project", w.shape[0]), w.shape[0]) if x is None else x.shape
            y = np.empty((rows, w.shape[1]), np.float32) if out else None
            self._check(self._lib.vad_mel_project(self._h, None if x is None else x.ctypes.data_as(C.POINTER(C.c_float)), rows, n_in, wp, bp,
                                                  w.shape[1], None if y is None else y.ctypes.data_as(C.POINTER(C.c_float))))
        return y if out else (rows, w.shape[1])

    def mel_project_device(self, op, bias=None, d_features: int = 0, rows: int = 0, d_out: int = 0, stream: int = 0) -> Tuple[int, int]:
        """``mel_project`` in device memory (``vad_mel_project_device``): ``d_features`` = 0: the resident matrix, else a float32 matrix
        [rows, n_in = op.shape[0]] on the GPU (an integer; 4-byte aligned); ``d_out`` a float32 [rows, n_out] there that does not
        overlap it, or 0: the projection replaces the resident matrix.  ``op`` and ``bias`` are host arrays, read before the call
        returns.  Asynchronous on ``stream``.  -> (rows, n_out)."""
        w, b, wp, bp = self._project_operator(op, bias)
        with self._scan_lock:
            if not d_features:
                rows = self._project_resident("mel_project_device", w.shape[0])
            self._check(self._lib.vad_mel_project_device(self._h, d_features or None, int(rows), w.shape[0], wp, bp, w.shape[1], d_out or None,
                                                         stream or None))
        return int(rows), w.shape[1]

    @staticmethod
    def _batch_start(start):
        """-> (start as int64 [n + 1] or None, its pointer, n), as every call of the family passes them on"""
        st = None if start is None else np.ascontiguousarray(np.asarray(start, np.int64).reshape(-1))
        return st, None if st is None else st.ctypes.data_as(C.POINTER(C.c_int64)), 0 if st is None else st.size - 1

    @staticmethod
    def _batch_source(features, start):
        """-> (features or None, its pointer, rows, n_mels or 0, start or None, its pointer, n) for the calls that take a matrix"""
        x = None if features is None else np.ascontiguousarray(np.asarray(features, np.float32))
        if x is not None and x.ndim != 2:
            raise AudioProcessingError(f"Model prediction failed: features are [rows, n_mels], got {x.shape}")
        st, sp, n = Engine._batch_start(start)
        if st is not None and st.size < 1:
            raise AudioProcessingError("Model prediction failed: start has n + 1 entries, got none")
        return x, None if x is None else x.ctypes.data_as(C.POINTER(C.c_float)), 0 if x is None else x.shape[0], 0 if x is None else x.shape[1], st, sp, n

    def mel_stats(self, features=None, start=None, moments: bool = True, group=None) -> dict:
        """Per-segment statistics of a feature matrix, reduced on the GPU (``vad_mel_stats``): ``features`` [rows, n_mels] float32 with
        the segments' first rows ``start`` [n + 1], or ``None`` for the resident matrix and its starts.  -> ``{"max": float32 [n]}`` -
        a segment's largest value, -inf for one without rows - and, with ``moments``, ``"sum"`` int64 [n, n_mels] and ``"sumsq"`` uint64
        [n, n_mels] of ``q = rint(clip(x, -2048, 2048) * 4096)`` and ``q * q``: exact integers, ``cutter_vad_amd.scan.batch_affine`` turns
        them into means and deviations.  With ``moments`` a segment has 2^17 rows at the most.  ``group`` [n] (``vad_mel_stats_grouped``):
        the statistics of every group of segments instead - ``max(group) + 1`` entries, or ``group=(array, ngroups)``; a group without
        rows has -inf and 0, and the 2^17 rows bound a group."""
        x, xp, rows, nm, st, sp, n = self._batch_source(features, start)
        gr = ng = None
        if group is not None:
            gr, ng = group if isinstance(group, tuple) else (group, None)
            gr = np.ascontiguousarray(np.asarray(gr, np.int32).reshape(-1))
            ng = (int(gr.max(initial=-1)) + 1) if ng is None else int(ng)
        with self._scan_lock:
            if x is None or st is None:
                r_rows, r_nm, r_n = self.mel_resident()
                rows, nm = (r_rows, r_nm) if x is None else (rows, nm)
                n = r_n if st is None else n
            if gr is not None and gr.size != n:
                raise AudioProcessingError(f"Model prediction failed: group has an entry per segment, got {gr.size} for {n}")
            nout = n if gr is None else ng
            out = {"max": np.empty(nout, np.float32)}
            if moments:
                out["sum"], out["sumsq"] = np.empty((nout, nm), np.int64), np.empty((nout, nm), np.uint64)
            outs = (out["max"].ctypes.data_as(C.POINTER(C.c_float)), out["sum"].ctypes.data_as(C.POINTER(C.c_int64)) if moments else None,
                    out["sumsq"].ctypes.data_as(C.POINTER(C.c_uint64)) if moments else None)
            if gr is None:
                self._check(self._lib.vad_mel_stats(self._h, xp, rows, nm, sp, n, *outs))
            else:
                gp = (gr if gr.size else np.zeros(1, np.int32)).ctypes.data_as(C.POINTER(C.c_int32))
                self._check(self._lib.vad_mel_stats_grouped(self._h, xp, rows, nm, sp, n, gp, ng, *outs))
        return out

    @staticmethod
    def _batch_record(batch, n_mels: int) -> _ffi.Batch:
        """``batch``: a ``_ffi.Batch``, an object with ``record(n_mels)`` (``cutter_vad_amd.scan.FeatureBatch``) or a dict of
        ``vad_batch``'s fields - ``frames``, and optionally ``n_mels``, ``deltas``, ``layout`` / ``dtype`` / ``pad`` (names or numbers),
        ``pad_value``"""
        if isinstance(batch, _ffi.Batch):
            return batch
        f = dict(batch.record(n_mels) if hasattr(batch, "record") else batch)
        enum = lambda table, what, v: Engine._cut_enum(table, what, v) if isinstance(v, str) else int(v)
        return _ffi.Batch(int(f.get("n_mels", n_mels)), int(f["frames"]), int(f.get("deltas", 0)),
                          enum(_ffi.BATCH_LAYOUTS, "layout", f.get("layout", "channel")), enum(_ffi.BATCH_DTYPES, "dtype", f.get("dtype", "f32")),
                          enum(_ffi.BATCH_PADS, "pad", f.get("pad", "value")), float(f.get("pad_value", 0.0)), 0)

    @staticmethod
    def _batch_table(records, dtype, ctype):
        """the windows (``_ffi.BATCH_WINDOW_DTYPE``, ``_ffi.BatchWindow``) or the pieces of a batch -> (the flat array, its pointer)"""
        t = np.ascontiguousarray(np.asarray(records, dtype).reshape(-1)) if not (
            isinstance(records, np.ndarray) and records.dtype == dtype) else np.ascontiguousarray(records.reshape(-1))
        return t, (t if t.size else np.zeros(1, dtype)).ctypes.data_as(C.POINTER(ctype))

    @staticmethod
    def _batch_affine(lo, shift, scale, n_mels: int):
        """-> (lo, shift, scale as float32 arrays or None, their pointers, nss)"""
        f32p = C.POINTER(C.c_float)
        lo = None if lo is None else np.ascontiguousarray(np.asarray(lo, np.float32).reshape(-1))
        two = []
        for a in (shift, scale):
            a = None if a is None else np.asarray(a, np.float32)
            if a is not None:
                a = np.full((1, n_mels), a, np.float32) if a.ndim == 0 else np.ascontiguousarray(a.reshape(1, -1) if a.ndim < 2 else a)
                if a.ndim != 2 or a.shape[1] != n_mels:
                    raise AudioProcessingError(f"Model prediction failed: shift and scale are [1 or n, n_mels = {n_mels}], got {a.shape}")
            two.append(a)
        rows = {a.shape[0] for a in two if a is not None}
        if len(rows) > 1:
            raise AudioProcessingError(f"Model prediction failed: shift and scale have the same number of rows, got {sorted(rows)}")
        ptr = lambda a: None if a is None else a.ctypes.data_as(f32p)
        return (lo, *two), (ptr(lo), ptr(two[0]), ptr(two[1])), (rows.pop() if rows else 1)

    def _batch_plan(self, batch, n_mels: int, records, dtype, ctype, nw, lo, shift, scale):
        """What the four batch methods share, in the order they raise: the ``vad_batch`` record, the table of windows or pieces, the
        affine arrays (held by the caller until its call returns), the batch's shape for ``nw`` windows (``None``: one per record)
        and its numpy dtype.  -> (record, table, its pointer, affine arrays, their pointers with nss, shape, dtype)"""
        b = self._batch_record(batch, n_mels)
        t, tp = self._batch_table(records, dtype, ctype)
        own, ptrs, nss = self._batch_affine(lo, shift, scale, b.n_mels)
        nw, chans = t.size if nw is None else int(nw), b.n_mels * (b.deltas + 1)
        shape = (nw, chans, b.frames) if b.layout == _ffi.VAD_BATCH_CHANNEL_MAJOR else (nw, b.frames, chans)
        return b, t, tp, own, (*ptrs, nss), shape, {_ffi.VAD_BATCH_F32: np.float32, _ffi.VAD_BATCH_F16: np.float16}.get(b.dtype, np.uint16)

    def mel_batch(self, windows, batch, lo=None, shift=None, scale=None, features=None, start=None) -> np.ndarray:
        """Normalised, padded windows of a feature matrix in a model's layout and number format (``vad_mel_batch``), one launch:
        ``windows`` lists ``(seg, nrows, row0)`` - rows ``row0 .. row0 + nrows - 1`` of segment ``seg``
        (``cutter_vad_amd.scan.batch_windows``) - ``batch`` is a ``cutter_vad_amd.scan.FeatureBatch`` with ``frames`` set, or a dict of
        ``vad_batch``'s fields.  A value is ``(max(x, lo[seg]) + shift[seg]) * scale[seg]`` in float32 (``lo`` [n] or ``None`` for
        -inf; ``shift`` / ``scale`` [n_mels], [1, n_mels] or [n, n_mels], ``None`` for 0 and 1), ``deltas`` appends first and second
        differences over the SEGMENT's rows, frames past ``nrows`` are pad cells (``include/vad_engine.h`` has the rule).
        ``features`` / ``start`` as in ``mel_stats``; ``None``: the resident matrix.  -> [B, C, T] (``layout="channel"``) or [B, T, C]
        with C = n_mels * (deltas + 1): float32, ``np.float16``, or the bfloat16 bit patterns as ``np.uint16``."""
        x, xp, rows, nm, st, sp, n = self._batch_source(features, start)
        with self._scan_lock:
            if x is None:
                nm = self.mel_resident()[1]
            b, w, wp, _own, affine, shape, dtype = self._batch_plan(batch, nm, windows, _ffi.BATCH_WINDOW_DTYPE, _ffi.BatchWindow, None, lo, shift, scale)
            out = np.empty(shape, dtype)
            self._check(self._lib.vad_mel_batch(self._h, xp, rows, sp, n, C.byref(b), wp, w.size, *affine, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def mel_batch_device(self, windows, batch, d_out: int, out_bytes: int, lo=None, shift=None, scale=None, d_features: int = 0, rows: int = 0,
                         n_mels: int = 0, start=None, stream: int = 0) -> Tuple[int, ...]:
        """``mel_batch`` into device memory (``vad_mel_batch_device``): the windows to ``d_out`` (an integer; 16-byte aligned, room for
        ``out_bytes``), where a model on the same GPU reads them - nothing crosses the link.  ``d_features`` = 0: the resident matrix,
        else a float32 matrix [rows, n_mels] on the GPU.  ``windows``, ``lo``, ``shift``, ``scale`` and ``start`` are host arrays, read
        before the call returns.  Asynchronous on ``stream``.  -> the shape of the batch."""
        _st, sp, n = self._batch_start(start)
        with self._scan_lock:
            nm = int(n_mels) if d_features else self.mel_resident()[1]
            b, w, wp, _own, affine, shape, _ = self._batch_plan(batch, nm, windows, _ffi.BATCH_WINDOW_DTYPE, _ffi.BatchWindow, None, lo, shift, scale)
            self._check(self._lib.vad_mel_batch_device(self._h, d_features or None, int(rows), sp, n, C.byref(b), wp, w.size, *affine, d_out or None,
                                                       int(out_bytes), stream or None))
        return shape

    def mel_batch_packed(self, pieces, nw: int, batch, lo=None, shift=None, scale=None, features=None, start=None) -> np.ndarray:
        """``mel_batch`` with several pieces of segments per window (``vad_mel_batch_packed``), one launch: ``pieces`` lists ``(seg,
        nrows, row0, window, offset)`` - rows ``row0 .. row0 + nrows - 1`` of segment ``seg`` at frames ``offset ..`` of window
        ``window`` (``cutter_vad_amd.scan.batch_pack`` places them) - in ``nw`` windows.  ``lo`` [nw], ``shift`` / ``scale`` [n_mels],
        [1, n_mels] or [nw, n_mels] are indexed by WINDOW; the differences of ``deltas`` run over the SEGMENT's rows; every frame no
        piece covers is a pad cell (``include/vad_engine.h`` has the rule).  The other arguments and the result as in ``mel_batch``,
        B = ``nw``."""
        x, xp, rows, nm, st, sp, n = self._batch_source(features, start)
        with self._scan_lock:
            if x is None:
                nm = self.mel_resident()[1]
            b, p, pp, _own, affine, shape, dtype = self._batch_plan(batch, nm, pieces, _ffi.BATCH_PIECE_DTYPE, _ffi.BatchPiece, nw, lo, shift, scale)
            out = np.empty(shape, dtype)
            self._check(self._lib.vad_mel_batch_packed(self._h, xp, rows, sp, n, C.byref(b), pp, p.size, int(nw), *affine,
                                                       out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def mel_batch_packed_device(self, pieces, nw: int, batch, d_out: int, out_bytes: int, lo=None, shift=None, scale=None, d_features: int = 0,
                                rows: int = 0, n_mels: int = 0, start=None, stream: int = 0) -> Tuple[int, ...]:
        """``mel_batch_packed`` into device memory (``vad_mel_batch_packed_device``); the arguments as in ``mel_batch_device``.
        Asynchronous on ``stream``.  -> the shape of the batch."""
        _st, sp, n = self._batch_start(start)
        with self._scan_lock:
            nm = int(n_mels) if d_features else self.mel_resident()[1]
            b, p, pp, _own, affine, shape, _ = self._batch_plan(batch, nm, pieces, _ffi.BATCH_PIECE_DTYPE, _ffi.BatchPiece, nw, lo, shift, scale)
            self._check(self._lib.vad_mel_batch_packed_device(self._h, d_features or None, int(rows), sp, n, C.byref(b), pp, p.size, int(nw), *affine,
                                                              d_out or None, int(out_bytes), stream or None))
        return shape

    # ------------------------------------------------------------------ rendered audio
    @staticmethod
    def _render_ramp(ramp) -> np.ndarray:
        return np.zeros(0, np.float32) if ramp is None else np.ascontiguousarray(np.asarray(ramp, np.float32).reshape(-1))

    def render(self, segments, out_start, out_samples: int, hop: Optional[int] = None, ramp=None, gains=None, denoise: Optional[float] = 0.01,
               out="pcm16", audio=None, law: Optional[str] = None, i16_scale: int = 32767, sample_rate: Optional[int] = None) -> np.ndarray:
        """One finished piece of audio (``vad_scan_render``): the sample range of segment i - ``segments`` as in ``cut`` - goes to
        ``out_start[i]`` (a multiple of 4) of an output of ``out_samples`` samples (a multiple of 4), faded by ``ramp`` - a float32
        table, ``cutter_vad_amd.scan.fade_ramp`` makes the usual ones - read forwards from the segment's first sample and from its
        last; where TWO segments share output samples their faded samples are added (a crossfade; three are refused), and every
        sample no segment covers is zero.  ``gains`` as in ``cut``; ``out="pcm16"`` / ``"f32"`` as there.  -> the ``out_samples``
        samples.  A sample of a segment is what ``cut(layout="range", out="f32", gains=gains)`` gives, times the two ramp entries,
        each a float32 multiply.  ``audio``, ``law``, ``i16_scale``, ``sample_rate`` and the ``scan_session()`` rule as in ``cut``;
        on a block at another rate the samples are input-rate samples and never gated."""
        of = self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        r = self._render_ramp(ramp)
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("render", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, channels, out_samples=out_start, rate=sr)
            n = len(start) - 1
            data = np.empty(max(int(out_samples), 0), np.int16 if of == _ffi.VAD_CUT_PCM16 else np.float32)
            thr = -1.0 if denoise is None else float(denoise)
            g = None if gains is None else self._cut_gains(gains, n)
            self._check(self._lib.vad_scan_render(self._h, items, n, None if g is None else _ptr(g, C.c_float),
                                                  _ptr(r, C.c_float) if r.size else None, r.size, ptr, total, channels, fmt, sr or 0, hop, thr,
                                                  of, data.ctypes.data_as(C.c_void_p), int(out_samples)))
        return data

    def render_device(self, segments, out_start, d_audio: int, audio_samples: int, d_out: int, out_samples: int, hop: Optional[int] = None,
                      ramp=None, gains=None, fmt: int = _ffi.VAD_FMT_F32, channels: int = 1, denoise: Optional[float] = 0.01, out="pcm16",
                      stream: int = 0, sample_rate: Optional[int] = None) -> None:
        """``render`` on device pointers (integers; ``vad_scan_render_device``): the block at ``d_audio`` as ``cut_device`` takes it,
        all ``out_samples`` samples to ``d_out`` (16-byte aligned) - no memset by the caller.  ``ramp`` and ``gains`` are host
        arrays, read before the call returns.  Asynchronous on ``stream``."""
        of = self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        r = self._render_ramp(ramp)
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._cut_items(segments, hop, _ffi.VAD_CUT_RANGE, int(channels), out_start, rate=sr)
        n = len(start) - 1
        thr = -1.0 if denoise is None else float(denoise)
        g = None if gains is None else self._cut_gains(gains, n)
        self._check(self._lib.vad_scan_render_device(self._h, items, n, None if g is None else _ptr(g, C.c_float),
                                                     _ptr(r, C.c_float) if r.size else None, r.size, d_audio or None, int(audio_samples),
                                                     int(channels), int(fmt), sr or 0, hop, thr, of, d_out or None, int(out_samples),
                                                     stream or None))

    # ------------------------------------------------------------------ two-channel segment audio
    def _stereo_items(self, segments, hop: int, layout: int, out_samples=None, rate: Optional[int] = None):
        """``_cut_items`` for the stereo calls: a segment is (sample_offset, first_frame, nframes) - no channel, both are written -
        and positions count sample frames"""
        segs = [tuple(sg) for sg in segments]
        for sg in segs:
            if len(sg) != 3:
                raise AudioProcessingError(f"Model prediction failed: a segment of a stereo cut is (sample_offset, first_frame, nframes): "
                                           f"both channels are written, got {sg!r}")
        items, start = self._cut_items(segs, hop, layout, 2, out_samples, rate=rate)
        for i in range(len(segs)):
            items[i].channel = _ffi.VAD_SCAN_BOTH
        return items, start

    def cut_stereo(self, segments, hop: Optional[int] = None, law: Optional[str] = None, i16_scale: int = 32767,
                   denoise: Optional[float] = 0.01, layout="frames", out="pcm16", audio=None, sample_rate: Optional[int] = None, gains=None):
        """``cut`` of a two-channel block with BOTH channels kept (``vad_scan_cut_stereo``): ``segments`` lists
        ``(sample_offset, first_frame, nframes)`` - a fourth element is refused.  -> (data, start): ``data`` is ``[frames, 2]``,
        segment i = ``data[start[i]:start[i + 1]]``; ``start`` counts sample frames.  ``data[:, c]`` is bit for bit what ``cut`` with
        the same arguments gives for segments that name channel ``c``; the gate acts per value.  Every other argument as in ``cut``;
        ``layout="frames"`` with a ``sample_rate`` other than the engine's is not supported (``"range"`` is)."""
        lay, of = self._cut_enum(_ffi.CUT_LAYOUTS, "layout", layout), self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("cut_stereo", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._stereo_items(segments, hop, lay, rate=sr)
            n = len(start) - 1
            data = np.empty((int(start[-1]), 2), np.int16 if of == _ffi.VAD_CUT_PCM16 else np.float32)
            thr = -1.0 if denoise is None else float(denoise)
            g = None if gains is None else self._cut_gains(gains, n)
            self._check(self._lib.vad_scan_cut_stereo(self._h, items, n, None if g is None else _ptr(g, C.c_float), ptr, total, channels, fmt,
                                                      sr or 0, hop, thr, lay, of, data.ctypes.data_as(C.c_void_p), data.shape[0]))
        return data, start

    def cut_stereo_device(self, segments, d_audio: int, audio_samples: int, d_out: int, out_samples: int, hop: Optional[int] = None,
                          fmt: int = _ffi.VAD_FMT_F32, channels: int = 2, denoise: Optional[float] = 0.01, layout="frames", out="pcm16",
                          stream: int = 0, out_start=None, sample_rate: Optional[int] = None, gains=None) -> np.ndarray:
        """``cut_stereo`` on device pointers (integers; ``vad_scan_cut_stereo_device``): the two-channel block at ``d_audio`` (8-byte
        aligned), the payloads to ``d_out`` (16-byte aligned, room for ``out_samples`` sample frames = ``2 * out_samples`` values),
        packed in the order listed or at sample frame ``out_start[i]`` (multiples of 4).  Asynchronous on ``stream``.
        -> start [n + 1] of the packed order, in sample frames."""
        lay, of = self._cut_enum(_ffi.CUT_LAYOUTS, "layout", layout), self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._stereo_items(segments, hop, lay, out_start, rate=sr)
        thr = -1.0 if denoise is None else float(denoise)
        n = len(start) - 1
        g = None if gains is None else self._cut_gains(gains, n)
        self._check(self._lib.vad_scan_cut_stereo_device(self._h, items, n, None if g is None else _ptr(g, C.c_float), d_audio or None,
                                                         int(audio_samples), int(channels), int(fmt), sr or 0, hop, thr, lay, of,
                                                         d_out or None, int(out_samples), stream or None))
        return start

    def render_stereo(self, segments, out_start, out_samples: int, hop: Optional[int] = None, ramp=None, gains=None,
                      denoise: Optional[float] = 0.01, out="pcm16", audio=None, law: Optional[str] = None, i16_scale: int = 32767,
                      sample_rate: Optional[int] = None) -> np.ndarray:
        """``render`` of a two-channel block with BOTH channels kept (``vad_scan_render_stereo``): ``segments`` as in ``cut_stereo``,
        ``out_start`` and ``out_samples`` in sample frames.  -> ``[out_samples, 2]``; column ``c`` is bit for bit what ``render``
        gives when every segment names channel ``c`` - gain and ramp are the same for both channels of a sample frame."""
        of = self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        r = self._render_ramp(ramp)
        with self._scan_lock:
            sr, total, channels, fmt, ptr, _keep = self._cut_block("render_stereo", audio, law, i16_scale, sample_rate)
            hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
            items, start = self._stereo_items(segments, hop, _ffi.VAD_CUT_RANGE, out_start, rate=sr)
            n = len(start) - 1
            data = np.empty((max(int(out_samples), 0), 2), np.int16 if of == _ffi.VAD_CUT_PCM16 else np.float32)
            thr = -1.0 if denoise is None else float(denoise)
            g = None if gains is None else self._cut_gains(gains, n)
            self._check(self._lib.vad_scan_render_stereo(self._h, items, n, None if g is None else _ptr(g, C.c_float),
                                                         _ptr(r, C.c_float) if r.size else None, r.size, ptr, total, channels, fmt, sr or 0,
                                                         hop, thr, of, data.ctypes.data_as(C.c_void_p), int(out_samples)))
        return data

    def render_stereo_device(self, segments, out_start, d_audio: int, audio_samples: int, d_out: int, out_samples: int,
                             hop: Optional[int] = None, ramp=None, gains=None, fmt: int = _ffi.VAD_FMT_F32, channels: int = 2,
                             denoise: Optional[float] = 0.01, out="pcm16", stream: int = 0, sample_rate: Optional[int] = None) -> None:
        """``render_stereo`` on device pointers (integers; ``vad_scan_render_stereo_device``): the two-channel block at ``d_audio``,
        all ``out_samples`` sample frames (``2 * out_samples`` values) to ``d_out`` (16-byte aligned).  Asynchronous on ``stream``."""
        of = self._cut_enum(_ffi.CUT_OUTPUTS, "out", out)
        r = self._render_ramp(ramp)
        sr = self._scan_rate(sample_rate)
        hop = self.scan_chunk_samples(sr) // 2 if hop is None else int(hop)
        items, start = self._stereo_items(segments, hop, _ffi.VAD_CUT_RANGE, out_start, rate=sr)
        n = len(start) - 1
        thr = -1.0 if denoise is None else float(denoise)
        g = None if gains is None else self._cut_gains(gains, n)
        self._check(self._lib.vad_scan_render_stereo_device(self._h, items, n, None if g is None else _ptr(g, C.c_float),
                                                            _ptr(r, C.c_float) if r.size else None, r.size, d_audio or None,
                                                            int(audio_samples), int(channels), int(fmt), sr or 0, hop, thr, of,
                                                            d_out or None, int(out_samples), stream or None))

    # ------------------------------------------------------------------ tick assembler (shared-pool serving)
    def tick_push(self, slot: int, frame, gate_on: bool = True, i16_scale: int = 32767, sample_rate: Optional[int] = None,
                  law: Optional[str] = None) -> None:
        """Queue one frame for ``slot`` (``vad_tick_push``): ``bytes`` = little-endian int16 PCM as it came off the wire,
        or a float32 array.  Written straight into the coming tick's page-locked staging; padded / truncated to the
        model's frame length.  ``sample_rate`` other than the engine's (8000 / 24000 / 48000 on a 16 kHz engine): the chunk
        that yields one frame, resampled on the GPU inside the tick (``vad_tick_push_rate``)."""
        i16_fmt = _ffi.VAD_FMT_I16_32768 if i16_scale == 32768 else _ffi.VAD_FMT_I16_32767
        g711 = _law_format(law, frame)
        if g711 is not None:                          # G.711 codes (bytes or uint8): decoded on push, staged as int16 / 32768
            buf = frame if isinstance(frame, bytes) else np.ascontiguousarray(frame).tobytes() if isinstance(frame, np.ndarray) else bytes(frame)
            count, fmt = len(buf), g711
        elif isinstance(frame, (bytes, bytearray, memoryview)):
            buf, count, fmt = bytes(frame), len(frame) // 2, i16_fmt
        else:
            f = np.ascontiguousarray(frame)
            fmt = i16_fmt
            if f.dtype != np.int16:
                f = np.ascontiguousarray(f, np.float32)
                fmt = _ffi.VAD_FMT_F32
            buf, count = f.ctypes.data_as(C.c_void_p), f.size
        if sample_rate is None or int(sample_rate) == self.sample_rate:
            self._check(self._lib.vad_tick_push(self._h, int(slot), buf, count, fmt, int(gate_on)))
        else:
            self._check(self._lib.vad_tick_push_rate(self._h, int(slot), buf, count, fmt, int(gate_on), int(sample_rate)))

    def tick_push_many(self, slots, frames, gate_on: bool = True, i16_scale: int = 32767, law: Optional[str] = None) -> None:
        """frames [n, L] (float32 or int16; uint8 G.711 codes with ``law``), one per listed slot (``vad_tick_push_many``)."""
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        f = np.ascontiguousarray(frames)
        g711 = _law_format(law, f)
        if g711 is not None:
            fmt = g711
        elif f.dtype == np.int16:
            fmt = _ffi.VAD_FMT_I16_32768 if i16_scale == 32768 else _ffi.VAD_FMT_I16_32767
        else:
            f = np.ascontiguousarray(f, np.float32)
            fmt = _ffi.VAD_FMT_F32
        if f.ndim != 2 or f.shape[0] != s.size:
            raise AudioProcessingError(f"Model prediction failed: frames have shape {f.shape}, expected ({s.size}, L)")
        self._check(self._lib.vad_tick_push_many(self._h, _ptr(s, C.c_int64), s.size, f.ctypes.data_as(C.c_void_p), f.shape[1],
                                                 fmt, int(gate_on)))

    def tick_enable_segments(self, on: bool = True) -> None:
        self._check(self._lib.vad_tick_enable_segments(self._h, int(on)), VADError)

    def tick_take_segment(self, slot: int) -> np.ndarray:
        """The finished segment of ``slot`` as float32 samples (``vad_tick_take_segment``); empty if there is none."""
        n = C.c_int64()
        self._check(self._lib.vad_tick_take_segment(self._h, int(slot), None, 0, C.byref(n)), VADError)
        out = np.empty(int(n.value), np.float32)
        self._check(self._lib.vad_tick_take_segment(self._h, int(slot), _ptr(out, C.c_float), out.size, C.byref(n)), VADError)
        return out

    def tick_push_status(self, slots, frames, nsamples: int, gate_on: bool = True, i16_scale: int = 32767,
                         law: Optional[str] = None) -> np.ndarray:
        """``frames``: int16 / float32 array [n, nsamples] or the same as one bytes object of int16 PCM; every frame is tried,
        -> int32 status per frame (``vad_tick_push_status``; 0 = queued)."""
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        g711 = _law_format(law, frames)
        if g711 is not None:                          # G.711 codes: bytes or a uint8 array, nsamples bytes per frame
            f = np.ascontiguousarray(np.frombuffer(frames, np.uint8) if isinstance(frames, (bytes, bytearray, memoryview)) else frames)
            if f.size != int(nsamples) * s.size:
                raise AudioProcessingError(f"Model prediction failed: {f.size} bytes for {s.size} G.711 frames of {nsamples} samples")
            buf, ptr, fmt = f, f.ctypes.data_as(C.c_void_p), g711
        elif isinstance(frames, (bytes, bytearray, memoryview)):
            buf, fmt = frames, (_ffi.VAD_FMT_I16_32768 if i16_scale == 32768 else _ffi.VAD_FMT_I16_32767)
            if len(frames) != 2 * int(nsamples) * s.size:
                raise AudioProcessingError(f"Model prediction failed: {len(frames)} bytes for {s.size} int16 frames of {nsamples} samples")
            ptr = C.cast(C.c_char_p(bytes(frames) if not isinstance(frames, bytes) else frames), C.c_void_p)
        else:
            f = np.ascontiguousarray(frames)
            if f.dtype == np.int16:
                fmt = _ffi.VAD_FMT_I16_32768 if i16_scale == 32768 else _ffi.VAD_FMT_I16_32767
            else:
                f, fmt = np.ascontiguousarray(f, np.float32), _ffi.VAD_FMT_F32
            if f.size != int(nsamples) * s.size:
                raise AudioProcessingError(f"Model prediction failed: frames {f.shape} for {s.size} slots of {nsamples} samples")
            buf, ptr = f, f.ctypes.data_as(C.c_void_p)
        status = np.zeros(s.size, np.int32)
        self._lib.vad_tick_push_status(self._h, _ptr(s, C.c_int64), s.size, ptr, int(nsamples), fmt, int(gate_on), _ptr(status, C.c_int32))
        del buf
        return status

    def tick_push_gather(self, slots, frames, nsamples: int, gate_on: bool = True, i16_scale: int = 32767,
                         law: Optional[str] = None) -> np.ndarray:
        """``frames``: a sequence of ``bytes`` objects (int16 PCM, ``nsamples`` samples each), one per listed slot; they are
        copied from where they are into the tick's staging (``vad_tick_push_gather``) -> int32 status per frame."""
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        n = s.size
        if len(frames) != n:
            raise AudioProcessingError(f"Model prediction failed: {len(frames)} frames for {n} slots")
        ptrs = (C.c_char_p * n)(*frames)               # borrows the bytes objects' buffers: `frames` stays alive through the call
        status = np.zeros(n, np.int32)
        fmt = _ffi.VAD_FMT_I16_32768 if i16_scale == 32768 else _ffi.VAD_FMT_I16_32767
        fmt = _law_format(law) or fmt                  # G.711: ``frames`` hold nsamples one-byte codes each
        self._lib.vad_tick_push_gather(self._h, _ptr(s, C.c_int64), n, ptrs, int(nsamples), fmt, int(gate_on), _ptr(status, C.c_int32))
        return status

    def tick_push_rate_gather(self, slots, frames, sample_rate: int, gate_on: bool = True, i16_scale: int = 32767,
                              law: Optional[str] = None) -> np.ndarray:
        """``frames``: a sequence of ``bytes`` objects, one int16 chunk of ``512 * sample_rate / 16000`` samples per listed slot, all
        at ONE input rate (``vad_tick_push_rate_gather``) -> int32 status per chunk."""
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        n = s.size
        if len(frames) != n:
            raise AudioProcessingError(f"Model prediction failed: {len(frames)} frames for {n} slots")
        g711 = _law_format(law)
        width = 1 if g711 is not None else 2           # bytes per sample on the wire
        nsamples = len(frames[0]) // width if n else 0
        if any(len(f) != width * nsamples for f in frames):
            raise AudioProcessingError("Model prediction failed: chunks of one call must have one length")
        ptrs = (C.c_char_p * n)(*frames)
        status = np.zeros(n, np.int32)
        fmt = g711 or (_ffi.VAD_FMT_I16_32768 if i16_scale == 32768 else _ffi.VAD_FMT_I16_32767)
        self._lib.vad_tick_push_rate_gather(self._h, _ptr(s, C.c_int64), n, ptrs, int(nsamples), fmt, int(gate_on), int(sample_rate),
                                            _ptr(status, C.c_int32))
        return status

    def tick_gather_entry(self):
        """(address of ``vad_tick_push_gather``, address of this engine, address of ``vad_tick_push_rate_gather``) for callers
        that push from C (server/_wirebox)."""
        if not self._h:
            raise VADError("engine is closed")
        return self._gather_fn, int(self._h.value), self._rate_gather_fn

    def tick_cancel(self, slot: int) -> None:
        self._check(self._lib.vad_tick_cancel(self._h, int(slot)), VADError)

    def tick_pending(self, slot: int) -> int:
        """frames of ``slot`` that have been pushed and not stepped yet (``vad_tick_pending``)"""
        k = C.c_int64()
        self._check(self._lib.vad_tick_pending(self._h, int(slot), C.byref(k)), VADError)
        return int(k.value)

    def save_segment(self, slot: int) -> bytes:
        """the slot's segment audio (pre-roll, open segment, finished one not yet taken) as an opaque blob
        (``vad_tick_segment_save``): with ``save_stream`` everything a session needs to continue on another engine"""
        k = C.c_int64()
        self._check(self._lib.vad_tick_segment_save(self._h, int(slot), None, 0, C.byref(k)), VADError)
        buf = C.create_string_buffer(int(k.value))
        self._check(self._lib.vad_tick_segment_save(self._h, int(slot), buf, int(k.value), C.byref(k)), VADError)
        return buf.raw[:int(k.value)]

    def restore_segment(self, slot: int, blob: bytes) -> None:
        self._check(self._lib.vad_tick_segment_restore(self._h, int(slot), blob, len(blob)), VADError)

    def tick_run(self, denoise: float = 0.01):
        """Advance every slot with a pending frame by one frame (``vad_tick_run``) ->
        ``(slots, probs, events, seg_frames, group_start, frames, nsamples)``: arrays over the stepped streams (views of
        engine-owned page-locked memory, valid until the next ``tick_run``), ``group_start`` [13], ``frames[g]`` = the staged
        audio of group g as an array [count, frame] or None - g = fmt * 2 + gate_on for g < 6 (float32 for g < 2, int16
        above), g = 6 + 3 * gate_on + {0: 8 kHz, 1: 24 kHz, 2: 48 kHz} for chunks at another rate (float32 [count, 256 / 768 /
        1536]) - and ``nsamples`` = the length each frame had when it was pushed."""
        r = _ffi.TickResult()
        r.struct_size = C.sizeof(_ffi.TickResult)
        rc = self._lib.vad_tick_run(self._h, float(denoise), C.byref(r))
        return self._tick_arrays(r, rc)

    def _tick_arrays(self, r, rc):
        self.last_tick_dropped = int(r.dropped)   # frames left out because their stream was closed after the push
        self.last_tick_staged_next = int(r.staged_next)   # frames that were waiting and are already staged for the next tick
        # a failed tick has consumed its frames: which streams lost one, and how long those frames were (TickFailure below)
        self.last_tick_lost = None
        if rc != _ffi.VAD_OK:
            if int(r.n) and r.slots and r.nsamples:
                self.last_tick_lost = (np.ctypeslib.as_array(r.slots, (int(r.n),)).copy(), np.ctypeslib.as_array(r.nsamples, (int(r.n),)).copy())
            self._check(rc)
        n = int(r.n)
        self.last_tick_us = tuple(r.host_us)       # (swap, copies + launches + wait, segment assembly) of this tick
        gs = np.array(list(r.group_start), np.int64)
        if n == 0:
            e = np.empty(0)
            return (e.astype(np.int64), e.astype(np.float32), e.astype(np.uint8), e.astype(np.int32), gs, [None] * TICK_GROUPS,
                    e.astype(np.int32))
        as_arr = np.ctypeslib.as_array
        slots, probs = as_arr(r.slots, (n,)), as_arr(r.probs, (n,))
        events, seg = as_arr(r.events, (n,)), as_arr(r.seg_frames, (n,))
        frames = []
        for g in range(TICK_GROUPS):
            cnt = int(gs[g + 1] - gs[g])
            if cnt == 0 or not r.group_frames[g]:
                frames.append(None)
                continue
            ct = C.c_int16 if 2 <= g < 6 else C.c_float
            flen = self.frame_samples if g < 6 else TICK_RATE_CHUNK[(g - 6) % 3]
            frames.append(as_arr(C.cast(r.group_frames[g], C.POINTER(ct)), (cnt, flen)))
        return slots, probs, events, seg, gs, frames, as_arr(r.nsamples, (n,))

    def tick_run_work(self, denoise: float, last_prob: np.ndarray, frames_done: np.ndarray, active: np.ndarray,
                      continue_cb: np.ndarray, continue_payload: np.ndarray):
        """``tick_run`` + the per-session bookkeeping of a serving front end in the same C call (``vad_tick_run_work``): the five
        per-slot arrays (float32, int64, bool, bool, bool; the caller's, updated in place) and ->
        ``(slots, group_start, frames, nsamples, work_index, work_kind, work_samples)``: ``work_index[j]`` = the entry of the tick's
        arrays the caller has something to do for, ``work_kind[j]`` = VAD_WORK_* bits (START, END, CONTINUE, PAYLOAD, LONG),
        ``work_samples[j]`` = the finished segment's length for END entries."""
        r, w = self.tick_work_begin(last_prob, frames_done, active, continue_cb, continue_payload)
        return self.tick_work_end(r, w, self._lib.vad_tick_run_work(self._h, float(denoise), C.byref(r), C.byref(w)))

    def tick_work_begin(self, last_prob: np.ndarray, frames_done: np.ndarray, active: np.ndarray, continue_cb: np.ndarray,
                        continue_payload: np.ndarray):
        """The two structs of a ``vad_tick_run_work`` call, inputs filled in - for callers that make the call themselves
        (``_wirebox.tick_shards``: several engines' ticks side by side); ``tick_work_end`` turns them into arrays afterwards."""
        r = _ffi.TickResult()
        r.struct_size = C.sizeof(_ffi.TickResult)
        w = _ffi.TickWork()
        w.struct_size = C.sizeof(_ffi.TickWork)
        w.n_slots = int(last_prob.size)
        assert frames_done.size == w.n_slots and active.size == w.n_slots and continue_cb.size == w.n_slots and continue_payload.size == w.n_slots
        w.last_prob = _ptr(last_prob, C.c_float)
        w.frames_done = _ptr(frames_done, C.c_int64)
        w.active = active.ctypes.data_as(C.POINTER(C.c_uint8))
        w.continue_cb = continue_cb.ctypes.data_as(C.POINTER(C.c_uint8))
        w.continue_payload = continue_payload.ctypes.data_as(C.POINTER(C.c_uint8))
        return r, w

    def tick_work_end(self, r, w, rc: int):
        slots, _p, _ev, _seg, gs, frames, nsamp = self._tick_arrays(r, rc)
        nw = int(w.n_work)
        if nw == 0:
            return slots, gs, frames, nsamp, np.empty(0, np.int32), np.empty(0, np.uint8), np.empty(0, np.int64)
        as_arr = np.ctypeslib.as_array
        return slots, gs, frames, nsamp, as_arr(w.work_index, (nw,)), as_arr(w.work_kind, (nw,)), as_arr(w.work_samples, (nw,))

    def tick_work_entry(self) -> int:
        """address of ``vad_tick_run_work``"""
        return C.cast(self._lib.vad_tick_run_work, C.c_void_p).value

    def tick_wav_entry(self):
        """(address of ``vad_tick_take_segment_wav16``, address of this engine) for callers that take segments from C
        (``_wirebox.take_wav16``: the payload is written straight into the bytes object)."""
        if not self._h:
            raise VADError("engine is closed")
        return C.cast(self._lib.vad_tick_take_segment_wav16, C.c_void_p).value, int(self._h.value)

    def tick_take_segment_wav16(self, slot: int, sample_rate: int) -> bytes:
        """The finished segment of ``slot`` as the ``voice_end_callback`` payload: RIFF/WAVE header + int16 PCM, built in the
        engine (``vad_tick_take_segment_wav16``), byte for byte ``WAVWriter(sample_rate, 16, 1).write_wav_data`` of it."""
        n = C.c_int64()
        self._check(self._lib.vad_tick_take_segment_wav16(self._h, int(slot), int(sample_rate), None, 0, C.byref(n)), VADError)
        buf = bytearray(int(n.value))
        self._check(self._lib.vad_tick_take_segment_wav16(self._h, int(slot), int(sample_rate),
                                                          (C.c_char * len(buf)).from_buffer(buf), len(buf), C.byref(n)), VADError)
        return bytes(buf)

    # ------------------------------------------------------------------ pipelined host ingest
    def submit(self, slots, frames, denoise: Optional[float] = 0.01, i16_scale: int = 32767, law: Optional[str] = None) -> int:
        """Enqueue copy-in -> step -> copy-out for ``frames`` [n, frame] or [n, T, frame] and return a ticket
        (``vad_step_submit``).  ``slots`` / ``frames`` must stay alive and unchanged until ``collect(ticket)``; frames in a
        ``pinned_array`` are DMA'd asynchronously, so the copy of this ticket overlaps the kernel of the previous one."""
        f0 = np.asarray(frames)
        T = int(f0.shape[1]) if f0.ndim == 3 else 1
        s, f, fmt = self._prep(slots, f0, T if f0.ndim == 3 else None, law)
        if fmt == _ffi.VAD_FMT_I16_32767 and i16_scale == 32768:
            fmt = _ffi.VAD_FMT_I16_32768
        thr = -1.0 if denoise is None else float(denoise)
        t = C.c_int64()
        self._check(self._lib.vad_step_submit(self._h, _ptr(s, C.c_int64), s.size, T, f.ctypes.data_as(C.c_void_p), fmt, thr,
                                              C.byref(t)))
        self._tickets[int(t.value)] = (s, f, T, f0.ndim == 3)      # keeps the buffers alive until collected
        return int(t.value)

    def collect(self, ticket: int):
        """-> (probs, events, seg_frames) of a submitted ticket; blocks until its results are on the host."""
        held = self._tickets.get(int(ticket))
        if held is None:
            raise AudioProcessingError(f"Model prediction failed: ticket {ticket} is not outstanding")
        s, _f, T, multi = held
        probs = np.empty((s.size, T), np.float32)
        ev = np.zeros((s.size, T), np.uint8)
        seg = np.zeros(s.size, np.int32)
        try:
            self._check(self._lib.vad_step_collect(self._h, int(ticket), _ptr(probs, C.c_float), _ptr(ev, C.c_uint8),
                                                   _ptr(seg, C.c_int32)))
        finally:
            self._tickets.pop(int(ticket), None)
        return (probs, ev, seg) if multi else (probs[:, 0], ev[:, 0], seg)

    def step_rates(self, segments, slots, denoise: Optional[float] = 0.01):
        """One tick for streams at other input rates (``vad_step_rates``): ``segments`` = [(chunks [n_k, n_in_k] float32,
        sr_in_k), ...] with n_in = 256 / 512 / 768 / 1536 at 8 / 16 / 24 / 48 kHz; ``slots`` lists the streams of all
        segments in order.  Resample + model step chained on the GPU -> (probs, events, seg_frames)."""
        k = len(segments)
        arrs = [np.ascontiguousarray(a, np.float32) for a, _ in segments]
        for a in arrs:
            if a.ndim != 2:
                raise AudioProcessingError(f"Failed to resample audio: expected [n, n_in], got {a.shape}")
        ptrs = (C.c_void_p * k)(*[a.ctypes.data for a in arrs])
        n = (C.c_int64 * k)(*[a.shape[0] for a in arrs])
        sr = (C.c_int32 * k)(*[int(r) for _, r in segments])
        for a, (_, r) in zip(arrs, segments):
            want = {8000: 256, 16000: 512, 24000: 768, 48000: 1536}.get(int(r))
            if want is not None and a.shape[1] != want:
                raise AudioProcessingError(f"Failed to resample audio from {r}Hz to 16000Hz: a chunk must hold {want} samples, got {a.shape[1]}")
        s = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        total = sum(a.shape[0] for a in arrs)
        if s.size != total:
            raise AudioProcessingError(f"Model prediction failed: {s.size} slots for {total} chunks")
        probs = np.empty(total, np.float32)
        ev = np.zeros(total, np.uint8)
        seg = np.zeros(total, np.int32)
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step_rates(self._h, k, ptrs, n, sr, _ptr(s, C.c_int64), thr, _ptr(probs, C.c_float),
                                             _ptr(ev, C.c_uint8), _ptr(seg, C.c_int32)))
        return probs, ev, seg

    def step_rates_device(self, segments, d_probs: int, d_slots: int = 0, d_events: int = 0, d_seg: int = 0,
                          denoise: Optional[float] = 0.01, stream: int = 0) -> None:
        """Device-pointer form: ``segments`` = [(d_in, n, sr_in), ...] (``vad_step_rates_device``), asynchronous."""
        k = len(segments)
        ptrs = (C.c_void_p * k)(*[int(a[0]) for a in segments])
        n = (C.c_int64 * k)(*[int(a[1]) for a in segments])
        sr = (C.c_int32 * k)(*[int(a[2]) for a in segments])
        thr = -1.0 if denoise is None else float(denoise)
        self._check(self._lib.vad_step_rates_device(self._h, k, ptrs, n, sr, d_slots or None, thr, d_probs, d_events or None,
                                                    d_seg or None, stream or None))

    def resample_multi_device(self, segments, stream: int = 0) -> None:
        """One launch for up to 4 segments ``(d_in, n, n_in, sr_in, d_out)`` of device pointers (integers)."""
        k = len(segments)
        d_in = (C.c_void_p * k)(*[int(s[0]) for s in segments])
        n = (C.c_int64 * k)(*[int(s[1]) for s in segments])
        n_in = (C.c_int32 * k)(*[int(s[2]) for s in segments])
        sr = (C.c_int32 * k)(*[int(s[3]) for s in segments])
        d_out = (C.c_void_p * k)(*[int(s[4]) for s in segments])
        self._check(self._lib.vad_resample_multi_device(self._h, k, d_in, n, n_in, sr, d_out, stream or None))

    # ------------------------------------------------------------------ resampler (a11)
    def resample(self, chunks, sr_in: int) -> np.ndarray:
        """chunks [n, n_in] float32 at ``sr_in`` -> [n, 512] at 16 kHz (``vad_resample``)."""
        x = np.ascontiguousarray(chunks, np.float32)
        if x.ndim != 2:
            raise AudioProcessingError(f"Failed to resample audio: expected [n, n_in], got {x.shape}")
        out = np.empty((x.shape[0], 512), np.float32)
        self._check(self._lib.vad_resample(self._h, _ptr(x, C.c_float), x.shape[0], x.shape[1], int(sr_in),
                                           _ptr(out, C.c_float)))
        return out

    def resample_generic_device(self, d_in: int, rows: int, n_in: int, n_out: int, d_out: int, f64: bool = False) -> None:
        """Device-pointer form (``vad_resample_generic_device``): ``d_in`` -> [rows, n_in] float32 (float64 with ``f64``),
        ``d_out`` -> [rows, n_out] float32; synchronous - the result is complete on return."""
        self._check(self._lib.vad_resample_generic_device(self._h, C.c_void_p(int(d_in)), int(bool(f64)), int(rows), int(n_in), int(n_out),
                                                          C.c_void_p(int(d_out))))

    def set_resample_path(self, mode: int) -> None:
        """0 = by size, 1 = the direct kernel, 2 = the chirp-z / FFT path (``vad_debug_resample_path``)"""
        self._check(self._lib.vad_debug_resample_path(self._h, int(mode)), VADError)

    def resample_generic(self, arrays, n_out: int) -> np.ndarray:
        """arrays [rows, n_in] (float32, or float64 for double-precision input) -> [rows, n_out] float32: each row through
        ``scipy.signal.resample(row, n_out)`` as a whole (``vad_resample_generic``; any lengths)."""
        x = np.ascontiguousarray(arrays)
        if x.dtype != np.float64:
            x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2:
            raise AudioProcessingError(f"Failed to resample audio: expected [rows, n_in], got {x.shape}")
        out = np.empty((x.shape[0], max(int(n_out), 0)), np.float32)
        self._check(self._lib.vad_resample_generic(self._h, x.ctypes.data_as(C.c_void_p), int(x.dtype == np.float64), x.shape[0],
                                                   x.shape[1], int(n_out), _ptr(out, C.c_float)))
        return out
