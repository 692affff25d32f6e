"""Whole recordings -> speech segments, and their audio: the corpus caller's face of ``Engine.scan`` and ``Engine.cut``
(``vad_scan``, ``vad_scan_cut``, include/vad_engine.h).

``VADWrapper.process_audio_data`` stays on its own path (its callback-abort contract needs the frame-by-frame replay); this
module is for callers who hold many finished recordings of different lengths and want the segments of each.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .core.config import VADConfig
from .core.exceptions import ConfigurationError


@dataclass(frozen=True)
class SegmentRefine:
    """How a segment table is refined behind the state machine (``vad_refine``, include/vad_engine.h, which has the rule in full;
    ``Engine.refine``).  All six count FRAMES: ``pad_before`` / ``pad_after`` frames of context around each segment (neighbours
    closer than both pads share the gap), ``merge_gap`` joins segments of a recording whose pause is that many frames or fewer
    (-1: never), ``min_frames`` drops joined segments shorter than that, before padding (<= 1: keep all), ``max_frames`` splits
    longer ones at the quietest frame near each cut point (0: no limit, else >= 2).  The default changes nothing."""
    pad_before: int = 0
    pad_after: int = 0
    merge_gap: int = -1
    min_frames: int = 0
    max_frames: int = 0
    reserved: int = 0

    @classmethod
    def from_durations(cls, hop: int, sample_rate: int, pad_ms: float = 0, merge_gap_ms: Optional[float] = None, min_speech_ms: float = 0,
                       max_speech_s: Optional[float] = None) -> "SegmentRefine":
        """The rule in the units of Silero's ``get_speech_timestamps`` (``speech_pad_ms``, ``min_silence_duration_ms``,
        ``min_speech_duration_ms``, ``max_speech_duration_s``) at a scan's ``hop`` (samples between frames) and ``sample_rate``: a
        duration becomes the nearest whole number of hops; ``max_speech_s`` is rounded DOWN, so that no record is longer, and is at
        least 2 frames.  None: no merging, no limit."""
        frames = lambda ms: int(round(float(ms) * sample_rate / (1000.0 * hop)))
        pad = frames(pad_ms)
        return cls(pad, pad, -1 if merge_gap_ms is None else frames(merge_gap_ms), frames(min_speech_ms),
                   0 if max_speech_s is None else max(int(float(max_speech_s) * sample_rate // hop), 2))


def speech_segments(events, seg_frames, frame: int, hop: int) -> List[Tuple[int, int]]:
    """The finished segments of one recording as sample ranges ``[(start_sample, end_sample), ...]`` (end exclusive), from the
    per-frame ``events`` and ``seg_frames`` of ``Engine.scan``: a ``VAD_EV_END`` at frame ``e`` with length ``L`` covers the
    frames ``e - L + 1 .. e``, i.e. the samples ``[(e - L + 1) * hop, e * hop + frame)``.  A segment still open at the
    recording's last frame has no END and is not listed (``scan_recordings(open_end=True)`` lists it)."""
    ev = np.asarray(events)
    seg = np.asarray(seg_frames)
    out = []
    for e in np.flatnonzero((ev & _ffi.VAD_EV_END) != 0):
        L = int(seg[e])
        out.append(((int(e) - L + 1) * hop, int(e) * hop + frame))
    return out


def segment_ranges(table, frame: int, hop: int) -> List[Tuple[int, int]]:
    """The records of ``Engine.scan_segments`` (a structured array with ``first_frame`` and ``nframes``) as the sample ranges
    ``speech_segments`` gives: ``(first_frame * hop, (first_frame + nframes - 1) * hop + frame)`` each, in the table's order."""
    return [(f * hop, (f + n - 1) * hop + frame) for f, n in zip(table["first_frame"].tolist(), table["nframes"].tolist())]


def _frame_stats(probs, events, e: int, L: int) -> Tuple[float, float]:
    """mean_prob and max_prob of ``vad_segment`` (include/vad_engine.h) from per-frame results, for engines without the kernel"""
    t0 = max(e - L + 1, 0)
    p = np.asarray(probs[t0:e + 1], np.float32)[(np.asarray(events[t0:e + 1]) & _ffi.VAD_EV_REJECTED) == 0]
    if p.size == 0:
        return 0.0, 0.0
    fixed = int(np.rint(p.astype(np.float64) * 2.0 ** 30).astype(np.int64).sum())
    return float(np.float32(fixed / (p.size * 2.0 ** 30))), float(p.max())


def _table_ranges(table, n: int, per: int, frame: int, hop: int, stats: bool) -> List[List[List]]:
    """A segment table of ``n`` recordings with ``per`` items each (``item = recording * per + channel``) -> per recording, per
    channel, the ranges ``(start_sample, end_sample)`` - with ``stats``: ``(start_sample, end_sample, mean_prob, max_prob)``."""
    out = [[[] for _ in range(per)] for _ in range(n)]
    extra = zip(table["mean_prob"].tolist(), table["max_prob"].tolist())
    for item, rg, st in zip(table["item"].tolist(), segment_ranges(table, frame, hop), extra):
        out[item // per][item % per].append(rg + st if stats else rg)
    return out


def _with_tails(table, tails):
    """``table`` with the tails that exist (``nframes > 0``) behind it: ``_table_ranges`` then lists each as its item's last range"""
    return np.concatenate([table, tails[tails["nframes"] > 0]])


def _need_tails(engine, who: str, what: str = "scan_tails") -> None:
    if not hasattr(engine, what):
        raise ConfigurationError("open_end", "True", f"{who}: open_end=True needs an engine with {what} (the length of a segment still open "
                                 f"at a recording's last frame is the state machine's to tell), {type(engine).__name__} has none")


def _need_refine(engine, who: str) -> None:
    if not hasattr(engine, "refine"):
        raise ConfigurationError("refine", "given", f"{who}: refine= needs an engine with refine (the split reads the per-frame probabilities "
                                 f"a scan left on the GPU), {type(engine).__name__} has none")


def _need_levels(engine, who: str, what: str = "levels=True") -> None:
    if not hasattr(engine, "levels"):
        raise ConfigurationError("levels", "given", f"{who}: {what} needs an engine with levels (the statistics are reduced from the block "
                                 f"a scan left on the GPU), {type(engine).__name__} has none")


def _need_render(engine, who: str) -> None:
    if not hasattr(engine, "render"):
        raise ConfigurationError("render", "given", f"{who} needs an engine with render (the audio is assembled from the block a scan "
                                 f"left on the GPU), {type(engine).__name__} has none")


def _need_stereo(engine, who: str, what: str) -> None:
    if not hasattr(engine, what):
        raise ConfigurationError("keep_channels", "True", f"{who}: keep_channels=True needs an engine with {what} (both channels are "
                                 f"written from the block a scan left on the GPU), {type(engine).__name__} has none")


def _need_resample(engine, who: str, what: str) -> None:
    if not hasattr(engine, "resample_cut"):
        raise ConfigurationError("sample_rate", "given", f"{who}: {what} needs an engine with resample_cut (the 16 kHz signal is filtered "
                                 f"from the block a scan left on the GPU), {type(engine).__name__} has none")


def resample_taps(sample_rate: int, half_width: int = 16, beta: float = 8.0, cutoff: Optional[float] = None) -> np.ndarray:
    """The default low-pass of ``Engine.resample_cut`` for recordings at ``sample_rate`` (8000, 24000 or 48000 Hz): with ``L / M =
    16000 / sample_rate`` in lowest terms, a Kaiser-windowed sinc at rate ``L * sample_rate`` of ``2 * half_width * max(L, M) + 1``
    taps - ``half_width`` zero crossings of the sinc on either side at the default cutoff - with ``cutoff`` in Hz (default:
    ``min(sample_rate, 16000) / 2``, the narrower Nyquist) and the window's ``beta``.  Designed in float64, scaled so that the taps
    sum to ``L`` (every polyphase branch then sums to about 1: unit gain at DC), rounded once to float32.  The defaults give 65, 97
    and 97 taps at 8, 24 and 48 kHz; ``scipy.signal.resample_poly(x, L, M, window=taps)`` applies the same filter."""
    sr = int(sample_rate)
    if sr not in (8000, 24000, 48000):
        raise ConfigurationError("sample_rate", repr(sample_rate), f"resample_taps: recordings at 8000, 24000 or 48000 Hz, got {sample_rate!r}")
    L, M = (2, 1) if sr == 8000 else (2, 3) if sr == 24000 else (1, 3)
    half_width = int(half_width)
    n = 2 * half_width * max(L, M) + 1
    if half_width < 0 or n > _ffi.VAD_RESAMPLE_CUT_MAX_TAPS:
        raise ConfigurationError("half_width", repr(half_width), f"resample_taps: 2 * half_width * {max(L, M)} + 1 taps must be 1 .. "
                                 f"{_ffi.VAD_RESAMPLE_CUT_MAX_TAPS}, got half_width = {half_width}")
    fc = min(sr, 16000) / 2.0 if cutoff is None else float(cutoff)
    if not 0.0 < fc <= min(sr, 16000) / 2.0:
        raise ConfigurationError("cutoff", repr(cutoff), f"resample_taps: 0 < cutoff <= {min(sr, 16000) / 2.0} Hz, got {cutoff!r}")
    t = np.arange(n, dtype=np.float64) - (n - 1) // 2
    h = np.sinc(2.0 * fc / (L * sr) * t) * np.kaiser(n, float(beta))
    return (h * (L / h.sum())).astype(np.float32)


def convert_ratio(sample_rate: int, engine_rate: int = 16000) -> Tuple[int, int]:
    """``(L, M)`` of ``Engine.convert`` for recordings at ``sample_rate``: ``engine_rate / sample_rate`` in lowest terms.  A rate the
    conversion does not accept - outside 4000 .. 192000 Hz, the engine's own, a period ``lcm(L, 16)`` above 640 outputs or ``M`` above
    640 - is a ``ConfigurationError``."""
    import math
    sr, R = int(sample_rate), int(engine_rate)
    g = math.gcd(sr, R) if sr > 0 and R > 0 else 1
    L, M = R // g, sr // g
    if not (_ffi.VAD_CONVERT_MIN_RATE <= sr <= _ffi.VAD_CONVERT_MAX_RATE) or sr == R or R < 1 or \
            L * 16 // math.gcd(L, 16) > _ffi.VAD_CONVERT_MAX_PERIOD or M > _ffi.VAD_CONVERT_MAX_PERIOD:
        raise ConfigurationError("sample_rate", repr(sample_rate), f"convert: recordings at {sample_rate!r} Hz on a {R} Hz engine (L / M = {L} / {M}): "
                                 f"accepted are {_ffi.VAD_CONVERT_MIN_RATE} .. {_ffi.VAD_CONVERT_MAX_RATE} Hz other than the engine's with lcm(L, 16) "
                                 f"and M of at most {_ffi.VAD_CONVERT_MAX_PERIOD}")
    return L, M


def convert_taps(sample_rate: int, engine_rate: int = 16000, half_width: int = 16, beta: float = 8.0, cutoff: Optional[float] = None) -> np.ndarray:
    """``resample_taps``' design for any rate ``Engine.convert`` accepts (44100, 22050, 11025, 32000, 12000, 96000 ..): with ``L / M =
    engine_rate / sample_rate`` in lowest terms, a Kaiser-windowed sinc at rate ``L * sample_rate`` of ``2 * half_width * max(L, M) + 1``
    taps, cutoff ``min(sample_rate, engine_rate) / 2`` Hz unless given, designed in float64, scaled to sum to ``L``, rounded once to
    float32 - byte for byte ``resample_taps(sample_rate)`` at 8000, 24000 and 48000 Hz.  The conversion takes at most ``128 * L`` taps:
    where ``M > 4 L`` (88200, 96000, 176400, 192000 Hz on a 16 kHz engine) the default ``half_width`` is too wide and a narrower one
    must be named (``Engine.convert``'s own default picks the widest that fits)."""
    L, M = convert_ratio(sample_rate, engine_rate)
    sr, R = int(sample_rate), int(engine_rate)
    half_width = int(half_width)
    n = 2 * half_width * max(L, M) + 1
    if half_width < 0 or n > _ffi.VAD_CONVERT_MAX_REACH * L:
        raise ConfigurationError("half_width", repr(half_width), f"convert_taps: 2 * half_width * {max(L, M)} + 1 taps must be 1 .. "
                                 f"{_ffi.VAD_CONVERT_MAX_REACH * L} (128 * L), got half_width = {half_width}; at most "
                                 f"{(_ffi.VAD_CONVERT_MAX_REACH * L - 1) // (2 * max(L, M))} fits")
    fc = min(sr, R) / 2.0 if cutoff is None else float(cutoff)
    if not 0.0 < fc <= min(sr, R) / 2.0:
        raise ConfigurationError("cutoff", repr(cutoff), f"convert_taps: 0 < cutoff <= {min(sr, R) / 2.0} Hz, got {cutoff!r}")
    t = np.arange(n, dtype=np.float64) - (n - 1) // 2
    h = np.sinc(2.0 * fc / (L * sr) * t) * np.kaiser(n, float(beta))
    return (h * (L / h.sum())).astype(np.float32)


def input_ranges(ranges, sample_rate: int, engine_rate: int, nsamples: int) -> List[Tuple]:
    """Ranges of a CONVERTED recording (``scan_recordings(convert=...)``: samples at ``engine_rate``) mapped back to the input samples
    they cover: ``(a, b, ...) -> (a M // L, min(ceil(b M / L), nsamples), ...)`` with ``L / M = engine_rate / sample_rate`` in lowest
    terms; whatever follows the two positions (statistics, levels) is kept."""
    import math
    g = math.gcd(int(sample_rate), int(engine_rate))
    L, M = int(engine_rate) // g, int(sample_rate) // g
    return [(int(a) * M // L, min(-((-int(b) * M) // L), int(nsamples))) + tuple(rest) for a, b, *rest in ranges]


def _convert_arg(who: str, engine, sample_rate, convert, split: bool = False, keep_channels: bool = False, resample=False):
    """``convert=`` of the corpus functions -> None, or ``(input rate, True or taps)``: the recordings are converted once to the engine's
    rate (``Engine.scan_segments(convert=...)``) and everything downstream treats them as recordings at the engine's own rate"""
    if convert is None or convert is False:
        return None
    if not hasattr(engine, "convert") or not hasattr(engine, "scan_segments"):
        raise ConfigurationError("convert", "given", f"{who}: convert= needs an engine with convert (the recordings are converted on the GPU "
                                 f"ahead of the scan), {type(engine).__name__} has none")
    if sample_rate is None or int(sample_rate) == int(engine.sample_rate):
        raise ConfigurationError("convert", "given", f"{who}: convert= converts recordings at another rate than the engine's {engine.sample_rate} "
                                 f"Hz: it needs sample_rate= (got {sample_rate!r})")
    if keep_channels:
        raise ConfigurationError("convert", "given", f"{who}: convert= with keep_channels=True: a converted recording is mono, two-channel "
                                 "converted output is not supported")
    if resample is not False and resample is not None:
        raise ConfigurationError("convert", "given", f"{who}: convert= with resample=: a converted recording is at the engine's rate already")
    if split:
        raise ConfigurationError("convert", "given", f"{who}: convert= with channel='split': a converted recording is mono - scan 'mix', 0 or 1")
    convert_ratio(int(sample_rate), int(engine.sample_rate))      # (a rate the conversion refuses: ConfigurationError)
    return int(sample_rate), convert


def _keep_channels_check(who: str, split: bool) -> None:
    if split:
        raise ConfigurationError("keep_channels", "True", f"{who}: keep_channels=True delivers both channels of a recording in one payload; "
                                 "channel='split' asks for one payload per channel - scan 'mix', 0 or 1")


def _joint_gains(engine, table, hop: int, denoise, normalize) -> np.ndarray:
    """``normalize`` for segments whose two channels are both kept: ONE ``Engine.levels`` call lists every segment twice - channel 0,
    then channel 1 - and a segment's factor is ``np.float32(normalize)`` over the larger of its two peaks (1 where that is 0 or not
    finite): one factor for both channels keeps their balance"""
    both = [sg + (0,) for sg in table] + [sg + (1,) for sg in table]
    peak = engine.levels(both, hop=hop, denoise=denoise)["peak"]
    peak = np.maximum(peak[:len(table)], peak[len(table):])
    usable = np.isfinite(peak) & (peak > 0)
    return np.where(usable, np.float32(normalize) / np.where(usable, peak, np.float32(1)), np.float32(1)).astype(np.float32)


def fade_ramp(n: int, shape: str = "linear") -> np.ndarray:
    """A fade table of ``n`` entries for ``Engine.render``, rising from just above 0 to just below 1: ``"linear"`` is
    ``(k + 0.5) / n``, ``"cosine"`` is ``0.5 - 0.5 cos(pi (k + 0.5) / n)`` - computed in float64 and rounded once to float32.
    Two linear ramps that cross sum to exactly 1 in float64; the half-sample offset keeps a faded edge from starting on a zero."""
    n = int(n)
    if n < 0:
        raise ConfigurationError("n", repr(n), f"fade_ramp: n is 0 or more, got {n}")
    if shape not in ("linear", "cosine"):
        raise ConfigurationError("shape", repr(shape), f"fade_ramp: shape is 'linear' or 'cosine', got {shape!r}")
    t = (np.arange(n, dtype=np.float64) + 0.5) / max(n, 1)
    return (t if shape == "linear" else 0.5 - 0.5 * np.cos(np.pi * t)).astype(np.float32)


def level_stats(levels, nsamples) -> Tuple[np.ndarray, np.ndarray]:
    """``Engine.levels`` records and the segments' sample counts -> ``(energy, rms)`` as float64 arrays: ``energy = energy_q32 /
    2^32`` (``AudioUtils.calculate_energy`` of the segment, samples beyond full scale counted as 1) and ``rms = sqrt(energy /
    nsamples)`` (``AudioUtils.calculate_rms``; 0 for a segment without samples)."""
    energy = np.asarray(levels["energy_q32"], np.float64) / 2.0 ** 32
    ns = np.asarray(nsamples, np.float64)
    return energy, np.sqrt(np.divide(energy, ns, out=np.zeros_like(energy), where=ns > 0))


def _cut_table(engine, ranges, chans, frame: int, hop: int) -> List[Tuple]:
    """ranges per (recording, channel) of the scan the engine packed last -> the segments ``Engine.cut`` / ``Engine.levels`` take, in
    the order listed"""
    return [(int(engine.last_scan["offsets"][k]), a // hop, (b - a - frame) // hop + 1, chans[c])
            for k, rc in enumerate(ranges) for c, rg in enumerate(rc) for a, b, *_ in rg]


def _append_levels(engine, ranges, chans, frame: int, hop: int, denoise) -> List[List[List]]:
    """every range of ``ranges`` with ``(rms, peak, clipped)`` behind what it holds: one ``Engine.levels`` call on the listed ranges,
    on the block the scan left on the GPU (the caller holds ``scan_session()``)"""
    table = _cut_table(engine, ranges, chans, frame, hop)
    if not table:
        return ranges
    lv = engine.levels(table, hop=hop, denoise=denoise)
    _, rms = level_stats(lv, [(n - 1) * hop + frame for _, _, n, _ in table])
    extra = iter(zip(rms.tolist(), lv["peak"].tolist(), lv["clipped"].tolist()))
    return [[[tuple(rg) + next(extra) for rg in one] for one in rc] for rc in ranges]


def _scan_ranges(engine, slots, recordings, per: int, frame: int, hop: int, law, denoise, channel, stats: bool = False,
                 rate: Optional[int] = None, open_end: bool = False, refine=None, levels: bool = False, convert=None) -> List[List[List]]:
    """One scan of ``recordings`` (all 1-D or all two-channel) on ``slots`` -> per recording, per channel scanned of it (``per``),
    the finished segments ``(start_sample, end_sample)`` - with ``stats``: ``(start_sample, end_sample, mean_prob, max_prob)``.
    An engine with ``scan_segments`` builds the table on the GPU and copies back that alone; any other goes through the per-frame
    results of ``scan``.  Same ranges either way.  ``rate``: the recordings' sample rate when it is not the engine's (``frame`` and
    ``hop`` are then a chunk and a hop in input samples; ``vad_scan_rate_segments`` builds the table).  ``open_end``: the segment
    still open at an item's last frame (``Engine.scan_tails``) is its last range.  ``refine``: the table - and, with
    ``open_end``, the tails as each item's last record - goes through ``Engine.refine`` on the GPU; the statistics are the refined records'.
    ``levels``: every range listed gets ``(rms, peak, clipped)`` appended (``Engine.levels`` on the ranges as listed).
    ``convert`` (``_convert_arg``): the recordings are converted to the engine's rate ahead of the scan; ``rate`` is None then, and
    ``frame``, ``hop`` and the ranges count samples of the converted signal."""
    if levels:
        _need_levels(engine, "scan_recordings")
        two = recordings[0].ndim == 2
        with engine.scan_session():
            ranges = _scan_ranges(engine, slots, recordings, per, frame, hop, law, denoise, channel, stats, rate, open_end, refine, convert=convert)
            return _append_levels(engine, ranges, (0, 1) if per == 2 else (channel if two and convert is None else 0,), frame, hop, denoise)
    sl = np.asarray(slots).reshape(len(recordings), per) if per == 2 else slots
    kw = {} if rate is None else {"sample_rate": rate}
    if convert is not None:
        kw = {"sample_rate": convert[0], "convert": convert[1]}
    if refine is not None:
        _need_refine(engine, "scan_recordings")
        if open_end:
            _need_tails(engine, "scan_recordings")
        with engine.scan_session():
            engine.scan_segments(sl, recordings, hop=hop, law=law, denoise=denoise, channel=channel, **kw)
            table = engine.refine(refine, None, engine.scan_tails() if open_end else None)      # the scan's own table, on the GPU
        return _table_ranges(table, len(recordings), per, frame, hop, stats)
    if open_end:
        _need_tails(engine, "scan_recordings")
        with engine.scan_session():
            table = engine.scan_segments(sl, recordings, hop=hop, law=law, denoise=denoise, channel=channel, **kw)
            table = _with_tails(table, engine.scan_tails())
        return _table_ranges(table, len(recordings), per, frame, hop, stats)
    if hasattr(engine, "scan_segments"):
        table = engine.scan_segments(sl, recordings, hop=hop, law=law, denoise=denoise, channel=channel, **kw)
        return _table_ranges(table, len(recordings), per, frame, hop, stats)
    probs, ev, seg = engine.scan(sl, recordings, hop=hop, law=law, denoise=denoise, channel=channel, **kw)
    out = []
    for p, e, g in zip(probs, ev, seg):
        one = []
        for c in range(per):
            pc, ec, gc = (p[c], e[c], g[c]) if per == 2 else (p, e, g)
            rgs = speech_segments(ec, gc, frame, hop)
            if stats:
                rgs = [(a, b) + _frame_stats(pc, ec, (b - frame) // hop, (b - a - frame) // hop + 1) for a, b in rgs]
            one.append(rgs)
        out.append(one)
    return out


def scan_recordings(recordings: Sequence[np.ndarray], config: Optional[VADConfig] = None, engine=None, hop: Optional[int] = None,
                    law: Optional[str] = None, channel="mix", stats: bool = False, sample_rate: Optional[int] = None,
                    open_end: bool = False, refine: Optional[SegmentRefine] = None, levels: bool = False, convert=None) -> List[List[Tuple]]:
    """Speech segments of every recording, one launch sequence for the lot: opens one stream per recording with the config's
    thresholds, scans (frames of ``engine.frame_samples`` at ``hop``, default half a frame as ``VADWrapper`` frames a chunk;
    the config's denoise gate), closes the streams -> per recording ``[(start_sample, end_sample), ...]``.
    ``engine``: an :class:`~cutter_vad_amd.engine.Engine`; default: the process-wide pool's engine for the config.
    A recording may be a ``[nsamples, 2]`` array, interleaved channels as WAV readers deliver a recorded call; a corpus may hold
    both kinds (at most two scans, results in the caller's order).  ``channel``: what is scanned of a two-channel recording -
    ``"mix"`` (the default: the mean of the channels, as ``VADWrapper`` mixes such an array down), ``0`` or ``1``: one segment
    list per recording; ``"split"``: one list per CHANNEL - ``[segments]`` for a 1-D recording, ``[left, right]`` for a 2-D one.
    ``sample_rate``: the RECORDINGS' rate when it is not the engine's: 8000, 24000 or 48000 on a 16 kHz Silero V5 engine.  The corpus
    is uploaded at that rate and resampled on the GPU chunk by chunk (``Engine.scan(sample_rate=...)``); chunks have
    ``512 * sample_rate / 16000`` samples, ``hop`` counts input samples (default half a chunk) and the ranges returned are in
    INPUT-rate samples.  None, or the engine's rate: as above.
    ``open_end``: a recording that stops inside speech - before the ``voice_end_frame_count`` low frames an END needs - has no END
    for its last segment, and by default that segment is not listed (a stream may go on).  ``True`` appends it, as the last range
    of its recording or channel: from the first frame the state machine buffered for it to the recording's last frame, with its
    mean and maximum under ``stats=True`` (``Engine.scan_tails``; an engine object without it: ``ConfigurationError``).
    ``refine``: a :class:`SegmentRefine` - the segments are padded, merged, thinned and split on the GPU before they are listed
    (``Engine.refine``; an engine object without it: ``ConfigurationError``): the ranges and, under ``stats=True``, the statistics
    are the refined records', and with ``open_end=True`` the open segment is refined with the others as its recording's last.
    ``levels``: ``True`` appends ``(rms, peak, clipped)`` to every range listed - refined records and open segments too - behind
    ``stats``' two values when both are given: the root mean square, the largest magnitude and the number of samples at or above
    0.95 (``AudioUtils.calculate_rms`` / ``detect_clipping``) of the range's samples as the model heard them - decoded, mixed and
    gated; input-rate samples, not gated, under ``sample_rate`` - reduced on the GPU from the block the scan left there
    (``Engine.levels``; an engine object without it: ``ConfigurationError``).
    ``convert``: ``True`` or a taps array (``Engine.convert``'s ``taps``; ``True``: the default design of ``convert_taps``) - the
    recordings are at ANY rate ``Engine.convert`` accepts (44100, 22050, 11025, 32000, 12000, 96000 .. - and 8000, 24000, 48000 too): each
    is converted ONCE on the GPU to a continuous signal at the engine's rate (``Engine.scan_segments(convert=...)``) and scanned as a
    recording at that rate: ``hop`` defaults to half a frame and the ranges count samples of the CONVERTED signal, at the engine's rate
    (``input_ranges`` maps them back to input samples).  It needs a ``sample_rate`` other than the engine's; ``channel="split"``, or an
    engine object without ``convert``: ``ConfigurationError``.  Without it ``sample_rate`` means what it meant."""
    from .pool import default_pool, resolve_model_path
    split = isinstance(channel, str) and channel == "split"
    # checked here, not by the scan: a corpus of 1-D recordings alone never shows the value to Engine.scan
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"scan_recordings: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    cfg = config or VADConfig()
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    if open_end:
        _need_tails(engine, "scan_recordings")
    if refine is not None:
        _need_refine(engine, "scan_recordings")
    if levels:
        _need_levels(engine, "scan_recordings")
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError(f"scan_recordings frames at the model's frame size: buffer_size = {cfg.buffer_size}, "
                                 f"the engine's frames have {frame} samples")
    rate = None if sample_rate is None or int(sample_rate) == int(engine.sample_rate) else int(sample_rate)
    conv = _convert_arg("scan_recordings", engine, sample_rate, convert, split)
    if conv is not None:
        rate = None                                  # downstream the recordings are at the engine's own rate
    if rate is not None:
        if rate not in (8000, 16000, 24000, 48000):
            raise ConfigurationError("sample_rate", repr(sample_rate), f"scan_recordings: recordings at 8000, 16000, 24000 or 48000 Hz, got {sample_rate!r}")
        frame = engine.scan_chunk_samples(rate)      # the ranges count input samples
    hop = frame // 2 if hop is None else int(hop)
    recordings = [np.asarray(r) for r in recordings]
    if not recordings:
        return []
    out: List = [None] * len(recordings)
    for two in (False, True):
        idx = [i for i, r in enumerate(recordings) if (r.ndim == 2) == two]
        if not idx:
            continue
        per = 2 if two and split else 1
        slots = engine.open_streams(len(idx) * per)
        try:
            engine.set_thresholds_many(slots, (cfg.vad_start_probability, cfg.vad_end_probability, cfg.voice_start_ratio,
                                               cfg.voice_end_ratio, cfg.voice_start_frame_count, cfg.voice_end_frame_count))
            ranges = _scan_ranges(engine, slots, [recordings[i] for i in idx], per, frame, hop, law, 0.01 if cfg.enable_denoising else None,
                                  channel, stats, rate, open_end, refine, levels, convert=conv)
        finally:
            for s in slots:
                engine.close_stream(int(s))
        for i, rc in zip(idx, ranges):
            out[i] = rc if split else rc[0]
    return out


def _thresholds_of(cfg: VADConfig) -> Tuple:
    return (cfg.vad_start_probability, cfg.vad_end_probability, cfg.voice_start_ratio, cfg.voice_end_ratio, cfg.voice_start_frame_count,
            cfg.voice_end_frame_count)


def sweep_recordings(recordings: Sequence[np.ndarray], configs: Sequence[VADConfig], engine=None, hop: Optional[int] = None,
                     law: Optional[str] = None, channel="mix", stats: bool = False, sample_rate: Optional[int] = None, convert=None,
                     open_end: bool = False, refine: Optional[SegmentRefine] = None, levels: bool = False) -> List[List]:
    """``scan_recordings`` under several configs for the price of one scan: ``sweep_recordings(recs, cfgs, **kw)[j] ==
    scan_recordings(recs, cfgs[j], **kw)``.  The model runs once per kind of recording (1-D, 2-D), with the first config's
    thresholds; the segment tables of all configs then come from ONE replay of the per-frame probabilities that scan left on the
    GPU (``Engine.resegment``, 64 configs per replay: the model's output does not depend on the thresholds).  The configs may differ
    in the six threshold fields alone; they must agree on what the probabilities depend on - ``model_version``, ``sample_rate``,
    ``buffer_size``, ``enable_denoising`` and ``model_path`` - or ``ConfigurationError`` names the field.  An engine object without
    ``resegment`` is served config by config.  ``open_end`` as in ``scan_recordings``: each config's open segments come from the
    same replay (``Engine.resegment_tails``).  ``refine`` as there too: each config's replayed table, with its tails, goes through
    ``Engine.refine``.  ``levels`` as there: one ``Engine.levels`` call per config on that config's ranges.  ``convert`` as there:
    the recordings are converted once (``Engine.scan_segments(convert=...)``) and every config replays the converted scan."""
    from .pool import default_pool, resolve_model_path
    configs = list(configs)
    if not configs:
        return []
    cfg = configs[0]
    for other in configs[1:]:
        for field in ("model_version", "sample_rate", "buffer_size", "enable_denoising", "model_path"):
            if getattr(other, field) != getattr(cfg, field):
                raise ConfigurationError(field, repr(getattr(other, field)),
                                         f"sweep_recordings: the configs of one sweep share {field} (the probabilities depend on it): "
                                         f"{getattr(cfg, field)!r} and {getattr(other, field)!r}")
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    if not hasattr(engine, "resegment") or not hasattr(engine, "scan_segments"):
        return [scan_recordings(recordings, c, engine=engine, hop=hop, law=law, channel=channel, stats=stats, sample_rate=sample_rate,
                                open_end=open_end, refine=refine, levels=levels, convert=convert) for c in configs]
    if open_end:
        _need_tails(engine, "sweep_recordings", "resegment_tails")
    if refine is not None:
        _need_refine(engine, "sweep_recordings")
    if levels:
        _need_levels(engine, "sweep_recordings")
    split = isinstance(channel, str) and channel == "split"
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"sweep_recordings: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError("buffer_size", repr(cfg.buffer_size), f"sweep_recordings frames at the model's frame size: buffer_size = "
                                 f"{cfg.buffer_size}, the engine's frames have {frame} samples")
    rate = None if sample_rate is None or int(sample_rate) == int(engine.sample_rate) else int(sample_rate)
    conv = _convert_arg("sweep_recordings", engine, sample_rate, convert, split)
    if conv is not None:
        rate = None                                  # (convert= as in scan_recordings)
    if rate is not None:
        if rate not in (8000, 16000, 24000, 48000):
            raise ConfigurationError("sample_rate", repr(sample_rate), f"sweep_recordings: recordings at 8000, 16000, 24000 or 48000 Hz, got {sample_rate!r}")
        frame = engine.scan_chunk_samples(rate)      # the ranges count input samples
    hop = frame // 2 if hop is None else int(hop)
    recordings = [np.asarray(r) for r in recordings]
    out: List[List] = [[None] * len(recordings) for _ in configs]
    kw = {} if rate is None else {"sample_rate": rate}
    if conv is not None:
        kw = {"sample_rate": conv[0], "convert": conv[1]}
    for two in (False, True):
        idx = [i for i, r in enumerate(recordings) if (r.ndim == 2) == two]
        if not idx:
            continue
        per = 2 if two and split else 1
        slots = engine.open_streams(len(idx) * per)
        try:
            engine.set_thresholds_many(slots, _thresholds_of(cfg))
            sl = np.asarray(slots).reshape(len(idx), per) if per == 2 else slots
            with engine.scan_session():
                engine.scan_segments(sl, [recordings[i] for i in idx], hop=hop, law=law, denoise=0.01 if cfg.enable_denoising else None,
                                     channel=channel, **kw)
                sets = [_thresholds_of(c) for c in configs]
                tables = [t for k in range(0, len(sets), 64) for t in engine.resegment(sets[k:k + 64])]      # 64 sets per replay
                if open_end:
                    tails = [t for k in range(0, len(sets), 64) for t in engine.resegment_tails(sets[k:k + 64])]
                if refine is not None:
                    tables = [engine.refine(refine, t, tails[k] if open_end else None) for k, t in enumerate(tables)]
                elif open_end:
                    tables = [_with_tails(t, tl) for t, tl in zip(tables, tails)]
                listed = [_table_ranges(t, len(idx), per, frame, hop, stats) for t in tables]
                if levels:
                    chans = (0, 1) if per == 2 else (channel if two and conv is None else 0,)
                    listed = [_append_levels(engine, r, chans, frame, hop, 0.01 if cfg.enable_denoising else None) for r in listed]
        finally:
            for s in slots:
                engine.close_stream(int(s))
        for res, ranges in zip(out, listed):
            for i, rc in zip(idx, ranges):
                res[i] = rc if split else rc[0]
    return out


def cut_recordings(recordings: Sequence[np.ndarray], config: Optional[VADConfig] = None, engine=None, hop: Optional[int] = None,
                   law: Optional[str] = None, channel="mix", layout: str = "frames", wav: bool = True,
                   sample_rate: Optional[int] = None, open_end: bool = False, refine: Optional[SegmentRefine] = None,
                   normalize: Optional[float] = None, keep_channels: bool = False, resample=False, convert=None) -> List:
    """``scan_recordings`` with each finished segment's audio: per recording ``[(start_sample, end_sample, payload), ...]`` (per
    channel for ``"split"``, as there).  ``payload`` is what ``VADWrapper``'s ``voice_end`` callback delivers for the same
    recording - the segment's frames back to back, decoded, mixed and gated as the model read them, as 16-bit PCM behind the WAV
    header of ``config.output_wav_sample_rate`` - or, with ``wav=False``, the int16 samples themselves; ``layout="range"`` gives
    the samples ``[start_sample, end_sample)`` once.  The corpus crosses the link once: one scan, then one cut of the block that
    the scan left on the GPU (``Engine.cut(audio=None)``, under ``Engine.scan_session()``), and one copy back of the speech alone
    - two of each for a corpus of 1-D and 2-D recordings.
    ``sample_rate`` as in ``scan_recordings``: the recordings are at 8000, 24000 or 48000 Hz, ``hop`` and the ranges count INPUT-rate
    samples, and the scan is the rate scan (``Engine.scan_segments(sample_rate=...)``).  ``layout="frames"`` is still the
    ``voice_end`` payload - the 16 kHz frames the model read, each chunk resampled on the GPU and gated, behind the header of
    ``config.output_wav_sample_rate``; ``layout="range"`` gives the samples ``[start_sample, end_sample)`` of the recording itself,
    at its own rate and not gated, behind a header that carries ``sample_rate``.
    ``open_end`` as in ``scan_recordings``: the segment still open at a recording's last frame is cut like any other.
    ``refine`` as in ``scan_recordings``: the audio is that of the refined records.
    ``normalize``: a target level, as ``AudioUtils.normalize_audio(target_level=...)`` per segment: each segment's samples are
    multiplied by ``np.float32(np.float32(normalize) / peak)`` ahead of the conversion to PCM - by 1 where the peak is 0 - with the
    peak of ``Engine.levels`` on the same table (the segment's sample range), so the corpus still crosses the link once and the
    factor is applied on the GPU (``Engine.cut(gains=...)``; an engine object without ``levels``: ``ConfigurationError``).
    ``keep_channels``: ``True`` delivers the audio of a two-channel recording as it was recorded, both channels in place
    (``Engine.cut_stereo``; an engine object without it: ``ConfigurationError``): the recording is still scanned as ``channel`` says
    (``"mix"``, 0 or 1; ``"split"`` is a ``ConfigurationError``), ranges count sample frames as before, and the payload is a
    ``[k, 2]`` int16 array or a WAV with a two-channel header.  ``layout="frames"`` with a ``sample_rate`` other than the engine's
    is a ``ConfigurationError``: use ``layout="range"``.  ``normalize`` then divides by the larger of the segment's two channel
    peaks (one ``Engine.levels`` call listing every segment for channel 0 and for channel 1): one factor for both channels, which
    keeps their balance.  1-D recordings of the same corpus are cut as without it.
    ``resample``: ``True`` or a taps array (``Engine.resample_cut``'s ``taps``; ``True``: ``resample_taps(sample_rate)``) delivers
    each segment of recordings at another rate as ONE continuous signal at the engine's rate: it needs a ``sample_rate`` other than
    the engine's and ``layout="range"`` (else ``ConfigurationError``).  The ranges stay in input-rate samples; the payload is the
    16 kHz PCM (``Engine.resample_cut_samples`` samples) behind a header of the engine's rate.  ``normalize`` then divides by the
    INPUT-rate peak of ``Engine.levels``: the peak of the resampled signal can differ slightly (the filter overshoots between
    samples), and PCM16 saturates where it exceeds full scale.  With ``keep_channels=True``: ``ConfigurationError`` (two-channel
    resampled output is not built).
    ``convert`` as in ``scan_recordings``: the recordings, at any rate ``Engine.convert`` accepts, are converted once and are recordings
    at the engine's rate from there on - ranges, ``hop`` and both layouts (``"frames"`` too) count converted samples, the audio is cut
    from the converted signal and the WAV header carries ``config.output_wav_sample_rate``.  With ``keep_channels=True`` or
    ``resample=``: ``ConfigurationError``."""
    from .pool import default_pool, resolve_model_path
    from .utils.wav_writer import WAVWriter
    split = isinstance(channel, str) and channel == "split"
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"cut_recordings: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    if layout not in _ffi.CUT_LAYOUTS:
        raise ConfigurationError("layout", repr(layout), f"cut_recordings: layout is 'frames' or 'range', got {layout!r}")
    if keep_channels:
        _keep_channels_check("cut_recordings", split)
    cfg = config or VADConfig()
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    if keep_channels:
        _need_stereo(engine, "cut_recordings", "cut_stereo")
    if open_end:
        _need_tails(engine, "cut_recordings")
    if refine is not None:
        _need_refine(engine, "cut_recordings")
    if normalize is not None:
        _need_levels(engine, "cut_recordings", "normalize=")
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError(f"cut_recordings frames at the model's frame size: buffer_size = {cfg.buffer_size}, "
                                 f"the engine's frames have {frame} samples")
    rate = None if sample_rate is None or int(sample_rate) == int(engine.sample_rate) else int(sample_rate)
    conv = _convert_arg("cut_recordings", engine, sample_rate, convert, split, keep_channels, resample)
    if conv is not None:
        rate = None                                  # downstream the recordings are at the engine's own rate
    resampled = resample is not False and resample is not None
    if resampled:
        if rate is None or layout != "range":
            raise ConfigurationError("resample", "given", f"cut_recordings: resample= delivers the sample range of recordings at another "
                                     f"rate than the engine's at {engine.sample_rate} Hz: it needs sample_rate= (got {sample_rate!r}) and "
                                     f"layout=\"range\" (got {layout!r})")
        if keep_channels:
            raise ConfigurationError("resample", "given", "cut_recordings: resample= with keep_channels=True: two-channel resampled "
                                     "output is not supported")
        _need_resample(engine, "cut_recordings", "resample=")
    taps = None if resample is True or not resampled else resample
    if rate is not None:
        if rate not in (8000, 16000, 24000, 48000):
            raise ConfigurationError("sample_rate", repr(sample_rate), f"cut_recordings: recordings at 8000, 16000, 24000 or 48000 Hz, got {sample_rate!r}")
        frame = engine.scan_chunk_samples(rate)      # the ranges count input samples
        if keep_channels and layout == "frames":
            raise ConfigurationError("layout", repr(layout), f"cut_recordings: keep_channels=True on recordings at {rate} Hz cuts their own "
                                     "samples: use layout=\"range\" (both channels of the resampled frames are not supported)")
    hop = frame // 2 if hop is None else int(hop)
    recordings = [np.asarray(r) for r in recordings]
    if not recordings:
        return []
    writer = WAVWriter(int(engine.sample_rate) if resampled else rate if rate is not None and layout == "range" else cfg.output_wav_sample_rate, 16, 1)
    writer2 = WAVWriter(writer.sample_rate, 16, 2) if keep_channels else None
    denoise = 0.01 if cfg.enable_denoising else None
    out: List = [None] * len(recordings)
    for two in (False, True):
        idx = [i for i, r in enumerate(recordings) if (r.ndim == 2) == two]
        if not idx:
            continue
        per = 2 if two and split else 1
        chans = (0, 1) if per == 2 else (channel if two and conv is None else 0,)
        slots = engine.open_streams(len(idx) * per)
        try:
            engine.set_thresholds_many(slots, (cfg.vad_start_probability, cfg.vad_end_probability, cfg.voice_start_ratio,
                                               cfg.voice_end_ratio, cfg.voice_start_frame_count, cfg.voice_end_frame_count))
            with engine.scan_session():
                # (recording, channel) -> its sample ranges; the cut's table lists them in that order
                ranges = _scan_ranges(engine, slots, [recordings[i] for i in idx], per, frame, hop, law, denoise, channel, rate=rate,
                                      open_end=open_end, refine=refine, convert=conv)
                table = _cut_table(engine, ranges, chans, frame, hop)
                if two and keep_channels:
                    table = [sg[:3] for sg in table]
                    if table:
                        gains = None if normalize is None else _joint_gains(engine, table, hop, denoise, normalize)
                        data, start = engine.cut_stereo(table, hop=hop, denoise=denoise, layout=layout, gains=gains)
                elif table and normalize is not None:
                    peak = engine.levels(table, hop=hop, denoise=denoise)["peak"]
                    usable = np.isfinite(peak) & (peak > 0)
                    gains = np.where(usable, np.float32(normalize) / np.where(usable, peak, np.float32(1)), np.float32(1)).astype(np.float32)
                    if resampled:
                        data, start = engine.resample_cut(table, rate, taps, hop=hop, gains=gains)
                    else:
                        data, start = engine.cut(table, hop=hop, denoise=denoise, layout=layout, gains=gains)
                elif table and resampled:
                    data, start = engine.resample_cut(table, rate, taps, hop=hop)
                elif table:
                    data, start = engine.cut(table, hop=hop, denoise=denoise, layout=layout)
        finally:
            for s in slots:
                engine.close_stream(int(s))
        j = 0
        for i, rc in zip(idx, ranges):
            lists = []
            for rg in rc:
                one = []
                for a, b in rg:
                    pcm = data[start[j]:start[j + 1]]
                    j += 1
                    if wav:
                        raw = pcm.tobytes()
                        one.append((a, b, (writer2 if two and keep_channels else writer).header(len(raw)) + raw))
                    else:
                        one.append((a, b, pcm.copy()))
                lists.append(one)
            out[i] = lists if split else lists[0]
    return out


def _join_places(counts: Sequence[int], nramp: int, gap: int) -> List[int]:
    """where the segments of one piece start in ``mode="join"``: back to back - neighbours ``gap`` samples apart, or, with no gap,
    overlapping by ``min(nramp, S_i / 2, S_{i+1} / 2)`` rounded down to a multiple of 4: a segment's two overlaps never meet, so no
    sample is covered three times, even around a segment shorter than the ramp"""
    at, places = 0, []
    for i, s in enumerate(counts):
        places.append(at)
        if i + 1 < len(counts):
            at += s + gap if gap > 0 else s - min(nramp, s // 2, counts[i + 1] // 2) // 4 * 4
    return places


def render_recordings(recordings: Sequence[np.ndarray], config: Optional[VADConfig] = None, engine=None, hop: Optional[int] = None,
                      law: Optional[str] = None, channel="mix", sample_rate: Optional[int] = None, open_end: bool = False,
                      refine: Optional[SegmentRefine] = None, normalize: Optional[float] = None, mode: str = "join", fade_ms: float = 10.0,
                      gap_ms: float = 0.0, shape: str = "linear", wav: bool = True, keep_channels: bool = False, convert=None) -> List:
    """One finished piece of audio per recording: per recording ``(payload, timeline)`` (per channel for ``"split"``, as in
    ``scan_recordings``).  ``mode="join"`` is silence removal: the recording's speech segments (their sample ranges, as
    ``cut_recordings(layout="range")`` cuts them) back to back, each faded in and out over ``fade_ms`` by a ``fade_ramp`` of
    ``shape``; with ``gap_ms == 0`` neighbours overlap by the ramp (by half the shorter segment where that is less) and crossfade,
    with ``gap_ms > 0`` they lie that much silence apart.  ``mode="mask"`` is a VAD-driven noise gate: the output has the
    recording's own length, each segment sits where it was, its edges faded, and every sample outside speech is zero; ranges of a
    recording that touch or overlap are first merged into one.  ``payload``: 16-bit PCM behind a WAV header - of ``sample_rate``
    when given, else ``config.output_wav_sample_rate`` - or, with ``wav=False``, the int16 samples.  ``timeline``:
    ``[(out_start, src_start, nsamples), ...]``, which maps the output back to the recording.  ``fade_ms`` and ``gap_ms`` are
    rounded to a multiple of 4 samples at the payload's rate.  One scan, at most one ``Engine.levels`` call (``normalize``, as in
    ``cut_recordings``: per listed segment - in ``"mask"`` per merged one) and one ``Engine.render`` of the block the scan left
    on the GPU, under ``Engine.scan_session()``: only the finished audio crosses the link back.  ``hop``, ``law``, ``sample_rate``,
    ``open_end`` and ``refine`` as in ``cut_recordings``; on recordings at another rate the samples are the recording's own,
    never gated.  An engine object without ``render``: ``ConfigurationError``.
    ``keep_channels`` as in ``cut_recordings``: the piece of a two-channel recording keeps both channels (``Engine.render_stereo``;
    an engine object without it: ``ConfigurationError``) - a ``[k, 2]`` int16 array or a WAV with a two-channel header; places,
    lengths and the timeline count sample frames and are what they are without it; gain and ramp are the same for both channels.
    ``convert`` as in ``cut_recordings``: the piece is made of the converted signal, at the engine's rate - places, lengths, the
    timeline and ``"mask"``'s length (``Engine.convert_samples`` of the recording's) count converted samples, and the header carries
    ``config.output_wav_sample_rate``."""
    from .pool import default_pool, resolve_model_path
    from .utils.wav_writer import WAVWriter
    who = "render_recordings"
    split = isinstance(channel, str) and channel == "split"
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"{who}: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    if mode not in ("join", "mask"):
        raise ConfigurationError("mode", repr(mode), f"{who}: mode is 'join' or 'mask', got {mode!r}")
    if not (fade_ms >= 0 and gap_ms >= 0):
        raise ConfigurationError("fade_ms", repr((fade_ms, gap_ms)), f"{who}: fade_ms and gap_ms are 0 or more, got {fade_ms!r} and {gap_ms!r}")
    if keep_channels:
        _keep_channels_check(who, split)
    cfg = config or VADConfig()
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    _need_render(engine, who)
    if keep_channels:
        _need_stereo(engine, who, "render_stereo")
    if open_end:
        _need_tails(engine, who)
    if refine is not None:
        _need_refine(engine, who)
    if normalize is not None:
        _need_levels(engine, who, "normalize=")
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError(f"{who} frames at the model's frame size: buffer_size = {cfg.buffer_size}, "
                                 f"the engine's frames have {frame} samples")
    rate = None if sample_rate is None or int(sample_rate) == int(engine.sample_rate) else int(sample_rate)
    conv = _convert_arg(who, engine, sample_rate, convert, split, keep_channels)
    if conv is not None:
        rate = None                                  # downstream the recordings are at the engine's own rate
    if rate is not None:
        if rate not in (8000, 16000, 24000, 48000):
            raise ConfigurationError("sample_rate", repr(sample_rate), f"{who}: recordings at 8000, 16000, 24000 or 48000 Hz, got {sample_rate!r}")
        frame = engine.scan_chunk_samples(rate)      # the ranges count input samples
    hop = frame // 2 if hop is None else int(hop)
    hz = rate if rate is not None else int(engine.sample_rate)
    nramp, gap = int(round(fade_ms * hz / 4000.0)) * 4, int(round(gap_ms * hz / 4000.0)) * 4
    if nramp > _ffi.VAD_RENDER_MAX_RAMP:
        raise ConfigurationError("fade_ms", repr(fade_ms), f"{who}: a fade of {nramp} samples, a ramp has {_ffi.VAD_RENDER_MAX_RAMP} at the most")
    ramp = fade_ramp(nramp, shape)
    recordings = [np.asarray(r) for r in recordings]
    if not recordings:
        return []
    writer = WAVWriter(int(sample_rate) if sample_rate is not None and conv is None else cfg.output_wav_sample_rate, 16, 1)
    # a recording's own length, as "mask" lays it out: of the converted signal under convert=
    own = (lambda r: int(r.shape[0])) if conv is None else (lambda r: max(engine.convert_samples(int(r.shape[0]), conv[0]), 0))
    writer2 = WAVWriter(writer.sample_rate, 16, 2) if keep_channels else None
    denoise = 0.01 if cfg.enable_denoising else None
    out: List = [None] * len(recordings)
    for two in (False, True):
        idx = [i for i, r in enumerate(recordings) if (r.ndim == 2) == two]
        if not idx:
            continue
        per = 2 if two and split else 1
        chans = (0, 1) if per == 2 else (channel if two and conv is None else 0,)
        slots = engine.open_streams(len(idx) * per)
        try:
            engine.set_thresholds_many(slots, (cfg.vad_start_probability, cfg.vad_end_probability, cfg.voice_start_ratio,
                                               cfg.voice_end_ratio, cfg.voice_start_frame_count, cfg.voice_end_frame_count))
            with engine.scan_session():
                ranges = _scan_ranges(engine, slots, [recordings[i] for i in idx], per, frame, hop, law, denoise, channel, rate=rate,
                                      open_end=open_end, refine=refine, convert=conv)
                ranges = [[[(a, b) for a, b, *_ in rg] for rg in rc] for rc in ranges]
                if mode == "mask":
                    # touching or overlapping ranges of one piece (neighbours from a split, small hops) become one, on the same hop grid
                    merged = []
                    for rc in ranges:
                        pieces = []
                        for rg in rc:
                            one: List[Tuple[int, int]] = []
                            for a, b in sorted(rg):
                                if one and a <= one[-1][1]:
                                    one[-1] = (one[-1][0], max(one[-1][1], b))
                                else:
                                    one.append((a, b))
                            pieces.append(one)
                        merged.append(pieces)
                    ranges = merged
                table = _cut_table(engine, ranges, chans, frame, hop)
                # every piece - (recording, channel) - owns a stretch of the one output, a multiple of 4 samples long
                places, lengths, base = [], [], 0
                for k, rc in enumerate(ranges):
                    for rg in rc:
                        counts = [b - a for a, b in rg]
                        if mode == "mask":
                            at, size = [a for a, _ in rg], (own(recordings[idx[k]]) + 3) // 4 * 4
                        else:
                            at = _join_places(counts, nramp, gap)
                            size = at[-1] + counts[-1] if counts else 0
                        places += [base + p for p in at]
                        lengths.append((base, size, at, counts))
                        base += size
                gains = None
                if two and keep_channels:
                    table = [sg[:3] for sg in table]
                    if table and normalize is not None:
                        gains = _joint_gains(engine, table, hop, denoise, normalize)
                    data = engine.render_stereo(table, places, base, hop=hop, ramp=ramp, gains=gains, denoise=denoise)
                else:
                    if table and normalize is not None:
                        peak = engine.levels(table, hop=hop, denoise=denoise)["peak"]
                        usable = np.isfinite(peak) & (peak > 0)
                        gains = np.where(usable, np.float32(normalize) / np.where(usable, peak, np.float32(1)), np.float32(1)).astype(np.float32)
                    data = engine.render(table, places, base, hop=hop, ramp=ramp, gains=gains, denoise=denoise)
        finally:
            for s in slots:
                engine.close_stream(int(s))
        j = 0
        for k, (i, rc) in enumerate(zip(idx, ranges)):
            lists = []
            for rg in rc:
                lo, size, at, counts = lengths[j]
                j += 1
                if mode == "mask":
                    size = own(recordings[i])               # the padding to a multiple of 4 is trimmed
                pcm = data[lo:lo + size]
                timeline = [(p, a, s) for p, (a, _), s in zip(at, rg, counts)]
                if wav:
                    raw = pcm.tobytes()
                    lists.append(((writer2 if two and keep_channels else writer).header(len(raw)) + raw, timeline))
                else:
                    lists.append((pcm.copy(), timeline))
            out[i] = lists if split else lists[0]
    return out


# ---------------------------------------------------------------------------------------------- log-mel features
def _hz_to_mel(f):
    """Slaney's scale (Auditory Toolbox): linear below 1 kHz, 3 mel per 200 Hz; logarithmic above, 27 steps per factor 6.4"""
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), f * (3.0 / 200.0))


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * (200.0 / 3.0))


def mel_filterbank(sample_rate: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """Slaney-style triangular mel filters ``[n_mels, n_fft // 2 + 1]`` as float64.  With ``mel(f) = 3 f / 200`` below 1 kHz and
    ``15 + 27 ln(f / 1000) / ln 6.4`` above, the ``n_mels + 2`` edges ``c_0 .. c_{n_mels + 1}`` are equally spaced in mel between
    ``fmin`` and ``fmax`` (default ``sample_rate / 2``); filter ``j`` at bin frequency ``f_k = k sample_rate / n_fft`` is

        ``w_j[k] = 2 / (c_{j+2} - c_j) * max(0, min((f_k - c_j) / (c_{j+1} - c_j), (c_{j+2} - f_k) / (c_{j+2} - c_{j+1})))``

    - one triangle from ``c_j`` up to 1 at ``c_{j+1}`` and down to ``c_{j+2}``, scaled by ``2 / (c_{j+2} - c_j)`` so that the
    CONTINUOUS triangle has area 1 in Hz ("area normalisation": a flat spectrum gives roughly the same energy in every band).  The
    sampled row sums to about ``n_fft / sample_rate`` (the area over the bin spacing) where the triangle spans several bins."""
    sample_rate, n_fft, n_mels = int(sample_rate), int(n_fft), int(n_mels)
    fmax = sample_rate / 2.0 if fmax is None else float(fmax)
    if not (0.0 <= float(fmin) < fmax <= sample_rate / 2.0) or n_mels < 1:
        raise ConfigurationError("fmin", repr((fmin, fmax, n_mels)), f"mel_filterbank: 0 <= fmin < fmax <= sample_rate / 2 and n_mels >= 1, got "
                                 f"fmin = {fmin}, fmax = {fmax}, n_mels = {n_mels}")
    c = _mel_to_hz(np.linspace(_hz_to_mel(float(fmin)), _hz_to_mel(fmax), n_mels + 2))
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / float(n_fft))
    up = (f[None, :] - c[:-2, None]) / (c[1:-1] - c[:-2])[:, None]
    down = (c[2:, None] - f[None, :]) / (c[2:] - c[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down)) * (2.0 / (c[2:] - c[:-2]))[:, None]


@dataclass(frozen=True)
class MelSpec:
    """A log-mel front end for ``Engine.mel`` / ``features_recordings``: frames of ``n_fft`` samples every ``hop``, a periodic
    ``window`` (``"hann"`` or ``"rect"``), ``pad`` ``"reflect"`` (``torch.stft(center=True)``) or ``"none"``, the power spectrum
    through ``mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax)``, then ``log`` ``"log10"``, ``"ln"`` or ``"linear"`` of
    ``max(E, floor)``.  The defaults are Whisper's geometry at 16 kHz; its two remaining lines are the caller's, per clip::

        x = np.maximum(features, features.max() - 8.0)
        x = (x + 4.0) / 4.0
    """
    sample_rate: int
    n_fft: int = 400
    hop: int = 160
    n_mels: int = 80
    fmin: float = 0.0
    fmax: Optional[float] = None
    window: str = "hann"
    pad: str = "reflect"
    log: str = "log10"
    floor: float = 1e-10

    def operators(self):
        """-> ``(fields, op_re, op_im, filters)`` as ``Engine.mel`` takes them: ``fields`` the ``vad_mel`` fields as a dict,
        ``op_re[n][k] = w[n] cos(2 pi ((n k) mod n_fft) / n_fft)``, ``op_im[n][k] = -w[n] sin(...)`` with the periodic window
        ``w[n] = 0.5 - 0.5 cos(2 pi n / n_fft)`` - the angle reduced in integers, everything in float64, rounded once to float32."""
        if self.window not in ("hann", "rect"):
            raise ConfigurationError("window", repr(self.window), f"MelSpec: window is 'hann' or 'rect', got {self.window!r}")
        if self.pad not in _ffi.MEL_PADS or self.log not in _ffi.MEL_LOGS:
            raise ConfigurationError("pad", repr((self.pad, self.log)), f"MelSpec: pad is one of {sorted(_ffi.MEL_PADS)} and log one of "
                                     f"{sorted(_ffi.MEL_LOGS)}, got {self.pad!r}, {self.log!r}")
        n_fft, n_bins = int(self.n_fft), int(self.n_fft) // 2 + 1
        n = np.arange(n_fft, dtype=np.int64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft) if self.window == "hann" else np.ones(n_fft)
        ang = 2.0 * np.pi * ((n[:, None] * np.arange(n_bins, dtype=np.int64)[None, :]) % n_fft).astype(np.float64) / n_fft
        filters = mel_filterbank(self.sample_rate, n_fft, self.n_mels, self.fmin, self.fmax)
        fields = {"n_fft": n_fft, "hop": int(self.hop), "n_bins": n_bins, "n_mels": int(self.n_mels), "pad": self.pad, "log": self.log,
                  "floor": float(self.floor)}
        return fields, (w[:, None] * np.cos(ang)).astype(np.float32), (-w[:, None] * np.sin(ang)).astype(np.float32), filters.astype(np.float32)


def _need_mel(engine, who: str) -> None:
    if not hasattr(engine, "mel"):
        raise ConfigurationError("mel", "given", f"{who} needs an engine with mel (the features are computed from the block a scan left "
                                 f"on the GPU), {type(engine).__name__} has none")


def features_recordings(recordings: Sequence[np.ndarray], spec: MelSpec, config: Optional[VADConfig] = None, engine=None,
                        hop: Optional[int] = None, law: Optional[str] = None, channel="mix", open_end: bool = False,
                        refine: Optional[SegmentRefine] = None, sample_rate: Optional[int] = None, taps=None, convert=None, project=None) -> List:
    """``scan_recordings`` with each finished segment's log-mel frames: per recording ``[(start_sample, end_sample,
    features [M, n_mels] float32), ...]`` (per channel for ``"split"``, as there).  The features are those of the samples
    ``cut_recordings(layout="range")`` cuts - decoded, mixed and gated as the model read them - computed on the GPU from the block
    the scan left there (one scan and one ``Engine.mel(audio=None)`` under ``Engine.scan_session()``; two of each for a corpus of 1-D
    and 2-D recordings): no sample crosses the link back.  ``hop`` is the scan's; the analysis hop is ``spec.hop``.
    ``open_end`` and ``refine`` as in ``scan_recordings``.  An engine object without ``mel``: ``ConfigurationError``; so is a
    ``spec.sample_rate`` other than the engine's.
    ``sample_rate``: the recordings are at 8000, 24000 or 48000 Hz - the scan is the rate scan, ``hop`` and the ranges count
    INPUT-rate samples, and the features are those of each segment's 16 kHz signal (``Engine.mel(sample_rate=..., taps=...)``:
    ``Engine.resample_cut``'s samples, never gated), so ``spec.sample_rate`` is still the engine's.  ``taps`` as in
    ``Engine.resample_cut``.  An engine object without ``resample_cut``: ``ConfigurationError``.
    ``convert`` as in ``scan_recordings``: recordings at any rate ``Engine.convert`` accepts, converted once; the ranges count converted
    samples and the features are those of the converted signal, gated as the model read it (``Engine.mel(audio=None)``; ``taps`` is
    not used).
    ``project``: a ``CepstralSpec`` or an ``(op, bias)`` pair - the features are ``[M, n_out]``, each row of the log-mel matrix through
    ``Engine.mel_project`` on the GPU (MFCC, LFCC, PCA ...): ``Engine.mel_keep``, the projection in place of the resident matrix, and
    ``Engine.mel_resident_read`` instead of ``Engine.mel``.  An engine object without ``mel_project``: ``ConfigurationError``."""
    from .pool import default_pool, resolve_model_path
    who = "features_recordings"
    split = isinstance(channel, str) and channel == "split"
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"{who}: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    cfg = config or VADConfig()
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    _need_mel(engine, who)
    if open_end:
        _need_tails(engine, who)
    if refine is not None:
        _need_refine(engine, who)
    if int(spec.sample_rate) != int(engine.sample_rate):
        raise ConfigurationError("sample_rate", repr(spec.sample_rate), f"{who}: the spec is for {spec.sample_rate} Hz, the engine's blocks "
                                 f"are at {engine.sample_rate} Hz")
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError(f"{who} frames at the model's frame size: buffer_size = {cfg.buffer_size}, the engine's frames have "
                                 f"{frame} samples")
    rate = None if sample_rate is None or int(sample_rate) == int(engine.sample_rate) else int(sample_rate)
    conv = _convert_arg(who, engine, sample_rate, convert, split)
    if conv is not None:
        rate = None                                  # downstream the recordings are at the engine's own rate
    mel_kw = {}
    if rate is not None:
        if rate not in (8000, 24000, 48000):
            raise ConfigurationError("sample_rate", repr(sample_rate), f"{who}: recordings at 8000, 16000, 24000 or 48000 Hz, got {sample_rate!r}")
        _need_resample(engine, who, "sample_rate=")
        frame = engine.scan_chunk_samples(rate)      # the ranges count input samples
        mel_kw = {"sample_rate": rate, "taps": taps}
    hop = frame // 2 if hop is None else int(hop)
    recordings = [np.asarray(r) for r in recordings]
    if not recordings:
        return []
    arrays = spec.operators()
    proj = _project_arg(who, engine, project, int(arrays[0]["n_mels"]))
    denoise = 0.01 if cfg.enable_denoising else None
    out: List = [None] * len(recordings)
    for two in (False, True):
        idx = [i for i, r in enumerate(recordings) if (r.ndim == 2) == two]
        if not idx:
            continue
        per = 2 if two and split else 1
        chans = (0, 1) if per == 2 else (channel if two and conv is None else 0,)
        slots = engine.open_streams(len(idx) * per)
        try:
            engine.set_thresholds_many(slots, _thresholds_of(cfg))
            with engine.scan_session():
                ranges = _scan_ranges(engine, slots, [recordings[i] for i in idx], per, frame, hop, law, denoise, channel, rate=rate,
                                      open_end=open_end, refine=refine, convert=conv)
                table = _cut_table(engine, ranges, chans, frame, hop)
                if table and proj is None:
                    data, start = engine.mel(table, arrays, hop=hop, denoise=denoise, **mel_kw)
                elif table:
                    start = engine.mel_keep(table, arrays, hop=hop, denoise=denoise, **mel_kw)
                    engine.mel_project(proj[0], proj[1], out=False)
                    data = engine.mel_resident_read()
        finally:
            for s in slots:
                engine.close_stream(int(s))
        j = 0
        for i, rc in zip(idx, ranges):
            lists = []
            for rg in rc:
                one = []
                for a, b, *_ in rg:
                    one.append((a, b, data[start[j]:start[j + 1]].copy()))
                    j += 1
                lists.append(one)
            out[i] = lists if split else lists[0]
    return out


@dataclass(frozen=True)
class FeatureBatch:
    """What a model takes of a corpus's log-mel features, for ``batch_recordings`` / ``Engine.mel_batch``: windows of ``frames`` rows
    every ``stride`` rows of each segment (``stride=None``: ``frames``; ``frames=None``: one window per segment, as long as the longest
    segment rounded up to a multiple of 4), normalised per SEGMENT by ``norm`` - ``"none"``, ``"whisper"`` (``max(x, max - 8)``, then
    ``(x + 4) / 4``), ``"cmn"`` (the band's mean taken off) or ``"cmvn"`` (and divided by ``max(std, eps)``) - with ``deltas`` 0, 1 or
    2 orders of differences appended, laid out ``"channel"`` [B, C, T] or ``"time"`` [B, T, C] as ``dtype`` ``"f32"``, ``"f16"`` or
    ``"bf16"`` (bit patterns as uint16).  Frames past a segment's end are ``pad_value`` as it is (``pad="value"``) or ``pad_value``
    through the segment's normalisation (``pad="feature"``: a frame of silence).  Whisper's setting, with ``MelSpec``'s defaults::

        FeatureBatch(frames=3000, norm="whisper", pad="feature", pad_value=-10.0)

    ``pack=True`` lays the segments of a recording (and channel) back to back, ``gap`` frames of padding apart, in as few windows
    of ``frames`` rows as hold them (``batch_pack``), and normalises per WINDOW: Whisper's ``max - 8`` is a property of the 30 s
    window.  ``scope`` names what the statistics of ``norm`` run over: ``None`` is ``"segment"`` unpacked and ``"window"`` packed;
    ``"recording"`` (all segments of a recording and channel, the usual scope of CMVN for speaker models) goes with either.
    """
    frames: Optional[int] = None
    stride: Optional[int] = None
    norm: str = "none"
    eps: float = 1e-5
    deltas: int = 0
    layout: str = "channel"
    dtype: str = "f32"
    pad: str = "value"
    pad_value: float = 0.0
    pack: bool = False
    gap: int = 0
    scope: Optional[str] = None

    def check(self) -> None:
        if self.norm not in ("none", "whisper", "cmn", "cmvn"):
            raise ConfigurationError("norm", repr(self.norm), f"FeatureBatch: norm is 'none', 'whisper', 'cmn' or 'cmvn', got {self.norm!r}")
        if self.layout not in _ffi.BATCH_LAYOUTS or self.dtype not in _ffi.BATCH_DTYPES or self.pad not in _ffi.BATCH_PADS:
            raise ConfigurationError("layout", repr((self.layout, self.dtype, self.pad)), f"FeatureBatch: layout is one of {sorted(_ffi.BATCH_LAYOUTS)}, "
                                     f"dtype one of {sorted(_ffi.BATCH_DTYPES)}, pad one of {sorted(_ffi.BATCH_PADS)}, got {self.layout!r}, "
                                     f"{self.dtype!r}, {self.pad!r}")
        if self.frames is not None and (int(self.frames) < 4 or int(self.frames) > 65536 or int(self.frames) % 4):
            raise ConfigurationError("frames", repr(self.frames), f"FeatureBatch: frames is a multiple of 4 from 4 to 65536, got {self.frames!r}")
        if self.stride is not None and int(self.stride) < 1:
            raise ConfigurationError("stride", repr(self.stride), f"FeatureBatch: stride is 1 or more, got {self.stride!r}")
        if int(self.deltas) not in (0, 1, 2):
            raise ConfigurationError("deltas", repr(self.deltas), f"FeatureBatch: deltas is 0, 1 or 2, got {self.deltas!r}")
        if self.scope not in (None, "segment", "window", "recording"):
            raise ConfigurationError("scope", repr(self.scope), f"FeatureBatch: scope is None, 'segment', 'window' or 'recording', got {self.scope!r}")
        if self.pack:
            if self.frames is None or self.stride is not None or self.scope == "segment":
                raise ConfigurationError("pack", "True", "FeatureBatch: pack=True takes a number of frames, no stride, and scope 'window' or "
                                         f"'recording', got frames={self.frames!r}, stride={self.stride!r}, scope={self.scope!r}")
            if int(self.gap) < 0 or int(self.gap) > int(self.frames):
                raise ConfigurationError("gap", repr(self.gap), f"FeatureBatch: gap is 0 .. frames = {self.frames}, got {self.gap!r}")
        elif self.scope == "window":
            raise ConfigurationError("scope", repr(self.scope), "FeatureBatch: scope='window' goes with pack=True; unpacked windows are normalised per "
                                     "'segment' or 'recording'")

    def record(self, n_mels: int) -> dict:
        """-> ``vad_batch``'s fields as ``Engine.mel_batch`` takes them (``frames`` must be set)"""
        self.check()
        if self.frames is None:
            raise ConfigurationError("frames", "None", "FeatureBatch: frames=None is resolved by batch_windows; Engine.mel_batch takes a number")
        return {"n_mels": int(n_mels), "frames": int(self.frames), "deltas": int(self.deltas), "layout": self.layout, "dtype": self.dtype,
                "pad": self.pad, "pad_value": float(self.pad_value)}


def batch_windows(start, frames: Optional[int] = None, stride: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """The windows of segments whose first rows are ``start`` [n + 1] -> (windows, T): per segment of M rows one window at ``row0 = 0,
    stride, 2 * stride, ...`` while ``row0 < M``, each of ``min(frames, M - row0)`` rows, as a ``(seg, nrows, row0)`` record array
    ``Engine.mel_batch`` takes.  ``stride=None``: ``frames``.  ``frames=None``: one window per segment (also one without rows) and T the
    longest segment rounded up to a multiple of 4 (4 at the least)."""
    start = np.asarray(start, np.int64).reshape(-1)
    M = np.diff(start)
    if start.size < 1 or (M < 0).any():
        raise ConfigurationError("start", repr(start[:8].tolist()), "batch_windows: start has n + 1 ascending entries")
    if frames is None:
        T = max(4, -(-int(M.max(initial=0)) // 4) * 4)
        if T > 65536:
            raise ConfigurationError("frames", "None", f"batch_windows: the longest segment has {int(M.max())} rows, a window 65536 at the most: give frames")
        w = np.zeros(M.size, _ffi.BATCH_WINDOW_DTYPE)
        w["seg"], w["nrows"] = np.arange(M.size), M
        return w, T
    T = int(frames)
    step = T if stride is None else int(stride)
    if T < 4 or T > 65536 or T % 4 or step < 1:
        raise ConfigurationError("frames", repr((frames, stride)), f"batch_windows: frames is a multiple of 4 from 4 to 65536 and stride 1 or more, "
                                 f"got {frames!r} and {stride!r}")
    rec = [(i, min(T, int(m) - r), r) for i, m in enumerate(M) for r in range(0, int(m), step)]
    return np.array(rec, _ffi.BATCH_WINDOW_DTYPE).reshape(-1), T


def batch_pack(start, frames: int, gap: int = 0, group=None) -> Tuple[np.ndarray, int]:
    """Several segments per window (``vad_mel_pack_plan``; ``include/vad_engine.h`` has the rule): the segments whose first rows are
    ``start`` [n + 1], in order, each in pieces of at most ``frames`` rows, a piece behind the window's last one at the next multiple
    of 4 past ``gap`` frames, or at frame 0 of a new window where it does not fit or its ``group`` [n] differs -> (pieces, nw):
    ``(seg, nrows, row0, window, offset)`` records as ``Engine.mel_batch_packed`` takes them, and the number of windows.  The
    pieces tile the rows in order: ``start[0] + cumsum(nrows)`` are their bounds."""
    st = np.ascontiguousarray(np.asarray(start, np.int64).reshape(-1))
    gr = None if group is None else np.ascontiguousarray(np.asarray(group, np.int32).reshape(-1))
    if st.size < 1 or (gr is not None and gr.size != st.size - 1):
        raise ConfigurationError("start", repr(st[:8].tolist()), "batch_pack: start has n + 1 entries and group n")
    lib = _ffi.lib()
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    gp = None if gr is None else (gr if gr.size else np.zeros(1, np.int32)).ctypes.data_as(i32p)
    np_, nw = C.c_int64(0), C.c_int64(0)
    head = (st.ctypes.data_as(i64p), st.size - 1, gp, int(frames), int(gap))
    rc = lib.vad_mel_pack_plan(*head, None, 0, C.byref(np_), C.byref(nw))
    pieces = np.zeros(max(int(np_.value), 0), _ffi.BATCH_PIECE_DTYPE)
    if rc == 0 and pieces.size:
        rc = lib.vad_mel_pack_plan(*head, pieces.ctypes.data_as(C.POINTER(_ffi.BatchPiece)), pieces.size, C.byref(np_), C.byref(nw))
    if rc != 0:
        raise ConfigurationError("frames", repr((frames, gap)), "batch_pack: frames is a multiple of 4 from 4 to 65536, gap 0 .. frames and start "
                                 f"ascends, got frames={frames!r}, gap={gap!r}, start={st[:8].tolist()}")
    return pieces, int(nw.value)


def batch_affine(stats: Optional[dict], start, norm: str = "none", eps: float = 1e-5):
    """``Engine.mel_stats``'s result -> ``(lo, shift, scale)`` as ``Engine.mel_batch`` takes them, for ``norm``: ``"none"``: three
    ``None``; ``"whisper"``: ``lo = float32(max) - float32(8)`` per segment, ``shift`` 4, ``scale`` 0.25; ``"cmn"``: ``shift = -mean``
    per segment and band; ``"cmvn"``: also ``scale = 1 / max(std, eps)`` - ``mean = sum / (4096 M)``, ``var = max(sumsq / (2^24 M) -
    mean^2, 0)``, in float64, rounded to float32 once.  A segment without rows gets 0 and 1 (and ``lo`` -inf)."""
    if norm == "none":
        return None, None, None
    if norm == "whisper":
        return np.asarray(stats["max"], np.float32) - np.float32(8.0), np.float32(4.0), np.float32(0.25)
    if norm not in ("cmn", "cmvn"):
        raise ConfigurationError("norm", repr(norm), f"batch_affine: norm is 'none', 'whisper', 'cmn' or 'cmvn', got {norm!r}")
    M = np.diff(np.asarray(start, np.int64).reshape(-1)).astype(np.float64)[:, None]
    some = M > 0
    Ms = np.where(some, M, 1.0)
    mean = np.where(some, np.asarray(stats["sum"]).astype(np.float64) / (4096.0 * Ms), 0.0)
    shift = (-mean).astype(np.float32)
    if norm == "cmn":
        return None, shift, None
    var = np.maximum(np.asarray(stats["sumsq"]).astype(np.float64) / (16777216.0 * Ms) - mean * mean, 0.0)
    scale = np.where(some, 1.0 / np.maximum(np.sqrt(var), float(eps)), 1.0).astype(np.float32)
    return None, shift, scale


def _dct64(n_in: int, n_out: int, norm, first: int) -> np.ndarray:
    n_in, n_out, first = int(n_in), int(n_out), int(first)
    if norm not in ("ortho", None) or n_in < 1 or n_out < 1 or first < 0 or first + n_out > n_in:
        raise ConfigurationError("norm", repr((n_in, n_out, norm, first)), "dct_operator: norm is 'ortho' or None, n_in and n_out are 1 or more, and "
                                 f"coefficients first .. first + n_out - 1 lie below n_in, got n_in={n_in}, n_out={n_out}, norm={norm!r}, first={first}")
    m = np.arange(n_in, dtype=np.int64)[:, None]
    c = np.arange(first, first + n_out, dtype=np.int64)[None, :]
    w = np.cos(np.pi * ((c * (2 * m + 1)) % (4 * n_in)).astype(np.float64) / (2.0 * n_in))
    if norm == "ortho":
        return w * np.where(c == 0, np.sqrt(1.0 / n_in), np.sqrt(2.0 / n_in))
    return 2.0 * w


def dct_operator(n_in: int, n_out: int, norm="ortho", first: int = 0) -> np.ndarray:
    """The DCT-II as an operator ``Engine.mel_project`` takes -> float32 [n_in, n_out]: column ``j`` is coefficient ``c = first + j``,
    ``op[m][j] = s_c cos(pi c (2 m + 1) / (2 n_in))`` - the angle reduced in integers mod ``4 n_in``, everything in float64, rounded
    once.  ``norm="ortho"``: ``s_0 = sqrt(1 / n_in)``, ``s_c = sqrt(2 / n_in)`` (Kaldi, ``scipy.fft.dct(norm="ortho")``, librosa,
    torchaudio); ``None``: ``s_c = 2`` (``scipy.fft.dct``'s default).  ``first=1`` drops c0."""
    return _dct64(n_in, n_out, norm, first).astype(np.float32)


@dataclass(frozen=True)
class CepstralSpec:
    """Cepstral coefficients of log-band features, for ``Engine.mel_project`` and ``features_recordings`` / ``batch_recordings(project=)``:
    coefficients ``first .. first + n_ceps - 1`` of the DCT-II (``dct_operator``'s ``norm``), each times the sine lifter
    ``1 + (lifter / 2) sin(pi (c + lifter_offset) / lifter)`` (``lifter=0``: none; ``lifter=22``: HTK and Kaldi; ``lifter_offset=1``:
    librosa's) and times ``scale`` (10 turns ``MelSpec(log="log10")`` into dB).  Over ``MelSpec``'s mel bands that is MFCC, over
    linear bands LFCC."""
    n_ceps: int = 13
    lifter: float = 0
    lifter_offset: int = 0
    scale: float = 1.0
    norm: Optional[str] = "ortho"
    first: int = 0

    def operator(self, n_mels: int):
        """-> ``(op float32 [n_mels, n_ceps], bias float32 [n_ceps] of zeros)``: lifter and scale folded into the DCT in float64,
        rounded once"""
        w = _dct64(n_mels, self.n_ceps, self.norm, self.first)
        if not np.isfinite(float(self.scale)) or float(self.lifter) < 0:
            raise ConfigurationError("lifter", repr((self.lifter, self.scale)), f"CepstralSpec: lifter is 0 or more and scale finite, got "
                                     f"{self.lifter!r}, {self.scale!r}")
        lift = np.ones(int(self.n_ceps))
        if float(self.lifter) > 0:
            c = np.arange(int(self.first), int(self.first) + int(self.n_ceps), dtype=np.float64) + int(self.lifter_offset)
            lift = 1.0 + 0.5 * float(self.lifter) * np.sin(np.pi * c / float(self.lifter))
        return (w * (lift * float(self.scale))[None, :]).astype(np.float32), np.zeros(int(self.n_ceps), np.float32)


def _need_project(engine, who: str) -> None:
    if not hasattr(engine, "mel_project") or not hasattr(engine, "mel_keep"):
        raise ConfigurationError("project", "given", f"{who}: project= needs an engine with mel_keep and mel_project (the features are projected "
                                 f"where the scan left them, on the GPU), {type(engine).__name__} has none")


def _project_arg(who: str, engine, project, n_mels: int):
    """``project``: None, a ``CepstralSpec`` or an ``(op, bias)`` pair -> None or (op float32 [n_mels, n_out], bias or None)"""
    if project is None:
        return None
    _need_project(engine, who)
    op, bias = project.operator(n_mels) if hasattr(project, "operator") else project
    op = np.ascontiguousarray(np.asarray(op, np.float32))
    if op.ndim != 2 or op.shape[0] != n_mels or not 1 <= op.shape[1] <= 128:
        raise ConfigurationError("project", repr(op.shape), f"{who}: project's operator is [n_mels = {n_mels}, 1 .. 128], got {op.shape}")
    return op, bias


def _need_batch(engine, who: str) -> None:
    if not hasattr(engine, "mel_batch"):
        raise ConfigurationError("batch", "given", f"{who} needs an engine with mel_batch (the windows are normalised and laid out from the "
                                 f"features a scan left on the GPU), {type(engine).__name__} has none")


def _need_pack(engine, who: str, what: str) -> None:
    if not hasattr(engine, "mel_batch_packed"):
        raise ConfigurationError("batch", "given", f"{who}: {what} needs an engine with mel_batch_packed and grouped mel_stats, "
                                 f"{type(engine).__name__} has none")


def _expand_affine(affine, which):
    """(lo, shift, scale) of groups -> of the segments or windows whose groups are ``which``; scalars and ``None`` stay"""
    return tuple(a if a is None or np.ndim(a) == 0 else np.asarray(a)[which] for a in affine)


def batch_recordings(recordings: Sequence[np.ndarray], spec: MelSpec, batch: FeatureBatch, config: Optional[VADConfig] = None, engine=None,
                     hop: Optional[int] = None, law: Optional[str] = None, channel="mix", open_end: bool = False,
                     refine: Optional[SegmentRefine] = None, sample_rate: Optional[int] = None, taps=None, convert=None, project=None):
    """``features_recordings`` as the tensor a model takes: the log-mel features of every finished segment of every recording,
    windowed, normalised, padded, laid out and converted as ``batch`` says -> ``(array, index)``: ``array`` [B, C, T] or [B, T, C]
    (``Engine.mel_batch``), ``index`` one ``(recording, channel, start_sample, end_sample, first_frame, nframes)`` per window - the
    segment it shows (samples of the recording, at its own rate), the window's first row in the segment and its rows.  One scan, one
    ``Engine.mel_keep``, at most one ``Engine.mel_stats`` and one ``Engine.mel_batch`` under ``Engine.scan_session()``: the features
    never leave the GPU, only the statistics and the batch cross the link.  The other arguments as in ``features_recordings``.  A
    corpus of 1-D and 2-D recordings is a ``ConfigurationError``: call it once per kind.  So is an engine object without
    ``mel_batch``.  No segment anywhere: an array with B = 0.  ``convert`` as in ``features_recordings``.

    ``batch.pack``: the segments of each (recording, channel) packed into windows (``batch_pack``): one scan, one keep, one grouped
    ``Engine.mel_stats`` and one ``Engine.mel_batch_packed``.  ``array`` has a window per row of B, ``index`` one ``(recording,
    channel, start_sample, end_sample, first_frame, nframes, window, offset)`` per PIECE.  ``batch.scope="recording"``, packed or
    not, normalises with the statistics of all segments of the (recording, channel).

    ``project`` as in ``features_recordings``: one ``Engine.mel_project`` behind the keep replaces the resident matrix by its
    projection, and the statistics, the windows and C = n_out * (deltas + 1) are those of the projected features."""
    from .pool import default_pool, resolve_model_path
    who = "batch_recordings"
    batch.check()
    by_recording = batch.scope == "recording"
    split = isinstance(channel, str) and channel == "split"
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"{who}: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    cfg = config or VADConfig()
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    _need_mel(engine, who)
    _need_batch(engine, who)
    if batch.pack or by_recording:
        _need_pack(engine, who, "pack=True" if batch.pack else "scope='recording'")
    if open_end:
        _need_tails(engine, who)
    if refine is not None:
        _need_refine(engine, who)
    if int(spec.sample_rate) != int(engine.sample_rate):
        raise ConfigurationError("sample_rate", repr(spec.sample_rate), f"{who}: the spec is for {spec.sample_rate} Hz, the engine's blocks "
                                 f"are at {engine.sample_rate} Hz")
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError(f"{who} frames at the model's frame size: buffer_size = {cfg.buffer_size}, the engine's frames have "
                                 f"{frame} samples")
    rate = None if sample_rate is None or int(sample_rate) == int(engine.sample_rate) else int(sample_rate)
    conv = _convert_arg(who, engine, sample_rate, convert, split)
    if conv is not None:
        rate = None                                  # downstream the recordings are at the engine's own rate
    mel_kw = {}
    if rate is not None:
        if rate not in (8000, 24000, 48000):
            raise ConfigurationError("sample_rate", repr(sample_rate), f"{who}: recordings at 8000, 16000, 24000 or 48000 Hz, got {sample_rate!r}")
        _need_resample(engine, who, "sample_rate=")
        frame = engine.scan_chunk_samples(rate)      # the ranges count input samples
        mel_kw = {"sample_rate": rate, "taps": taps}
    hop = frame // 2 if hop is None else int(hop)
    recordings = [np.asarray(r) for r in recordings]
    kinds = {r.ndim == 2 for r in recordings}
    if len(kinds) > 1:
        raise ConfigurationError("recordings", "1-D and 2-D", f"{who}: one batch holds recordings of one kind; call it once for the 1-D and once "
                                 "for the two-channel recordings")
    arrays = spec.operators()
    n_mels = int(arrays[0]["n_mels"])
    proj = _project_arg(who, engine, project, n_mels)
    if proj is not None:
        n_mels = int(proj[0].shape[1])               # downstream the features are the projected ones
    chans_out = n_mels * (int(batch.deltas) + 1)
    np_dtype = {"f32": np.float32, "f16": np.float16}.get(batch.dtype, np.uint16)
    T0 = int(batch.frames) if batch.frames is not None else 4
    empty = np.empty((0, chans_out, T0) if batch.layout == "channel" else (0, T0, chans_out), np_dtype)
    if not recordings:
        return empty, []
    two = kinds.pop()
    denoise = 0.01 if cfg.enable_denoising else None
    per = 2 if two and split else 1
    chans = (0, 1) if per == 2 else (channel if two and conv is None else 0,)
    slots = engine.open_streams(len(recordings) * per)
    out = None
    try:
        engine.set_thresholds_many(slots, _thresholds_of(cfg))
        with engine.scan_session():
            ranges = _scan_ranges(engine, slots, recordings, per, frame, hop, law, denoise, channel, rate=rate, open_end=open_end, refine=refine,
                                  convert=conv)
            table = _cut_table(engine, ranges, chans, frame, hop)
            if table:
                start = engine.mel_keep(table, arrays, hop=hop, denoise=denoise, **mel_kw)
                if proj is not None:
                    engine.mel_project(proj[0], proj[1], out=False)
                moments = batch.norm != "whisper"
                # the group of a segment: its (recording, channel), numbered in the table's order
                group = np.array([i * per + c for i, rc in enumerate(ranges) for c, rg in enumerate(rc) for _ in rg], np.int32)
                ngroups = len(recordings) * per
                rows_of = lambda which, count: np.concatenate([[0], np.cumsum(np.bincount(which, weights=np.diff(start), minlength=count))]).astype(np.int64)
                if batch.pack:
                    windows, nw = batch_pack(start, batch.frames, batch.gap, group)
                    T = int(batch.frames)
                    if batch.norm == "none":
                        affine = (None, None, None)
                    elif by_recording:
                        stats = engine.mel_stats(moments=moments, group=(group, ngroups))
                        wgroup = np.zeros(nw, np.int64)
                        wgroup[windows["window"]] = group[windows["seg"]]
                        affine = _expand_affine(batch_affine(stats, rows_of(group, ngroups), batch.norm, batch.eps), wgroup)
                    else:
                        bounds = np.concatenate([[0], np.cumsum(windows["nrows"], dtype=np.int64)]) + start[0]
                        stats = engine.mel_stats(start=bounds, moments=moments, group=(windows["window"], nw))
                        wrows = np.concatenate([[0], np.cumsum(np.bincount(windows["window"], weights=windows["nrows"], minlength=nw))]).astype(np.int64)
                        affine = batch_affine(stats, wrows, batch.norm, batch.eps)
                    lo, shift, scale = affine
                    out = engine.mel_batch_packed(windows, nw, batch.record(n_mels), lo=lo, shift=shift, scale=scale)
                else:
                    windows, T = batch_windows(start, batch.frames, batch.stride)
                    if batch.norm == "none":
                        lo, shift, scale = None, None, None
                    elif by_recording:
                        stats = engine.mel_stats(moments=moments, group=(group, ngroups))
                        lo, shift, scale = _expand_affine(batch_affine(stats, rows_of(group, ngroups), batch.norm, batch.eps), group)
                    else:
                        lo, shift, scale = batch_affine(engine.mel_stats(moments=moments), start, batch.norm, batch.eps)
                    rec = replace(batch, frames=T).record(n_mels)
                    out = engine.mel_batch(windows, rec, lo=lo, shift=shift, scale=scale)
    finally:
        for s in slots:
            engine.close_stream(int(s))
    if out is None:
        return empty, []
    where = [(i, chans[c], a, b) for i, rc in enumerate(ranges) for c, rg in enumerate(rc) for a, b, *_ in rg]
    if batch.pack:
        return out, [where[int(w["seg"])] + (int(w["row0"]), int(w["nrows"]), int(w["window"]), int(w["offset"])) for w in windows]
    index = [where[int(w["seg"])] + (int(w["row0"]), int(w["nrows"])) for w in windows]
    return out, index


@dataclass(frozen=True)
class AudioBatch:
    """What a model that takes the waveform itself is fed, for ``audio_recordings`` / ``Engine.audio_batch``: windows of ``samples``
    samples every ``stride`` samples of each segment (``stride=None``: ``samples``; ``samples=None``: one window per segment, as long
    as the longest segment rounded up to a multiple of 4), normalised by ``norm`` - ``"none"``, ``"mean"`` (the mean taken off),
    ``"zscore"`` (and divided by ``sqrt(var + eps)``: wav2vec 2.0's feature extractor) or ``"peak"`` (times ``target / peak``:
    ``AudioUtils.normalize_audio``) - with the statistics of the ``scope``: the ``"segment"``, or all segments of the
    ``"recording"`` (and channel).  ``dtype`` is ``"f32"``, ``"f16"`` or ``"bf16"`` (bit patterns as uint16).  Samples past a
    segment's end are ``pad_value`` as it is (``pad="value"``) or silence through the normalisation (``pad="feature"``).  wav2vec
    2.0's setting::

        AudioBatch(norm="zscore", eps=1e-7)
    """
    samples: Optional[int] = None
    stride: Optional[int] = None
    norm: str = "none"
    eps: float = 1e-7
    target: float = 0.9
    scope: str = "segment"
    dtype: str = "f32"
    pad: str = "value"
    pad_value: float = 0.0

    def check(self) -> None:
        if self.norm not in ("none", "mean", "zscore", "peak"):
            raise ConfigurationError("norm", repr(self.norm), f"AudioBatch: norm is 'none', 'mean', 'zscore' or 'peak', got {self.norm!r}")
        if self.dtype not in _ffi.BATCH_DTYPES or self.pad not in _ffi.BATCH_PADS:
            raise ConfigurationError("dtype", repr((self.dtype, self.pad)), f"AudioBatch: dtype is one of {sorted(_ffi.BATCH_DTYPES)}, pad one of "
                                     f"{sorted(_ffi.BATCH_PADS)}, got {self.dtype!r}, {self.pad!r}")
        if self.samples is not None and (int(self.samples) < 4 or int(self.samples) > 1 << 24 or int(self.samples) % 4):
            raise ConfigurationError("samples", repr(self.samples), f"AudioBatch: samples is a multiple of 4 from 4 to 2^24, got {self.samples!r}")
        if self.stride is not None and (int(self.stride) < 4 or int(self.stride) % 4):
            raise ConfigurationError("stride", repr(self.stride), f"AudioBatch: stride is a multiple of 4, 4 or more, got {self.stride!r}")
        if self.scope not in ("segment", "recording"):
            raise ConfigurationError("scope", repr(self.scope), f"AudioBatch: scope is 'segment' or 'recording', got {self.scope!r}")
        if not (np.isfinite(self.eps) and float(self.eps) >= 0):
            raise ConfigurationError("eps", repr(self.eps), f"AudioBatch: eps is a finite number, 0 or more, got {self.eps!r}")
        if not (np.isfinite(self.target) and float(self.target) > 0):
            raise ConfigurationError("target", repr(self.target), f"AudioBatch: target is a finite number above 0, got {self.target!r}")
        if not np.isfinite(self.pad_value):
            raise ConfigurationError("pad_value", repr(self.pad_value), f"AudioBatch: pad_value is a finite number, got {self.pad_value!r}")

    def record(self) -> dict:
        """-> ``vad_audio_batch``'s fields as ``Engine.audio_batch`` takes them (``samples`` must be set)"""
        self.check()
        if self.samples is None:
            raise ConfigurationError("samples", "None", "AudioBatch: samples=None is resolved by audio_windows; Engine.audio_batch takes a number")
        return {"samples": int(self.samples), "dtype": self.dtype, "pad": self.pad, "pad_value": float(self.pad_value)}


def audio_windows(nsamples, samples: Optional[int] = None, stride: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """``batch_windows`` for samples: the windows of segments of ``nsamples`` [n] samples each -> (windows, T): per segment of S
    samples one window at ``sample0 = 0, stride, 2 * stride, ...`` while ``sample0 < S``, each of ``min(samples, S - sample0)``
    samples, as a ``(seg, nsamples, sample0)`` record array ``Engine.audio_batch`` takes.  ``stride`` is a multiple of 4;
    ``stride=None``: ``samples``.  ``samples=None``: one window per segment (also one without samples) and T the longest segment
    rounded up to a multiple of 4 (4 at the least)."""
    S = np.asarray(nsamples, np.int64).reshape(-1)
    if (S < 0).any():
        raise ConfigurationError("nsamples", repr(S[:8].tolist()), "audio_windows: a segment has 0 or more samples")
    if samples is None:
        T = max(4, -(-int(S.max(initial=0)) // 4) * 4)
        if T > 1 << 24:
            raise ConfigurationError("samples", "None", f"audio_windows: the longest segment has {int(S.max())} samples, a window 2^24 at the most: "
                                     "give samples")
        w = np.zeros(S.size, _ffi.AUDIO_WINDOW_DTYPE)
        w["seg"], w["nsamples"] = np.arange(S.size), S
        return w, T
    T = int(samples)
    step = T if stride is None else int(stride)
    if T < 4 or T > 1 << 24 or T % 4 or step < 4 or step % 4:
        raise ConfigurationError("samples", repr((samples, stride)), "audio_windows: samples is a multiple of 4 from 4 to 2^24 and stride a multiple "
                                 f"of 4, 4 or more, got {samples!r} and {stride!r}")
    rec = [(i, min(T, int(s) - r), r) for i, s in enumerate(S) for r in range(0, int(s), step)]
    return np.array(rec, _ffi.AUDIO_WINDOW_DTYPE).reshape(-1), T


def audio_affine(moments, levels, nsamples, norm: str = "none", eps: float = 1e-7, target: float = 0.9):
    """``Engine.moments`` / ``Engine.levels`` records and the sample counts they run over -> ``(shift, scale)`` as ``Engine.audio_batch``
    takes them, for ``norm``: ``"none"``: two ``None``; ``"mean"``: ``shift = -mean``; ``"zscore"``: also ``scale = 1 / sqrt(max(var,
    0) + eps)`` - ``mean = sum_q31 / (2^31 N)``, ``var = energy_q32 / (2^32 N) - mean^2``, in float64 from the integers, rounded to
    float32 once; ``"peak"``: ``scale = np.float32(np.float32(target) / peak)``, 1 where the peak is 0 or not finite (it needs
    ``levels``; the other two need ``moments``).  An entry without samples gets 0 and 1."""
    if norm == "none":
        return None, None
    if norm == "peak":
        peak = np.asarray(levels["peak"], np.float32)
        usable = np.isfinite(peak) & (peak > 0)
        return None, np.where(usable, np.float32(target) / np.where(usable, peak, np.float32(1)), np.float32(1)).astype(np.float32)
    if norm not in ("mean", "zscore"):
        raise ConfigurationError("norm", repr(norm), f"audio_affine: norm is 'none', 'mean', 'zscore' or 'peak', got {norm!r}")
    N = np.asarray(nsamples, np.int64).reshape(-1).astype(np.float64)
    some = N > 0
    Ns = np.where(some, N, 1.0)
    mean = np.where(some, np.asarray(moments["sum_q31"]).astype(np.float64) / (2147483648.0 * Ns), 0.0)
    shift = (-mean).astype(np.float32)
    if norm == "mean":
        return shift, None
    var = np.asarray(moments["energy_q32"]).astype(np.float64) / (4294967296.0 * Ns) - mean * mean
    scale = np.where(some, 1.0 / np.sqrt(np.maximum(var, 0.0) + float(eps)), 1.0).astype(np.float32)
    return shift, scale


def _need_audio_batch(engine, who: str) -> None:
    if not hasattr(engine, "audio_batch") or not hasattr(engine, "moments"):
        raise ConfigurationError("batch", "given", f"{who} needs an engine with audio_batch and moments (the windows are normalised and padded "
                                 f"from the block a scan left on the GPU), {type(engine).__name__} has none")


def audio_recordings(recordings: Sequence[np.ndarray], batch: AudioBatch, config: Optional[VADConfig] = None, engine=None,
                     hop: Optional[int] = None, law: Optional[str] = None, channel="mix", open_end: bool = False,
                     refine: Optional[SegmentRefine] = None, sample_rate: Optional[int] = None, convert=None, mask: bool = False):
    """``cut_recordings(layout="range")`` as the tensor a waveform model takes: the samples of every finished segment of every
    recording, windowed, normalised, padded and converted as ``batch`` says -> ``(array, index)`` or, with ``mask=True``, ``(array,
    index, mask)``: ``array`` [B, T] (``Engine.audio_batch``), ``mask`` [B, T] uint8 (1 on a window's samples), ``index`` one
    ``(recording, channel, start_sample, end_sample, first_sample, nsamples)`` per window - the segment it shows, the window's first
    sample in the segment and its samples.  One scan, at most one ``Engine.moments`` or ``Engine.levels`` and one
    ``Engine.audio_batch`` under ``Engine.scan_session()``: the samples never leave the GPU as float32, only 16 bytes per segment
    and the batch cross the link.  ``batch.scope="recording"`` adds the integer records of a (recording, channel) on the host first.
    The other arguments as in ``cut_recordings``.  Recordings at another rate than the engine's go through ``convert=`` (as in
    ``scan_recordings``: the windows and the ranges of ``index`` count samples of the converted signal, ``input_ranges`` maps them
    back); a ``sample_rate`` other than the engine's without ``convert`` is a ``ConfigurationError``.  A corpus of 1-D and 2-D
    recordings is a ``ConfigurationError``: call it once per kind.  No segment anywhere: an array with B = 0."""
    from .pool import default_pool, resolve_model_path
    who = "audio_recordings"
    batch.check()
    split = isinstance(channel, str) and channel == "split"
    if not (channel in ("mix", "split") if isinstance(channel, str) else isinstance(channel, (int, np.integer)) and int(channel) in (0, 1)):
        raise ConfigurationError("channel", repr(channel), f"{who}: channel is 'mix', 0, 1 or 'split' for the whole corpus, got {channel!r}")
    cfg = config or VADConfig()
    if engine is None:
        engine = default_pool().engine_for(resolve_model_path(cfg), cfg.model_version, sample_rate=int(cfg.sample_rate))
    _need_audio_batch(engine, who)
    if batch.norm == "peak":
        _need_levels(engine, who, "norm='peak'")
    if open_end:
        _need_tails(engine, who)
    if refine is not None:
        _need_refine(engine, who)
    frame = engine.frame_samples
    if cfg.buffer_size != frame:
        raise ConfigurationError(f"{who} frames at the model's frame size: buffer_size = {cfg.buffer_size}, the engine's frames have "
                                 f"{frame} samples")
    conv = _convert_arg(who, engine, sample_rate, convert, split)
    if conv is None and sample_rate is not None and int(sample_rate) != int(engine.sample_rate):
        raise ConfigurationError("sample_rate", repr(sample_rate), f"{who}: recordings at {sample_rate} Hz on an engine at {engine.sample_rate} Hz "
                                 "need convert= (the batch does not resample: the recordings are converted once, ahead of the scan)")
    hop = frame // 2 if hop is None else int(hop)
    recordings = [np.asarray(r) for r in recordings]
    kinds = {r.ndim == 2 for r in recordings}
    if len(kinds) > 1:
        raise ConfigurationError("recordings", "1-D and 2-D", f"{who}: one batch holds recordings of one kind; call it once for the 1-D and once "
                                 "for the two-channel recordings")
    np_dtype = {"f32": np.float32, "f16": np.float16}.get(batch.dtype, np.uint16)
    T0 = int(batch.samples) if batch.samples is not None else 4
    none = (np.empty((0, T0), np_dtype), []) + ((np.empty((0, T0), np.uint8),) if mask else ())
    if not recordings:
        return none
    two = kinds.pop()
    denoise = 0.01 if cfg.enable_denoising else None
    per = 2 if two and split else 1
    chans = (0, 1) if per == 2 else (channel if two and conv is None else 0,)
    slots = engine.open_streams(len(recordings) * per)
    out = None
    try:
        engine.set_thresholds_many(slots, _thresholds_of(cfg))
        with engine.scan_session():
            ranges = _scan_ranges(engine, slots, recordings, per, frame, hop, law, denoise, channel, open_end=open_end, refine=refine, convert=conv)
            table = _cut_table(engine, ranges, chans, frame, hop)
            if table:
                ns = np.array([(n - 1) * hop + frame for _, _, n, _ in table], np.int64)
                windows, T = audio_windows(ns, batch.samples, batch.stride)
                mo = lv = None
                if batch.norm in ("mean", "zscore"):
                    mo = engine.moments(table, hop=hop, denoise=denoise)
                elif batch.norm == "peak":
                    lv = engine.levels(table, hop=hop, denoise=denoise)
                if batch.scope == "recording" and batch.norm != "none":
                    # the group of a segment: its (recording, channel), numbered in the table's order; integers add exactly
                    group = np.array([i * per + c for i, rc in enumerate(ranges) for c, rg in enumerate(rc) for _ in rg], np.int64)
                    ngroups = len(recordings) * per
                    gn = np.zeros(ngroups, np.int64)
                    np.add.at(gn, group, ns)
                    if mo is not None:
                        gm = np.zeros(ngroups, _ffi.MOMENTS_DTYPE)
                        np.add.at(gm["sum_q31"], group, mo["sum_q31"])
                        np.add.at(gm["energy_q32"], group, mo["energy_q32"])
                        mo = gm
                    else:
                        gl = np.zeros(ngroups, _ffi.LEVEL_DTYPE)
                        # (the maximum of the bit patterns of |x|, as the kernel takes it)
                        np.maximum.at(gl["peak"].view(np.uint32), group, lv["peak"].view(np.uint32))
                        lv = gl
                    shift, scale = (None if a is None else a[group] for a in audio_affine(mo, lv, gn, batch.norm, batch.eps, batch.target))
                else:
                    shift, scale = audio_affine(mo, lv, ns, batch.norm, batch.eps, batch.target)
                out = engine.audio_batch(table, windows, replace(batch, samples=T).record(), shift=shift, scale=scale, mask=mask, hop=hop,
                                         denoise=denoise)
    finally:
        for s in slots:
            engine.close_stream(int(s))
    if out is None:
        return none
    where = [(i, chans[c], a, b) for i, rc in enumerate(ranges) for c, rg in enumerate(rc) for a, b, *_ in rg]
    index = [where[int(w["seg"])] + (int(w["sample0"]), int(w["nsamples"])) for w in windows]
    return (out[0], index, out[1]) if mask else (out, index)
