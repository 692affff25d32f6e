// TEST-ONLY host stand-ins for the vadk_launch_* entry points of the .hip files (see hip/hip_runtime_api.h): the "model" is
// p = clamp(|first sample of the frame|, 0, 1) - the harness scripts a stream's probabilities through its audio - and the events
// come from the REAL state machine (csrc/sm_device.h) on the slot's SmSlot, exactly as the kernels apply it.  A float32 frame
// with a NaN / Inf sample is rejected as the kernels reject it (include/vad_engine.h VAD_EV_REJECTED): NaN, the bit, no state change.
#include "../../include/vad_engine.h"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "resample_generic.h"
#include "sm_device.h"
#include "vad_layout.h"

int fake_hip_fail_after = 0;

hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) {
    if (fake_hip_fail_after > 0 && --fake_hip_fail_after == 0) return hipErrorInvalidValue;
    std::memcpy(d, s, n);
    return hipSuccess;
}

using namespace vadk;

// ITU-T G.711 code -> 16-bit linear PCM (include/vad_engine.h has the two formulas)
static int16_t g711_pcm(uint8_t b, bool alaw) {
    if (!alaw) {
        const int u = ~b & 0xFF, t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
        return (int16_t)((u & 0x80) ? 0x84 - t : t - 0x84);
    }
    const int a = b ^ 0x55, seg = (a & 0x70) >> 4;
    int t = (a & 0x0F) << 4;
    t = seg == 0 ? t + 8 : seg == 1 ? t + 0x108 : (t + 0x108) << (seg - 1);
    return (int16_t)((a & 0x80) ? t : -t);
}

static float first_sample(const void *frames, size_t index, int fmt, int frame_samples) {
    if (fmt == VAD_FMT_F32) return static_cast<const float *>(frames)[index * (size_t)frame_samples];
    if (fmt == VAD_FMT_ULAW8 || fmt == VAD_FMT_ALAW8)
        return (float)g711_pcm(static_cast<const uint8_t *>(frames)[index * (size_t)frame_samples], fmt == VAD_FMT_ALAW8) / 32768.0f;
    const int16_t q = static_cast<const int16_t *>(frames)[index * (size_t)frame_samples];
    return (float)q / (fmt == VAD_FMT_I16_32767 ? 32767.0f : 32768.0f);
}

static bool has_nonfinite(const void *frames, size_t index, int fmt, int frame_samples) {
    if (fmt != VAD_FMT_F32) return false;
    const float *x = static_cast<const float *>(frames) + index * (size_t)frame_samples;
    for (int k = 0; k < frame_samples; ++k)
        if (!std::isfinite(x[k])) return true;
    return false;
}

static hipError_t fake_step(const StepParams *p, int frame_samples) {
    for (int i = 0; i < p->n; ++i) {
        const int slot = p->slots ? p->slots[i] : i;
        SmSlot &s = p->sm[slot];
        int seg_last = 0;
        for (int t = 0; t < p->T; ++t) {
            if (has_nonfinite(p->frames, (size_t)i * p->T + t, p->fmt, frame_samples)) {
                p->probs[(size_t)i * p->T + t] = std::nanf("");
                if (p->events) p->events[(size_t)i * p->T + t] = (uint8_t)EV_REJECTED;
                continue;
            }
            float x = first_sample(p->frames, (size_t)i * p->T + t, p->fmt, frame_samples);
            if (p->thresh >= 0.f && !(std::fabs(x) > p->thresh)) x = 0.f;
            const float prob = std::fmin(1.0f, std::fabs(x));
            int sg = 0;
            const int ev = sm_step(s, prob, &sg);
            if (ev & 2) seg_last = sg;
            p->probs[(size_t)i * p->T + t] = prob;
            if (p->events) p->events[(size_t)i * p->T + t] = (uint8_t)ev;
            p->state[(size_t)slot * 256] += 1.0f;              // "h" counts the frames this stream has seen
        }
        if (p->seg_frames) p->seg_frames[i] = seg_last;
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_silero_v5(const StepParams *p, hipStream_t) { return fake_step(p, p->variant ? 256 : 512); }
extern "C" hipError_t vadk_launch_silero_v4(const StepParams *p, hipStream_t) { return fake_step(p, 512); }
extern "C" hipError_t vadk_launch_silero_v5_t16(const StepParams *p, hipStream_t) { return fake_step(p, p->variant ? 256 : 512); }
extern "C" hipError_t vadk_launch_silero_v5_t16_pair(const StepParams *p, hipStream_t) { return fake_step(p, 512); }
extern "C" hipError_t vadk_launch_silero_v4_t16(const StepParams *p, int, hipStream_t) { return fake_step(p, 512); }

// whole recordings (csrc/silero_v5_t16.hip: silero_v5_scan16), the same rule as fake_step: p = |first sample of the frame|, the
// real state machine, a float32 frame with a NaN / Inf sample rejected; a stream past its recording's end is held (nothing
// stepped, nothing written).  The "frames" are addressed as the kernel addresses them: sample 4 (quad0 + t hopq) of the block.
// a->channels == 2 (silero_v5_stereo16): the block is interleaved, positions count sample frames, and the item's mode (the top
// bits of quad0) picks the left samples, the right ones or the float32 mean of the decoded pair - the same rule on those.
extern "C" hipError_t vadk_launch_silero_v5_scan16(const StepParams *p, const ScanItem *items, const ScanArgs *a, hipStream_t) {
    const int frame_samples = p->variant ? 256 : 512;
    for (int i = 0; i < p->n; ++i) {
        const ScanItem &it = items[i];
        SmSlot &s = p->sm[it.slot];
        const bool two = a->channels == 2;
        const uint32_t mode = two ? it.quad0 >> SCAN_MODE_SHIFT : 0u, quad0 = two ? it.quad0 & ((1u << SCAN_MODE_SHIFT) - 1u) : it.quad0;
        // sample k of the stream, decoded (first_sample indexes frames of `stride` samples: a stride of one addresses the block itself)
        auto sample = [&](size_t k) -> float {
            if (!two) return first_sample(p->frames, k, p->fmt, 1);
            const float l = first_sample(p->frames, 2 * k, p->fmt, 1), r = first_sample(p->frames, 2 * k + 1, p->fmt, 1);
            return mode == SCAN_MIX ? (l + r) * 0.5f : mode == SCAN_RIGHT ? r : l;
        };
        for (int t = a->t0; t < a->t0 + p->T && t < it.nframes; ++t) {
            const size_t first = 4 * ((size_t)quad0 + (size_t)t * a->hopq), o = (size_t)it.out0 + (size_t)t;
            bool bad = false;
            if (p->fmt == VAD_FMT_F32)
                for (int k = 0; k < frame_samples; ++k) bad = bad || !std::isfinite(sample(first + k));
            if (bad) {
                p->probs[o] = std::nanf("");
                if (p->events) p->events[o] = (uint8_t)EV_REJECTED;
                if (p->seg_frames) p->seg_frames[o] = 0;
                continue;
            }
            float x = sample(first);
            if (p->thresh >= 0.f && !(std::fabs(x) > p->thresh)) x = 0.f;
            const float prob = std::fmin(1.0f, std::fabs(x));
            int sg = 0;
            const int ev = sm_step(s, prob, &sg);
            p->probs[o] = prob;
            if (p->events) p->events[o] = (uint8_t)ev;
            if (p->seg_frames) p->seg_frames[o] = (ev & 2) ? sg : 0;
            p->state[(size_t)it.slot * 256] += 1.0f;
        }
    }
    return hipSuccess;
}

// finished segments cut out of a block (csrc/scan_cut.hip: vadk_scan_cut), the kernel's arithmetic in plain C++, quad by quad as
// its workgroups are listed: decode (s / 32767 or s / 32768 as IEEE quotients, G.711 / 32768), left | right | (L + R) * 0.5f, the
// strict gate, then the float32 itself or clip(x * 32767, -32768, 32767) converted toward zero.  gains (vadk_scan_cut_gain): the
// gated value times gains[segment], one float32 multiply, ahead of either.  levels (csrc/scan_levels.hip: vadk_seg_levels): nothing
// is stored - the gated values of a segment are folded into its vad_level (a.out, zeroed by the caller): energy_q32 +=
// min(rint((double)x * x * 2^32), 2^32), peak = the larger bit pattern of |x|, clipped += |x| >= clip in float32.  stereo
// (csrc/scan_cut.hip: vadk_scan_cut_stereo): the mode bits are ignored, sample frame o takes two output values - the left
// channel's at 2 o, the right one's at 2 o + 1 - each gated, gained and converted on its own
static hipError_t fake_cut(const CutArgs *a, const float *gains, bool levels, float clip, bool stereo = false) {
    if (stereo && a->channels != 2) return hipErrorInvalidValue;
    const uint32_t fmask = a->frame_shift >= 31u ? 0x7fffffffu : (1u << a->frame_shift) - 1u;
    const size_t ch = a->channels == 2 ? 2 : 1;
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const CutWork w = a->work[b];
        const CutSeg sg = a->segs[w.seg];
        const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
        for (uint32_t oq = w.quad0; oq < w.quad0 + (uint32_t)CUT_WG_QUADS && oq < sg.nquads; ++oq) {
            const uint32_t iq = qin + (oq >> a->frame_shift) * a->hopq + (oq & fmask);
            for (int kc = 0; kc < (stereo ? 8 : 4); ++kc) {
                const int k = stereo ? kc >> 1 : kc, c = kc & 1;
                const size_t i = 4 * (size_t)iq + k, of = 4 * ((size_t)sg.quad_out + oq) + k, o = stereo ? 2 * of + c : of;
                if ((i + 1) * ch * (a->fmt == VAD_FMT_F32 ? 4 : a->fmt >= VAD_FMT_ULAW8 ? 1 : 2) > a->audio_bytes) return hipErrorInvalidValue;
                float x;
                if (ch == 1) x = first_sample(a->audio, i, a->fmt, 1);
                else {
                    const float l = first_sample(a->audio, 2 * i, a->fmt, 1), r = first_sample(a->audio, 2 * i + 1, a->fmt, 1);
                    x = stereo ? (c ? r : l) : mode == SCAN_MIX ? (l + r) * 0.5f : mode == SCAN_RIGHT ? r : l;
                }
                if (a->thresh >= 0.f && !(std::fabs(x) > a->thresh)) x = 0.f;
                if (levels) {
                    vad_level &lv = static_cast<vad_level *>(a->out)[w.seg];
                    const float ax = std::fabs(x);
                    uint32_t bits, top;
                    std::memcpy(&bits, &ax, 4);
                    std::memcpy(&top, &lv.peak, 4);
                    if (bits > top) lv.peak = ax;
                    lv.clipped += ax >= clip ? 1 : 0;
                    const double q = std::rint((double)x * (double)x * 4294967296.0);
                    lv.energy_q32 += (int64_t)(q < 4294967296.0 ? q : 4294967296.0);      // (a NaN counts as 1: unspecified)
                    continue;
                }
                if (gains) x = x * gains[w.seg];
                if (a->out_fmt == VAD_CUT_F32) static_cast<float *>(a->out)[o] = x;
                else {
                    const float v = x * 32767.0f;
                    static_cast<int16_t *>(a->out)[o] = (int16_t)(int)(v < -32768.0f ? -32768.0f : v > 32767.0f ? 32767.0f : v);
                }
            }
        }
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_scan_cut(const CutArgs *a, hipStream_t) { return fake_cut(a, nullptr, false, 0.f); }
extern "C" hipError_t vadk_launch_scan_cut_gain(const CutArgs *a, const float *gains, hipStream_t) { return fake_cut(a, gains, false, 0.f); }
extern "C" hipError_t vadk_launch_seg_levels(const CutArgs *a, float clip, hipStream_t) { return fake_cut(a, nullptr, true, clip); }
extern "C" hipError_t vadk_launch_scan_cut_stereo(const CutArgs *a, const float *gains, hipStream_t) { return fake_cut(a, gains, false, 0.f, true); }

// sample frame i of a block as the cut reads it: decoded, channel-selected by `mode`, gated; false: past the block
static bool fake_heard(const void *audio, uint32_t audio_bytes, int fmt, int channels, uint32_t mode, float thresh, size_t i, float *x) {
    const size_t ch = channels == 2 ? 2 : 1;
    if ((i + 1) * ch * (fmt == VAD_FMT_F32 ? 4 : fmt >= VAD_FMT_ULAW8 ? 1 : 2) > audio_bytes) return false;
    if (ch == 1) *x = first_sample(audio, i, fmt, 1);
    else {
        const float l = first_sample(audio, 2 * i, fmt, 1), r = first_sample(audio, 2 * i + 1, fmt, 1);
        *x = mode == SCAN_MIX ? (l + r) * 0.5f : mode == SCAN_RIGHT ? r : l;
    }
    if (thresh >= 0.f && !(std::fabs(*x) > thresh)) *x = 0.f;
    return true;
}

// a segment's moments (csrc/scan_levels.hip: vadk_seg_moments), sample by sample over the levels' work list: sum_q31 +=
// rint(clamp(x, -1, 1) * 2^31) in float64, energy_q32 as fake_cut's levels have it; a.out is zeroed by the caller
extern "C" hipError_t vadk_launch_seg_moments(const CutArgs *a, hipStream_t) {
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const CutWork w = a->work[b];
        const CutSeg sg = a->segs[w.seg];
        const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
        vad_moments &mo = static_cast<vad_moments *>(a->out)[w.seg];
        for (uint32_t oq = w.quad0; oq < w.quad0 + (uint32_t)CUT_WG_QUADS && oq < sg.nquads; ++oq)
            for (int k = 0; k < 4; ++k) {
                float x;
                if (!fake_heard(a->audio, a->audio_bytes, a->fmt, a->channels, mode, a->thresh, 4 * ((size_t)qin + oq) + k, &x)) return hipErrorInvalidValue;
                const double cl = x < -1.0f ? -1.0 : x > 1.0f ? 1.0 : (double)x;
                mo.sum_q31 += (int64_t)std::rint(cl * 2147483648.0);                        // (a NaN: unspecified)
                const double q = std::rint((double)x * (double)x * 4294967296.0);
                mo.energy_q32 += (int64_t)(q < 4294967296.0 ? q : 4294967296.0);
            }
    }
    return hipSuccess;
}

static uint16_t f16_bits(float f);

// normalised, padded windows of segment audio (csrc/audio_batch.hip: vadk_audio_batch): include/vad_engine.h's rule cell by cell
// over the host's work list, every operation a float32 of its own (volatile: each is rounded where it stands)
extern "C" hipError_t vadk_launch_audio_batch(const AudioBatchArgs *a, hipStream_t) {
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const AudioWork w = a->work[b];
        const AudioWin win = a->win[w.window];
        const CutSeg sg = a->segs[win.seg];
        if (w.quad0 >= a->tq || win.nsamples > 4 * a->tq || (uint64_t)4 * win.quad0 + win.nsamples > (uint64_t)4 * sg.nquads) return hipErrorInvalidValue;
        const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = (sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u)) + win.quad0;
        const float shift = a->shift[a->per_seg ? win.seg : 0u], scale = a->scale[a->per_seg ? win.seg : 0u];
        auto norm = [&](float x) -> float {
            volatile float s = x + shift;
            return s * scale;
        };
        for (uint32_t q = w.quad0; q < w.quad0 + (uint32_t)CUT_WG_QUADS && q < a->tq; ++q)
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t t = 4 * q + k;
                float val;
                if (t < win.nsamples) {
                    float x;
                    if (!fake_heard(a->audio, a->audio_bytes, a->fmt, a->channels, mode, a->thresh, 4 * (size_t)qin + t, &x)) return hipErrorInvalidValue;
                    val = norm(x);
                } else {
                    val = a->pad_mode == VAD_BATCH_PAD_FEATURE ? norm(0.0f) : a->pad_value;
                }
                const size_t o = (size_t)w.window * 4 * a->tq + t;
                if (a->dtype == VAD_BATCH_F32) static_cast<float *>(a->out)[o] = val;
                else {
                    uint32_t bits;
                    std::memcpy(&bits, &val, 4);
                    static_cast<uint16_t *>(a->out)[o] = a->dtype == VAD_BATCH_F16 ? f16_bits(val) : melb_bf16(bits);
                }
                if (a->mask) a->mask[o] = t < win.nsamples ? 1 : 0;
            }
    }
    return hipSuccess;
}

// log-mel frames of finished segments (csrc/scan_mel.hip: vadk_seg_mel), the header's rule in plain float32 loops, tile by tile as
// the workgroups are listed, over the UNPACKED view of the same tables: the cut's decoded, channel-selected, gated sample, reflected
// by index, op_re / op_im / filters read back out of the packed streams (vad_layout.h: mel_op_index, mel_filter_index), sums in
// ascending n and k, P = re * re + im * im, then the floor and std::log / std::log10 in float32
extern "C" hipError_t vadk_launch_seg_mel(const MelArgs *a, hipStream_t) {
    const size_t ch = a->channels == 2 ? 2 : 1, bytes = a->fmt == VAD_FMT_F32 ? 4 : a->fmt >= VAD_FMT_ULAW8 ? 1 : 2;
    std::vector<float> P(a->bins_pad);
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const MelWork w = a->work[b];
        const CutSeg sg = a->segs[w.seg];
        const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
        const int64_t S = (int64_t)sg.nquads * 4, half = a->pad == VAD_MEL_PAD_REFLECT ? a->n_fft / 2 : 0, len = S + 2 * half;
        if (len < (int64_t)a->n_fft || (w.frame0 % MEL_TILE) != 0) return hipErrorInvalidValue;
        const int64_t M = (len - a->n_fft) / a->hop + 1;
        if ((int64_t)w.frame0 >= M) return hipErrorInvalidValue;
        auto sample = [&](int64_t j, float *x) -> bool {          // p[j] of the header
            int64_t r = j - half;
            r = r < 0 ? -r : r >= S ? 2 * (S - 1) - r : r;
            if (r < 0 || r >= S) return false;
            const size_t i = 4 * (size_t)qin + (size_t)r;
            if ((i + 1) * ch * bytes > a->audio_bytes) return false;
            if (ch == 1) *x = first_sample(a->audio, i, a->fmt, 1);
            else {
                const float l = first_sample(a->audio, 2 * i, a->fmt, 1), rr = first_sample(a->audio, 2 * i + 1, a->fmt, 1);
                *x = mode == SCAN_MIX ? (l + rr) * 0.5f : mode == SCAN_RIGHT ? rr : l;
            }
            if (a->thresh >= 0.f && !(std::fabs(*x) > a->thresh)) *x = 0.f;
            return true;
        };
        for (int64_t f = w.frame0; f < M && f < (int64_t)w.frame0 + MEL_TILE; ++f) {
            for (uint32_t k = 0; k < a->bins_pad; ++k) {
                float re = 0.f, im = 0.f;
                for (uint32_t n = 0; n < a->n_fft; ++n) {
                    float x;
                    if (!sample(f * a->hop + n, &x)) return hipErrorInvalidValue;
                    const size_t at = mel_op_index(n, k, a->n_fft);
                    re += x * a->op[at];
                    im += x * a->op[at + 1];
                }
                P[k] = re * re + im * im;
            }
            float *row = a->out + ((size_t)sg.quad_out + (size_t)f) * a->n_mels;
            for (uint32_t j = 0; j < a->n_mels; ++j) {
                float e = 0.f;
                for (uint32_t k = 0; k < a->bins_pad; ++k) e += a->filters[mel_filter_index(j, k, a->bins_pad)] * P[k];
                if (a->log != VAD_MEL_LINEAR) {
                    e = e > a->floor ? e : a->floor;
                    e = a->log == VAD_MEL_LN ? std::log(e) : std::log10(e);
                }
                row[j] = e;
            }
        }
    }
    return hipSuccess;
}

// finished segments of a rate block at 16 kHz (csrc/scan_resample_cut.hip: vadk_resample_cut), the header's rule in plain float32:
// for output m of a segment, y = sum over k ASCENDING of x[k] * h[m M - k L + C] with x the cut's decoded, channel-selected, ungated
// sample inside [0, S_in) and nothing outside it, h read back out of the packed operator (vad_layout.h: rsc_pack_index; T[o][n]
// with o = m % 16 and n = k - (m / 16) A + n0), then the gain as a multiply of its own and the cut's conversion
extern "C" hipError_t vadk_launch_resample_cut(const ResampleCutArgs *a, hipStream_t) {
    const size_t ch = a->channels == 2 ? 2 : 1, bytes = a->fmt == VAD_FMT_F32 ? 4 : a->fmt >= VAD_FMT_ULAW8 ? 1 : 2;
    if (a->sr_in != 8000 && a->sr_in != 24000 && a->sr_in != 48000) return hipErrorInvalidValue;
    const int64_t A = rsc_A(a->sr_in), K = (int64_t)a->ksteps * 16;
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const CutWork w = a->work[b];
        const CutSeg sg = a->segs[w.seg];
        const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
        const int64_t S_in = (int64_t)a->inq[w.seg] * 4;
        if (w.quad0 % (RSC_WG_SAMPLES / 4) != 0 || w.quad0 >= sg.nquads) return hipErrorInvalidValue;
        const int64_t m1 = std::min<int64_t>((int64_t)sg.nquads * 4, (int64_t)w.quad0 * 4 + RSC_WG_SAMPLES);
        for (int64_t m = (int64_t)w.quad0 * 4; m < m1; ++m) {
            const int64_t k0 = (m / 16) * A - (int64_t)a->n0;
            float y = 0.f;
            for (int64_t n = 0; n < K; ++n) {
                const int64_t k = k0 + n;
                if (k < 0 || k >= S_in) continue;
                const size_t i = 4 * (size_t)qin + (size_t)k;
                if ((i + 1) * ch * bytes > a->audio_bytes) return hipErrorInvalidValue;
                float x;
                if (ch == 1) x = first_sample(a->audio, i, a->fmt, 1);
                else {
                    const float l = first_sample(a->audio, 2 * i, a->fmt, 1), r = first_sample(a->audio, 2 * i + 1, a->fmt, 1);
                    x = mode == SCAN_MIX ? (l + r) * 0.5f : mode == SCAN_RIGHT ? r : l;
                }
                y += x * a->op[rsc_pack_index((uint32_t)(m % 16), (uint32_t)n)];
            }
            if (a->gains) y = y * a->gains[w.seg];
            const size_t o = 4 * (size_t)sg.quad_out + (size_t)m;
            if (a->out_fmt == VAD_CUT_F32) static_cast<float *>(a->out)[o] = y;
            else {
                const float v = y * 32767.0f;
                static_cast<int16_t *>(a->out)[o] = (int16_t)(int)(v < -32768.0f ? -32768.0f : v > 32767.0f ? 32767.0f : v);
            }
        }
    }
    return hipSuccess;
}

// per-segment statistics of a feature matrix (csrc/mel_batch.hip: vadk_mel_stats), part by part as the workgroups are listed, into
// the -inf and the zeros the caller stored: the maximum by the order of the bit patterns, the sums of q and q * q in integers
// whole recordings converted to the engine's rate (csrc/scan_convert.hip: vadk_convert), the header's rule in plain float32: for
// output m of an item, y = sum over k ASCENDING of x[k] * h[m M - k L + C] with x the loader's decoded, channel-selected, ungated
// sample inside [0, S_in) and nothing outside it, h read back out of the packed operators (vad_layout.h: cv_pack_index; T_r[o][n]
// with r = (m % P) / 16, o = m % 16 and n = k - (m / P) PI - base_r); the samples up to roundup4(S_out) are +0.0
extern "C" hipError_t vadk_launch_convert(const ConvertArgs *a, hipStream_t) {
    const size_t ch = a->channels == 2 ? 2 : 1;
    if (a->nper == 0 || a->ntiles * 16u != a->P) return hipErrorInvalidValue;
    const int64_t K = (int64_t)a->ksteps * 16, run = (int64_t)a->nper * a->P;
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const ConvertWork w = a->work[b];
        const ConvertItem it = a->items[w.item];
        const uint32_t mode = it.quad_in >> SCAN_MODE_SHIFT, qin = it.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
        const int64_t S_in = it.s_in, S_out = it.s_out, m0 = (int64_t)w.run * run;
        if (m0 >= S_out) return hipErrorInvalidValue;
        const int64_t m1 = std::min<int64_t>((S_out + 3) & ~(int64_t)3, m0 + run);
        for (int64_t m = m0; m < m1; ++m) {
            float y = 0.f;
            const uint32_t r = (uint32_t)((m % a->P) / 16);
            const int64_t k0 = (m / a->P) * (int64_t)a->PI + cv_base(r, a->ntaps, a->L, a->M);
            for (int64_t n = 0; n < K && m < S_out; ++n) {
                const int64_t k = k0 + n;
                if (k < 0 || k >= S_in) continue;
                const size_t i = 4 * (size_t)qin + (size_t)k;
                float x;
                if (ch == 1) x = first_sample(a->audio, i, a->fmt, 1);
                else {
                    const float l = first_sample(a->audio, 2 * i, a->fmt, 1), rr = first_sample(a->audio, 2 * i + 1, a->fmt, 1);
                    x = mode == SCAN_MIX ? (l + rr) * 0.5f : mode == SCAN_RIGHT ? rr : l;
                }
                y += x * a->op[cv_pack_index(r, (uint32_t)(m % 16), (uint32_t)n, (uint32_t)K)];
            }
            a->out[4 * (size_t)it.quad_out + (size_t)m] = y;
        }
    }
    return hipSuccess;
}

static bool bits_above(uint32_t y, uint32_t x) {                       // y is the larger float32: -0.0 below +0.0
    const bool xn = x >> 31, yn = y >> 31;
    return xn != yn ? xn : xn ? y < x : y > x;
}

extern "C" hipError_t vadk_launch_mel_stats(const MelStatsArgs *a, hipStream_t) {
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const MelStatsWork w = a->work[b];
        if (w.nrows < 1 || w.nrows > (uint32_t)MELB_STATS_ROWS) return hipErrorInvalidValue;
        for (uint32_t r = 0; r < w.nrows; ++r)
            for (uint32_t j = 0; j < a->n_mels; ++j) {
                const float v = a->x[((size_t)w.row0 + r) * a->n_mels + j];
                if (a->max_out) {
                    uint32_t vb, mb;
                    std::memcpy(&vb, &v, 4);
                    std::memcpy(&mb, &a->max_out[w.seg], 4);
                    if (bits_above(vb, mb)) a->max_out[w.seg] = v;
                }
                const long long q = melb_q(v);
                if (a->sum_out) a->sum_out[(size_t)w.seg * a->n_mels + j] += q;
                if (a->sumsq_out) a->sumsq_out[(size_t)w.seg * a->n_mels + j] += (unsigned long long)(q * q);
            }
    }
    return hipSuccess;
}

// a projection of a feature matrix (csrc/mel_project.hip: vadk_mel_project): include/vad_engine.h's rule - a chain of fused
// multiply-adds from the bias, k ascending - over the host's packed operator (vad_layout.h: proj_pack_index)
extern "C" hipError_t vadk_launch_mel_project(const ProjArgs *a, hipStream_t) {
    if (a->rows == 0) return hipSuccess;
    if (a->n_in < 1 || a->n_in > (uint32_t)PROJ_MAX || a->n_out < 1 || a->n_out > (uint32_t)PROJ_MAX) return hipErrorInvalidValue;
    const uint32_t K4 = proj_up4(a->n_in), N16 = proj_up16(a->n_out);
    const float *bias = a->op + (size_t)K4 * N16;
    for (uint64_t r = 0; r < a->rows; ++r)
        for (uint32_t c = 0; c < a->n_out; ++c) {
            float acc = bias[c];
            for (uint32_t k = 0; k < K4; ++k) acc = std::fmaf(k < a->n_in ? a->x[(size_t)r * a->n_in + k] : 0.0f, a->op[proj_pack_index(k, c, K4)], acc);
            a->out[(size_t)r * a->n_out + c] = acc;
        }
    return hipSuccess;
}

// float32 -> float16 bits, round to nearest even, overflow to inf
static uint16_t f16_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);            // 65520 and above
    if (x < 0x38800000u) return (uint16_t)(sign | (uint32_t)std::nearbyintf(std::fabs(f) * 16777216.0f));   // below 2^-14: units of 2^-24
    return (uint16_t)(sign | ((x + 0xfffu + ((x >> 13) & 1u) - 0x38000000u) >> 13));
}

// The batch cell rule of include/vad_engine.h, once, as both kernels share melb_tile_body (csrc/mel_batch.hip): frames t0 .. t0 + nt of
// window `window`, the first nv of them rows row0 .. of the segment of M rows at seg_row, the rest pad cells, under lo, shift and
// scale number `affine`.  Every operation a float32 of its own (volatile: each is rounded where it stands)
static void fake_batch_cells(const MelBatchArgs *a, uint32_t window, uint32_t t0, uint32_t nt, uint32_t nv, uint64_t seg_row, uint32_t M, uint32_t row0,
                             uint32_t affine) {
    const uint32_t nm = a->n_mels, T = a->frames, C = nm * (a->deltas + 1u);
    const float lo = a->lo[affine];
    const float *shift = a->shift + (size_t)(a->per_seg ? affine : 0u) * nm, *scale = a->scale + (size_t)(a->per_seg ? affine : 0u) * nm;
    auto norm = [&](float x, uint32_t j) -> float {
        volatile float s = (x > lo ? x : lo) + shift[j];
        return s * scale[j];
    };
    auto c = [&](int64_t s) -> int64_t { return s < 0 ? 0 : s > (int64_t)M - 1 ? (int64_t)M - 1 : s; };
    auto v = [&](int64_t s, uint32_t j) -> float { return norm(a->x[((size_t)seg_row + (size_t)c(s)) * nm + j], j); };
    auto delta = [&](float m2, float m1, float p1, float p2) -> float {
        volatile float d1 = p1 - m1, d2 = p2 - m2, t2 = 2.0f * d2, sum = d1 + t2;
        return sum * 0.1f;
    };
    auto d1 = [&](int64_t s, uint32_t j) -> float { s = c(s); return delta(v(s - 2, j), v(s - 1, j), v(s + 1, j), v(s + 2, j)); };
    auto d2 = [&](int64_t s, uint32_t j) -> float { return delta(d1(s - 2, j), d1(s - 1, j), d1(s + 1, j), d1(s + 2, j)); };
    for (uint32_t ch = 0; ch < C; ++ch)
        for (uint32_t tt = 0; tt < nt; ++tt) {
            const uint32_t k = ch / nm, j = ch % nm, t = t0 + tt;
            const int64_t s = (int64_t)row0 + tt;
            float val;
            if (tt >= nv) val = k ? 0.0f : a->pad_mode == VAD_BATCH_PAD_FEATURE ? norm(a->pad_value, j) : a->pad_value;
            else val = k == 0 ? v(s, j) : k == 1 ? d1(s, j) : d2(s, j);
            const size_t o = a->layout == VAD_BATCH_TIME_MAJOR ? ((size_t)window * T + t) * C + ch : ((size_t)window * C + ch) * T + t;
            if (a->dtype == VAD_BATCH_F32) static_cast<float *>(a->out)[o] = val;
            else {
                uint32_t bits;
                std::memcpy(&bits, &val, 4);
                static_cast<uint16_t *>(a->out)[o] = a->dtype == VAD_BATCH_F16 ? f16_bits(val) : melb_bf16(bits);
            }
        }
}

// model-ready windows of a feature matrix (csrc/mel_batch.hip: vadk_mel_batch): a window is its T frames, under its SEGMENT's lo,
// shift and scale
extern "C" hipError_t vadk_launch_mel_batch(const MelBatchArgs *a, hipStream_t) {
    if (a->tile != melb_tile(a->n_mels, a->deltas)) return hipErrorInvalidValue;
    for (uint32_t wi = 0; wi < a->nw; ++wi) {
        const MelBatchWin w = a->win[wi];
        if (w.nrows > a->frames || (uint64_t)w.row0 + w.nrows > w.M) return hipErrorInvalidValue;
        fake_batch_cells(a, wi, 0u, a->frames, w.nrows, w.seg_row, w.M, w.row0, w.seg);
    }
    return hipSuccess;
}

// packed windows (csrc/mel_batch.hip: vadk_mel_batch_packed): the same cells over the host's work list - the frames a workgroup
// owns, the first nv of them segment rows, the rest pad cells - with lo, shift and scale of the WINDOW
extern "C" hipError_t vadk_launch_mel_batch_packed(const MelPackArgs *p, hipStream_t) {
    const MelBatchArgs *a = &p->b;
    if (a->tile != melb_tile(a->n_mels, a->deltas)) return hipErrorInvalidValue;
    for (uint32_t b = 0; b < p->nwork; ++b) {
        const MelPackWork w = p->work[b];
        if (w.window >= a->nw || w.nt < 4 || (w.nt & 3) || (w.t0 & 3) || w.nt > a->tile || (uint64_t)w.t0 + w.nt > a->frames || w.nv > w.nt ||
            (uint64_t)w.row0 + w.nv > w.M)
            return hipErrorInvalidValue;
        fake_batch_cells(a, w.window, w.t0, w.nt, w.nv, w.seg_row, w.M, w.row0, w.window);
    }
    return hipSuccess;
}

// one finished piece of audio (csrc/scan_render.hip: vadk_scan_render), the kernel's arithmetic in plain C++, output quad by output
// quad as its workgroups are listed: per covering segment the cut's decoded, channel-selected, gated sample, times the gain, times
// the fade-in entry (or 1), times the fade-out entry (or 1) - three float32 multiplies - then the sum of the two where two segments
// cover the sample, zero where none does, and the cut's conversion.  stereo (csrc/scan_render.hip: vadk_scan_render_stereo):
// the mode bits are ignored, sample frame s takes two output values - left at 2 s, right at 2 s + 1 - under the same gain and ramp
static hipError_t fake_render(const RenderArgs *a, bool stereo = false) {
    if (stereo && a->channels != 2) return hipErrorInvalidValue;
    const size_t ch = a->channels == 2 ? 2 : 1;
    const uint32_t nramp = 4 * a->nrampq;
    for (uint32_t b = 0; b < a->nwork; ++b) {
        const RenderWork w = a->work[b];
        if (w.nquads < 1 || w.nquads > (uint32_t)CUT_WG_QUADS) return hipErrorInvalidValue;
        for (uint64_t sc = (stereo ? 8 : 4) * w.quad_out; sc < (stereo ? 8 : 4) * (w.quad_out + w.nquads); ++sc) {
            const uint64_t s = stereo ? sc >> 1 : sc;
            const int c = (int)(sc & 1);
            float acc = 0.f;
            for (int src = 0; src < 2; ++src) {
                const uint32_t si = src == 0 ? w.seg_a : w.seg_b;
                if (si == RENDER_NONE) continue;
                const CutSeg sg = a->segs[si];
                const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, qin = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
                if (s < 4 * sg.quad_out || s >= 4 * (sg.quad_out + sg.nquads)) return hipErrorInvalidValue;
                const uint64_t k = s - 4 * sg.quad_out, back = 4 * (uint64_t)sg.nquads - 1 - k;
                const size_t i = 4 * (size_t)qin + k;
                if ((i + 1) * ch * (a->fmt == VAD_FMT_F32 ? 4 : a->fmt >= VAD_FMT_ULAW8 ? 1 : 2) > a->audio_bytes) return hipErrorInvalidValue;
                float x;
                if (ch == 1) x = first_sample(a->audio, i, a->fmt, 1);
                else {
                    const float l = first_sample(a->audio, 2 * i, a->fmt, 1), r = first_sample(a->audio, 2 * i + 1, a->fmt, 1);
                    x = stereo ? (c ? r : l) : mode == SCAN_MIX ? (l + r) * 0.5f : mode == SCAN_RIGHT ? r : l;
                }
                if (a->thresh >= 0.f && !(std::fabs(x) > a->thresh)) x = 0.f;
                if (a->gains) x = x * a->gains[si];
                volatile float y = x * (k < nramp ? a->ramp[k] : 1.0f);            // (volatile: each product is rounded on its own)
                volatile float z = y * (back < nramp ? a->ramp[back] : 1.0f);
                acc = src == 0 || w.seg_a == RENDER_NONE ? (float)z : acc + z;
            }
            if (a->out_fmt == VAD_CUT_F32) static_cast<float *>(a->out)[sc] = acc;
            else {
                const float v = acc * 32767.0f;
                static_cast<int16_t *>(a->out)[sc] = (int16_t)(int)(v < -32768.0f ? -32768.0f : v > 32767.0f ? 32767.0f : v);
            }
        }
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_scan_render(const RenderArgs *a, hipStream_t) { return fake_render(a); }
extern "C" hipError_t vadk_launch_scan_render_stereo(const RenderArgs *a, hipStream_t) { return fake_render(a, true); }

// the segment table of a scan (csrc/scan_segments.hip), the kernels' arithmetic in plain C++ and in one sweep: an END is a byte with
// VAD_EV_END set and VAD_EV_REJECTED clear, its item the last one whose first index is not above it, the records in ascending
// index up to seg_cap, the true count always; the statistics over the accepted frames max(first_frame, 0) .. e, the mean from the
// fixed-point sum of rint(p * 2^30)
extern "C" hipError_t vadk_launch_scan_segments(const SegArgs *a, hipStream_t) {
    long long count = 0;
    int32_t item = 0;
    for (uint32_t k = a->first; k < a->total; ++k) {
        if ((a->events[k] & SEG_EV_MASK) != SEG_EV_END) continue;
        while ((uint32_t)a->out_start[item + 1] <= k) ++item;      // k < out_start[n]: stops at n - 1 or before
        if (count < (long long)a->seg_cap) {
            const uint32_t base = (uint32_t)a->out_start[item], e = k - base, L = (uint32_t)a->seg_frames[k];
            SegRecord r{item, (int32_t)(e - L + 1u), (int32_t)L, 0, 0.0f, 0.0f};
            long long S = 0;
            float mx = -INFINITY;
            for (uint32_t t = r.first_frame > 0 ? (uint32_t)r.first_frame : 0u; t <= e; ++t) {
                if (a->events[base + t] & EV_REJECTED) continue;
                const float p = a->probs[base + t];
                r.counted += 1;
                S += (long long)std::rint((double)p * (double)(1ll << SEG_PROB_SHIFT));
                mx = std::fmax(mx, p);
            }
            if (r.counted > 0) {
                r.mean_prob = (float)((double)S / ((double)r.counted * (double)(1ll << SEG_PROB_SHIFT)));
                r.max_prob = mx;
            }
            a->segs[count] = r;
        }
        ++count;
    }
    *a->nsegs = count;
    return hipSuccess;
}

// the statistics of a table's first min(*nsegs, seg_cap) records (csrc/scan_segments.hip: vadk_launch_seg_stats), as above
extern "C" hipError_t vadk_launch_seg_stats(const SegArgs *a, uint32_t, hipStream_t) {
    const long long all = *a->nsegs, nrec = all < (long long)a->seg_cap ? all : (long long)a->seg_cap;
    for (long long q = 0; q < nrec; ++q) {
        SegRecord &r = a->segs[q];
        const uint32_t base = (uint32_t)a->out_start[r.item], e = (uint32_t)r.first_frame + (uint32_t)r.nframes - 1u;
        long long S = 0;
        float mx = -INFINITY;
        r.counted = 0;
        r.mean_prob = r.max_prob = 0.0f;
        for (uint32_t t = r.first_frame > 0 ? (uint32_t)r.first_frame : 0u; t <= e; ++t) {
            if (a->events[base + t] & EV_REJECTED) continue;
            const float p = a->probs[base + t];
            r.counted += 1;
            S += (long long)std::rint((double)p * (double)(1ll << SEG_PROB_SHIFT));
            mx = std::fmax(mx, p);
        }
        if (r.counted > 0) {
            r.mean_prob = (float)((double)S / ((double)r.counted * (double)(1ll << SEG_PROB_SHIFT)));
            r.max_prob = mx;
        }
    }
    return hipSuccess;
}

// segment tables at other thresholds (csrc/scan_resegment.hip), in plain C++ over the real sm_step: per (set, item) in the output's
// order, the accepted frames of the item through a copy of sm0[set].  The count call leaves cnt as the exclusive prefix and the true
// counts in set_start; the fill call replays again and writes what lies below seg_cap.
static uint32_t fake_reseg_replay(const ResegArgs *a, int32_t set, int32_t item, bool fill, unsigned long long base) {
    SmSlot s = a->sm0[set];
    const uint32_t k0 = (uint32_t)a->out_start[item], k1 = (uint32_t)a->out_start[item + 1];
    uint32_t j = 0;
    for (uint32_t k = k0; k < k1; ++k) {
        if (a->events[k] & EV_REJECTED) continue;
        int L = 0;
        if (!(sm_step(s, a->probs[k], &L) & 2)) continue;
        if (fill && base + j < (unsigned long long)a->seg_cap) {
            SegRecord &r = a->segs[base + j];
            r.item = item;
            r.first_frame = (int32_t)(k - k0) - L + 1;
            r.nframes = L;
        }
        ++j;
    }
    return j;
}

extern "C" hipError_t vadk_launch_reseg_count(const ResegArgs *a, hipStream_t) {
    unsigned long long carry = 0;
    for (int32_t set = 0; set < a->nt; ++set) {
        a->set_start[set] = (long long)carry;
        for (int32_t item = 0; item < a->n; ++item) {
            const uint32_t c = fake_reseg_replay(a, set, item, false, 0);
            a->cnt[(size_t)set * (size_t)a->n + (size_t)item] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
            carry += c;
        }
    }
    a->set_start[a->nt] = (long long)carry;
    return hipSuccess;
}

// the tails (csrc/scan_tails.hip; csrc/scan_resegment.hip: vadk_tails_reseg_count), in plain C++: the length of the segment open
// behind an item's last frame out of the stream's slot, or out of a replay over the real sm_step; then one record per entry
static uint32_t fake_tail_len(const SmSlot &s, bool any) { return any && s.active != 0 && s.seg_frames >= 1 ? (uint32_t)s.seg_frames : 0u; }

extern "C" hipError_t vadk_launch_tail_snapshot(const TailArgs *a, hipStream_t) {
    for (int32_t i = 0; i < a->n; ++i) a->tail_len[i] = fake_tail_len(a->sm[a->slots[i]], a->out_start[i + 1] > a->out_start[i]);
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_reseg_tails(const ResegArgs *a, uint32_t *tail_len, hipStream_t) {
    for (int32_t set = 0; set < a->nt; ++set)
        for (int32_t item = 0; item < a->n; ++item) {
            SmSlot s = a->sm0[set];
            const uint32_t k0 = (uint32_t)a->out_start[item], k1 = (uint32_t)a->out_start[item + 1];
            uint32_t j = 0;
            for (uint32_t k = k0; k < k1; ++k) {
                if (a->events[k] & EV_REJECTED) continue;
                int L = 0;
                j += (sm_step(s, a->probs[k], &L) & 2) ? 1u : 0u;
            }
            a->cnt[(size_t)set * (size_t)a->n + (size_t)item] = j;
            tail_len[(size_t)set * (size_t)a->n + (size_t)item] = fake_tail_len(s, k1 > k0);
        }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_seg_tails(const TailArgs *a, hipStream_t) {
    for (long long q = 0; q < (long long)a->n * a->nt; ++q) {
        SegRecord r{0, 0, 0, 0, 0.0f, 0.0f};
        const uint32_t L = a->tail_len[q];
        const int32_t item = (int32_t)(q % a->n);
        const uint32_t base = (uint32_t)a->out_start[item], nf = (uint32_t)a->out_start[item + 1] - base;
        if (L != 0u && L <= 0x7fffffffu && nf != 0u) {
            r.item = item;
            r.first_frame = (int32_t)nf - (int32_t)L;
            r.nframes = (int32_t)L;
            long long S = 0;
            float mx = -INFINITY;
            for (uint32_t t = L < nf ? nf - L : 0u; t < nf; ++t) {
                if (a->events[base + t] & EV_REJECTED) continue;
                const float p = a->probs[base + t];
                r.counted += 1;
                S += (long long)std::rint((double)p * (double)(1ll << SEG_PROB_SHIFT));
                mx = std::fmax(mx, p);
            }
            if (r.counted > 0) {
                r.mean_prob = (float)((double)S / ((double)r.counted * (double)(1ll << SEG_PROB_SHIFT)));
                r.max_prob = mx;
            }
        }
        a->tails[q] = r;
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_reseg_fill(const ResegArgs *a, hipStream_t) {
    if (a->seg_cap == 0) return hipSuccess;
    for (int32_t set = 0; set < a->nt; ++set)
        for (int32_t item = 0; item < a->n; ++item)
            (void)fake_reseg_replay(a, set, item, true, a->cnt[(size_t)set * (size_t)a->n + (size_t)item]);
    return hipSuccess;
}

// the refinement (csrc/scan_refine.hip), as a plain statement of include/vad_engine.h's rule: the item's first run and its tail are
// clipped into a list, the list is merged into groups, the groups are thinned, padded and split, step by step, each on the whole list
static std::vector<SegRecord> fake_refine_item(const RefineArgs *a, int32_t item) {
    struct Span { long long s, e; };
    const long long nf = std::max(a->out_start[item + 1] - a->out_start[item], 0);
    const long long rows = std::min<long long>(std::max<long long>(*a->nsegs_in, 0), a->in_cap);
    std::vector<Span> recs, groups, kept, padded;
    auto clip = [&](const SegRecord &x) {
        const long long s = std::max<long long>(x.first_frame, 0), e = std::min<long long>((long long)x.first_frame + x.nframes, nf);
        if (x.nframes >= 1 && s < e) recs.push_back({s, e});
    };
    long long r = 0;
    while (r < rows && !(a->segs_in[r].item == item && (r == 0 || a->segs_in[r - 1].item != item))) ++r;
    for (; r < rows && a->segs_in[r].item == item; ++r) clip(a->segs_in[r]);
    if (a->tails && a->tails[item].nframes > 0) clip(a->tails[item]);
    for (size_t q = 0; q < recs.size(); ++q) {
        if (q > 0 && a->merge_gap >= 0 && recs[q].s - recs[q - 1].e <= a->merge_gap) groups.back().e = recs[q].e;
        else groups.push_back(recs[q]);
    }
    for (const Span &g : groups)
        if (g.e - g.s >= 1 && g.e - g.s >= a->min_frames) kept.push_back(g);
    const long long pb = a->pad_before, pa = a->pad_after;
    for (size_t q = 0; q < kept.size(); ++q) {
        long long left = pb, right = pa;
        if (q > 0) {
            const long long g = kept[q].s - kept[q - 1].e;
            if (g < pb + pa) left = g <= 0 ? 0 : g - g * pa / (pb + pa);
        }
        if (q + 1 < kept.size()) {
            const long long g = kept[q + 1].s - kept[q].e;
            if (g < pb + pa) right = g <= 0 ? 0 : g * pa / (pb + pa);
        }
        padded.push_back({std::max(kept[q].s - left, 0ll), std::min(kept[q].e + right, nf)});
    }
    std::vector<SegRecord> out;
    const uint32_t base = (uint32_t)a->out_start[item];
    for (const Span &g : padded) {
        const long long len = g.e - g.s, mf = a->max_frames;
        if (mf <= 0 || len <= mf) {
            out.push_back(SegRecord{item, (int32_t)g.s, (int32_t)len, 0, 0.0f, 0.0f});
            continue;
        }
        const long long k = (len + mf - 1) / mf, sz = (len + k - 1) / k, h = (mf - sz) / 2;
        long long b = g.s;
        for (long long j = 1; j <= k; ++j) {
            long long next = g.e;
            if (j < k) {
                const long long c = g.s + j * len / k;
                next = c;
                // "smallest" is by bit pattern, as the header says: value order for every probability with the sign bit clear
                uint32_t best = 0;
                bool any = false;
                for (long long t = std::max(c - h, 0ll); t <= std::min(c + h, nf - 1); ++t) {
                    if (a->events[base + t] & EV_REJECTED) continue;
                    uint32_t bits;
                    std::memcpy(&bits, &a->probs[base + t], sizeof bits);
                    if (!any || bits < best) best = bits, next = t, any = true;
                }
            }
            out.push_back(SegRecord{item, (int32_t)b, (int32_t)(next - b), 0, 0.0f, 0.0f});
            b = next;
        }
    }
    return out;
}

extern "C" hipError_t vadk_launch_refine_count(const RefineArgs *a, hipStream_t) {
    unsigned long long carry = 0;
    for (int32_t i = 0; i < a->n; ++i) {
        a->cnt[i] = carry;
        carry += fake_refine_item(a, i).size();
    }
    *a->nsegs_out = (long long)carry;
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_refine_fill(const RefineArgs *a, hipStream_t) {
    for (int32_t i = 0; i < a->n; ++i) {
        const std::vector<SegRecord> recs = fake_refine_item(a, i);
        for (size_t j = 0; j < recs.size(); ++j)
            if (a->cnt[i] + j < (unsigned long long)a->seg_cap) a->segs_out[a->cnt[i] + j] = recs[j];
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_silero_v5_t16_rates(const StepParams *p, const RateParams *r, hipStream_t) {
    for (int k = 0; k < r->nseg; ++k) {
        StepParams q = *p;
        q.n = r->seg[k].n;
        q.T = 1;
        q.fmt = VAD_FMT_F32;
        q.frames = r->seg[k].in;
        q.slots = p->slots ? p->slots + r->seg[k].stream0 : nullptr;
        q.probs = p->probs + r->seg[k].stream0;
        q.events = p->events ? p->events + r->seg[k].stream0 : nullptr;
        q.seg_frames = p->seg_frames ? p->seg_frames + r->seg[k].stream0 : nullptr;
        fake_step(&q, r->seg[k].n_in);                         // a chunk's first sample stands for its resampled frame's
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_resample(const ResampleParams *p, hipStream_t) {
    for (int k = 0; k < p->nseg; ++k)
        for (int i = 0; i < p->seg[k].n; ++i) {
            float *o = p->seg[k].out + (size_t)i * 512;
            std::memset(o, 0, 512 * sizeof(float));
            o[0] = p->seg[k].in[(size_t)i * p->seg[k].n_in];
        }
    return hipSuccess;
}

// one window of a rate scan (csrc/scan_resample.hip: vadk_scan_resample), the rule of vadk_launch_resample above on chunks framed
// out of the block as the kernel frames them: row i W + tt = a frame of zeros whose first sample is the first decoded, channel-
// selected sample of chunk t0 + tt of item i (a NaN when the float32 chunk holds a NaN / Inf, as the real operator spreads one
// over the frame); rows past an item's last chunk are not written.  And the window's item table, as the kernel writes it.
extern "C" hipError_t vadk_launch_scan_resample(const ScanResampleArgs *a, hipStream_t) {
    const bool two = a->channels == 2;
    const size_t fb = (size_t)(two ? 2 : 1) * (a->fmt == VAD_FMT_F32 ? 4 : a->fmt >= VAD_FMT_ULAW8 ? 1 : 2);
    for (int i = 0; i < a->live; ++i) {
        const ScanItem it = a->items[i];
        const uint32_t mode = it.quad0 >> SCAN_MODE_SHIFT, quad0 = it.quad0 & ((1u << SCAN_MODE_SHIFT) - 1u);
        auto sample = [&](size_t k) -> float {
            if (!two) return first_sample(a->audio, k, a->fmt, 1);
            const float l = first_sample(a->audio, 2 * k, a->fmt, 1), r = first_sample(a->audio, 2 * k + 1, a->fmt, 1);
            return mode == SCAN_MIX ? (l + r) * 0.5f : mode == SCAN_RIGHT ? r : l;
        };
        const int left = it.nframes - a->t0, nw = left < 0 ? 0 : left > a->W ? a->W : left;
        for (int tt = 0; tt < nw; ++tt) {
            const size_t first = 4 * ((size_t)quad0 + (size_t)(a->t0 + tt) * a->hopq);
            if ((first + (size_t)a->n_in) * fb > a->audio_bytes) return hipErrorInvalidValue;
            float *o = a->win + ((size_t)i * a->W + tt) * 512;
            std::memset(o, 0, 512 * sizeof(float));
            o[0] = sample(first);
            if (a->fmt == VAD_FMT_F32)
                for (int k = 0; k < a->n_in; ++k)
                    if (!std::isfinite(sample(first + k))) o[0] = std::nanf("");
        }
        a->items_win[i] = ScanItem{it.slot, (uint32_t)i * (uint32_t)a->W * 128u, nw, it.out0 + (uint32_t)a->t0};
    }
    return hipSuccess;
}

// one window of a rate cut's frames (csrc/scan_cut_resample.hip: vadk_cut_resample), under the rule of vadk_launch_scan_resample
// above: row r of the call = a frame of zeros whose first sample is the first decoded, channel-selected sample of chunk r - row0 of
// the segment that owns the row (a NaN when the float32 chunk holds a NaN / Inf), written at row r - r0 of the window.  The row's
// segment is found as the kernel finds it: from the tile's first segment on.
extern "C" hipError_t vadk_launch_cut_resample(const CutResampleArgs *a, hipStream_t) {
    const bool two = a->channels == 2;
    const size_t fb = (size_t)(two ? 2 : 1) * (a->fmt == VAD_FMT_F32 ? 4 : a->fmt >= VAD_FMT_ULAW8 ? 1 : 2);
    if (a->r0 % (uint32_t)MT) return hipErrorInvalidValue;
    for (uint32_t r = a->r0; r < a->rows_end; ++r) {
        uint32_t s = a->tile_seg[r / (uint32_t)MT];
        if (a->segs[s].row0 > r - r % (uint32_t)MT) return hipErrorInvalidValue;
        int steps = 0;
        while (a->segs[s + 1].row0 <= r) ++s, ++steps;
        if (steps >= MT) return hipErrorInvalidValue;
        const CutResampleSeg sg = a->segs[s];
        const uint32_t mode = sg.quad_in >> SCAN_MODE_SHIFT, quad0 = sg.quad_in & ((1u << SCAN_MODE_SHIFT) - 1u);
        auto sample = [&](size_t k) -> float {
            if (!two) return first_sample(a->audio, k, a->fmt, 1);
            const float l = first_sample(a->audio, 2 * k, a->fmt, 1), rr = first_sample(a->audio, 2 * k + 1, a->fmt, 1);
            return mode == SCAN_MIX ? (l + rr) * 0.5f : mode == SCAN_RIGHT ? rr : l;
        };
        const size_t first = 4 * ((size_t)quad0 + (size_t)(r - sg.row0) * a->hopq);
        if ((first + (size_t)a->n_in) * fb > a->audio_bytes) return hipErrorInvalidValue;
        float *o = a->win + (size_t)(r - a->r0) * 512;
        std::memset(o, 0, 512 * sizeof(float));
        o[0] = sample(first);
        if (a->fmt == VAD_FMT_F32)
            for (int k = 0; k < a->n_in; ++k)
                if (!std::isfinite(sample(first + k))) o[0] = std::nanf("");
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_g711_expand(const void *d_in, int16_t *d_out, int64_t nbytes, int alaw, hipStream_t) {
    for (int64_t i = 0; i < nbytes; ++i) d_out[i] = g711_pcm(static_cast<const uint8_t *>(d_in)[i], alaw != 0);
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_rsg_partial(const RsgParams *, hipStream_t) { return hipErrorInvalidValue; }
extern "C" hipError_t vadk_launch_rsg_finish(const RsgParams *, hipStream_t) { return hipErrorInvalidValue; }
extern "C" hipError_t vadk_rsf_build_tables(const RsfParams *, hipStream_t) { return hipErrorInvalidValue; }
extern "C" hipError_t vadk_rsf_run(const RsfParams *, hipStream_t) { return hipErrorInvalidValue; }

extern "C" hipError_t vadk_launch_slot_control(SmSlot *sm, float *state, const int32_t *slots, int n, int op, const SmSlot *def,
                                               const vad_thresholds *thr, int nthr, hipStream_t) {
    for (int i = 0; i < n; ++i) {                              // csrc/vad_util.hip: vadk_slot_control, statement for statement
        const int s = slots[i];
        if (op & 1) std::memset(state + (size_t)s * 256, 0, 256 * sizeof(float));
        SmSlot cur = sm[s];
        if (op & 2) cur = *def;
        if (op & 4) {
            SmSlot fresh = *def;
            fresh.start_prob = cur.start_prob; fresh.end_prob = cur.end_prob;
            fresh.start_ratio = cur.start_ratio; fresh.end_ratio = cur.end_ratio;
            fresh.start_count = cur.start_count; fresh.end_count = cur.end_count;
            cur = fresh;
        }
        if (op & 8) {
            const vad_thresholds t = thr[nthr == 1 ? 0 : i];
            cur.start_prob = t.start_probability; cur.end_prob = t.end_probability;
            cur.start_ratio = t.start_ratio; cur.end_ratio = t.end_ratio;
            cur.start_count = t.start_frame_count; cur.end_count = t.end_frame_count;
        }
        sm[s] = cur;
    }
    return hipSuccess;
}

extern "C" hipError_t vadk_launch_sm_replay(SmSlot *sm, int slot, const float *probs, int n, uint8_t *events, int32_t *seg, hipStream_t) {
    SmSlot s = sm[slot];
    for (int i = 0; i < n; ++i) {
        int sg = 0;
        const int ev = sm_step(s, probs[i], &sg);
        events[i] = (uint8_t)ev;
        seg[i] = (ev & 2) ? sg : 0;
    }
    sm[slot] = s;
    return hipSuccess;
}
