// Developer micro-benchmark for the fused V5 kernel (not part of the product, not a test).
//
//   tools/kbench.sh [-DVADK_STAMPS] -- <B> <steps>
//
// Builds silero_v5.hip + pack_weights.cpp directly (so kernel variants can be compiled with
// extra -D flags on the GPU box) and times back-to-back launches with hipEvents.  With
// -DVADK_STAMPS the kernel records s_memtime at every phase boundary per wave and this program
// prints the per-phase cycle budget (shares only: stamped builds are slower, see
// cdna_hip_programming.md "In-kernel stamps").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../cutter_vad_amd/csrc/pack_weights.h"
#include "../cutter_vad_amd/csrc/vad_layout.h"

extern "C" hipError_t vadk_launch_silero_v5(const vadk::StepParams *p, hipStream_t stream);
#ifdef KB_TILE16      // tools/kbench16.sh: the 16-stream tile kernel (link silero_v5_t16.hip instead of silero_v5.hip)
extern "C" hipError_t vadk_launch_silero_v5_t16(const vadk::StepParams *p, hipStream_t stream);
extern "C" hipError_t vadk_launch_silero_v5_t16_pair(const vadk::StepParams *p, hipStream_t stream);
// KB_PAIR=1: the paired launch (two tiles per workgroup, one-frame calls only); the stamps stay indexed by tile and wave
static bool kb_pair = false;
static hipError_t kb_launch16(const vadk::StepParams *p, hipStream_t stream) {
    return kb_pair ? vadk_launch_silero_v5_t16_pair(p, stream) : vadk_launch_silero_v5_t16(p, stream);
}
#define vadk_launch_silero_v5 kb_launch16
#define PACK vadk::pack_silero_v5_t16
#else
#define PACK vadk::pack_silero_v5
#endif

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));         \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

int main(int argc, char **argv) {
    const char *blob_path = argc > 1 ? argv[1] : "cutter_vad_amd/weights/silero_v5_16k.svw";
    const int B = argc > 2 ? atoi(argv[2]) : 8192;
    const int K = argc > 3 ? atoi(argv[3]) : 100;
    const int T = argc > 4 ? atoi(argv[4]) : 1;
#ifdef KB_TILE16
    kb_pair = getenv("KB_PAIR") && atoi(getenv("KB_PAIR")) != 0;
    if (kb_pair && T != 1) { fprintf(stderr, "KB_PAIR: one frame per call\n"); return 1; }
    if (kb_pair) printf("paired launch: %d workgroups of 512 threads\n", ((B + 15) / 16 + 1) / 2);
#endif
    FILE *f = fopen(blob_path, "rb");
    if (!f) { perror(blob_path); return 1; }
    std::vector<unsigned char> blob;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    vadk::PackedWeights pw;
    std::string err;
    if (!PACK(blob.data(), blob.size(), pw, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }

    vadk::StepParams p{};
    float *d_w, *d_state, *d_frames, *d_probs;
    vadk::SmSlot *d_sm;
    CK(hipMalloc(&d_w, pw.data.size() * 4));
    CK(hipMemcpy(d_w, pw.data.data(), pw.data.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&d_state, (size_t)B * 256 * 4));
    CK(hipMemset(d_state, 0, (size_t)B * 256 * 4));
    std::vector<vadk::SmSlot> sm(B);
    for (auto &s : sm) { memset(&s, 0, sizeof s); s.start_prob = s.end_prob = 0.7; s.start_ratio = 0.8; s.end_ratio = 0.95; s.start_count = 10; s.end_count = 50; s.seg_frames = -1; }
    CK(hipMalloc(&d_sm, sizeof(vadk::SmSlot) * B));
    CK(hipMemcpy(d_sm, sm.data(), sizeof(vadk::SmSlot) * B, hipMemcpyHostToDevice));
    const int RING = getenv("KB_RING") ? atoi(getenv("KB_RING")) : 8;
    const float sigma = getenv("KB_SIGMA") ? (float)atof(getenv("KB_SIGMA")) : 0.1f;
    std::vector<float> fr((size_t)RING * B * T * 512);
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, sigma);
    for (auto &v : fr) v = nd(rng);
    CK(hipMalloc(&d_frames, fr.size() * 4));
    CK(hipMemcpy(d_frames, fr.data(), fr.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&d_probs, (size_t)B * T * 4));
    p.wstream = d_w;
    p.wstream_bytes = (uint32_t)(pw.data.size() * 4);
    if (!pw.data_x.empty()) {        // the second stream (the 16-stream V5 packing's split encoder.0)
        float *d_wx;
        CK(hipMalloc(&d_wx, pw.data_x.size() * 4));
        CK(hipMemcpy(d_wx, pw.data_x.data(), pw.data_x.size() * 4, hipMemcpyHostToDevice));
        p.wstream_x = d_wx;
        p.wstream_x_bytes = (uint32_t)(pw.data_x.size() * 4);
    }
    if (!pw.data_y.empty()) {        // the third stream (the 16-stream V5 packing's split encoder.1), the split enc2 / enc3 behind it
        pw.data_y.insert(pw.data_y.end(), pw.data_z.begin(), pw.data_z.end());
        pw.data_y.insert(pw.data_y.end(), pw.data_d.begin(), pw.data_d.end());      // and the split DFT behind those
        float *d_wy;
        CK(hipMalloc(&d_wy, pw.data_y.size() * 4));
        CK(hipMemcpy(d_wy, pw.data_y.data(), pw.data_y.size() * 4, hipMemcpyHostToDevice));
        p.wstream_y = d_wy;
        p.wstream_y_bytes = (uint32_t)(pw.data_y.size() * 4);
    }
    memcpy(p.sect, pw.sect, sizeof pw.sect);
    p.state = d_state; p.sm = d_sm; p.slots = nullptr; p.probs = d_probs; p.events = nullptr; p.seg_frames = nullptr;
    p.n = B; p.T = T; p.fmt = 0; p.thresh = 0.01f;
    if (getenv("KB_SLOTS")) {          // identity slot map, like vad_step_device
        std::vector<int> sl(B);
        for (int i = 0; i < B; ++i) sl[i] = i;
        int *d_sl; CK(hipMalloc(&d_sl, B * 4)); CK(hipMemcpy(d_sl, sl.data(), B * 4, hipMemcpyHostToDevice));
        p.slots = d_sl;
    }
    if (getenv("KB_EVENTS")) { unsigned char *d_ev; CK(hipMalloc(&d_ev, (size_t)B * T)); p.events = d_ev; }
#ifdef VADK_STAMPS
#ifdef KB_TILE16
    const int tiles = ((B + 15) / 16 + 1) & ~1;      // (a paired launch's last workgroup stamps both its halves)
#else
    const int tiles = (B + vadk::MT - 1) / vadk::MT;
#endif
    unsigned long long *d_st;
    CK(hipMalloc(&d_st, (size_t)tiles * 4 * 32 * 8));
    CK(hipMemset(d_st, 0, (size_t)tiles * 4 * 32 * 8));
    p.stamps = d_st;
#endif
    hipStream_t s;
    CK(hipStreamCreate(&s));
    for (int i = 0; i < 5; ++i) { p.frames = d_frames + (size_t)(i % RING) * B * T * 512; CK(vadk_launch_silero_v5(&p, s)); }
    CK(hipStreamSynchronize(s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> rounds;
    // KB_SPLIT=n: the B streams as n independent groups, each stepped K times on a HIP stream of its own - the groups' launches are
    // not ordered against each other, so the start of one group's launch runs under the other groups' tiles
    const int NS = getenv("KB_SPLIT") ? atoi(getenv("KB_SPLIT")) : 1;
    std::vector<hipStream_t> ss(NS, s);
    std::vector<hipEvent_t> ej(NS);
    for (int g = 1; g < NS; ++g) CK(hipStreamCreate(&ss[g]));
    for (int g = 0; g < NS; ++g) CK(hipEventCreate(&ej[g]));
    for (int r = 0; r < 5; ++r) {
        CK(hipEventRecord(e0, s));
        if (NS == 1) {
            for (int i = 0; i < K; ++i) { p.frames = d_frames + (size_t)(i % RING) * B * T * 512; CK(vadk_launch_silero_v5(&p, s)); }
        } else {
            const int per = B / NS;
            static std::vector<float *> wcopy;           // KB_SPLIT_OWN_WEIGHTS: a copy of the weight stream per group (two engines)
            if (getenv("KB_SPLIT_OWN_WEIGHTS") && wcopy.empty()) {
                wcopy.assign(NS, d_w);
                for (int g = 1; g < NS; ++g) {
                    CK(hipMalloc(&wcopy[g], pw.data.size() * 4));
                    CK(hipMemcpy(wcopy[g], d_w, pw.data.size() * 4, hipMemcpyDeviceToDevice));
                }
            }
            for (int g = 1; g < NS; ++g) CK(hipStreamWaitEvent(ss[g], e0, 0));
            for (int i = 0; i < K; ++i)
                for (int g = 0; g < NS; ++g) {
                    vadk::StepParams q = p;
                    q.n = per;
                    q.state = p.state + (size_t)g * per * 256;
                    q.sm = p.sm + (size_t)g * per;
                    q.probs = p.probs + (size_t)g * per * T;
                    q.frames = d_frames + ((size_t)(i % RING) * B + (size_t)g * per) * T * 512;
                    if (!wcopy.empty()) q.wstream = wcopy[g];
                    CK(vadk_launch_silero_v5(&q, ss[g]));
                }
            for (int g = 1; g < NS; ++g) { CK(hipEventRecord(ej[g], ss[g])); CK(hipStreamWaitEvent(s, ej[g], 0)); }
        }
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        rounds.push_back(ms * 1e3f / K);
    }
    std::sort(rounds.begin(), rounds.end());
    const double us = rounds[rounds.size() / 2];
    const double fps = (double)B * T / (us * 1e-6);
    printf("B=%d T=%d: median %.1f us/launch (min %.1f)  %.2f M frames/s  %.1f TFLOP/s = %.3f of fp32 peak\n", B, T, us,
           rounds[0], fps / 1e6, fps * 988160 / 1e12, fps * 988160 / 157.3e12);
#ifdef VADK_STAMPS
    std::vector<unsigned long long> st((size_t)tiles * 4 * 32);
    CK(hipMemcpy(st.data(), d_st, st.size() * 8, hipMemcpyDeviceToHost));
    static const char *names[16] = {"", "load", "bar1", "stft", "bar2", "enc0", "bar3", "enc1", "bar4", "enc2", "bar5", "enc3", "bar6", "lstm", "bar7", "cell+bar8"};
    auto S = [&](int b, int w, int k) { return st[((size_t)b * 4 + w) * 32 + k]; };
    for (int w = 0; w < 4; ++w) {
        printf("wave %d:", w);
        double tot = 0;
        for (int k = 1; k < 16; ++k) {
            double acc = 0;
            for (int b = 0; b < tiles; ++b) acc += (double)(S(b, w, k) - S(b, w, k - 1));
            acc /= tiles;
            tot += acc;
            printf(" %s=%.0f", names[k], acc);
        }
        double l1 = 0, l2 = 0, l3 = 0;
        for (int b = 0; b < tiles; ++b) { l1 += (double)(S(b, w, 16) - S(b, w, 2)); l2 += (double)(S(b, w, 17) - S(b, w, 4)); l3 += (double)(S(b, w, 18) - S(b, w, 12)); }
#ifdef KB_TILE16      // the 16-stream body stamps the end of the LSTM's main loop only, and one ingest group per STFT column
        printf("  total=%.0f | mainloops: lstm=%.0f\n", tot, l3 / tiles);
        const int ngroups = 3;
        if (kb_pair) {
            // the paired kernel runs frames first: folds, barrier (1), STFT .. enc3, then the recurrent half (stamps 31 .. 26) inside the
            // phase printed as enc3, in front of barrier (6); its ingest groups are printed since kernel entry, further down
            double e3 = 0, rh = 0;
            for (int b = 0; b < tiles; ++b) { e3 += (double)(S(b, w, 31) - S(b, w, 10)); rh += (double)(S(b, w, 26) - S(b, w, 31)); }
            printf("        of enc3 above: enc3 itself = %.0f, recurrent half = %.0f\n", e3 / tiles, rh / tiles);
        }
        printf("        ingest groups (a column's quads have arrived, in front of its fold; cycles since frame start):");
#else
        printf("  total=%.0f | mainloops: stft=%.0f enc0=%.0f lstm=%.0f\n", tot, l1 / tiles, l2 / tiles, l3 / tiles);
        const int ngroups = 8;
        printf("        ingest groups (cycles since frame start):");
#endif
        for (int k = 20; k < 20 + ngroups; ++k) {
            double acc = 0;
            for (int b = 0; b < tiles; ++b) acc += (double)(S(b, w, k) - S(b, w, 0));
            printf(" g%d=%.0f", k - 20, acc / tiles);
        }
        double pro = 0;
        for (int b = 0; b < tiles; ++b) pro += (double)(S(b, w, 0) - S(b, w, 19));
        printf("   prologue (kernel entry -> frame loop) = %.0f\n", pro / tiles);
        // (s_memtime is a per-CU counter: stamps of different tiles cannot be set against each other)
        double a29 = 0, a30 = 0, a31 = 0;
        for (int b = 0; b < tiles; ++b) {
            a29 += (double)(S(b, w, 29) - S(b, w, 19)); a30 += (double)(S(b, w, 30) - S(b, w, 19)); a31 += (double)(S(b, w, 31) - S(b, w, 19));
        }
#ifdef KB_TILE16
        {   // every wave: barrier (8) -> its last store issued (27) -> all its stores acknowledged (28)
            double ti = 0, ta = 0;
            for (int b = 0; b < tiles; ++b) { ti += (double)(S(b, w, 27) - S(b, w, 15)); ta += (double)(S(b, w, 28) - S(b, w, 27)); }
            printf("        tail: barrier (8) -> last store issued = %.0f, -> stores acknowledged = +%.0f;  kernel entry -> end = %.0f\n", ti / tiles,
                   ta / tiles, pro / tiles + tot + (ti + ta) / tiles);
        }
#else
        if (w == 0 && S(0, 0, 28)) {
            double tl = 0;
            for (int b = 0; b < tiles; ++b) tl += (double)(S(b, 0, 28) - S(b, 0, 15));
            printf("        head + state machine (32 lanes of wave 0, behind barrier (8)) = %.0f\n", tl / tiles);
        }
#endif
#ifdef KB_TILE16
        if (kb_pair) {
            double g[3] = {0, 0, 0}, b1 = 0, r1 = 0;
            for (int b = 0; b < tiles; ++b) {
                for (int k = 0; k < 3; ++k) g[k] += (double)(S(b, w, 20 + k) - S(b, w, 19));
                b1 += (double)(S(b, w, 2) - S(b, w, 19)); r1 += (double)(S(b, w, 26) - S(b, w, 19));
            }
            printf("        since kernel entry: all first requests issued %.0f, frame column 0 / 1 / 2 arrived %.0f / %.0f / %.0f, past barrier (1) %.0f,\n"
                   "                            h in LDS (behind barrier (4)) %.0f, recurrent half %.0f .. %.0f\n",
                   a29 / tiles, g[0] / tiles, g[1] / tiles, g[2] / tiles, b1 / tiles, a30 / tiles, a31 / tiles, r1 / tiles);
        } else
#endif
        if (S(0, w, 29)) printf("        since kernel entry: all first requests issued %.0f, h in LDS %.0f, past barrier (0) %.0f\n", a29 / tiles, a30 / tiles, a31 / tiles);
    }
#ifdef KB_TILE16
    if (kb_pair) {
        // The end of the launch by half: wave (hf, w) = wave w of tile 2 b + hf.  The two tiles of a workgroup share a CU and its
        // counter, so their stamps compare: cycles since wave (0, w) passed barrier (6).  A build whose cell runs in place (no
        // barrier (7)) stamps 14 at the end of its cell, 15 behind barrier (8) and 16 behind (8b); before that 14 was behind
        // barrier (7), 15 behind (8) and 16 is not written.
        const bool inplace = S(0, 0, 16) != 0;
        const int wgs = tiles / 2;
        printf("launch end by half, cycles since wave (0, w) passed barrier (6); %s\n",
               inplace ? "cell in place: input half end, cell end, behind (8), behind (8b), last store issued, acknowledged"
                       : "input half end, behind (7), behind (8), last store issued, acknowledged");
        for (int w = 0; w < 4; ++w) {
            for (int hf = 0; hf < 2; ++hf) {
                const int ks[6] = {13, 14, 15, 16, 27, 28};
                printf("wave (%d, %d):", hf, w);
                for (int k : ks) {
                    if (k == 16 && !inplace) continue;
                    double acc = 0;
                    for (int b = 0; b < wgs; ++b) acc += (double)((long long)S(2 * b + hf, w, k) - (long long)S(2 * b, w, 12));
                    printf(" %.0f", acc / wgs);
                }
                printf("\n");
            }
            double sk = 0, ab = 0, lo = 1e30, hi = -1e30;
            int older1 = 0;
            for (int b = 0; b < wgs; ++b) {
                const double d = (double)((long long)S(2 * b + 1, w, 13) - (long long)S(2 * b, w, 13));
                sk += d; ab += d < 0 ? -d : d; lo = std::min(lo, d); hi = std::max(hi, d);
                older1 += d < 0;
            }
            printf("        skew at the end of the input half, wave (1, %d) - wave (0, %d): mean %.0f, mean |.| %.0f, min %.0f, max %.0f; wave (1, w) first in %d of %d workgroups\n",
                   w, w, sk / wgs, ab / wgs, lo, hi, older1, wgs);
        }
    }
#endif
#endif
    return 0;
}
