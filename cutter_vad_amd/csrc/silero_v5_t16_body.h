// The body of the 16-stream Silero V5 step kernel: the text between the braces of a __global__ function, included by
// silero_v5_t16.hip once per entry point (silero_v5_step16, silero_v5_step16_g711, silero_v5_scan16) - textually, not as a __device__ function the
// entries call: the compiler schedules and allocates an inlined callee differently (other register counts for every existing
// instantiation), and the float32 / int16 kernels were to stay instruction for instruction what they were.  The including
// function provides the arguments k_wstream .. k_T, P, R and the constants FMT (wire format: 0 float32, 1 int16 of either scale,
// 2 / 3 ITU-T G.711 mu-law / A-law, one byte per sample), RS, K8, ONE, SCAN (silero_v5_t16.hip explains them).  SCAN: the entry
// also provides k_items and S (vad_layout.h: ScanItem, ScanArgs); the other entries a null k_items and an empty S.
// CH: the channels of the audio block, 1 everywhere but in the scan of interleaved two-channel recordings (silero_v5_stereo16).
// PAIR (silero_v5_pair16): the workgroup is TWO tiles - 512 threads, wave (hf, w) = wave w of half-tile hf with its own half of the LDS;
// `tid` is the thread's index inside its half, tilei its tile, ldsO the partner half's LDS.  Both halves run every barrier.
// XFIRST (silero_v5_pair16 only): the one-frame launch's phase order - the frame is requested first and folded as it arrives, with
// nothing of the state in front of barrier (1); h_{t-1} goes to its planes behind barrier (4) and the recurrent gate half runs behind
// enc3, in front of barrier (6).  Every other entry keeps the order of the frame loop: the recurrent half first, the ingest under it.
#define KP(f) k_##f
    using namespace vadk::v5;
    constexpr bool F32IN = FMT == 0;
    constexpr bool G711 = FMT >= 2;
    static_assert(!RS || F32IN, "resampled frames are float32");
    static_assert(!(RS && K8), "the fused resampler feeds the 16 kHz model");
    static_assert(!SCAN || (!RS && !ONE), "a scan is the frame-loop form on audio in HBM");
    static_assert(CH == 1 || (CH == 2 && SCAN), "two interleaved channels: whole recordings only");
    static_assert(!PAIR || (ONE && !RS && !K8 && !G711 && !SCAN), "paired tiles: one-frame calls of the 16 kHz model, float32 / int16");
    static_assert(!XFIRST || PAIR, "frames first: the paired one-frame kernel (no next frame whose h the cell would hand on)");
    constexpr int QL = K8 ? 8 : 16;               // loader lanes per stream = quads per quarter column
    constexpr int CS = 4 * QL;                    // folded-operand rows per column
    constexpr int PP = K8 ? 24 : 48;              // quad rows per |STFT| column (enc0's input) as planes: 12 per K-step
    constexpr int LDS_HALF = T_LDS_F4 + (RS ? MT16 * FQ : 0) + (F32IN ? T_FLAG_F4 : 0);
    static_assert(!PAIR || 2 * LDS_HALF * 16 <= 160 * 1024, "both halves' LDS on one CU");
    __shared__ f32x4 lds[(PAIR ? 2 : 1) * LDS_HALF];     // RS: + the tile's 16 kHz frames F (one workgroup per CU either way)
    const int hf = PAIR ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8) : 0;
    f32x4 *const ldsH = PAIR ? lds + hf * LDS_HALF : lds;     // the tile's LDS (PAIR: its half of the workgroup's)
    [[maybe_unused]] f32x4 *const ldsO = PAIR ? lds + (1 - hf) * LDS_HALF : lds;
    f32x4 *const RX = ldsH;
    [[maybe_unused]] f32x4 *const REV = ldsH + T_EVEN_Q;   // 16 kHz: the even tile's folded operands, loader view
    f32x4 *const RE = ldsH + T_ROW_E * QSD;
    f32x4 *const RP0 = ldsH + T_ROW_E0 * QSD;
    f32x4 *const RH = ldsH + T_ROW_H * QSD;
    float *const headp = reinterpret_cast<float *>(RH + T_ROWS_H * QSD);   // [4][16]
    float *const nyqv = headp + 64;              // [3][16]
    float *const fcor = nyqv + 48;               // [3 columns][y128, a64, b64][16 streams]
    constexpr int FCOR_SINK = 144;               // [64] floats after fcor
    SmSlot *const smL = reinterpret_cast<SmSlot *>(fcor + 144 + 64);
    f32x4 *const biasL = reinterpret_cast<f32x4 *>(smL + MT16);          // gate biases, compact: [4 waves][4 gates][8 quads of units]
    // F32IN: [2][16] bytes, stream s rejected when flagL[s] (8 kHz: flagL[s] | flagL[16 + s], the two halves of the workgroup)
    uint8_t *const flagL = reinterpret_cast<uint8_t *>(ldsH + T_LDS_F4 + (RS ? MT16 * FQ : 0));

    const int tid = PAIR ? (int)threadIdx.x & 255 : (int)threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    [[maybe_unused]] const int tilei = PAIR ? 2 * (int)blockIdx.x + hf : (int)blockIdx.x;
    if constexpr (!RS) STAMP(19);                 // kernel entry
    const int n = lane & 15;                      // stream of this lane's MFMA column
    const int kq = lane >> 4;                     // channel group (B operand) = row quad of the D tile
    const int nq = kq * QSD + n;                  // lane's offset inside a group of 4 quad rows (dense view)
    const int nqL = kq * QSL + n;                 // the same in the loader view
    // RS: the tile carries the virtual streams 16 b .. 16 b + 15 of the segments laid end to end (vad_layout.h); which segment a
    // column belongs to is a handful of compares on kernel arguments
    const int vcol = (PAIR ? tilei : (int)blockIdx.x) * MT16 + n;
    int gf = vcol;
    bool live = vcol < KP(n);
    if constexpr (RS) {
        int s0 = R.seg[0].stream0, vs = 0;
#pragma unroll
        for (int k = 1; k < RATE_MAX_SEGS; ++k)
            if (k < R.nseg && vcol >= R.seg[k].vstart) { s0 = R.seg[k].stream0; vs = R.seg[k].vstart; }
        gf = s0 + vcol - vs;
        live = vcol < R.total;
    }
    const int tile0 = (PAIR ? tilei : (int)blockIdx.x) * MT16;                      // (not RS: the tile's first stream in the call's arrays)
    // SCAN: the stream of this lane's MFMA column is work item vcol: its slot, how many of its frames lie at and behind the
    // launch's first (ncol; frame t of the launch is held for this column when t >= ncol) and where its results go; the
    // loader's stream (item tile0 + lms, below) gives this thread the quad its frames start at.  Items past the table: no frames.
    int slot, ncol = 0;
    uint32_t obase = 0;
    if constexpr (SCAN) {
        const u32x4 it = live ? *reinterpret_cast<const u32x4 *>(k_items + vcol) : u32x4{0u, 0u, 0u, 0u};
        slot = (int)it.x;
        ncol = (int)it.z - S.t0;
        obase = it.w + (uint32_t)S.t0;
    } else {
        slot = live ? (KP(slots) ? KP(slots)[gf] : gf) : 0;
    }
    // PAIR: the lane's stream in the partner half's tile.  The wave runs the cell of its row tile for both tiles (behind the input
    // half), so it needs that stream's c_{t-1} and where its h' and c' go; nothing in front of barrier (1) waits for this load.
    // (a column past n takes stream 0's slot: it reads that c and stores nothing, as such columns of the own tile read slot 0's.  No
    //  select BEHIND the load - it would put a wait for the load here, in front of the frame's requests)
    [[maybe_unused]] bool live_o = false;
    [[maybe_unused]] int slot_o = 0;
    if constexpr (PAIR) {
        const int vcol_o = (tilei ^ 1) * MT16 + n;
        live_o = vcol_o < KP(n);
        slot_o = live_o ? vcol_o : 0;
        if (KP(slots)) slot_o = KP(slots)[slot_o];
    }
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(KP(wstream)), 0, (int)KP(wstream_bytes), 0x00020000);
    const int lane16 = lane * 16;
#define WL(blk) ldw(wrs, lane16, (blk))
    // the second weight stream: encoder.0 on the bf16 split (S_ENC0_X3)
    const __amdgpu_buffer_rsrc_t wrx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.wstream_x), 0, (int)P.wstream_x_bytes, 0x00020000);
#define WX(blk) ldw(wrx, lane16, (blk))
    // the third: encoder.1 on the bf16 split (S_ENC1_X3)
    const __amdgpu_buffer_rsrc_t wry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.wstream_y), 0, (int)P.wstream_y_bytes, 0x00020000);
#define WY(blk) ldw(wry, lane16, (blk))
    const int o_stft = (int)P.sect[w][S_STFT], o_nyq = (int)P.sect[w][S_NYQ], o_x0 = (int)P.sect[w][S_ENC0_X3];
    // enc2 and enc3 on the bf16 split: the fourth block range, behind the third stream in its buffer (vad_layout.h, ENC23_X3_BLOCKS)
    const int o_y1 = (int)P.sect[w][S_ENC1_X3], o_z = 4 * ENC1_X3_BLOCKS + w * ENC23_X3_BLOCKS;
    const int o_l = (int)P.sect[w][S_LSTM], o_x3 = (int)P.sect[w][S_LSTM_X3];
    // SCAN: the items are sorted by frame count, so the tile's first item has the most: its count, clipped to the launch's window
    int T = (ONE || RS) ? 1 : KP(T);
    if constexpr (SCAN) {
        T = min(T, k_items[tile0].nframes - S.t0);
        if (T < 1) return;                        // nothing of this tile in the window (block-uniform, before every barrier)
    }

    // ---- frame ingest set-up: 16 lanes per stream, 16 streams per fold call (ms = tid >> 4) ----
    const float thr = P.thresh;
    const int q = tid & (QL - 1);
    const bool q0 = q == 0;
    const int lms = K8 ? (tid >> 3) & 15 : tid >> 4;      // the loader's stream of this thread
    const int lcol = tid >> 7;                            // K8: which of a fold call's two columns
    constexpr bool f32in = F32IN;
    constexpr int qsh = (f32in ? 4 : G711 ? 2 : 3) + (CH == 2 ? 1 : 0);   // a quad of samples: 16 / 8 / 4 bytes, of every channel
    const float sc = P.fmt == 1 ? 32767.0f : 32768.0f, rsc = 1.0f / sc;
    const __amdgpu_buffer_rsrc_t frs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void *>(KP(frames)), 0,
        SCAN ? (int)S.audio_bytes : (int)((unsigned)KP(n) * (unsigned)T * ((f32in ? 2048u : G711 ? 512u : 1024u) >> (K8 ? 1 : 0))), 0x00020000);
    // The frames are read once and are two thirds of what a one-frame launch fetches (8 192 streams: 16.8 MB beside 9 MB of state):
    // requested non-temporal, they stream past the L2 lines that hold the state and the weights
    // (16 kHz model; the 8 kHz sub-model's loader is what it was: at 8 192 streams it measured 1.2 us slower with this and the late
    //  request below, once - profiles/r09_launch_ends_other_configs.jsonl)
    constexpr int X_NT = K8 ? 0 : 2;               // the buffer loads' cache policy bits: nt
    // one quad of raw samples: 16 bytes (float32; int16 uses the first 8), G.711: the quad is one dword, fetched as such
    // CH == 2: a quad of sample frames L0 R0 L1 R1 L2 R2 L3 R3 - twice the bytes: two b128 | the int16 loader's b128, all of it | b64
    struct XQ2F { u32x4 a, b; };
    using XQ = std::conditional_t<CH == 2, std::conditional_t<f32in, XQ2F, std::conditional_t<G711, u32x2, u32x4>>,
                                  std::conditional_t<G711, uint32_t, u32x4>>;
    auto x_load = [&](int off) -> XQ {
        if constexpr (CH == 2 && f32in)
            return XQ2F{__builtin_amdgcn_raw_buffer_load_b128(frs, off, 0, X_NT), __builtin_amdgcn_raw_buffer_load_b128(frs, off + 16, 0, X_NT)};   // (both offsets range-checked)
        else if constexpr (CH == 2 && G711) return __builtin_amdgcn_raw_buffer_load_b64(frs, off, 0, X_NT);
        else if constexpr (G711) return __builtin_amdgcn_raw_buffer_load_b32(frs, off, 0, X_NT);
        else return __builtin_amdgcn_raw_buffer_load_b128(frs, off, 0, X_NT);
    };
    XQ xa_[4], xb_[4], xc_[4];                     // raw quads of the three columns
    // 16 kHz, frames from memory: column c + 1's quads k = 0, 1 ARE column c's k = 2, 3, in the same thread - they are requested and
    // decoded once, by column c, and X_FOLD hands them on decoded (RS reads its columns from LDS and keeps all four; 8 kHz: the
    // next column belongs to another thread)
    constexpr bool XCARRY = !RS && !K8;
#define X_K0(c) ((XCARRY && (c) > 0) ? 2 : 0)
    f32x4 *const F4 = ldsH + T_LDS_F4;              // RS: the tile's resampled frames
    // SCAN: frame tt of the launch, for the loader's stream, starts at quad xq0 + tt hopq of the audio block - frames overlap in
    // memory when hop < frame, nothing is copied.  Unsigned: a stream past its end keeps walking (into its neighbour's samples, or
    // past the block, where the descriptor answers 0); what it loads reaches selects only.
    // CH == 2: positions count sample frames, and the item's quad0 carries the stream's channel mode in its two top bits
    // (SCAN_MODE_SHIFT: 0 left, 1 right, 2 the mean of the two - a block is under 2 GiB, so a quad index stays below 2^29).
    uint32_t xq0 = 0;
    [[maybe_unused]] uint32_t xmode = 0;
    if constexpr (SCAN) {
        const int li = tile0 + lms;
        if constexpr (CH == 2) {
            const uint32_t qm = li < KP(n) ? k_items[li].quad0 : 0u;
            xmode = qm >> SCAN_MODE_SHIFT;
            xq0 = (qm & ((1u << SCAN_MODE_SHIFT) - 1u)) + (uint32_t)S.t0 * S.hopq;
        } else {
        xq0 = (li < KP(n) ? k_items[li].quad0 : 0u) + (uint32_t)S.t0 * S.hopq;
        }
    }
#define X_ISSUE(c, XR, tt)                                                                                      \
    if constexpr (RS) {                                                                                         \
        _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                           \
            XR[k] = __builtin_bit_cast(u32x4, F4[(tid >> 4) * FQ + 32 * (c) + q + 16 * k]);                     \
    } else if constexpr (SCAN) {                                                                                \
        const uint32_t fq = xq0 + (uint32_t)(tt) * S.hopq + 32 * (c) + q;                                       \
        _Pragma("unroll") for (int k = X_K0(c); k < 4; ++k)                                                     \
            XR[k] = x_load((int)((fq + 16 * k) << qsh));                                                        \
    } else {                                                                                                    \
        const int fq = ((tile0 + (tid >> 4)) * T + (tt)) * 128 + 32 * (c) + q;                                  \
        _Pragma("unroll") for (int k = X_K0(c); k < 4; ++k)                                                     \
            XR[k] = x_load((fq + 16 * k) << qsh);                                                               \
    }

    // 8 kHz: a frame is 64 quads, column c = quads 16 c .. 16 c + 31; lane q of a stream's 8 loads quads q, 8 + q, 16 + q, 24 + q
    // of column min(c0 + lcol, 2) (the second call's upper half repeats column 2: same values to the same places)
#define X_ISSUE8(c0, XR, tt)                                                                                    \
    {                                                                                                           \
        const int cc_ = (c0) + lcol < 2 ? (c0) + lcol : 2;                                                      \
        if constexpr (SCAN) {                                                                                   \
            const uint32_t fq = xq0 + (uint32_t)(tt) * S.hopq + 16 * cc_ + q;                                   \
            _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                       \
                XR[k] = x_load((int)((fq + 8 * k) << qsh));                                                     \
        } else {                                                                                                \
        const int fq = ((tile0 + lms) * T + (tt)) * 64 + 16 * cc_ + q;                                          \
        _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                           \
            XR[k] = x_load((fq + 8 * k) << qsh);                                                                \
        }                                                                                                       \
    }

    // ---- RS: the tile's parts.  A part = the columns c0 .. c1 - 1 of this tile that belong to one segment (one input rate); a tile
    //      at a rate boundary has two.
    struct Part {
        RateSeg S;
        int sk, c0, c1, ls0, Q, Kc, shape;
        bool valid;
    };
    constexpr int DEAD = 1 << 26;                  // an index (in quads / samples) past every buffer: loads return 0
    const int v0 = (int)blockIdx.x * MT16;
    auto mk_part = [&](int from) {
        Part pt{};
        pt.valid = false;
        if constexpr (RS) {
            for (int k = from; k < R.nseg; ++k) {                    // block-uniform: kernel arguments only
                const int a0 = max(R.seg[k].vstart, v0) - v0, a1 = min(R.seg[k].vstart + R.seg[k].n, v0 + MT16) - v0;
                if (a0 < a1) {
                    pt.S = R.seg[k];
                    pt.sk = k; pt.c0 = a0; pt.c1 = a1;
                    pt.ls0 = v0 - pt.S.vstart;                       // column c holds the segment's stream ls0 + c (c0 <= c < c1)
                    pt.Q = pt.S.n_in >> 2;
                    // the operator stream says how the part is contracted (pack_resample_operator_t16): 0 = every folded sample, two row
                    // tiles per wave; 1 / 2 = 48 / 24 kHz with every third sample copied ("P3"); 3 = 8 kHz with the even outputs copied
                    // and only the odd row tile contracted ("U2")
                    const int wbk = (int)pt.S.wave_blocks;
                    pt.shape = wbk == 4 + (pt.Q >> 4) * 8 ? 0 : wbk == 2 + (pt.Q >> 4) * 4 ? 3 : pt.S.n_in == 1536 ? 1 : 2;
                    pt.Kc = (pt.shape == 1 || pt.shape == 2) ? (2 * pt.Q) / 3 : pt.Q;      // contraction length per folded part
                    pt.valid = true;
                    break;
                }
            }
        }
        return pt;
    };
    // chunk loader: 16 streams x 16 folded quads = one per thread (stream ms = tid >> 4, quad ql = tid & 15)
    u32x4 xlA[6], xlB[6];
    const int cms = tid >> 4, cql = tid & 15;
    auto load_chunk = [&](auto p3tag, const Part &pt, int c, u32x4 *xl) {
        const __amdgpu_buffer_rsrc_t xrs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pt.S.in), 0, (int)((unsigned)pt.S.n * (unsigned)pt.S.n_in * 4u), 0x00020000);
        const int Q = pt.Q, qq = cql + 16 * c, base = (cms >= pt.c0 && cms < pt.c1) ? (pt.ls0 + cms) * Q : DEAD;
        if constexpr (decltype(p3tag)::value == 1 || decltype(p3tag)::value == 2) {
            // P3 (24 / 48 kHz, see the part loop): compact quad g = the folded samples j = 6g+1, 6g+2, 6g+4, 6g+5; the thread reads
            // six consecutive samples of each of the four regions - x[6g ..], x[H + 6g ..], x[H - 6g - 6 ..], x[n - 6g - 6 ..] -
            // which hold those four j and the two samples 3 i' in between (8-byte aligned; wide loads need dword alignment only)
            const int s6 = 6 * qq, sb = base * 4, H = 2 * Q, nn = 4 * Q;
            xl[0] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (sb + s6) * 4, 0, 0);
            xl[1] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (sb + H + s6) * 4, 0, 0);
            xl[2] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (sb + H - s6 - 4) * 4, 0, 0);
            xl[3] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (sb + nn - s6 - 4) * 4, 0, 0);
            const u32x2 a2 = __builtin_amdgcn_raw_buffer_load_b64(xrs, (sb + s6 + 4) * 4, 0, 0);
            const u32x2 c2 = __builtin_amdgcn_raw_buffer_load_b64(xrs, (sb + H + s6 + 4) * 4, 0, 0);
            const u32x2 b2 = __builtin_amdgcn_raw_buffer_load_b64(xrs, (sb + H - s6 - 6) * 4, 0, 0);
            const u32x2 d2 = __builtin_amdgcn_raw_buffer_load_b64(xrs, (sb + nn - s6 - 6) * 4, 0, 0);
            xl[4] = u32x4{a2.x, a2.y, c2.x, c2.y};
            xl[5] = u32x4{b2.x, b2.y, d2.x, d2.y};
        } else {
            xl[0] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (base + qq) * 16, 0, 0);
            xl[1] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (base + qq + (Q >> 1)) * 16, 0, 0);
            xl[2] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (base + (Q >> 1) - qq) * 16, 0, 0);
            xl[3] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (base + (Q >> 1) - qq - 1) * 16, 0, 0);
            xl[4] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (base + (qq == 0 ? 0 : Q - qq)) * 16, 0, 0);
            xl[5] = __builtin_amdgcn_raw_buffer_load_b128(xrs, (base + Q - qq - 1) * 16, 0, 0);
        }
    };
    Part cur = mk_part(0);
    // (requesting the first part's first chunk right here, IN FRONT of the state loads, was measured: 48.6 - 49.7 us against
    //  47.9 - 48.2 for 4 096 streams at 48 kHz on one box - it delays the state loads queued behind it.  Behind them: below.)

    // ---- prologue: h_{t-1} -> LDS planes (wave w cuts K-step w: the quads of units 32 w + 16 rt + 4 kq .., the cell's own layout),
    //      c_{t-1} -> registers, state machines -> LDS ----
    // Request order = the order in which the frame loop needs things (vmcnt retires in issue order): h, the wave's gate biases
    // (compact: 128 floats, kept in LDS for the call) and the tile's state machines (their 16 threads only), then - not RS, where
    // a whole resampling phase sits in front of the frame loop - the frame loop's first weight requests: the W_hh blocks of its
    // first units depend on kernel arguments only, and W_hh is the coldest part of the weight stream; then the window and c, and
    // behind the wait for h the frame's first two columns (below).  Streams past n (the last tile's tail) read slot 0's state and
    // compute on it: a stream is a column of every MFMA, nothing crosses columns, and every store of the kernel is guarded by `live`.
    // XFIRST: the frame's columns are requested first, then what the fold and the STFT need of the weight stream, and the state
    // behind them (H_STATE_H, H_STATE_SM below): h_{t-1} feeds only the recurrent half, whose result nothing needs before the input half adds
    // onto it behind barrier (6), while every phase in front of that depends on the frame.
    f32x4 hv[2];                                   // (tid & 15 == n: ONE slot lookup serves h, c and the state machine)
    decltype(__builtin_amdgcn_raw_buffer_load_b64(wrs, 0, 0, 0)) bias2;
#define H_STATE_H                                                                                               \
    {                                                                                                           \
        _Pragma("unroll") for (int rt = 0; rt < 2; ++rt)                                                        \
            hv[rt] = *reinterpret_cast<const f32x4 *>(KP(state) + (size_t)slot * 256 + 32 * w + 16 * rt + 4 * kq); \
        SB();                                                                                                   \
        bias2 = __builtin_amdgcn_raw_buffer_load_b64(wrs, lane * 8, (o_l + T_LSTM_BIAS_BLOCK) * 1024, 0);       \
    }
    if constexpr (!XFIRST) H_STATE_H
    const bool sm_thread = (tid < MT16) && live;
    const int sm_slot = slot;
    f32x4 smq[6];
#define H_STATE_SM                                                                                              \
    {                                                                                                           \
        if (tid < MT16) {                                                                                       \
            _Pragma("unroll") for (int k = 0; k < 6; ++k) smq[k] = reinterpret_cast<const f32x4 *>(KP(sm) + slot)[k]; \
        }                                                                                                       \
        SB();                                                                                                   \
    }
    if constexpr (XFIRST) { X_ISSUE(0, xa_, 0) SB(); }
    else H_STATE_SM
    // The LSTM's weights come from S_LSTM_X3 (vad_layout.h): per half 32 units u = 8 s + tile (K-step s, tile = 2 q + rt), each the
    // three bf16 pieces of the tile's A fragment (3 blocks).  They stream through a ring of X3_NR units, requested X3_D units ahead.
    // encoder.0 streams its own through the same ring (S_ENC0_X3, X3_CONV).
    f32x4 xw[X3_NR][3];
    // 16 kHz: the ring runs on from the recurrent half through the STFT's odd tile (vad_layout.h, DFT_X3_BLOCKS: four units, in the third
    // stream's buffer) into encoder.0, whose unit 0 sits in slot 0: the recurrent half's NH units start at XU_H with XU_H + NH + 4 = 0
    // (mod X3_NR), the DFT's unit v has slot XU_D + v
    // XFIRST: the ring starts at the DFT's units (requested by the prologue), and the recurrent half's follow enc3's (XU_R below)
    constexpr int NH = PAIR ? 16 : 32, XU_H = K8 ? 0 : (2 * X3_NR - (NH + 4) % X3_NR) % X3_NR, XU_D = XFIRST ? X3_NR - 4 : XU_H + NH;
    static_assert(K8 || (XU_D + 4) % X3_NR == 0, "encoder.0's units follow the DFT's in the ring");
    [[maybe_unused]] const int o_d = 4 * ENC1_X3_BLOCKS + 4 * ENC23_X3_BLOCKS + w * DFT_X3_BLOCKS;
#define X3_LDD(v, slot) X3_LDY(o_d + 3 * (v), slot)
#define X3_LDR(blk, slot) _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) xw[(slot) % X3_NR][p_] = WL((blk) + p_);
    // (U0: the ring slot of the half's unit 0 - 0 for the recurrent half, behind enc3's units for the input half)
#define X3_LD(B, u, U0) X3_LDR((B) + 3 * (u), (U0) + (u))
    // PAIR: unit v = 4 s + q of a wave's 16 = the stream's unit 8 s + 2 q + hf, ring slot U0 + v
#define X3_LDP(B, v, U0) X3_LDR((B) + 3 * (8 * ((v) >> 2) + 2 * ((v) & 3) + hf), (U0) + (v))
#define X3_LDU(B, u, U0) if constexpr (PAIR) { X3_LDP(B, u, U0) } else { X3_LD(B, u, U0) }
#define X3_LDX(blk, slot) _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) xw[(slot) % X3_NR][p_] = WX((blk) + p_);
#define X3_LDY(blk, slot) _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) xw[(slot) % X3_NR][p_] = WY((blk) + p_);
#define H_FIRSTX(tt)                                                                                            \
    {                                                                                                           \
        if constexpr (K8) { X_ISSUE8(0, xa_, tt) X_ISSUE8(2, xb_, tt) }                                         \
        else { X_ISSUE(0, xa_, tt) X_ISSUE(1, xb_, tt) }                                                        \
    }
#define H_FIRST(L, tt, WITHX)                                                                                   \
    {                                                                                                           \
        _Pragma("unroll") for (int u_ = 0; u_ < X3_D; ++u_) { X3_LDU((L) + LSTM_X3_HALF_BLOCKS, u_, XU_H) }         \
        if constexpr (WITHX) H_FIRSTX(tt)                                                                       \
        SB();                                                                                                   \
        if constexpr (RS) { X_ISSUE(2, xc_, tt) SB(); }                                                         \
    }
    if constexpr (!RS && !XFIRST) STAMP(29);
    if constexpr (!RS && !XFIRST) H_FIRST(o_x3, 0, K8)   // frames t > 0 request theirs at the end of frame t - 1; RS: at the top of the frame
    const f32x4 W1 = ldw(wrs, q * 16, o_nyq), W3 = ldw(wrs, (2 * QL + q) * 16, o_nyq);   // w[n], w[128 + n]  (8 kHz: w[64 + n])
    const float w64 = ldw(wrs, QL * 16, o_nyq).x;                                          // w[64]             (8 kHz: w[32])
    // XFIRST: behind column 0 and the window (the first fold waits for no more than those), the other two columns, the STFT's first
    // fp32 blocks, the DFT's four ring units - and only then the state
    [[maybe_unused]] f32x4 SwF[2];
    if constexpr (XFIRST) {
        X_ISSUE(1, xb_, 0) X_ISSUE(2, xc_, 0)
        SB();
#pragma unroll
        for (int k = 0; k < 2; ++k) SwF[k] = WL(o_stft + 8 + k);
#pragma unroll
        for (int v = 0; v < 4; ++v) { X3_LDD(v, XU_D + v) }
        SB();
        H_STATE_H
        H_STATE_SM
    }
    f32x4 cst[2];                                  // c of units 32 w + 16 rt + 4 kq + i
    if constexpr (PAIR) {                          // PAIR: of units 32 w + 16 hf + 4 kq + i, [0] the lane's own stream, [1] its stream in the partner tile
        cst[0] = *reinterpret_cast<const f32x4 *>(KP(state) + (size_t)slot * 256 + 128 + 32 * w + 16 * hf + 4 * kq);
        cst[1] = *reinterpret_cast<const f32x4 *>(KP(state) + (size_t)slot_o * 256 + 128 + 32 * w + 16 * hf + 4 * kq);
    } else {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) cst[rt] = *reinterpret_cast<const f32x4 *>(KP(state) + (size_t)slot * 256 + 128 + 32 * w + 16 * rt + 4 * kq);
    }
    // RS, first part at 48 kHz (the tiles that set a mixed tick's time): its first chunk is requested right BEHIND the state loads -
    // loads return in order, so the state is not delayed - and has its HBM round trip under the state's waits, the LDS writes and
    // the operator prefetch.  Same box: 43.3 -> 42.9 us (4 096 streams at 48 kHz), configs[3] 46.0 -> 45.5; for 8 / 24 kHz first
    // parts it changes nothing (+- 0.1), so they keep the request where the part begins.
    bool chunk0_requested = false;
    if constexpr (RS) {
        if (cur.valid && cur.S.wstream != nullptr && cur.S.n_in == 1536) {
            if (cur.shape == 0) load_chunk(std::integral_constant<int, 0>{}, cur, 0, xlA);
            else load_chunk(std::integral_constant<int, 1>{}, cur, 0, xlA);
            chunk0_requested = true;
        }
    }
    SB();
    if constexpr (XFIRST) STAMP(29);
    // (XFIRST: h, the biases and the state machines go to LDS behind barrier (4) - H_TO_LDS in the frame loop)
#define H_TO_LDS                                                                                                \
    {                                                                                                           \
        STAMP_ON(30, hv[1]);                           /* h has arrived */                                      \
        st_planes(RH + 12 * w * QSD + nq, hv[0], hv[1]);                                                        \
        reinterpret_cast<decltype(bias2) *>(biasL + 32 * w)[lane] = bias2;                                      \
        if (tid < MT16) {                                                                                       \
            _Pragma("unroll") for (int k = 0; k < 6; ++k) reinterpret_cast<f32x4 *>(smL + tid)[k] = smq[k];     \
        }                                                                                                       \
    }
    if constexpr (!XFIRST) {
    STAMP_ON(30, hv[1]);                           // h has arrived
    st_planes(RH + 12 * w * QSD + nq, hv[0], hv[1]);
    }
    // The call's first frame is requested HERE, behind the wait for h, and not with the first weight blocks: with two tiles per CU all
    // asking at once the memory system serves the launch's first requests roughly in order (8 192 streams: h arrives 7.5 k cycles
    // after kernel entry, 3.0 k at 4 096), and the frame's 32 KB per tile in front of h and c only delay what the first MFMAs wait
    // for; the first fold is 15 units of MFMAs away.  Same box: 36.81 -> 36.54 us per headline step.
    if constexpr (!RS && !K8 && !XFIRST) { SB(); H_FIRSTX(0) SB(); }
    if constexpr (!XFIRST) reinterpret_cast<decltype(bias2) *>(biasL + 32 * w)[lane] = bias2;
    int seg_last = 0;
    if (!XFIRST && tid < MT16) {
#pragma unroll
        for (int k = 0; k < 6; ++k) reinterpret_cast<f32x4 *>(smL + tid)[k] = smq[k];
    }
    const float hb = KP(wstream)[(size_t)P.sect[0][S_HEADB] * BLK_FLOATS];

    if constexpr (RS) {
        // ---- the tile's 16 chunks -> 512 samples at 16 kHz each, into F (resample.hip has the algebra; pack_resample_operator_t16
        //      the operator layout): four folded inputs ue / ve / uo / vo of length Q = n_in / 4 against four 128-row operators
        //      (se, ae, so, ao); wave w owns rows o = 32 w .. 32 w + 31 (two row tiles) of all four
        float *const Ff = reinterpret_cast<float *>(F4);
        while (cur.valid) {
        const RateSeg S = cur.S;
        const int c0 = cur.c0, c1 = cur.c1, ls0 = cur.ls0;
        auto in_part = [&](int c) { return c >= c0 && c < c1; };
        if (S.wstream == nullptr) {                                   // already 16 kHz (resample_audio returns its input): copy
            const __amdgpu_buffer_rsrc_t xrs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(S.in), 0, (int)((unsigned)S.n * 2048u), 0x00020000);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int idx = it * NTHREADS + tid, ms = idx >> 7, qd = idx & 127;
                if (in_part(ms))
                    F4[ms * FQ + qd] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, ((ls0 + ms) * 128 + qd) * 16, 0, 0));
            }
        } else {
          auto run_part = [&](auto p3tag) {
            // P3 (24 / 48 kHz: n_in = 3 n'): the samples x[3 i'] sit ON output instants - R[o][3 i'] = (512 / n_in) [o == m i'] +
            // (-1)^(o - m i') / n_in with m = 1536 / n_in (pack_resample_operator_t16 checks it and leaves those columns out of the
            // stream) - so the loader threads copy them, scaled, straight to their place in F and add them into one alternating sum
            // per stream, and the MFMAs contract only the other two thirds of the folded samples: 4 chunks instead of 6 (48 kHz),
            // 2 instead of 3 (24 kHz).  x[0], x[H], x[Q], x[3Q] - the samples the fold cannot pair - are all of that kind.
            // U2 (8 kHz: up by two): every input sample IS an even output sample (R[2 i][i'] = [i == i'], checked by the packer), and
            // the parity of an output is the parity of its folded row - so the loader threads copy the chunk into the even places of
            // F, the stream holds ONE 16-row tile per wave (the odd rows 32 w + 2 r + 1) and half the MFMAs and the VALU rows go.
            // Compile-time per part shape (tag 0: every sample contracted, 1: 48 kHz, 2: 24 kHz, 3: 8 kHz - four instantiations of
            // this body): branches inside the chunk loop cost ~0.4 us per chunk.
            constexpr int SHAPE = decltype(p3tag)::value;
            constexpr bool P3 = SHAPE == 1 || SHAPE == 2, U2 = SHAPE == 3;
            constexpr int NB = U2 ? 4 : 8;                            // operator blocks per k-iteration
            constexpr int om = SHAPE;                                 // P3: output steps between two copied samples = 1536 / n_in
            const int Q = S.n_in >> 2, Kc = cur.Kc, nchunks = Kc >> 6;
            const float sc0 = 512.0f / (float)S.n_in;
            constexpr float sg3 = om == 1 ? -1.f : 1.f;
            float pA = 0.f;                                           // this thread's share of sum_i' (-1)^(m i') x[3 i']
            const __amdgpu_buffer_rsrc_t ors =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(S.wstream), 0, (int)S.wstream_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t xrs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(S.in), 0, (int)((unsigned)S.n * (unsigned)S.n_in * 4u), 0x00020000);
#define OL(blk) ldw(ors, lane16, (blk))
            const int wbase = w * (int)S.wave_blocks;
            if (!chunk0_requested) load_chunk(p3tag, cur, 0, xlA);
            chunk0_requested = false;
            // (input chunks are requested TWO chunks ahead - two register sets - so that a chunk's HBM round trip has a whole
            // chunk of MFMAs, ~1.7 us, more to hide under than it needs; chunk 0 has been on its way since before this part began)
            auto store_chunk = [&](int c, int buf, const u32x4 *xl) {
                if constexpr (P3) {
                    const f32x4 A4 = __builtin_bit_cast(f32x4, xl[0]), C4 = __builtin_bit_cast(f32x4, xl[1]);
                    const f32x4 B4 = __builtin_bit_cast(f32x4, xl[2]), D4 = __builtin_bit_cast(f32x4, xl[3]);
                    const f32x4 AC = __builtin_bit_cast(f32x4, xl[4]), BD = __builtin_bit_cast(f32x4, xl[5]);
                    // j = 6g+1, 6g+2, 6g+4, 6g+5: x[j], x[j+H] ascending; x[H-j], x[n-j] descending through their windows
                    const f32x4 a = f32x4{A4.y, A4.z, AC.x, AC.y}, cc = f32x4{C4.y, C4.z, AC.z, AC.w};
                    const f32x4 b = f32x4{B4.w, B4.z, B4.x, BD.y}, d = f32x4{D4.w, D4.z, D4.x, BD.w};
                    const f32x4 pe = a + cc, me = a - cc, qe = b + d, qo = b - d;
                    f32x4 *dst = lds + buf * RS_BUF + cql * QSL + cms;
                    dst[0] = pe + qe;
                    dst[RS_CH_ROWS * QSL] = pe - qe;
                    dst[2 * RS_CH_ROWS * QSL] = me + qo;
                    dst[3 * RS_CH_ROWS * QSL] = me - qo;
                    // the copied samples: x[6g], x[6g+3] (and the same past H) -> outputs ob, ob + m; x[H-6g-3], x[H-6g-6] -> 256 - ob - m,
                    // 256 - ob - 2m (likewise below 512): every output instant m i' exactly once over the part's chunks
                    const float e0 = A4.x + C4.x + BD.x + BD.z, e3 = A4.w + C4.w + B4.y + D4.y;
                    pA += e0 + sg3 * e3;
                    if (cms >= c0 && cms < c1) {
                        float *o = Ff + cms * (4 * FQ);
                        const int ob = om * 2 * (cql + 16 * c);
                        typedef float f32x2 __attribute__((ext_vector_type(2)));
                        if constexpr (om == 1) {          // 48 kHz: neighbours - four aligned pairs
                            *reinterpret_cast<f32x2 *>(o + ob) = f32x2{sc0 * A4.x, sc0 * A4.w};
                            *reinterpret_cast<f32x2 *>(o + 256 + ob) = f32x2{sc0 * C4.x, sc0 * C4.w};
                            *reinterpret_cast<f32x2 *>(o + 254 - ob) = f32x2{sc0 * BD.x, sc0 * B4.y};
                            *reinterpret_cast<f32x2 *>(o + 510 - ob) = f32x2{sc0 * BD.z, sc0 * D4.y};
                        } else {                          // 24 kHz: every other output; the odd ones get nothing but the alternation
                            *reinterpret_cast<f32x4 *>(o + ob) = f32x4{sc0 * A4.x, 0.f, sc0 * A4.w, 0.f};
                            *reinterpret_cast<f32x4 *>(o + 256 + ob) = f32x4{sc0 * C4.x, 0.f, sc0 * C4.w, 0.f};
                            *reinterpret_cast<f32x4 *>(o + 252 - ob) = f32x4{sc0 * BD.x, 0.f, sc0 * B4.y, 0.f};
                            *reinterpret_cast<f32x4 *>(o + 508 - ob) = f32x4{sc0 * BD.z, 0.f, sc0 * D4.y, 0.f};
                        }
                    }
                } else {
                    const f32x4 a = __builtin_bit_cast(f32x4, xl[0]), cc = __builtin_bit_cast(f32x4, xl[1]);
                    const f32x4 b0 = __builtin_bit_cast(f32x4, xl[2]), b1 = __builtin_bit_cast(f32x4, xl[3]);
                    const f32x4 d0 = __builtin_bit_cast(f32x4, xl[4]), d1 = __builtin_bit_cast(f32x4, xl[5]);
                    const f32x4 b = f32x4{b0.x, b1.w, b1.z, b1.y}, d = f32x4{d0.x, d1.w, d1.z, d1.y};
                    const f32x4 pe = a + cc, me = a - cc, qe = b + d, qo = b - d;
                    f32x4 ue = pe + qe, ve = pe - qe, uo = me + qo, vo = me - qo;
                    if (cql + 16 * c == 0) { ue.x = pe.x; ve.x = 0.f; uo.x = 0.f; vo.x = me.x; }     // j = 0 has no partner
                    f32x4 *dst = lds + buf * RS_BUF + cql * QSL + cms;
                    dst[0] = ue;
                    dst[RS_CH_ROWS * QSL] = ve;
                    dst[2 * RS_CH_ROWS * QSL] = uo;
                    dst[3 * RS_CH_ROWS * QSL] = vo;
                    if constexpr (U2) {
                        // y[2 i] = x[i]: the four aligned quads this thread holds - x[4 qq ..], x[H + 4 qq ..], x[H - 4 qq - 4 ..],
                        // x[n - 4 qq - 4 ..] - cover every sample of the chunk exactly once over the 16 loader threads of a stream;
                        // the odd places get zeros here and their values from the recombination, behind the barrier
                        if (cms >= c0 && cms < c1) {
                            float *o = Ff + cms * (4 * FQ);
                            const int qq = cql + 16 * c;
                            auto put = [&](int first, f32x4 v) {
                                *reinterpret_cast<f32x4 *>(o + 2 * first) = f32x4{v.x, 0.f, v.y, 0.f};
                                *reinterpret_cast<f32x4 *>(o + 2 * first + 4) = f32x4{v.z, 0.f, v.w, 0.f};
                            };
                            put(4 * qq, a);
                            put(2 * Q + 4 * qq, cc);
                            put(2 * Q - 4 * qq - 4, b1);
                            put(4 * Q - 4 * qq - 4, d1);
                        }
                    }
                }
            };
            // the sample each half-size product cannot pair, x[Q] +- x[Q + H], is a rank-1 term (accumulator init, rows 128 / 384)
            const int sb = in_part(n) ? (ls0 + n) * S.n_in : (DEAD << 2);         // columns of other segments contract zeros
            float xa = 0.f, xb = 0.f;
            f32x4 mid = f32x4{0.f, 0.f, 0.f, 0.f}, ini[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) ini[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (!P3) {                                                  // (P3: x[Q] and x[3Q] are copied samples)
                xa = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (sb + Q) * 4, 0, 0));
                xb = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (sb + 3 * Q) * 4, 0, 0));
                if constexpr (U2) {                                               // (rows 128 / 384 are even: copies)
                    ini[0] = OL(wbase);
                    ini[1] = OL(wbase + 1);
                } else {
                    mid = ldw(ors, (Q >> 1) * 16, (int)S.row128_block);           // floats 2Q, 2Q + 1: RE[128][Q] / 2, RO[128][Q] / 2
#pragma unroll
                    for (int k = 0; k < 4; ++k) ini[k] = OL(wbase + k);
                }
            }
            // output rows 128 / 384 on the VALU: thread = (stream tid & 15, part tid >> 4); parts 0..7 dot ue with GSE[128],
            // 8..15 uo with GSO[128], two quads of every chunk each
            float r128 = 0.f;
            const int rpart = tid >> 4, pr = rpart & 7, psel = rpart >> 3;
#ifndef RS_D
#define RS_D 4
#endif
            constexpr int D = RS_D;                                   // operator blocks run D - 1 k-iterations ahead, across chunks (4 or 8: the slot of
                                                                      // a k-iteration must be static inside the two-chunk loop body)
            f32x4 wq[D][NB], xqA[4], xqB[4];
            int ws = wbase + (U2 ? 2 : 4);
#define R_LDW0(slot, j) _Pragma("unroll") for (int k = 0; k < NB; ++k) wq[slot][k] = OL(ws + NB * (j) + k);
            // (tools/variants.sh experiments, never defined in the product build: RS_EXP_NOLDW = the operator is not streamed,
            //  RS_EXP_NOMFMA = 4 VALU FMAs stand in for each group of 4 MFMAs, RS_EXP_NOX = the input chunks are loaded once)
#ifdef RS_EXP_NOLDW
#define R_LDW(slot, j)
#else
#define R_LDW(slot, j) R_LDW0(slot, j)
#endif
#ifdef RS_EXP_NOMFMA
#define RS_MMA(W, X, A) ((A) + (W) * (X))
#else
#define RS_MMA(W, X, A) mfma16((W), (X), (A))
#endif
#ifdef RS_EXP_NOLDW
#pragma unroll
            for (int d = 0; d < D; ++d) { R_LDW0(d, d % (D - 1)) }
#endif
#pragma unroll
            for (int d = 0; d < D - 1; ++d) { R_LDW0(d, d) }
            if (nchunks > 1) load_chunk(p3tag, cur, 1, xlB);
            f32x4 acc[NB];                                            // part p (se, ae, so, ao), row tile rt -> acc[2 p + rt]; U2: acc[p]
            if constexpr (U2) {
                acc[0] = ini[0] * (xa + xb);
                acc[2] = ini[1] * (xa - xb);
                acc[1] = acc[3] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    acc[0 + rt] = ini[rt] * (xa + xb);
                    acc[4 + rt] = ini[2 + rt] * (xa - xb);
                    acc[2 + rt] = acc[6 + rt] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            store_chunk(0, 0, xlA);
            __syncthreads();
            // Chunk c: the MFMAs read staging buffer c & 1.  Software pipeline inside a chunk: the activation quads of k-iteration
            // j + 1 are read from LDS BEFORE the MFMAs of j are issued (two register sets), chunk c + 1 (requested two chunks ago,
            // in `XS`) is folded into the other staging buffer while the MFMAs of j = 1 run, the VALU rows under j = 2, chunk c + 2
            // is requested into `XL` at the start - so that the chunk's only exposed LDS round trip is the first read behind
            // the barrier at its end.  (Before: four exposed reads + fold + barrier per chunk = 1.3 us on top of 1.7 us of MFMAs.)
#ifdef RS_EXP_NOX
#define RS_LOADX(c, XL)
#else
#define RS_LOADX(c, XL) load_chunk(p3tag, cur, (c), XL)
#endif
#define RS_XQ(XQ, X, j) _Pragma("unroll") for (int p4 = 0; p4 < 4; ++p4) XQ[p4] = (X)[(p4 * RS_CH_ROWS + 4 * (j)) * QSL + nqL];
#define RS_STEP(j, XC, XN, EXTRA)                                                                               \
                {                                                                                               \
                    R_LDW((4 * PAR_ + (j) + D - 1) % D, (j) + D - 1)   /* past j = 3: the next chunks' blocks (the stream is contiguous) */ \
                    if ((j) < 3) { RS_XQ(XN, X, (j) + 1) }                                                      \
                    EXTRA                                                                                       \
                    SB();                                                                                       \
                    _Pragma("unroll") for (int k = 0; k < NB; ++k) acc[k] = RS_MMA(wq[(4 * PAR_ + (j)) % D][k], XC[U2 ? k : k >> 1], acc[k]); \
                    SB();                                                                                       \
                }
#define RS_CHUNK(c, XS, XL, PAR)                                                                                \
            {                                                                                                   \
                constexpr int PAR_ = PAR;                                                                       \
                const f32x4 *X = lds + ((c) & 1) * RS_BUF;                                                      \
                asm volatile("" : "+s"(ws));                                                                    \
                f32x4 g128[2];                                                                                  \
                RS_STEP(0, xqA, xqB,                                                                            \
                        if ((c) + 2 < nchunks) RS_LOADX((c) + 2, XL);                                           \
                        if constexpr (!U2) {                                                                    \
                            _Pragma("unroll") for (int i = 0; i < 2; ++i)                                       \
                                g128[i] = ldw(ors, (psel * (Kc >> 2) + 16 * (c) + 2 * pr + i) * 16, (int)S.row128_block); \
                        })                                                                                      \
                RS_STEP(1, xqB, xqA, if ((c) + 1 < nchunks) store_chunk((c) + 1, ((c) + 1) & 1, XS);)           \
                RS_STEP(2, xqA, xqB, if constexpr (!U2) {                                                       \
                    const int ms = tid & 15;                                                                    \
                    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                             \
                        const f32x4 uu = X[(psel * 2 * RS_CH_ROWS + 2 * pr + i) * QSL + ms];                    \
                        r128 += g128[i].x * uu.x + g128[i].y * uu.y + g128[i].z * uu.z + g128[i].w * uu.w;      \
                    }                                                                                           \
                })                                                                                              \
                RS_STEP(3, xqB, xqA, )                                                                          \
                ws += 4 * NB;                                                                                   \
                __syncthreads();                                                                                \
                if ((c) + 1 < nchunks) { RS_XQ(xqA, lds + (((c) + 1) & 1) * RS_BUF, 0) }                        \
            }
            RS_XQ(xqA, lds, 0)
            for (int c = 0; c < nchunks; c += 2) {
                RS_CHUNK(c, xlB, xlA, 0)
                if (c + 1 < nchunks) RS_CHUNK(c + 1, xlA, xlB, 1)
            }
#undef RS_CHUNK
#undef RS_STEP
#undef RS_XQ
#undef RS_LOADX
#undef RS_MMA
#undef R_LDW
#undef R_LDW0
            if constexpr (U2) {
                // the odd outputs: lane (n, kq) holds rows o = 32 w + 8 kq + 2 i + 1 of se, ae, so, ao.  The barrier that ended the
                // chunk is also the one that separates these scalars from the loader's zeros in the same places.
                const f32x4 se = acc[0], ae = acc[1], so = acc[2], ao = acc[3];
                const f32x4 pe = se + ae, me = se - ae, pO = so + ao, mO = so - ao;
                const f32x4 y0 = pe + pO, y1 = pe - pO, lo = me + mO, hi = me - mO;
                if (in_part(n)) {
                    float *o = Ff + n * (4 * FQ);
                    const int o0 = 32 * w + 8 * kq + 1;
                    o[o0] = y0.x;     o[o0 + 256] = y1.x; o[256 - o0] = lo.x; o[512 - o0] = hi.x;
                    o[o0 + 2] = y0.y; o[o0 + 258] = y1.y; o[254 - o0] = lo.y; o[510 - o0] = hi.y;
                    o[o0 + 4] = y0.z; o[o0 + 260] = y1.z; o[252 - o0] = lo.z; o[508 - o0] = hi.z;
                    o[o0 + 6] = y0.w; o[o0 + 262] = y1.w; o[250 - o0] = lo.w; o[506 - o0] = hi.w;
                }
            } else if constexpr (!P3) {
                // recombine: y[o] = se+ae+so+ao, y[o+256] = se+ae-so-ao, y[256-o] = se-ae+so-ao, y[512-o] = se-ae-so+ao
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const int row = 32 * w + 16 * rt + 4 * kq;
                    const f32x4 se = acc[0 + rt], ae = acc[2 + rt], so = acc[4 + rt], ao = acc[6 + rt];
                    const f32x4 pe = se + ae, me = se - ae, pO = so + ao, mO = so - ao;
                    if (in_part(n)) {
                        F4[n * FQ + (row >> 2)] = pe + pO;
                        F4[n * FQ + 64 + (row >> 2)] = pe - pO;
                        const f32x4 lo = me + mO, hi = me - mO;
                        float *o = Ff + n * (4 * FQ);
                        if (row != 0) { o[256 - row] = lo.x; o[512 - row] = hi.x; }     // o = 0: y[256] and y[0] are written above
                        o[255 - row] = lo.y; o[511 - row] = hi.y;
                        o[254 - row] = lo.z; o[510 - row] = hi.z;
                        o[253 - row] = lo.w; o[509 - row] = hi.w;
                    }
                }
                headp[rpart * 16 + (tid & 15)] = r128;               // [16 parts][16 streams]: headp .. fcor are idle before the frame loop
                __syncthreads();
                if (tid < MT16 && in_part(tid)) {                     // tid < 16: this thread's MFMA column n is stream tid - xa / xb are its x[Q], x[3Q]
                    float e = 0.f, od = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) { e += headp[k * 16 + tid]; od += headp[(8 + k) * 16 + tid]; }
                    e += mid.x * (xa + xb);
                    od += mid.y * (xa - xb);
                    Ff[tid * (4 * FQ) + 128] = e + od;
                    Ff[tid * (4 * FQ) + 384] = e - od;
                }
            } else {
                // rows 128 / 384 and the alternating sum meet in LDS first: the recombination needs the sum
                headp[rpart * 16 + (tid & 15)] = r128;
                float *const altL = fcor + FCOR_SINK;                 // [16 streams]
                float a = pA;
                a += __shfl_xor(a, 1, 16);
                a += __shfl_xor(a, 2, 16);
                a += __shfl_xor(a, 4, 16);
                a += __shfl_xor(a, 8, 16);
                if (cql == 0) altL[cms] = a * (1.0f / (float)S.n_in);
                __syncthreads();
                // the same recombination, on top of the copied samples already in F, plus (-1)^o times the stream's sum / n_in
                const float altv = altL[n];
                const f32x4 altq = f32x4{altv, -altv, altv, -altv};
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const int row = 32 * w + 16 * rt + 4 * kq;
                    const f32x4 se = acc[0 + rt], ae = acc[2 + rt], so = acc[4 + rt], ao = acc[6 + rt];
                    const f32x4 pe = se + ae, me = se - ae, pO = so + ao, mO = so - ao;
                    if (in_part(n)) {
                        float *o = Ff + n * (4 * FQ);
                        F4[n * FQ + (row >> 2)] += pe + pO + altq;
                        F4[n * FQ + 64 + (row >> 2)] += pe - pO + altq;
                        const f32x4 lo = me + mO + altq, hi = me - mO + altq;       // 256 - row - k and 512 - row - k have the parity of k
                        if (row != 0) { o[256 - row] += lo.x; o[512 - row] += hi.x; }
                        o[255 - row] += lo.y; o[511 - row] += hi.y;
                        o[254 - row] += lo.z; o[510 - row] += hi.z;
                        o[253 - row] += lo.w; o[509 - row] += hi.w;
                    }
                }
                if (tid < MT16 && in_part(tid)) {                     // rows 128 / 384 (even): on top of the copied x[Q], x[3Q]
                    float e = altv, od = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) { e += headp[k * 16 + tid]; od += headp[(8 + k) * 16 + tid]; }
                    Ff[tid * (4 * FQ) + 128] += e + od;
                    Ff[tid * (4 * FQ) + 384] += e - od;
                }
            }
          };
          if (cur.shape == 0) run_part(std::integral_constant<int, 0>{});
          else if (cur.shape == 1) run_part(std::integral_constant<int, 1>{});
          else if (cur.shape == 2) run_part(std::integral_constant<int, 2>{});
          else run_part(std::integral_constant<int, 3>{});
#undef OL
        }
        __syncthreads();                                              // this part of F is complete; staging and headp are free again
        cur = mk_part(cur.sk + 1);
        }                                                             // next part
    }

    STAMP(0);
    for (int t = 0;;) {                          // T >= 1; the back edge is at the bottom, behind the next frame's first requests
        int ws_stft = o_stft, ws_x0 = o_x0, ws_y1 = o_y1, ws_z = o_z, ws_l = o_l, ws_x3 = o_x3;
        asm volatile("" : "+s"(ws_stft), "+s"(ws_x0), "+s"(ws_y1), "+s"(ws_z), "+s"(ws_l), "+s"(ws_x3));
        // ---- recurrent gate half W_hh . h_{t-1} (4 K-steps x {4 gates x 2 row tiles}, bf16 split) with the frame ingested under it ----
        [[maybe_unused]] f32x4 G[8];              // gate q, row tile rt -> G[2 q + rt] (not PAIR)
        [[maybe_unused]] f32x4 Gp[4][2];          // PAIR: gate q's row tile hf of the wave's own tile [0] and of the partner half's [1]
        {
            [[maybe_unused]] const int wh = ws_x3 + LSTM_X3_HALF_BLOCKS;
            f32x4 xcA, xcB;                       // XCARRY: the decoded quads k = 2, 3 of the column folded last
            float xm = 0.f;                       // float32: running max |x| of this thread's raw samples (vadk_device.h absmax4)
            auto decode = [&](XQ b) -> f32x4 {
                f32x4 v;
                if constexpr (CH == 2) {
                    // both channels through the mono decoders, then the stream's own: left | right | (dL + dR) * 0.5f, which is
                    // np.mean(x, axis=1) of a float32 [N, 2] array bit for bit (an add, then a multiply: nothing to contract).
                    // The rejection and the gate see what the model sees: the selected channel or the mixed values.
                    f32x4 dl, dr;
                    if constexpr (G711) {
                        dl = g711_quad<FMT == 3>(__builtin_amdgcn_perm(b.y, b.x, 0x06040200u));    // codes L0 L1 L2 L3
                        dr = g711_quad<FMT == 3>(__builtin_amdgcn_perm(b.y, b.x, 0x07050301u));
                    } else if constexpr (!f32in) {
                        dl = f32x4{i16_div((int)(short)(b.x & 0xffffu), sc, rsc), i16_div((int)(short)(b.y & 0xffffu), sc, rsc),
                                   i16_div((int)(short)(b.z & 0xffffu), sc, rsc), i16_div((int)(short)(b.w & 0xffffu), sc, rsc)};
                        dr = f32x4{i16_div((int)(short)(b.x >> 16), sc, rsc), i16_div((int)(short)(b.y >> 16), sc, rsc),
                                   i16_div((int)(short)(b.z >> 16), sc, rsc), i16_div((int)(short)(b.w >> 16), sc, rsc)};
                    } else {
                        dl = __builtin_bit_cast(f32x4, u32x4{b.a.x, b.a.z, b.b.x, b.b.z});
                        dr = __builtin_bit_cast(f32x4, u32x4{b.a.y, b.a.w, b.b.y, b.b.w});
                    }
                    const bool right = xmode == 1u, mix = xmode >= 2u;
                    const f32x4 mx = pk::mul(pk::add(dl, dr), f32x4{0.5f, 0.5f, 0.5f, 0.5f});
                    v.x = mix ? mx.x : right ? dr.x : dl.x;
                    v.y = mix ? mx.y : right ? dr.y : dl.y;
                    v.z = mix ? mx.z : right ? dr.z : dl.z;
                    v.w = mix ? mx.w : right ? dr.w : dl.w;
                    if constexpr (f32in) xm = absmax4(xm, v);
                } else if constexpr (G711) {
                    v = g711_quad<FMT == 3>(b);
                } else if constexpr (!f32in) {
                    const int s0 = (int)(short)(b.x & 0xffffu), s1 = (int)(short)(b.x >> 16);
                    const int s2 = (int)(short)(b.y & 0xffffu), s3 = (int)(short)(b.y >> 16);
                    v = f32x4{i16_div(s0, sc, rsc), i16_div(s1, sc, rsc), i16_div(s2, sc, rsc), i16_div(s3, sc, rsc)};
                } else {
                    v = __builtin_bit_cast(f32x4, b);
                    xm = absmax4(xm, v);          // before the gate: gate on and off reject the same frames
                }
                return gate4(v, thr);
            };
            // after the frame's last fold call: the stream's QL loader lanes of this row vote (a ballot, no branch), every one of
            // them writes the verdict; barrier (1) publishes it to the cell and the head
#define X_FLAG                                                                                                  \
    if constexpr (f32in) {                                                                                      \
        const unsigned long long b_ = __builtin_amdgcn_ballot_w64(nonfinite(xm));                               \
        flagL[(K8 ? 16 * lcol : 0) + lms] = (uint8_t)(((b_ >> (lane & (64 - QL))) & ((1ull << QL) - 1)) != 0);   \
    }
            // (8 kHz: 8 lanes per stream - row_half_mirror, and lane 8 of a row, which row_shr:1 would feed from the neighbouring
            // stream's lane 7, takes `edge` by a select)
            auto mirror = [](float v) -> float {
                return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), K8 ? 0x141 : 0x140, 0xf, 0xf, true));
            };
            auto shr1 = [&](float edge, float v) -> float {
                const float r = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, false));
                return (K8 && q0) ? edge : r;
            };
            auto shl8 = [](float v) -> float {        // row_shl:8: lane q gets lane q + 8 (lanes 8..15: zero)
                return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x108, 0xf, 0xf, true));
            };
            // row_ror:8 with bank mask 0xc: lanes 8..15 of a row get lane q - 8's `hi`, lanes 0..7 keep their own `lo`
            [[maybe_unused]] auto ror8hi = [](float lo, float hi) -> float {
                return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, lo), __builtin_bit_cast(int, hi), 0x128, 0xf, 0xc, false));
            };
            // 16 kHz: where the lane's halves of po's fragments go inside a column's plane groups (K-step q >> 3, kq = q & 3, the
            // stream swizzled: silero_v5_t16.hip, T_ROWS_DFT)
            [[maybe_unused]] const int fold_og = (12 * (q >> 3) + (q & 3)) * QSD + (lms ^ ((q & 3) | ((q >> 3) << 2)));
            // the fold of silero_v5.hip, one call per column: stream ms = tid >> 4, n = 4 q + j
#define X_FOLD(c, XR, NEXT)                                                                                     \
    {                                                                                                           \
        _Pragma("clang fp contract(off)")                                                                       \
        const int ms = lms;                                                                                     \
        STAMP_ON(20 + (NEXT), XR[3]);                                                                           \
        f32x4 xA, xB;                                                                                           \
        if constexpr (XCARRY && (NEXT)) { xA = xcA; xB = xcB; }                                                 \
        else { xA = decode(XR[0]); xB = decode(XR[1]); }                                                        \
        const f32x4 xC = decode(XR[2]), xD = decode(XR[3]);                                                     \
        if constexpr (XCARRY) { xcA = xC; xcB = xD; }                                                           \
        const float mBx = mirror(xB.x), mDx = mirror(xD.x);                                                     \
        const f32x4 y1 = pk::mul(xA, W1), y3 = pk::mul(xC, W3);                                                 \
        const f32x4 y2 = pk::mul(f32x4{shr1(xC.x, mBx), mirror(xB.w), mirror(xB.z), mirror(xB.y)}, W3);         \
        const f32x4 y4 = pk::mul(f32x4{shr1(0.f, mDx), mirror(xD.w), mirror(xD.z), mirror(xD.y)}, W1);          \
        const f32x4 s14 = pk::add(y1, y4), d14 = pk::sub(y1, y4), s23 = pk::add(y2, y3), d23 = pk::sub(y2, y3); \
        f32x4 pe = pk::add(s14, s23), po = pk::sub(s14, s23), qe = pk::sub(d14, d23), qo = pk::add(d14, d23);   \
        {                                                                                                       \
            pe.x = q0 ? 0.f : pe.x; po.x = q0 ? 0.f : po.x; qe.x = q0 ? 0.f : qe.x; qo.x = q0 ? 0.f : qo.x;        \
            const float y64 = xB.x * w64, y192 = xD.x * w64;                                                    \
            const int fo = q0 ? (c) * 48 + ms : FCOR_SINK + lane;                                               \
            fcor[fo] = y3.x;                                                                                    \
            fcor[fo + (q0 ? 16 : 0)] = y64 + y192;                                                              \
            fcor[fo + (q0 ? 32 : 0)] = y64 - y192;                                                              \
        }                                                                                                       \
        if constexpr (K8) {                                                                                     \
            st2(&RX[(CS * (c) + q) * QSL + ms], pe);                                                            \
            st2(&RX[(CS * (c) + QL + q) * QSL + ms], po);                                                       \
            st2(&RX[(CS * (c) + 2 * QL + q) * QSL + ms], qe);                                                   \
            st2(&RX[(CS * (c) + 3 * QL + q) * QSL + ms], qo);                                                   \
        } else {                                                                                                \
        /* the odd bins contract po | qo on the bf16 split: the lane cuts its two quads - half (q >> 2) & 1 of lane (ms, kq = q & 3)'s \
           fragments of K-step q >> 3 - into the column's plane groups (silero_v5_t16.hip, T_ROWS_DFT).  The even bins' operands fold   \
           once more, about n = 32 (vad_layout.h, bin_of_channel_fold3; silero_v5.hip has the lane algebra): lanes q < 8 hold n =      \
           0..31, lanes q >= 8 the same values again - so lane q < 8 stores pe+ and pe-, lane q + 8 fetches that lane's qe- and qe+     \
           (row_ror:8 into lanes 8..15 only, the other lanes keep pe+-: the select rides in the DPP's bank mask) and stores those,       \
           rows q and 16 + q of the column for every lane: no sink rows, no branch, half the stores.  Slot n = 0 carries the unpaired \
           n = 32 (lane 8, component 0): pe[32] | qe[32] */                                                    \
        const f32x4 pm = f32x4{shr1(0.f, mirror(pe.x)), mirror(pe.w), mirror(pe.z), mirror(pe.y)};               \
        const f32x4 qm = f32x4{shr1(0.f, mirror(qe.x)), mirror(qe.w), mirror(qe.z), mirror(qe.y)};               \
        f32x4 pep = pk::add(pe, pm), pen = pk::sub(pe, pm), qen = pk::sub(qe, qm), qep = pk::add(qe, qm);       \
        const float pe32 = shl8(pe.x), qe32 = shl8(qe.x);                                                       \
        pep.x = q0 ? pe32 : pep.x; pen.x = q0 ? 0.f : pen.x; qen.x = q0 ? 0.f : qen.x; qep.x = q0 ? qe32 : qep.x;   \
        f32x4 *const og = RX + (PP * (c)) * QSD + fold_og;                                                      \
        st_planes_half(og, (q >> 2) & 1, po);                                                                   \
        st_planes_half(og + 24 * QSD, (q >> 2) & 1, qo);                                                        \
        const f32x4 eA = f32x4{ror8hi(pep.x, qen.x), ror8hi(pep.y, qen.y), ror8hi(pep.z, qen.z), ror8hi(pep.w, qen.w)};   \
        const f32x4 eB = f32x4{ror8hi(pen.x, qep.x), ror8hi(pen.y, qep.y), ror8hi(pen.z, qep.z), ror8hi(pen.w, qep.w)};   \
        st2(&REV[(32 * (c) + q) * QSL + ms], eA);                                                               \
        st2(&REV[(32 * (c) + 16 + q) * QSL + ms], eB);                                                          \
        }                                                                                                       \
    }
#define H_MIX                                                                                                   \
    _Pragma("unroll") for (int i_ = 0; i_ < 6; ++i_) {                                                          \
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                      \
        __builtin_amdgcn_sched_group_barrier(0x002, 28, 0);                                                     \
    }
            if constexpr (XFIRST) {
                // the three folds as their columns arrive, on an MFMA pipe that has nothing else to do yet: h is still on its way
                X_FOLD(0, xa_, 0) X_FOLD(1, xb_, 1) X_FOLD(2, xc_, 2) X_FLAG
            } else {
            if constexpr (RS) H_FIRST(ws_x3, t, true)           // F is dead once every wave has passed the barrier below
            {   // the accumulators start at the gate biases: G[2 q + rt] register i of a lane = unit 16 rt + 4 kq + i of gate q (the
                // 16 lanes of a row group read the same 16 bytes: a broadcast).  The wave reads what the wave itself wrote.
                const f32x4 *const bq = biasL + 32 * w + kq;
                if constexpr (PAIR) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) Gp[k][0] = Gp[k][1] = bq[k * 8 + hf * 4];
                } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) G[k] = bq[(k >> 1) * 8 + (k & 1) * 4];
                }
            }
            __syncthreads();   // (0) h_{t-1} visible (t > 0: follows barrier (8))
            STAMP(31);
            // 4 K-steps x 8 tiles on the bf16 split (X3_HALF); the frame's columns are folded in the shadow of the last three units
            // of K-steps 1, 2, 3 (8 kHz: two fold calls, columns (0 | 1) by half of the workgroup, then column 2, in K-steps 1, 2)
#define H_EXTRA(u)                                                                                              \
            if constexpr (!K8 && (u) + X3_D >= 32) { X3_LDD((u) + X3_D - 32, XU_H + (u) + X3_D) }                \
            if constexpr ((u) == 2 && !RS && !K8) { X_ISSUE(2, xc_, t) }                                        \
            if constexpr ((u) == 15) { if constexpr (K8) { X_FOLD(lcol, xa_, 0) } else { X_FOLD(0, xa_, 0) } H_MIX }   \
            if constexpr ((u) == 23) { if constexpr (K8) { X_FOLD(2, xb_, 1) X_FLAG } else { X_FOLD(1, xb_, 1) } H_MIX }   \
            if constexpr ((u) == 31 && !K8) { X_FOLD(2, xc_, 2) X_FLAG H_MIX }
#define H_FOLDREGION(u) (((u) & 7) >= 5 && (u) >= 8 && ((u) < 24 || !K8))
            // PAIR: the same work at the matching places of the 16-unit sequence - a unit is twelve MFMAs, the fold regions two units
#define HP_MIX                                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < 6; ++i_) {                                                          \
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                                      \
        __builtin_amdgcn_sched_group_barrier(0x002, 28, 0);                                                     \
    }
#define HP_EXTRA(v)                                                                                             \
            if constexpr ((v) + X3_D >= 16) { X3_LDD((v) + X3_D - 16, XU_H + (v) + X3_D) }                      \
            if constexpr ((v) == 1) { X_ISSUE(2, xc_, t) }                                                      \
            if constexpr ((v) == 7) { X_FOLD(0, xa_, 0) HP_MIX }                                                \
            if constexpr ((v) == 11) { X_FOLD(1, xb_, 1) HP_MIX }                                               \
            if constexpr ((v) == 15) { X_FOLD(2, xc_, 2) X_FLAG HP_MIX }
#define HP_FOLDREGION(v) (((v) & 3) >= 2 && (v) >= 4)
            if constexpr (PAIR) {
                X3P_HALF(XU_H, wh, RH, (ldsO + T_ROW_H * QSD), HP_EXTRA, HP_FOLDREGION)
            } else {
            X3_HALF(XU_H, wh, RH, H_EXTRA, H_FOLDREGION)
            }
            }
#undef HP_EXTRA
#undef HP_FOLDREGION
#undef HP_MIX
#undef H_EXTRA
#undef H_FOLDREGION
#undef H_MIX
#undef X_FOLD
#undef X_FLAG
        }
        f32x4 Sw[2];                              // the STFT's first fp32 blocks, cos and -sin: 8 kHz k-iteration 0, 16 kHz the even tile's first
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if constexpr (XFIRST) Sw[k] = SwF[k];     // requested by the prologue
            else Sw[k] = WL(ws_stft + (K8 ? 0 : 8) + k);
        }
        SB();
        STAMP(1);
        __syncthreads();   // (1) folded x visible
        STAMP(2);

        // ---- bin 128 on the VALU: 48 (column, stream) pairs, 4 lanes each ----
        {
            const int pair = tid >> 2, pt = tid & 3;
            const int c = pair >> 4, ms = pair & 15;
            float a = 0.f;
            if (pair < 48) {
#pragma unroll
                // 16 kHz: sum_n pe[n] (-1)^n = the same sum over the pe+ rows (slot 0 = pe[32], sign +); 8 kHz: over its 8 pe rows
                for (int i = 0; i < 2; ++i) {
                    const f32x4 pp = K8 ? RX[(CS * c + pt * 2 + i) * QSL + ms] : REV[(32 * c + pt * 2 + i) * QSL + ms];
                    a += (pp.x - pp.y) + (pp.z - pp.w);
                }
            }
            a += __shfl_xor(a, 1);
            a += __shfl_xor(a, 2);
            if (pair < 48 && pt == 0) nyqv[c * 16 + ms] = fabsf(a + fcor[(c * 3 + 0) * 16 + ms] + fcor[(c * 3 + 1) * 16 + ms]);
        }

        // enc0's fp32 blocks (bias, Nyquist taps) and its first X3_D units, requested before barrier (1b): 8 kHz in one block behind
        // the STFT (E0_FIRST), 16 kHz by the DFT's ring units, one each, and the fp32 blocks behind them
        f32x4 e0f[ENC0_X3_F32_BLOCKS];
    // PAIR: the wave's row tile is hf - its bias in e0f[0], its three Nyquist taps in e0f[1 ..]; unit v = (K-step, tap) = the stream's
    // unit 2 v + hf
#define E0P_BLK(v) (ws_x0 + ENC0_X3_F32_BLOCKS + 3 * (2 * (v) + hf))
#define E0_FIRST                                                                                                \
    _Pragma("unroll") for (int k = 0; k < ENC0_X3_F32_BLOCKS; ++k) e0f[k] = WX(ws_x0 + k);                      \
    _Pragma("unroll") for (int u_ = 0; u_ < X3_D; ++u_) { X3_LDX(ws_x0 + ENC0_X3_F32_BLOCKS + 3 * u_, u_) }
        if constexpr (K8) {
            // ---- STFT, 8 kHz sub-model: 64 complex bins = four 16-row tiles, ONE per wave (pack_dft4_wave_128_t16): wave w owns the
            //      bins 2 (16 (w & 1) + r) + (w >> 1), r = 0..15 - waves 0 / 1 the even bins (pe | qe), 2 / 3 the odd ones (po | qo);
            //      K = 32 = two k-iterations; the accumulators start from the rank-1 terms of n = 0, 32, 64 as in the 16 kHz model ----
            const bool even = w < 2;
            f32x4 sre[3], sim[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float y128 = fcor[(c * 3 + 0) * 16 + n], a64 = fcor[(c * 3 + 1) * 16 + n], b64 = fcor[(c * 3 + 2) * 16 + n];
                const float rp = even ? y128 + a64 : -y128, rm = even ? y128 - a64 : -y128;
                const float ip = even ? 0.f : -b64, im_ = even ? 0.f : b64;
                sre[c] = f32x4{rp, rm, rp, rm};
                sim[c] = f32x4{ip, im_, ip, im_};
            }
            const int rR = even ? 0 : QL, rI = even ? 2 * QL : 3 * QL;
            const f32x4 wr0 = Sw[0], wi0 = Sw[1], wr1 = WL(ws_stft + 2), wi1 = WL(ws_stft + 3);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x4 wr = j ? wr1 : wr0, wi = j ? wi1 : wi0;
                f32x4 u[3], v[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    u[c] = RX[(CS * c + rR + 4 * j) * QSL + nqL];
                    v[c] = RX[(CS * c + rI + 4 * j) * QSL + nqL];
                }
                SB();
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sre[c] = mfma16(wr, u[c], sre[c]);
                    sim[c] = mfma16(wi, v[c], sim[c]);
                }
                SB();
            }
            E0_FIRST
            SB();
            __syncthreads();   // (1b) every wave is done reading the folded operands: the magnitudes may overwrite them
            {   // |.| of the three columns -> planes: the wave's row tile (channels 16 w + 4 kq + i) is half w & 1 of K-step w >> 1's
                // fragments, plane group 24 c + 12 (w >> 1)
                f32x4 *o = RX + 12 * (w >> 1) * QSD + nq;
#pragma unroll
                for (int c = 0; c < 3; ++c) st_planes_half(o + PP * c * QSD, w & 1, pk::mag(sre[c], sim[c]));
            }
        } else
        // ---- STFT: wave w owns bins bin_of_channel_fold3(32 w + 16 rt + r).  Row tile 0 = 16 odd bins, cos on po, -sin on qo, K = 64, on
        //      the bf16 split: four ring units (part, K-step s) = 2 part + s of vad_layout.h's DFT_X3_BLOCKS, each feeding the three
        //      columns' plane groups (72 bf16 MFMAs where the fp32 form had 96 of twice the length).  Row tile 1 = 16 even bins on the
        //      once-more-folded operands pe+- | qe-+ (waves 2, 3 | 0, 1), K = 32: two fp32 k-iterations, 48 MFMAs ----
        {
            f32x4 are[3][2], aim[3][2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float y128 = fcor[(c * 3 + 0) * 16 + n], a64 = fcor[(c * 3 + 1) * 16 + n], b64 = fcor[(c * 3 + 2) * 16 + n];
                const float re1 = w < 2 ? y128 - a64 : y128 + a64;
                // register i of a D quad is tile row 4 rq + i: odd k: re = -y128, im = -+ b64 along the rows; even k = 2 m:
                // re = y128 + (-1)^m a64, im = 0
                are[c][0] = f32x4{-y128, -y128, -y128, -y128};
                aim[c][0] = f32x4{-b64, b64, -b64, b64};
                are[c][1] = f32x4{re1, re1, re1, re1};
                aim[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // the odd tile.  Piece p of the lane's fragment of plane group g of column c (the stream swizzled as the loader wrote it);
            // a column's pieces of unit v + 1 are read behind its MFMAs of unit v.  Every unit requests the encoder.0 unit X3_D units
            // behind it in the ring.
            const int nqs[2] = {kq * QSD + (n ^ kq), kq * QSD + (n ^ (kq | 4))};
#define D_RD(c, g, p) __builtin_bit_cast(u32x4, RX[(PP * (c) + 12 * (g) + 4 * (p)) * QSD + nqs[(g) & 1]])
            const int eR = w < 2 ? 16 : 0, eI = w < 2 ? 24 : 8;
            const f32x4 *const XB = REV + nqL;                                                  // loader view
            f32x4 Aw[2], Bw[2], Au[3], Av[3], Bu[3], Bv[3];
            {
                u32x4 F_[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int p_ = 0; p_ < 3; ++p_) F_[c][p_] = D_RD(c, 0, p_);
                SB();
                x3_units([&](auto uc_) {
                    constexpr int v_ = decltype(uc_)::value;
                    if constexpr (PAIR) { X3_LDX(E0P_BLK(v_), v_) } else { X3_LDX(ws_x0 + ENC0_X3_F32_BLOCKS + 3 * v_, v_) }
                    if constexpr (v_ == 3) {              // the even tile's first operands (its first blocks: Sw)
#pragma unroll
                        for (int c = 0; c < 3; ++c) { Au[c] = XB[(32 * c + eR) * QSL]; Av[c] = XB[(32 * c + eI) * QSL]; }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if constexpr (v_ < 2) are[c][0] = mfma_x3(xw[(XU_D + v_) % X3_NR], F_[c], are[c][0]);
                        else aim[c][0] = mfma_x3(xw[(XU_D + v_) % X3_NR], F_[c], aim[c][0]);
                        if constexpr (v_ + 1 < 4) {
#pragma unroll
                            for (int p_ = 0; p_ < 3; ++p_) F_[c][p_] = D_RD(c, v_ + 1, p_);
                        }
                    }
                    SB();
                }, std::make_integer_sequence<int, 4>{});
            }
#undef D_RD
            // encoder.0's fp32 blocks (bias, Nyquist taps), behind its first units
            if constexpr (PAIR) {
                e0f[0] = WX(ws_x0 + hf);
#pragma unroll
                for (int k = 0; k < 3; ++k) e0f[1 + k] = WX(ws_x0 + 2 + 2 * k + hf);
            } else {
#pragma unroll
                for (int k = 0; k < ENC0_X3_F32_BLOCKS; ++k) e0f[k] = WX(ws_x0 + k);
            }
            SB();
            // the even tile: k-iterations 4, 5 of S_STFT
#pragma unroll
            for (int k = 0; k < 2; ++k) Aw[k] = Sw[k];
#define S_LD(S, tt)                                                                        \
    _Pragma("unroll") for (int k = 0; k < 2; ++k) S##w[k] = WL(ws_stft + 2 * (tt) + k);    \
    _Pragma("unroll") for (int c = 0; c < 3; ++c) { S##u[c] = XB[(32 * c + eR + 4 * ((tt) - 4)) * QSL]; S##v[c] = XB[(32 * c + eI + 4 * ((tt) - 4)) * QSL]; }
#define S_MMA(S, rt)                                                                       \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                       \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                    \
            are[c][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(S##w[0][j_], S##u[c][j_], are[c][rt], 0, 0, 0); \
            aim[c][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(S##w[1][j_], S##v[c][j_], aim[c][rt], 0, 0, 0); \
        }
#define S_IL                                                                               \
    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 6; ++i_) {                                     \
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                 \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                 \
    }
            S_LD(B, 5) S_MMA(A, 1) S_IL SB();
            S_MMA(B, 1) SB();
#undef S_IL
#undef S_LD
#undef S_MMA
            SB();
            __syncthreads();   // (1b) every wave is done reading the folded operands: the magnitudes may overwrite them
            // |.| of the three columns -> planes: the wave's two row tiles are K-step w's fragments, plane group 48 c + 12 w
#pragma unroll
            for (int c = 0; c < 3; ++c)
                st_planes(RX + (PP * c + 12 * w) * QSD + nq, pk::mag(are[c][0], aim[c][0]), pk::mag(are[c][1], aim[c][1]));
        }
#undef E0_FIRST
        STAMP(3);
        __syncthreads();   // (2) magnitudes complete
        STAMP(4);

        // ---- enc0: 129 (8 kHz: 65) -> 128 ch, k3 s1 p1, 3 -> 3 columns, as a direct 3-tap convolution on the bf16 split (X3_CONV):
        //      per K-step 3 taps x 2 row tiles = 6 units, 7 column products per tile; the Nyquist channel and the bias on the VALU ----
        constexpr int NU0 = (K8 ? 2 : 4) * 3 * (PAIR ? 1 : 2);     // enc0's units: its K-steps x 3 taps x 2 row tiles (PAIR: one)
        f32x4 e1b;
        // enc1's bias and its first X3_D units ride in enc0's last units: the ring goes on, unit v of enc1 in slot NU0 + v
        // PAIR: enc1 runs by output column (below) - the wave's unit v = (K-step, j) is the stream's unit (K-step, tap j + 1 - hf)
#define E1P_BLK(v) (ws_y1 + ENC1_X3_F32_BLOCKS + 3 * (3 * ((v) >> 1) + ((v) & 1) + 1 - hf))
#define E0_EXTRA(u)                                                                                             \
            if constexpr ((u) == NU0 - X3_D) e1b = WY(ws_y1);                                                   \
            if constexpr ((u) + X3_D >= NU0) {                                                                  \
                if constexpr (PAIR) { X3_LDY(E1P_BLK((u) + X3_D - NU0), (u) + X3_D) }                           \
                else { X3_LDY(ws_y1 + ENC1_X3_F32_BLOCKS + 3 * ((u) + X3_D - NU0), (u) + X3_D) }                \
            }
        if constexpr (PAIR) {
            // wave (hf, w): row tile hf (channels 32 w + 16 hf ..) of the three output columns for BOTH half-tiles: 12 units of 3 KiB
            // where a tile's wave streams 24, the same 336 MFMAs.  acc[o][st], F_[st][c]: st = 0 the wave's own tile, 1 the partner's.
            // One K-step's 18 pieces are held; the next K-step's replace them as the taps let go of them: column 0 behind tap 1,
            // column 2 behind tap 2, column 1 - read by tap 2 and at once by the next tap 0 - through N1_, requested in tap 1.
            f32x4 acc[3][2];
            const float *const nyqO = reinterpret_cast<const float *>(ldsO + (T_ROW_H + T_ROWS_H) * QSD) + 64;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const float *const nq_ = st ? nyqO : nyqv;
                const float nv[3] = {nq_[n], nq_[16 + n], nq_[32 + n]};
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    f32x4 a = e0f[0];
#pragma unroll
                    for (int t = 0; t < 3; ++t)
                        if (o + t - 1 >= 0 && o + t - 1 < 3) a = pk::fma(e0f[1 + t], pk::splat(nv[o + t - 1]), a);
                    acc[o][st] = a;
                }
            }
#define E0P_SRC(st, c) (((st) ? ldsO : RX) + PP * (c) * QSD)
            u32x4 F_[2][3][3], N1_[2][3];
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int c_ = 0; c_ < 3; ++c_)
#pragma unroll
                    for (int p_ = 0; p_ < 3; ++p_) F_[st][c_][p_] = PL_RD(E0P_SRC(st, c_), 0, p_);
            SB();
            x3_units([&](auto uc_) {
                constexpr int v_ = decltype(uc_)::value, s_ = v_ / 3, t_ = v_ % 3;
                if constexpr (v_ + X3_D < NU0) { X3_LDX(E0P_BLK(v_ + X3_D), v_ + X3_D) }
                if constexpr (t_ == 1 && s_ + 1 < 4) {
#pragma unroll
                    for (int st = 0; st < 2; ++st)
#pragma unroll
                        for (int p_ = 0; p_ < 3; ++p_) N1_[st][p_] = PL_RD(E0P_SRC(st, 1), s_ + 1, p_);
                }
                E0_EXTRA(v_)
#pragma unroll
                for (int o_ = 0; o_ < 3; ++o_) {
                    const int c_ = o_ + t_ - 1;
                    if (c_ >= 0 && c_ < 3) {
#pragma unroll
                        for (int st = 0; st < 2; ++st) acc[o_][st] = mfma_x3(xw[v_ % X3_NR], F_[st][c_], acc[o_][st]);
                    }
                }
                if constexpr (s_ + 1 < 4 && t_ >= 1) {
#pragma unroll
                    for (int st = 0; st < 2; ++st)
#pragma unroll
                        for (int p_ = 0; p_ < 3; ++p_) {
                            if constexpr (t_ == 1) F_[st][0][p_] = PL_RD(E0P_SRC(st, 0), s_ + 1, p_);
                            else { F_[st][1][p_] = N1_[st][p_]; F_[st][2][p_] = PL_RD(E0P_SRC(st, 2), s_ + 1, p_); }
                        }
                }
                SB();
            }, std::make_integer_sequence<int, NU0>{});
#undef E0P_SRC
            // ReLU -> planes: half hf of K-step w's fragments in each half-tile's plane group 144 + 48 c + 12 w
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    st_planes_half((st ? ldsO : ldsH) + (T_ROW_E0 + 48 * c + 12 * w) * QSD + nq, hf, relu4(acc[c][st]));
        } else {
            f32x4 acc[3][2];
            {   // accumulators start at the bias plus the Nyquist channel's terms sum_tap W[tap] |X_N|[o + tap - 1], exact fp32 fmas
                const float nv[3] = {nyqv[n], nyqv[16 + n], nyqv[32 + n]};
#pragma unroll
                for (int o = 0; o < 3; ++o)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) {
                        f32x4 a = e0f[rt];
#pragma unroll
                        for (int t = 0; t < 3; ++t)
                            if (o + t - 1 >= 0 && o + t - 1 < 3) a = pk::fma(e0f[2 + 2 * t + rt], pk::splat(nv[o + t - 1]), a);
                        acc[o][rt] = a;
                    }
            }
#define E0_SRC(c) (RX + PP * (c) * QSD)
            X3_CONV(K8 ? 2 : 4, 2, 1, 3, X3_LDX, ws_x0 + ENC0_X3_F32_BLOCKS, 0, E0_SRC, acc, E0_EXTRA)
#undef E0_SRC
            // ReLU -> planes: the wave's channels 32 w .. are K-step w of enc1's fragments, plane group 144 + 48 c + 12 w
#pragma unroll
            for (int c = 0; c < 3; ++c) st_planes(RP0 + (48 * c + 12 * w) * QSD + nq, relu4(acc[c][0]), relu4(acc[c][1]));
        }
#undef E0_EXTRA
#undef E0P_BLK
        STAMP(5);
        __syncthreads();   // (3) enc0 out
        STAMP(6);

        // ---- enc1: 128 -> 64 ch, k3 s2 p1, 3 -> 2 columns, on the bf16 split (X3_CONV, S_ENC1_X3): wave w = channels 16 w .. 16 w + 15
        //      (one row tile) of BOTH output columns; per K-step 3 taps = 3 units, 4 column products (tap 0 -> column 1 on x1, tap 1 ->
        //      column 0 on x0 and column 1 on x2, tap 2 -> column 0 on x1): 96 bf16 MFMAs where the fp32 form had 128 of twice the length ----
        // The ring goes on through enc2 and enc3 (vad_layout.h, ENC23_X3_BLOCKS; the blocks lie behind the third stream) into the LSTM's
        // input half: enc2's unit v in slot XU_2 + v, enc3's in XU_3 + v, the input half's from XU_L on - every unit requests the
        // one X3_D units behind it, whichever layer that belongs to.
        // PAIR: enc1 and enc3 serve both half-tiles from every unit, as the LSTM halves and enc0 do, and stream two thirds | half of the
        // units: enc1 by output column (8 of the 12), enc3 by row tile (2 of the 4).  The ring's sequence is then enc1's 8, enc2's 4,
        // enc3's 2, the input half's 16: enc2's units request enc3's two and the input half's first two, enc3's the next two.
        // XFIRST: the recurrent half's 16 units follow enc3's, from XU_R on, and the input half's follow those - enc2's and enc3's units
        // request the recurrent half's first four, the recurrent half's last four the input half's first.
        constexpr int NU1 = PAIR ? 4 * 2 : 4 * 3, NU2 = 4, NU3 = PAIR ? 2 : 4, XU_2 = NU0 + NU1, XU_3 = XU_2 + NU2, XU_R = XU_3 + NU3;
        constexpr int XU_L = XFIRST ? XU_R + NH : XU_R;
        static_assert(!XFIRST || ((XU_D + 4) % X3_NR == 0 && XU_R == NU0 + NU1 + NU2 + NU3 && XU_L == XU_R + NH && NH >= X3_D),
                      "frames first: the ring runs DFT -> enc0 -> enc1 -> enc2 -> enc3 -> recurrent half -> input half, every unit one slot on");
        // the unit X3_D behind enc2's / enc3's in the ring, counted from the LSTM half that follows enc3
#define X3_LDN(v) if constexpr (XFIRST) { X3_LDP(ws_x3 + LSTM_X3_HALF_BLOCKS, v, XU_R) } else { X3_LDU(ws_x3, v, XU_L) }
        static_assert(NU1 >= X3_D && NU2 == X3_D && (PAIR || NU3 == X3_D),
                      "enc1's last X3_D units request enc2's units, enc2's units enc3's, enc3's the input half's first");
        static_assert(!PAIR || (NU3 <= X3_D && NU2 + NU3 >= X3_D),
                      "paired: enc2's units request enc3's NU3 and the input half's first X3_D - NU3, enc3's the input half's next NU3");
        f32x4 e2b, e3b[2];
        // enc3's unit v of the wave: PAIR (K-step v, row tile hf) = the stream's unit 2 v + hf
#define E3_BLK(v) (ws_z + ENC2_X3_BLOCKS + 2 + 3 * (PAIR ? 2 * (v) + hf : (v)))
        if constexpr (PAIR) {
            // wave (hf, w): output column hf of row tile w for BOTH half-tiles.  Column 0 = taps 1, 2 on input columns 0, 1; column 1 =
            // taps 0, 1 on input columns 1, 2: unit v = (K-step s, j) is tap j + 1 - hf on input column hf + j, in the stream's K-step-
            // major order - an accumulator sees the mfma_x3 it sees in the unpaired form, in the same order.  8 units of 3 KiB where a
            // tile's wave streams 12, the same 96 MFMAs.  acc[st], F_[st][j]: st = 0 the wave's own tile, 1 the partner's.  One
            // K-step's 12 pieces are held; the next K-step's replace input column hf + j's behind the unit that read them.
            f32x4 acc[2] = {e1b, e1b};
#define E1P_SRC(st, j) (((st) ? ldsO + T_ROW_E0 * QSD : RP0) + 48 * (hf + (j)) * QSD)
#define E1_EXTRA(u)                                                                                             \
            if constexpr ((u) == NU1 - X3_D) {     /* the fp32 blocks of the next two layers: their biases */    \
                e2b = WY(ws_z);                                                                                 \
                e3b[0] = WY(ws_z + ENC2_X3_BLOCKS + hf);     /* enc3's row tile hf */                           \
            }                                                                                                   \
            if constexpr ((u) + X3_D >= NU1) { X3_LDY(ws_z + 1 + 3 * ((u) + X3_D - NU1), XU_2 + (u) + X3_D - NU1) }
            u32x4 F_[2][2][3];
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int j_ = 0; j_ < 2; ++j_)
#pragma unroll
                    for (int p_ = 0; p_ < 3; ++p_) F_[st][j_][p_] = PL_RD(E1P_SRC(st, j_), 0, p_);
            SB();
            x3_units([&](auto uc_) {
                constexpr int v_ = decltype(uc_)::value, s_ = v_ >> 1, j_ = v_ & 1;
                if constexpr (v_ + X3_D < NU1) { X3_LDY(E1P_BLK(v_ + X3_D), NU0 + v_ + X3_D) }
                E1_EXTRA(v_)
#pragma unroll
                for (int st = 0; st < 2; ++st) acc[st] = mfma_x3(xw[(NU0 + v_) % X3_NR], F_[st][j_], acc[st]);
                if constexpr (s_ + 1 < 4) {
#pragma unroll
                    for (int st = 0; st < 2; ++st)
#pragma unroll
                        for (int p_ = 0; p_ < 3; ++p_) F_[st][j_][p_] = PL_RD(E1P_SRC(st, j_), s_ + 1, p_);
                }
                SB();
            }, std::make_integer_sequence<int, NU1>{});
#undef E1P_SRC
#undef E1_EXTRA
            // ReLU -> planes: half w & 1 of K-step w >> 1 of output column hf, in each half-tile's plane group 24 hf + 12 (w >> 1)
#pragma unroll
            for (int st = 0; st < 2; ++st)
                st_planes_half((st ? ldsO : ldsH) + (24 * hf + 12 * (w >> 1)) * QSD + nq, w & 1, relu4(acc[st]));
        } else {
            f32x4 acc[2][1] = {{e1b}, {e1b}};
#define E1_SRC(c) (RP0 + 48 * (c) * QSD)
#define E1_EXTRA(u)                                                                                             \
            if constexpr ((u) == NU1 - X3_D) {     /* the fp32 blocks of the next two layers: their biases */    \
                e2b = WY(ws_z);                                                                                 \
                e3b[0] = WY(ws_z + ENC2_X3_BLOCKS); e3b[1] = WY(ws_z + ENC2_X3_BLOCKS + 1);                     \
            }                                                                                                   \
            if constexpr ((u) + X3_D >= NU1) { X3_LDY(ws_z + 1 + 3 * ((u) + X3_D - NU1), XU_2 + (u) + X3_D - NU1) }
            X3_CONV(4, 1, 2, 2, X3_LDY, ws_y1 + ENC1_X3_F32_BLOCKS, NU0, E1_SRC, acc, E1_EXTRA)
#undef E1_SRC
#undef E1_EXTRA
            // ReLU -> planes: the wave's channels 16 w .. are half w & 1 of K-step w >> 1 of their column; column o's two K-steps are enc2's
            // units 2 o, 2 o + 1, plane group 24 o + 12 (w >> 1) (the |STFT| planes there are dead behind barrier (3))
#pragma unroll
            for (int o = 0; o < 2; ++o) st_planes_half(RX + (24 * o + 12 * (w >> 1)) * QSD + nq, w & 1, relu4(acc[o][0]));
        }
#undef E1P_BLK
        STAMP(7);
        __syncthreads();   // (4) enc1 out as planes in rows 0..47
        STAMP(8);
        // XFIRST: h_{t-1} -> its planes, now that enc0's output above them is dead (rows 248..295; enc2's planes, rows 168..191, the x
        // planes, rows 0..47, and the head exchange rows 144..175 stay clear of them), and the biases and the state machines to their
        // places: the recurrent half reads the planes of both halves behind barrier (5)
        if constexpr (XFIRST) H_TO_LDS

        // ---- enc2: 64 -> 64 ch, k3 s2 p1, 2 -> 1 column, on the bf16 split: wave w = channels 16 w .. 16 w + 15 (one row tile) over the
        //      whole K = 128: four units (input column c on tap 1 + c - tap 0 meets the padding only -, K-step s) = enc1's plane group
        //      2 c + s, one accumulator from the bias on: 24 bf16 MFMAs where the split-K fp32 form had 32 of twice the length and a
        //      round trip of the partial sums through LDS ----
        {
            f32x4 acc = e2b;
            u32x4 F_[2][3];
#pragma unroll
            for (int p_ = 0; p_ < 3; ++p_) F_[0][p_] = PL_RD(RX, 0, p_);
            SB();
            x3_units([&](auto uc_) {
                constexpr int v_ = decltype(uc_)::value;
                if constexpr (v_ < NU3) { X3_LDY(E3_BLK(v_), XU_3 + v_) }           // enc3's unit v
                else { X3_LDN(v_ - NU3) }                                           // PAIR: behind enc3's two, the next LSTM half's first
                if constexpr (v_ + 1 < NU2) {
#pragma unroll
                    for (int p_ = 0; p_ < 3; ++p_) F_[(v_ + 1) & 1][p_] = PL_RD(RX, v_ + 1, p_);
                }
                acc = mfma_x3(xw[(XU_2 + v_) % X3_NR], F_[v_ & 1], acc);
                SB();
            }, std::make_integer_sequence<int, NU2>{});
            // ReLU -> planes: half w & 1 of K-step w >> 1 of enc3's input (enc0's output there is dead behind barrier (4))
            st_planes_half(RE + 12 * (w >> 1) * QSD + nq, w & 1, relu4(acc));
        }
        STAMP(9);
        __syncthreads();   // (5) enc2 out as planes
        STAMP(10);

        // ---- enc3: 64 -> 128 ch, centre tap, on the bf16 split: two row tiles over two K-steps, units (K-step s, rt); a K-step's
        //      pieces are read once for both row tiles ----
        if constexpr (PAIR) {
            // wave (hf, w): row tile hf of wave w's two (channels 32 w + 16 hf ..) for BOTH half-tiles: unit s = the stream's unit
            // (K-step s, rt = hf), two units of 3 KiB where a tile's wave streams four, the same 24 MFMAs.  acc[st], F_[st][s]: st = 0 the
            // wave's own tile, 1 the partner's (its enc2 planes: complete behind barrier (5), which both halves run).
            f32x4 acc[2] = {e3b[0], e3b[0]};
#define E3P_SRC(st) ((st) ? ldsO + T_ROW_E * QSD : RE)
            u32x4 F_[2][2][3];
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int p_ = 0; p_ < 3; ++p_) F_[st][0][p_] = PL_RD(E3P_SRC(st), 0, p_);
            SB();
            x3_units([&](auto uc_) {
                constexpr int v_ = decltype(uc_)::value;
                X3_LDN(v_ + X3_D - NU3)                                             // the next LSTM half's unit v + 2
                if constexpr (v_ == 0) {
#pragma unroll
                    for (int st = 0; st < 2; ++st)
#pragma unroll
                        for (int p_ = 0; p_ < 3; ++p_) F_[st][1][p_] = PL_RD(E3P_SRC(st), 1, p_);
                }
#pragma unroll
                for (int st = 0; st < 2; ++st) acc[st] = mfma_x3(xw[(XU_3 + v_) % X3_NR], F_[st][v_], acc[st]);
                SB();
            }, std::make_integer_sequence<int, NU3>{});
#undef E3P_SRC
            // ReLU -> planes: half hf of K-step w of the LSTM's input half, in each half-tile's x planes
#pragma unroll
            for (int st = 0; st < 2; ++st) st_planes_half((st ? ldsO : ldsH) + 12 * w * QSD + nq, hf, relu4(acc[st]));
            if constexpr (XFIRST) {
                // ---- the recurrent gate half W_hh . h_{t-1}, from the biases on (the wave reads what the wave itself wrote), on both
                //      halves' h planes (complete behind barrier (5)); its last units request the input half's first, and the input
                //      half adds onto the same accumulators behind barrier (6): every accumulator sees the MFMAs it saw, in their order ----
                STAMP(31);
                const f32x4 *const bq = biasL + 32 * w + kq;
#pragma unroll
                for (int k = 0; k < 4; ++k) Gp[k][0] = Gp[k][1] = bq[k * 8 + hf * 4];
#define HX_EXTRA(v) if constexpr ((v) + X3_D >= NH) { X3_LDP(ws_x3, (v) + X3_D - NH, XU_L) }
#define HX_FOLDREGION(v) false
                X3P_HALF(XU_R, (ws_x3 + LSTM_X3_HALF_BLOCKS), RH, (ldsO + T_ROW_H * QSD), HX_EXTRA, HX_FOLDREGION)
#undef HX_EXTRA
#undef HX_FOLDREGION
                STAMP(26);
            }
        } else {
            f32x4 acc[2] = {e3b[0], e3b[1]};
            u32x4 F_[2][3];
#pragma unroll
            for (int p_ = 0; p_ < 3; ++p_) F_[0][p_] = PL_RD(RE, 0, p_);
            SB();
            x3_units([&](auto uc_) {
                constexpr int v_ = decltype(uc_)::value, s_ = v_ >> 1, rt_ = v_ & 1;
                X3_LDU(ws_x3, v_, XU_L)                                             // the LSTM input half's unit v
                if constexpr (v_ == 0) {
#pragma unroll
                    for (int p_ = 0; p_ < 3; ++p_) F_[1][p_] = PL_RD(RE, 1, p_);
                }
                acc[rt_] = mfma_x3(xw[(XU_3 + v_) % X3_NR], F_[s_], acc[rt_]);
                SB();
            }, std::make_integer_sequence<int, NU3>{});
            st_planes(RX + 12 * w * QSD + nq, relu4(acc[0]), relu4(acc[1]));      // channels 32 w .. = K-step w of the LSTM's input half
        }
#undef E3_BLK
#undef X3_LDN
        STAMP(11);
        __syncthreads();   // (6) LSTM input x as planes in rows 0..47
        STAMP(12);

        // ---- LSTM: input half W_ih . x on top of the recurrent half, cell, head partial ----
        {
            const int ws = ws_l + 8;
            f32x4 hw[2];
#define L_EXTRA(u) if constexpr ((u) == 24) { hw[0] = WL(ws + 128); hw[1] = WL(ws + 129); }
#define L_FOLDREGION(u) false
#define LP_EXTRA(v) if constexpr ((v) == 12) { hw[0] = WL(ws + 128 + hf); }      /* the head weights of the wave's own row tile */
            if constexpr (PAIR) {
                X3P_HALF(XU_L, ws_x3, RX, ldsO, LP_EXTRA, L_FOLDREGION)
            } else {
            X3_HALF(XU_L, ws_x3, RX, L_EXTRA, L_FOLDREGION)
            }
#undef LP_EXTRA
#undef L_EXTRA
#undef L_FOLDREGION
            STAMP(18);
            STAMP(13);
            if constexpr (PAIR) {
                // PAIR, the cell in place: the wave holds all four gates of units 32 w + 16 hf + 4 kq + i for both tiles' streams
                // (Gp[q][st]) and their c_{t-1} (cst[st]), so it runs the cell of its row tile for both tiles the moment its own
                // MFMAs end - no barrier (7): that barrier orders the cell's rewriting of the h planes against the recurrent half's
                // reads of them, and a one-frame launch (PAIR implies ONE: the assert below) never rewrites them; what it orders here is
                // nothing: behind barrier (6) the other waves read the x planes (rows 0 .. T_ROWS_H - 1 of both halves) and
                // registers only, and this wave writes global state (its own lanes' units) and the exchange rows below.
                // Gates, c' and h' are lane-local, the parent's formulas and order.  Only the head partial crosses row tiles:
                // part4 = fma(hw[1], relu(h'_rt1), fma(hw[0], relu(h'_rt0), 0)) - wave (0, w) forms the inner fma (WITH its zero addend:
                // a negative weight times +0 stays +0) for both tiles and hands the two quads to wave (1, w) across barrier (8) through
                // half 0's rows T_ROW_E0 + 8 w + 4 (the tile's half) + kq (enc0's output, dead since barrier (4), enc2's planes, dead since (6):
                // silero_v5_t16.hip, T_ROWS_HEADX); wave (1, w) forms the outer fma, reduces as ever and writes each tile's own headp.
                static_assert(!PAIR || ONE, "no barrier (7): nothing rewrites the h planes");
                const uint8_t *const flagO = reinterpret_cast<const uint8_t *>(ldsO + T_LDS_F4);       // the partner half's flagL
                float *const headpO = reinterpret_cast<float *>(ldsO + (T_ROW_H + T_ROWS_H) * QSD);    // and its headp
                f32x4 *const hx = lds + (T_ROW_E0 + 8 * w) * QSD + nq;
                f32x4 hr[2];
                // (the two slots cross the launch as one register each: opaque here, so that the store addresses are formed here
                //  and not kept, two registers apiece, from the prologue's loads on - the launch's register peak is in enc0)
                int sl[2] = {slot, slot_o};
                asm volatile("" : "+v"(sl[0]), "+v"(sl[1]));
                // the head weights have long arrived (requested in unit 12); saying so HERE, in front of the state stores, keeps the
                // wait for them from landing behind the stores, where it is a vmcnt(0) that also waits for the stores' acknowledgement
                asm volatile("" ::"v"(hw[0]) : "memory");
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const f32x4 i4 = Gp[0][st], f4 = Gp[1][st], g4 = Gp[2][st], o4 = Gp[3][st], c4 = cst[st];
                    const f32x4 cn = pk::fma(pk::sigmoid4(f4), c4, pk::mul(pk::sigmoid4(i4), pk::tanh4(g4)));
                    const f32x4 hn = pk::mul(pk::sigmoid4(o4), pk::tanh4(cn));
                    hr[st] = relu4(hn);
                    // a rejected frame (float32 only) leaves the stream's h and c as they were; per tile, each by its own half's verdict
                    const bool bad = f32in && (st ? flagO[n] : flagL[n]) != 0;
                    if ((st ? live_o : live) && !bad) {
                        float *const sp = KP(state) + (size_t)sl[st] * 256 + 32 * w + 16 * hf + 4 * kq;
                        *reinterpret_cast<f32x4 *>(sp) = hn;
                        *reinterpret_cast<f32x4 *>(sp + 128) = cn;
                    }
                }
                if (hf == 0) {
#pragma unroll
                    for (int st = 0; st < 2; ++st) hx[4 * st * QSD] = pk::fma(hw[0], hr[st], f32x4{0.f, 0.f, 0.f, 0.f});   // st = the tile's half
                }
                STAMP(14);
                __syncthreads();   // (8) the row tile 0 terms of the head partials are visible
                STAMP(15);
                if (hf != 0) {
                    // the parent's sums in the parent's order.  The exchanges are spelled out on `lane`: __shfl_xor's own lane
                    // arithmetic is hoisted to its first use in the STFT and held in two registers across enc0, the launch's register
                    // peak.  (The two tiles' chains written side by side, so that their LDS round trips overlap, build with 242 / 238
                    // registers instead of 238 / 236: not taken.)
#pragma unroll
                    for (int st = 0; st < 2; ++st) {
                        const f32x4 part4 = pk::fma(hw[0], hr[st], hx[4 * (1 - st) * QSD]);     // this wave's tile st is half 1 - st
                        float part_ = (part4.x + part4.y) + (part4.z + part4.w);
                        part_ += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, __builtin_bit_cast(int, part_)));
                        part_ += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __builtin_bit_cast(int, part_)));
                        if (kq == 0) (st ? headpO : headp)[w * 16 + n] = part_;
                    }
                }
                __syncthreads();   // (8b) head partials visible
                STAMP(16);
            } else {
            __syncthreads();   // (7) every wave is done reading h_{t-1}
            STAMP(14);
            f32x4 part4 = f32x4{0.f, 0.f, 0.f, 0.f};
            // a rejected frame (float32 only) leaves the stream's h and c as they were: not stored, and held for the next frame
            // SCAN: so does, in every format, a frame past the end of the stream's recording
            const bool rej = f32in && (K8 ? (flagL[n] | flagL[16 + n]) : flagL[n]) != 0;
            const bool bad = SCAN ? (rej || t >= ncol) : rej;
            f32x4 hq[2];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const f32x4 i4 = G[0 + rt], f4 = G[2 + rt], g4 = G[4 + rt], o4 = G[6 + rt], c4 = cst[rt], hwv = hw[rt];
                // c' = sigma(f) c + sigma(i) tanh(g); h' = sigma(o) tanh(c'); head partial += w relu(h') - a quad at a time, the
                // full-rate arithmetic packed (pk::), the transcendentals per component
                f32x4 cn = pk::fma(pk::sigmoid4(f4), c4, pk::mul(pk::sigmoid4(i4), pk::tanh4(g4)));
                f32x4 hn = pk::mul(pk::sigmoid4(o4), pk::tanh4(cn));
                part4 = pk::fma(hwv, relu4(hn), part4);
                if constexpr ((f32in || SCAN) && !ONE && !RS) {   // (the head ignores z of a rejected stream)
                    hn = bad ? hv[rt] : hn;             // h_{t-1}: the lane's own units, kept in registers beside c (LDS holds pieces)
                    cn = bad ? c4 : cn;
                    hv[rt] = hn;
                }
                hq[rt] = hn;
                // (one frame: a rejected stream skips the store; more: the held values go back, the last accepted frame's)
                if (t == T - 1 && live && !((ONE || RS) && bad)) {
                    *reinterpret_cast<f32x4 *>(KP(state) + (size_t)slot * 256 + 32 * w + 16 * rt + 4 * kq) = hn;
                    *reinterpret_cast<f32x4 *>(KP(state) + (size_t)slot * 256 + 128 + 32 * w + 16 * rt + 4 * kq) = cn;
                }
                cst[rt] = cn;
            }
            // h_t for the next frame's recurrent half, as planes (a single-frame call has no next frame)
            if constexpr (!ONE && !RS) st_planes(RH + 12 * w * QSD + nq, hq[0], hq[1]);
            float part_ = (part4.x + part4.y) + (part4.z + part4.w);
            part_ += __shfl_xor(part_, 16);
            part_ += __shfl_xor(part_, 32);
            if (kq == 0) headp[w * 16 + n] = part_;
            }
        }
        if constexpr (!PAIR) {
        __syncthreads();   // (8) head partials + new h visible
        STAMP(15);
        }

        if (tid < MT16) {
            const float z = hb + ((headp[tid] + headp[16 + tid]) + (headp[32 + tid] + headp[48 + tid]));
            const float p = fminf(sigmoidf_(z), 1.0f);
            if (sm_thread) {
                // rejected (include/vad_engine.h): NaN and VAD_EV_REJECTED alone, no sm_step, the state machine as it was
                const bool bad = f32in && (K8 ? (flagL[tid] | flagL[16 + tid]) : flagL[tid]) != 0;
                if constexpr (SCAN) {
                    // tid < 16: this thread's column is the item whose ncol / obase it holds.  A frame past the recording's end
                    // writes nothing and steps nothing; the slot goes back as it is.  seg: the finished segment's length on
                    // every END, 0 on every other frame of the recording (one entry per frame)
                    SmSlot sm = smL[tid];
                    if (t < ncol) {
                        const size_t o = (size_t)obase + (size_t)t;
                        int seg = 0;
                        const int ev = bad ? EV_REJECTED : sm_step(sm, p, &seg);
                        P.probs[o] = bad ? __builtin_nanf("") : p;
                        if (P.events) P.events[o] = (uint8_t)ev;
                        if (P.seg_frames) P.seg_frames[o] = (ev & 2) ? seg : 0;
                    }
                    if (t == T - 1) KP(sm)[sm_slot] = sm;
                    else smL[tid] = sm;
                } else {
                P.probs[(size_t)gf * T + t] = bad ? __builtin_nanf("") : p;   // tid < 16: this thread's column is stream gf
                SmSlot sm = smL[tid];
                int seg = 0;
                const int ev = bad ? EV_REJECTED : sm_step(sm, p, &seg);
                if (t == T - 1) { if (!((ONE || RS) && bad)) KP(sm)[sm_slot] = sm; }
                else smL[tid] = sm;
                if (ev & 2) seg_last = seg;
                if (P.events) P.events[(size_t)gf * T + t] = (uint8_t)ev;
                }
            }
        }
        if (++t >= T) break;
        if constexpr (!RS) H_FIRST(ws_x3, t, true) // the next frame's first requests
    }
#undef H_TO_LDS
#undef H_STATE_SM
#undef H_STATE_H
#undef H_FIRST
#undef H_FIRSTX
#undef X3_LDU
#undef X3_LDP
#undef X3_LD
#undef X3_LDR
#undef X3_LDX
#undef X3_LDD
#undef X3_LDY
#undef WY
#undef WX
#undef X_ISSUE
#undef X_K0
#undef WL
    if constexpr (!SCAN) { if (sm_thread && P.seg_frames) P.seg_frames[gf] = seg_last; }
    if constexpr (!RS) STAMP(27);                 // the wave's last store is issued ...
    STAMP_DRAIN(28);                              // ... and acknowledged
#undef KP
