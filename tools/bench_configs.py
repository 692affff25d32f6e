#!/usr/bin/env python3
"""The other BASELINE.json configs on ONE GPU (bench.py measures the headline, configs[2]):

  configs[1]  batch=1024 streams, V5
  configs[3]  batch=4096 streams mixed 8/24/48 kHz -> on-GPU resample -> V5
  configs[4]  per-GPU share of the 65 536-stream job: 4096 V4 + 4096 V5 streams (two engines, two HIP streams)

Prints one JSON object per config (frames/s, us per step).  Device-resident inputs, HIP-event timing.
"""
import json
import os
import sys

# VAD_BENCH_TREE (the scan_segments comparison of two commits, nothing else; never set by the product or the tests): import the
# package from another checkout, its library built, and time it with this file's code.  It holds for whatever config is run with it
# - the package is imported once, here - so set it for scan_segments alone: an older tree need not have what the other configs call.
sys.path.insert(0, os.environ.get("VAD_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cutter_vad_amd import weights_io  # noqa: E402
from cutter_vad_amd.engine import Engine  # noqa: E402

K, WU = int(os.environ.get("VAD_BENCH_K", "400")), int(os.environ.get("VAD_BENCH_WU", "50"))     # (tools/pmc_rs.sh shortens the runs under --pmc)


def blob(v):
    return open(weights_io.packaged_blob_path(v), "rb").read()


def timed(fn, streams):
    for i in range(WU):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(streams[0])
    for i in range(K):
        fn(WU + i)
    for s in streams[1:]:
        streams[0].wait_stream(s)
    e1.record(streams[0])
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / K


def config1():
    B = 1024
    eng = Engine(blob(5), max_streams=B)
    eng.open_streams(B)
    ring = (0.1 * torch.randn(32, B, 512, device="cuda")).contiguous()
    probs = torch.empty(B, device="cuda")
    ts = torch.cuda.Stream()
    dt = timed(lambda i: eng.step_device(B, ring[i % 32].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
    eng.close()
    return {"config": "configs[1]: batch=1024, V5, 16 kHz", "us_per_step": dt * 1e6, "frames_per_s": B / dt}


def tile_shapes():
    """V5, device-resident, both tile shapes at the batch sizes where the choice matters (vad_debug_set_tile)."""
    out = []
    for B in (256, 1024, 2048, 4096, 8192):
        eng = Engine(blob(5), max_streams=B)
        eng.open_streams(B)
        ring = (0.1 * torch.randn(16, B, 512, device="cuda")).contiguous()
        probs = torch.empty(B, device="cuda")
        ts = torch.cuda.Stream()
        row = {"config": f"batch={B}, V5, device-resident", "streams": B}
        for tile in (32, 16):
            eng.set_tile(tile)
            dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
            row[f"us_per_step_tile{tile}"] = dt * 1e6
            row[f"frames_per_s_tile{tile}"] = B / dt
        eng.close()
        out.append(row)
    return out


def config3(per=None):
    """configs[3]: 4 096 streams, a third each at 8 / 24 / 48 kHz (1 365 + 1 365 + 1 366) unless `per` names another split"""
    B = 4096
    per = list(per) if per is not None else [1365, 1365, 1366]
    eng = Engine(blob(5), max_streams=B)
    eng.open_streams(B)
    rates = ((8000, 256), (24000, 768), (48000, 1536))
    rings = [(0.1 * torch.randn(8, per[k], n_in, device="cuda")).contiguous() for k, (_, n_in) in enumerate(rates)]
    total = sum(per)
    probs = torch.empty(total, device="cuda")
    ts = torch.cuda.Stream()

    def step(i):
        # ONE product call (vad_step_rates_device)
        eng.step_rates_device([(rings[k][i % 8].data_ptr(), per[k], sr) for k, (sr, _n) in enumerate(rates)], probs.data_ptr(),
                              stream=ts.cuda_stream)

    dt = timed(step, [ts])
    eng.set_tile(-1)                  # the two-launch form of the same call: resample kernel, then the model kernel
    dt2 = timed(step, [ts])
    eng.close()
    tiles = (total + 15) // 16
    return {"config": f"configs[3]: batch={total} ({' + '.join(map(str, per))}) mixed 8/24/48 kHz -> vad_step_rates_device; {tiles} 16-stream tiles "
                      "(the tiles walk the segments end to end; a tile at a rate boundary resamples its two parts in turn): "
                      + ("ONE fused launch (every tile resamples its chunks into LDS and steps from there)" if tiles <= 256 else
                         "more tiles than CUs -> resample launch + model launch"),
            "us_per_step": dt * 1e6, "frames_per_s": total / dt, "us_per_step_two_launches_forced": dt2 * 1e6}


def rates_one(which):
    """every tile at ONE input rate (4 096 streams): the fused launch's time = model tile + that rate's resample prologue"""
    per = [0, 0, 0]
    per[which] = 4096
    r = config3(per)
    r["config"] = f"4 096 streams, all at {(8000, 24000, 48000)[which]} Hz, fused resample -> step"
    return r


def rates8():
    return rates_one(0)


def rates24():
    return rates_one(1)


def rates48():
    return rates_one(2)


def config3_255_tiles():
    """configs[3] with the three thirds rounded to whole tiles (3 x 1 360 = 4 080 streams = 255 tiles): the fused launch"""
    return config3([1360, 1360, 1360])


def config3_pipelined():
    """configs[3] with the caller's software pipeline: the resample launch of tick t+1 runs on a second HIP stream beside
    the model step of tick t (4 095 streams leave half the CUs free, and the resample workgroups fit beside nothing else of
    the model kernel's).  Every tick is still resampled and then stepped in order; two 16 kHz buffers alternate."""
    B = 4096
    per = B // 3
    eng = Engine(blob(5), max_streams=B)
    eng.open_streams(B)
    rates = ((8000, 256), (24000, 768), (48000, 1536))
    rings = [(0.1 * torch.randn(8, per, n_in, device="cuda")).contiguous() for _, n_in in rates]
    f16 = [torch.empty(3 * per, 512, device="cuda") for _ in range(2)]
    probs = torch.empty(3 * per, device="cuda")
    sr_, sm_ = torch.cuda.Stream(), torch.cuda.Stream()
    resampled = [torch.cuda.Event() for _ in range(2)]
    consumed = [torch.cuda.Event() for _ in range(2)]
    for ev in consumed:
        ev.record(sm_)

    def step(i):
        b = i & 1
        sr_.wait_event(consumed[b])                    # the model step two ticks back has read this buffer
        eng.resample_multi_device([(rings[k][i % 8].data_ptr(), per, n_in, sr, f16[b][k * per:(k + 1) * per].data_ptr())
                                   for k, (sr, n_in) in enumerate(rates)], stream=sr_.cuda_stream)
        resampled[b].record(sr_)
        sm_.wait_event(resampled[b])
        eng.step_device(3 * per, f16[b].data_ptr(), probs.data_ptr(), stream=sm_.cuda_stream)
        consumed[b].record(sm_)

    dt = timed(step, [sm_, sr_])
    eng.close()
    return {"config": "configs[3], resample of tick t+1 on a second HIP stream beside the model step of tick t",
            "us_per_step": dt * 1e6, "frames_per_s": 3 * per / dt}


def config4_per_gpu():
    B = 4096
    # two engines share the GPU: VAD_ENGINE_SHARED_GPU keeps V5 on 32-stream tiles (128 CUs), V4's 128 tiles run beside it
    e5, e4 = Engine(blob(5), max_streams=B, shared_gpu=True), Engine(blob(4), model_version=4, max_streams=B, shared_gpu=True)
    e5.open_streams(B)
    e4.open_streams(B)
    ring = (0.1 * torch.randn(16, 2 * B, 512, device="cuda")).contiguous()
    p5, p4 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    s5, s4 = torch.cuda.Stream(), torch.cuda.Stream()

    def step(i):
        e5.step_device(B, ring[i % 16, :B].data_ptr(), p5.data_ptr(), stream=s5.cuda_stream)
        e4.step_device(B, ring[i % 16, B:].data_ptr(), p4.data_ptr(), stream=s4.cuda_stream)

    dt = timed(step, [s5, s4])
    e5.close()
    e4.close()
    return {"config": "configs[4] per GPU: 4096 V4 + 4096 V5 streams, two engines on two HIP streams",
            "us_per_step": dt * 1e6, "frames_per_s": 2 * B / dt, "x8_gpus_frames_per_s": 16 * B / dt}


def two_pools_one_gpu():
    """configs[2]'s 8 192 streams as TWO independent pools of 4 096 on one GPU (two engines, a HIP stream each; what
    ShardedStreamPool(devices=[0, 0]) gives a serving process): the pools' launches are not ordered against each other, so the
    start of one pool's launch - cold L2, state and first weights on their way - runs under the other pool's tiles."""
    B = 4096
    R = int(os.environ.get("VAD_BENCH_RING", "16"))
    ea, eb = Engine(blob(5), max_streams=B), Engine(blob(5), max_streams=B)
    ea.open_streams(B)
    eb.open_streams(B)
    ring = (0.1 * torch.randn(R, 2 * B, 512, device="cuda")).contiguous()
    pa, pb = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    fa = [ring[k, :B].data_ptr() for k in range(R)]        # pointers taken once: two tensor views per step would cost the host
    fb = [ring[k, B:].data_ptr() for k in range(R)]        # more than the launches it has to stay ahead of
    qa, qb, ha, hb = pa.data_ptr(), pb.data_ptr(), sa.cuda_stream, sb.cuda_stream

    def step(i):
        ea.step_device(B, fa[i % R], qa, stream=ha)
        eb.step_device(B, fb[i % R], qb, stream=hb)

    dt = timed(step, [sa, sb])
    one = Engine(blob(5), max_streams=2 * B)
    one.open_streams(2 * B)
    p1 = torch.empty(2 * B, device="cuda")
    q1 = p1.data_ptr()
    dt1 = timed(lambda i: one.step_device(2 * B, fa[i % R], q1, stream=ha), [sa])
    for e in (ea, eb, one):
        e.close()
    return {"config": "8192 V5 streams as two independent pools of 4096 on one GPU (two engines, two HIP streams)",
            "us_per_step": dt * 1e6, "frames_per_s": 2 * B / dt, "us_per_step_one_pool_of_8192": dt1 * 1e6,
            "frames_per_s_one_pool_of_8192": 2 * B / dt1}


def v4_alone():
    B = 8192
    eng = Engine(blob(4), model_version=4, max_streams=B)
    eng.open_streams(B)
    ring = (0.1 * torch.randn(16, B, 512, device="cuda")).contiguous()
    probs = torch.empty(B, device="cuda")
    ts = torch.cuda.Stream()
    dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
    eng.close()
    return {"config": "batch=8192, V4, 16 kHz (device-resident)", "us_per_step": dt * 1e6, "frames_per_s": B / dt,
            "frac_of_fp32_peak_at_1.38_MFLOP_per_frame": 1.38e6 * B / dt / 157.3e12}


def v4_tile_shapes():
    """V4 (both sub-models), device-resident, both tile shapes (vad_debug_set_tile): the 32-stream kernel with one wave per SIMD
    against 16-stream tiles, two workgroups per CU."""
    out = []
    for sr in (16000, 8000):
        for B in (256, 1024, 2048, 4096, 8192):
            eng = Engine(open(weights_io.packaged_blob_path(4, sr), "rb").read(), model_version=4, max_streams=B, sample_rate=sr)
            eng.open_streams(B)
            ring = (0.1 * torch.randn(16, B, 512, device="cuda")).contiguous()
            probs = torch.empty(B, device="cuda")
            ts = torch.cuda.Stream()
            row = {"config": f"batch={B}, V4 {sr} Hz sub-model, device-resident", "streams": B}
            for tile in (32, 16):
                eng.set_tile(tile)
                dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
                row[f"us_per_step_tile{tile}"] = dt * 1e6
                row[f"frames_per_s_tile{tile}"] = B / dt
            eng.close()
            out.append(row)
    return out


def resampler_alone():
    """vadk_resample_512 alone: 4096 chunks per launch, device-resident, per input rate."""
    B = 4096
    eng = Engine(blob(5), max_streams=64)
    out = []
    ts = torch.cuda.Stream()
    y = torch.empty(B, 512, device="cuda")
    for sr, n_in in ((8000, 256), (24000, 768), (48000, 1536)):
        x = (0.1 * torch.randn(4, B, n_in, device="cuda")).contiguous()
        lib = eng._lib

        def step(i):
            assert lib.vad_resample_device(eng.handle, x[i % 4].data_ptr(), B, n_in, sr, y.data_ptr(), ts.cuda_stream) == 0

        dt = timed(step, [ts])
        flop = 2.0 * 512 * n_in * B
        out.append({"config": f"resampler alone: {B} chunks of {n_in} samples ({sr} Hz) -> 512", "us_per_launch": dt * 1e6,
                    "chunks_per_s": B / dt, "TFLOP_s_dense_operator": flop / dt / 1e12,
                    "frac_of_fp32_peak": flop / dt / 157.3e12})
    eng.close()
    return out


def v4_8k():
    B = 8192
    eng = Engine(open(weights_io.packaged_blob_path(4, 8000), "rb").read(), model_version=4, max_streams=B,
                 sample_rate=8000)
    eng.open_streams(B)
    ring = (0.1 * torch.randn(16, B, 512, device="cuda")).contiguous()
    probs = torch.empty(B, device="cuda")
    ts = torch.cuda.Stream()
    dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
    eng.close()
    return {"config": "batch=8192, V4 8 kHz sub-model (a9; two LSTM steps per frame)", "us_per_step": dt * 1e6, "frames_per_s": B / dt}


def v5_8k():
    """Silero V5's 8 kHz sub-model: native 8 kHz audio in 256-sample frames (32 ms as well), 32-stream tiles."""
    B = 8192
    eng = Engine(open(weights_io.packaged_blob_path(5, 8000), "rb").read(), model_version=5, max_streams=B, sample_rate=8000)
    eng.open_streams(B)
    ring = (0.1 * torch.randn(16, B, 256, device="cuda")).contiguous()
    probs = torch.empty(B, device="cuda")
    ts = torch.cuda.Stream()
    dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
    eng.close()
    return {"config": "batch=8192, V5 8 kHz sub-model (256-sample frames)", "us_per_step": dt * 1e6, "frames_per_s": B / dt}


def v5_8k_tile_shapes():
    """Silero V5's 8 kHz sub-model on 16- against 32-stream tiles, 256 ... 8 192 streams (the engine picks 16-stream tiles up to 4 096)."""
    out = []
    eng = Engine(open(weights_io.packaged_blob_path(5, 8000), "rb").read(), model_version=5, max_streams=8192, sample_rate=8000)
    eng.open_streams(8192)
    ring = (0.1 * torch.randn(16, 8192, 256, device="cuda")).contiguous()
    probs = torch.empty(8192, device="cuda")
    ts = torch.cuda.Stream()
    for B in (256, 1024, 4096, 8192):
        row = {"config": f"batch={B}, V5 8 kHz sub-model, device-resident", "streams": B}
        for tile in (32, 16):
            eng.set_tile(tile)
            dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), stream=ts.cuda_stream), [ts])
            row[f"us_per_step_tile{tile}"] = dt * 1e6
            row[f"frames_per_s_tile{tile}"] = B / dt
        out.append(row)
    eng.close()
    return out


def int16_ingest():
    """Device-resident int16 frames (the wire format of the serving path) against float32 ones, V5 and V4, 8 192 streams."""
    from cutter_vad_amd import _ffi
    out = []
    B = 8192
    for v in (5, 4):
        eng = Engine(blob(v), model_version=v, max_streams=B)
        eng.open_streams(B)
        f32 = (0.1 * torch.randn(16, B, 512, device="cuda")).contiguous()
        i16 = (f32 * 32767.0).round().clamp(-32768, 32767).to(torch.int16).contiguous()
        probs = torch.empty(B, device="cuda")
        ts = torch.cuda.Stream()
        row = {"config": f"batch={B}, V{v}, device-resident frames, float32 vs int16 (/32767) ingest"}
        for name, ring, fmt in (("f32", f32, _ffi.VAD_FMT_F32), ("i16", i16, _ffi.VAD_FMT_I16_32767)):
            dt = timed(lambda i: eng.step_device(B, ring[i % 16].data_ptr(), probs.data_ptr(), fmt=fmt, stream=ts.cuda_stream), [ts])
            row[f"us_per_step_{name}"] = dt * 1e6
        eng.close()
        out.append(row)
    return out


def g711_ingest():
    """ITU-T G.711 frames (VAD_FMT_ULAW8 / VAD_FMT_ALAW8, one byte per sample) beside int16 and float32, Silero V5 16 kHz and 8 kHz:
    (1) vad_step on 8 192 streams from pageable and page-locked host memory (H2D + kernel + D2H + sync per step), (2) the
    pipelined submit / collect rate from page-locked memory, (3) the kernel alone on device-resident frames, 8 192 and 1 024
    streams (HIP events; VAD_BENCH_K=700 gives the 2 100 steps DESIGN 2.1c quotes).  The codes are uniform random bytes: the
    kernel's time does not depend on the values.  Every figure is the median of three repetitions, all three reported."""
    import time
    import numpy as np
    from cutter_vad_amd import _ffi
    B = 8192
    out = []
    for rate, fs in ((16000, 512), (8000, 256)):
        eng = Engine(open(weights_io.packaged_blob_path(5, rate), "rb").read(), model_version=5, max_streams=B, sample_rate=rate)
        slots = eng.open_streams(B)
        has_g711 = hasattr(_ffi, "VAD_FMT_ULAW8")             # the same entry runs on a checkout without the formats
        rng = np.random.default_rng(0)
        x32 = (0.1 * rng.standard_normal((4, B, fs))).astype(np.float32)
        x16 = np.clip(x32 * 32767.0, -32768, 32767).astype(np.int16)
        xu8 = rng.integers(0, 256, (4, B, fs), dtype=np.uint8)
        forms = [("f32", x32, {}), ("int16", x16, {})] + ([("ulaw", xu8, {"law": "ulaw"})] if has_g711 else [])
        for name, x, kw in forms:
            pin = eng.pinned_array(x.shape, x.dtype)
            pin[:] = x
            for where, buf in (("pageable", x), ("page-locked", pin)):
                for i in range(5):
                    eng.step(slots, buf[i % 4], **kw)
                reps = []
                for _ in range(3):                          # three repetitions: their spread is the run-to-run figure
                    t0 = time.perf_counter()
                    for i in range(40):
                        eng.step(slots, buf[i % 4], **kw)
                    reps.append((time.perf_counter() - t0) / 40)
                out.append({"config": f"g711_ingest: V5 {rate} Hz, batch={B}, vad_step from {where} host memory, {name} frames",
                            "us_per_step": float(np.median(reps)) * 1e6, "us_per_step_runs": [r * 1e6 for r in reps],
                            "bytes_per_step": int(x[0].nbytes)})
            t = [eng.submit(slots, pin[0], **kw)]
            for i in range(1, 10):
                t.append(eng.submit(slots, pin[i % 4], **kw))
                eng.collect(t.pop(0))
            reps = []
            for _ in range(3):
                t0 = time.perf_counter()
                for i in range(100):
                    t.append(eng.submit(slots, pin[i % 4], **kw))
                    eng.collect(t.pop(0))
                reps.append((time.perf_counter() - t0) / 100)
            eng.collect(t.pop(0))
            out.append({"config": f"g711_ingest: V5 {rate} Hz, batch={B}, pipelined submit / collect from page-locked memory, {name} frames",
                        "us_per_step": float(np.median(reps)) * 1e6, "us_per_step_runs": [r * 1e6 for r in reps],
                        "frames_per_s": B / float(np.median(reps))})
        # the kernel alone: device-resident frames
        i16 = torch.from_numpy(x16).cuda()
        u8 = torch.from_numpy(xu8).cuda()
        probs = torch.empty(B, device="cuda")
        ts = torch.cuda.Stream()
        dev = [("int16", i16, _ffi.VAD_FMT_I16_32768)]
        if has_g711:
            dev += [("ulaw", u8, _ffi.VAD_FMT_ULAW8), ("alaw", u8, _ffi.VAD_FMT_ALAW8)]
        for n in (B, 1024):
            row = {"config": f"g711_ingest: V5 {rate} Hz, batch={n}, device-resident frames, kernel time (HIP events, {3 * K} steps)"}
            for name, ring, fmt in dev:
                reps = [timed(lambda i: eng.step_device(n, ring[i % 4].data_ptr(), probs.data_ptr(), fmt=fmt, stream=ts.cuda_stream), [ts])
                        for _ in range(3)]
                row[f"us_per_step_{name}"] = float(np.median(reps)) * 1e6
                row[f"us_per_step_{name}_runs"] = [r * 1e6 for r in reps]
            out.append(row)
        eng.close()
    return out


def scan_ingest():
    """Whole recordings (vad_scan), two things on one box, interleaved, three runs each:
    (a) a corpus of int16 recordings of 5 - 30 s (seeded lengths; VAD_SCAN_BENCH_N of them, default 1 024) from page-locked host
        memory: Engine.scan against the route a caller had before it - AudioUtils.split_into_frames on the host to float32, then
        vad_step_multi on all streams, padded to the longest recording (in windows of T frames: one call addresses < 2 GiB);
    (b) the kernel alone: vad_scan_device against vad_step_multi_device at n = 1 024 / 4 096, T = 32, on the same pre-framed
        float32 audio in HBM (hop = frame, one length: only the addressing differs), HIP events around every call."""
    import time
    import numpy as np
    from cutter_vad_amd import _ffi
    from cutter_vad_amd.utils.audio import AudioUtils
    out = []
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    part = os.environ.get("VAD_SCAN_BENCH_PART", "ab")
    eng = Engine(blob(5), max_streams=4096)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    if "a" in part:
        rng = np.random.default_rng(0)
        lens = rng.integers(5 * 16000, 30 * 16000 + 1, N)
        offs = np.concatenate([[0], np.cumsum((lens[:-1] + 3) & ~3)])
        total = int(offs[-1] + lens[-1])
        block = eng.pinned_array(total, np.int16)
        block[:] = (2000.0 * rng.standard_normal(total)).astype(np.int16)
        recs = [block[o:o + n] for o, n in zip(offs, lens)]
        slots = eng.open_streams(N)
        counts = np.array([eng.scan_frame_count(int(n), hop) for n in lens])
        TW = max(1, min(int(counts.max()), ((1 << 31) - 1) // (N * frame * 4)))
        buf = np.zeros((N, TW, frame), np.float32)

        def route_scan():
            t0 = time.perf_counter()
            probs, _, _ = eng.scan(slots, recs, hop=hop)
            return time.perf_counter() - t0, sum(p.size for p in probs)

        def route_frames():
            t0 = time.perf_counter()
            framed = [AudioUtils.split_into_frames(r.astype(np.float32) / np.float32(32767.0), frame, hop) for r in recs]
            t_split = time.perf_counter() - t0
            for w0 in range(0, int(counts.max()), TW):
                tw = min(TW, int(counts.max()) - w0)
                buf[:, :tw] = 0
                for i, f in enumerate(framed):
                    k = max(0, min(tw, len(f) - w0))
                    buf[i, :k] = f[w0:w0 + k]
                eng.step_multi(slots, buf[:, :tw])
            return time.perf_counter() - t0, t_split

        route_scan()                                    # warm: buffers, code objects
        runs_scan, runs_frames, splits = [], [], []
        for _ in range(3):
            eng.reset(slots)
            dt, nf = route_scan()
            runs_scan.append(dt)
            eng.reset(slots)
            dt, ts = route_frames()
            runs_frames.append(dt)
            splits.append(ts)
        out.append({"config": f"scan_ingest (a): {N} int16 recordings of 5 - 30 s, page-locked host memory, hop = frame / 2",
                    "frames": int(counts.sum()), "frames_padded": int(N * counts.max()), "audio_MB": total * 2 / 1e6,
                    "framed_float32_MB_padded": N * int(counts.max()) * frame * 4 / 1e6,
                    "s_scan_runs": runs_scan, "s_split_then_step_multi_runs": runs_frames, "s_of_that_host_split_runs": splits,
                    "s_scan": float(np.median(runs_scan)), "s_split_then_step_multi": float(np.median(runs_frames)),
                    "ratio": float(np.median(runs_frames) / np.median(runs_scan))})
        for s in slots:
            eng.close_stream(int(s))
        del buf
    if "b" in part:
        T = 32
        for n in (1024, 4096):
            slots = eng.open_streams(n)
            d_slots = torch.from_numpy(np.asarray(slots, np.int32)).cuda()
            x = (0.1 * torch.randn(n, T, frame, device="cuda")).contiguous()
            d_p = torch.empty(n * T, device="cuda")
            d_e = torch.empty(n * T, dtype=torch.uint8, device="cuda")
            d_s = torch.empty(n * T, dtype=torch.int32, device="cuda")
            ts = torch.cuda.Stream()
            offsets, lengths = np.arange(n, dtype=np.int64) * T * frame, np.full(n, T * frame, np.int64)

            def one(scan):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(ts)
                if scan:
                    eng.scan_device(slots, offsets, lengths, x.data_ptr(), n * T * frame, d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(),
                                    hop=frame, fmt=_ffi.VAD_FMT_F32, stream=ts.cuda_stream)
                else:
                    eng.step_multi_device(n, T, x.data_ptr(), d_p.data_ptr(), d_slots.data_ptr(), d_e.data_ptr(), d_s[:n].data_ptr(),
                                          stream=ts.cuda_stream)
                e1.record(ts)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e-3

            for _ in range(5):
                one(True), one(False)
            reps = max(10, K // 20)
            row = {"config": f"scan_ingest (b): kernel alone, n={n}, T={T}, float32 in HBM, hop = frame; median of {reps} calls per run"}
            runs = {"scan": [], "step_multi": []}
            for _ in range(3):
                a, b = [], []
                for _ in range(reps):
                    a.append(one(True))
                    b.append(one(False))
                runs["scan"].append(float(np.median(a)))
                runs["step_multi"].append(float(np.median(b)))
            for k, v in runs.items():
                row[f"us_per_call_{k}_runs"] = [r * 1e6 for r in v]
                row[f"us_per_frame_{k}"] = float(np.median(v)) * 1e6 / T
            row["scan_over_step_multi"] = float(np.median(runs["scan"]) / np.median(runs["step_multi"]))
            out.append(row)
            eng.synchronize()
            for s in slots:
                eng.close_stream(int(s))
    eng.close()
    return out


def scan_stereo():
    """Two-channel recordings (vad_scan_channels), interleaved runs, three each:
    (a) the kernel alone, audio resident in HBM: vad_scan_channels_device in split mode (both channels of every recording, 2 n
        streams) on n = 512 and 2 048 interleaved int16 recordings against vad_scan_device on the 2 n mono recordings a host
        gets by de-interleaving them - the same samples, the same streams in the same order; HIP events around every call, after
        warm-up calls that are scans themselves.  Lengths are seeded, 5 - 30 s at n = 512; at n = 2 048 5 - 20 s, so that the
        block (4 bytes per sample frame) stays under the 2 GiB one call addresses;
    (b) host-inclusive, n = 512 from page-locked memory: Engine.scan(channel="split") against numpy's de-interleave (one
        strided copy per channel and recording) followed by Engine.scan."""
    import time
    import numpy as np
    from cutter_vad_amd import _ffi
    out = []
    eng = Engine(blob(5), max_streams=4096)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    for n, longest in ((512, 30), (2048, 20)):
        rng = np.random.default_rng(n)
        lens = rng.integers(5 * 16000, longest * 16000 + 1, n)
        pad = (lens + 3) & ~3
        offs = np.concatenate([[0], np.cumsum(pad[:-1])])
        total = int(offs[-1] + lens[-1])
        assert total * 4 < (1 << 31)
        block = eng.pinned_array((total, 2), np.int16) if n == 512 else np.empty((total, 2), np.int16)
        for o in range(0, total, 1 << 24):
            block[o:o + (1 << 24)] = (2000.0 * rng.standard_normal((min(1 << 24, total - o), 2))).astype(np.int16)
        recs = [block[o:o + k] for o, k in zip(offs, lens)]
        # the host's de-interleave: left and right of recording i one after the other, each on a multiple of 4 samples
        moffs = np.concatenate([[0], np.cumsum(np.repeat(pad, 2))[:-1]])
        mono = np.zeros(int(moffs[-1] + lens[-1]), np.int16)
        for i, r in enumerate(recs):
            for c in range(2):
                mono[moffs[2 * i + c]:moffs[2 * i + c] + lens[i]] = r[:, c]
        slots = eng.open_streams(2 * n)
        counts = np.array([eng.scan_frame_count(int(k), hop) for k in lens])
        nf = 2 * int(counts.sum())
        d_st, d_mo = torch.from_numpy(block).cuda(), torch.from_numpy(mono).cuda()
        d_p = torch.empty(nf, device="cuda")
        d_e = torch.empty(nf, dtype=torch.uint8, device="cuda")
        d_s = torch.empty(nf, dtype=torch.int32, device="cuda")
        ts = torch.cuda.Stream()
        st_off, st_len, st_ch = np.repeat(offs, 2), np.repeat(lens, 2), [0, 1] * n

        def one(stereo):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(ts)
            if stereo:
                eng.scan_device(slots, st_off, st_len, d_st.data_ptr(), total, d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), hop=hop,
                                fmt=_ffi.VAD_FMT_I16_32767, stream=ts.cuda_stream, channels=2, channel=st_ch)
            else:
                eng.scan_device(slots, moffs, st_len, d_mo.data_ptr(), mono.size, d_p.data_ptr(), d_e.data_ptr(), d_s.data_ptr(), hop=hop,
                                fmt=_ffi.VAD_FMT_I16_32767, stream=ts.cuda_stream)
            e1.record(ts)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        for _ in range(2):
            one(True), one(False)
        runs = {"channels_split": [], "mono_deinterleaved": []}
        for _ in range(3):
            runs["channels_split"].append(one(True))
            runs["mono_deinterleaved"].append(one(False))
        row = {"config": f"scan_stereo (a): kernel alone, {n} interleaved int16 recordings of 5 - {longest} s in HBM = {2 * n} streams, hop = frame / 2",
               "frames": nf, "launches_per_call": -(-int(counts.max()) // 192), "audio_MB": total * 4 / 1e6}
        for k, v in runs.items():
            row[f"ms_{k}_runs"] = [r * 1e3 for r in v]
            row[f"ms_{k}"] = float(np.median(v)) * 1e3
            row[f"us_per_launched_frame_{k}"] = float(np.median(v)) * 1e6 / int(counts.max())
        row["spread_mono_pct"] = 100.0 * (max(runs["mono_deinterleaved"]) - min(runs["mono_deinterleaved"])) / float(np.median(runs["mono_deinterleaved"]))
        row["channels_over_mono"] = float(np.median(runs["channels_split"]) / np.median(runs["mono_deinterleaved"]))
        out.append(row)
        del d_st, d_mo
        if n == 512:
            sl2 = np.asarray(slots).reshape(n, 2)

            def route_split():
                t0 = time.perf_counter()
                probs, _, _ = eng.scan(sl2, recs, hop=hop, channel="split")
                return time.perf_counter() - t0, 0.0

            def route_deinterleave():
                t0 = time.perf_counter()
                chans = [np.ascontiguousarray(r[:, c]) for r in recs for c in range(2)]
                t_copy = time.perf_counter() - t0
                eng.scan(slots, chans, hop=hop)
                return time.perf_counter() - t0, t_copy

            route_split(), route_deinterleave()         # warm: the engine's page-locked block grows to its size
            a, b, copies = [], [], []
            for _ in range(3):
                eng.reset(slots)
                a.append(route_split()[0])
                eng.reset(slots)
                dt, tc = route_deinterleave()
                b.append(dt)
                copies.append(tc)
            out.append({"config": f"scan_stereo (b): host-inclusive, {n} interleaved int16 recordings of 5 - {longest} s, page-locked host memory",
                        "frames": nf, "audio_MB": total * 4 / 1e6, "s_scan_split_runs": a, "s_deinterleave_then_scan_runs": b,
                        "s_of_that_strided_copies_runs": copies, "s_scan_split": float(np.median(a)),
                        "s_deinterleave_then_scan": float(np.median(b)), "ratio": float(np.median(b) / np.median(a))})
        eng.synchronize()
        for s in slots:
            eng.close_stream(int(s))
        torch.cuda.empty_cache()
    eng.close()
    return out


def scan_cut():
    """Finished segments' audio (vad_scan_cut):
    (a) the kernel alone, HIP events: 2 048 int16 recordings of 5 - 20 s in HBM, synthetic segments of 1 - 3 s that cover about half
        of every recording, FRAMES layout at hop = frame / 2, PCM16 out.  The kernel is launched through the library's own
        launcher (vadk_launch_scan_cut) on tables that already lie in device memory - built here as the engine builds them, and
        the payload is compared with vad_scan_cut_device's - against hipMemcpyAsync device-to-device of the payload's byte count
        in the same run (it reads and writes what the kernel gathers and writes: the yardstick, no code of the project).  The
        whole call, vad_scan_cut_device with the upload of its tables, is timed beside them;
    (b) host-inclusive: cut_recordings (interleaved int16 speech, mix, page-locked memory) against the same build's
        scan_recordings followed by the numpy pass that produces the same bytes; runs interleaved, three each after two warm-ups."""
    import ctypes as C
    import time
    import numpy as np
    from cutter_vad_amd import VADConfig, _ffi, cut_recordings, scan_recordings
    from cutter_vad_amd.utils.wav_writer import WAVWriter
    out = []
    eng = Engine(blob(5), max_streams=4096)
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n = 2048
    rng = np.random.default_rng(n)
    lens = rng.integers(5 * 16000, 20 * 16000 + 1, n)
    offs = np.concatenate([[0], np.cumsum((lens[:-1] + 3) & ~3)])
    total = int(offs[-1] + lens[-1])
    d_audio = torch.randint(-3000, 3000, (total,), dtype=torch.int16, device="cuda")
    segs = []
    for o, k in zip(offs, lens):
        nf, t = (int(k) - frame) // hop + 1, 0
        while True:
            L = int(rng.integers(16000 // hop, 3 * 16000 // hop))       # speech of 1 - 3 s, then as much silence
            if t + L > nf:
                break
            segs.append((int(o), t, L))
            t += 2 * L
    out_samples = sum(L for _, _, L in segs) * frame
    d_out = torch.empty(out_samples, dtype=torch.int16, device="cuda")
    d_copy = torch.empty(out_samples, dtype=torch.int16, device="cuda")
    ts = torch.cuda.Stream()

    # the call builds its tables on the host and uploads them before the launch.  A matrix product on the same stream in front of
    # the first event keeps the GPU busy meanwhile, so the events bracket the table's upload (16 bytes per segment, 8 per
    # workgroup) and the kernel, not the host's loop; the ctypes items are built once, outside
    items, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_FRAMES, 1)
    busy = torch.randn(6144, 6144, device="cuda")

    # the same tables as the engine's (vad_layout.h: CutSeg, CutWork, CutArgs), in device memory before the clock starts
    wgq = _ffi.VAD_CUT_WG_SAMPLES // 4
    seg_t = np.zeros(len(segs), np.dtype([("quad_in", "<u4"), ("nquads", "<u4"), ("quad_out", "<u8")]))
    work, o = [], 0
    for i, (off, first, L) in enumerate(segs):
        seg_t[i] = ((off + first * hop) // 4, L * frame // 4, o // 4)
        work += [(i, q) for q in range(0, L * frame // 4, wgq)]
        o += L * frame
    work_t = np.array(work, np.uint32)
    d_seg, d_work = torch.from_numpy(seg_t.view(np.uint8)).cuda(), torch.from_numpy(work_t.view(np.uint8).reshape(-1)).cuda()
    d_out2 = torch.zeros(out_samples, dtype=torch.int16, device="cuda")

    class CutArgs(C.Structure):
        _fields_ = [("audio", C.c_void_p), ("out", C.c_void_p), ("segs", C.c_void_p), ("work", C.c_void_p), ("audio_bytes", C.c_uint32),
                    ("nwork", C.c_uint32), ("hopq", C.c_uint32), ("frame_shift", C.c_uint32), ("fmt", C.c_int32), ("channels", C.c_int32),
                    ("out_fmt", C.c_int32), ("thresh", C.c_float)]

    args = CutArgs(d_audio.data_ptr(), d_out2.data_ptr(), d_seg.data_ptr(), d_work.data_ptr(), 2 * total, len(work), hop // 4,
                   (frame // 4).bit_length() - 1, _ffi.VAD_FMT_I16_32767, 1, _ffi.VAD_CUT_PCM16, 0.01)
    launch = eng._lib.vadk_launch_scan_cut
    launch.argtypes, launch.restype = [C.POINTER(CutArgs), C.c_void_p], C.c_int

    def one(kind):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            torch.mm(busy, busy)
        e0.record(ts)
        if kind == "kernel":
            assert launch(C.byref(args), ts.cuda_stream) == 0
        elif kind == "call":
            rc = eng._lib.vad_scan_cut_device(eng.handle, items, len(segs), d_audio.data_ptr(), total, 1, _ffi.VAD_FMT_I16_32767, hop, 0.01,
                                              _ffi.VAD_CUT_FRAMES, _ffi.VAD_CUT_PCM16, d_out.data_ptr(), out_samples, ts.cuda_stream)
            assert rc == 0, rc
        else:
            assert hip.hipMemcpyAsync(d_copy.data_ptr(), d_out.data_ptr(), 2 * out_samples, 3, ts.cuda_stream) == 0
        e1.record(ts)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    kinds = ("kernel", "call", "memcpy_d2d")
    for _ in range(2):
        for k in kinds:
            one(k)
    assert torch.equal(d_out, d_out2), "the launcher on the tables built here must write the call's payload"
    runs = {k: [] for k in kinds}
    for _ in range(3):
        for k in kinds:
            runs[k].append(one(k))
    moved = 4.0 * out_samples                                           # int16 gathered + int16 written
    row = {"config": f"scan_cut (a): kernel alone (kernel), and vad_scan_cut_device with the upload of its tables (call), {n} int16 recordings of 5 - 20 s in HBM, {len(segs)} segments over "
                     "about half of every recording, FRAMES at hop = frame / 2, PCM16 out",
           "segments": len(segs), "audio_MB": total * 2 / 1e6, "payload_MB": out_samples * 2 / 1e6,
           "workgroups": sum(-(-L * frame // _ffi.VAD_CUT_WG_SAMPLES) for _, _, L in segs)}
    row["table_MB"] = (16 * len(segs) + 8 * row["workgroups"]) / 1e6
    for k, v in runs.items():
        row[f"ms_{k}_runs"] = [r * 1e3 for r in v]
        row[f"ms_{k}"] = float(np.median(v)) * 1e3
        row[f"GBps_{k}"] = moved / float(np.median(v)) / 1e9
    row["spread_memcpy_pct"] = 100.0 * (max(runs["memcpy_d2d"]) - min(runs["memcpy_d2d"])) / float(np.median(runs["memcpy_d2d"]))
    row["kernel_rate_over_memcpy_rate"] = float(np.median(runs["memcpy_d2d"]) / np.median(runs["kernel"]))
    row["call_rate_over_memcpy_rate"] = float(np.median(runs["memcpy_d2d"]) / np.median(runs["call"]))
    out.append(row)
    del d_audio, d_out, d_out2, d_copy
    torch.cuda.empty_cache()

    # (b) speech, so that the scan finds segments: the golden clip against itself 3 s later, cut at seeded places
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.load(gold)["pcm"].astype(np.int16)
    pair = np.stack([pcm, np.roll(pcm, 3 * 16000)], axis=1)
    m = 256
    rng = np.random.default_rng(m)
    lens = rng.integers(5 * 16000, min(30 * 16000, pcm.size) + 1, m)
    pad = (lens + 3) & ~3
    offs = np.concatenate([[0], np.cumsum(pad[:-1])])
    block = eng.pinned_array((int(offs[-1] + lens[-1]), 2), np.int16)
    for o, k in zip(offs, lens):
        a = int(rng.integers(0, pcm.size - int(k) + 1))
        block[o:o + k] = pair[a:a + k]
    recs = [block[o:o + k] for o, k in zip(offs, lens)]
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    writer = WAVWriter(cfg.output_wav_sample_rate, 16, 1)

    def route_cut():
        t0 = time.perf_counter()
        got = cut_recordings(recs, cfg, engine=eng)
        return time.perf_counter() - t0, got

    def route_numpy():
        t0 = time.perf_counter()
        got = []
        for x, sg in zip(recs, scan_recordings(recs, cfg, engine=eng)):
            one_rec = []
            for a, b in sg:
                v = np.mean(x[a:b].astype(np.float32) / np.float32(32767.0), axis=1)
                v = np.where(np.abs(v) > np.float32(0.01), v, np.float32(0.0)).astype(np.float32)
                fr = np.concatenate([v[t:t + frame] for t in range(0, b - a - frame + 1, hop)])
                one_rec.append((a, b, writer.write_wav_data(fr)))
            got.append(one_rec)
        return time.perf_counter() - t0, got

    (_, g1), (_, g2) = route_cut(), route_numpy()
    assert g1 == g2, "the two routes must produce the same bytes"
    route_cut(), route_numpy()
    a, b = [], []
    for _ in range(3):
        a.append(route_cut()[0])
        b.append(route_numpy()[0])
    nseg = sum(len(g) for g in g1)
    out.append({"config": f"scan_cut (b): host-inclusive, {m} interleaved int16 recordings of 5 - 30 s of speech (mix), page-locked host memory, "
                          "client thresholds", "segments": nseg, "audio_MB": block.nbytes / 1e6,
                "payload_MB": sum(len(w) - 44 for g in g1 for _, _, w in g) / 1e6, "s_cut_recordings_runs": a,
                "s_scan_recordings_then_numpy_runs": b, "s_cut_recordings": float(np.median(a)),
                "s_scan_recordings_then_numpy": float(np.median(b)), "spread_cut_pct": 100.0 * (max(a) - min(a)) / float(np.median(a)),
                "ratio": float(np.median(b) / np.median(a))})
    eng.close()
    return out


def scan_segments():
    """The corpus path end to end: scan_recordings and cut_recordings on VAD_SCAN_BENCH_N (default 1 024) int16
    recordings of 5 - 30 s of speech - the golden clip, repeated, cut at seeded places - from page-locked host memory, client
    thresholds, hop = frame / 2; one warm-up, then three timed calls of each, the median reported.  The functions are the public
    ones, so the same code times a checkout without Engine.scan_segments (VAD_BENCH_TREE = its path): run the two trees in
    turn, three processes each, and compare the medians against the spread of the older tree's three.  The bytes copied back
    per scan are arithmetic on the counts: 9 per frame (probs, events, seg_frames) on the per-frame path, 8 + 24 per segment
    on the table's."""
    import time
    import numpy as np
    import cutter_vad_amd
    from cutter_vad_amd import VADConfig, cut_recordings, scan_recordings
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.tile(np.load(gold)["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    lens = rng.integers(5 * 16000, 30 * 16000 + 1, N)
    recs = []
    for k in lens:
        a = int(rng.integers(0, pcm.size - int(k) + 1))
        recs.append(pcm[a:a + int(k)].copy())
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    runs = {"scan_recordings": [], "cut_recordings": []}
    segs = scan_recordings(recs, cfg, engine=eng)
    cuts = cut_recordings(recs, cfg, engine=eng)
    assert [[c[:2] for c in r] for r in cuts] == segs
    for _ in range(3):
        t0 = time.perf_counter()
        scan_recordings(recs, cfg, engine=eng)
        runs["scan_recordings"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        cut_recordings(recs, cfg, engine=eng)
        runs["cut_recordings"].append(time.perf_counter() - t0)
    frames = int(sum(eng.scan_frame_count(int(k), hop) for k in lens))
    nseg = sum(len(r) for r in segs)
    table = hasattr(eng, "scan_segments")
    row = {"config": f"scan_segments: scan_recordings and cut_recordings, {N} int16 recordings of 5 - 30 s of speech in host memory, "
                     "client thresholds, hop = frame / 2", "tree": os.path.dirname(os.path.dirname(os.path.abspath(cutter_vad_amd.__file__))),
           "path": "segment table built on the GPU" if table else "per-frame results reduced on the host",
           "recordings": N, "frames": frames, "segments": nseg, "audio_MB": float(lens.sum()) * 2 / 1e6,
           "d2h_bytes_per_scan": 8 + 24 * nseg if table else 9 * frames,
           "payload_MB_per_cut": sum(len(w) - 44 for r in cuts for _, _, w in r) / 1e6}
    for k, v in runs.items():
        row[f"s_{k}_runs"] = v
        row[f"s_{k}"] = float(np.median(v))
    eng.close()
    return row


def scan_resegment():
    """A threshold sweep over an archive: VAD_SCAN_BENCH_N (default 1 024) int16 recordings of 30 s at 16 kHz in one call,
    hop 256.  (a) Engine.scan_segments once, then Engine.resegment with 1, 8 and 64 threshold sets - the replay of the probabilities
    the scan left on the GPU; (b) the way to the same tables without it: per set, the streams reset, the thresholds set and a full
    Engine.scan_segments; (c) Engine.resegment_device alone on synthetic probabilities, ONE recording of 112 500 frames (an hour at
    hop 512) under 64 sets, next to one default launch window of a scan (192 frames of the N recordings, Engine.scan_device on
    device memory), HIP-event timed.  One warm-up, then three timed passes of each; medians, wall clock for (a) and (b)."""
    import time
    import numpy as np
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    frame, hop = eng.frame_samples, 256
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.tile(np.load(gold)["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    base = [(0.4, 0.3, 0.8, 0.95, 6, 12), (0.7, 0.7, 0.8, 0.95, 10, 50), (0.3, 0.2, 0.8, 0.95, 2, 2), (0.5, 0.35, 0.6, 0.9, 4, 57),
            (0.85, 0.6, 0.5, 0.75, 3, 8)]
    sets = [(a - 0.004 * (k // 5), b - 0.003 * (k // 5), c, d, m + (k // 5) % 3, n + (k // 5) % 4) for k in range(64) for a, b, c, d, m, n in [base[k % 5]]]
    slots = eng.open_streams(N)
    med = lambda v: float(np.median(v))
    note = lambda what: print(f"scan_resegment: {what}", file=sys.stderr, flush=True)      # a pass of (b) takes a while

    def full_scan(thr):
        eng.reset(slots)
        eng.set_thresholds_many(slots, thr)
        return eng.scan_segments(slots, recs, hop=hop, denoise=0.01)

    row = {"config": f"scan_resegment: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}", "recordings": N,
           "frames": N * eng.scan_frame_count(ns, hop), "passes": 3}
    with eng.scan_session():
        first = full_scan(sets[0])                       # the warm-up of both paths
        assert np.array_equal(eng.resegment(sets[:1])[0], first)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            full_scan(sets[0])
            runs.append(time.perf_counter() - t0)
        row["a_s_scan_segments_runs"], row["a_s_scan_segments"] = runs, med(runs)
        note(f"scan_segments {runs}")
        for nt in (1, 8, 64):
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                tables = eng.resegment(sets[:nt])
                runs.append(time.perf_counter() - t0)
            row[f"a_s_resegment_nt{nt}_runs"], row[f"a_s_resegment_nt{nt}"] = runs, med(runs)
            row[f"records_nt{nt}"] = int(sum(len(t) for t in tables))
            note(f"resegment nt = {nt} {runs}")
        for nt in (1, 8, 64):
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                for thr in sets[:nt]:
                    full_scan(thr)
                runs.append(time.perf_counter() - t0)
                note(f"full scans nt = {nt} {runs[-1]:.3f} s")
            row[f"b_s_full_scans_nt{nt}_runs"], row[f"b_s_full_scans_nt{nt}"] = runs, med(runs)
            row[f"ratio_b_over_a_nt{nt}"] = row[f"b_s_full_scans_nt{nt}"] / (row["a_s_scan_segments"] + row[f"a_s_resegment_nt{nt}"])
    # (c) device pointers, no model: one long recording under 64 sets, and one launch window of a scan for scale
    T = 112500
    run = rng.integers(1, 40, T)
    p, k, speech = np.empty(T, np.float32), 0, False
    while k < T:
        r = int(run[k])
        p[k:k + r] = rng.uniform(0.5, 0.95, min(r, T - k)) if speech else rng.uniform(0.0, 0.45, min(r, T - k))
        k, speech = k + r, not speech
    d_p = torch.from_numpy(p).cuda()
    d_ev = torch.zeros(T, dtype=torch.uint8, device="cuda")
    d_tab = torch.zeros(24 * (1 << 20), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(65, dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()

    def event_timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            fn()
            e1.record(ts)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    runs = event_timed(lambda: eng.resegment_device(d_ev.data_ptr(), d_p.data_ptr(), [0, T], sets, d_tab.data_ptr(), 1 << 20, d_cnt.data_ptr(),
                                                    stream=ts.cuda_stream))
    row["c_s_resegment_device_1x112500_nt64_runs"], row["c_s_resegment_device_1x112500_nt64"] = runs, med(runs)
    row["c_records"] = int(d_cnt.cpu()[64])
    win = frame + 191 * hop
    d_audio = torch.from_numpy(np.concatenate([r[:win] for r in recs])).cuda()
    d_probs = torch.zeros(N * 192, dtype=torch.float32, device="cuda")
    d_events = torch.zeros(N * 192, dtype=torch.uint8, device="cuda")
    offs, lens = np.arange(N) * win, np.full(N, win)
    runs = event_timed(lambda: eng.scan_device(slots, offs, lens, d_audio.data_ptr(), N * win, d_probs.data_ptr(), d_events.data_ptr(), hop=hop,
                                               fmt=1, stream=ts.cuda_stream))
    row["c_s_scan_window_192_frames_runs"], row["c_s_scan_window_192_frames"] = runs, med(runs)
    row["ratio_c_replay_over_window"] = row["c_s_resegment_device_1x112500_nt64"] / row["c_s_scan_window_192_frames"]
    eng.close()
    return row


def scan_tails():
    """What the tails cost, on scan_resegment's corpus: VAD_SCAN_BENCH_N (default 1 024) int16 recordings of 30 s at
    16 kHz in one call, hop 256.  Engine.scan_segments - with VAD_BENCH_TREE set to a checkout of the parent commit the same lines
    time the scan without the snapshot launch; the difference is that launch - then, where the engine has them, Engine.scan_tails and
    Engine.resegment_tails with 1 and 64 sets.  One warm-up, then three timed passes of each in one process; wall clock, medians."""
    import time
    import numpy as np
    import cutter_vad_amd
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop = 256
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.tile(np.load(gold)["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    base = [(0.4, 0.3, 0.8, 0.95, 6, 12), (0.7, 0.7, 0.8, 0.95, 10, 50), (0.3, 0.2, 0.8, 0.95, 2, 2), (0.5, 0.35, 0.6, 0.9, 4, 57),
            (0.85, 0.6, 0.5, 0.75, 3, 8)]
    sets = [(a - 0.004 * (k // 5), b - 0.003 * (k // 5), c, d, m + (k // 5) % 3, n + (k // 5) % 4) for k in range(64) for a, b, c, d, m, n in [base[k % 5]]]
    slots = eng.open_streams(N)
    med = lambda v: float(np.median(v))

    def passes(fn):
        fn()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn()
            runs.append(time.perf_counter() - t0)
        return runs, out

    def full_scan():
        eng.reset(slots)
        eng.set_thresholds_many(slots, sets[1])
        return eng.scan_segments(slots, recs, hop=hop, denoise=0.01)

    row = {"config": f"scan_tails: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, the default thresholds",
           "tree": os.path.dirname(os.path.dirname(os.path.abspath(cutter_vad_amd.__file__))), "recordings": N,
           "frames": N * eng.scan_frame_count(ns, hop), "passes": 3}
    with eng.scan_session():
        runs, table = passes(full_scan)
        row["s_scan_segments_runs"], row["s_scan_segments"], row["records"] = runs, med(runs), int(len(table))
        row["s_scan_segments_spread"] = max(runs) - min(runs)
        if hasattr(eng, "scan_tails"):
            runs, tails = passes(eng.scan_tails)
            row["s_scan_tails_runs"], row["s_scan_tails"], row["tails"] = runs, med(runs), int((tails["nframes"] > 0).sum())
            for nt in (1, 64):
                runs, per_set = passes(lambda: eng.resegment_tails(sets[:nt]))
                row[f"s_resegment_tails_nt{nt}_runs"], row[f"s_resegment_tails_nt{nt}"] = runs, med(runs)
                row[f"tails_nt{nt}"] = int(sum((t["nframes"] > 0).sum() for t in per_set))
    eng.close()
    return row


def scan_refine():
    """What the refinement costs, on scan_resegment's corpus: VAD_SCAN_BENCH_N (default 1 024) int16 recordings of 30 s at
    16 kHz in one call, hop 256.  (a) Engine.scan_segments, then Engine.refine on the table and the tails that scan left on the GPU,
    under a pad + merge + 30 s split rule (no recording is longer, so nothing is split) and under a rule whose pads share gaps, which
    drops blips and splits at 1 s, so that every step and the cut search run;
    (b) the way to the same records today: Engine.scan, which copies the per-frame results back, then the numpy reference
    (tests/refine_ref.py) on the same table and tails - its records are compared with (a)'s; (c) Engine.refine_device alone on
    synthetic per-frame arrays: ONE recording of 1 125 000 frames (10 hours at hop 512) with the segments its alternating runs give,
    HIP-event timed - the count and fill walks are one thread for it.  One warm-up, then three timed passes of each; medians."""
    import time
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cutter_vad_amd import SegmentRefine
    from tests import refine_ref
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop = 256
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.tile(np.load(gold)["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    thr = (0.4, 0.3, 0.8, 0.95, 6, 12)
    rules = {"30s": SegmentRefine.from_durations(hop, 16000, pad_ms=100, merge_gap_ms=300, max_speech_s=30),
             "1s": SegmentRefine.from_durations(hop, 16000, pad_ms=200, merge_gap_ms=100, min_speech_ms=250, max_speech_s=1)}
    slots = eng.open_streams(N)
    med = lambda v: float(np.median(v))

    def passes(fn):
        fn()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn()
            runs.append(time.perf_counter() - t0)
        return runs, out

    def fresh():
        eng.reset(slots)
        eng.set_thresholds_many(slots, thr)

    row = {"config": f"scan_refine: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}", "recordings": N,
           "frames": N * eng.scan_frame_count(ns, hop), "passes": 3, "rules": {k: list(refine_ref.rule_of(v)) for k, v in rules.items()}}
    with eng.scan_session():
        runs, per_frame = passes(lambda: (fresh(), eng.scan(slots, recs, hop=hop, denoise=0.01))[1])
        row["b_s_scan_per_frame_runs"], row["b_s_scan_per_frame"] = runs, med(runs)
        probs, ev, _ = per_frame
        start = np.concatenate([[0], np.cumsum([len(p) for p in probs])]).astype(np.int64)
        flat_p, flat_e = np.concatenate(probs).astype(np.float32), np.concatenate(ev).astype(np.uint8)
        runs, table = passes(lambda: (fresh(), eng.scan_segments(slots, recs, hop=hop, denoise=0.01))[1])
        row["a_s_scan_segments_runs"], row["a_s_scan_segments"], row["records_in"] = runs, med(runs), int(len(table))
        tails = eng.scan_tails()
        row["tails_in"] = int((tails["nframes"] > 0).sum())
        for name, rule in rules.items():
            runs, fine = passes(lambda: eng.refine(rule, None, tails))
            row[f"a_s_refine_{name}_runs"], row[f"a_s_refine_{name}"], row[f"records_{name}"] = runs, med(runs), int(len(fine))
            t0 = time.perf_counter()
            want = refine_ref.refine(table, tails, flat_e, flat_p, start, rule)
            row[f"b_s_numpy_refine_{name}"] = time.perf_counter() - t0
            row[f"equal_{name}"] = bool(refine_ref.same(np.ascontiguousarray(fine), want))
            row[f"census_{name}"] = refine_ref.census(table, tails, start, rule)
            row[f"ratio_b_over_a_{name}"] = (row["b_s_scan_per_frame"] + row[f"b_s_numpy_refine_{name}"]) / (row["a_s_scan_segments"] + row[f"a_s_refine_{name}"])
    # (c) device pointers, no model: one recording of 10 hours
    T = 1125000
    run = rng.integers(1, 40, T)
    p, k, speech, rows = np.empty(T, np.float32), 0, False, []
    while k < T:
        r = min(int(run[k]), T - k)
        p[k:k + r] = rng.uniform(0.5, 0.95, r) if speech else rng.uniform(0.0, 0.45, r)
        if speech:
            rows.append((0, k, r, 0, 0.0, 0.0))
        k, speech = k + r, not speech
    tab = np.array(rows, refine_ref.DTYPE)
    d_p = torch.from_numpy(p).cuda()
    d_ev = torch.zeros(T, dtype=torch.uint8, device="cuda")
    d_in = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    d_nin = torch.tensor([len(tab)], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(24 * (1 << 18), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()
    rule = SegmentRefine(6, 6, 19, 16, 938)              # the 30 s rule at hop 512

    def event_timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            fn()
            e1.record(ts)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    runs = event_timed(lambda: eng.refine_device(d_in.data_ptr(), d_nin.data_ptr(), len(tab), 0, d_ev.data_ptr(), d_p.data_ptr(), [0, T], rule,
                                                 d_out.data_ptr(), 1 << 18, d_cnt.data_ptr(), stream=ts.cuda_stream))
    row["c_s_refine_device_1x1125000_runs"], row["c_s_refine_device_1x1125000"] = runs, med(runs)
    row["c_records_in"], row["c_records"] = int(len(tab)), int(d_cnt.cpu()[0])
    got = d_out.cpu().numpy()[:24 * row["c_records"]].view(refine_ref.DTYPE)
    row["c_equal"] = bool(refine_ref.same(np.ascontiguousarray(got), refine_ref.refine(tab, None, np.zeros(T, np.uint8), p, [0, T], rule)))
    eng.close()
    return row


def scan_levels():
    """What segment levels and gained cuts cost, on scan_refine's corpus: VAD_SCAN_BENCH_N (default 1 024) int16
    recordings of 30 s at 16 kHz, hop 256, the table of its scan.  (a) Engine.levels on the block the scan left on the GPU;
    (b) the way to the same numbers without it: Engine.cut(layout="range", out="f32") of the same table, then the statistics in numpy
    (tests/levels_ref.py) - its records are compared with (a)'s; (a) and (b) alternate; (c) on device pointers, HIP-event timed, the
    same table: vad_scan_levels_device against vad_scan_cut_device(RANGE, F32), which reads the same bytes and writes 4 per sample -
    the traffic yardstick; (d) the cut with a gain per segment against the cut without, host calls and device forms (frames, PCM16).
    One warm-up, then three timed passes of each; medians."""
    import ctypes as C
    import time
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cutter_vad_amd import level_stats
    from tests import levels_ref
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, frame = 256, 512
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.tile(np.load(gold)["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    med = lambda v: float(np.median(v))
    row = {"config": f"scan_levels: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}", "recordings": N, "passes": 3}
    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        last = eng.last_scan
        offs = [int(o) for o in last["offsets"]]
        segs = [(offs[i], f, n) for i, f, n in zip(table["item"].tolist(), table["first_frame"].tolist(), table["nframes"].tolist())]
        counts = np.array([(n - 1) * hop + frame for _, _, n in segs], np.int64)
        row.update(segments=len(segs), speech_samples=int(counts.sum()), block_samples=int(last["samples"]))

        def route_a():
            return eng.levels(segs, hop=hop, denoise=0.01)

        def route_b():
            t0 = time.perf_counter()
            data, start = eng.cut(segs, hop=hop, denoise=0.01, layout="range", out="f32")
            t1 = time.perf_counter()
            rec = levels_ref.records([data[start[i]:start[i + 1]] for i in range(len(segs))])
            return rec, t1 - t0, time.perf_counter() - t1

        got, (want, _, _) = route_a(), route_b()
        row["equal_a_b"] = bool(got.tobytes() == want.tobytes())
        a_runs, b_runs, b_cut, b_np = [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            route_a()
            a_runs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _, c, s = route_b()
            b_runs.append(time.perf_counter() - t0)
            b_cut.append(c)
            b_np.append(s)
        row.update(a_s_levels_runs=a_runs, a_s_levels=med(a_runs), b_s_cut_numpy_runs=b_runs, b_s_cut_numpy=med(b_runs), b_s_cut_f32=med(b_cut),
                   b_s_numpy=med(b_np), ratio_b_over_a=med(b_runs) / med(a_runs), bytes_back_a=16 * len(segs), bytes_back_b=int(4 * counts.sum()))
        _, rms = level_stats(got, counts)
        row.update(rms_median=float(np.median(rms)), peak_max=float(got["peak"].max()), clipped_total=int(got["clipped"].sum()))
        # (d) host calls: the gain rides along the cut
        gains = rng.uniform(0.5, 2.0, len(segs)).astype(np.float32)
        for name, kw in (("d_s_cut", {}), ("d_s_cut_gain", {"gains": gains})):
            eng.cut(segs, hop=hop, denoise=0.01, **kw)
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                eng.cut(segs, hop=hop, denoise=0.01, **kw)
                runs.append(time.perf_counter() - t0)
            row[name + "_runs"], row[name] = runs, med(runs)
    # (c), (d) on device pointers: the kernels alone
    block = np.zeros(last["samples"], np.int16)
    for r, o in zip(recs, offs):
        block[o:o + r.size] = r
    d_audio = torch.from_numpy(block).cuda()
    frames_out = int(sum(n for _, _, n in segs)) * frame
    d_out = torch.empty(max(int(counts.sum()), (frames_out + 1) // 2) + 16, dtype=torch.float32, device="cuda")
    d_lv = torch.zeros(2 * len(segs), dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()
    fmt = last["fmt"]

    # a call builds its tables on the host and uploads them before the launch.  The ctypes items are built once, outside, and a
    # matrix product on the same stream in front of the first event keeps the GPU busy while the host checks and builds, so the
    # events bracket the upload of the tables (16 bytes per segment, 8 per workgroup), the clear and the kernel - as scan_cut (a) does
    from cutter_vad_amd import _ffi
    busy = torch.randn(6144, 6144, device="cuda")
    lib, h, n = eng._lib, eng.handle, len(segs)
    it_range, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, 1)
    it_frames, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_FRAMES, 1)
    gp = gains.ctypes.data_as(C.POINTER(C.c_float))
    where = (d_audio.data_ptr(), block.size, 1, fmt)

    def event_timed(fn):
        out = []
        for k in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 2:                           # two warm-ups
                out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    tail = (d_out.data_ptr(), frames_out, ts.cuda_stream)
    calls = {"c_s_levels_device": lambda: lib.vad_scan_levels_device(h, it_range, n, *where, 0, hop, 0.01, 0.95, d_lv.data_ptr(), ts.cuda_stream),
             "c_s_cut_range_f32_device": lambda: lib.vad_scan_cut_device(h, it_range, n, *where, hop, 0.01, _ffi.VAD_CUT_RANGE, _ffi.VAD_CUT_F32,
                                                                         d_out.data_ptr(), int(counts.sum()), ts.cuda_stream),
             "d_s_cut_frames_pcm16_device": lambda: lib.vad_scan_cut_device(h, it_frames, n, *where, hop, 0.01, _ffi.VAD_CUT_FRAMES,
                                                                            _ffi.VAD_CUT_PCM16, *tail),
             "d_s_cut_gain_frames_pcm16_device": lambda: lib.vad_scan_cut_gain_device(h, it_frames, n, gp, *where, 0, hop, 0.01, _ffi.VAD_CUT_FRAMES,
                                                                                      _ffi.VAD_CUT_PCM16, *tail)}
    for name, fn in calls.items():
        runs = event_timed(fn)
        row[name + "_runs"], row[name] = runs, med(runs)
    row["c_equal"] = bool(d_lv.cpu().numpy().tobytes() == got.tobytes())
    read = int(counts.sum()) * 2
    row["c_levels_GBps_read"] = read / row["c_s_levels_device"] / 1e9
    row["c_cut_GBps_read_plus_written"] = (read + 4 * int(counts.sum())) / row["c_s_cut_range_f32_device"] / 1e9
    row["c_ratio_levels_over_cut"] = row["c_s_levels_device"] / row["c_s_cut_range_f32_device"]
    eng.close()
    return row


def scan_audio_batch():
    """What audio batches cost, on scan_levels' corpus: VAD_SCAN_BENCH_N (default 1 024) int16 recordings of 30 s at
    16 kHz, hop 256, the table of its scan.  (a) on device pointers, HIP-event timed: vad_scan_moments_device against
    vad_scan_levels_device on the same table; (b) likewise vad_scan_audio_batch_device (float16, z-score, one window per segment, T the
    longest segment, with its mask) against vad_scan_cut_gain_device(RANGE, F32), with the bytes each moves; (c) audio_recordings
    against the way to the same bytes without it: Engine.cut(layout="range", out="f32") behind the same scan, then the moments, the
    z-score, the padding and the conversion in numpy on 16 host threads - the two alternate, the scan is part of both.  One warm-up,
    then three timed passes of each; medians.  The result goes to profiles/scan_audio_batch.json."""
    import ctypes as C
    import time
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cutter_vad_amd import AudioBatch, VADConfig, _ffi, audio_affine, audio_recordings, audio_windows
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, frame = 256, 512
    gold = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "speech16k_i16.npz")
    pcm = np.tile(np.load(gold)["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    thr = (0.4, 0.3, 0.8, 0.95, 6, 12)
    cfg = VADConfig(sample_rate=16000, buffer_size=frame, vad_start_probability=thr[0], vad_end_probability=thr[1], voice_start_ratio=thr[2],
                    voice_end_ratio=thr[3], voice_start_frame_count=thr[4], voice_end_frame_count=thr[5])
    batch = AudioBatch(norm="zscore", dtype="f16")
    med = lambda v: float(np.median(v))
    row = {"config": f"scan_audio_batch: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, float16, z-score", "recordings": N, "passes": 3}
    pool = ThreadPoolExecutor(16)

    def numpy_route():
        """the same scan, the float32 range cut across the link, then numpy on 16 threads -> (batch, mask, seconds of the numpy part)"""
        slots = eng.open_streams(N)
        try:
            eng.set_thresholds_many(slots, thr)
            with eng.scan_session():
                table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
                offs = [int(o) for o in eng.last_scan["offsets"]]
                segs = [(offs[i], f, n) for i, f, n in zip(table["item"].tolist(), table["first_frame"].tolist(), table["nframes"].tolist())]
                data, start = eng.cut(segs, hop=hop, denoise=0.01, layout="range", out="f32")
        finally:
            for s in slots:
                eng.close_stream(int(s))
        t0 = time.perf_counter()
        n = len(segs)
        mo = np.zeros(n, _ffi.MOMENTS_DTYPE)

        def moment(i):
            x = data[start[i]:start[i + 1]].astype(np.float64)
            mo[i] = (np.rint(np.clip(x, -1.0, 1.0) * 2147483648.0).astype(np.int64).sum(),
                     np.minimum(np.rint(x * x * 4294967296.0), 4294967296.0).astype(np.int64).sum())
        list(pool.map(moment, range(n)))
        counts = np.diff(start)
        shift, scale = audio_affine(mo, None, counts, "zscore", batch.eps)
        _, T = audio_windows(counts)
        out, mask = np.zeros((n, T), np.float16), np.zeros((n, T), np.uint8)

        def fill(i):
            out[i, :counts[i]] = ((data[start[i]:start[i + 1]] + shift[i]) * scale[i]).astype(np.float16)
            mask[i, :counts[i]] = 1
        list(pool.map(fill, range(n)))
        return out, mask, time.perf_counter() - t0, segs, int(data.nbytes)

    got, index, gmask = audio_recordings(recs, batch, cfg, engine=eng, hop=hop, mask=True)
    want, wmask, _, segs, cut_bytes = numpy_route()
    row.update(segments=len(segs), windows=int(got.shape[0]), T=int(got.shape[1]),
               c_equal=bool(got.tobytes() == want.tobytes() and gmask.tobytes() == wmask.tobytes()))
    a_runs, b_runs, b_np = [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        audio_recordings(recs, batch, cfg, engine=eng, hop=hop, mask=True)
        a_runs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = numpy_route()
        b_runs.append(time.perf_counter() - t0)
        b_np.append(r[2])
    block_bytes = int(sum(r.nbytes for r in recs))
    row.update(c_s_audio_recordings_runs=a_runs, c_s_audio_recordings=med(a_runs), c_s_cut_numpy_runs=b_runs, c_s_cut_numpy=med(b_runs),
               c_s_numpy_part=med(b_np), c_ratio_numpy_over_gpu=med(b_runs) / med(a_runs),
               c_link_up_gpu=block_bytes, c_link_back_gpu=int(16 * len(segs) + got.nbytes + gmask.nbytes),
               c_link_up_numpy=block_bytes, c_link_back_numpy=cut_bytes)
    del want, wmask, got, gmask
    # (a), (b) on device pointers: the kernels alone, bracketed by events as scan_levels (c) brackets them
    counts = np.array([(n - 1) * hop + frame for _, _, n in segs], np.int64)
    slots = eng.open_streams(N)
    with eng.scan_session():
        eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        last = eng.last_scan
        block = np.zeros(last["samples"], np.int16)
        for r, o in zip(recs, last["offsets"]):
            block[int(o):int(o) + r.size] = r
        fmt = last["fmt"]
    d_audio = torch.from_numpy(block).cuda()
    windows, T = audio_windows(counts)
    n = len(segs)
    d_cut = torch.empty(int(counts.sum()) + 16, dtype=torch.float32, device="cuda")
    d_out = torch.empty(n * T + 16, dtype=torch.float16, device="cuda")
    d_mask = torch.empty(n * T + 16, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()
    busy = torch.randn(6144, 6144, device="cuda")
    lib, h = eng._lib, eng.handle
    items, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, 1)
    where = (d_audio.data_ptr(), block.size, 1, fmt)
    mo = eng.moments(segs, hop=hop, denoise=0.01, audio=block)
    shift, scale = audio_affine(mo, None, counts, "zscore", batch.eps)
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rec = _ffi.AudioBatchRecord(T, _ffi.VAD_BATCH_F16, _ffi.VAD_BATCH_PAD_VALUE, 0.0)
    wp = windows.ctypes.data_as(C.POINTER(_ffi.AudioWindow))

    def event_timed(fn):
        out = []
        for k in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 2:                           # two warm-ups
                out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    calls = {"a_s_moments_device": lambda: lib.vad_scan_moments_device(h, items, n, *where, 0, hop, 0.01, d_rec.data_ptr(), ts.cuda_stream),
             "a_s_levels_device": lambda: lib.vad_scan_levels_device(h, items, n, *where, 0, hop, 0.01, 0.95, d_rec.data_ptr(), ts.cuda_stream),
             "b_s_audio_batch_device": lambda: lib.vad_scan_audio_batch_device(h, items, n, *where, 0, hop, 0.01, C.byref(rec), wp, n, f32p(shift),
                                                                               f32p(scale), n, d_out.data_ptr(), n * T * 2, d_mask.data_ptr(),
                                                                               ts.cuda_stream),
             "b_s_cut_gain_range_f32_device": lambda: lib.vad_scan_cut_gain_device(h, items, n, f32p(scale), *where, 0, hop, 0.01, _ffi.VAD_CUT_RANGE,
                                                                                   _ffi.VAD_CUT_F32, d_cut.data_ptr(), int(counts.sum()),
                                                                                   ts.cuda_stream)}
    for name, fn in calls.items():
        runs = event_timed(fn)
        row[name + "_runs"], row[name] = runs, med(runs)
    read = int(counts.sum()) * 2
    row["a_ratio_moments_over_levels"] = row["a_s_moments_device"] / row["a_s_levels_device"]
    row["a_moments_GBps_read"] = read / row["a_s_moments_device"] / 1e9
    row["b_batch_bytes_read"], row["b_batch_bytes_written"] = read, int(n * T * 3)
    row["b_cut_bytes_read"], row["b_cut_bytes_written"] = read, int(4 * counts.sum())
    row["b_batch_TBps"] = (read + n * T * 3) / row["b_s_audio_batch_device"] / 1e12
    row["b_cut_TBps"] = (read + 4 * int(counts.sum())) / row["b_s_cut_gain_range_f32_device"] / 1e12
    row["b_ratio_batch_over_cut"] = row["b_s_audio_batch_device"] / row["b_s_cut_gain_range_f32_device"]
    row["not_measured"] = "the bfloat16 and float32 batches, strided windows, the peak and recording scopes, two-channel and rate blocks"
    for s in slots:
        eng.close_stream(int(s))
    eng.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "scan_audio_batch.json"), "w") as f_:
        json.dump({"what": "Audio batches (vad_scan_moments, vad_scan_audio_batch, csrc/scan_levels.hip, csrc/audio_batch.hip): DESIGN 2.1x",
                   "how": "python tools/bench_configs.py scan_audio_batch on one MI355X, one process.  (a), (b) device forms: HIP events "
                          "behind a matrix product that keeps the stream busy while the host builds the tables, two warm-ups and three timed "
                          "passes; the bytes are computed from the shapes (samples read once, cells and mask written once), not counted.  "
                          "(c) the two routes alternate, wall clock around the Python calls, scan included in both, one warm-up and three "
                          "timed passes, medians; the numpy route uses only code the parent has.  Not measured: " + row["not_measured"] +
                          ", L2 hit rates, the spread between processes and boxes",
                   "runs": [row]}, f_, indent=1)
        f_.write("\n")
    return row


def scan_mel():
    """What log-mel features of segment audio cost, on scan_levels' corpus: VAD_SCAN_BENCH_N (default 1 024) int16
    recordings of 30 s at 16 kHz, hop 256, the table of its scan, Whisper's geometry (n_fft 400, hop 160, 201 bins, 80 mels, Hann,
    reflect, log10).  (a) Engine.mel on the block the scan left on the GPU; (b) the way to the same features without it:
    Engine.cut(layout="range", out="f32") of the same table, then frames, two matrix products and the logarithm in numpy float32 on
    the host (tests/mel_ref.py's rule; threads as the box gives them); (a) and (b) alternate.  Agreement: the first 256 segments of
    (a) with the logarithm off against the float64 reference, within the header's bound.  (c) vad_scan_mel_device alone, HIP-event
    timed as scan_levels' (c), against vad_scan_cut_device(RANGE, F32), which moves the samples the host route needs.  One warm-up,
    then three timed passes of each; medians; the result goes to profiles/scan_mel.json."""
    import ctypes as C
    import time
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import MelSpec, _ffi
    from tests import mel_ref as R
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, frame = 256, 512
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    med = lambda v: float(np.median(v))
    spec = MelSpec(16000)
    arrays = spec.operators()
    flds, op_re, op_im, filters = arrays
    f = R.fields(400, 160, 201, 80, R.REFLECT, R.LOG10, 1e-10)
    row = {"config": f"scan_mel: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, n_fft 400 / hop 160 / 201 bins / 80 mels",
           "recordings": N, "passes": 3}
    op = np.concatenate([op_re, op_im], axis=1)

    def numpy_route(data, start):
        out = []
        for i in range(len(start) - 1):
            p = np.pad(data[start[i]:start[i + 1]], 200, mode="reflect")
            fr = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(p, 400)[::160])      # (a strided view would miss BLAS)
            z = fr @ op
            out.append(np.log10(np.maximum((z[:, :201] ** 2 + z[:, 201:] ** 2) @ filters.T, np.float32(1e-10))))
        return np.concatenate(out)

    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        last = eng.last_scan
        offs = [int(o) for o in last["offsets"]]
        segs = [(offs[i], a, n) for i, a, n in zip(table["item"].tolist(), table["first_frame"].tolist(), table["nframes"].tolist())]
        counts = np.array([(n - 1) * hop + frame for _, _, n in segs], np.int64)
        row.update(segments=len(segs), speech_samples=int(counts.sum()), block_samples=int(last["samples"]))

        def route_b():
            t0 = time.perf_counter()
            data, start = eng.cut(segs, hop=hop, denoise=0.01, layout="range", out="f32")
            t1 = time.perf_counter()
            return numpy_route(data, start), t1 - t0, time.perf_counter() - t1, data, start

        got, gstart = eng.mel(segs, arrays, hop=hop, denoise=0.01)
        want, _, _, data, dstart = route_b()
        row.update(rows=int(gstart[-1]), bytes_back_a=int(got.nbytes), bytes_back_b=int(data.nbytes),
                   max_abs_log10_difference_a_b=float(np.abs(got - want).max()))
        # agreement within the header's bound, logarithm off, on the first 256 segments, against float64
        k = min(256, len(segs))
        lin, lstart = eng.mel(segs[:k], ({**flds, "log": "linear"}, op_re, op_im, filters), hop=hop, denoise=0.01)
        worst, worst32, ok = 0.0, 0.0, True
        for i in range(k):
            E, D = R.energies(data[dstart[i]:dstart[i + 1]], f, op_re, op_im, filters)
            g = lin[lstart[i]:lstart[i + 1]].astype(np.float64)
            fr = R.frames(data[dstart[i]:dstart[i + 1]], f)
            z = fr @ op
            E32 = (z[:, :201] ** 2 + z[:, 201:] ** 2) @ filters.T
            live = D > 0
            ok = ok and bool((np.abs(g - E) <= R.bound(f) * D).all())
            if live.any():
                worst = max(worst, float((np.abs(g - E)[live] / (R.U * D[live])).max()))
                worst32 = max(worst32, float((np.abs(E32 - E)[live] / (R.U * D[live])).max()))
        row.update(agree_within_bound=ok, max_err_over_uD_gpu=worst, max_err_over_uD_numpy_f32=worst32, allowed_over_uD=R.bound(f) / R.U)
        a_runs, b_runs, b_cut, b_np = [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.mel(segs, arrays, hop=hop, denoise=0.01)
            a_runs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _, c, s_, _, _ = route_b()
            b_runs.append(time.perf_counter() - t0)
            b_cut.append(c)
            b_np.append(s_)
        row.update(a_s_mel_runs=a_runs, a_s_mel=med(a_runs), b_s_cut_numpy_runs=b_runs, b_s_cut_numpy=med(b_runs), b_s_cut_f32=med(b_cut),
                   b_s_numpy=med(b_np), ratio_b_over_a=med(b_runs) / med(a_runs), host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")))
    # (c) on device pointers: the kernel call alone
    block = np.zeros(last["samples"], np.int16)
    for r, o in zip(recs, offs):
        block[o:o + r.size] = r
    d_audio = torch.from_numpy(block).cuda()
    rows = int(gstart[-1])
    d_out = torch.empty(max(rows * 80, int(counts.sum())) + 16, dtype=torch.float32, device="cuda")
    ts = torch.cuda.Stream()
    busy = torch.randn(6144, 6144, device="cuda")
    lib, h, n = eng._lib, eng.handle, len(segs)
    it_range, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, 1)
    m, a32, b32, w32 = eng._mel_arrays(arrays)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    where = (d_audio.data_ptr(), block.size, 1, last["fmt"])

    def event_timed(fn):
        out = []
        for k in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 2:                           # two warm-ups
                out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    calls = {"c_s_mel_device": lambda: lib.vad_scan_mel_device(h, it_range, n, C.byref(m), fp(a32), fp(b32), fp(w32), *where, hop, 0.01,
                                                               d_out.data_ptr(), rows, ts.cuda_stream),
             "c_s_cut_range_f32_device": lambda: lib.vad_scan_cut_device(h, it_range, n, *where, hop, 0.01, _ffi.VAD_CUT_RANGE, _ffi.VAD_CUT_F32,
                                                                         d_out.data_ptr(), int(counts.sum()), ts.cuda_stream)}
    for name, fn in calls.items():
        runs = event_timed(fn)
        row[name + "_runs"], row[name] = runs, med(runs)
    assert calls["c_s_mel_device"]() == 0
    torch.cuda.synchronize()
    row["c_equal"] = bool(d_out[:rows * 80].cpu().numpy().tobytes() == got.tobytes())
    flop = 2.0 * rows * (400 * 2 * 208 + 208 * 80)
    row["c_mfma_TFLOPs_with_padding"] = flop / row["c_s_mel_device"] / 1e12
    row["c_operator_rereads_GB"] = (rows + 15) // 16 * (2 * 400 * 208 + 80 * 208) * 4 / 1e9
    row["ratio_b_over_c"] = row["b_s_cut_numpy"] / row["c_s_mel_device"]
    eng.close()
    with open(os.path.join(root, "profiles", "scan_mel.json"), "w") as f_:
        json.dump({"what": "Log-mel features of segment audio (vad_scan_mel, csrc/scan_mel.hip): DESIGN 2.1s",
                   "how": "python tools/bench_configs.py scan_mel on one MI355X, one process.  (a) Engine.mel and (b) Engine.cut(range, f32) + "
                          "numpy float32 on the host alternate, wall clock around the Python calls, one warm-up and three timed passes, medians; "
                          "(b) uses only code the parent has.  (c) device forms: HIP events behind a matrix product that keeps the stream "
                          "busy while the host builds the tables, ctypes items built outside the clock, two warm-ups and three timed passes; "
                          "the operator pack is cached after the first call.  c_operator_rereads_GB is computed from the tile count, not "
                          "counted.  Not measured: other geometries, formats and corpus sizes, L2 hit rates, the spread between "
                          "processes and boxes", "runs": [row]}, f_, indent=1)
        f_.write("\n")
    return row


def scan_mel_batch():
    """What model-ready feature batches cost, on scan_mel's corpus and geometry, Whisper's normalisation, float16,
    windows of 1 000 frames.  (a) Engine.mel_keep + Engine.mel_stats(moments=False) + Engine.mel_batch_device into device memory,
    up to the synchronise; (b) the parent commit's way to the same bytes: Engine.mel, then per segment the clamp, the scaling, the
    windows, the padding, the transpose and astype(float16) in numpy on 16 host threads; (a) and (b) alternate, one warm-up and
    three timed passes, medians.  (c) the two kernels alone on the resident matrix, HIP-event timed as scan_mel's (c), with the
    bytes each moves.  The result goes to profiles/scan_mel_batch.json."""
    import ctypes as C
    import time
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import FeatureBatch, MelSpec, _ffi, batch_windows
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, frame, T = 256, 512, 1000
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    med = lambda v: float(np.median(v))
    arrays = MelSpec(16000).operators()
    rec = FeatureBatch(frames=T, norm="whisper", pad="feature", pad_value=-10.0, dtype="f16").record(80)
    row = {"config": f"scan_mel_batch: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, Whisper's geometry and normalisation, "
                     f"float16 windows of {T} frames", "recordings": N, "passes": 3, "host_threads": 16}
    pool = ThreadPoolExecutor(16)

    def numpy_windows(x):
        """one segment's rows -> its windows [k, 80, T] float16, Whisper's two lines and its padding"""
        lo = x.max() - np.float32(8.0)
        v = (np.maximum(x, lo) + np.float32(4.0)) * np.float32(0.25)
        k = -(-x.shape[0] // T)
        out = np.empty((k, T, 80), np.float32)
        out[:] = (np.maximum(np.float32(-10.0), lo) + np.float32(4.0)) * np.float32(0.25)
        out.reshape(k * T, 80)[:x.shape[0]] = v
        return out.transpose(0, 2, 1).astype(np.float16)

    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        offs = [int(o) for o in eng.last_scan["offsets"]]
        segs = [(offs[i], a, n) for i, a, n in zip(table["item"].tolist(), table["first_frame"].tolist(), table["nframes"].tolist())]
        start = eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
        windows, _ = batch_windows(start, T)
        nbytes = windows.size * 80 * T * 2
        d_out = torch.empty(nbytes // 2 + 8, dtype=torch.float16, device="cuda")
        row.update(segments=len(segs), rows=int(start[-1]), windows=int(windows.size), batch_bytes=nbytes, matrix_bytes=int(start[-1]) * 320)

        def route_a():
            eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
            lo = eng.mel_stats(moments=False)["max"] - np.float32(8.0)
            eng.mel_batch_device(windows, rec, d_out.data_ptr(), nbytes, lo=lo, shift=4.0, scale=0.25)
            eng.synchronize()

        def route_b():
            t0 = time.perf_counter()
            feats, st = eng.mel(segs, arrays, hop=hop, denoise=0.01)
            t1 = time.perf_counter()
            parts = list(pool.map(numpy_windows, [feats[st[i]:st[i + 1]] for i in range(len(segs)) if st[i + 1] > st[i]]))
            return np.concatenate(parts), t1 - t0, time.perf_counter() - t1

        route_a()
        want, _, _ = route_b()
        row["a_equals_b"] = bool(d_out[:nbytes // 2].cpu().numpy().tobytes() == want.tobytes())
        a_runs, b_runs, b_mel, b_np = [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            route_a()
            a_runs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _, c, s_ = route_b()
            b_runs.append(time.perf_counter() - t0)
            b_mel.append(c)
            b_np.append(s_)
        row.update(a_s_keep_stats_batch_runs=a_runs, a_s_keep_stats_batch=med(a_runs), b_s_mel_numpy_runs=b_runs, b_s_mel_numpy=med(b_runs),
                   b_s_mel=med(b_mel), b_s_numpy=med(b_np), ratio_b_over_a=med(b_runs) / med(a_runs))
        # (c) the two kernels alone, on the resident matrix
        ts = torch.cuda.Stream()
        busy = torch.randn(6144, 6144, device="cuda")
        lib, h = eng._lib, eng.handle
        d_max = torch.empty(len(segs), dtype=torch.float32, device="cuda")
        lo = eng.mel_stats(moments=False)["max"] - np.float32(8.0)
        b = eng._batch_record(rec, 80)
        w = np.ascontiguousarray(np.asarray(windows, _ffi.BATCH_WINDOW_DTYPE).reshape(-1))      # built here: VAD_BENCH_TREE may name a checkout whose Engine has other helpers
        wp = w.ctypes.data_as(C.POINTER(_ffi.BatchWindow))
        sh, sc = np.full((1, 80), 4.0, np.float32), np.full((1, 80), 0.25, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

        def event_timed(fn):
            out = []
            for k in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                with torch.cuda.stream(ts):
                    torch.mm(busy, busy)
                e0.record(ts)
                assert fn() == 0
                e1.record(ts)
                torch.cuda.synchronize()
                if k >= 2:                           # two warm-ups
                    out.append(e0.elapsed_time(e1) * 1e-3)
            return out

        calls = {"c_s_stats_max_device": (lambda: lib.vad_mel_stats_device(h, None, 0, 0, None, 0, d_max.data_ptr(), None, None, ts.cuda_stream),
                                          int(start[-1]) * 320),
                 "c_s_batch_device": (lambda: lib.vad_mel_batch_device(h, None, 0, None, 0, C.byref(b), wp, w.size, fp(lo), fp(sh), fp(sc), 1,
                                                                       d_out.data_ptr(), nbytes, ts.cuda_stream), int(start[-1]) * 320 + nbytes)}
        for name, (fn, moved) in calls.items():
            runs = event_timed(fn)
            row[name + "_runs"], row[name], row[name + "_bytes"], row[name + "_GBps"] = runs, med(runs), moved, moved / med(runs) / 1e9
    eng.close()
    with open(os.path.join(root, "profiles", "scan_mel_batch.json"), "w") as f_:
        json.dump({"what": "Model-ready feature batches (vad_scan_mel_keep, vad_mel_stats, vad_mel_batch, csrc/mel_batch.hip): DESIGN 2.1u",
                   "how": "python tools/bench_configs.py scan_mel_batch on one MI355X, one process.  (a) and (b) alternate, wall clock around "
                          "the Python calls up to a device synchronise, one warm-up and three timed passes, medians; (b) uses only code the "
                          "parent has.  (c) device forms on the resident matrix: HIP events behind a matrix product that keeps the stream "
                          "busy while the host builds the tables, two warm-ups and three timed passes; the bytes are computed from the "
                          "shapes (matrix read once, batch written once), not counted.  Not measured: deltas, cmvn statistics, other "
                          "layouts and number formats, other window lengths, L2 hit rates, the spread between processes and boxes",
                   "runs": [row]}, f_, indent=1)
        f_.write("\n")
    return row


def mel_project():
    """What a projection of the resident matrix costs, on scan_mel's corpus and geometry, the 80 -> 13 ortho DCT.
    (a) vad_mel_project_device in the replace form on the matrix a keep left (a fresh keep before each pass, outside the events)
    against a device-to-device copy of the same rows x 80 floats in the same run, HIP-event timed as scan_mel_batch's (c).  (b) keep +
    project + stats + batch (cmvn, float16, windows of 1 000 frames, back on the host) against the parent's only route to the same
    tensor: keep + mel_resident_read + numpy float32 @ on 16 threads + mel_stats(features=host) + mel_batch(features=host); the two
    projected matrices are compared with float64 on the first rows.  One warm-up and three timed passes, medians.  The result goes
    to profiles/mel_project.json."""
    import ctypes as C
    import time
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import FeatureBatch, MelSpec, batch_affine, batch_windows, dct_operator
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, T, n_in, n_out = 256, 1000, 80, 13
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    med = lambda v: float(np.median(v))
    arrays = MelSpec(16000).operators()
    op = dct_operator(n_in, n_out)
    rec = FeatureBatch(frames=T, norm="cmvn", dtype="f16").record(n_out)
    row = {"config": f"mel_project: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, Whisper's geometry, 80 -> 13 ortho DCT, cmvn, "
                     f"float16 windows of {T} frames", "recordings": N, "passes": 3, "host_threads": 16}
    pool = ThreadPoolExecutor(16)

    def numpy_project(x):
        parts = np.array_split(np.arange(x.shape[0]), 16)
        return np.concatenate(list(pool.map(lambda p: x[p[0]:p[-1] + 1] @ op if p.size else np.empty((0, n_out), np.float32), parts)))

    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        offs = [int(o) for o in eng.last_scan["offsets"]]
        segs = [(offs[i], a, n) for i, a, n in zip(table["item"].tolist(), table["first_frame"].tolist(), table["nframes"].tolist())]
        start = eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
        rows = int(start[-1])
        windows, _ = batch_windows(start, T)
        row.update(segments=len(segs), rows=rows, windows=int(windows.size), matrix_bytes=rows * n_in * 4, projected_bytes=rows * n_out * 4)

        def route_a():
            eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
            eng.mel_project(op, out=False)
            lo, sh, sc = batch_affine(eng.mel_stats(), start, "cmvn")
            return eng.mel_batch(windows, rec, lo=lo, shift=sh, scale=sc)

        def route_b():
            t0 = time.perf_counter()
            eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
            x = eng.mel_resident_read()
            t1 = time.perf_counter()
            y = numpy_project(x)
            t2 = time.perf_counter()
            lo, sh, sc = batch_affine(eng.mel_stats(y, start), start, "cmvn")
            return eng.mel_batch(windows, rec, lo=lo, shift=sh, scale=sc, features=y, start=start), x, y, t1 - t0, t2 - t1

        got_a = route_a()
        ya = eng.mel_resident_read()
        got_b, x, yb, _, _ = route_b()
        # the two projections against float64 on the first rows, in units of u D (the header's bound: n_in + 2 = 82 for the kernel's
        # fused chain, 2 n_in + 2 = 162 for a chain of separate multiplies and adds)
        k = min(rows, 100000)
        x64, o64 = x[:k].astype(np.float64), op.astype(np.float64)
        uD = 2.0 ** -24 * np.maximum(np.abs(x64) @ np.abs(o64), 1e-300)
        row.update(worst_uD_kernel=float((np.abs(ya[:k] - x64 @ o64) / uD).max()), worst_uD_numpy=float((np.abs(yb[:k] - x64 @ o64) / uD).max()),
                   compared_rows=k, batch_cells_differ=int((got_a.view(np.uint16) != got_b.view(np.uint16)).sum()), batch_cells=int(got_a.size),
                   batch_max_abs_diff=float(np.abs(got_a.astype(np.float32) - got_b.astype(np.float32)).max(initial=0.0)))
        a_runs, b_runs, b_read, b_np = [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            route_a()
            a_runs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _, _, _, c, s_ = route_b()
            b_runs.append(time.perf_counter() - t0)
            b_read.append(c)
            b_np.append(s_)
        row.update(b_s_project_route_runs=a_runs, b_s_project_route=med(a_runs), b_s_host_route_runs=b_runs, b_s_host_route=med(b_runs),
                   b_s_host_keep_read=med(b_read), b_s_host_numpy=med(b_np), b_ratio_host_over_project=med(b_runs) / med(a_runs))
        # (a) the kernel alone against a device-to-device copy of the matrix
        ts = torch.cuda.Stream()
        busy = torch.randn(6144, 6144, device="cuda")
        lib, h = eng._lib, eng.handle
        d_src = torch.empty(rows * n_in, dtype=torch.float32, device="cuda")
        d_dst = torch.empty(rows * n_in, dtype=torch.float32, device="cuda")
        fp = op.ctypes.data_as(C.POINTER(C.c_float))

        def event_timed(fn, before=None):
            out = []
            for k in range(5):
                if before:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                with torch.cuda.stream(ts):
                    torch.mm(busy, busy)
                e0.record(ts)
                assert fn() in (0, None)
                e1.record(ts)
                torch.cuda.synchronize()
                if k >= 2:                           # two warm-ups
                    out.append(e0.elapsed_time(e1) * 1e-3)
            return out

        def copy():
            with torch.cuda.stream(ts):
                d_dst.copy_(d_src)

        moved = rows * (n_in + n_out) * 4
        runs = event_timed(lambda: lib.vad_mel_project_device(h, None, 0, 0, fp, None, n_out, None, ts.cuda_stream),
                           before=lambda: (eng.mel_keep(segs, arrays, hop=hop, denoise=0.01), eng.synchronize()))
        row.update(a_s_project_device_runs=runs, a_s_project_device=med(runs), a_project_bytes=moved, a_project_GBps=moved / med(runs) / 1e9)
        runs = event_timed(copy)
        row.update(a_s_copy_d2d_runs=runs, a_s_copy_d2d=med(runs), a_copy_bytes=rows * n_in * 8, a_copy_GBps=rows * n_in * 8 / med(runs) / 1e9,
                   a_ratio_project_over_copy=row["a_s_project_device"] / med(runs))
    eng.close()
    with open(os.path.join(root, "profiles", "mel_project.json"), "w") as f_:
        json.dump({"what": "Cepstral features: a projection of the resident feature matrix (vad_mel_project, csrc/mel_project.hip): DESIGN 2.1y",
                   "how": "python tools/bench_configs.py mel_project on one MI355X, one process.  (a) the replace form on the resident matrix "
                          "and a device-to-device copy of rows x 80 floats: HIP events behind a matrix product that keeps the stream busy "
                          "while the host checks and packs, a fresh keep before each pass outside the events, two warm-ups and three timed "
                          "passes; the bytes are computed from the shapes (the copy reads and writes the matrix once), not counted.  (b) the "
                          "two routes alternate, wall clock around the Python calls with the batch back on the host, one warm-up and three "
                          "timed passes, medians; the host route uses only code the parent has.  Not measured: other operator shapes "
                          "(128 -> 128 is MFMA-bound by the arithmetic of DESIGN 2.1y), the with-an-out forms, L2 hit rates, the spread "
                          "between processes and boxes",
                   "runs": [row]}, f_, indent=1)
        f_.write("\n")
    return row


def scan_mel_pack():
    """What packing several segments into a window saves, on scan_mel_batch's corpus and setting with Whisper's own
    window: float16, T = 3 000.  The windows and bytes of the unpacked batch (batch_windows: a window per segment) and of the packed
    one (batch_pack per recording), exact counts.  (a) the unpacked route, the parent's unchanged code - Engine.mel_keep +
    Engine.mel_stats(moments=False) + Engine.mel_batch_device - and (b) the packed one - mel_keep + batch_pack + the grouped
    mel_stats over the windows + Engine.mel_batch_packed_device - each up to the synchronise; (a) and (b) alternate, one warm-up and
    three timed passes, medians.  (c) the two batch calls alone on the resident matrix, HIP-event timed as scan_mel_batch's (c).
    The result goes to profiles/scan_mel_pack.json."""
    import ctypes as C
    import time
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import FeatureBatch, MelSpec, _ffi, batch_pack, batch_windows
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, T = 256, 3000
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    med = lambda v: float(np.median(v))
    arrays = MelSpec(16000).operators()
    rec = FeatureBatch(frames=T, norm="whisper", pad="feature", pad_value=-10.0, dtype="f16").record(80)
    row = {"config": f"scan_mel_pack: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, Whisper's geometry and normalisation, "
                     f"float16 windows of {T} frames, unpacked against packed per recording", "recordings": N, "passes": 3}
    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        offs = [int(o) for o in eng.last_scan["offsets"]]
        items = table["item"].tolist()
        segs = [(offs[i], a, n) for i, a, n in zip(items, table["first_frame"].tolist(), table["nframes"].tolist())]
        group = np.asarray(items, np.int32)
        start = eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
        windows, _ = batch_windows(start, T)
        pieces, nw = batch_pack(start, T, 0, group)
        a_bytes, b_bytes = windows.size * 80 * T * 2, nw * 80 * T * 2
        d_out = torch.empty(a_bytes // 2 + 8, dtype=torch.float16, device="cuda")
        rows = int(start[-1])
        row.update(segments=len(segs), rows=rows, matrix_bytes=rows * 320, a_windows=int(windows.size), a_batch_bytes=a_bytes,
                   a_padding_share=1.0 - rows / (windows.size * T), b_pieces=int(pieces.size), b_windows=nw, b_batch_bytes=b_bytes,
                   b_padding_share=1.0 - rows / (nw * T))

        def route_a():
            eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
            lo = eng.mel_stats(moments=False)["max"] - np.float32(8.0)
            eng.mel_batch_device(windows, rec, d_out.data_ptr(), a_bytes, lo=lo, shift=4.0, scale=0.25)
            eng.synchronize()

        def route_b():
            st = eng.mel_keep(segs, arrays, hop=hop, denoise=0.01)
            p, k = batch_pack(st, T, 0, group)
            bounds = np.concatenate([[0], np.cumsum(p["nrows"], dtype=np.int64)])
            lo = eng.mel_stats(start=bounds, moments=False, group=(p["window"], k))["max"] - np.float32(8.0)
            eng.mel_batch_packed_device(p, k, rec, d_out.data_ptr(), b_bytes, lo=lo, shift=4.0, scale=0.25)
            eng.synchronize()

        route_a()
        route_b()
        a_runs, b_runs = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            route_a()
            a_runs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            route_b()
            b_runs.append(time.perf_counter() - t0)
        row.update(a_s_keep_stats_batch_runs=a_runs, a_s_keep_stats_batch=med(a_runs), b_s_keep_pack_stats_batch_runs=b_runs,
                   b_s_keep_pack_stats_batch=med(b_runs), ratio_a_over_b=med(a_runs) / med(b_runs))
        # (c) the two batch calls alone, on the resident matrix
        ts = torch.cuda.Stream()
        busy = torch.randn(6144, 6144, device="cuda")
        lib, h = eng._lib, eng.handle
        b = eng._batch_record(rec, 80)
        w = np.ascontiguousarray(np.asarray(windows, _ffi.BATCH_WINDOW_DTYPE).reshape(-1))      # built here: VAD_BENCH_TREE may name a checkout whose Engine has other helpers
        p = np.ascontiguousarray(np.asarray(pieces, _ffi.BATCH_PIECE_DTYPE).reshape(-1))
        wp, pp = w.ctypes.data_as(C.POINTER(_ffi.BatchWindow)), p.ctypes.data_as(C.POINTER(_ffi.BatchPiece))
        lo_a = eng.mel_stats(moments=False)["max"] - np.float32(8.0)
        bounds = np.concatenate([[0], np.cumsum(pieces["nrows"], dtype=np.int64)])
        lo_b = eng.mel_stats(start=bounds, moments=False, group=(pieces["window"], nw))["max"] - np.float32(8.0)
        sh, sc = np.full((1, 80), 4.0, np.float32), np.full((1, 80), 0.25, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

        def event_timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0
            e1.record(ts)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        calls = {"c_s_batch_device": (lambda: lib.vad_mel_batch_device(h, None, 0, None, 0, C.byref(b), wp, w.size, fp(lo_a), fp(sh), fp(sc), 1,
                                                                       d_out.data_ptr(), a_bytes, ts.cuda_stream), rows * 320 + a_bytes),
                 "c_s_batch_packed_device": (lambda: lib.vad_mel_batch_packed_device(h, None, 0, None, 0, C.byref(b), pp, p.size, nw, fp(lo_b), fp(sh),
                                                                                     fp(sc), 1, d_out.data_ptr(), b_bytes, ts.cuda_stream),
                                             rows * 320 + b_bytes)}
        for k in range(5):                           # the two calls alternate: two warm-up passes, three timed ones
            for name, (fn, moved) in calls.items():
                t = event_timed(fn)
                if k >= 2:
                    row.setdefault(name + "_runs", []).append(t)
        for name, (fn, moved) in calls.items():
            runs = row[name + "_runs"]
            row[name], row[name + "_bytes"], row[name + "_GBps"] = med(runs), moved, moved / med(runs) / 1e9
        row["c_ratio_unpacked_over_packed"] = row["c_s_batch_device"] / row["c_s_batch_packed_device"]
    eng.close()
    with open(os.path.join(root, "profiles", "scan_mel_pack.json"), "w") as f_:
        json.dump({"what": "Packed feature batches (vad_mel_pack_plan, vad_mel_stats_grouped, vad_mel_batch_packed, csrc/mel_batch.hip): DESIGN 2.1w",
                   "how": "python tools/bench_configs.py scan_mel_pack on one MI355X, one process.  The windows and bytes are exact counts.  (a) "
                          "unpacked and (b) packed alternate, wall clock around the Python calls up to a device synchronise, one warm-up and "
                          "three timed passes, medians; (a) uses only code the parent has.  (c) device forms on the resident matrix: HIP events "
                          "behind a matrix product that keeps the stream busy while the host builds the tables, the two calls alternating, "
                          "two warm-up passes and three timed ones; the bytes are computed from the shapes (matrix read once, batch "
                          "written once), not counted.  Not measured: deltas, cmvn statistics, other layouts, number formats, window lengths "
                          "and gaps, L2 hit rates, the spread between processes and boxes", "runs": [row]}, f_, indent=1)
        f_.write("\n")
    return row


def scan_resample_cut():
    """What segment audio and log-mel features at 16 kHz from 48 kHz recordings cost: VAD_SCAN_BENCH_N (default 1 024)
    int16 recordings of 30 s at 48 kHz - the golden clip, every sample three times - hop = chunk / 2, resample_taps' default 97 taps,
    in calls of VAD_SCAN_BENCH_PER_CALL (default 512) recordings: one call addresses under 2 GiB.  Per call, on the block its scan
    (vad_scan_rate_segments, client thresholds) left on the GPU:
      (1) vad_scan_resample_cut_device(F32) against vad_scan_cut_gain_device(RANGE, F32, sr_in = 48000, gains of 1) on the same table,
          which only moves the samples: HIP events as scan_mel's (c);
      (2) Engine.resample_cut(f32) against Engine.cut(range, f32, sample_rate=48000) + scipy.signal.resample_poly(x, 1, 3,
          window=taps) on 16 host threads;
      (3) Engine.mel(sample_rate=48000), Whisper's geometry, against route (2)'s host side followed by scan_mel's numpy float32 mel.
    One warm-up, then three timed passes of each, alternating; medians per call, summed over the calls.  Agreement: the first 64
    segments of the first call against tests/resample_cut_ref.py's float64, within the header's bound.  The result goes to
    profiles/scan_resample_cut.json."""
    import ctypes as C
    import time
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import MelSpec, _ffi, resample_taps
    from tests import resample_cut_ref as R
    try:
        from scipy.signal import resample_poly
    except ImportError:
        resample_poly = None
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    per_call = int(os.environ.get("VAD_SCAN_BENCH_PER_CALL", "512"))
    sr, chunk = 48000, 1536
    hop = chunk // 2
    taps = resample_taps(sr)
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns16 = 30 * 16000
    firsts = rng.integers(0, pcm.size - ns16 + 1, N)
    eng = Engine(blob(5), max_streams=max(per_call, 16))
    slots = eng.open_streams(min(per_call, N))
    med = lambda v: float(np.median(v))
    spec = MelSpec(16000)
    arrays = spec.operators()
    flds, op_re, op_im, filters = arrays
    op = np.concatenate([op_re, op_im], axis=1)
    threads = 16
    pool = ThreadPoolExecutor(threads)
    row = {"config": f"scan_resample_cut: {N} int16 recordings of 30 s at 48 kHz, hop {hop}, {taps.size} taps, calls of {per_call} recordings",
           "recordings": N, "passes": 3, "host_threads": threads, "scipy": resample_poly is not None}
    keys = ("1_s_resample_cut_device", "1_s_cut_gain_range_f32_device", "2_s_resample_cut", "2_s_cut_f32", "2_s_resample_poly", "3_s_rate_mel",
            "3_s_numpy_mel")
    total = {k: 0.0 for k in keys}
    per_group = []
    counts_all = dict(segments=0, speech_samples_48k=0, samples_16k=0, rows=0, tiles=0)

    def host_resample(data, start):
        if resample_poly is None:
            return None
        return list(pool.map(lambda i: resample_poly(data[start[i]:start[i + 1]], 1, 3, window=taps), range(len(start) - 1)))

    def numpy_mel(signals):
        out = []
        for y in signals:
            p = np.pad(y.astype(np.float32), 200, mode="reflect")
            fr = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(p, 400)[::160])
            z = fr @ op
            out.append(np.log10(np.maximum((z[:, :201] ** 2 + z[:, 201:] ** 2) @ filters.T, np.float32(1e-10))))
        return out

    busy = torch.randn(6144, 6144, device="cuda")
    ts = torch.cuda.Stream()

    def event_timed(fn):
        out = []
        for k in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 2:                           # two warm-ups
                out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    for g0 in range(0, N, per_call):
        recs = [np.repeat(pcm[a:a + ns16], 3) for a in firsts[g0:g0 + per_call]]
        sl = slots[:len(recs)]
        eng.reset(sl)
        eng.set_thresholds_many(sl, (0.4, 0.3, 0.8, 0.95, 6, 12))
        grp = {"recordings": len(recs)}
        with eng.scan_session():
            table = eng.scan_segments(sl, recs, hop=hop, denoise=0.01, sample_rate=sr)
            last = eng.last_scan
            offs = [int(o) for o in last["offsets"]]
            segs = [(offs[i], a, n) for i, a, n in zip(table["item"].tolist(), table["first_frame"].tolist(), table["nframes"].tolist())]
            s_in = np.array([(n - 1) * hop + chunk for _, _, n in segs], np.int64)
            s16 = np.array([R.s16(int(s), sr) for s in s_in], np.int64)
            got, gstart = eng.resample_cut(segs, sr, taps, hop=hop, out="f32")
            feat, fstart = eng.mel(segs, arrays, hop=hop, sample_rate=sr, taps=taps)
            grp.update(segments=len(segs), speech_samples_48k=int(s_in.sum()), samples_16k=int(s16.sum()), rows=int(fstart[-1]))
            if g0 == 0:
                data, dstart = eng.cut(segs[:64], hop=hop, layout="range", out="f32", sample_rate=sr)
                worst, ok = 0.0, True
                for i in range(min(64, len(segs))):
                    y, D = R.evaluate(data[dstart[i]:dstart[i + 1]], taps, sr)
                    err = np.abs(got[gstart[i]:gstart[i + 1]].astype(np.float64) - y)
                    ok = ok and bool((err <= R.bound(taps.size, sr) * D).all())
                    live = D > 0
                    if live.any():
                        worst = max(worst, float((err[live] / (R.U * D[live])).max()))
                row.update(agree_within_bound=ok, max_err_over_uD_gpu=worst, allowed_over_uD=R.bound(taps.size, sr) / R.U)
                if resample_poly is not None:
                    hs = host_resample(data, dstart)
                    row["max_abs_difference_to_resample_poly"] = max(
                        float(np.abs(got[gstart[i]:gstart[i] + min(hs[i].size, int(s16[i]))] - hs[i][:int(s16[i])]).max()) for i in range(len(hs)))
            runs = {k: [] for k in keys if not k.startswith("1_")}
            for p in range(4):
                t0 = time.perf_counter()
                eng.resample_cut(segs, sr, taps, hop=hop, out="f32")
                t1 = time.perf_counter()
                data, dstart = eng.cut(segs, hop=hop, layout="range", out="f32", sample_rate=sr)
                t2 = time.perf_counter()
                sig = host_resample(data, dstart)
                t3 = time.perf_counter()
                eng.mel(segs, arrays, hop=hop, sample_rate=sr, taps=taps)
                t4 = time.perf_counter()
                if sig is not None:
                    numpy_mel(sig)
                t5 = time.perf_counter()
                del data, sig
                if p:                            # the first pass is the warm-up
                    for k, v in zip(runs, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                        runs[k].append(v)
            for k, v in runs.items():
                grp[k + "_runs"], grp[k] = v, med(v)
        # (1) on device pointers: the kernel calls alone
        block = np.zeros(last["samples"], np.int16)
        for r, o in zip(recs, offs):
            block[o:o + r.size] = r
        d_audio = torch.from_numpy(block).cuda()
        d_out = torch.empty(int(s_in.sum()) + 16, dtype=torch.float32, device="cuda")
        lib, h, n = eng._lib, eng.handle, len(segs)
        it_rs, _ = eng._resample_items(segs, sr, hop, 1)
        it_cut, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, 1, rate=sr)
        ones = np.ones(n, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        where = (d_audio.data_ptr(), block.size, 1, last["fmt"], sr, hop)
        calls = {"1_s_resample_cut_device": lambda: lib.vad_scan_resample_cut_device(h, it_rs, n, None, fp(taps), taps.size, *where, _ffi.VAD_CUT_F32,
                                                                                     d_out.data_ptr(), int(s16.sum()), ts.cuda_stream),
                 "1_s_cut_gain_range_f32_device": lambda: lib.vad_scan_cut_gain_device(h, it_cut, n, fp(ones), *where, -1.0, _ffi.VAD_CUT_RANGE,
                                                                                       _ffi.VAD_CUT_F32, d_out.data_ptr(), int(s_in.sum()),
                                                                                       ts.cuda_stream)}
        for name, fn in calls.items():
            r_ = event_timed(fn)
            grp[name + "_runs"], grp[name] = r_, med(r_)
        assert calls["1_s_resample_cut_device"]() == 0
        torch.cuda.synchronize()
        grp["1_equal"] = bool(d_out[:int(s16.sum())].cpu().numpy().tobytes() == got.tobytes())
        grp["tiles"] = int(((s16 + 255) // 256).sum())
        del d_audio, d_out, block, recs, got, feat
        torch.cuda.empty_cache()
        for k in keys:
            total[k] += grp[k]
        for k in counts_all:
            counts_all[k] += grp[k]
        per_group.append(grp)
    row.update(counts_all)
    row.update(total)
    K = 144                                      # vad_layout.h: rsc_K(97, 1, 3)
    t = total["1_s_resample_cut_device"]
    row["1_ratio_resample_over_move"] = t / total["1_s_cut_gain_range_f32_device"]
    row["1_bytes_per_s"] = (counts_all["speech_samples_48k"] * 2 + counts_all["samples_16k"] * 4) / t
    row["1_mfma_TFLOPs_with_padding"] = 2.0 * K * 256 * counts_all["tiles"] / t / 1e12
    if resample_poly is not None:
        row["2_ratio_host_over_gpu"] = (total["2_s_cut_f32"] + total["2_s_resample_poly"]) / total["2_s_resample_cut"]
        row["3_ratio_host_over_gpu"] = (total["2_s_cut_f32"] + total["2_s_resample_poly"] + total["3_s_numpy_mel"]) / total["3_s_rate_mel"]
    row["calls"] = per_group
    eng.close()
    pool.shutdown()
    with open(os.path.join(root, "profiles", "scan_resample_cut.json"), "w") as f_:
        json.dump({"what": "Segment audio and log-mel features at 16 kHz from 48 kHz recordings (vad_scan_resample_cut, vad_scan_rate_mel, "
                           "csrc/scan_resample_cut.hip): DESIGN 2.1t",
                   "how": "python tools/bench_configs.py scan_resample_cut on one MI355X, one process; the corpus goes through in calls of 512 "
                          "recordings, each on the block its own rate scan left on the GPU.  (1) device forms: HIP events behind a matrix "
                          "product that keeps the stream busy while the host builds the tables, ctypes items built outside the clock, two "
                          "warm-ups and three timed passes; the operator pack is cached after the first call.  (2), (3): wall clock around the "
                          "Python calls, one warm-up and three timed passes, alternating, medians per call, summed over the calls; the host "
                          "routes use only code the parent has plus scipy and numpy.  1_bytes_per_s counts every input sample of a segment "
                          "once (int16) and every output sample (float32); 1_mfma_TFLOPs_with_padding counts the packed operator's zeros.  Not "
                          "measured: 8 and 24 kHz, other formats, tap counts and corpus sizes, L2 hit rates, the spread between processes and "
                          "boxes", "runs": [row]}, f_, indent=1)
        f_.write("\n")
    return row


def scan_convert():
    """Recordings at 44.1 kHz and any rational rate, converted once on the GPU: VAD_SCAN_BENCH_N (default 1 024) int16
    recordings of 30 s - the golden clip, stretched by index to the rate - in calls of 256 recordings (a call's block and its converted
    block stay under 2 GiB).  Three measurements, one warm-up pass and three timed passes each, medians:
      (a) Engine.scan_segments(sample_rate=44100, convert=True) against the host route - scipy.signal.resample_poly(x, 160, 441,
          window=taps / 160) of every recording on 16 threads (AudioUtils.resample_audio where scipy is missing), then Engine.scan_segments
          of the float32 arrays at 16 kHz;
      (b) vad_convert_device alone on one call's block in device memory, under HIP events, as bytes read and written per second;
      (c) at 48 kHz, the converted scan against the chunk route, Engine.scan_segments(sample_rate=48000) (vad_scan_rate_segments),
          hop = half a frame of each.
    The result goes to profiles/scan_convert.json."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from cutter_vad_amd.scan import convert_taps
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    per_call, seconds = 256, 30
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pcm = np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16)
    one16 = np.resize(pcm, seconds * 16000)
    at_rate = lambda sr: np.ascontiguousarray(one16[(np.arange(seconds * sr, dtype=np.int64) * 16000) // sr])
    eng = Engine(blob(5), max_streams=per_call)
    slots = eng.open_streams(per_call)
    groups = [min(per_call, N - a) for a in range(0, N, per_call)]
    row = {"config": f"scan_convert: {N} int16 recordings of {seconds} s, calls of {per_call} recordings", "recordings": N, "calls": len(groups)}

    def passes(fn):
        fn()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            runs.append(time.perf_counter() - t0)
        return runs

    # (a) 44.1 kHz: the new call against the host route
    sr = 44100
    one = at_rate(sr)
    taps = convert_taps(sr)
    s16 = seconds * 16000
    segs = {}

    def converted(rate, rec, key):
        def run():
            total = 0
            for g in groups:
                eng.reset(slots)
                total += len(eng.scan_segments(slots[:g], [rec] * g, sample_rate=rate, convert=True))
            segs[key] = total
        return run

    try:
        from scipy.signal import resample_poly
        # (resample_poly multiplies a window it is given by `up`: taps / L is this project's filter)
        host_one = lambda x: resample_poly(x.astype(np.float32) / np.float32(32767.0), 160, 441, window=taps.astype(np.float64) / 160.0).astype(np.float32)
        row["host_resampler"] = "scipy.signal.resample_poly(window=taps / L), 16 threads"
    except ImportError:
        from cutter_vad_amd.utils.audio import AudioUtils
        host_one = lambda x: AudioUtils.resample_audio(x.astype(np.float32) / np.float32(32767.0), sr, 16000)
        row["host_resampler"] = "AudioUtils.resample_audio, 16 threads"
    pool = ThreadPoolExecutor(16)

    def host_route():
        total = 0
        for g in groups:
            ys = list(pool.map(host_one, [one] * g))
            eng.reset(slots)
            total += len(eng.scan_segments(slots[:g], ys))
        segs["host"] = total

    row["a_s_convert_runs"] = passes(converted(sr, one, "convert"))
    row["a_s_host_runs"] = passes(host_route)
    pool.shutdown()
    row["a_s_convert"], row["a_s_host"] = float(np.median(row["a_s_convert_runs"])), float(np.median(row["a_s_host_runs"]))
    row["a_host_over_convert"] = row["a_s_host"] / row["a_s_convert"]
    row["a_segments"] = dict(segs)
    row["a_link_GB_convert"], row["a_link_GB_host"] = N * one.size * 2 / 1e9, N * seconds * 16000 * 4 / 1e9
    y_gpu, y_host = eng.convert([one], sr, taps=taps)[0][:s16], host_one(one)
    row["a_max_abs_diff_of_the_two_signals"] = float(np.abs(y_gpu - y_host[:s16]).max())

    # (b) the kernel alone
    g = groups[0]
    block = torch.from_numpy(np.tile(one, g)).cuda()
    s_out = eng.convert_samples(one.size, sr)
    d_out = torch.empty(g * ((s_out + 3) & ~3), device="cuda")
    offs, lens = np.arange(g, dtype=np.int64) * one.size, np.full(g, one.size, np.int64)
    stream = torch.cuda.Stream()
    busy = torch.randn(6144, 6144, device="cuda")
    ms = []
    for i in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            torch.mm(busy, busy)                # keeps the stream busy while the host checks, plans and builds the tables
            a.record()
            eng.convert_device(offs, lens, sr, block.data_ptr(), g * one.size, d_out.data_ptr(), d_out.numel(), taps=taps, fmt=1,
                               stream=stream.cuda_stream)
            b.record()
        stream.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    moved = g * one.size * 2 + d_out.numel() * 4
    row["b_ms_runs"], row["b_ms"] = ms, float(np.median(ms))
    row["b_bytes_moved"], row["b_GB_per_s"] = moved, moved / (float(np.median(ms)) * 1e-3) / 1e9
    row["b_note"] = ("HIP events around vad_convert_device on the caller's stream, behind a matrix product that keeps the stream busy while the "
                     "host plans: the upload of the item and workgroup tables is inside, the operators' pack is cached")
    del block, d_out, busy
    torch.cuda.empty_cache()

    # (c) 48 kHz: the converted scan against the chunk route
    sr = 48000
    one48 = at_rate(sr)

    def chunk_route():
        total = 0
        for g_ in groups:
            eng.reset(slots)
            total += len(eng.scan_segments(slots[:g_], [one48] * g_, sample_rate=sr))
        segs["chunk_48k"] = total

    row["c_s_convert_runs"] = passes(converted(sr, one48, "convert_48k"))
    row["c_s_chunk_runs"] = passes(chunk_route)
    row["c_s_convert"], row["c_s_chunk"] = float(np.median(row["c_s_convert_runs"])), float(np.median(row["c_s_chunk_runs"]))
    row["c_convert_over_chunk"] = row["c_s_convert"] / row["c_s_chunk"]
    row["c_segments"] = {k: segs[k] for k in ("convert_48k", "chunk_48k")}
    eng.close()
    with open(os.path.join(root, "profiles", "scan_convert.json"), "w") as f_:
        json.dump({"what": "Recordings at 44.1 kHz and any rational rate converted once on the GPU (vad_convert, vad_scan_convert_segments, "
                           "csrc/scan_convert.hip): DESIGN 2.1v",
                   "how": "python tools/bench_configs.py scan_convert on one MI355X, one process; per measurement one warm-up pass over the "
                          "corpus and three timed ones (time.perf_counter around the Python calls, which pack, upload and wait; (b): HIP "
                          "events behind a busy stream, the first of four launches dropped); medians.  The parent commit has neither call: (a)'s host route and "
                          "(c)'s chunk route are what it offers, measured in the same process.  One process on one box: the spread "
                          "between processes is not known", "result": row}, f_, indent=1)
        f_.write("\n")
    return row


def scan_rate():
    """Whole recordings at 48 kHz, resampled on the GPU in the scan: vad_scan_rate_device on VAD_SCAN_BENCH_N (default
    4 096) int16 recordings of 30 s at 48 kHz - the golden clip, every sample three times - already in device memory, hop = chunk / 2,
    against vad_scan_device on recordings of the same durations at 16 kHz, which the parent commit has.  One call addresses under
    2 GiB, and 30 s at 48 kHz are 2.88 MB: the corpus goes through in calls of 728 recordings (the same grouping for both rates), on
    one device block per rate that every call of that rate reads.  One warm-up pass over the corpus, then three timed ones (wall
    clock around the calls and the engine's synchronize); the medians and their ratio go to profiles/scan_rate.json."""
    import time
    import numpy as np
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "4096"))
    per_call, seconds = 728, 30
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pcm = np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16)
    one16 = np.resize(pcm, seconds * 16000)
    eng = Engine(blob(5), max_streams=max(per_call, 16))
    slots = eng.open_streams(per_call)
    groups = [min(per_call, N - a) for a in range(0, N, per_call)]
    row = {"config": f"scan_rate: {N} int16 recordings of {seconds} s in device memory, hop = chunk / 2, calls of {per_call} recordings",
           "recordings": N, "calls": len(groups)}
    for sr in (48000, 16000):
        one = np.repeat(one16, sr // 16000)
        chunk = eng.scan_chunk_samples(sr)
        hop = chunk // 2
        block = torch.from_numpy(np.tile(one, per_call)).cuda()
        offs = np.arange(per_call, dtype=np.int64) * one.size
        lens = np.full(per_call, one.size, np.int64)
        nf = eng.scan_frame_count(one.size, hop, sample_rate=sr)
        probs = torch.empty(per_call * nf, device="cuda")
        ev = torch.empty(per_call * nf, dtype=torch.uint8, device="cuda")
        seg = torch.empty(per_call * nf, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def corpus():
            for g in groups:
                eng.reset(slots)
                eng.scan_device(slots[:g], offs[:g], lens[:g], block.data_ptr(), g * one.size, probs.data_ptr(), ev.data_ptr(), seg.data_ptr(),
                                hop=hop, fmt=1, denoise=0.01, sample_rate=sr)
            eng.synchronize()

        corpus()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            corpus()
            runs.append(time.perf_counter() - t0)
        key = f"{sr // 1000}k"
        row[f"s_{key}_runs"] = runs
        row[f"s_{key}"] = float(np.median(runs))
        row[f"frames_{key}"] = N * nf
        row[f"audio_GB_{key}"] = N * one.size * 2 / 1e9
        del block, probs, ev, seg
        torch.cuda.empty_cache()
    row["entry_points"] = {"48k": "vad_scan_rate_device", "16k": "vad_scan_device"}
    row["s_48k_over_s_16k"] = row["s_48k"] / row["s_16k"]
    row["us_per_frame_48k"] = row["s_48k"] / row["frames_48k"] * 1e6
    row["us_per_frame_16k"] = row["s_16k"] / row["frames_16k"] * 1e6
    eng.close()
    with open(os.path.join(root, "profiles", "scan_rate.json"), "w") as f:
        json.dump({"what": "whole recordings at 48 kHz resampled on the GPU in a scan (vad_scan_rate, csrc/scan_resample.hip): DESIGN 2.1j",
                   "how": "python tools/bench_configs.py scan_rate on one MI355X, one process: per rate one warm-up pass over the corpus, "
                          "then three timed passes (time.perf_counter around the six vad_scan*_device calls of 728 recordings and the "
                          "engine's synchronize); s_48k and s_16k are the medians.  One process on one box: the spread between "
                          "processes is not known", "result": row}, f, indent=1)
        f.write("\n")
    return row


def scan_rate_cut():
    """The audio of finished segments of recordings at 48 kHz, resampled on the GPU in the cut: vad_scan_rate_cut_device
    (VAD_CUT_FRAMES, PCM16) on VAD_SCAN_BENCH_N (default 4 096) int16 recordings of 30 s at 48 kHz - the golden clip, every sample
    three times - already in device memory, hop = chunk / 2, against vad_scan_cut_device on recordings of the same durations at
    16 kHz, which the parent commit has.  The segments of a recording come from vad_scan_rate_segments (vad_scan_segments at 16 kHz)
    on a few copies of it, client thresholds; every recording of the corpus is that recording, so it has those segments.  The corpus
    goes through in calls of 728 recordings (one call addresses under 2 GiB), on one device block per rate, into one device output
    that every call of that rate overwrites.  One warm-up pass over the corpus, then three timed ones (wall clock around the calls
    and the engine's synchronize, alternating the two rates); the medians and their ratio go to profiles/scan_rate_cut.json."""
    import time
    import numpy as np
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "4096"))
    per_call, seconds = int(os.environ.get("VAD_SCAN_BENCH_PER_CALL", "728")), 30
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pcm = np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16)
    one16 = np.resize(pcm, seconds * 16000)
    eng = Engine(blob(5), max_streams=16)
    slots = eng.open_streams(4)
    groups = [min(per_call, N - a) for a in range(0, N, per_call)]
    row = {"config": f"scan_rate_cut: {N} int16 recordings of {seconds} s in device memory, hop = chunk / 2, frames as PCM16, calls of "
                     f"{per_call} recordings", "recordings": N, "calls": len(groups)}
    passes = {}
    for sr in (48000, 16000):
        one = np.repeat(one16, sr // 16000)
        chunk = eng.scan_chunk_samples(sr)
        hop = chunk // 2
        eng.reset(slots)
        eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
        table = eng.scan_segments(slots, [one] * 4, hop=hop, denoise=0.01, sample_rate=sr)
        mine = [(int(r["first_frame"]), int(r["nframes"])) for r in table if r["item"] == 0]
        assert mine and all([(int(r["first_frame"]), int(r["nframes"])) for r in table if r["item"] == k] == mine for k in range(4))
        block = torch.from_numpy(np.tile(one, per_call)).cuda()
        segs = [(k * one.size, f, n) for k in range(per_call) for f, n in mine]
        per_rec = sum(n for _, n in mine) * 512
        d_out = torch.empty(per_call * per_rec, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()

        # the calls' item tables, built once: the timed window holds the C entry points alone
        tables = {g: eng._cut_items(segs[:g * len(mine)], hop, 0, 1, rate=None if sr == 16000 else sr)[0] for g in set(groups)}

        def corpus(sr=sr, block=block, tables=tables, d_out=d_out, hop=hop, size=one.size, nseg=len(mine), per_rec=per_rec):
            for g in groups:
                where = (eng.handle, tables[g], g * nseg, block.data_ptr(), g * size, 1, 1)
                res = (0.01, 0, 0, d_out.data_ptr(), g * per_rec, None)
                rc = eng._lib.vad_scan_rate_cut_device(*where, sr, hop, *res) if sr != 16000 else eng._lib.vad_scan_cut_device(*where, hop, *res)
                assert rc == 0, rc
            eng.synchronize()

        key = f"{sr // 1000}k"
        passes[key] = corpus
        row[f"segments_per_recording_{key}"] = len(mine)
        row[f"frames_cut_{key}"] = N * per_rec // 512
        row[f"payload_GB_{key}"] = N * per_rec * 2 / 1e9
        row[f"audio_GB_{key}"] = N * one.size * 2 / 1e9
    runs = {k: [] for k in passes}
    for fn in passes.values():
        fn()
    for _ in range(3):
        for k, fn in passes.items():
            t0 = time.perf_counter()
            fn()
            runs[k].append(time.perf_counter() - t0)
    for k, v in runs.items():
        row[f"s_{k}_runs"] = v
        row[f"s_{k}"] = float(np.median(v))
        row[f"us_per_frame_{k}"] = row[f"s_{k}"] / row[f"frames_cut_{k}"] * 1e6
    row["entry_points"] = {"48k": "vad_scan_rate_cut_device", "16k": "vad_scan_cut_device"}
    row["s_48k_over_s_16k"] = row["s_48k"] / row["s_16k"]
    eng.close()
    with open(os.path.join(root, "profiles", "scan_rate_cut.json"), "w") as f:
        json.dump({"what": "finished segments' frames of recordings at 48 kHz, resampled on the GPU in the cut (vad_scan_rate_cut, "
                           "csrc/scan_cut_resample.hip): DESIGN 2.1k",
                   "how": "python tools/bench_configs.py scan_rate_cut on one MI355X, one process: one warm-up pass over the corpus per "
                          "rate, then three timed passes per rate, alternating (time.perf_counter around the vad_scan*_cut_device calls "
                          "of 728 recordings - table building and upload included - and the engine's synchronize); s_48k and s_16k are "
                          "the medians.  One process on one box: the spread between processes is not known", "result": row}, f, indent=1)
        f.write("\n")
    return row


def scan_render():
    """What one finished piece of audio per recording costs, on scan_levels' corpus: VAD_SCAN_BENCH_N (default 1 024)
    int16 recordings of 30 s at 16 kHz, hop 256, the table of its scan.  (a) silence removal: every recording's segments joined
    with a 10 ms linear crossfade to PCM16 - Engine.render on the block the scan left on the GPU, against today's way to the same
    bytes: Engine.cut(layout="range", out="f32") of the same table, then the fades, the overlap-add and the conversion in numpy;
    the two alternate and their bytes are compared.  (b) the kernel call alone on device pointers, HIP-event timed as scan_levels'
    (c): vad_scan_render_device without overlaps or ramp - the segments packed back to back - against
    vad_scan_cut_gain_device(VAD_CUT_RANGE, gains of ones) on the same table and output format, which writes the same bytes.
    One warm-up, then three timed passes of each; medians; the result goes to profiles/scan_render.json."""
    import ctypes as C
    import json
    import time
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import _ffi, fade_ramp
    from cutter_vad_amd.scan import _join_places
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, frame, nramp = 256, 512, 160
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [pcm[a:a + ns] for a in rng.integers(0, pcm.size - ns + 1, N)]
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    med = lambda v: float(np.median(v))
    ramp = fade_ramp(nramp)
    row = {"config": f"scan_render: {N} int16 recordings of 30 s at 16 kHz in one call, hop {hop}, joined with a 10 ms crossfade to PCM16",
           "recordings": N, "passes": 3}
    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
        last = eng.last_scan
        offs = [int(o) for o in last["offsets"]]
        item = table["item"].tolist()
        segs = [(offs[i], f, n) for i, f, n in zip(item, table["first_frame"].tolist(), table["nframes"].tolist())]
        counts = [(n - 1) * hop + frame for _, _, n in segs]
        # a recording's segments back to back, crossfaded; the recordings' pieces one behind the other in one output
        places, base, k = [], 0, 0
        while k < len(segs):
            m = k
            while m < len(segs) and item[m] == item[k]:
                m += 1
            at = _join_places(counts[k:m], nramp, 0)
            places += [base + p for p in at]
            base += at[-1] + counts[m - 1]
            k = m
        row.update(segments=len(segs), speech_samples=int(sum(counts)), out_samples=base, block_samples=int(last["samples"]))

        def route_a():
            return eng.render(segs, places, base, hop=hop, ramp=ramp, denoise=0.01)

        def route_b():
            t0 = time.perf_counter()
            data, start = eng.cut(segs, hop=hop, denoise=0.01, layout="range", out="f32")
            t1 = time.perf_counter()
            acc = np.zeros(base, np.float32)
            for i, p in enumerate(places):
                w = data[start[i]:start[i + 1]].copy()
                m = min(nramp, w.size)
                w[:m] *= ramp[:m]
                w[w.size - m:] *= ramp[:m][::-1]
                acc[p:p + w.size] += w
            out = np.clip(acc * 32767, -32768, 32767).astype(np.int16)
            return out, t1 - t0, time.perf_counter() - t1

        got, (want, _, _) = route_a(), route_b()
        # (numpy adds a segment to +0.0f where the kernel stores it: the same value, and PCM16 has one zero)
        row["a_equal"] = bool(got.tobytes() == want.tobytes())
        a_runs, b_runs, b_cut, b_np = [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            route_a()
            a_runs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _, c, s = route_b()
            b_runs.append(time.perf_counter() - t0)
            b_cut.append(c)
            b_np.append(s)
        row.update(a_s_render_runs=a_runs, a_s_render=med(a_runs), a_s_cut_numpy_runs=b_runs, a_s_cut_numpy=med(b_runs), a_s_cut_f32=med(b_cut),
                   a_s_numpy=med(b_np), a_ratio_cut_numpy_over_render=med(b_runs) / med(a_runs), a_bytes_back_render=2 * base, a_bytes_back_cut=int(4 * sum(counts)))
    # (b) on device pointers: the kernels alone, the segments packed back to back
    block = np.zeros(last["samples"], np.int16)
    for r, o in zip(recs, offs):
        block[o:o + r.size] = r
    d_audio = torch.from_numpy(block).cuda()
    total = int(sum(counts))
    d_out = torch.empty(total + 16, dtype=torch.int16, device="cuda")
    d_ref = torch.empty(total + 16, dtype=torch.int16, device="cuda")
    ts = torch.cuda.Stream()
    fmt = last["fmt"]
    busy = torch.randn(6144, 6144, device="cuda")
    lib, h, n = eng._lib, eng.handle, len(segs)
    items, _ = eng._cut_items(segs, hop, _ffi.VAD_CUT_RANGE, 1)
    ones = np.ones(n, np.float32)
    gp = ones.ctypes.data_as(C.POINTER(C.c_float))
    where = (d_audio.data_ptr(), block.size, 1, fmt)

    def event_timed(fn):
        out = []
        for k in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 2:                           # two warm-ups
                out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    calls = {"b_s_render_device": lambda: lib.vad_scan_render_device(h, items, n, None, None, 0, *where, 0, hop, 0.01, _ffi.VAD_CUT_PCM16,
                                                                     d_out.data_ptr(), total, ts.cuda_stream),
             "b_s_cut_gain_range_device": lambda: lib.vad_scan_cut_gain_device(h, items, n, gp, *where, 0, hop, 0.01, _ffi.VAD_CUT_RANGE,
                                                                               _ffi.VAD_CUT_PCM16, d_ref.data_ptr(), total, ts.cuda_stream)}
    for name, fn in calls.items():
        runs = event_timed(fn)
        row[name + "_runs"], row[name] = runs, med(runs)
    row["b_equal"] = bool(torch.equal(d_out[:total], d_ref[:total]))
    row["b_GBps_read_plus_written"] = 4 * total / row["b_s_render_device"] / 1e9
    row["b_ratio_render_over_cut"] = row["b_s_render_device"] / row["b_s_cut_gain_range_device"]
    eng.close()
    with open(os.path.join(root, "profiles", "scan_render.json"), "w") as f:
        json.dump({"what": "One finished piece of audio per recording (vad_scan_render, csrc/scan_render.hip): DESIGN 2.1q",
                   "how": "python tools/bench_configs.py scan_render on one MI355X, one process.  (a) Engine.render and Engine.cut(range, "
                          "f32) + numpy alternate, wall clock around the Python calls, one warm-up and three timed passes, medians; the latter uses "
                          "only code the parent has.  (b) device forms: HIP events behind a matrix product that keeps the stream busy while "
                          "the host builds the tables, ctypes items built outside the clock, two warm-ups and three timed passes.  Not "
                          "measured: other corpus sizes, formats, rates and ramps, the mask mode, the spread between processes and boxes",
                   "runs": [row]}, f, indent=1)
        f.write("\n")
    return row


def scan_cut_stereo():
    """What segment audio with both channels kept costs: VAD_SCAN_BENCH_N (default 1 024) two-channel int16
    recordings of 30 s at 16 kHz - speech on the left, other speech at half the level on the right - hop 256, the table of one scan
    of their mix.  (a) device calls, HIP-event timed as scan_render's (b): vad_scan_cut_stereo_device (VAD_CUT_RANGE, PCM16)
    against the parent's way to the same samples on the device - two vad_scan_cut_gain_device calls, channel 0 and channel 1, which
    leave them as two planes - and vad_scan_render_stereo_device (every recording's segments joined with a 10 ms crossfade) against
    two vad_scan_render_device calls; the stereo call and the pair alternate.  (b) end to end: cut_recordings(keep_channels=True,
    layout="range", wav=False) against two cut_recordings calls (channel 0, channel 1) and the numpy interleave - timed on arrays
    of the stereo result's own sizes, since two scans of different channels need not list the same ranges.  One warm-up, then three
    timed passes of each; medians; the result goes to profiles/scan_cut_stereo.json."""
    import ctypes as C
    import json
    import time
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from cutter_vad_amd import VADConfig, _ffi, cut_recordings, fade_ramp
    from cutter_vad_amd.scan import _join_places
    N = int(os.environ.get("VAD_SCAN_BENCH_N", "1024"))
    eng = Engine(blob(5), max_streams=max(N, 16))
    hop, frame, nramp = 256, 512, 160
    pcm = np.tile(np.load(os.path.join(root, "tests", "golden", "speech16k_i16.npz"))["pcm"].astype(np.int16), 3)
    rng = np.random.default_rng(N)
    ns = 30 * 16000
    recs = [np.ascontiguousarray(np.stack([pcm[a:a + ns], pcm[b:b + ns] >> 1], axis=1))
            for a, b in zip(rng.integers(0, pcm.size - ns + 1, N), rng.integers(0, pcm.size - ns + 1, N))]
    med = lambda v: float(np.median(v))
    row = {"config": f"scan_cut_stereo: {N} two-channel int16 recordings of 30 s at 16 kHz, hop {hop}, both channels kept", "recordings": N,
           "passes": 3}
    slots = eng.open_streams(N)
    eng.set_thresholds_many(slots, (0.4, 0.3, 0.8, 0.95, 6, 12))
    with eng.scan_session():
        table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01, channel="mix")
        last = eng.last_scan
        offs = [int(o) for o in last["offsets"]]
        block_samples, fmt = int(last["samples"]), last["fmt"]
    for s in slots:
        eng.close_stream(int(s))
    item = table["item"].tolist()
    segs = [(offs[i], f, n) for i, f, n in zip(item, table["first_frame"].tolist(), table["nframes"].tolist())]
    counts = [(n - 1) * hop + frame for _, _, n in segs]
    total = int(sum(counts))
    places, base, k = [], 0, 0                       # a recording's segments back to back, crossfaded; the pieces one behind the other
    while k < len(segs):
        m = k
        while m < len(segs) and item[m] == item[k]:
            m += 1
        at = _join_places(counts[k:m], nramp, 0)
        places += [base + p for p in at]
        base += at[-1] + counts[m - 1]
        k = m
    row.update(segments=len(segs), speech_frames=total, render_frames=base, block_frames=block_samples)
    # (a) on device pointers
    block = np.zeros((block_samples, 2), np.int16)
    for r, o in zip(recs, offs):
        block[o:o + r.shape[0]] = r
    d_audio = torch.from_numpy(block).cuda()
    room = max(total, base) + 16
    d_st = torch.empty((room, 2), dtype=torch.int16, device="cuda")
    d_pl = torch.empty((2, room), dtype=torch.int16, device="cuda")
    ts = torch.cuda.Stream()
    busy = torch.randn(6144, 6144, device="cuda")
    lib, h, n = eng._lib, eng.handle, len(segs)
    ramp = fade_ramp(nramp)
    rp = ramp.ctypes.data_as(C.POINTER(C.c_float))
    ones = np.ones(n, np.float32)
    gp = ones.ctypes.data_as(C.POINTER(C.c_float))
    cut_st, _ = eng._stereo_items(segs, hop, _ffi.VAD_CUT_RANGE)
    cut_ch = [eng._cut_items([sg + (c,) for sg in segs], hop, _ffi.VAD_CUT_RANGE, 2)[0] for c in (0, 1)]
    ren_st, _ = eng._stereo_items(segs, hop, _ffi.VAD_CUT_RANGE, places)
    ren_ch = [eng._cut_items([sg + (c,) for sg in segs], hop, _ffi.VAD_CUT_RANGE, 2, places)[0] for c in (0, 1)]
    where = (d_audio.data_ptr(), block_samples, 2, fmt)
    P16, RNG_ = _ffi.VAD_CUT_PCM16, _ffi.VAD_CUT_RANGE

    def pair(one):
        return lambda: one(0) or one(1)

    calls = {
        "a_s_cut_stereo_device": lambda: lib.vad_scan_cut_stereo_device(h, cut_st, n, None, *where, 0, hop, 0.01, RNG_, P16, d_st.data_ptr(), total,
                                                                        ts.cuda_stream),
        "a_s_two_cut_gain_device": pair(lambda c: lib.vad_scan_cut_gain_device(h, cut_ch[c], n, gp, *where, 0, hop, 0.01, RNG_, P16,
                                                                               d_pl[c].data_ptr(), total, ts.cuda_stream)),
        "a_s_render_stereo_device": lambda: lib.vad_scan_render_stereo_device(h, ren_st, n, None, rp, nramp, *where, 0, hop, 0.01, P16,
                                                                              d_st.data_ptr(), base, ts.cuda_stream),
        "a_s_two_render_device": pair(lambda c: lib.vad_scan_render_device(h, ren_ch[c], n, None, rp, nramp, *where, 0, hop, 0.01, P16,
                                                                           d_pl[c].data_ptr(), base, ts.cuda_stream)),
    }
    runs = {name: [] for name in calls}
    equal = {}
    for k in range(5):                               # two warm-ups; the stereo call and the pair alternate
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                torch.mm(busy, busy)
            e0.record(ts)
            assert fn() == 0, name
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 2:
                runs[name].append(e0.elapsed_time(e1) * 1e-3)
            if k == 0 and "two" in name:
                size = total if "cut" in name else base
                equal[name] = bool(torch.equal(d_st[:size, 0], d_pl[0, :size]) and torch.equal(d_st[:size, 1], d_pl[1, :size]))
    for name, v in runs.items():
        row[name + "_runs"], row[name] = v, med(v)
    row["a_cut_equal"], row["a_render_equal"] = equal["a_s_two_cut_gain_device"], equal["a_s_two_render_device"]
    row["a_ratio_two_cuts_over_stereo"] = row["a_s_two_cut_gain_device"] / row["a_s_cut_stereo_device"]
    row["a_ratio_two_cuts_over_stereo_spread"] = [min(row["a_s_two_cut_gain_device_runs"]) / max(row["a_s_cut_stereo_device_runs"]),
                                                  max(row["a_s_two_cut_gain_device_runs"]) / min(row["a_s_cut_stereo_device_runs"])]
    row["a_ratio_two_renders_over_stereo"] = row["a_s_two_render_device"] / row["a_s_render_stereo_device"]
    row["a_ratio_two_renders_over_stereo_spread"] = [min(row["a_s_two_render_device_runs"]) / max(row["a_s_render_stereo_device_runs"]),
                                                     max(row["a_s_two_render_device_runs"]) / min(row["a_s_render_stereo_device_runs"])]
    row["a_cut_stereo_GBps_read_plus_written"] = 8 * total / row["a_s_cut_stereo_device"] / 1e9
    del d_audio, d_st, d_pl, busy, block
    torch.cuda.empty_cache()
    # (b) end to end
    cfg = VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6, voice_end_frame_count=12)
    kw = dict(engine=eng, hop=hop, layout="range", wav=False)

    def route_a():
        return cut_recordings(recs, cfg, keep_channels=True, **kw)

    def route_b(shapes):
        t0 = time.perf_counter()
        left = cut_recordings(recs, cfg, channel=0, **kw)
        right = cut_recordings(recs, cfg, channel=1, **kw)
        t1 = time.perf_counter()
        planes = [(np.empty(m, np.int16), np.empty(m, np.int16)) for m in shapes]
        t2 = time.perf_counter()
        both = [np.ascontiguousarray(np.stack(p, axis=1)) for p in planes]
        return (left, right, both), t1 - t0, time.perf_counter() - t2

    got = route_a()
    shapes = [p.shape[0] for one in got for _, _, p in one]
    row.update(b_segments=len(shapes), b_speech_frames=int(sum(shapes)))
    route_b(shapes)
    a_runs, b_runs, b_cuts, b_np = [], [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        route_a()
        a_runs.append(time.perf_counter() - t0)
        _, c, s = route_b(shapes)
        b_runs.append(c + s)
        b_cuts.append(c)
        b_np.append(s)
    row.update(b_s_keep_channels_runs=a_runs, b_s_keep_channels=med(a_runs), b_s_two_calls_interleave_runs=b_runs,
               b_s_two_calls_interleave=med(b_runs), b_s_two_calls=med(b_cuts), b_s_interleave=med(b_np),
               b_ratio_two_calls_over_keep_channels=med(b_runs) / med(a_runs),
               b_ratio_two_calls_over_keep_channels_spread=[min(b_runs) / max(a_runs), max(b_runs) / min(a_runs)])
    eng.close()
    with open(os.path.join(root, "profiles", "scan_cut_stereo.json"), "w") as f:
        json.dump({"what": "Segment audio with both channels kept (vad_scan_cut_stereo, vad_scan_render_stereo): DESIGN 2.1r",
                   "how": "python tools/bench_configs.py scan_cut_stereo on one MI355X, one process.  (a) device forms: HIP events behind a "
                          "matrix product that keeps the stream busy while the host builds the tables, ctypes items built outside the clock, "
                          "the stereo call and the pair of mono calls alternating, two warm-ups and three timed passes, medians; the pair "
                          "leaves two planes, the stereo call the interleaved samples.  (b) cut_recordings(keep_channels=True) against two "
                          "cut_recordings calls and a numpy interleave of arrays of the same sizes, wall clock, one warm-up and three timed "
                          "passes.  The spreads are min / max and max / min of the runs.  Not measured: rate blocks, the render in mask mode, "
                          "other formats, sizes and ramps, the spread between processes and boxes",
                   "runs": [row]}, f, indent=1)
        f.write("\n")
    return row


def single_stream_wrapper():
    """configs[0]: ONE stream through the drop-in VADWrapper (host framing + one launch + sync + callbacks per chunk)."""
    import time
    import numpy as np
    from cutter_vad_amd import VADConfig, VADWrapper
    pcm = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                               "speech16k_i16.npz"))["pcm"]
    x = pcm.astype(np.float32) / 32767.0
    out = []
    for chunk in (512, 480, 1024):
        n = min(x.size // chunk, 600)
        seg = [0]
        with VADWrapper(VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=6,
                                  voice_end_frame_count=12, buffer_size=chunk if chunk < 512 else 512)) as w:
            w.set_callbacks(None, lambda wav: seg.__setitem__(0, seg[0] + 1), None)
            for i in range(20):
                w.process_audio_data(x[i * chunk:(i + 1) * chunk])
            w.reset()
            t0 = time.perf_counter()
            for i in range(n):
                w.process_audio_data(x[i * chunk:(i + 1) * chunk])
            dt = (time.perf_counter() - t0) / n
            frames = w.get_statistics()["total_frames_processed"]
        out.append({"config": f"configs[0]: single stream, VADWrapper.process_audio_data, {chunk}-sample chunks",
                    "us_per_chunk": dt * 1e6, "frames_per_chunk": frames / n, "real_time_factor": (chunk / 16000) / dt,
                    "segments": seg[0]})
    return out


def host_api():
    """PCIe-inclusive: vad_step with HOST pointers (pageable numpy arrays): H2D frames, kernel, D2H probs, sync."""
    import time
    import numpy as np
    B = 8192
    out = []
    eng = Engine(blob(5), max_streams=B)
    slots = eng.open_streams(B)
    rng = np.random.default_rng(0)
    x32 = (0.1 * rng.standard_normal((4, B, 512))).astype(np.float32)
    x16 = np.clip(x32 * 32767.0, -32768, 32767).astype(np.int16)
    p32, p16 = eng.pinned_array(x32.shape, np.float32), eng.pinned_array(x16.shape, np.int16)
    p32[:], p16[:] = x32, x16
    for name, x in (("f32", x32), ("int16", x16), ("f32 (page-locked: Engine.pinned_array)", p32),
                    ("int16 (page-locked: Engine.pinned_array)", p16)):
        for i in range(5):
            eng.step(slots, x[i % 4])
        t0 = time.perf_counter()
        n = 40
        for i in range(n):
            eng.step(slots, x[i % 4])
        dt = (time.perf_counter() - t0) / n
        where = "" if "page-locked" in name else " in pageable host memory"
        out.append({"config": f"batch=8192, V5, host-pointer API (vad_step, {name} frames{where}, "
                              "H2D + kernel + D2H + sync per step)", "us_per_step": dt * 1e6, "frames_per_s": B / dt,
                    "h2d_GBps": x[0].nbytes / dt / 1e9})
    eng.close()
    return out


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:                      # e.g. `bench_configs.py config3 config3_pipelined`
        for name in sys.argv[1:]:
            r = globals()[name]()
            for row in (r if isinstance(r, list) else [r]):
                print(json.dumps(row), flush=True)
        sys.exit(0)
    for r in host_api():
        print(json.dumps(r), flush=True)
    for r in single_stream_wrapper():
        print(json.dumps(r), flush=True)
    for r in resampler_alone():
        print(json.dumps(r), flush=True)
    for fn in (config1, config3, config3_255_tiles, config3_pipelined, config4_per_gpu, two_pools_one_gpu, v4_alone, v4_8k):
        print(json.dumps(fn()), flush=True)
