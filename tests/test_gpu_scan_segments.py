"""The segment table on the GPU (csrc/scan_segments.hip: count, prefix, fill, statistics; vad_segments_device, vad_scan_segments).
The bar is equality with the numpy reference of tests/seg_ref.py: record for record in ascending flat index, the counts and both
statistics bit for bit (the mean's sum is fixed point, so no order of summation can move it).  Hand-built event arrays reach every
pattern - the chunk's and the wave's edges, the densest table, empty items, a segment longer than two chunks, a prefix of more than
one round, truncation with a sentinel behind the table - and the speech golden goes end to end against Engine.scan on a twin."""
import os

import numpy as np
import pytest

from cutter_vad_amd import _ffi, weights_io
from cutter_vad_amd.scan import segment_ranges, speech_segments
from tests import g711_ref as G
from tests import seg_ref
from tests.test_gpu_scan import GOLD, _engine

pytestmark = pytest.mark.gpu

CHUNK = 4096
CLIENT = (0.4, 0.3, 0.8, 0.95, 6, 12)       # the "client" thresholds of tests/test_gpu_scan_cut.py as a threshold tuple
SENT = 0x5A


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(key):
        if key not in made:
            if key == "v4":
                from cutter_vad_amd.engine import Engine
                with open(weights_io.packaged_blob_path(4, 16000), "rb") as f:
                    made[key] = Engine(f.read(), model_version=4, max_streams=64, sample_rate=16000)
            else:
                made[key] = _engine(key[0])
        return made[key]

    yield get
    for e in made.values():
        e.close()


# ---- hand-built arrays ------------------------------------------------------------------------------------------------
def extract(eng, ev, seg, probs, start, cap, stream=None):
    """Engine.segments_device on torch tensors -> (the written records, the count, the bytes behind them)"""
    import torch
    d_ev, d_seg, d_p = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ev, seg, probs))
    tab = torch.full(((cap + 2) * 24,), SENT, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.segments_device(d_ev.data_ptr(), d_seg.data_ptr(), d_p.data_ptr(), start, tab.data_ptr(), cap, cnt.data_ptr(),
                        stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    else:
        eng.synchronize()
    count = int(cnt.cpu()[0])
    raw = tab.cpu().numpy()
    k = min(count, cap)
    return raw[:k * 24].view(seg_ref.DTYPE).copy(), count, raw[k * 24:]


def check(eng, ev, seg, probs, start, caps=None, stream=None):
    want = seg_ref.table(ev, seg, probs, start)
    for cap in ([len(want)] if caps is None else caps):
        got, count, tail = extract(eng, ev, seg, probs, start, cap, stream)
        assert count == len(want), (count, len(want), cap)
        assert seg_ref.same(got, want[:cap]), (cap, got[:4], want[:4])
        assert tail.size >= 48 and (tail == SENT).all(), cap
    return want


def arrays(rng, total, p_end=0.0, ends=()):
    """events without an END but with every other bit pattern, rejected frames with NaN probabilities, ENDs where asked"""
    ev = rng.choice(np.array([0, 1, 4, 5, 0x80, 0x82, 0x86], np.uint8), total)
    ev[rng.random(total) < p_end] = 0x02
    ev[list(ends)] = 0x02
    seg = np.where(ev == 0x02, rng.integers(1, 60, total), rng.integers(0, 3, total)).astype(np.int32)      # L is read on ENDs alone
    probs = np.where(ev & 0x80, np.float32(np.nan), rng.random(total, np.float32)).astype(np.float32)
    return ev, seg, probs


def split_items(rng, total, n):
    return np.concatenate([[0], np.sort(rng.integers(0, total + 1, n - 1)), [total]]).astype(np.int64)


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17])
def test_totals_around_the_wave_and_the_chunk(engines, total):
    eng = engines((16000,))
    rng = np.random.default_rng(total)
    ev, seg, probs = arrays(rng, total, p_end=0.1, ends=[total - 1] if total else [])
    want = check(eng, ev, seg, probs, split_items(rng, total, 4))
    assert len(want) >= (1 if total else 0)
    check(eng, ev, seg, probs, [0, total])


def test_ends_exactly_on_the_edges_and_on_the_last_index(engines):
    eng = engines((16000,))
    rng = np.random.default_rng(5)
    total = 2 * CHUNK + 77
    edges = [63, 64, 255, 256, 4095, 4096, total - 1]
    ev, seg, probs = arrays(rng, total, ends=edges)
    seg[64] = 5                                            # frame 0 of its item
    want = check(eng, ev, seg, probs, [0, 60, 64, 4096, total])
    assert len(want) == len(edges) and [int(w["item"]) for w in want] == [1, 2, 2, 2, 2, 3, 3]
    assert want["first_frame"].min() < 0                   # L > e + 1 on the way: the statistics start at the item's frame 0
    # every edge alone, and each next to its neighbours
    for k in edges[:-1]:
        for ends in ([k], [k - 1, k, k + 1]):
            e2, s2, p2 = arrays(rng, total, ends=ends)
            assert len(check(eng, e2, s2, p2, [0, total])) == len(ends)


def test_an_end_on_every_second_frame_and_no_end_at_all(engines):
    eng = engines((16000,))
    rng = np.random.default_rng(6)
    total = 8200
    ev = np.zeros(total, np.uint8)
    ev[1::2] = 0x02
    ev[0::2] = rng.choice(np.array([0, 1, 5], np.uint8), total // 2)
    seg = np.where(ev == 2, 2, 0).astype(np.int32)
    probs = rng.random(total, np.float32)
    want = check(eng, ev, seg, probs, [0, 4100, total])
    assert len(want) == 4100 and (want["counted"] == 2).all()
    # every frame an END: more than any scan writes, but a table like any other
    ev[:] = 0x02
    assert len(check(eng, ev, np.ones(total, np.int32), probs, [0, total])) == total
    ev2, seg2, probs2 = arrays(rng, total)
    assert len(check(eng, ev2, seg2, probs2, [0, 17, total], caps=[0, 5])) == 0


def test_300_items_of_0_to_3_frames_in_one_chunk(engines):
    eng = engines((16000,))
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 4, 300)
    lens[[0, 1, 150, 298, 299]] = 0                        # empty items, the first and the last among them
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(start[-1])
    assert total < CHUNK and (lens == 0).sum() > 50
    ev, seg, probs = arrays(rng, total, p_end=0.5)
    want = check(eng, ev, seg, probs, start)
    assert len(want) > 100 and set(want["item"].tolist()) <= set(np.flatnonzero(lens).tolist())
    assert (want["first_frame"] < 0).any() and (want["first_frame"] + want["nframes"] <= lens[want["item"]]).all()


def test_a_segment_of_9000_frames_across_three_chunks(engines):
    eng = engines((16000,))
    rng = np.random.default_rng(8)
    total = 3 * CHUNK + 500
    k = 2 * CHUNK + 1234                                   # in the third chunk
    ev, seg, probs = arrays(rng, total, ends=[k, 40])
    seg[k] = 9000
    start = [0, 100, total]                                # the item spans all of the rest: e = k - 100 >= 9000 - 1
    want = check(eng, ev, seg, probs, start)
    long = want[-1]
    assert long["nframes"] == 9000 and long["first_frame"] == k - 100 - 8999 and 4500 < long["counted"] < 9000      # rejected frames inside
    seg[k] = 12000                                         # L > e + 1: from the item's frame 0
    want = check(eng, ev, seg, probs, start)
    assert want[-1]["first_frame"] < 0 and want[-1]["counted"] == ((ev[100:k + 1] & 0x80) == 0).sum()


def test_rejected_and_end_together_is_no_end_and_nan_probabilities_stay_out(engines):
    eng = engines((16000,))
    total = 700
    ev = np.zeros(total, np.uint8)
    ev[[10, 300, 650]] = 0x82
    ev[[20, 320, 699]] = 0x02
    ev[[5, 15, 16, 310, 698]] = 0x80
    ev[[100, 200]] = 0x86
    seg = np.zeros(total, np.int32)
    seg[[10, 300, 650, 20, 320, 699]] = [7, 7, 7, 18, 30, 200]
    probs = np.linspace(0.001, 0.999, total).astype(np.float32)
    probs[(ev & 0x80) != 0] = np.nan
    want = check(eng, ev, seg, probs, [0, total])
    assert [int(w["first_frame"] + w["nframes"] - 1) for w in want] == [20, 320, 699]
    assert want["counted"].tolist() == [18 - 4, 30 - 2, 200 - 2] and np.isfinite(want["mean_prob"]).all() and np.isfinite(want["max_prob"]).all()


def test_a_prefix_of_more_than_one_round_and_truncation(engines):
    eng = engines((16000,))
    rng = np.random.default_rng(9)
    total = (1 << 20) + 5                                  # 257 chunks: the prefix workgroup takes 256 per round
    ev = np.zeros(total, np.uint8)
    ev[rng.random(total) < 1 / 50] = 0x02
    ev[-1] = 0x02
    seg = np.where(ev == 2, rng.integers(1, 80, total), 0).astype(np.int32)
    probs = rng.random(total, np.float32)
    start = split_items(rng, total, 40)
    want = seg_ref.table(ev, seg, probs, start)
    assert 19000 < len(want) < 23000
    import torch
    for cap in (len(want), len(want) - 1, 0):
        got, count, tail = extract(eng, ev, seg, probs, start, cap, stream=torch.cuda.Stream() if cap == len(want) - 1 else None)
        assert count == len(want) and seg_ref.same(got, want[:cap]) and (tail == SENT).all(), cap


def test_a_v4_engine_extracts_too(engines):
    eng = engines("v4")
    rng = np.random.default_rng(10)
    total = 2 * CHUNK + 3
    ev, seg, probs = arrays(rng, total, p_end=0.05, ends=[total - 1])
    want = check(eng, ev, seg, probs, split_items(rng, total, 7), caps=[0, 3, 10000])
    assert len(want) > 200


# ---- end to end -------------------------------------------------------------------------------------------------------
def _corpus(rate, kind):
    """the speech golden whole and in ragged parts, a part without a frame and a silent one -> (mono recordings, the [N, 2]
    recording of the clip against itself 3 s later), in the wire format `kind`"""
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"]
    if rate == 8000:
        pcm = pcm[::2]
    f = pcm.astype(np.float32) / np.float32(32767.0)
    conv = {"f32": lambda x: x, "i16": lambda x: np.round(x * 32767.0).astype(np.int16), "ulaw": lambda x: G.encode(x, "ulaw")}[kind]
    delayed = np.concatenate([np.zeros(3 * rate, np.float32), f[:-3 * rate]])
    mono = [f, f[:f.size // 2 + 13], f[f.size // 3:], f[:300], np.zeros(5 * rate + 7, np.float32), f[f.size // 5:f.size // 5 * 3 + 2]]
    return [conv(x) for x in mono], np.ascontiguousarray(np.stack([conv(f), conv(delayed)], axis=1))


def _flat(per_item):
    rows = [r for a in per_item for r in (list(a) if np.asarray(a).ndim == 2 else [a])]
    start = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return np.concatenate(rows), start, rows


@pytest.mark.parametrize("cap", [7, 0], ids=["launch7", "launch_default"])
@pytest.mark.parametrize("kind", ["f32", "i16", "ulaw"])
@pytest.mark.parametrize("hop_div", [2, 1], ids=["hop_half", "hop_frame"])
@pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
def test_the_golden_corpus_equals_the_scan_of_a_twin(engines, rate, hop_div, kind, cap):
    eng, twin = engines((rate,)), engines((rate, "twin"))
    frame = eng.frame_samples
    hop = frame // hop_div
    mono, stereo = _corpus(rate, kind)
    kw = dict(law="ulaw" if kind == "ulaw" else None, denoise=0.01)
    totals = []
    for recs, channel, per in ((mono, "mix", 1), ([stereo], "split", 2), ([stereo, stereo[:stereo.shape[0] // 2]], "mix", 1)):
        shape = (len(recs), 2) if per == 2 else (len(recs),)
        s, t = (np.asarray(e.open_streams(len(recs) * per)) for e in (eng, twin))
        try:
            for e, k in ((eng, s), (twin, t)):
                e.set_thresholds_many(k, CLIENT)
                e.set_scan_launch_frames(cap)
            got = eng.scan_segments(s.reshape(shape), recs, hop=hop, channel=channel, **kw)
            probs, ev, seg = twin.scan(t.reshape(shape), recs, hop=hop, channel=channel, **kw)
            fp, start, _ = _flat(probs)
            fe, _, erows = _flat(ev)
            fs, _, srows = _flat(seg)
            want = seg_ref.table(fe, fs, fp, start)
            assert seg_ref.same(got, want), (len(got), len(want))
            ranges = [[] for _ in erows]
            for it, rg in zip(got["item"].tolist(), segment_ranges(got, frame, hop)):
                ranges[it].append(rg)
            assert ranges == [speech_segments(e_, g_, frame, hop) for e_, g_ in zip(erows, srows)]
            assert [eng.save_stream(int(k)) for k in s] == [twin.save_stream(int(k)) for k in t]
            assert (got["counted"] == got["nframes"]).all() and (got["max_prob"] >= got["mean_prob"]).all() and (got["max_prob"] > 0.4).all()
            totals.append([len(r) for r in ranges])
        finally:
            for e, k in ((eng, s), (twin, t)):
                e.set_scan_launch_frames(0)
                for q in k:
                    e.close_stream(int(q))
    print(f"scan_segments [{rate} hop {hop} {kind} cap {cap}]: segments per item {totals}")
    # the corpus - mono parts and the two-channel recording - holds a recording without a segment, one with two or more, and six
    # segments or more in all; no call above compared empty tables
    counts = [c for group in totals for c in group]
    assert min(counts) == 0 and max(counts) >= 2 and sum(counts) >= 6, totals
    assert all(sum(group) >= 1 for group in totals), totals


@pytest.mark.parametrize("rate", [16000, 8000], ids=["v5_16k", "v5_8k"])
def test_scan_and_cut_recordings_equal_the_hand_composition_on_a_twin(engines, rate):
    from cutter_vad_amd import VADConfig, cut_recordings, scan_recordings
    eng, twin = engines((rate,)), engines((rate, "twin"))
    frame = eng.frame_samples
    hop = frame // 2
    mono, stereo = _corpus(rate, "f32")
    recs = mono[:4] + [stereo]
    cfg = VADConfig(sample_rate=rate, buffer_size=frame, vad_start_probability=CLIENT[0], vad_end_probability=CLIENT[1],
                    voice_start_frame_count=CLIENT[4], voice_end_frame_count=CLIENT[5])
    assert (cfg.voice_start_ratio, cfg.voice_end_ratio) == CLIENT[2:4]
    denoise = 0.01 if cfg.enable_denoising else None
    segs = scan_recordings(recs, cfg, engine=eng)
    stats = scan_recordings(recs, cfg, engine=eng, stats=True)
    cuts = cut_recordings(recs, cfg, engine=eng, wav=False)
    n = 0
    for group in (list(range(4)), [4]):
        t = twin.open_streams(len(group))
        try:
            twin.set_thresholds_many(t, CLIENT)
            with twin.scan_session():
                probs, ev, seg = twin.scan(t, [recs[i] for i in group], hop=hop, denoise=denoise)
                offs = twin.last_scan["offsets"]
                want = [speech_segments(e, g, frame, hop) for e, g in zip(ev, seg)]
                table = [(int(offs[k]), a // hop, (b - a - frame) // hop + 1) for k, rg in enumerate(want) for a, b in rg]
                data, start = twin.cut(table, hop=hop, denoise=denoise)
        finally:
            for q in t:
                twin.close_stream(int(q))
        j = 0
        for k, i in enumerate(group):
            assert segs[i] == want[k] and [c[:2] for c in cuts[i]] == want[k] and [s[:2] for s in stats[i]] == want[k]
            flat = seg_ref.table(ev[k], seg[k], probs[k], [0, probs[k].size])
            assert [(float(r["mean_prob"]), float(r["max_prob"])) for r in flat] == [s[2:] for s in stats[i]]
            for c in cuts[i]:
                assert np.array_equal(c[2], data[start[j]:start[j + 1]]) and c[2].size == (c[1] - c[0] - frame) // hop * frame + frame
                j += 1
                n += 1
        assert j == len(table)
    assert n >= 5 and segs[3] == []
