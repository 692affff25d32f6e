"""Segment tables refined on the GPU (csrc/scan_refine.hip: heads, count, prefix, fill, cuts; vadk_seg_stats behind them;
vad_refine_device, vad_scan_refine).  The bar is BYTE equality with tests/refine_ref.py - written from the rule in
include/vad_engine.h - in all 24 bytes of every record and in the count, with the bytes around every output buffer untouched: the
device form on the synthetic cases of tests/refine_cases.py (no model run: the shapes are exact), on a Silero V4 and an 8 kHz
engine, and one end-to-end run on the golden speech clip through scan_recordings and cut_recordings."""
import os

import numpy as np
import pytest

from cutter_vad_amd import weights_io
from tests import refine_cases as cases
from tests import refine_ref
from tests.cut_ref import decode, gate, pcm16
from tests.test_gpu_scan import GOLD, THR, _engine

pytestmark = pytest.mark.gpu

DTYPE = refine_ref.DTYPE


@pytest.fixture(scope="module")
def eng():
    e = _engine(16000, max_streams=64)
    yield e
    e.close()


def _on_gpu():
    """(dev, back, sync) of cases.run: arrays as torch tensors on the GPU"""
    import torch

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        return (t, a.dtype), t.data_ptr()

    def back(h):
        return h[0].cpu().numpy().view(h[1])

    return dev, back, torch.cuda.synchronize


def _check(e, c, what, caps=None, want=None):
    want = cases.want(c) if want is None else want
    dev, back, sync = _on_gpu()
    for cap in caps or (len(want) + 3, len(want) // 2):
        sync()
        count, got, clean = cases.run(e, c, cap, dev, back, lambda: (e.synchronize(), sync()))
        print(f"refine_device [{what}]: {len(c.table)} records in, {count} out, cap {cap}")
        assert count == len(want), (what, cap, count, len(want))
        assert clean, (what, cap)
        assert refine_ref.same(got, want[:cap]), (what, cap, got[:4], want[:4])
    return want


RULES = {
    "pad_merge_drop_split": (3, 5, 6, 4, 25, 0),
    "ties_small_windows": (4, 1, 2, 3, 9, 0),
    "pairs": (0, 2, -1, 2, 2, 0),
}


@pytest.mark.parametrize("name", list(RULES))
def test_37_items_equal_the_reference(eng, name):
    c = cases.corpus37(np.random.default_rng(1 + list(RULES).index(name)), RULES[name], ties=name != "pad_merge_drop_split")
    nf = np.diff(c.start)
    per_item = np.bincount(c.table["item"], minlength=37)
    assert len(nf) == 37 and nf.min() == 0 and nf.max() == 400 and 1 in nf and 0 in per_item and 1 in per_item
    assert (c.table["first_frame"] < 0).any() and (c.events & 0x80).any()
    seen = refine_ref.census(c.table, c.tails, c.start, c.rule)
    if name == "pairs":                 # never joins: drops, shared gaps and splits alone
        assert seen["merges"] == 0 and seen["drops"] >= 1 and seen["shared"] >= 1 and seen["splits"] >= 50, seen
    else:
        assert min(seen.values()) >= 1 and seen["splits"] >= 5 and seen["merges"] >= 5, seen
    want = _check(eng, c, name, caps=(len(cases.want(c)) + 3, len(cases.want(c)), 7, 0))
    assert max(want["nframes"]) <= c.rule[4]


def test_the_neutral_rule_returns_its_input(eng):
    # records inside their items, statistics by the rule: the output is the input, byte for byte
    c = cases.corpus37(np.random.default_rng(3), refine_ref.NEUTRAL, with_tails=False)
    inside = cases.want(c)
    assert len(inside) > 60
    c = c._replace(table=inside, nsegs=len(inside), in_cap=len(inside))
    want = _check(eng, c, "neutral", caps=(len(inside) + 2,))
    assert want.tobytes() == inside.tobytes()


@pytest.mark.parametrize("name", ["chain", "pads", "drops", "splits", "pairs", "garbage"])
def test_the_named_cases_equal_the_reference(eng, name):
    c = getattr(cases, name)(np.random.default_rng(40 + len(name)))
    seen = refine_ref.census(c.table[:min(c.nsegs, c.in_cap)], c.tails, c.start, c.rule)
    need = {"chain": ("merges", 329), "pads": ("shared", 3), "drops": ("drops", 3), "splits": ("splits", 5), "pairs": ("splits", 2),
            "garbage": ("splits", 2)}[name]
    assert seen[need[0]] >= need[1], seen
    want = _check(eng, c, name)
    if name == "splits":
        first = want[want["item"] == 3]
        k, h, cuts = refine_ref.split_plan(50, 20)
        assert int(first["first_frame"][1]) == 10 + cuts[0] - 1 and int(first["first_frame"][2]) == 10 + cuts[1]


@pytest.mark.parametrize("name", cases.PAST)
def test_past_a_wave_a_workgroup_and_a_grid(eng, name):
    """what the count / prefix / fill / cuts kernels do beyond one wave, one workgroup and one grid - tests/refine_cases.py: past,
    each case's conditions asserted there on the reference before the engine runs.  edges<n>: the prefix's sums across waves and its
    second round, init / count / fill in more than one workgroup, a cap inside a split group; w199, w499, w133: the lane loop of
    the cut going round two to eight times, equal minima a round apart; many: the cut kernel's grid stride and more than 8192
    records through the statistics; heads: first records at rows 255, 256, 257 and 512; bits: +0.0, denormals and 1.0 as minima."""
    c, want, caps = cases.past(name)
    _check(eng, c, name, caps=caps, want=want)


def test_every_cap_of_a_small_table(eng):
    c = cases.splits(np.random.default_rng(7))
    want = cases.want(c)
    _check(eng, c, "splits, every cap", caps=cases.every_cap(c, want), want=want)


def test_negative_probabilities_order_by_bit_pattern(eng):
    """include/vad_engine.h, step 5: a caller's -0.0 and negative values lie above every non-negative probability - by hand, the
    reference does not state this case"""
    c, rows = cases.negzero(np.random.default_rng(0))
    dev, back, sync = _on_gpu()
    count, got, clean = cases.run(eng, c, 6, dev, back, lambda: (eng.synchronize(), sync()))
    assert count == 4 and clean and [tuple(r)[:3] for r in got.tolist()] == rows, got


@pytest.mark.parametrize("version,rate", [(4, 16000), (5, 8000)], ids=["v4", "v5_8k"])
def test_every_engine_has_the_device_form(version, rate):
    from cutter_vad_amd.engine import Engine
    with open(weights_io.packaged_blob_path(version, rate), "rb") as f:
        e = Engine(f.read(), model_version=version, max_streams=16, sample_rate=rate)
    try:
        _check(e, cases.corpus37(np.random.default_rng(12), (3, 5, 6, 4, 25, 0)), f"v{version} {rate}")
    finally:
        e.close()


E2E_RULE = (5, 7, 3, 12, 60, 0)


def test_the_golden_clip_end_to_end(eng):
    """scan_recordings(refine=, stats=True, open_end=True) is refine_ref on the unrefined scan, and cut_recordings(refine=) returns the
    audio of exactly those ranges.  The recordings and the rule were chosen with the f64 oracle's probabilities of the clip: 9 merges,
    3 drops, 2 shared pads and 6 splits there, and the second recording stops inside speech."""
    from cutter_vad_amd import SegmentRefine, VADConfig, cut_recordings, scan_recordings
    pcm = np.load(os.path.join(GOLD, "speech16k_i16.npz"))["pcm"]
    frame, hop = eng.frame_samples, eng.frame_samples // 2
    recs = [pcm, pcm[40000:86500], pcm[100000:101000], pcm[:0], pcm[150000:271360]]
    cfg = VADConfig(vad_start_probability=THR[0], vad_end_probability=THR[1], voice_start_ratio=THR[2], voice_end_ratio=THR[3],
                    voice_start_frame_count=THR[4], voice_end_frame_count=THR[5])
    rule = SegmentRefine(*E2E_RULE)
    assert cfg.enable_denoising                       # the scans below gate at 0.01, as scan_recordings does for this config
    # the unrefined scan: the per-frame results for the reference, the table and the tails
    slots = eng.open_streams(len(recs))
    try:
        eng.set_thresholds_many(slots, THR)
        probs, ev, _ = eng.scan(slots, recs, hop=hop, denoise=0.01)
        eng.reset(slots)
        eng.set_thresholds_many(slots, THR)
        with eng.scan_session():
            table = eng.scan_segments(slots, recs, hop=hop, denoise=0.01)
            tails = eng.scan_tails()
            fine = eng.refine(rule, None, tails)
    finally:
        for s in slots:
            eng.close_stream(int(s))
    start = np.concatenate([[0], np.cumsum([len(p) for p in probs])]).astype(np.int64)
    flat_p, flat_e = np.concatenate(probs).astype(np.float32), np.concatenate(ev).astype(np.uint8)
    seen = refine_ref.census(table, tails, start, E2E_RULE)
    print(f"refine [golden clip]: {len(table)} records, {int((tails['nframes'] > 0).sum())} tails, {seen}")
    assert min(seen.values()) >= 1 and (tails["nframes"] > 0).any(), seen
    want = refine_ref.refine(table, tails, flat_e, flat_p, start, E2E_RULE)
    assert refine_ref.same(np.ascontiguousarray(fine), want) and max(want["nframes"]) <= 60
    lists = [[] for _ in recs]
    for r in want:
        a = int(r["first_frame"]) * hop
        lists[int(r["item"])].append((a, (int(r["first_frame"]) + int(r["nframes"]) - 1) * hop + frame, float(r["mean_prob"]), float(r["max_prob"])))
    got = scan_recordings(recs, cfg, engine=eng, hop=hop, stats=True, open_end=True, refine=rule)
    assert got == lists
    assert got != scan_recordings(recs, cfg, engine=eng, hop=hop, stats=True, open_end=True)
    cut = cut_recordings(recs, cfg, engine=eng, hop=hop, wav=False, layout="range", open_end=True, refine=rule)
    assert [[(a, b) for a, b, _ in one] for one in cut] == [[rg[:2] for rg in one] for one in lists]
    for rec, one in zip(recs, cut):
        for a, b, audio in one:
            assert audio.dtype == np.int16 and np.array_equal(audio, pcm16(gate(decode(rec, "i16_32767"), 0.01))[a:b]) and b - a <= 59 * hop + frame
