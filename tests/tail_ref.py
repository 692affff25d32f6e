"""The reference of the tails (vad_scan_tails, vad_scan_resegment_tails and their device forms; include/vad_engine.h) for
tests/test_scan_tails_host.py and tests/test_gpu_scan_tails.py, written from the header's text on the oracle's restatement of the
state machine and tests/seg_ref.py's statistics - never the code under test.  No test, no library of the engine's."""
import numpy as np

from tests import seg_ref


def step_item(sm, events, probs):
    """ONE item's arrays through `sm` (an oracle.StateMachine, fresh or continued), one frame per step: rejected frames skipped"""
    for e, p in zip(events, probs):
        if not (e & seg_ref.REJECTED):
            sm.step(float(p), 1)
    return sm


def record(item, sm, events, probs):
    """the tail of ONE item whose frames took `sm` to where it is -> a tuple for seg_ref.DTYPE: all zero without a tail"""
    nf = len(probs)
    L = int(sm.counts()["seg_samples"])          # frame_len = 1: samples are frames
    if nf < 1 or not sm.active or L < 1:
        return (0, 0, 0, 0, 0.0, 0.0)
    first = nf - L
    if ((np.asarray(events[max(first, 0):nf]) & seg_ref.REJECTED) == 0).any():
        st = seg_ref.stats(np.asarray(probs, np.float32), np.asarray(events, np.uint8), first, nf - 1)
    else:
        st = (0, 0.0, 0.0)
    return (item, first, L) + tuple(st)


def tails(events, probs, out_start, machines):
    """flat CSR arrays, out_start [n + 1] and one state machine per item (stepped in place) -> the n records"""
    events, probs = np.asarray(events, np.uint8), np.asarray(probs, np.float32)
    rows = []
    for i, sm in enumerate(machines):
        lo, hi = int(out_start[i]), int(out_start[i + 1])
        step_item(sm, events[lo:hi], probs[lo:hi])
        rows.append(record(i, sm, events[lo:hi], probs[lo:hi]))
    return np.array(rows, seg_ref.DTYPE).reshape(-1)


def fresh(events, probs, out_start, sets):
    """... per threshold 6-tuple, every item on a fresh state machine with that set -> one array per set"""
    from oracle import oracle
    return [tails(events, probs, out_start, [oracle.StateMachine(*s) for _ in range(len(out_start) - 1)]) for s in sets]
