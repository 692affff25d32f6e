"""The reference of a replay (vad_resegment_device, vad_scan_resegment; include/vad_engine.h) for
tests/test_scan_resegment_host.py and tests/test_gpu_scan_resegment.py, written from the header's text on the oracle's restatement
of the state machine and tests/seg_ref.py's statistics - never the code under test.  No test, no library of the engine's."""
import numpy as np

from tests import seg_ref


def tables(events, probs, out_start, sets):
    """flat CSR arrays, out_start [n + 1] and threshold 6-tuples -> one table per set: per item a fresh state machine with the set's
    thresholds, the accepted frames in order, one record per END"""
    from oracle import oracle
    events, probs = np.asarray(events, np.uint8), np.asarray(probs, np.float32)
    out = []
    for s in sets:
        rows = []
        for i in range(len(out_start) - 1):
            sm = oracle.StateMachine(*s)
            lo, hi = int(out_start[i]), int(out_start[i + 1])
            for k in range(lo, hi):
                if events[k] & seg_ref.REJECTED:
                    continue
                ev, L = sm.step(float(probs[k]), 1)
                if ev & seg_ref.END:
                    rows.append((i, k - lo - L + 1, L) + seg_ref.stats(probs[lo:hi], events[lo:hi], k - lo - L + 1, k - lo))
        out.append(np.array(rows, seg_ref.DTYPE))
    return out
