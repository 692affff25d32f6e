"""The numpy reference of the segment table (vad_segments_device, vad_scan_segments; include/vad_engine.h: vad_segment) for
tests/test_scan_segments_host.py (CPU stand-in) and tests/test_gpu_scan_segments.py: a loop over np.flatnonzero of the END rule and
the fixed-point mean, written from the header's text - never the code under test.  No test, no library: importing it loads neither
the stand-in nor the engine."""
import numpy as np

DTYPE = np.dtype([("item", np.int32), ("first_frame", np.int32), ("nframes", np.int32), ("counted", np.int32),
                  ("mean_prob", np.float32), ("max_prob", np.float32)])
END, REJECTED = 0x02, 0x80


def stats(probs, events, first_frame, e):
    """the accepted frames max(first_frame, 0) .. e of ONE item's arrays -> (counted, mean_prob, max_prob)"""
    p = probs[max(first_frame, 0):e + 1][(events[max(first_frame, 0):e + 1] & REJECTED) == 0]
    S = int(np.rint(p.astype(np.float64) * 2.0 ** 30).astype(np.int64).sum())
    return p.size, np.float32(S / (p.size * 2.0 ** 30)), p.max()


def table(events, seg_frames, probs, out_start):
    """the flat CSR arrays of a scan and its out_start [n + 1] -> every record, in ascending flat index"""
    events, seg_frames, probs = np.asarray(events, np.uint8), np.asarray(seg_frames, np.int32), np.asarray(probs, np.float32)
    start = np.asarray(out_start, np.int64)
    rows = []
    if start.size > 1:
        lo, hi = int(start[0]), int(start[-1])
        for k in lo + np.flatnonzero((events[lo:hi] & (END | REJECTED)) == END):
            i = int(np.searchsorted(start, k, side="right")) - 1          # the last item with out_start[i] <= k
            e, L = int(k - start[i]), int(seg_frames[k])
            rows.append((i, e - L + 1, L) + stats(probs[start[i]:start[i + 1]], events[start[i]:start[i + 1]], e - L + 1, e))
    return np.array(rows, DTYPE)


def same(got, want):
    """record for record, the statistics bit for bit"""
    return got.dtype == DTYPE and want.dtype == DTYPE and got.shape == want.shape and got.tobytes() == want.tobytes()
