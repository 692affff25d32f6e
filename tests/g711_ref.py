"""ITU-T G.711 for the tests, in NumPy and independent of the product: the two decode formulas (include/vad_engine.h quotes them),
the pins of their 256-entry tables, and an encoder - the product has none - that maps a float signal to the code whose decoded
value is nearest."""
import hashlib

import numpy as np

LAWS = ("ulaw", "alaw")
SHA256 = {"ulaw": "3dab54339e520bb2c924826e3b72a917a2b612e9fd12fc867500f1d983a75827",
          "alaw": "e04788d110e58ff8c70c93b8480190d973e3b67876b6119abbaec766cc75c174"}
ABS_SUM = {"ulaw": 1532928, "alaw": 1564672}
PEAK = {"ulaw": 32124, "alaw": 32256}
DISTINCT = {"ulaw": 255, "alaw": 256}


def table(law):
    """int16 [256]: the decoded value of every code."""
    b = np.arange(256, dtype=np.int64)
    if law == "ulaw":
        u = ~b & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
        s = np.where(u & 0x80, 0x84 - t, t - 0x84)
    else:
        a = b ^ 0x55
        t = (a & 0x0F) << 4
        seg = (a & 0x70) >> 4
        t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
        s = np.where(a & 0x80, t, -t)
    return s.astype(np.int16)


def table_sha256(tab):
    return hashlib.sha256(np.asarray(tab).astype("<i2").tobytes()).hexdigest()


def encode(x, law):
    """float array (full scale 1.0) -> uint8 codes of the same shape: the code whose decoded value / 32768 is nearest."""
    tab = table(law).astype(np.float64)
    order = np.argsort(tab, kind="stable")
    vals = tab[order]
    v = np.asarray(x, np.float64) * 32768.0
    hi = np.clip(np.searchsorted(vals, v), 1, 255)
    lo = hi - 1
    pick = np.where(np.abs(vals[hi] - v) < np.abs(v - vals[lo]), hi, lo)
    return order[pick].astype(np.uint8)


def all_codes_frame(frame_samples, roll=0):
    """one frame that holds every code 0..255 (tiled to the frame length)"""
    assert frame_samples >= 256
    return np.roll(np.resize(np.arange(256, dtype=np.uint8), frame_samples), roll)


def speechlike(n_streams, n_frames, frame_samples, seed, sigma=0.3):
    """Gaussian bursts with silences, clipped to full scale: [n_streams, n_frames, frame_samples] float64"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, sigma, (n_streams, n_frames, frame_samples))
    env = rng.uniform(0.0, 1.0, (n_streams, n_frames, 1)) ** 2
    return np.clip(x * env, -1.0, 1.0)
