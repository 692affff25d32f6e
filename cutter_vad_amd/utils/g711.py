"""ITU-T G.711 (mu-law / A-law) -> 16-bit linear PCM, over the engine library's own decoder (``vad_g711_decode``): the table the
engine uses where it decodes on the host, and what its kernels compute on the GPU.  No reference counterpart: the reference
server takes PCM16 / float32 frames only (websocket_service/server/vad_websocket_server.py:326-382)."""

from __future__ import annotations

import numpy as np

from ..core.exceptions import AudioProcessingError


def g711_decode(data, law: str) -> np.ndarray:
    """``data``: G.711 codes (``bytes`` or a uint8 array of any shape), ``law``: "ulaw" | "alaw" -> int16 array of the same shape
    (a flat array for ``bytes``).  A value s stands for the sample s / 32768."""
    from .. import _ffi
    if law not in _ffi.G711_LAWS:
        raise AudioProcessingError(f"Audio conversion failed: unknown G.711 law {law!r} (expected 'ulaw' or 'alaw')")
    if isinstance(data, (bytes, bytearray, memoryview)):
        codes = np.frombuffer(data, np.uint8)
    else:
        codes = np.asarray(data)
        if codes.dtype != np.uint8:
            raise AudioProcessingError(f"Audio conversion failed: G.711 codes must be uint8, got {codes.dtype}")
        codes = np.ascontiguousarray(codes)
    out = np.empty(codes.shape, np.int16)
    rc = _ffi.lib().vad_g711_decode(_ffi.G711_LAWS[law], codes.ctypes.data, codes.size, out.ctypes.data)
    if rc != 0:
        raise AudioProcessingError(f"Audio conversion failed: vad_g711_decode returned {rc}")
    return out
