"""ITU-T G.711 (mu-law / A-law) frames, the parts that need no GPU: the host decoder and its pins, the C ABI's additions, the
occupancy contract of the new kernel instantiations, the serving layer on the scripted engine, and the argument checks."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cutter_vad_amd import VADConfig, _ffi
from cutter_vad_amd.core.exceptions import AudioProcessingError
from cutter_vad_amd.utils import g711_decode
from tests import g711_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"ulaw": 3, "alaw": 4}


def _decode_c(fmt, codes):
    codes = np.ascontiguousarray(codes, np.uint8)
    out = np.full(codes.size, 12345, np.int16)
    rc = _ffi.lib().vad_g711_decode(fmt, codes.ctypes.data, codes.size, out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("law", G.LAWS)
def test_decoder_gives_the_itu_tables(law):
    rc, out = _decode_c(FMT[law], np.arange(256, dtype=np.uint8))
    assert rc == _ffi.VAD_OK
    assert np.array_equal(out, G.table(law))                            # the formula, evaluated in NumPy
    assert G.table_sha256(out) == G.SHA256[law]
    assert int(np.abs(out.astype(np.int64)).sum()) == G.ABS_SUM[law]
    assert int(out.min()) == -G.PEAK[law] and int(out.max()) == G.PEAK[law]
    assert len(set(out.tolist())) == G.DISTINCT[law]
    try:
        import audioop                                                  # gone from newer Pythons: this part only
    except ImportError:
        audioop = None
    if audioop is not None:
        lin = (audioop.ulaw2lin if law == "ulaw" else audioop.alaw2lin)(bytes(range(256)), 2)
        assert np.array_equal(out, np.frombuffer(lin, "<i2"))
    # the exactness the design rests on: s / 32768 is a float32, and the way back is exact
    f = out.astype(np.float32) / np.float32(32768)
    assert f.dtype == np.float32 and np.array_equal(f * np.float32(32768), out.astype(np.float32))
    assert np.array_equal(f.astype(np.float64) * 32768.0, out.astype(np.float64))
    # the Python wrapper: bytes and arrays of any shape
    assert np.array_equal(g711_decode(bytes(range(256)), law), G.table(law))
    codes = np.arange(512, dtype=np.uint16).astype(np.uint8).reshape(2, 256)
    assert np.array_equal(g711_decode(codes, law), G.table(law)[codes])


def test_decoder_spot_values_and_refusals():
    u, a = G.table("ulaw"), G.table("alaw")
    assert (u[0x00], u[0x80], u[0x01], u[0x7F], u[0xFF]) == (-32124, 32124, -31100, 0, 0)
    assert (a[0x55], a[0xD5], a[0x2A], a[0xAA]) == (-8, 8, -32256, 32256) and int(np.abs(a).min()) == 8
    for fmt in (_ffi.VAD_FMT_F32, _ffi.VAD_FMT_I16_32767, _ffi.VAD_FMT_I16_32768, 5, -1):
        rc, out = _decode_c(fmt, np.arange(256, dtype=np.uint8))
        assert rc == _ffi.VAD_ERR_INVALID_ARG and np.all(out == 12345)
    assert _ffi.lib().vad_g711_decode(3, None, 4, None) == _ffi.VAD_ERR_INVALID_ARG
    assert _ffi.lib().vad_g711_decode(3, None, 0, None) == _ffi.VAD_OK
    with pytest.raises(AudioProcessingError):
        g711_decode(b"\0", "xyz")
    with pytest.raises(AudioProcessingError):
        g711_decode(np.zeros(4, np.int16), "ulaw")


def test_header_ffi_and_library_agree_on_the_additions():
    with open(os.path.join(ROOT, "include", "vad_engine.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+VAD_ABI_VERSION\s+5\b", src)                       # additive: the ABI number did not move
    assert re.search(r"#define\s+VAD_TICK_GROUPS\s+12\b", src)
    enum = dict(re.findall(r"\b(VAD_FMT_\w+)\s*=\s*(-?\d+)", src))
    assert enum == {"VAD_FMT_F32": "0", "VAD_FMT_I16_32767": "1", "VAD_FMT_I16_32768": "2", "VAD_FMT_ULAW8": "3", "VAD_FMT_ALAW8": "4"}
    assert (_ffi.VAD_FMT_ULAW8, _ffi.VAD_FMT_ALAW8) == (3, 4)
    assert re.search(r"^VAD_API\s+int\s+vad_g711_decode\s*\(\s*int\s+frame_fmt\s*,\s*const\s+uint8_t\s*\*\s*in\s*,\s*int64_t\s+n\s*,"
                     r"\s*int16_t\s*\*\s*out\s*\)\s*;", src, re.M)
    assert "vad_g711_decode" in _ffi.SIGNATURES and hasattr(_ffi.lib(), "vad_g711_decode")
    res, args = _ffi.SIGNATURES["vad_g711_decode"]
    assert res is C.c_int and len(args) == 4 and args[0] is C.c_int and args[2] is C.c_int64


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_g711_instantiations_of_the_16_stream_kernel_keep_the_occupancy_contract(tmp_path):
    """The method of tests/test_occupancy_contract.py, for the new entry point: the single-frame G.711 instantiations must fit
    two workgroups per CU like the float32 / int16 ones they sit beside (<= 256 registers, <= 80 KB LDS, no scratch)."""
    from cutter_vad_amd import _build
    out = tmp_path / "t16.s"
    flags = ["-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=8"]
    subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", *flags, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16.hip")], check=True, capture_output=True, timeout=900)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?"
                         r"\.vgpr_count:\s*(\d+)", text, re.S):
        kernels[m.group(2)] = (int(m.group(1)), int(m.group(3)), int(m.group(4)))
    # _Z21silero_v5_step16_g711ILb<ALAW>ELb<K8>ELb<ONE>EEv...: {mu-law, A-law} x {16 kHz, 8 kHz} x {one frame, frame loop}
    g711 = {k: v for k, v in kernels.items() if re.match(r"_Z21silero_v5_step16_g711ILb[01]ELb[01]ELb[01]EE", k)}
    assert len(g711) == 8, sorted(kernels)
    one = {k: v for k, v in g711.items() if re.match(r"_Z21silero_v5_step16_g711ILb[01]ELb[01]ELb1EE", k)}
    assert len(one) == 4
    for name, (lds, scratch, regs) in one.items():
        assert regs <= 256, (name, regs)
        assert lds <= 80 * 1024, (name, lds)
        assert scratch == 0, (name, scratch)
    assert all(scratch == 0 for _, scratch, _ in g711.values())
    assert all(lds <= 160 * 1024 for lds, _, _ in kernels.values())
    # the four names the existing contract test matches are still there
    assert len([k for k in kernels if re.match(r"_Z16silero_v5_step16ILb[01]ELb0ELb[01]ELb1EE", k)]) == 4


# ---- serving on the scripted engine ---------------------------------------------------------------------------------------------
def _pool():
    from cutter_vad_amd.server import SharedStreamPool
    from tests.fakes import FakeEngine, FakePool
    eng = FakeEngine(fn=lambda fr: 0.9 if np.abs(fr).max() > 0.3 else 0.05)
    return SharedStreamPool(pool=FakePool(eng)), eng


def _utterance(law, n=480):
    """loud x 3, quiet x 4 as G.711 frames (every code appears in the first one)"""
    rng = np.random.default_rng(7)
    loud = [G.encode(np.clip(rng.normal(0, 0.4, n), -1, 1), law) for _ in range(3)]
    loud[0][:256] = np.arange(256, dtype=np.uint8)
    quiet = [G.encode(np.zeros(n), law) for _ in range(4)]
    return [f.tobytes() for f in loud + quiet]


@pytest.mark.parametrize("law", G.LAWS)
def test_submit_g711_equals_submit_pcm16_of_the_decoded_frames(law):
    logs, seen = [], []
    for kind in ("g711", "pcm16"):
        pool, eng = _pool()
        s = pool.open_session(VADConfig(vad_start_probability=0.4, vad_end_probability=0.3, voice_start_frame_count=2,
                                        voice_end_frame_count=3, buffer_size=480))
        log = []
        s.set_callbacks(lambda log=log: log.append("S"), lambda wav, log=log: log.append(("E", bytes(wav))),
                        lambda pcm, log=log: log.append(("C", bytes(pcm))))
        for fr in _utterance(law):
            if kind == "g711":
                s.submit_g711(fr, law)
            else:
                s.submit_pcm16(G.table(law)[np.frombuffer(fr, np.uint8)].astype("<i2").tobytes())
        pool.drain()
        logs.append(log)
        seen.append([f.copy() for f in eng.frames_seen])
        with pytest.raises(AudioProcessingError):
            s.submit_g711(b"\0" * 480, "xyz")
        pool.close()
    assert logs[0] == logs[1] and logs[0][0] == "S" and any(isinstance(e, tuple) and e[0] == "E" for e in logs[0])
    assert len(seen[0]) == len(seen[1]) and all(np.array_equal(a, b) for a, b in zip(seen[0], seen[1]))


def test_ulaw_and_alaw_modes_over_asgi():
    from fastapi.testclient import TestClient
    from cutter_vad_amd.server.app import create_app, create_client_config, frame_bytes, parse_query_params
    cfg = create_client_config(parse_query_params("mode=ulaw&sample_rate=8000"))
    assert cfg["audio"]["sample_width"] == 1 and frame_bytes(cfg) == 240          # the pcm default of 2 does not apply
    assert create_client_config(parse_query_params("mode=alaw&sample_width=2"))["audio"]["sample_width"] == 2
    assert create_client_config(parse_query_params("mode=pcm"))["audio"]["sample_width"] == 2

    def recv_until(ws, kind, limit=200):
        got = []
        for _ in range(limit):
            m = json.loads(ws.receive_text())
            got.append(m)
            if m["event"] == kind:
                return got
        raise AssertionError(f"no {kind} in {got}")

    def run(url, frames):
        pool, eng = _pool()
        app = create_app(pool, tick_interval=0.002)
        events = []
        with TestClient(app) as client:
            with client.websocket_connect(url) as ws:
                assert json.loads(ws.receive_text())["event"] == "INFO"
                ws.send_bytes(b"\0" * 100)
                events.append(json.loads(ws.receive_text())["message"])
                for fr in frames:
                    ws.send_bytes(fr)
                events += [m["event"] for m in recv_until(ws, "VOICE_END")]
        frames_seen = np.concatenate([f.reshape(-1, f.shape[-1]) for f in eng.frames_seen])
        return events, frames_seen

    for law in G.LAWS:
        frames = _utterance(law)
        pcm = [G.table(law)[np.frombuffer(fr, np.uint8)].astype("<i2").tobytes() for fr in frames]
        ev_g, seen_g = run(f"/vad?mode={law}&start_frame_count=2&end_frame_count=3", frames)
        ev_p, seen_p = run("/vad?mode=pcm&sample_width=2&start_frame_count=2&end_frame_count=3", pcm)
        assert ev_g[0] == "Invalid frame size: expected 480, got 100" and ev_p[0] == "Invalid frame size: expected 960, got 100"
        assert ev_g[1:] == ev_p[1:] and ev_g[1] == "VOICE_START" and ev_g[-1] == "VOICE_END"
        # the engine saw the same samples (the socket closes on VOICE_END, the 6th frame's event: whether the ticker still
        # steps the 7th before the session goes is a matter of timing, so the comparison covers what both runs stepped)
        k = min(len(seen_g), len(seen_p))
        assert k >= 6 and np.array_equal(seen_g[:k], seen_p[:k])

    pool, eng = _pool()
    with TestClient(create_app(pool, tick_interval=0.002)) as client:
        with client.websocket_connect("/vad?mode=ulaw&sample_width=2") as ws:
            assert json.loads(ws.receive_text())["event"] == "INFO"
            ws.send_bytes(b"\xff" * 960)
            m = json.loads(ws.receive_text())
            assert m["event"] == "ERROR" and m["message"] == "Unsupported sample width: 2"
        with client.websocket_connect("/vad?mode=opus") as ws:
            m = json.loads(ws.receive_text())
            assert m["event"] == "ERROR" and "PyAV is required for opus" in m["message"]
        with client.websocket_connect("/vad?mode=g722") as ws:
            m = json.loads(ws.receive_text())
            assert m["event"] == "ERROR" and m["message"] == "Unsupported audio mode: g722"


def test_law_argument_is_checked_before_the_engine_is_touched():
    from cutter_vad_amd.engine import Engine
    e = Engine.__new__(Engine)                                            # no device: the checks come first
    e.frame_samples = 512
    e._h = None
    codes = np.zeros((2, 512), np.uint8)
    s, f, fmt = e._prep([0, 1], codes, None, "alaw")
    assert fmt == _ffi.VAD_FMT_ALAW8 and f.dtype == np.uint8 and e._prep([0, 1], codes, None, "ulaw")[2] == _ffi.VAD_FMT_ULAW8
    assert e._prep([0, 1], codes, None)[1].dtype == np.float32            # without `law` a uint8 array means what it meant
    for call in (e.step, e.step_events, e.step_multi, e.submit, e.tick_push_many):
        frames = codes[:, None, :] if call == e.step_multi else codes
        with pytest.raises(AudioProcessingError, match="unknown G.711 law"):
            call([0, 1], frames, law="xyz")
        with pytest.raises(AudioProcessingError, match="must be uint8"):
            call([0, 1], frames.astype(np.float32), law="ulaw")
    with pytest.raises(AudioProcessingError, match="unknown G.711 law"):
        e.tick_push(0, b"\0" * 512, law="mulaw")
    with pytest.raises(AudioProcessingError, match="must be uint8"):
        e.tick_push(0, np.zeros(512, np.float32), law="ulaw")
    with pytest.raises(AudioProcessingError, match="expected"):
        e._prep([0, 1], np.zeros((2, 511), np.uint8), None, "ulaw")       # a row is frame_samples bytes
