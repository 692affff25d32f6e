"""The launch shape of the paired 16-stream kernel (cutter_vad_amd/csrc/silero_v5_t16.hip: silero_v5_pair16; engine.cpp: launch()),
from the code object's own metadata: ONE workgroup of 512 threads per CU - eight waves, two per SIMD - so each wave may have at most
256 registers and must not spill (scratch would put the weight ring in memory), and the two halves' LDS must fit the CU's 160 KiB.
The unpaired single-frame entries the engine keeps for calls of at most one tile per CU must still be there.  Compiled to assembly
for gfx950 with the product's flags; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_paired_entries_fit_one_workgroup_of_eight_waves_on_a_cu(tmp_path):
    from cutter_vad_amd import _build
    out = tmp_path / "t16.s"
    flags = ["-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-amdgpu-kernarg-preload-count=8"]
    subprocess.run([_hipcc(), f"--offload-arch={_build.ARCH}", *flags, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "cutter_vad_amd", "csrc", "silero_v5_t16.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for entry in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        field = lambda k: int(re.search(r"\.%s:\s*(\d+)" % k, entry).group(1))
        kernels[re.search(r"\.name:\s*(\S+)", entry).group(1)] = {
            "lds": field("group_segment_fixed_size"), "regs": field("vgpr_count"), "scratch": field("private_segment_fixed_size"),
            "spill": field("vgpr_spill_count"), "threads": field("max_flat_workgroup_size")}
    # _Z16silero_v5_pair16ILb<F32IN>EEv...
    pair = {k: v for k, v in kernels.items() if re.match(r"_Z16silero_v5_pair16ILb[01]EE", k)}
    assert len(pair) == 2, sorted(kernels)
    for name, m in pair.items():
        assert m["regs"] <= 256, (name, m)
        assert m["scratch"] == 0 and m["spill"] == 0, (name, m)
        assert m["lds"] <= 160 * 1024, (name, m)
        assert m["threads"] == 512, (name, m)
    one = [k for k in kernels if re.match(r"_Z16silero_v5_step16ILb[01]ELb0ELb[01]ELb1EE", k)]
    assert len(one) == 4, sorted(kernels)
