"""The ISA of the step record's kernels (nl-partsol_amd/csrc/nlps_record.hpp, prefix k_rec_): the four exist in the library's
device code and none of them uses scratch memory.  Compiles the device code to assembly with the product flags, as
tests/test_isa_newton.py does (hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_record_kernels_exist_and_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "dev.s")
    subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(ROOT, "nl-partsol_amd", "csrc", "nlps_gpu.hip")], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    rec = {name: body for name, body in blocks if "k_rec_" in name}
    assert rec, "no k_rec_ kernel in the device code"
    for stem in ("k_rec_particles", "k_rec_finish", "k_rec_reactions", "k_rec_probes"):
        assert any(stem in name for name in rec), f"{stem} missing"
    for name, body in rec.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
