"""The ISA of the fluid law's kernels: the rate-carrying residual instantiations of k3_tile (MODE 4, 2-D and 3-D, with and
without the per-law filter) and k_expand_reset_rates exist in the library's device code, and none of them holds a workgroup
barrier that a wave can skip.  The barrier check is tests/test_isa.py's own, run on the assembly compiled here (hipcc
cross-compiles without a GPU; its compile is skipped only if it is this one to the letter); what this file adds is that the
new instantiations are among the kernels it looked at."""
import os
import re
import subprocess

import pytest

import test_isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# k3_tile<ND, NLPS_KLAW_FLUID = 5, MODE = 4, FILT, 256, false>
FLUID_K3 = [r"k3_tileILi%dELi5ELi4ELb%dELi256ELb0EE" % (nd, filt) for nd in (2, 3) for filt in (0, 1)]


@pytest.mark.timeout(900)
def test_fluid_kernels_exist_and_hold_no_skippable_barrier(tmp_path, monkeypatch):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "dev.s")
    mine = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
            "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--cuda-device-only", "-S", "-o", out,
            os.path.join(ROOT, "nl-partsol_amd", "csrc", "nlps_gpu.hip")]
    subprocess.check_call(mine, stderr=subprocess.DEVNULL)
    txt = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", txt)
    for pat in FLUID_K3 + ["k_expand_reset_rates"]:
        hits = [k for k in kernels if re.search(pat, k)]
        assert len(hits) == 1, f"{pat}: {hits}"
        if "k3_tile" in pat:  # the tile kernels do hold barriers: the check below has something to look at
            name = hits[0]
            body = txt[txt.find("\n" + name + ":"):txt.find(".amdhsa_kernel " + name)]
            assert "s_barrier" in body, name
    # the existing check on the assembly of this compile: its own compile is skipped only when it asks for exactly what
    # was compiled above (same command line, same output file); anything else runs as it is
    real = subprocess.check_call
    monkeypatch.setattr(test_isa.subprocess, "check_call",
                        lambda cmd, *a, **k: 0 if list(cmd) == mine else real(cmd, *a, **k))
    test_isa.test_no_kernel_holds_a_barrier_a_wave_can_skip(tmp_path)
