"""The ISA of the device GMRES kernels (nl-partsol_amd/csrc/nlps_krylov.hpp, prefix k_ksp_): they exist in the library's
device code and none of them uses scratch memory.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_krylov_kernels_exist_and_use_no_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    ksp = {name: body for name, body in blocks if "k_ksp_" in name}
    assert ksp, "no k_ksp_ kernel in the device code"
    # the streaming kernels, the small-state kernels and the preconditioner ones (2-D and 3-D) are all there
    for stem in ("k_ksp_mdot", "k_ksp_maxpy", "k_ksp_finish", "k_ksp_resid", "k_ksp_scale", "k_ksp_arnoldi", "k_ksp_hsolve",
                 "k_ksp_pc_expand", "k_ksp_update", "k_ksp_pc_build"):
        assert any(stem in name for name in ksp), f"{stem} missing"
    for name, body in ksp.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
