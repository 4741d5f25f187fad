"""The ISA of the device Lanczos kernels (nl-partsol_amd/csrc/nlps_eigen.hpp, prefix k_eig_): they exist in the library's
device code and none of them uses scratch memory.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_eigen_kernels_exist_and_use_no_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    eig = {name: body for name, body in blocks if "k_eig_" in name}
    assert eig, "no k_eig_ kernel in the device code"
    # the start vector, the folded expansion and the nodal epilogue (2-D and 3-D), the one-wave Ritz kernel, the closing two
    for stem in ("k_eig_start", "k_eig_expand", "k_eig_nodal", "k_eig_ritz", "k_eig_ritzvec", "k_eig_resid"):
        assert any(stem in name for name in eig), f"{stem} missing"
    for stem in ("k_eig_expand", "k_eig_nodal"):
        assert sum(stem in name for name in eig) == 2, f"{stem}: one instance per dimension"
    for name, body in eig.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
    # the Ritz kernel is one wave with T, the pivots and the vector in LDS: 6 arrays of 256 doubles
    m = re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", next(b for nm, b in eig.items() if "k_eig_ritz" in nm and "vec" not in nm))
    assert m and int(m.group(1)) == 6 * 256 * 8
