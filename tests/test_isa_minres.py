"""The ISA of the device MINRES kernels (nl-partsol_amd/csrc/nlps_minres.hpp, prefix k_minres_): they exist in the
library's device code, the node kernel for 2-D and 3-D, and none of them uses scratch memory.  Reads the device assembly
tests/isa_asm.py compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_minres_kernels_exist_and_use_no_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    mr = {name: body for name, body in blocks if "k_minres_" in name}
    assert mr, "no k_minres_ kernel in the device code"
    for stem in ("k_minres_dot", "k_minres_lanczos", "k_minres_rotate", "k_minres_update"):
        assert any(stem in name for name in mr), f"{stem} missing"
    # the node kernel is a template of the dimension: both instantiations (Itanium mangling: ILi2E / ILi3E)
    lanczos = [name for name in mr if "k_minres_lanczos" in name]
    for nd in (2, 3):
        assert any(f"ILi{nd}E" in name for name in lanczos), f"k_minres_lanczos<{nd}> missing: {lanczos}"
    for name, body in mr.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
