"""The ISA of the Newton solve's kernels (nl-partsol_amd/csrc/nlps_newton.hpp, prefix k_snes_): they exist in the library's
device code and none of them uses scratch memory.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_newton_kernels_exist_and_use_no_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    snes = {name: body for name, body in blocks if "k_snes_" in name}
    assert snes, "no k_snes_ kernel in the device code"
    for stem in ("k_snes_trial", "k_snes_dots", "k_snes_finish"):
        assert any(stem in name for name in snes), f"{stem} missing"
    for name, body in snes.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
