"""The ISA of the step record's kernels (nl-partsol_amd/csrc/nlps_record.hpp, prefix k_rec_): the four exist in the library's
device code and none of them uses scratch memory.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_record_kernels_exist_and_use_no_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    rec = {name: body for name, body in blocks if "k_rec_" in name}
    assert rec, "no k_rec_ kernel in the device code"
    for stem in ("k_rec_particles", "k_rec_finish", "k_rec_reactions", "k_rec_probes"):
        assert any(stem in name for name in rec), f"{stem} missing"
    for name, body in rec.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
