"""The ISA of the snapshot's pack kernel (nl-partsol_amd/csrc/nlps_snapshot.hpp, prefix k_snap_): it exists in the library's
device code in both dimensions and both mappings and uses no scratch memory.  Reads the device assembly tests/isa_asm.py compiles (the
product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_snapshot_kernels_exist_and_use_no_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)
    snap = {name: body for name, body in blocks if "k_snap_" in name}
    assert snap, "no k_snap_ kernel in the device code"
    for stem in ("k_snap_packILi2ELb0E", "k_snap_packILi2ELb1E", "k_snap_packILi3ELb0E", "k_snap_packILi3ELb1E"):
        assert any(stem in name for name in snap), f"{stem} missing"
    for name, body in snap.items():
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        assert int(m.group(1)) == 0, f"{name}: {m.group(1)} bytes of scratch"
