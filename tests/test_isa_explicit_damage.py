"""The ISA of the kernels of the explicit step with the damage hooks: they exist in the library's device
code, the list, roll and force kernels use no scratch memory, and the state half of K3 (k3_tile<., ., 5, ...>) uses no
more than a few registers' worth beyond the fused kernel of the same law, which it is cut from (it stores tau and W on
top).  The barrier check of tests/test_isa.py covers every kernel, these included.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm

# what the state half may spill beyond its fused sibling: eight 4-byte registers per lane
STATE_HALF_EXTRA_SCRATCH = 32


@pytest.mark.timeout(900)
def test_damage_step_kernels_exist_and_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)

    def scratch(name, body):
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        return int(m.group(1))

    for stem in ("k3f_tile", "k_run_count", "k_run_first", "k_run_fill", "k_damage_roll"):
        mine = [(name, body) for name, body in blocks if stem in name]
        assert mine, f"{stem} missing"
        for name, body in mine:
            assert scratch(name, body) == 0, f"{name}: {scratch(name, body)} bytes of scratch"
    # k3_tile<ND, LAW, MODE, FILT, NT, UMAT>
    k3 = {}
    for name, body in blocks:
        m = re.match(r"_Z7k3_tileILi(\d)ELi(n?\d)ELi(\d)ELb([01])ELi(\d+)ELb([01])EE", name)
        if m:
            k3[tuple(m.groups())] = scratch(name, body)
    state = {k: v for k, v in k3.items() if k[2] == "5"}
    assert len(state) >= 20, "the state half exists per dimension and law, plain and per-law (FILT)"
    for nd in ("2", "3"):
        for law in ("0", "1", "2", "3", "4", "n1"):
            assert (nd, law, "5", "0", "256", "0") in state, f"state half {nd}-D law {law} missing"
    for k, v in state.items():
        sibling = k3[(k[0], k[1], "1", k[3], k[4], k[5])]
        assert v <= sibling + STATE_HALF_EXTRA_SCRATCH, f"k3_tile{k}: {v} bytes of scratch, the fused kernel {sibling}"
