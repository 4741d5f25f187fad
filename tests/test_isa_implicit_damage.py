"""The ISA of the kernels of the fused damage residual (nlps_gpu_set_implicit_damage): the state half of
MODE 3 (k3_tile<., ., 6, ...>) exists in the launch forms the residual's call site has -- plain per dimension and law,
per-law (FILT), and the one-material form (UMAT) of the 3-D laws 1-3 -- and uses no more than a few registers' worth of
scratch beyond the fused residual kernel of the same law, which it is cut from; both force halves (k3f_tile<ND, false>, the
explicit step's, and k3f_tile<ND, true>, the residual's) use no scratch.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm

# what a state half may spill beyond its fused sibling: eight 4-byte registers per lane (tests/test_isa_explicit_damage.py)
STATE_HALF_EXTRA_SCRATCH = 32


@pytest.mark.timeout(900)
def test_fused_damage_residual_kernels_exist_and_scratch():
    txt = isa_asm.device_asm()
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)

    def scratch(name, body):
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert m, f"{name}: no private segment size"
        return int(m.group(1))

    # k3f_tile<ND, PLUS>: false = the explicit step's, true = the residual's
    k3f = {}
    for name, body in blocks:
        m = re.match(r"_Z8k3f_tileILi(\d)ELb([01])EE", name)
        if m:
            k3f[(m.group(1), m.group(2))] = scratch(name, body)
    for nd in ("2", "3"):
        for plus in ("0", "1"):
            assert (nd, plus) in k3f, f"k3f_tile {nd}-D {'sign +1' if plus == '1' else 'sign -1'} missing"
    for k, v in k3f.items():
        assert v == 0, f"k3f_tile{k}: {v} bytes of scratch"
    # k3_tile<ND, LAW, MODE, FILT, NT, UMAT>
    k3 = {}
    for name, body in blocks:
        m = re.match(r"_Z7k3_tileILi(\d)ELi(n?\d)ELi(\d)ELb([01])ELi(\d+)ELb([01])EE", name)
        if m:
            k3[tuple(m.groups())] = scratch(name, body)
    state = {k: v for k, v in k3.items() if k[2] == "6"}
    want = [(nd, law, "6", filt, "256", "0") for nd in ("2", "3") for law in "01234" for filt in "01"]
    want += [("3", law, "6", "0", "256", "1") for law in "123"]
    for k in want:
        assert k in state, f"state half of the residual {k} missing"
    assert sorted(state) == sorted(want), "no slab, 64-thread or dispatch form of the state half"
    for k, v in sorted(state.items()):
        sibling = k3[(k[0], k[1], "3", k[3], k[4], k[5])]
        print(f"k3_tile{k}: scratch {v}, MODE 3 sibling {sibling}")
        assert v <= sibling + STATE_HALF_EXTRA_SCRATCH, f"k3_tile{k}: {v} bytes of scratch, the fused residual kernel {sibling}"
