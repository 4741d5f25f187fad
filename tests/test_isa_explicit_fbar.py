"""The ISA of the kernels of the explicit step with F-bar (nlps_gpu_set_explicit_fbar): the kinematic half
k3_kin_tile (k3_tile's MODE 8) in 2-D and 3-D, the stress kernel k_fbar_stress per dimension, law and filter, and the clear
kernel exist exactly once in the library's device code; none uses scratch where its law does not in the level-B stress
kernel; their registers fit the occupancy they are launched for; the kinematic half holds barriers, and none a wave can
skip.  The barrier check is tests/test_isa.py's own, run on the same assembly text (tests/isa_asm.py)."""
import re

import pytest

import isa_asm
import test_isa

# k_fbar_stress<ND, LAW, FILT>: laws 0 .. 5 plain and filtered, and the run-time dispatch (LAW = -1, "n1") unfiltered
STRESS = [(nd, law, filt) for nd in (2, 3) for law in ("0", "1", "2", "3", "4", "5") for filt in (0, 1)] + \
         [(nd, "n1", 0) for nd in (2, 3)]
FRICTIONAL = "4"  # Matsuoka-Nakai / Lade-Duncan: its 5 x 5 Newton system spills in every kernel that holds it


def descriptor(txt, name):
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, re.S)
    assert m, name
    get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, m.group(1)).group(1))  # noqa: E731
    return {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size")}


@pytest.mark.timeout(900)
def test_fbar_kernels_exist_fit_their_occupancy_and_hold_no_skippable_barrier():
    txt = isa_asm.device_asm()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", txt)
    kin = [k for k in kernels if "k3_kin_tile" in k]
    assert len(kin) == 2, kin
    for nd in (2, 3):
        name = [k for k in kin if "k3_kin_tileILi%dEE" % nd in k]
        assert len(name) == 1, name
        d = descriptor(txt, name[0])
        print(name[0], d)
        # launched for two waves per SIMD (K3Waves<ND, -1, 8>): 512 registers a SIMD lane, 256 a wave; 160 KiB of LDS a CU
        assert d["vgpr"] <= 256 and d["scratch"] == 0 and 2 * d["lds"] <= 160 * 1024, d
        body = txt[txt.find("\n" + name[0] + ":"):txt.find(".amdhsa_kernel " + name[0])]
        assert body.count("s_barrier") >= 2, "the window load and the patch flush meet at barriers"
    stress = [k for k in kernels if "k_fbar_stress" in k]
    assert len(stress) == len(STRESS), stress
    for nd, law, filt in STRESS:
        name = [k for k in stress if "k_fbar_stressILi%dELi%sELb%dEE" % (nd, law, filt) in k]
        assert len(name) == 1, (nd, law, filt, name)
        d = descriptor(txt, name[0])
        print(name[0], d)
        assert d["lds"] == 0 and d["vgpr"] <= 256, d
        if law != FRICTIONAL:
            assert d["scratch"] == 0, (name[0], d)
        if law in ("0", "5"):  # the laws that read F-bar: four waves per SIMD and more
            assert d["vgpr"] <= 128, (name[0], d)
    assert len([k for k in kernels if "k_fbar_clear" in k]) == 1
    test_isa.check_no_skippable_barrier(txt)  # the existing check, on the text these kernels were found in
