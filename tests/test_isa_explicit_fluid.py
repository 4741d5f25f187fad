"""The ISA of the explicit step's fluid kernels (nlps_gpu_set_explicit_fluid): the MODE 7 instantiations of
k3_tile -- 2-D and 3-D, plain and with the per-law filter at 256 threads, and the one-wave filter form of the
deterministic mode -- exist exactly once in the library's device code, the 256-thread forms hold a barrier, and none holds
one that a wave can skip.  The barrier check is tests/test_isa.py's own, run on the same assembly text (tests/isa_asm.py)."""
import re

import pytest

import isa_asm
import test_isa

# k3_tile<ND, NLPS_KLAW_FLUID = 5, MODE = 7, FILT, NT, false, 0>: the overload that takes dt
FLUID_K3 = [(r"k3_tileILi%dELi5ELi7ELb%dELi%dELb0E" % (nd, filt, nt), nt)
            for nd in (2, 3) for filt, nt in ((0, 256), (1, 256), (1, 64))]


@pytest.mark.timeout(900)
def test_explicit_fluid_kernels_exist_and_hold_no_skippable_barrier():
    txt = isa_asm.device_asm()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", txt)
    assert len([k for k in kernels if "k3_tileILi" in k and "ELi5ELi7E" in k]) == len(FLUID_K3), "MODE 7: these six, nothing else"
    for pat, nt in FLUID_K3:
        hits = [k for k in kernels if re.search(pat, k)]
        assert len(hits) == 1, f"{pat}: {hits}"
        name = hits[0]
        assert name.endswith("Pid"), f"{name}: the last argument is dt"
        if nt == 256:  # (the check below has something to look at)
            body = txt[txt.find("\n" + name + ":"):txt.find(".amdhsa_kernel " + name)]
            assert "s_barrier" in body, name
    test_isa.check_no_skippable_barrier(txt)  # the existing check, on the text these kernels were found in
