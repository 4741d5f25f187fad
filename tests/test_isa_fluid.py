"""The ISA of the fluid law's kernels: the rate-carrying residual instantiations of k3_tile (MODE 4, 2-D and 3-D, with and
without the per-law filter) and k_expand_reset_rates exist in the library's device code, and none of them holds a workgroup
barrier that a wave can skip.  The barrier check is tests/test_isa.py's own, run on the same assembly text
(tests/isa_asm.py); what this file adds is that the new instantiations are among the kernels it looked at."""
import re

import pytest

import isa_asm
import test_isa

# k3_tile<ND, NLPS_KLAW_FLUID = 5, MODE = 4, FILT, 256, false>
FLUID_K3 = [r"k3_tileILi%dELi5ELi4ELb%dELi256ELb0EE" % (nd, filt) for nd in (2, 3) for filt in (0, 1)]


@pytest.mark.timeout(900)
def test_fluid_kernels_exist_and_hold_no_skippable_barrier():
    txt = isa_asm.device_asm()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", txt)
    for pat in FLUID_K3 + ["k_expand_reset_rates"]:
        hits = [k for k in kernels if re.search(pat, k)]
        assert len(hits) == 1, f"{pat}: {hits}"
        if "k3_tile" in pat:  # the tile kernels do hold barriers: the check below has something to look at
            name = hits[0]
            body = txt[txt.find("\n" + name + ":"):txt.find(".amdhsa_kernel " + name)]
            assert "s_barrier" in body, name
    test_isa.check_no_skippable_barrier(txt)  # the existing check, on the text these kernels were found in
