"""The ISA of the product kernels: no workgroup barrier that a wave can skip.  An `s_barrier` directly behind an
`s_cbranch_execz` is jumped over by a wave whose exec mask is empty there while its sibling waves execute it -- the
workgroup never meets again (a GPU hang; the first revision of round 3's k_step_fused held one).  Reads the
library's device code as assembly (tests/isa_asm.py: the product flags, one compile per process) and checks every kernel."""
import re

import pytest

import isa_asm


def check_no_skippable_barrier(txt):
    """asserts that no kernel of the assembly text holds an s_barrier directly behind an exec-mask branch"""
    kernels = re.findall(r"\.amdhsa_kernel (\S+)", txt)
    assert len(kernels) > 50
    nbar = 0
    for name in kernels:
        body = [l.strip() for l in txt[txt.find("\n" + name + ":"):txt.find(".amdhsa_kernel " + name)].split("\n")]
        ins = [l for l in body if l and not l.startswith((";", "."))]
        for k, l in enumerate(ins):
            if l.startswith("s_barrier"):
                nbar += 1
                assert k == 0 or not ins[k - 1].startswith(("s_cbranch_execz", "s_cbranch_execnz")), \
                    "%s: s_barrier behind %s" % (name, ins[k - 1])
    assert nbar > 20  # (the tile kernels do hold barriers: the check looked at something)


@pytest.mark.timeout(900)
def test_no_kernel_holds_a_barrier_a_wave_can_skip():
    check_no_skippable_barrier(isa_asm.device_asm())
