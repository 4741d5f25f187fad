"""The ISA of the CSR assembly kernels (nl-partsol_amd/csrc/nlps_tangent_csr.hpp, prefix k_tancsr_): they exist in the
library's device code, the per-dimension ones twice, none of them holds a floating-point atomic to global memory (the
check tests/test_isa_deterministic_implicit.py makes for its kernels) or to LDS, and none uses scratch memory -- the
resource table of DESIGN.md 5o.  Reads the device assembly tests/isa_asm.py compiles (the product flags, once per
process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm

# scratch bytes and LDS bytes per kernel stem, 2-D and 3-D instance
PER_DIMENSION = {"k_tancsr_setup": ((0, 0), (0, 0)), "k_tancsr_pattern": ((0, 0), (0, 0)), "k_tancsr_rowptr": ((0, 0), (0, 0)),
                 "k_tancsr_rows": ((0, 3568), (0, 20960))}


def _kernels():
    txt = isa_asm.device_asm()
    desc = dict(re.findall(r"\.amdhsa_kernel (\S*k_tancsr_\S*)(.*?)\.end_amdhsa_kernel", txt, re.S))
    bodies = {}
    for name in desc:  # the code of a kernel: from its label to the end of the function
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.S | re.M)
        if m:
            bodies[name] = m.group(1)
    return bodies, desc


@pytest.mark.timeout(900)
def test_csr_kernels_exist_without_float_atomics_or_scratch():
    bodies, desc = _kernels()
    assert desc, "no k_tancsr_ kernel in the device code"
    assert set(bodies) == set(desc), "every kernel descriptor has its code"
    assert sum("k_tancsr_runs" in name for name in desc) == 1
    for stem in PER_DIMENSION:
        assert sum(stem in name for name in desc) == 2, f"{stem}: one instance per dimension"
    assert len(desc) == 1 + 2 * len(PER_DIMENSION)
    for name, body in bodies.items():
        assert len(body) > 100, name
        assert "global_atomic_add_f64" not in body, f"{name}: a float atomic to global memory"
        assert not re.search(r"(global|flat|buffer|ds)_\w*(add|min|max|pk_add)\w*_f(16|32|64)", body), f"{name}: a float atomic"
        assert not re.search(r"_cmpswap", body), f"{name}: a compare-and-swap loop"

    def num(name, key):
        m = re.search(r"\.amdhsa_%s\s+(\d+)" % key, desc[name])
        assert m, f"{name}: no {key}"
        return int(m.group(1))

    for name in desc:
        if "k_tancsr_runs" in name:
            expect = (0, 0)
        else:
            stem = next(s for s in PER_DIMENSION if s in name)
            expect = PER_DIMENSION[stem][1 if "ILi3E" in name else 0]
            assert "ILi3E" in name or "ILi2E" in name, name
        got = (num(name, "private_segment_fixed_size"), num(name, "group_segment_fixed_size"))
        assert got == expect, f"{name}: (scratch, LDS) = {got}, DESIGN.md 5o records {expect}"
