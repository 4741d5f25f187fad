"""The ISA of the block-CSR assembly kernels (nl-partsol_amd/csrc/nlps_tangent_bsr.hpp, prefix k_tanbsr_), as
tests/test_isa_tangent_csr.py does for the CSR ones: they exist in the library's device code, once per dimension (the
row kernel once per dimension and form), none of them holds a floating-point atomic to global memory or to LDS, and
none uses scratch memory -- the resource table of DESIGN.md 5p.  Reads the device assembly tests/isa_asm.py compiles."""
import re

import pytest

import isa_asm

# instances per dimension: the count kernel; the row kernel walking every member (false) and the kept half (true)
PER_DIMENSION = {"k_tanbsr_count": 1, "k_tanbsr_rows": 2}


def _kernels():
    txt = isa_asm.device_asm()
    desc = dict(re.findall(r"\.amdhsa_kernel (\S*k_tanbsr_\S*)(.*?)\.end_amdhsa_kernel", txt, re.S))
    bodies = {}
    for name in desc:  # the code of a kernel: from its label to the end of the function
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.S | re.M)
        if m:
            bodies[name] = m.group(1)
    return bodies, desc


@pytest.mark.timeout(900)
def test_bsr_kernels_exist_without_float_atomics_or_scratch():
    bodies, desc = _kernels()
    assert desc, "no k_tanbsr_ kernel in the device code"
    assert set(bodies) == set(desc), "every kernel descriptor has its code"
    for stem, per_dim in PER_DIMENSION.items():
        for dim in ("ILi2E", "ILi3E"):
            assert sum(stem in name and dim in name for name in desc) == per_dim, f"{stem}: instances of {dim}"
    assert sum("k_tanbsr_rows" in name and name.count("Lb1E") == 1 for name in desc) == 2, "the half walk, once per dimension"
    assert len(desc) == 2 * sum(PER_DIMENSION.values())
    for name, body in bodies.items():
        assert len(body) > 100, name
        assert "global_atomic_add_f64" not in body, f"{name}: a float atomic to global memory"
        assert not re.search(r"(global|flat|buffer|ds)_\w*(add|min|max|pk_add)\w*_f(16|32|64)", body), f"{name}: a float atomic"
        assert not re.search(r"_cmpswap", body), f"{name}: a compare-and-swap loop"
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc[name])
        assert m and int(m.group(1)) == 0, f"{name}: scratch"
