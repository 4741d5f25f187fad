"""The ISA of the deterministic mode for clouds with the damage hooks (nlps_gpu_set_deterministic_damage):
the one-wave force half k3f_wave<ND, PLUS> exists for both dimensions and both signs, holds no global f64 atomic add (its
window leaves as a plain slab copy) while k3f_tile of the same dimension and sign does, and uses no scratch; the run sort
k_run_sort exists and uses no scratch.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm


@pytest.mark.timeout(900)
def test_one_wave_force_half_and_run_sort():
    txt = isa_asm.device_asm()
    blocks = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S))

    def scratch(name):
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", blocks[name])
        assert m, f"{name}: no private segment size"
        return int(m.group(1))

    def text(name):
        """the instructions of a kernel: from its label to the end of its function"""
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.S | re.M)
        assert m, f"{name}: no code"
        return m.group(1)

    def find(pattern, what):
        hits = [n for n in blocks if re.fullmatch(pattern, n)]
        assert len(hits) == 1, f"{what}: {len(hits)} kernels match"
        return hits[0]

    for nd in (2, 3):
        for plus in (0, 1):
            wave = find(r"_Z8k3f_waveILi%dELb%dEEv.*" % (nd, plus), f"k3f_wave<{nd}, {bool(plus)}>")
            tile = find(r"_Z8k3f_tileILi%dELb%dEEv.*" % (nd, plus), f"k3f_tile<{nd}, {bool(plus)}>")
            body = text(wave)
            assert "s_endpgm" in body, f"{wave}: the text of the kernel was not found whole"
            assert "global_atomic_add_f64" not in body, f"{wave}: a global f64 atomic in the one-wave force half"
            assert "global_atomic_add_f64" in text(tile), f"{tile}: the check reads the wrong text (k3f_tile flushes with atomics)"
            assert "ds_add_f64" in body or "ds_add_rtn_f64" in body, f"{wave}: no LDS accumulation"
            assert scratch(wave) == 0, f"{wave}: {scratch(wave)} bytes of scratch"
            m = re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", blocks[wave])
            assert m and int(m.group(1)) == int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", blocks[tile]).group(1)), \
                f"{wave}: another window than k3f_tile's"
    sort = find(r"_Z10k_run_sort.*", "k_run_sort")
    assert scratch(sort) == 0, f"{sort}: {scratch(sort)} bytes of scratch"
    assert "s_endpgm" in text(sort)
    for stem in ("k_run_count", "k_run_first", "k_run_fill"):
        assert stem not in sort
