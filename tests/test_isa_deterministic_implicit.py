"""The ISA of the deterministic mode on the implicit path: the one-wave-per-tile forms of the fused
residual, the matrix-free tangent and the level-B scatters exist in the library's device code, the slab gather exists
for their field counts, none of the tile kernels holds a global f64 atomic add (their windows leave as plain slab
copies), and none uses more scratch than the 256-thread kernel it is cut from.  Reads the device assembly tests/isa_asm.py
compiles (the product flags, once per process; hipcc cross-compiles without a GPU)."""
import re

import pytest

import isa_asm

FLUID = 5  # NLPS_KLAW_FLUID


@pytest.mark.timeout(900)
def test_one_wave_forms_exist_without_global_atomics():
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
        hits = [n for n in blocks if re.match(pattern, n)]
        assert len(hits) == 1, f"{what}: {len(hits)} kernels match"
        return hits[0]

    pairs = []  # (one-wave form, its 256-thread sibling)
    # k3_tile<ND, LAW, MODE, FILT, NT, UMAT>
    for nd in (2, 3):
        for law, mode in [(q, 3) for q in range(5)] + [(FLUID, 4)]:
            name = lambda nt: r"_Z7k3_tileILi%dELi%dELi%dELb1ELi%dELb0EE" % (nd, law, mode, nt)  # noqa: E731
            pairs.append((find(name(64), f"k3_tile<{nd}, {law}, {mode}, true, 64, false>"),
                          find(name(256), f"k3_tile<{nd}, {law}, {mode}, true, 256, false>")))
        for stem in ("k_tanop_apply", "k_tanop_bdiag", "kb_fint_tile"):
            name = lambda nt: r"_Z%d%sILi%dELi%dEE" % (len(stem), stem, nd, nt)  # noqa: E731
            pairs.append((find(name(64), f"{stem}<{nd}, 64>"), find(name(256), f"{stem}<{nd}, 256>")))
        for mode in (0, 1):
            name = lambda nt: r"_Z11kb_p2g_tileILi%dELi%dELi%dEE" % (nd, mode, nt)  # noqa: E731
            pairs.append((find(name(64), f"kb_p2g_tile<{nd}, {mode}, 64>"), find(name(256), f"kb_p2g_tile<{nd}, {mode}, 256>")))
        # the slab gather: lumped mass (1), forces / K x (d), nodal field (2 d), diagonal blocks (d^2)
        for nf in sorted({1, nd, 2 * nd, nd * nd}):
            find(r"_Z13k_slab_gatherILi%dELi%dEE" % (nd, nf), f"k_slab_gather<{nd}, {nf}>")
    assert len(pairs) == 2 * (6 + 3 + 2)
    for wave, sibling in pairs:
        body = text(wave)
        assert "s_endpgm" in body, f"{wave}: the text of the kernel was not found whole"
        assert "global_atomic_add_f64" not in body, f"{wave}: a global f64 atomic in the one-wave form"
        assert "global_atomic_add_f64" in text(sibling), f"{sibling}: the check reads the wrong text (the sibling flushes with atomics)"
        assert scratch(wave) <= scratch(sibling), f"{wave}: {scratch(wave)} bytes of scratch, {sibling} {scratch(sibling)}"
