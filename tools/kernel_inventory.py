#!/usr/bin/env python3
"""Developer tool: which kernels a tree compiles to, and whether a host-side refactor left every one of them alone.

    hipcc <the flags of tests/test_isa.py> --cuda-device-only -S -o new.s nl-partsol_amd/csrc/nlps_gpu.hip
    python tools/kernel_inventory.py new.s              one line per kernel: name, hash, instructions, VGPRs, SGPRs, scratch, LDS
    python tools/kernel_inventory.py old.s new.s        exit 0 if every kernel of new.s is in old.s unchanged; lists the rest

The hash is taken over the instruction lines between `NAME:` and the kernel descriptor, comments and directives dropped
and the function index taken out of block labels (.LBB<n>_<k> -> .LBB_<k>), so kernels that appear or vanish elsewhere in
the file do not disturb it."""
import hashlib
import re
import sys


def inventory(path):
    txt = open(path).read()
    inv = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        name, meta = m.group(1), m.group(2)
        ins = []
        for line in txt[txt.find("\n" + name + ":"):txt.find(".amdhsa_kernel " + name)].split("\n")[2:]:
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not re.match(r"\.LBB\d+_\d+:", line)):
                continue
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        fig = [re.search(r"\.amdhsa_%s (\S+)" % k, meta).group(1) for k in
               ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")]
        inv[name] = (hashlib.sha1("\n".join(ins).encode()).hexdigest()[:16], len(ins), *fig)
    return inv


if __name__ == "__main__":
    new = inventory(sys.argv[-1])
    if len(sys.argv) == 2:
        for name in sorted(new):
            print(name, *new[name])
        sys.exit(0)
    old = inventory(sys.argv[1])
    added = sorted(k for k in new if k not in old)
    changed = sorted(k for k in new if k in old and new[k] != old[k])
    removed = sorted(k for k in old if k not in new)
    print("kernels: %d -> %d; %d identical, %d changed, %d new, %d removed" % (
        len(old), len(new), len(new) - len(added) - len(changed), len(changed), len(added), len(removed)))
    for tag, names in (("changed", changed), ("new", added), ("removed", removed)):
        for k in names:
            print(tag, k, *(old[k] if tag == "removed" else new[k]))
    sys.exit(1 if added or changed else 0)
