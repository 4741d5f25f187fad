"""Register, scratch, LDS and occupancy figures of the library's kernels, from the compiled device code.

    python tools/kernel_resources.py [--match k3_tile] [--asm dev.s]

Without --asm the device code is compiled to assembly with the product flags (hipcc cross-compiles without a GPU).  One
line per kernel, sorted by name, so two runs can be compared with diff."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics", "-fvisibility=hidden",
         "-fvisibility-inlines-hidden", "--cuda-device-only", "-S"]


def compile_asm(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-o", out, os.path.join(ROOT, "nl-partsol_amd", "csrc", "nlps_gpu.hip")],
                          stderr=subprocess.DEVNULL)


def resources(txt):
    """{kernel name: (vgprs, agprs, scratch bytes, lds bytes, occupancy)} from the comment block behind every kernel"""
    out = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)(?=\.amdhsa_kernel |\Z)", txt, re.S):
        def num(key):
            m = re.search(r";\s*%s:\s*(\d+)" % key, body)
            return int(m.group(1)) if m else -1
        out[name] = (num("NumVgprs"), num("NumAgprs"), num("ScratchSize"), num("LDSByteSize"), num("Occupancy"))
    return out


def demangle(names):
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, p.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--match", action="append", default=[])
    a = ap.parse_args()
    if a.asm:
        txt = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(os.path.join(d, "dev.s"))
            txt = open(os.path.join(d, "dev.s")).read()
    res = resources(txt)
    pretty = demangle(list(res))
    rows = sorted((re.sub(r"\(.*", "", pretty[n]), v) for n, v in res.items())
    for name, (v, ag, sc, lds, occ) in rows:
        if a.match and not any(m in name for m in a.match):
            continue
        print("%-90s vgpr %3d agpr %3d scratch %4d lds %6d occupancy %d" % (name, v, ag, sc, lds, occ))
    return 0


if __name__ == "__main__":
    sys.exit(main())
