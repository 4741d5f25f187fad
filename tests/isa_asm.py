"""The device assembly of the library, for the tests/test_isa*.py files: nl-partsol_amd/csrc/nlps_gpu.hip compiled with the
product flags (hipcc cross-compiles without a GPU), once per process however many tests read it."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nl-partsol_amd", "csrc", "nlps_gpu.hip")
# the product flags of nl-partsol_amd/build.py that decide the device code, and "device assembly only"
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
         "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--cuda-device-only", "-S"]
_text = None


def device_asm():
    """The assembly text of every kernel of the library; skips the calling test where there is no hipcc."""
    global _text
    if _text is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc")
        with tempfile.TemporaryDirectory(prefix="nlps_isa_") as tmp:
            out = os.path.join(tmp, "dev.s")
            subprocess.check_call([hipcc] + FLAGS + ["-o", out, SRC], stderr=subprocess.DEVNULL)
            with open(out) as f:
                _text = f.read()
    return _text
