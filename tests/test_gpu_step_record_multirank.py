"""The step record on slab ranks (nlps_gpu_set_step_record): two ranks on the one card (gloo and host staging
behind the halo callback, as test_gpu_tangent_operator.py::test_two_ranks_on_one_gpu)."""
import os
import subprocess
import sys

import pytest

from util import ROOT, free_port

pytestmark = pytest.mark.gpu


def test_two_ranks_sums_add_up_to_the_whole_cloud():
    """each rank's row is its share: the sums added and the minima / maxima taken across the ranks are the whole cloud's
    row; reaction totals are refused on a rank handle (tests/mr_gpu_record_worker.py)"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "mr_gpu_record_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "MULTIRANK_RECORD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
