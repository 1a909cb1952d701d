"""GPU test: bk_flow_create and bk_shooting_create on a two-rank context (both ranks on cuda:0 through the host-staged communicator,
as tests/test_distributed.py runs them) return their "single rank" message and leave the context usable
(tests/shooting_ranks_worker.py)."""
import os
import subprocess
import sys

import pytest

from test_distributed import ROOT, _free_port

pytestmark = pytest.mark.gpu


def test_flow_and_shooting_refuse_two_ranks():
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PYTHONPATH=ROOT,
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "shooting_ranks_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("the two ranks did not finish within 120 s")
        outs.append(o)
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
        assert "shooting rank checks OK" in o, o[-2000:]
