"""`amgh_dist_pcg_d` without a GPU: gloo worlds of 2 and 3 ranks run the library's own recurrence in host memory around its own
sharded cycle (tests/dist_pcg_host_worker.py) against the oracle's pcg; a plans-only handle refuses."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import amg_amd as AMG
from amg_amd import sharded as SH
from conftest import ROOT


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


@pytest.mark.parametrize("nranks", [2, 3])
def test_gloo_drives_the_library_sharded_pcg_on_the_host(nranks):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", AMGH_IPC_TIMEOUT_S="120")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nranks}",
           "--master-addr", "127.0.0.1", "--master-port", free_port(), os.path.join(ROOT, "tests", "dist_pcg_host_worker.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode()
    assert r.returncode == 0 and "DIST_PCG_HOST_WORKER_OK" in out, (nranks, out[-4000:])


def test_a_plans_only_handle_has_no_cg():
    ml = AMG.ruge_stuben(AMG.poisson((8, 8, 6)))
    name = "/amgh_pp_%d_%s" % (os.getpid(), os.urandom(3).hex())
    sh = SH.ShardedHierarchy.from_multilevel(ml, 0, 1, -1, ("ipc", name), 100)
    try:
        assert sh.plans_only
        with pytest.raises(AMG.AMGError):
            sh.cg(np.ones(sh.nloc))
    finally:
        sh.close()
