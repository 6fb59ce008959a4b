"""Worker of tests/test_dist_pcg_host.py: one rank of a gloo world (CPU, launched by torch.distributed.run).  `amgh_dist_pcg_d`
ITSELF — the recurrence, its all-reduces, the failure flag travelling with them — executed in host memory (device = -1 +
amgh_dist_set_host_tail, the IPC transport's shared-memory rendezvous carrying exchanges and reductions) around the library's
own sharded cycle, against the single-process oracle's pcg and IterativeSolvers' recurrence in numpy.  gloo launches the
ranks, hands out the segment name and gathers the results; the collapsed levels are the oracle's cycle on rank 0.
Bounds as in tests/test_gpu_dist_pcg.py."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import amg_amd as AMG  # noqa: E402
import chebyshev_ref as CR  # noqa: E402
from amg_amd import sharded as SH  # noqa: E402
from conftest import uniform  # noqa: E402
from oracle import oracle as O  # noqa: E402

X_TOL = 1e-9
HIST_TOL = 1e-9


def gather(x_local):
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, x_local)
    return np.concatenate(parts)


def rel(x, y):
    return np.linalg.norm(x - y) / np.linalg.norm(y)


def same_everywhere(hist):
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, hist)
    return all(p.shape == parts[0].shape and np.all(p == parts[0]) for p in parts)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    A = AMG.poisson((14, 12, 10))
    b = uniform(A.m, 5) - 0.3
    tail_of = lambda tail: (lambda bb: O.OracleHierarchy(tail).precond(bb))   # noqa: E731  (one visit of the collapsed levels from x = 0)
    seq = [0]

    def sharded(ml, gs_mode):
        box = ["/amgh_p_%d_%d_%s" % (os.getppid(), seq[0], os.urandom(3).hex())] if rank == 0 else [None]
        seq[0] += 1
        dist.broadcast_object_list(box, src=0)
        return SH.ShardedHierarchy.from_multilevel(ml, rank, world, -1, ("ipc", box[0]), 100, gs_mode=gs_mode, host_tail=tail_of)

    jac = AMG.Jacobi(2.0 / 3.0, iter=2)
    for name, ml in (("jacobi", AMG.ruge_stuben(A, presmoother=jac, postsmoother=jac)), ("gauss-seidel", AMG.ruge_stuben(A))):
        sh = sharded(ml, "exact")
        assert sh.lc >= 2 and sh.host_exec
        bl = b[sh.r0:sh.r1]
        sh.stats()
        x_loc, hist = sh.cg(bl, reltol=1e-10, log=True)
        xo, ho, ito = O.OracleHierarchy(ml).pcg(b, reltol=1e-10)
        x = gather(x_loc)
        err_h = float(np.max(np.abs(hist - ho) / ho)) if len(hist) == len(ho) else None
        if rank == 0:
            print("DIST_PCG", name, world, "iters", len(hist) - 1, ito, "x", rel(x, xo), "hist", err_h)
        assert len(hist) - 1 == ito, (name, len(hist) - 1, ito)
        assert err_h <= HIST_TOL and rel(x, xo) <= X_TOL, (name, err_h, rel(x, xo))
        assert same_everywhere(hist)
        assert sh.stats()["halo_exchanges"] > 0
        assert np.array_equal(sh.cg(bl, reltol=1e-10), x_loc)                 # (no log: x alone; a second call: the same bits)
        if name == "jacobi":
            # plain CG: IterativeSolvers' recurrence in numpy on the level-0 operator
            xr, hr, itr = CR.pcg(ml.levels[0].A.to_scipy(), b, Pl=lambda r: r, reltol=1e-8)
            x_loc, hist = sh.cg(bl, use_precond=False, reltol=1e-8, log=True)
            assert len(hist) - 1 == itr and rel(gather(x_loc), xr) <= 1e-9, (len(hist) - 1, itr)
            assert same_everywhere(hist)
            # maxiter = 0 and b = 0
            x_loc, hist = sh.cg(bl, maxiter=0, log=True)
            assert np.all(x_loc == 0.0) and len(hist) == 1 and abs(hist[0] - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b)
            x_loc, hist = sh.cg(np.zeros_like(bl), log=True)
            assert np.all(x_loc == 0.0) and hist.tolist() == [0.0]
            # argument checks, the same on every rank (nothing collective has started when they return)
            it = SH.C.c_int(0)
            assert sh.lib.amgh_dist_pcg_d(sh.h, sh._b.ptr, sh._x.ptr, 3, 1, 5, 0.0, 1e-8, None, SH.C.byref(it)) == -2
            assert sh.lib.amgh_dist_pcg_d(sh.h, sh._b.ptr, sh._x.ptr, 0, 1, -1, 0.0, 1e-8, None, SH.C.byref(it)) == -2
        sh.close()
    dist.barrier()
    if rank == 0:
        print("DIST_PCG_HOST_WORKER_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
