#!/usr/bin/env python3
"""dist_pcg_bench.py — the device-resident PCG of a row-sharded hierarchy (amgh_dist_pcg_d) beside its two building blocks.
It is a measurement tool and is not part of bench.py.

3-D Poisson size^3 (default 256), ruge_stuben defaults, exact Gauss-Seidel across the shards (the library's default), N
VIRTUAL ranks of the LOCAL transport: threads of one process sharing ONE GPU.  That is an arrangement for tests and for
this measurement — the ranks' kernels take turns on the one device and every exchange is a device-to-device copy behind
a host rendezvous — so the figures say what an iteration costs OVER its cycle and its SpMV on the same handles in the
same process, not how the iteration scales; more than one device has not been available to this project.

Per rank count, on the same handles, every window closed by a barrier and the maximum over the ranks taken:
  cycle_ms        amgh_dist_precond_apply_d, mean of `reps` calls after warm-up
  spmv_ms         amgh_dist_spmv_d on the fine level, mean of `reps` calls after warm-up
  pcg             amgh_dist_pcg_d to reltol (x0 = 0): one warm-up call (first-use buffers), one timed call: iterations, seconds,
                  ms per iteration, the overhead of an iteration over cycle_ms + spmv_ms, the true relative residual
                  |b - A x| / |b| of the assembled x computed on the host
  solve           amgh_dist_solve_d (the stationary iteration) to the same reltol, timed the same way: cycles, seconds

    python tools/dist_pcg_bench.py [--size 256] [--ranks 2,4] [--reltol 1e-8] [--reps 10] [--out profiles/dist_pcg_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(ml, As, b, nranks, reltol, reps, shard_min_rows):
    import numpy as np
    from amg_amd import sharded as SH

    def work(rank, group):
        t0 = time.perf_counter()
        sh = SH.ShardedHierarchy.from_multilevel(ml, rank, nranks, 0, ("local", group), shard_min_rows)
        shard_s = time.perf_counter() - t0
        bl = b[sh.r0:sh.r1]

        def window(call, n):
            sh.barrier()
            t = time.perf_counter()
            for _ in range(n):
                call()
            sh.barrier()                                   # (sync + barrier: the enqueued work has run on every rank)
            return float(sh.allreduce([time.perf_counter() - t], "max")[0]) / n

        sh.set_rhs(bl)
        window(lambda: sh.precond_apply_d(0), 2)
        cycle_ms = 1e3 * window(lambda: sh.precond_apply_d(0), reps)
        spmv = lambda: sh.lib.amgh_dist_spmv_d(sh.h, 0, None, sh._x.ptr)   # noqa: E731  (the level's resident x, as bench_dist.py times it)
        window(spmv, 2)
        spmv_ms = 1e3 * window(spmv, reps)
        res = {}
        sh.cg(bl, reltol=reltol, maxiter=200)              # warm-up: first-use buffers
        sh.stats()
        res["t_pcg"] = window(lambda: res.__setitem__("pcg", sh.cg(bl, reltol=reltol, maxiter=200, log=True)), 1)
        st = sh.stats()
        sh.solve(bl, reltol=reltol, maxiter=3)              # warm-up
        res["t_solve"] = window(lambda: res.__setitem__("solve", sh.solve(bl, reltol=reltol, maxiter=100)), 1)
        out = dict(cycle_ms=cycle_ms, spmv_ms=spmv_ms, shard_s=shard_s, lc=sh.lc, pipelined=sh.gs_pipelined(), stats=st, **res)
        sh.barrier()
        sh.close()
        return out

    res = SH.run_local_ranks(nranks, work)
    r0 = res[0]
    x = np.concatenate([r["pcg"][0] for r in res])
    hist = r0["pcg"][1]
    its = len(hist) - 1
    xs = np.concatenate([r["solve"][0] for r in res])
    hs = r0["solve"][1]
    nb = float(np.linalg.norm(b))
    ms_it = 1e3 * r0["t_pcg"] / max(1, its)
    return {
        "ranks": nranks, "sharded_levels": r0["lc"], "gs_pipelined": r0["pipelined"], "shard_s": max(r["shard_s"] for r in res),
        "cycle_ms": r0["cycle_ms"], "spmv_ms": r0["spmv_ms"],
        "pcg": {"iterations": its, "seconds": r0["t_pcg"], "ms_per_iteration": ms_it,
                "overhead_ms_over_cycle_plus_spmv": ms_it - r0["cycle_ms"] - r0["spmv_ms"],
                "overhead_fraction": (ms_it - r0["cycle_ms"] - r0["spmv_ms"]) / (r0["cycle_ms"] + r0["spmv_ms"]),
                "recurrence_rel_residual": float(hist[-1] / hist[0]) if hist[0] else 0.0,
                "true_rel_residual": float(np.linalg.norm(b - As @ x) / nb),
                "halo_exchanges_per_iteration": r0["stats"]["halo_exchanges"] / max(1, its)},
        "solve": {"cycles": len(hs) - 1, "seconds": r0["t_solve"], "ms_per_cycle": 1e3 * r0["t_solve"] / max(1, len(hs) - 1),
                  "true_rel_residual": float(np.linalg.norm(b - As @ xs) / nb)},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ranks", default="2,4")
    ap.add_argument("--reltol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shard-min-rows", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_pcg_bench.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch's HIP runtime first, as the test suite does)
    import numpy as np
    import amg_amd as AMG
    if not AMG.gpu_available():
        raise SystemExit("dist_pcg_bench: no HIP device visible (a measurement needs the GPU)")
    t0 = time.perf_counter()
    A = AMG.poisson((a.size,) * 3)
    ml = AMG.ruge_stuben(A)
    setup_s = time.perf_counter() - t0
    As = A.to_scipy()
    b = As @ np.ones(A.m)
    results = []
    for nranks in [int(s) for s in a.ranks.split(",")]:
        results.append(measure(ml, As, b, nranks, a.reltol, a.reps, a.shard_min_rows))
        print("# " + json.dumps(results[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"tool": "dist_pcg_bench", "problem": "poisson %d^3, ruge_stuben defaults" % a.size, "n": A.m,
                       "arrangement": "virtual ranks: threads of one process on ONE GPU (LOCAL transport)", "reltol": a.reltol,
                       "reps": a.reps, "host_setup_s": setup_s, "results": results})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
