#!/usr/bin/env python3
"""pcg_block_bench.py — the device-resident PCG on a block of right-hand sides (amgh_pcg_block_d) against the same columns
solved one after another by the one-column PCG (amgh_pcg_d).  It is a measurement tool and is not part of bench.py.

3-D Poisson 256^3, ruge_stuben defaults, V-cycle preconditioner, reltol 1e-8 (default), bs in {1, 2, 4, 8}.  Column j of
the block is a seeded random vector (the same column for every bs).  B and X stay resident in HBM.  For each bs, in a child
process of its own under a time limit:
  block       one warm-up call (first-use buffers, graph capture), then one timed call of amgh_pcg_block_d: total ms,
              iterations per column, ms per iteration (of the longest column), ms per column-iteration, and the true
              relative residual |b_j - A x_j| / |b_j| of every column computed on the host
  sequential  the same bs columns solved one after another with amgh_pcg_d on a one-column handle (warm-up first):
              total ms, iterations per column, true relative residuals
  speedup     sequential ms / block ms (columns solved per second, block over sequential)

    python tools/pcg_block_bench.py [--bs 1,2,4,8] [--reltol 1e-8] [--out profiles/pcg_block_bench_256.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT_S = 300


def run_one(bs, reltol, m):
    import torch  # noqa: F401  (torch's HIP runtime first, as the test suite does)
    import numpy as np
    import amg_amd as AMG
    t0 = time.perf_counter()
    A = AMG.poisson((m, m, m))
    ml = AMG.ruge_stuben(A)
    As = A.to_scipy()
    t_setup = time.perf_counter() - t0
    n = As.shape[0]
    rng = np.random.default_rng(2026)
    B = np.asfortranarray(rng.standard_normal((n, 8))[:, :bs])
    maxiter = 500
    out = {"problem": "poisson%d" % m, "n": n, "bs": bs, "reltol": reltol, "setup_s": t_setup}

    def true_res(X):
        return [float(np.linalg.norm(B[:, j] - As @ X[:, j]) / np.linalg.norm(B[:, j])) for j in range(bs)]

    # the block
    dev = ml.device(nrhs=bs)
    lib = dev.lib
    bd = AMG.DeviceBuffer(n * bs, 0, B.ravel(order="F"))
    xd = AMG.DeviceBuffer(n * bs, 0, np.zeros(n * bs))
    its = np.zeros(bs, dtype=np.intc)

    def block_call():
        rc = lib.amgh_pcg_block_d(dev.h, bd.ptr, xd.ptr, 0, 1, maxiter, 0.0, reltol, None, 0, its.ctypes.data)
        if rc != 0:
            raise RuntimeError(lib.amgh_strerror(rc).decode())

    block_call()                          # warm-up
    t = time.perf_counter()
    block_call()                          # synchronous on return
    ms = 1e3 * (time.perf_counter() - t)
    X = xd.download().reshape((n, bs), order="F")
    kmax = int(its.max())
    out["block"] = {"ms": ms, "iterations": its.tolist(), "ms_per_iteration": ms / max(1, kmax),
                    "ms_per_column_iteration": ms / max(1, int(its.sum())), "true_rel_residual": true_res(X),
                    "device_bytes": dev.device_bytes()}
    del bd, xd
    # the same columns one after another
    dev1 = ml.device()
    b1 = AMG.DeviceBuffer(n, 0, B[:, 0])
    x1 = AMG.DeviceBuffer(n, 0, np.zeros(n))
    it1 = C.c_int(0)

    def one_call():
        rc = lib.amgh_pcg_d(dev1.h, b1.ptr, x1.ptr, 0, 1, maxiter, 0.0, reltol, None, C.byref(it1))
        if rc != 0:
            raise RuntimeError(lib.amgh_strerror(rc).decode())

    one_call()                            # warm-up
    total, iters, Xs = 0.0, [], np.zeros((n, bs), order="F")
    for j in range(bs):
        b1.upload(B[:, j])
        t = time.perf_counter()
        one_call()
        total += 1e3 * (time.perf_counter() - t)
        iters.append(it1.value)
        Xs[:, j] = x1.download()
    out["sequential"] = {"ms": total, "iterations": iters, "ms_per_iteration": total / max(1, sum(iters)),
                         "true_rel_residual": true_res(Xs)}
    out["speedup"] = total / ms
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="1,2,4,8")
    ap.add_argument("--reltol", type=float, default=1e-8)
    ap.add_argument("--m", type=int, default=256, help="grid points per direction")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_block_bench_256.json"))
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        run_one(a.one, a.reltol, a.m)
        return 0
    results, rc = [], 0
    for bs in (int(s) for s in a.bs.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(bs), "--reltol", str(a.reltol), "--m", str(a.m)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            results.append({"bs": bs, "error": "time limit"})
            rc = 1
            break                        # nothing more on the GPU after a run that did not end
        lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            results.append({"bs": bs, "error": "rc=%d" % r.returncode, "tail": r.stdout.decode(errors="replace")[-2000:]})
            rc = 1
            break                        # a failed GPU child ends the run
        results.append(json.loads(lines[-1][len("RESULT "):]))
        print(json.dumps({k: results[-1][k] for k in ("bs", "speedup")}), flush=True)
    line = json.dumps({"tool": "pcg_block_bench", "results": results})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
