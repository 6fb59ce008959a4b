#!/usr/bin/env python3
"""gmres_bench.py — the device-resident restarted GMRES (amgh_gmres_d) on its two workloads.  It is a measurement tool
and is not part of bench.py.

  poisson256   3-D Poisson 256^3, ruge_stuben defaults.  GMRES and, for comparison, PCG (amgh_pcg_d) on the same hierarchy
  cd128, cd256 3-D first-order upwind convection-diffusion (-0.01 Laplacian + (1, 0.6, 0.3) . grad), built with scipy,
               solved on a NoSymmetry ruge_stuben hierarchy

b and x stay resident in HBM.  There is one warm-up call (first-use buffers), then one timed call.  For each problem the
tool reports iterations, total ms, ms per Arnoldi step, the true relative residual |b - A x| / |b| computed on the host,
and the DGKS re-orthogonalisation passes the run took.  Each problem runs in a child process under a time limit of
its own.

    python tools/gmres_bench.py [--problems poisson256,cd128,cd256] [--restart 20] [--reltol 1e-8] [--out profiles/...]
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

LIMIT_S = {"poisson256": 240, "cd128": 120, "cd256": 300}


def upwind3(m, eps=0.01, v=(1.0, 0.6, 0.3)):
    import scipy.sparse as sp
    h = 1.0 / (m + 1)
    I = sp.identity(m, format="csr")
    lap = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m), format="csr") / h**2
    d = sp.diags([-1.0, 1.0], [-1, 0], shape=(m, m), format="csr") / h
    A = None
    for axis in range(3):
        ops = [I, I, I]
        ops[axis] = eps * lap + v[axis] * d
        t = sp.kron(sp.kron(ops[0], ops[1], format="csr"), ops[2], format="csr")
        A = t if A is None else A + t
    return sp.csc_matrix(A)


def run_one(name, restart, reltol):
    import torch  # noqa: F401  (torch's HIP runtime first, as the test suite does)
    import numpy as np
    import amg_amd as AMG
    t0 = time.perf_counter()
    if name == "poisson256":
        A = AMG.poisson((256, 256, 256))
        ml = AMG.ruge_stuben(A)
        As = A.to_scipy()
    else:
        As = upwind3(int(name[2:]))
        ml = AMG.ruge_stuben(As, symmetry=AMG.NoSymmetry())
    t_setup = time.perf_counter() - t0
    n = As.shape[0]
    b = As @ np.ones(n)
    dev = ml.device()
    lib = dev.lib
    bd = AMG.DeviceBuffer(n, 0, b)
    xd = AMG.DeviceBuffer(n, 0, np.zeros(n))
    maxiter = 500
    hist = np.zeros(maxiter + 1)
    its = C.c_int(0)
    out = {"problem": name, "n": n, "restart": restart, "reltol": reltol, "setup_s": t_setup}

    def timed(call):
        rc = call()                      # warm-up (first-use allocations)
        if rc != 0:
            raise RuntimeError(lib.amgh_strerror(rc).decode())
        t = time.perf_counter()
        rc = call()                      # synchronous on return
        ms = 1e3 * (time.perf_counter() - t)
        if rc != 0:
            raise RuntimeError(lib.amgh_strerror(rc).decode())
        x = xd.download()
        return ms, float(np.linalg.norm(b - As @ x) / np.linalg.norm(b))

    ms, res = timed(lambda: lib.amgh_gmres_d(dev.h, bd.ptr, xd.ptr, 0, 1, restart, maxiter, 0.0, reltol, hist.ctypes.data,
                                             C.byref(its)))
    k = its.value
    out["gmres"] = {"iterations": k, "ms": ms, "ms_per_step": ms / max(1, k), "true_rel_residual": res,
                    "estimate_rel": float(hist[k] / hist[0]) if hist[0] else 0.0,
                    "dgks_extra_passes": int(lib.amgh_debug_gmres_reorth(dev.h)), "device_bytes": dev.device_bytes()}
    if name == "poisson256":
        ms, res = timed(lambda: lib.amgh_pcg_d(dev.h, bd.ptr, xd.ptr, 0, 1, maxiter, 0.0, reltol, hist.ctypes.data, C.byref(its)))
        out["pcg"] = {"iterations": its.value, "ms": ms, "ms_per_iteration": ms / max(1, its.value), "true_rel_residual": res}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="poisson256,cd128,cd256")
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--reltol", type=float, default=1e-8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres_bench.json"))
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        run_one(a.one, a.restart, a.reltol)
        return 0
    results, rc = [], 0
    for name in a.problems.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--restart", str(a.restart), "--reltol", str(a.reltol)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=LIMIT_S.get(name, 900))
        except subprocess.TimeoutExpired:
            results.append({"problem": name, "error": "time limit"})
            rc = 1
            break                        # nothing more on the GPU after a run that did not end
        lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            results.append({"problem": name, "error": "rc=%d" % r.returncode, "tail": r.stdout.decode(errors="replace")[-2000:]})
            rc = 1
            break                        # a failed GPU child ends the run
        results.append(json.loads(lines[-1][len("RESULT "):]))
    line = json.dumps({"tool": "gmres_bench", "results": results})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
