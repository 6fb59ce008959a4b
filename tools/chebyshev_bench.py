#!/usr/bin/env python3
"""The Chebyshev polynomial smoother beside the other smoothers on ONE hierarchy — ruge_stuben(poisson((N,N,N)), setup="gpu"),
only the smoothers changed — in one process:
  1. one fine-level Chebyshev step, one Jacobi sweep, one value-coded residual pass: time and achieved bytes/s from the
     algorithmic bytes of each, as fractions of the read rate a dot product of two fine vectors reaches in this run;
  2. V-cycle time and cg time to reltol = 1e-8 (iterations x time) for symmetric Gauss-Seidel, Jacobi(2/3), Chebyshev degree 1..4;
  3. the bs = 8 block cycle with Chebyshev degree 3;
  4. the cost of the spectral-radius estimates (15 Lanczos steps per level) beside the setup time.
Every timing is repeated REPS times; min / median / max are printed (the spread the comparisons are read against).
usage: python tools/chebyshev_bench.py [N=256] [log=profiles/chebyshev.log]"""
import ctypes as C
import gc
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import amg_amd as AMG  # noqa: E402
from amg_amd.device import DeviceBuffer, DeviceHierarchy  # noqa: E402
from bench import uniform  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
LOG = sys.argv[2] if len(sys.argv) > 2 else None
REPS = 5
out = open(LOG, "w") if LOG else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def spread(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:.3f} ms (min {v[0]:.3f}, max {v[-1]:.3f})"


def med(v):
    return sorted(v)[len(v) // 2]


def with_smoothers(ml, pre, post):
    levels = [AMG.Level(l.A, l.P, l.R, pre, post) for l in ml.levels]
    return AMG.MultiLevel(levels, ml.final_A, ml.coarse_solver, pre, post, ml.symmetry, method=ml.method)


def cycle_ms(dev, bd, zd, reps=20):
    lib = dev.lib
    for _ in range(3):
        lib.amgh_precond_apply_d(dev.h, bd.ptr, zd.ptr, 0)
    lib.amgh_dev_sync(0)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(reps):
            lib.amgh_precond_apply_d(dev.h, bd.ptr, zd.ptr, 0)
        lib.amgh_dev_sync(0)
        ts.append(1e3 * (time.perf_counter() - t0) / reps)
    return ts


if not AMG.gpu_available():
    raise SystemExit("chebyshev_bench: no HIP device visible")
A = AMG.poisson((N, N, N))
n, nnz = A.m, A.nnz
t0 = time.perf_counter()
base = AMG.ruge_stuben(A, setup="gpu")
setup_s = time.perf_counter() - t0
say(f"# poisson(({N},{N},{N})): n = {n}, nnz = {nnz}, {len(base.levels)} levels + coarsest; setup (host hierarchy, setup=\"gpu\") {setup_s:.2f} s")
b = uniform(n, 0)
lib = AMG.hip_lib()

# ---- the run's read ceiling: a dot product of two fine vectors (16 n bytes read, nothing written)
xd, yd, sd = DeviceBuffer(n, 0, b), DeviceBuffer(n, 0, b[::-1].copy()), DeviceBuffer(1025, 0)
res = C.c_double(0)
for _ in range(3):
    lib.amgh_dot_d(0, n, xd.ptr, yd.ptr, sd.ptr, C.byref(res), None)
ts = []
for _ in range(REPS):
    t0 = time.perf_counter()
    for _ in range(20):
        lib.amgh_dot_d(0, n, xd.ptr, yd.ptr, sd.ptr, C.byref(res), None)
    ts.append(1e3 * (time.perf_counter() - t0) / 20)
ceiling = 16.0 * n / (min(ts) * 1e-3)
say(f"read ceiling of this run (dot product of two fine vectors, host clock around synchronising calls): {spread(ts)} -> {ceiling / 1e12:.2f} TB/s at the fastest repetition")
del xd, yd, sd


def frac(nbytes, ms):
    return f"{nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {nbytes / (ms * 1e-3) / ceiling:.2f} of the ceiling"


# ---- 1. fine-level passes (amgh_bench_op: device events around back-to-back launches)
say("\n## 1. fine-level passes")
results = {}
configs = [("jacobi", AMG.Jacobi(2.0 / 3.0, iter=2))] + [(f"chebyshev{k}", AMG.Chebyshev(degree=k)) for k in (2, 4)]
for name, sm in configs:
    dev = DeviceHierarchy(with_smoothers(base, sm, sm), 0, 1)
    results[name] = [dev.bench_op(0, 4, reps=20, warmup=3) for _ in range(REPS)]
    if name == "chebyshev2":
        results["coded"] = int(lib.amgh_debug_coded_ops(dev.h, 0))
        results["residual"] = [dev.bench_op(0, 3, reps=20, warmup=3) for _ in range(REPS)]
    del dev
    gc.collect()
coded = bool(results["coded"] & 8)
ent = 4 if coded else 12
jac = [t / 2 for t in results["jacobi"]]
step = [(t4 - t2) / 2 for t4, t2 in zip(sorted(results["chebyshev4"]), sorted(results["chebyshev2"]))]
first = [t2 - s for t2, s in zip(sorted(results["chebyshev2"]), step)]
B_jac = 12 * nnz + 40 * n          # entries 12 B; rowptr 4, diagonal position 4, diagonal 8, b 8, x 8 read, x 8 written
B_step = ent * nnz + 52 * n        # entries; rowptr 4, diagonal 8, b 8, x 8 read, x 8 written, d 8 read + 8 written
B_first = ent * nnz + 44 * n       # the first step does not read d
B_res = ent * nnz + 28 * n         # entries; rowptr 4, x 8, b 8, r 8
say(f"smoother matrix streams value-coded columns: {coded}")
say(f"Jacobi sweep (plain columns; half of Jacobi(iter=2)):       {spread(jac)}; {B_jac / 1e9:.2f} GB -> {frac(B_jac, med(jac))}")
say(f"residual pass (same operator):                              {spread(results['residual'])}; {B_res / 1e9:.2f} GB -> {frac(B_res, med(results['residual']))}")
say(f"Chebyshev step k >= 2 ((degree 4 - degree 2) / 2):          {spread(step)}; {B_step / 1e9:.2f} GB -> {frac(B_step, med(step))}")
say(f"Chebyshev step 1 (degree 2 - one later step):               {spread(first)}; {B_first / 1e9:.2f} GB -> {frac(B_first, med(first))}")

# ---- 2. cycles and cg
say("\n## 2. V-cycle and cg to reltol = 1e-8 (b ~ U[0,1), seed 0)")
rows = [("GaussSeidel() [default]", AMG.GaussSeidel()), ("Jacobi(2/3)", AMG.Jacobi(2.0 / 3.0))]
rows += [(f"Chebyshev(degree={k})", AMG.Chebyshev(degree=k)) for k in (1, 2, 3, 4)]
bd, zd = DeviceBuffer(n, 0, b), DeviceBuffer(n, 0)
est_s = None
for name, sm in rows:
    t0 = time.perf_counter()
    dev = DeviceHierarchy(with_smoothers(base, sm, sm), 0, 1)
    build_s = time.perf_counter() - t0
    cyc = cycle_ms(dev, bd, zd)
    cg = []
    for _ in range(3):
        t0 = time.perf_counter()
        x, hist, iters = dev.pcg(b, 0, True, 200, 0.0, 1e-8)
        cg.append(1e3 * (time.perf_counter() - t0))
    conv = hist[-1] <= 1e-8 * hist[0]
    say(f"{name:26s} V-cycle {spread(cyc)}; cg {iters} iterations{'' if conv else ' (NOT converged)'}, {spread(cg)}; handle built in {build_s:.2f} s")
    if name == "Chebyshev(degree=3)":
        t0 = time.perf_counter()
        rho = [dev.spectral_radius(l) for l in range(len(base.levels))]
        est_s = time.perf_counter() - t0
        bounds = dev.chebyshev_bounds(0, 0)
    del dev
    gc.collect()
del bd, zd

# ---- 3. the bs = 8 block cycle
say("\n## 3. block of 8 right-hand sides, Chebyshev(degree=3)")
sm = AMG.Chebyshev(degree=3)
dev = DeviceHierarchy(with_smoothers(base, sm, sm), 0, 8)
B = np.asfortranarray(np.stack([uniform(n, j) for j in range(8)], axis=1))
bd, zd = DeviceBuffer(8 * n, 0, B.ravel(order="F")), DeviceBuffer(8 * n, 0)
say(f"bs = 8 V-cycle {spread(cycle_ms(dev, bd, zd, reps=10))}")
del dev, bd, zd
gc.collect()

# ---- 4. the estimates
say("\n## 4. spectral-radius estimates")
say(f"15 Lanczos steps on every level (what amgh_finalize runs for sides without bounds): {est_s:.3f} s beside setup {setup_s:.2f} s")
say("estimates per level: " + ", ".join(f"{r:.4f}" for r in rho) + f"; fine-level bounds [{bounds[0]:.4f}, {bounds[1]:.4f}]")
if out:
    out.close()
