"""The device-resident restarted GMRES (amgh_gmres, AMG.gmres) against its host restatement (tests/gmres_ref.py) with
the CPU oracle's cycle as the preconditioner."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import scipy.sparse as sp

import amg_amd as AMG
import gmres_ref as G
from conftest import ROOT
from krylov_cases import upwind
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CYCLES = {"V": (AMG.V, 0), "W": (AMG.W, 1), "F": (AMG.F, 2)}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def issue95():
    rng = np.random.default_rng(95)
    N = 10000
    return sp.random(N, N, 0.001, random_state=rng, format="csc") + 5 * sp.identity(N, format="csc")


def check_against_checker(A, ml, b, cycle="V", restart=None, reltol=None, maxiter=None, xtol=1e-8, htol=1e-8):
    cyc, code = CYCLES[cycle]
    oh = O.OracleHierarchy(ml)
    Pl = lambda r: oh.precond(r, code)   # noqa: E731
    xr, hr, itr = G.gmres(A, b, Pl=Pl, restart=restart, reltol=reltol, maxiter=maxiter)
    x, info = AMG.gmres(A, b, Pl=AMG.aspreconditioner(ml, cyc), restart=restart, reltol=reltol, maxiter=maxiter, log=True)
    hist = np.concatenate([[np.linalg.norm(Pl(b))], info["resnorm"]])
    assert info["iters"] == itr, (info["iters"], itr)
    assert len(hist) == len(hr) and np.all(np.abs(hist - hr) <= htol * np.abs(hr)), np.max(np.abs(hist - hr) / hr)
    assert rel(x, xr) <= xtol, rel(x, xr)
    tol = (np.sqrt(np.finfo(np.float64).eps) if reltol is None else reltol) * hr[0]
    assert info["isconverged"]
    assert np.linalg.norm(Pl(b - A @ x)) <= tol * (1 + 1e-6)
    return x, info


@pytest.mark.parametrize("builder", ["rs", "sa"])
@pytest.mark.parametrize("cycle", ["V", "W", "F"])
def test_issue95_nosymmetry(builder, cycle):
    M = issue95()
    f = AMG.ruge_stuben if builder == "rs" else AMG.smoothed_aggregation
    ml = f(M, symmetry=AMG.NoSymmetry())
    check_against_checker(M, ml, np.ones(M.shape[0]), cycle)


@pytest.mark.parametrize("restart", [5, 20])
def test_upwind_convection_diffusion_2d(restart):
    A = upwind(256, 2)
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry())
    b = np.ones(A.shape[0])
    _, info = check_against_checker(A, ml, b, "V", restart=restart, reltol=1e-8)
    if restart == 5:
        assert info["iters"] > 5   # several restarts


def test_no_preconditioner_against_checker():
    rng = np.random.default_rng(7)
    n = 2000
    A = sp.csc_matrix(sp.random(n, n, 0.003, random_state=rng) + 3 * sp.identity(n) + sp.diags(np.ones(n - 1), 1))
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry())
    b = np.cos(np.arange(n))
    xr, hr, itr = G.gmres(A, b, restart=10, reltol=1e-10)
    x, hist, it = ml.device().gmres(b, use_precond=False, restart=10, reltol=1e-10)
    assert it == itr and len(hist) == len(hr)
    # 1e-8 relative, down to a floor of 1e-15 |b|: every restart recomputes b - A x, whose rounding is ~eps |b| absolute —
    # at reltol 1e-10 that is more than 1e-8 of the last estimates (measured 1.1e-16 absolute = 1.9e-8 relative)
    assert np.all(np.abs(hist - hr) <= 1e-8 * hr + 1e-15 * hr[0]), np.max(np.abs(hist - hr) / hr)
    assert rel(x, xr) <= 1e-8 and rel(x, np.linalg.solve(A.toarray(), b)) <= 1e-8


def test_lucky_breakdown_n_le_restart():
    n = 30
    rng = np.random.default_rng(3)
    A = sp.csc_matrix(sp.random(n, n, 0.2, random_state=rng) + 2 * sp.identity(n) + sp.diags(np.ones(n - 1), -1))
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry())
    b = np.arange(1.0, n + 1)
    x, hist, it = ml.device().gmres(b, use_precond=False, restart=40, reltol=1e-14)
    assert it <= n and np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert rel(x, np.linalg.solve(A.toarray(), b)) <= 1e-10
    # an exactly invariant subspace: A = 2 I and b a multiple of a unit vector give H[1, 0] == 0 after one step, in floating
    # point too (v1 = e3, h = 2, w - v1 h = 0): x from the first column, v2 never used, no NaN
    e = np.zeros(n)
    e[2] = 3.0
    ml2 = AMG.ruge_stuben(sp.csc_matrix(2.0 * sp.identity(n)), symmetry=AMG.NoSymmetry())
    x2, h2, it2 = ml2.device().gmres(e, use_precond=False, restart=8)
    assert it2 == 1 and h2[-1] == 0.0 and np.all(np.isfinite(x2)) and np.array_equal(x2, e / 2)


def test_edge_cases():
    M = issue95()
    ml = AMG.ruge_stuben(M, symmetry=AMG.NoSymmetry())
    d = ml.device()
    n = M.shape[0]
    x, hist, it = d.gmres(np.zeros(n))
    assert it == 0 and list(hist) == [0.0] and not np.any(x)
    x, hist, it = d.gmres(np.ones(n), maxiter=0)
    assert it == 0 and len(hist) == 1 and hist[0] > 0 and not np.any(x)
    for bad in (0, 65):
        with pytest.raises(AMG.AMGError, match="rc=-2"):
            d.gmres(np.ones(n), restart=bad)
    with pytest.raises(AMG.AMGError, match="rc=-2"):
        d.gmres(np.ones(n), maxiter=-1)
    with pytest.raises(AMG.AMGError, match="rc=-5"):
        ml.device(nrhs=2).gmres(np.ones(n))
    with pytest.raises(AMG.AMGError):
        AMG.gmres(M, np.ones(n))            # no preconditioner
    with pytest.raises(AMG.AMGError):
        AMG.gmres(M + sp.identity(n, format="csc"), np.ones(n), Pl=AMG.aspreconditioner(ml))


def test_deterministic():
    M = issue95()
    ml = AMG.smoothed_aggregation(M, symmetry=AMG.NoSymmetry())
    d = ml.device()
    b = np.linspace(-1.0, 1.0, M.shape[0])
    x1, h1, i1 = d.gmres(b, restart=7)
    x2, h2, i2 = d.gmres(b, restart=7)
    assert i1 == i2 and np.array_equal(x1, x2) and np.array_equal(h1, h2)
    assert d.gmres_reorth_passes() >= 0


def test_float32_instance_issue95():
    M = issue95()
    ml = AMG.ruge_stuben(M, symmetry=AMG.NoSymmetry())
    ml32 = AMG.ruge_stuben(sp.csc_matrix(M, dtype=np.float32), symmetry=AMG.NoSymmetry())
    b = np.ones(M.shape[0])
    oh = O.OracleHierarchy(ml)
    xr, hr, itr = G.gmres(M, b, Pl=oh.precond, reltol=1e-4)
    x, info = AMG.gmres(ml32.levels[0].A, b.astype(np.float32), Pl=AMG.aspreconditioner(ml32), reltol=1e-4, log=True)
    assert x.dtype == np.float32 and info["isconverged"]
    assert abs(info["iters"] - itr) <= 1
    assert rel(x.astype(np.float64), xr) <= 1e-3
    assert np.linalg.norm(M @ x - b) <= 1e-3 * np.linalg.norm(b)


def test_fullsize_poisson_256():
    """256^3 Poisson, ruge_stuben defaults, reltol 1e-8.  The checker runs the oracle's V-cycle on the host once per
    step (stated cost: ~1.4 s per cycle, ~25 s in all; not measured)."""
    A = AMG.poisson((256, 256, 256))
    ml = AMG.ruge_stuben(A)
    b = A @ np.ones(A.m)
    oh = O.OracleHierarchy(ml)
    As = A.to_scipy()
    xr, hr, itr = G.gmres(As, b, Pl=oh.precond, reltol=1e-8)
    del oh
    x, info = AMG.gmres(A, b, Pl=AMG.aspreconditioner(ml), reltol=1e-8, log=True)
    assert info["isconverged"] and abs(info["iters"] - itr) <= 1
    assert np.linalg.norm(b - As @ x) <= 1e-7 * np.linalg.norm(b)


CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import torch  # noqa: F401  (torch's HIP runtime first, as the suite's conftest does)
    import numpy as np, scipy.sparse as sp
    import amg_amd as AMG, gmres_ref as G
    from oracle import oracle as O
    rng = np.random.default_rng(95)
    N = 10000
    M = sp.random(N, N, 0.001, random_state=rng, format="csc") + 5 * sp.identity(N, format="csc")
    b = np.ones(N)
    ml = AMG.ruge_stuben(M, symmetry=AMG.NoSymmetry())
    x, info = AMG.gmres(M, b, Pl=AMG.aspreconditioner(ml), log=True)
    xr, hr, itr = G.gmres(M, b, Pl=O.OracleHierarchy(ml).precond)
    err = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    print("RESULT", int(info["isconverged"]), info["iters"], itr, err)
""")


def test_shipping_configuration_fresh_process():
    """The library's shipping tunables (no session pins): a child process that never sets one."""
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1].split()
    conv, it, itr, err = int(line[1]), int(line[2]), int(line[3]), float(line[4])
    assert conv == 1 and abs(it - itr) <= 1 and err <= 1e-8, line
