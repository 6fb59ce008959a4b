"""The inputs of tests/test_gpu_krylov_edges.py (tests/krylov_cases.py) under the references alone, no GPU: every
(case, restart) pair reaches the width it is there for, and the references' own answers move by at most a quarter of the
GPU tolerances when the summation order changes (the same system with rows and columns reversed).  So a GPU test that
passes has run the kernels it names, and one that fails has not met rounding of the reference.

The reversed system is the same preconditioned iteration only where the preconditioner does not depend on the order of the
rows: GMRES runs unpreconditioned here, the oracle's pcg runs plain and under a Jacobi-smoothed hierarchy whose levels are
reversed one by one (a symmetric Gauss-Seidel sweep over reversed rows is another smoother).  For the Gauss-Seidel
hierarchies the GPU file runs, the oracle's histories are shown to keep away from their tolerances by far more than the
1e-9 the device may differ by, so that no iteration count hangs on rounding."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_ref as G
import krylov_cases as K
from oracle import oracle as O

GPU_TOL = 1e-8      # GMRES: history within GPU_TOL * hr + 1e-15 * hr[0], x within GPU_TOL
PCG_TOL = 1e-9      # block PCG: x and history within PCG_TOL


def spread(A, b, **kw):
    """gmres_ref on the system and on its reversal: (steps, reorth) must agree; returns them with the largest history
    difference in units of the GPU tolerance and the x difference in units of GPU_TOL."""
    Ar, br = K.reverse_system(A, b)
    s1, s2 = {}, {}
    x, h, it = G.gmres(sp.csr_matrix(A), b, stats=s1, **kw)
    xr, hr, itr = G.gmres(Ar, br, stats=s2, **kw)
    assert it == itr and s1 == s2, (it, itr, s1, s2)
    dh = float(np.max(np.abs(h - hr) / (GPU_TOL * h + 1e-15 * h[0])))
    dx = float(np.linalg.norm(x - xr[::-1]) / np.linalg.norm(x)) / GPU_TOL
    return it, s1, dh, dx


_ops = {}


def operator(name):
    if name not in _ops:
        _ops[name] = sp.csr_matrix(K.gmres_operator(name))
    return _ops[name]


def test_cases_cover_every_residue_and_the_tail_carries_the_norm():
    assert sorted(n % 4 for n in K.GMRES_ROWS.values()) == [0, 1, 2, 3]
    assert sorted(int(np.prod(s)) % 4 for s in K.POISSON_CASES.values()) == [0, 1, 2, 3]
    assert all(int(np.prod(K.POISSON_CASES[c])) % 4 for c in K.SCALAR_POISSON)
    assert all(int(np.prod(K.POISSON_CASES[c])) % 2 for c in K.ODD_POISSON)
    assert K.CAPPED_M ** 3 % 2 == 1 and K.CAPPED_M ** 3 > 2 * 262144
    for n in (1, 3, 2500, 2601, 2002, 12167):
        b = K.tail_heavy(n)
        t = n % 4
        if n > 4:
            assert np.sum(b[n - max(t, 1):] ** 2) >= 0.7 * np.sum(b ** 2), n    # the rows past the last whole vector
    assert np.array_equal(K.staggered_block(50, 17), K.staggered_block(50, 64)[:, :17])


@pytest.mark.parametrize("name", list(K.GMRES_CASES))
def test_tails_runs_restart_and_the_reference_is_stable(name):
    A = operator(name)
    b = K.tail_heavy(A.shape[0])
    it, st, dh, dx = spread(A, b, restart=K.TAILS_RESTART, reltol=K.TAILS_RELTOL)
    print(name, it, st, dh, dx)
    assert it >= K.TAILS_RESTART and st["restarts"] >= 1
    assert dh <= 0.25 and dx <= 0.25, (dh, dx)
    # the Float32 runs stop at TAILS_RELTOL_F32: more than one vector's worth of steps there too
    assert G.gmres(A, b, restart=K.TAILS_RESTART, reltol=K.TAILS_RELTOL_F32)[2] >= 8


@pytest.mark.parametrize("name,restart,reltol,maxiter", K.WIDTH_RUNS)
def test_width_is_reached_and_the_reference_is_stable(name, restart, reltol, maxiter):
    A = operator(name)
    b = K.tail_heavy(A.shape[0])
    it, st, dh, dx = spread(A, b, restart=restart, reltol=reltol, maxiter=maxiter)
    print(name, restart, it, st, dh, dx)
    assert it >= restart and st["restarts"] >= 1, (it, st)       # k = restart is reached, and a restart follows it
    assert dh <= 0.25 and dx <= 0.25, (dh, dx)


def test_every_accumulator_count_runs_at_its_first_and_last_width():
    for case in ("upwind_23^3", "upwind_51x51"):
        rs = sorted(r for c, r, _, _ in K.WIDTH_RUNS if c == case)
        assert rs == [8, 9, 16, 17, 32, 33, 64], (case, rs)
    name, restart, reltol = K.F32_WIDTH
    A = operator(name)
    assert restart == 64 and G.gmres(A, K.tail_heavy(A.shape[0]), restart=restart, reltol=reltol)[2] > 64


def test_stops_inside_a_cycle_and_by_abstol():
    A = operator(K.STOP_CASE)
    b = K.tail_heavy(A.shape[0])
    r = K.STOP_RESTART
    _, h, full = G.gmres(A, b, restart=r, reltol=1e-8)
    assert full > 4 * r
    for maxiter in (r + 3, r):
        it, st, dh, dx = spread(A, b, restart=r, reltol=1e-8, maxiter=maxiter)
        assert it == maxiter and dh <= 0.25 and dx <= 0.25, (maxiter, it, dh, dx)
    abstol = 1e-4 * h[0]
    assert abstol > 1e-8 * h[0]
    for reltol in (1e-8, 0.0):
        it, st, dh, dx = spread(A, b, restart=r, reltol=reltol, abstol=abstol)
        _, ha, _ = G.gmres(A, b, restart=r, reltol=reltol, abstol=abstol)
        assert it < full // 2 and ha[-1] <= abstol < ha[-2] and it % r != 0, (it, full)    # abstol decides, inside a cycle
        assert dh <= 0.25 and dx <= 0.25, (reltol, dh, dx)


def test_capped_grid_case():
    A = sp.csr_matrix(K.upwind(K.CAPPED_M, 3))
    it, st, dh, dx = spread(A, K.tail_heavy(A.shape[0]), restart=20, reltol=1e-8, maxiter=25)
    assert it == 25 and st["restarts"] == 1 and dh <= 0.25 and dx <= 0.25, (it, st, dh, dx)


# ---- the oracle's pcg ------------------------------------------------------------------------------------------------
def pcg_spread(oh, ohr, b, **kw):
    b = np.ascontiguousarray(b)
    x, h, it = oh.pcg(b, 0, **kw)
    xr, hr, itr = ohr.pcg(np.ascontiguousarray(b[::-1]), 0, **kw)
    assert it == itr, (it, itr)
    nx = np.linalg.norm(x)
    dx = float(np.linalg.norm(x - xr[::-1]) / nx) if nx else float(np.linalg.norm(xr))
    dh = float(np.max(np.abs(h - hr) / np.maximum(np.abs(h), 1e-300))) if h[0] else float(np.max(np.abs(hr)))
    return it, dx / PCG_TOL, dh / PCG_TOL


@pytest.mark.parametrize("name", K.ODD_POISSON)
def test_oracle_pcg_is_stable_under_reversal(name):
    ml = K.poisson_hierarchy(name, "jacobi")
    oh, ohr = O.OracleHierarchy(ml), O.OracleHierarchy(K.reversed_hierarchy(ml))
    n = ml.levels[0].A.m
    B = K.tail_block(n, 8)
    for j in range(8):
        it, dx, dh = pcg_spread(oh, ohr, B[:, j], reltol=1e-10)
        print(name, j, it, dx, dh)
        assert dx <= 0.25 and dh <= 0.25, (name, j, dx, dh)
    it, dx, dh = pcg_spread(oh, ohr, B[:, 0], use_precond=False, reltol=1e-8)      # plain CG: many more iterations
    print(name, "plain", it, dx, dh)
    assert it > 50 and dx <= 0.25 and dh <= 0.25, (name, it, dx, dh)


def margin(h, tol):
    """The smallest relative distance of a residual history from its tolerance."""
    return float(np.min(np.abs(h - tol) / tol)) if tol > 0 else np.inf


@pytest.mark.parametrize("name", K.SCALAR_POISSON)
def test_no_oracle_iteration_count_hangs_on_rounding(name):
    """The Gauss-Seidel hierarchies of the GPU file: every residual of every column is further than 1e-4 of its
    tolerance away from it, 1e5 times what the device's residual may differ by."""
    ml = K.poisson_hierarchy(name)
    oh = O.OracleHierarchy(ml)
    n = ml.levels[0].A.m
    B = K.tail_block(n, 8)
    for j in range(8):
        _, h, it = oh.pcg(np.ascontiguousarray(B[:, j]), 0, reltol=1e-10)
        assert (it == 0) == (j == 1) and margin(h, 1e-10 * h[0]) >= 1e-4, (name, j, it, margin(h, 1e-10 * h[0]))
    _, h, it = oh.pcg(np.ascontiguousarray(B[:, 0]), 0, use_precond=False, reltol=1e-8)
    assert it > 50 and margin(h, 1e-8 * h[0]) >= 1e-4, (name, it)


def test_wide_block_columns_stop_at_different_iterations():
    import amg_amd as AMG
    ml = AMG.ruge_stuben(AMG.poisson((24, 24, 24)))
    oh = O.OracleHierarchy(ml)
    n = ml.levels[0].A.m
    B = K.staggered_block(n, 64)
    abstol = K.staggered_abstol(B)
    its = []
    for j in range(64):
        _, h, it = oh.pcg(np.ascontiguousarray(B[:, j]), 0, reltol=1e-10, abstol=abstol)
        tol = max(1e-10 * h[0], abstol)
        assert margin(h, tol) >= 1e-4, (j, margin(h, tol))
        its.append(it)
    for bs in (17, 32, 33, 64):
        assert len(set(its[:bs])) >= 2, (bs, its[:bs])
