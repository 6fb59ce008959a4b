"""The host restatement of the device GMRES (tests/gmres_ref.py) against dense solves (no GPU needed)."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_ref as G
from conftest import uniform


def nonsym(n, seed, shift=4.0):
    """A sparse nonsymmetric, diagonally dominated test operator."""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, 0.05, random_state=rng, format="csr") + shift * sp.identity(n, format="csr")
    M = M + sp.diags(uniform(n - 1, seed), 1) - sp.diags(0.5 * uniform(n - 1, seed + 1), -1)
    return sp.csr_matrix(M)


def upwind_2d(m, eps=0.05, vx=1.0, vy=0.5):
    """-eps Laplacian + first-order upwind (vx, vy) . grad on an m x m grid, Dirichlet boundary."""
    h = 1.0 / (m + 1)
    I = sp.identity(m, format="csr")
    lap = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m)) / h**2
    dx = sp.diags([-1.0, 1.0], [-1, 0], shape=(m, m)) / h
    return sp.csr_matrix(eps * (sp.kron(I, lap) + sp.kron(lap, I)) + vx * sp.kron(I, dx) + vy * sp.kron(dx, I))


@pytest.mark.parametrize("restart", [3, 7, 20])
def test_identity_preconditioner_solves_nonsymmetric_system(restart):
    A = nonsym(120, 1)
    b = np.cos(np.arange(120))
    x, hist, it = G.gmres(A, b, restart=restart, reltol=1e-12)
    xd = np.linalg.solve(A.toarray(), b)
    assert np.linalg.norm(x - xd) <= 1e-9 * np.linalg.norm(xd)
    assert len(hist) == it + 1 and 0 < it <= 120
    assert hist[0] == pytest.approx(np.linalg.norm(b), rel=1e-15)
    assert hist[-1] <= 1e-12 * hist[0]
    # the estimate is the true residual of the iterate whenever x was just formed (the last step forms x)
    assert np.linalg.norm(b - A @ x) <= 1e-11 * hist[0] * 10


def test_restarts_converge_slower_than_full_gmres():
    A = sp.csr_matrix(upwind_2d(16))
    b = np.ones(A.shape[0])
    st5, st64 = {}, {}
    x5, h5, it5 = G.gmres(A, b, restart=5, reltol=1e-10, stats=st5)
    x64, h64, it64 = G.gmres(A, b, restart=64, reltol=1e-10, stats=st64)
    xd = np.linalg.solve(A.toarray(), b)
    for x in (x5, x64):
        assert np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)
    assert st5["restarts"] > 0 and it5 > it64
    assert np.all(np.diff(h64) <= 1e-12 * h64[0])     # full (unrestarted within 64 steps) GMRES: monotone estimate


def test_dense_inverse_preconditioner_converges_in_one_step():
    A = nonsym(80, 2)
    b = uniform(80, 3) - 0.5
    x, hist, it = G.gmres(A, b, Pl=G.dense_inverse(A), reltol=1e-10)
    assert it == 1
    assert np.linalg.norm(x - np.linalg.solve(A.toarray(), b)) <= 1e-12 * np.linalg.norm(x)
    assert hist[0] == pytest.approx(np.linalg.norm(np.linalg.solve(A.toarray(), b)), rel=1e-12)


def test_lucky_breakdown_small_system():
    """n <= restart: the Krylov space is exhausted after at most n steps; x is the dense solve, no NaN."""
    n = 12
    A = nonsym(n, 4, shift=3.0)
    b = np.arange(1.0, n + 1)
    x, hist, it = G.gmres(A, b, restart=20, reltol=1e-14)
    assert it <= n and np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert np.linalg.norm(x - np.linalg.solve(A.toarray(), b)) <= 1e-10 * np.linalg.norm(x)
    # an exactly invariant subspace: A = I and b a multiple of a unit vector give H[1, 0] == 0 after one step, in exact arithmetic
    # and in floating point (v1 = e3, h = 1, w - v1 h = 0)
    e = np.zeros(n)
    e[2] = 3.0
    x1, h1, it1 = G.gmres(sp.identity(n, format="csr"), e, restart=5)
    assert it1 == 1 and h1[-1] == 0.0 and np.array_equal(x1, e)


def test_history_semantics_and_edge_cases():
    A = nonsym(60, 5)
    b = np.sin(np.arange(60.0))
    x, hist, it = G.gmres(A, b, restart=4, maxiter=7, reltol=1e-15)
    assert it == 7 and len(hist) == 8 and not hist[-1] <= 1e-15 * hist[0]
    x0, h0, i0 = G.gmres(A, np.zeros(60))
    assert i0 == 0 and list(h0) == [0.0] and not np.any(x0)
    xm, hm, im = G.gmres(A, b, maxiter=0)
    assert im == 0 and len(hm) == 1 and not np.any(xm)
    # abstol dominates when reltol is 0
    xa, ha, ia = G.gmres(A, b, reltol=0.0, abstol=1e-6)
    assert ha[-1] <= 1e-6 < ha[-2]
    for bad in (0, 65):
        with pytest.raises(ValueError):
            G.gmres(A, b, restart=bad)
