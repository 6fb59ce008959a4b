"""The per-row sweep bound of tests/sweep_bound.py on the host (no GPU): the oracle's own scalar sweeps pass it in Float64 and
Float32, and it rejects a value moved by 4x its bound, a row that read a stale x, and a zero-diagonal row that changed."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_amd as AMG
from conftest import uniform
from oracle import oracle as O
from sweep_bound import assert_sweep_within_bound, directional, sweep_errors

SWEEPS = [AMG.GaussSeidel(AMG.ForwardSweep()), AMG.GaussSeidel(AMG.BackwardSweep()), AMG.SOR(1.3, AMG.ForwardSweep()),
          AMG.SOR(0.7, AMG.BackwardSweep())]


def _galerkin_19_point():
    A1 = AMG.ruge_stuben(AMG.poisson((24, 22, 20))).levels[1].A
    assert int(np.diff(A1.to_scipy().tocsr().indptr).max()) - 1 > 12
    return A1


def _zero_and_divide_rows(dtype):
    """test_gpu_late's planted rows: zero diagonals and diagonals far outside the ordinary range (scaled into Float32's)"""
    M = AMG.poisson((20, 18, 16)).to_scipy().tolil()
    n = M.shape[0]
    big, small = (6.0e120, 3.0e-130) if dtype == np.float64 else (6.0e30, 3.0e-30)
    for r in (0, 777, 3000, n - 1):
        M[r, r] = 0.0
    for r in (5, 1234, 4000):
        M[r, r] = big
    for r in (9, 2222):
        M[r, r] = small
    return AMG.SparseMatrixCSC.from_scipy(sp.csc_matrix(M.tocsr())), (0, 777, 3000, n - 1)


def _case(case, dtype):
    if case == "poisson3d":
        return AMG.poisson((20, 18, 16)), ()
    if case == "galerkin19":
        return _galerkin_19_point(), ()
    return _zero_and_divide_rows(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", ["poisson3d", "galerkin19", "zero_divide"])
def test_the_oracles_sweeps_are_within_the_bound(case, dtype):
    A, zeros = _case(case, dtype)
    x0, b = (uniform(A.m, 31) - 0.5).astype(dtype), uniform(A.m, 32).astype(dtype)
    for pre in SWEEPS:
        back, omega = directional(pre)
        x = O.smooth(pre, A, x0, b, hermitian=True, dtype=dtype)
        worst = assert_sweep_within_bound(A, x0, b, x, back, omega, dtype, what=repr(pre))
        assert worst <= 1.0
        for r in zeros:
            assert x[r] == x0[r]


def test_directional_only_for_single_directional_sweeps():
    assert directional(AMG.GaussSeidel()) is None and directional(AMG.GaussSeidel(AMG.ForwardSweep(), iter=2)) is None
    assert directional(AMG.Jacobi(0.5)) is None
    assert directional(AMG.GaussSeidel(AMG.BackwardSweep())) == (True, 1.0)
    assert directional(AMG.SOR(1.2, AMG.ForwardSweep())) == (False, 1.2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_bound_rejects_a_value_moved_by_four_times_its_bound(dtype):
    A = _galerkin_19_point()
    x0, b = (uniform(A.m, 41) - 0.5).astype(dtype), uniform(A.m, 42).astype(dtype)
    for pre in (SWEEPS[0], SWEEPS[3]):
        back, omega = directional(pre)
        x = O.smooth(pre, A, x0, b, hermitian=True, dtype=dtype)
        err, tol, zero, checked = sweep_errors(A, x0, b, x, back, omega, dtype)
        for i in (0, A.m // 2, A.m - 1):
            bad = x.copy()
            bad[i] = dtype(float(x[i]) + 4.0 * float(tol[i]))
            assert abs(float(bad[i]) - float(x[i])) >= 3.5 * float(tol[i])      # (the move survives the rounding)
            with pytest.raises(AssertionError, match="of its bound"):
                assert_sweep_within_bound(A, x0, b, bad, back, omega, dtype)
            e2, t2, _, _ = sweep_errors(A, x0, b, bad, back, omega, dtype)
            assert e2[i] > 3 * t2[i]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("backward", [False, True])
def test_the_bound_rejects_a_stale_dependency(dtype, backward):
    """One row recomputed — exactly, in Float64 — from x0_k for a neighbour k the sweep had already updated: that row alone is
    inconsistent with its inputs, by |a_ik (xhat_k - x0_k) / a_ii|, far above rounding."""
    A = AMG.poisson((20, 18, 16))
    x0, b = (uniform(A.m, 51) - 0.5).astype(dtype), uniform(A.m, 52).astype(dtype)
    pre = AMG.GaussSeidel(AMG.BackwardSweep() if backward else AMG.ForwardSweep())
    x = O.smooth(pre, A, x0, b, hermitian=True, dtype=dtype)
    assert_sweep_within_bound(A, x0, b, x, backward, 1.0, dtype)
    cp, rv, nz = A.colptr, A.rowval, A.nzval
    i = A.m // 2
    ks = [int(k) for k in rv[cp[i]:cp[i + 1]] if (k > i if backward else k < i)]
    k_stale = ks[0]
    s, d = 0.0, 0.0
    for j in range(cp[i], cp[i + 1]):
        k = int(rv[j])
        if k == i:
            d = float(nz[j])
        else:
            done = k > i if backward else k < i
            s += float(nz[j]) * float(x0[k] if (k == k_stale or not done) else x[k])
    bad = x.copy()
    bad[i] = dtype((float(b[i]) - s) / d)
    assert bad[i] != x[i]
    with pytest.raises(AssertionError, match="of its bound"):
        assert_sweep_within_bound(A, x0, b, bad, backward, 1.0, dtype)
    e2, t2, _, _ = sweep_errors(A, x0, b, bad, backward, 1.0, dtype)
    assert e2[i] > 100 * t2[i]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_bound_rejects_a_zero_diagonal_row_that_changed(dtype):
    A, zeros = _zero_and_divide_rows(dtype)
    x0, b = (uniform(A.m, 61) - 0.5).astype(dtype), uniform(A.m, 62).astype(dtype)
    pre = AMG.GaussSeidel(AMG.ForwardSweep())
    x = O.smooth(pre, A, x0, b, hermitian=True, dtype=dtype)
    assert_sweep_within_bound(A, x0, b, x, False, 1.0, dtype)
    bad = x.copy()
    bad[zeros[1]] = np.nextafter(x[zeros[1]], dtype(np.inf))
    with pytest.raises(AssertionError, match="zero-diagonal rows changed"):
        assert_sweep_within_bound(A, x0, b, bad, False, 1.0, dtype)
