"""The host half of the Chebyshev polynomial smoother (no GPU): the coefficients against the closed form of the polynomial,
the configuration's argument checks and the unchanged layout of amgh_smoother_t."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import amg_amd as AMG
import chebyshev_ref as R


def cheb_T(k, t):
    """T_k(t) by the three-term recurrence (valid for every real t)."""
    t = np.asarray(t, dtype=np.float64)
    a, b = np.ones_like(t), t.copy()
    if k == 0:
        return a
    for _ in range(2, k + 1):
        a, b = b, 2.0 * t * b - a
    return b


@pytest.mark.parametrize("lo,hi", [(0.05, 1.6), (1.0 / 30.0 * 1.97, 1.1 * 1.97), (0.3, 0.9)])
@pytest.mark.parametrize("degree", range(1, 9))
def test_coefficients_give_the_scaled_chebyshev_polynomial(degree, lo, hi):
    """Applied by the numpy loop to a DIAGONAL operator (D = I, so D^-1 S = S) with entries spread over [lo, hi] and
    beyond, x0 = 1, b = 0: the error propagator is T_k((theta - lam) / delta) / T_k(sigma), and its maximum over
    [lo, hi] is 1 / T_k(sigma) — both closed forms."""
    lam = np.concatenate([np.linspace(lo, hi, 401), [0.25 * lo, 0.5 * lo, 1.05 * hi, 1.2 * hi]])
    # a diagonal operator acts on each eigenvector as a scalar: run the recurrence per eigenvalue lam of D^-1 S
    coef = AMG.Chebyshev(degree=degree).coefficients(lo, hi)
    assert len(coef) == degree and coef[0][0] == 0.0
    x = np.ones_like(lam)
    d = np.zeros_like(lam)
    for k, (c1, c2) in enumerate(coef):       # D^-1 (b - S x) = -lam x on the eigenvector of eigenvalue lam
        t = -lam * x
        d = c2 * t if k == 0 else c1 * d + c2 * t
        x = x + d
    theta, delta = (hi + lo) / 2.0, (hi - lo) / 2.0
    sigma = theta / delta
    want = cheb_T(degree, (theta - lam) / delta) / cheb_T(degree, np.array(sigma))
    assert np.max(np.abs(x - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    inside = (lam >= lo) & (lam <= hi)
    peak = 1.0 / float(cheb_T(degree, np.array(sigma)))
    assert abs(np.max(np.abs(x[inside])) - peak) <= 1e-12
    assert np.max(np.abs(want[inside])) <= peak * (1 + 1e-12)


@pytest.mark.parametrize("degree", [1, 2, 5, 8])
def test_reference_loop_on_a_diagonal_operator(degree):
    """The same through chebyshev_ref.smooth on an actual matrix: unit diagonal plus a skew part would not be diagonal,
    so the operator is block diagonal with 2 x 2 blocks [[1, e], [e, 1]] (diagonal 1, eigenvalues 1 +- e): D = I and the
    propagator acts on each eigenvector as the scalar polynomial."""
    lo, hi = 0.1, 1.9
    e = np.linspace(0.0, 0.95, 64)
    n = 2 * e.size
    S = sp.block_diag([np.array([[1.0, v], [v, 1.0]]) for v in e], format="csr")
    theta, delta = (hi + lo) / 2.0, (hi - lo) / 2.0
    sigma = theta / delta
    x0 = np.tile([1.0, 1.0], e.size)          # eigenvector of eigenvalue 1 + e in every block
    x = R.smooth(S, x0, np.zeros(n), degree, lo, hi, coef=AMG.Chebyshev(degree=degree).coefficients(lo, hi))
    want = cheb_T(degree, (theta - (1.0 + e)) / delta) / cheb_T(degree, np.array(sigma))
    assert np.max(np.abs(x[0::2] - want)) <= 1e-12 and np.max(np.abs(x[1::2] - want)) <= 1e-12
    x1 = np.tile([1.0, -1.0], e.size)         # eigenvalue 1 - e
    y = R.smooth(S, x1, np.zeros(n), degree, lo, hi)
    want = cheb_T(degree, (theta - (1.0 - e)) / delta) / cheb_T(degree, np.array(sigma))
    assert np.max(np.abs(y[0::2] - want)) <= 1e-12


def test_one_definition_of_the_coefficients():
    """Package, test helper and library (a host-only entry point of both instances) give the same pairs, bit for bit."""
    for degree, lo, hi in [(1, 0.1, 2.0), (3, 1.97 / 30, 1.1 * 1.97), (8, 0.3, 0.9), (16, 1e-3, 4.0)]:
        py = AMG.Chebyshev(degree=degree).coefficients(lo, hi)
        assert py == R.coefficients(degree, lo, hi)
        for dt in ("float64", "float32"):
            out = np.zeros(2 * degree)
            assert AMG.hip_lib(dt).amgh_chebyshev_coefficients(degree, lo, hi, out.ctypes.data) == 0
            assert [tuple(p) for p in out.reshape(degree, 2)] == py
    lib = AMG.hip_lib()
    out = np.zeros(40)
    for degree, lo, hi in [(0, 0.1, 1.0), (17, 0.1, 1.0), (2, 0.0, 1.0), (2, -1.0, 1.0), (2, 1.0, 1.0), (2, 2.0, 1.0),
                           (2, float("nan"), 1.0), (2, 0.1, float("inf"))]:
        assert lib.amgh_chebyshev_coefficients(degree, lo, hi, out.ctypes.data) == -2
    assert lib.amgh_chebyshev_coefficients(2, 0.1, 1.0, None) == -2


def test_configuration_argument_checks_and_layout():
    c = AMG.Chebyshev()
    assert (c.degree, c.lower, c.upper, c.iter, c.rho) == (3, 1.0 / 30.0, 1.1, 1, None)
    assert repr(AMG.Chebyshev(2, rho=1.5, iter=2)) == f"Chebyshev(degree=2, lower={1.0 / 30.0}, upper=1.1, iter=2, rho=1.5)"
    for kw in (dict(degree=0), dict(degree=17), dict(degree=2.5), dict(lower=0.0), dict(lower=-1.0), dict(lower=1.2),
               dict(upper=float("inf")), dict(lower=float("nan")), dict(rho=0.0), dict(rho=-2.0), dict(rho=float("nan")),
               dict(iter=-1)):
        with pytest.raises(AMG.AMGError):
            AMG.Chebyshev(**kw)
    s = AMG.Chebyshev(degree=4, iter=2, rho=2.0).c_struct()
    assert ctypes.sizeof(s) == 24 and ctypes.sizeof(type(s)) == 24
    assert (s.kind, s.sweep, s.iter, s.pad_) == (4, 4, 2, 0)
    assert [f[0] for f in type(s)._fields_] == ["kind", "sweep", "iter", "pad_", "omega"]
    assert AMG.Chebyshev(rho=2.0).c_bounds() == (2.0 / 30.0, 2.2, 0)
    assert AMG.Chebyshev(lower=0.1, upper=1.2).c_bounds() == (0.1, 1.2, 1)
    assert AMG.Chebyshev(rho=2.0, lower=0.25, upper=1.0).bounds() == (0.5, 2.0)
    with pytest.raises(AMG.AMGError):
        AMG.Chebyshev().bounds()
    with pytest.raises(AMG.AMGError):
        AMG.Chebyshev().coefficients(1.0, 0.5)
    # a NoSymmetry() hierarchy does not guess the spectral radius
    A = AMG.poisson((12, 12))
    with pytest.raises(AMG.AMGError, match="rho"):
        AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry(), presmoother=AMG.Chebyshev(), postsmoother=AMG.Chebyshev())
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry(), presmoother=AMG.Chebyshev(rho=2.0), postsmoother=AMG.Chebyshev(rho=2.0))
    assert isinstance(ml.levels[0].presmoother, AMG.Chebyshev)
    assert hasattr(AMG, "approximate_spectral_radius")


def test_lanczos_restatement_meets_the_two_conditions_on_small_operators():
    """The host restatement of the device estimate (what the GPU test compares the library with): never above the
    spectrum, and 1.1 x the estimate covers it."""
    for A in (AMG.poisson(1000), AMG.poisson((50, 50)), AMG.poisson((16, 16, 16))):
        S = R.smoother_matrix(A)
        est = R.lanczos_radius(S, 15)
        dinv = 1.0 / S.diagonal()
        sym = sp.diags(np.sqrt(dinv)) @ S @ sp.diags(np.sqrt(dinv))
        true = float(np.max(np.abs(np.linalg.eigvalsh(sym.toarray())))) if S.shape[0] <= 4096 else None
        if true is None:
            continue
        assert est <= true * (1 + 1e-10) and 1.1 * est >= true, (est, true)
