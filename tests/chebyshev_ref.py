"""Host restatement (numpy / scipy) of what the Chebyshev polynomial smoother adds: the smoother itself, the cycle of
multilevel.jl:200-239 over `ml.levels` with it, `_solve!` (multilevel.jl:158-198), IterativeSolvers.jl's cg around that
cycle, and the Lanczos estimate of the spectral radius of D^-1 S.  A plain helper module (not a conftest): the tests
import it as `chebyshev_ref`.  Bounds are INPUTS here: every function that smooths takes the per-level (lo, hi).

The smoother, for S, D = diag(S), 0 < lo < hi, degree >= 1:
    theta = (hi + lo) / 2;  delta = (hi - lo) / 2;  sigma = theta / delta;  rho = 1 / sigma
    d = (1 / theta) D^-1 (b - S x);  x += d
    k = 2 .. degree:  rho' = 1 / (2 sigma - rho);  d = (rho' rho) d + (2 rho' / delta) D^-1 (b - S x);  x += d;  rho = rho'
rows whose diagonal is zero keep their x (d = 0)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_amd as AMG


def smoother_matrix(A, hermitian=True):
    """scipy CSR of the matrix the smoothers sweep row-wise: column i of A read as row i under HermitianSymmetry()
    (smoother.jl:81-86), the true rows under NoSymmetry()."""
    M = AMG.SparseMatrixCSC.coerce(A).to_scipy()
    return (M.T if hermitian else M).tocsr()


def coefficients(degree, lo, hi):
    """The (c1, c2) pairs straight from the recurrence above (written out once more on purpose: the tests compare the
    package's `Chebyshev.coefficients` and the library's amgh_chebyshev_coefficients with these)."""
    theta, delta = (hi + lo) / 2.0, (hi - lo) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    out = [(0.0, 1.0 / theta)]
    for _ in range(2, degree + 1):
        rho_new = 1.0 / (2.0 * sigma - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return out


def smooth(S, x, b, degree, lo, hi, iters=1, coef=None):
    """`iters` polynomials of `degree` steps on x (a copy is returned).  coef: the (c1, c2) pairs to apply instead of
    the ones of (lo, hi) — how the CPU test runs the package's coefficients through this loop."""
    S = sp.csr_matrix(S)
    dg = S.diagonal()
    ok = dg != 0
    dinv = np.where(ok, 1.0 / np.where(ok, dg, 1.0), 0.0)
    coef = coefficients(degree, lo, hi) if coef is None else coef
    x = np.array(x, dtype=np.float64, copy=True)
    for _ in range(iters):
        d = np.zeros_like(x)
        for k, (c1, c2) in enumerate(coef):
            t = dinv * (b - S @ x)
            d = c2 * t if k == 0 else c1 * d + c2 * t
            x = x + d
    return x


def gauss_seidel(S, x, b, sweep="symmetric", iters=1):
    """GaussSeidel(sweep, iters) over the rows of S in lexicographic order (smoother.jl:61-90); rows with a zero
    diagonal are skipped — not needed by the operators of these tests, which have none."""
    S = sp.csr_matrix(S)
    Lo, Up = sp.tril(S, 0, format="csr"), sp.triu(S, 0, format="csr")
    Ls, Us = sp.tril(S, -1, format="csr"), sp.triu(S, 1, format="csr")
    x = np.array(x, dtype=np.float64, copy=True)
    for _ in range(iters):
        if sweep in ("forward", "symmetric"):
            x = spla.spsolve_triangular(Lo, b - Us @ x, lower=True)
        if sweep in ("backward", "symmetric"):
            x = spla.spsolve_triangular(Up, b - Ls @ x, lower=False)
    return x


class RefHierarchy:
    """The levels of `ml` as scipy CSR and the cycle over them.  bounds[l] = (lo, hi) for level l's Chebyshev sides,
    or {"pre": (lo, hi), "post": (lo, hi)}."""

    def __init__(self, ml, bounds):
        herm = isinstance(ml.symmetry, AMG.HermitianSymmetry)
        self.A = [lev.A.to_scipy().tocsr() for lev in ml.levels]
        self.S = [smoother_matrix(lev.A, herm) for lev in ml.levels]
        self.P = [lev.P.to_scipy().tocsr() for lev in ml.levels]
        self.R = [lev.R.to_scipy().tocsr() for lev in ml.levels]
        self.pre = [lev.presmoother for lev in ml.levels]
        self.post = [lev.postsmoother for lev in ml.levels]
        self.bounds = list(bounds)
        self.coarse = np.asarray(ml.coarse_solver.dense_operator(), dtype=np.float64)
        assert len(self.bounds) == len(self.A)

    def _smooth(self, l, side, x, b):
        s = self.pre[l] if side == "pre" else self.post[l]
        if isinstance(s, AMG.Chebyshev):
            bd = self.bounds[l]
            lo, hi = bd[side] if isinstance(bd, dict) else bd
            return smooth(self.S[l], x, b, s.degree, lo, hi, s.iter)
        if isinstance(s, AMG.GaussSeidel):
            return gauss_seidel(self.S[l], x, b, s.sweep_name, s.iter)
        raise NotImplementedError(repr(s))

    def cycle(self, l, x, b, cyc="V"):
        """__solve!(x, ml, cycle, b, lvl), multilevel.jl:214-239."""
        x = self._smooth(l, "pre", x, b)
        res = b - self.A[l] @ x
        cb = self.R[l] @ res
        cx = np.zeros(cb.shape[0])
        if l == len(self.A) - 1:
            cx = self.coarse @ cb
        elif cyc == "V":
            cx = self.cycle(l + 1, cx, cb, "V")
        elif cyc == "W":
            cx = self.cycle(l + 1, self.cycle(l + 1, cx, cb, "W"), cb, "W")
        else:
            cx = self.cycle(l + 1, self.cycle(l + 1, cx, cb, "F"), cb, "V")
        x = x + self.P[l] @ cx
        return self._smooth(l, "post", x, b)

    def precond(self, r, cyc="V"):
        """ldiv!: one cycle from x = 0 (preconditioner.jl:12-19)."""
        return self.cycle(0, np.zeros_like(r, dtype=np.float64), np.asarray(r, dtype=np.float64), cyc)

    def solve(self, b, cyc="V", maxiter=100, abstol=0.0, reltol=None, calculate_residual=True):
        """_solve(ml, b, cycle): returns (x, residual history) — multilevel.jl:158-198."""
        b = np.asarray(b, dtype=np.float64)
        reltol = float(np.sqrt(np.finfo(np.float64).eps)) if reltol is None else reltol
        x = np.zeros_like(b)
        normres = normb = float(np.linalg.norm(b))
        if normb != 0:
            abstol = max(reltol * normb, abstol)
        hist = [normb]
        itr = 1
        while itr <= maxiter and (not calculate_residual or normres > abstol):
            x = self.cycle(0, x, b, cyc)
            if calculate_residual:
                normres = float(np.linalg.norm(b - self.A[0] @ x))
                hist.append(normres)
            itr += 1
        return x, np.array(hist)


def pcg(A, b, Pl, abstol=0.0, reltol=None, maxiter=None):
    """IterativeSolvers.jl's cg(A, b; Pl, abstol, reltol, maxiter) with x0 = 0: returns (x, residual norms, iterations)."""
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    maxiter = n if maxiter is None else maxiter
    reltol = float(np.sqrt(np.finfo(np.float64).eps)) if reltol is None else reltol
    x = np.zeros(n)
    r = b.copy()
    u = np.zeros(n)
    rho = 1.0
    resid = float(np.linalg.norm(r))
    tol = max(reltol * resid, abstol)
    hist = [resid]
    it = 0
    while it < maxiter and resid > tol:
        c = Pl(r)
        rho_prev, rho = rho, float(np.dot(c, r))
        u = c + (rho / rho_prev) * u
        c = A @ u
        alpha = rho / float(np.dot(u, c))
        x = x + alpha * u
        r = r - alpha * c
        resid = float(np.linalg.norm(r))
        hist.append(resid)
        it += 1
    return x, np.array(hist), it


def uniform(n, seed=0):
    """U[0,1) of the suite's splitmix64 stream (conftest.uniform)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def lanczos_radius(S, steps=15, seed=0):
    """The device estimate restated: `steps` Lanczos steps (clamped to n) for D^-1 S in the D-inner product from the
    start vector uniform(n, seed); the largest Ritz value in magnitude."""
    S = sp.csr_matrix(S)
    n = S.shape[0]
    dg = S.diagonal()
    dinv = np.where(dg != 0, 1.0 / np.where(dg != 0, dg, 1.0), 0.0)
    w = uniform(n, seed)
    v = w / np.sqrt(np.sum(dg * w * w))
    u = np.zeros(n)
    al, be = [], []
    beta = 0.0
    m = min(steps, n)
    for j in range(m):
        w = dinv * (S @ v)
        alpha = float(np.sum(dg * w * v))
        w = (w - alpha * v) - beta * u
        beta = float(np.sqrt(max(np.sum(dg * w * w), 0.0)))
        al.append(alpha)
        if j + 1 == m or not beta > 1e-13 * abs(alpha):
            break
        be.append(beta)
        u, v = v, w / beta
    T = np.diag(al) + np.diag(be, 1) + np.diag(be, -1)
    return float(np.max(np.abs(np.linalg.eigvalsh(T))))


def true_radius(S):
    """max |eig(D^-1 S)| by a dense eigensolve (small operators)."""
    M = np.asarray(sp.csr_matrix(S).todense())
    dg = np.diag(M)
    ok = dg != 0
    B = M[np.ix_(ok, ok)] / dg[ok][:, None]
    return float(np.max(np.abs(np.linalg.eigvals(B))))
