"""Smoother configurations — host mirror of smoother.jl:1-49,92-99,173-180.

`GaussSeidel(sweep, iter)`, `Jacobi(ω; iter)`, `SOR(ω, sweep, iter)`, the Chebyshev
polynomial smoother `Chebyshev(degree, lower, upper, iter, rho)` (no counterpart in the
reference: PyAMG's, hypre's and AmgX's polynomial relaxation) and the
in-place convenience call `(config)(A, x, b, symmetry=HermitianSymmetry())`
(smoother.jl:33-38), which runs the sweep on the GPU through libamghip's
stand-alone CSR operators.
"""
import numpy as np

from ._libs import AMGError, amgh_smoother_t

KIND_NONE, KIND_GS, KIND_JACOBI, KIND_SOR, KIND_CHEBYSHEV = 0, 1, 2, 3, 4
CHEBYSHEV_MAX_DEGREE = 16
SWEEP_FORWARD, SWEEP_BACKWARD, SWEEP_SYMMETRIC = 0, 1, 2


class Sweep:
    code = None
    name = None


class ForwardSweep(Sweep):
    code, name = SWEEP_FORWARD, "forward"


class BackwardSweep(Sweep):
    code, name = SWEEP_BACKWARD, "backward"


class SymmetricSweep(Sweep):
    code, name = SWEEP_SYMMETRIC, "symmetric"


def _sweep(s):
    if isinstance(s, type) and issubclass(s, Sweep):
        s = s()
    if not isinstance(s, Sweep):
        raise AMGError("sweep must be ForwardSweep(), BackwardSweep() or SymmetricSweep()")
    return s


class SingularException(ArithmeticError):
    """LinearAlgebra.SingularException(col) — thrown by the NoSymmetry smoothers' setup
    when a diagonal entry is missing or zero (smoother.jl:239-241)."""

    def __init__(self, col):
        super().__init__(f"SingularException({col})")
        self.col = col


class Smoother:
    kind = KIND_NONE
    iter = 1
    omega = 1.0
    sweep_code = SWEEP_SYMMETRIC

    def c_struct(self):
        return amgh_smoother_t(self.kind, self.sweep_code, int(self.iter), 0, float(self.omega))

    def check_no_symmetry(self, A):
        """DiagonalIndices(A) check of the NoSymmetry family (smoother.jl:226-257)."""
        d = A.diagonal()
        stored = np.zeros(A.m, dtype=bool)
        cols = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(A.colptr))
        stored[A.rowval[A.rowval == cols]] = True
        bad = np.nonzero(~stored | (d == 0))[0]
        if bad.size:
            raise SingularException(int(bad[0]) + 1)

    def __call__(self, A, x, b, symmetry=None):
        """In-place `smooth!` on freshly set-up smoother (smoother.jl:33-38). x is updated in place."""
        from .device import smooth_standalone
        smooth_standalone(self, A, x, b, symmetry)
        return None


class GaussSeidel(Smoother):
    """GaussSeidel(; iter=1) = symmetric sweep; GaussSeidel(sweep; iter=1); GaussSeidel(sweep, iter)."""
    kind = KIND_GS

    def __init__(self, sweep=None, iter=1):
        s = _sweep(sweep if sweep is not None else SymmetricSweep())
        self.sweep = s
        self.sweep_code = s.code
        self.sweep_name = s.name
        self.iter = int(iter)

    def __repr__(self):
        return f"GaussSeidel({type(self.sweep).__name__}(), {self.iter})"


class Jacobi(Smoother):
    """Jacobi(ω; iter=1) (smoother.jl:97)."""
    kind = KIND_JACOBI

    def __init__(self, omega=0.5, iter=1):
        self.omega = float(omega)
        self.iter = int(iter)

    def check_no_symmetry(self, A):  # JacobiSmoother skips zero diagonals (smoother.jl:162-168)
        return None

    def __repr__(self):
        return f"Jacobi({self.omega}, iter={self.iter})"


class SOR(Smoother):
    """SOR(ω; iter=1) symmetric; SOR(ω, sweep); SOR(ω, sweep, iter) (smoother.jl:173-180)."""
    kind = KIND_SOR

    def __init__(self, omega, sweep=None, iter=1):
        s = _sweep(sweep if sweep is not None else SymmetricSweep())
        self.omega = float(omega)
        self.sweep = s
        self.sweep_code = s.code
        self.sweep_name = s.name
        self.iter = int(iter)

    def __repr__(self):
        return f"SOR({self.omega}, {type(self.sweep).__name__}(), {self.iter})"


class Chebyshev(Smoother):
    """Chebyshev(degree=3, lower=1/30, upper=1.1, iter=1, rho=None): the polynomial smoother

        theta = (hi + lo) / 2;  delta = (hi - lo) / 2;  sigma = theta / delta;  r = 1 / sigma
        d = (1 / theta) D⁻¹ (b - S x);  x += d
        k = 2 .. degree:  r' = 1 / (2 sigma - r);  d = (r' r) d + (2 r' / delta) D⁻¹ (b - S x);  x += d;  r = r'

    on the eigenvalue interval [lo, hi] = [lower * rho, upper * rho] of D⁻¹S, S the matrix the smoothers sweep, D its
    diagonal; `iter` repeats the polynomial.  rho = None: every level's spectral radius is estimated on the device when
    the hierarchy is finalized (`approximate_spectral_radius`; symmetric operators) — lower / upper are PyAMG's
    defaults.  One fused pass over the matrix per step, as parallel as Jacobi, and symmetric: with the same polynomial
    before and after the coarse correction the cycle is a valid `cg` preconditioner."""
    kind = KIND_CHEBYSHEV

    def __init__(self, degree=3, lower=1.0 / 30.0, upper=1.1, iter=1, rho=None):
        if int(degree) != degree or not 1 <= int(degree) <= CHEBYSHEV_MAX_DEGREE:
            raise AMGError(f"Chebyshev: degree must be an integer in 1..{CHEBYSHEV_MAX_DEGREE}, got {degree!r}")
        if int(iter) != iter or int(iter) < 0:
            raise AMGError(f"Chebyshev: iter must be a non-negative integer, got {iter!r}")
        lower, upper = float(lower), float(upper)
        if not (np.isfinite(lower) and np.isfinite(upper) and 0.0 < lower < upper):
            raise AMGError(f"Chebyshev: need 0 < lower < upper, got {lower!r}, {upper!r}")
        if rho is not None:
            rho = float(rho)
            if not (np.isfinite(rho) and rho > 0.0):
                raise AMGError(f"Chebyshev: rho must be a positive number, got {rho!r}")
        self.degree = int(degree)
        self.lower, self.upper = lower, upper
        self.iter = int(iter)
        self.rho = rho
        self.sweep_code = self.degree   # amgh_smoother_t.sweep carries the degree for this kind

    def bounds(self, rho=None):
        """(lo, hi) for the spectral radius rho (default: the one given at construction)."""
        rho = self.rho if rho is None else float(rho)
        if rho is None:
            raise AMGError("Chebyshev: no spectral radius given")
        return self.lower * rho, self.upper * rho

    def c_bounds(self):
        """(lo, hi, relative) as amgh_set_chebyshev_bounds takes them."""
        if self.rho is None:
            return self.lower, self.upper, 1
        return (*self.bounds(), 0)

    @staticmethod
    def coefficients_of(degree, lo, hi):
        """The (c1, c2) pairs of the `degree` steps on [lo, hi]: d = c1 d + c2 D⁻¹(b - S x); c1 of step 1 is 0.  Host
        arithmetic in double, operation for operation what libamghip computes (amgh_chebyshev_coefficients)."""
        lo, hi = float(lo), float(hi)
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
            raise AMGError(f"Chebyshev: need 0 < lo < hi, got {lo!r}, {hi!r}")
        theta = (hi + lo) / 2.0
        delta = (hi - lo) / 2.0
        sigma = theta / delta
        rho = 1.0 / sigma
        out = [(0.0, 1.0 / theta)]
        for _ in range(1, int(degree)):
            rho_new = 1.0 / (2.0 * sigma - rho)
            out.append((rho_new * rho, 2.0 * rho_new / delta))
            rho = rho_new
        return out

    def coefficients(self, lo, hi):
        return self.coefficients_of(self.degree, lo, hi)

    def check_no_symmetry(self, A):
        # the estimate is a Lanczos process: it assumes a symmetric operator, and nothing here guesses for another one
        if self.rho is None:
            raise AMGError("Chebyshev: a NoSymmetry() hierarchy needs the spectral radius of D⁻¹A: pass rho=...")
        return None

    def __repr__(self):
        return (f"Chebyshev(degree={self.degree}, lower={self.lower}, upper={self.upper}, iter={self.iter}, "
                f"rho={self.rho})")
