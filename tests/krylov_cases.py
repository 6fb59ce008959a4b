"""Inputs of the Krylov solvers' edge tests, shared by tests/test_krylov_cases_host.py (CPU) and
tests/test_gpu_krylov_edges.py (GPU): operators whose row count covers every residue modulo the widest 16-byte vector
(four Float32), right-hand sides that put their weight into the tail rows, and the (case, restart) pairs the GPU tests
run.  A plain helper module (not a conftest), like gmres_ref.py."""
import numpy as np
import scipy.sparse as sp

VW = 4   # reals of the widest 16-byte vector (Float32); Float64 takes two


def upwind(m, dim, eps=0.01, v=(1.0, 0.6, 0.3)):
    """-eps Laplacian + first-order upwind v . grad on the unit square / cube, m points per direction, Dirichlet."""
    h = 1.0 / (m + 1)
    I = sp.identity(m, format="csr")
    lap = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m), format="csr") / h**2
    d = sp.diags([-1.0, 1.0], [-1, 0], shape=(m, m), format="csr") / h
    terms = []
    for axis in range(dim):
        ops = [I] * dim
        ops[axis] = eps * lap + v[axis] * d
        t = ops[0]
        for o in ops[1:]:
            t = sp.kron(t, o, format="csr")
        terms.append(t)
    return sp.csc_matrix(sum(terms))


def block(n, bs, seed=7):
    """bs right-hand sides with different shapes and scales (column j of a wider block is the same column)."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, max(bs, 16)))
    B[:, 1] = np.sin(np.arange(n) * 0.37) + 2.0
    B[:, 2] *= 1e3
    return np.asfortranarray(B[:, :bs])


def random_nonsymmetric(n, seed=7):
    """The random nonsymmetric operator of test_gpu_gmres.test_no_preconditioner_against_checker, at any n."""
    rng = np.random.default_rng(seed)
    return sp.csc_matrix(sp.random(n, n, 0.003, random_state=rng) + 3 * sp.identity(n) + sp.diags(np.ones(n - 1), 1))


def small_nonsymmetric(n):
    """A dense-ish nonsymmetric operator smaller than one Float32 vector (n = 1, 3)."""
    M = 3.0 * np.eye(n) + np.diag(np.ones(n - 1), 1) - 0.5 * np.diag(np.ones(n - 1), -1)
    M[n - 1, 0] += 0.25
    return sp.csc_matrix(M)


# ---- operators by residue n % 4 --------------------------------------------------------------------------------------
# GMRES (nonsymmetric).  m^dim is never 2 mod 4: residue 2 is the random operator.
GMRES_CASES = {
    "upwind_50x50": lambda: upwind(50, 2),               # 2500, residue 0
    "upwind_51x51": lambda: upwind(51, 2),               # 2601, residue 1
    "random_2002": lambda: random_nonsymmetric(2002),    # 2002, residue 2
    "upwind_23^3": lambda: upwind(23, 3),                # 12167, residue 3
}
GMRES_ROWS = {"upwind_50x50": 2500, "upwind_51x51": 2601, "random_2002": 2002, "upwind_23^3": 12167}
# block PCG (symmetric positive definite): the shape handed to poisson()
POISSON_CASES = {
    "poisson_50x50": (50, 50),         # 2500, residue 0
    "poisson_51x51": (51, 51),         # 2601, residue 1
    "poisson_50x51": (50, 51),         # 2550, residue 2
    "poisson_23^3": (23, 23, 23),      # 12167, residue 3
}
ODD_POISSON = ["poisson_51x51", "poisson_23^3"]
SCALAR_POISSON = ["poisson_51x51", "poisson_50x51", "poisson_23^3"]    # n % 4 != 0: one real at a time in both precisions
CAPPED_M = 81   # 81^3 = 531441 rows: odd, and more than the 2 x 262144 at which the Float64 block count is capped

# The tails runs: restart 10, preconditioner off.  At reltol 1e-8 the 2-D upwind operators take 16 near-stagnating restarts
# and the reference's own history then moves by 8 to 15 times the GPU tolerance when the summation order changes (measured
# with reverse_system); at 1e-6 it moves by less than 0.05 of it, still over 12 or more restarts.
TAILS_RESTART, TAILS_RELTOL, TAILS_RELTOL_F32 = 10, 1e-6, 1e-4
# The width runs, preconditioner off: every instantiation of the accumulator count KC (8, 16, 32, 64) at its first and last
# k, on odd n.  (case, restart, reltol, maxiter).  reltol is 1e-8 but for restart 64 on 23^3 rows, which converges in 62
# steps at 1e-8 and so runs to 1e-10 (81 steps: k = 64 and a restart).  On 2601 rows the runs at restart 8, 9, 16 and 32
# stop after four cycles and three steps: run to 1e-8 their late, near-stagnating cycles amplify a change of summation
# order in the reference itself to between 2 and 1400 times the GPU tolerance (restart 17, 33 and 64 do not).
WIDTH_RESTARTS = [8, 9, 16, 17, 32, 33, 64]
WIDTH_RUNS = ([("upwind_23^3", r, 1e-10 if r == 64 else 1e-8, None) for r in WIDTH_RESTARTS]
              + [("upwind_51x51", r, 1e-8, None if r in (17, 33, 64) else 4 * r + 3) for r in WIDTH_RESTARTS])
# the Float32 run at restart 64: a tolerance Float32 can meet that still takes more than 32 steps
F32_WIDTH = ("upwind_51x51", 64, 1e-5)
# stops inside a cycle
STOP_CASE, STOP_RESTART = "upwind_51x51", 12


def gmres_operator(name):
    A = GMRES_CASES[name]()
    assert A.shape[0] == GMRES_ROWS[name]
    return A


def tail_heavy(n):
    """Zero except in the last max(n % 4, 1) + 1 rows, plus 1e-3 cos(i) everywhere (so that the Krylov space is not
    degenerate).  With the preconditioner off v1 = b / |b|: the rows past the last whole vector carry almost all of every
    dot product, and a kernel that drops or double-counts them is wrong by O(1), not by 1 / n."""
    b = 1e-3 * np.cos(np.arange(n, dtype=np.float64))
    t = min(max(n % VW, 1) + 1, n)
    b[n - t:] += 1.0 + np.arange(t)
    return b


def tail_block(n, bs):
    """block() with the tail-heavy vector as column 0, a zero column (bs >= 2) and the tail-heavy vector scaled by 1e3
    (bs >= 3); the other columns are block()'s."""
    B = block(n, bs).copy(order="F")
    B[:, 0] = tail_heavy(n)
    if bs >= 2:
        B[:, 1] = 0.0
    if bs >= 3:
        B[:, 2] = 1e3 * tail_heavy(n)
    return B


def staggered_block(n, bs):
    """Up to 64 columns (column j of a wider block is the same column): the tail-heavy vector, then random columns,
    every fifth one smooth, column j scaled by 10^-(j % 7).  With an abstol next to the reltol the scale moves the
    iteration at which a column meets its tolerance max(reltol |b_j|, abstol)."""
    rng = np.random.default_rng(64)
    B = np.asfortranarray(rng.standard_normal((n, 64)))
    i = np.arange(n)
    for j in range(64):
        if j % 5 == 4:
            B[:, j] = np.sin(i * (0.01 + 0.003 * j)) + 0.5
        B[:, j] *= 10.0 ** -(j % 7)
    B[:, 0] = tail_heavy(n)
    return np.asfortranarray(B[:, :bs])


def staggered_abstol(B):
    return 1e-9 * float(np.max(np.linalg.norm(B, axis=0)))


def reversed_hierarchy(ml):
    """The hierarchy of the system with rows and columns reversed on every level (the same splitting and weights, so
    the same preconditioner wherever the smoothers do not depend on the order of the rows, as Jacobi's)."""
    import amg_amd as AMG
    rev = lambda M: AMG.SparseMatrixCSC.from_scipy(sp.csc_matrix(M.to_scipy()[::-1, :][:, ::-1]))   # noqa: E731
    levels = [AMG.Level(rev(l.A), rev(l.P), rev(l.R), l.presmoother, l.postsmoother) for l in ml.levels]
    fA = rev(ml.final_A)
    return AMG.MultiLevel(levels, fA, type(ml.coarse_solver)(fA), ml.presmoother, ml.postsmoother, ml.symmetry,
                          method=ml.method)


def poisson_hierarchy(name, smoother="gs", dtype=None):
    """ruge_stuben on a POISSON_CASES operator: the default symmetric Gauss-Seidel, or Jacobi(2/3)."""
    import amg_amd as AMG
    A = AMG.poisson(POISSON_CASES[name])
    if dtype is not None:
        A = AMG.SparseMatrixCSC.from_scipy(A.to_scipy().astype(dtype))
    if smoother == "jacobi":
        jac = AMG.Jacobi(2.0 / 3.0)
        return AMG.ruge_stuben(A, presmoother=jac, postsmoother=jac)
    return AMG.ruge_stuben(A)


def reverse_system(A, b):
    """The same system with rows and columns reversed: another summation order in every product and norm."""
    A = sp.csr_matrix(A)
    Ar = sp.csr_matrix(A[::-1, :][:, ::-1])
    return Ar, np.ascontiguousarray(np.asarray(b)[::-1])
