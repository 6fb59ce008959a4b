"""The Chebyshev polynomial smoother on the GPU against its host restatement (tests/chebyshev_ref.py): the stand-alone
smoother, the cycle and the solvers on hierarchies that carry it, the spectral-radius estimate, the setup paths and the
argument errors.  Tests that compare numbers pass `rho` (a dense eigensolve), so that the estimate and the smoother are
tested separately.  Tolerance: 1e-10 of max|x| of the reference, the project's GPU-versus-CPU bar."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_amd as AMG
import chebyshev_ref as R
from amg_amd.device import DeviceBuffer, DeviceCSR, DeviceHierarchy
from conftest import load_csc, load_npz, uniform

pytestmark = pytest.mark.gpu

TOL = 1e-10
F32_TOL = 5e-5          # tests/test_gpu_float32.py
CYCLES = {"V": AMG.V, "W": AMG.W, "F": AMG.F}


def err(x, ref):
    return float(np.max(np.abs(np.asarray(x, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))


def operators():
    return {"poisson1000": AMG.poisson(1000), "poisson50x50": AMG.poisson((50, 50)), "poisson16^3": AMG.poisson((16, 16, 16)),
            "randlap": load_csc("randlap"), "lin_elastic_2d": load_csc("lin_elastic_2d")}


def sym_radius(S):
    """max |eig(D^-1 S)| of a symmetric S with a positive diagonal: dense eigensolve of D^-1/2 S D^-1/2."""
    S = sp.csr_matrix(S)
    q = sp.diags(1.0 / np.sqrt(S.diagonal()))
    return float(np.max(np.abs(np.linalg.eigvalsh((q @ S @ q).toarray()))))


def hierarchy_rho(ml):
    """One rho for every level: the largest spectral radius of D^-1 S over the levels (the bounds then cover each)."""
    return max(sym_radius(R.smoother_matrix(lev.A)) for lev in ml.levels)


def build(kind, pre, post, **kw):
    if kind == "rs":
        A = AMG.poisson((50, 50))
        return A, AMG.ruge_stuben(A, presmoother=pre, postsmoother=post, **kw)
    d = load_npz("lin_elastic_2d")
    A = load_csc("lin_elastic_2d")
    return A, AMG.smoothed_aggregation(A, B=d["B"], presmoother=pre, postsmoother=post, **kw)


def with_rho(kind, degree=3, iters=1, mixed=False):
    """(A, ml, reference hierarchy) with Chebyshev(rho = dense eigensolve) pre and post (mixed: Gauss-Seidel post)."""
    A, probe = build(kind, AMG.GaussSeidel(), AMG.GaussSeidel())
    rho = hierarchy_rho(probe)
    ch = AMG.Chebyshev(degree=degree, iter=iters, rho=rho)
    A, ml = build(kind, ch, AMG.GaussSeidel() if mixed else ch)
    return A, ml, R.RefHierarchy(ml, [ch.bounds()] * len(ml.levels))


# ---- the stand-alone smoother ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(operators()))
def test_standalone_smoother_against_the_reference(name):
    A = operators()[name]
    S = R.smoother_matrix(A)
    rho = sym_radius(S)
    n = A.m
    b = uniform(n, 3) - 0.5
    for degree in range(1, 6):
        for iters in (1, 2):
            ch = AMG.Chebyshev(degree=degree, iter=iters, rho=rho)
            for x0 in (uniform(n, 7) - 0.3, np.zeros(n)):
                x = x0.copy()
                ch(A, x, b, AMG.HermitianSymmetry())
                ref = R.smooth(S, x0, b, degree, *ch.bounds(), iters)
                e = err(x, ref)
                print(f"{name} degree {degree} iter {iters}: {e:.2e}")
                assert e <= TOL, (name, degree, iters, e)
    # Float32 against the Float64 reference
    ch = AMG.Chebyshev(degree=3, iter=2, rho=rho)
    x0 = uniform(n, 7) - 0.3
    x = x0.astype(np.float32)
    from amg_amd.device import smooth_standalone
    smooth_standalone(ch, A, x, b.astype(np.float32), None, dtype=np.float32)
    assert x.dtype == np.float32 and err(x, R.smooth(S, x0, b, 3, *ch.bounds(), 2)) <= F32_TOL


def test_rows_without_a_diagonal_come_back_untouched():
    A = AMG.poisson((20, 20)).to_scipy().tolil()
    dead = [0, 17, 211, 399]
    for i in dead:
        A[i, i] = 0.0
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    Ac = AMG.SparseMatrixCSC.from_scipy(A)
    n = A.shape[0]
    x0, b = uniform(n, 1) - 0.5, uniform(n, 2)
    ch = AMG.Chebyshev(degree=4, iter=2, rho=2.0)
    x = x0.copy()
    ch(Ac, x, b)
    assert np.array_equal(x[dead], x0[dead])
    assert err(x, R.smooth(R.smoother_matrix(Ac), x0, b, 4, *ch.bounds(), 2)) <= TOL
    # a stored zero on the diagonal is the same case
    B = AMG.poisson((20, 20)).to_scipy().tocsc()
    B.data[B.indices == np.repeat(np.arange(n), np.diff(B.indptr))] *= (np.arange(n) % 50 != 0)
    Bc = AMG.SparseMatrixCSC.from_scipy(B)
    y = x0.copy()
    ch(Bc, y, b)
    assert np.array_equal(y[::50], x0[::50])


def test_first_step_on_a_zero_vector_skips_the_matrix_pass_bitwise():
    """Every pre-smoother below the fine level (and the fine one of ldiv!) starts from x = 0: step 1 is then
    d = c2 ((b - 0) / diag), x = 0 + d — the stream kernel's expression with a row sum of +0, by a vector kernel.
    Bitwise the full step (tunable jacobi_zero = 0), V / W / F, blocks of right-hand sides."""
    lib = AMG.hip_lib()
    A = AMG.poisson((48, 40))
    b = uniform(A.m, 12) - 0.4
    B = np.stack([b, uniform(A.m, 13), -b], axis=1)
    for degree, iters in ((1, 1), (3, 2)):
        ch = AMG.Chebyshev(degree=degree, iter=iters, rho=2.0)
        ml = AMG.smoothed_aggregation(A, presmoother=ch, postsmoother=ch)
        out = {}
        for flag in (1, 0):
            assert lib.amgh_debug_set_tunable(b"jacobi_zero", flag) == 0
            try:
                dev1, dev3 = DeviceHierarchy(ml, 0, 1), DeviceHierarchy(ml, 0, 3)
                for cyc in (0, 1, 2):
                    out[(flag, cyc, 1)] = dev1.precond_apply(b, cyc)
                    out[(flag, cyc, 3)] = dev3.precond_apply(B, cyc)
            finally:
                lib.amgh_debug_set_tunable(b"jacobi_zero", 1)
        for (flag, cyc, bs), v in out.items():
            if flag == 1:
                assert np.array_equal(v, out[(0, cyc, bs)]), (degree, cyc, bs)
        ref = R.RefHierarchy(ml, [ch.bounds()] * len(ml.levels))
        assert err(out[(1, 0, 1)], ref.precond(b)) <= TOL


def test_value_coded_and_plain_columns_give_the_same_step_bitwise():
    """poisson((64,64,64)) has 2^18 rows and two distinct values: the step streams 4-byte coded columns (tunable
    stream_code = 1, the default) or the 12-byte entries (0) — the same products in the same order."""
    lib = AMG.hip_lib()
    A = AMG.poisson((64, 64, 64))
    n = A.m
    x0, b = uniform(n, 5) - 0.5, uniform(n, 6)
    ch = AMG.Chebyshev(degree=3, rho=2.0)
    lo, hi = ch.bounds()
    op = DeviceCSR(n, n, A.colptr, A.rowval, A.nzval)
    bd, work = DeviceBuffer(n, 0, b), DeviceBuffer(2 * n, 0)
    got = {}
    for flag in (1, 0, 1):
        assert lib.amgh_debug_set_tunable(b"stream_code", flag) == 0
        try:
            xd = DeviceBuffer(n, 0, x0)
            assert lib.amgh_csr_chebyshev_d(op.h, 3, lo, hi, xd.ptr, bd.ptr, work.ptr, None) == 0
            op.sync()
            got.setdefault(flag, []).append(xd.download())
        finally:
            lib.amgh_debug_set_tunable(b"stream_code", 1)
    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][0], got[1][1])
    assert err(got[1][0], R.smooth(R.smoother_matrix(A), x0, b, 3, lo, hi)) <= TOL
    # the level smoother of a hierarchy takes the same two paths
    ml = AMG.ruge_stuben(A, presmoother=ch, postsmoother=ch)
    dev = ml.device()
    assert lib.amgh_debug_coded_ops(dev.h, 0) & 8 and not lib.amgh_debug_coded_ops(dev.h, 1) & 8   # (level 1 is below 2^18 rows)
    y1 = dev.smooth(0, 0, x0, b)
    lib.amgh_debug_set_tunable(b"stream_code", 0)
    try:
        assert not lib.amgh_debug_coded_ops(dev.h, 0) & 8
        y0 = dev.smooth(0, 0, x0, b)
    finally:
        lib.amgh_debug_set_tunable(b"stream_code", 1)
    assert np.array_equal(y0, y1) and np.array_equal(y1, got[1][0])


# ---- cycles and solvers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind", ["rs", "sa"])
def test_one_cycle_and_a_converged_solve_against_the_reference(kind, mixed):
    A, ml, ref = with_rho(kind, degree=3, mixed=mixed)
    n = A.m
    b = uniform(n, 21) - 0.5
    for cyc in "VWF":
        x1 = AMG._solve(ml, b, CYCLES[cyc](), maxiter=1, calculate_residual=False)
        e1 = err(x1, ref.solve(b, cyc, maxiter=1, calculate_residual=False)[0])
        x, hist = AMG._solve(ml, b, CYCLES[cyc](), log=True, reltol=1e-10)
        xr, hr = ref.solve(b, cyc, reltol=1e-10)
        print(f"{kind} mixed={mixed} {cyc}: one cycle {e1:.2e}, solve {err(x, xr):.2e}, {len(hist) - 1} cycles")
        assert e1 <= TOL
        assert len(hist) == len(hr) and err(x, xr) <= TOL
        assert hist[-1] <= 1e-10 * hist[0]
        z = AMG.aspreconditioner(ml, CYCLES[cyc]()).ldiv(b)
        assert err(z, ref.precond(b, cyc)) <= TOL


@pytest.mark.parametrize("kind", ["rs", "sa"])
def test_collapsed_tail_and_graph_replay(kind):
    """The smoother is linear in (x, b): the collapsed coarse tail (built from the library's own recursion) keeps working,
    against the reference cycle and against the per-level cycle of the same handle; a graph-replayed cycle is bitwise the
    eager one."""
    lib = AMG.hip_lib()
    A, ml, ref = with_rho(kind, degree=2, iters=2)
    b = uniform(A.m, 31) - 0.5
    lib.amgh_debug_set_tunable(b"tail_dense_rows", 6144)
    lib.amgh_debug_set_tunable(b"tail_dense", 1)
    try:
        dev = DeviceHierarchy(ml, 0, 1)
        assert dev.tail_dense_info(0)[0] >= 0
        for cyc, code in (("V", 0), ("W", 1), ("F", 2)):
            zt = dev.precond_apply(b, code)
            lib.amgh_debug_set_tunable(b"tail_dense", 0)
            zl = dev.precond_apply(b, code)
            lib.amgh_debug_set_tunable(b"tail_dense", 1)
            zr = ref.precond(b, cyc)
            print(f"{kind} {cyc}: tail {err(zt, zr):.2e} per level {err(zl, zr):.2e}")
            assert err(zt, zr) <= TOL and err(zl, zr) <= TOL
    finally:
        lib.amgh_debug_set_tunable(b"tail_dense_rows", 0)
        lib.amgh_debug_set_tunable(b"tail_dense", 1)
    dev = DeviceHierarchy(ml, 0, 1)      # per level (tail_dense_rows = 0)
    n = A.m
    bd, zd = DeviceBuffer(n, 0, b), DeviceBuffer(n, 0)
    for code in (0, 1, 2):
        assert lib.amgh_set_use_graph(dev.h, 0) == 0
        assert lib.amgh_precond_apply_d(dev.h, bd.ptr, zd.ptr, code) == 0
        lib.amgh_dev_sync(0)
        eager = zd.download()
        assert lib.amgh_set_use_graph(dev.h, 1) == 0
        for _ in range(4):
            assert lib.amgh_precond_apply_d(dev.h, bd.ptr, zd.ptr, code) == 0
            lib.amgh_dev_sync(0)
            assert np.array_equal(zd.download(), eager)
        assert lib.amgh_set_use_graph(dev.h, 0) == 0


@pytest.mark.parametrize("bs", [2, 3, 8])
def test_blocks_of_right_hand_sides_equal_their_columns(bs):
    A, ml, ref = with_rho("rs", degree=3)
    n = A.m
    B = np.stack([uniform(n, 40 + j) - 0.5 for j in range(bs)], axis=1)
    X = AMG._solve(ml, B, reltol=1e-9)
    Xc = AMG.cg(A, B, Pl=AMG.aspreconditioner(ml), reltol=1e-9)
    for j in range(bs):
        xj = AMG._solve(ml, B[:, j].copy(), reltol=1e-9)
        assert err(X[:, j], xj) <= TOL, (bs, j)
        assert err(Xc[:, j], AMG.cg(A, B[:, j].copy(), Pl=AMG.aspreconditioner(ml), reltol=1e-9)) <= TOL, (bs, j)
    assert err(X[:, 0], ref.solve(B[:, 0], reltol=1e-9)[0]) <= TOL


@pytest.mark.parametrize("kind", ["rs", "sa"])
@pytest.mark.parametrize("cyc", ["V", "W", "F"])
def test_reference_acceptance_for_cycles(kind, cyc):
    """cycle_tests.jl:6-30 with the new smoother at its defaults (bounds from the device estimate): on poisson((50,50)),
    b = A 1, |b - A x| < 1e-8 |b| stand-alone and as cg preconditioner."""
    A = AMG.poisson((50, 50))
    b = A @ np.ones(A.m)
    ch = AMG.Chebyshev()
    f = AMG.ruge_stuben if kind == "rs" else AMG.smoothed_aggregation
    ml = f(A, presmoother=ch, postsmoother=ch)
    x = AMG._solve(ml, b, CYCLES[cyc](), reltol=1e-8)
    assert np.linalg.norm(b - A @ x) < 1e-8 * np.linalg.norm(b)
    x, info = AMG.cg(A, b, Pl=AMG.aspreconditioner(ml, CYCLES[cyc]()), reltol=1e-8, log=True)
    assert info["isconverged"] and np.linalg.norm(b - A @ x) < 1e-8 * np.linalg.norm(b)
    lo, hi = ml.device().chebyshev_bounds(0, 0)
    rho = sym_radius(R.smoother_matrix(A))
    assert hi >= rho and lo * 30.0 <= rho * (1 + 1e-10) and abs(hi / lo - 33.0) < 1e-9


@pytest.mark.parametrize("kind", ["rs", "sa"])
@pytest.mark.parametrize("cyc", ["V", "W", "F"])
def test_cg_iteration_counts_and_symmetry_of_the_preconditioner(kind, cyc):
    A, ml, ref = with_rho(kind, degree=3)
    n = A.m
    b = A @ np.ones(n)
    As = A.to_scipy().tocsr()
    x, info = AMG.cg(A, b, Pl=AMG.aspreconditioner(ml, CYCLES[cyc]()), reltol=1e-8, log=True)
    xr, hr, itr = R.pcg(As, b, lambda r: ref.precond(r, cyc), reltol=1e-8)
    assert info["isconverged"] and info["iters"] == itr, (info["iters"], itr)
    assert err(x, xr) <= 1e-8
    u, v = uniform(n, 50) - 0.5, uniform(n, 51) - 0.5
    p = AMG.aspreconditioner(ml, CYCLES[cyc]())
    Mu, Mv = p.ldiv(u), p.ldiv(v)
    a, c = float(u @ Mv), float(Mu @ v)
    size = np.linalg.norm(u) * np.linalg.norm(Mv)
    print(f"{kind} {cyc}: <u, M v> - <M u, v> = {abs(a - c):.2e} of {size:.2e}")
    if cyc != "F":   # (an F-cycle visits V after F on the way up only: not a symmetric operator, with any smoother)
        assert abs(a - c) <= 1e-10 * size


def test_gmres_on_upwind_convection_diffusion_with_a_nosymmetry_hierarchy():
    """The operator of test_upwind_convection_diffusion_2d.  rho = max |eig(D^-1 A)|: the operator has 65 536 rows, a dense
    eigensolve is out of reach, so ARPACK finds the eigenvalue of largest magnitude; Gershgorin bounds it by 2 (every row
    of D^-1 A has absolute sum <= 2), which the test checks.  The residual check is that test's: the preconditioned
    residual of the solution within the tolerance."""
    import scipy.sparse.linalg as spla
    from test_gpu_gmres import upwind
    A = upwind(256, 2)
    Dinv = sp.diags(1.0 / A.diagonal())
    lam = spla.eigs((Dinv @ A).tocsr(), k=1, which="LM", tol=1e-8, return_eigenvectors=False)
    rho = float(np.max(np.abs(lam)))
    assert 1.0 < rho <= 2.0 + 1e-12
    ch = AMG.Chebyshev(degree=3, rho=rho)
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry(), presmoother=ch, postsmoother=ch)
    b = np.ones(A.shape[0])
    x, info = AMG.gmres(A, b, Pl=AMG.aspreconditioner(ml), restart=20, reltol=1e-8, log=True)
    assert info["isconverged"]
    p = AMG.aspreconditioner(ml)
    tol = 1e-8 * np.linalg.norm(p.ldiv(b))
    assert np.linalg.norm(p.ldiv(b - A @ x)) <= tol * (1 + 1e-6)


# ---- the estimate ------------------------------------------------------------------------------------------------------
def test_spectral_radius_estimate_never_exceeds_and_covers_the_spectrum():
    mats = dict(operators(), thing=load_csc("thing"), **{"poisson24^3": AMG.poisson((24, 24, 24))})
    for name, A in mats.items():
        S = R.smoother_matrix(A)
        if S.shape[0] <= 4096:
            true = sym_radius(S)
        else:   # 24^3: the 7-point stencil's D^-1 A has the spectrum 1 - (cos + cos + cos) / 3 in closed form
            true = 1.0 + np.cos(np.pi / 25.0)
        est = AMG.approximate_spectral_radius(A)
        again = AMG.approximate_spectral_radius(A)
        host = R.lanczos_radius(S, 15)
        print(f"{name}: estimate / true = {est / true:.4f} (host restatement {host / true:.4f})")
        assert est == again
        assert est <= true * (1 + 1e-10) and 1.1 * est >= true, (name, est, true)
        # (the device adds its sums in another order than numpy: roundings of 1e-16 per step, which 15 steps of the recurrence
        # amplify by far less than ten orders of magnitude on the converged top Ritz value)
        assert abs(est - host) <= 1e-6 * true
        # through a pushed level
        ch = AMG.Chebyshev()
        ml = AMG.ruge_stuben(A, presmoother=ch, postsmoother=ch, max_levels=2)
        if ml.levels:
            dev = ml.device()
            assert dev.spectral_radius(0) == est
            lo, hi = dev.chebyshev_bounds(0, 1)
            assert lo == est * (1.0 / 30.0) and hi == est * 1.1


# ---- setup paths ---------------------------------------------------------------------------------------------------------
def test_gpu_setup_path_gives_the_host_built_cycle_bitwise():
    A = AMG.poisson((50, 50))
    b = uniform(A.m, 60) - 0.5
    ch = AMG.Chebyshev()
    host = AMG.ruge_stuben(A, presmoother=ch, postsmoother=ch)
    gpu = AMG.ruge_stuben(A, setup="gpu", device=0, presmoother=ch, postsmoother=ch)
    assert len(gpu.levels) == len(host.levels)
    for cyc in (AMG.V(), AMG.W(), AMG.F()):
        assert np.array_equal(AMG.aspreconditioner(gpu, cyc).ldiv(b), AMG.aspreconditioner(host, cyc).ldiv(b))
    assert gpu.device().chebyshev_bounds(1, 0) == host.device().chebyshev_bounds(1, 0)
    # solve / init / the preconditioner builders take the configuration too
    x = AMG.solve(A, b, AMG.RugeStubenAMG(), presmoother=ch, postsmoother=ch, reltol=1e-8)
    assert np.linalg.norm(b - A @ x) < 1e-8 * np.linalg.norm(b)
    x = AMG.solve(A, b, AMG.SmoothedAggregationAMG(), presmoother=ch, postsmoother=ch, reltol=1e-8)
    assert np.linalg.norm(b - A @ x) < 1e-8 * np.linalg.norm(b)
    for builder in (AMG.RugeStubenPreconBuilder, AMG.SmoothedAggregationPreconBuilder):
        p = builder(presmoother=ch, postsmoother=ch)(A)[0]
        x, info = AMG.cg(A, b, Pl=p, reltol=1e-8, log=True)
        assert info["isconverged"]


# ---- errors ----------------------------------------------------------------------------------------------------------------
def _push_poisson(lib, h, pre, post, zero_diag=False):
    A = AMG.poisson((12, 12))
    ml = AMG.ruge_stuben(A, max_levels=2)
    lev = ml.levels[0]
    Ar, Ac, Av = lev.A.csr_arrays()
    Av = np.array(Av, copy=True)
    if zero_diag:
        Av[Ac == np.repeat(np.arange(lev.A.m), np.diff(Ar))] = 0.0
    Pr, Pc, Pv = lev.R.colptr, lev.R.rowval, lev.R.nzval
    Rr, Rc, Rv = lev.P.colptr, lev.P.rowval, lev.P.nzval
    p = lambda a: a.ctypes.data   # noqa: E731
    rc = lib.amgh_push_level(h, lev.A.m, lev.P.n, p(Ar), p(Ac), p(Av), None, None, None, p(Pr), p(Pc), p(Pv), p(Rr), p(Rc), p(Rv),
                             C.byref(pre), C.byref(post))
    return rc, ml


def test_argument_errors_leave_the_handle_usable():
    from amg_amd._libs import amgh_smoother_t
    lib = AMG.hip_lib()
    h = C.c_void_p()
    assert lib.amgh_create(C.byref(h), 0, 1) == 0
    try:
        good = amgh_smoother_t(4, 3, 1, 0, 0.0)
        for degree in (0, -1, 17):
            assert _push_poisson(lib, h, amgh_smoother_t(4, degree, 1, 0, 0.0), good)[0] == -2
        assert lib.amgh_num_levels(h) == 0
        gs = amgh_smoother_t(1, 2, 1, 0, 1.0)
        rc, ml = _push_poisson(lib, h, good, gs)
        assert rc == 0 and lib.amgh_num_levels(h) == 1
        for lo, hi in ((0.0, 1.0), (-0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.1, float("inf"))):
            assert lib.amgh_set_chebyshev_bounds(h, 0, 0, lo, hi, 0) == -2
        assert lib.amgh_set_chebyshev_bounds(h, 0, 1, 0.1, 2.0, 0) == -2     # the post side is Gauss-Seidel
        assert lib.amgh_set_chebyshev_bounds(h, 1, 0, 0.1, 2.0, 0) == -2     # no such level
        assert lib.amgh_set_chebyshev_bounds(h, 0, 2, 0.1, 2.0, 0) == -2
        assert lib.amgh_set_chebyshev_bounds(h, 0, 0, 0.07, 2.2, 0) == 0
        fA = ml.final_A
        fr, fc, fv = fA.csr_arrays()
        op = np.asfortranarray(ml.coarse_solver.dense_operator())
        assert lib.amgh_set_coarse(h, fA.m, fr.ctypes.data, fc.ctypes.data, fv.ctypes.data, op.ctypes.data) == 0
        assert lib.amgh_finalize(h) == 0
        assert lib.amgh_set_chebyshev_bounds(h, 0, 0, 0.07, 2.2, 0) == -3    # finalized
        lo, hi = C.c_double(), C.c_double()
        assert lib.amgh_chebyshev_bounds(h, 0, 0, C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (0.07, 2.2)
        assert lib.amgh_chebyshev_bounds(h, 0, 1, C.byref(lo), C.byref(hi)) == -2
        n = ml.levels[0].A.m
        b = uniform(n, 70)
        x = np.zeros(n)
        it = C.c_int(0)
        assert lib.amgh_solve(h, b.ctypes.data, x.ctypes.data, 0, 50, 0.0, 1e-8, 1, None, C.byref(it)) == 0
        A0 = ml.levels[0].A
        assert np.linalg.norm(b - A0 @ x) <= 1e-8 * np.linalg.norm(b)
    finally:
        lib.amgh_destroy(h)
    # an estimate that is not positive (all-zero diagonal): amgh_finalize refuses, bounds given by hand then pass
    h = C.c_void_p()
    assert lib.amgh_create(C.byref(h), 0, 1) == 0
    try:
        good = amgh_smoother_t(4, 2, 1, 0, 0.0)
        rc, ml = _push_poisson(lib, h, good, good, zero_diag=True)
        assert rc == 0
        fA = ml.final_A
        fr, fc, fv = fA.csr_arrays()
        op = np.asfortranarray(ml.coarse_solver.dense_operator())
        assert lib.amgh_set_coarse(h, fA.m, fr.ctypes.data, fc.ctypes.data, fv.ctypes.data, op.ctypes.data) == 0
        assert lib.amgh_finalize(h) == -2
        assert lib.amgh_set_chebyshev_bounds(h, 0, 0, 0.1, 2.0, 0) == 0 and lib.amgh_set_chebyshev_bounds(h, 0, 1, 0.1, 2.0, 0) == 0
        assert lib.amgh_finalize(h) == 0
        n = ml.levels[0].A.m
        b, x = uniform(n, 71), np.zeros(n)
        assert lib.amgh_precond_apply(h, b.ctypes.data, x.ctypes.data, 0) == 0 and np.all(np.isfinite(x))
    finally:
        lib.amgh_destroy(h)
    # stand-alone operator
    A = AMG.poisson((12, 12))
    op = DeviceCSR(A.m, A.n, A.colptr, A.rowval, A.nzval)
    xd, bd, wd = DeviceBuffer(A.m, 0, np.zeros(A.m)), DeviceBuffer(A.m, 0, np.ones(A.m)), DeviceBuffer(2 * A.m, 0)
    for degree, lo, hi in ((0, 0.1, 2.0), (17, 0.1, 2.0), (2, 0.0, 2.0), (2, 2.0, 2.0), (2, 3.0, 2.0), (2, float("nan"), 2.0)):
        assert lib.amgh_csr_chebyshev_d(op.h, degree, lo, hi, xd.ptr, bd.ptr, wd.ptr, None) == -2
    assert lib.amgh_csr_chebyshev_d(op.h, 2, 0.1, 2.0, xd.ptr, bd.ptr, None, None) == -2
    assert lib.amgh_csr_chebyshev_d(op.h, 2, 0.1, 2.0, xd.ptr, bd.ptr, wd.ptr, None) == 0
    op.sync()
    assert err(xd.download(), R.smooth(R.smoother_matrix(A), np.zeros(A.m), np.ones(A.m), 2, 0.1, 2.0)) <= TOL
    Z = sp.csc_matrix(sp.diags([np.ones(9)], [1], shape=(10, 10)) + sp.diags([np.ones(9)], [-1], shape=(10, 10)))
    Zc = AMG.SparseMatrixCSC.from_scipy(Z)
    with pytest.raises(AMG.AMGError):
        AMG.approximate_spectral_radius(Zc)
    assert AMG.approximate_spectral_radius(A) > 1.0


def test_sharded_push_refuses_the_kind():
    from amg_amd._libs import amgh_smoother_t
    lib = AMG.hip_lib()
    g, d = C.c_void_p(), C.c_void_p()
    assert lib.amgh_local_group_create(C.byref(g), 1) == 0
    try:
        assert lib.amgh_dist_create_local(C.byref(d), 0, 0, g) == 0
        try:
            A = AMG.poisson((12, 12))
            ml = AMG.ruge_stuben(A, max_levels=2)
            lev = ml.levels[0]
            n, nc = lev.A.m, lev.P.n
            Ar, Ac, Av = lev.A.csr_arrays()
            Pr, Pc, Pv = lev.R.colptr, lev.R.rowval, lev.R.nzval
            Rr, Rc, Rv = lev.P.colptr, lev.P.rowval, lev.P.nzval
            cuts, ccuts = np.array([0, n], dtype=np.int64), np.array([0, nc], dtype=np.int64)
            p = lambda a: a.ctypes.data   # noqa: E731
            ch, gs = amgh_smoother_t(4, 3, 1, 0, 0.0), amgh_smoother_t(1, 2, 1, 0, 1.0)
            args = (d, n, nc, p(cuts), p(ccuts), p(Ar), p(Ac), p(Av), None, None, None, p(Pr), p(Pc), p(Pv), p(Rr), p(Rc), p(Rv))
            assert lib.amgh_dist_push_level(*args, C.byref(ch), C.byref(gs)) == -5
            assert lib.amgh_dist_push_level(*args, C.byref(gs), C.byref(ch)) == -5
            assert lib.amgh_dist_num_sharded_levels(d) == 0
            assert lib.amgh_dist_push_level(*args, C.byref(gs), C.byref(gs)) == 0      # the handle is still usable
            assert lib.amgh_dist_num_sharded_levels(d) == 1
        finally:
            lib.amgh_dist_destroy(d)
    finally:
        lib.amgh_local_group_destroy(g)


# ---- full size -------------------------------------------------------------------------------------------------------------
def test_256cubed_degree_3_v_cycle_against_the_reference_cycle():
    """One degree-3 Chebyshev V-cycle on ruge_stuben(poisson((256,256,256))) against the scipy cycle (a few seconds of
    host SpMV).  rho = 2: the 7-point stencil's D^-1 A has its spectrum in (0, 2) in closed form; the comparison itself
    holds for any bounds (both sides apply the same polynomial)."""
    A = AMG.poisson((256, 256, 256))
    ch = AMG.Chebyshev(degree=3, rho=2.0)
    ml = AMG.ruge_stuben(A, setup="gpu", device=0, presmoother=ch, postsmoother=ch)
    ref = R.RefHierarchy(ml, [ch.bounds()] * len(ml.levels))
    b = uniform(A.m, 0)
    z = AMG.aspreconditioner(ml).ldiv(b)
    zr = ref.precond(b)
    e = err(z, zr)
    print(f"256^3 degree-3 V-cycle: {e:.2e}")
    assert e <= TOL
