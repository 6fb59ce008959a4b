"""The Krylov kernels (gmres_kernels.hpp, pcg_block_kernels.hpp) at the tails, widths and stops their own test files do
not reach: row counts of every residue modulo the 16-byte vector with right-hand sides that live in the tail rows
(tests/krylov_cases.py), Arnoldi steps past 32 columns, blocks of 17 to 64 right-hand sides, the scalar family of the
block-PCG kernels, an X off the 16-byte boundary, a NaN column, and the grid-stride second trip on 81^3 rows.
tests/test_krylov_cases_host.py shows on the CPU that the references reach these widths and are themselves stable to a
quarter of the tolerances used here, which are the project's: test_gpu_gmres.py's for GMRES, test_gpu_pcg_block.py's
check_columns for block PCG, test_gpu_float32.py's F32_TOL.

Not covered: the cap on the DGKS repetition (a second extra pass).  No input tried reaches it (I + eps N for eps down
to 1e-16, near-constant and steeply graded diagonals: gmres_ref gives the same counts with a cap of 1, 2 or 3)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_amd as AMG
import gmres_ref as G
import krylov_cases as K
from amg_amd.device import DeviceBuffer
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
F32_TOL = 5e-5
CYCLES = {"V": (AMG.V, 0), "W": (AMG.W, 1)}
_gm, _pb, _or = {}, {}, {}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---- GMRES -----------------------------------------------------------------------------------------------------------
def gmres_case(name, dtype=None):
    """(A, hierarchy) of a GMRES_CASES operator; the hierarchy is there for its handle (and for the cycle tests)."""
    key = (name, dtype)
    if key not in _gm:
        A = K.gmres_operator(name)
        if dtype is not None:
            A = sp.csc_matrix(A, dtype=dtype)
        _gm[key] = (A, AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry()))
    return _gm[key]


def check_gmres(A, dev, b, reorth=True, **kw):
    """The unpreconditioned device GMRES against gmres_ref with the same arguments: test_no_preconditioner_against_checker's
    tolerances, and the DGKS pass count."""
    st = {}
    xr, hr, itr = G.gmres(sp.csr_matrix(A), b, stats=st, **kw)
    x, hist, it = dev.gmres(b, use_precond=False, **kw)
    passes = dev.gmres_reorth_passes()
    dh = float(np.max(np.abs(hist - hr) / (1e-8 * hr + 1e-15 * hr[0]))) if len(hist) == len(hr) and hr[0] > 0 else -1.0
    print("gmres", A.shape[0], kw, "steps", it, itr, "reorth", passes, st, "hist/tol", dh, "x", rel(x, xr))
    assert it == itr and len(hist) == len(hr), (it, itr)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert np.all(np.abs(hist - hr) <= 1e-8 * hr + 1e-15 * hr[0]), dh
    assert rel(x, xr) <= 1e-8, rel(x, xr)
    if reorth:
        assert passes == st["reorth"], (passes, st)
    return x, hist, it, (xr, hr, itr)


@pytest.mark.parametrize("name", list(K.GMRES_CASES))
def test_gmres_tail_rows_float64(name):
    A, ml = gmres_case(name)
    b = K.tail_heavy(A.shape[0])
    x, hist, it, _ = check_gmres(A, ml.device(), b, restart=K.TAILS_RESTART, reltol=K.TAILS_RELTOL)
    assert it > K.TAILS_RESTART and np.linalg.norm(b - A @ x) <= 10 * K.TAILS_RELTOL * np.linalg.norm(b)


@pytest.mark.parametrize("name", list(K.GMRES_CASES))
def test_gmres_tail_rows_float32(name):
    """Step counts within 1 and x within 1e-3 of the Float64 reference on the same (Float32-valued) system, as
    test_float32_instance_issue95."""
    A32, ml32 = gmres_case(name, F32)
    b32 = K.tail_heavy(A32.shape[0]).astype(F32)
    A64, b64 = sp.csr_matrix(A32, dtype=np.float64), b32.astype(np.float64)
    xr, hr, itr = G.gmres(A64, b64, restart=K.TAILS_RESTART, reltol=K.TAILS_RELTOL_F32)
    x, hist, it = ml32.device(dtype=F32).gmres(b32, use_precond=False, restart=K.TAILS_RESTART, reltol=K.TAILS_RELTOL_F32)
    print("gmres f32", name, "steps", it, itr, "x", rel(x, xr), "h1", hist[1] / hr[1] - 1)
    assert x.dtype == F32 and abs(it - itr) <= 1, (it, itr)
    assert rel(x, xr) <= 1e-3, rel(x, xr)
    # the first step's estimate is one SpMV and one pass of the dot and update kernels from b: Float32 rounding only
    assert abs(hist[0] / hr[0] - 1) <= F32_TOL and abs(hist[1] / hr[1] - 1) <= F32_TOL


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", [np.float64, F32])
def test_gmres_smaller_than_one_vector(n, dtype):
    A = sp.csc_matrix(K.small_nonsymmetric(n), dtype=dtype)
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry())
    dev = ml.device(dtype=dtype) if dtype is F32 else ml.device()
    b = K.tail_heavy(n).astype(dtype)
    x, hist, it = dev.gmres(b, use_precond=False, restart=10, reltol=1e-12 if dtype is not F32 else 1e-5)
    xd = np.linalg.solve(A.toarray().astype(np.float64), b.astype(np.float64))
    print("small", n, dtype, it, hist, rel(x, xd))
    assert 1 <= it <= n and np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert rel(x, xd) <= (1e-10 if dtype is not F32 else 1e-5)
    if dtype is not F32:
        check_gmres(A, dev, b, restart=10, reltol=1e-12)


@pytest.mark.parametrize("name", ["upwind_51x51", "upwind_23^3"])
@pytest.mark.parametrize("cycle", ["V", "W"])
def test_gmres_tail_rows_with_a_cycle(name, cycle):
    """The odd upwind operators under their NoSymmetry ruge_stuben cycle, against gmres_ref with the oracle's precond:
    check_against_checker of test_gpu_gmres.py."""
    A, ml = gmres_case(name)
    b = K.tail_heavy(A.shape[0])
    cyc, code = CYCLES[cycle]
    oh = O.OracleHierarchy(ml)
    Pl = lambda r: oh.precond(r, code)   # noqa: E731
    xr, hr, itr = G.gmres(A, b, Pl=Pl, restart=3, reltol=1e-8)
    x, info = AMG.gmres(A, b, Pl=AMG.aspreconditioner(ml, cyc()), restart=3, reltol=1e-8, log=True)
    hist = np.concatenate([[np.linalg.norm(Pl(b))], info["resnorm"]])
    print("cycle", name, cycle, info["iters"], itr, rel(x, xr))
    assert info["iters"] == itr and info["isconverged"], (info["iters"], itr)
    assert len(hist) == len(hr) and np.all(np.abs(hist - hr) <= 1e-8 * np.abs(hr)), np.max(np.abs(hist - hr) / hr)
    assert rel(x, xr) <= 1e-8, rel(x, xr)
    assert np.linalg.norm(Pl(b - A @ x)) <= 1e-8 * hr[0] * (1 + 1e-6)


@pytest.mark.parametrize("name,restart,reltol,maxiter", K.WIDTH_RUNS)
def test_gmres_every_accumulator_count_at_its_first_and_last_width(name, restart, reltol, maxiter):
    """Restart 8 | 9, 16 | 17, 32 | 33, 64: the last k of gmres_dots_kernel / gmres_update_kernel <8>, <16>, <32>, <64> and
    the first k of the next one, on 2601 and 12167 rows (odd: the tail loop runs in every launch)."""
    A, ml = gmres_case(name)
    b = K.tail_heavy(A.shape[0])
    x, hist, it, _ = check_gmres(A, ml.device(), b, restart=restart, reltol=reltol, maxiter=maxiter)
    assert it >= restart


def test_gmres_restart_64_float32():
    name, restart, reltol = K.F32_WIDTH
    A32, ml32 = gmres_case(name, F32)
    b32 = K.tail_heavy(A32.shape[0]).astype(F32)
    xr, hr, itr = G.gmres(sp.csr_matrix(A32, dtype=np.float64), b32.astype(np.float64), restart=restart, reltol=reltol)
    x, hist, it = ml32.device(dtype=F32).gmres(b32, use_precond=False, restart=restart, reltol=reltol)
    print("gmres f32 restart 64", "steps", it, itr, "x", rel(x, xr))
    assert it > 64 and abs(it - itr) <= 1, (it, itr)
    assert rel(x, xr) <= 1e-3, rel(x, xr)


def test_gmres_stops_inside_a_cycle():
    A, ml = gmres_case(K.STOP_CASE)
    dev = ml.device()
    b = K.tail_heavy(A.shape[0])
    r = K.STOP_RESTART
    _, hr, full = G.gmres(sp.csr_matrix(A), b, restart=r, reltol=1e-8)
    # maxiter inside the second cycle: x is the first cycle's update plus the partial least-squares update of three columns
    x, hist, it, _ = check_gmres(A, dev, b, restart=r, reltol=1e-8, maxiter=r + 3)
    assert it == r + 3 < full and len(hist) == r + 4 and hist[-1] > 1e-8 * hist[0]
    # the same stop through AMG.gmres (under the cycle, restart 2): isconverged is false
    Pl = O.OracleHierarchy(ml).precond
    xr, hp, itr = G.gmres(A, b, Pl=Pl, restart=2, reltol=1e-12, maxiter=5)
    assert itr == 5 and hp[-1] > 1e-12 * hp[0]
    xp, info = AMG.gmres(A, b, Pl=AMG.aspreconditioner(ml), restart=2, reltol=1e-12, maxiter=5, log=True)
    assert not info["isconverged"] and info["iters"] == 5 and len(info["resnorm"]) == 5
    assert rel(xp, xr) <= 1e-8 and np.all(np.abs(info["resnorm"] - hp[1:]) <= 1e-8 * hp[1:])
    # maxiter == restart: the update at the end of the cycle and no restart after it
    x, hist, it, _ = check_gmres(A, dev, b, restart=r, reltol=1e-8, maxiter=r)
    assert it == r and len(hist) == r + 1
    # abstol above reltol * beta decides, many steps before reltol would; and alone
    abstol = 1e-4 * hr[0]
    for reltol in (1e-8, 0.0):
        x, hist, it, _ = check_gmres(A, dev, b, restart=r, reltol=reltol, abstol=abstol)
        assert it < full // 2 and hist[-1] <= abstol < hist[-2], (it, full)


def test_gmres_capped_grid():
    """81^3 = 531441 rows: n / 2 vectors are more than kRedBlocks x kThreads, so the block count is capped and threads
    of the dot and update kernels take a second grid-stride trip; n is odd, so the tail loop runs too."""
    A = K.upwind(K.CAPPED_M, 3)
    ml = AMG.ruge_stuben(A, symmetry=AMG.NoSymmetry())
    b = K.tail_heavy(A.shape[0])
    x, hist, it, _ = check_gmres(A, ml.device(), b, restart=20, reltol=1e-8, maxiter=25)
    assert it == 25


# ---- block PCG -------------------------------------------------------------------------------------------------------
def pb_case(name, smoother="gs", dtype=None):
    key = (name, smoother, dtype)
    if key not in _pb:
        if name == "poisson_24^3":
            _pb[key] = AMG.ruge_stuben(AMG.poisson((24, 24, 24)))
        elif name == "poisson_81^3":
            _pb[key] = AMG.ruge_stuben(AMG.poisson((K.CAPPED_M,) * 3))
        else:
            _pb[key] = K.poisson_hierarchy(name, smoother, dtype)
    return _pb[key]


def oracle_for(key, dtype=np.float64):
    if (key, dtype) not in _or:
        _or[(key, dtype)] = O.OracleHierarchy(_pb[key], dtype=dtype)
    return _or[(key, dtype)]


def check_columns(key, B, X, hists, iters, tol=1e-9, htol=None, dtype=np.float64, **kw):
    """test_gpu_pcg_block.py's check_columns: every column against the oracle's pcg on it."""
    htol = tol if htol is None else htol
    oh = oracle_for(key, dtype)
    worst = 0.0
    for j in range(B.shape[1]):
        xo, ho, ito = oh.pcg(np.ascontiguousarray(B[:, j]), 0, **kw)
        dx = rel(X[:, j], xo) if np.any(xo) else float(np.linalg.norm(X[:, j]))
        worst = max(worst, dx)
        assert iters[j] == ito, (key, j, iters[j], ito)
        assert dx <= tol, (key, j, dx)
        assert len(hists[j]) == len(ho), (key, j)
        assert np.all(np.abs(hists[j].astype(np.float64) - ho) <= htol * np.abs(ho)), (key, j)
    print("pcg_block", key, B.shape, kw, "iters", list(iters), "worst x", worst)


@pytest.mark.parametrize("name", K.SCALAR_POISSON)
@pytest.mark.parametrize("bs", [1, 2, 3, 8])
def test_block_pcg_scalar_family(name, bs):
    """n % 4 != 0: pcg_block_launch<1>.  With bs > 1 and n odd every second column of the workspace starts off a 16-byte
    boundary.  Columns: tail-heavy, zero, tail-heavy x 1e3, then block()'s."""
    ml = pb_case(name)
    n = ml.levels[0].A.m
    B = K.tail_block(n, bs)
    X, hists, iters = ml.device(nrhs=bs).pcg_block(B, 0, True, None, 0.0, 1e-10)
    check_columns((name, "gs", None), B, X, hists, iters, reltol=1e-10)
    if bs >= 2:
        assert iters[1] == 0 and not np.any(X[:, 1]) and hists[1].tolist() == [0.0]
    if bs >= 3:
        assert iters[2] == iters[0]


@pytest.mark.parametrize("name", K.ODD_POISSON)
def test_block_pcg_scalar_family_jacobi_and_plain_cg(name):
    """The hierarchy whose oracle the host file reverses (Jacobi smoothers), and plain CG: 84 to 169 iterations of the dot,
    xpby and update kernels with nothing else between them but the SpMV."""
    ml = pb_case(name, "jacobi")
    n = ml.levels[0].A.m
    B = K.tail_block(n, 3)
    dev = ml.device(nrhs=3)
    X, hists, iters = dev.pcg_block(B, 0, True, None, 0.0, 1e-10)
    check_columns((name, "jacobi", None), B, X, hists, iters, reltol=1e-10)
    X, hists, iters = dev.pcg_block(B, 0, False, None, 0.0, 1e-8)
    assert iters[0] > 50
    check_columns((name, "jacobi", None), B, X, hists, iters, use_precond=False, reltol=1e-8)


@pytest.mark.parametrize("name", K.SCALAR_POISSON)
def test_block_pcg_scalar_family_float32(name):
    """Equal counts and x within F32_TOL of the Float32 oracle in the 2-norm, as test_gpu_float32.py compares vectors.  The
    residual norms are compared at that file's tolerance for Float32 histories, 1e-3: a residual brought down by a
    factor f carries the roundings of residuals f times its size, so two Float32 recurrences agree on it to about
    f eps(Float32), and f reaches 80 per iteration here."""
    ml = pb_case(name, "gs", F32)
    n = ml.levels[0].A.m
    B = K.tail_block(n, 4).astype(F32, order="F")
    X, hists, iters = ml.device(nrhs=4, dtype=F32).pcg_block(B, 0, True, None, 0.0, 1e-4)
    assert X.dtype == F32
    check_columns((name, "gs", F32), B, X, hists, iters, tol=F32_TOL, htol=1e-3, dtype=F32, reltol=1e-4)


def _pcg_block_d(dev, Bd, xptr, n, bs, reltol):
    H = np.zeros((64, bs), order="F")
    it = np.zeros(bs, dtype=np.intc)
    fn = dev.lib.amgh_pcg_block_d
    rc = fn(C.c_void_p(dev.h), C.c_void_p(Bd.ptr), C.c_void_p(xptr), 0, 1, n, C.c_double(0.0), C.c_double(reltol),
            C.c_void_p(H.ctypes.data), 64, C.c_void_p(it.ctypes.data))
    assert rc == 0, rc
    return H, it


@pytest.mark.parametrize("dtype", [np.float64, F32])
def test_block_pcg_unaligned_x(dtype):
    """amgh_pcg_block_d with X one real past a 16-byte boundary: pcg_block_update_kernel<W, false>.  The same element
    operations as the aligned kernel, so the same bits."""
    f32 = dtype is F32
    ml = pb_case("poisson_50x50", "gs", F32 if f32 else None)
    n, bs = ml.levels[0].A.m, 3
    assert n % 4 == 0
    dev = ml.device(nrhs=bs, dtype=F32) if f32 else ml.device(nrhs=bs)
    B = K.tail_block(n, bs).astype(dtype, order="F")
    reltol = 1e-4 if f32 else 1e-10
    item = np.dtype(dtype).itemsize
    Bd = DeviceBuffer(n * bs, host=B.ravel(order="F"), dtype=dtype)
    Xd = DeviceBuffer(n * bs + 1, dtype=dtype)
    assert Xd.ptr % 16 == 0
    H0, it0 = _pcg_block_d(dev, Bd, Xd.ptr, n, bs, reltol)
    X0 = Xd.download()[:n * bs].copy()
    Xd.upload(np.full(n * bs + 1, -7.0, dtype=dtype))
    H1, it1 = _pcg_block_d(dev, Bd, Xd.ptr + item, n, bs, reltol)
    full = Xd.download()
    assert full[0] == -7.0                                  # nothing written before the pointer
    assert np.array_equal(full[1:], X0) and np.array_equal(H0, H1) and np.array_equal(it0, it1)
    assert np.all(it0[[0, 2]] > 2) and it0[1] == 0
    X, hists, iters = dev.pcg_block(B, 0, True, None, 0.0, reltol)
    assert np.array_equal(X.ravel(order="F"), X0) and np.array_equal(iters, it0)


@pytest.mark.parametrize("bs", [17, 32, 33, 64])
def test_block_pcg_wide_blocks(bs):
    """24^3 rows are nb = 27 blocks of partials; with P = 32 or 64 column groups a column has G = 32 or 16 lanes, so lanes
    sum more than one partial.  The columns stop at different iterations (an abstol next to the reltol)."""
    ml = pb_case("poisson_24^3")
    n = ml.levels[0].A.m
    B = K.staggered_block(n, bs)
    abstol = K.staggered_abstol(K.staggered_block(n, 64))
    dev = ml.device(nrhs=bs)
    X, hists, iters = dev.pcg_block(B, 0, True, None, abstol, 1e-10)
    assert len(set(iters.tolist())) >= 2, iters
    check_columns(("poisson_24^3", "gs", None), B, X, hists, iters, reltol=1e-10, abstol=abstol)
    if bs == 33:
        # no column sees another's values: change some, the others keep their bits
        rng = np.random.default_rng(33)
        for changed in (tuple(range(0, 33, 2)), (1, 16, 31, 32)):
            B2 = B.copy(order="F")
            for j in changed:
                B2[:, j] = 3.0 * rng.standard_normal(n) + (j == 0) * 1e5
            other = dev.pcg_block(B2, 0, True, None, abstol, 1e-10)
            for j in set(range(33)) - set(changed):
                assert np.array_equal(other[0][:, j], X[:, j]), (changed, j)
                assert np.array_equal(other[1][j], hists[j]) and other[2][j] == iters[j], (changed, j)


@pytest.mark.parametrize("name", ["poisson_50x50", "poisson_51x51"])
def test_block_pcg_nan_column(name):
    """A NaN in one column stops that column at once (|b_j| > tol_j is false) and cannot reach another column's bits."""
    ml = pb_case(name)
    n = ml.levels[0].A.m
    dev = ml.device(nrhs=4)
    B = K.tail_block(n, 4)
    B[:, 1] = K.block(n, 4)[:, 1]
    base = dev.pcg_block(B, 0, True, None, 0.0, 1e-10)
    assert np.all(base[2] > 0)
    for where in (0, n // 2, n - 1):
        B2 = B.copy(order="F")
        B2[where, 1] = np.nan
        X, hists, iters = dev.pcg_block(B2, 0, True, None, 0.0, 1e-10)
        assert iters[1] == 0 and len(hists[1]) == 1 and np.isnan(hists[1][0]) and not np.any(X[:, 1])
        for j in (0, 2, 3):
            assert np.array_equal(X[:, j], base[0][:, j]) and np.array_equal(hists[j], base[1][j]) and iters[j] == base[2][j], (where, j)
    again = dev.pcg_block(B, 0, True, None, 0.0, 1e-10)     # and nothing of it stays in the workspace
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[2], base[2])


def test_block_pcg_capped_grid():
    """Poisson 81^3, two columns: n is odd (one real at a time), and n is more than twice kRedBlocks x kThreads, so every
    thread takes a second grid-stride trip and some a third."""
    ml = pb_case("poisson_81^3")
    n = ml.levels[0].A.m
    B = K.tail_block(n, 2)
    B[:, 1] = K.block(n, 2)[:, 1]
    X, hists, iters = ml.device(nrhs=2).pcg_block(B, 0, True, None, 0.0, 1e-8)
    check_columns(("poisson_81^3", "gs", None), B, X, hists, iters, reltol=1e-8)
    _pb.clear()
    _or.clear()
