"""The device-resident PCG on a block of right-hand sides (amgh_pcg_block, DeviceHierarchy.pcg_block, AMG.cg with an n x bs
b): every column is IterativeSolvers.jl's cg on its own right-hand side, checked column by column against the CPU oracle's
pcg and against the one-column device path."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import amg_amd as AMG
from krylov_cases import block
from oracle import oracle as O
from shipping_defaults import shipping_defaults

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
CYCLES = {"V": AMG.V, "W": AMG.W, "F": AMG.F}
F32 = np.float32


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _jacobi_sa(A):
    jac = AMG.Jacobi(2.0 / 3.0)
    return AMG.smoothed_aggregation(A, presmoother=jac, postsmoother=jac)


BUILDERS = {
    "rs_50x50": lambda: AMG.ruge_stuben(AMG.poisson((50, 50))),
    "rs_24^3": lambda: AMG.ruge_stuben(AMG.poisson((24, 24, 24))),
    "sa_jacobi_50x50": lambda: _jacobi_sa(AMG.poisson((50, 50))),
}
_ml, _oracle = {}, {}


def hierarchy(name):
    if name not in _ml:
        _ml[name] = BUILDERS[name]()
    return _ml[name]


def oracle_pcg(name, b, cycle, **kw):
    b = np.ascontiguousarray(b)
    key = (name, hashlib.sha1(b.tobytes()).hexdigest(), cycle, tuple(sorted(kw.items())))
    if key not in _oracle:
        _oracle[key] = O.OracleHierarchy(hierarchy(name)).pcg(b, cycle, **kw)
    return _oracle[key]


def check_columns(name, ml, B, X, hists, iters, cycle, **kw):
    for j in range(B.shape[1]):
        xo, ho, ito = oracle_pcg(name, B[:, j], cycle, **kw)
        assert iters[j] == ito, (name, j, iters[j], ito)
        assert rel(X[:, j], xo) <= 1e-9, (name, j, rel(X[:, j], xo))
        assert len(hists[j]) == len(ho) and np.all(np.abs(hists[j] - ho) <= 1e-9 * np.abs(ho)), (name, j)


# ---- 1. parity with the oracle, column by column ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BUILDERS))
@pytest.mark.parametrize("bs", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("cyc", ["V", "W", "F"])
def test_every_column_is_the_oracle_cg(name, bs, cyc):
    ml = hierarchy(name)
    n = ml.levels[0].A.m
    B = block(n, bs)
    code = CYCLES[cyc].code
    X, hists, iters = ml.device(nrhs=bs).pcg_block(B, code, True, None, 0.0, 1e-10)
    assert X.shape == (n, bs) and X.flags.f_contiguous and iters.shape == (bs,)
    check_columns(name, ml, B, X, hists, iters, code, reltol=1e-10)


# ---- 2. columns stop at different iterations; frozen columns stay frozen; no column sees another's values -----------------
@pytest.mark.parametrize("name", ["rs_50x50", "rs_24^3"])
def test_columns_converge_independently_and_bitwise_alone(name):
    ml = hierarchy(name)
    A = ml.levels[0].A
    n = A.m
    rng = np.random.default_rng(11)
    B = np.zeros((n, 4), order="F")
    B[:, 1] = rng.standard_normal(n)
    B[:, 2] = A @ np.ones(n)
    B[:, 3] = 1e8 * rng.standard_normal(n)
    p = AMG.aspreconditioner(ml)
    X, info = AMG.cg(A, B, Pl=p, reltol=1e-10, log=True)
    it = info["iters"]
    assert len(set(it.tolist())) >= 2, it
    assert it[0] == 0 and np.all(X[:, 0] == 0.0) and len(info["resnorm"][0]) == 0 and info["isconverged"].all()
    _, hists, iters = ml.device(nrhs=4).pcg_block(B, 0, True, None, 0.0, 1e-10)
    assert hists[0].tolist() == [0.0]
    check_columns(name, ml, B, X, hists, iters, 0, reltol=1e-10)
    dev = ml.device(nrhs=4)
    base = dev.pcg_block(B, 0, True, None, 0.0, 1e-10)
    for changed in ((1, 3), (0, 2)):
        B2 = B.copy(order="F")
        for j in changed:
            B2[:, j] = 3.0 * rng.standard_normal(n) + (j == 0) * 1e5
        other = dev.pcg_block(B2, 0, True, None, 0.0, 1e-10)
        for j in set(range(4)) - set(changed):
            assert np.array_equal(other[0][:, j], base[0][:, j]), (changed, j)
            assert np.array_equal(other[1][j], base[1][j]), (changed, j)
            assert other[2][j] == base[2][j], (changed, j)


# ---- 3. agreement with the one-column path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rs_50x50", "sa_jacobi_50x50"])
def test_columns_match_the_one_column_cg(name):
    ml = hierarchy(name)
    A = ml.levels[0].A
    B = block(A.m, 3, seed=3)
    p = AMG.aspreconditioner(ml, AMG.W())
    X, info = AMG.cg(A, B, Pl=p, reltol=1e-10, log=True)
    for j in range(3):
        x1, l1 = AMG.cg(A, B[:, j], Pl=p, reltol=1e-10, log=True)
        assert info["iters"][j] == l1["iters"] and rel(X[:, j], x1) <= 1e-10, (j, rel(X[:, j], x1))
        assert info["isconverged"][j] == l1["isconverged"]
    dev = ml.device()
    b = B[:, 0]
    X1, h1, it1 = dev.pcg_block(b.reshape(-1, 1), 1, True, None, 0.0, 1e-10)
    x, h, it = dev.pcg(b, 1, True, None, 0.0, 1e-10)
    assert it1[0] == it and rel(X1[:, 0], x) <= 1e-10 and np.allclose(h1[0], h, rtol=1e-10, atol=0)


# ---- 4. edge cases ------------------------------------------------------------------------------------------------------------
def test_maxiter_abstol_and_plain_cg():
    name = "rs_50x50"
    ml = hierarchy(name)
    n = ml.levels[0].A.m
    B = block(n, 4)
    dev = ml.device(nrhs=4)
    X, hists, iters = dev.pcg_block(B, 0, True, 0, 0.0, 1e-10)
    assert np.all(X == 0.0) and np.all(iters == 0)
    for j in range(4):
        assert len(hists[j]) == 1 and np.isclose(hists[j][0], np.linalg.norm(B[:, j]), rtol=1e-12)
    X, hists, iters = dev.pcg_block(B, 0, True, 3, 0.0, 1e-10)
    assert np.all(iters == 3)
    check_columns(name, ml, B, X, hists, iters, 0, maxiter=3, reltol=1e-10)
    # abstol above reltol * |b_j| for every column: tol_j = abstol
    abstol = 1e-6 * float(np.min(np.linalg.norm(B, axis=0)))
    X, hists, iters = dev.pcg_block(B, 0, True, None, abstol, 0.0)
    check_columns(name, ml, B, X, hists, iters, 0, abstol=abstol, reltol=0.0)
    assert all(h[-1] <= abstol < 1e-10 * h[0] or h[-1] <= abstol for h in hists)
    # use_precond = 0: plain CG
    X, hists, iters = dev.pcg_block(B, 0, False, None, 0.0, 1e-8)
    check_columns(name, ml, B, X, hists, iters, 0, use_precond=False, reltol=1e-8)


def test_short_history_leaves_the_solution_alone_and_runs_are_bitwise_reproducible():
    ml = hierarchy("rs_24^3")
    n = ml.levels[0].A.m
    B = block(n, 8)
    dev = ml.device(nrhs=8)
    X, hists, iters = dev.pcg_block(B, 2, True, None, 0.0, 1e-10)
    X2, hists2, iters2 = dev.pcg_block(B, 2, True, None, 0.0, 1e-10)
    assert np.array_equal(X, X2) and np.array_equal(iters, iters2)
    assert all(np.array_equal(a, b) for a, b in zip(hists, hists2))
    assert np.all(iters > 3)
    Xs, hs, its = dev.pcg_block(B, 2, True, None, 0.0, 1e-10, ldh=3)
    assert np.array_equal(Xs, X) and np.array_equal(its, iters)
    for j in range(8):
        assert len(hs[j]) == 3 and np.array_equal(hs[j], hists[j][:3])
    # the raw ABI: ldh = 2 rows per column and 5 iterations; nothing past the 2 x 8 history is written
    lib = dev.lib
    H = np.full(2 * 8 + 4, -7.0)
    Xr = np.zeros((n, 8), order="F")
    it = np.zeros(8, dtype=np.intc)
    assert lib.amgh_pcg_block(dev.h, B.ctypes.data, Xr.ctypes.data, 2, 1, 5, 0.0, 1e-10, H.ctypes.data, 2, it.ctypes.data) == 0
    assert np.all(it == 5) and np.all(H[16:] == -7.0)
    assert np.array_equal(H[:16].reshape((2, 8), order="F"), np.stack([h[:2] for h in hists], axis=1))


def test_error_codes():
    ml = hierarchy("rs_50x50")
    n = ml.levels[0].A.m
    dev = ml.device(nrhs=2)
    lib = dev.lib
    B = np.ones((n, 2), order="F")
    X = np.zeros((n, 2), order="F")
    H = np.zeros((10, 2), order="F")
    it = np.zeros(2, dtype=np.intc)
    bp, xp, hp, ip = B.ctypes.data, X.ctypes.data, H.ctypes.data, it.ctypes.data
    for fn in (lib.amgh_pcg_block, lib.amgh_pcg_block_d):
        assert fn(dev.h, None, xp, 0, 1, 10, 0.0, 1e-8, hp, 10, ip) == EINVAL
        assert fn(dev.h, bp, None, 0, 1, 10, 0.0, 1e-8, hp, 10, ip) == EINVAL
        assert fn(None, bp, xp, 0, 1, 10, 0.0, 1e-8, hp, 10, ip) == EINVAL
    assert lib.amgh_pcg_block(dev.h, bp, xp, 0, 1, 10, 0.0, 1e-8, hp, 10, None) == EINVAL
    assert lib.amgh_pcg_block(dev.h, bp, xp, 3, 1, 10, 0.0, 1e-8, hp, 10, ip) == EINVAL
    assert lib.amgh_pcg_block(dev.h, bp, xp, -1, 1, 10, 0.0, 1e-8, hp, 10, ip) == EINVAL
    assert lib.amgh_pcg_block(dev.h, bp, xp, 0, 1, -1, 0.0, 1e-8, hp, 10, ip) == EINVAL
    assert lib.amgh_pcg_block(dev.h, bp, xp, 0, 1, 10, 0.0, 1e-8, hp, 0, ip) == EINVAL
    assert lib.amgh_pcg_block(dev.h, bp, xp, 0, 1, 10, 0.0, 1e-8, None, 0, ip) == 0    # (no history: ldh unused)
    h = C.c_void_p()
    assert lib.amgh_create(C.byref(h), 0, 2) == 0
    try:
        assert lib.amgh_pcg_block(h, bp, xp, 0, 1, 10, 0.0, 1e-8, hp, 10, ip) == ESTATE
        assert lib.amgh_pcg_block_d(h, bp, xp, 0, 1, 10, 0.0, 1e-8, hp, 10, ip) == ESTATE
    finally:
        lib.amgh_destroy(h)
    with pytest.raises(AMG.AMGError):
        AMG.cg(ml.levels[0].A, np.ones((n, 65)), Pl=AMG.aspreconditioner(ml))


def test_workspace_is_counted_and_the_builder_handle_is_reused():
    A = AMG.poisson((40, 40))
    p, _ = AMG.RugeStubenPreconBuilder(blocksize=4)(A, None)
    ml = p.ml
    dev = ml.device(nrhs=4)
    before = dev.device_bytes()
    B = block(A.m, 4)
    X = AMG.cg(A, B, Pl=p, reltol=1e-10)
    assert ml.device(nrhs=4) is dev and len([k for k in ml._dev if k[1] == 4]) == 1
    assert dev.device_bytes() - before >= 3 * 8 * A.m * 4
    assert np.linalg.norm(B - A.to_scipy() @ X) <= 1e-9 * np.linalg.norm(B)


# ---- 5. the Float32 instance ------------------------------------------------------------------------------------------------
def test_float32_block():
    A = AMG.SparseMatrixCSC.from_scipy(AMG.poisson((24, 24, 24)).to_scipy().astype(F32))
    ml = AMG.ruge_stuben(A)
    n = A.m
    B = block(n, 4).astype(F32, order="F")
    X, info = AMG.cg(A, B, Pl=AMG.aspreconditioner(ml), reltol=1e-4, log=True)
    assert X.dtype == F32 and (0, 4, "f32") in ml._dev
    assert info["isconverged"].all()
    S = A.to_scipy().astype(np.float64)
    d32 = ml.device(dtype=F32)
    for j in range(4):
        b = B[:, j].astype(np.float64)
        assert np.linalg.norm(b - S @ X[:, j].astype(np.float64)) <= 2e-4 * np.linalg.norm(b), j
        _, _, it1 = d32.pcg(B[:, j], 0, True, None, 0.0, 1e-4)
        assert info["iters"][j] == it1, (j, info["iters"][j], it1)


# ---- 6. the shipping configuration -------------------------------------------------------------------------------------------
def test_block_pcg_at_shipping_defaults():
    with shipping_defaults():
        ml = AMG.ruge_stuben(AMG.poisson((24, 24, 24)))
        n = ml.levels[0].A.m
        B = block(n, 8)
        X, hists, iters = ml.device(nrhs=8).pcg_block(B, 0, True, None, 0.0, 1e-10)
        oh = O.OracleHierarchy(ml)
        for j in range(8):
            xo, ho, ito = oh.pcg(np.ascontiguousarray(B[:, j]), 0, reltol=1e-10)
            assert iters[j] == ito and rel(X[:, j], xo) <= 1e-9, (j, iters[j], ito, rel(X[:, j], xo))
            assert len(hists[j]) == len(ho) and np.all(np.abs(hists[j] - ho) <= 1e-9 * np.abs(ho)), j
        del ml


# ---- 7. full size ---------------------------------------------------------------------------------------------------------------
def test_poisson_256_cubed_block_of_eight():
    A = AMG.poisson((256, 256, 256))
    n = A.m
    ml = AMG.ruge_stuben(A)
    p = AMG.aspreconditioner(ml)
    B = block(n, 8, seed=256)
    X, info = AMG.cg(A, B, Pl=p, reltol=1e-8, log=True)
    assert info["isconverged"].all()
    S = A.to_scipy()
    for j in range(8):
        b = B[:, j]
        assert np.linalg.norm(b - S @ X[:, j]) <= 1e-7 * np.linalg.norm(b), j
        _, l1 = AMG.cg(A, b, Pl=p, reltol=1e-8, log=True)
        assert info["iters"][j] == l1["iters"], (j, info["iters"][j], l1["iters"])
