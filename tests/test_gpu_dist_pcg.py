"""cg(A, b; Pl = aspreconditioner(ml)) on a row-sharded hierarchy (`amgh_dist_pcg_d`, `ShardedHierarchy.cg`): the recurrence of
`amgh_pcg` run over N virtual ranks of the LOCAL transport (threads of this process on one GPU), every vector resident on the
device, the scalars all-reduced.  Against the oracle's `pcg` (cycle_tests.jl:23-27, runtests.jl:186,204 use the hierarchy this
way), IterativeSolvers' recurrence restated in numpy for plain CG, and the single-handle `AMG.cg`.

Bounds.  x: 1e-9 relative and equal iteration counts — what tests/test_gpu_parity.py asks of `amgh_pcg` against the oracle.
Residual history: 1e-9 relative per entry — what the suite asks of the other device PCG's histories against the oracle
(tests/test_gpu_pcg_block.py, tests/test_krylov_cases_host.py: PCG_TOL).  Float32: the bounds of the sharded case of
tests/test_gpu_float32.py (5e-5 on x, 1e-3 on the history, a fixed number of iterations)."""
import functools

import numpy as np
import pytest

import amg_amd as AMG
import chebyshev_ref as CR
from amg_amd import sharded as SH
from conftest import uniform
from oracle import oracle as O

pytestmark = pytest.mark.gpu

X_TOL = 1e-9
HIST_TOL = 1e-9
F32 = np.float32
F32_TOL = 5e-5


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


def hist_err(h, ho):
    return float(np.max(np.abs(np.asarray(h, dtype=np.float64) - ho) / np.abs(ho)))


def sharded_cg(ml, b, nranks, shard_min_rows, calls=({},), gs_mode="exact", dtype=np.float64):
    """One handle per rank, `sh.cg(b_local, log=True, **kw)` for every kw of `calls`.  Returns per call (x, [hist of every
    rank]), then lc and the ranks' stats over all the calls."""
    def work(rank, group):
        sh = SH.ShardedHierarchy.from_multilevel(ml, rank, nranks, 0, ("local", group), shard_min_rows, dtype=dtype, gs_mode=gs_mode)
        sh.stats()
        outs = []
        for kw in calls:
            kw = dict(kw)
            rhs = np.asarray(kw.pop("b", b))
            outs.append(sh.cg(rhs[sh.r0:sh.r1], log=True, **kw))
        return outs, sh.lc, sh.stats()
    res = SH.run_local_ranks(nranks, work, dtype=dtype)
    per_call = [(np.concatenate([r[0][k][0] for r in res]), [r[0][k][1] for r in res]) for k in range(len(calls))]
    return per_call, res[0][1], [r[2] for r in res]


def same_on_every_rank(hists):
    return all(h.shape == hists[0].shape and np.all(h == hists[0]) for h in hists)


@functools.lru_cache(maxsize=None)
def problem():
    A = AMG.poisson((40, 36, 48))
    return A, uniform(A.m, 6) - 0.3


@functools.lru_cache(maxsize=None)
def hierarchy(kind):
    A, _ = problem()
    if kind == "gs":
        return AMG.ruge_stuben(A)
    jac = AMG.Jacobi(2.0 / 3.0, iter=2)
    return AMG.ruge_stuben(A, presmoother=jac, postsmoother=jac)


@functools.lru_cache(maxsize=None)
def oracle_pcg(kind, cycle):
    return O.OracleHierarchy(hierarchy(kind)).pcg(problem()[1], cycle=cycle, reltol=1e-10)


@functools.lru_cache(maxsize=None)
def small():
    A = AMG.poisson((20, 20, 20))
    b = uniform(A.m, 7)
    ml = AMG.ruge_stuben(A)
    x, log = AMG.cg(A, b, Pl=AMG.aspreconditioner(ml), reltol=1e-8, log=True)
    return A, b, ml, x, log


@pytest.mark.parametrize("kind", ["gs", "jacobi"])
@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_sharded_pcg_is_the_oracle_pcg(nranks, kind):
    """Exact Gauss-Seidel across the shards and Jacobi: both sharded cycles are the oracle's at 1e-10, so the PCG around them
    is the oracle's PCG — count, history, x.  With 3 ranks the cuts do not fall on grid planes."""
    _, b = problem()
    xo, ho, ito = oracle_pcg(kind, 0)
    [(x, hists)], lc, stats = sharded_cg(hierarchy(kind), b, nranks, 4000, calls=({"reltol": 1e-10},))
    print(kind, nranks, "iters", len(hists[0]) - 1, ito, "x", rel(x, xo), "hist", hist_err(hists[0], ho) if len(hists[0]) == len(ho) else None)
    assert lc >= 2
    assert len(hists[0]) - 1 == ito
    assert hist_err(hists[0], ho) <= HIST_TOL
    assert rel(x, xo) <= X_TOL
    assert same_on_every_rank(hists)
    assert all(s["halo_exchanges"] > 0 for s in stats)


def test_w_cycle_preconditioner():
    _, b = problem()
    xo, ho, ito = oracle_pcg("jacobi", 1)
    [(x, hists)], lc, _ = sharded_cg(hierarchy("jacobi"), b, 2, 4000, calls=({"reltol": 1e-10, "cycle": SH.CYCLE_W},))
    print("W", "iters", len(hists[0]) - 1, ito, "x", rel(x, xo))
    assert lc >= 2 and len(hists[0]) - 1 == ito
    assert hist_err(hists[0], ho) <= HIST_TOL and rel(x, xo) <= X_TOL


@pytest.mark.parametrize("nranks", [2, 3])
def test_plain_cg_is_the_recurrence_in_numpy(nranks):
    A, b = problem()
    ml = hierarchy("jacobi")
    xr, hr, itr = CR.pcg(ml.levels[0].A.to_scipy(), b, Pl=lambda r: r, reltol=1e-8)
    [(x, hists)], lc, stats = sharded_cg(ml, b, nranks, 4000, calls=({"reltol": 1e-8, "use_precond": False},))
    print("plain", nranks, "iters", len(hists[0]) - 1, itr, "x", rel(x, xr))
    assert lc >= 2 and itr > 50
    assert len(hists[0]) - 1 == itr
    assert rel(x, xr) <= 1e-9
    assert same_on_every_rank(hists)
    assert all(s["halo_exchanges"] >= itr for s in stats)     # one exchange per SpMV, none for a cycle that did not run


def test_edges_of_the_iteration():
    """maxiter = 0, b = 0 and a tolerance that cannot be met, on one handle."""
    A, b, ml, _, _ = small()
    calls = ({"maxiter": 0}, {"b": np.zeros(A.m)}, {"maxiter": 3, "reltol": 1e-30})
    (x0, h0), (xz, hz), (x3, h3) = sharded_cg(ml, b, 2, 500, calls=calls)[0]
    assert np.all(x0 == 0.0) and len(h0[0]) == 1 and h0[0][0] == pytest.approx(np.linalg.norm(b), rel=1e-13)
    assert np.all(xz == 0.0) and hz[0].tolist() == [0.0]
    assert len(h3[0]) == 4 and np.all(np.isfinite(h3[0])) and np.all(np.isfinite(x3))
    xo, ho, ito = O.OracleHierarchy(ml).pcg(b, maxiter=3, reltol=1e-30)
    assert ito == 3 and hist_err(h3[0], ho) <= HIST_TOL and rel(x3, xo) <= X_TOL
    assert same_on_every_rank(h0) and same_on_every_rank(hz) and same_on_every_rank(h3)


def test_one_rank_and_nothing_sharded_equal_the_single_handle():
    A, b, ml, xs, log = small()
    # one rank, two sharded levels: the single handle's arithmetic up to the order of the sums, and no exchange at all
    [(x, hists)], lc, stats = sharded_cg(ml, b, 1, 500, calls=({"reltol": 1e-8},))
    print("one rank", rel(x, xs))
    assert lc >= 2 and len(hists[0]) - 1 == log["iters"] and rel(x, xs) <= 1e-12 and stats[0]["halo_exchanges"] == 0
    # below the shard threshold: rank 0 runs amgh_pcg's loop on the whole hierarchy, rank 1 owns nothing and learns count and history
    [(x, hists)], lc, _ = sharded_cg(ml, b, 2, 10 ** 9, calls=({"reltol": 1e-8},))
    assert lc == 0 and len(hists[0]) - 1 == log["iters"] and rel(x, xs) <= 1e-12
    assert hist_err(hists[0][1:], np.asarray(log["resnorm"])) <= 1e-12 and same_on_every_rank(hists)


def test_two_calls_are_bitwise_the_same():
    _, b = problem()
    (x1, h1), (x2, h2) = sharded_cg(hierarchy("gs"), b, 3, 4000, calls=({"reltol": 1e-10}, {"reltol": 1e-10}))[0]
    assert np.array_equal(x1, x2) and np.array_equal(h1[0], h2[0])
    assert same_on_every_rank(h1) and same_on_every_rank(h2)


def test_float32_instance():
    A = AMG.poisson((32, 24, 20))
    A32 = AMG.SparseMatrixCSC.from_scipy(A.to_scipy().astype(F32))
    b = uniform(A.m, 5).astype(F32)
    jac = AMG.Jacobi(2.0 / 3.0, iter=2)
    ml = AMG.ruge_stuben(A32, presmoother=jac, postsmoother=jac)
    xo, ho, ito = O.OracleHierarchy(ml, dtype=F32).pcg(b, maxiter=4, reltol=1e-30)
    [(x, hists)], lc, _ = sharded_cg(ml, b, 2, 500, calls=({"maxiter": 4, "reltol": 1e-30},), gs_mode="hybrid", dtype=F32)
    print("float32", "x", rel(x, xo), "hist", hist_err(hists[0], ho.astype(np.float64)))
    assert x.dtype == F32 and hists[0].dtype == F32 and lc >= 2 and ito == 4
    assert len(hists[0]) == 5 and np.allclose(hists[0], ho, rtol=1e-3) and rel(x, xo) <= F32_TOL
    assert same_on_every_rank(hists)
