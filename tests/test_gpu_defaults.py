"""The library at its SHIPPING configuration — the LATE row sum of the relayed walk (gs_bw_inorder = 0), the four-lane single-wave
walk (gs_wave_quad = 1) and the collapsed dense coarse tail (tail_dense_rows = 6144) — on the paths the rest of the suite runs
with those pinned off (tests/conftest.py): the local-transport sharded cycle, hipGraph replay of whole cycles, blocks of
right-hand sides, Float32, user timing around a first W-cycle.  The module sets the compiled-in values for itself and puts the
session's back afterwards (tests/shipping_defaults.py); every handle is created inside it.  Each test first shows, through the
library's diagnostics, that the default path really ran.  Small sizes force the block layout (gs_bw = 2, gs_bw_rows = 64) as
test_gpu_late.py does; the arithmetic tunables stay at their defaults."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import amg_amd as AMG
from amg_amd import sharded as SH
from amg_amd.device import DeviceHierarchy
from conftest import ROOT, load_csc, load_npz, uniform
from oracle import oracle as O
from shipping_defaults import pinned, shipping_defaults

pytestmark = pytest.mark.gpu

TOL = 1e-10
TIGHT = 1e-12
F32 = np.float32
F32_TOL = 5e-5          # (test_gpu_float32.py)
V, W, F = 0, 1, 2


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


@pytest.fixture(scope="module", autouse=True)
def defaults():
    with shipping_defaults() as d:
        yield d


def _f32_matrix(A):
    return AMG.SparseMatrixCSC.from_scipy(A.to_scipy().astype(F32))


def _cycles(dev, b, cyc, k=3):
    """iterates after 1..k cycles from x = 0 (calculate_residual = False)"""
    z = np.zeros_like(np.asarray(b, dtype=dev.dtype))
    return [dev.solve(b, z, cyc, j, 0.0, 0.0, False, False)[0] for j in range(1, k + 1)]


# ---- the anchor: the fixture IS the shipping configuration -------------------------------------------------------------------

_ANCHOR = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import amg_amd as AMG
from amg_amd.device import DeviceHierarchy
from conftest import uniform
A = AMG.poisson((24, 20, 16))
ml = AMG.ruge_stuben(A)
dev = DeviceHierarchy(ml, 0, 1)
b = uniform(A.m, 77) - 0.4
out = {"z": dev.precond_apply(b), "lv": np.array(dev.tail_dense_info(0)[:2])}
for cyc in (0, 1, 2):
    for k in (1, 2, 3):
        out["c%d_%d" % (cyc, k)] = dev.solve(b, np.zeros(A.m), cyc, k, 0.0, 0.0, False, False)[0]
np.savez(sys.argv[2], **out)
"""


def test_anchor_a_process_that_sets_no_tunable_computes_the_same_bits(tmp_path):
    """A fresh child touches no tunable: its ldiv! and three V / W / F cycles are this module's bit for bit."""
    out = str(tmp_path / "anchor.npz")
    r = subprocess.run([sys.executable, "-c", _ANCHOR, ROOT, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    ref = np.load(out)
    A = AMG.poisson((24, 20, 16))
    ml = AMG.ruge_stuben(A)
    dev = DeviceHierarchy(ml, 0, 1)
    lv, rows, _ = dev.tail_dense_info(0)
    assert lv >= 1 and rows <= 6144 and [lv, rows] == ref["lv"].tolist()       # the tail is built, in both processes
    b = uniform(A.m, 77) - 0.4
    assert np.array_equal(dev.precond_apply(b), ref["z"])
    for cyc in (V, W, F):
        for k in (1, 2, 3):
            x = dev.solve(b, np.zeros(A.m), cyc, k, 0.0, 0.0, False, False)[0]
            assert np.array_equal(x, ref["c%d_%d" % (cyc, k)]), (cyc, k)
    # and not the suite's pinned configuration: the per-level cycle of the same handle gives other bits
    with pinned(AMG.hip_lib(), tail_dense=0):
        assert not np.array_equal(dev.precond_apply(b), ref["z"])


# ---- the local-transport sharded cycle -----------------------------------------------------------------------------------

def _sharded(ml, nranks, shard_min_rows, fn, gs_mode="exact", dtype=np.float64):
    def work(rank, group):
        sh = SH.ShardedHierarchy.from_multilevel(ml, rank, nranks, 0, ("local", group), shard_min_rows, dtype=dtype, gs_mode=gs_mode)
        return fn(sh)
    return SH.run_local_ranks(nranks, work, dtype=dtype)


def _sharded_cycles(ml, b, nranks, thr, cycs, k=2, gs_mode="exact", dtype=np.float64):
    """{cyc: [iterate after 1..k cycles]} and the tail handle's (level, rows) for V"""
    def fn(sh):
        out = {c: [sh.solve(b[sh.r0:sh.r1], cycle=c, maxiter=j, calculate_residual=False)[0] for j in range(1, k + 1)] for c in cycs}
        return out, (sh.tail.tail_dense_info(0)[:2] if sh.tail is not None else None), sh.lc
    res = _sharded(ml, nranks, thr, fn, gs_mode, dtype)
    cyc_out = {c: [np.concatenate([r[0][c][j] for r in res]) for j in range(k)] for c in cycs}
    return cyc_out, res[0][1], res[0][2]


A_SH = (40, 36, 48)          # levels 69 120 / 34 560 / 5 759 / 899 / ...
THR_BIG_TAIL = 40000         # one sharded level: the tail handle starts at 34 560 rows, its dense tail at its level 1 (5 759 rows)
THR_ONE_OP = 4000            # three sharded levels: the tail handle (899 rows and below) is one dense operator altogether


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_sharded_exact_gauss_seidel_at_defaults(nranks):
    """gs_mode = "exact" (lexicographic over the whole level), V / W / F cycle for cycle against the oracle for symmetric GS,
    forward / backward GS and SOR, plus a solve; two shard thresholds.

    Whether the dense tail is applied inside the sharded cycle (compared with tail_dense = 0 on the same configuration):
    - tail handle with levels above its dense tail (THR_BIG_TAIL): the sharded cycle enters the tail handle through its level-0
      recursion, which hands level 1 to the dense V operator built at setup — V-cycles and the V-visits of F-cycles use it (not
      bitwise the per-level cycle, within 1e-12); the W operator is only built by the single-GPU entry points (apply_cycle), so
      sharded W-cycles run the per-level tail, bit for bit;
    - tail handle that is one operator altogether (THR_ONE_OP): the level-0 recursion never consults the dense operator (only
      the single-GPU entry points apply a whole-hierarchy tail), so every cycle type is the per-level cycle bit for bit."""
    lib = AMG.hip_lib()
    A = AMG.poisson(A_SH)
    b = uniform(A.m, 6) - 0.3
    cases = [(AMG.GaussSeidel(), AMG.GaussSeidel(), (V, W, F)),
             (AMG.GaussSeidel(AMG.ForwardSweep(), iter=2), AMG.GaussSeidel(AMG.BackwardSweep()), (V,)),
             (AMG.SOR(1.2), AMG.SOR(0.9, AMG.ForwardSweep()), (V,))]
    for thr, one_op in ((THR_BIG_TAIL, False), (THR_ONE_OP, True)):
        for pre, post, cycs in cases:
            ml = AMG.ruge_stuben(A, presmoother=pre, postsmoother=post)
            oh = O.OracleHierarchy(ml)
            got, tinfo, lc = _sharded_cycles(ml, b, nranks, thr, cycs)
            assert lc >= 1 and tinfo is not None
            if one_op:
                assert tinfo[0] == 0, tinfo
            else:
                assert tinfo[0] >= 1 and ml.levels[lc].A.m > 6144, tinfo
            with pinned(lib, tail_dense=0):
                per_level, _, _ = _sharded_cycles(ml, b, nranks, thr, cycs)
            for cyc in cycs:
                for k in range(2):
                    xo, _, _ = oh.solve(b, cycle=cyc, maxiter=k + 1, calculate_residual=False)
                    assert rel(got[cyc][k], xo) <= TOL, (nranks, thr, repr(pre), cyc, k)
                    if one_op or cyc == W:
                        assert np.array_equal(got[cyc][k], per_level[cyc][k]), (nranks, thr, repr(pre), cyc, k)
                    else:
                        assert not np.array_equal(got[cyc][k], per_level[cyc][k]), (nranks, thr, repr(pre), cyc, k)
                        assert rel(got[cyc][k], per_level[cyc][k]) <= TIGHT, (nranks, thr, repr(pre), cyc, k)
        ml = AMG.ruge_stuben(A)
        res = _sharded(ml, nranks, thr, lambda sh: (*sh.solve(b[sh.r0:sh.r1], reltol=1e-9, maxiter=60), sh.lc))
        x, hist = np.concatenate([r[0] for r in res]), res[0][1]
        xo, ho, _ = O.OracleHierarchy(ml).solve(b, reltol=1e-9, maxiter=60)
        assert res[0][2] >= 1 and len(hist) == len(ho) and np.allclose(hist, ho, rtol=1e-8) and rel(x, xo) <= TOL


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_sharded_pipelined_sweep_at_defaults_is_the_oracle_and_the_turns_bit_for_bit(nranks):
    """Exact order as one sweep pipelined across the ranks (forced block layout on small shards, THR_BIG_TAIL: level 0 sharded):
    the oracle's iterate and, row for row the same arithmetic, the ranks' turns bit for bit.  What runs, shown by the diagnostics:
    the pipelined sweep on level 0 of every rank (amgh_dist_gs_pipelined); the LATE sum on the tail handle's relayed level 0
    (34 560 rows — the shards' own sweeps keep the stored order: the split sum needs a schedule over all of an operator's
    columns, which a shard with halo columns is not); the tail handle's dense V operator, applied in V-cycles (other bits
    than tail_dense = 0).  Ranks whose streams share a hardware queue sweep in turns: then the pipeline did not run — skipped
    with fewer than 8 hardware queues, a failure with 8 or more, as in test_gpu_sharded.py."""
    lib = AMG.hip_lib()
    A = AMG.poisson(A_SH)
    b = uniform(A.m, 6) - 0.3

    def fn(sh, cycs, diag):
        out = {c: [sh.solve(b[sh.r0:sh.r1], cycle=c, maxiter=j, calculate_residual=False)[0] for j in (1, 2)] for c in cycs}
        if not diag:
            return out
        late = sh.lib.amgh_debug_bw_late(sh.tail.h, 0) if sh.tail is not None else None
        tinfo = sh.tail.tail_dense_info(0)[:2] if sh.tail is not None else None
        return out, sh.gs_pipelined(), sh.pipe_serialized(), late, tinfo

    def run(ml, cycs, mode="exact", diag=True):
        res = _sharded(ml, nranks, THR_BIG_TAIL, lambda sh: fn(sh, cycs, diag), mode)
        outs = [r[0] for r in res] if diag else res
        return {c: [np.concatenate([o[c][j] for o in outs]) for j in range(2)] for c in cycs}, res

    serialized = False
    with pinned(lib, gs_bw=2, gs_bw_rows=64):
        for pre, post, cycs in [(AMG.GaussSeidel(), AMG.GaussSeidel(), (V, W)), (AMG.SOR(1.2), AMG.SOR(0.9, AMG.ForwardSweep()), (V,))]:
            ml = AMG.ruge_stuben(A, presmoother=pre, postsmoother=post)
            oh = O.OracleHierarchy(ml)
            got, res = run(ml, cycs)
            turns, _ = run(ml, cycs, "exact-turns", diag=False)
            assert res[0][3] == 1 and res[0][4][0] >= 1, (res[0][3], res[0][4])    # LATE and the dense tail on the tail handle
            serialized = serialized or any(r[2] for r in res)
            if not serialized:
                assert all(r[1] == [True] for r in res), [r[1] for r in res]
            with pinned(lib, tail_dense=0):
                per_level, _ = run(ml, (V,), diag=False)
            assert not np.array_equal(got[V][0], per_level[V][0]) and rel(got[V][0], per_level[V][0]) <= TIGHT
            for cyc in cycs:
                for k in range(2):
                    xo, _, _ = oh.solve(b, cycle=cyc, maxiter=k + 1, calculate_residual=False)
                    assert rel(got[cyc][k], xo) <= TOL, (nranks, repr(pre), cyc, k)
                    assert np.array_equal(got[cyc][k], turns[cyc][k]), (nranks, repr(pre), cyc, k)
        assert lib.amgh_dev_sync(0) == 0
    if serialized:
        msg = "the virtual ranks' streams shared a hardware queue in this process: swept in turns (oracle parity held)"
        if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) >= 8:
            pytest.fail(msg + " although 8 or more hardware queues were available: the pipelined sweep did not run")
        pytest.skip(msg)


@pytest.mark.parametrize("nranks", [2, 4])
def test_sharded_float32_at_defaults(nranks):
    A = _f32_matrix(AMG.poisson(A_SH))
    ml = AMG.ruge_stuben(A)
    b = (uniform(A.m, 8) - 0.3).astype(F32)
    oh = O.OracleHierarchy(ml, dtype=F32)
    for thr in (THR_BIG_TAIL, THR_ONE_OP):
        got, tinfo, _ = _sharded_cycles(ml, b, nranks, thr, (V, W, F), dtype=F32)
        assert tinfo[0] == (0 if thr == THR_ONE_OP else 1), tinfo
        for cyc in (V, W, F):
            for k in range(2):
                assert got[cyc][k].dtype == F32
                xo, _, _ = oh.solve(b, cycle=cyc, maxiter=k + 1, calculate_residual=False)
                assert rel(got[cyc][k], xo) <= F32_TOL, (nranks, thr, cyc, k, rel(got[cyc][k], xo))


@pytest.mark.parametrize("nranks", [2, 4])
def test_sharded_jacobi_at_defaults_against_the_single_gpu_handle(nranks):
    """Jacobi / residual / R / P on the shards are the single-GPU arithmetic, and the sharded tail handle (THR_BIG_TAIL: from
    34 560 rows) has its dense operator at the same level (5 759 rows) as the single-GPU handle's, built from the same
    recursion: V-cycles are the single-GPU handle's bit for bit.  W / F: the single-GPU handle applies the dense W / F tail
    operators (built at their first cycle), the sharded cycle the per-level W tail (see the exact test): within 1e-12."""
    A = AMG.poisson(A_SH)
    jac = AMG.Jacobi(2.0 / 3.0, iter=2)
    ml = AMG.ruge_stuben(A, presmoother=jac, postsmoother=jac)
    b = uniform(A.m, 5)
    dev = DeviceHierarchy(ml, 0, 1)
    assert dev.tail_dense_info(0)[1] == 5759
    got, tinfo, lc = _sharded_cycles(ml, b, nranks, THR_BIG_TAIL, (V, W, F))
    assert lc == 1 and tinfo == (1, 5759)
    oh = O.OracleHierarchy(ml)
    for cyc in (V, W, F):
        single = _cycles(dev, b, cyc, 2)
        for k in range(2):
            xo, _, _ = oh.solve(b, cycle=cyc, maxiter=k + 1, calculate_residual=False)
            assert rel(got[cyc][k], xo) <= TOL
            if cyc == V:
                assert np.array_equal(got[cyc][k], single[k]), (nranks, k)
            else:
                assert rel(got[cyc][k], single[k]) <= TIGHT, (nranks, cyc, k)


# ---- hipGraph replay of whole cycles -----------------------------------------------------------------------------------------

def _late_handles(ml, nrhs):
    lib = AMG.hip_lib()
    with pinned(lib, gs_bw=2, gs_bw_rows=64):
        g, e = DeviceHierarchy(ml, 0, nrhs), DeviceHierarchy(ml, 0, nrhs)
    for d in (g, e):
        # (the LATE sum is the relayed SINGLE-column walk's: a block handle sweeps its columns with the multi-column dataflow kernel)
        if nrhs == 1:
            assert lib.amgh_debug_bw_late(d.h, 0) == 1 and lib.amgh_debug_bw_late(d.h, 1) == 1
        else:
            assert lib.amgh_debug_bw_mode(d.h, 0) == 3 and lib.amgh_debug_bw_late(d.h, 0) == 0
        assert d.tail_dense_info(0)[0] >= 1
    return g, e


@pytest.mark.parametrize("nrhs", [1, 4])
def test_graph_replay_of_whole_cycles_at_defaults(nrhs):
    """A graph handle and its eager twin (LATE kernels on levels 0 and 1 — bs = 4: the multi-column dataflow sweep —, dense tail built): graphs switched on BEFORE the first
    cycle of each type — the W / F tail operators are built lazily right before the capture.  Warm-up, capture and replays
    equal the eager twin bit for bit and the oracle to 1e-10; tail_dense toggled between replays re-captures (the epoch) and
    gives the per-level cycle's bits; a solve through the cached graphs is the eager solve (x and history) bit for bit."""
    lib = AMG.hip_lib()
    A = AMG.poisson((40, 36, 32))
    ml = AMG.ruge_stuben(A)
    oh = O.OracleHierarchy(ml)
    n = A.m
    b = uniform(n, 5) - 0.4 if nrhs == 1 else np.asfortranarray(np.stack([uniform(n, 5 + c) - 0.1 * c for c in range(nrhs)], axis=1))
    bcols = [b] if nrhs == 1 else [b[:, c].copy() for c in range(nrhs)]
    for cyc in (V, W, F):
        g, e = _late_handles(ml, nrhs)
        assert lib.amgh_set_use_graph(g.h, 1) == 0
        if cyc != V:
            assert g.tail_dense_info(cyc)[0] == -1            # not built yet: the first cycle builds it, outside the capture
        xo = [oh.solve(bc, cycle=cyc, maxiter=2, calculate_residual=False)[0] for bc in bcols]
        ref = e.solve(b, np.zeros_like(b), cyc, 2, 0.0, 0.0, False, False)[0]
        for rep in range(4):                                    # warm-up, capture, replays
            x = g.solve(b, np.zeros_like(b), cyc, 2, 0.0, 0.0, False, False)[0]
            assert np.array_equal(x, ref), (cyc, rep)
        assert g.tail_dense_info(cyc)[0] >= 1
        xs = [x] if nrhs == 1 else [x[:, c] for c in range(nrhs)]
        for c in range(nrhs):
            assert rel(xs[c], xo[c]) <= TOL, (cyc, c)
        z_ref = e.precond_apply(b, cyc)
        for rep in range(3):
            assert np.array_equal(g.precond_apply(b, cyc), z_ref), (cyc, rep)
        with pinned(lib, tail_dense=0):                        # epoch bump: captured again, the per-level cycle
            ref0 = e.solve(b, np.zeros_like(b), cyc, 2, 0.0, 0.0, False, False)[0]
            assert not np.array_equal(ref0, ref)
            for rep in range(3):
                assert np.array_equal(g.solve(b, np.zeros_like(b), cyc, 2, 0.0, 0.0, False, False)[0], ref0), (cyc, rep)
        for rep in range(2):                                    # and back
            assert np.array_equal(g.solve(b, np.zeros_like(b), cyc, 2, 0.0, 0.0, False, False)[0], ref), (cyc, rep)
        xs_e, hs_e, it_e = e.solve(b, np.zeros_like(b), cyc, 100, 0.0, 1e-9, True, True)
        for rep in range(2):
            xs_g, hs_g, it_g = g.solve(b, np.zeros_like(b), cyc, 100, 0.0, 1e-9, True, True)
            assert it_g == it_e and np.array_equal(xs_g, xs_e) and np.array_equal(hs_g, hs_e), (cyc, rep)
        assert lib.amgh_debug_bw_poll_giveups(g.h, 0) == 0
        del g, e


# ---- blocks of right-hand sides --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [2, 3, 4, 8])
def test_blocks_of_right_hand_sides_at_defaults(bs):
    """V / W / F applies and solves of a block at the shipping defaults (only the block layout forced, gs_bw = 2): every column
    the oracle's (1e-10) and the single-column default handle's (1e-12).  Then gs_bw_inorder = 1 alone (dense tail and four-lane
    walk still on): still within 1e-12 of the single columns.  Bit for bit only with gs_lpr = 1 and gs_ept = 1 as well — a
    discrepancy by design: single-column launches of merged dependency-level groups sum long composite rows with several lanes
    per row (gs_lpr = 0 picks 8 or 16 lanes by row length) and two entries per thread on large groups, block launches with one
    thread per row; the same sums in another order.  The tail forms a column's sum the same way whatever the block
    (dense_rm_gemv_kernel's thread count depends on n alone)."""
    lib = AMG.hip_lib()
    A = AMG.poisson((32, 28, 24))
    ml = AMG.ruge_stuben(A)
    oh = O.OracleHierarchy(ml)
    n = A.m
    B = np.asfortranarray(np.stack([uniform(n, 60 + c) - 0.2 * c for c in range(bs)], axis=1))
    with pinned(lib, gs_bw=2, gs_bw_rows=128):
        dev1 = DeviceHierarchy(ml, 0, 1)
        devb = DeviceHierarchy(ml, 0, bs)
    assert lib.amgh_debug_bw_mode(devb.h, 0) == 3 and lib.amgh_debug_bw_mode(dev1.h, 0) == 3
    assert lib.amgh_debug_bw_late(dev1.h, 0) == 1 and devb.tail_dense_info(0)[0] >= 1
    for cyc in (V, W, F):
        Z = devb.precond_apply(B, cyc)
        X = devb.solve(B, np.zeros_like(B), cyc, 3, 0.0, 0.0, False, False)[0]
        for c in range(bs):
            bc = B[:, c].copy()
            z1 = dev1.precond_apply(bc, cyc)
            x1 = dev1.solve(bc, np.zeros(n), cyc, 3, 0.0, 0.0, False, False)[0]
            assert rel(Z[:, c], oh.precond(bc, cyc)) <= TOL, (bs, cyc, c)
            assert rel(X[:, c], oh.solve(bc, cycle=cyc, maxiter=3, calculate_residual=False)[0]) <= TOL, (bs, cyc, c)
            assert rel(Z[:, c], z1) <= TIGHT and rel(X[:, c], x1) <= TIGHT, (bs, cyc, c)
    with pinned(lib, gs_bw_inorder=1):
        for cyc in (V, W, F):
            Z = devb.precond_apply(B, cyc)
            for c in range(bs):
                assert rel(Z[:, c], dev1.precond_apply(B[:, c].copy(), cyc)) <= TIGHT, (bs, cyc, c)
        with pinned(lib, gs_lpr=1, gs_ept=1):
            for cyc in (V, W, F):
                Z = devb.precond_apply(B, cyc)
                X = devb.solve(B, np.zeros_like(B), cyc, 2, 0.0, 0.0, False, False)[0]
                for c in range(bs):
                    bc = B[:, c].copy()
                    assert np.array_equal(Z[:, c], dev1.precond_apply(bc, cyc)), (bs, cyc, c)
                    assert np.array_equal(X[:, c], dev1.solve(bc, np.zeros(n), cyc, 2, 0.0, 0.0, False, False)[0]), (bs, cyc, c)
    assert lib.amgh_debug_bw_poll_giveups(devb.h, 0) == 0


@pytest.mark.parametrize("bs", [2, 3, 8])
def test_multi_column_dataflow_sweep_is_within_the_per_row_bound(bs):
    """Each column of the multi-column dataflow sweep (one launch for the whole block, at the shipping defaults) against the
    per-row bound of tests/sweep_bound.py: forward / backward Gauss-Seidel and SOR, as pre- and post-smoothers of level 0."""
    from sweep_bound import assert_sweep_within_bound, directional, smooth_block
    lib = AMG.hip_lib()
    A = AMG.poisson((32, 28, 24))
    n = A.m
    X0 = np.stack([uniform(n, 80 + c) - 0.5 for c in range(bs)], axis=1)
    B = np.stack([uniform(n, 90 + c) - 0.1 * c for c in range(bs)], axis=1)
    for pre, post in ((AMG.GaussSeidel(AMG.ForwardSweep()), AMG.GaussSeidel(AMG.BackwardSweep())),
                      (AMG.SOR(1.3, AMG.ForwardSweep()), AMG.SOR(0.7, AMG.BackwardSweep()))):
        ml = AMG.ruge_stuben(A, presmoother=pre, postsmoother=post)
        with pinned(lib, gs_bw=2, gs_bw_rows=128):
            devb = DeviceHierarchy(ml, 0, bs)
        assert lib.amgh_debug_bw_mode(devb.h, 0) == 3
        for which, sm in ((0, pre), (1, post)):
            XS = smooth_block(devb, 0, which, X0, B)
            for c in range(bs):
                assert not np.array_equal(XS[:, c], X0[:, c]), (bs, c)          # every column swept
                assert_sweep_within_bound(A, X0[:, c], B[:, c], XS[:, c], *directional(sm), what="block %d column %d %r" % (bs, c, sm))
                assert rel(XS[:, c], O.smooth(sm, A, X0[:, c], B[:, c], hermitian=True)) <= 1e-14, (bs, c, repr(sm))
        assert lib.amgh_debug_bw_poll_giveups(devb.h, 0) == 0


def _elastic():
    d = load_npz("lin_elastic_2d")
    return load_csc("lin_elastic_2d"), d["b"], d["B"]


@pytest.mark.parametrize("bs", [3, 8])
def test_blocks_on_lin_elastic_at_defaults(bs):
    """lin_elastic_2d (smoothed aggregation with B): the hierarchy is one dense tail altogether, built with the four-lane walk
    (a handle built with gs_wave_quad = 0 gives other bits).  Every column of a block is the single-column handle's bit for bit
    (with gs_bw_inorder = 1 as well as without: no relayed level here) and the oracle's to 1e-10."""
    lib = AMG.hip_lib()
    A, b, Bn = _elastic()
    ml = AMG.smoothed_aggregation(A, B=Bn)
    oh = O.OracleHierarchy(ml)
    n = A.m
    Bm = np.asfortranarray(np.stack([b] + [uniform(n, 70 + c) - 0.5 for c in range(bs - 1)], axis=1))
    dev1, devb = DeviceHierarchy(ml, 0, 1), DeviceHierarchy(ml, 0, bs)
    assert dev1.tail_dense_info(0)[0] == 0 and devb.tail_dense_info(0)[0] == 0
    with pinned(lib, gs_wave_quad=0):
        dev_1lane = DeviceHierarchy(ml, 0, 1)
    assert not np.array_equal(dev_1lane.precond_apply(b), dev1.precond_apply(b))      # the four-lane walk built the tail
    for inorder in (0, 1):
        with pinned(lib, gs_bw_inorder=inorder):
            for cyc in (V, W, F):
                Z = devb.precond_apply(Bm, cyc)
                for c in range(bs):
                    bc = Bm[:, c].copy()
                    assert np.array_equal(Z[:, c], dev1.precond_apply(bc, cyc)), (bs, inorder, cyc, c)
                    assert rel(Z[:, c], oh.precond(bc, cyc)) <= TOL, (bs, cyc, c)


# ---- Float32 --------------------------------------------------------------------------------------------------------------

def test_float32_cycles_and_solves_at_defaults():
    """Float32 V / W / F cycles and a solve against the Float32 oracle, with the dense tail built (V at setup, W / F at their
    first cycle) and the LATE kernels forced onto levels 0 and 1."""
    lib32 = AMG.hip_lib("float32")
    A = _f32_matrix(AMG.poisson((40, 36, 32)))
    ml = AMG.ruge_stuben(A)
    oh = O.OracleHierarchy(ml, dtype=F32)
    b = (uniform(A.m, 12) - 0.3).astype(F32)
    with pinned(lib32, gs_bw=2, gs_bw_rows=64):
        dev = DeviceHierarchy(ml, 0, 1, dtype=F32)
    assert lib32.amgh_debug_bw_late(dev.h, 0) == 1 and lib32.amgh_debug_bw_late(dev.h, 1) == 1
    assert dev.tail_dense_info(0)[0] >= 1
    for cyc in (V, W, F):
        xs = _cycles(dev, b, cyc, 3)
        for k in range(3):
            xo, _, _ = oh.solve(b, cycle=cyc, maxiter=k + 1, calculate_residual=False)
            assert xs[k].dtype == F32 and rel(xs[k], xo) <= F32_TOL, (cyc, k, rel(xs[k], xo))
        assert dev.tail_dense_info(cyc)[0] >= 1
        assert rel(dev.precond_apply(b, cyc), oh.precond(b, cyc)) <= F32_TOL
    x, hist, _ = dev.solve(b, np.zeros(A.m, F32), V, 100, 0.0, 1e-5, True, True)
    xo, ho, _ = oh.solve(b, reltol=1e-5, maxiter=100)
    # (the residual norms are b - A x in Float32: each carries an error of order eps(Float32) ||b||, so they are compared on
    #  that scale — the last ones sit a few hundred ulp of ||b|| above it, where their relative differences reach percents)
    assert len(hist) == len(ho) and rel(x, xo) <= F32_TOL, (len(hist), len(ho), rel(x, xo))
    assert np.max(np.abs(hist.astype(np.float64) - ho.astype(np.float64))) <= F32_TOL * float(ho[0])


def test_float32_lin_elastic_four_lane_walk_and_tail():
    """Float32 lin_elastic_2d: the tail (the whole hierarchy) built with the four-lane walk — a handle built with one lane gives
    other bits — and the Float32 oracle's ldiv! and cycles to F32_TOL."""
    lib32 = AMG.hip_lib("float32")
    A, b, Bn = _elastic()
    A32 = _f32_matrix(A)
    ml = AMG.smoothed_aggregation(A32, B=Bn.astype(F32))
    b32 = b.astype(F32)
    oh = O.OracleHierarchy(ml, dtype=F32)
    dev = DeviceHierarchy(ml, 0, 1, dtype=F32)
    assert dev.tail_dense_info(0)[0] == 0
    with pinned(lib32, gs_wave_quad=0):
        dev1 = DeviceHierarchy(ml, 0, 1, dtype=F32)
    z = dev.precond_apply(b32)
    assert not np.array_equal(z, dev1.precond_apply(b32))
    assert z.dtype == F32 and rel(z, oh.precond(b32)) <= F32_TOL
    for cyc in (W, F):
        x = _cycles(dev, b32, cyc, 2)[-1]
        assert rel(x, oh.solve(b32, cycle=cyc, maxiter=2, calculate_residual=False)[0]) <= F32_TOL


# ---- user timing ----------------------------------------------------------------------------------------------------------

def _timed(dev, fn):
    dev.timer_begin()
    fn()
    return dev.timer_end()


def test_timer_region_around_a_first_w_cycle():
    """amgh_timer_begin / _end time the caller's region, also when it holds the first W-cycle of a handle (which builds the
    tail's W operator first, with events of its own).  Two probes:
    - 0.3 s of host sleep inside the region count, around a V-cycle and around the first W-cycle;
    - GPU work inside the region counts: ~1 s of V-cycles followed by the first W-cycle report at least the V-cycles' time."""
    A = AMG.poisson((24, 20, 16))
    ml = AMG.ruge_stuben(A)
    b = uniform(A.m, 3)
    z = np.zeros(A.m)
    warm = DeviceHierarchy(ml, 0, 1)
    warm.precond_apply(b, W)                 # (the W kernels' code is loaded: a first W-cycle below costs its build and itself)
    dev = DeviceHierarchy(ml, 0, 1)
    assert dev.tail_dense_info(0)[0] >= 1 and dev.tail_dense_info(W)[0] == -1
    dev.precond_apply(b)
    t_v = _timed(dev, lambda: (time.sleep(0.3), dev.precond_apply(b, V)))
    assert t_v >= 270.0, t_v
    per = _timed(dev, lambda: dev.solve(b, z, V, 200, 0.0, 0.0, False, False)) / 200
    k = int(min(20000, max(200, 1000.0 / max(per, 1e-3))))
    t_ref = _timed(dev, lambda: dev.solve(b, z, V, k, 0.0, 0.0, False, False))
    assert t_ref >= 300.0, (t_ref, k)
    t_w = _timed(dev, lambda: (dev.solve(b, z, V, k, 0.0, 0.0, False, False), dev.precond_apply(b, W)))
    assert dev.tail_dense_info(W)[0] >= 1 and dev.tail_dense_info(W)[2] > 0.0
    assert t_w >= 0.9 * t_ref, (t_w, t_ref, k)
    dev2 = DeviceHierarchy(ml, 0, 1)
    t_ws = _timed(dev2, lambda: (time.sleep(0.3), dev2.precond_apply(b, W)))     # sleep, then the first W-cycle
    assert t_ws >= 270.0, t_ws
    assert dev.bench_op(0, 0, reps=3, warmup=1) > 0.0      # (amgh_bench_op times with the library's events too)
