"""The order changes of the fine level folded into its Gauss-Seidel sweeps (csrc/hip/gs_relay.hpp, template flags PB / PX;
switch amgh_debug_set_perm_io): the relayed sweep that starts a smooth! call reads b through the schedule's permutation instead of
a gather kernel, the one that ends it writes x in natural order instead of a scatter kernel.  The change only moves data, so
with the switch on and off every output is the same BIT FOR BIT (raw bytes compared, no tolerance).

Which sizes run the fused kernels without forcing anything (ruge_stuben defaults, gs_bw = 1): a level takes the block layout
from 30 000 rows, 7-point operators from 15 000 (gs_schedule.hpp, kGsBwMinRows), where the cost model of the dataflow sweep
(gs_blocks.hpp, Plan::est_flow_seconds) beats the merged groups by 20 % — it does for every 3-D grid of that size: 40^3
(64 000 rows: ~66 us modelled against ~156 us) and 48 x 20 x 33 (31 680 rows: ~57 against ~129).  24^3 (13 824 rows) is below
the size threshold: level schedules, nothing fused — that case is skipped, with a message, never passed.  Every case checks
amgh_debug_bw_mode(level 0) == 3 before it claims anything, and `both()` reads amgh_debug_perm_io_sweeps around every call: with
the switch on the call must have launched sweeps with b folded in (and with x folded in, where the case says so), with the
switch off none."""
import functools
import subprocess
import sys

import numpy as np
import pytest

import amg_amd as AMG
from amg_amd.device import DeviceHierarchy
from conftest import ROOT, uniform
from oracle import oracle as O
from shipping_defaults import pinned

pytestmark = pytest.mark.gpu

TOL = 1e-10            # the project's tolerance for a cycle against the oracle
F32 = np.float32
F32_TOL = 5e-5         # (test_gpu_float32.py)
V, W, F = 0, 1, 2
SIZES = [(24, 24, 24), (40, 40, 40), (48, 20, 33)]


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


def same_bytes(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def both(lib, fn, b=True, x=True):
    """fn() with the order changes folded into the sweeps, then with the kernels of their own.  b / x: whether fn() must run
    sweeps that read b through the permutation / write x in natural order (False: it must run none, None: not asked — the
    counters are the library's, over all levels)"""
    def count():
        return lib.amgh_debug_perm_io_sweeps(0), lib.amgh_debug_perm_io_sweeps(1)
    saved = lib.amgh_debug_get_perm_io()
    try:
        assert lib.amgh_debug_set_perm_io(1) == 0 and lib.amgh_debug_get_perm_io() == 1
        c0 = count()
        on = fn()
        c1 = count()
        assert b is None or (c1[0] > c0[0]) == b, ("sweeps with b folded in", c0, c1, b)
        assert x is None or (c1[1] > c0[1]) == x, ("sweeps with x folded in", c0, c1, x)
        assert lib.amgh_debug_set_perm_io(0) == 0 and lib.amgh_debug_get_perm_io() == 0
        off = fn()
        assert count() == c1, ("switched off, yet folded in", c1, count())
    finally:
        assert lib.amgh_debug_set_perm_io(saved) == 0
    return on, off


@functools.lru_cache(maxsize=None)
def _level0_mode(shape, dtype):
    """amgh_debug_bw_mode of level 0 of poisson(shape) — the schedule depends on the matrix, not on the smoother: asked once a shape"""
    A = AMG.poisson(shape)
    if dtype is F32:
        A = AMG.SparseMatrixCSC.from_scipy(A.to_scipy().astype(F32))
    dev = DeviceHierarchy(AMG.ruge_stuben(A), 0, 1, dtype=dtype)
    return AMG.hip_lib("float32" if dtype is F32 else "float64").amgh_debug_bw_mode(dev.h, 0)


def skip_unless_on_the_dataflow_path(shape, dtype=np.float64):
    """before a case builds anything: level 0 runs the relayed dataflow sweep — or the case tests nothing: skipped (the 24^3 grid
    only), never passed"""
    mode = _level0_mode(tuple(shape), dtype)
    if mode != 3:
        assert tuple(shape) == (24, 24, 24), (shape, mode)      # every other size must have the block layout
        pytest.skip("poisson(%r): level 0 keeps the level schedules (amgh_debug_bw_mode = %d), no sweep to fold anything into" % (shape, mode))


def on_the_dataflow_path(lib, dev, shape):
    """... and the handle of the case itself is"""
    assert lib.amgh_debug_bw_mode(dev.h, 0) == 3, shape


SMOOTHERS = {
    "symmetric": lambda: (AMG.GaussSeidel(), AMG.GaussSeidel()),
    "forward": lambda: (AMG.GaussSeidel(AMG.ForwardSweep()), AMG.GaussSeidel(AMG.ForwardSweep())),
    "backward": lambda: (AMG.GaussSeidel(AMG.BackwardSweep()), AMG.GaussSeidel(AMG.BackwardSweep())),
    "forward2-backward": lambda: (AMG.GaussSeidel(AMG.ForwardSweep(), iter=2), AMG.GaussSeidel(AMG.BackwardSweep())),
    "sor1.2": lambda: (AMG.SOR(1.2), AMG.SOR(1.2)),
    "sor1.2-forward": lambda: (AMG.SOR(1.2, AMG.ForwardSweep()), AMG.SOR(1.2, AMG.ForwardSweep())),
}


@pytest.mark.parametrize("shape", SIZES)
@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_apply_and_solve_are_bitwise_the_separate_kernels(shape, smoother):
    """amgh_precond_apply (x = 0 on entry: both order changes folded in) and amgh_solve from a non-zero x (its gather of x
    stays a kernel of its own) for V, W and F cycles, with the stored-order row sum and with the dependency-aware one."""
    skip_unless_on_the_dataflow_path(shape)
    lib = AMG.hip_lib()
    A = AMG.poisson(shape)
    pre, post = SMOOTHERS[smoother]()
    ml = AMG.ruge_stuben(A, presmoother=pre, postsmoother=post)
    dev = DeviceHierarchy(ml, 0, 1)
    on_the_dataflow_path(lib, dev, shape)
    oh = O.OracleHierarchy(ml)
    b = uniform(A.m, 11) - 0.4
    x0 = uniform(A.m, 12) - 0.5
    for inorder in (1, 0):
        with pinned(lib, gs_bw_inorder=inorder):
            for cyc in (V, W, F):
                z_on, z_off = both(lib, lambda: dev.precond_apply(b, cyc))
                assert same_bytes(z_on, z_off), (shape, smoother, inorder, cyc)
                assert rel(z_on, oh.precond(b, cyc)) <= TOL, (shape, smoother, inorder, cyc)
                s_on, s_off = both(lib, lambda: dev.solve(b, x0, cyc, 3, 0.0, 0.0, True, True))
                assert same_bytes(s_on[0], s_off[0]) and same_bytes(s_on[1], s_off[1]) and s_on[2] == s_off[2], (shape, smoother, inorder, cyc)
                xo, _, _ = oh.solve(b, x0=x0, cycle=cyc, maxiter=3, abstol=0.0, reltol=0.0)
                assert rel(s_on[0], xo) <= TOL, (shape, smoother, inorder, cyc)
    assert lib.amgh_debug_bw_poll_giveups(dev.h, 0) == 0


@pytest.mark.parametrize("shape", SIZES)
def test_graph_replay_on_and_off(shape):
    """Captured cycles bake the path in; the switch bumps the epoch, so each setting is warmed up, captured and replayed."""
    skip_unless_on_the_dataflow_path(shape)
    lib = AMG.hip_lib()
    A = AMG.poisson(shape)
    ml = AMG.ruge_stuben(A)
    g, e = DeviceHierarchy(ml, 0, 1), DeviceHierarchy(ml, 0, 1)
    on_the_dataflow_path(lib, g, shape)
    assert lib.amgh_set_use_graph(g.h, 1) == 0 and lib.amgh_set_use_graph(e.h, 0) == 0
    b = uniform(A.m, 21) - 0.3
    x0 = uniform(A.m, 22) - 0.5
    for cyc in (V, W, F):
        def run(dev):
            return [dev.precond_apply(b, cyc) for _ in range(4)] + [dev.solve(b, x0, cyc, 2, 0.0, 0.0, False, False)[0] for _ in range(4)]
        g_on, g_off = both(lib, lambda: run(g))
        e_on, e_off = both(lib, lambda: run(e))
        for k in range(8):
            assert same_bytes(g_on[k], e_on[0 if k < 4 else 4]), (shape, cyc, k)
            assert same_bytes(g_on[k], g_off[k]) and same_bytes(e_on[k], e_off[k]) and same_bytes(g_off[k], e_off[k]), (shape, cyc, k)
    assert lib.amgh_debug_bw_poll_giveups(g.h, 0) == 0


def _float32_case(lib32, A, what, x):
    """Float32 cycles and solves on A with the switch on and off; x: whether the last sweep must have written x in natural order"""
    b = (uniform(A.m, 31) - 0.3).astype(F32)
    x0 = (uniform(A.m, 32) - 0.5).astype(F32)
    for pre, post in ((AMG.GaussSeidel(), AMG.GaussSeidel()), (AMG.SOR(1.2, AMG.ForwardSweep()), AMG.SOR(1.2, AMG.BackwardSweep()))):
        ml = AMG.ruge_stuben(A, presmoother=pre, postsmoother=post)
        dev = DeviceHierarchy(ml, 0, 1, dtype=F32)
        on_the_dataflow_path(lib32, dev, what)
        oh = O.OracleHierarchy(ml, dtype=F32)
        for inorder in (1, 0):
            with pinned(lib32, gs_bw_inorder=inorder):
                for cyc in (V, W, F):
                    z_on, z_off = both(lib32, lambda: dev.precond_apply(b, cyc), x=x)
                    assert z_on.dtype == F32 and same_bytes(z_on, z_off), (what, repr(pre), inorder, cyc)
                    assert rel(z_on, oh.precond(b, cyc)) <= F32_TOL, (what, repr(pre), inorder, cyc)
                    s_on, s_off = both(lib32, lambda: dev.solve(b, x0, cyc, 2, 0.0, 0.0, False, False)[0], x=x)
                    assert same_bytes(s_on, s_off), (what, repr(pre), inorder, cyc)
        assert lib32.amgh_debug_bw_poll_giveups(dev.h, 0) == 0


@pytest.mark.parametrize("shape", SIZES)
def test_float32_library(shape):
    """The Float32 library is built from the same source.  7-point operators at shipping defaults are on the dictionary layout
    with rows of <= 12 entries: b through the permutation, and the scatter kernel kept (gs_relay.hpp RelayPermX: those kernels
    would lose a wave of occupancy with the extra store) on level 0; a coarser level with longer rows may fold x in, so that
    counter is not asked here.  The two tests below are the ones in which Float32 sweeps must write x in natural order."""
    skip_unless_on_the_dataflow_path(shape, F32)
    lib32 = AMG.hip_lib("float32")
    A = AMG.SparseMatrixCSC.from_scipy(AMG.poisson(shape).to_scipy().astype(F32))
    _float32_case(lib32, A, shape, x=None)


@pytest.mark.parametrize("shape", SIZES[1:])
def test_float32_library_writes_x_in_natural_order_from_plain_records(shape):
    """Without the dictionary (gs_bw_dict = 0 when the schedule is built) the same levels run the plain-record kernels, which
    take both order changes.  Blocks of the planner's own size: 512 rows with a halo of fewer entries than rows, where the
    block's slice of the permutation (4 bytes a row) is as large as the block's x in LDS."""
    skip_unless_on_the_dataflow_path(shape, F32)
    lib32 = AMG.hip_lib("float32")
    A = AMG.SparseMatrixCSC.from_scipy(AMG.poisson(shape).to_scipy().astype(F32))
    with pinned(lib32, gs_bw_dict=0):
        _float32_case(lib32, A, shape, x=True)


@pytest.mark.parametrize("rows", [64, 512])
def test_float32_library_writes_x_in_natural_order_on_a_19_point_operator(rows):
    """Rows of up to 18 off-diagonal entries (the second level of a Poisson hierarchy as a fine operator, block layout forced as
    in test_gpu_late.py): the dictionary layout at MAXK 18 takes both order changes in Float32 too.  Blocks of 64 rows (halo
    larger than the block) and of 512 (smaller)."""
    lib32 = AMG.hip_lib("float32")
    A1 = AMG.ruge_stuben(AMG.poisson((32, 30, 28))).levels[1].A.to_scipy().tocsr()
    assert int(np.diff(A1.indptr).max()) - 1 > 12
    A = AMG.SparseMatrixCSC.from_scipy(A1.astype(F32))
    with pinned(lib32, gs_bw=2, gs_bw_rows=rows, gs_lean=0):
        _float32_case(lib32, A, ("galerkin19", rows), x=True)


@pytest.mark.parametrize("shape", SIZES)
def test_pcg_iterations_and_residual_history(shape):
    """Every preconditioner application inside amgh_pcg runs the two folded sweeps: the same iterates, count and history."""
    skip_unless_on_the_dataflow_path(shape)
    lib = AMG.hip_lib()
    A = AMG.poisson(shape)
    ml = AMG.ruge_stuben(A)
    dev = DeviceHierarchy(ml, 0, 1)
    on_the_dataflow_path(lib, dev, shape)
    b = uniform(A.m, 41) - 0.2
    for fused in (1, 0):
        with pinned(lib, pcg_fused=fused):
            (x_on, h_on, it_on), (x_off, h_off, it_off) = both(lib, lambda: dev.pcg(b, V, True, 60, 0.0, 1e-10))
            assert it_on == it_off and 0 < it_on < 60, (shape, fused, it_on, it_off)
            assert same_bytes(h_on, h_off) and same_bytes(x_on, x_off), (shape, fused)
            assert h_on[-1] <= 1e-10 * h_on[0] * 1.0000001
    g_on, g_off = both(lib, lambda: dev.gmres(b, V, True, 10, 40, 0.0, 1e-10))
    assert g_on[2] == g_off[2] and same_bytes(g_on[0], g_off[0]) and same_bytes(g_on[1], g_off[1]), shape


def test_a_block_of_four_right_hand_sides_still_runs_the_kernels_of_their_own():
    """ncolv = 4: the multi-column dataflow sweep, gather and scatter kernels as before, whatever the switch says."""
    lib = AMG.hip_lib()
    A = AMG.poisson((40, 40, 40))
    ml = AMG.ruge_stuben(A)
    with pinned(lib, gs_bw_nrhs=1):
        devb = DeviceHierarchy(ml, 0, 4)
    dev1 = DeviceHierarchy(ml, 0, 1)
    assert lib.amgh_debug_bw_mode(devb.h, 0) == 3 and lib.amgh_debug_bw_mode(dev1.h, 0) == 3
    oh = O.OracleHierarchy(ml)
    n = A.m
    B = np.asfortranarray(np.stack([uniform(n, 50 + c) - 0.1 * c for c in range(4)], axis=1))
    X0 = np.asfortranarray(np.stack([uniform(n, 60 + c) - 0.5 for c in range(4)], axis=1))
    for cyc in (V, W, F):
        z_on, z_off = both(lib, lambda: devb.precond_apply(B, cyc), b=False, x=False)
        s_on, s_off = both(lib, lambda: devb.solve(B, X0, cyc, 2, 0.0, 0.0, False, False)[0], b=False, x=False)
        assert same_bytes(z_on, z_off) and same_bytes(s_on, s_off), cyc
        for c in range(4):
            bc = B[:, c].copy()
            assert rel(z_on[:, c], oh.precond(bc, cyc)) <= TOL, (cyc, c)
            assert same_bytes(z_on[:, c].copy(), dev1.precond_apply(bc, cyc)), (cyc, c)      # (stored-order sums, one thread per row: the single column's bits)
    assert lib.amgh_debug_bw_poll_giveups(devb.h, 0) == 0


_FULL = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import amg_amd as AMG
from conftest import uniform
from oracle import oracle as O
lib = AMG.hip_lib()
A = AMG.poisson((256, 256, 256))
ml = AMG.ruge_stuben(A, setup="gpu", device=0)
dev = ml.device(0, 1)
assert lib.amgh_debug_bw_mode(dev.h, 0) == 3 and lib.amgh_debug_bw_late(dev.h, 0) == 1
b = uniform(A.m, 0)
out = {}
for v in (1, 0, 1):
    assert lib.amgh_debug_set_perm_io(v) == 0          # the only switch this process ever sets: every tunable at its compiled-in value
    z = dev.precond_apply(b)
    out.setdefault(v, []).append(z)
assert lib.amgh_debug_bw_poll_giveups(dev.h, 0) == 0
zo = O.OracleHierarchy(ml).precond(b)
err = float(np.linalg.norm(out[1][0] - zo) / np.linalg.norm(zo))
eq = [bool(np.array_equal(out[1][0].view(np.uint8), z.view(np.uint8))) for z in (out[0][0], out[1][1])]
print("PERM_IO_256 equal_off=%d equal_again=%d err=%.3e" % (eq[0], eq[1], err))
"""


def test_256_cubed_at_shipping_defaults_in_a_process_that_sets_no_other_tunable():
    """The benchmark's cycle: z of amgh_precond_apply bitwise equal under both settings and within 1e-10 of the oracle."""
    r = subprocess.run([sys.executable, "-c", _FULL, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith("PERM_IO_256")][-1]
    print(line)
    f = dict(kv.split("=") for kv in line.split()[1:])
    assert f["equal_off"] == "1" and f["equal_again"] == "1", line
    assert float(f["err"]) <= TOL, line
