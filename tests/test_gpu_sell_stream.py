"""The sliced-ELL launches of the level-ordered single-column cycle (csrc/hip/amghip_kernels.hpp sell_stream_kernel; switch
amgh_debug_set_sell_stream): residual, restriction and prolongation of the big operators read a copy with one row per lane —
slices of 64 consecutive rows, entry t of the 64 rows adjacent in memory.  A lane adds its row's products in CSR entry order
from 0.0, so with the switch on and off every output is the same BIT FOR BIT (raw bytes compared, no tolerance), and the
stand-alone operators equal a scalar in-order loop on the host bit for bit.

The copies are built at amgh_finalize for operators of >= 2^18 rows; the cases lower that through the switch's second argument
before they build a handle, and read amgh_debug_sell_stream_launches around every call: with the switch on the operators that
have a copy must have gone through the new kernel, with the switch off none."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import amg_amd as AMG
from amg_amd.device import DeviceBuffer, DeviceCSR, DeviceHierarchy
from conftest import uniform
from oracle import oracle as O
from shipping_defaults import pinned

pytestmark = pytest.mark.gpu

TOL = 1e-10            # the project's tolerance for a cycle against the oracle
F32 = np.float32
F32_TOL = 5e-5         # (test_gpu_float32.py)
V, W = 0, 1
A_, P_, R_ = 0, 1, 2   # AMGH_OP_A / P / R


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


def same_bytes(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _bind(lib):
    lib.amgh_debug_set_sell_stream.argtypes = [C.c_int, C.c_int64, C.c_int]
    lib.amgh_debug_sell_stream_launches.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.amgh_debug_sell_stream_padded.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.amgh_debug_sell_stream_padded.restype = C.c_int64
    lib.amgh_debug_csr_sell.argtypes = [C.c_void_p, C.c_int]
    lib.amgh_debug_csr_sell.restype = C.c_int64
    lib.amgh_debug_csr_sell_launches.argtypes = [C.c_void_p]
    lib.amgh_debug_csr_sell_apply.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    return lib


@contextlib.contextmanager
def sell(lib, min_rows=64, cap_pct=0):
    """the threshold lowered (and the cap as asked) for what is BUILT inside; the compiled-in values afterwards"""
    try:
        assert lib.amgh_debug_set_sell_stream(1, min_rows, cap_pct) == 0 and lib.amgh_debug_get_sell_stream() == 1
        yield
    finally:
        assert lib.amgh_debug_set_sell_stream(1, 0, 0) == 0


def taken(lib, dev, nlev):
    """the (level, operator) pairs that have a sliced-ELL copy"""
    return {(l, w) for l in range(nlev) for w in (A_, P_, R_) if lib.amgh_debug_sell_stream_padded(dev.h, l, w) > 0}


def counts(lib, dev, nlev):
    return {(l, w): lib.amgh_debug_sell_stream_launches(dev.h, l, w) for l in range(nlev) for w in (A_, P_, R_)}


def both(lib, dev, nlev, fn, must):
    """fn() with the switch on, then off.  On: exactly operators that have a copy launch the new kernel, every pair of `must` among
    them; off: none does."""
    have = taken(lib, dev, nlev)
    assert must <= have, (must, have)
    try:
        assert lib.amgh_debug_set_sell_stream(1, 64, 0) == 0
        c0 = counts(lib, dev, nlev)
        on = fn()
        c1 = counts(lib, dev, nlev)
        ran = {k for k in c1 if c1[k] > c0[k]}
        assert must <= ran <= have, (must, ran, have)
        assert lib.amgh_debug_set_sell_stream(0, 64, 0) == 0 and lib.amgh_debug_get_sell_stream() == 0
        off = fn()
        assert counts(lib, dev, nlev) == c1, "switched off, yet launched"
    finally:
        assert lib.amgh_debug_set_sell_stream(1, 0, 0) == 0
    return on, off


def permuted(A, seed):
    """P A P^T for the permutation that sorts a splitmix64 stream: the same operator, its columns no lattice walk"""
    S = A.to_scipy().tocsr()
    p = np.argsort(uniform(S.shape[0], seed), kind="stable")
    return AMG.SparseMatrixCSC.from_scipy(S[p][:, p].tocsc())


def _poisson3():
    return AMG.poisson((40, 40, 40))


NATURAL = "the rule, on the host"   # level 0 runs in natural order: the pairs are what the structural rule gives for A, P, R as they stand

CASES = {
    # name: (matrix, dtype, tunables pinned while the handle is built, pairs of level 0 that must — and alone may — run the new kernel)
    # 40^3 (plain form: value-coded words exist from 2^18 rows): 7-point A, R with 7 entries in every row, and the 1-or-6-entry P, which
    # pads to 171 % and stays on csr_stream_kernel; 19-point and longer rows on the levels below
    "poisson40^3": (_poisson3, np.float64, {}, {(0, A_), (0, R_)}),
    # (the coarsening of the permuted operator is another one: what its R and P pad to is not known here, A's rows keep their lengths)
    "poisson40^3-permuted": (lambda: permuted(_poisson3(), 2024), np.float64, {}, None),
    # (hierarchies this small are collapsed into one dense operator by default: tail_dense_rows = 0 keeps the per-level cycle; their
    #  levels sweep dense triangles, so the cycle runs in natural order and multiplies with A, R, P themselves)
    "poisson300": (lambda: AMG.poisson((300,)), np.float64, {"tail_dense_rows": 0}, NATURAL),     # 300 = 4 * 64 + 44: a short last slice
    "poisson37x41": (lambda: AMG.poisson((37, 41)), np.float64, {"tail_dense_rows": 0}, NATURAL),  # 1517 = 23 * 64 + 45
    "poisson40^3-plain": (_poisson3, np.float64, {"stream_code": 0}, {(0, A_), (0, R_)}),
    "poisson40^3-float32": (_poisson3, F32, {}, {(0, A_), (0, R_)}),
    # 270 336 rows: A in the value-coded form, at the size it is built from (R, 135 168 rows, in the plain form; P is ragged)
    "poisson64x64x66-coded": (lambda: AMG.poisson((64, 64, 66)), np.float64, {}, {(0, A_), (0, R_)}),
}
CAP_PLAIN = 110      # kSellCapPlainPct (amghip_internal.hpp)


def rule(M, min_rows=64, cap=CAP_PLAIN):
    """the structural rule for an operator in the row order given: at least min_rows rows, padded entries within the cap"""
    S = M.to_scipy().tocsr()
    ln = np.diff(S.indptr)
    padded = 64 * sum(int(ln[s:s + 64].max()) for s in range(0, len(ln), 64))
    return len(ln) >= min_rows and S.nnz > 0 and padded * 100 <= S.nnz * cap


@pytest.mark.parametrize("case", sorted(CASES))
def test_cycles_are_bitwise_the_csr_launches(case):
    """ldiv! (a V cycle from x = 0) and a W cycle (solve from a non-zero x, one iteration), switch on against off."""
    make, dtype, tun, must = CASES[case]
    lib = _bind(AMG.hip_lib("float32" if dtype is F32 else "float64"))
    A = make()
    if dtype is F32:
        A = AMG.SparseMatrixCSC.from_scipy(A.to_scipy().astype(F32))
    ml = AMG.ruge_stuben(A)
    nlev = len(ml.levels)
    # (both copies kept: the cases switch between them at run time; the coded words exist from the lowered threshold on)
    with sell(lib), pinned(lib, trim_coded=0, **tun):
        dev = DeviceHierarchy(ml, 0, 1, dtype=dtype)
    assert lib.amgh_debug_coded_ops(dev.h, 0) & 1 == (1 if case.endswith("-coded") else 0), case      # the form the case is about
    level0 = {k for k in taken(lib, dev, nlev) if k[0] == 0}
    if must is NATURAL:
        lv = ml.levels[0]
        must = {(0, w) for w, M in ((A_, lv.A), (P_, lv.P), (R_, lv.R)) if rule(M)}
        assert (0, A_) in must, case
    if must is None:
        must = {(0, A_)}
        assert (0, P_) not in level0, case
    else:
        assert level0 == must, (case, level0, must)
    b = (uniform(A.m, 31) - 0.4).astype(dtype)
    x0 = (uniform(A.m, 32) - 0.5).astype(dtype)
    z_on, z_off = both(lib, dev, nlev, lambda: dev.precond_apply(b), must)
    assert same_bytes(z_on, z_off), case
    s_on, s_off = both(lib, dev, nlev, lambda: dev.solve(b, x0, W, 1, 0.0, 0.0, True, True), must)
    assert same_bytes(s_on[0], s_off[0]) and same_bytes(s_on[1], s_off[1]), case
    if case == "poisson40^3":
        assert rel(z_on, O.OracleHierarchy(ml).precond(b)) <= TOL
    if dtype is F32:
        assert rel(z_on, O.OracleHierarchy(ml).precond(b.astype(np.float64))) <= F32_TOL


def test_blocks_of_right_hand_sides_stay_on_the_csr_launches():
    lib = _bind(AMG.hip_lib())
    A = _poisson3()
    ml = AMG.ruge_stuben(A)
    nlev = len(ml.levels)
    with sell(lib):
        dev = DeviceHierarchy(ml, 0, 2)
        B = np.stack([uniform(A.m, 41) - 0.4, uniform(A.m, 42) - 0.6], axis=1)
        assert taken(lib, dev, nlev) == set()
        c0 = counts(lib, dev, nlev)
        z_on = dev.precond_apply(B)
        assert counts(lib, dev, nlev) == c0 and all(v == 0 for v in c0.values())
        assert lib.amgh_debug_set_sell_stream(0, 64, 0) == 0
        z_off = dev.precond_apply(B)
    assert same_bytes(z_on, z_off)
    oh = O.OracleHierarchy(ml)
    for c in range(2):
        assert rel(z_on[:, c], oh.precond(B[:, c])) <= TOL


# ---- the layout itself: stand-alone operators (amgh_debug_csr_sell gives one its copy, amgh_debug_csr_sell_apply launches as the cycle does)

def host_rows(rowptr, col, val, x):
    """acc = 0.0, then acc = acc + v * x[c] in entry order, the product rounded on its own: the scalar loop, all rows at once"""
    n = len(rowptr) - 1
    ln = np.diff(rowptr)
    acc = np.zeros(n, dtype=val.dtype)
    for t in range(int(ln.max()) if n else 0):
        m = np.nonzero(ln > t)[0]
        k = rowptr[m] + t
        acc[m] = acc[m] + val[k] * x[col[k]]
    return acc


def random_rows(lengths, ncols, seed, values=None, dtype=np.float64):
    lengths = np.asarray(lengths, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = np.minimum((uniform(nnz, seed) * ncols).astype(np.int64), ncols - 1).astype(np.int32)
    if values is None:
        val = (uniform(nnz, seed + 1) - 0.5).astype(dtype)
    else:
        val = np.asarray(values, dtype=dtype)[(uniform(nnz, seed + 1) * len(values)).astype(np.int64) % len(values)]
    return rowptr, col, val


def check_operator(lib, rowptr, col, val, ncols, coded, expect_copy, cap_pct, dtype=np.float64):
    n = len(rowptr) - 1
    op = DeviceCSR(n, ncols, rowptr, col, val, dtype=dtype)
    with sell(lib, 1, cap_pct):
        padded = lib.amgh_debug_csr_sell(op.h, coded)
    assert padded >= 0
    if expect_copy:
        # as many steps as the longest row of every slice of 64
        ln = np.diff(rowptr)
        assert padded == 64 * sum(int(ln[s:s + 64].max()) for s in range(0, n, 64))
    else:
        assert padded == 0
    x = (uniform(ncols, 7) - 0.5).astype(dtype)
    b = (uniform(n, 8) + 1.0).astype(dtype)
    y0 = (uniform(n, 9) - 2.0).astype(dtype)        # M_ADD into a non-zero y
    acc = host_rows(rowptr, col, val, x)
    want = {"spmv": acc, "residual": b - acc, "add": y0 + acc}
    out = {}
    try:
        for on in (1, 0):
            assert lib.amgh_debug_set_sell_stream(on, 0, 0) == 0
            c0 = lib.amgh_debug_csr_sell_launches(op.h)
            out[on] = {}
            for k, mode in (("spmv", 0), ("residual", 1), ("add", 2)):
                xd, bd = DeviceBuffer(ncols, 0, x, dtype=dtype), DeviceBuffer(n, 0, b, dtype=dtype)
                yd = DeviceBuffer(n, 0, y0, dtype=dtype)
                assert lib.amgh_debug_csr_sell_apply(op.h, mode, xd.ptr, bd.ptr, yd.ptr) == 0
                out[on][k] = yd.download()
            assert lib.amgh_debug_csr_sell_launches(op.h) - c0 == (3 if on and expect_copy else 0)
    finally:
        assert lib.amgh_debug_set_sell_stream(1, 0, 0) == 0
    for k in want:
        assert same_bytes(out[1][k], out[0][k]), k
        assert same_bytes(out[1][k], want[k]), k


@pytest.mark.parametrize("coded", [0, 1])
@pytest.mark.parametrize("nrows", [63, 64, 65, 192])
def test_slices_tails_and_empty_rows(nrows, coded):
    """63 / 64 / 65 rows (a short, a full, a full and a one-row slice); an empty row; 192 rows whose middle slice is all empty"""
    lib = _bind(AMG.hip_lib())
    ln = 1 + (uniform(nrows, 3) * 9).astype(np.int64)
    ln[5] = 0
    if nrows == 192:
        ln[64:128] = 0
    rowptr, col, val = random_rows(ln, 500, 100 + nrows, values=[-1.0, 6.0, 0.25, -0.0, 1e-3])
    check_operator(lib, rowptr, col, val, 500, coded, True, 1000)


@pytest.mark.parametrize("long_row", [200, 300])
def test_one_long_row_among_short_ones(long_row):
    """65 rows of 3 entries and one of 200 / 300: far above the cap, the operator keeps csr_stream_kernel and the counter says so;
    with the cap lifted it takes the copy (300 entries: the lengths no longer fit a byte, they come from the row pointers)."""
    lib = _bind(AMG.hip_lib())
    ln = np.full(65, 3, dtype=np.int64)
    ln[17] = long_row
    rowptr, col, val = random_rows(ln, 4096, 200 + long_row)
    check_operator(lib, rowptr, col, val, 4096, 0, False, 0)
    check_operator(lib, rowptr, col, val, 4096, 0, True, 100000)


def test_the_word_of_all_ones_is_an_entry():
    """2^24 columns, entries in column 2^24 - 1 carrying the table's code 255: the word 0xFFFFFFFF is a legal entry, and rows of
    other lengths beside it are padded — a lane tells the two apart by its row's length alone."""
    lib = _bind(AMG.hip_lib())
    ncols = 1 << 24
    table = np.concatenate([np.arange(1, 256, dtype=np.float64) / 8.0, [-3.0]])      # by bit pattern -3.0 sorts last: code 255
    ln = 3 + (np.arange(130) % 5)
    rowptr, col, val = random_rows(ln, ncols, 77)
    last = rowptr[1:] - 1                                  # the last entry of every row: column 2^24 - 1, value -3.0
    rest = np.setdiff1d(np.arange(len(val)), last)
    val[rest] = table[np.arange(len(rest)) % 255]          # (every other code is used too)
    col[last] = ncols - 1
    val[last] = -3.0
    used = np.unique(val)
    assert len(used) == 256 and np.array_equal(np.sort(used.view(np.uint64))[-1:], np.array([-3.0]).view(np.uint64))
    check_operator(lib, rowptr, col, val, ncols, 1, True, 1000)


def test_float32_operator():
    lib = _bind(AMG.hip_lib("float32"))
    ln = 1 + (uniform(150, 5) * 12).astype(np.int64)
    rowptr, col, val = random_rows(ln, 300, 55, values=[-1.0, 6.0, 0.125, 3.0], dtype=F32)
    for coded in (0, 1):
        check_operator(lib, rowptr, col, val, 300, coded, True, 1000, dtype=F32)
