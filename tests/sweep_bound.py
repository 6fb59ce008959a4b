"""A per-row error bound for ONE directional row-by-row sweep (Gauss-Seidel or SOR, forward or backward), checked against a
long-double restatement of every row that uses the sweep's own output.

For row i of the operator the oracle reads (oracle/amg_oracle.c: with `hermitian`, column i of the CSC; otherwise row i of A)
let y_k = xhat_k for the rows the sweep has already done and y_k = x0_k for the rest.  Then, in np.longdouble,

    x*_i = (1 - w) x0_i + w (b_i - sum_{k != i} a_ik y_k) / a_ii

and the sweep's value must satisfy

    |xhat_i - x*_i| <= (m_i + 4) u (|w| (|b_i| + sum |a_ik y_k|) / |a_ii| + |1 - w| |x0_i|) + floor_i

with m_i the row's off-diagonal count, u = 2^-53 (Float64) or 2^-24 (Float32) and floor_i = (m_i + 4) tiny (|w| / |a_ii| + 1)
for underflow (tiny: the smallest normal number).  A zero diagonal requires xhat_i == x0_i exactly (smoother.jl:87).
Every y_k is known once the sweep is done, so the check is vectorised: no sequential loop.  It holds for ANY order of the
row's additions, fused or not, and for a quotient formed from a rounded reciprocal — what the stored-order scalar loop,
the relayed walk's split (LATE) row sum, the four-lane single-wave walk and the multi-column dataflow sweep compute — and
it fails for an iterate that read an old value where the sweep had already produced a new one (a stale dependency).

Kernels it does NOT apply to, because none of them computes one sum and one division per row from the sweep's inputs:
- merged groups with composite rows (gs_merge_dev.hpp: a composite row folds several dependency levels' rows together);
- block inverses (gs_block_inverse: a small block is solved through its explicit inverse, rows mixed together);
- dense triangles (gs_dense_tri: the sweep of a small operator through the dense inverse of its whole triangle);
- the collapsed dense tail (tail_dense: a whole coarse recursion applied as one dense operator, no sweep at all).
Those are checked against the oracle with norm tolerances where they are tested.  Symmetric and repeated smoothers are not
judged either: they make two or more passes, and the iterate between them is not observable from outside the kernel."""
import numpy as np

SLACK = 4


def _rows(A, hermitian):
    """(rowptr, col, val) of the operator row by row as the oracle reads it."""
    if hermitian:
        return np.asarray(A.colptr, np.int64), np.asarray(A.rowval, np.int64), np.asarray(A.nzval)
    S = A.to_scipy().tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data


def sweep_errors(A, x0, b, xhat, backward=False, omega=1.0, dtype=np.float64, hermitian=True):
    """(err, tol, zero_diag, checked) per row: |xhat - x*| in long double, the bound, the rows whose diagonal is zero, and the
    rows whose inputs and exact update are finite (the others are not judged)."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "needs an 80-bit (or wider) long double"
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    u = ld(2.0) ** -(fi.nmant + 1)
    n = A.m
    rp, ci, va = _rows(A, hermitian)
    va = va.astype(dtype).astype(ld)                   # the operator as the sweep's arithmetic type holds it
    x0 = np.asarray(x0, dtype=dtype).astype(ld)
    b = np.asarray(b, dtype=dtype).astype(ld)
    xh = np.asarray(xhat, dtype=dtype).astype(ld)
    row = np.repeat(np.arange(n), np.diff(rp))
    diag = ci == row
    d = np.zeros(n, dtype=ld)
    d[row[diag]] = va[diag]                            # (the oracle's loop keeps the last diagonal entry it meets)
    off = ~diag
    r_off, c_off, v_off = row[off], ci[off], va[off]
    done = c_off > r_off if backward else c_off < r_off
    y = np.where(done, xh[c_off], x0[c_off])
    p = v_off * y
    s = np.zeros(n, dtype=ld)
    sa = np.zeros(n, dtype=ld)
    np.add.at(s, r_off, p)
    np.add.at(sa, r_off, np.abs(p))
    m = np.bincount(r_off, minlength=n).astype(ld)
    w = ld(omega)
    zero = d == 0
    dd = np.where(zero, ld(1), d)
    xs = (ld(1) - w) * x0 + w * (b - s) / dd
    ad = np.abs(dd)
    tol = (m + SLACK) * u * (np.abs(w) * (np.abs(b) + sa) / ad + np.abs(ld(1) - w) * np.abs(x0))
    tol += (m + SLACK) * ld(fi.tiny) * (np.abs(w) / ad + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(xh - xs)
        fin_in = np.ones(n, dtype=bool)
        np.logical_and.at(fin_in, r_off, np.isfinite(y))
        checked = fin_in & np.isfinite(x0) & np.isfinite(b) & np.isfinite(xs) & np.isfinite(tol) & (np.abs(xs) <= ld(fi.max))
    return err, tol, zero, checked


def assert_sweep_within_bound(A, x0, b, xhat, backward=False, omega=1.0, dtype=np.float64, hermitian=True, what=""):
    """Raise AssertionError naming the worst row unless every judged row is within its bound; returns the worst err / tol."""
    xhat = np.asarray(xhat)
    err, tol, zero, checked = sweep_errors(A, x0, b, xhat, backward, omega, dtype, hermitian)
    x0c = np.asarray(x0, dtype=dtype)
    xhc = np.asarray(xhat, dtype=dtype)
    moved = zero & ~(xhc == x0c)
    assert not moved.any(), "%s: zero-diagonal rows changed: %s" % (what, np.flatnonzero(moved)[:8].tolist())
    nz = checked & ~zero
    assert np.all(np.isfinite(xhc[nz])), "%s: non-finite values where the exact update is finite" % what
    ratio = np.zeros(len(err))
    ratio[nz] = (err[nz] / np.maximum(tol[nz], np.finfo(np.longdouble).tiny)).astype(np.float64)
    worst = int(np.argmax(ratio)) if len(ratio) else 0
    assert np.all(err[nz] <= tol[nz]), "%s: row %d off by %.3g of its bound (%d rows over, %d judged)" % (
        what, worst, ratio[worst], int(np.count_nonzero(err[nz] > tol[nz])), int(np.count_nonzero(nz)))
    assert np.count_nonzero(nz) >= 0.9 * np.count_nonzero(~zero), "%s: too few rows judged" % what
    return float(ratio[worst]) if len(ratio) else 0.0


def directional(pre):
    """(backward, omega) of a smoother that makes exactly ONE directional sweep (iter = 1, forward or backward), else None."""
    if getattr(pre, "iter", 1) != 1 or getattr(pre, "sweep_code", None) not in (0, 1):
        return None
    return pre.sweep_code == 1, float(getattr(pre, "omega", 1.0))


def smooth_block(dev, level, post, X0, B):
    """the level's smoother on all columns of a block handle at once (amgh_debug_level_smooth_block_d: the cycle's multi-column
    sweep); X0, B: n x nrhs"""
    from amg_amd.device import DeviceBuffer
    n, bs = X0.shape
    assert bs == dev.nrhs
    xd = DeviceBuffer(n * bs, host=np.asarray(X0, dtype=dev.dtype).ravel(order="F"), dtype=dev.dtype)
    bd = DeviceBuffer(n * bs, host=np.asarray(B, dtype=dev.dtype).ravel(order="F"), dtype=dev.dtype)
    assert dev.lib.amgh_debug_level_smooth_block_d(dev.h, level, int(post), xd.ptr, bd.ptr) == 0
    return xd.download().reshape((n, bs), order="F")
