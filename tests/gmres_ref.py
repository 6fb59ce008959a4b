"""Host restatement of the device GMRES (amgh_gmres): IterativeSolvers.jl's restarted, left-preconditioned gmres with
x0 = 0, classical Gram-Schmidt with the DGKS test capped at two extra passes, the null-vector residual estimate and
Givens least squares.  A plain helper module (not a conftest): the tests import it as `gmres_ref`.

Pl is a callable r -> Pl \\ r: `OracleHierarchy(ml).precond` (one cycle from x = 0, the reference's ldiv!,
preconditioner.jl:12-19) or the identity."""
import numpy as np

MAX_EXTRA = 2   # DGKS re-orthogonalisation passes per Arnoldi step, at most (the device's kGmMaxExtra)


def identity(r):
    return np.array(r, dtype=np.float64, copy=True)


def _lsq(H, beta, k):
    """min_y |beta e1 - H[:k+1, :k] y| by Givens rotations and back substitution (IterativeSolvers' FastHessenberg)."""
    R = H[:k + 1, :k].copy()
    rhs = np.zeros(k + 1)
    rhs[0] = beta
    for i in range(k):
        a, b = R[i, i], R[i + 1, i]
        r = np.sqrt(a * a + b * b)
        c, s = (a / r, b / r) if r != 0.0 else (1.0, 0.0)
        R[i, i] = c * a + s * b
        R[i + 1, i] = 0.0
        hi, hn = R[i, i + 1:].copy(), R[i + 1, i + 1:].copy()
        R[i, i + 1:] = c * hi + s * hn
        R[i + 1, i + 1:] = -s * hi + c * hn
        rhs[i], rhs[i + 1] = c * rhs[i] + s * rhs[i + 1], -s * rhs[i] + c * rhs[i + 1]
    y = np.zeros(k)
    for i in range(k - 1, -1, -1):
        t = rhs[i]
        for j in range(i + 1, k):
            t -= R[i, j] * y[j]
        y[i] = t / R[i, i]
    return y


def gmres(A, b, Pl=identity, restart=None, maxiter=None, abstol=0.0, reltol=None, stats=None):
    """Returns (x, hist, iters): hist[0] = |Pl \\ b|, then the residual estimate after each Arnoldi step.
    stats: an optional dict that receives {"reorth": extra DGKS passes, "restarts": restarts}."""
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    restart = min(20, n) if restart is None else int(restart)
    maxiter = n if maxiter is None else int(maxiter)
    reltol = float(np.sqrt(np.finfo(np.float64).eps)) if reltol is None else float(reltol)
    if restart < 1 or restart > 64 or maxiter < 0:
        raise ValueError("restart in [1, 64], maxiter >= 0")
    x = np.zeros(n)
    V = np.zeros((n, restart + 1), order="F")
    H = np.zeros((restart + 1, restart))
    reorth = restarts = 0

    def start(r):
        v = Pl(r)
        beta = float(np.linalg.norm(v))
        V[:, 0] = v * (1.0 / beta if beta != 0.0 else 0.0)
        nullvec = np.zeros(restart + 1)
        nullvec[0] = 1.0
        return beta, nullvec, 1.0

    beta, nullvec, acc = start(b)
    tol = max(reltol * beta, abstol)
    hist = [beta]
    current = beta
    it = k = 0
    while it < maxiter and current > tol:
        w = Pl(A @ V[:, k])
        h = V[:, :k + 1].T @ w
        w = w - V[:, :k + 1] @ h
        nrm, proj = float(np.linalg.norm(w)), float(np.linalg.norm(h))
        extra = 0
        while extra < MAX_EXTRA and nrm < proj / np.sqrt(2.0):
            c = V[:, :k + 1].T @ w
            proj = float(np.linalg.norm(c))
            w = w - V[:, :k + 1] @ c
            h = h + c
            nrm = float(np.linalg.norm(w))
            extra += 1
        reorth += extra
        H[:k + 1, k] = h
        H[k + 1, k] = nrm
        if nrm == 0.0:   # lucky breakdown: the Krylov space is invariant, the residual of the least squares is 0
            current = 0.0
        else:
            V[:, k + 1] = w * (1.0 / nrm)
            nu = -float(np.dot(nullvec[:k + 1], H[:k + 1, k])) / nrm
            nullvec[k + 1] = nu
            acc += nu * nu
            current = beta / np.sqrt(acc)
        it += 1
        k += 1
        hist.append(current)
        done = it >= maxiter or current <= tol
        if k == restart or done:
            x = x + V[:, :k] @ _lsq(H, beta, k)
            k = 0
            if not done:
                restarts += 1
                beta, nullvec, acc = start(b - A @ x)
                current = beta
    if stats is not None:
        stats.update(reorth=reorth, restarts=restarts)
    return x, np.array(hist), it


def dense_inverse(A):
    """Pl = A^-1 as a callable (exact preconditioner)."""
    Ainv = np.linalg.inv(np.asarray(A.todense() if hasattr(A, "todense") else A))
    return lambda r: Ainv @ r
