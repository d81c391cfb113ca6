"""Numpy float64 restatement of the exact GP's cached predictive variance (henbun_amd/gp/exact.py: VarianceCache;
hb_gram_predict).  With K^ = k_var K(X, X) + noise_var I and a full-row-rank basis C [r, N]:

    C: the rows of the pivoted incomplete Cholesky of K(X, X) (greedy_ref's steps, stopped at `threshold`), each scaled
       to unit norm -- or any basis handed in;
    T = C K^ C^T, symmetrised, + eps tr(T) / r I with eps = 1e-13, times 100 after a failed factorisation, three times
       at most;  T = L L^T;  R_c = L^-1 C;
    v_cache(x) = k_var - |R_c k*|^2,  k* = k_var K(X, x)   >=   v_exact(x) = k_var - k*^T K^^-1 k*.

The bound: G = C^T (C K^ C^T)^-1 C is K^^-1/2 Pi K^^-1/2 with Pi the orthogonal projector onto the range of K^^1/2 C^T,
so G <= K^^-1; jitter makes G smaller still.  The acquisition tails are those of tests/acq_ref.py."""
import numpy as np

import acq_ref as AR
import exact_gp_ref as E
import greedy_ref as GR

JITTER, TRIES = 1e-13, 3


def basis(X, ell, rank, threshold=0.0, dtype=np.float32):
    """C [count, N] float64: the rows greedy selection produces in `dtype` arithmetic before the largest conditional
    variance falls to `threshold` or below (count <= rank), as they are (not yet unit rows)."""
    X, ell = GR._cast(X, ell, dtype)
    N = X.shape[0]
    rank = min(int(rank), N)
    C, dvar = np.zeros((rank, N), dtype=dtype), np.ones(N, dtype=dtype)
    count = rank
    for j in range(rank):
        i = int(np.argmax(dvar))
        if float(dvar[i]) <= threshold:
            count = j
            break
        GR._step(X, ell, C, dvar, j, i, "forward")
    return C[:count].astype(np.float64)


def build(X, ell, k_var, noise_var, rank=None, threshold=0.0, C=None, select_dtype=np.float32, rc_dtype=None):
    """dict(C [r, N] unit rows, Rc [r, N], rank, jitter, trace, cond) from the selection at `rank`, or from a given
    basis C (any full-row-rank matrix).  rc_dtype: R_c rounded once to that type, as the device holds it."""
    X = np.asarray(X, np.float64)
    if C is None:
        C = basis(X, ell, rank, threshold, select_dtype)
    C = np.asarray(C, np.float64)
    C = C / np.sqrt((C * C).sum(1, keepdims=True))
    r = C.shape[0]
    T = (E.dense(X, ell, k_var, noise_var) @ C.T).T @ C.T
    T = 0.5 * (T + T.T)
    trace, eps = float(np.trace(T)), JITTER
    for attempt in range(TRIES + 1):
        try:
            L = np.linalg.cholesky(T + eps * trace / r * np.eye(r))
            break
        except np.linalg.LinAlgError:
            if attempt == TRIES:
                raise
            eps *= 100.0
    from scipy.linalg import solve_triangular

    Rc = solve_triangular(L, C, lower=True)
    if rc_dtype is not None:
        Rc = Rc.astype(rc_dtype).astype(np.float64)
    return dict(C=C, Rc=Rc, rank=r, jitter=eps, trace=trace, cond=float(np.linalg.cond(T)))


def products(cache, X, ell, k_var, Xnew):
    """t [r, n] = R_c k*, the cache rows of the product."""
    return cache["Rc"] @ (k_var * E.rbf(np.asarray(X, np.float64), np.asarray(Xnew, np.float64), ell))


def v_cache(cache, X, ell, k_var, Xnew):
    """k_var - |R_c k*|^2 [n], not clamped."""
    t = products(cache, X, ell, k_var, Xnew)
    return k_var - (t * t).sum(0)


def v_exact(X, ell, k_var, noise_var, Xnew):
    """The exact predictive variance [n] from the dense Cholesky (it does not depend on Y)."""
    return E.posterior(X, np.zeros((np.shape(X)[0], 1)), ell, k_var, noise_var, Xnew)[2]


def acquisition(kind, mean, var, best=0.0, param=0.0, largest=True, var_floor=0.0):
    """The tail of acq_ref at (mean, var) in data units (scale 1)."""
    return AR.tail(kind, mean, var, best, param, 1.0, largest, var_floor)[0]


def square_case(N, side, noise_var=0.09, k_var=1.0, ell=1.0, n_test=256, seed=0):
    """(X [N, 2] ~ U(0, side)^2, ell [1], k_var, noise_var, Xnew [n_test, 2] ~ U(-0.2 side, 1.2 side)^2: some outside the
    data).  N = 48, side 2 and N = 600, side 5 are the cases the bound was first measured on."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, side, (N, 2))
    Xnew = rng.uniform(-0.2 * side, 1.2 * side, (n_test, 2))
    return X, np.array([ell]), k_var, noise_var, Xnew
