"""Numpy restatement of greedy conditional-variance selection of inducing points (hb_sgp_select; Burt, Rasmussen, van der
Wilk 2020): a pivoted incomplete Cholesky of K(X, X) for the UnitRBF kernel k = exp(-0.5 sum_d ((x_d - x'_d) / ell_d)^2).

State: dvar [N] = kdiag = 1, history C [M, N].  For j = 0 .. M - 1:
    i_j = argmax_i dvar_i (exact ties: the lowest index);  stop if dvar_{i_j} <= threshold (count = j);
    pivots_j = dvar_{i_j};  C[j, i] = (k(x_i, x_{i_j}) - sum_{t < j} C[t, i] C[t, i_j]) / sqrt(pivots_j);
    dvar_i <- max(dvar_i - C[j, i]^2, 0);  dvar_{i_j} <- 0.
trace = sum_i dvar_i at the end.

`select` chooses; `replay` does NOT choose: it follows a given index sequence and reports, per step, the pivot (the dvar of
the given index) and the largest dvar there was to choose from -- the GPU tests replay the device's own choice, because
float32 and float64 selections part ways within the first steps on nearly tied conditional variances."""
import numpy as np


def kcol(X, i, ell):
    """k(x_., x_i) [N] in the dtype of X, term by term as csrc/gram_value.cuh forms it."""
    il = (1.0 / ell).astype(X.dtype)
    r2 = np.zeros(X.shape[0], dtype=X.dtype)
    for k in range(X.shape[1]):
        s = il[0] if ell.size == 1 else il[k]
        a, b = X[:, k] * s, X[i, k] * s
        r2 += (a - b) * (a - b)
    return np.exp(X.dtype.type(-0.5) * r2)


def _step(X, ell, C, dvar, j, i, order):
    """Row j of the factor for pivot i (the sum over t one term at a time, forward or reversed), dvar downdated in place."""
    acc = np.zeros(X.shape[0], dtype=X.dtype)
    ts = range(j) if order == "forward" else range(j - 1, -1, -1)
    for t in ts:
        acc += C[t] * C[t, i]
    C[j] = (kcol(X, i, ell) - acc) / np.sqrt(dvar[i])
    np.maximum(dvar - C[j] * C[j], 0, out=dvar)
    dvar[i] = 0


def _cast(X, ell, dtype):
    X = np.ascontiguousarray(np.asarray(X, dtype=dtype))
    return X, np.reshape(np.asarray(ell, dtype=dtype), [-1])


def select(X, M, ell, threshold=0.0, dtype=np.float64):
    """(idx int64 [M], pivots [M], count, trace): entries from count on are -1 / 0.  All arithmetic in `dtype`; the trace
    is summed in float64."""
    X, ell = _cast(X, ell, dtype)
    N = X.shape[0]
    C = np.zeros((M, N), dtype=dtype)
    dvar = np.ones(N, dtype=dtype)
    idx, pivots, count = -np.ones(M, dtype=np.int64), np.zeros(M, dtype=dtype), M
    for j in range(M):
        i = int(np.argmax(dvar))                 # numpy's argmax returns the first of equal maxima
        if float(dvar[i]) <= threshold:
            count = j
            break
        idx[j], pivots[j] = i, dvar[i]
        _step(X, ell, C, dvar, j, i, "forward")
    return idx, pivots, count, float(dvar.astype(np.float64).sum())


def replay(X, idx, ell, order="forward", dtype=np.float64):
    """Follow idx [m]: (pivots [m], dmax [m], trace) -- pivots_j = dvar[idx_j] and dmax_j = max_i dvar_i BEFORE step j,
    trace = sum dvar after the last step.  float64 unless a dtype is asked for; `order` ('forward' / 'reversed') is the
    order of the sum over t: the spread between the two is the restatement's own sensitivity to rounding."""
    assert order in ("forward", "reversed")
    X, ell = _cast(X, ell, dtype)
    idx = np.asarray(idx, dtype=np.int64)
    m, N = idx.shape[0], X.shape[0]
    C = np.zeros((m, N), dtype=dtype)
    dvar = np.ones(N, dtype=dtype)
    pivots, dmax = np.zeros(m), np.zeros(m)
    for j in range(m):
        i = int(idx[j])
        pivots[j], dmax[j] = dvar[i], dvar.max()
        _step(X, ell, C, dvar, j, i, order)
    return pivots, dmax, float(dvar.astype(np.float64).sum())


def tolerance(X, idx, ell, dtype, multiple=4.0):
    """(tol, deviation, floor, forward replay): tol = multiple x max(deviation, floor); deviation = the largest pivot
    difference between the dtype restatement following idx and the float64 replay (0 for float64); floor = the largest
    pivot difference between the forward and the reversed float64 replays."""
    fwd = replay(X, idx, ell, "forward")
    rev = replay(X, idx, ell, "reversed")
    floor = float(np.abs(fwd[0] - rev[0]).max())
    dev = 0.0
    if np.dtype(dtype) != np.float64:
        # the float64 replay runs on the SAME (already rounded) inputs the dtype restatement sees
        Xr, ellr = _cast(X, ell, dtype)
        q = replay(Xr, idx, ellr, "forward", dtype=dtype)
        r = replay(Xr.astype(np.float64), idx, ellr.astype(np.float64), "forward")
        dev = float(np.abs(q[0] - r[0]).max())
    return multiple * max(dev, floor), dev, floor, fwd


def clustered(N=4096, dom=32.0, d=1, seed=1):
    """The 12-cluster set: centres uniform on [0, dom]^d, points 0.08 dom around them; Y = sin(x_0) + 0.3 noise."""
    rng = np.random.RandomState(seed)
    cent = rng.uniform(0, dom, (12, d))
    X = cent[rng.randint(0, 12, N)] + 0.08 * dom * rng.randn(N, d)
    Y = np.sin(X[:, :1]) + 0.3 * rng.randn(N, 1)
    return X, Y
