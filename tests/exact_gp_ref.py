"""Numpy float64 restatement of exact GP regression by conjugate gradients (henbun_amd/gp/exact.py, hb_gram_matvec,
hb_pcg_*): the chunked matrix-free product, the pivoted incomplete Cholesky preconditioner and its Woodbury inverse,
lockstep preconditioned CG, and the coefficients of the exact pathwise draws.

    K^ = k_var K(X, X) + noise_var I,   P = k_var C^T C + noise_var I,   C [R, N] from greedy_ref.select at threshold 0
    P^-1 r = (r - k_var C^T (noise_var I + k_var C C^T)^-1 C r) / noise_var
    v_s = sqrt(k_var) K^^-1 (y - sqrt(k_var) g_s(X) - sqrt(noise_var) eps_s),  coef_s = [ w_s / sqrt(L) | v_s ]
"""
import numpy as np

import greedy_ref as GR
import pathwise_ref as PR


def rbf(x2, x, ell):
    """K(x2, x) [N, n]: the difference first, scaled afterwards, as the strip kernels form it."""
    ell = np.reshape(np.asarray(ell, dtype=np.float64), [-1])
    r2 = np.zeros((x2.shape[0], x.shape[0]))
    for k in range(x.shape[1]):
        t = (x2[:, k, None] - x[None, :, k]) / ell[0 if ell.size == 1 else k]
        r2 += t * t
    return np.exp(-0.5 * r2)


def matvec(x, x2, ell, V, scale=1.0, shift=0.0, chunk=2048):
    """out [S, n] = scale sum_i V[s, i] k(x2_i, x_j) + shift V[s, j]: one partial per chunk of rows, the partials added in
    chunk order, then scale and shift.  x2 None: the symmetric form."""
    x, V = np.asarray(x, np.float64), np.asarray(V, np.float64)
    x2 = x if x2 is None else np.asarray(x2, np.float64)
    assert shift == 0.0 or x2 is x
    N = x2.shape[0]
    total = np.zeros((V.shape[0], x.shape[0]))
    for i0 in range(0, N, chunk):
        total = total + V[:, i0:i0 + chunk] @ rbf(x2[i0:i0 + chunk], x, ell)
    return scale * total + (shift * V if shift != 0.0 else 0.0)


def matvec_magnitude(x, x2, ell, V):
    """(sum_i |V_si| [S, 1], sum_i |V_si| K_ij [S, n]): what the bounds of the product are stated in."""
    x, V = np.asarray(x, np.float64), np.abs(np.asarray(V, np.float64))
    x2 = x if x2 is None else np.asarray(x2, np.float64)
    K = rbf(x2, x, ell)
    return V.sum(1, keepdims=True), V @ K


def factor(X, ell, rank):
    """C [count, N]: the rows greedy_ref.select produces at threshold 0 (a pivoted incomplete Cholesky of K(X, X))."""
    X = np.asarray(X, np.float64)
    ell = np.reshape(np.asarray(ell, np.float64), [-1])
    N = X.shape[0]
    C, dvar = np.zeros((rank, N)), np.ones(N)
    count = rank
    for j in range(rank):
        i = int(np.argmax(dvar))
        if dvar[i] <= 0.0:
            count = j
            break
        GR._step(X, ell, C, dvar, j, i, "forward")
    return C[:count]


def precond_apply(C, k_var, noise_var, r):
    """P^-1 r for the rows of r [S, N] by Woodbury; C None or empty: r itself (plain CG)."""
    if C is None or C.shape[0] == 0:
        return r.copy()
    G = noise_var * np.eye(C.shape[0]) + k_var * C @ C.T
    L = np.linalg.cholesky(G)
    t = np.linalg.solve(L.T, np.linalg.solve(L, C @ r.T))
    return (r - k_var * (C.T @ t).T) / noise_var


def pcg(X, ell, k_var, noise_var, B, C=None, tol=1e-6, max_iter=1000, chunk=2048):
    """Lockstep preconditioned CG on the rows of B [S, N] -> (x, info): every row its own alpha, beta; a row with
    |r| <= tol |b| stops moving; info = dict(iterations, residual [S] = |b - K^ x| / |b|, converged).  (In float64 the
    recurrence's residual is the true one to rounding: the restart pcg_solve makes when they part is not restated.)"""
    B = np.asarray(B, np.float64)
    A = lambda V: matvec(X, None, ell, V, k_var, noise_var, chunk)
    x, r = np.zeros_like(B), B.copy()
    bb = (B * B).sum(1)
    thr = tol * tol * bb
    rr = bb.copy()
    z = precond_apply(C, k_var, noise_var, r)
    p, rz = z.copy(), (r * z).sum(1)
    it = 0
    while it < max_iter and not np.all(rr <= thr):
        act = rr > thr
        Ap = A(p)
        pAp = (p * Ap).sum(1)
        alpha = np.where(act & (pAp > 0), rz / np.where(pAp > 0, pAp, 1.0), 0.0)
        x += alpha[:, None] * p
        r -= alpha[:, None] * Ap
        rr = np.where(act, (r * r).sum(1), rr)
        it += 1
        z = precond_apply(C, k_var, noise_var, r)
        rzn = (r * z).sum(1)
        beta = np.where(rz > 0, rzn / np.where(rz > 0, rz, 1.0), 0.0)
        upd = rr > thr
        p = np.where(upd[:, None], z + beta[:, None] * p, p)
        rz = np.where(upd, rzn, rz)
    res = np.sqrt(((B - A(x)) ** 2).sum(1) / np.where(bb > 0, bb, 1.0))
    return x, dict(iterations=it, residual=res, converged=bool(np.all(rr <= thr)))


def dense(X, ell, k_var, noise_var):
    """K^ [N, N]."""
    X = np.asarray(X, np.float64)
    return k_var * rbf(X, X, ell) + noise_var * np.eye(X.shape[0])


def posterior(X, Y, ell, k_var, noise_var, Xnew):
    """(alpha [P, N], mean [P, n], var [n]) from the dense Cholesky."""
    from scipy.linalg import cho_factor, cho_solve

    cf = cho_factor(dense(X, ell, k_var, noise_var), lower=True)
    alpha = cho_solve(cf, np.asarray(Y, np.float64)).T
    ks = k_var * rbf(np.asarray(X, np.float64), np.asarray(Xnew, np.float64), ell)          # [N, n]
    return alpha, alpha @ ks, k_var - (ks * cho_solve(cf, ks)).sum(0)


def pathwise_coefficients(X, y, ell, k_var, noise_var, omega, w, eps, solve):
    """coef [S, 2L + N] = [ w / sqrt(L) | v ]; `solve(B)` returns K^^-1 applied to the rows of B [S, N]."""
    X, y, omega, w, eps = (np.asarray(a, np.float64) for a in (X, y, omega, w, eps))
    cw = w / np.sqrt(omega.shape[0])
    prior = np.sqrt(k_var) * PR.evaluate(X, omega, None, np.reshape(np.asarray(ell, np.float64), [-1]), cw)    # [S, N]
    v = np.sqrt(k_var) * solve(y.reshape(1, -1) - prior - np.sqrt(noise_var) * eps)
    return np.concatenate([cw, v], axis=1)


def plane_case(N=600):
    """The case the preconditioner's effect was measured on: X ~ U(0, 5)^2, Y = sin(sum x) + 0.1 noise, ell 0.5,
    noise_var 0.01, k_var 1 -> (X, Y [N, 1], ell, k_var, noise_var)."""
    rng = np.random.default_rng(0)
    X = rng.uniform(0.0, 5.0, (N, 2))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    return X, Y, np.array([0.5]), 1.0, 0.01


def pcg_update(x, r, p, Ap, rz, rr, thr):
    """One hb_pcg_update on copies: rows with rr > thr get alpha = rz / (p . Ap), x += alpha p, r -= alpha Ap,
    rr = |r|^2; the others are untouched -> (x, r, rr)."""
    x, r, rr = x.copy(), r.copy(), rr.copy()
    for s in np.nonzero(rr > thr)[0]:
        pAp = p[s] @ Ap[s]
        alpha = rz[s] / pAp if pAp > 0 else 0.0
        x[s] += alpha * p[s]
        r[s] -= alpha * Ap[s]
        rr[s] = r[s] @ r[s]
    return x, r, rr


def pcg_direction(r, w, p, rz, rr, thr, wscale, zscale, first):
    """One hb_pcg_direction on copies: rows with rr > thr get z = (r - wscale w) zscale (w None: r),
    beta = (r . z) / rz (first: 0), p = z + beta p, rz = r . z -> (p, rz)."""
    p, rz = p.copy(), rz.copy()
    for s in np.nonzero(rr > thr)[0]:
        z = r[s] if w is None else (r[s] - wscale * w[s]) * zscale
        rzn = r[s] @ z
        beta = 0.0 if first or not rz[s] > 0 else rzn / rz[s]
        p[s] = z + beta * (0.0 if first else p[s])
        rz[s] = rzn
    return p, rz
