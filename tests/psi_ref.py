"""Numpy float64 restatement of the psi statistics of the unit RBF kernel under Gaussian inputs x ~ N(mu, diag(s)), s >= 0
(Titsias & Lawrence 2010), written from the formulas:

    psi1(m)     = prod_k (1 + s_k / l_k^2)^-1/2   exp(-1/2 sum_k (mu_k - z_mk)^2 / (l_k^2 + s_k))
    psi2(m, m') = prod_k (1 + 2 s_k / l_k^2)^-1/2 exp(-sum_k [(z_mk - z_m'k)^2 / (4 l_k^2) + (mu_k - zbar_k)^2 / (l_k^2 + 2 s_k)])
    zbar = (z_m + z_m') / 2

(the midpoint form; the device kernels evaluate the equivalent form without the midpoint), the statistics of a data set

    Psi2 = sum_n psi2_n [M, M],   C[p, m] = sum_n psi1_n(m) Y_np,   yy_p = sum_n Y_np^2,
    Phi = W Psi2 W^T,   b_p = W C_p,   a2sum = tr Phi            (the tuple of SparseGP.statistics)

and the predictive moments at a Gaussian test input under q(u) = N(m, S S^T):

    beta = W^T m,   Q = W^T (rho I - S S^T) W - beta beta^T,   rho = 1 ('diagonal') or 0 ('neglected')
    mean = sqrt(k_var) beta^T psi1,   var = k_var (rho - sum Q psi2 - (beta^T psi1)^2).

tests/test_psi_cpu.py pins all of it against tensor Gauss-Hermite quadrature."""
import numpy as np

import optimal_q_ref as R


def _ell(ell, d):
    return np.broadcast_to(np.asarray(ell, np.float64).reshape(-1), (d,))


def psi1(mu, s, z, ell):
    """[N, M]"""
    mu, s, z = (np.asarray(a, np.float64) for a in (mu, s, z))
    l2 = _ell(ell, z.shape[1]) ** 2
    e = np.zeros((mu.shape[0], z.shape[0]))
    for k in range(z.shape[1]):
        e += (mu[:, k, None] - z[None, :, k]) ** 2 / (l2[k] + s[:, k, None])
    return np.prod(1.0 + s / l2, axis=1)[:, None] ** -0.5 * np.exp(-0.5 * e)


def psi2_pairs(mu, s, z, ell, im, iq):
    """psi2_n(z[im], z[iq]) for index arrays im, iq [L]: [N, L]"""
    mu, s, z = (np.asarray(a, np.float64) for a in (mu, s, z))
    l2 = _ell(ell, z.shape[1]) ** 2
    e = np.zeros((mu.shape[0], len(im)))
    for k in range(z.shape[1]):
        zm, zq = z[im, k], z[iq, k]
        e += ((zm - zq) ** 2 / (4.0 * l2[k]))[None, :]
        e += (mu[:, k, None] - 0.5 * (zm + zq)[None, :]) ** 2 / (l2[k] + 2.0 * s[:, k, None])
    return np.prod(1.0 + 2.0 * s / l2, axis=1)[:, None] ** -0.5 * np.exp(-e)


def psi2(mu, s, z, ell):
    """[N, M, M] (small problems only)"""
    M = z.shape[0]
    im, iq = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    return psi2_pairs(mu, s, z, ell, im.reshape(-1), iq.reshape(-1)).reshape(-1, M, M)


def stats_raw(mu, s, Y, z, ell, chunk=None):
    """(Psi2 [M, M], C [P, M], yy [P]): the lower triangle summed over the points in chunks and mirrored."""
    mu, s, Y, z = (np.asarray(a, np.float64) for a in (mu, s, Y, z))
    N, M = mu.shape[0], z.shape[0]
    im, iq = np.tril_indices(M)
    chunk = chunk or max(1, (1 << 21) // len(im))
    low = np.zeros(len(im))
    for n0 in range(0, N, chunk):
        low += psi2_pairs(mu[n0:n0 + chunk], s[n0:n0 + chunk], z, ell, im, iq).sum(0)
    Psi2 = np.zeros((M, M))
    Psi2[im, iq] = low
    Psi2[iq, im] = low
    return Psi2, (psi1(mu, s, z, ell).T @ Y).T, (Y ** 2).sum(0)


def whiten(Psi2, C, yy, W):
    """(Phi, b, yy, a2sum) from the raw statistics and W = chol(K(z, z) + jitter I)^-1"""
    W = np.asarray(W, np.float64)
    Phi = W @ Psi2 @ W.T
    Phi = 0.5 * (Phi + Phi.T)
    return Phi, C @ W.T, yy, float(np.trace(Phi))


def stats(mu, s, Y, z, ell, jitter=None, W=None):
    if W is None:
        _, W = R.chol_factor(np.asarray(z, np.float64), np.asarray(ell, np.float64).reshape(-1), jitter)
    return whiten(*stats_raw(mu, s, Y, z, ell), W)


def predict_terms(m, S, W, residual="diagonal"):
    """(beta [M], Q [M, M], rho) for q(u) = N(m, S S^T); S [M, M] or the standard deviations s [M]"""
    W = np.asarray(W, np.float64)
    m = np.asarray(m, np.float64).reshape(-1)
    S = np.asarray(S, np.float64)
    SS = np.diag(S ** 2) if S.ndim == 1 else S @ S.T
    rho = 1.0 if residual == "diagonal" else 0.0
    beta = W.T @ m
    return beta, W.T @ (rho * np.eye(len(m)) - SS) @ W - np.outer(beta, beta), rho


def contractions(mu, s, z, ell, beta, Q):
    """(e1 [n], e2 [n]): sum_m beta_m psi1(m) and sum_mm' Q_mm' psi2(m, m') per point, Q symmetric"""
    M = z.shape[0]
    im, iq = np.tril_indices(M)
    w = np.where(im == iq, 1.0, 2.0) * (0.5 * (Q + Q.T))[im, iq]
    return psi1(mu, s, z, ell) @ beta, psi2_pairs(mu, s, z, ell, im, iq) @ w


def predict_uncertain(mu, s, z, ell, W, m, S, k_var=1.0, residual="diagonal"):
    """(mean [n], var [n]) of f at x* ~ N(mu, diag(s))"""
    beta, Q, rho = predict_terms(m, S, W, residual)
    e1, e2 = contractions(mu, s, z, ell, beta, Q)
    return np.sqrt(k_var) * e1, k_var * (rho - e2 - e1 * e1)


def elbo_direct(m, S, mu, s, Y, z, ell, W, noise_var, k_var=1.0, residual="diagonal"):
    """E_q(u) E_x [log p(Y | f)] - KL(q || N(0, I)) for q(u_p) = N(m_p, S S^T) and x_n ~ N(mu_n, diag(s_n)), term by term
    from the per-point psi1_n, psi2_n (no shortcut through Lambda, nor through the summed statistics):
    E (y - f)^2 = y^2 - 2 y sqrt(k) m^T W psi1 + k [m^T W psi2 W^T m + tr(S^T W psi2 W^T S) + rho (1 - tr(W psi2 W^T))]."""
    P, M = m.shape
    W = np.asarray(W, np.float64)
    rho = 1.0 if residual == "diagonal" else 0.0
    p1 = psi1(mu, s, z, ell) @ W.T                                       # [N, M]: W psi1_n
    p2 = np.einsum("im,nmq,jq->nij", W, psi2(mu, s, z, ell), W)          # [N, M, M]: W psi2_n W^T
    SS = S @ S.T
    val = 0.0
    for p in range(P):
        quad = np.einsum("i,nij,j->n", m[p], p2, m[p]) + np.einsum("ij,nij->n", SS, p2) + rho * (1.0 - np.trace(p2, axis1=1, axis2=2))
        err2 = Y[:, p] ** 2 - 2.0 * Y[:, p] * np.sqrt(k_var) * (p1 @ m[p]) + k_var * quad
        val += np.sum(-0.5 * np.log(2 * np.pi * noise_var) - err2 / (2 * noise_var))
        val -= 0.5 * (np.trace(SS) + m[p] @ m[p] - M - np.linalg.slogdet(SS)[1])
    return float(val)


def gauss_hermite_expect(fn, mu, s, nodes=60):
    """E fn(x) for x ~ N(mu, diag(s)), mu, s [d] with d <= 2, by the tensor Gauss-Hermite rule; fn maps [K, d] points to
    [K, ...] values.  A zero variance collapses its axis onto the mean, exactly."""
    t, w = np.polynomial.hermite.hermgauss(nodes)
    d = len(mu)
    grids = np.meshgrid(*([t] * d), indexing="ij")
    wts = np.ones_like(grids[0])
    for k in range(d):
        wts = wts * w.reshape([-1 if a == k else 1 for a in range(d)])
    pts = np.stack([mu[k] + np.sqrt(2.0 * s[k]) * grids[k].reshape(-1) for k in range(d)], 1)
    vals = fn(pts)
    return np.tensordot(wts.reshape(-1), vals, axes=(0, 0)) / np.pi ** (0.5 * d)
