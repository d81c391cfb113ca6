"""Numpy float64 restatement of the gradient of the collapsed bound (SparseGP.collapsed_bound_and_grad), on top of
optimal_q_ref.py and in its notation:

    K = K(z, X) [M, N],  Kmm = K(z, z) + jitter I = L L^T,  W = L^-1,  A = W K,  Phi = A A^T,  b = (A Y)^T [P, M],
    Lambda = I + (k / s2) Phi,  c = sqrt(k) b / s2,  m = c Lambda^-1 [P, M],  F = collapsed_bound,
    rho = 1 for residual 'diagonal', 0 for 'neglected'.

1. tail (from Phi and b only):   D = dF/dLambda = -1/2 m^T m - (P / 2) Lambda^-1,
                                 G = dF/dPhi = (k / s2) D + rho P k / (2 s2) I,     g = dF/db = (sqrt(k) / s2) m
2. weights of the streamed part: Q = 2 W^T G W [M, M],  R = W^T g^T [M, P]
3. streamed part:                Kbar = Q K + R Y^T,  E = Kbar o K,
                                 zbar_id = -sum_j E_ij (z_id - x_jd) / ell_d^2,  ellbar_d = sum_ij E_ij (z_id - x_jd)^2 / ell_d^3
4. Kmm part (K K^T = L Phi L^T and K Y = L b^T, so no second pass over the data):
                                 L^T Lbar = T = -(2 G Phi + g^T b),  Pm = tril(T) with the diagonal halved,
                                 S = W^T Pm W,  Kmmbar = (S + S^T) / 2,  then the VJP of K(z, z) (both arguments are z)
5. scalars, tau = sum(D o Phi):  dF/dk  = tau / s2 + sum(m o b) / (2 sqrt(k) s2) - rho P (N - tr Phi) / (2 s2)
                                 dF/ds2 = -N P / (2 s2) + sum(yy) / (2 s2^2) - (k / s2^2) tau - sum(m o c) / s2
                                          + rho P k (N - tr Phi) / (2 s2^2)

The streamed and the Kmm parts of zbar / ellbar are returned separately as well as summed: their difference is about
1000 times smaller than either (tests/test_collapsed_grad_cpu.py prints the figures)."""
import numpy as np

import optimal_q_ref as R


def tail(Phi, b, yy, N, noise_var, k_var=1.0, residual="diagonal"):
    """(F, D, G, g, m, c, tau) from the statistics alone."""
    P, M = b.shape
    rho = 1.0 if residual == "diagonal" else 0.0
    k, s2 = float(k_var), float(noise_var)
    Lam = np.eye(M) + (k / s2) * Phi
    c = np.sqrt(k) * b / s2
    Lami = np.linalg.inv(Lam)
    Lami = 0.5 * (Lami + Lami.T)
    m = np.linalg.solve(Lam, c.T).T
    D = -0.5 * m.T @ m - 0.5 * P * Lami
    G = (k / s2) * D + rho * P * k / (2.0 * s2) * np.eye(M)
    g = (np.sqrt(k) / s2) * m
    F = R.collapsed_bound(Phi, b, yy, float(np.trace(Phi)), N, s2, k, residual)
    return F, D, G, g, m, c, float(np.sum(D * Phi))


def weights(W, G, g):
    """(Q [M, M], R [M, P]) of the streamed part."""
    return 2.0 * W.T @ G @ W, W.T @ g.T


def streamed(X, Y, z, ell, Q, Rw):
    """(zbar [M, d], ellbar [dl]) of the streamed part for given weights: the semantics of hb_sgp_kgrad."""
    X, Y, z, ell = (np.asarray(a, np.float64) for a in (X, Y, z, ell))
    K = R.rbf(z, X, ell)
    E = (Q @ K + Rw @ Y.T) * K
    d = z.shape[1]
    l = np.broadcast_to(ell, (d,))
    zbar = np.zeros_like(z)
    ellbar = np.zeros(d)
    for k in range(d):
        diff = z[:, k, None] - X[None, :, k]
        zbar[:, k] = -(E * diff).sum(1) / l[k] ** 2
        ellbar[k] = (E * diff * diff).sum() / l[k] ** 3
    return zbar, (ellbar if ell.shape[0] == d else ellbar.sum(keepdims=True))


def kmm_part(z, ell, W, G, g, Phi, b):
    """(zbar [M, d], ellbar [dl]) through Kmm = K(z, z) + jitter I (the jitter has no gradient)."""
    z, ell = np.asarray(z, np.float64), np.asarray(ell, np.float64)
    T = -(2.0 * G @ Phi + g.T @ b)
    Pm = np.tril(T)
    Pm[np.diag_indices_from(Pm)] *= 0.5
    S = W.T @ Pm @ W
    Kbar = 0.5 * (S + S.T)
    E = Kbar * R.rbf(z, z, ell)
    d = z.shape[1]
    l = np.broadcast_to(ell, (d,))
    zbar = np.zeros_like(z)
    ellbar = np.zeros(d)
    for k in range(d):
        diff = z[:, k, None] - z[None, :, k]
        zbar[:, k] = -((E + E.T) * diff).sum(1) / l[k] ** 2
        ellbar[k] = (E * diff * diff).sum() / l[k] ** 3
    return zbar, (ellbar if ell.shape[0] == d else ellbar.sum(keepdims=True))


def bound_and_grad(X, Y, z, ell, jitter, noise_var, k_var=1.0, residual="diagonal"):
    """dict(value, z, lengthscales, noise_var, k_var, z_streamed, z_kmm, ell_streamed, ell_kmm, Q, R, ..): the bound and
    its gradient with respect to z [M, d], ell [dl], noise_var and k_var."""
    X, Y, z, ell = (np.asarray(a, np.float64) for a in (X, Y, z, ell))
    N, P = X.shape[0], Y.shape[1]
    k, s2 = float(k_var), float(noise_var)
    rho = 1.0 if residual == "diagonal" else 0.0
    _, W = R.chol_factor(z, ell, jitter)
    Phi, b, yy, a2sum = R.stats_from_W(X, Y, z, ell, W)
    F, D, G, g, m, c, tau = tail(Phi, b, yy, N, s2, k, residual)
    Q, Rw = weights(W, G, g)
    zs, es = streamed(X, Y, z, ell, Q, Rw)
    zk, ek = kmm_part(z, ell, W, G, g, Phi, b)
    dk = tau / s2 + np.sum(m * b) / (2.0 * np.sqrt(k) * s2) - rho * P * (N - a2sum) / (2.0 * s2)
    ds2 = (-N * P / (2.0 * s2) + yy.sum() / (2.0 * s2 ** 2) - (k / s2 ** 2) * tau - np.sum(m * c) / s2
           + rho * P * k * (N - a2sum) / (2.0 * s2 ** 2))
    # the sums of the absolute terms of the two scalars: what their rounding error scales with
    dk_abs = abs(tau / s2) + abs(np.sum(m * b) / (2.0 * np.sqrt(k) * s2)) + rho * P * abs(N - a2sum) / (2.0 * s2)
    ds2_abs = (N * P / (2.0 * s2) + yy.sum() / (2.0 * s2 ** 2) + abs((k / s2 ** 2) * tau) + abs(np.sum(m * c) / s2)
               + rho * P * k * abs(N - a2sum) / (2.0 * s2 ** 2))
    return dict(value=F, z=zs + zk, lengthscales=es + ek, noise_var=float(ds2), k_var=float(dk),
                z_streamed=zs, z_kmm=zk, ell_streamed=es, ell_kmm=ek, Q=Q, R=Rw, W=W, Phi=Phi, b=b,
                noise_var_abs=float(ds2_abs), k_var_abs=float(dk_abs))


def bound_autograd(X, Y, z, ell, jitter, noise_var, k_var=1.0, residual="diagonal"):
    """The same five numbers from torch.autograd in float64 on optimal_q_ref's bound written in torch ops: an independent
    evaluation (no formula of this file is used).  Returns dict(value, z, lengthscales, noise_var, k_var)."""
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    X, Y = t(X), t(Y)
    z, ell = t(z).requires_grad_(True), t(ell).requires_grad_(True)
    s2, k = t(noise_var).requires_grad_(True), t(k_var).requires_grad_(True)
    N, P = X.shape[0], Y.shape[1]
    M = z.shape[0]

    def rbf(a, c):
        a_, c_ = a / ell, c / ell
        r2 = 0.0
        for k_ in range(a.shape[1]):   # one [M, N] term per dimension: no [M, N, d] intermediate
            r2 = r2 + (a_[:, k_, None] - c_[None, :, k_]) ** 2
        return torch.exp(-0.5 * r2)

    L = torch.linalg.cholesky(rbf(z, z) + jitter * torch.eye(M, dtype=torch.float64))
    A = torch.linalg.solve_triangular(L, rbf(z, X), upper=False)
    Phi, b, yy = A @ A.T, (A @ Y).T, (Y ** 2).sum(0)
    Lam = torch.eye(M, dtype=torch.float64) + (k / s2) * Phi
    c = torch.sqrt(k) * b / s2
    LL = torch.linalg.cholesky(Lam)
    tt = torch.linalg.solve_triangular(LL, c.T, upper=False)
    val = torch.sum(-0.5 * N * torch.log(2 * np.pi * s2) - yy / (2 * s2) + 0.5 * (tt * tt).sum(0))
    val = val - P * torch.log(torch.diagonal(LL)).sum()
    if residual == "diagonal":
        val = val - P * k * (N - torch.trace(Phi)) / (2 * s2)
    val.backward()
    return dict(value=float(val.detach()), z=z.grad.numpy(), lengthscales=ell.grad.numpy(), noise_var=float(s2.grad),
                k_var=float(k.grad))


def case(N, M, d, P, seed=0, scalar_ell=False):
    """(X, Y, z, ell) in float64, svgp_data-style: d = 1: X ~ U(0, M / 2), z = linspace (spacing half a lengthscale),
    ell = 1; d = 3: X ~ U(0, 4)^3, z uniform, ARD ell (or one scalar); Y_p = sin(sum_d X + p) + 0.3 eps (noise variance
    0.09)."""
    rng = np.random.RandomState(seed)
    dom = 0.5 * M if d == 1 else 4.0
    X = rng.uniform(0, dom, (N, d))
    Y = np.sin(X.sum(1, keepdims=True) + np.arange(P)[None, :]) + 0.3 * rng.randn(N, P)
    z = np.linspace(0, dom, M)[:, None] if d == 1 else rng.uniform(0, dom, (M, d))
    ell = np.ones(1) if d == 1 else (np.array([1.1]) if scalar_ell else np.array([0.9, 1.1, 1.3])[:d])
    return X, Y, z, ell


def directional_fd(f, x, direction, h):
    """Central difference (f(x + h u) - f(x - h u)) / (2 h) of a scalar function of an array."""
    return (f(x + h * direction) - f(x - h * direction)) / (2.0 * h)
