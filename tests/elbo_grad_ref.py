"""Numpy float64 restatement of the hyper-parameter gradient of the ELBO at a FIXED q(u) for a factorising likelihood
(SparseGP.elbo_and_grad), on top of sites_ref.py, optimal_q_ref.py and collapsed_grad_ref.py and in their notation:

    K = K(z, X) [M, N],  W = chol(K(z, z) + jitter I)^-1,  A = W K,  q(u) = N(m, S S^T),  Sigma = S S^T,
    mu_j = sqrt(k) m a_j,  v_j = k (a_j^T Sigma a_j + rho (1 - a_j^T a_j))      (rho = 1 'diagonal', 0 'neglected'; no |.|),
    F = sum_j l_j(mu_j, v_j) - KL(q || N(0, I)).

With per-point weights w_j = -2 dl_j/dv_j and r_j = dl_j/dmu_j (the sites: w = lam, r = gamma = beta - lam mu; Stein):
    Abar = 2 G A diag(w) + g^T r^T,   G = -(k / 2) (Sigma - rho I),   g = sqrt(k) m [1, M]
    streamed part:  Kbar = (Q K) diag(w) + R r^T,  Q = 2 W^T G W,  R = W^T g^T;  E = Kbar o K and the sums of hb_sgp_kgrad
    K(z, z) part:   T = -(2 G Phi_w + g^T b_w),  Phi_w = A diag(w) A^T,  b_w = (A r)^T   (collapsed_grad_ref.kmm_part)
    dF/dk = sum_j (r_j mu_j - w_j v_j) / (2 k)

`grad_from_weights` takes ANY w, r (the kernel tests draw w with both signs and exact zeros); for fixed w, r it is the
exact gradient of the surrogate sum_j (r_j mu_j - w_j v_j / 2), which `surrogate_autograd` differentiates with
torch.autograd -- an independent float64 evaluation that uses no formula of this file.  `elbo_autograd` is the ELBO
itself through torch.autograd with a differentiable 20-node quadrature for Bernoulli."""
import numpy as np

import collapsed_grad_ref as C
import optimal_q_ref as R
import sites_ref as S_

GAUSSIAN, BERNOULLI, POISSON = S_.GAUSSIAN, S_.BERNOULLI, S_.POISSON


def marginals(m, S, A, k_var, residual="diagonal"):
    """(mu [N], v [N]) in float64 WITHOUT the |.| on the residual (the function the gradient differentiates)."""
    rho = 1.0 if residual == "diagonal" else 0.0
    mu = np.sqrt(k_var) * (np.reshape(m, -1) @ A)
    v = k_var * (((S.T @ A) ** 2).sum(0) + rho * (1.0 - (A * A).sum(0)))
    return mu, v


def streamed(X, w, r, z, ell, Q, Rw):
    """(zbar [M, d], ellbar [dl]) of the streamed part for given weights: the semantics of hb_sgp_wkgrad."""
    X, z, ell = (np.asarray(a, np.float64) for a in (X, z, ell))
    K = R.rbf(z, X, ell)
    E = ((Q @ K) * np.reshape(w, (1, -1)) + Rw @ np.reshape(r, (1, -1))) * K
    d = z.shape[1]
    l = np.broadcast_to(ell, (d,))
    zbar, ellbar = np.zeros_like(z), np.zeros(d)
    for k in range(d):
        diff = z[:, k, None] - X[None, :, k]
        zbar[:, k] = -(E * diff).sum(1) / l[k] ** 2
        ellbar[k] = (E * diff * diff).sum() / l[k] ** 3
    return zbar, (ellbar if ell.shape[0] == d else ellbar.sum(keepdims=True))


def grad_from_weights(X, w, r, z, ell, jitter, m, S, k_var=1.0, residual="diagonal"):
    """dict(z, lengthscales, k_var, z_streamed, z_kmm, ell_streamed, ell_kmm, Q, R, w, r, W, Phi, b, k_var_abs) for given
    per-point weights."""
    X, z, ell = (np.asarray(a, np.float64) for a in (X, z, ell))
    w, r = np.asarray(w, np.float64).reshape(-1), np.asarray(r, np.float64).reshape(-1)
    m, S = np.asarray(m, np.float64).reshape(1, -1), np.tril(np.asarray(S, np.float64))
    k = float(k_var)
    rho = 1.0 if residual == "diagonal" else 0.0
    M = z.shape[0]
    _, W = R.chol_factor(z, ell, jitter)
    A = R.A_of(W, z, X, ell)
    G = -0.5 * k * (S @ S.T - rho * np.eye(M))
    g = np.sqrt(k) * m
    Q, Rw = C.weights(W, G, g)
    zs, es = streamed(X, w, r, z, ell, Q, Rw)
    Phi = A @ (A * w[None, :]).T
    Phi = np.tril(Phi) + np.tril(Phi, -1).T
    b = (A @ r)[None, :]
    zk, ek = C.kmm_part(z, ell, W, G, g, Phi, b)
    mu, v = marginals(m, S, A, k, residual)
    t1, t2 = float(np.sum(r * mu)), float(np.sum(w * v))
    return dict(z=zs + zk, lengthscales=es + ek, k_var=(t1 - t2) / (2.0 * k), z_streamed=zs, z_kmm=zk, ell_streamed=es,
                ell_kmm=ek, Q=Q, R=Rw, w=w, r=r, W=W, Phi=Phi, b=b, k_var_abs=(abs(t1) + abs(t2)) / (2.0 * k))


def kl(m, S):
    """KL(N(m, S S^T) || N(0, I))."""
    m, S = np.reshape(m, -1), np.tril(S)
    return 0.5 * (float((S * S).sum()) + float(m @ m) - m.size) - float(np.log(np.abs(np.diag(S))).sum())


def elbo_and_grad(X, y, z, ell, jitter, lik, m, S, param=1.0, k_var=1.0, residual="diagonal"):
    """grad_from_weights at the sites w = lam, r = gamma = beta - lam mu of the likelihood, plus `value` = the ELBO."""
    X, z, ell = (np.asarray(a, np.float64) for a in (X, z, ell))
    m, S = np.asarray(m, np.float64).reshape(1, -1), np.tril(np.asarray(S, np.float64))
    _, W = R.chol_factor(z, ell, jitter)
    mu, v = marginals(m, S, R.A_of(W, z, X, ell), float(k_var), residual)
    l, lam, beta, _ = S_.sites(lik, y, mu, v, param)
    out = grad_from_weights(X, lam, beta - lam * mu, z, ell, jitter, m, S, k_var, residual)
    out["value"] = float(l.sum()) - kl(m, S)
    return out


def _torch_marginals(X, z, ell, k, jitter, m, S, residual):
    import torch

    M = z.shape[0]

    def rbf(a, c):
        a_, c_ = a / ell, c / ell
        r2 = 0.0
        for k_ in range(a.shape[1]):
            r2 = r2 + (a_[:, k_, None] - c_[None, :, k_]) ** 2
        return torch.exp(-0.5 * r2)

    L = torch.linalg.cholesky(rbf(z, z) + jitter * torch.eye(M, dtype=torch.float64))
    A = torch.linalg.solve_triangular(L, rbf(z, X), upper=False)
    mu = torch.sqrt(k) * (m.reshape(1, -1) @ A).reshape(-1)
    v = ((S.T @ A) ** 2).sum(0)
    if residual == "diagonal":
        v = v + (1.0 - (A * A).sum(0))
    return mu, k * v


def _autograd(X, z, ell, jitter, m, S, k_var, residual, objective):
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    z, ell, k = t(z).requires_grad_(True), t(ell).requires_grad_(True), t(k_var).requires_grad_(True)
    mu, v = _torch_marginals(t(X), z, ell, k, jitter, t(m), t(np.tril(S)), residual)
    val = objective(mu, v)
    val.backward()
    return dict(value=float(val.detach()), z=z.grad.numpy(), lengthscales=ell.grad.numpy(), k_var=float(k.grad))


def surrogate_autograd(X, w, r, z, ell, jitter, m, S, k_var=1.0, residual="diagonal"):
    """dict(value, z, lengthscales, k_var) of sum_j (r_j mu_j - w_j v_j / 2) for FIXED w, r through torch.autograd."""
    import torch

    w, r = (torch.tensor(np.asarray(a, np.float64).reshape(-1)) for a in (w, r))
    return _autograd(X, z, ell, jitter, m, S, k_var, residual, lambda mu, v: (r * mu).sum() - 0.5 * (w * v).sum())


def elbo_autograd(X, y, z, ell, jitter, lik, m, S, param=1.0, k_var=1.0, residual="diagonal"):
    """dict(value, z, lengthscales, k_var): the ELBO at the fixed q through torch.autograd in float64.  Gaussian and
    Poisson: the closed forms; Bernoulli: the 20-node Gauss-Hermite rule differentiated as it stands (so its gradient
    is the derivative of the quadrature VALUE, where the restatement uses Stein's identity on the quadrature of the
    second derivative)."""
    import torch

    y = torch.tensor(np.asarray(y, np.float64).reshape(-1))

    def objective(mu, v):
        if lik == GAUSSIAN:
            l = -0.5 * np.log(2 * np.pi * param) - ((y - mu) ** 2 + v) / (2 * param)
        elif lik == POISSON:
            l = y * mu - torch.exp(mu + 0.5 * v) - torch.lgamma(y + 1.0)
        else:
            x, wq = S_.gh(20)
            f = mu[:, None] + torch.sqrt(2.0 * v)[:, None] * torch.tensor(x)[None, :]
            l = ((y[:, None] * f - torch.nn.functional.softplus(f)) * torch.tensor(wq)).sum(1)
        return l.sum() - kl(m, S)

    return _autograd(X, z, ell, jitter, m, S, k_var, residual, objective)


def q_case(M, seed=0):
    """A full-rank q away from any optimum: (m [1, M], S [M, M] lower with a positive diagonal)."""
    rng = np.random.RandomState(1000 + seed)
    S = np.tril(0.05 * rng.randn(M, M), -1) + np.diag(rng.uniform(0.3, 0.8, M))
    return 0.5 * rng.randn(1, M), S


def weights_case(N, seed=0):
    """(w [N] with both signs and about 10 % exact zeros, r [N])."""
    rng = np.random.RandomState(2000 + seed)
    w = rng.randn(N)
    w[rng.uniform(size=N) < 0.1] = 0.0
    return w, rng.randn(N)
