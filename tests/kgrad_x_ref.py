"""Float64 host references for the INPUT gradient of the sparse-GP bounds (hb_sgp_kgrad_x / hb_sgp_wkgrad_x,
SparseGP.collapsed_bound_and_grad(x_grad=True), SparseGP.elbo_and_grad(x_grad=True), models.DeepKernelSVGP), on top of
collapsed_grad_ref.py and elbo_grad_ref.py and in their notation:

    K = K(z, X) [M, N],  Kbar = (Q K) diag(w) + R r^T  (w = 1, r = Y: Kbar = Q K + R Y^T),  E = Kbar o K,
    xbar_jd = +sum_i E_ij (z_id - x_jd) / ell_d^2                 (streamed_x / streamed_x_w: the kernels' semantics)
    scale_jd = sum_i (sum_k |Q_ik| K_kj |w_j| + sum_p |R_ip r_jp|) K_ij |z_id - x_jd| / ell_d^2      (abs_scale)

Every dependence of the bounds on X goes through K(z, X) (k(x, x) = 1), so with Q, R of the bound's tail xbar is the
complete dF/dX.  The autograd functions differentiate the bound / the ELBO / a fixed-weight surrogate written in torch
ops with X.requires_grad and use no formula of this file; `mlp` and `dkl_bound` restate models.DeepKernelSVGP."""
import numpy as np

import elbo_grad_ref as E
import optimal_q_ref as R
import sites_ref as S_


def _terms(X, z, ell, Kbar, K):
    X, z, ell = (np.asarray(a, np.float64) for a in (X, z, ell))
    d = z.shape[1]
    l = np.broadcast_to(ell, (d,))
    out = np.zeros((X.shape[0], d))
    Em = Kbar * K
    for k in range(d):
        out[:, k] = (Em * (z[:, k, None] - X[None, :, k])).sum(0) / l[k] ** 2
    return out


def streamed_x(X, Y, z, ell, Q, Rw):
    """xbar [N, d] for given weights: the semantics of hb_sgp_kgrad_x."""
    K = R.rbf(np.asarray(z, np.float64), np.asarray(X, np.float64), np.asarray(ell, np.float64))
    return _terms(X, z, ell, Q @ K + Rw @ np.asarray(Y, np.float64).T, K)


def streamed_x_w(X, w, r, z, ell, Q, Rw):
    """xbar [N, d] of the column-weighted form: the semantics of hb_sgp_wkgrad_x."""
    K = R.rbf(np.asarray(z, np.float64), np.asarray(X, np.float64), np.asarray(ell, np.float64))
    return _terms(X, z, ell, (Q @ K) * np.reshape(w, (1, -1)) + Rw @ np.reshape(r, (1, -1)), K)


def abs_scale(X, Y, z, ell, Q, Rw, w=None):
    """scale [N, d]: the sum of the absolute terms of xbar (Y [N, P]; the weighted form: Y = r [N, 1] and w [N])."""
    X, z, ell = (np.asarray(a, np.float64) for a in (X, z, ell))
    K = R.rbf(z, X, ell)
    QK = np.abs(Q) @ K
    if w is not None:
        QK = QK * np.abs(np.reshape(w, (1, -1)))
    Kabs = QK + np.abs(Rw) @ np.abs(np.asarray(Y, np.float64)).T
    d = z.shape[1]
    l = np.broadcast_to(ell, (d,))
    out = np.zeros((X.shape[0], d))
    for k in range(d):
        out[:, k] = (Kabs * K * np.abs(z[:, k, None] - X[None, :, k])).sum(0) / l[k] ** 2
    return out


def gamma(M, P):
    """(2 M + P + 16) 2^-53: the a-priori bound of summing 2 M + P terms plus 16 ulp for the rounding of K and the
    products."""
    return (2 * M + P + 16) * 2.0 ** -53


def bound(gap, scale, M, P):
    """The project's rule: 4 x max(gap of the two CPU evaluations, gamma x the sum of absolute terms)."""
    return 4.0 * max(gap, gamma(M, P) * scale)


# ---------------------------------------------------------------------------------------------------- torch, float64
def _t(a):
    import torch

    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)


def _rbf(a, c, ell):
    import torch

    a_, c_ = a / ell, c / ell
    r2 = 0.0
    for k in range(a.shape[1]):
        r2 = r2 + (a_[:, k, None] - c_[None, :, k]) ** 2
    return torch.exp(-0.5 * r2)


def _torch_bound(X, Y, z, ell, jitter, s2, k, residual):
    """optimal_q_ref's collapsed bound in torch ops (tensors in, a scalar tensor out)."""
    import torch

    N, P, M = X.shape[0], Y.shape[1], z.shape[0]
    eye = torch.eye(M, dtype=torch.float64)
    L = torch.linalg.cholesky(_rbf(z, z, ell) + jitter * eye)
    A = torch.linalg.solve_triangular(L, _rbf(z, X, ell), upper=False)
    Phi, b, yy = A @ A.T, (A @ Y).T, (Y ** 2).sum(0)
    LL = torch.linalg.cholesky(eye + (k / s2) * Phi)
    tt = torch.linalg.solve_triangular(LL, (torch.sqrt(k) * b / s2).T, upper=False)
    val = torch.sum(-0.5 * N * torch.log(2 * np.pi * s2) - yy / (2 * s2) + 0.5 * (tt * tt).sum(0))
    val = val - P * torch.log(torch.diagonal(LL)).sum()
    if residual == "diagonal":
        val = val - P * k * (N - torch.trace(Phi)) / (2 * s2)
    return val


def bound_autograd_x(X, Y, z, ell, jitter, noise_var, k_var=1.0, residual="diagonal"):
    """dF/dX [N, d] of the collapsed bound through torch.autograd."""
    Xt = _t(X).requires_grad_(True)
    _torch_bound(Xt, _t(Y), _t(z), _t(ell), jitter, _t(noise_var), _t(k_var), residual).backward()
    return Xt.grad.numpy()


def surrogate_autograd_x(X, w, r, z, ell, Q, Rw):
    """d/dX of f = 1/2 sum_ij w_j K_ij (Q K)_ij + sum_ij R_i r_j K_ij for FIXED symmetric Q, R, w, r: df/dK = Kbar, so this
    is xbar of the weighted form (w = 1, r = Y [N, P], R [M, P]: the unweighted one) without its formula."""
    Xt = _t(X).requires_grad_(True)
    K = _rbf(_t(z), Xt, _t(ell))
    rr = _t(np.reshape(r, (np.shape(X)[0], -1)))
    f = 0.5 * ((_t(Q) @ K) * K * _t(np.reshape(w, (1, -1)))).sum() + ((_t(Rw) @ rr.T) * K).sum()
    f.backward()
    return Xt.grad.numpy()


def elbo_autograd_x(X, y, z, ell, jitter, lik, m, S, param=1.0, k_var=1.0, residual="diagonal"):
    """dF/dX [N, d] of the ELBO at the fixed q through torch.autograd: elbo_grad_ref's torch marginals with
    X.requires_grad and its objectives (Gaussian and Poisson closed forms, Bernoulli the 20-node rule as it stands)."""
    import torch

    Xt = _t(X).requires_grad_(True)
    yt = _t(np.reshape(y, -1))
    mu, v = E._torch_marginals(Xt, _t(z), _t(ell), _t(k_var), jitter, _t(m), _t(np.tril(S)), residual)
    if lik == E.GAUSSIAN:
        l = -0.5 * np.log(2 * np.pi * param) - ((yt - mu) ** 2 + v) / (2 * param)
    elif lik == E.POISSON:
        l = yt * mu - torch.exp(mu + 0.5 * v) - torch.lgamma(yt + 1.0)
    else:
        x, wq = S_.gh(20)
        f = mu[:, None] + torch.sqrt(2.0 * v)[:, None] * torch.tensor(x)[None, :]
        l = ((yt[:, None] * f - torch.nn.functional.softplus(f)) * torch.tensor(wq)).sum(1)
    l.sum().backward()
    return Xt.grad.numpy()


# ---------------------------------------------------------------------------------------------------- deep kernel
def mlp(X, weights, activation="tanh"):
    """hb.nn.NeuralNet restated in float64 torch: weights = [(w0, b0), (w1, b1), ..] (tensors or arrays), the activation
    after every layer but the last.  Returns a torch tensor [N, feature_dim]."""
    import torch

    act = dict(tanh=torch.tanh, relu=torch.relu, sigmoid=torch.sigmoid)[activation]
    h = X if isinstance(X, torch.Tensor) else _t(X)
    for i, (w, b) in enumerate(weights):
        w, b = (a if isinstance(a, torch.Tensor) else _t(a) for a in (w, b))
        h = h @ w + b.reshape(1, -1)
        if i < len(weights) - 1:
            h = act(h)
    return h


def dkl_bound(X, Y, weights, z, ell, jitter, noise_var, k_var, activation="tanh", grad=False):
    """The collapsed bound of models.DeepKernelSVGP on the features mlp(X) in float64 torch: its value (a float), and
    with grad=True also dict(z, lengthscales, noise_var, k_var, net=[(dw0, db0), ..]) from torch.autograd, with respect
    to the CONSTRAINED values."""
    import torch

    ws = [(_t(w).requires_grad_(grad), _t(b).requires_grad_(grad)) for w, b in weights]
    zt, et, s2, k = (_t(a).requires_grad_(grad) for a in (z, ell, noise_var, k_var))
    with torch.set_grad_enabled(grad):
        val = _torch_bound(mlp(X, ws, activation), _t(Y), zt, et, jitter, s2, k, "diagonal")
    if not grad:
        return float(val)
    val.backward()
    return float(val.detach()), dict(z=zt.grad.numpy(), lengthscales=et.grad.numpy(), noise_var=float(s2.grad),
                                     k_var=float(k.grad), net=[(w.grad.numpy(), b.grad.numpy()) for w, b in ws])
