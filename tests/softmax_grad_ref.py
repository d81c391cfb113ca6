"""Numpy float64 restatement of the hyper-parameter gradient of the multi-class (softmax) ELBO at FIXED q(u_c)
(hb_lik_softmax_grad, SparseGP.elbo_and_grad_multi), on top of softmax_ref.py and elbo_grad_ref.py and in
their notation.  The value is the fixed-node sum natgrad_q reports,

    F = sum_j l_j - sum_c KL(q_c || N(0, I)),   l_j = mean_s log softmax(f_s)_{y_j},   f_sc = mu_jc + sqrt(v_jc) eps_sc,

and the weights are ITS derivatives in the marginals (reparameterisation: df_sc/dmu = 1, df_sc/dv = eps_sc / (2 sqrt(v))):

    r_jc = dl_j/dmu_jc = mean_s d_sc,   w_jc = -2 dl_j/dv_jc = -mean_s(d_sc eps_sc) / sqrt(v_jc),   d_sc = [c = y_j] - p_sc

(v_jc <= 0: w_jc = mean_s p_sc (1 - p_sc), Price's form, the limit of the exact expectation's derivative).  Class by class
they go through elbo_grad_ref.grad_from_weights, and the classes add.  `elbo_autograd` differentiates the node sum itself
with torch.autograd -- an independent float64 evaluation that uses none of these formulas."""
import numpy as np

import elbo_grad_ref as E
import optimal_q_ref as R
import softmax_ref as F

_SUMMED = ("z", "lengthscales", "k_var", "z_streamed", "z_kmm", "ell_streamed", "ell_kmm", "k_var_abs")


def weights(y, mu, v, nodes):
    """(l [N], w [C, N], r [C, N], a [C, N], lam [C, N]) in float64 for f_jc ~ N(mu[c, j], v[c, j]) and nodes [S, C].
    a_jc = mean_s |d_sc eps_sc| / sqrt(v_jc) is the scale of w's summands (what its rounding error is measured against);
    where v_jc <= 0, w = lam and a = lam."""
    mu, v, nodes = (np.asarray(a, np.float64) for a in (mu, v, nodes))
    lab = np.asarray(y).reshape(-1).astype(np.int64)
    C, N = mu.shape
    S = nodes.shape[0]
    l, lam, r, t, ta = np.zeros(N), np.zeros((C, N)), np.zeros((C, N)), np.zeros((C, N)), np.zeros((C, N))
    for j0, j1 in F._blocks(N, S, C):
        p, q, lp = F.softmax_parts(F._f(mu, v, nodes, j0, j1))
        hot = (np.arange(C)[None, :] == lab[j0:j1, None])[:, None, :]
        d = np.where(hot, q, -p)                                            # [n, S, C]
        r[:, j0:j1] = (d.sum(1) / S).T
        t[:, j0:j1] = ((d * nodes[None]).sum(1) / S).T
        ta[:, j0:j1] = (np.abs(d * nodes[None]).sum(1) / S).T
        lam[:, j0:j1] = ((p * q).sum(1) / S).T
        l[j0:j1] = np.where(hot, lp, 0.0).sum((1, 2)) / S
    pos = v > 0.0
    sd = np.sqrt(np.where(pos, v, 1.0))
    return l, np.where(pos, -t / sd, lam), r, np.where(pos, ta / sd, lam), lam


def _A(X, z, ell, jitter):
    X, z, ell = (np.asarray(a, np.float64) for a in (X, z, ell))
    _, W = R.chol_factor(z, ell, jitter)
    return R.A_of(W, z, X, ell)


def marginals(X, z, ell, jitter, m, S, k_var, residual="diagonal"):
    """(mu [C, N], v [C, N]) WITHOUT the |.| on the residual (elbo_grad_ref.marginals per class)."""
    A = _A(X, z, ell, jitter)
    out = [E.marginals(m[c], np.tril(S[c]), A, float(k_var), residual) for c in range(len(m))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def value(X, y, z, ell, jitter, nodes, m, S, k_var=1.0, residual="diagonal"):
    """The fixed-node ELBO at the fixed q."""
    mu, v = marginals(X, z, ell, jitter, m, S, k_var, residual)
    return float(weights(y, mu, v, nodes)[0].sum()) - sum(E.kl(m[c], S[c]) for c in range(len(m)))


def grad_from_class_weights(X, w, r, z, ell, jitter, m, S, k_var=1.0, residual="diagonal"):
    """The sum over the classes of elbo_grad_ref.grad_from_weights(w[c], r[c], m[c], S[c]): dict(z, lengthscales, k_var,
    z_streamed, z_kmm, ell_streamed, ell_kmm, k_var_abs)."""
    parts = [E.grad_from_weights(X, w[c], r[c], z, ell, jitter, m[c], S[c], k_var, residual) for c in range(len(m))]
    return {n: sum(p[n] for p in parts) for n in _SUMMED}


def elbo_and_grad(X, y, z, ell, jitter, nodes, m, S, k_var=1.0, residual="diagonal", price=False):
    """grad_from_class_weights at the weights of the node sum, plus `value`, `w`, `r`.  price=True substitutes Price's
    lam = mean_s p (1 - p) for w: the curvature site of the natural-gradient step, NOT the derivative of the value."""
    mu, v = marginals(X, z, ell, jitter, m, S, k_var, residual)
    l, w, r, _, lam = weights(y, mu, v, nodes)
    out = grad_from_class_weights(X, lam if price else w, r, z, ell, jitter, m, S, k_var, residual)
    out["value"] = float(l.sum()) - sum(E.kl(m[c], S[c]) for c in range(len(m)))
    out["w"], out["r"] = (lam if price else w), r
    return out


def elbo_autograd(X, y, z, ell, jitter, nodes, m, S, k_var=1.0, residual="diagonal"):
    """dict(value, z, lengthscales, k_var): the fixed-node ELBO at the fixed q through torch.autograd in float64, the
    node sum differentiated as it stands (torch.log_softmax over the classes, sqrt(v) under the nodes)."""
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    zt, et, kt = t(z).requires_grad_(True), t(ell).requires_grad_(True), t(k_var).requires_grad_(True)
    Xt, C = t(X), len(m)
    cols = [E._torch_marginals(Xt, zt, et, kt, jitter, t(m[c]), t(np.tril(S[c])), residual) for c in range(C)]
    mu, v = torch.stack([c[0] for c in cols], 1), torch.stack([c[1] for c in cols], 1)      # [N, C]
    f = mu[:, None, :] + torch.sqrt(v)[:, None, :] * t(nodes)[None, :, :]                   # [N, S, C]
    lab = torch.tensor(np.asarray(y).reshape(-1).astype(np.int64))
    lp = torch.log_softmax(f, -1)
    l = torch.gather(lp, 2, lab[:, None, None].expand(-1, f.shape[1], 1))[:, :, 0].mean(1)
    val = l.sum() - sum(E.kl(m[c], S[c]) for c in range(C))
    val.backward()
    return dict(value=float(val.detach()), z=zt.grad.numpy(), lengthscales=et.grad.numpy(), k_var=float(kt.grad))


def q_case(C, M, seed=0):
    """C full-rank blocks away from any optimum: (m [C, M], S [C, M, M] lower with positive diagonals)."""
    qs = [E.q_case(M, seed + 17 * c) for c in range(C)]
    return np.concatenate([q[0] for q in qs]), np.stack([q[1] for q in qs])
