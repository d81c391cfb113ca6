"""Numpy restatement of multi-class classification with the softmax likelihood (hb_lik_softmax_*, SparseGP.natgrad_q with
likelihoods.Softmax, models.SVGPMulticlass), float64 unless a dtype is asked for, built on optimal_q_ref / sites_ref.

Model (whitened): u_c ~ N(0, I_M) independent, f_c = sqrt(k) (u_c A + residual), y_j in {0 .. C-1}; q(u_c) = N(m_c, S_c S_c^T)
independent per class, kept as Lambda_c, eta_c.  With S standard-normal nodes eps [S, C] shared by all points:

    mu_jc = sqrt(k) m_c a_j,   v_jc = k (|S_c^T a_j|^2 + r_j)
    f_sc = mu_jc + sqrt(max(v_jc, 0)) eps_sc,   p_s = softmax_c(f_s)
    l_j = mean_s log p_{s, y_j},   g_jc = mean_s ([c = y_j] - p_sc),   lam_jc = mean_s p_sc (1 - p_sc),   beta = g + lam mu
    Phi_c = A diag(lam_c) A^T,  b_c = A beta_c,  Lambda_c <- (1 - rho) Lambda_c + rho (I + k Phi_c),  eta_c likewise with sqrt(k) b_c
    ELBO = sum_j l_j - sum_c KL(q_c || N(0, I)).

The softmax is formed as the device forms it: with mx the maximum over classes and `first` the lowest class attaining it,
e_c = exp(f_c - mx) for c != first, rest = sum_{c != first} e_c, p_first = 1 / (1 + rest), 1 - p_first = rest / (1 + rest),
log p_c = f_c - mx - log1p(rest) -- no 1 - p where p is near 1."""
import numpy as np

import optimal_q_ref as R
import sites_ref as SR


def softmax_parts(f):
    """(p, 1 - p, log p) of softmax over the LAST axis of f."""
    C = f.shape[-1]
    mx = f.max(-1, keepdims=True)
    first = np.arange(C) == np.argmax(f, -1)[..., None]
    d = f - mx
    e = np.where(first, 0.0, np.exp(d))
    rest = e.sum(-1, keepdims=True)
    inv = 1.0 / (1.0 + rest)
    return np.where(first, inv, e * inv), np.where(first, rest * inv, 1.0 - e * inv), d - np.log1p(rest)


def _blocks(N, S, C):
    step = max(1, (1 << 21) // (S * C))
    return [(j0, min(N, j0 + step)) for j0 in range(0, N, step)]


def _f(mu, v, nodes, j0, j1):
    """f [n, S, C] of the points j0 .. j1."""
    sd = np.sqrt(np.maximum(v[:, j0:j1], 0.0))
    return mu[:, j0:j1].T[:, None, :] + sd.T[:, None, :] * nodes[None, :, :]


def sites(y, mu, v, nodes):
    """(l [N], lam [C, N], beta [C, N], g [C, N]) in float64 for f_jc ~ N(mu[c, j], v[c, j]) and nodes [S, C]."""
    mu, v, nodes = (np.asarray(a, np.float64) for a in (mu, v, nodes))
    lab = np.asarray(y).reshape(-1).astype(np.int64)
    C, N = mu.shape
    S = nodes.shape[0]
    l, lam, g = np.zeros(N), np.zeros((C, N)), np.zeros((C, N))
    for j0, j1 in _blocks(N, S, C):
        p, q, lp = softmax_parts(_f(mu, v, nodes, j0, j1))
        hot = (np.arange(C)[None, :] == lab[j0:j1, None])[:, None, :]
        g[:, j0:j1] = (np.where(hot, q, -p).sum(1) / S).T
        lam[:, j0:j1] = ((p * q).sum(1) / S).T
        l[j0:j1] = np.where(hot, lp, 0.0).sum((1, 2)) / S
    return l, lam, g + lam * mu, g


def predict(mu, v, nodes, y=None):
    """(prob [C, N], logdens [N] or None): mean_s softmax(f_s) and log mean_s softmax(f_s)_{y_j} (log-sum-exp over nodes)."""
    mu, v, nodes = (np.asarray(a, np.float64) for a in (mu, v, nodes))
    C, N = mu.shape
    S = nodes.shape[0]
    prob = np.zeros((C, N))
    ld = None if y is None else np.zeros(N)
    for j0, j1 in _blocks(N, S, C):
        p, q, lp = softmax_parts(_f(mu, v, nodes, j0, j1))
        prob[:, j0:j1] = (p.sum(1) / S).T
        if y is not None:
            lab = np.asarray(y).reshape(-1).astype(np.int64)[j0:j1]
            py, qy, lpy = (np.take_along_axis(a, lab[:, None, None], 2)[:, :, 0] for a in (p, q, lp))       # [n, S]
            top = lpy.max(1)
            # a density above 1/2 from the mean of 1 - p (its digits survive as it goes to 1), else the log-sum-exp
            with np.errstate(divide="ignore"):                                  # log1p(-1) on the branch not taken
                ld[j0:j1] = np.where(py.sum(1) / S > 0.5, np.log1p(-(qy.sum(1) / S)),
                                     top + np.log(np.exp(lpy - top[:, None]).sum(1)) - np.log(S))
    return prob, ld


def log_softmax(f):
    """log softmax over the FIRST axis of f [C, n]."""
    return np.moveaxis(softmax_parts(np.moveaxis(np.asarray(f, np.float64), 0, -1))[2], -1, 0)


def marginals(m, S, A, k_var, residual="diagonal"):
    """(mu [C, N], v [C, N]) for the C blocks m [C, M], S [C, M, M]."""
    out = [SR.marginals(m[c], S[c], A, k_var, residual) for c in range(m.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def natgrad(X, y, z, ell, jitter, C, nodes, k_var=1.0, residual="diagonal", q0=None, steps=20, rho=0.5, tol=1e-8,
            dtype=np.float64, W=None, ksplit=None):
    """(m [C, M], S [C, M, M], info): the natural-gradient iteration on a dense A.  info = dict(elbo, residual, steps);
    the residual is the largest over the classes of max|Lambda_c - (I + k Phi_c)| / max|I + k Phi_c|.  dtype float32: A, the
    marginals and the weighted products in float32 (lam, beta rounded to float32), the tails in float64, for a given W."""
    z64, ell64 = np.asarray(z, np.float64), np.asarray(ell, np.float64)
    if W is None:
        _, W = R.chol_factor(z64, ell64, jitter)
    M = z64.shape[0]
    A = R.A_of(*(np.asarray(a, dtype) for a in (W, z, X, ell)))
    if q0 is None:
        Lam, eta = np.stack([np.eye(M)] * C), np.zeros((C, M))
    else:
        m0, S0 = (np.asarray(a, np.float64) for a in q0)
        Lam = np.stack([np.linalg.inv(S0[c] @ S0[c].T) for c in range(C)])
        eta = np.stack([Lam[c] @ m0[c] for c in range(C)])
    out = dict(elbo=[], residual=[])
    for it in range(steps + 1):
        tails = [SR.tail(Lam[c], eta[c]) for c in range(C)]
        m, S = np.concatenate([t[0] for t in tails]), np.stack([t[1] for t in tails])
        kl = sum(0.5 * (np.trace(t[2]) + t[0].reshape(-1) @ t[0].reshape(-1) - M + t[3]) for t in tails)
        mu, v = marginals(m, S, A, k_var, residual)
        l, lam, beta, _ = sites(y, mu, v, nodes)
        lam, beta = lam.astype(dtype), beta.astype(dtype)
        Lt, et = np.zeros((C, M, M)), np.zeros((C, M))
        for c in range(C):
            Phi, b, _ = SR.wstats_from_W(X, lam[c], beta[c], z, ell, W, dtype=dtype, ksplit=ksplit)
            Lt[c], et[c] = np.eye(M) + k_var * Phi, np.sqrt(k_var) * b.reshape(-1)
        out["elbo"].append(float(l.sum() - kl))
        out["residual"].append(float(max(np.abs(Lam[c] - Lt[c]).max() / np.abs(Lt[c]).max() for c in range(C))))
        if it == steps or (it > 0 and abs(out["elbo"][-1] - out["elbo"][-2]) <= tol * abs(out["elbo"][-1])):
            break
        Lam, eta = (1 - rho) * Lam + rho * Lt, (1 - rho) * eta + rho * et
    out["elbo"], out["residual"], out["steps"] = np.asarray(out["elbo"]), np.asarray(out["residual"]), it
    return m, S, out


def halton_normal(S, C):
    """[S, C] equal-weight quasi-random standard-normal nodes: the Halton sequence (bases 2, 3, 5, ..; points 1 .. S)
    through the inverse normal distribution function.  On the three-class ring (N = 600, M = 32, k_var = 4) the q(u) fitted
    with S = 1024 of these nodes leaves a gradient of the exact expected log-likelihood (24^3 Gauss-Hermite rule per point)
    with respect to m of at most 0.04, 0.27 standard errors of a 128-draw Monte-Carlo gradient; the 128 pseudo-random
    nodes of ring() leave 0.48, about 12 standard errors."""
    from statistics import NormalDist

    primes = [2, 3, 5, 7, 11, 13, 17, 19][:C]
    assert len(primes) == C, "halton_normal: at most 8 classes"
    inv, out = NormalDist().inv_cdf, np.zeros((S, C))
    for c, base in enumerate(primes):
        for i in range(S):
            frac, x, n = 1.0, 0.0, i + 1
            while n > 0:
                frac /= base
                x += frac * (n % base)
                n //= base
            out[i, c] = inv(x)
    return out


def ring(C, N, M, S, seed):
    """(X [N, 2], y [N], Z [M, 2], eps [S, C]): C blobs of radius 0.5 on a ring of radius 3."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(C) / C
    cent = 3.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    y = rng.integers(0, C, N)
    X = cent[y] + 0.5 * rng.standard_normal((N, 2))
    Z = X[rng.choice(N, M, replace=False)]
    eps = rng.standard_normal((S, C))
    return X, y, Z, eps
