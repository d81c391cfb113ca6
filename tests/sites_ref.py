"""Numpy restatement of the natural-gradient fit of q(u) for a factorising likelihood (SparseGP.natgrad_q), built on
optimal_q_ref, in float64 unless a dtype is asked for.  Model:

    u ~ N(0, I_M),  f_j = sqrt(k) (u^T A_j + sqrt(r_j) eps_j),  A = Lm^-1 K(z, X),  r_j = |1 - sum_m A_mj^2| or 0,
    y_j ~ p(y_j | f_j),  q(u) = N(m, S S^T) kept as Lambda = (S S^T)^-1, eta = Lambda m.

One iteration: marginals mu_j = sqrt(k) m^T A_j, v_j = k (|S^T A_j|^2 + r_j); sites l_j = E log p, g_j = E dlog p/df,
lam_j = E -d2 log p/df2, beta_j = g_j + lam_j mu_j; Phi = A diag(lam) A^T, b = A beta; Lambda~ = I + k Phi,
eta~ = sqrt(k) b; Lambda <- (1 - rho) Lambda + rho Lambda~, eta likewise.  ELBO = sum_j l_j - KL(q || N(0, I)).
Likelihood ids: 0 Gaussian(param = variance), 1 Bernoulli (logit), 2 Poisson (exp)."""
import math

import numpy as np

import optimal_q_ref as R

GAUSSIAN, BERNOULLI, POISSON = 0, 1, 2
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def gh(n=20):
    """Gauss-Hermite nodes x_i and weights w_i / sqrt(pi): E_{N(mu, v)} h(f) ~ sum_i w_i h(mu + sqrt(2 v) x_i)."""
    x, w = np.polynomial.hermite.hermgauss(n)
    return x, w / np.sqrt(np.pi)


def _sig_pair(f):
    """(sigmoid(f), sigmoid(-f)) from e = exp(-|f|): no 1 - sigmoid, the tails keep their digits."""
    e = np.exp(-np.abs(f))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(f >= 0, big, small), np.where(f >= 0, small, big), e


def sites(lik, y, mu, v, param=1.0, nodes=20):
    """(l [N], lam [N], beta [N], g [N]) in float64 for f_j ~ N(mu_j, v_j)."""
    y, mu, v = (np.asarray(a, np.float64).reshape(-1) for a in (y, mu, v))
    if lik == GAUSSIAN:
        l = -0.5 * np.log(2 * np.pi * param) - ((y - mu) ** 2 + v) / (2 * param)
        lam = np.full_like(mu, 1.0 / param)
        g = (y - mu) / param
        return l, lam, y / param, g
    if lik == BERNOULLI:
        x, w = gh(nodes)
        f = mu[:, None] + np.sqrt(2.0 * v)[:, None] * x[None, :]
        sp, sn, e = _sig_pair(f)
        softplus = np.maximum(f, 0.0) + np.log1p(e)
        l = ((y[:, None] * f - softplus) * w).sum(1)
        g = ((y[:, None] * sn - (1.0 - y[:, None]) * sp) * w).sum(1)
        lam = ((sp * sn) * w).sum(1)
        return l, lam, g + lam * mu, g
    if lik == POISSON:
        e = np.exp(mu + 0.5 * v)
        l = y * mu - e - _lgamma(y + 1.0)
        g = y - e
        return l, e, g + e * mu, g
    raise ValueError(lik)


def predict_y(lik, mu, v, param=1.0, nodes=20):
    """Mean and variance of a new y given f ~ N(mu, v)."""
    mu, v = np.asarray(mu, np.float64), np.asarray(v, np.float64)
    if lik == GAUSSIAN:
        return mu.copy(), v + param
    if lik == BERNOULLI:
        x, w = gh(nodes)
        sp, sn, _ = _sig_pair(mu[..., None] + np.sqrt(2.0 * v)[..., None] * x)
        return (sp * w).sum(-1), (sp * w).sum(-1) * (sn * w).sum(-1)      # p (1 - p), 1 - p = E sigmoid(-f) summed on its own
    e = np.exp(mu + 0.5 * v)
    return e, e + np.expm1(v) * e * e


def wstats_from_W(X, w, r, z, ell, W, dtype=np.float64, chunk=32768, ksplit=None):
    """(Phi_w = A diag(w) A^T, b = (A r)^T [1, M], tr Phi_w) as float64 for a given W = Lm^-1, the way
    optimal_q_ref.stats_from_W forms Phi and b: float32 means inputs rounded, A and A diag(w) formed in float32, the
    products taken in float32 over column blocks, the block results summed in float64."""
    X, z, ell, W = (np.asarray(a, dtype=dtype) for a in (X, z, ell, W))
    w, r = np.asarray(w, dtype=dtype).reshape(-1), np.asarray(r, dtype=dtype).reshape(-1)
    N, M = X.shape[0], z.shape[0]
    Phi, b = np.zeros((M, M)), np.zeros((1, M))
    step = N if dtype == np.float64 else min(chunk, ksplit or chunk)
    for j0 in range(0, N, step):
        A = R.A_of(W, z, X[j0:j0 + step], ell)
        Phi += (A @ (A * w[None, j0:j0 + step]).T).astype(np.float64)
        b += (A @ r[j0:j0 + step])[None, :].astype(np.float64)
    Phi = np.tril(Phi) + np.tril(Phi, -1).T
    return Phi, b, float(np.trace(Phi))


def marginals(m, S, A, k_var, residual="diagonal"):
    """(mu [N], v [N]) in the dtype of A (m, S are rounded to it)."""
    dt = A.dtype
    m, S = np.asarray(m, dt).reshape(-1), np.asarray(S, dt)
    r = np.abs(dt.type(1.0) - (A * A).sum(0)) if residual == "diagonal" else np.zeros(A.shape[1], dt)
    mean = m @ A
    var = ((S.T @ A) ** 2).sum(0) + r
    return np.sqrt(k_var) * mean.astype(np.float64), k_var * var.astype(np.float64)


def tail(Lam, eta):
    """(m [1, M], S lower with positive diagonal, Sigma, log|Lambda|)."""
    Sig = np.linalg.inv(Lam)
    Sig = 0.5 * (Sig + Sig.T)
    return (Sig @ eta.reshape(-1))[None, :], np.linalg.cholesky(Sig), Sig, np.linalg.slogdet(Lam)[1]


def elbo(m, S, A, y, lik, param=1.0, k_var=1.0, residual="diagonal", nodes=20):
    """sum_j E_q log p(y_j | f_j) - KL(q || N(0, I)) for ANY q(u) = N(m, S S^T), term by term."""
    M = A.shape[0]
    mu, v = marginals(m, S, A, k_var, residual)
    Sig = S @ S.T
    m = np.reshape(m, -1)
    kl = 0.5 * (np.trace(Sig) + m @ m - M - np.linalg.slogdet(Sig)[1])
    return float(sites(lik, y, mu, v, param, nodes)[0].sum() - kl)


def natgrad(X, y, z, ell, jitter, lik, param=1.0, k_var=1.0, residual="diagonal", q0=None, steps=20, rho=1.0, tol=1e-8,
            dtype=np.float64, W=None, ksplit=None):
    """(m [1, M], S, info): info = dict(elbo, residual, steps, marginals = [(mu, v) at every iterate]).  dtype float32:
    A, the marginals and the weighted products in float32 (lam, beta rounded to float32), the tail in float64, for a
    given float32 W."""
    z64, ell64 = np.asarray(z, np.float64), np.asarray(ell, np.float64)
    if W is None:
        _, W = R.chol_factor(z64, ell64, jitter)
    M = z64.shape[0]
    A = R.A_of(*(np.asarray(a, dtype) for a in (W, z, X, ell)))
    if q0 is None:
        Lam, eta = np.eye(M), np.zeros(M)
    else:
        S0 = np.asarray(q0[1], np.float64)
        Lam = np.linalg.inv(S0 @ S0.T)
        eta = Lam @ np.reshape(q0[0], -1)
    out = dict(elbo=[], residual=[], marginals=[])
    for it in range(steps + 1):
        m, S, Sig, logdet = tail(Lam, eta)
        mu, v = marginals(m, S, A, k_var, residual)
        l, lam, beta, _ = sites(lik, y, mu, v, param)
        lam, beta = lam.astype(dtype), beta.astype(dtype)
        Phi, b, _ = wstats_from_W(X, lam, beta, z, ell, W, dtype=dtype, ksplit=ksplit)
        Lt, et = np.eye(M) + k_var * Phi, np.sqrt(k_var) * b.reshape(-1)
        out["elbo"].append(float(l.sum() - 0.5 * (np.trace(Sig) + m.reshape(-1) @ m.reshape(-1) - M + logdet)))
        out["residual"].append(float(np.abs(Lam - Lt).max() / np.abs(Lt).max()))
        out["marginals"].append((mu, v))
        if it == steps or (it > 0 and abs(out["elbo"][-1] - out["elbo"][-2]) <= tol * abs(out["elbo"][-1])):
            break
        Lam, eta = (1 - rho) * Lam + rho * Lt, (1 - rho) * eta + rho * et
    out["elbo"], out["residual"], out["steps"] = np.asarray(out["elbo"]), np.asarray(out["residual"]), it
    return m, S, out


# ---------------------------------------------------------------------------------------- the inputs of the tests
ELL, K_VAR, JITTER = np.array([0.9]), 1.3, 1e-5


def problem(lik, N=3000, M=32, seed=0):
    """(X [N, 1], y [N, 1], Z [M, 1]): svgp_data's X and Z, latent 1.5 sin X, labels drawn with a fixed seed."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 0.5 * M, (N, 1))
    Z = np.linspace(0, 0.5 * M, M)[:, None]
    f = 1.5 * np.sin(X)
    lab = np.random.RandomState(1234 + lik)
    if lik == BERNOULLI:
        y = (lab.uniform(size=f.shape) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64)
    elif lik == POISSON:
        y = lab.poisson(np.exp(f)).astype(np.float64)
    else:
        y = f + 0.3 * lab.randn(*f.shape)
    return X, y, Z


def stats_case(N, M, d, seed):
    """(X, w, r, Y, z, ell, W) for the kernel tests: a mixed-sign w with exact zeros."""
    rng = np.random.RandomState(seed)
    dom = 0.5 * M if d == 1 else 4.0
    X = rng.uniform(0, dom, (N, d))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.3 * rng.randn(N, 1)
    w = rng.randn(N)
    w[rng.uniform(size=N) < 0.1] = 0.0
    if N > 3:
        w[:2] = (-1.5, 0.0)
    r = rng.randn(N)
    z = np.linspace(0, dom, M)[:, None] if d == 1 else rng.uniform(0, dom, (M, d))
    ell = np.ones(1) if d == 1 else np.array([0.9, 1.1, 1.3])
    _, W = R.chol_factor(z, ell, 1e-5 if d == 1 else 1e-3)
    return X, w, r, Y, z, ell, W
