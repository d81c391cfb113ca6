"""Numpy restatement of the likelihoods with a parameter of their own (HB_LIK_LAPLACE = 16, _GAMMA = 17, _NEGBINOMIAL = 18,
_BINOMIAL = 19), built on tests/sites_ref.py, which keeps ids 0..2: sites, d l / d param, predictive moments, predictive
log density, the natural-gradient iteration and the loop that learns the parameter.  float64 throughout.  Every function
takes any id, the three of sites_ref included.  tests/test_lik_zoo_cpu.py pins this file against adaptive quadrature and
torch autograd (the `l_torch` twin below); tests/test_lik_zoo_gpu.py holds the kernels and the models to it.

Under f ~ N(mu, v), delta = mu - y:
  Laplace(b)    A = E|y - f| = sqrt(2v/pi) exp(-delta^2/2v) + delta erf(delta/sqrt(2v)); l = -log 2b - A/b,
                g = erf((y - mu)/sqrt(2v))/b, lam = (2/b) N(y; mu, v), dl/db = -1/b + A/b^2             (closed form)
  Gamma(a)      E = exp(-mu + v/2); l = a log a - lgamma a + (a-1) log y - a mu - a y E, g = -a + a y E, lam = a y E,
                dl/da = log a + 1 - psi(a) + log y - mu - y E                                             (closed form)
  NegBin(r)     t = f - log r; log p = lgamma(y+r) - lgamma r - lgamma(y+1) + y t - (y+r) softplus t      (Gauss-Hermite)
  Binomial(n)   log p = lgamma(n+1) - lgamma(y+1) - lgamma(n-y+1) + y f - n softplus f                    (Gauss-Hermite)"""
import numpy as np
import scipy.special as sp

import optimal_q_ref as R
import sites_ref as SR

GAUSSIAN, BERNOULLI, POISSON = SR.GAUSSIAN, SR.BERNOULLI, SR.POISSON
LAPLACE, GAMMA, NEGBINOMIAL, BINOMIAL = 16, 17, 18, 19
NEW = (LAPLACE, GAMMA, NEGBINOMIAL, BINOMIAL)
TRAINABLE = (GAUSSIAN, LAPLACE, GAMMA, NEGBINOMIAL)
QUADRATURE = (NEGBINOMIAL, BINOMIAL)
NAMES = {GAUSSIAN: "gaussian", BERNOULLI: "bernoulli", POISSON: "poisson", LAPLACE: "laplace", GAMMA: "gamma",
         NEGBINOMIAL: "negbinomial", BINOMIAL: "binomial"}


def _flat(*arrays):
    return tuple(np.asarray(a, np.float64).reshape(-1) for a in arrays)


def _laplace_moments(y, mu, v):
    """(A = E|y - f|, erf(delta / sqrt(2v)), N(y; mu, v)); v = 0: (|delta|, sign(delta), 0)."""
    d = mu - y
    pos = v > 0
    vs = np.where(pos, v, 1.0)
    s = np.sqrt(2.0 * vs)
    ex = np.exp(-(d * d) / (2.0 * vs))
    er = sp.erf(d / s)
    return (np.where(pos, s * ex / np.sqrt(np.pi) + d * er, np.abs(d)), np.where(pos, er, np.sign(d)),
            np.where(pos, ex / (s * np.sqrt(np.pi)), 0.0))


def _quad_parts(lik, y, mu, v, param, nodes):
    """The node sums the two Gauss-Hermite likelihoods share: log p = c + y t - n softplus(t), t = f - shift."""
    nb = lik == NEGBINOMIAL
    shift = np.log(param) if nb else 0.0
    n = y + param if nb else np.full_like(y, param)
    neg = np.full_like(y, param) if nb else param - y
    x, w = SR.gh(nodes)
    t = (mu - shift)[:, None] + np.sqrt(2.0 * v)[:, None] * x[None, :]
    s_pos, s_neg, e = SR._sig_pair(t)
    softplus, softminus = np.maximum(t, 0.0) + np.log1p(e), np.maximum(-t, 0.0) + np.log1p(e)
    if nb:
        c = sp.gammaln(y + param) - sp.gammaln(param) - sp.gammaln(y + 1.0)
    else:
        c = sp.gammaln(param + 1.0) - sp.gammaln(y + 1.0) - sp.gammaln(param - y + 1.0)
    return dict(c=c, n=n, neg=neg, t=t, w=w, sp=s_pos, sn=s_neg, softplus=softplus, softminus=softminus)


def site_terms(lik, y, mu, v, param=1.0, nodes=20):
    """dict(l, g, lam, dl) [N] of the site under f_j ~ N(mu_j, v_j) and l_mag, g_mag, dl_mag, the sums of the magnitudes
    of the terms l, g and dl are added from (what a relative error of them is measured against).  dl = d l / d param
    (zeros where the parameter is not continuous)."""
    y, mu, v = _flat(y, mu, v)
    if lik in (GAUSSIAN, BERNOULLI, POISSON):
        l, lam, _, g = SR.sites(lik, y, mu, v, param, nodes)
        out = dict(l=l, g=g, lam=lam, dl=np.zeros_like(l), l_mag=np.abs(l), g_mag=np.abs(g), dl_mag=np.ones_like(l))
        if lik == GAUSSIAN:
            q = ((y - mu) ** 2 + v) / (2.0 * param ** 2)
            out.update(dl=-1.0 / (2.0 * param) + q, dl_mag=1.0 / (2.0 * param) + q)
        return out
    if lik == LAPLACE:
        A, er, dens = _laplace_moments(y, mu, v)
        return dict(l=-np.log(2.0 * param) - A / param, g=-er / param, lam=2.0 * dens / param,
                    dl=-1.0 / param + A / param ** 2, l_mag=np.abs(np.log(2.0 * param)) + A / param,
                    g_mag=np.full_like(y, 1.0 / param), dl_mag=1.0 / param + A / param ** 2)
    if lik == GAMMA:
        a = param
        yE, ly = y * np.exp(-mu + 0.5 * v), np.log(y)
        return dict(l=a * np.log(a) - sp.gammaln(a) + (a - 1.0) * ly - a * mu - a * yE, g=-a + a * yE, lam=a * yE,
                    dl=np.log(a) + 1.0 - sp.digamma(a) + ly - mu - yE,
                    l_mag=abs(a * np.log(a)) + abs(sp.gammaln(a)) + np.abs((a - 1.0) * ly) + np.abs(a * mu) + a * yE,
                    g_mag=a + a * yE, dl_mag=abs(np.log(a)) + 1.0 + abs(sp.digamma(a)) + np.abs(ly) + np.abs(mu) + yE)
    if lik in QUADRATURE:
        q = _quad_parts(lik, y, mu, v, param, nodes)
        w, n, neg, t = q["w"], q["n"][:, None], q["neg"][:, None], q["t"]
        # y t - n softplus(t) = -y softplus(-t) - (n - y) softplus(t): summed in the second form, whose terms share a sign
        sl = -((y[:, None] * q["softminus"] + neg * q["softplus"]) * w).sum(1)
        g = ((y[:, None] * q["sn"] - neg * q["sp"]) * w).sum(1)
        sh = ((q["sp"] * q["sn"]) * w).sum(1)
        out = dict(l=q["c"] + sl, g=g, lam=q["n"] * sh, dl=np.zeros_like(g), dl_mag=np.ones_like(g),
                   l_mag=np.abs(q["c"]) + np.abs(sl),
                   g_mag=((y[:, None] * q["sn"] + neg * q["sp"]) * w).sum(1))
        if lik == NEGBINOMIAL:
            r = param
            ssp, ssg = (q["softplus"] * w).sum(1), (q["sp"] * w).sum(1)
            out["dl"] = sp.digamma(y + r) - sp.digamma(r) - y / r - ssp + (q["n"] / r) * ssg
            out["dl_mag"] = np.abs(sp.digamma(y + r)) + abs(sp.digamma(r)) + y / r + ssp + (q["n"] / r) * ssg
        return out
    raise ValueError(lik)


def sites(lik, y, mu, v, param=1.0, nodes=20):
    """(l [N], lam [N], beta [N], g [N]) as sites_ref.sites returns them, for any id."""
    y, mu, v = _flat(y, mu, v)
    s = site_terms(lik, y, mu, v, param, nodes)
    return s["l"], s["lam"], s["g"] + s["lam"] * mu, s["g"]


def predict_y(lik, mu, v, param=1.0, nodes=20):
    """Mean and variance of a new y given f ~ N(mu, v)."""
    mu, v = np.asarray(mu, np.float64), np.asarray(v, np.float64)
    if lik in (GAUSSIAN, BERNOULLI, POISSON):
        return SR.predict_y(lik, mu, v, param, nodes)
    if lik == LAPLACE:
        return mu.copy(), v + 2.0 * param ** 2
    if lik == BINOMIAL:
        x, w = SR.gh(nodes)
        s_pos, s_neg, _ = SR._sig_pair(mu[..., None] + np.sqrt(2.0 * v)[..., None] * x)
        p = (s_pos * w).sum(-1)
        return param * p, param * (s_pos * s_neg * w).sum(-1) + param ** 2 * ((s_pos - p[..., None]) ** 2 * w).sum(-1)
    e = np.exp(mu + 0.5 * v)
    over = np.expm1(v) + np.exp(v) / param
    return e, e * e * over if lik == GAMMA else e + e * e * over


def log_p(lik, y, f, param=1.0):
    """log p(y | f) itself (y [N] or [N, 1] against f [N] or [N, nodes])."""
    if lik == GAUSSIAN:
        return -0.5 * np.log(2 * np.pi * param) - (y - f) ** 2 / (2 * param)
    if lik == BERNOULLI:
        return y * f - np.logaddexp(0.0, f)
    if lik == POISSON:
        return y * f - np.exp(f) - sp.gammaln(y + 1.0)
    if lik == LAPLACE:
        return -np.log(2.0 * param) - np.abs(y - f) / param
    if lik == GAMMA:
        a = param
        return a * np.log(a) - sp.gammaln(a) + (a - 1.0) * np.log(y) - a * f - a * y * np.exp(-f)
    if lik == NEGBINOMIAL:
        r, t = param, f - np.log(param)
        return sp.gammaln(y + r) - sp.gammaln(r) - sp.gammaln(y + 1.0) + y * t - (y + r) * np.logaddexp(0.0, t)
    if lik == BINOMIAL:
        n = param
        return sp.gammaln(n + 1.0) - sp.gammaln(y + 1.0) - sp.gammaln(n - y + 1.0) + y * f - n * np.logaddexp(0.0, f)
    raise ValueError(lik)


def logdens(lik, y, mu, v, param=1.0, nodes=20):
    """log integral p(y_j | f) N(f; mu_j, v_j) df [N]: closed form for Gaussian and Laplace (in log space through erfcx),
    the Gauss-Hermite rule over p(y | f_i) combined by log-sum-exp for the others (log_p above is NOT used: it is the plain
    formula the quadrature tests integrate, this is the tail-safe form the kernel takes)."""
    y, mu, v = _flat(y, mu, v)
    if lik == GAUSSIAN:
        return -0.5 * np.log(2 * np.pi * (v + param)) - (y - mu) ** 2 / (2 * (v + param))
    if lik == LAPLACE:
        b, d = param, y - mu
        pos = v > 0
        vs = np.where(pos, v, 1.0)
        s, q, c = np.sqrt(2.0 * vs), d * d / (2.0 * vs), vs / (2.0 * b * b)
        z1, z2 = (vs / b - d) / s, (vs / b + d) / s
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            t1 = np.where(z1 >= 0, -q + np.log(sp.erfcx(np.maximum(z1, 0.0))), c - d / b + np.log(sp.erfc(np.minimum(z1, 0.0))))
            t2 = np.where(z2 >= 0, -q + np.log(sp.erfcx(np.maximum(z2, 0.0))), c + d / b + np.log(sp.erfc(np.minimum(z2, 0.0))))
        top = np.maximum(t1, t2)
        return np.where(pos, -np.log(4.0 * b) + top + np.log(np.exp(t1 - top) + np.exp(t2 - top)),
                        -np.log(2.0 * b) - np.abs(d) / b)
    x, w = SR.gh(nodes)
    yy = y[:, None]
    shift = np.log(param) if lik == NEGBINOMIAL else 0.0
    t = (mu - shift)[:, None] + np.sqrt(2.0 * v)[:, None] * x[None, :]
    if lik in (BERNOULLI, NEGBINOMIAL, BINOMIAL):
        # log p - c = -y softplus(-t) - (n - y) softplus(t): terms of one sign (y t - n softplus(t) cancels in the tails)
        neg = {BERNOULLI: 1.0 - yy, NEGBINOMIAL: param, BINOMIAL: param - yy}[lik]
        l1pe = np.log1p(np.exp(-np.abs(t)))
        lp = -(yy * (np.maximum(-t, 0.0) + l1pe) + neg * (np.maximum(t, 0.0) + l1pe))
        c = {BERNOULLI: 0.0, NEGBINOMIAL: sp.gammaln(y + param) - sp.gammaln(param) - sp.gammaln(y + 1.0),
             BINOMIAL: sp.gammaln(param + 1.0) - sp.gammaln(y + 1.0) - sp.gammaln(param - y + 1.0)}[lik]
    elif lik == POISSON:
        lp, c = yy * t - np.exp(t), -sp.gammaln(y + 1.0)
    else:
        a = param
        lp, c = -a * t - a * yy * np.exp(-t), a * np.log(a) - sp.gammaln(a) + (a - 1.0) * np.log(y)
    top = lp.max(1)
    # c + top + log S, S = sum_i w_i exp(lp_i - top).  S > 1/2: log1p(sum_i w_i expm1(lp_i - top)), every term <= 0, so a
    # result near 0 keeps its digits; S small (one far node carries it): that sum is 1 - (nearly 1), log S directly
    d = lp - top[:, None]
    S, S1 = (np.exp(d) * w).sum(1), (np.expm1(d) * w).sum(1)
    return c + top + np.where(S > 0.5, np.log1p(np.where(S > 0.5, S1, 0.0)), np.log(S))


# ------------------------------------------------------------------------------------- the torch twin, for autograd
def l_torch(lik, y, mu, v, param, nodes=20):
    """l = E log p as a differentiable float64 torch expression of mu, v, param (tensors): the same formulas as
    site_terms, so torch.autograd gives dl/dmu (= g), dl/dv (= -lam / 2) and dl/dparam to compare against."""
    import torch

    if lik == GAUSSIAN:
        return -0.5 * torch.log(2 * np.pi * param) - ((y - mu) ** 2 + v) / (2 * param)
    if lik == LAPLACE:
        d = mu - y
        A = torch.sqrt(2 * v / np.pi) * torch.exp(-d * d / (2 * v)) + d * torch.erf(d / torch.sqrt(2 * v))
        return -torch.log(2 * param) - A / param
    if lik == GAMMA:
        a = param
        return a * torch.log(a) - torch.lgamma(a) + (a - 1) * torch.log(y) - a * mu - a * y * torch.exp(-mu + v / 2)
    x, w = (torch.as_tensor(a) for a in SR.gh(nodes))
    f = mu[:, None] + torch.sqrt(2 * v)[:, None] * x[None, :]
    softplus = torch.nn.functional.softplus
    if lik == NEGBINOMIAL:
        r, t = param, f - torch.log(param)
        lp = (torch.lgamma(y + r) - torch.lgamma(r) - torch.lgamma(y + 1))[:, None] + y[:, None] * t - (y + r)[:, None] * softplus(t)
    elif lik == BINOMIAL:
        n = param
        lp = (torch.lgamma(n + 1) - torch.lgamma(y + 1) - torch.lgamma(n - y + 1))[:, None] + y[:, None] * f - n * softplus(f)
    else:
        raise ValueError(lik)
    return (lp * w).sum(1)


# ------------------------------------------------------------------------------------- the iteration and the learning loop
def natgrad(X, y, z, ell, jitter, lik, param=1.0, k_var=1.0, q0=None, steps=20, rho=1.0, tol=1e-8):
    """sites_ref.natgrad (float64, residual 'diagonal') with the sites of this file: (m [1, M], S, info), info as there."""
    z, ell = np.asarray(z, np.float64), np.asarray(ell, np.float64)
    _, W = R.chol_factor(z, ell, jitter)
    M = z.shape[0]
    A = R.A_of(W, z, np.asarray(X, np.float64), ell)
    if q0 is None:
        Lam, eta = np.eye(M), np.zeros(M)
    else:
        S0 = np.asarray(q0[1], np.float64)
        Lam = np.linalg.inv(S0 @ S0.T)
        eta = Lam @ np.reshape(q0[0], -1)
    out = dict(elbo=[], residual=[], marginals=[])
    for it in range(steps + 1):
        m, S, Sig, logdet = SR.tail(Lam, eta)
        mu, v = SR.marginals(m, S, A, k_var)
        l, lam, beta, _ = sites(lik, y, mu, v, param)
        Phi, b, _ = SR.wstats_from_W(X, lam, beta, z, ell, W)
        Lt, et = np.eye(M) + k_var * Phi, np.sqrt(k_var) * b.reshape(-1)
        out["elbo"].append(float(l.sum() - 0.5 * (np.trace(Sig) + m.reshape(-1) @ m.reshape(-1) - M + logdet)))
        out["residual"].append(float(np.abs(Lam - Lt).max() / np.abs(Lt).max()))
        out["marginals"].append((mu, v))
        if it == steps or (it > 0 and abs(out["elbo"][-1] - out["elbo"][-2]) <= tol * abs(out["elbo"][-1])):
            break
        Lam, eta = (1 - rho) * Lam + rho * Lt, (1 - rho) * eta + rho * et
    out["elbo"], out["residual"], out["steps"] = np.asarray(out["elbo"]), np.asarray(out["residual"]), it
    return m, S, out


def marginals_of(X, z, ell, jitter, m, S, k_var):
    """(mu [N], v [N]) of f under q(u) = N(m, S S^T), residual 'diagonal'."""
    z, ell = np.asarray(z, np.float64), np.asarray(ell, np.float64)
    _, W = R.chol_factor(z, ell, jitter)
    return SR.marginals(m, S, R.A_of(W, z, np.asarray(X, np.float64), ell), k_var)


def learn(X, y, z, ell, jitter, lik, theta0, k_var=1.0, steps=30, lr=0.05, q_steps=5, rho=1.0):
    """The learning loop in the restatement alone: every outer step runs q_steps natural-gradient steps from the current
    q (the first from the prior), then one Adam ASCENT step on log theta with the restated gradient theta sum_j dl_j/dtheta at
    that q; a closing fit (20 steps, tol 1e-8) at the final theta.  Returns (theta trace [steps + 1], ELBO trace [steps + 1])."""
    log_t, m1, m2 = np.log(theta0), 0.0, 0.0
    q, thetas, elbos = None, [], []
    for t in range(steps + 1):
        last = t == steps
        m, S, info = natgrad(X, y, z, ell, jitter, lik, np.exp(log_t), k_var, q0=q, steps=20 if last else q_steps, rho=rho,
                             tol=1e-8 if last else 0.0)
        q = (m, S)
        thetas.append(float(np.exp(log_t)))
        elbos.append(float(info["elbo"][-1]))
        if last:
            break
        mu, v = info["marginals"][-1]
        grad = np.exp(log_t) * site_terms(lik, y, mu, v, np.exp(log_t))["dl"].sum()
        m1, m2 = 0.9 * m1 + 0.1 * grad, 0.999 * m2 + 0.001 * grad ** 2
        log_t += lr * (m1 / (1 - 0.9 ** (t + 1))) / (np.sqrt(m2 / (1 - 0.999 ** (t + 1))) + 1e-8)
    return np.asarray(thetas), np.asarray(elbos)


# ------------------------------------------------------------------------------------- the inputs of the tests
ELL, K_VAR, JITTER = SR.ELL, SR.K_VAR, SR.JITTER
THETA_STAR = {LAPLACE: 0.3, GAMMA: 4.0, NEGBINOMIAL: 2.0, GAUSSIAN: 0.09}
RHO = {LAPLACE: 0.25}   # likelihoods.Laplace.natgrad_rho: the damping its iteration needs (1 for every other likelihood)
PARAM = {LAPLACE: 0.3, GAMMA: 4.0, NEGBINOMIAL: 2.0, BINOMIAL: 12.0, GAUSSIAN: 0.09}   # what the model tests fit with
# ... except the test that follows the UNDAMPED iteration (rho = 1 and 0.5) step by step: at the Laplace scale 0.3 that
# iteration diverges and the restatement itself is not reproducible to the 1e-8 the test asks (a one-ulp change of the
# labels moves its residual trace by 9.5e-7 at rho = 1); at scale 1 it converges at both rho and moves by 5e-14
# (tests/test_lik_zoo_cpu.py holds every case of that test to 1e-10 under such a change)
NATGRAD_PARAM = dict(PARAM)
NATGRAD_PARAM[LAPLACE] = 1.0


def draw(lik, f, param, rng):
    """Labels from the likelihood at the latent values f."""
    if lik == GAUSSIAN:
        return f + np.sqrt(param) * rng.randn(*f.shape)
    if lik == BERNOULLI:
        return (rng.uniform(size=f.shape) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64)
    if lik == POISSON:
        return rng.poisson(np.exp(f)).astype(np.float64)
    if lik == LAPLACE:
        return f + rng.laplace(0.0, param, f.shape)
    if lik == GAMMA:
        return rng.gamma(param, np.exp(f) / param)
    if lik == NEGBINOMIAL:
        return rng.negative_binomial(param, param / (param + np.exp(f))).astype(np.float64)
    if lik == BINOMIAL:
        return rng.binomial(int(param), 1.0 / (1.0 + np.exp(-f))).astype(np.float64)
    raise ValueError(lik)


def problem(lik, param=None, N=3000, M=32, seed=0):
    """(X [N, 1], y [N, 1], Z [M, 1]): sites_ref.problem's X, Z and latent 1.5 sin X, labels drawn from the likelihood
    with `param` (default PARAM[lik]) and a fixed seed."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 0.5 * M, (N, 1))
    Z = np.linspace(0, 0.5 * M, M)[:, None]
    y = draw(lik, 1.5 * np.sin(X), PARAM[lik] if param is None else param, np.random.RandomState(1234 + lik))
    return X, y, Z


def site_inputs(lik, N, seed, param):
    """(y, mu, v) as tests/test_sites_gpu.py builds them: mu = 2 randn, v = exp(U(-6, 1)), the corners mu = +-30,
    v in {1e-12, 25} in front (as many as fit), y drawn from the likelihood at clip(mu, -3, 3); the last count is 1000
    (the binomial's: its total count, so `param` must be >= it there), the last Gamma y 1e-6."""
    rng = np.random.RandomState(seed)
    mu, v = 2.0 * rng.randn(N), np.exp(rng.uniform(-6, 1, N))
    for i, (a, c) in enumerate([(30.0, 25.0), (-30.0, 1e-12), (30.0, 1e-12), (-30.0, 25.0)][:N]):
        mu[i], v[i] = a, c
    if lik == BERNOULLI:
        y = (rng.uniform(size=N) < 0.5).astype(np.float64)
    else:
        y = draw(lik, np.clip(mu, -3, 3), param, rng)
    if lik in (POISSON, NEGBINOMIAL):
        y[-1] = 1000.0
    if lik == BINOMIAL:
        y[-1] = param
    if lik == GAMMA:
        y[-1] = 1e-6
    return y, mu, v
