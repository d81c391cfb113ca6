"""Heteroscedastic Gaussian regression with two sparse GPs, restated in numpy float64 from the definitions: the
likelihood y ~ N(f, exp(g + c)) under independent Gaussian marginals of f and g (sites, predictive, the 20-node
predictive log density), the two-latent natural-gradient loop of SparseGP.natgrad_q for the whitened model, and the ELBO
as a function of (z, ell, k_var, c) at a fixed q, for finite differences.  Nothing here imports the package."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


# ------------------------------------------------------------------------------------------------ the likelihood
def sites(y, mean, var, c, mscale=1.0, vscale=1.0):
    """(lam [2, N], beta [2, N], r [2, N], l [N]) at the marginals mu = mscale mean, v = vscale var (rows: f, g)."""
    y, mean, var = (np.asarray(a, dtype=np.float64) for a in (y, mean, var))
    mf, mg, vf, vg = mscale * mean[0], mscale * mean[1], vscale * var[0], vscale * var[1]
    dy = y - mf
    s = dy * dy + vf
    with np.errstate(over="ignore"):
        e = np.exp(-mg - c + 0.5 * vg)
        hse = 0.5 * (s * e)
    lam = np.stack([e, hse])
    r = np.stack([dy * e, -0.5 + hse])
    beta = r + lam * np.stack([mf, mg])
    l = -0.5 * LOG_2PI - 0.5 * (mg + c) - hse
    return lam, beta, r, l


def expected_logdens(y, mf, vf, mg, vg, c):
    """l alone, at already scaled marginals (for central differences in mu and v)."""
    return -0.5 * LOG_2PI - 0.5 * (mg + c) - 0.5 * ((y - mf) ** 2 + vf) * np.exp(-mg - c + 0.5 * vg)


def predictive(mean, var, c):
    """(E y, var y) at already scaled marginals mean, var [2, n]."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return mean[0].copy(), var[0] + np.exp(mean[1] + c + 0.5 * var[1])


def logdens(y, mean, var, c, mscale=1.0, vscale=1.0, nodes=20):
    """log sum_i w_i N(y; mu_f, v_f + exp(mu_g + c + sqrt(2 v_g) x_i)) over the `nodes`-point Gauss-Hermite rule."""
    y, mean, var = (np.asarray(a, dtype=np.float64) for a in (y, mean, var))
    x, w = np.polynomial.hermite.hermgauss(nodes)
    w = w / np.sqrt(np.pi)
    mf, mg, vf, vg = mscale * mean[0], mscale * mean[1], vscale * var[0], vscale * var[1]
    tot = vf[None] + np.exp(mg[None] + c + np.sqrt(2.0 * vg)[None] * x[:, None])
    lp = -0.5 * np.log(2.0 * np.pi * tot) - (y - mf)[None] ** 2 / (2.0 * tot)
    top = lp.max(0)
    keep = w > 0.0                      # (the far weights of a 200-node rule underflow to zero)
    return top + np.log((w[keep, None] * np.exp(lp[keep] - top)).sum(0))


# ------------------------------------------------------------------------------------------------ the sparse GPs
def rbf(a, b, ell):
    d = (a[:, None, :] - b[None, :, :]) / np.asarray(ell, dtype=np.float64).reshape(1, 1, -1)
    return np.exp(-0.5 * (d * d).sum(-1))


def whitened(X, z, ell, jitter):
    """A = L^-1 K(z, X) [M, N], L = chol(K(z, z) + jitter I)."""
    L = np.linalg.cholesky(rbf(z, z, ell) + jitter * np.eye(len(z)))
    return np.linalg.solve(L, rbf(z, X, ell))


def marginals(A, m, S, residual):
    """Unit-variance mean, var [C, N] of C latent functions: m [C, M], S [C, M, M] lower (in the dtype of the operands)."""
    a2 = (A * A).sum(0)
    r = np.abs(A.dtype.type(1.0) - a2) if residual == "diagonal" else 0 * a2
    return m @ A, np.stack([((np.tril(Sc).T @ A) ** 2).sum(0) + r for Sc in S])


def kl(m, S):
    """sum_c KL(N(m_c, S_c S_c^T) || N(0, I))."""
    M = m.shape[1]
    return sum(0.5 * ((np.tril(Sc) ** 2).sum() + mc @ mc - M) - np.log(np.abs(np.diagonal(Sc))).sum() for mc, Sc in zip(m, S))


def elbo(X, y, z, ell, k_var, c, m, S, residual="diagonal", jitter=1e-5):
    """sum_j l_j - KL at the fixed q = (m [2, M], S [2, M, M])."""
    mean, var = marginals(whitened(X, np.asarray(z, dtype=np.float64), ell, jitter), m, S, residual)
    return sites(y, mean, var, c, np.sqrt(k_var), k_var)[3].sum() - kl(m, S)


def natgrad(X, y, z, ell, k_var, c, residual="diagonal", rho=0.5, steps=40, tol=1e-8, jitter=1e-5, q0=None,
            dtype=np.float64, W=None, ksplit=None):
    """The two-latent natural-gradient loop of SparseGP.natgrad_q: (m [2, M], S [2, M, M], dict(elbo, residual, steps)).
    W: a given Lm^-1 (None: from the definition).  dtype float32: the inputs rounded, A = W K, the marginals and the
    weighted products (over blocks of `ksplit` columns, summed in float64) in float32, lam and beta rounded to float32,
    the tails in float64 -- the arithmetic of a float32 session."""
    dt = np.dtype(dtype).type
    X, z, ell = (np.asarray(a, dtype=dt) for a in (X, z, ell))
    if W is None:
        W = np.linalg.inv(np.linalg.cholesky(rbf(z.astype(np.float64), z.astype(np.float64), ell) + jitter * np.eye(len(z))))
    d = (z[:, None, :] - X[None, :, :]) / ell.reshape(1, 1, -1)
    A = np.asarray(W, dtype=dt) @ np.exp(dt(-0.5) * (d * d).sum(-1))
    assert A.dtype == dt
    M, N = A.shape
    eye = np.eye(M)
    if q0 is None:
        Lam, eta = np.stack([eye, eye]), np.zeros((2, M))
    else:
        Lam = np.stack([np.linalg.inv(np.tril(Sc) @ np.tril(Sc).T) for Sc in q0[1]])
        eta = np.stack([L @ mc for L, mc in zip(Lam, q0[0])])
    step = N if dt is np.float64 else (ksplit or N)
    trace, resid = [], []
    for it in range(steps + 1):
        Sig = np.stack([np.linalg.inv(L) for L in Lam])
        Sig = 0.5 * (Sig + Sig.transpose(0, 2, 1))
        m = np.stack([Sg @ e for Sg, e in zip(Sig, eta)])
        S = np.stack([np.linalg.cholesky(Sg) for Sg in Sig])
        mean, var = marginals(A, m.astype(dt), S.astype(dt), residual)
        lam, beta, _, l = sites(y, mean.astype(np.float64), var.astype(np.float64), c, np.sqrt(k_var), k_var)
        lam, beta = lam.astype(dt), beta.astype(dt)
        Phi, b = np.zeros((2, M, M)), np.zeros((2, M))
        for j0 in range(0, N, step):
            Ab = A[:, j0:j0 + step]
            for k in range(2):
                Phi[k] += (Ab @ (Ab * lam[k, None, j0:j0 + step]).T).astype(np.float64)
                b[k] += (Ab @ beta[k, j0:j0 + step]).astype(np.float64)
        Lt, et = eye + k_var * Phi, np.sqrt(k_var) * b
        trace.append(l.sum() - kl(m, S))
        resid.append(max(np.abs(p - q).max() / np.abs(q).max() for p, q in zip(Lam, Lt)))
        if it == steps or (it > 0 and abs(trace[-1] - trace[-2]) <= tol * abs(trace[-1])):
            break
        Lam, eta = (1.0 - rho) * Lam + rho * Lt, (1.0 - rho) * eta + rho * et
    return m, S, dict(elbo=np.asarray(trace), residual=np.asarray(resid), steps=it)


def data(N, M, c, seed, d=1):
    """Inputs on [0, 10]^d, a smooth mean, and a noise standard deviation that is a sigmoid of the first coordinate
    scaled so that its log variance is centred near c: (X [N, d], Y [N, 1], Z [M, d], noise_sd [N])."""
    rs = np.random.RandomState(seed)
    X = np.sort(rs.uniform(0.0, 10.0, (N, d)), axis=0) if d == 1 else rs.uniform(0.0, 10.0, (N, d))
    sd = np.exp(0.5 * c) * (0.4 + 1.6 / (1.0 + np.exp(-(X[:, 0] - 5.0))))
    f = np.sin(X).sum(1)
    Y = (f + sd * rs.randn(N))[:, None]
    Z = np.linspace(0.0, 10.0, M)[:, None] if d == 1 else rs.uniform(0.0, 10.0, (M, d))
    return X, Y, Z, sd


def central(fun, x, h):
    """Central differences of the scalar fun at the array x, entry by entry."""
    x = np.array(x, dtype=np.float64)
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (fun(xp) - fun(xm)) / (2.0 * h)
    return g
