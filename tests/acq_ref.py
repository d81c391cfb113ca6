"""Numpy restatement of the input gradients of the sparse GP's closed-form predictive and of the closed-form acquisition
functions on them (hb_sgp_predict_grad, hb_sgp_acq), for one expert, one latent function and the UnitRBF kernel.  With
K_kj = k(z_k, x_j), t_kjd = (z_kd - x_jd) / ell_d^2 (so dK_kj / dx_jd = K_kj t_kjd), A = W K and C = S^T A:

    mean_j = m A_j                      dmean_jd = sum_k alpha_k K_kj t_kjd,   alpha = W^T m^T
    var_j  = ||C_j||^2 + r_j            dvar_jd  = 2 sum_k G_kj K_kj t_kjd,    G = W^T (S C - A diag rho)
    r_j = |1 - sum_m A_mj^2|, rho_j = sign(1 - sum_m A_mj^2)   ('diagonal')
    r_j = 0, rho_j = 0   ('neglected');     r_j = 1 - sum_m A_mj^2 + jitter, rho_j = 1   ('fullrank')

Acquisition tail (always float64), sc = sqrt(k_var), s = +1 (largest) or -1:  mu' = s sc mean, v = max(sc^2 var,
var_floor), sigma = sqrt(v), u = (mu' - s best - xi) / sigma, Phi(u) = erfc(-u / sqrt 2) / 2:

    EI  = sigma (u Phi + phi)     d/dmu' = Phi            d/dv = phi / (2 sigma)
    PI  = Phi                     d/dmu' = phi / sigma    d/dv = -u phi / (2 v)
    UCB = mu' + beta sigma        d/dmu' = 1              d/dv = beta / (2 sigma)
    grad_jd = s sc a_mu' dmean_jd + sc^2 a_v dvar_jd      (a_v = 0 where v was clamped)

float64 unless a dtype is asked for."""
import math

import numpy as np

import optimal_q_ref as OQ

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _parts(x, z, ell, W, m, S, mode, dtype):
    """(K, A, C, V, G, alpha, T [d, M, n], sa2) in `dtype`: every product taken, and every result held, in that type."""
    x, z, ell, W, m, S = (np.asarray(a, dtype=dtype) for a in (x, z, ell, W, m, S))
    m = m.reshape(-1)
    K = OQ.rbf(z, x, ell)
    A = W @ K
    sa2 = (A * A).sum(0)
    one = np.ones(1, dtype)[0]
    rho = {"diagonal": np.sign(one - sa2), "neglected": np.zeros_like(sa2), "fullrank": np.ones_like(sa2)}[mode]
    if S.ndim == 1:
        C = S[:, None] * A
        V = (S * S)[:, None] * A - rho[None, :] * A
    else:
        S = np.tril(S)
        C = S.T @ A
        V = S @ C - rho[None, :] * A
    G = W.T @ V
    alpha = W.T @ m
    d = x.shape[1]
    ellk = np.broadcast_to(ell, (d,)).astype(dtype)
    T = np.stack([(z[:, k][:, None] - x[:, k][None, :]) * (one / (ellk[k] * ellk[k])) for k in range(d)])
    return K, A, C, V, G, alpha, T, sa2, m


def moments_grad(x, z, ell, W, m, S, mode="diagonal", jitter=0.0, dtype=np.float64):
    """(mean [n], var [n], dmean [n, d], dvar [n, d]) as float64.  S [M, M] lower or the standard deviations s [M].
    dtype float32: the inputs rounded to float32, K, A, C, V, G rounded to float32 and every product and sum in float32."""
    K, A, C, V, G, alpha, T, sa2, m = _parts(x, z, ell, W, m, S, mode, dtype)
    one = np.ones(1, dtype)[0]
    r = {"diagonal": np.abs(one - sa2), "neglected": np.zeros_like(sa2), "fullrank": (one - sa2) + np.asarray(jitter, dtype)}[mode]
    mean = m @ A
    var = (C * C).sum(0) + r
    dmean = np.stack([((alpha[:, None] * K) * T[k]).sum(0) for k in range(T.shape[0])], axis=1)
    dvar = np.stack([(one + one) * ((G * K) * T[k]).sum(0) for k in range(T.shape[0])], axis=1)
    return tuple(np.asarray(a, np.float64) for a in (mean, var, dmean, dvar))


def predict_torch(x, z, ell, W, m, S, mode="diagonal", jitter=0.0):
    """(mean [n], var [n]) on torch tensors, written as optimal_q_ref.predict writes them (no derivative formula): what
    autograd differentiates to pin moments_grad."""
    import torch

    ellk = ell.expand(x.shape[1])
    r2 = (((z[:, None, :] - x[None, :, :]) / ellk) ** 2).sum(-1)
    A = W @ torch.exp(-0.5 * r2)
    Sm = torch.diag(S) if S.dim() == 1 else torch.tril(S)
    sa2 = (A * A).sum(0)
    r = {"diagonal": torch.abs(1.0 - sa2), "neglected": torch.zeros_like(sa2), "fullrank": 1.0 - sa2 + jitter}[mode]
    return m.reshape(-1) @ A, ((Sm.T @ A) ** 2).sum(0) + r


def grad_scale(x, z, ell, W, m, S, mode="diagonal"):
    """(scale of dmean [d], scale of dvar [d]): max_j sum_k |alpha_k K_kj t_kjd| and max_j 2 sum_k |G_kj K_kj t_kjd|, the
    absolute sums of the two folds, in float64."""
    K, A, C, V, G, alpha, T, sa2, m = _parts(x, z, ell, W, m, S, mode, np.float64)
    sm = np.array([np.abs((alpha[:, None] * K) * T[k]).sum(0).max() for k in range(T.shape[0])])
    sv = np.array([2.0 * np.abs((G * K) * T[k]).sum(0).max() for k in range(T.shape[0])])
    return sm, sv


def tail(kind, mean, var, best=0.0, param=0.0, sc=1.0, largest=True, var_floor=0.0):
    """(val, a_mu, a_v, clamped) of the acquisition `kind` ('ei', 'pi', 'ucb'; param = xi or beta) in float64."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    s, sc = (1.0 if largest else -1.0), float(sc)
    mu, vraw = s * sc * mean, (sc * sc) * var
    clamped = vraw < var_floor
    v = np.where(clamped, float(var_floor), vraw)
    sg = np.sqrt(v)
    if kind == "ucb":
        val, a_mu, a_v = mu + param * sg, np.ones_like(mu), param / (2.0 * sg)
    else:
        u = (mu - s * best - param) / sg
        Phi = 0.5 * _erfc(-u * 0.70710678118654752440)
        phi = 0.39894228040143267794 * np.exp(-0.5 * u * u)
        if kind == "ei":
            val, a_mu, a_v = sg * (u * Phi + phi), Phi, phi / (2.0 * sg)
        elif kind == "pi":
            val, a_mu, a_v = Phi, phi / sg, -u * phi / (2.0 * v)
        else:
            raise ValueError(kind)
    return val, a_mu, np.where(clamped, 0.0, a_v), clamped


def acquisition(kind, mean, var, dmean, dvar, best=0.0, param=0.0, sc=1.0, largest=True, var_floor=0.0):
    """(val [n], grad [n, d]) from the unscaled moments and their gradients (moments_grad)."""
    val, a_mu, a_v, _ = tail(kind, mean, var, best, param, sc, largest, var_floor)
    s = 1.0 if largest else -1.0
    grad = (s * sc * a_mu)[:, None] * np.asarray(dmean, np.float64) + (sc * sc * a_v)[:, None] * np.asarray(dvar, np.float64)
    return val, grad


def maximise(x, z, ell, W, m, S, kind, mode="diagonal", jitter=0.0, k_var=1.0, best=0.0, param=0.0, largest=True,
             var_floor=0.0, steps=50, lr=0.05, bounds=None, starts=None):
    """SparsePosterior.maximise in float64: (x_best [R, d], a_best [R], start_idx or None).  Projected Adam ascent (beta
    0.9 / 0.999, epsilon 1e-8) on the acquisition in u = x / ell from its best candidate among the rows of x (R = 1), or
    from the rows of `starts`; the best (value, point) seen is kept, the start and the last point included."""
    x, ell = np.asarray(x, np.float64), np.asarray(ell, np.float64)
    d = x.shape[1]
    ellk = np.broadcast_to(ell, (d,))
    sc = np.sqrt(k_var)

    def f_and_g(xc):
        return acquisition(kind, *moments_grad(xc, z, ell, W, m, S, mode, jitter), best, param, sc, largest, var_floor)

    lo, hi = (x.min(0), x.max(0)) if bounds is None else (np.asarray(b, np.float64) for b in bounds)
    idx = None
    if starts is None:
        F = f_and_g(x)[0]
        idx = int(np.argmax(F))
        xc = x[idx:idx + 1].copy()
    else:
        xc = np.asarray(starts, np.float64).copy()
    x_best, f_best = xc.copy(), f_and_g(xc)[0]
    u = xc / ellk
    m1, m2 = np.zeros_like(u), np.zeros_like(u)
    b1, b2, eps = 0.9, 0.999, 1e-8
    if steps:
        for t in range(steps + 1):
            f, g = f_and_g(xc)
            better = f > f_best
            x_best[better], f_best[better] = xc[better], f[better]
            if t == steps:
                break
            gu = ellk * g
            m1 = b1 * m1 + (1.0 - b1) * gu
            m2 = b2 * m2 + (1.0 - b2) * gu ** 2
            u = u + lr * (m1 / (1.0 - b1 ** (t + 1))) / (np.sqrt(m2 / (1.0 - b2 ** (t + 1))) + eps)
            u = np.clip(u, lo / ellk, hi / ellk)
            xc = np.clip(u * ellk, lo, hi)
            xc = np.where(u >= hi / ellk, hi, np.where(u <= lo / ellk, lo, xc))
    return x_best, f_best, idx


def case(n, M, d, dl=1, seed=0, wscale=1.0):
    """(x [n, d], z [M, d], ell [dl], W [M, M], m [M], S [M, M] generic lower, s [M] > 0, jitter) in float64, built like the
    statistics cases of the optimal-q tests: d = 1 puts z on a half-lengthscale grid with jitter 1e-5, d > 1 draws z
    uniformly in a box of 4 units with jitter 1e-3; m has mixed signs; wscale multiplies W (1.5: sum A^2 > 1 on most columns,
    so that rho = -1 is exercised)."""
    rng = np.random.RandomState(seed)
    dom = 0.5 * M if d == 1 else 4.0
    x = rng.uniform(0, dom, (n, d))
    z = np.linspace(0, dom, M)[:, None] if d == 1 else rng.uniform(0, dom, (M, d))
    ell = (np.ones(1) if d == 1 else np.array([1.1])) if dl == 1 else np.array([0.9, 1.1, 1.3, 1.0, 1.2])[:d]
    jitter = 1e-5 if d == 1 else 1e-3
    _, W = OQ.chol_factor(z, ell, jitter)
    m = rng.randn(M)
    S = np.tril(rng.randn(M, M)) * (0.4 / np.sqrt(M)) + 0.3 * np.eye(M)
    s = 0.2 + 0.6 * rng.uniform(size=M)
    return x, z, ell, wscale * W, m, S, s, jitter
