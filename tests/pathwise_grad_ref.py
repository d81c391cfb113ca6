"""Numpy restatement of the input gradient of pathwise function draws and of PathwiseDraws.maximise (hb_sgp_pathwise_grad,
hb_sgp_pathwise_argmax), on pathwise_ref.basis.  With p_lj = sum_k omega_lk x_jk / ell_k and B = pathwise_ref.basis(x):

    d f_s(x_j) / d x_jk = scale sum_row coef[s, row] E_k[row, j]
    E_k[2l] = -B[2l + 1] omega_lk / ell_k,   E_k[2l + 1] = B[2l] omega_lk / ell_k        (d cos = -sin dp, d sin = cos dp)
    E_k[2L + m] = B[2L + m] (z_mk - x_jk) / ell_k^2

float64 unless a dtype is asked for."""
import numpy as np

import pathwise_ref as PR


def operands(x, omega, z, ell):
    """E [d, 2L + M, n] in the dtype of x, formed from the value basis as the kernel forms it: the trig rows swapped and
    scaled by the signed omega_lk / ell_k, the RBF rows scaled by (z_mk - x_jk) (1 / ell_k^2)."""
    n, d = x.shape
    L = omega.shape[0]
    B = PR.basis(x, omega, z, ell)
    ellk = np.broadcast_to(ell, (d,)).astype(x.dtype)
    E = np.empty((d,) + B.shape, dtype=x.dtype)
    for k in range(d):
        q = (omega[:, k] * (np.ones(1, x.dtype)[0] / ellk[k]))[:, None]          # [L, 1]
        E[k, 0:2 * L:2] = B[1:2 * L:2] * (-q)
        E[k, 1:2 * L:2] = B[0:2 * L:2] * q
        if z is not None and z.shape[0]:
            ie2 = np.ones(1, x.dtype)[0] / (ellk[k] * ellk[k])
            E[k, 2 * L:] = B[2 * L:] * ((z[:, k][:, None] - x[:, k][None, :]) * ie2)
    return E


def grad(x, omega, z, ell, coef, scale=1.0, dtype=np.float64):
    """grad [S, n, d] = scale coef E_k as float64.  dtype float32: the inputs rounded to float32, the operands and the
    product formed in float32, the rows taken in blocks of pathwise_ref.KSTEP in the kernel's K order (the trig rows,
    the last block short, then the RBF rows) with the running sum kept in float32 -- as pathwise_ref.evaluate."""
    x, omega, ell, coef = (np.asarray(a, dtype=dtype) for a in (x, omega, ell, coef))
    z = None if z is None else np.asarray(z, dtype=dtype)
    E = operands(x, omega, z, ell)
    L, K = omega.shape[0], E.shape[1]
    acc = np.zeros((x.shape[1], coef.shape[0], x.shape[0]), dtype=dtype)
    for k0 in list(range(0, 2 * L, PR.KSTEP)) + list(range(2 * L, K, PR.KSTEP)):
        k1 = min(k0 + PR.KSTEP, 2 * L if k0 < 2 * L else K)
        acc = acc + np.matmul(coef[None, :, k0:k1], E[:, k0:k1])
    return np.transpose(np.asarray(scale, dtype=dtype) * acc, (1, 2, 0)).astype(np.float64)


def grad_scale(x, omega, z, ell, coef, scale=1.0):
    """[d]: scale max_s sum_row |coef[s, row]| g[row, k] with g = |omega_lk| / ell_k on the two trig rows of frequency l
    and e^-1/2 / ell_k on the RBF rows: a bound on every partial sum of derivative k, since |cos|, |sin| <= 1 and
    max_t |t e^(-t^2 / 2)| = e^-1/2."""
    omega, ell, coef = (np.asarray(a, np.float64) for a in (omega, ell, coef))
    L, d = omega.shape
    ellk = np.broadcast_to(ell, (d,))
    M = coef.shape[1] - 2 * L
    g = np.concatenate([np.repeat(np.abs(omega) / ellk, 2, axis=0), np.tile(np.exp(-0.5) / ellk, (M, 1))])   # [2L + M, d]
    return float(scale) * (np.abs(coef) @ g).max(0)


def maximise(x, omega, z, ell, coef, scale=1.0, steps=50, lr=0.05, bounds=None, largest=True):
    """PathwiseDraws.maximise in float64 on pathwise_ref.evaluate and grad above: (x_best [S, d], f_best [S], start_idx
    [S]).  Draw s starts at its best candidate among the rows of x; `steps` steps of Adam (beta 0.9 / 0.999, epsilon
    1e-8) in u = x / ell on sign ell d f / d x, each followed by the projection onto the box (default: the per-column
    minimum and maximum of the candidates); the best (value, point) seen is kept, the start and the last point included."""
    x, omega, ell, coef = (np.asarray(a, np.float64) for a in (x, omega, ell, coef))
    S, d = coef.shape[0], x.shape[1]
    ellk = np.broadcast_to(ell, (d,))
    sign = 1.0 if largest else -1.0
    lo, hi = (x.min(0), x.max(0)) if bounds is None else (np.asarray(b, np.float64) for b in bounds)
    F = PR.evaluate(x, omega, z, ell, coef, scale)
    idx = np.argmax(sign * F, axis=1)
    ar = np.arange(S)
    xc = x[idx].copy()
    x_best, f_best = xc.copy(), F[ar, idx].copy()
    u = xc / ellk
    m1, m2 = np.zeros_like(u), np.zeros_like(u)
    b1, b2, eps = 0.9, 0.999, 1e-8
    if steps:   # steps + 1 evaluations: the start (for its gradient) and the point after every step
        for t in range(steps + 1):
            f = PR.evaluate(xc, omega, z, ell, coef, scale)[ar, ar]
            g = grad(xc, omega, z, ell, coef, scale)[ar, ar]
            better = sign * f > sign * f_best
            x_best[better], f_best[better] = xc[better], f[better]
            if t == steps:
                break
            gu = sign * ellk * g
            m1 = b1 * m1 + (1.0 - b1) * gu
            m2 = b2 * m2 + (1.0 - b2) * gu ** 2
            u = u + lr * (m1 / (1.0 - b1 ** (t + 1))) / (np.sqrt(m2 / (1.0 - b2 ** (t + 1))) + eps)
            u = np.clip(u, lo / ellk, hi / ellk)
            xc = np.clip(u * ellk, lo, hi)
            xc = np.where(u >= hi / ellk, hi, np.where(u <= lo / ellk, lo, xc))   # on a face: the face itself, exactly
    return x_best, f_best, idx
