"""Numpy float64 restatement of the input gradients of the exact GP's cached predictive (hb_gram_predict_grad;
henbun_amd/gp/exact.py: ExactPosterior.predict_grad, acquisition(grad=True), maximise).  With V = [P mean rows; S - P cache
rows], K_ij = k(x2_i, x_j) the unit RBF and t[s, j] = scale sum_i V[s, i] K_ij:

    u[s, j, k]     = d t[s, j] / d x_jk = scale sum_i V[s, i] K_ij (x2_ik - x_jk) / ell_k^2
    dmean[p, j, k] = u[p, j, k], p < P
    dvar[j, k]     = -2 sum_{s >= P} t[s, j] u[s, j, k]   (s ascending); 0 where prior - q_j < 0, q_j = sum_{s >= P} t[s, j]^2
    dval[j, k]     = sgn a_mu u[0, j, k] + a_v dvar-sum   (P = 1; a_mu, a_v from acq_ref.tail at (t[0, j], prior - q_j))

t and u are formed as the device forms them: one partial per chunk of rows, the partials added in chunk order, then the
scale (exact_gp_ref.matvec)."""
import numpy as np

import acq_ref as AR
import exact_gp_ref as E


def _ell(ell, d):
    ell = np.reshape(np.asarray(ell, np.float64), [-1])
    return np.broadcast_to(ell, (d,)) if ell.size == 1 else ell


def products(x, x2, ell, V, scale=1.0, chunk=2048):
    """(t [S, n], u [S, n, d])."""
    x, x2, V = (np.asarray(a, np.float64) for a in (x, x2, V))
    (n, d), N, S = x.shape, x2.shape[0], V.shape[0]
    l2 = _ell(ell, d) ** 2
    t, u = np.zeros((S, n)), np.zeros((S, n, d))
    for i0 in range(0, N, chunk):
        K = E.rbf(x2[i0:i0 + chunk], x, ell)
        Vc = V[:, i0:i0 + chunk]
        t = t + Vc @ K
        part = np.empty((S, n, d))
        for k in range(d):
            part[:, :, k] = Vc @ (K * ((x2[i0:i0 + chunk, k, None] - x[None, :, k]) / l2[k]))
        u = u + part
    return scale * t, scale * u


def magnitudes(x, x2, ell, V):
    """(A [S, 1], W [S, n], G [n, d], Wd [S, n, d]): A_s = sum_i |V_si|, W_sj = sum_i |V_si| K_ij (exact_gp_ref's),
    G_jk = max_i |x2_ik - x_jk| / ell_k^2 and Wd_sjk = sum_i |V_si| K_ij |x2_ik - x_jk| / ell_k^2: what the bounds of t and u
    are stated in."""
    x, x2, Va = np.asarray(x, np.float64), np.asarray(x2, np.float64), np.abs(np.asarray(V, np.float64))
    n, d = x.shape
    l2 = _ell(ell, d) ** 2
    K = E.rbf(x2, x, ell)
    G, Wd = np.empty((n, d)), np.empty((Va.shape[0], n, d))
    for k in range(d):
        D = np.abs(x2[:, k, None] - x[None, :, k]) / l2[k]
        G[:, k] = D.max(0)
        Wd[:, :, k] = Va @ (K * D)
    return Va.sum(1, keepdims=True), Va @ K, G, Wd


def ordered_q(t, P):
    """q [n] = sum_{s >= P} t[s]^2, s ascending, each square and each sum rounded once."""
    q = np.zeros(t.shape[1])
    for s in range(P, t.shape[0]):
        q = q + t[s] * t[s]
    return q


def ordered_dq(t, u, P):
    """[n, d] = sum_{s >= P} t[s, :, None] u[s], s ascending, each product and each sum rounded once."""
    dq = np.zeros(u.shape[1:])
    for s in range(P, t.shape[0]):
        dq = dq + t[s][:, None] * u[s]
    return dq


def moments_grad(t, u, P, prior):
    """(mean [P, n], var [n] clamped at 0, dmean [P, n, d], dvar [n, d], raw [n] = prior - q)."""
    raw = prior - ordered_q(t, P)
    dvar = -2.0 * ordered_dq(t, u, P)
    if t.shape[0] == P:
        dvar = np.zeros_like(dvar)
    dvar = np.where((raw < 0.0)[:, None], 0.0, dvar)
    return t[:P], np.maximum(raw, 0.0), u[:P], dvar, raw


def acquisition_grad(kind, t, u, prior, best=0.0, param=0.0, largest=True, var_floor=0.0):
    """(val [n], dval [n, d], clamped [n]) for one latent function: the tail of acq_ref at (t[0], prior - q)."""
    _, _, dmean, dvar, raw = moments_grad(t, u, 1, prior)
    val, a_mu, a_v, clamped = AR.tail(kind, t[0], raw, best, param, 1.0, largest, var_floor)
    sgn = 1.0 if largest else -1.0
    return val, (sgn * a_mu)[:, None] * dmean[0] + a_v[:, None] * dvar, clamped
