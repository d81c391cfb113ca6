"""Numpy float64 restatement of the exact GP's log marginal likelihood by conjugate gradients (henbun_amd/gp/exact.py:
log_marginal_likelihood, hb_gram_bilinear_grad, hb_pcg_*_coef), on top of tests/exact_gp_ref.py.

    K^ = k_var K(X, X) + noise_var I,  alpha_c = K^^-1 y_c,  P_ = k_var C^T C + noise_var I (no factor: P_ = I)
    L = -1/2 sum_c y_c . alpha_c - P/2 logdet K^ - N P / 2 log 2 pi
    dL/dtheta = sum_pairs w_p a_p^T (dK^/dtheta) b_p,   pairs (alpha_c, alpha_c, 1/2), (u_t, P_^-1 z_t, -P / 2T), u_t = K^^-1 z_t
    dK^/dk_var = K,  dK^/dnoise_var = I,  dK^/dell_k = k_var K_ij (x_ik - x_jk)^2 / ell_k^3 (one lengthscale: summed over k)
    logdet K^ ~ logdet P_ + 1/T sum_t (z_t^T P_^-1 z_t) e_1^T log(T_t) e_1,  T_t the Lanczos tridiagonal of probe t's CG.
"""
import numpy as np

import exact_gp_ref as E


def _ell(ell):
    return np.reshape(np.asarray(ell, dtype=np.float64), [-1])


def bilinear_grad(x, ell, A, B, w, block=16, magnitude=False):
    """g [1 + dl]: g[0] = sum_s w_s sum_ij A_si B_sj K_ij, g[1 + k] = sum_s w_s sum_ij A_si B_sj K_ij (x_ik - x_jk)^2 /
    ell_k^3 (dl = 1: summed over k), dense, `block` rows of K at a time (K as exact_gp_ref.rbf forms it: the difference
    first, scaled afterwards), each block contracted as sum_s w_s A_s[rows] . (K[rows] B_s).  magnitude=True: (g, M) with
    M the same sums over |w_s| |A_si| |B_sj| -- what the bounds are stated in."""
    x, A, B, w, ell = (np.asarray(a, dtype=np.float64) for a in (x, A, B, w, _ell(ell)))
    N, d = x.shape
    dl = ell.size
    g, M = np.zeros(1 + dl), np.zeros(1 + dl)
    wA = A * w[:, None]
    left = [wA.T] + ([np.abs(wA).T] if magnitude else [])                        # [N, S] each
    right = np.ascontiguousarray(np.concatenate([B] + ([np.abs(B)] if magnitude else [])).T)   # [N, S] or [N, 2 S]
    S = A.shape[0]

    def add(comp, Km, rows):
        KB = Km @ right                                                          # [rb, S or 2 S]
        for o, (out, lf) in enumerate(zip((g, M), left)):
            out[comp] += (lf[rows] * KB[:, o * S:(o + 1) * S]).sum()

    for i0 in range(0, N, block):                    # (in-place passes over blocks small enough to stay in cache)
        rows = slice(i0, i0 + block)
        D = [np.square(x[rows, k, None] - x[None, :, k]) for k in range(d)]
        r2 = D[0] / ell[0] ** 2
        for k in range(1, d):
            r2 += D[k] / ell[0 if dl == 1 else k] ** 2
        K = np.multiply(r2, -0.5)
        np.exp(K, out=K)
        add(0, K, rows)
        if dl == 1:
            add(1, np.multiply(K, r2, out=r2), rows)                             # sum_k (x_ik - x_jk)^2 / ell^2 = r2
        else:
            for k in range(d):
                add(1 + k, np.multiply(K, D[k], out=D[k]), rows)
    for out in (g, M):                                # K r2 / ell and K D_k / ell_k^3: the factors last
        out[1:] /= ell if dl == 1 else ell ** 3
    return (g, M) if magnitude else g


def pcg_record(X, ell, k_var, noise_var, B, C=None, tol=1e-6, max_iter=1000):
    """exact_gp_ref.pcg with the recurrence logged -> (x, info): info = dict(iterations, coef [iterations, 2, S] -- alpha_j,
    beta_j per row, NaN from where a row had converged --, rz0 [S] = b . P_^-1 b, lanczos_steps [S])."""
    B = np.asarray(B, np.float64)
    S = B.shape[0]
    A = lambda V: E.matvec(X, None, ell, V, k_var, noise_var)
    x, r = np.zeros_like(B), B.copy()
    bb = (B * B).sum(1)
    thr = tol * tol * bb
    rr = bb.copy()
    z = E.precond_apply(C, k_var, noise_var, r)
    p, rz = z.copy(), (r * z).sum(1)
    rz0, coef, it = rz.copy(), [], 0
    while it < max_iter and not np.all(rr <= thr):
        act = rr > thr
        row = np.full((2, S), np.nan)
        Ap = A(p)
        pAp = (p * Ap).sum(1)
        alpha = np.where(act & (pAp > 0), rz / np.where(pAp > 0, pAp, 1.0), 0.0)
        row[0, act] = alpha[act]
        x += alpha[:, None] * p
        r -= alpha[:, None] * Ap
        rr = np.where(act, (r * r).sum(1), rr)
        it += 1
        z = E.precond_apply(C, k_var, noise_var, r)
        rzn = (r * z).sum(1)
        beta = np.where(rz > 0, rzn / np.where(rz > 0, rz, 1.0), 0.0)
        upd = rr > thr
        row[1, upd] = beta[upd]
        p = np.where(upd[:, None], z + beta[:, None] * p, p)
        rz = np.where(upd, rzn, rz)
        coef.append(row)
    coef = np.asarray(coef).reshape(it, 2, S)
    steps = np.array([int(np.argmin(np.append(coef[:, 0, s] > 0, False))) for s in range(S)])
    return x, dict(iterations=it, coef=coef, rz0=rz0, lanczos_steps=steps)


def tridiagonal(alpha, beta):
    """The Lanczos tridiagonal [m, m] of a CG recurrence: diagonal 1 / alpha_0, then 1 / alpha_j + beta_{j-1} / alpha_{j-1};
    off-diagonal sqrt(beta_{j-1}) / alpha_{j-1}."""
    alpha = np.asarray(alpha, np.float64)
    m = alpha.size
    beta = np.asarray(beta, np.float64)[:max(m - 1, 0)]
    T = np.zeros((m, m))
    for j in range(m):
        T[j, j] = 1.0 / alpha[j] + (beta[j - 1] / alpha[j - 1] if j else 0.0)
        if j:
            T[j, j - 1] = T[j - 1, j] = np.sqrt(beta[j - 1]) / alpha[j - 1]
    return T


def logquad(alpha, beta):
    """e_1^T log(T) e_1 of tridiagonal(alpha, beta); 0 for no steps."""
    if np.size(alpha) == 0:
        return 0.0
    lam, V = np.linalg.eigh(tridiagonal(alpha, beta))
    return float(np.sum(V[0] ** 2 * np.log(lam)))


def precond_dense(X, C, k_var, noise_var):
    """P_ [N, N]: k_var C^T C + noise_var I, or I without a factor."""
    N = np.shape(X)[0]
    if C is None or C.shape[0] == 0:
        return np.eye(N)
    return k_var * C.T @ C + noise_var * np.eye(N)


def factor_along(X, ell, idx):
    """C [len(idx), N]: exact_gp_ref.factor's rows in float64 for a GIVEN pivot sequence -- the factor of a session whose
    own selection took those pivots.  (In float32 the conditional variances of far-apart points round to exactly 1 and
    tie to the lowest index, where float64 still tells them apart: the two dtypes pick different, equally valid pivots.)"""
    import greedy_ref as GR

    X, ell = np.asarray(X, np.float64), _ell(ell)
    C, dvar = np.zeros((len(idx), X.shape[0])), np.ones(X.shape[0])
    for j, i in enumerate(idx):
        GR._step(X, ell, C, dvar, j, int(i), "forward")
    return C


def orthogonal_probes(Pd):
    """Z [N, N] = sqrt(N) chol(P_)^T: 1/N sum_t z_t z_t^T = P_ exactly, so the estimators equal what they estimate."""
    return np.sqrt(Pd.shape[0]) * np.linalg.cholesky(Pd).T


def _dK(X, ell, k_var):
    """[K, the list of dK^/dell_k] dense."""
    X, ell = np.asarray(X, np.float64), _ell(ell)
    K = E.rbf(X, X, ell)
    D = [(X[:, k, None] - X[None, :, k]) ** 2 for k in range(X.shape[1])]
    if ell.size == 1:
        return K, [k_var * K * sum(D) / ell[0] ** 3]
    return K, [k_var * K * D[k] / ell[k] ** 3 for k in range(X.shape[1])]


def mll_dense(X, Y, ell, k_var, noise_var):
    """(value, grad, mag) from the dense Cholesky: grad = dict(lengthscales [dl], k_var, noise_var), the analytic
    1/2 sum_c alpha_c^T dK^ alpha_c - P/2 tr(K^^-1 dK^); mag = the sums of the magnitudes of the terms of the value and of
    each gradient component (keys value, lengthscales, k_var, noise_var): what the bounds of the GPU tests are stated in."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    N, P = Y.shape
    Kh = E.dense(X, ell, k_var, noise_var)
    L = np.linalg.cholesky(Kh)
    Kinv = np.linalg.inv(Kh)
    alpha = Kinv @ Y                                                   # [N, P]
    logdet = 2.0 * np.log(np.diag(L)).sum()
    fit = (Y * alpha).sum(0)
    value = -0.5 * fit.sum() - 0.5 * P * logdet - 0.5 * N * P * np.log(2.0 * np.pi)
    K, dells = _dK(X, ell, k_var)

    def comp(dK):
        q = np.einsum("ic,ij,jc->c", alpha, dK, alpha)
        tr = np.sum(Kinv * dK)
        return 0.5 * q.sum() - 0.5 * P * tr, 0.5 * np.abs(q).sum() + 0.5 * P * abs(tr)

    parts = dict(k_var=comp(K), noise_var=comp(np.eye(N)))
    ls = [comp(dK) for dK in dells]
    grad = dict(lengthscales=np.array([v for v, _ in ls]), k_var=parts["k_var"][0], noise_var=parts["noise_var"][0])
    mag = dict(value=0.5 * np.abs(fit).sum() + 0.5 * P * abs(logdet) + 0.5 * N * P * np.log(2.0 * np.pi),
               lengthscales=np.array([m for _, m in ls]), k_var=parts["k_var"][1], noise_var=parts["noise_var"][1])
    return float(value), grad, mag


def logdet_precond(C, k_var, noise_var, N):
    """logdet P_ = (N - R) log noise_var + logdet(noise_var I + k_var C C^T); 0 without a factor."""
    if C is None or C.shape[0] == 0:
        return 0.0
    R = C.shape[0]
    return (N - R) * np.log(noise_var) + 2.0 * np.log(np.diag(np.linalg.cholesky(noise_var * np.eye(R) + k_var * C @ C.T))).sum()


def mll_estimate(X, Y, ell, k_var, noise_var, Z, C=None, tol=1e-6, max_iter=1000):
    """(value, grad, info): the same-probe estimator -- one recorded lockstep PCG over [Y columns; Z], the quadrature of
    the probes' tridiagonals, the pairs contracted by bilinear_grad.  info = dict(iterations, logdet, logdet_precond,
    lanczos_steps [T])."""
    X, Y, Z = (np.asarray(a, np.float64) for a in (X, Y, Z))
    N, P = Y.shape
    T = Z.shape[0]
    sol, rec = pcg_record(X, ell, k_var, noise_var, np.concatenate([Y.T, Z]), C, tol, max_iter)
    coef, steps = rec["coef"], rec["lanczos_steps"]
    ld_p = logdet_precond(C, k_var, noise_var, N)
    quad = [rec["rz0"][P + t] * logquad(coef[:steps[P + t], 0, P + t], coef[:steps[P + t], 1, P + t]) for t in range(T)]
    logdet = ld_p + np.sum(quad) / T
    value = -0.5 * (Y.T * sol[:P]).sum() - 0.5 * P * logdet - 0.5 * N * P * np.log(2.0 * np.pi)
    Bm = np.concatenate([sol[:P], E.precond_apply(C, k_var, noise_var, Z)])
    w = np.concatenate([np.full(P, 0.5), np.full(T, -0.5 * P / T)])
    g = bilinear_grad(X, ell, sol, Bm, w)
    grad = dict(lengthscales=k_var * g[1:], k_var=float(g[0]), noise_var=float(w @ (sol * Bm).sum(1)))
    return float(value), grad, dict(iterations=rec["iterations"], logdet=float(logdet), logdet_precond=float(ld_p),
                                    lanczos_steps=steps[P:])


def logquad_dense(X, ell, k_var, noise_var, Z, C=None):
    """1/T sum_t q_t^T log(P_^-1/2 K^ P_^-1/2) q_t with q_t = P_^-1/2 z_t, from dense eigen-decompositions: what the
    tridiagonal quadrature of the probes' CG recurrences converges to."""
    X, Z = np.asarray(X, np.float64), np.asarray(Z, np.float64)
    lam, V = np.linalg.eigh(precond_dense(X, C, k_var, noise_var))
    Ph = (V / np.sqrt(lam)) @ V.T
    mu, U = np.linalg.eigh(Ph @ E.dense(X, ell, k_var, noise_var) @ Ph)
    Q = Z @ Ph @ U
    return float(((Q * Q) @ np.log(mu)).mean())


def adam_ascent(objective, raw0, forward, dforward, steps, lr):
    """Adam ASCENT in the raw parameters (the loop of henbun_amd.models._adam_ascent): raw0 a dict of arrays,
    objective(cons) -> (value, grad with respect to the constrained values forward(raw)) -> (trace [steps + 1], raw)."""
    raw = {n: np.array(v, dtype=np.float64) for n, v in raw0.items()}
    m1 = {n: np.zeros_like(v) for n, v in raw.items()}
    m2 = {n: np.zeros_like(v) for n, v in raw.items()}
    b1, b2, eps, trace = 0.9, 0.999, 1e-8, []
    for t in range(steps + 1):
        value, gc = objective({n: forward(v) for n, v in raw.items()})
        trace.append(value)
        if t == steps:
            break
        for n in raw:
            g = np.reshape(gc[n], raw[n].shape) * dforward(raw[n])
            m1[n] = b1 * m1[n] + (1.0 - b1) * g
            m2[n] = b2 * m2[n] + (1.0 - b2) * g ** 2
            raw[n] = raw[n] + lr * (m1[n] / (1.0 - b1 ** (t + 1))) / (np.sqrt(m2[n] / (1.0 - b2 ** (t + 1))) + eps)
    return np.asarray(trace), raw
