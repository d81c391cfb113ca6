"""Numpy float64 restatement of the gradients of the psi statistics (hb_sgp_psi_grad) and of the collapsed bound under
uncertain inputs (SparseGP.psi_bound_and_grad, models.BayesianGPLVM), on top of psi_ref.py and collapsed_grad_ref.py and in
their notation.  For

    F = 1/2 sum_n sum_{m, m'} Q_mm' psi2_n(m, m') + sum_n sum_m rho_nm psi1_n(m),   rho_nm = sum_p R_mp Y_np,

with u_k = l_k^2, a_k = 1 / (u_k + 2 s_k), a1_k = 1 / (u_k + s_k), t_k = mu_k - (z_mk + z_m'k) / 2, dz_k = z_mk - z_m'k and
tau_k = mu_k - z_mk:

    dlog psi2 / dmu_k  = -2 a_k t_k                                        dlog psi1 / dmu_k  = -a1_k tau_k
    dlog psi2 / ds_k   = -a_k + 2 a_k^2 t_k^2                              dlog psi1 / ds_k   = -1/2 a1_k + 1/2 a1_k^2 tau_k^2
    dlog psi2 / dz_mk  = a_k t_k - dz_k / (2 u_k)   (and the mirror image) dlog psi1 / dz_mk  = a1_k tau_k
    dlog psi2 / du_k   = s_k a_k / u_k + dz_k^2 / (4 u_k^2) + a_k^2 t_k^2  dlog psi1 / du_k   = 1/2 s_k a1_k / u_k + 1/2 a1_k^2 tau_k^2
    d / dl_k = 2 l_k d / du_k   (one shared lengthscale: summed over k)

The sum runs over the lower triangle of Q with the diagonal halved.  Every summand above counts as one TERM: psi_grad also
returns, per output entry, the sum of the absolute values of its terms (with |R| |Y| in the place of rho) -- what the
rounding error of any order of summation scales with -- and the number of terms."""
import numpy as np

import collapsed_grad_ref as CG
import optimal_q_ref as R
import psi_ref as PR


def psi_grad(mu, s, Y, z, ell, Q, Rw, chunk=None):
    """dict(mubar [N, d], sbar [N, d], zbar [M, d], ellbar [dl]; the same names + '_abs': the absolute term sums; the same
    names + '_terms': the number of terms of one entry)."""
    mu, s, Y, z, Q, Rw = (np.asarray(a, np.float64) for a in (mu, s, Y, z, Q, Rw))
    ell = np.asarray(ell, np.float64).reshape(-1)
    N, d = mu.shape
    M = z.shape[0]
    l = PR._ell(ell, d)
    u = l ** 2
    im, iq = np.tril_indices(M)
    L = len(im)
    w = np.where(im == iq, 0.5, 1.0) * (0.5 * (Q + Q.T))[im, iq]
    chunk = chunk or max(1, (1 << 20) // L)
    out = {k: np.zeros(sh) for k, sh in (("mubar", (N, d)), ("sbar", (N, d)), ("zbar", (M, d)), ("ubar", (d,)))}
    ab = {k: np.zeros_like(v) for k, v in out.items()}

    for n0 in range(0, N, chunk):
        sl = slice(n0, n0 + chunk)
        mc, sc, Yc = mu[sl], s[sl], Y[sl]
        wv = w[None, :] * PR.psi2_pairs(mc, sc, z, ell, im, iq)            # [n, L]: the weighted psi2 of the pairs
        p1 = PR.psi1(mc, sc, z, ell)                                       # [n, M]
        w1, w1_abs = (Yc @ Rw.T) * p1, (np.abs(Yc) @ np.abs(Rw).T) * p1    # rho psi1, and with |R| |Y| for the absolute sums
        for k in range(d):
            sk = sc[:, k, None]
            a, a1 = 1.0 / (u[k] + 2.0 * sk), 1.0 / (u[k] + sk)
            t = mc[:, k, None] - 0.5 * (z[im, k] + z[iq, k])[None, :]
            dz = (z[im, k] - z[iq, k])[None, :]
            tau = mc[:, k, None] - z[None, :, k]
            # (weights, factor) of every term; the value sums weights * factor, the absolute sum |weights| * |factor|
            for tgt, W2, W1, f in ((out, wv, w1, lambda x: x), (ab, np.abs(wv), w1_abs, np.abs)):
                tgt["mubar"][sl, k] += (W2 * f(-2.0 * a * t)).sum(1) + (W1 * f(-a1 * tau)).sum(1)
                tgt["sbar"][sl, k] += ((W2 * f(-a)).sum(1) + (W2 * f(2.0 * a * a * t * t)).sum(1)
                                       + (W1 * f(-0.5 * a1)).sum(1) + (W1 * f(0.5 * a1 * a1 * tau * tau)).sum(1))
                at, dzu = (W2 * f(a * t)).sum(0), (W2 * f(dz / (2.0 * u[k]))).sum(0)
                np.add.at(tgt["zbar"][:, k], im, at + (dzu if tgt is ab else -dzu))
                np.add.at(tgt["zbar"][:, k], iq, at + dzu)                 # the mirror image: dz changes sign
                tgt["zbar"][:, k] += (W1 * f(a1 * tau)).sum(0)
                tgt["ubar"][k] += ((W2 * f(sk * a / u[k])).sum() + (W2 * f(dz * dz / (4.0 * u[k] ** 2))).sum()
                                   + (W2 * f(a * a * t * t)).sum() + (W1 * f(0.5 * sk * a1 / u[k])).sum()
                                   + (W1 * f(0.5 * a1 * a1 * tau * tau)).sum())
    res = dict(mubar=out["mubar"], sbar=out["sbar"], zbar=out["zbar"], mubar_abs=ab["mubar"], sbar_abs=ab["sbar"],
               zbar_abs=ab["zbar"])
    eb, ea = 2.0 * l * out["ubar"], 2.0 * l * ab["ubar"]
    one = ell.shape[0] == 1 and d > 1
    res["ellbar"] = eb.sum(keepdims=True) if one else eb
    res["ellbar_abs"] = ea.sum(keepdims=True) if one else ea
    res.update(mubar_terms=L + M, sbar_terms=2 * (L + M), zbar_terms=N * (2 * (M + 1) + 1),
               ellbar_terms=N * (3 * L + 2 * M) * (d if one else 1))
    return res


def kl(mu, s):
    """KL(prod_n N(mu_n, diag s_n) || N(0, I)) and its gradients with respect to mu and s"""
    mu, s = np.asarray(mu, np.float64), np.asarray(s, np.float64)
    return 0.5 * float(np.sum(s + mu * mu - 1.0 - np.log(s))), mu.copy(), 0.5 * (1.0 - 1.0 / s)


def bound_and_grad(mu, s, Y, z, ell, jitter, noise_var, k_var=1.0, residual="diagonal", with_kl=False):
    """dict(value, X_mean, X_var, z, lengthscales, noise_var, k_var; z_streamed, z_kmm, ell_streamed, ell_kmm; X_mean_abs,
    X_var_abs, noise_var_abs, k_var_abs; Q, R, W, Phi, b): the collapsed bound under uncertain inputs (minus the KL of q(X)
    with_kl=True) and its gradient."""
    mu, s, Y, z = (np.asarray(a, np.float64) for a in (mu, s, Y, z))
    ell = np.asarray(ell, np.float64).reshape(-1)
    N, P = Y.shape
    k, s2 = float(k_var), float(noise_var)
    rho = 1.0 if residual == "diagonal" else 0.0
    _, W = R.chol_factor(z, ell, jitter)
    Phi, b, yy, a2sum = PR.stats(mu, s, Y, z, ell, W=W)
    F, D, G, g, m, c, tau = CG.tail(Phi, b, yy, N, s2, k, residual)
    Q, Rw = CG.weights(W, G, g)
    pg = psi_grad(mu, s, Y, z, ell, Q, Rw)
    zk, ek = CG.kmm_part(z, ell, W, G, g, Phi, b)
    dk = tau / s2 + np.sum(m * b) / (2.0 * np.sqrt(k) * s2) - rho * P * (N - a2sum) / (2.0 * s2)
    ds2 = (-N * P / (2.0 * s2) + yy.sum() / (2.0 * s2 ** 2) - (k / s2 ** 2) * tau - np.sum(m * c) / s2
           + rho * P * k * (N - a2sum) / (2.0 * s2 ** 2))
    dk_abs = abs(tau / s2) + abs(np.sum(m * b) / (2.0 * np.sqrt(k) * s2)) + rho * P * abs(N - a2sum) / (2.0 * s2)
    ds2_abs = (N * P / (2.0 * s2) + yy.sum() / (2.0 * s2 ** 2) + abs((k / s2 ** 2) * tau) + abs(np.sum(m * c) / s2)
               + rho * P * k * abs(N - a2sum) / (2.0 * s2 ** 2))
    gm, gs = pg["mubar"].copy(), pg["sbar"].copy()
    gm_abs, gs_abs = pg["mubar_abs"].copy(), pg["sbar_abs"].copy()
    if with_kl:
        kv, km, ks = kl(mu, s)
        F, gm, gs = F - kv, gm - km, gs - ks
        gm_abs, gs_abs = gm_abs + np.abs(km), gs_abs + 0.5 * (1.0 + 1.0 / s)
    return dict(value=F, X_mean=gm, X_var=gs, z=pg["zbar"] + zk, lengthscales=pg["ellbar"] + ek, noise_var=float(ds2),
                k_var=float(dk), z_streamed=pg["zbar"], z_kmm=zk, ell_streamed=pg["ellbar"], ell_kmm=ek, X_mean_abs=gm_abs,
                X_var_abs=gs_abs, noise_var_abs=float(ds2_abs), k_var_abs=float(dk_abs), Q=Q, R=Rw, W=W, Phi=Phi, b=b)


def bound_autograd(mu, s, Y, z, ell, jitter, noise_var, k_var=1.0, residual="diagonal", with_kl=False):
    """The same numbers from torch.autograd in float64 on the bound written in torch ops from the definitions of psi1 and
    psi2 (midpoint form): an independent evaluation (no formula of this file is used).  Small problems: psi2 is [N, M, M].
    Returns dict(value, X_mean, X_var, z, lengthscales, noise_var, k_var)."""
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    Y = t(Y)
    mu, s = t(mu).requires_grad_(True), t(s).requires_grad_(True)
    z, ell = t(z).requires_grad_(True), t(np.asarray(ell, np.float64).reshape(-1)).requires_grad_(True)
    s2, k = t(noise_var).requires_grad_(True), t(k_var).requires_grad_(True)
    N, P = Y.shape
    M, d = z.shape
    u = (ell ** 2).expand(d)
    e1 = ((mu[:, None, :] - z[None, :, :]) ** 2 / (u + s)[:, None, :]).sum(-1)
    psi1 = torch.prod(1.0 + s / u, 1)[:, None] ** -0.5 * torch.exp(-0.5 * e1)                     # [N, M]
    zb = 0.5 * (z[:, None, :] + z[None, :, :])
    e2 = (((z[:, None, :] - z[None, :, :]) ** 2 / (4.0 * u)).sum(-1)[None]
          + ((mu[:, None, None, :] - zb[None]) ** 2 / (u + 2.0 * s)[:, None, None, :]).sum(-1))
    Psi2 = (torch.prod(1.0 + 2.0 * s / u, 1)[:, None, None] ** -0.5 * torch.exp(-e2)).sum(0)       # [M, M]
    zs = z / ell
    Kmm = torch.exp(-0.5 * ((zs[:, None, :] - zs[None, :, :]) ** 2).sum(-1)) + jitter * torch.eye(M, dtype=torch.float64)
    L = torch.linalg.cholesky(Kmm)
    Phi = torch.linalg.solve_triangular(L, torch.linalg.solve_triangular(L, Psi2, upper=False).T, upper=False)
    Phi = 0.5 * (Phi + Phi.T)
    b = torch.linalg.solve_triangular(L, psi1.T @ Y, upper=False).T                                # [P, M]
    yy = (Y ** 2).sum(0)
    Lam = torch.eye(M, dtype=torch.float64) + (k / s2) * Phi
    c = torch.sqrt(k) * b / s2
    LL = torch.linalg.cholesky(Lam)
    tt = torch.linalg.solve_triangular(LL, c.T, upper=False)
    val = torch.sum(-0.5 * N * torch.log(2 * np.pi * s2) - yy / (2 * s2) + 0.5 * (tt * tt).sum(0))
    val = val - P * torch.log(torch.diagonal(LL)).sum()
    if residual == "diagonal":
        val = val - P * k * (N - torch.trace(Phi)) / (2 * s2)
    if with_kl:
        val = val - 0.5 * torch.sum(s + mu * mu - 1.0 - torch.log(s))
    val.backward()
    return dict(value=float(val.detach()), X_mean=mu.grad.numpy(), X_var=s.grad.numpy(), z=z.grad.numpy(),
                lengthscales=ell.grad.numpy(), noise_var=float(s2.grad), k_var=float(k.grad))


def bound_value(mu, s, Y, z, ell, jitter, noise_var, k_var=1.0, residual="diagonal", with_kl=False):
    """The value alone (for central differences)."""
    Phi, b, yy, a2sum = PR.stats(mu, s, Y, z, ell, jitter)
    F = R.collapsed_bound(Phi, b, yy, a2sum, Y.shape[0], float(noise_var), float(k_var), residual)
    return F - kl(mu, s)[0] if with_kl else F


def case(N, M, d, P, seed=0, scalar_ell=False, zero_rows=True):
    """(mu, s, Y, z, ell): collapsed_grad_ref.case with input variances up to 0.3 l^2; zero_rows: exact zeros in a whole
    row and in single dimensions."""
    mu, Y, z, ell = CG.case(N, M, d, P, seed, scalar_ell)
    rng = np.random.RandomState(seed + 100)
    s = rng.uniform(0.01, 0.3, (N, d)) * PR._ell(ell, d) ** 2
    if zero_rows:
        s[0] = 0.0
        s[min(1, N - 1), 0] = 0.0
    return mu, s, Y, z, ell
