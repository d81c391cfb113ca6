"""Numpy restatement of the pathwise posterior function draws (SparseGP.pathwise_draws, hb_sgp_pathwise), built on
optimal_q_ref, in float64 unless a dtype is asked for.  In the whitened convention, x~ = x / ell, W = Lm^-1,
A(x) = W K(z, x), q(u) = N(m, S S^T):

    g_s(x) = L^-1/2 sum_l [ w_s,2l cos(omega_l . x~) + w_s,2l+1 sin(omega_l . x~) ]        omega_l ~ N(0, I_d), w_s ~ N(0, I_2L)
    u_s = m + eps_s S^T,  t_s = u_s - g_s(z) W^T,  v_s = t_s W,   coef_s = [ w_s / sqrt(L) | v_s ]
    f_s(x) = scale coef_s B(x),   B = [ cos / sin rows interleaved | K(z_m, x) ]  [2L + M, n]

Given omega, f is Gaussian with mean scale m A(x) and covariance scale^2 (C^T C + A^T S S^T A), C(x) = phi(x) - phi(z) W^T
A(x), phi the 2L trig rows over sqrt(L); as L grows C^T C tends to K(x, x') - A^T A."""
import numpy as np

import optimal_q_ref as R

KSTEP = 32      # basis rows per block of the float32 product (the K-step of the device kernel)


def basis(x, omega, z, ell):
    """B(x) [2L + M, n] in the dtype of x: rows 2l, 2l + 1 = cos, sin(omega_l . x / ell), rows 2L + m = K(z_m, x).
    z None: the trig rows only."""
    L = omega.shape[0]
    p = omega @ (x / ell).T                               # [L, n]
    B = np.empty((2 * L + (0 if z is None else z.shape[0]), x.shape[0]), dtype=x.dtype)
    B[0:2 * L:2], B[1:2 * L:2] = np.cos(p), np.sin(p)
    if z is not None and z.shape[0]:
        B[2 * L:] = R.rbf(z, x, ell)
    return B


def evaluate(x, omega, z, ell, coef, scale=1.0, dtype=np.float64):
    """out [S, n] = scale coef B(x) as float64.  dtype float32: the inputs rounded to float32, the basis and the product
    formed in float32, the rows taken in blocks of KSTEP in the kernel's order (the trig rows, the last block short, then
    the RBF rows) with the running sum kept in float32."""
    x, omega, ell, coef = (np.asarray(a, dtype=dtype) for a in (x, omega, ell, coef))
    z = None if z is None else np.asarray(z, dtype=dtype)
    B = basis(x, omega, z, ell)
    L, K = omega.shape[0], B.shape[0]
    acc = np.zeros((coef.shape[0], x.shape[0]), dtype=dtype)
    for k0 in list(range(0, 2 * L, KSTEP)) + list(range(2 * L, K, KSTEP)):
        k1 = min(k0 + KSTEP, 2 * L if k0 < 2 * L else K)
        acc = acc + coef[:, k0:k1] @ B[k0:k1]
    return (np.asarray(scale, dtype=dtype) * acc).astype(np.float64)


def coefficients(m, S, W, z, ell, omega, w, eps):
    """coef [S, 2L + M] = [ w / sqrt(L) | v ] in float64: m [1, M]; S [M, M] lower or the mean-field s [M]; w [S, 2L];
    eps [S, M]."""
    m, S, W, z, ell, omega, w, eps = (np.asarray(a, np.float64) for a in (m, S, W, z, ell, omega, w, eps))
    cw = w / np.sqrt(omega.shape[0])
    U = m.reshape(1, -1) + (eps @ S.T if S.ndim == 2 else eps * S)
    T = U - evaluate(z, omega, None, ell, cw) @ W.T
    return np.concatenate([cw, T @ W], axis=1)


def covariance(x, omega, z, ell, W, S):
    """Exact covariance [n, n] of the draws at fixed omega for scale = 1: C^T C + A^T S S^T A."""
    x, omega, z, ell, W, S = (np.asarray(a, np.float64) for a in (x, omega, z, ell, W, S))
    rt = np.sqrt(omega.shape[0])
    A = R.A_of(W, z, x, ell)
    C = basis(x, omega, None, ell) / rt - (basis(z, omega, None, ell) / rt) @ W.T @ A
    SA = S.T @ A if S.ndim == 2 else S[:, None] * A
    return C.T @ C + SA.T @ SA


def exact_covariance(x, z, ell, W, S):
    """K(x, x') - A^T A + A^T S S^T A: the 'fullrank' residual of predict_f(full_cov=True) without its jitter term."""
    A = R.A_of(W, z, x, ell)
    SA = S.T @ A if S.ndim == 2 else S[:, None] * A
    return R.rbf(x, x, ell) - A.T @ A + SA.T @ SA


# ---------------------------------------------------------------------------------------- the inputs of the tests
def kernel_case(n, L, M, d, S, dl, span, seed):
    """(x [n, d], omega [L, d], z [M, d] or None, ell [dl], coef [S, 2L + M]) for the kernel tests: x and z uniform on
    [0, span]^d, coef of mixed sign with the trailing M entries about 1e3 (the size of v at cond(K(z, z)) ~ 1e6, so the
    cancellation of the update is present)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, span, (n, d))
    omega = rng.standard_normal((L, d))
    z = rng.uniform(0.0, span, (M, d)) if M else None
    ell = np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d)
    coef = rng.standard_normal((S, 2 * L + M))
    coef[:, 2 * L:] *= 1e3
    return x, omega, z, ell, coef


def cov_case(d, L, seed):
    """(x [300, d], omega [L, d], z [32, d], ell, W, S_q): z and x uniform on [0, 16] (d = 1) or [0, 4]^d, ell = 0.8,
    jitter 1e-5, S_q = 0.3 I + 0.05 tril(N(0, 1))."""
    rng = np.random.default_rng(seed)
    M, box = 32, 16.0 if d == 1 else 4.0
    z = rng.uniform(0.0, box, (M, d))
    x = rng.uniform(0.0, box, (300, d))
    Sq = 0.3 * np.eye(M) + 0.05 * np.tril(rng.standard_normal((M, M)))
    omega = rng.standard_normal((L, d))
    ell = np.array([0.8])
    _, W = R.chol_factor(z, ell, 1e-5)
    return x, omega, z, ell, W, Sq
