"""Numpy restatement of the closed-form optimal q(u) and the collapsed bound of the whitened sparse GP regression model

    u_p ~ N(0, I_M),   f_p = sqrt(k_var) (u_p A + residual),   Y_p ~ N(f_p, noise_var),   A = Lm^-1 K(z, X)  [M, N],
    Lm = chol(K(z, z) + jitter I),   k = UnitRBF:  exp(-0.5 sum_d ((x_d - z_d) / ell_d)^2)

written from the formulas (Titsias 2009), in float64 unless a dtype is asked for.  Sufficient statistics of the data:

    Phi = A A^T [M, M],   b = (A Y)^T [P, M],   yy = sum_j Y_jp^2 [P],   a2sum = tr Phi.

With c_p = sqrt(k_var) b_p / noise_var and Lambda = I + (k_var / noise_var) Phi the optimum over q(u_p) = N(m_p, S S^T) is
m_p = Lambda^-1 c_p, S S^T = Lambda^-1, and the ELBO there is `collapsed_bound`.  `elbo_direct` is the ELBO of ANY (m, S),
written out term by term with no shortcut through Lambda: the tests pin one against the other."""
import numpy as np


def rbf(z, x, ell):
    """K(z, x) [M, N] for z [M, d], x [N, d], ell [1] or [d], in the dtype of z."""
    zs, xs = z / ell, x / ell
    r2 = np.zeros((z.shape[0], x.shape[0]), dtype=zs.dtype)
    for k in range(z.shape[1]):
        r2 += (zs[:, k, None] - xs[None, :, k]) ** 2
    return np.exp(-0.5 * r2)


def chol_factor(z, ell, jitter):
    """(Lm, W = Lm^-1) of K(z, z) + jitter I."""
    K = rbf(z, z, ell) + jitter * np.eye(z.shape[0], dtype=z.dtype)
    L = np.linalg.cholesky(K)
    W = np.linalg.solve(L, np.eye(z.shape[0], dtype=z.dtype)).astype(z.dtype)
    return L, np.tril(W)


def A_of(W, z, x, ell):
    return W @ rbf(z, x, ell)


def stats_from_W(X, Y, z, ell, W, dtype=np.float64, chunk=32768, ksplit=None):
    """(Phi, b, yy, a2sum) as float64 for a given W = Lm^-1.  dtype float64: one product over all of X.  dtype float32:
    the float32 form of the device kernel -- inputs rounded to float32, A formed in float32, the products taken in float32
    over column blocks of at most `ksplit` (inside chunks of `chunk`), the block results summed in float64."""
    X, Y, z, ell, W = (np.asarray(a, dtype=dtype) for a in (X, Y, z, ell, W))
    N, M, P = X.shape[0], z.shape[0], Y.shape[1]
    Phi = np.zeros((M, M))
    b = np.zeros((P, M))
    step = N if dtype == np.float64 else min(chunk, ksplit or chunk)
    for j0 in range(0, N, step):
        A = A_of(W, z, X[j0:j0 + step], ell)
        Phi += (A @ A.T).astype(np.float64)
        b += (A @ Y[j0:j0 + step]).T.astype(np.float64)
    Phi = np.tril(Phi) + np.tril(Phi, -1).T
    yy = (Y.astype(np.float64) ** 2).sum(0)
    return Phi, b, yy, float(np.trace(Phi))


def stats(X, Y, z, ell, jitter):
    _, W = chol_factor(np.asarray(z, np.float64), np.asarray(ell, np.float64), jitter)
    return stats_from_W(X, Y, z, ell, W)


def optimal_q(Phi, b, noise_var, k_var=1.0):
    """(m [P, M], S [M, M] lower with positive diagonal, s_diag [M], Lambda)."""
    M = Phi.shape[0]
    Lam = np.eye(M) + (k_var / noise_var) * Phi
    c = np.sqrt(k_var) * b / noise_var
    m = np.linalg.solve(Lam, c.T).T
    S = np.linalg.cholesky(np.linalg.inv(Lam))
    return m, S, 1.0 / np.sqrt(np.diag(Lam)), Lam


def collapsed_bound(Phi, b, yy, a2sum, N, noise_var, k_var=1.0, residual="diagonal"):
    P, M = b.shape
    Lam = np.eye(M) + (k_var / noise_var) * Phi
    c = np.sqrt(k_var) * b / noise_var
    L = np.linalg.cholesky(Lam)
    t = np.linalg.solve(L, c.T)                       # [M, P]
    val = np.sum(-0.5 * N * np.log(2 * np.pi * noise_var) - yy / (2 * noise_var) + 0.5 * (t * t).sum(0))
    val -= P * np.log(np.diag(L)).sum()
    if residual == "diagonal":
        val -= P * k_var * (N - a2sum) / (2 * noise_var)
    return float(val)


def elbo_direct(m, S, A, Y, noise_var, k_var=1.0, residual="diagonal"):
    """E_q[log p(Y | f)] - KL(q || N(0, I)) of q(u_p) = N(m_p, S S^T), S [M, M] (shared) or [P, M, M], written out:
    E (y - f)^2 = (y - sqrt(k) m A_j)^2 + k (|S^T A_j|^2 + r_j), r_j = |1 - sum_m A_mj^2| ('diagonal') or 0."""
    P, M = m.shape
    N = A.shape[1]
    S = np.broadcast_to(S, (P, M, M))
    r = np.abs(1.0 - (A * A).sum(0)) if residual == "diagonal" else np.zeros(N)
    val = 0.0
    for p in range(P):
        mean = np.sqrt(k_var) * (m[p] @ A)
        var = k_var * (((S[p].T @ A) ** 2).sum(0) + r)
        val += np.sum(-0.5 * np.log(2 * np.pi * noise_var) - ((Y[:, p] - mean) ** 2 + var) / (2 * noise_var))
        Sig = S[p] @ S[p].T
        val -= 0.5 * (np.trace(Sig) + m[p] @ m[p] - M - np.linalg.slogdet(Sig)[1])
    return float(val)


def predict(Xs, z, ell, jitter, m, S, k_var=1.0, residual="diagonal", W=None):
    """Posterior (mean [P, n], var [P, n]) of f at Xs for q(u_p) = N(m_p, S S^T); S [M, M] or the diagonal's s [M]."""
    z = np.asarray(z, np.float64)
    if W is None:
        _, W = chol_factor(z, np.asarray(ell, np.float64), jitter)
    A = A_of(np.asarray(W, np.float64), z, np.asarray(Xs, np.float64), np.asarray(ell, np.float64))
    S = np.diag(S) if np.ndim(S) == 1 else S
    r = np.abs(1.0 - (A * A).sum(0)) if residual == "diagonal" else 0.0
    mean = np.sqrt(k_var) * (m @ A)
    var = k_var * (((S.T @ A) ** 2).sum(0) + r)
    return mean, np.broadcast_to(var, mean.shape).copy()
