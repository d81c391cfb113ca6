"""float64 numpy reference for the stationary Gram kernels (csrc/gram.hip, csrc/gram_value.cuh) and their VJP.

With a = x / ell, b = x2 / ell, E- = exp(-|a - b|^2 / 2), E+ = exp(-|a + b|^2 / 2):
    RBF       K = E-                SQDIST   K = |a - b|^2            CSYM_RBF   K = E- + E+
Every function also returns, for each output entry, S: the sum of the magnitudes of the terms the entry is a sum of,
taken down to the terms that are rounded.  The kernels round a and b before they subtract them, so a difference a - b
carries an absolute error of 2^-24 (|a| + |b|) however small it is: wherever a factor a - b (or a + b) enters a term, S
takes |a| + |b| for it.  The squared distance is thus measured by c = sum_k |a_k - b_k| (|a_k| + |b_k|) >= r^2, and each
exponential is weighted by (1 + c / 2): an error delta * c of r^2 becomes delta * c / 2 * exp(-r^2 / 2).
A float32 kernel is allowed k * 2^-24 * S, with k counted from its operation sequence.
"""
import numpy as np

RBF, CSYM, SQDIST = 0, 1, 2


def _pairs(X, X2, ell):
    """X [B,n,d], X2 [B or 1,n2,d], ell [B or 1,dl] -> il [B|1,1,1,d], a - b, a + b, |a| + |b| [B,n,n2,d], r2, r2p and
    their magnitudes cm, cp [B,n,n2]"""
    d = X.shape[-1]
    il = 1.0 / np.broadcast_to(ell[:, None, None, :], (ell.shape[0], 1, 1, d))
    a, b = X[:, :, None, :] * il, X2[:, None, :, :] * il
    dm, dp, ab = a - b, a + b, np.abs(a) + np.abs(b)
    return il, dm, dp, ab, (dm * dm).sum(-1), (dp * dp).sum(-1), (np.abs(dm) * ab).sum(-1), (np.abs(dp) * ab).sum(-1)


def gram(kind, X, X2, ell):
    """K [B,n,n2] and its S"""
    _, _, _, _, r2, r2p, cm, cp = _pairs(X, X2, ell)
    if kind == SQDIST:
        return r2, cm
    em = np.exp(-0.5 * r2)
    K, S = em, em * (1 + 0.5 * cm)
    if kind == CSYM:
        ep = np.exp(-0.5 * r2p)
        K, S = K + ep, S + ep * (1 + 0.5 * cp)
    return K, S


def gram_vjp(kind, X, X2, ell, Kbar):
    """(Xbar [B,n,d], X2bar [B,n2,d], ellbar [B,d]) per batch entry and per dimension, and their S in the same layout;
    the caller sums over the batch for shared operands and over d for a single lengthscale (S adds up alike)."""
    il, dm, dp, ab, r2, r2p, cm, cp = _pairs(X, X2, ell)
    if kind == SQDIST:
        km, wm = np.full_like(r2, -2.0), np.full_like(r2, 2.0)
    else:
        km = np.exp(-0.5 * r2)
        wm = km * (1 + 0.5 * cm)
    if kind == CSYM:
        kp = np.exp(-0.5 * r2p)
        wp = kp * (1 + 0.5 * cp)
    else:
        kp = wp = np.zeros_like(r2)
    kb, akb = Kbar[..., None], np.abs(Kbar)[..., None]
    km, kp, wm, wp = km[..., None], kp[..., None], wm[..., None], wp[..., None]
    tx = kb * (-dm * km - dp * kp) * il
    tx2 = kb * (dm * km - dp * kp) * il
    tl = kb * (dm * dm * km + dp * dp * kp) * il
    sx = akb * (ab * wm + ab * wp) * il
    sl = akb * (np.abs(dm) * ab * wm + np.abs(dp) * ab * wp) * il
    out = (tx.sum(2), tx2.sum(1), tl.sum((1, 2)))
    S = (sx.sum(2), sx.sum(1), sl.sum((1, 2)))
    return out, S
