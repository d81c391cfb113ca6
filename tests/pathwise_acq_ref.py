"""Numpy restatement of the acquisition over pathwise function draws (hb_sgp_pathwise_acq, PathwiseDraws.acquisition /
select_batch), in float64, from a matrix of values F [S, n] = draws(X).  With sigma = +1 (largest) or -1 and per-draw
incumbents b [S]:

    ei[j] = mean_s max(sigma (F[s, j] - b_s), 0)         pi[j] = mean_s 1[sigma (F[s, j] - b_s) > 0]
    greedy batch: pick j* = argmax (first occurrence), stop at gain 0, b_s <- max / min(b_s, F[s, j*]), up to q times
    joint(F_batch, b0) = mean_s max_i max(sigma (F_batch[s, i] - b0_s), 0)  -- the q-point improvement the gains sum to,
        since max(sigma (f - b), 0) = sigma (max / min(b, f) - b) telescopes over the picks."""
import numpy as np


def _terms(F, b, kind, largest):
    F = np.asarray(F, np.float64)
    b = np.broadcast_to(np.asarray(b, np.float64), (F.shape[0],))[:, None]
    t = (F - b) if largest else (b - F)
    if kind == "ei":
        u = np.where(t > 0.0, t, 0.0)
    elif kind == "pi":
        u = np.where(t > 0.0, 1.0, 0.0)
    else:
        raise ValueError("kind must be 'ei' or 'pi', got %r" % (kind,))
    return np.where(np.isnan(t), t, u)


def mc_acq(F, b, kind="ei", largest=True):
    """The acquisition [n] of the values F [S, n] over the incumbents b (a scalar or [S]); a NaN in a column makes it NaN."""
    u = _terms(F, b, kind, largest)
    return u.sum(0) / u.shape[0]


def pi_count(F, b, largest=True):
    """The number of draws that improve, per column, as integers: pi = count / S exactly."""
    return np.nan_to_num(_terms(F, b, "pi", largest)).sum(0).astype(np.int64)


def greedy_batch(F, b, q, kind="ei", largest=True):
    """(idx int64 [q'], gains [q'], b_final [S]) of the greedy batch over the columns of F."""
    F = np.asarray(F, np.float64)
    b = np.array(np.broadcast_to(np.asarray(b, np.float64), (F.shape[0],)))
    idx, gains = [], []
    for _ in range(q):
        a = mc_acq(F, b, kind, largest)
        if np.all(np.isnan(a)):
            break
        j = int(np.nanargmax(a))
        if a[j] == 0.0:
            break
        idx.append(j)
        gains.append(a[j])
        b = np.maximum(b, F[:, j]) if largest else np.minimum(b, F[:, j])
    return np.asarray(idx, np.int64), np.asarray(gains, np.float64), b


def joint(F_batch, b0, largest=True):
    """mean_s max_i max(sigma (F_batch[s, i] - b0_s), 0): the joint improvement of the batch whose values are F_batch [S, q]."""
    u = _terms(F_batch, b0, "ei", largest)
    return float(u.max(1).sum() / u.shape[0]) if u.shape[1] else 0.0
