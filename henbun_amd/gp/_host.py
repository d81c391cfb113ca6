"""Host-side steps the eager inference routes share (gp/sparse.py, gp/exact.py, the GP methods of gp/gp.py that call
them, models.py): who may call, uploads, the factorise-and-raise idiom, the chunk size of the float64 walks and the
scalar value of the collapsed bound.  Nothing here launches a kernel of its own; everything that does not take a
session or `H` (hip_ops) runs without a device."""
import numpy as np

from .. import graph as G
from ..param import Data, Variable
from .kernels import UnitRBF


def rbf_model_inputs(gp, who):
    """(sess, kern, ls) for a GP the eager routes cover: part of a Model (else ValueError), the UnitRBF kernel with its
    lengthscales one Variable [dl] (else NotImplementedError).  Pending assignments are uploaded once all of it holds."""
    root = gp.highest_parent
    sess = getattr(root, "_session", None)
    if sess is None:
        raise ValueError("%s needs the GP to be part of a Model" % who)
    kern = object.__getattribute__(gp, "kern")
    if not isinstance(kern, UnitRBF):
        raise NotImplementedError("%s is implemented for the UnitRBF kernel only (got %s)" % (who, type(kern).__name__))
    ls = object.__getattribute__(kern, "lengthscales")
    if not isinstance(ls, Variable) or len(ls.shape) != 1:
        raise NotImplementedError("%s: one expert only, the lengthscales must be one Variable [dl]" % who)
    root.initialize()
    return sess, kern, ls


def upload(sess, a, dtype=None, carry=None):
    """`a` as a contiguous device tensor, rounded to `dtype` (None: the session's) on the host.  carry=np.float64 then
    stores the ROUNDED values in double: the parameters as a float32 session holds them, for the float64 routes."""
    a = np.asarray(a, dtype=sess.np_dtype if dtype is None else dtype)
    if carry is not None:
        a = a.astype(carry)
    return sess.torch.as_tensor(np.ascontiguousarray(a)).to(sess.device)


def lengthscales(sess, ls, dtype=None, carry=None):
    """The value of the lengthscale Variable `ls` as a flat device tensor [dl]; dtype, carry as for upload."""
    return upload(sess, np.reshape(sess.read_value(ls), [-1]), dtype, carry)


def device_data(sess, a, name):
    """X / Y as a contiguous [N, k] device tensor of the session's dtype: a Data / MinibatchData of the model is read
    from its device-resident buffer (all rows), a device tensor is taken as it is, anything else is uploaded."""
    if isinstance(a, Data):
        t = sess.data_buffer(a)
    elif isinstance(a, sess.torch.Tensor):
        t = a.to(device=sess.device, dtype=sess.torch_dtype)
    else:
        t = upload(sess, a)
    if t.dim() != 2:
        raise ValueError("%s must be 2-D [N, k], got %s" % (name, tuple(t.shape)))
    return t.contiguous()


def pathwise_noise(sess, who, noise, seed, shapes, double=False):
    """(omega, w, eps) of a PathwiseDraws with the given shapes, in the session's dtype or (double) float64: drawn from
    hip_ops.Rng(seed) in that order (noise=None), or the arrays of noise=dict(omega=, w=, eps=), else ValueError."""
    names = ("omega", "w", "eps")
    if noise is None:
        rng = sess.H.Rng(seed, device=sess.device)
        return tuple(rng.normal(s, dtype=sess.torch.float64 if double else sess.torch_dtype) for s in shapes)
    if not isinstance(noise, dict) or set(noise) != set(names) or any(np.shape(noise[k]) != s for k, s in zip(names, shapes)):
        raise ValueError("%s: noise must be dict(omega=%s, w=%s, eps=%s)" % ((who,) + tuple(shapes)))
    return tuple(upload(sess, noise[k], np.float64 if double else None) for k in names)


def ascent_box(who, Xd, bounds, d, dt):
    """(lo, hi, lo_r, hi_r) of a projected ascent over candidates Xd [n, d]: bounds = (lo [d], hi [d]) in float64 (None:
    the per-column minimum and maximum of the candidates) and the box as the numpy type `dt` can hold it, so that the
    rounded iterates stay inside [lo, hi].  Bounds of another shape or with lo > hi raise ValueError."""
    if bounds is None:
        lo, hi = (np.asarray(t.cpu().numpy(), np.float64) for t in (Xd.min(dim=0).values, Xd.max(dim=0).values))
    else:
        if len(bounds) != 2:
            raise ValueError("%s: bounds = (lo [d], hi [d]) expected" % who)
        lo, hi = (np.asarray(b, np.float64) for b in bounds)
        if lo.shape != (d,) or hi.shape != (d,) or not np.all(lo <= hi):
            raise ValueError("%s: bounds = (lo [%d], hi [%d]) with lo <= hi expected" % (who, d, d))
    lo_r, hi_r = lo.astype(dt), hi.astype(dt)
    lo_r = np.where(lo_r < lo, np.nextafter(lo_r, dt(np.inf)), lo_r)
    hi_r = np.where(hi_r > hi, np.nextafter(hi_r, dt(-np.inf)), hi_r)
    return lo, hi, lo_r, hi_r


def adam_ascent(evaluate, x, f0, ell, box, sign, steps, lr, dt):
    """(x_best [R, d], f_best [R]): R independent projected Adam ascents (descents with sign = -1) from the rows of x
    [R, d] (numpy, type `dt`) whose values f0 [R] are known.  evaluate(x) -> (f [R], g [R, d] float64) at the current
    points.  The optimiser runs on the host in float64 (beta = 0.9 / 0.999, epsilon = 1e-8) in lengthscale units
    u = x / ell, d f / d u = ell d f / d x; after each step u is projected onto `box` (ascent_box) and rounded to `dt`.
    `steps` steps take steps + 1 evaluations -- the start, for its gradient, and the point after every step; steps = 0
    takes none.  The best (value, point) seen is kept per row, the start included."""
    lo, hi, lo_r, hi_r = box
    x_best, f_best = x.copy(), f0.copy()
    u = x.astype(np.float64) / ell
    m1, m2 = np.zeros_like(u), np.zeros_like(u)
    b1, b2, eps = 0.9, 0.999, 1e-8
    if steps:   # steps + 1 evaluations: t = 0 is the start (its value is known, its gradient is not)
        for t in range(steps + 1):
            f, g = evaluate(x)
            better = sign * f.astype(np.float64) > sign * f_best.astype(np.float64)
            x_best[better], f_best[better] = x[better], f[better]
            if t == steps:
                break
            gu = sign * ell * g
            m1 = b1 * m1 + (1.0 - b1) * gu
            m2 = b2 * m2 + (1.0 - b2) * gu ** 2
            u = u + float(lr) * (m1 / (1.0 - b1 ** (t + 1))) / (np.sqrt(m2 / (1.0 - b2 ** (t + 1))) + eps)
            u = np.clip(u, lo / ell, hi / ell)
            x = np.clip((u * ell).astype(dt), lo_r, hi_r)
            x = np.where(u >= hi / ell, hi_r, np.where(u <= lo / ell, lo_r, x))   # on a face: the face itself, exactly
    return x_best, f_best


def greedy_batch(argmax_fn, eval_fn, b0, q, sign):
    """(picks, gains float64 [q'], b [S]): the greedy construction of a batch for the joint Monte-Carlo improvement
    E max_i (sign (f(x_i) - b0))_+ of S function draws with per-draw incumbents b0 [S] (Wilson et al. 2020, section 5).
    Up to q times: argmax_fn(b) -> (idx, gain, x), the best next point under the current incumbents b and its marginal
    gain mean_s (sign (f_s(x) - b_s))_+; the loop ends early, before taking the point, when idx < 0 (nothing comparable)
    or the gain is exactly 0 (no draw improves anywhere: every further gain would be 0 too), so q' <= q; otherwise
    eval_fn(x) -> f [S], the draws at the point, and b <- max(b, f) (min for sign = -1).  picks: the (idx, x) pairs in
    order.  The gains telescope: their sum is mean_s sign (b_s - b0_s), the joint improvement of the batch; with exact
    arg-max values they never increase, since b only rises.  Callables only: runs without a device."""
    b = np.array(b0, copy=True)
    picks, gains = [], []
    for _ in range(int(q)):
        idx, gain, x = argmax_fn(b)
        if idx < 0 or gain == 0:
            break
        f = np.asarray(eval_fn(x), dtype=b.dtype).reshape(b.shape)
        b = np.maximum(b, f) if sign > 0 else np.minimum(b, f)
        picks.append((int(idx), x))
        gains.append(float(gain))
    return picks, np.asarray(gains, np.float64), b


def check_info(info, who, of, exc=G.CholeskyError):
    """ONE read-back of a factorisation's `info`; a leading minor of `of` that is not positive raises `exc`."""
    bad = int(info.cpu()[0])
    if bad != 0:
        raise exc("%s: leading minor %d of %s is not positive definite" % (who, bad, of))


def factor(H, A, who, of, exc=G.CholeskyError):
    """L = chol(A) by hb_cholesky, checked by check_info."""
    L, info = H.cholesky(A)
    check_info(info, who, of, exc)
    return L


def f64_chunk_rows(M, align=1):
    """Rows per chunk of a float64 walk over the data: 2^24 / M, within [32, 32768], rounded down to a multiple of
    `align`.  The chunks' sums are added in chunk order, so a walk's bits depend on its cuts: each keeps its `align`."""
    return int(min(32768, max(32, (1 << 24) // int(M)))) // align * align


def collapsed_value(N, P, noise_var, k_var, yy, quad, logdet, a2sum, residual):
    """The collapsed bound (SparseGP.collapsed_bound) from its scalars: logdet = log|Lambda|, a2sum = tr Phi, and yy =
    sum_j Y_jp^2, quad = c_p^T Lambda^-1 c_p either per column [P] (added over p last: collapsed_bound's order) or as
    floats summed over p on the device (the gradient route).  For P > 1 the two can differ in the last bit."""
    s2 = float(noise_var)
    if np.ndim(yy):
        val = float(np.sum(-0.5 * N * np.log(2.0 * np.pi * s2) - yy / (2.0 * s2) + 0.5 * quad))
    else:
        val = -0.5 * N * P * np.log(2.0 * np.pi * s2) - yy / (2.0 * s2) + 0.5 * quad
    val -= 0.5 * P * logdet
    if residual == "diagonal":
        val -= P * float(k_var) * (N - a2sum) / (2.0 * s2)
    return float(val)
