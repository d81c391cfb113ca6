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
