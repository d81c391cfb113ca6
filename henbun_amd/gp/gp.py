"""GP / SparseGP posterior draws (reference Henbun/gp/gp.py:9-192).

`SparseGP.samples` with a 2-D x, the UnitRBF kernel and q_shape in
{'diagonal','neglected'} lowers to the fused HIP path (hb_sgp_fwd/bwd: the RBF
cross-covariance block is never materialised and the M^2 n contraction runs on
MFMA); every other case is composed from the generic graph ops the way the
reference composes TensorFlow ops.
"""
from __future__ import annotations

import numpy as np

from .. import graph as G
from .._settings import settings
from ..param import Parameterized, Variable, graph_key
from . import _host, exact
from .kernels import UnitRBF
from .sparse import SparseInference


class GP(Parameterized):
    """Dense GP: samples = u @ chol(K(x))^T (reference gp/gp.py:9-50)."""

    def __init__(self, kern):
        Parameterized.__init__(self)
        self.kern = kern

    def _kern(self):
        return object.__getattribute__(self, "kern")

    def samples(self, x, u):
        L = self._kern().Cholesky(x)
        return G.matmul(u, L, transpose_b=True)

    # -- exact regression at scale: conjugate gradients on a matrix-free kernel product (gp/exact.py) ----------------
    def condition(self, X, Y, noise_var, k_var=1.0, precond_rank=64, tol=None, max_iter=1000):
        """The EXACT posterior of f ~ GP(0, k_var k) given Y = f(X) + N(0, noise_var) at the current lengthscales, as an
        hb.gp.ExactPosterior: alpha = (k_var K(X, X) + noise_var I)^-1 Y from preconditioned conjugate gradients on the
        matrix-free product hb_gram_matvec -- O(N (P + precond_rank)) memory, N^2 d kernel evaluations per iteration, so
        N is limited by time, not by the [N, N] matrix DenseGPR factors.  X [N, d], Y [N, P] with P <= 64 (the columns are
        solved in lockstep): Data / MinibatchData of the model, device tensors or arrays.  precond_rank: rank of the
        pivoted incomplete Cholesky preconditioner (hb_sgp_select on X at threshold 0; 0: plain CG); 64 is a default, not
        a measurement -- profiles/exact_gp_bench.txt records iterations against rank.  tol: |r| <= tol |y| per column on
        the residual itself; None means 1e-6 in a float64 session and 1e-3 in a float32 one.  A float32 session has a
        floor: on 600 points with cond(K^) = 4e3 the smallest tolerance it reached was 3e-5 (50 iterations at rank 64; at
        1e-5 the residual stalls near 3e-5 -- profiles/exact_gp_bench.txt), and the floor rises with the conditioning.
        Not reaching the tolerance within max_iter iterations raises hb.gp.NotConverged, which carries the solve's info.
        UnitRBF with the lengthscales one Variable [dl] only, as SparseGP.statistics: anything else raises
        NotImplementedError.  Hyper-parameters: log_marginal_likelihood_and_grad below (ExactGPR.fit_hyper)."""
        sess, Xd, Yt, ell, tol, precond = self._exact_inputs("condition", X, Y, noise_var, k_var, precond_rank, tol)
        alpha, info = exact.pcg_solve(sess, Xd, ell, k_var, noise_var, Yt, precond, tol, max_iter)
        return exact.ExactPosterior(sess, Xd, Yt, ell, k_var, noise_var, alpha, precond, info, tol, max_iter)

    def _exact_inputs(self, who, X, Y, noise_var, k_var, precond_rank, tol):
        """The validation condition and log_marginal_likelihood share -> (sess, Xd [N, d], Yt [P, N], ell, tol, precond)."""
        sess, _, ls = _host.rbf_model_inputs(self, who)
        Xd, Yd = _host.device_data(sess, X, "X"), _host.device_data(sess, Y, "Y")
        N, d = Xd.shape
        if Yd.shape[0] != N or N < 1:
            raise ValueError("%s: X %s and Y %s do not match" % (who, tuple(Xd.shape), tuple(Yd.shape)))
        if Yd.shape[1] > 64:
            raise NotImplementedError("%s: at most 64 output columns are solved in lockstep (Y has %d)" % (who, Yd.shape[1]))
        if int(ls.shape[0]) not in (1, d):
            raise ValueError("%s: %d lengthscales for X %s" % (who, int(ls.shape[0]), tuple(Xd.shape)))
        ell = _host.lengthscales(sess, ls)
        if tol is None:
            tol = 1e-6 if sess.torch_dtype == sess.torch.float64 else 1e-3
        precond = exact.Preconditioner(sess, Xd, ell, k_var, noise_var, precond_rank) if int(precond_rank) > 0 else None
        return sess, Xd, Yd.t().contiguous(), ell, tol, precond

    def log_marginal_likelihood_and_grad(self, X, Y, noise_var, k_var=1.0, precond_rank=64, tol=None, max_iter=1000,
                                         num_probes=16, seed=0, probes=None, grad=True):
        """(value, grad, info): the log marginal likelihood log p(Y | X) of Y = f(X) + N(0, noise_var), f ~ GP(0, k_var k),
        at the current lengthscales and its gradient grad = dict(lengthscales [dl], k_var, noise_var) (float64, with
        respect to the constrained values), from conjugate gradients on the matrix-free product -- no [N, N] matrix, no
        factorisation (gp/exact.py: log_marginal_likelihood).  The data-fit term is exact to the solve's tolerance; the
        log-determinant and the traces of the gradient are stochastic estimates from num_probes probe vectors, Lanczos
        quadrature on the coefficients of the probes' own solves and one hb_gram_bilinear_grad pass over the kernel
        entries.  The result is a deterministic function of `seed` (common random numbers: the same seed at every step of
        an optimiser gives it a fixed function to climb); probes= injects the probe vectors [T, N], which should have
        covariance P = k_var C^T C + noise_var I, the preconditioner (I at precond_rank = 0).  16 probes is a default,
        not a measurement.  Arguments, validation and NotConverged as for condition."""
        sess, Xd, Yt, ell, tol, precond = self._exact_inputs("log_marginal_likelihood", X, Y, noise_var, k_var, precond_rank, tol)
        return exact.log_marginal_likelihood(sess, Xd, Yt, ell, k_var, noise_var, precond, tol, max_iter, num_probes=num_probes,
                                             seed=seed, probes=probes, grad=grad)

    def log_marginal_likelihood(self, X, Y, noise_var, k_var=1.0, precond_rank=64, tol=None, max_iter=1000, num_probes=16,
                                seed=0, probes=None):
        """The value of log_marginal_likelihood_and_grad alone (the pass over the kernel entries is skipped)."""
        return self.log_marginal_likelihood_and_grad(X, Y, noise_var, k_var, precond_rank, tol, max_iter, num_probes, seed,
                                                     probes, grad=False)[0]


class SparseGP(GP, SparseInference):
    def __init__(self, kern, z, collections=[graph_key.VARIABLES]):
        GP.__init__(self, kern)
        z = np.asarray(z)
        self.z = Variable(shape=z.shape, collections=collections)
        self.z = z  # deferred assignment of the initial inducing locations
        self.m = z.shape[-2]  # z is [m,d], or [E,m,d] for E independent GPs evaluated as one batch

    def _z(self):
        return object.__getattribute__(self, "z").tensor()

    def samples(self, x, u, q_shape="diagonal", eps=None):
        """reference gp/gp.py:99-143.  `eps` optionally injects the standard-normal
        draw of the residual term (shape x.shape[:-1] for 'diagonal')."""
        assert q_shape in ["diagonal", "neglected", "fullrank"]
        x, u = G.as_tensor(x), G.as_tensor(u)
        kern = self._kern()
        z = self._z()
        if len(x.shape) == 2 and isinstance(kern, UnitRBF) and q_shape in ("diagonal", "neglected"):
            Lm = kern.Cholesky(z)
            f, _, _, _ = G.sgp_samples(x, z, kern._ell(), Lm, u, mode=q_shape, eps=eps)
            return f
        # generic composition
        jitter = settings.numerics.jitter_level
        LnT = self._effective_LT(x)
        if len(x.shape) == 2:
            samples = G.matmul(u, LnT)
        else:
            samples = G.squeeze(G.matmul(G.expand_dims(u, 1), LnT), [1])
        if q_shape == "neglected":
            return samples
        if q_shape == "diagonal":
            diag_cov = self._additional_cov(x, LnT, "diagonal")
            noise = G.random_normal(x.shape[:-1]) if eps is None else G.as_tensor(eps)
            return G.add(samples, G.mul(G.unary("SQRT", G.unary("ABS", diag_cov)), noise))
        n = x.shape[-2]
        N = u.shape[0]
        chol = G.cholesky(G.add_eye(self._additional_cov(x, LnT, "fullrank"), jitter))
        if len(x.shape) == 2:
            noise = G.random_normal([N, n]) if eps is None else G.as_tensor(eps)
            return G.add(samples, G.matmul(noise, chol, transpose_b=True))
        noise = G.random_normal([N, 1, n]) if eps is None else G.as_tensor(eps)
        return G.add(samples, G.squeeze(G.matmul(noise, chol, transpose_b=True), [1]))

    def predict_f(self, x, q, q_shape="diagonal", full_cov=False):
        """Closed-form (mean, var) of the draw `samples(x, u, q_shape)` makes, u being the sample of the Variational `q`:
        with A = Lm^-1 K(z, x) and u ~ N(m, S S^T),
            mean = m A,   var = ||S^T A_j||^2 + r_j,
        r = |kdiag - colsum(A^2)| ('diagonal', the |v| samples() takes the root of), 0 ('neglected'),
        kdiag - colsum(A^2) + jitter ('fullrank': the diagonal of the covariance samples() factorises).
        Both are graph tensors with the shape of samples()' output.  Not in the reference (its only route to a
        prediction is averaging draws); in the spirit of GPflow's predict_f.  Forward only: gradients through either
        output raise NotImplementedError.  `q` is read through its parameters -- no noise is drawn and the
        Variational's per-trace draw is left alone.  A 2-D x with the UnitRBF kernel lowers to hb_sgp_predict (fused
        streaming kernel or column chunks, settings.runtime.fused_predict); every other case is composed from generic
        graph ops with the same semantics.

        full_cov=True returns (mean, cov) instead: the same mean tensor and cov [.., P, n, n], the exact covariance of
        that draw,
            cov_p = A^T S_p S_p^T A + K(x, x) - A^T A + jitter I   ('fullrank': what samples() factorises, plus u)
                  = A^T S_p S_p^T A + diag(|kdiag - colsum(A^2)|)  ('diagonal': independent residuals)
                  = A^T S_p S_p^T A                                ('neglected'),
        so diag(cov) == var.  A 2-D x with UnitRBF and a diagonal S, or a full-rank S for one latent function of one
        expert, lowers to hb_sgp_predict_cov (bitwise symmetric) while settings.runtime.fused_predict is on; everything
        else is composed from generic graph ops.  3-D x raises NotImplementedError."""
        assert q_shape in ["diagonal", "neglected", "fullrank"]
        m, s, s_kind = _posterior_of(q)
        x = G.as_tensor(x)
        kern = self._kern()
        z = self._z()
        jitter = settings.numerics.jitter_level
        if full_cov and len(x.shape) != 2:
            raise NotImplementedError("predict_f(full_cov=True) takes a 2-D x [n, d] only (got %s)" % (tuple(x.shape),))
        if len(x.shape) == 2:
            lead = tuple(z.shape[:-2])
            if len(m.shape) < 2 or tuple(m.shape[:-2]) != lead or m.shape[-1] != z.shape[-2]:
                raise ValueError("predict_f: the variational's shape %s does not match [.., P, %d] for z %s"
                                 % (tuple(m.shape), z.shape[-2], tuple(z.shape)))
            if isinstance(kern, UnitRBF):
                mean, var = G.sgp_predict(x, z, kern._ell(), kern.Cholesky(z), m, s, mode=q_shape, s_kind=s_kind,
                                          jitter=jitter)
                if not full_cov:
                    return mean, var
                P = m.shape[-2]
                E = int(np.prod(lead)) if lead else 1
                if bool(getattr(settings.runtime, "fused_predict", True)) and (s_kind == "diag" or E * P == 1):
                    return mean, G.sgp_predict_cov(x, z, kern._ell(), kern.Cholesky(z), s, P, mode=q_shape,
                                                   s_kind=s_kind, jitter=jitter)
                return mean, self._predict_cov_generic(x, m, s, s_kind, q_shape, jitter)
        mean, var = self._predict_generic(x, m, s, s_kind, q_shape, jitter)
        if not full_cov:
            return mean, var
        return mean, self._predict_cov_generic(x, m, s, s_kind, q_shape, jitter)

    def predict_f_samples(self, x, q, num_samples, q_shape="fullrank"):
        """num_samples joint posterior draws at x, [.., P, num_samples, n]: mean + eps L^T with (mean, cov) of
        predict_f(x, q, q_shape, full_cov=True), L = cholesky(cov) and a fresh standard-normal eps every run.  'neglected'
        raises ValueError (its cov has rank at most the number of inducing points).  A cov that is not positive definite
        reports through plan.check() like every factorisation: fp32 draws on a grid much denser than the lengthscale
        need a larger settings.numerics.jitter_level.  Forward only; no draw is taken from q."""
        if q_shape == "neglected":
            raise ValueError("predict_f_samples: the 'neglected' covariance A^T S S^T A has rank at most M and cannot be "
                             "factorised; use 'fullrank' or 'diagonal'")
        mean, cov = self.predict_f(x, q, q_shape=q_shape, full_cov=True)
        chol = G.cholesky(cov)                                              # [.., P, n, n]
        S, n = int(num_samples), cov.shape[-1]
        eps = G.random_normal(tuple(cov.shape[:-2]) + (S, n))               # [.., P, S, n]
        return G.add(G.expand_dims(mean, -2), G.matmul(eps, chol, transpose_b=True))

    def _predict_generic(self, x, m, s, s_kind, q_shape, jitter):
        """predict_f composed from generic graph ops (non-RBF kernels, 3-D x), the way samples() composes its draw."""
        LnT = self._effective_LT(x)                       # 2-D x: [.., M, n];  3-D x [N, n, d]: [N, M, n]
        A2 = G.reduce_sum(G.square(LnT), -2)              # [.., n] / [N, n]
        kd = self._kern().Kdiag(x)
        if len(x.shape) == 2:
            P, M = m.shape[-2], m.shape[-1]
            lead = tuple(m.shape[:-2])
            mean = G.matmul(m, LnT)
            if s_kind == "diag":
                var = G.matmul(G.square(s), G.square(LnT))
            else:
                R = s.shape[-1]
                A4 = G.broadcast_to(G.expand_dims(LnT, -3), lead + (P, M, LnT.shape[-1]))
                C = G.matmul(G.reshape(s, lead + (P, M, R)), A4, transpose_a=True)     # S_ep^T A_e  [.., P, R, n]
                var = G.reduce_sum(G.square(C), -2)
            kd, A2 = G.expand_dims(kd, -2), G.expand_dims(A2, -2)
        else:
            N, M = m.shape[0], m.shape[-1]
            mean = G.squeeze(G.matmul(G.expand_dims(m, 1), LnT), [1])
            if s_kind == "diag":
                var = G.squeeze(G.matmul(G.expand_dims(G.square(s), 1), G.square(LnT)), [1])
            else:
                C = G.matmul(G.reshape(s, [N, M, s.shape[-1]]), LnT, transpose_a=True)  # [N, R, n]
                var = G.reduce_sum(G.square(C), -2)
        if q_shape == "diagonal":
            var = G.add(var, G.unary("ABS", G.sub(kd, A2)))
        elif q_shape == "fullrank":
            var = G.add(var, G.affine(G.sub(kd, A2), 1.0, jitter))
        return mean, var

    def _predict_cov_generic(self, x, m, s, s_kind, q_shape, jitter):
        """predict_f(full_cov=True)'s covariance [.., P, n, n] composed from generic graph ops (2-D x): other kernels, a
        full-rank S for several latent functions, settings.runtime.fused_predict = False."""
        LnT = self._effective_LT(x)                       # [.., M, n]
        P, M, n = m.shape[-2], m.shape[-1], LnT.shape[-1]
        lead = tuple(m.shape[:-2])
        A4 = G.broadcast_to(G.expand_dims(LnT, -3), lead + (P, M, n))
        if s_kind == "diag":
            C = G.mul(G.expand_dims(s, -1), A4)                                           # diag(s_p) A    [.., P, M, n]
        else:
            C = G.matmul(G.reshape(s, lead + (P, M, s.shape[-1])), A4, transpose_a=True)  # S_ep^T A_e     [.., P, R, n]
        cov = G.matmul(C, C, transpose_a=True)
        if q_shape == "fullrank":
            cov = G.add(cov, G.expand_dims(G.add_eye(self._additional_cov(x, LnT, "fullrank"), jitter), -3))
        elif q_shape == "diagonal":
            r = G.unary("ABS", self._additional_cov(x, LnT, "diagonal"))                 # [.., n]
            cov = G.add(cov, G.expand_dims(G.matrix_diag(r), -3))
        return cov

    def _effective_LT(self, x):
        """Lm^{-1} K(z, x) (reference gp/gp.py:146-174)."""
        x = G.as_tensor(x)
        kern = self._kern()
        z = self._z()
        Lm = kern.Cholesky(z)
        if len(x.shape) == 2:
            return G.triangular_solve(Lm, kern.K(z, x))
        if len(x.shape) == 3:
            # batched branch: explicit inverse, broadcast over the batch (no tiling needed)
            return G.matmul(G.trinv(Lm), kern.K(z, x))
        raise ValueError("shape is not specified for tensor x")

    def _additional_cov(self, x, LnT, q_shape):
        """K(x,x) - K(x,z) Kmm^-1 K(z,x) (reference gp/gp.py:177-192)."""
        kern = self._kern()
        if q_shape == "diagonal":
            return G.sub(kern.Kdiag(x), G.reduce_sum(G.square(LnT), -2))
        return G.sub(kern.K(x), G.matmul(LnT, LnT, transpose_a=True))


def _posterior_of(q):
    """(m, s, s_kind) of u ~ N(m, S S^T) for the Variational whose sample samples() consumes, as graph tensors read from
    its parameters (never from its sample): m shaped like the sample; s = the standard deviations (s_kind 'diag') or the
    dense lower-triangular factor [size, size] ('tril').  Gaussian: m = scale m, S = diag(scale) S."""
    from .. import transforms
    from ..variationals import Gaussian, Normal, Variational

    if isinstance(q, (G.Tensor, np.ndarray)) or not isinstance(q, Variational):
        raise TypeError("predict_f needs the Variational object itself, not a sample of it (got %s): call predict_f "
                        "outside tf_mode, or pass object.__getattribute__(model, 'u')" % type(q).__name__)
    if type(q) not in (Normal, Gaussian):
        raise NotImplementedError("predict_f: closed-form moments for %s are not implemented (Normal and Gaussian only)"
                                  % type(q).__name__)
    if q.is_local:
        raise NotImplementedError("predict_f: a LOCAL variational (fed by an encoder) has no closed-form prediction here")
    if q.n_layers or q.n_batch is not None:
        raise NotImplementedError("predict_f: variationals with n_layers / n_batch are not supported")
    if not isinstance(q.transform, transforms.Identity):
        raise NotImplementedError("predict_f: the moments are closed-form only for the Identity transform")
    mu, sq = q._raw_params()
    shape = list(q._shape)
    m = G.reshape(mu, shape)
    scale = object.__getattribute__(q, "scale").tensor() if type(q) is Gaussian else None
    if q.q_shape == "diagonal":
        s, kind = G.reshape(G.unary("EXP", sq), shape), "diag"
        if scale is not None:
            s = G.mul(scale, s)
    else:
        s, kind = (q._dense_sqrt(sq) if q.packed else G.band_part(sq, -1, 0)), "tril"
        if scale is not None:
            s = G.mul(G.reshape(G.broadcast_to(scale, shape), [q.size, 1]), s)
    if scale is not None:
        m = G.mul(scale, m)
    return m, s, kind
