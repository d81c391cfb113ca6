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
from .kernels import UnitRBF


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
        from . import exact

        sess, Xd, Yt, ell, tol, precond = self._exact_inputs("condition", X, Y, noise_var, k_var, precond_rank, tol)
        alpha, info = exact.pcg_solve(sess, Xd, ell, k_var, noise_var, Yt, precond, tol, max_iter)
        return exact.ExactPosterior(sess, _device_data, Xd, Yt, ell, k_var, noise_var, alpha, precond, info, tol, max_iter)

    def _exact_inputs(self, who, X, Y, noise_var, k_var, precond_rank, tol):
        """The validation condition and log_marginal_likelihood share -> (sess, Xd [N, d], Yt [P, N], ell, tol, precond)."""
        from . import exact

        root = self.highest_parent
        sess = getattr(root, "_session", None)
        if sess is None:
            raise ValueError("%s needs the GP to be part of a Model" % who)
        kern = self._kern()
        if not isinstance(kern, UnitRBF):
            raise NotImplementedError("%s: exact regression is implemented for the UnitRBF kernel only (got %s)"
                                      % (who, type(kern).__name__))
        ls = object.__getattribute__(kern, "lengthscales")
        if not isinstance(ls, Variable) or len(ls.shape) != 1:
            raise NotImplementedError("%s: one expert only, the lengthscales must be one Variable [dl]" % who)
        root.initialize()
        Xd, Yd = _device_data(sess, X, "X"), _device_data(sess, Y, "Y")
        N, d = Xd.shape
        if Yd.shape[0] != N or N < 1:
            raise ValueError("%s: X %s and Y %s do not match" % (who, tuple(Xd.shape), tuple(Yd.shape)))
        if Yd.shape[1] > 64:
            raise NotImplementedError("%s: at most 64 output columns are solved in lockstep (Y has %d)" % (who, Yd.shape[1]))
        if int(ls.shape[0]) not in (1, d):
            raise ValueError("%s: %d lengthscales for X %s" % (who, int(ls.shape[0]), tuple(Xd.shape)))
        torch = sess.torch
        ell = torch.as_tensor(np.ascontiguousarray(np.reshape(sess.read_value(ls), [-1]).astype(sess.np_dtype))).to(sess.device)
        if tol is None:
            tol = 1e-6 if sess.torch_dtype == torch.float64 else 1e-3
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
        from . import exact

        sess, Xd, Yt, ell, tol, precond = self._exact_inputs("log_marginal_likelihood", X, Y, noise_var, k_var, precond_rank, tol)
        return exact.log_marginal_likelihood(sess, Xd, Yt, ell, k_var, noise_var, precond, tol, max_iter, num_probes=num_probes,
                                             seed=seed, probes=probes, grad=grad)

    def log_marginal_likelihood(self, X, Y, noise_var, k_var=1.0, precond_rank=64, tol=None, max_iter=1000, num_probes=16,
                                seed=0, probes=None):
        """The value of log_marginal_likelihood_and_grad alone (the pass over the kernel entries is skipped)."""
        return self.log_marginal_likelihood_and_grad(X, Y, noise_var, k_var, precond_rank, tol, max_iter, num_probes, seed,
                                                     probes, grad=False)[0]


class SparseGP(GP):
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

    # -- closed-form posterior (Titsias 2009; the whitened model of models.SVGP) ------------------------------------
    def _stats_session(self):
        root = self.highest_parent
        sess = getattr(root, "_session", None)
        if sess is None:
            raise ValueError("statistics / optimal_q / collapsed_bound need the SparseGP to be part of a Model")
        kern = self._kern()
        if not isinstance(kern, UnitRBF):
            raise NotImplementedError("statistics: the closed-form optimal q(u) is implemented for the UnitRBF kernel only "
                                      "(got %s)" % type(kern).__name__)
        zvar = object.__getattribute__(self, "z")
        if len(zvar.shape) != 2:
            raise NotImplementedError("statistics: one expert only (z must be [M, d], got %s)" % (tuple(zvar.shape),))
        ls = object.__getattribute__(kern, "lengthscales")
        if not isinstance(ls, Variable) or len(ls.shape) != 1:
            raise NotImplementedError("statistics: the lengthscales must be one Variable [dl]")
        root.initialize()
        return sess, zvar, ls

    def _device_data(self, sess, a, name):
        return _device_data(sess, a, name)

    def statistics(self, X, Y):
        """(Phi [M, M], b [P, M], yy [P], a2sum [1]) of the whole data set X [N, d], Y [N, P] for the current z,
        lengthscales and settings.numerics.jitter_level, as float64 device tensors (hb_sgp_stats: one streaming pass):
        Phi = A A^T, b = (A Y)^T, yy_p = sum_j Y_jp^2, a2sum = tr Phi, A = Lm^-1 K(z, X), Lm = chol(K(z, z) + jitter I)
        from the fused factor + inverse the plans use.  A failed factorisation raises graph.CholeskyError."""
        sess, zvar, ls = self._stats_session()
        Xd, Yd = self._device_data(sess, X, "X"), self._device_data(sess, Y, "Y")
        z, ell, W, frag = self._whitening(sess, zvar, ls, Xd, Yd, "statistics")
        return sess.H.sgp_stats(Xd, Yd, z, ell, W, wfrag=frag)

    def _whitening(self, sess, zvar, ls, Xd, Yd, who, as_plans=False):
        """(z, ell, W, frag) on the device in the session's dtype: W = chol(K(z, z) + jitter I)^-1 from the fused factor
        + inverse the plans use, frag its fragment-major images (float32, M % 32 == 0; else None).
        z and the lengthscales are their transforms of the raw parameters taken on the host in double and rounded;
        as_plans=True takes them from a plan instead, i.e. as the session's dtype transforms them on the device -- the
        values predict_f and the ELBO see.  In a float32 session the two can differ in the last bit of a lengthscale,
        which moves W by cond(K(z, z)) times that; a q(u) that a plan reads must be fitted in the plan's whitening
        ("Natural-gradient fit")."""
        torch, H = sess.torch, sess.H
        up = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=sess.np_dtype))).to(sess.device)
        if as_plans:
            sess.read_value(zvar), sess.read_value(ls)      # uploads a value that was assigned and not yet written
            cache = object.__getattribute__(self, "__dict__").setdefault("_whitening_plans", {})
            key = (id(sess), sess.layout_version, id(zvar), id(ls))
            if key not in cache:
                zt, et = zvar.tensor(), G.reshape(ls.tensor(), [-1])
                cache.clear()
                cache[key] = (sess.make_plan([zt, et]), zt, et)
            plan, zt, et = cache[key]
            plan.run()
            z, ell = plan.buf(zt).clone().contiguous(), plan.buf(et).clone().contiguous()
        else:
            z, ell = up(sess.read_value(zvar)), up(np.reshape(sess.read_value(ls), [-1]))
        if Xd is not None and (Xd.shape[0] != Yd.shape[0] or Xd.shape[1] != z.shape[1]):   # (pathwise_draws has no data)
            raise ValueError("%s: X %s, Y %s do not match z %s" % (who, tuple(Xd.shape), tuple(Yd.shape), tuple(z.shape)))
        M = z.shape[0]
        K = H.gram_fwd(z, z, ell, diag_add=float(settings.numerics.jitter_level))
        frag = None
        if sess.torch_dtype == torch.float32 and M % 32 == 0:
            frag = torch.empty(2 * M * M, dtype=sess.torch_dtype, device=sess.device)
        _, W, info = H.cholesky_inverse(K, frag=frag)
        bad = int(info.cpu()[0])
        if bad != 0:
            raise G.CholeskyError("%s: leading minor %d of K(z, z) + jitter I is not positive definite" % (who, bad))
        return z, ell, W, frag

    def select_inducing(self, X, threshold=None):
        """Move z to the M = z.shape[0] rows of X [N, d] that greedy conditional-variance selection picks at the CURRENT
        lengthscales (hb_sgp_select; see greedy_inducing), in selection order, and return their row indices as numpy
        int64 [M].  X: a Data / MinibatchData of the model (read in full from its device buffer), a device tensor or an
        array.  threshold=None: settings.numerics.jitter_level.  Same restrictions and exception types as statistics():
        UnitRBF, one expert, the lengthscales one Variable.  If fewer than M points have a conditional variance above
        the threshold, ValueError is raised and z is left untouched.  q(u) is not touched: the optimum for the new z is
        one optimal_q / fit_q away."""
        sess, zvar, ls = self._stats_session()
        torch, H = sess.torch, sess.H
        Xd = self._device_data(sess, X, "X")
        M, d = int(zvar.shape[0]), int(zvar.shape[1])
        if Xd.shape[1] != d:
            raise ValueError("select_inducing: X %s does not match z %s" % (tuple(Xd.shape), tuple(zvar.shape)))
        if M > Xd.shape[0]:
            raise ValueError("select_inducing: z holds %d points, X only %d rows" % (M, Xd.shape[0]))
        ell = torch.as_tensor(np.ascontiguousarray(np.reshape(sess.read_value(ls), [-1]).astype(sess.np_dtype))).to(sess.device)
        thr = float(settings.numerics.jitter_level if threshold is None else threshold)
        idx, _, count, _ = H.sgp_select(Xd, ell, M, thr)
        count = int(count.cpu()[0])
        if count < M:
            raise ValueError("select_inducing: only %d of the %d points asked for have a conditional variance above the "
                             "threshold %g; z is unchanged (use fewer inducing points or a lower threshold)"
                             % (count, M, thr))
        Z = Xd[idx].cpu().numpy()
        sess.write_raw(zvar, zvar.transform.backward(Z.astype(np.float64)))
        return idx.cpu().numpy()

    def _lambda_solve(self, stats, noise_var, k_var):
        """(Lam, L, V, t, c): Lambda = I + (k_var / noise_var) Phi = L L^T, V = L^-1, c = sqrt(k_var) b / noise_var [P, M],
        t = c V^T [P, M] (so |t_p|^2 = c_p^T Lambda^-1 c_p and t V = Lambda^-1 c), float64 on the device."""
        root = self.highest_parent
        H = root._session.H
        Phi, b = stats[0], stats[1]
        noise_var, k_var = float(noise_var), float(k_var)
        if not (noise_var > 0.0 and k_var > 0.0):
            raise ValueError("noise_var and k_var must be positive (got %r, %r)" % (noise_var, k_var))
        Lam = H.matutil((Phi * (k_var / noise_var)).contiguous(), H.MATUTIL_ADD_EYE, alpha=1.0)
        L, info = H.cholesky(Lam)
        bad = int(info.cpu()[0])
        if bad != 0:
            raise G.CholeskyError("optimal_q: leading minor %d of Lambda = I + (k_var / noise_var) Phi is not positive "
                                  "definite" % bad)
        V = H.trinv(L)
        c = (b * (np.sqrt(k_var) / noise_var)).contiguous()
        t = H.matmul(c, V, transB=True)
        return Lam, L, V, t, c

    @staticmethod
    def _check_residual(residual):
        if residual == "fullrank":
            raise NotImplementedError("the closed-form posterior is implemented for residual 'diagonal' and 'neglected' "
                                      "(the 'fullrank' residual couples the data points)")
        if residual not in ("diagonal", "neglected"):
            raise ValueError("residual must be 'diagonal' or 'neglected', got %r" % (residual,))

    def optimal_q(self, X, Y, noise_var, k_var=1.0, q_shape="fullrank", residual="diagonal", stats=None):
        """The optimum of the ELBO over q(u_p) = N(m_p, S S^T) at fixed hyper-parameters, for the whitened model
        u_p ~ N(0, I), f_p = sqrt(k_var) (u_p A + residual), Y_p ~ N(f_p, noise_var):
            Lambda = I + (k_var / noise_var) Phi,  c_p = sqrt(k_var) b_p / noise_var,  m_p = Lambda^-1 c_p,
        q_shape 'fullrank': S = chol(Lambda^-1), lower-triangular [M, M] with a positive diagonal, the same for every p;
        'diagonal': s = diag(Lambda)^-1/2 [M], the optimum of the mean-field family (the mean is the same).
        Returns (m [P, M], S or s) as float64 numpy.  `residual` ('diagonal' / 'neglected') does not change q*: that
        term of the ELBO does not depend on q.  The M^3 tail runs on the device in float64 (hb_cholesky, hb_trinv,
        hb_matmul).  `stats`: the tuple statistics(X, Y) returned, to share one pass between calls."""
        self._check_residual(residual)
        if q_shape not in ("fullrank", "diagonal"):
            raise ValueError("q_shape must be 'fullrank' or 'diagonal', got %r" % (q_shape,))
        if stats is None:
            stats = self.statistics(X, Y)
        H = self.highest_parent._session.H
        Lam, L, V, t, _ = self._lambda_solve(stats, noise_var, k_var)
        m = H.matmul(t, V).cpu().numpy()
        if q_shape == "diagonal":
            return m, 1.0 / np.sqrt(np.diagonal(Lam.cpu().numpy()).copy())
        Sig = H.matmul(V, V, transA=True)              # Lambda^-1 = V^T V
        S, info = H.cholesky(Sig)
        bad = int(info.cpu()[0])
        if bad != 0:
            raise G.CholeskyError("optimal_q: leading minor %d of Lambda^-1 is not positive definite" % bad)
        return m, np.tril(S.cpu().numpy())

    def collapsed_bound(self, X, Y, noise_var, k_var=1.0, residual="diagonal", stats=None):
        """The ELBO at the optimal q(u) of optimal_q (the collapsed bound), a float:
            sum_p [ -N/2 log(2 pi noise_var) - yy_p / (2 noise_var) + 1/2 c_p^T Lambda^-1 c_p ] - P/2 log|Lambda|
            - P k_var (N - a2sum) / (2 noise_var)          ('diagonal'; 'neglected' drops the last term).
        N - a2sum is sum_j (kdiag_j - sum_m A_mj^2) for the unit-variance kernel.  samples() takes the absolute value of
        that difference per point, so the two agree except where round-off makes a term negative."""
        self._check_residual(residual)
        if stats is None:
            stats = self.statistics(X, Y)
        _, L, _, t, _ = self._lambda_solve(stats, noise_var, k_var)
        noise_var, k_var = float(noise_var), float(k_var)
        yy, a2sum = stats[2].cpu().numpy(), float(stats[3].cpu()[0])
        from ..param import Data

        N = int(self.highest_parent._session.data_buffer(X).shape[0] if isinstance(X, Data) else np.shape(X)[0])
        P = yy.shape[0]
        quad = (t.cpu().numpy() ** 2).sum(-1)                                  # [P]
        logdet = 2.0 * float(np.log(np.diagonal(L.cpu().numpy())).sum())
        val = float(np.sum(-0.5 * N * np.log(2.0 * np.pi * noise_var) - yy / (2.0 * noise_var) + 0.5 * quad))
        val -= 0.5 * P * logdet
        if residual == "diagonal":
            val -= P * k_var * (N - a2sum) / (2.0 * noise_var)
        return val

    def natgrad_q(self, X, Y, likelihood, k_var=1.0, residual="diagonal", q0=None, steps=20, rho=1.0, tol=1e-8):
        """Natural-gradient fit of q(u) = N(m, S S^T) for a factorising likelihood (henbun_amd.likelihoods: Gaussian,
        Bernoulli, Poisson) at fixed hyper-parameters, for the whitened model u ~ N(0, I), f = sqrt(k_var) (u A +
        residual), y_j ~ p(y_j | f_j).  q is kept as Lambda = (S S^T)^-1, eta = Lambda m; one step is the conjugate
        update with per-point pseudo-observations (conjugate-computation VI, Khan & Lin 2017):
            mu_j, v_j            the marginals of f_j under q                         (hb_sgp_predict, one pass over X)
            lam_j, beta_j, l_j   E[-d2 log p], E[d log p] + lam_j mu_j, E[log p]      (hb_lik_sites)
            Phi = A diag(lam) A^T,  b = A beta                                        (hb_sgp_wstats, one pass over X)
            Lambda <- (1 - rho) Lambda + rho (I + k_var Phi),   eta <- (1 - rho) eta + rho sqrt(k_var) b
        and m = Lambda^-1 eta, S = chol(Lambda^-1) from the float64 tail of optimal_q.  With the Gaussian likelihood one
        step at rho = 1 is optimal_q.  K(z, z) is factorised once per call, from z and the lengthscales as the session's
        plans transform them on the device, so the q(u) returned lives in the whitening predict_f and the ELBO use.
        Returns (m [1, M], S [M, M] lower with a positive diagonal, info) as float64 numpy; info = dict(elbo, residual,
        steps): the ELBO sum_j l_j - KL(q || N(0, I)) and the fixed-point residual max|Lambda - (I + k_var Phi)| /
        max|I + k_var Phi| at every iterate, the starting one included (steps + 1 entries), and the steps taken.  m, S
        are the last iterate evaluated.  q0=None starts at the prior; q0 = (m, S) at a given full-rank q.  Stops when
        the relative change of the ELBO is <= tol, or after `steps`.  X, Y as for statistics(), Y [N, 1].  Same
        restrictions and exception types as statistics(); residual 'fullrank' and a mean-field q0 raise
        NotImplementedError; a Lambda that is not positive definite raises graph.CholeskyError.  A full step (rho = 1)
        is not guaranteed to raise the ELBO from a q far from the optimum (info['elbo'] shows an overshoot): start at
        the prior or damp with rho < 1."""
        from ..likelihoods import Likelihood

        self._check_residual(residual)
        if not isinstance(likelihood, Likelihood):
            raise TypeError("natgrad_q: likelihood must be a henbun_amd.likelihoods.Likelihood, got %s" % type(likelihood).__name__)
        k_var, rho, steps = float(k_var), float(rho), int(steps)
        if not (k_var > 0.0 and 0.0 < rho <= 1.0 and steps >= 0):
            raise ValueError("natgrad_q: k_var > 0, 0 < rho <= 1 and steps >= 0 expected (got %r, %r, %r)" % (k_var, rho, steps))
        sess, zvar, ls = self._stats_session()
        torch, H = sess.torch, sess.H
        Xd, Yd = self._device_data(sess, X, "X"), self._device_data(sess, Y, "Y")
        if Yd.shape[1] != 1:
            raise NotImplementedError("natgrad_q: one latent function only (Y must be [N, 1], got %s)" % (tuple(Yd.shape),))
        z, ell, W, frag = self._whitening(sess, zvar, ls, Xd, Yd, "natgrad_q", as_plans=True)
        N, d, M = Xd.shape[0], Xd.shape[1], z.shape[0]
        f64 = dict(dtype=torch.float64, device=sess.device)
        if q0 is None:
            Lam, eta = torch.eye(M, **f64), torch.zeros((1, M), **f64)
        else:
            m0, S0 = (np.asarray(a, dtype=np.float64) for a in q0)
            if S0.ndim != 2:
                raise NotImplementedError("natgrad_q: q0 must be a full-rank q, (m [1, M], S [M, M]); a mean-field q "
                                          "does not stay mean-field under the update")
            if m0.size != M or S0.shape != (M, M):
                raise ValueError("natgrad_q: q0 = (m [1, %d], S [%d, %d]) expected, got %s %s" % (M, M, M, m0.shape, S0.shape))
            Sinv = H.trinv(torch.as_tensor(np.ascontiguousarray(np.tril(S0))).to(sess.device))
            Lam = H.matmul(Sinv, Sinv, transA=True)
            eta = H.matmul(torch.as_tensor(np.ascontiguousarray(m0.reshape(1, M))).to(sess.device), Lam)
        mode = H.SGP_DIAGONAL if residual == "diagonal" else H.SGP_NEGLECTED
        fused = bool(getattr(settings.runtime, "fused_predict", True)) and H.sgp_predict_fused(
            sess.torch_dtype, 1, N, M, d, 1, H.SGP_S_TRIL, frag is not None)
        mean = torch.empty((1, N), dtype=sess.torch_dtype, device=sess.device)
        var, lam, beta = (torch.empty_like(mean) for _ in range(3))
        eye = torch.eye(M, **f64)
        elbo, resid = [], []
        for it in range(steps + 1):
            # the float64 tail of optimal_q: Lambda = L L^T, V = L^-1, m = eta V^T V, S = chol(V^T V)
            L, info = H.cholesky(Lam.contiguous())
            bad = int(info.cpu()[0])
            if bad != 0:
                raise G.CholeskyError("natgrad_q: leading minor %d of Lambda is not positive definite (step %d)" % (bad, it))
            V = H.trinv(L)
            m = H.matmul(H.matmul(eta.contiguous(), V, transB=True), V)
            Sig = H.matmul(V, V, transA=True)
            S, info = H.cholesky(Sig)
            bad = int(info.cpu()[0])
            if bad != 0:
                raise G.CholeskyError("natgrad_q: leading minor %d of Lambda^-1 is not positive definite (step %d)" % (bad, it))
            H.sgp_predict(Xd, z, ell, W, m.to(sess.torch_dtype), S.to(sess.torch_dtype), s_kind=H.SGP_S_TRIL, mode=mode,
                          out=(mean, var), wfrag=frag if fused else None)
            _, _, lsum = H.lik_sites(likelihood.lik_id, Yd, mean, var, param=likelihood.param, mscale=np.sqrt(k_var),
                                     vscale=k_var, out=(lam, beta))
            Phi, b, _ = H.sgp_wstats(Xd, lam, beta, z, ell, W, wfrag=frag)
            Lt, et = Phi * k_var + eye, b * np.sqrt(k_var)
            kl = 0.5 * (float(torch.diagonal(Sig).sum().cpu()) + float((m * m).sum().cpu()) - M
                        + 2.0 * float(np.log(np.diagonal(L.cpu().numpy())).sum()))
            elbo.append(float(lsum.cpu()[0]) - kl)
            resid.append(float(((Lam - Lt).abs().max() / Lt.abs().max()).cpu()))
            if it == steps or (it > 0 and abs(elbo[-1] - elbo[-2]) <= tol * abs(elbo[-1])):
                break
            Lam, eta = (1.0 - rho) * Lam + rho * Lt, (1.0 - rho) * eta + rho * et
        return (m.cpu().numpy(), np.tril(S.cpu().numpy()),
                dict(elbo=np.asarray(elbo), residual=np.asarray(resid), steps=it))

    def collapsed_bound_and_grad(self, X, Y, noise_var, k_var=1.0, residual="diagonal"):
        """(value, grad): the collapsed bound of collapsed_bound() and its exact gradient with respect to the CONSTRAINED
        values, grad = dict(z=[M, d], lengthscales=[dl], noise_var=float, k_var=float), float64 numpy.  One pass over
        the data for the statistics, the M^3 tail, one more pass for the part of the gradient that goes through
        K(z, X) (hb_sgp_kgrad) and the Gram VJP of K(z, z) + jitter I.

        Everything is FLOAT64 ARITHMETIC on the device whatever the session's dtype: the z gradient is the difference of
        two terms about 1000 times its size whose weights carry Lm^-1 twice, and float32 anywhere in the chain --
        reusing the float32-formed Phi, b of statistics() included -- returns noise ("Gradient of the
        collapsed bound").  A float32 session's X, Y, z, lengthscales are read as they are stored and are exact in
        double.  `value` is the bound of this same float64 evaluation, so value and gradient are consistent; in a
        float32 session it can differ from collapsed_bound() by the float32 error of statistics().  Same restrictions
        and exception types as statistics(): UnitRBF, one expert, the lengthscales one Variable; residual 'fullrank'
        raises NotImplementedError; a K(z, z) + jitter I or Lambda that is not positive definite raises
        graph.CholeskyError."""
        self._check_residual(residual)
        if not (float(noise_var) > 0.0 and float(k_var) > 0.0):
            raise ValueError("noise_var and k_var must be positive (got %r, %r)" % (noise_var, k_var))
        sess, Xd, Yd, z, ell, W = self._grad_inputs(X, Y)
        stats = self._statistics_f64(sess, Xd, Yd, z, ell, W)
        return self._grad_from_statistics(sess, Xd, Yd, z, ell, W, stats, noise_var, k_var, residual)

    def _grad_inputs(self, X, Y, who="collapsed_bound_and_grad"):
        """(sess, Xd, Yd, z, ell, W): the data as the session stores it, z and the lengthscales as the session stores
        them carried in double, and W = chol(K(z, z) + jitter I)^-1 in double."""
        sess, zvar, ls = self._stats_session()
        torch, H = sess.torch, sess.H
        Xd, Yd = self._device_data(sess, X, "X"), self._device_data(sess, Y, "Y")
        up = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=sess.np_dtype).astype(np.float64))).to(sess.device)
        z, ell = up(sess.read_value(zvar)), up(np.reshape(sess.read_value(ls), [-1]))
        if Xd.shape[0] != Yd.shape[0] or Xd.shape[1] != z.shape[1]:
            raise ValueError("%s: X %s, Y %s do not match z %s" % (who, tuple(Xd.shape), tuple(Yd.shape), tuple(z.shape)))
        L, info = H.cholesky(H.gram_fwd(z, z, ell, diag_add=float(settings.numerics.jitter_level)))
        bad = int(info.cpu()[0])
        if bad != 0:
            raise G.CholeskyError("%s: leading minor %d of K(z, z) + jitter I is not positive definite" % (who, bad))
        return sess, Xd, Yd, z, ell, H.trinv(L)

    def _statistics_f64(self, sess, Xd, Yd, z, ell, W):
        """(Phi [M, M], b [P, M], yy [P]) with float64 ARITHMETIC whatever the storage type of Xd, Yd: column chunks are
        up-converted, A_c = W K(z, X_c) by hb_sgp_A_f64, the three products by hb_matmul_f64, the chunks' results added in
        chunk order.  (statistics() forms A in the session's dtype: its float32 rounding of Phi, b is harmless for
        optimal_q and collapsed_bound and fatal for the gradient)"""
        torch, H = sess.torch, sess.H
        N, M = Xd.shape[0], z.shape[0]
        chunk = int(min(32768, max(32, (1 << 24) // M)))
        Phi = b = yy = None
        for c0 in range(0, N, chunk):
            Xc = Xd[c0:c0 + chunk].to(torch.float64).contiguous()
            Yc = Yd[c0:c0 + chunk].to(torch.float64).contiguous()
            A = H.sgp_A(Xc, z, ell, W)                                      # [M, nc]
            parts = (H.matmul(A, A, transB=True), H.matmul(Yc, A, transA=True, transB=True), H.matmul(Yc, Yc, transA=True))
            Phi, b, yy = parts if Phi is None else (Phi + parts[0], b + parts[1], yy + parts[2])
        return H.matutil(Phi.contiguous(), H.MATUTIL_SYM), b.contiguous(), torch.diagonal(yy).contiguous()

    def _grad_from_statistics(self, sess, Xd, Yd, z, ell, W, stats, noise_var, k_var, residual):
        """The tail and the two gradient passes of collapsed_bound_and_grad for given float64 (Phi, b, yy)."""
        torch, H = sess.torch, sess.H
        Phi, b, yy = stats
        s2, k = float(noise_var), float(k_var)
        rho = 1.0 if residual == "diagonal" else 0.0
        N, (M, d), P = int(Xd.shape[0]), z.shape, int(Yd.shape[1])
        # tail: D = dF/dLambda, G = dF/dPhi, g = dF/db
        _, LL, V, t, c = self._lambda_solve((Phi, b), s2, k)                  # t [P, M], |t_p|^2 = c_p^T Lambda^-1 c_p
        m = H.matmul(t, V)                                                   # [P, M] = c Lambda^-1
        D = (H.matmul(m, m, transA=True, alpha=-0.5) - (0.5 * P) * H.matmul(V, V, transA=True)).contiguous()
        Gm = H.matutil((D * (k / s2)).contiguous(), H.MATUTIL_ADD_EYE, alpha=rho * P * k / (2.0 * s2))
        g = (m * (np.sqrt(k) / s2)).contiguous()
        zg, eg = self._kernel_grads(sess, z, ell, W, Gm, g, Phi, b, lambda Q, R: H.sgp_kgrad(Xd, Yd, z, ell, Q, R))
        # scalars and the value, on the host
        tau, mb, mc = float((D * Phi).sum().cpu()), float((m * b).sum().cpu()), float((m * c).sum().cpu())
        a2sum, yys = float(torch.diagonal(Phi).sum().cpu()), float(yy.sum().cpu())
        quad = float((t * t).sum().cpu())
        logdet = 2.0 * float(np.log(np.diagonal(LL.cpu().numpy())).sum())
        val = -0.5 * N * P * np.log(2.0 * np.pi * s2) - yys / (2.0 * s2) + 0.5 * quad - 0.5 * P * logdet
        val -= rho * P * k * (N - a2sum) / (2.0 * s2)
        dk = tau / s2 + mb / (2.0 * np.sqrt(k) * s2) - rho * P * (N - a2sum) / (2.0 * s2)
        ds2 = (-N * P / (2.0 * s2) + yys / (2.0 * s2 ** 2) - (k / s2 ** 2) * tau - mc / s2
               + rho * P * k * (N - a2sum) / (2.0 * s2 ** 2))
        grad = dict(z=zg.cpu().numpy(), lengthscales=eg.cpu().numpy(), noise_var=float(ds2), k_var=float(dk))
        return float(val), grad

    def _kernel_grads(self, sess, z, ell, W, Gm, g, Phi, b, streamed):
        """(zbar [M, d], ellbar [dl]) of a bound whose dependence on A = W K(z, X) is Abar = 2 G A diag(w) + g^T r^T, given
        G = `Gm` [M, M], g [P, M] and the statistics Phi = A diag(w) A^T, b = (A r)^T (w = 1, r = Y for the collapsed
        bound).  `streamed(Q, R)` returns the part through K(z, X) for Q = 2 W^T G W, R = W^T g^T (hb_sgp_kgrad /
        hb_sgp_wkgrad); the part through K(z, z) is L^T Lbar = T = -Abar A^T = -(2 G Phi + g^T b), the Cholesky VJP and
        the symmetric Gram VJP."""
        torch, H = sess.torch, sess.H
        M, d = z.shape
        Q = H.matmul(W, H.matmul(Gm, W), transA=True, alpha=2.0)
        R = H.matmul(W, g, transA=True, transB=True)
        zbar, ellbar = streamed(Q, R)
        T = (H.matmul(Gm, Phi, alpha=-2.0) - H.matmul(g, b, transA=True)).contiguous()
        S = H.matmul(W, H.matmul(H.matutil(T, H.MATUTIL_PHI), W), transA=True)
        Kmmbar = H.matutil(S, H.MATUTIL_SYM)
        zk = torch.empty((M, d), dtype=torch.float64, device=sess.device)
        ek = torch.empty((ell.numel(),), dtype=torch.float64, device=sess.device)
        H.gram_bwd_raw(H.KERN_RBF | H.KERN_KBAR_SYMMETRIC, z, 0, z, 0, ell, 0, ell.numel(), Kmmbar, zk, zk, ek, 1, M, M, d,
                       H.workspace(torch.float64, sess.device, max(M * d, 1)))
        return zbar + zk, ellbar + ek

    def elbo_and_grad(self, X, Y, likelihood, q, k_var=1.0, residual="diagonal"):
        """(value, grad): the ELBO sum_j E_q log p(y_j | f_j) - KL(q || N(0, I)) of a factorising likelihood at a FIXED
        q(u) = N(m, S S^T), q = (m [1, M], S [M, M] lower), and its partial gradient with respect to the CONSTRAINED
        z, lengthscales and k_var at that q: grad = dict(z=[M, d], lengthscales=[dl], k_var=float), float64 numpy.  At
        the q natgrad_q converges to, the partial gradient is the total derivative of the fitted ELBO (envelope
        property); with the Gaussian likelihood and q = optimal_q it is the gradient of collapsed_bound_and_grad.

        With the sites lam_j = E[-d2 log p], gamma_j = E[d log p] of hb_lik_sites at the marginals mu_j, v_j:
        dl_j/dmu_j = gamma_j, dl_j/dv_j = -lam_j / 2 (Stein's identity: exact for the Gaussian and Poisson sites, for
        Bernoulli the derivative of the 20-node quadrature up to its error), so
            Abar = 2 G A diag(lam) + g^T gamma^T,   G = -(k_var / 2) (S S^T - rho I),   g = sqrt(k_var) m
        (rho = 1 for residual 'diagonal', 0 for 'neglected'; the |.| samples() applies to 1 - a_j^T a_j is ignored, as
        for collapsed_bound), which is the form of the collapsed bound's gradient with column weights: the streamed part
        is hb_sgp_wkgrad, the K(z, z) part needs Phi_w = A diag(lam) A^T and b_w = (A gamma)^T, and
        dF/dk_var = sum_j (gamma_j mu_j - lam_j v_j) / (2 k_var).

        FLOAT64 ARITHMETIC end to end whatever the session's dtype, for the reason collapsed_bound_and_grad gives.  The
        data is walked in fixed-size column chunks up-converted to double: the marginals (hb_sgp_predict_f64), the
        sites (hb_lik_sites_f64) and the weighted statistics (hb_sgp_wstats_f64), the chunks' sums added in chunk order;
        then the M^3 tail, hb_sgp_wkgrad over all of X in its stored dtype and the Gram VJP of K(z, z).  Restrictions
        and exception types are natgrad_q's: UnitRBF, one expert, Y [N, 1]; residual 'fullrank' and a mean-field q
        raise NotImplementedError; a K(z, z) + jitter I that is not positive definite raises graph.CholeskyError; a
        likelihood that is no henbun_amd.likelihoods.Likelihood raises TypeError."""
        from ..likelihoods import Likelihood

        self._check_residual(residual)
        if not isinstance(likelihood, Likelihood):
            raise TypeError("elbo_and_grad: likelihood must be a henbun_amd.likelihoods.Likelihood, got %s"
                            % type(likelihood).__name__)
        k = float(k_var)
        if not k > 0.0:
            raise ValueError("elbo_and_grad: k_var must be positive (got %r)" % (k_var,))
        m0, S0 = (np.asarray(a, dtype=np.float64) for a in q)
        if S0.ndim != 2:
            raise NotImplementedError("elbo_and_grad: q must be a full-rank q, (m [1, M], S [M, M]); a mean-field q is "
                                      "not covered")
        sess, Xd, Yd, z, ell, W = self._grad_inputs(X, Y, "elbo_and_grad")
        torch, H = sess.torch, sess.H
        if Yd.shape[1] != 1:
            raise NotImplementedError("elbo_and_grad: one latent function only (Y must be [N, 1], got %s)" % (tuple(Yd.shape),))
        N, M = int(Xd.shape[0]), int(z.shape[0])
        if m0.size != M or S0.shape != (M, M):
            raise ValueError("elbo_and_grad: q = (m [1, %d], S [%d, %d]) expected, got %s %s" % (M, M, M, m0.shape, S0.shape))
        rho = 1.0 if residual == "diagonal" else 0.0
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(sess.device)
        m, S = up(m0.reshape(1, M)), up(np.tril(S0))
        mode = H.SGP_DIAGONAL if residual == "diagonal" else H.SGP_NEGLECTED
        lam = torch.empty((N,), dtype=torch.float64, device=sess.device)
        gam = torch.empty_like(lam)
        chunk = int(min(32768, max(32, (1 << 24) // M))) & ~31            # a multiple of 32: every chunk of lam stays 16-byte aligned
        Phi = b = lsum = dks = None
        for c0 in range(0, N, chunk):
            Xc = Xd[c0:c0 + chunk].to(torch.float64).contiguous()
            yc = Yd[c0:c0 + chunk, 0].to(torch.float64).contiguous()
            mean, var = H.sgp_predict(Xc, z, ell, W, m, S, s_kind=H.SGP_S_TRIL, mode=mode)       # unit-variance moments [1, nc]
            lc, bc = lam[c0:c0 + chunk], gam[c0:c0 + chunk]
            _, _, ls = H.lik_sites(likelihood.lik_id, yc, mean, var, param=likelihood.param, mscale=np.sqrt(k), vscale=k,
                                   out=(lc, bc))
            mu = mean.reshape(-1) * np.sqrt(k)
            bc -= lc * mu                                                   # gamma = beta - lam mu
            Pc, rc, _ = H.sgp_wstats(Xc, lc, bc, z, ell, W)
            dc = (bc * mu - lc * var.reshape(-1) * k).sum()
            Phi, b, lsum, dks = (Pc, rc, ls, dc) if Phi is None else (Phi + Pc, b + rc, lsum + ls, dks + dc)
        # tail: G = dF/dPhi_w, g = dF/db_w
        Gm = H.matutil((H.matmul(S, S, transB=True) * (-0.5 * k)).contiguous(), H.MATUTIL_ADD_EYE, alpha=0.5 * rho * k)
        g = (m * np.sqrt(k)).contiguous()
        zg, eg = self._kernel_grads(sess, z, ell, W, Gm, g, Phi.contiguous(), b.contiguous(),
                                    lambda Q, R: H.sgp_wkgrad(Xd, lam, gam, z, ell, Q, R))
        # KL(q || N(0, I)) and dF/dk_var: scalars on the host
        Sl = np.tril(S0)
        kl = 0.5 * (float((Sl * Sl).sum()) + float((m0 * m0).sum()) - M) - float(np.log(np.abs(np.diagonal(Sl))).sum())
        grad = dict(z=zg.cpu().numpy(), lengthscales=eg.cpu().numpy(), k_var=float(dks.cpu()) / (2.0 * k))
        return float(lsum.cpu()[0]) - kl, grad

    # -- pathwise posterior function draws (Wilson et al. 2020) -----------------------------------------------------
    def pathwise_draws(self, q, num_samples, num_features=1024, k_var=1.0, seed=0, noise=None):
        """num_samples posterior FUNCTION draws as a PathwiseDraws: each is drawn once, as 2 num_features + M
        coefficients, and can then be evaluated anywhere at O((M + num_features) n) per draw -- no [n, n] covariance, no
        factorisation, no jitter; the same object gives values of the same sample paths on every call.  For the whitened
        model u ~ q = N(m, S S^T), with x~ = x / ell, W = Lm^-1, A(x) = W K(z, x) and L = num_features:
            omega_l ~ N(0, I_d),  w_s ~ N(0, I_2L),  eps_s ~ N(0, I_M)
            g_s(x) = L^-1/2 sum_l [ w_s,2l cos(omega_l . x~) + w_s,2l+1 sin(omega_l . x~) ]      (prior path, unit RBF)
            u_s = m + eps_s S^T,   t_s = u_s - g_s(z) W^T,   v_s = t_s W
            f_s(x) = sqrt(k_var) ( g_s(x) + v_s K(z, x) )  =  sqrt(k_var) ( g_s(x) + t_s A(x) ).
        Given omega the draws are Gaussian with mean sqrt(k_var) m A(x) -- predict_f's mean exactly -- and covariance
        k_var (C(x)^T C(x') + A^T S S^T A), C(x) = phi(x) - phi(z)^T W^T A(x), which tends to k_var (K(x, x') - A^T A +
        A^T S S^T A) as L grows: the EXACT conditional, i.e. the 'fullrank' residual of predict_f(full_cov=True) without
        its jitter term, whatever `residual` the model trains with.  The error of the covariance falls as 1 / sqrt(L)
        (at most 8 / sqrt(L) observed inside the hull of the inducing points at moderate conditioning; outside the hull
        the interpolation weights amplify the feature error, 13 / sqrt(L) was seen there).

        q: a Normal / Gaussian Variational (read through its parameters by a plan: the values predict_f reads), or a
        tuple (m [1, M], S [M, M] lower) or (m, s [M]) as numpy.  K(z, z) is factorised as the plans do it
        (_whitening(as_plans=True)), so the draws live in the whitening predict_f and the ELBO use.  The M-sized tail runs
        in float64 on the device whatever the session's dtype (forming t in float32 moves it by up to 9e-3 at
        cond 1e6): g(z) by hb_sgp_pathwise_f64, the two products by hb_matmul_f64; omega and the
        coefficients [w / sqrt(L) | v] are then stored in the session's dtype.  noise=None draws omega [L, d], w [S, 2L],
        eps [S, M] from hip_ops.Rng(seed), in that order; noise=dict(omega=, w=, eps=) injects them (float64 arrays).
        Restrictions and exception types are those of statistics(): UnitRBF, one expert, the lengthscales one Variable;
        more than one latent function raises NotImplementedError; malformed q or noise raise ValueError."""
        S, L, k_var = int(num_samples), int(num_features), float(k_var)
        if not (S >= 1 and L >= 1 and k_var > 0.0):
            raise ValueError("pathwise_draws: num_samples >= 1, num_features >= 1 and k_var > 0 expected (got %r, %r, %r)"
                             % (num_samples, num_features, k_var))
        sess, zvar, ls = self._stats_session()
        torch, H = sess.torch, sess.H
        M, d = int(zvar.shape[0]), int(zvar.shape[1])
        f64 = dict(dtype=torch.float64, device=sess.device)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(sess.device)
        m, s = self._q_moments(sess, q, M)
        z, ell, W, _ = self._whitening(sess, zvar, ls, None, None, "pathwise_draws", as_plans=True)
        if noise is None:
            rng = H.Rng(seed, device=sess.device)
            omega, w, eps = (rng.normal(shape, dtype=torch.float64) for shape in ((L, d), (S, 2 * L), (S, M)))
        else:
            want = dict(omega=(L, d), w=(S, 2 * L), eps=(S, M))
            if not isinstance(noise, dict) or set(noise) != set(want) or any(np.shape(noise[k]) != want[k] for k in want):
                raise ValueError("pathwise_draws: noise must be dict(omega=%s, w=%s, eps=%s), got %s"
                                 % (want["omega"], want["w"], want["eps"],
                                    {k: np.shape(v) for k, v in noise.items()} if isinstance(noise, dict) else type(noise).__name__))
            omega, w, eps = (up(noise[k]) for k in ("omega", "w", "eps"))
        # the frequencies and the prior weights ARE what the session's dtype stores: g(z) below is taken from their
        # rounded values, so the update interpolates the same prior path evaluate() adds it to
        omega = omega.to(sess.torch_dtype).contiguous()
        cw = (w * (1.0 / np.sqrt(L))).to(sess.torch_dtype).contiguous()
        z64, ell64, W64 = z.to(torch.float64), ell.to(torch.float64), W.to(torch.float64)
        U = m + (H.matmul(eps, s, transB=True) if s.dim() == 2 else eps * s)              # [S, M]
        Gz = H.sgp_pathwise(z64, omega.to(torch.float64), None, ell64, cw.to(torch.float64))   # g_s(z_m)  [S, M]
        T = (U - H.matmul(Gz, W64, transB=True)).contiguous()
        V = H.matmul(T, W64)
        coef = torch.cat([cw, V.to(sess.torch_dtype)], dim=1).contiguous()
        return PathwiseDraws(sess, self._device_data, omega, coef, z, ell, float(np.sqrt(k_var)))

    def _q_moments(self, sess, q, M):
        """(m [1, M], S [M, M] lower or s [M]) of q(u) as float64 device tensors, for pathwise_draws."""
        torch = sess.torch
        if isinstance(q, (tuple, list)):
            if len(q) != 2:
                raise ValueError("pathwise_draws: q = (m [1, M], S [M, M] or s [M]) expected")
            m, s = (np.asarray(a, dtype=np.float64) for a in q)
        else:
            mt, st, _ = _posterior_of(q)
            from ..variationals import Gaussian

            for v in ("q_mu", "q_sqrt") + (("scale",) if type(q) is Gaussian else ()):
                sess.read_value(object.__getattribute__(q, v))      # uploads a value that was assigned and not yet written
            plan = sess.make_plan([mt, st])
            plan.run()
            plan.check()
            m, s = (np.asarray(plan.value(t), dtype=np.float64) for t in (mt, st))
        if m.ndim >= 2 and int(np.prod(m.shape[:-1])) > 1:
            raise NotImplementedError("pathwise_draws: one latent function only (q has shape %s)" % (m.shape,))
        if s.ndim >= 2 and s.shape[-2:] == (M, M):
            s = np.tril(s.reshape(M, M))
        elif s.size == M:
            s = s.reshape(M)
        else:
            raise ValueError("pathwise_draws: S [%d, %d] lower or s [%d] expected, got %s" % (M, M, M, s.shape))
        if m.size != M:
            raise ValueError("pathwise_draws: m [1, %d] expected, got %s" % (M, m.shape))
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(sess.device)
        return up(m.reshape(1, M)), up(s)

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


class PathwiseDraws:
    """S posterior function draws of a SparseGP (SparseGP.pathwise_draws): a snapshot of the frequencies omega [L, d], the
    coefficient rows coef [S, 2L + M], z [M, d], the lengthscales and scale = sqrt(k_var), on the device in the session's
    dtype.  Later changes to the model do not move it.  Every evaluation is ONE launch of hb_sgp_pathwise, linear in n;
    the value at a point does not depend on the other points of the call, so the same draws can be evaluated in pieces,
    on a grid now and at candidates later, and maximised."""

    def __init__(self, sess, device_data, omega, coef, z, ell, scale):
        self._sess, self._device_data = sess, device_data
        self._omega, self._coef, self._z, self._ell, self.scale = omega, coef, z, ell, float(scale)
        self.num_samples, self.num_features = int(coef.shape[0]), int(omega.shape[0])

    def evaluate(self, X, out=None):
        """The draws at the rows of X as a device tensor [S, n] of the session's dtype (`out`: written in place).  X: a
        Data / MinibatchData of the model (read in full from its device buffer), a device tensor or an array [n, d]."""
        Xd = self._device_data(self._sess, X, "X")
        if Xd.shape[1] != self._z.shape[1]:
            raise ValueError("PathwiseDraws: X %s does not match z %s" % (tuple(Xd.shape), tuple(self._z.shape)))
        return self._sess.H.sgp_pathwise(Xd, self._omega, self._z, self._ell, self._coef, scale=self.scale, out=out)

    def __call__(self, X):
        """The draws at the rows of X as numpy [S, n]."""
        return self.evaluate(X).cpu().numpy()

    def _view(self, t):
        a = t.cpu().numpy()
        a.flags.writeable = False
        return a

    omega = property(lambda self: self._view(self._omega), doc="frequencies [L, d] (read-only numpy)")
    coef = property(lambda self: self._view(self._coef), doc="coefficient rows [S, 2L + M] = [w / sqrt(L) | v]")
    z = property(lambda self: self._view(self._z), doc="inducing points [M, d]")
    lengthscales = property(lambda self: self._view(self._ell), doc="lengthscales [1] or [d]")


def _device_data(sess, a, name):
    """X / Y as a contiguous [N, k] device tensor of the session's dtype: a Data / MinibatchData of the model is read
    from its device-resident buffer (all rows), a device tensor is taken as it is, anything else is uploaded."""
    from ..param import Data

    torch = sess.torch
    if isinstance(a, Data):
        t = sess.data_buffer(a)
    elif isinstance(a, torch.Tensor):
        t = a.to(device=sess.device, dtype=sess.torch_dtype)
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=sess.np_dtype))).to(sess.device)
    if t.dim() != 2:
        raise ValueError("%s must be 2-D [N, k], got %s" % (name, tuple(t.shape)))
    return t.contiguous()


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


def greedy_inducing(X, M, lengthscales=1.0, threshold=None, return_info=False, dtype=None):
    """Z [M, d] (numpy, selection order): the M rows of X [N, d] that greedy conditional-variance selection picks for the
    UnitRBF kernel with the given lengthscales (a scalar, [1] or [d]) -- a pivoted incomplete Cholesky of K(X, X) (Burt,
    Rasmussen, van der Wilk 2020), each step taking the point whose variance given the points chosen so far is largest
    (exact ties: the lowest row, so X[0] is always first).  Deterministic; needs no model, so it can make the Z a model
    is built with.  X is uploaded in the configured float type (`dtype`: as for Model) to the device a Session would
    pick; the work is M launches of hb_sgp_select with no read-back, and O(M N) device memory for the duration.
    threshold=None: settings.numerics.jitter_level -- a point whose conditional variance is below the jitter adds
    nothing that K(z, z) + jitter I can resolve.  If fewer than M points clear the threshold ValueError is raised, naming
    the count reached.  return_info=True: (Z, dict(idx int64 [M], pivots [M], trace float, count int)); trace is the
    residual tr(K_XX - K_XZ K_ZZ^-1 K_ZX), the N - a2sum term of collapsed_bound at zero jitter."""
    from ..session import Session

    sess = Session(None, dtype=dtype)
    sess._ensure_device()
    torch, H = sess.torch, sess.H
    X = np.asarray(X, dtype=sess.np_dtype)
    if X.ndim != 2:
        raise ValueError("greedy_inducing: X must be 2-D [N, d], got %s" % (X.shape,))
    ell = np.reshape(np.asarray(lengthscales, dtype=sess.np_dtype), [-1])
    if ell.size not in (1, X.shape[1]) or not np.all(ell > 0):
        raise ValueError("greedy_inducing: lengthscales must be positive, a scalar or one per column of X")
    M = int(M)
    if not 1 <= M <= X.shape[0]:
        raise ValueError("greedy_inducing: 1 <= M <= N expected, got M=%d, N=%d" % (M, X.shape[0]))
    thr = float(settings.numerics.jitter_level if threshold is None else threshold)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(sess.device)
    idx, pivots, count, trace = H.sgp_select(up(X), up(ell), M, thr)
    count = int(count.cpu()[0])
    if count < M:
        raise ValueError("greedy_inducing: only %d of the %d points asked for have a conditional variance above the "
                         "threshold %g (use fewer inducing points or a lower threshold)" % (count, M, thr))
    idx = idx.cpu().numpy()
    Z = X[idx].copy()
    if not return_info:
        return Z
    return Z, dict(idx=idx, pivots=pivots.cpu().numpy(), trace=float(trace.cpu()[0]), count=count)
