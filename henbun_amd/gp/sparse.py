"""The direct (eager, non-graph) inference routes of SparseGP: closed-form q(u) and collapsed bound (Titsias 2009), their
float64 gradients, the natural-gradient fit for non-Gaussian likelihoods, greedy inducing-point selection and pathwise
function draws.  None of it is in the reference.  gp.py traces graphs; this module and exact.py call hip_ops on device
tensors as they go, and _host.py holds the host steps both share.  `SparseInference` is mixed into gp.SparseGP, which
owns every public method below.
"""
import numpy as np

from .. import graph as G
from .._settings import settings
from ..likelihoods import Likelihood
from ..param import Data
from ..variationals import Gaussian
from . import _host


def _check_residual(residual):
    if residual == "fullrank":
        raise NotImplementedError("the closed-form posterior is implemented for residual 'diagonal' and 'neglected' "
                                  "(the 'fullrank' residual couples the data points)")
    if residual not in ("diagonal", "neglected"):
        raise ValueError("residual must be 'diagonal' or 'neglected', got %r" % (residual,))


def _check_lik_inputs(who, name, likelihood, k_var, residual, q, Y, M=None):
    """The argument checks natgrad_q, elbo_and_grad and elbo_and_grad_multi share, all decided on the host before the
    session is touched: residual, a henbun_amd.likelihoods.Likelihood (TypeError), k_var > 0, the targets by the
    likelihood's own rule (Likelihood.check_targets: Y [N, 1]; a numpy Y also by value) and q (`name`: what the route calls
    it) as the blocks of C = likelihood.num_latent latent functions, (m [C, M], S [C, M, M]) -- for C = 1 the public form
    (m [1, M], S [M, M]) is lifted to its one block.  M: the number of inducing points, where it is known.  Returns (m, S)
    as float64 numpy, or None for q = None."""
    _check_residual(residual)
    if not isinstance(likelihood, Likelihood):
        raise TypeError("%s: likelihood must be a henbun_amd.likelihoods.Likelihood, got %s" % (who, type(likelihood).__name__))
    if not float(k_var) > 0.0:
        raise ValueError("%s: k_var must be positive (got %r)" % (who, k_var))
    if isinstance(Y, np.ndarray):
        likelihood.check_targets(who, Y)
    if q is None:
        return None
    C = int(likelihood.num_latent)
    form = "%s = (m [%d, %%s], S [%s%%s, %%s])" % (name, C, "%d, " % C if C > 1 else "")
    m0, S0 = (np.asarray(a, dtype=np.float64) for a in q)
    got = "got %s %s" % (m0.shape, S0.shape)
    if C == 1 and S0.ndim < 3:
        m0, S0 = m0.reshape(1, -1), S0[None]
    if S0.ndim == 2 and S0.shape == m0.shape:
        raise NotImplementedError("%s: %s must be full-rank; a mean-field q is not covered" % (who, form % ("M", "M", "M")))
    if m0.ndim != 2 or m0.shape[0] != C or S0.shape != (C, m0.shape[1], m0.shape[1]):
        raise ValueError("%s: %s expected, %s" % (who, form % ("M", "M", "M"), got))
    if M is not None and m0.shape[1] != M:
        raise ValueError("%s: %s expected, %s" % (who, form % (M, M, M), got))
    return m0, S0


def _q_tail(H, Lam, c, who, of="Lambda"):
    """(L, V, t), the float64 tail every route shares: Lambda = L L^T (one read-back), V = L^-1, t = c V^T [P, M]; the
    mean is m = t V.  (m and Sigma are separate steps: a route that needs neither launches neither.)"""
    L = _host.factor(H, Lam.contiguous(), who, of)
    V = H.trinv(L)
    return L, V, H.matmul(c.contiguous(), V, transB=True)


def _q_cov(H, V, who):
    """(Sigma, S) on top of _q_tail: Sigma = Lambda^-1 = V^T V and its lower factor S (one more read-back)."""
    Sig = H.matmul(V, V, transA=True)
    return Sig, _host.factor(H, Sig, who, "Lambda^-1")


def _marginals(H, likelihood, X, z, ell, W, m, S, mode, out, wfrag=None):
    """The unit-variance marginals of the C latent functions at X under the blocks m [C, M], S [C, M, M], into out =
    (mean, var) [C, n]: ONE hb_sgp_predict_multi (A = W K(z, X) formed once for all C) where the likelihood asks for it
    (Likelihood.fused_marginals), else C calls of hb_sgp_predict -- the same bits (hip_ops.sgp_predict_multi)."""
    if likelihood.fused_marginals:
        H.sgp_predict_multi(X, z, ell, W, m, S, mode=mode, out=out, wfrag=wfrag)
    else:
        for c in range(m.shape[0]):
            H.sgp_predict(X, z, ell, W, m[c:c + 1], S[c], s_kind=H.SGP_S_TRIL, mode=mode,
                          out=(out[0][c:c + 1], out[1][c:c + 1]), wfrag=wfrag)


def _weighted_stats(H, X, w, r, z, ell, W, wfrag=None):
    """(Phi [C, M, M], b [C, M]) float64 of the weight sets w, r [C, n]: Phi_c = A diag(w_c) A^T, b_c = (A r_c)^T.  One set
    is hb_sgp_wstats, several are ONE hb_sgp_mwstats (A formed once per chunk for all of them).  Set by set the two return
    the same bits (hip_ops.sgp_mwstats), but hb_sgp_mwstats has not been timed at C = 1, so one set keeps its own entry."""
    if w.shape[0] == 1:
        Phi, b, _ = H.sgp_wstats(X, w, r, z, ell, W, wfrag=wfrag)
        return Phi[None], b
    return H.sgp_mwstats(X, w, r, z, ell, W, wfrag=wfrag)[:2]


def _input_variance(sess, X_var, Xd, who):
    """The input variances as a contiguous [n, d] device tensor of the session's dtype, for points Xd [n, d]: X_var
    [n, d], [d] or a scalar (broadcast).  Another shape, a negative or a non-finite entry raises ValueError -- the
    entries are checked by ONE device reduction, before the broadcast."""
    torch = sess.torch
    if isinstance(X_var, torch.Tensor):
        v = X_var.to(device=sess.device, dtype=sess.torch_dtype)
    else:
        v = _host.upload(sess, np.asarray(X_var, dtype=np.float64))
        if np.ndim(X_var) == 0:
            v = v.reshape(())                                  # (upload hands a scalar back as [1]: a [d] only for d = 1)
    n, d = Xd.shape
    if tuple(v.shape) not in ((), (d,), (n, d)):
        raise ValueError("%s: X_var must be [%d, %d], [%d] or a scalar, got %s" % (who, n, d, d, tuple(v.shape)))
    if not bool(((v >= 0) & torch.isfinite(v)).all().cpu()):
        raise ValueError("%s: X_var must be finite and >= 0" % who)
    return v.expand(n, d).contiguous()


def _walk_f64(torch, Xd, Yd, M, align, per_chunk):
    """The float64 walk over the data: row chunks of Xd, Yd (f64_chunk_rows(M, align) rows) are up-converted to double
    and handed to per_chunk(c0, Xc, Yc), whose tuples are added entry by entry in chunk order."""
    chunk = _host.f64_chunk_rows(M, align)
    total = None
    for c0 in range(0, Xd.shape[0], chunk):
        Xc = Xd[c0:c0 + chunk].to(torch.float64).contiguous()
        Yc = Yd[c0:c0 + chunk].to(torch.float64).contiguous()
        parts = per_chunk(c0, Xc, Yc)
        total = parts if total is None else tuple(a + b for a, b in zip(total, parts))
    return total


class SparseInference:
    """The eager methods of gp.SparseGP, a mixin: it reads the `kern` and `z` a SparseGP holds."""

    # -- closed-form posterior (Titsias 2009; the whitened model of models.SVGP) ------------------------------------
    def _stats_session(self, who):
        zvar = object.__getattribute__(self, "z")
        if len(zvar.shape) != 2:
            raise NotImplementedError("%s: one expert only (z must be [M, d], got %s)" % (who, tuple(zvar.shape)))
        sess, _, ls = _host.rbf_model_inputs(self, who)
        return sess, zvar, ls

    def statistics(self, X, Y):
        """(Phi [M, M], b [P, M], yy [P], a2sum [1]) of the whole data set X [N, d], Y [N, P] for the current z,
        lengthscales and settings.numerics.jitter_level, as float64 device tensors (hb_sgp_stats: one streaming pass):
        Phi = A A^T, b = (A Y)^T, yy_p = sum_j Y_jp^2, a2sum = tr Phi, A = Lm^-1 K(z, X), Lm = chol(K(z, z) + jitter I)
        from the fused factor + inverse the plans use.  A failed factorisation raises graph.CholeskyError."""
        sess, zvar, ls = self._stats_session("statistics")
        Xd, Yd = _host.device_data(sess, X, "X"), _host.device_data(sess, Y, "Y")
        z, ell, W, frag = self._whitening(sess, zvar, ls, Xd, Yd, "statistics")
        return sess.H.sgp_stats(Xd, Yd, z, ell, W, wfrag=frag)

    def psi_statistics(self, X_mean, X_var, Y):
        """statistics() for UNCERTAIN inputs x_n ~ N(X_mean_n, diag(X_var_n)): (Phi [M, M], b [P, M], yy [P], a2sum [1])
        as float64 device tensors, with the kernel expectations (psi statistics, Titsias & Lawrence 2010) in the place
        of the kernel values,
            Psi2 = sum_n E k(z, x_n) k(x_n, z),   C_p = sum_n E k(z, x_n) Y_np        (hb_sgp_psi_stats)
            Phi = W Psi2 W^T,   b_p = W C_p,   a2sum = tr Phi,   W = chol(K(z, z) + jitter I)^-1,
        so that optimal_q(.., stats=) returns the optimal q(u) and collapsed_bound(.., stats=) with residual 'diagonal'
        the collapsed bound under input uncertainty: its trace term N - a2sum is psi0 - tr(Kmm^-1 Psi2).  (The
        KL(q(X) || p(X)) of a latent-variable model is not part of it.)  X_var: [N, d], [d] or a scalar, the last two
        shared by all points; X_var = 0 gives statistics(X_mean, Y).  A negative or non-finite entry raises ValueError.
        The psi statistics are evaluated in DOUBLE whatever the session's dtype -- the sandwich amplifies an error of
        Psi2 by |W|^2 ~ 1 / jitter -- from the inputs as the session stores them; W is _whitening's, up-converted, and
        the sandwich is hb_matmul_f64.  Phi is bitwise symmetric.  Cost: N M (M + 1) / 2 double exponentials (Psi2 is no
        rank update once the variances differ from point to point), against the MFMA rank update of statistics().
        Restrictions and exception types are those of statistics()."""
        sess, zvar, ls = self._stats_session("psi_statistics")
        torch, H = sess.torch, sess.H
        Xd, Yd = _host.device_data(sess, X_mean, "X_mean"), _host.device_data(sess, Y, "Y")
        Vd = _input_variance(sess, X_var, Xd, "psi_statistics")
        z, ell, W, _ = self._whitening(sess, zvar, ls, Xd, Yd, "psi_statistics")
        Psi2, C, yy = H.sgp_psi_stats(Xd, Vd, Yd, z, ell)
        W64 = W.to(torch.float64)
        Phi = H.matutil(H.matmul(W64, H.matmul(Psi2, W64, transB=True)), H.MATUTIL_SYM)
        return Phi, H.matmul(C, W64, transB=True), yy, torch.diagonal(Phi).sum().reshape(1)

    def _whitening(self, sess, zvar, ls, Xd, Yd, who, as_plans=False):
        """(z, ell, W, frag) on the device in the session's dtype: W = chol(K(z, z) + jitter I)^-1 from the fused factor
        + inverse the plans use, frag its fragment-major images (float32, M % 32 == 0; else None).
        z and the lengthscales are their transforms of the raw parameters taken on the host in double and rounded;
        as_plans=True takes them from a plan instead, i.e. as the session's dtype transforms them on the device -- the
        values predict_f and the ELBO see.  In a float32 session the two can differ in the last bit of a lengthscale,
        which moves W by cond(K(z, z)) times that; a q(u) that a plan reads must be fitted in the plan's whitening
        ("Natural-gradient fit")."""
        torch, H = sess.torch, sess.H
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
            z, ell = _host.upload(sess, sess.read_value(zvar)), _host.lengthscales(sess, ls)
        if Xd is not None and (Xd.shape[0] != Yd.shape[0] or Xd.shape[1] != z.shape[1]):   # (pathwise_draws has no data)
            raise ValueError("%s: X %s, Y %s do not match z %s" % (who, tuple(Xd.shape), tuple(Yd.shape), tuple(z.shape)))
        M = z.shape[0]
        K = H.gram_fwd(z, z, ell, diag_add=float(settings.numerics.jitter_level))
        frag = None
        if sess.torch_dtype == torch.float32 and M % 32 == 0:
            frag = torch.empty(2 * M * M, dtype=sess.torch_dtype, device=sess.device)
        _, W, info = H.cholesky_inverse(K, frag=frag)
        _host.check_info(info, who, "K(z, z) + jitter I")
        return z, ell, W, frag

    def select_inducing(self, X, threshold=None):
        """Move z to the M = z.shape[0] rows of X [N, d] that greedy conditional-variance selection picks at the CURRENT
        lengthscales (hb_sgp_select; see greedy_inducing), in selection order, and return their row indices as numpy
        int64 [M].  X: a Data / MinibatchData of the model (read in full from its device buffer), a device tensor or an
        array.  threshold=None: settings.numerics.jitter_level.  Same restrictions and exception types as statistics():
        UnitRBF, one expert, the lengthscales one Variable.  If fewer than M points have a conditional variance above
        the threshold, ValueError is raised and z is left untouched.  q(u) is not touched: the optimum for the new z is
        one optimal_q / fit_q away."""
        sess, zvar, ls = self._stats_session("select_inducing")
        Xd = _host.device_data(sess, X, "X")
        M, d = int(zvar.shape[0]), int(zvar.shape[1])
        if Xd.shape[1] != d:
            raise ValueError("select_inducing: X %s does not match z %s" % (tuple(Xd.shape), tuple(zvar.shape)))
        if M > Xd.shape[0]:
            raise ValueError("select_inducing: z holds %d points, X only %d rows" % (M, Xd.shape[0]))
        thr = float(settings.numerics.jitter_level if threshold is None else threshold)
        idx, _, count, _ = sess.H.sgp_select(Xd, _host.lengthscales(sess, ls), M, thr)
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
        H = self.highest_parent._session.H
        Phi, b = stats[0], stats[1]
        noise_var, k_var = float(noise_var), float(k_var)
        if not (noise_var > 0.0 and k_var > 0.0):
            raise ValueError("noise_var and k_var must be positive (got %r, %r)" % (noise_var, k_var))
        Lam = H.matutil((Phi * (k_var / noise_var)).contiguous(), H.MATUTIL_ADD_EYE, alpha=1.0)
        c = (b * (np.sqrt(k_var) / noise_var)).contiguous()
        return (Lam,) + _q_tail(H, Lam, c, "optimal_q", "Lambda = I + (k_var / noise_var) Phi") + (c,)

    def optimal_q(self, X, Y, noise_var, k_var=1.0, q_shape="fullrank", residual="diagonal", stats=None):
        """The optimum of the ELBO over q(u_p) = N(m_p, S S^T) at fixed hyper-parameters, for the whitened model
        u_p ~ N(0, I), f_p = sqrt(k_var) (u_p A + residual), Y_p ~ N(f_p, noise_var):
            Lambda = I + (k_var / noise_var) Phi,  c_p = sqrt(k_var) b_p / noise_var,  m_p = Lambda^-1 c_p,
        q_shape 'fullrank': S = chol(Lambda^-1), lower-triangular [M, M] with a positive diagonal, the same for every p;
        'diagonal': s = diag(Lambda)^-1/2 [M], the optimum of the mean-field family (the mean is the same).
        Returns (m [P, M], S or s) as float64 numpy.  `residual` ('diagonal' / 'neglected') does not change q*: that
        term of the ELBO does not depend on q.  The M^3 tail runs on the device in float64 (hb_cholesky, hb_trinv,
        hb_matmul).  `stats`: the tuple statistics(X, Y) returned, to share one pass between calls -- or the tuple of
        psi_statistics(X_mean, X_var, Y), for the optimum under uncertain inputs (X is then not read)."""
        _check_residual(residual)
        if q_shape not in ("fullrank", "diagonal"):
            raise ValueError("q_shape must be 'fullrank' or 'diagonal', got %r" % (q_shape,))
        if stats is None:
            stats = self.statistics(X, Y)
        H = self.highest_parent._session.H
        Lam, _, V, t, _ = self._lambda_solve(stats, noise_var, k_var)
        m = H.matmul(t, V).cpu().numpy()
        if q_shape == "diagonal":
            return m, 1.0 / np.sqrt(np.diagonal(Lam.cpu().numpy()).copy())
        return m, np.tril(_q_cov(H, V, "optimal_q")[1].cpu().numpy())

    def collapsed_bound(self, X, Y, noise_var, k_var=1.0, residual="diagonal", stats=None):
        """The ELBO at the optimal q(u) of optimal_q (the collapsed bound), a float:
            sum_p [ -N/2 log(2 pi noise_var) - yy_p / (2 noise_var) + 1/2 c_p^T Lambda^-1 c_p ] - P/2 log|Lambda|
            - P k_var (N - a2sum) / (2 noise_var)          ('diagonal'; 'neglected' drops the last term).
        N - a2sum is sum_j (kdiag_j - sum_m A_mj^2) for the unit-variance kernel.  samples() takes the absolute value of
        that difference per point, so the two agree except where round-off makes a term negative.  `stats` may come
        from psi_statistics(X_mean, X_var, Y): the bound under uncertain inputs (only the row count of X is read)."""
        _check_residual(residual)
        if stats is None:
            stats = self.statistics(X, Y)
        _, L, _, t, _ = self._lambda_solve(stats, noise_var, k_var)
        yy, a2sum = stats[2].cpu().numpy(), float(stats[3].cpu()[0])
        # N from X's shape, not through device_data: that would upload a host array only to count its rows
        N = int(self.highest_parent._session.data_buffer(X).shape[0] if isinstance(X, Data) else np.shape(X)[0])
        quad = (t.cpu().numpy() ** 2).sum(-1)                                  # [P]
        logdet = 2.0 * float(np.log(np.diagonal(L.cpu().numpy())).sum())
        return _host.collapsed_value(N, yy.shape[0], noise_var, k_var, yy, quad, logdet, a2sum, residual)

    def _inducing_count(self):
        """M of a z [M, d], read without touching the session (None for another shape: _stats_session refuses it)."""
        zshape = tuple(object.__getattribute__(self, "z").shape)
        return zshape[0] if len(zshape) == 2 else None

    def natgrad_q(self, X, Y, likelihood, k_var=1.0, residual="diagonal", q0=None, steps=20, rho=1.0, tol=1e-8):
        """Natural-gradient fit of q(u) for a factorising likelihood (henbun_amd.likelihoods) over C = likelihood.num_latent
        latent functions at fixed hyper-parameters, for the whitened model u_c ~ N(0, I_M) independent, f_c = sqrt(k_var)
        (u_c A + residual), y_j ~ p(y_j | f_j1 .. f_jC), with C independent q(u_c) = N(m_c, S_c S_c^T) that share z, the
        lengthscales and W.  C = 1: Gaussian, Bernoulli, Poisson, Laplace, Gamma, Exponential, NegativeBinomial, Binomial --
        all log-concave in f, so lam_j >= 0 and Lambda stays positive definite; C > 1: Softmax (C classes),
        HeteroscedasticGaussian (C = 2).  q_c is kept as Lambda_c = (S_c S_c^T)^-1, eta_c = Lambda_c m_c; one step is the
        conjugate update with per-point pseudo-observations (conjugate-computation VI, Khan & Lin 2017):
            mu_jc, v_jc              the marginals of f_jc under q_c: C calls of hb_sgp_predict, or ONE hb_sgp_predict_multi
                                     (A formed once for all C) where the likelihood has fused_marginals
            lam_jc, beta_jc, l_j     E[-d2 log p], E[d log p] + lam mu, E[log p]: ONE sites launch, the likelihood's
                                     (Likelihood.sites: hb_lik_sites, hb_lik_softmax_sites over the likelihood's nodes
                                     [S, C], hb_lik_hetgauss_sites)
            Phi_c = A diag(lam_c) A^T,  b_c = A beta_c      one pass over X: hb_sgp_wstats (C = 1) or ONE hb_sgp_mwstats,
                                     A = W K(z, X) formed once per chunk for all C weight sets
            Lambda_c <- (1 - rho) Lambda_c + rho (I + k_var Phi_c),   eta_c <- (1 - rho) eta_c + rho sqrt(k_var) b_c
        and m_c = Lambda_c^-1 eta_c, S_c = chol(Lambda_c^-1) from C float64 tails of optimal_q.  With the Gaussian
        likelihood one step at rho = 1 is optimal_q.  K(z, z) is factorised once per call, from z and the lengthscales as
        the session's plans transform them on the device, so the q(u) returned lives in the whitening predict_f and the
        ELBO use.
        X, Y as for statistics(), Y [N, 1]: the targets, checked by the likelihood's own rule (Likelihood.check_targets: a
        numpy Y of Softmax must hold integers in 0 .. C-1, of HeteroscedasticGaussian finite numbers; targets already on
        the device are the caller's duty).  q0=None starts at the prior; q0 at a given full-rank q: (m [1, M], S [M, M])
        for one latent function, (m [C, M], S [C, M, M]) for C > 1.  Returns (m [1, M], S [M, M], info) resp. (m [C, M],
        S [C, M, M], info) as float64 numpy, S lower with a positive diagonal; info = dict(elbo, residual, steps): the ELBO
        sum_j l_j - sum_c KL(q_c || N(0, I)) and the fixed-point residual max|Lambda_c - (I + k_var Phi_c)| / max|I + k_var
        Phi_c| (the largest over c) at every iterate, the starting one included (steps + 1 entries), and the steps taken.
        m, S are the last iterate evaluated.  Stops when the relative change of the ELBO is <= tol, or after `steps`.
        Same restrictions and exception types as statistics(); residual 'fullrank' and a mean-field q0 raise
        NotImplementedError, other shapes and bad targets ValueError, all before the session is touched; a Lambda that is
        not positive definite raises graph.CholeskyError.  A full step (rho = 1) is not guaranteed to raise the ELBO from a
        q far from the optimum (info['elbo'] shows an overshoot): start at the prior or damp with rho < 1.
        Softmax: the ELBO is a fixed-node sum and lam is Price's form, not the derivative of that sum: from step to step
        the ELBO can wiggle by about 1e-4 near the fixed point.  A full step does not settle (it cycles or diverges, see
        likelihoods.Softmax); the likelihood's natgrad_rho (0.5) is what models.SVGPMulticlass passes.
        HeteroscedasticGaussian: its expectation is exact, so the ELBO has no node wiggle; natgrad_rho 0.5 as well."""
        who = "natgrad_q"
        q0 = _check_lik_inputs(who, "q0", likelihood, k_var, residual, q0, Y, self._inducing_count())
        k_var, rho, steps = float(k_var), float(rho), int(steps)
        if not (0.0 < rho <= 1.0 and steps >= 0):
            raise ValueError("%s: 0 < rho <= 1 and steps >= 0 expected (got %r, %r)" % (who, rho, steps))
        sess, zvar, ls = self._stats_session(who)
        torch, H = sess.torch, sess.H
        Xd, Yd = _host.device_data(sess, X, "X"), _host.device_data(sess, Y, "Y")
        likelihood.check_targets(who, Yd)
        C, M = int(likelihood.num_latent), int(zvar.shape[0])
        z, ell, W, frag = self._whitening(sess, zvar, ls, Xd, Yd, who, as_plans=True)
        N, d = Xd.shape
        dt = sess.torch_dtype
        f64 = dict(dtype=torch.float64, device=sess.device)
        eye = torch.eye(M, **f64)
        if q0 is None:
            Lam, eta = eye.repeat(C, 1, 1), torch.zeros((C, M), **f64)
        else:
            Lam, eta = torch.empty((C, M, M), **f64), torch.empty((C, M), **f64)
            for c in range(C):
                Sinv = H.trinv(_host.upload(sess, np.tril(q0[1][c]), np.float64))
                Lam[c] = H.matmul(Sinv, Sinv, transA=True)
                eta[c:c + 1] = H.matmul(_host.upload(sess, q0[0][c].reshape(1, M), np.float64), Lam[c].contiguous())
        state = likelihood.device_state(sess)
        yv = Yd.reshape(-1).contiguous()
        mode = H.SGP_DIAGONAL if residual == "diagonal" else H.SGP_NEGLECTED
        fused = bool(getattr(settings.runtime, "fused_predict", True)) and (
            H.sgp_predict_multi_fused(dt, N, M, d, C, frag is not None) if likelihood.fused_marginals else
            H.sgp_predict_fused(dt, 1, N, M, d, 1, H.SGP_S_TRIL, frag is not None))
        mean, var, lam, beta = (torch.empty((C, N), dtype=dt, device=sess.device) for _ in range(4))
        m, S = torch.empty((C, M), **f64), torch.empty((C, M, M), **f64)
        elbo, resid = [], []
        for it in range(steps + 1):
            kl = 0.0
            for c in range(C):
                whoc = "natgrad_q (step %d, latent function %d)" % (it, c)
                L, V, t = _q_tail(H, Lam[c], eta[c:c + 1], whoc)
                mc = H.matmul(t, V)
                Sig, Sc = _q_cov(H, V, whoc)
                m[c:c + 1], S[c] = mc, Sc
                # KL(q_c || N(0, I)) from Sigma and the factor of Lambda.  elbo_and_grad forms it from S instead: equal in
                # exact arithmetic, not in the last bits, so neither borrows the other's
                kl += 0.5 * (float(torch.diagonal(Sig).sum().cpu()) + float((mc * mc).sum().cpu()) - M
                             + 2.0 * float(np.log(np.diagonal(L.cpu().numpy())).sum()))
            _marginals(H, likelihood, Xd, z, ell, W, m.to(dt), S.to(dt), mode, (mean, var), frag if fused else None)
            lsum = likelihood.sites(H, state, yv, mean, var, np.sqrt(k_var), k_var, (lam, beta))
            Phi, b = _weighted_stats(H, Xd, lam, beta, z, ell, W, frag)
            Lt, et = Phi * k_var + eye, b * np.sqrt(k_var)
            elbo.append(float(lsum.cpu()[0]) - kl)
            resid.append(float(((Lam - Lt).abs().amax(dim=(1, 2)) / Lt.abs().amax(dim=(1, 2))).max().cpu()))
            if it == steps or (it > 0 and abs(elbo[-1] - elbo[-2]) <= tol * abs(elbo[-1])):
                break
            Lam, eta = (1.0 - rho) * Lam + rho * Lt, (1.0 - rho) * eta + rho * et
        m, S = m.cpu().numpy(), np.tril(S.cpu().numpy())
        return m, S[0] if C == 1 else S, dict(elbo=np.asarray(elbo), residual=np.asarray(resid), steps=it)

    def collapsed_bound_and_grad(self, X, Y, noise_var, k_var=1.0, residual="diagonal", x_grad=False):
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
        graph.CholeskyError.

        x_grad=True: grad also holds X [N, d], the gradient with respect to the INPUTS as the session stores them
        (float64 numpy; a float32 session's X is exact in double, so it is the exact gradient at the stored values).
        The bound depends on X through K(z, X) alone (k(x, x) = 1), so it is the column sums of the products whose row
        sums are the streamed part of the z gradient, from the same pass (hb_sgp_kgrad_x; DESIGN.md 3, "Input gradient
        and deep kernels").  The other entries and the value are the bits of x_grad=False."""
        val, grad, xbar = self._collapsed_bound_and_grad(X, Y, noise_var, k_var, residual, x_grad)
        if x_grad:
            grad["X"] = xbar.cpu().numpy()
        return val, grad

    def _collapsed_bound_and_grad(self, X, Y, noise_var, k_var, residual, x_grad):
        """(value, grad, xbar): collapsed_bound_and_grad with the input gradient left ON THE DEVICE (float64 [N, d]; None
        without x_grad) -- models.DeepKernelSVGP chains it through its network there."""
        _check_residual(residual)
        if not (float(noise_var) > 0.0 and float(k_var) > 0.0):
            raise ValueError("noise_var and k_var must be positive (got %r, %r)" % (noise_var, k_var))
        sess, Xd, Yd, z, ell, W = self._grad_inputs(X, Y)
        stats = self._statistics_f64(sess, Xd, Yd, z, ell, W)
        H = sess.H
        point = {"X": None}

        def streamed(Q, R):
            if not x_grad:
                return H.sgp_kgrad(Xd, Yd, z, ell, Q, R)
            zbar, ellbar, point["X"] = H.sgp_kgrad(Xd, Yd, z, ell, Q, R, x_grad=True)
            return zbar, ellbar

        val, grad = self._grad_from_statistics(sess, z, ell, W, stats, noise_var, k_var, residual, streamed,
                                               int(Xd.shape[0]), int(Yd.shape[1]))
        return val, grad, point["X"]

    def psi_bound_and_grad(self, X_mean, X_var, Y, noise_var, k_var=1.0, residual="diagonal"):
        """collapsed_bound_and_grad() for UNCERTAIN inputs x_n ~ N(X_mean_n, diag(X_var_n)): (value, grad) with the
        collapsed bound from the psi statistics (collapsed_bound(stats=psi_statistics(..)), evaluated in float64) and its
        exact gradient with respect to the CONSTRAINED values, grad = dict(X_mean=[N, d], X_var, z=[M, d],
        lengthscales=[dl], noise_var=float, k_var=float), float64 numpy.  X_var: [N, d], [d] or a scalar, as
        psi_statistics takes it; grad["X_var"] has the shape given (the shared forms: summed over the points).  The
        KL(q(X) || p(X)) of a latent-variable model is NOT part of it (models.BayesianGPLVM adds it on the host).

        FLOAT64 ARITHMETIC end to end whatever the session's dtype, as collapsed_bound_and_grad: X_mean, X_var and Y are
        up-converted (N (2 d + P) numbers), Psi2 and C come from hb_sgp_psi_stats_f64, the sandwich W Psi2 W^T from
        hb_matmul_f64; the tail, the weights Q = 2 W^T G W, R = W^T g^T and the Cholesky / Gram VJP of K(z, z) are those of
        collapsed_bound_and_grad, and the pass that turns (Q, R) into gradients is hb_sgp_psi_grad_f64: two passes of one
        double exponential per point and pair of inducing points ("Bayesian GP-LVM").  X_var = 0 gives the z,
        lengthscale and scalar gradients of collapsed_bound_and_grad(X_mean, Y, ..).  Restrictions and exception types are
        those of psi_statistics and collapsed_bound_and_grad."""
        _check_residual(residual)
        if not (float(noise_var) > 0.0 and float(k_var) > 0.0):
            raise ValueError("noise_var and k_var must be positive (got %r, %r)" % (noise_var, k_var))
        who = "psi_bound_and_grad"
        sess, Xd, Yd, z, ell, W = self._grad_inputs(X_mean, Y, who)
        torch, H = sess.torch, sess.H
        Vd = _input_variance(sess, X_var, Xd, who)
        var_shape = tuple(X_var.shape) if isinstance(X_var, torch.Tensor) else np.shape(X_var)
        mu, sv, Y64 = (t.to(torch.float64).contiguous() for t in (Xd, Vd, Yd))
        Psi2, C, yy = H.sgp_psi_stats(mu, sv, Y64, z, ell)
        Phi = H.matutil(H.matmul(W, H.matmul(Psi2, W, transB=True)), H.MATUTIL_SYM)
        b = H.matmul(C, W, transB=True)
        point = {}

        def streamed(Q, R):
            point["mu"], point["s"], zbar, ellbar = H.sgp_psi_grad(mu, sv, Y64, z, ell, Q, R)
            return zbar, ellbar

        val, grad = self._grad_from_statistics(sess, z, ell, W, (Phi, b, yy), noise_var, k_var, residual, streamed,
                                               int(Xd.shape[0]), int(Yd.shape[1]))
        sbar = point["s"]
        if len(var_shape) < 2:                                               # a shared variance: summed over the points
            sbar = sbar.sum(0) if len(var_shape) == 1 else sbar.sum()
        grad["X_mean"], grad["X_var"] = point["mu"].cpu().numpy(), sbar.cpu().numpy()
        return val, grad

    def _grad_inputs(self, X, Y, who="collapsed_bound_and_grad"):
        """(sess, Xd, Yd, z, ell, W): the data as the session stores it, z and the lengthscales as the session stores
        them carried in double, and W = chol(K(z, z) + jitter I)^-1 in double."""
        sess, zvar, ls = self._stats_session(who)
        H = sess.H
        Xd, Yd = _host.device_data(sess, X, "X"), _host.device_data(sess, Y, "Y")
        z = _host.upload(sess, sess.read_value(zvar), carry=np.float64)
        ell = _host.lengthscales(sess, ls, carry=np.float64)
        if Xd.shape[0] != Yd.shape[0] or Xd.shape[1] != z.shape[1]:
            raise ValueError("%s: X %s, Y %s do not match z %s" % (who, tuple(Xd.shape), tuple(Yd.shape), tuple(z.shape)))
        L = _host.factor(H, H.gram_fwd(z, z, ell, diag_add=float(settings.numerics.jitter_level)), who, "K(z, z) + jitter I")
        return sess, Xd, Yd, z, ell, H.trinv(L)

    def _statistics_f64(self, sess, Xd, Yd, z, ell, W):
        """(Phi [M, M], b [P, M], yy [P]) with float64 ARITHMETIC whatever the storage type of Xd, Yd: column chunks are
        up-converted, A_c = W K(z, X_c) by hb_sgp_A_f64, the three products by hb_matmul_f64, the chunks' results added in
        chunk order.  (statistics() forms A in the session's dtype: its float32 rounding of Phi, b is harmless for
        optimal_q and collapsed_bound and fatal for the gradient)"""
        torch, H = sess.torch, sess.H

        def per_chunk(c0, Xc, Yc):
            A = H.sgp_A(Xc, z, ell, W)                                      # [M, nc]
            return H.matmul(A, A, transB=True), H.matmul(Yc, A, transA=True, transB=True), H.matmul(Yc, Yc, transA=True)

        Phi, b, yy = _walk_f64(torch, Xd, Yd, z.shape[0], 1, per_chunk)
        return H.matutil(Phi.contiguous(), H.MATUTIL_SYM), b.contiguous(), torch.diagonal(yy).contiguous()

    def _grad_from_statistics(self, sess, z, ell, W, stats, noise_var, k_var, residual, streamed, N, P):
        """The tail and the two gradient passes of collapsed_bound_and_grad / psi_bound_and_grad for given float64
        (Phi, b, yy) of N points and P outputs; `streamed(Q, R)` returns the part of (zbar, ellbar) through K(z, X) or
        through the psi statistics (hb_sgp_kgrad / hb_sgp_psi_grad)."""
        torch, H = sess.torch, sess.H
        Phi, b, yy = stats
        s2, k = float(noise_var), float(k_var)
        rho = 1.0 if residual == "diagonal" else 0.0
        # tail: D = dF/dLambda, G = dF/dPhi, g = dF/db
        _, LL, V, t, c = self._lambda_solve((Phi, b), s2, k)                  # t [P, M], |t_p|^2 = c_p^T Lambda^-1 c_p
        m = H.matmul(t, V)                                                   # [P, M] = c Lambda^-1
        D = (H.matmul(m, m, transA=True, alpha=-0.5) - (0.5 * P) * H.matmul(V, V, transA=True)).contiguous()
        Gm = H.matutil((D * (k / s2)).contiguous(), H.MATUTIL_ADD_EYE, alpha=rho * P * k / (2.0 * s2))
        g = (m * (np.sqrt(k) / s2)).contiguous()
        zg, eg = self._kernel_grads(sess, z, ell, W, Gm, g, Phi, b, streamed)
        # scalars and the value, on the host
        tau, mb, mc = float((D * Phi).sum().cpu()), float((m * b).sum().cpu()), float((m * c).sum().cpu())
        a2sum, yys = float(torch.diagonal(Phi).sum().cpu()), float(yy.sum().cpu())
        quad = float((t * t).sum().cpu())
        logdet = 2.0 * float(np.log(np.diagonal(LL.cpu().numpy())).sum())
        val = _host.collapsed_value(N, P, s2, k, yys, quad, logdet, a2sum, residual)
        dk = tau / s2 + mb / (2.0 * np.sqrt(k) * s2) - rho * P * (N - a2sum) / (2.0 * s2)
        ds2 = (-N * P / (2.0 * s2) + yys / (2.0 * s2 ** 2) - (k / s2 ** 2) * tau - mc / s2
               + rho * P * k * (N - a2sum) / (2.0 * s2 ** 2))
        grad = dict(z=zg.cpu().numpy(), lengthscales=eg.cpu().numpy(), noise_var=float(ds2), k_var=float(dk))
        return val, grad

    def _kernel_grads(self, sess, z, ell, W, Gm, g, Phi, b, streamed):
        """(zbar [M, d], ellbar [dl]) of a bound whose dependence on A = W K(z, X) is Abar = 2 G A diag(w) + g^T r^T, given
        G = `Gm` [M, M], g [P, M] and the statistics Phi = A diag(w) A^T, b = (A r)^T (w = 1, r = Y for the collapsed
        bound).  `streamed(Q, R)` returns the part through K(z, X) for Q = 2 W^T G W, R = W^T g^T (hb_sgp_kgrad /
        hb_sgp_wkgrad); the part through K(z, z) is L^T Lbar = T = -Abar A^T = -(2 G Phi + g^T b), the Cholesky VJP and
        the symmetric Gram VJP."""
        H = sess.H
        Q = H.matmul(W, H.matmul(Gm, W), transA=True, alpha=2.0)
        R = H.matmul(W, g, transA=True, transB=True)
        zbar, ellbar = streamed(Q, R)
        T = (H.matmul(Gm, Phi, alpha=-2.0) - H.matmul(g, b, transA=True)).contiguous()
        zk, ek = self._kmm_grads(sess, z, ell, W, T)
        return zbar + zk, ellbar + ek

    def _kmm_grads(self, sess, z, ell, W, T):
        """(zk [M, d], ek [dl]): the part of a bound's gradient through K(z, z) given L^T Lbar = T = -Abar A^T [M, M] -- the
        Cholesky VJP and the symmetric Gram VJP of K(z, z) + jitter I."""
        torch, H = sess.torch, sess.H
        M, d = z.shape
        S = H.matmul(W, H.matmul(H.matutil(T, H.MATUTIL_PHI), W), transA=True)
        Kmmbar = H.matutil(S, H.MATUTIL_SYM)
        zk = torch.empty((M, d), dtype=torch.float64, device=sess.device)
        ek = torch.empty((ell.numel(),), dtype=torch.float64, device=sess.device)
        H.gram_bwd_raw(H.KERN_RBF | H.KERN_KBAR_SYMMETRIC, z, 0, z, 0, ell, 0, ell.numel(), Kmmbar, zk, zk, ek, 1, M, M, d,
                       H.workspace(torch.float64, sess.device, max(M * d, 1)))
        return zk, ek

    def elbo_and_grad(self, X, Y, likelihood, q, k_var=1.0, residual="diagonal", lik_grad=False, x_grad=False):
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
        likelihood that is no henbun_amd.likelihoods.Likelihood raises TypeError.

        lik_grad=True: grad also holds lik_param, the derivative with respect to the likelihood's own parameter
        (likelihood.param: the Gaussian variance, the Laplace scale, the Gamma shape, the negative binomial dispersion) --
        sum_j dl_j / dparam at the marginals of that q (hb_lik_param_grad_f64 on every chunk of the same walk, added in
        chunk order).  Like the other entries it is the partial derivative at fixed q, hence the total derivative at the
        fitted q.  A likelihood that is not `trainable` raises ValueError.  The other entries and the value are the bits
        of lik_grad=False.

        x_grad=True: grad also holds X [N, d], the partial gradient at that q with respect to the INPUTS as the session
        stores them, float64 numpy: the marginals depend on X through K(z, X) alone, so it is the column sums of the
        products of the hb_sgp_wkgrad pass, whose E carries lam_j and gamma_j (hb_sgp_wkgrad_x, one call over all of X).
        The other entries and the value are the bits of x_grad=False.

        A likelihood over several latent functions (likelihoods.Softmax) raises NotImplementedError: that route has its
        own weights, q and name, elbo_and_grad_multi (both run _elbo_and_grad)."""
        if getattr(likelihood, "num_latent", 1) > 1:
            raise NotImplementedError("elbo_and_grad: one latent function only (%s has %d: use elbo_and_grad_multi)"
                                      % (type(likelihood).__name__, likelihood.num_latent))
        return self._elbo_and_grad("elbo_and_grad", X, Y, likelihood, q, k_var, residual, lik_grad, x_grad=x_grad)

    def elbo_and_grad_multi(self, X, Y, likelihood, q, k_var=1.0, residual="diagonal", lik_grad=False):
        """(value, grad): elbo_and_grad for a likelihood over C = likelihood.num_latent latent functions
        (likelihoods.Softmax) at FIXED q(u_c) = N(m_c, S_c S_c^T), q = (m [C, M], S [C, M, M] lower), labels Y [N, 1]:
        value = sum_j l_j - sum_c KL(q_c || N(0, I)), l_j the mean of log softmax over the likelihood's fixed nodes -- the
        ELBO natgrad_q reports -- and grad = dict(z=[M, d], lengthscales=[dl], k_var=float), float64 numpy.

        What the number is: the EXACT partial gradient of that fixed-node value at fixed q.  The weights are the
        derivatives of the node sum itself (hb_lik_softmax_grad), r_jc = dl_j/dmu_jc = g_jc and w_jc = -2 dl_j/dv_jc =
        -mean_s(([c = y_j] - p_sc) eps_sc) / sqrt(v_jc), NOT Price's curvature lam = mean_s p (1 - p) of the
        natural-gradient step, which is the derivative of the exact expectation and misses that of the node sum by up to
        17 % in z at 128 nodes ("Multi-class classification").  w has either sign; that is harmless for a
        gradient (only the conjugate update needs lam >= 0).  Where v_jc = 0 the node sum has no derivative in v and
        w_jc is p (1 - p), the limit of the exact expectation's.  In m the fixed point of natgrad_q is stationary for this
        value; in S only up to the node error, because the step uses Price's lam: at the fitted q the partial gradient
        is the total derivative of the fitted ELBO up to that error.

        Per class the gradient has elbo_and_grad's form, Abar_c = 2 G_c A diag(w_c) + g_c^T r_c^T with G_c = -(k_var / 2)
        (S_c S_c^T - rho I), g_c = sqrt(k_var) m_c, and it is linear in the classes: the streamed part is C calls of
        hb_sgp_wkgrad over all of X with Q_c = 2 W^T G_c W, R_c = W^T g_c^T, added in class order (a one-pass kernel over
        all classes measured 1.6 x slower: at M = 512 one packed Q_c fills half an L2 and C of them do not fit, DESIGN.md
        3), the K(z, z) part runs once with T = -sum_c (2 G_c Phi_c + g_c^T b_c), and dF/dk_var = sum_jc (r_jc mu_jc -
        w_jc v_jc) / (2 k_var).
        FLOAT64 ARITHMETIC end to end on the chunk walk of elbo_and_grad: per chunk C calls of hb_sgp_predict_f64, ONE
        hb_lik_softmax_grad_f64 and ONE hb_sgp_mwstats_f64.  Refusals and exception types are natgrad_q's for such a
        likelihood ('fullrank' and a mean-field q: NotImplementedError; other shapes and bad labels: ValueError), decided
        before the session is touched; a likelihood over ONE latent function raises ValueError: use elbo_and_grad.

        The weights call is the likelihood's (Likelihood.weights).  likelihoods.HeteroscedasticGaussian: Y [N, 1]
        real, w = lam and r = dl/dmu from ONE hb_lik_hetgauss_sites_f64 per chunk (its expectation is exact, so lam IS
        -2 dl/dv) and the marginals from ONE hb_sgp_predict_multi_f64.  lik_grad=True (a `trainable` likelihood: ValueError
        otherwise) adds grad['lik_param'] = sum_j dl_j / dparam at the marginals of that q, added in chunk order -- for
        HeteroscedasticGaussian sum_j r_gj; the other entries and the value are the bits of lik_grad=False."""
        who = "elbo_and_grad_multi"
        if isinstance(likelihood, Likelihood) and likelihood.num_latent < 2:
            raise ValueError("%s: a likelihood over several latent functions expected (%s has one: use elbo_and_grad)"
                             % (who, type(likelihood).__name__))
        return self._elbo_and_grad(who, X, Y, likelihood, q, k_var, residual, lik_grad)

    def _elbo_and_grad(self, who, X, Y, likelihood, q, k_var, residual, lik_grad, x_grad=False):
        """The one route behind elbo_and_grad and elbo_and_grad_multi (which document it), on the blocks q = (m [C, M],
        S [C, M, M]) of C = likelihood.num_latent latent functions: the float64 chunk walk -- marginals (_marginals), the
        likelihood's weights w, r (Likelihood.weights), weighted statistics (_weighted_stats) -- then per latent function the
        tail G_c, g_c, Q_c, R_c with hb_sgp_wkgrad over all of X, ONE Cholesky and Gram VJP of K(z, z) for T = -sum_c (2 G_c
        Phi_c + g_c^T b_c), and the KL from S.  x_grad (one latent function only): the input gradient of that call too."""
        if lik_grad and not getattr(likelihood, "trainable", False):
            raise ValueError("%s: lik_grad=True needs a likelihood with a continuous parameter (got %s)"
                             % (who, type(likelihood).__name__))
        q = _check_lik_inputs(who, "q", likelihood, k_var, residual, q, Y, self._inducing_count())
        if q is None:
            raise ValueError("%s: q = (m, S) expected, got None" % who)
        m0, S0 = q[0], np.tril(q[1])
        sess, Xd, Yd, z, ell, W = self._grad_inputs(X, Y, who)
        likelihood.check_targets(who, Yd)
        torch, H = sess.torch, sess.H
        N, (C, M) = int(Xd.shape[0]), m0.shape
        k = float(k_var)
        rho = 1.0 if residual == "diagonal" else 0.0
        f64 = dict(dtype=torch.float64, device=sess.device)
        m, S = _host.upload(sess, m0, np.float64), _host.upload(sess, S0, np.float64)
        state = likelihood.device_state(sess)
        mode = H.SGP_DIAGONAL if residual == "diagonal" else H.SGP_NEGLECTED
        ldN = -(-N // 2) * 2                         # rows padded to 16 bytes: what hb_sgp_mwstats asks of the weights
        w, r = (torch.zeros((C, ldN), **f64) for _ in range(2))

        def per_chunk(c0, Xc, Yc):
            nc = Xc.shape[0]
            mean, var = (torch.empty((C, nc), **f64) for _ in range(2))      # unit-variance moments
            _marginals(H, likelihood, Xc, z, ell, W, m, S, mode, (mean, var))
            wc, rc = w[:, c0:c0 + nc], r[:, c0:c0 + nc]
            mu = mean * np.sqrt(k)
            ls, dp = likelihood.weights(H, state, Yc.reshape(-1), mean, var, np.sqrt(k), k, (wc, rc), mu, lik_grad=lik_grad)
            Pc, bc = _weighted_stats(H, Xc, wc, rc, z, ell, W)
            parts = (Pc, bc, ls, (rc * mu - wc * var * k).sum())
            return parts + (dp,) if lik_grad else parts

        # chunks of a multiple of 32 rows: every chunk of a row of w stays 16-byte aligned
        Phi, b, lsum, dks, *dps = _walk_f64(torch, Xd, Yd, M, 32, per_chunk)
        # tail: G_c = dF/dPhi_c, g_c = dF/db_c; T is linear in the latent functions, so one Cholesky VJP and one Gram VJP
        # serve all
        zbar = ellbar = T = None
        for c in range(C):
            Gm = H.matutil((H.matmul(S[c], S[c], transB=True) * (-0.5 * k)).contiguous(), H.MATUTIL_ADD_EYE, alpha=0.5 * rho * k)
            g = (m[c:c + 1] * np.sqrt(k)).contiguous()
            Q = H.matmul(W, H.matmul(Gm, W), transA=True, alpha=2.0)
            R = H.matmul(W, g, transA=True, transB=True)
            if x_grad:
                zc, ec, xbar = H.sgp_wkgrad(Xd, w[c, :N], r[c, :N], z, ell, Q, R, x_grad=True)
            else:
                zc, ec = H.sgp_wkgrad(Xd, w[c, :N], r[c, :N], z, ell, Q, R)
            Tc = H.matmul(Gm, Phi[c].contiguous(), alpha=-2.0) - H.matmul(g, b[c:c + 1].contiguous(), transA=True)
            zbar, ellbar, T = (zc, ec, Tc) if T is None else (zbar + zc, ellbar + ec, T + Tc)
        zk, ek = self._kmm_grads(sess, z, ell, W, T.contiguous())
        # KL(q_c || N(0, I)) from S_c itself (natgrad_q forms it from Sigma and the factor of Lambda; see there), and
        # dF/dk_var: scalars on the host
        kl = sum(0.5 * (float((S0[c] * S0[c]).sum()) + float((m0[c] * m0[c]).sum()) - M)
                 - float(np.log(np.abs(np.diagonal(S0[c]))).sum()) for c in range(C))
        grad = dict(z=(zbar + zk).cpu().numpy(), lengthscales=(ellbar + ek).cpu().numpy(), k_var=float(dks.cpu()) / (2.0 * k))
        if lik_grad:
            grad["lik_param"] = float(dps[0].cpu()[0])
        if x_grad:
            grad["X"] = xbar.cpu().numpy()
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
        sess, zvar, ls = self._stats_session("pathwise_draws")
        torch, H = sess.torch, sess.H
        M, d = int(zvar.shape[0]), int(zvar.shape[1])
        m, s = self._q_moments(sess, q, M)
        z, ell, W, _ = self._whitening(sess, zvar, ls, None, None, "pathwise_draws", as_plans=True)
        omega, w, eps = _host.pathwise_noise(sess, "pathwise_draws", noise, seed, ((L, d), (S, 2 * L), (S, M)), double=True)
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
        return PathwiseDraws(sess, omega, coef, z, ell, float(np.sqrt(k_var)))

    # -- closed-form posterior: input gradients and acquisition functions ----------------------------------------------
    def posterior(self, q, k_var=1.0, residual="diagonal"):
        """The closed-form posterior of f = sqrt(k_var) (u A(x) + residual) under q(u) as a SparsePosterior: a snapshot
        (like PathwiseDraws) of z, the lengthscales, W = Lm^-1 with its fragment-major images, and (m, S) of q(u), on the
        device in the session's dtype, from which predict / predict_grad / acquisition / argmax / maximise run without
        a graph: the mean and variance of predict_f, their exact input gradients, and the closed-form acquisition
        functions EI, PI and UCB with their gradients and arg-max over any number of candidates (hb_sgp_predict_grad,
        hb_sgp_acq).  q as for pathwise_draws; K(z, z) is factorised as the plans do it (_whitening(as_plans=True)).
        residual: 'diagonal' or 'neglected'.  Restrictions and exception types are those of pathwise_draws."""
        _check_residual(residual)
        k_var = float(k_var)
        if not k_var > 0.0:
            raise ValueError("posterior: k_var > 0 expected (got %r)" % (k_var,))
        sess, zvar, ls = self._stats_session("posterior")
        M = int(zvar.shape[0])
        m, s = self._q_moments(sess, q, M, who="posterior")
        z, ell, W, frag = self._whitening(sess, zvar, ls, None, None, "posterior", as_plans=True)
        dt = sess.torch_dtype
        return SparsePosterior(sess, z, ell, W, frag, m.reshape(M).to(dt).contiguous(), s.to(dt).contiguous(), residual,
                               float(settings.numerics.jitter_level), k_var)

    def predict_multi(self, X, q, residual="diagonal"):
        """Unit-variance marginals (mean [C, n], var [C, n]) as device tensors of C latent functions with independent
        full-rank q(u_c), q = (m [C, M], S [C, M, M] lower), at the rows of X, from ONE pass (hb_sgp_predict_multi: A = W
        K(z, X) is formed once for all C).  K(z, z) is factorised as the plans do it.  residual: 'diagonal' or
        'neglected'.  Restrictions and exception types are those of natgrad_q for a multi-latent likelihood."""
        _check_residual(residual)
        m0, S0 = (np.asarray(a, dtype=np.float64) for a in q)
        if m0.ndim != 2 or S0.shape != (m0.shape[0], m0.shape[1], m0.shape[1]):
            raise ValueError("predict_multi: q = (m [C, M], S [C, M, M]) expected, got %s %s" % (m0.shape, S0.shape))
        sess, zvar, ls = self._stats_session("predict_multi")
        if m0.shape[1] != int(zvar.shape[0]):
            raise ValueError("predict_multi: q is over %d inducing points, z holds %d" % (m0.shape[1], int(zvar.shape[0])))
        H = sess.H
        Xd = _host.device_data(sess, X, "X")
        z, ell, W, frag = self._whitening(sess, zvar, ls, None, None, "predict_multi", as_plans=True)
        if Xd.shape[1] != z.shape[1]:
            raise ValueError("predict_multi: X %s does not match z %s" % (tuple(Xd.shape), tuple(z.shape)))
        fused = bool(getattr(settings.runtime, "fused_predict", True)) and H.sgp_predict_multi_fused(
            sess.torch_dtype, Xd.shape[0], m0.shape[1], Xd.shape[1], m0.shape[0], frag is not None)
        return H.sgp_predict_multi(Xd, z, ell, W, _host.upload(sess, m0), _host.upload(sess, np.tril(S0)),
                                   mode=H.SGP_DIAGONAL if residual == "diagonal" else H.SGP_NEGLECTED,
                                   wfrag=frag if fused else None)

    def _q_moments(self, sess, q, M, who="pathwise_draws"):
        """(m [1, M], S [M, M] lower or s [M]) of q(u) as float64 device tensors, for pathwise_draws and posterior."""
        if isinstance(q, (tuple, list)):
            if len(q) != 2:
                raise ValueError("%s: q = (m [1, M], S [M, M] or s [M]) expected" % who)
            m, s = (np.asarray(a, dtype=np.float64) for a in q)
        else:
            from .gp import _posterior_of

            mt, st, _ = _posterior_of(q)
            for v in ("q_mu", "q_sqrt") + (("scale",) if type(q) is Gaussian else ()):
                sess.read_value(object.__getattribute__(q, v))      # uploads a value that was assigned and not yet written
            plan = sess.make_plan([mt, st])
            plan.run()
            plan.check()
            m, s = (np.asarray(plan.value(t), dtype=np.float64) for t in (mt, st))
        if m.ndim >= 2 and int(np.prod(m.shape[:-1])) > 1:
            raise NotImplementedError("%s: one latent function only (q has shape %s)" % (who, m.shape))
        if s.ndim >= 2 and s.shape[-2:] == (M, M):
            s = np.tril(s.reshape(M, M))
        elif s.size == M:
            s = s.reshape(M)
        else:
            raise ValueError("%s: S [%d, %d] lower or s [%d] expected, got %s" % (who, M, M, M, s.shape))
        if m.size != M:
            raise ValueError("%s: m [1, %d] expected, got %s" % (who, M, m.shape))
        return _host.upload(sess, m.reshape(1, M), np.float64), _host.upload(sess, s, np.float64)


class PathwiseDraws:
    """S posterior function draws of a SparseGP (SparseGP.pathwise_draws): a snapshot of the frequencies omega [L, d], the
    coefficient rows coef [S, 2L + M], z [M, d], the lengthscales and scale = sqrt(k_var), on the device in the session's
    dtype.  Later changes to the model do not move it.  Every evaluation is ONE launch of hb_sgp_pathwise, linear in n;
    the value at a point does not depend on the other points of the call, so the same draws can be evaluated in pieces,
    on a grid now and at candidates later, and maximised: evaluate_grad / grad give the exact input gradient in one launch
    (hb_sgp_pathwise_grad), argmax the best of any number of candidates without writing the [S, n] values
    (hb_sgp_pathwise_argmax), maximise refines each draw's best candidate by gradient ascent (Thompson sampling);
    acquisition / acquisition_argmax reduce the draws to a Monte-Carlo EI / PI over per-draw incumbents inside the kernel
    (hb_sgp_pathwise_acq) and select_batch builds a batch of q points from it."""

    def __init__(self, sess, omega, coef, z, ell, scale):
        self._sess = sess
        self._omega, self._coef, self._z, self._ell, self.scale = omega, coef, z, ell, float(scale)
        self.num_samples, self.num_features = int(coef.shape[0]), int(omega.shape[0])

    def evaluate(self, X, out=None):
        """The draws at the rows of X as a device tensor [S, n] of the session's dtype (`out`: written in place).  X: a
        Data / MinibatchData of the model (read in full from its device buffer), a device tensor or an array [n, d]."""
        return self._sess.H.sgp_pathwise(self._points(X), self._omega, self._z, self._ell, self._coef, scale=self.scale, out=out)

    def __call__(self, X):
        """The draws at the rows of X as numpy [S, n]."""
        return self.evaluate(X).cpu().numpy()

    def _points(self, X):
        Xd = _host.device_data(self._sess, X, "X")
        if Xd.shape[1] != self._z.shape[1]:
            raise ValueError("PathwiseDraws: X %s does not match z %s" % (tuple(Xd.shape), tuple(self._z.shape)))
        return Xd

    def evaluate_grad(self, X, values=True):
        """(values [S, n] or None, grad [S, n, d]) as device tensors: grad[s, j, k] = d f_s(x_j) / d x_jk, exact (a draw is
        a closed-form function), from ONE launch of hb_sgp_pathwise_grad.  The values are the bits of evaluate(X)."""
        return self._sess.H.sgp_pathwise_grad(self._points(X), self._omega, self._z, self._ell, self._coef, scale=self.scale,
                                              values=values)

    def grad(self, X):
        """The input gradients of the draws at the rows of X as numpy [S, n, d]."""
        return self.evaluate_grad(X, values=False)[1].cpu().numpy()

    def argmax(self, X, largest=True):
        """(idx int64 [S], value [S]) as numpy: for every draw the row of X at which it is largest (smallest with
        largest=False; ties: the first row) and its value there -- np.argmax(draws(X), 1) and the values it points at, bit
        for bit, from hb_sgp_pathwise_argmax: the [S, n] matrix is never written, so n can be millions of candidates."""
        best, idx = self._sess.H.sgp_pathwise_argmax(self._points(X), self._omega, self._z, self._ell, self._coef,
                                                     scale=self.scale, largest=largest)
        return idx.cpu().numpy(), best.cpu().numpy()

    def maximise(self, X, steps=50, lr=0.05, bounds=None, largest=True):
        """(x_best [S, d], f_best [S], info): every draw maximised (minimised with largest=False) over the box `bounds`,
        starting from its own best candidate among the rows of X (argmax) and refined by `steps` steps of Adam ascent on
        the exact input gradient.  The optimiser runs on the host in float64 (beta = 0.9 / 0.999, epsilon = 1e-8, as the
        hyper-parameter fits) in lengthscale units u = x / ell, d f / d u = ell d f / d x, so that lr is a fraction of a
        lengthscale whatever the units of the data; after each step u is projected onto the box.  bounds = (lo [d],
        hi [d]); default: the per-column minimum and maximum of the candidates.  Each evaluation is ONE evaluate_grad launch
        at the S current points rounded to the session's dtype (the diagonal of its [S, S] result is used); `steps` steps
        take steps + 1 of them -- the start, for its gradient, and the point after every step -- on top of the two
        launches of argmax; steps = 0 takes none.  The best (value,
        point) seen is kept per draw, the start included: f_best is never worse than the candidates' extremum, and it is
        the bits of evaluate(x_best)[s, s].  info = dict(start_idx int64 [S], start_value [S], steps).  steps = 50 and
        lr = 0.05 are defaults, not measurements: with Adam's unit-sized steps they move a point by at most about 2.5
        lengthscales and settle within a few hundredths of one.  steps < 0, lr <= 0, bounds of another shape or with
        lo > hi, and X of another width raise ValueError."""
        sess = self._sess
        Xd = self._points(X)
        d, S, dt = int(Xd.shape[1]), self.num_samples, np.dtype(sess.np_dtype).type
        steps = int(steps)
        if steps < 0 or not float(lr) > 0.0:
            raise ValueError("maximise: steps >= 0 and lr > 0 expected (got %r, %r)" % (steps, lr))
        if Xd.shape[0] < 1:
            raise ValueError("maximise: at least one candidate expected")
        box = _host.ascent_box("maximise", Xd, bounds, d, dt)
        ell = np.broadcast_to(np.asarray(self._ell.cpu().numpy(), np.float64), (d,))
        idx, f0 = self.argmax(Xd, largest=largest)
        if np.any(idx < 0):
            raise ValueError("maximise: draw %d has no comparable value among the candidates" % int(np.argmax(idx < 0)))
        x = Xd[sess.torch.as_tensor(idx, device=Xd.device)].cpu().numpy()       # [S, d], the session's dtype
        info = dict(start_idx=idx, start_value=f0.copy(), steps=steps)
        ar = np.arange(S)

        def evaluate(xc):   # ONE launch at the S current points; the diagonal of its [S, S] result
            f, g = self.evaluate_grad(xc)
            return f.cpu().numpy()[ar, ar], g.cpu().numpy()[ar, ar].astype(np.float64)

        x_best, f_best = _host.adam_ascent(evaluate, x, f0, ell, box, 1.0 if largest else -1.0, steps, float(lr), dt)
        return x_best, f_best, info

    ACQ_KINDS = ("ei", "pi")

    def _acq_inputs(self, who, X, kind, best):
        """(candidates on the device, per-draw incumbents [S] as numpy of the session's dtype), checked."""
        if kind not in self.ACQ_KINDS:
            raise ValueError("%s: kind must be one of %s, got %r" % (who, self.ACQ_KINDS, kind))
        Xd = self._points(X)
        if Xd.shape[0] < 1:
            raise ValueError("%s: at least one candidate expected" % who)
        b = np.asarray(best, dtype=np.float64)
        if b.ndim == 0:
            if not np.isfinite(b):
                raise ValueError("%s: a finite incumbent `best` expected, got %r" % (who, best))
            b = np.full(self.num_samples, float(b))
        elif b.shape != (self.num_samples,):
            raise ValueError("%s: best must be a scalar or [%d] (one incumbent per draw), got %s" % (who, self.num_samples, b.shape))
        return Xd, b.astype(self._sess.np_dtype)

    def _acq(self, Xd, kind, b, largest, values):
        return self._sess.H.sgp_pathwise_acq(Xd, self._omega, self._z, self._ell, self._coef, _host.upload(self._sess, b),
                                             scale=self.scale, acq=kind, largest=bool(largest), values=values)

    def acquisition(self, X, kind="ei", best=0.0, largest=True):
        """The Monte-Carlo acquisition of the draws at the rows of X, as numpy [n]:
        'ei'  mean_s max(sigma (f_s(x) - best_s), 0)      'pi'  mean_s 1[sigma (f_s(x) - best_s) > 0]
        for maximising f (largest, sigma = +1) or minimising it (sigma = -1; the acquisition itself is to be MAXIMISED).
        `best`: the incumbent value of f, a finite scalar, or [S] -- one incumbent per draw, which is what makes the joint
        improvement of a BATCH cheap (select_batch).  The draws are reduced inside the evaluating kernel
        (hb_sgp_pathwise_acq), summed in double: the [S, n] values are never written, and the value at a point does not
        depend on the other points.  Another kind or shape of best, or an empty X, raise ValueError."""
        Xd, b = self._acq_inputs("acquisition", X, kind, best)
        return self._acq(Xd, kind, b, largest, True)[0].cpu().numpy()

    def acquisition_argmax(self, X, kind="ei", best=0.0, largest=True):
        """(idx, value): the row of X at which acquisition(X, ...) is largest (ties: the first row; a NaN is never chosen)
        and its value there, bit for bit, without writing anything of size n.  No comparable value: (-1, -inf)."""
        Xd, b = self._acq_inputs("acquisition_argmax", X, kind, best)
        _, bv, bi = self._acq(Xd, kind, b, largest, False)
        return int(bi.cpu().numpy()[0]), bv.cpu().numpy()[0]

    def select_batch(self, X, q, best, kind="ei", largest=True, steps=0, lr=0.05, bounds=None):
        """(x [q', d], gains [q'], info): a batch of up to q points to evaluate in parallel, built greedily for the joint
        improvement  qEI(x_1 .. x_q) = E max_i (sigma (f(x_i) - best))_+  ~  mean_s max_i (sigma (f_s(x_i) - best_s))_+
        of the draws (Wilson et al. 2020, section 5; kind 'pi': the probability that some point of the batch improves).
        Each round is ONE acquisition_argmax launch over the rows of X under PER-DRAW incumbents b_s -- its value the
        marginal gain of the point given the points before it -- and one evaluate at the chosen point x*, after which
        b_s <- max(b_s, f_s(x*)) (min with largest=False) on the host.  The loop ends early once the gain is exactly 0,
        so q' <= q.  steps > 0 ('ei' only): every chosen candidate is first refined by `steps` steps of the projected
        Adam ascent of maximise (_host.adam_ascent; lr, bounds as there) on its marginal gain mean_s (sigma (f_s - b_s))_+
        with the gradient mean_s 1[sigma (f_s - b_s) > 0] sigma grad f_s, both from ONE evaluate_grad launch at the
        current point; the best point seen is kept, the candidate included.  gains: float64; with steps = 0 they are the
        kernel's values and never increase.  info = dict(idx int64 [q'] the starting candidates, incumbents [S] the final
        b, joint = sum of the gains = the joint acquisition of the batch, steps).  q < 1, an empty X, X of another width,
        steps < 0, lr <= 0, malformed bounds or best, and steps > 0 with 'pi' (its gradient is zero almost everywhere)
        raise ValueError."""
        who = "select_batch"
        sess = self._sess
        Xd, b0 = self._acq_inputs(who, X, kind, best)
        d, dt, steps = int(Xd.shape[1]), np.dtype(sess.np_dtype).type, int(steps)
        if int(q) < 1:
            raise ValueError("%s: q >= 1 expected (got %r)" % (who, q))
        if steps < 0 or not float(lr) > 0.0:
            raise ValueError("%s: steps >= 0 and lr > 0 expected (got %r, %r)" % (who, steps, lr))
        if steps and kind != "ei":
            raise ValueError("%s: steps > 0 needs kind 'ei' (the gradient of %r is zero almost everywhere)" % (who, kind))
        box = _host.ascent_box(who, Xd, bounds, d, dt)
        ell = np.broadcast_to(np.asarray(self._ell.cpu().numpy(), np.float64), (d,))
        sign = 1.0 if largest else -1.0

        def argmax_fn(b):
            _, bv, bi = self._acq(Xd, kind, b, largest, False)
            idx, gain = int(bi.cpu().numpy()[0]), float(bv.cpu().numpy()[0])
            if idx < 0 or gain == 0 or not steps:
                return idx, gain, (Xd[idx:idx + 1].cpu().numpy() if idx >= 0 else None)
            b64 = b.astype(np.float64)[:, None]

            def evaluate(xc):   # ONE launch at the single current point: the gain and its gradient
                f, g = self.evaluate_grad(xc)
                t = sign * (f.cpu().numpy().astype(np.float64) - b64)                        # [S, 1]
                on = (t > 0.0)[:, :, None]
                return np.maximum(t, 0.0).mean(0), (on * (sign * g.cpu().numpy().astype(np.float64))).mean(0)

            x, a = _host.adam_ascent(evaluate, Xd[idx:idx + 1].cpu().numpy(), np.array([gain]), ell, box, 1.0, steps, float(lr), dt)
            return idx, float(a[0]), x

        picks, gains, b = _host.greedy_batch(argmax_fn, lambda x: self.evaluate(x).cpu().numpy()[:, 0], b0, int(q), sign)
        xs = np.concatenate([x for _, x in picks], 0) if picks else np.zeros((0, d), dt)
        info = dict(idx=np.asarray([i for i, _ in picks], np.int64), incumbents=b, joint=float(np.sum(gains)), steps=steps)
        return xs, gains, info

    def _view(self, t):
        a = t.cpu().numpy()
        a.flags.writeable = False
        return a

    omega = property(lambda self: self._view(self._omega), doc="frequencies [L, d] (read-only numpy)")
    coef = property(lambda self: self._view(self._coef), doc="coefficient rows [S, 2L + M] = [w / sqrt(L) | v]")
    z = property(lambda self: self._view(self._z), doc="inducing points [M, d]")
    lengthscales = property(lambda self: self._view(self._ell), doc="lengthscales [1] or [d]")


class SparsePosterior:
    """The closed-form posterior of a SparseGP at one q(u) (SparseGP.posterior): a snapshot of z [M, d], the lengthscales,
    W = chol(K(z, z) + jitter I)^-1 with its fragment-major images, m [M] and S ([M, M] lower, or s [M]) of q(u), the
    residual mode, the jitter and k_var, on the device in the session's dtype.  Later changes to the model do not move it.
    Inputs are a Data / MinibatchData of the model (read in full from its device buffer), a device tensor or an array
    [n, d]; outputs are numpy.  Every result at a point is independent of the other points of the call."""

    KINDS = ("ei", "pi", "ucb")

    def __init__(self, sess, z, ell, W, frag, m, s, residual, jitter, k_var):
        self._sess = sess
        self._z, self._ell, self._W, self._frag, self._m, self._s = z, ell, W, frag, m, s
        H = sess.H
        self._s_kind = H.SGP_S_TRIL if s.dim() == 2 else H.SGP_S_DIAG
        self._mode = H.SGP_DIAGONAL if residual == "diagonal" else H.SGP_NEGLECTED
        self.residual, self.jitter, self.k_var = residual, float(jitter), float(k_var)

    def _points(self, X, who="X"):
        Xd = _host.device_data(self._sess, X, who)
        if Xd.shape[1] != self._z.shape[1]:
            raise ValueError("SparsePosterior: %s %s does not match z %s" % (who, tuple(Xd.shape), tuple(self._z.shape)))
        return Xd

    def _model(self):
        return (self._z, self._ell, self._W, self._m, self._s)

    def _kw(self):
        return dict(s_kind=self._s_kind, mode=self._mode, jitter=self.jitter, wfrag=self._frag)

    def predict(self, X):
        """(mean [n], var [n]) of f at the rows of X: the numbers of SVGP.predict_f (hb_sgp_predict, scaled by
        sqrt(k_var) / k_var)."""
        H = self._sess.H
        z, ell, W, m, s = self._model()
        mean, var = H.sgp_predict(self._points(X), z, ell, W, m.reshape(1, -1), s, **self._kw())
        return np.sqrt(self.k_var) * mean.cpu().numpy().reshape(-1), self.k_var * var.cpu().numpy().reshape(-1)

    def predict_uncertain(self, X_mean, X_var):
        """(mean [n], var [n]) of f at GAUSSIAN inputs x*_j ~ N(X_mean_j, diag(X_var_j)), as numpy float64: the exact first
        two moments of f(x*) over both the posterior and the input (Girard et al. 2003; Quinonero-Candela et al. 2003),
            beta = W^T m,   Q = W^T (rho I - S S^T) W - beta beta^T        (rho = 1 for 'diagonal', 0 for 'neglected')
            mean = sqrt(k_var) beta^T psi1,   var = k_var (rho - sum_mm' Q_mm' psi2(m, m') - (beta^T psi1)^2),
        the law of total variance over the conditional k_var (rho (1 - sum A^2) + |S^T A|^2), with psi1 = E k(z, x*),
        psi2 = E k(z, x*) k(x*, z) (hb_sgp_psi_predict).  X_var: [n, d], [d] or a scalar, finite and >= 0 (ValueError
        otherwise).  predict() takes |1 - sum A^2|; an absolute value cannot pass through the expectation, so this
        takes the difference itself: with X_var = 0 the two agree wherever 1 - sum A^2 >= 0, which the jitter guarantees
        up to round-off.  beta and Q are built in float64 from the snapshot (a mean-field q: S S^T = diag(s^2)), and the
        expectations are evaluated in double whatever the session's dtype."""
        sess = self._sess
        torch, H = sess.torch, sess.H
        Xd = self._points(X_mean, "X_mean")
        Vd = _input_variance(sess, X_var, Xd, "predict_uncertain")
        z, ell, W, m, s = self._model()
        M = int(z.shape[0])
        rho = 1.0 if self.residual == "diagonal" else 0.0
        W64, s64 = W.to(torch.float64), s.to(torch.float64)
        beta = H.matmul(m.to(torch.float64).reshape(1, M).contiguous(), W64)              # beta^T = m^T W  [1, M]
        SS = H.matmul(s64, s64, transB=True) if s.dim() == 2 else torch.diag(s64 * s64)
        inner = H.matutil((SS * -1.0).contiguous(), H.MATUTIL_ADD_EYE, alpha=rho)         # rho I - S S^T
        Q = H.matmul(W64, H.matmul(inner, W64), transA=True) - H.matmul(beta, beta, transA=True)
        e1, e2 = H.sgp_psi_predict(Xd, Vd, z, ell, beta.reshape(M), H.matutil(Q.contiguous(), H.MATUTIL_SYM))
        e1, e2 = e1.cpu().numpy(), e2.cpu().numpy()
        return np.sqrt(self.k_var) * e1, self.k_var * (rho - e2 - e1 * e1)

    def predict_grad(self, X):
        """(mean [n], var [n], dmean [n, d], dvar [n, d]): predict's moments and their exact input gradients
        dmean[j, k] = d mean[j] / d x_jk from ONE pass (hb_sgp_predict_grad), scaled by sqrt(k_var) / k_var."""
        out = self._sess.H.sgp_predict_grad(self._points(X), *self._model(), **self._kw())
        mean, var, dmean, dvar = (t.cpu().numpy() for t in out)
        sc = np.sqrt(self.k_var)
        return sc * mean, self.k_var * var, sc * dmean, self.k_var * dvar

    def _acq_args(self, who, kind, best, xi, beta, var_floor):
        if kind not in self.KINDS:
            raise ValueError("%s: kind must be one of %s, got %r" % (who, self.KINDS, kind))
        if kind != "ucb" and best is None:
            raise ValueError("%s: the acquisition %r needs `best`, the incumbent value" % (who, kind))
        var_floor = self.k_var * self.jitter if var_floor is None else float(var_floor)
        if not var_floor >= 0.0:
            raise ValueError("%s: var_floor >= 0 expected (got %r)" % (who, var_floor))
        return dict(best=0.0 if best is None else float(best), param=float(beta if kind == "ucb" else xi),
                    scale=float(np.sqrt(self.k_var)), var_floor=var_floor)

    def _acq(self, Xd, kind, largest, args, **what):
        return self._sess.H.sgp_acq(Xd, *self._model(), kind, largest=bool(largest), **args, **self._kw(), **what)

    def acquisition(self, X, kind, best=None, xi=0.0, beta=2.0, largest=True, grad=False, var_floor=None):
        """The acquisition function `kind` at the rows of X, as numpy [n] -- with grad=True (values [n], gradient [n, d]):
        'ei'  expected improvement       sigma (u Phi(u) + phi(u)),   u = (s mean - s best - xi) / sigma
        'pi'  probability of improvement Phi(u)
        'ucb' upper confidence bound     s mean + beta sigma
        for maximising f (largest, s = +1) or minimising it (s = -1; every acquisition itself is to be MAXIMISED), with
        mean and sigma^2 = max(var, var_floor) those of predict.  `best`, the incumbent value of f, is required for 'ei'
        and 'pi' (ValueError without it).  var_floor=None: k_var * jitter_level; where the variance was clamped the
        gradient does not pass through it.  The tail is evaluated per point in double whatever the session's dtype
        (hb_sgp_acq)."""
        args = self._acq_args("acquisition", kind, best, xi, beta, var_floor)
        val, g, _, _ = self._acq(self._points(X), kind, largest, args, value=True, grad=bool(grad))
        return (val.cpu().numpy(), g.cpu().numpy()) if grad else val.cpu().numpy()

    def argmax(self, X, kind, best=None, xi=0.0, beta=2.0, largest=True, var_floor=None):
        """(idx, value): the row of X at which the acquisition is largest (ties: the first row; a NaN is never chosen) and
        its value there -- np.argmax(acquisition(X)) and the value it points at, bit for bit, without writing anything of
        size n, so X can be millions of candidates.  No comparable value: (-1, -inf)."""
        args = self._acq_args("argmax", kind, best, xi, beta, var_floor)
        Xd = self._points(X)
        if Xd.shape[0] < 1:
            raise ValueError("argmax: at least one candidate expected")
        _, _, bv, bi = self._acq(Xd, kind, largest, args, value=False, argmax=True)
        return int(bi.cpu().numpy()[0]), bv.cpu().numpy()[0]

    def maximise(self, X, kind, best=None, xi=0.0, beta=2.0, largest=True, var_floor=None, steps=50, lr=0.05, bounds=None,
                 starts=None):
        """(x_best [R, d], a_best [R], info): the acquisition maximised over the box `bounds` by `steps` steps of projected
        Adam ascent on its exact input gradient, from its best candidate among the rows of X (R = 1), or from every row
        of starts [R, d].  The optimiser is the one of PathwiseDraws.maximise: on the host in float64, in lengthscale
        units so that lr is a fraction of a lengthscale, each evaluation ONE hb_sgp_acq launch at the R current points
        rounded to the session's dtype; bounds = (lo [d], hi [d]), default the per-column minimum and maximum of X.  The
        best (value, point) seen is kept, the start included: a_best is never below the start's value and is the bits
        of acquisition(x_best).  info = dict(start_idx (None with starts), start_value [R], steps).  steps < 0, lr <= 0,
        malformed bounds or starts and X of another width raise ValueError."""
        sess = self._sess
        args = self._acq_args("maximise", kind, best, xi, beta, var_floor)
        Xd = self._points(X)
        d, dt = int(Xd.shape[1]), np.dtype(sess.np_dtype).type
        steps = int(steps)
        if steps < 0 or not float(lr) > 0.0:
            raise ValueError("maximise: steps >= 0 and lr > 0 expected (got %r, %r)" % (steps, lr))
        if Xd.shape[0] < 1:
            raise ValueError("maximise: at least one candidate expected")
        box = _host.ascent_box("maximise", Xd, bounds, d, dt)
        ell = np.broadcast_to(np.asarray(self._ell.cpu().numpy(), np.float64), (d,))

        def evaluate(xc):
            val, g, _, _ = self._acq(_host.upload(sess, xc), kind, largest, args, value=True, grad=True)
            return val.cpu().numpy(), g.cpu().numpy().astype(np.float64)

        if starts is None:
            _, _, bv, bi = self._acq(Xd, kind, largest, args, value=False, argmax=True)
            idx, f0 = bi.cpu().numpy(), bv.cpu().numpy()
            if idx[0] < 0:
                raise ValueError("maximise: the acquisition has no comparable value among the candidates")
            x = Xd[bi].cpu().numpy()
        else:
            x = np.ascontiguousarray(np.asarray(starts, dtype=dt))
            if x.ndim != 2 or x.shape[1] != d or x.shape[0] < 1:
                raise ValueError("maximise: starts [R, %d] expected, got %s" % (d, x.shape))
            idx, f0 = None, evaluate(x)[0]
        info = dict(start_idx=idx, start_value=f0.copy(), steps=steps)
        x_best, a_best = _host.adam_ascent(evaluate, x, f0, ell, box, 1.0, steps, float(lr), dt)
        return x_best, a_best, info

    def _view(self, t):
        a = t.cpu().numpy()
        a.flags.writeable = False
        return a

    z = property(lambda self: self._view(self._z), doc="inducing points [M, d] (read-only numpy)")
    lengthscales = property(lambda self: self._view(self._ell), doc="lengthscales [1] or [d]")
    W = property(lambda self: self._view(self._W), doc="W = chol(K(z, z) + jitter I)^-1 [M, M]")
    m = property(lambda self: self._view(self._m), doc="mean of q(u) [M]")
    S = property(lambda self: self._view(self._s), doc="factor of q(u): [M, M] lower, or the standard deviations [M]")


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
    idx, pivots, count, trace = sess.H.sgp_select(_host.upload(sess, X), _host.upload(sess, ell), M, thr)
    count = int(count.cpu()[0])
    if count < M:
        raise ValueError("greedy_inducing: only %d of the %d points asked for have a conditional variance above the "
                         "threshold %g (use fewer inducing points or a lower threshold)" % (count, M, thr))
    idx = idx.cpu().numpy()
    Z = X[idx].copy()
    if not return_info:
        return Z
    return Z, dict(idx=idx, pivots=pivots.cpu().numpy(), trace=float(trace.cpu()[0]), count=count)
