"""The build's own model counterparts of the BASELINE configurations: SVGP (cfg 1/2/3),
Amortised (cfg 4), ExpertsGPR (cfg 5), plus the dense GPR and the two-expert form of the notebooks.
Used by bench.py, __graft_entry__.smoke() and the test suites.

Written the way a reference user would write them (SURVEY.md Appendix C;
reference notebooks/GaussianProcess.ipynb:109-159), with `tf = hb.tf`.
"""
import numpy as np

import henbun_amd as hb  # noqa: E402  (the package is fully imported before this module is)
from henbun_amd.gp._host import upload
from henbun_amd.param import tri_pack, tri_unpack

tf = hb.tf


def _adam_ascent(model, evaluate, steps, lr, train_z):
    """The host-side float64 Adam ASCENT loop SVGP.fit_hyper, SVGPLik.fit_hyper and SVGPMulticlass.fit_hyper share: `steps` steps on the raw
    parameters of model._hyper_variables() (z only with train_z) with the (value, raw gradient) `evaluate()` returns,
    written back after every step.  Returns the trace of values, steps + 1 entries.  A graph.CholeskyError out of
    `evaluate` is re-raised with the raw parameters of the last successful evaluation restored."""
    from henbun_amd.graph import CholeskyError

    model.initialize()
    sess = model._session
    hv = model._hyper_variables()
    names = [n for n in hv if train_z or n != "z"]
    for v in hv.values():
        sess.read_value(v)   # uploads a value that was assigned and not yet written
    raw = {n: sess.read_raw(hv[n]).astype(np.float64) for n in names}
    m1 = {n: np.zeros_like(raw[n]) for n in names}
    m2 = {n: np.zeros_like(raw[n]) for n in names}
    b1, b2, eps = 0.9, 0.999, 1e-8
    good = {n: raw[n].copy() for n in names}
    trace = []
    for t in range(int(steps) + 1):
        try:
            value, grad = evaluate()
        except CholeskyError:
            for n in names:
                sess.write_raw(hv[n], good[n])
            raise
        trace.append(value)
        good = {n: raw[n].copy() for n in names}
        if t == int(steps):
            break
        for n in names:
            m1[n] = b1 * m1[n] + (1.0 - b1) * grad[n]
            m2[n] = b2 * m2[n] + (1.0 - b2) * grad[n] ** 2
            step = lr * (m1[n] / (1.0 - b1 ** (t + 1))) / (np.sqrt(m2[n] / (1.0 - b2 ** (t + 1))) + eps)
            sess.write_raw(hv[n], raw[n] + step)
            raw[n] = sess.read_raw(hv[n]).astype(np.float64)   # what the session holds (rounded in a float32 session)
    return np.asarray(trace)


def _chain_to_raw(model, cons):
    """Gradients with respect to the RAW parameters of model._hyper_variables() from those with respect to the constrained
    values `cons` (same names): shaped like the raw arrays and multiplied by the transforms' dforward, float64 numpy."""
    sess = model._session
    grad = {}
    for name, v in model._hyper_variables().items():
        raw = sess.read_raw(v)
        grad[name] = np.reshape(np.asarray(cons[name], dtype=np.float64), raw.shape) * v.transform.dforward(raw)
    return grad


def _part(model, name):
    """The child object `name` itself, also inside tf_mode (where plain attribute access hands out its tensor)."""
    return object.__getattribute__(model, name)


def _scalar(model, name):
    """The value of the [1] Variable `name` as a float."""
    return float(np.ravel(_part(model, name).value)[0])


def _write_q(model, m, S):
    """Write q(u) = N(m, S S^T) into model.u in its own parametrisation: q_mu = m; q_sqrt = the log standard deviations
    for q_shape 'diagonal' (S is then s [M]), the lower-triangular factor (packed or dense) for 'fullrank'."""
    q, sess = _part(model, "u"), model._session
    sess.write_raw(_part(q, "q_mu"), np.reshape(m, -1))
    if q.q_shape == "diagonal":
        sess.write_raw(_part(q, "q_sqrt"), np.log(S))
    else:
        sess.write_raw(_part(q, "q_sqrt"), tri_pack(S) if q.packed else S)


def _suggest_batch(model, mean, Xcand, q, kind, largest, num_samples, num_features, seed, steps, kw):
    """The shared body of the models' suggest_batch: the incumbent from the posterior mean over the training inputs,
    the draws from sample_functions, the batch from PathwiseDraws.select_batch."""
    best = float(np.max(mean) if largest else np.min(mean))
    draws = model.sample_functions(num_samples, num_features=num_features, seed=seed)
    x, gains, info = draws.select_batch(Xcand, q, best, kind=kind, largest=largest, steps=steps, **kw)
    info["best"], info["draws"] = best, draws
    return x, gains, info


class SVGP(hb.model.Model):
    """Sparse variational GP regression: cfg 1/2 (q_shape='diagonal') and cfg 3 ('fullrank')."""

    def setUp(self, X, Y, Z, q_shape="diagonal", residual="diagonal", eps=None):
        self.N = X.shape[0]
        self.X = hb.param.MinibatchData(X)
        self.Y = hb.param.MinibatchData(Y)
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
        self.u = hb.variationals.Normal(shape=[1, Z.shape[0]], q_shape=q_shape)
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.residual = residual
        self.eps = None if eps is None else hb.param.MinibatchData(eps)  # injected residual noise (parity runs)

    @hb.model.AutoOptimize()
    def ELBO(self):
        f = self.gp.samples(self.X, self.u, q_shape=self.residual, eps=self.eps) * tf.sqrt(self.k_var)
        n = tf.shape(self.X)[0]
        ll = tf.reduce_sum(hb.densities.gaussian(tf.transpose(self.Y), f, self.var))
        return (self.N / n) * ll - self.KL()

    def _predict(self, Xnew, noise, full_cov=False, num_samples=None):
        """One plan: (mean sqrt(k_var), var k_var [+ var of the likelihood]) at Xnew, as numpy -- with full_cov the
        covariance [1, n, n] times k_var instead of var; with num_samples joint draws [num_samples, n] of f (the model's
        ELBO convention f = samples * sqrt(k_var) for all three)."""
        Xnew = np.asarray(Xnew)
        q = _part(self, "u")
        self.initialize()
        with self.tf_mode():
            if num_samples is not None:
                f = self.gp.predict_f_samples(Xnew, q, num_samples, q_shape=self.residual)
                outs = [tf.reshape(f * tf.sqrt(self.k_var), [int(num_samples), Xnew.shape[0]])]
            else:
                mean, var = self.gp.predict_f(Xnew, q, q_shape=self.residual, full_cov=full_cov)
                mean = mean * tf.sqrt(self.k_var)
                var = var * self.k_var
                if noise:
                    var = var + self.var
                outs = [mean, var]
        plan = self._session.make_plan(outs)
        plan.run()
        plan.check()
        return tuple(plan.value(o) for o in plan.outputs) if num_samples is None else plan.value(plan.outputs[0])

    def predict_f(self, Xnew, full_cov=False):
        """Closed-form posterior mean and variance of the latent f at Xnew [n, 1]: arrays [1, n] (SparseGP.predict_f
        scaled by k_var, the model's ELBO convention f = samples * sqrt(k_var)); full_cov=True: the covariance [1, n, n]
        in place of the variance."""
        return self._predict(Xnew, False, full_cov=full_cov)

    def predict_f_samples(self, Xnew, num_samples):
        """num_samples joint posterior draws of the latent f at Xnew [n, 1]: array [num_samples, n]
        (SparseGP.predict_f_samples with the model's residual, scaled by sqrt(k_var))."""
        return self._predict(Xnew, False, num_samples=num_samples)

    def predict_y(self, Xnew):
        """predict_f plus the Gaussian likelihood's variance: the predictive of a new observation y at Xnew."""
        return self._predict(Xnew, True)

    def sample_functions(self, num_samples, num_features=1024, seed=0, noise=None):
        """num_samples posterior function draws of the latent f as an hb.gp.PathwiseDraws (SparseGP.pathwise_draws at the
        model's q(u), scaled by sqrt(k_var)): draws = model.sample_functions(16); draws(Xnew) is numpy [16, n], linear in
        n, and every call evaluates the SAME sample paths.  The draws carry the exact conditional of the sparse GP (the
        'fullrank' residual) whatever `residual` the model trains with; predict_f_samples stays the exact joint route for
        small n.  draws.argmax(candidates) and draws.maximise(candidates) pick each draw's next point (Thompson sampling)."""
        self.initialize()
        return _part(self, "gp").pathwise_draws(_part(self, "u"), num_samples, num_features=num_features,
                                                k_var=_scalar(self, "k_var"), seed=seed, noise=noise)

    def posterior(self):
        """The closed-form posterior of the latent f at the model's q(u) as an hb.gp.SparsePosterior (SparseGP.posterior
        with the model's k_var and residual): post.predict(X) are the numbers of predict_f, post.predict_grad(X) their
        input gradients, post.acquisition / argmax / maximise the closed-form EI, PI and UCB over candidates."""
        self.initialize()
        return _part(self, "gp").posterior(_part(self, "u"), k_var=_scalar(self, "k_var"), residual=self.residual)

    def suggest(self, Xcand, kind="ei", largest=True, steps=50, **kw):
        """(x_next [d], value, info): the next point of a sequential design -- the acquisition `kind` ('ei', 'pi', 'ucb')
        of posterior() maximised from its best candidate among the rows of Xcand [n, d] (SparsePosterior.maximise; **kw:
        xi, beta, var_floor, lr, bounds).  The incumbent `best` is the largest (smallest with largest=False) posterior
        mean over the model's training inputs, from one predict pass; info also holds it."""
        post = self.posterior()
        mean, _ = post.predict(_part(self, "X"))
        best = float(mean.max() if largest else mean.min())
        x, a, info = post.maximise(Xcand, kind, best=best, largest=largest, steps=steps, **kw)
        info["best"] = best
        return x[0], a[0], info

    def suggest_batch(self, Xcand, q, kind="ei", largest=True, num_samples=64, num_features=1024, seed=0, steps=0, **kw):
        """(X_next [q', d], gains [q'], info): up to q points of Xcand [n, d] to evaluate IN PARALLEL -- the greedy batch
        for the joint Monte-Carlo improvement ('ei'; 'pi': probability of improvement) of num_samples posterior function
        draws (sample_functions(num_samples, num_features, seed); PathwiseDraws.select_batch; **kw: lr, bounds).  The
        incumbent is suggest's: the largest (smallest with largest=False) posterior mean over the model's training
        inputs.  gains[i] is the marginal gain of point i given the points before it and info['joint'] their sum, the
        joint acquisition of the batch; info also holds 'best', the incumbent, and 'draws', the PathwiseDraws used.
        steps > 0 refines every point by gradient ascent ('ei' only); q' < q when no draw improves any further."""
        mean, _ = self.posterior().predict(_part(self, "X"))
        return _suggest_batch(self, mean, Xcand, q, kind, largest, num_samples, num_features, seed, steps, kw)

    def _closed_form_inputs(self):
        """(X, Y, noise variance, k_var) of the whole data set at the current hyper-parameters."""
        self.initialize()
        return _part(self, "X"), _part(self, "Y"), _scalar(self, "var"), _scalar(self, "k_var")

    def _psi_stats(self, X_var):
        """None, or the statistics of the model's X read as input MEANS with variances X_var (SparseGP.psi_statistics)."""
        if X_var is None:
            return None
        X, Y, _, _ = self._closed_form_inputs()
        return _part(self, "gp").psi_statistics(X, X_var, Y)

    def fit_q(self, X_var=None):
        """Set q(u) to its closed-form optimum at the current z, lengthscales, k_var and var, from ONE pass over the
        model's full device-resident X, Y (SparseGP.optimal_q; not a minibatch, no Adam step).  u.q_mu / u.q_sqrt are
        written in their own parametrisation -- log standard deviations for q_shape 'diagonal' (the mean-field optimum),
        the lower-triangular factor (packed or dense) for 'fullrank'.  Returns (m [1, M], S or s) as optimal_q does.
        X_var ([N, d], [d] or a scalar): the model's X are the MEANS of Gaussian inputs with these variances (known input
        noise), and q(u) is the optimum under them (SparseGP.psi_statistics)."""
        X, Y, var, k_var = self._closed_form_inputs()
        m, S = _part(self, "gp").optimal_q(X, Y, var, k_var, q_shape=_part(self, "u").q_shape, residual=self.residual,
                                           stats=self._psi_stats(X_var))
        _write_q(self, m, S)
        return m, S

    def predict_f_uncertain(self, Xmean, Xvar):
        """Mean and variance of the latent f at Gaussian inputs N(Xmean_j, diag(Xvar_j)) -- the exact first two moments
        over posterior and input -- as arrays [1, n] in the units of predict_f (SparsePosterior.predict_uncertain at the
        model's q(u), k_var and residual).  Xvar: [n, d], [d] or a scalar."""
        mean, var = self.posterior().predict_uncertain(np.asarray(Xmean), Xvar)
        return mean.reshape(1, -1), var.reshape(1, -1)

    def predict_y_uncertain(self, Xmean, Xvar):
        """predict_f_uncertain plus the Gaussian likelihood's variance, in the units of predict_y."""
        mean, var = self.predict_f_uncertain(Xmean, Xvar)
        return mean, var + _scalar(self, "var")

    def select_inducing(self, threshold=None):
        """Move z to the M rows of the model's own full X that greedy conditional-variance selection picks at the current
        lengthscales (SparseGP.select_inducing: one launch per point over the device-resident X); returns their row
        indices.  q(u) is NOT touched and no longer fits the new z: call fit_q() afterwards."""
        self.initialize()
        return _part(self, "gp").select_inducing(_part(self, "X"), threshold=threshold)

    def collapsed_bound(self, X_var=None):
        """The ELBO at the optimal q(u) for the current hyper-parameters (SparseGP.collapsed_bound on the full X, Y):
        what fit_q() followed by an exact evaluation of ELBO over all rows would give.  X_var: as for fit_q -- the bound
        under Gaussian inputs with means X and these variances."""
        X, Y, var, k_var = self._closed_form_inputs()
        return _part(self, "gp").collapsed_bound(X, Y, var, k_var, residual=self.residual, stats=self._psi_stats(X_var))

    def _hyper_variables(self):
        """The Variables collapsed_bound() depends on, by the names the gradient uses."""
        gp = _part(self, "gp")
        return dict(z=_part(gp, "z"), lengthscales=_part(_part(gp, "kern"), "lengthscales"), k_var=_part(self, "k_var"),
                    var=_part(self, "var"))

    def collapsed_bound_and_grad(self, X_var=None):
        """(value, grad): the collapsed bound and its exact gradient with respect to the RAW (free) parameters,
        grad = dict(z, lengthscales, k_var, var) in the shapes of the raw arrays, float64 numpy.
        SparseGP.collapsed_bound_and_grad on the full X, Y (float64 arithmetic whatever the session's dtype), chained
        through the transforms' dforward.  X_var ([N, d], [d] or a scalar; as for fit_q): the bound of
        collapsed_bound(X_var=X_var) and its gradient under Gaussian inputs with means X and these variances
        (SparseGP.psi_bound_and_grad; the gradients with respect to the inputs themselves are not returned)."""
        X, Y, var, k_var = self._closed_form_inputs()
        if X_var is None:
            value, gr = _part(self, "gp").collapsed_bound_and_grad(X, Y, var, k_var, residual=self.residual)
        else:
            value, gr = _part(self, "gp").psi_bound_and_grad(X, X_var, Y, var, k_var, residual=self.residual)
        return value, _chain_to_raw(self, dict(z=gr["z"], lengthscales=gr["lengthscales"], k_var=gr["k_var"], var=gr["noise_var"]))

    def fit_hyper(self, steps, lr=0.01, train_z=True, X_var=None):
        """Full-batch fit of the hyper-parameters: `steps` Adam ASCENT steps on the collapsed bound in the raw
        parameters of lengthscales, k_var, var and (train_z) z, on the host in float64 with the exact gradient of
        collapsed_bound_and_grad -- M d + dl + 2 numbers, two passes over the data per step, no minibatch noise.  The
        parameters are written back after every step and q(u) is set to its optimum (fit_q) at the end.  Returns the
        trace of bound values, steps + 1 entries: before the first step .. at the final parameters.  A step after
        which K(z, z) + jitter I or Lambda is no longer positive definite raises graph.CholeskyError with the last good
        parameters restored.  X_var: known input noise, as for fit_q -- the fit climbs collapsed_bound(X_var=X_var) and
        ends with fit_q(X_var=X_var)."""
        if X_var is None:
            trace = _adam_ascent(self, self.collapsed_bound_and_grad, steps, lr, train_z)
        else:
            trace = _adam_ascent(self, lambda: self.collapsed_bound_and_grad(X_var=X_var), steps, lr, train_z)
        self.fit_q(X_var=X_var)
        return trace


class BayesianGPLVM(hb.model.Model):
    """Bayesian GP latent-variable model (Titsias & Lawrence 2010): Y [N, P] = f(X) + noise with UNOBSERVED inputs, a
    variational q(X) = prod_n N(X_mean_n, diag(X_var_n)) over a latent space of `latent_dim` dimensions, the prior
    p(X) = N(0, I), a sparse GP with ARD lengthscales (one per latent dimension: a dimension the data do not need is
    switched off by a long lengthscale) and full-batch training on the collapsed bound from psi statistics minus
    KL(q(X) || p(X)):
        m = BayesianGPLVM(Y=Y, latent_dim=2, M=16);  trace = m.fit(200, lr=0.05);  mean, var = m.latent()
    X_mean: initial means [N, Q] (None: the first Q principal components of Y, scaled to unit variance); X_var: initial
    variances (a scalar or [N, Q]); Z: inducing points [M, Q] (None: hb.gp.greedy_inducing on the initial means).  Not in
    scope: a sampled ELBO, minibatches, back-constraints, the latent of a new observation, other priors."""

    def setUp(self, Y, latent_dim, M, X_mean=None, X_var=0.1, Z=None):
        Y = np.asarray(Y)
        N, Q = Y.shape[0], int(latent_dim)
        if X_mean is None:
            Yc = np.asarray(Y, np.float64) - np.mean(Y, 0)
            _, _, Vt = np.linalg.svd(Yc, full_matrices=False)
            X_mean = np.zeros((N, Q))
            r = min(Q, Vt.shape[0])
            X_mean[:, :r] = Yc @ Vt[:r].T
            sd = X_mean.std(0)
            X_mean = X_mean / np.where(sd > 0, sd, 1.0)
        X_mean = np.asarray(X_mean, np.float64)
        X_var = np.array(np.broadcast_to(np.asarray(X_var, np.float64), (N, Q)))
        if X_mean.shape != (N, Q) or not (np.all(np.isfinite(X_var)) and np.all(X_var > 0)):
            raise ValueError("BayesianGPLVM: X_mean must be [%d, %d] and X_var positive, a scalar or [%d, %d]" % (N, Q, N, Q))
        if Z is None:
            Z = hb.gp.greedy_inducing(X_mean, M, np.ones(Q), dtype=self._session.np_dtype)
        Z = np.asarray(Z, np.float64)
        if Z.shape != (int(M), Q):
            raise ValueError("BayesianGPLVM: Z must be [%d, %d], got %s" % (int(M), Q, Z.shape))
        self.Y = hb.param.Data(Y)
        self.X_mean = hb.param.Variable([N, Q])
        self.X_mean = X_mean
        self.X_var = hb.param.Variable([N, Q], transform=hb.transforms.positive)
        self.X_var = X_var
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(Q)), z=Z)
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        scale = float(np.mean(np.var(np.asarray(Y, np.float64), 0)))      # initial k_var: the mean column variance of Y
        self.k_var = np.ones(1) * (scale if scale > 0 else 1.0)
        self.var = np.ones(1) * (0.1 * scale if scale > 0 else 0.1)        # initial noise variance: a tenth of it
        self.residual = "diagonal"

    def _hyper_variables(self):
        """The Variables bound() depends on, by the names the gradient uses."""
        gp = _part(self, "gp")
        return dict(X_mean=_part(self, "X_mean"), X_var=_part(self, "X_var"), z=_part(gp, "z"),
                    lengthscales=_part(_part(gp, "kern"), "lengthscales"), k_var=_part(self, "k_var"), var=_part(self, "var"))

    def _inputs(self):
        """(X_mean [N, Q], X_var [N, Q] as the session stores them, float64 numpy; Y; noise variance; k_var)."""
        self.initialize()
        sess = self._session
        mu, s = (np.asarray(sess.read_value(_part(self, n)), np.float64) for n in ("X_mean", "X_var"))
        return mu, s, _part(self, "Y"), _scalar(self, "var"), _scalar(self, "k_var")

    def latent(self):
        """(mean [N, Q], var [N, Q]) of q(X), float64 numpy."""
        mu, s, _, _, _ = self._inputs()
        return mu, s

    @staticmethod
    def _kl(mu, s):
        """KL(q(X) || N(0, I)) and its gradients with respect to the means and the variances, on the host in double."""
        return 0.5 * float(np.sum(s + mu * mu - 1.0 - np.log(s))), mu, 0.5 * (1.0 - 1.0 / s)

    def bound(self):
        """The collapsed bound from psi statistics (SparseGP.collapsed_bound(stats=psi_statistics(..))) minus
        KL(q(X) || p(X)): a lower bound of log p(Y)."""
        mu, s, Y, var, k_var = self._inputs()
        gp = _part(self, "gp")
        return (gp.collapsed_bound(mu, Y, var, k_var, residual=self.residual, stats=gp.psi_statistics(mu, s, Y))
                - self._kl(mu, s)[0])

    def bound_and_grad(self):
        """(value, grad): the bound of bound(), evaluated in float64 (SparseGP.psi_bound_and_grad), and its exact gradient
        with respect to the RAW (free) parameters, grad = dict(X_mean, X_var, z, lengthscales, k_var, var) in the shapes of
        the raw arrays, float64 numpy.  The KL term and its gradient are added on the host in double."""
        mu, s, Y, var, k_var = self._inputs()
        value, gr = _part(self, "gp").psi_bound_and_grad(mu, s, Y, var, k_var, residual=self.residual)
        kl, kl_mu, kl_s = self._kl(mu, s)
        cons = dict(X_mean=gr["X_mean"] - kl_mu, X_var=gr["X_var"] - kl_s, z=gr["z"], lengthscales=gr["lengthscales"],
                    k_var=gr["k_var"], var=gr["noise_var"])
        return value - kl, _chain_to_raw(self, cons)

    def fit(self, steps, lr=0.01, train_z=True):
        """Full-batch fit: `steps` Adam ASCENT steps on bound_and_grad in the raw parameters of q(X), the lengthscales,
        k_var, var and (train_z) z, on the host in float64 (the loop of SVGP.fit_hyper).  Returns the trace of bound
        values, steps + 1 entries: before the first step .. at the final parameters."""
        return _adam_ascent(self, self.bound_and_grad, steps, lr, train_z)

    def fit_q(self):
        """(m [P, M], S [M, M]): the optimal q(u) at the current parameters under q(X) (SparseGP.optimal_q with the psi
        statistics), float64 numpy; S is shared by the P outputs."""
        mu, s, Y, var, k_var = self._inputs()
        gp = _part(self, "gp")
        return gp.optimal_q(mu, Y, var, k_var, residual=self.residual, stats=gp.psi_statistics(mu, s, Y))

    def predict_y(self, Xnew):
        """(mean [n, P], var [n]) of a new observation at the latent points Xnew [n, Q] under the optimal q(u) of
        fit_q(); S is shared by the outputs, so the variance is too.  Float64 on the device (hb_sgp_A_f64, hb_matmul_f64)."""
        m, S = self.fit_q()
        mu, _, Y, var, k_var = self._inputs()
        sess, _, _, z, ell, W = _part(self, "gp")._grad_inputs(mu, Y, "predict_y")
        torch, H = sess.torch, sess.H
        Xnew = np.asarray(Xnew, np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != mu.shape[1]:
            raise ValueError("predict_y: Xnew must be [n, %d], got %s" % (mu.shape[1], Xnew.shape))
        A = H.sgp_A(upload(sess, Xnew, carry=np.float64), z, ell, W)                          # [M, n]
        md, Sd = (upload(sess, a, dtype=np.float64) for a in (m, S))
        mean = H.matmul(A, md, transA=True, transB=True) * np.sqrt(k_var)                   # [n, P]
        SA = H.matmul(Sd, A, transA=True)
        v = k_var * ((1.0 - (A * A).sum(0)) + (SA * SA).sum(0)) + var
        return mean.cpu().numpy(), v.cpu().numpy()


class DeepKernelSVGP(hb.model.Model):
    """Deep kernel learning (Wilson et al. 2016): GP regression with a Gaussian likelihood on the FEATURES h = net(x) of a
    hb.nn.NeuralNet [D_in, *hidden, feature_dim], an RBF sparse GP with ARD lengthscales and M inducing points z in
    feature space, trained full-batch on the collapsed bound:
        m = DeepKernelSVGP(X=X, Y=Y, M=64, hidden=[32, 32], feature_dim=2);  trace = m.fit(200, lr=0.02)
        mean, var = m.predict_y(Xnew)
    X [N, D_in] and Y [N, P] are full-batch Data; activation: 'tanh', 'relu' or 'sigmoid' (after every layer but the
    last); Z: initial inducing points [M, feature_dim] (None: the features of the rows i N / M of X under the initial
    network, taken the first time they are needed; select_inducing() moves them to a greedy selection).  The weights start at N(0, 1 / fan-in) draws of numpy's global generator, the
    biases at 0.  feature_dim <= 4 takes the column-strip form of the gradient pass (M % 16 == 0, M <= 512), larger
    feature spaces its plain form.

    The gradient of the bound with respect to the features comes from the gradient pass itself (hb_sgp_kgrad_x,
    SparseGP.collapsed_bound_and_grad(x_grad=True)) and is chained through the network by the graph autodiff.  In a
    float32 session the features are float32: the bound and its gradient are taken at those stored values, exact in
    double like every float32 X, and the chain through the network is float32.
    Not in scope: a classification variant (on elbo_and_grad(x_grad=True)), minibatches, a MAP GP-LVM."""

    _ACTIVATIONS = dict(tanh=hb.nn.tanh, relu=hb.nn.relu, sigmoid=hb.nn.sigmoid)

    def setUp(self, X, Y, M, hidden=(32,), feature_dim=2, activation="tanh", Z=None):
        X, Y = np.asarray(X), np.asarray(Y)
        if activation not in self._ACTIVATIONS:
            raise ValueError("DeepKernelSVGP: activation must be one of %s, got %r" % (sorted(self._ACTIVATIONS), activation))
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError("DeepKernelSVGP: X [N, D_in] and Y [N, P] expected, got %s %s" % (X.shape, Y.shape))
        N, F = X.shape[0], int(feature_dim)
        nodes = [int(X.shape[1])] + [int(h) for h in hidden] + [F]
        self.X = hb.param.Data(X)
        self.Y = hb.param.Data(Y)
        self.Hbar = hb.param.Data(np.zeros((N, F)))               # the cotangent dF/dfeatures, written on the device
        self.net = hb.nn.NeuralNet(nodes, neuron_types=self._ACTIVATIONS[activation])
        for i in range(len(nodes) - 1):
            self.net[i].w = np.random.randn(nodes[i], nodes[i + 1]) / np.sqrt(nodes[i])
            self.net[i].b = np.zeros((1, nodes[i + 1]))
        self._z_given = Z is not None
        Z = np.zeros((int(M), F)) if Z is None else np.asarray(Z, np.float64)
        if Z.shape != (int(M), F):
            raise ValueError("DeepKernelSVGP: Z must be [%d, %d], got %s" % (int(M), F, Z.shape))
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(F)), z=Z)
        self.u = hb.variationals.Normal(shape=[Y.shape[1], int(M)], q_shape="fullrank")
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.residual = "diagonal"
        self._plans = {}

    def _net_variables(self):
        """The network's Variables by the names the gradient uses: net0.w, net0.b, net1.w, .."""
        net = _part(self, "net")
        return {"net%d.%s" % (i, n): _part(net[i], n) for i in range(len(net.nodes) - 1) for n in ("w", "b")}

    def _hyper_variables(self):
        """The Variables collapsed_bound() depends on, by the names the gradient uses."""
        gp = _part(self, "gp")
        hv = dict(z=_part(gp, "z"), lengthscales=_part(_part(gp, "kern"), "lengthscales"), k_var=_part(self, "k_var"),
                  var=_part(self, "var"))
        hv.update(self._net_variables())
        return hv

    def _plan(self, what):
        """The two plans over all rows, built once per parameter layout: 'forward' leaves H = net(X) [N, feature_dim] on
        the device; 'backward' returns J^T Hbar for every network variable, the gradients of sum(net(X) * Hbar) taken by
        the graph autodiff with Hbar a Data buffer."""
        sess = self._session
        key = (what, sess.layout_version)
        if key not in self._plans:
            Ht = _part(self, "net")(_part(self, "X").tensor())
            if what == "forward":
                outs = [Ht]
            else:
                leaves = [v._leaf for v in self._net_variables().values()]
                outs = hb.graph.gradients(hb.graph.reduce_sum(Ht * _part(self, "Hbar").tensor()), leaves)
            self._plans[key] = (sess.make_plan(outs), outs)
        return self._plans[key]

    def _features(self):
        """H = net(X) at the current weights as a device tensor [N, feature_dim] of the session's dtype (the forward
        plan's own buffer: valid until the plan runs again).  The first call without a given Z moves z to the features
        of the rows i N / M."""
        self.initialize()
        plan, outs = self._plan("forward")
        plan.run()
        plan.check()
        H = plan.buf(outs[0])
        if not self._z_given:
            self._z_given = True
            zvar = _part(_part(self, "gp"), "z")
            rows = (np.arange(zvar.shape[0]) * H.shape[0]) // zvar.shape[0]
            self._session.write_raw(zvar, zvar.transform.backward(H[rows.tolist()].cpu().numpy().astype(np.float64)))
        return H

    def features(self, Xnew=None):
        """net(X) (Xnew=None: the model's own inputs) or net(Xnew) as numpy [n, feature_dim], from one plan over all
        rows."""
        if Xnew is None:
            return self._features().cpu().numpy()
        self.initialize()
        return self.run(_part(self, "net")(hb.graph.as_tensor(np.asarray(Xnew))))

    def _closed_form_inputs(self):
        """(features on the device, Y, noise variance, k_var) at the current parameters."""
        H = self._features()
        return H, _part(self, "Y"), _scalar(self, "var"), _scalar(self, "k_var")

    def collapsed_bound(self):
        """The ELBO at the optimal q(u) for the current parameters (SparseGP.collapsed_bound on the features)."""
        H, Y, var, k_var = self._closed_form_inputs()
        return _part(self, "gp").collapsed_bound(H, Y, var, k_var, residual=self.residual)

    def bound_and_grad(self):
        """(value, grad): the collapsed bound and its exact gradient with respect to the RAW parameters, grad = dict(z,
        lengthscales, k_var, var, net0.w, net0.b, ..) in the shapes of the raw arrays, float64 numpy.  Four steps: the
        forward plan leaves H = net(X) on the device; SparseGP.collapsed_bound_and_grad(H, Y, .., x_grad=True) (float64
        arithmetic whatever the session's dtype) returns the value, the gradients of z, the lengthscales and the two
        variances and Hbar = dF/dH [N, feature_dim]; Hbar goes into the model's Data buffer on the device (rounded to
        the session's dtype); the backward plan returns J^T Hbar for the network's variables."""
        H, Y, var, k_var = self._closed_form_inputs()
        value, gr, xbar = _part(self, "gp")._collapsed_bound_and_grad(H, Y, var, k_var, self.residual, True)
        sess = self._session
        sess.data_buffer(_part(self, "Hbar")).copy_(xbar)
        sess.torch.cuda.synchronize()
        plan, outs = self._plan("backward")
        plan.run()
        plan.check()
        cons = dict(z=gr["z"], lengthscales=gr["lengthscales"], k_var=gr["k_var"], var=gr["noise_var"])
        for name, g in zip(self._net_variables(), outs):
            cons[name] = plan.value(g)
        return value, _chain_to_raw(self, cons)

    def fit(self, steps, lr=0.01, train_z=True):
        """Full-batch fit: `steps` Adam ASCENT steps on bound_and_grad in the raw parameters of the network, the
        lengthscales, k_var, var and (train_z) z, on the host in float64 (the loop of SVGP.fit_hyper: a step after which
        a factorisation fails raises graph.CholeskyError with the last good parameters restored), then fit_q().  Returns
        the trace of bound values, steps + 1 entries: before the first step .. at the final parameters."""
        self._features()                     # (a pending initial z is written before the loop reads it)
        trace = _adam_ascent(self, self.bound_and_grad, steps, lr, train_z)
        self.fit_q()
        return trace

    def fit_q(self):
        """Set q(u) to its closed-form optimum at the current parameters (SparseGP.optimal_q on the features); returns
        (m [P, M], S [M, M])."""
        H, Y, var, k_var = self._closed_form_inputs()
        m, S = _part(self, "gp").optimal_q(H, Y, var, k_var, q_shape="fullrank", residual=self.residual)
        _write_q(self, m, S)
        return m, S

    def select_inducing(self, threshold=None):
        """Move z to the features of the M rows greedy conditional-variance selection picks on the CURRENT features
        (SparseGP.select_inducing); returns their row indices.  q(u) is not touched: call fit_q() afterwards."""
        self._z_given = True
        return _part(self, "gp").select_inducing(self._features(), threshold=threshold)

    def _predict(self, Xnew, noise):
        Xnew = np.asarray(Xnew)
        q = _part(self, "u")
        self._features()
        with self.tf_mode():
            mean, var = self.gp.predict_f(self.net(hb.graph.as_tensor(Xnew)), q, q_shape=self.residual)
            mean, var = mean * tf.sqrt(self.k_var), var * self.k_var
            if noise:
                var = var + self.var
        plan = self._session.make_plan([mean, var])
        plan.run()
        plan.check()
        return tuple(plan.value(o) for o in plan.outputs)

    def predict_f(self, Xnew):
        """Closed-form posterior mean and variance of the latent f at Xnew [n, D_in], arrays [P, n]: the features of
        Xnew, then SparseGP.predict_f at the model's q(u), in one plan (units as SVGP.predict_f)."""
        return self._predict(Xnew, False)

    def predict_y(self, Xnew):
        """predict_f plus the Gaussian likelihood's variance."""
        return self._predict(Xnew, True)


class _SVGPNonConjugate(hb.model.Model):
    """What SVGPLik, SVGPMulticlass and SVGPHetero share: a likelihood (hb.likelihoods) over C = likelihood.num_latent
    latent functions of one SparseGP `gp`, a full-rank q(u) `u` of C blocks -- Normal(shape=[1, M]) or Normal(shape=[M],
    n_layers=[C]), packed or dense -- the Variable `k_var`, `residual`, the data X, Y, and optionally the likelihood's
    parameter as the Variable `lik_param` (learn_likelihood).  The deterministic full-batch routes live here once; a
    model adds setUp, the sampled ELBO, its predictions and its fit_q defaults."""

    learn_likelihood = False                  # True: `lik_param` holds the likelihood's parameter and fit_hyper learns it
    _gp_elbo_and_grad = "elbo_and_grad_multi"   # the SparseGP method elbo_and_grad() calls

    def current_likelihood(self):
        """The likelihood in use: the one handed in, or with learn_likelihood=True a copy that carries the current value
        of lik_param."""
        lik = _part(self, "likelihood")
        if not _part(self, "learn_likelihood"):
            return lik
        self.initialize()
        return lik.with_param(_scalar(self, "lik_param"))

    select_inducing = SVGP.select_inducing

    def _likelihood_residual(self):
        """The residual mode of the moments the closed-form routes hand to the likelihood: the model's own."""
        return self.residual

    def reset_q(self):
        """Set every block of q(u) to the prior N(0, I), where natgrad_q's own default starts.  A freshly built model holds
        a RANDOM q(u), from which a full natural-gradient step (rho = 1) overshoots: call this before the first fit_q() /
        fit_hyper()."""
        self.initialize()
        C, M = _part(self, "likelihood").num_latent, _part(self, "u").size
        self._write_blocks(np.zeros((C, M)), np.broadcast_to(np.eye(M), (C, M, M)))

    def _write_blocks(self, m, S):
        """Write q(u_c) = N(m_c, S_c S_c^T) into u in its own parametrisation: m [C, M]; S [C, M, M] (or [M, M] for one
        block) lower-triangular, stored packed or dense."""
        q, sess = _part(self, "u"), self._session
        mu, sq = _part(q, "q_mu"), _part(q, "q_sqrt")
        sess.write_raw(mu, np.reshape(m, mu._full_shape))
        sess.write_raw(sq, np.reshape(tri_pack(S) if q.packed else S, sq._full_shape))

    def _current_blocks(self):
        """(m [C, M], S [C, M, M] lower) of the model's q(u) as the session stores it, float64 numpy."""
        self.initialize()
        q, sess = _part(self, "u"), self._session
        M = q.size
        S = np.asarray(sess.read_raw(_part(q, "q_sqrt")), dtype=np.float64)
        S = tri_unpack(S.reshape(-1, M * (M + 1) // 2)) if q.packed else np.tril(S.reshape(-1, M, M))
        return np.asarray(sess.read_raw(_part(q, "q_mu")), dtype=np.float64).reshape(-1, M), S

    def _hyper_variables(self):
        """The Variables the ELBO at a fixed q(u) depends on, by the names the gradient uses."""
        gp = _part(self, "gp")
        hv = dict(z=_part(gp, "z"), lengthscales=_part(_part(gp, "kern"), "lengthscales"), k_var=_part(self, "k_var"))
        if _part(self, "learn_likelihood"):
            hv["lik_param"] = _part(self, "lik_param")
        return hv

    def _fit_q(self, steps, rho, tol):
        """fit_q of every model: SparseGP.natgrad_q from the model's CURRENT q(u) over the model's full device-resident X,
        Y at the current z, lengthscales, k_var and likelihood parameter; the blocks are written back.  rho=None: the
        likelihood's natgrad_rho."""
        self.initialize()
        lik = self.current_likelihood()
        m, S, info = _part(self, "gp").natgrad_q(_part(self, "X"), _part(self, "Y"), lik, k_var=_scalar(self, "k_var"),
                                                 residual=self._likelihood_residual(), q0=self._current_blocks(),
                                                 steps=steps, rho=lik.natgrad_rho if rho is None else rho, tol=tol)
        self._write_blocks(m, S)
        return m, S, info

    def elbo_and_grad(self):
        """(value, grad): the ELBO over the model's full X, Y at the model's CURRENT q(u) -- the value fit_q reports -- and
        its partial gradient at that q with respect to the RAW (free) parameters, grad = dict(z, lengthscales, k_var) and,
        with learn_likelihood=True, lik_param, in the shapes of the raw arrays, float64 numpy.  SparseGP.elbo_and_grad for
        one latent function, SparseGP.elbo_and_grad_multi for several (float64 arithmetic whatever the session's dtype;
        the moments fit_q takes, for SVGPMulticlass those without the residual), chained through the transforms'
        dforward.  After fit_q() has converged this is the total derivative of the fitted ELBO -- for SVGPMulticlass up to
        the node error of the step's curvature (see elbo_and_grad_multi)."""
        self.initialize()
        kw = dict(lik_grad=True) if _part(self, "learn_likelihood") else {}
        route = getattr(_part(self, "gp"), self._gp_elbo_and_grad)
        value, cons = route(_part(self, "X"), _part(self, "Y"), self.current_likelihood(), self._current_blocks(),
                            k_var=_scalar(self, "k_var"), residual=self._likelihood_residual(), **kw)
        return value, _chain_to_raw(self, cons)

    def fit_hyper(self, steps, lr=0.01, train_z=True, q_steps=5, rho=None):
        """Deterministic full-batch fit of the hyper-parameters, alternating as GPflow's natural-gradient recipe does:
        every outer step runs fit_q(steps=q_steps, rho=rho) from the current q(u), then takes ONE Adam ASCENT step on
        elbo_and_grad() in the raw parameters of lengthscales, k_var, (train_z) z and, with learn_likelihood=True, the
        likelihood's parameter -- on the host in float64, the loop of SVGP.fit_hyper.  No minibatch noise.  Ends with a
        fit_q() at the final parameters (at the likelihood's natgrad_rho, whatever `rho`).  Returns the trace of ELBO
        values, steps + 1 entries: after the first fit_q at the starting parameters .. after the closing fit_q()
        at the final ones.  A step after which a factorisation fails raises graph.CholeskyError with the last good
        parameters restored.  The first fit_q starts at the model's current q(u): from a freshly initialised (random)
        q a full step overshoots (see fit_q), so call reset_q() first (or fit q(u) some other way, or pass rho < 1).
        rho=None: the likelihood's natgrad_rho, as for fit_q."""
        steps, done = int(steps), [0]

        def evaluate():
            if done[0] == steps:
                self.fit_q()
            else:
                self.fit_q(steps=q_steps, rho=rho)
            done[0] += 1
            return self.elbo_and_grad()

        return _adam_ascent(self, evaluate, steps, lr, train_z)


class SVGPLik(_SVGPNonConjugate):
    """Sparse variational GP with a non-conjugate factorising likelihood (hb.likelihoods: Bernoulli, Poisson, Gaussian,
    Laplace, Gamma, Exponential, NegativeBinomial, Binomial) and a full-rank q(u): SVGP's latent model, the sampled ELBO
    with likelihood.logp, and a deterministic fit of q(u) by natural-gradient steps (SparseGP.natgrad_q).

    learn_likelihood=True (a `trainable` likelihood only: ValueError otherwise) makes the likelihood's own parameter a
    positive Variable `lik_param`, initialised to likelihood.param: the sampled ELBO reads it, fit_q, predict_y,
    predict_log_density and elbo_and_grad use its current value, and fit_hyper learns it with the other
    hyper-parameters.  The likelihood object handed in is never modified; current_likelihood() is the one in use."""

    def setUp(self, X, Y, Z, likelihood, residual="diagonal", eps=None, learn_likelihood=False):
        if learn_likelihood and not getattr(likelihood, "trainable", False):
            raise ValueError("SVGPLik: learn_likelihood=True needs a likelihood with a continuous parameter (got %s)"
                             % type(likelihood).__name__)
        self.N = X.shape[0]
        self.X = hb.param.MinibatchData(X)
        self.Y = hb.param.MinibatchData(Y)
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
        self.u = hb.variationals.Normal(shape=[1, Z.shape[0]], q_shape="fullrank")
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.likelihood = likelihood
        self.learn_likelihood = bool(learn_likelihood)
        if self.learn_likelihood:
            self.lik_param = hb.param.Variable([1], transform=hb.transforms.positive)
            self.lik_param = np.ones(1) * likelihood.param
        self.residual = residual
        self.eps = None if eps is None else hb.param.MinibatchData(eps)  # injected residual noise (parity runs)

    @hb.model.AutoOptimize()
    def ELBO(self):
        f = self.gp.samples(self.X, self.u, q_shape=self.residual, eps=self.eps) * tf.sqrt(self.k_var)
        n = tf.shape(self.X)[0]
        if self.learn_likelihood:
            ll = tf.reduce_sum(self.likelihood.logp(f, tf.transpose(self.Y), param=self.lik_param))
        else:
            ll = tf.reduce_sum(self.likelihood.logp(f, tf.transpose(self.Y)))
        return (self.N / n) * ll - self.KL()

    _gp_elbo_and_grad = "elbo_and_grad"
    _predict = SVGP._predict                      # reads gp, u, k_var and residual only when no noise is asked for
    predict_f = SVGP.predict_f
    predict_f_samples = SVGP.predict_f_samples
    sample_functions = SVGP.sample_functions
    posterior = SVGP.posterior
    suggest_batch = SVGP.suggest_batch

    def predict_y(self, Xnew):
        """Mean and variance [1, n] of a new observation y at Xnew [n, 1]: the likelihood's predictive under the
        Gaussian marginals of predict_f (hb_lik_predict)."""
        mean, var = self.predict_f(Xnew)
        sess, lik = self._session, self.current_likelihood()
        ym, yv = sess.H.lik_predict(lik.lik_id, upload(sess, mean), upload(sess, var), param=lik.param)
        return ym.cpu().numpy(), yv.cpu().numpy()

    def predict_log_density(self, Xnew, Ynew):
        """(per point [1, n], their sum as a float): the predictive log density log E p(y_j | f_j) of observations Ynew
        [n, 1] at Xnew [n, 1] under the Gaussian marginals of predict_f (hb_lik_logdens), for any likelihood -- the
        figure two likelihoods are compared on with held-out data.  Closed form for Gaussian and Laplace, the 20-node
        rule combined by log-sum-exp for the others; the sum is taken in double on the device."""
        mean, var = self.predict_f(Xnew)
        Ynew = np.asarray(Ynew)
        if Ynew.size != mean.size:
            raise ValueError("predict_log_density: Ynew must hold one observation per row of Xnew (got %s for %d rows)"
                             % (Ynew.shape, mean.size))
        sess, lik = self._session, self.current_likelihood()
        yd = upload(sess, Ynew.reshape(mean.shape))
        out, total = sess.H.lik_logdens(lik.lik_id, yd.reshape(-1), upload(sess, mean).reshape(-1),
                                        upload(sess, var).reshape(-1), param=lik.param)
        return out.cpu().numpy().reshape(mean.shape), float(total.cpu()[0])

    def fit_q(self, steps=20, rho=None, tol=1e-8):
        """Fit q(u) at the current z, lengthscales and k_var by natural-gradient steps from the model's CURRENT q, over
        the model's full device-resident X, Y (SparseGP.natgrad_q: per step one marginals pass, the sites, one weighted
        statistics pass and the M^3 tail; no minibatch, no Adam step).  u.q_mu / u.q_sqrt are written as SVGP.fit_q
        writes them for 'fullrank'.  Returns (m [1, M], S [M, M], info) as natgrad_q does.  A full step (rho = 1) from a q
        far from the optimum, such as a freshly initialised one, can overshoot before it settles: info['elbo'] shows it,
        and rho < 1 damps it.  rho=None takes the likelihood's natgrad_rho: 1, except Laplace's 0.25."""
        return self._fit_q(steps, rho, tol)


class SVGPMulticlass(_SVGPNonConjugate):
    """Sparse variational GP classification of C = num_classes classes with the softmax likelihood (hb.likelihoods.Softmax;
    GPflow's Softmax / MultiClass): C latent functions that share z, the lengthscales and k_var, f_c = sqrt(k_var) (u_c A +
    residual), with C independent full-rank blocks q(u_c) = N(m_c, S_c S_c^T) -- one Normal with n_layers = [C].
    y: the labels 0 .. C-1, [N] or [N, 1].  The sampled ELBO trains z, the lengthscales, k_var and q by the minibatch route;
    fit_q() fits q(u) deterministically by natural-gradient steps over the full data (SparseGP.natgrad_q: per step C
    marginals passes, one softmax sites launch, ONE weighted statistics pass that forms A once for all classes, C tails).
    elbo_and_grad() is the exact partial gradient of the fixed-node ELBO fit_q reports, at the current q, with respect to
    z, the lengthscales and k_var (SparseGP.elbo_and_grad_multi); fit_hyper() alternates fit_q steps with Adam steps on it:
    "select z, fit the hyper-parameters, fit q(u)" without a minibatch, as SVGPLik does for one latent function.

    The residual.  SparseGP.samples draws the 'diagonal' residual as ONE number per data point, shared by all latent
    functions of the SparseGP (the reference's semantics), and softmax does not see a shift common to all classes: in this
    model the residual never reaches the likelihood, whatever `residual` is.  So that the closed-form routes describe the
    model the sampled ELBO trains, fit_q, predict_proba, predict and predict_log_density take the moments WITHOUT the
    residual ('neglected') for `residual` 'diagonal' as well; predict_f returns each latent function's own marginal, which
    does carry it.  (SparseGP.natgrad_q itself gives every class its own residual when asked for 'diagonal'; with that
    fit the gradient of this model's sampled ELBO is not zero -- observed on three blobs with 1024 quasi-random nodes: 11 %
    of the entries of d ELBO / d q_mu beyond 4 standard errors, the worst at 8.5, the Monte-Carlo ELBO 7 above the fit's.)"""

    def setUp(self, X, y, Z, num_classes, residual="diagonal", num_nodes=128, seed=None, nodes=None):
        """X [N, d]; y: N integer labels in 0 .. num_classes - 1; Z [M, d].
        residual: 'diagonal' or 'neglected', the residual mode of the sampled ELBO (SparseGP.samples) and of predict_f.
            NOTE: it does NOT reach fit_q, predict_proba, predict or predict_log_density -- those always take the moments
            without the residual, because the sampled model shares one residual draw among the classes and softmax ignores
            a common shift (class docstring).  So with 'diagonal' predict_proba is not the softmax average over predict_f's
            variances; predict_f(Xnew, residual='neglected') returns the moments predict_proba uses.
        num_nodes: the likelihood's fixed nodes, drawn on the device from the MODEL's seed -- `seed=` in the constructor is
            Model's own argument (the session's seed, default settings.runtime.seed) and never reaches setUp, so
            SVGPMulticlass(..., seed=7) seeds the session and the nodes alike; nodes: an [S, C] array to use instead."""
        seed = self._session.seed if seed is None else seed
        self.likelihood = hb.likelihoods.Softmax(num_classes, num_nodes=num_nodes, seed=seed, nodes=nodes)
        C = self.likelihood.num_classes
        lab = np.asarray(y, dtype=np.float64).reshape(-1)
        if lab.shape[0] != X.shape[0] or not (np.all(lab == np.floor(lab)) and lab.min() >= 0 and lab.max() <= C - 1):
            raise ValueError("SVGPMulticlass: y must hold one integer label in 0 .. %d per row of X" % (C - 1))
        self.N, self.num_classes = X.shape[0], C
        self.X = hb.param.MinibatchData(X)
        self.Y = hb.param.MinibatchData(lab.reshape(-1, 1).astype(X.dtype))
        self.Yhot = hb.param.MinibatchData(np.eye(C, dtype=X.dtype)[lab.astype(np.int64)])      # [N, C]
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
        self.u = hb.variationals.Normal(shape=[Z.shape[0]], n_layers=[C], q_shape="fullrank")
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.residual = residual

    @hb.model.AutoOptimize()
    def ELBO(self):
        f = self.gp.samples(self.X, self.u, q_shape=self.residual) * tf.sqrt(self.k_var)      # [C, n]
        n = tf.shape(self.X)[0]
        ll = tf.reduce_sum(self.likelihood.logp(f, tf.transpose(self.Yhot)))
        return (self.N / n) * ll - self.KL()

    def fit_q(self, steps=50, rho=None, tol=1e-8):
        """Fit the C blocks of q(u) at the current z, lengthscales and k_var by natural-gradient steps from the model's
        CURRENT q, over the model's full device-resident X and labels, and write them back.  Returns (m [C, M],
        S [C, M, M], info) as SparseGP.natgrad_q does.  rho=None: the likelihood's natgrad_rho, 0.5 -- a full step
        diverges.  Start from reset_q(), not from the random initial q.  The fit takes the moments without the residual
        (natgrad_q(residual='neglected')) whatever the model's `residual`: see setUp."""
        return self._fit_q(steps, rho, tol)

    def _likelihood_residual(self):
        """The residual mode whose moments the likelihood sees: 'neglected' for 'diagonal' too (the class docstring)."""
        return "neglected" if self.residual == "diagonal" else self.residual

    def predict_f(self, Xnew, residual=None):
        """(mean [C, n], var [C, n]) of the latent functions at Xnew [n, d]: SparseGP.posterior((m_c, S_c)) per class.
        residual=None: the model's own, so var is each function's marginal variance."""
        m, S = self._current_blocks()
        gp, k_var = _part(self, "gp"), _scalar(self, "k_var")
        residual = self.residual if residual is None else residual
        out = [gp.posterior((m[c:c + 1], S[c]), k_var=k_var, residual=residual).predict(Xnew)
               for c in range(self.num_classes)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def _lik_predict(self, Xnew, ynew=None, prob=True):
        mean, var = self.predict_f(Xnew, residual=self._likelihood_residual())
        sess, lik = self._session, _part(self, "likelihood")
        y = None
        if ynew is not None:
            y = np.asarray(ynew, dtype=np.float64).reshape(-1)
            if y.size != mean.shape[1] or not (np.all(y == np.floor(y)) and y.min() >= 0 and y.max() <= self.num_classes - 1):
                raise ValueError("predict_log_density: ynew must hold one label in 0 .. %d per row of Xnew"
                                 % (self.num_classes - 1))
            y = upload(sess, y)
        return sess.H.lik_softmax_predict(upload(sess, mean), upload(sess, var), upload(sess, lik.nodes(), np.float64), y=y,
                                          prob=prob)

    def predict_proba(self, Xnew):
        """Class probabilities [C, n] at Xnew: mean over the likelihood's nodes of softmax(f) under the marginals
        predict_f(Xnew, residual='neglected') returns -- WITHOUT the residual, whatever the model's `residual` (setUp) --
        by hb_lik_softmax_predict."""
        return self._lik_predict(Xnew)[0].cpu().numpy()

    def predict(self, Xnew):
        """The arg-max labels [n] of predict_proba (ties: the lowest class)."""
        return np.argmax(self.predict_proba(Xnew), axis=0)

    def predict_log_density(self, Xnew, ynew):
        """(per point [n], their sum as a float): log mean_s softmax(f_s)_{y_j} of the labels ynew at Xnew, the sum taken
        in double on the device."""
        _, ld, total = self._lik_predict(Xnew, ynew, prob=False)
        return ld.cpu().numpy(), float(total.cpu()[0])


class SVGPHetero(_SVGPNonConjugate):
    """Sparse variational GP regression with input-dependent noise: y ~ N(f(x), exp(g(x) + c)) with the likelihood
    hb.likelihoods.HeteroscedasticGaussian -- two latent functions, the mean f and the log noise variance g, that share z,
    the lengthscales and k_var (f_c = sqrt(k_var) u_c A), with two independent full-rank blocks q(u_f), q(u_g): one Normal
    with n_layers = [2], as SVGPMulticlass holds its classes.  c = log_var_mean is the prior mean of the log variance:
    a Variable `lik_param` (any real number) with learn_likelihood=True, which fit_hyper then learns.
    The sampled ELBO trains everything by the minibatch route; fit_q() fits q(u) deterministically by natural-gradient
    steps over the full data (SparseGP.natgrad_q: per step ONE marginals pass for both latent functions, one sites launch,
    one weighted statistics pass, two tails); elbo_and_grad() is the exact partial gradient of the closed-form ELBO at the
    current q (SparseGP.elbo_and_grad_multi); fit_hyper() alternates the two.

    Limits.  Both latent functions share the lengthscales and k_var (per-latent hyper-parameters are not built).  The
    residual: SparseGP.samples draws ONE residual per data point, shared by all latent functions of the SparseGP; a shared
    draw would couple f and g, which the closed-form routes (independent marginals) cannot describe.  So the sampled ELBO
    and the closed-form routes both use 'neglected', and 'diagonal' is refused."""

    def setUp(self, X, Y, Z, log_var_mean=None, learn_likelihood=True, residual="neglected"):
        """X [N, d]; Y [N, 1] real; Z [M, d].  log_var_mean=None: log(0.1 var Y), a tenth of the data's variance as
        noise."""
        if residual != "neglected":
            raise NotImplementedError(
                "SVGPHetero: residual %r is not covered: SparseGP.samples draws one residual per data point, shared by the "
                "two latent functions, which would couple f and g, while the closed-form routes take independent marginals; "
                "only 'neglected' describes one model on both routes" % (residual,))
        Y = np.asarray(Y)
        if Y.ndim != 2 or Y.shape != (X.shape[0], 1):
            raise ValueError("SVGPHetero: Y must be [N, 1] with one row per row of X (got %s for %d rows)" % (Y.shape, X.shape[0]))
        if log_var_mean is None:
            log_var_mean = float(np.log(0.1 * max(float(np.var(Y)), 1e-12)))
        self.likelihood = hb.likelihoods.HeteroscedasticGaussian(log_var_mean)
        self.N = X.shape[0]
        self.X = hb.param.MinibatchData(X)
        self.Y = hb.param.MinibatchData(Y)
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
        self.u = hb.variationals.Normal(shape=[Z.shape[0]], n_layers=[2], q_shape="fullrank")
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.learn_likelihood = bool(learn_likelihood)
        if self.learn_likelihood:
            self.lik_param = hb.param.Variable([1])
            self.lik_param = np.ones(1) * self.likelihood.param
        self.residual = residual

    @hb.model.AutoOptimize()
    def ELBO(self):
        f = self.gp.samples(self.X, self.u, q_shape=self.residual) * tf.sqrt(self.k_var)      # [2, n]
        n = tf.shape(self.X)[0]
        if self.learn_likelihood:
            ll = tf.reduce_sum(self.likelihood.logp(f, tf.transpose(self.Y), param=self.lik_param))
        else:
            ll = tf.reduce_sum(self.likelihood.logp(f, tf.transpose(self.Y)))
        return (self.N / n) * ll - self.KL()

    def fit_q(self, steps=50, rho=None, tol=1e-8):
        """Fit the two blocks of q(u) at the current z, lengthscales, k_var and c by natural-gradient steps from the model's
        CURRENT q, over the model's full device-resident X, Y, and write them back.  Returns (m [2, M], S [2, M, M], info) as
        SparseGP.natgrad_q does.  rho=None: the likelihood's natgrad_rho, 0.5 -- a full step diverges.  Start from
        reset_q(), not from the random initial q."""
        return self._fit_q(steps, rho, tol)

    def predict_f(self, Xnew):
        """(mean [2, n], var [2, n]) of the two latent functions at Xnew [n, d] (rows: f, g), from ONE pass
        (hb_sgp_predict_multi), scaled by sqrt(k_var) / k_var."""
        m, S = self._current_blocks()
        gp, k_var = _part(self, "gp"), _scalar(self, "k_var")
        mean, var = gp.predict_multi(Xnew, (m, S), residual=self.residual)
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        return (mean * np.sqrt(k_var)).astype(mean.dtype), (var * k_var).astype(var.dtype)

    def predict_y(self, Xnew):
        """Mean and variance [n] of a new observation at Xnew: (mu_f, v_f + exp(mu_g + c + v_g / 2)) (hb_lik_hetgauss_predict)."""
        mean, var = self.predict_f(Xnew)
        sess = self._session
        ym, yv = sess.H.lik_hetgauss_predict(upload(sess, mean), upload(sess, var), param=self.current_likelihood().param)
        return ym.cpu().numpy(), yv.cpu().numpy()

    def predict_noise_variance(self, Xnew):
        """E exp(g + c) = exp(mu_g + c + v_g / 2) [n] at Xnew: the noise variance the model predicts there (predict_y's
        variance without the part of f)."""
        mean, var = self.predict_f(Xnew)
        sess = self._session
        zero = np.zeros_like(var[:1])
        _, yv = sess.H.lik_hetgauss_predict(upload(sess, mean), upload(sess, np.concatenate([zero, var[1:]])),
                                            param=self.current_likelihood().param)
        return yv.cpu().numpy()

    def predict_log_density(self, Xnew, Ynew):
        """(per point [n], their sum as a float): the predictive log density of observations Ynew [n, 1] at Xnew, f
        integrated in closed form and g by the 20-node rule (hb_lik_hetgauss_logdens); the sum is taken in double on the
        device."""
        mean, var = self.predict_f(Xnew)
        Ynew = np.asarray(Ynew)
        if Ynew.size != mean.shape[1]:
            raise ValueError("predict_log_density: Ynew must hold one observation per row of Xnew (got %s for %d rows)"
                             % (Ynew.shape, mean.shape[1]))
        sess = self._session
        out, total = sess.H.lik_hetgauss_logdens(upload(sess, Ynew.reshape(-1)), upload(sess, mean), upload(sess, var),
                                                 param=self.current_likelihood().param)
        return out.cpu().numpy(), float(total.cpu()[0])


class Amortised(hb.model.Model):
    """cfg 4: NeuralNet encoder -> LOCAL Normal -> linear Gaussian decoder."""

    def setUp(self, Y, L=16, H=256, stddev=None):
        Din = Y.shape[1]
        self.Y = hb.param.MinibatchData(Y)
        self.z = hb.variationals.Normal([L], collections=hb.param.graph_key.LOCAL)
        self.enc = hb.nn.NeuralNet([Din, H, 2 * L], stddev=stddev or 1.0 / np.sqrt(Din))
        self.dec = hb.nn.NeuralNet([L, Din], stddev=stddev or 1.0 / np.sqrt(L))
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)

    @hb.model.AutoOptimize()
    def ELBO(self):
        self.z = self.enc(self.Y)
        ll = tf.reduce_sum(hb.densities.gaussian(self.Y, self.dec(self.z), self.var))
        return ll - self.KL()


class DenseGPR(hb.model.Model):
    """Dense variational GP regression, the form of notebooks/GaussianProcess.ipynb:109-148."""

    def setUp(self, X, Y):
        self.X = hb.param.Data(X)
        self.Y = hb.param.Data(Y)
        self.kern = hb.gp.kernels.UnitRBF(np.ones(1))
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.q = hb.variationals.Normal(shape=[X.shape[0], 1], q_shape="fullrank")

    @hb.model.AutoOptimize()
    def ELBO(self):
        f = tf.matmul(self.kern.Cholesky(self.X), self.q) * tf.sqrt(self.k_var)
        return tf.reduce_sum(hb.densities.gaussian(self.Y, f, self.var)) - self.KL()


class ExactGPR(hb.model.Model):
    """Exact GP regression at scale: kern, k_var and var as in SVGP, the posterior from conjugate gradients on the
    matrix-free kernel product (GP.condition) instead of an [N, N] factorisation.  The objective is the log marginal
    likelihood, estimated with its gradient from the same solves (GP.log_marginal_likelihood_and_grad):
        m.fit_hyper(100, lr=0.05);  mean, var = m.predict_y(Xnew);  draws = m.sample_functions(16)
    or set lengthscales, k_var and var by hand and call m.fit().
    Predictions are in data units: mean [P, n] and var [n] of f ~ GP(0, k_var k) given Y = f(X) + N(0, var)."""

    def setUp(self, X, Y):
        self.X = hb.param.Data(X)
        self.Y = hb.param.Data(Y)
        self.gp = hb.gp.GP(kern=hb.gp.kernels.UnitRBF(np.ones(1)))
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.posterior = None

    def fit(self, precond_rank=64, tol=None, max_iter=1000, cache_rank=None):
        """Condition on the model's X, Y at the CURRENT lengthscales, k_var and var and keep the hb.gp.ExactPosterior
        (also returned as self.posterior); hyper-parameters changed afterwards need another fit().  cache_rank: also
        build the posterior's variance cache at that rank (ExactPosterior.build_cache), for predict_f(var='cache') and
        suggest.  Returns self."""
        X, Y, var, k_var = self._closed_form_inputs()
        post = _part(self, "gp").condition(X, Y, var, k_var=k_var, precond_rank=precond_rank, tol=tol, max_iter=max_iter)
        if cache_rank is not None:
            post.build_cache(rank=cache_rank)
        self.posterior = post
        return self

    _closed_form_inputs = SVGP._closed_form_inputs

    def _hyper_variables(self):
        """The Variables the log marginal likelihood depends on, by the names the gradient uses."""
        return dict(lengthscales=_part(_part(_part(self, "gp"), "kern"), "lengthscales"), k_var=_part(self, "k_var"),
                    var=_part(self, "var"))

    def log_marginal_likelihood_and_grad(self, num_probes=16, seed=0, precond_rank=64, tol=None, max_iter=1000, probes=None):
        """(value, grad): the log marginal likelihood of the model's X, Y at the current hyper-parameters and its gradient
        with respect to the RAW (free) parameters, grad = dict(lengthscales, k_var, var) in the shapes of the raw arrays,
        float64 numpy: GP.log_marginal_likelihood_and_grad chained through the transforms' dforward.  A stochastic
        estimate, deterministic given `seed` (or `probes`)."""
        X, Y, var, k_var = self._closed_form_inputs()
        value, gr, _ = _part(self, "gp").log_marginal_likelihood_and_grad(
            X, Y, var, k_var=k_var, precond_rank=precond_rank, tol=tol, max_iter=max_iter, num_probes=num_probes, seed=seed,
            probes=probes)
        return value, _chain_to_raw(self, dict(lengthscales=gr["lengthscales"], k_var=gr["k_var"], var=gr["noise_var"]))

    def log_marginal_likelihood(self, num_probes=16, seed=0, precond_rank=64, tol=None, max_iter=1000, probes=None):
        """The value alone (no pass over the kernel entries)."""
        X, Y, var, k_var = self._closed_form_inputs()
        return _part(self, "gp").log_marginal_likelihood(
            X, Y, var, k_var=k_var, precond_rank=precond_rank, tol=tol, max_iter=max_iter, num_probes=num_probes, seed=seed,
            probes=probes)

    def fit_hyper(self, steps, lr=0.01, num_probes=16, seed=0, precond_rank=64, tol=None):
        """Fit lengthscales, k_var and var: `steps` Adam ASCENT steps on log_marginal_likelihood_and_grad in the raw
        parameters, on the host in float64 (the loop of SVGP.fit_hyper), with the SAME seed at every step -- common random
        numbers, so the function climbed is deterministic -- then fit() at the final parameters.  Each step is one
        lockstep solve of 1 + num_probes rows and one pass over the kernel entries.  Returns the trace of the estimated
        objective, steps + 1 entries: before the first step .. at the final parameters.  hb.gp.NotConverged propagates."""
        evaluate = lambda: self.log_marginal_likelihood_and_grad(num_probes=num_probes, seed=seed, precond_rank=precond_rank,
                                                                 tol=tol)
        trace = _adam_ascent(self, evaluate, steps, lr, True)
        self.fit(precond_rank=precond_rank, tol=tol)
        return trace

    def _posterior(self):
        post = _part(self, "posterior")
        if post is None:
            raise ValueError("ExactGPR: call fit() first")
        return post

    def predict_f(self, Xnew, var=True):
        """(mean [P, n], var [n]) of the latent f at Xnew; the variance costs one solve per 64 points (var=False skips it).
        var='cache': the cached upper bound of the variance instead, from ONE pass over Xnew (fit(cache_rank=...) or
        posterior.build_cache() first) -- tight once the rank covers the data's volume in lengthscale units, loose but
        still an upper bound below that."""
        return self._posterior().predict_f(Xnew, var=var)

    def predict_y(self, Xnew, var=True):
        """predict_f plus the likelihood's variance."""
        return self._posterior().predict_y(Xnew, var=var)

    def suggest(self, Xcand, kind="ei", largest=True, cache_rank=256, steps=0, lr=0.05, bounds=None, **kw):
        """(x_next [d], value, info): the next point of a sequential design -- the row of Xcand [n, d] at which the
        closed-form acquisition `kind` ('ei', 'pi', 'ucb') of the exact posterior is largest, from ONE arg-max pass over
        the candidates (ExactPosterior.argmax; **kw: param, var_floor), however many there are.  The incumbent is
        suggest_batch's: the largest (smallest with largest=False) posterior mean over the training inputs,
        predict_f(X, var=False).  The variance is the cached upper bound, built at cache_rank if the posterior has none.
        info = dict(best, index, cache = the posterior's cache_info).  steps > 0 then refines that candidate by `steps`
        steps of projected gradient ascent on the acquisition's exact input gradient (ExactPosterior.maximise with lr
        and bounds, default the candidates' box): x_next leaves the grid, value is the acquisition there (never below
        the candidate's) and info also holds start_value, the candidate's value, and steps."""
        if int(steps) < 0:
            raise ValueError("suggest: steps >= 0 expected (got %r)" % (steps,))
        post = self._posterior()
        mean, _ = post.predict_f(_part(self, "X"), var=False)
        best = float(mean.max() if largest else mean.min())
        if post.cache_info is None:
            post.build_cache(rank=cache_rank)
        Xd = post._new_points(Xcand)
        idx, value = post.argmax(Xd, kind, best=best, largest=largest, **kw)
        if idx < 0:
            raise ValueError("suggest: no candidate has a comparable acquisition value")
        x_next, info = Xd[idx].cpu().numpy(), dict(best=best, index=idx, cache=dict(post.cache_info))
        if int(steps) > 0:
            xb, ab, _ = post.maximise(Xd, kind, best=best, largest=largest, steps=steps, lr=lr, bounds=bounds, starts=x_next[None],
                                      **kw)
            info.update(start_value=value, steps=int(steps))
            x_next, value = xb[0], ab[0]
        return x_next, value, info

    def sample_functions(self, num_samples, num_features=1024, seed=0, noise=None):
        """num_samples exact posterior function draws as an hb.gp.PathwiseDraws (ExactPosterior.sample_functions); its
        grad, argmax and maximise work as for the sparse models."""
        return self._posterior().sample_functions(num_samples, num_features=num_features, seed=seed, noise=noise)

    def suggest_batch(self, Xcand, q, kind="ei", largest=True, num_samples=64, num_features=1024, seed=0, steps=0, **kw):
        """(X_next [q', d], gains [q'], info) as SVGP.suggest_batch: the exact GP's acquisition -- EI / PI and batches
        from its function draws, with no predictive variance (a solve per 64 points) anywhere.  The incumbent is the
        largest (smallest) posterior mean over the training inputs, predict_f(X, var=False)."""
        mean, _ = self.predict_f(_part(self, "X"), var=False)
        return _suggest_batch(self, mean, Xcand, q, kind, largest, num_samples, num_features, seed, steps, kw)


def svgp_data(N, M, seed=0, domain=None, dtype=np.float64):
    """Synthetic regression set of the BASELINE configs: X ~ U(0, domain),
    Y = sin X + 0.3 eps, Z = linspace(0, domain, M) (spacing 0.5 lengthscales)."""
    rng = np.random.RandomState(seed)
    domain = 0.5 * M if domain is None else domain
    X = rng.uniform(0, domain, (N, 1))
    Y = np.sin(X) + 0.3 * rng.randn(N, 1)
    Z = np.linspace(0, domain, M)[:, None]
    return X.astype(dtype), Y.astype(dtype), Z.astype(dtype)


class ExpertGPR(hb.model.Model):
    """Mixture of two sparse-GP experts with a sparse-GP gate: the sparse form of
    notebooks/Expert_GPR.ipynb:101-160 (three independent GPs with their own kernels;
    f = (sigmoid(f_r) f_s + (1 - sigmoid(f_r)) f_l) * k_var  -- times k_var, not its root,
    as the notebook writes it)."""

    def setUp(self, X, Y, Z, ells=(0.3, 2.0, 1.0), eps=None):
        self.N = X.shape[0]
        self.X = hb.param.MinibatchData(X)
        self.Y = hb.param.MinibatchData(Y)
        self.gp_s = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1) * ells[0]), z=Z)
        self.gp_l = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1) * ells[1]), z=Z)
        self.gp_r = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1) * ells[2]), z=Z)
        M = Z.shape[0]
        self.u_s = hb.variationals.Normal(shape=[1, M])
        self.u_l = hb.variationals.Normal(shape=[1, M])
        self.u_r = hb.variationals.Normal(shape=[1, M])
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.k_var_r = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        # injected residual noise, one column per GP (parity runs)
        self.eps = None if eps is None else hb.param.MinibatchData(eps)

    @hb.model.AutoOptimize()
    def ELBO(self):
        e = self.eps
        es, el, er = (None, None, None) if e is None else (e[:, 0], e[:, 1], e[:, 2])
        f_s = self.gp_s.samples(self.X, self.u_s, eps=es)
        f_l = self.gp_l.samples(self.X, self.u_l, eps=el)
        f_r = self.gp_r.samples(self.X, self.u_r, eps=er) * tf.sqrt(self.k_var_r)
        frac = tf.sigmoid(f_r)
        f = (frac * f_s + (1.0 - frac) * f_l) * self.k_var
        n = tf.shape(self.X)[0]
        ll = tf.reduce_sum(hb.densities.gaussian(tf.transpose(self.Y), f, self.var))
        return (self.N / n) * ll - self.KL()


class ExpertsGPR(hb.model.Model):
    """cfg 5: E sparse-GP experts with E sparse-GP gates (softmax gating; E = 2 with r = g_2 - g_1
    reduces to the sigmoid form of notebooks/Expert_GPR.ipynb:139-147).  The 2E independent GPs
    -- own inducing points, own lengthscale, own q(u) -- are ONE batched SparseGP, so their Gram
    matrices, Cholesky factors and M^2 n contractions run as single expert-batched launches."""

    def setUp(self, X, Y, Z, ells, eps=None):
        E2 = len(ells)
        self.E = E2 // 2
        self.N = X.shape[0]
        self.X = hb.param.MinibatchData(X)
        self.Y = hb.param.MinibatchData(Y)
        M = Z.shape[0]
        z = np.broadcast_to(Z, (E2,) + Z.shape).copy()
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.asarray(ells, dtype=np.float64).reshape(E2, 1)), z=z)
        self.u = hb.variationals.Normal(shape=[E2, 1, M])
        self.k_var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.k_var_r = hb.param.Variable([1], transform=hb.transforms.positive)
        self.var = hb.param.Variable([1], transform=hb.transforms.positive)
        self.eps = None if eps is None else hb.param.MinibatchData(eps)  # [N, 2E] injected residual noise

    @hb.model.AutoOptimize()
    def ELBO(self):
        E = self.E
        eps = None if self.eps is None else tf.transpose(self.eps)        # [2E, n]
        f_all = self.gp.samples(self.X, self.u, eps=eps)                   # [2E, 1, n]
        f_e = f_all[:E, 0, :]                                              # [E, n]
        g_e = f_all[E:, 0, :] * tf.sqrt(self.k_var_r)
        g_max = tf.reduce_max(g_e, 0, keep_dims=True)
        w = tf.exp(g_e - g_max)
        w = w / tf.reduce_sum(w, 0, keep_dims=True)
        f = tf.reduce_sum(w * f_e, 0, keep_dims=True) * self.k_var         # [1, n]
        n = tf.shape(self.X)[0]
        ll = tf.reduce_sum(hb.densities.gaussian(tf.transpose(self.Y), f, self.var))
        return (self.N / n) * ll - self.KL()
