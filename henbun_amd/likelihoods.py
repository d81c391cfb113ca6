"""Factorising likelihoods p(y_j | f_j) for the natural-gradient fit of q(u) (SparseGP.natgrad_q, models.SVGPLik; not
in the reference, which offers the densities only).  Each class carries the id and the parameter the native entries
hb_lik_sites_* / hb_lik_predict_* / hb_lik_param_grad_* / hb_lik_logdens_* take (include/henbun_hip.h, HB_LIK_*) and
`logp(f, y)`, the same log-density as a graph expression built from henbun_amd.densities -- so the sampled ELBO of a model
and its closed-form fit use one likelihood.

    Gaussian(var)                y ~ N(f, var)                                          trainable (var)
    Bernoulli()                  y in {0, 1}, logit link
    Poisson()                    y in {0, 1, ..}, rate exp(f)
    Laplace(scale)               y ~ Laplace(f, scale): regression with outliers        trainable (scale)
    Gamma(shape)                 y > 0, mean exp(f), variance mean^2 / shape            trainable (shape)
    Exponential()                Gamma(1)
    NegativeBinomial(dispersion) y in {0, 1, ..}, mean exp(f), variance mean + mean^2 / dispersion   trainable (dispersion)
    Binomial(total_count)        y successes out of total_count trials, logit link
    Softmax(num_classes)         y in {0, .., C - 1}, p(y = c | f) = softmax(f)_c: C latent functions (num_latent = C),
                                 its own native entries hb_lik_softmax_*, natgrad_rho = 0.5
    HeteroscedasticGaussian(log_var_mean)   y ~ N(f, exp(g + log_var_mean)): two latent functions (num_latent = 2), the
                                 mean f and the log noise variance g; native entries hb_lik_hetgauss_*, natgrad_rho = 0.5;
                                 trainable (log_var_mean, any real number)

All are log-concave in f, which keeps the natural-gradient step positive definite.  `trainable` says that the parameter
is continuous and has a gradient (hb_lik_param_grad_*; HeteroscedasticGaussian: with its sites): SparseGP.elbo_and_grad(lik_grad=True) returns it and
models.SVGPLik(learn_likelihood=True) learns it.  `logp(f, y, param=t)` takes the parameter from the graph tensor t
instead of the stored float, which is how such a model's sampled ELBO sees its Variable.  `natgrad_rho` is the damping
SVGPLik.fit_q and fit_hyper use unless told otherwise: 1 (full steps) except for Laplace."""
from __future__ import annotations

import copy
import math

import numpy as np

from . import densities, tf
from . import graph as G


class Likelihood:
    lik_id = None
    num_latent = 1      # latent functions per data point (Softmax: the number of classes)
    param = 1.0
    trainable = False
    param_name = None
    natgrad_rho = 1.0   # the damping models.SVGPLik.fit_q / fit_hyper take by default

    def _check(self, value):
        raise ValueError("%s has no parameter" % type(self).__name__)

    def with_param(self, value):
        """A copy of this likelihood with the parameter `value` (validated as the constructor validates it)."""
        new = copy.copy(self)
        new.param = self._check(value)
        return new

    def _positive(self, value):
        value = float(value)
        if not value > 0.0:
            raise ValueError("%s: %s must be positive (got %r)" % (type(self).__name__, self.param_name, value))
        return value

    def logp(self, f, y, param=None):
        raise NotImplementedError

    # -- what SparseGP.natgrad_q / elbo_and_grad / elbo_and_grad_multi ask of a likelihood over C = num_latent latent
    # functions.  The defaults below serve every likelihood over ONE (the entries hb_lik_sites / hb_lik_param_grad by
    # lik_id); Softmax and HeteroscedasticGaussian bring their own.
    fused_marginals = False   # True: the C marginals come from ONE hip_ops.sgp_predict_multi (else C calls of sgp_predict)

    def check_targets(self, who, Y):
        """The targets Y must be [N, 1]: the shape of a numpy array or a device tensor, and for a numpy array (the host
        side) the values too, where a likelihood restricts them -- targets already on the device are the caller's duty."""
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise NotImplementedError("%s: one latent function only (Y must be [N, 1], got %s)" % (who, tuple(Y.shape)))

    def device_state(self, sess):
        """What the sites and weights calls need on the device besides the marginals (Softmax: its nodes); built once
        per route, before the first step."""
        return None

    def sites(self, H, state, y, mean, var, mscale, vscale, out):
        """lam, beta [C, N] into out = (lam, beta) at the marginals mean, var [C, N]; returns lsum (float64 [1])."""
        return H.lik_sites(self.lik_id, y, mean, var, param=self.param, mscale=mscale, vscale=vscale, out=out)[2]

    def weights(self, H, state, y, mean, var, mscale, vscale, out, mu, lik_grad=False):
        """The weights of the hyper-parameter gradient at fixed q into out = (w, r), float64 [C, N] views of padded rows;
        returns (lsum, dparam): sum_j l_j and, with lik_grad=True (a trainable likelihood), sum_j dl_j / dparam as a float64
        device tensor [1], else None.  mu = mscale mean, which the caller holds already.  Here w = lam and r = gamma = beta
        - lam mu (Stein's identity), and the parameter gradient is one more launch (hb_lik_param_grad), issued only when
        asked for."""
        lam, r = out
        lsum = self.sites(H, state, y, mean, var, mscale, vscale, out)
        r -= lam * mu
        dparam = None
        if lik_grad:
            dparam = H.lik_param_grad(self.lik_id, y, mean, var, param=self.param, mscale=mscale, vscale=vscale)[1:]
        return lsum, dparam


class Gaussian(Likelihood):
    """y ~ N(f, var)."""

    lik_id = 0
    trainable = True
    param_name = "var"
    _check = Likelihood._positive

    def __init__(self, var):
        self.param = self._check(var)

    def logp(self, f, y, param=None):
        return densities.gaussian(y, f, self.param if param is None else param)


class Bernoulli(Likelihood):
    """y in {0, 1}, p(y = 1 | f) = sigmoid(f)."""

    lik_id = 1

    def logp(self, f, y, param=None):
        return densities.bernoulli(tf.sigmoid(f), y)


class Poisson(Likelihood):
    """y in {0, 1, 2, ..}, rate exp(f)."""

    lik_id = 2

    def logp(self, f, y, param=None):
        return densities.poisson(tf.exp(f), y)


class Laplace(Likelihood):
    """y ~ Laplace(f, scale): log p = -log(2 scale) - |y - f| / scale.  Its sites are closed form.  The curvature site
    lam_j = (2 / scale) N(y_j; mu_j, v_j) is not bounded as v_j falls (the kink), so full natural-gradient steps overshoot:
    on the 3000-point test problem the iteration diverges at rho = 1 and 0.5 and converges at 0.25, the default here."""

    lik_id = 16
    natgrad_rho = 0.25
    trainable = True
    param_name = "scale"
    _check = Likelihood._positive

    def __init__(self, scale):
        self.param = self._check(scale)

    def logp(self, f, y, param=None):
        return densities.laplace(f, self.param if param is None else param, y)


class Gamma(Likelihood):
    """y > 0 with mean exp(f) and the given shape (variance mean^2 / shape): the Gamma density with scale exp(f) / shape.
    y > 0 is the caller's duty: log y is taken as it comes."""

    lik_id = 17
    trainable = True
    param_name = "shape"
    _check = Likelihood._positive

    def __init__(self, shape):
        self.param = self._check(shape)

    def logp(self, f, y, param=None):
        a = G.as_tensor(self.param if param is None else param)
        return densities.gamma(a, G.div(tf.exp(f), a), y)


class Exponential(Gamma):
    """y > 0 with mean exp(f): Gamma(1).  Its shape is fixed, so it is not trainable."""

    trainable = False

    def __init__(self):
        self.param = 1.0

    def _check(self, value):
        raise ValueError("Exponential has no parameter (use Gamma(shape) to learn a shape)")


class NegativeBinomial(Likelihood):
    """y in {0, 1, 2, ..} with mean exp(f) and variance mean + mean^2 / dispersion.  With t = f - log(dispersion):
    log p = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y t - (y + r) softplus(t)."""

    lik_id = 18
    trainable = True
    param_name = "dispersion"
    _check = Likelihood._positive

    def __init__(self, dispersion):
        self.param = self._check(dispersion)

    def logp(self, f, y, param=None):
        r, y = G.as_tensor(self.param if param is None else param), G.as_tensor(y)
        t = G.sub(f, G.unary("LOG", r))
        yr = G.add(y, r)
        const = G.sub(G.sub(G.unary("LGAMMA", yr), G.unary("LGAMMA", r)), G.unary("LGAMMA", G.affine(y, 1.0, 1.0)))
        return G.add(const, G.sub(G.mul(y, t), G.mul(yr, tf.nn.softplus(t))))


class Binomial(Likelihood):
    """y successes out of total_count trials, p(success | f) = sigmoid(f); total_count an integer >= 1 (1: Bernoulli).
    log p = lgamma(n + 1) - lgamma(y + 1) - lgamma(n - y + 1) + y f - n softplus(f)."""

    lik_id = 19
    param_name = "total_count"

    def __init__(self, total_count):
        self.param = self._check(total_count)

    def _check(self, value):
        value = float(value)
        if not (value >= 1.0 and value == math.floor(value)):
            raise ValueError("Binomial: total_count must be an integer >= 1 (got %r)" % (value,))
        return value

    def logp(self, f, y, param=None):
        n, y = self.param, G.as_tensor(y)
        const = G.affine(G.add(G.unary("LGAMMA", G.affine(y, 1.0, 1.0)), G.unary("LGAMMA", G.affine(y, -1.0, n + 1.0))),
                         -1.0, math.lgamma(n + 1.0))
        return G.add(const, G.sub(G.mul(y, f), G.affine(tf.nn.softplus(f), n)))


class Softmax(Likelihood):
    """Multi-class classification: y in {0, .., C - 1}, p(y = c | f) = softmax(f)_c over num_classes = C latent functions
    (the only likelihood here with num_latent > 1; SparseGP.natgrad_q fits C independent q(u_c), models.SVGPMulticlass is
    the model).  E log softmax(f)_y under C independent Gaussian marginals is a C-dimensional expectation: it is taken over
    num_nodes standard-normal draws eps [S, C] shared by all points and fixed for the life of the object (a fixed-node
    sum, so a fit is deterministic).  `nodes()` returns them: drawn on the device from hip_ops.Rng(seed) on first use, or
    the array handed in as `nodes` ([S, C], any S in 1 .. 1024).  128 nodes is a default, not a measurement.  The curvature
    site is Price's form mean_s p (1 - p) >= 0, which keeps every Lambda_c positive definite.  A full natural-gradient step
    does not settle with it (tests/softmax_ref.py on blobs on a ring, k_var = 4: three classes end in a period-2 cycle
    between ELBO -51 and -140, ten classes diverge past -40000 within 10 steps); rho = 0.5 converges, hence natgrad_rho."""

    lik_id = 32
    natgrad_rho = 0.5
    MAX_CLASSES, MAX_NODES = 64, 1024

    def __init__(self, num_classes, num_nodes=128, seed=0, nodes=None):
        C = int(num_classes)
        if C != num_classes or not 2 <= C <= self.MAX_CLASSES:
            raise ValueError("Softmax: num_classes must be an integer in 2 .. %d (got %r)" % (self.MAX_CLASSES, num_classes))
        self.num_classes = self.num_latent = C
        self.seed = int(seed)
        self._nodes = None
        if nodes is not None:
            nodes = np.array(nodes, dtype=np.float64)
            if nodes.ndim != 2 or nodes.shape[1] != C or not 1 <= nodes.shape[0] <= self.MAX_NODES or not np.all(np.isfinite(nodes)):
                raise ValueError("Softmax: nodes must be a finite [S, %d] array with 1 <= S <= %d (got shape %s)"
                                 % (C, self.MAX_NODES, nodes.shape))
            self._nodes, num_nodes = nodes, nodes.shape[0]
        S = int(num_nodes)
        if S != num_nodes or not 1 <= S <= self.MAX_NODES:
            raise ValueError("Softmax: num_nodes must be an integer in 1 .. %d (got %r)" % (self.MAX_NODES, num_nodes))
        self.num_nodes = S

    def _check(self, value):
        raise ValueError("Softmax has no parameter")

    def nodes(self):
        """The [S, C] float64 standard-normal nodes (numpy): the injected array, or drawn once from hip_ops.Rng(seed)."""
        if self._nodes is None:
            import torch

            from . import hip_ops

            self._nodes = hip_ops.Rng(self.seed).normal((self.num_nodes, self.num_classes), dtype=torch.float64).cpu().numpy()
        return self._nodes

    def check_targets(self, who, Y):
        C = self.num_classes
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise ValueError("%s: Y must hold the labels as [N, 1], got %s" % (who, tuple(Y.shape)))
        if isinstance(Y, np.ndarray) and not (np.all(Y == np.floor(Y)) and Y.size and Y.min() >= 0 and Y.max() <= C - 1):
            raise ValueError("%s: the labels must be integers in 0 .. %d" % (who, C - 1))

    def device_state(self, sess):
        from .gp import _host

        return _host.upload(sess, self.nodes(), np.float64)

    def sites(self, H, state, y, mean, var, mscale, vscale, out):
        return H.lik_softmax_sites(y, mean, var, state, mscale=mscale, vscale=vscale, out=out)[2]

    def weights(self, H, state, y, mean, var, mscale, vscale, out, mu, lik_grad=False):
        return H.lik_softmax_grad(y, mean, var, state, mscale=mscale, vscale=vscale, out=out)[2], None

    def logp(self, f, y, param=None):
        """log softmax(f)_y as a graph expression [1, n]: f [C, n], y the ONE-HOT labels [C, n];
        sum_c y_c f_c - logsumexp_c f, the log-sum-exp shifted by the maximum over classes."""
        f, y = G.as_tensor(f), G.as_tensor(y)
        top = tf.reduce_max(f, 0, keep_dims=True)
        lse = G.add(top, tf.log(tf.reduce_sum(tf.exp(G.sub(f, top)), 0, keep_dims=True)))
        return G.sub(tf.reduce_sum(G.mul(y, f), 0, keep_dims=True), lse)


class HeteroscedasticGaussian(Likelihood):
    """Regression with input-dependent noise: y ~ N(f, exp(g + c)) over TWO latent functions (num_latent = 2), the mean f
    and the log noise variance g, with c = log_var_mean the prior mean of the log variance (any real number; trainable).
    SparseGP.natgrad_q fits two independent q(u_f), q(u_g); models.SVGPHetero is the model.  Under independent Gaussian
    marginals the expected log density, both sites and every derivative are closed forms (include/henbun_hip.h,
    hb_lik_hetgauss_*), with s = (y - mu_f)^2 + v_f and e = exp(-mu_g - c + v_g / 2):
        l = -1/2 log 2 pi - 1/2 (mu_g + c) - 1/2 s e,   lam_f = e,   lam_g = 1/2 s e   (both >= 0, and lam = -2 dl/dv exactly)
    so the weights of the hyper-parameter gradient are the sites themselves, and dl/dc = dl/dmu_g.
    Full natural-gradient steps overshoot (tests/hetgauss_ref.py on 300 .. 400 points with a sigmoid noise level, M = 24:
    at rho = 1 the second step throws the ELBO from -281 to -18623, six times below the prior's value); at rho = 0.5 it
    rose at every step and settled to 1e-6 relative in 14 .. 22 steps, hence natgrad_rho."""

    lik_id = 33
    num_latent = 2
    natgrad_rho = 0.5
    trainable = True
    param_name = "log_var_mean"
    fused_marginals = True

    def __init__(self, log_var_mean=0.0):
        self.param = self._check(log_var_mean)

    def _check(self, value):
        value = float(value)
        if not math.isfinite(value):
            raise ValueError("HeteroscedasticGaussian: log_var_mean must be finite (got %r)" % (value,))
        return value

    def check_targets(self, who, Y):
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise ValueError("%s: Y must hold the observations as [N, 1], got %s" % (who, tuple(Y.shape)))
        if isinstance(Y, np.ndarray) and not (Y.size and np.all(np.isfinite(Y))):
            raise ValueError("%s: the observations must be finite numbers" % who)

    def sites(self, H, state, y, mean, var, mscale, vscale, out):
        return H.lik_hetgauss_sites(y, mean, var, param=self.param, mscale=mscale, vscale=vscale, out=out)[3]

    def weights(self, H, state, y, mean, var, mscale, vscale, out, mu, lik_grad=False):
        # w = lam and r = dl/dmu from the one launch (dparam = sum_j r_gj comes with it, asked for or not); the entry keeps
        # one row stride for inputs and outputs, so the (float64, per chunk) results are copied into the padded rows
        lam, _, r, lsum = H.lik_hetgauss_sites(y, mean, var, param=self.param, mscale=mscale, vscale=vscale, grad=True)
        out[0].copy_(lam)
        out[1].copy_(r)
        return lsum, r[1].sum().reshape(1)

    def logp(self, f, y, param=None):
        """log N(y; f_0, exp(f_1 + c)) as a graph expression [1, n]: f [2, n] (rows: the mean, the log variance), y [1, n]."""
        f, y = G.as_tensor(f), G.as_tensor(y)
        c = G.as_tensor(self.param if param is None else param)
        lv = G.add(tf.slice(f, [1, 0], [1, -1]), c)
        d = G.sub(y, tf.slice(f, [0, 0], [1, -1]))
        return G.affine(G.add(lv, G.mul(G.mul(d, d), tf.exp(G.affine(lv, -1.0)))), -0.5, -0.5 * math.log(2.0 * math.pi))
