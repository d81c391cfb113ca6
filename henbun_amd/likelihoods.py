"""Factorising likelihoods p(y_j | f_j) for the natural-gradient fit of q(u) (SparseGP.natgrad_q, models.SVGPLik; not
in the reference, which offers the densities only).  Each class carries the id and the parameter the native entries
hb_lik_sites_* / hb_lik_predict_* take (include/henbun_hip.h, HB_LIK_*) and `logp(f, y)`, the same log-density as a graph
expression built from henbun_amd.densities -- so the sampled ELBO of a model and its closed-form fit use one likelihood."""
from __future__ import annotations

from . import densities, tf


class Likelihood:
    lik_id = None
    param = 1.0

    def logp(self, f, y):
        raise NotImplementedError


class Gaussian(Likelihood):
    """y ~ N(f, var)."""

    lik_id = 0

    def __init__(self, var):
        var = float(var)
        if not var > 0.0:
            raise ValueError("Gaussian: var must be positive (got %r)" % (var,))
        self.param = var

    def logp(self, f, y):
        return densities.gaussian(y, f, self.param)


class Bernoulli(Likelihood):
    """y in {0, 1}, p(y = 1 | f) = sigmoid(f)."""

    lik_id = 1

    def logp(self, f, y):
        return densities.bernoulli(tf.sigmoid(f), y)


class Poisson(Likelihood):
    """y in {0, 1, 2, ..}, rate exp(f)."""

    lik_id = 2

    def logp(self, f, y):
        return densities.poisson(tf.exp(f), y)
