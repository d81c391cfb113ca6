"""The public face of the three models over non-conjugate likelihoods (models.SVGPLik, SVGPMulticlass, SVGPHetero), without
a device: every public method each class had before the deterministic routes moved into one private base class is still
there with the same signature, and the shared routes are inherited, not copied from class to class."""
import inspect

import pytest

from henbun_amd import models
from henbun_amd.models import SVGPHetero, SVGPLik, SVGPMulticlass

FIT_HYPER = "(self, steps, lr=0.01, train_z=True, q_steps=5, rho=None)"
PUBLIC = {
    SVGPLik: [
        ("setUp", "(self, X, Y, Z, likelihood, residual='diagonal', eps=None, learn_likelihood=False)"),
        ("ELBO", "(self)"),
        ("current_likelihood", "(self)"),
        ("elbo_and_grad", "(self)"),
        ("fit_hyper", FIT_HYPER),
        ("fit_q", "(self, steps=20, rho=None, tol=1e-08)"),
        ("posterior", "(self)"),
        ("predict_f", "(self, Xnew, full_cov=False)"),
        ("predict_f_samples", "(self, Xnew, num_samples)"),
        ("predict_log_density", "(self, Xnew, Ynew)"),
        ("predict_y", "(self, Xnew)"),
        ("reset_q", "(self)"),
        ("sample_functions", "(self, num_samples, num_features=1024, seed=0, noise=None)"),
        ("select_inducing", "(self, threshold=None)"),
        ("suggest_batch", "(self, Xcand, q, kind='ei', largest=True, num_samples=64, num_features=1024, seed=0, steps=0, **kw)"),
    ],
    SVGPMulticlass: [
        ("setUp", "(self, X, y, Z, num_classes, residual='diagonal', num_nodes=128, seed=None, nodes=None)"),
        ("ELBO", "(self)"),
        ("elbo_and_grad", "(self)"),
        ("fit_hyper", FIT_HYPER),
        ("fit_q", "(self, steps=50, rho=None, tol=1e-08)"),
        ("predict", "(self, Xnew)"),
        ("predict_f", "(self, Xnew, residual=None)"),
        ("predict_log_density", "(self, Xnew, ynew)"),
        ("predict_proba", "(self, Xnew)"),
        ("reset_q", "(self)"),
        ("select_inducing", "(self, threshold=None)"),
    ],
    SVGPHetero: [
        ("setUp", "(self, X, Y, Z, log_var_mean=None, learn_likelihood=True, residual='neglected')"),
        ("ELBO", "(self)"),
        ("current_likelihood", "(self)"),
        ("elbo_and_grad", "(self)"),
        ("fit_hyper", FIT_HYPER),
        ("fit_q", "(self, steps=50, rho=None, tol=1e-08)"),
        ("predict_f", "(self, Xnew)"),
        ("predict_log_density", "(self, Xnew, Ynew)"),
        ("predict_noise_variance", "(self, Xnew)"),
        ("predict_y", "(self, Xnew)"),
        ("reset_q", "(self)"),
        ("select_inducing", "(self, threshold=None)"),
    ],
}
SHARED = ("fit_hyper", "reset_q", "elbo_and_grad", "_hyper_variables", "current_likelihood")


@pytest.mark.parametrize("cls", list(PUBLIC), ids=lambda c: c.__name__)
def test_public_methods_keep_their_signatures(cls):
    for name, sig in PUBLIC[cls]:
        assert callable(getattr(cls, name, None)), name
        assert str(inspect.signature(getattr(cls, name))) == sig, name


@pytest.mark.parametrize("cls", list(PUBLIC), ids=lambda c: c.__name__)
def test_shared_routes_resolve_through_the_mro(cls):
    """One definition of each shared route, found on a common base: none of the three carries a copy (or a borrowed
    class attribute) of its own."""
    for name in SHARED:
        assert name not in cls.__dict__, name
        owners = [k for k in cls.__mro__ if name in k.__dict__]
        assert owners and owners[0] is not cls and issubclass(cls, owners[0]), name
        assert getattr(cls, name) is getattr(owners[0], name)
    assert len({inspect.getattr_static(c, name) for c in PUBLIC for name in SHARED}) == len(SHARED)
    assert "num_classes" not in inspect.getsource(SVGPHetero)
    assert issubclass(cls, models._SVGPNonConjugate) and "setUp" in cls.__dict__ and "ELBO" in cls.__dict__
