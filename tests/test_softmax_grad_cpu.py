"""Hyper-parameter gradient of the multi-class ELBO at fixed q(u_c) on the host: the numpy restatement the GPU tests lean on
(tests/softmax_grad_ref.py) against torch.autograd of the fixed-node sum itself, Price's lam shown NOT to be that
derivative, the refusals of SparseGP.elbo_and_grad_multi without a device, and the new C entries' argument checks (which
run before any launch).  No HIP kernel runs here.

The restatement tests pin the REFERENCE, not the library: they would pass without the feature.  The refusal and C ABI
tests, and everything in tests/test_softmax_grad_gpu.py, need it.

Bound of restatement against autograd: two float64 evaluations of the same function, 1e-10 x the cancelling scale
max|streamed part| + max|K(z, z) part| of the class sums (k_var: 1e-10 x the sum of its absolute terms) -- the floor the
GPU bounds of test_elbo_grad_gpu.py use.  Observed: <= 2.6e-13 of the largest entry."""
import os

import numpy as np
import pytest

import henbun_amd as hb
import softmax_grad_ref as MG
import softmax_ref as F

JITTER = 1e-6
K_VAR = 4.0


def _errors(r, a):
    """(name, |restatement - autograd|, cancelling scale, largest entry) per gradient."""
    return [("z", np.abs(r["z"] - a["z"]).max(), np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max(), np.abs(a["z"]).max()),
            ("lengthscales", np.abs(r["lengthscales"] - a["lengthscales"]).max(),
             np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max(), np.abs(a["lengthscales"]).max()),
            ("k_var", abs(r["k_var"] - a["k_var"]), r["k_var_abs"], abs(a["k_var"]))]


@pytest.mark.parametrize("fitted", [False, True])
@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
@pytest.mark.parametrize("C", [3, 5])
def test_restatement_is_the_autograd_of_the_node_sum_and_prices_lam_is_not(C, residual, fitted):
    """ring(C, 300, 16, 128), k_var = 4, at a random full-rank q and at the q of the natural-gradient fit: the class sum of
    grad_from_weights at the reparameterised weights reproduces torch.autograd of the fixed-node value within 1e-10 x the
    cancelling scale in z, the lengthscale and k_var, and the value to 1e-12.  With Price's lam = mean_s p (1 - p) in place
    of w the same formula misses that bound in z and the lengthscale: lam is the derivative of the exact expectation, not
    of the node sum -- which is why the gradient has weights of its own.
    Observed: restatement <= 2.6e-13 of the largest entry in all 8 cases (<= 1e-4 of the bound); Price's lam off by
    1.6e-3 .. 0.17 of the largest entry in z, 1.8e-3 .. 0.17 in the lengthscale, 1.1e-2 .. 3.1 in k_var."""
    X, y, Z, eps = F.ring(C, 300, 16, 128, 1)
    ell = np.ones(1)
    if fitted:
        m, S, info = F.natgrad(X, y, Z, ell, JITTER, C, eps, k_var=K_VAR, residual=residual, steps=60, rho=0.5, tol=1e-10)
    else:
        m, S = MG.q_case(C, 16, seed=C)
    r = MG.elbo_and_grad(X, y, Z, ell, JITTER, eps, m, S, K_VAR, residual)
    a = MG.elbo_autograd(X, y, Z, ell, JITTER, eps, m, S, K_VAR, residual)
    p = MG.elbo_and_grad(X, y, Z, ell, JITTER, eps, m, S, K_VAR, residual, price=True)
    assert (p["w"] >= 0).all() and not np.array_equal(p["w"], r["w"])    # Price's are never negative; w may be
    print("C=%d %s fitted=%s: value %.9f autograd %.9f" % (C, residual, fitted, r["value"], a["value"]))
    assert abs(r["value"] - a["value"]) <= 1e-12 * abs(a["value"])
    missed = {}
    for (name, err, scale, size), (_, perr, _, _) in zip(_errors(r, a), _errors(p, a)):
        print("   %-12s restatement %.3e (%.2e of the largest entry %.3e), bound %.3e; with Price's lam %.3e (%.2e)"
              % (name, err, err / size, size, 1e-10 * scale, perr, perr / size))
        assert err <= 1e-10 * scale, name
        missed[name] = perr > 1e-10 * scale
    assert missed["z"] and missed["lengthscales"]


def test_weights_are_the_derivatives_of_the_node_sum_point_by_point():
    """w = -2 dl/dv and r = dl/dmu of softmax_grad_ref.weights against central differences of l in mu and v at v in
    [0.05, 3] (h = 1e-5: truncation 1e-10, rounding 1e-11 of l); where v = 0, w is Price's p (1 - p) at mu."""
    rng = np.random.RandomState(0)
    C, N, S, h = 4, 40, 64, 1e-5
    mu, v = 2.0 * rng.randn(C, N), rng.uniform(0.05, 3.0, (C, N))
    y, nodes = rng.randint(0, C, N), rng.randn(S, C)
    l, w, r, a, lam = MG.weights(y, mu, v, nodes)
    for c in range(C):
        e = np.zeros((C, 1))
        e[c] = h
        dmu = (MG.weights(y, mu + e, v, nodes)[0] - MG.weights(y, mu - e, v, nodes)[0]) / (2 * h)
        dv = (MG.weights(y, mu, v + e, nodes)[0] - MG.weights(y, mu, v - e, nodes)[0]) / (2 * h)
        assert np.abs(dmu - r[c]).max() <= 1e-8 and np.abs(-2.0 * dv - w[c]).max() <= 1e-7 * (1.0 + a[c].max())
    v[:, ::3] = 0.0
    _, w0, _, _, lam0 = MG.weights(y, mu, v, nodes)
    p0 = np.exp(F.log_softmax(mu))
    assert np.array_equal(w0[:, ::3], lam0[:, ::3]) and np.abs(w0[:, ::3] - (p0 * (1 - p0))[:, ::3]).max() <= 1e-15


# ---------------------------------------------------------------- refusals without a device
class _Holder(hb.model.Model):
    def setUp(self, gp):
        self.gp = gp


def test_elbo_and_grad_multi_refuses_before_the_session_is_touched():
    lik = hb.likelihoods.Softmax(3, nodes=np.zeros((2, 3)))
    X, Y, M = np.zeros((5, 2)), np.zeros((5, 1)), 4
    Z = np.linspace(0, 1, 2 * M).reshape(M, 2)
    q = (np.zeros((3, M)), np.stack([np.eye(M)] * 3))
    m = _Holder(gp=hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z))
    with pytest.raises(ValueError, match="use elbo_and_grad"):
        m.gp.elbo_and_grad_multi(X, Y, hb.likelihoods.Bernoulli(), q)
    with pytest.raises(TypeError):
        m.gp.elbo_and_grad_multi(X, Y, "softmax", q)
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.elbo_and_grad_multi(X, Y, lik, q, residual="fullrank")
    with pytest.raises(ValueError, match="residual"):
        m.gp.elbo_and_grad_multi(X, Y, lik, q, residual="other")
    with pytest.raises(NotImplementedError, match="mean-field"):
        m.gp.elbo_and_grad_multi(X, Y, lik, (np.zeros((3, M)), np.ones((3, M))))
    with pytest.raises(ValueError, match=r"q = \(m \[3, M\]"):
        m.gp.elbo_and_grad_multi(X, Y, lik, (np.zeros((1, M)), np.eye(M)))       # the single-latent shape
    with pytest.raises(ValueError, match=r"q = \(m \[3, 4\]"):
        m.gp.elbo_and_grad_multi(X, Y, lik, (np.zeros((3, 5)), np.stack([np.eye(5)] * 3)))   # M of another z
    with pytest.raises(ValueError, match="got None"):
        m.gp.elbo_and_grad_multi(X, Y, lik, None)
    with pytest.raises(ValueError, match="labels"):
        m.gp.elbo_and_grad_multi(X, Y + 3.0, lik, q)
    with pytest.raises(ValueError, match="labels"):
        m.gp.elbo_and_grad_multi(X, np.zeros((5, 3)), lik, q)
    with pytest.raises(ValueError, match="k_var"):
        m.gp.elbo_and_grad_multi(X, Y, lik, q, k_var=0.0)
    with pytest.raises(NotImplementedError, match="one latent function"):     # the single-latent route still refuses
        m.gp.elbo_and_grad(X, Y, lik, q)
    assert not m._session._ready                                           # none of this opened the device
    alone = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
    with pytest.raises(ValueError, match="part of a Model"):
        alone.elbo_and_grad_multi(X, Y, lik, q)


# ---------------------------------------------------------------- C ABI
NEW = ("hb_lik_softmax_grad_f32", "hb_lik_softmax_grad_f64")


def test_new_symbols_are_declared_exported_and_bound():
    from henbun_amd import _lib

    names, lib = _lib.declared_symbols(), _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in NEW:
        assert n in names and n + "(" in header and lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(C=1), "classes"), (dict(C=65), "classes"), (dict(S=0), "nodes"), (dict(S=1025), "nodes"), (dict(N=-1), "negative N"),
    (dict(vscale=-1.0), "vscale"), (dict(lsum=None), "NULL output"), (dict(ws=None), "NULL output"), (dict(ldo=99), "ldo"),
    (dict(w=None), "NULL pointer"), (dict(r=None), "NULL pointer"), (dict(y=None), "NULL pointer"),
    (dict(nodes=None), "NULL pointer"),
])
def test_lik_softmax_grad_validates_before_any_launch(suffix, bad, word):
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(y=1, mean=1, var=1, mscale=1.0, vscale=1.0, nodes=1, S=8, w=1, r=1, ldo=100, lsum=1, N=100, C=3, ws=1)
    a.update(bad)
    rc = lib.raw("hb_lik_softmax_grad" + suffix)(a["y"], a["mean"], a["var"], a["mscale"], a["vscale"], a["nodes"], a["S"],
                                                 a["w"], a["r"], a["ldo"], a["lsum"], a["N"], a["C"], a["ws"], None)
    assert rc < 0 and word in lib.last_error() and "hb_lik_softmax_grad" in lib.last_error()
