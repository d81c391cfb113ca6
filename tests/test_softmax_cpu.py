"""Multi-class classification with the softmax likelihood, without a device: the numpy restatement tests/softmax_ref.py
against the figures its design was checked with, the host-side checks of likelihoods.Softmax, its graph log-density on
the CPU graph oracle, and the refusals SparseGP.natgrad_q / elbo_and_grad decide before a session is touched."""
import numpy as np
import pytest

import henbun_amd as hb
from henbun_amd import graph as G

import softmax_ref as F

_RUNS = {}


def _run(C, k_var, rho, steps, seed=0):
    """The ring problem (N = 600, M = 32, ell = 1, jitter 1e-6, S = 128) from the prior, computed once per setting."""
    key = (C, k_var, rho, steps, seed)
    if key not in _RUNS:
        X, y, Z, eps = F.ring(C, 600, 32, 128, seed)
        _RUNS[key] = (X, y, Z, eps) + F.natgrad(X, y, Z, np.ones(1), 1e-6, C, eps, k_var=k_var, steps=steps, rho=rho, tol=0.0)
    return _RUNS[key]


def test_restatement_reproduces_the_design_figures_at_half_steps():
    """C = 3, k_var = 4, seed 0, rho = 0.5: the ELBO is -58.08 / -35.48 / -35.1658 at steps 1 / 5 / 40 to the printed
    digits, settled to 6 digits by step 20; the fixed-point residual at step 40 is <= 3e-5 and the training accuracy 1.0."""
    X, y, Z, eps, m, S, info = _run(3, 4.0, 0.5, 40)
    e = info["elbo"]
    print("elbo[1, 5, 20, 40] = %.4f %.4f %.6f %.6f, residual[40] = %.2e" % (e[1], e[5], e[20], e[40], info["residual"][40]))
    assert "%.2f" % e[1] == "-58.08" and "%.2f" % e[5] == "-35.48" and "%.4f" % e[40] == "-35.1658"
    assert "%.4f" % e[20] == "%.4f" % e[40]
    assert info["residual"][40] <= 3e-5
    A = F.R.A_of(F.R.chol_factor(Z, np.ones(1), 1e-6)[1], Z, X, np.ones(1))
    prob, _ = F.predict(*F.marginals(m, S, A, 4.0), eps)
    assert np.mean(np.argmax(prob, 0) == y) == 1.0


def test_full_steps_do_not_settle():
    """rho = 1.  On the ten-class ring (k_var = 4, seed 0) the iteration diverges: the ELBO at step 10 is below -1000
    (-655, -1865, -5966 at steps 1 .. 3, -41640 at step 10).  On the three-class ring of the test above it does not
    diverge but never settles either: it falls into a period-2 cycle (-74.4, -609.6, -63.5, .. then -51.3 / -140.0
    alternating), so the ELBO at step 10 is -140.0, not below -1000.  What is asserted for three classes is what the
    restatement shows: steps 9 and 10 still differ by more than 50, steps 8 and 10 by less than 1, while rho = 0.5 has
    settled to 1e-3 by then."""
    e10 = _run(10, 4.0, 1.0, 10)[6]["elbo"]
    e3 = _run(3, 4.0, 1.0, 10)[6]["elbo"]
    half = _run(3, 4.0, 0.5, 40)[6]["elbo"]
    print("rho = 1: C = 10 elbo", np.round(e10, 1), "\n         C = 3 elbo", np.round(e3, 1))
    assert e10[10] < -1000.0
    assert abs(e3[10] - e3[9]) > 50.0 and abs(e3[10] - e3[8]) < 1.0
    assert abs(half[10] - half[9]) < 1e-3


@pytest.mark.parametrize("C", [2, 3, 10, 64])
def test_site_identities(C):
    """lam >= 0, |sum_c g_c| <= 1e-14 and prob sums to 1 (1e-14), on means up to +-40 and variances from exact 0 to 50;
    with var = 0 the sites are the closed forms g = onehot - softmax(mu), lam = p (1 - p) and l = log softmax(mu)_y."""
    rng = np.random.RandomState(C)
    N, S = 50, 16
    mu = rng.randn(C, N) * rng.choice([0.5, 5.0, 40.0], size=(1, N))
    v = np.exp(rng.uniform(-6, np.log(50.0), (C, N)))
    v[:, ::5] = 0.0
    v[0, 1] = 50.0
    y = rng.randint(0, C, N)
    y[:2] = (0, C - 1)
    nodes = rng.randn(S, C)
    l, lam, beta, g = F.sites(y, mu, v, nodes)
    prob, ld = F.predict(mu, v, nodes, y)
    assert np.all(lam >= 0.0) and np.all(np.isfinite(beta)) and np.all(l <= 0.0)
    assert np.abs(g.sum(0)).max() <= 1e-14
    assert np.abs(prob.sum(0) - 1.0).max() <= 1e-14
    assert np.all(ld >= l - 1e-12)                                     # Jensen: log E p >= E log p
    z = v.sum(0) == 0.0
    p0 = np.exp(F.log_softmax(mu[:, z]))
    hot = (np.arange(C)[:, None] == y[None, z]).astype(np.float64)
    assert np.abs(g[:, z] - (hot - p0)).max() <= 1e-15 and np.abs(lam[:, z] - p0 * (1 - p0)).max() <= 1e-15
    assert np.abs(prob[:, z] - p0).max() <= 1e-15
    assert np.abs(l[z] - (hot * F.log_softmax(mu[:, z])).sum(0)).max() <= 1e-13 * 80


def _naive(y, mu, v, nodes):
    """(l, lam, g, prob, logdens) from the textbook softmax exp(f - max) / sum, 1 - p by subtraction, log of the mean: no
    line shared with softmax_ref.softmax_parts."""
    C, N = mu.shape
    f = mu.T[:, None, :] + np.sqrt(v).T[:, None, :] * nodes[None]                    # [N, S, C]
    e = np.exp(f - f.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    hot = np.zeros((N, 1, C))
    hot[np.arange(N), 0, y] = 1.0
    py = (p * hot).sum(-1)                                                            # [N, S]
    return np.log(py).mean(1), (p * (1 - p)).mean(1).T, (hot - p).mean(1).T, p.mean(1).T, np.log(py.mean(1))


@pytest.mark.parametrize("C", [2, 3, 10, 64])
def test_restatement_against_a_naive_softmax_where_that_is_accurate(C):
    """softmax_parts is written the way the device forms a softmax (first maximal class, `rest`, log1p, the branch at a
    mean p above 1/2), so an error in that formulation would be in both.  Here it is held to the textbook form on inputs
    where the textbook form is accurate in the sense each bound states: |mu| <= 3, v <= 4 and |nodes| <= 3 keep |f| <= 9,
    so every p is above e^-18 / 64 and p, log p carry a relative error of a few ulp (1e-13 relative for prob, 1e-13 absolute
    for l and the log density, |log p| <= 23); 1 - p by subtraction is wrong by up to an ulp of 1 ABSOLUTELY, so lam is held
    to 1e-15 absolute plus 1e-13 relative and g to 1e-14 absolute."""
    rng = np.random.RandomState(10 + C)
    N, S = 40, 32
    mu, v = rng.uniform(-3, 3, (C, N)), np.exp(rng.uniform(-6, np.log(4.0), (C, N)))
    v[:, ::7] = 0.0
    y = rng.randint(0, C, N)
    nodes = np.clip(rng.randn(S, C), -3, 3)
    l, lam, beta, g = F.sites(y, mu, v, nodes)
    prob, ld = F.predict(mu, v, nodes, y)
    nl, nlam, ng, nprob, nld = _naive(y, mu, v, nodes)
    assert np.all(np.abs(lam - nlam) <= 1e-15 + 1e-13 * nlam) and np.abs(prob / nprob - 1).max() <= 1e-13
    assert np.abs(g - ng).max() <= 1e-14 and np.abs(beta - (ng + nlam * mu)).max() <= 1e-13
    assert np.abs(l - nl).max() <= 1e-13 and np.abs(ld - nld).max() <= 1e-13


def test_softmax_validates_its_arguments():
    L = hb.likelihoods
    lik = L.Softmax(3)
    assert (lik.lik_id, lik.num_latent, lik.num_classes, lik.num_nodes, lik.natgrad_rho) == (32, 3, 3, 128, 0.5)
    from henbun_amd import hip_ops

    assert hip_ops.LIK_SOFTMAX == 32 and L.Likelihood.num_latent == 1 and L.Bernoulli().num_latent == 1
    for bad in (1, 65, 2.5, 0):
        with pytest.raises(ValueError, match="num_classes"):
            L.Softmax(bad)
    for bad in (0, 1025, 7.5):
        with pytest.raises(ValueError, match="num_nodes"):
            L.Softmax(3, num_nodes=bad)
    for bad in (np.zeros((4, 2)), np.zeros(3), np.zeros((0, 3)), np.zeros((1025, 3)), np.full((4, 3), np.nan)):
        with pytest.raises(ValueError, match="nodes"):
            L.Softmax(3, nodes=bad)
    with pytest.raises(ValueError, match="no parameter"):
        lik.with_param(2.0)
    nodes = np.arange(12.0).reshape(4, 3)
    inj = L.Softmax(3, nodes=nodes)
    nodes[0, 0] = 99.0                                                   # the likelihood keeps its own copy
    assert inj.num_nodes == 4 and inj.nodes().dtype == np.float64 and inj.nodes()[0, 0] == 0.0
    # the model hands num_nodes and ITS seed (Model's constructor argument, the session's seed) to its likelihood
    from henbun_amd.models import SVGPMulticlass

    X, y, Z, _ = F.ring(3, 30, 4, 2, 0)
    for kw, want in ((dict(seed=7), 7), (dict(), hb.settings.runtime.seed)):
        lik = object.__getattribute__(SVGPMulticlass(X=X, y=y, Z=Z, num_classes=3, num_nodes=64, dtype="float64", **kw), "likelihood")
        assert (lik.num_nodes, lik.seed, lik.num_classes) == (64, want, 3)
    with pytest.raises(ValueError, match="label"):
        SVGPMulticlass(X=X, y=y + 1, Z=Z, num_classes=3, dtype="float64")


def test_logp_graph_value_equals_the_restatements_log_softmax():
    import graph_oracle

    rng = np.random.RandomState(5)
    C, n = 5, 40
    f = rng.randn(C, n) * rng.choice([1.0, 30.0], size=(1, n))
    y = rng.randint(0, C, n)
    hot = (np.arange(C)[:, None] == y[None, :]).astype(np.float64)
    out = hb.likelihoods.Softmax(C).logp(G.constant(f), G.constant(hot))
    got = graph_oracle.evaluate([out], {})[out].numpy()
    ref = (hot * F.log_softmax(f)).sum(0, keepdims=True)
    assert got.shape == (1, n)
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()


class _Holder(hb.model.Model):
    def setUp(self, gp):
        self.gp = gp


def test_natgrad_q_and_elbo_and_grad_refusals_without_a_device():
    lik = hb.likelihoods.Softmax(3, nodes=np.zeros((2, 3)))
    X, Y, M = np.zeros((5, 2)), np.zeros((5, 1)), 4
    Z = np.linspace(0, 1, 2 * M).reshape(M, 2)
    alone = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
    with pytest.raises(ValueError, match="part of a Model"):
        alone.natgrad_q(X, Y, lik)
    m = _Holder(gp=hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z))
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.natgrad_q(X, Y, lik, residual="fullrank")
    with pytest.raises(NotImplementedError, match="mean-field"):
        m.gp.natgrad_q(X, Y, lik, q0=(np.zeros((3, M)), np.ones((3, M))))
    with pytest.raises(ValueError, match=r"q0 = \(m \[3, M\]"):
        m.gp.natgrad_q(X, Y, lik, q0=(np.zeros((1, M)), np.eye(M)))         # the single-latent shape
    with pytest.raises(ValueError, match="labels"):
        m.gp.natgrad_q(X, Y + 3.0, lik)
    with pytest.raises(ValueError, match="labels"):
        m.gp.natgrad_q(X, np.zeros((5, 3)), lik)
    with pytest.raises(ValueError, match="rho"):
        m.gp.natgrad_q(X, Y, lik, rho=0.0)
    with pytest.raises(NotImplementedError, match="one latent function"):
        m.gp.elbo_and_grad(X, Y, lik, (np.zeros((3, M)), np.stack([np.eye(M)] * 3)))
    assert not m._session._ready                                           # none of this opened the device
