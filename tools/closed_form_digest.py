"""Digest of everything the eager (non-graph) GP routes return, for comparing two trees bit by bit.

    python tools/closed_form_digest.py > digest.txt

Fixed-seed problems, the PUBLIC API only (so the script runs unchanged on an older tree), one line `name sha256` per
returned array or float, taken over its float64 bytes; a call that raises prints `name raised <ExceptionType>`.  Two runs
of one tree must agree first (the kernels fold in fixed order); then two trees whose host code differs only in where it
lives must agree line by line.  Sessions float32 and float64; (N, M, d, P) = (97, 32, 1, 1): one chunk, fragment images
in float32; (40001, 96, 3, 2): two chunks; (4096, 50, 1, 1): M no multiple of 32, the plain forms.  The likelihoods over
several latent functions (Softmax with 3 classes over 16 fixed nodes, HeteroscedasticGaussian) run natgrad_q,
elbo_and_grad_multi and the fit_hyper of their models on the same problems."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import henbun_amd as hb  # noqa: E402
from henbun_amd.models import SVGP, ExactGPR, SVGPHetero, SVGPLik, SVGPMulticlass  # noqa: E402

CASES = [(97, 32, 1, 1), (40001, 96, 3, 2), (4096, 50, 1, 1)]
NOISE, K_VAR = 0.4, 1.3
NODES = np.random.RandomState(7).randn(16, 3)          # the softmax likelihood's fixed nodes [S, C]


def digest(name, v):
    if isinstance(v, dict):
        for k in sorted(v):
            digest("%s.%s" % (name, k), v[k])
    elif isinstance(v, (tuple, list)):
        for i, a in enumerate(v):
            digest("%s.%d" % (name, i), a)
    elif v is not None:
        a = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.float64)
        print("%s %s" % (name, hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def call(name, fn):
    try:
        out = fn()
    except Exception as e:  # noqa: BLE001  (which exception is part of the digest)
        print("%s raised %s" % (name, type(e).__name__), flush=True)
        return None
    digest(name, out)
    return out


def problem(N, M, d, P):
    """The data of tests/test_optimal_q_gpu.py::_stats_case, plus labels and counts for the other likelihoods (the
    three-class labels from a stream of their own: the draws above are those of the earlier digests)."""
    rng = np.random.RandomState(N + M + d + P)
    dom = 0.5 * M if d == 1 else 4.0
    X = rng.uniform(0, dom, (N, d))
    F = np.sin(X.sum(1, keepdims=True) + np.arange(P)[None, :])
    Y = F + 0.3 * rng.randn(N, P)
    Z = np.linspace(0, dom, M)[:, None] if d == 1 else rng.uniform(0, dom, (M, d))
    ell = np.ones(1) * 0.9 if d == 1 else np.array([0.9, 1.1, 1.3])
    ybin = (rng.uniform(size=(N, 1)) < 1.0 / (1.0 + np.exp(-2.0 * F[:, :1]))).astype(np.float64)
    ycnt = rng.poisson(np.exp(F[:, :1])).astype(np.float64)
    score = np.stack([F[:, 0], -F[:, 0], np.zeros(N)], 1) + 0.5 * np.random.RandomState(N + M + d + P + 1).randn(N, 3)
    return X, Y, Z, ell, ybin, ycnt, np.argmax(score, 1).astype(np.float64)[:, None]


class Host(hb.model.Model):
    def setUp(self, X, Y, Z, ell):
        self.X, self.Y = hb.param.Data(X), hb.param.Data(Y)
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(ell), z=Z)


def sparse_routes(tag, dtype, X, Y, Z, ell, ybin, ycnt, ycls):
    m = Host(X=X, Y=Y, Z=Z, ell=ell, dtype=dtype)
    m.gp.kern.lengthscales = ell.copy()
    m.initialize()
    gp, M = m.gp, Z.shape[0]
    stats = call(tag + "statistics", lambda: gp.statistics(m.X, m.Y))
    q = None
    for shape in ("fullrank", "diagonal"):
        out = call(tag + "optimal_q.%s" % shape, lambda: gp.optimal_q(m.X, m.Y, NOISE, K_VAR, q_shape=shape, stats=stats))
        q = out if shape == "fullrank" else q
    for res in ("diagonal", "neglected"):
        call(tag + "collapsed_bound.%s.stats" % res, lambda: gp.collapsed_bound(m.X, m.Y, NOISE, K_VAR, residual=res, stats=stats))
        call(tag + "collapsed_bound.%s" % res, lambda: gp.collapsed_bound(X, Y, NOISE, K_VAR, residual=res))
        call(tag + "collapsed_bound_and_grad.%s" % res, lambda: gp.collapsed_bound_and_grad(m.X, m.Y, NOISE, K_VAR, residual=res))
    q0 = (0.1 * np.cos(np.arange(M))[None, :], 0.5 * np.eye(M) + np.tril(0.01 * np.sin(np.arange(M * M)).reshape(M, M), -1))
    for lname, lik, y in (("bernoulli", hb.likelihoods.Bernoulli(), ybin), ("poisson", hb.likelihoods.Poisson(), ycnt)):
        for rho in (1.0, 0.5):
            for start, qs in (("prior", None), ("q0", q0)):
                call(tag + "natgrad_q.%s.rho%g.%s" % (lname, rho, start),
                     lambda: gp.natgrad_q(X, y, lik, k_var=K_VAR, q0=qs, steps=3, rho=rho))
        call(tag + "elbo_and_grad.%s" % lname, lambda: gp.elbo_and_grad(X, y, lik, q0, k_var=K_VAR))
    for lname, lik in (("gaussian", hb.likelihoods.Gaussian(NOISE)), ("laplace", hb.likelihoods.Laplace(0.5))):
        call(tag + "elbo_and_grad.%s.lik_grad" % lname, lambda: gp.elbo_and_grad(X, Y[:, :1], lik, q0, k_var=K_VAR, lik_grad=True))
    for lname, lik, y in (("softmax", hb.likelihoods.Softmax(3, nodes=NODES), ycls),
                          ("hetgauss", hb.likelihoods.HeteroscedasticGaussian(-1.0), Y[:, :1])):
        scale = 1.0 + 0.1 * np.arange(lik.num_latent)
        qC = (scale[:, None] * q0[0], scale[:, None, None] * q0[1])          # blocks (m [C, M], S [C, M, M]) that differ
        for start, qs in (("prior", None), ("q0", qC)):
            call(tag + "natgrad_q.%s.rho0.5.%s" % (lname, start),
                 lambda: gp.natgrad_q(X, y, lik, k_var=K_VAR, q0=qs, steps=3, rho=0.5))
        call(tag + "elbo_and_grad_multi.%s" % lname, lambda: gp.elbo_and_grad_multi(X, y, lik, qC, k_var=K_VAR))
        if lik.trainable:
            call(tag + "elbo_and_grad_multi.%s.lik_grad" % lname,
                 lambda: gp.elbo_and_grad_multi(X, y, lik, qC, k_var=K_VAR, lik_grad=True))
    if q is not None:
        xs = np.linspace(X.min(), X.max(), 33 * X.shape[1]).reshape(33, X.shape[1])
        call(tag + "pathwise_draws", lambda: gp.pathwise_draws((q[0][:1], q[1]), 4, num_features=256, k_var=K_VAR, seed=1)(xs))
    call(tag + "select_inducing", lambda: (gp.select_inducing(m.X), gp.z.value))     # moves z: the last call on this model


def exact_routes(tag, dtype, X, Y, ell):
    n = min(X.shape[0], 1500)            # the exact routes cost N^2 per iteration: the first rows are enough
    X, Y = X[:n], Y[:n]
    m = ExactGPR(X=X, Y=Y, dtype=dtype)
    m.gp.kern.lengthscales = ell[:1].copy()         # the models hold one lengthscale
    m.k_var, m.var = np.ones(1) * K_VAR, np.ones(1) * NOISE
    m.initialize()
    xs = X[np.linspace(0, n - 1, 600).astype(int) % n] + 0.01
    call(tag + "condition.predict_f", lambda: m.gp.condition(m.X, m.Y, NOISE, K_VAR).predict_f(xs))
    call(tag + "log_marginal_likelihood_and_grad", lambda: m.gp.log_marginal_likelihood_and_grad(m.X, m.Y, NOISE, K_VAR, seed=0)[:2])
    call(tag + "ExactGPR.fit_hyper", lambda: (m.fit_hyper(2), m.gp.kern.lengthscales.value, m.k_var.value, m.var.value))


def model_routes(tag, dtype, X, Y, Z, ell, ybin, ycls):
    def fresh(cls, y, **kw):
        np.random.seed(0)                # the models draw their initial q(u) from numpy's global stream
        m = cls(X=X, Z=Z, dtype=dtype, **{"y" if cls is SVGPMulticlass else "Y": y}, **kw)
        m.gp.kern.lengthscales = ell[:1].copy()
        m.k_var = np.ones(1) * K_VAR
        return m

    hyper = lambda m: (m.gp.z.value, m.gp.kern.lengthscales.value, m.k_var.value, m.u.q_mu.value, m.u.q_sqrt.value)
    for shape in ("fullrank", "diagonal"):
        m = fresh(SVGP, Y[:, :1], q_shape=shape)
        m.var = np.ones(1) * NOISE
        call(tag + "SVGP.fit_q.%s" % shape, lambda: (m.fit_q(), hyper(m)))
    call(tag + "SVGP.fit_hyper", lambda: (m.fit_hyper(3), hyper(m), m.var.value))
    ml = fresh(SVGPLik, ybin, likelihood=hb.likelihoods.Bernoulli())
    call(tag + "SVGPLik.reset_q.fit_hyper", lambda: (ml.reset_q(), ml.fit_hyper(2, q_steps=2), hyper(ml)))
    ml = fresh(SVGPLik, Y[:, :1], likelihood=hb.likelihoods.Gaussian(NOISE), learn_likelihood=True)
    call(tag + "SVGPLik.learn_likelihood.reset_q.fit_hyper",
         lambda: (ml.reset_q(), ml.fit_hyper(2, q_steps=2), hyper(ml), ml.lik_param.value))
    mc = fresh(SVGPMulticlass, ycls, num_classes=3, nodes=NODES)
    call(tag + "SVGPMulticlass.reset_q.fit_hyper", lambda: (mc.reset_q(), mc.fit_hyper(2, q_steps=2), hyper(mc)))
    mh = fresh(SVGPHetero, Y[:, :1])
    call(tag + "SVGPHetero.reset_q.fit_hyper", lambda: (mh.reset_q(), mh.fit_hyper(2, q_steps=2), hyper(mh), mh.lik_param.value))
    call(tag + "greedy_inducing", lambda: hb.gp.greedy_inducing(X, Z.shape[0], ell, return_info=True, dtype=dtype))


def main():
    for dtype in ("float32", "float64"):
        for N, M, d, P in CASES:
            tag = "%s.N%d.M%d.d%d.P%d." % (dtype, N, M, d, P)
            X, Y, Z, ell, ybin, ycnt, ycls = problem(N, M, d, P)
            cfg = hb.settings.get_settings()
            cfg.numerics.jitter_level = 1e-5 if d == 1 else 1e-3
            with hb.settings.temp_settings(cfg):
                sparse_routes(tag, dtype, X, Y, Z, ell, ybin, ycnt, ycls)
                exact_routes(tag, dtype, X, Y, ell)
                model_routes(tag, dtype, X, Y, Z, ell, ybin, ycls)


if __name__ == "__main__":
    main()
