"""SparseGP.predict_f on the MI355X: the fused streaming kernel (fp32) and the chunked form (fp32 / fp64) of
hb_sgp_predict against an fp64 reference written here from the definition,

    A = Lm^-1 K(z, x),  u ~ N(m, S S^T):   mean = m A,   var = ||S^T A_j||^2 + r_j,
    r = |1 - colsum A^2| ('diagonal'), 0 ('neglected'), 1 - colsum A^2 + jitter ('fullrank'),

with Lm and K from henbun_oracle; the forms against each other; the moments against draws of samples(); the full size
(N = 1e6, M = 512) with its memory bound; the planner's choice; the SVGP helpers."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
import henbun_oracle as O
from henbun_amd import graph as G
from henbun_amd.models import SVGP, svgp_data
from parity import observe, rel_err

pytestmark = pytest.mark.gpu
tf = hb.tf
FUSED = "fused streaming prediction"


class PredModel(hb.model.Model):
    def setUp(self, Z, ell, cls, shape, q_shape, tri_pack=None):
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(ell), z=Z)
        kw = dict(shape=shape, q_shape=q_shape)
        if tri_pack is not None:
            kw["tri_pack"] = tri_pack
        self.u = cls(**kw)


def _build(dtype, case, seed=0):
    d, M, E, P, cls, qs, packed = (case[k] for k in ("d", "M", "E", "P", "cls", "qs", "packed"))
    rng = np.random.RandomState(seed)
    box = 0.6 * M ** (1.0 / d)
    Z = rng.uniform(0, box, ((E,) if E > 1 else ()) + (M, d))
    ell = rng.uniform(0.8, 1.3, (E, d) if E > 1 else (d,))
    shape = ([E] if E > 1 else []) + [P, M]
    m = PredModel(Z=Z, ell=ell, cls=cls, shape=shape, q_shape=qs, tri_pack=(True if packed else None), dtype=dtype)
    q = object.__getattribute__(m, "u")
    size = E * P * M
    q.q_mu = rng.randn(size)
    if qs == "diagonal":
        q.q_sqrt = np.log(rng.uniform(0.2, 1.0, size))
    else:
        S = np.tril(0.3 * rng.randn(size, size) / np.sqrt(size)) + np.diag(rng.uniform(0.2, 0.9, size))
        q.q_sqrt = S
    if cls is hb.variationals.Gaussian:
        q.scale = np.full([1] * len(shape), 1.7)
    m.initialize()
    x = rng.uniform(-0.5, box + 0.5, (case["n"], d))
    return m, q, x


def _values(m, q):
    """The stored parameters (fp64 copies) of the model and its variational."""
    s = m._session
    val = lambda v: np.asarray(s.read_value(v), dtype=np.float64)
    z = val(object.__getattribute__(m.gp, "z"))
    ell = val(object.__getattribute__(m.gp.kern, "lengthscales"))
    mu = val(object.__getattribute__(q, "q_mu"))
    sq = val(object.__getattribute__(q, "q_sqrt"))
    scale = val(object.__getattribute__(q, "scale")).reshape(-1)[0] if type(q) is hb.variationals.Gaussian else 1.0
    return z, ell, mu, sq, scale, q.packed


def reference(x, z, ell, mu, sq, scale, packed, q, mode, jitter):
    """fp64 moments from the definition (henbun_oracle's Gram and Cholesky)."""
    shape = list(q._shape)
    P, M = shape[-2], shape[-1]
    E = z.shape[0] if z.ndim == 3 else 1
    z3 = z.reshape(E, M, -1)
    ell2 = ell.reshape(E, -1) if ell.ndim == 2 else np.broadcast_to(ell, (E, ell.size))
    m = scale * mu.reshape(E, P, M)
    if q.q_shape == "diagonal":
        s = scale * np.exp(sq).reshape(E, P, M)
    else:
        S = O.vec_to_tri(O.T(sq)).numpy() if packed else np.tril(sq)
        S = scale * S
    xt = O.T(x)
    mean, var = np.zeros((E, P, len(x))), np.zeros((E, P, len(x)))
    for e in range(E):
        zt, lt = O.T(z3[e]), O.T(ell2[e])
        # the kernel from the coordinate difference (as the HIP kernels form it): the reference's |a|^2 + |b|^2 - 2ab
        # alone costs ~1e-10 here in fp64 at inputs out to 300 lengthscales
        Lm = O.kern_cholesky(zt, lt, jitter, K=O.rbf_K_difference)
        A = torch.linalg.solve_triangular(Lm, O.rbf_K_difference(zt, xt, lt), upper=False).numpy()
        a2 = (A * A).sum(0)
        r = np.abs(1.0 - a2) if mode == "diagonal" else (1.0 - a2 + jitter) if mode == "fullrank" else 0.0 * a2
        for p in range(P):
            mean[e, p] = m[e, p] @ A
            if q.q_shape == "diagonal":
                var[e, p] = (s[e, p] ** 2) @ (A * A) + r
            else:
                Sep = S[(e * P + p) * M:(e * P + p + 1) * M, :]
                C = Sep.T @ A
                var[e, p] = (C * C).sum(0) + r
    lead = (E,) if z.ndim == 3 else ()
    return mean.reshape(lead + (P, len(x))), var.reshape(lead + (P, len(x)))


def _predict(m, q, x, mode, fused=True, jitter=1e-3, generic=False):
    """(mean, var, plan notes) of one plan with both outputs."""
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = jitter
    cfg.runtime.fused_predict = fused
    with hb.settings.temp_settings(cfg):
        with m.tf_mode():
            if generic:
                from henbun_amd.gp.gp import _posterior_of

                mm, s, kind = _posterior_of(q)
                mean, var = m.gp._predict_generic(G.as_tensor(x), mm, s, kind, mode, jitter)
            else:
                mean, var = m.gp.predict_f(x, q, q_shape=mode)
        plan = m._session.make_plan([mean, var])
        plan.run()
        plan.check()
        notes = [e for e in plan.explain if e[0].startswith(FUSED)]
        return plan.value(plan.outputs[0]), plan.value(plan.outputs[1]), notes


N_, G_ = hb.variationals.Normal, hb.variationals.Gaussian
CASES = [
    dict(d=1, M=64, n=1000, E=1, P=1, cls=N_, qs="diagonal", packed=False, mode="diagonal"),
    dict(d=2, M=512, n=777, E=1, P=3, cls=N_, qs="diagonal", packed=False, mode="neglected"),
    dict(d=3, M=64, n=1001, E=4, P=1, cls=G_, qs="diagonal", packed=False, mode="diagonal"),
    dict(d=1, M=512, n=2049, E=1, P=1, cls=N_, qs="fullrank", packed=False, mode="fullrank"),
    dict(d=2, M=64, n=333, E=1, P=1, cls=N_, qs="fullrank", packed=True, mode="diagonal"),
    dict(d=1, M=512, n=5003, E=4, P=3, cls=G_, qs="diagonal", packed=False, mode="fullrank"),
    dict(d=3, M=512, n=999, E=1, P=1, cls=G_, qs="fullrank", packed=False, mode="neglected"),
]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_fused_fp32_and_chunked_fp64_match_the_definition(ci):
    case = CASES[ci]
    mode = case["mode"]
    m, q, x = _build("float32", case)
    mean, var, notes = _predict(m, q, x, mode)
    assert notes and all(n[2] for n in notes), notes       # the fused kernel ran
    z, ell, mu, sq, scale, packed = _values(m, q)
    x32 = x.astype(np.float32).astype(np.float64)
    rm, rv = reference(x32, z, ell, mu, sq, scale, packed, q, mode, 1e-3)
    assert mean.shape == rm.shape and var.shape == rv.shape
    # the chunked fp32 form on the same inputs (same factor W: only the contraction and the sums differ)
    cm, cv, notes = _predict(m, q, x, mode, fused=False)
    assert notes and not any(n[2] for n in notes)
    observe("predict chunked-vs-fused mean case %d" % ci, rel_err(cm, mean), 2e-5)
    observe("predict chunked-vs-fused var case %d" % ci, rel_err(cv, var), 2e-5)
    # against fp64: dominated by the fp32 factorisation of Kmm + jitter I, shared by both forms (random z in d >= 2
    # clusters; with jitter 1e-4 instead of 1e-3 the d = 2, M = 512 case measured 2.5e-4 in the mean)
    observe("predict fused mean case %d" % ci, rel_err(mean, rm), 5e-4)
    observe("predict fused var case %d" % ci, rel_err(var, rv), 5e-4)
    # fp64: the chunked form, to fp64 rounding
    m64, q64, _ = _build("float64", case)
    mean64, var64, _ = _predict(m64, q64, x, mode)
    z, ell, mu, sq, scale, packed = _values(m64, q64)
    rm, rv = reference(x, z, ell, mu, sq, scale, packed, q64, mode, 1e-3)
    assert rel_err(mean64, rm) <= 1e-10 and rel_err(var64, rv) <= 1e-10, (rel_err(mean64, rm), rel_err(var64, rv))


@pytest.mark.parametrize("ci", [0, 3, 4])
def test_fused_chunked_and_generic_composition_agree(ci):
    case = dict(CASES[ci], n=300)
    m, q, x = _build("float32", case, seed=3)
    fm, fv, _ = _predict(m, q, x, case["mode"])
    cm, cv, _ = _predict(m, q, x, case["mode"], fused=False)
    gm, gv, _ = _predict(m, q, x, case["mode"], generic=True)
    # chunked and fused share the factor W; the generic plan factorises Kmm in a launch of its own (no sgp_predict
    # consumer, no fragment-major images), whose fp32 rounding moves A by ~cond(Kmm) 2^-24 (2.5e-4 measured at M = 512)
    for name, a, b, tol in [("chunked mean", cm, fm, 2e-5), ("chunked var", cv, fv, 2e-5),
                            ("generic mean", gm, fm, 1e-3), ("generic var", gv, fv, 1e-3)]:
        observe("predict forms agree: " + name, rel_err(a, b), tol)


@pytest.mark.parametrize("qs, mode, cls", [("diagonal", "diagonal", N_), ("fullrank", "neglected", N_),
                                           ("diagonal", "fullrank", G_)])
def test_moments_are_those_of_samples(qs, mode, cls):
    case = dict(d=1, M=64, n=48, E=1, P=1, cls=cls, qs=qs, packed=False, mode=mode)
    m, q, x = _build("float32", case, seed=5)
    pm, pv, _ = _predict(m, q, x, mode)
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 1e-3
    with hb.settings.temp_settings(cfg):
        with m.tf_mode():
            f = m.gp.samples(x, m.u, q_shape=mode)
        plan = m._session.make_plan([f])
    K = 4000
    draws = np.empty((K,) + tuple(f.shape))
    for i in range(K):
        plan.run()
        draws[i] = plan.value(plan.outputs[0])
    plan.check()
    smean, svar = draws.mean(0), draws.var(0, ddof=1)
    z_mean = np.abs(smean - pm) / np.sqrt(pv / K)
    z_var = np.abs(svar - pv) / (pv * np.sqrt(2.0 / (K - 1)))
    assert z_mean.max() < 5.0, z_mean.max()
    assert z_var.max() < 5.0, z_var.max()


def test_full_size_streaming_and_planner():
    """N = 1e6 test points, M = 512, d = 1, cfg-2-like data after 50 Adam steps: diagonal and full-rank q(u) against the
    fp64 reference on a strided subset; the peak device memory stays far below what materialising A would take; the
    planner takes the fused form at M = 512 and the chunked form at M = 1024."""
    X, Y, Z = svgp_data(16384, 512, 0, dtype=np.float32)
    N = 10 ** 6
    xs = np.linspace(-2.0, 258.0, N)[:, None]
    x32 = xs.astype(np.float32).astype(np.float64)
    for qs in ("diagonal", "fullrank"):
        np.random.seed(0)
        m = SVGP(X=X, Y=Y, Z=Z, q_shape=qs)
        m.ELBO().compile(optimizer=tf.train.AdamOptimizer(0.01))
        m.ELBO().optimize(maxiter=50, minibatch_size=8192)
        q = object.__getattribute__(m, "u")
        jitter = hb.settings.numerics.jitter_level
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with m.tf_mode():
            mean, var = m.gp.predict_f(xs, q, q_shape="diagonal")
        plan = m._session.make_plan([mean, var])
        plan.run()
        plan.check()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base - 3 * N * 4    # x, mean, var
        assert rise < 64 * 2 ** 20, rise / 2 ** 20
        notes = [e for e in plan.explain if e[0].startswith(FUSED)]
        assert notes and all(e[2] for e in notes), notes
        pm, pv = plan.value(plan.outputs[0]), plan.value(plan.outputs[1])
        idx = np.arange(0, N, 15)          # 66 667 points
        z, ell, mu, sq, scale, packed = _values(m, q)
        rm, rv = reference(x32[idx], z, ell, mu, sq, scale, packed, q, "diagonal", jitter)
        # fp32 factorisation of Kmm + 1e-5 I at cond ~5e5 (spacing 0.5 lengthscales): 1.2e-3 measured in the mean
        observe("predict full size mean " + qs, rel_err(pm[:, idx], rm), 5e-3)
        observe("predict full size var " + qs, rel_err(pv[:, idx], rv), 5e-3)
        del plan
    # planner: M = 1024 (cfg 3 size) takes the chunked form
    case = dict(d=1, M=1024, n=4096, E=1, P=1, cls=N_, qs="fullrank", packed=False, mode="diagonal")
    m, q, x = _build("float32", case)
    _, _, notes = _predict(m, q, x, "diagonal")
    assert notes and not any(e[2] for e in notes), notes


def test_svgp_predict_helpers():
    np.random.seed(0)
    X, Y, Z = svgp_data(3000, 48, 0)
    m = SVGP(X=X, Y=Y, Z=Z, dtype="float64")
    m.ELBO().compile(optimizer=tf.train.AdamOptimizer(0.01))
    m.ELBO().optimize(maxiter=200, minibatch_size=512)
    xs = np.linspace(0, 24, 50)[:, None]
    fm, fv = m.predict_f(xs)
    ym, yv = m.predict_y(xs)
    assert fm.shape == fv.shape == (1, 50)
    s = m._session
    k_var = float(s.read_value(object.__getattribute__(m, "k_var"))[0])
    noise = float(s.read_value(object.__getattribute__(m, "var"))[0])
    _, _, mu, sq, scale, packed = _values(m, object.__getattribute__(m, "u"))
    z, ell = _values(m, object.__getattribute__(m, "u"))[:2]
    rm, rv = reference(xs, z, ell, mu, sq, scale, packed, object.__getattribute__(m, "u"), "diagonal",
                       hb.settings.numerics.jitter_level)
    assert rel_err(fm, rm * np.sqrt(k_var)) < 1e-10 and rel_err(fv, rv * k_var) < 1e-10
    assert np.allclose(ym, fm) and np.allclose(yv, fv + noise, rtol=1e-12)
    assert np.all(fv > 0)
    assert np.mean((fm[0] - np.sin(xs[:, 0])) ** 2) < 0.3
