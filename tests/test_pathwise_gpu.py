"""Pathwise posterior function draws on the GPU, against the numpy restatement tests/pathwise_ref.py (itself pinned on the
host by tests/test_pathwise_cpu.py).

fp64 bounds are fixed: 1e-11 of scale (max|out| + max_s sum_k |coef_sk|) for the kernel (|B| <= 1, so the second term
bounds every partial sum), 1e-8 of max|f| end to end.  fp32 bounds are not constants: the device's error against float64
arithmetic on the same rounded inputs is held to 4 x the error the float32 restatement makes (as tests/test_sites_gpu.py
does).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, SVGPLik

import optimal_q_ref as R
import pathwise_ref as PR
import sites_ref as SR

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (n, L, M, d, S, span): S crosses 16 and 32, L is no multiple of a K-step (16 frequencies), M ragged and 0, n ragged
# against the 128-column strip, one strip only; in the last case x spans 200 lengthscales (phases in the hundreds)
SHAPES = [(1, 1, 0, 1, 1, 8.0), (70, 33, 0, 1, 3, 8.0), (257, 64, 96, 2, 5, 8.0), (1000, 130, 160, 3, 17, 4.0),
          (4099, 256, 512, 1, 33, 160.0)]
CASES = [s + (dl,) for s in SHAPES for dl in sorted({1, s[3]})]
SCALE = 1.7
_CASE = {}


def _case(shape, dtype):
    """Inputs rounded to the dtype, the float64 reference on them and (float32) the restatement's error: computed once."""
    key = (shape, dtype)
    if key not in _CASE:
        n, L, M, d, S, span, dl = shape
        arrs = PR.kernel_case(n, L, M, d, S, dl, span, seed=n + L + M + d + S + dl)
        x, omega, z, ell, coef = (None if a is None else a.astype(NP[dtype]) for a in arrs)
        ref = PR.evaluate(x, omega, z, ell, coef, SCALE)
        rerr = None
        if dtype == "float32":
            rerr = float(np.abs(PR.evaluate(x, omega, z, ell, coef, SCALE, dtype=np.float32) - ref).max())
        _CASE[key] = (x, omega, z, ell, coef, ref, rerr)
    return _CASE[key]


def _run(x, omega, z, ell, coef, dt):
    return H.sgp_pathwise(dev(x, dt), dev(omega, dt), None if z is None else dev(z, dt), dev(ell, dt), dev(coef, dt), scale=SCALE)


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "n%d-L%d-M%d-d%d-S%d-dl%d" % (s[0], s[1], s[2], s[3], s[4], s[6]))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernel_against_the_restatement(dtype, shape):
    """hb_sgp_pathwise_f64 / _f32 with scale = 1.7 and a mixed-sign coef whose trailing M entries are about 1e3.
    Observed on MI355X: see DESIGN.md 3, "Pathwise function draws"."""
    x, omega, z, ell, coef, ref, rerr = _case(shape, dtype)
    out = _run(x, omega, z, ell, coef, TORCH[dtype])
    torch.cuda.synchronize()
    assert out.shape == ref.shape and out.dtype == TORCH[dtype]
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    err = float(np.abs(got - ref).max())
    scale = np.abs(ref).max() + SCALE * np.abs(coef.astype(np.float64)).sum(1).max()
    if dtype == "float64":
        print("sgp_pathwise float64 %s: max error %.3e = %.3e of the scale %.3e" % (shape, err, err / scale, scale))
        assert err <= 1e-11 * scale
        return
    print("sgp_pathwise float32 %s: device %.3e, float32 restatement %.3e (%.2f x); scale %.3e"
          % (shape, err, rerr, err / max(rerr, 1e-300), scale))
    assert err <= 4.0 * rerr


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_draw_is_a_function(dtype):
    """(4099, 256, 512, 1, 33): two calls are bitwise equal, and rows [0:1000], [1000:1031], [1031:4099] evaluated on
    their own carry the bits of the whole call -- strip boundaries and ragged tails fall elsewhere in every piece."""
    dt = TORCH[dtype]
    x, omega, z, ell, coef, _, _ = _case(CASES[-1], dtype)
    xd, od, zd, ed, cd = (dev(a, dt) for a in (x, omega, z, ell, coef))
    whole = H.sgp_pathwise(xd, od, zd, ed, cd, scale=SCALE)
    again = H.sgp_pathwise(xd, od, zd, ed, cd, scale=SCALE)
    pieces = [H.sgp_pathwise(xd[a:b].contiguous(), od, zd, ed, cd, scale=SCALE) for a, b in ((0, 1000), (1000, 1031), (1031, 4099))]
    buf = torch.full_like(whole, float("nan"))
    H.sgp_pathwise(xd, od, zd, ed, cd, scale=SCALE, out=buf)
    torch.cuda.synchronize()
    assert torch.equal(whole, again) and torch.equal(whole, buf)
    assert torch.equal(whole, torch.cat(pieces, dim=1))


# ------------------------------------------------------------------------------------------------ 2. the model
_MODEL = {}


def _fitted(kind, dtype):
    """A fitted model per (class, dtype), built once: SVGPLik (Bernoulli, full-rank q from fit_q) or SVGP (mean-field q)."""
    key = (kind, dtype)
    if key not in _MODEL:
        if kind == "lik":
            X, y, Z = SR.problem(SR.BERNOULLI)
            m = SVGPLik(X=X, Y=y, Z=Z, likelihood=hb.likelihoods.Bernoulli(), dtype=dtype)
        else:
            X, y, Z = SR.problem(SR.GAUSSIAN)
            m = SVGP(X=X, Y=y, Z=Z, dtype=dtype)
            m.var = np.ones(1) * 0.09
        m.gp.kern.lengthscales = SR.ELL.copy()
        m.k_var = np.ones(1) * SR.K_VAR
        m.initialize()
        if kind == "lik":
            m.reset_q()
        m.fit_q()
        _MODEL[key] = (m, X)
    return _MODEL[key]


def _q_of(m):
    """(mean [1, M], S [M, M] lower or s [M]) as the session stores them, float64."""
    q, sess = object.__getattribute__(m, "u"), m._session
    if q.q_shape == "fullrank":
        qm, (qS,) = m._current_blocks()
        return qm, qS
    raw = lambda k: np.asarray(sess.read_raw(object.__getattribute__(q, k)), dtype=np.float64).reshape(-1)
    return raw("q_mu").reshape(1, -1), np.exp(raw("q_sqrt"))


def _factor(z, ell, dtype):
    """W of the model's whitening as float64: numpy for a float64 session; for float32 the float32 factor + inverse
    launches the model itself runs (tests/test_sites_gpu.py)."""
    jitter = hb.settings.numerics.jitter_level
    if dtype == "float64":
        return R.chol_factor(z.astype(np.float64), ell.astype(np.float64), jitter)[1]
    zd = dev(z, torch.float32)
    _, W, info = H.cholesky_inverse(H.gram_fwd(zd, zd, dev(ell, torch.float32), diag_add=float(jitter)))
    assert int(info.cpu()[0]) == 0
    return W.cpu().numpy().astype(np.float64)


XNEW = np.linspace(-1.0, 17.0, 257)[:, None]


@pytest.mark.parametrize("kind", ["lik", "gauss"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_model_draws_follow_the_restatement(dtype, kind):
    """sample_functions(5, num_features=64, noise=...)(Xnew) against pathwise_ref on the model's own z, lengthscales, W,
    q and k_var; with w = 0, eps = 0 every row is the mean of the model's predict_f (an independent HIP path); Xnew as
    numpy and as the model's Data object give the same bits.  fp64: 1e-8 of max|f|; fp32: 4 x the error of the float32
    restatement of the same evaluation."""
    m, X = _fitted(kind, dtype)
    rng = np.random.default_rng(5)
    S, L, M = 5, 64, 32
    noise = dict(omega=rng.standard_normal((L, 1)), w=rng.standard_normal((S, 2 * L)), eps=rng.standard_normal((S, M)))
    draws = m.sample_functions(S, num_features=L, noise=noise)
    assert isinstance(draws, hb.gp.PathwiseDraws) and draws.coef.shape == (S, 2 * L + M) and not draws.omega.flags.writeable
    f = draws(XNEW)
    z, ell, omega = (np.asarray(a, np.float64) for a in (draws.z, draws.lengthscales, draws.omega))
    k_var = float(np.ravel(object.__getattribute__(m, "k_var").value)[0])
    assert draws.scale == pytest.approx(np.sqrt(k_var), rel=1e-6)
    qm, qs = _q_of(m)
    W = _factor(z, ell, dtype)
    x = XNEW.astype(NP[dtype]).astype(np.float64)
    zero = dict(omega=noise["omega"], w=np.zeros((S, 2 * L)), eps=np.zeros((S, M)))
    fmean = m.sample_functions(S, num_features=L, noise=zero)(XNEW)
    pmean = m.predict_f(XNEW)[0].reshape(1, -1)
    for name, got, w, eps in (("draws", f, noise["w"], noise["eps"]), ("mean", fmean, zero["w"], zero["eps"])):
        coef = PR.coefficients(qm, qs, W, z, ell, omega, w, eps)
        ref = PR.evaluate(x, omega, z, ell, coef, draws.scale)
        err = float(np.abs(got - ref).max())
        if dtype == "float64":
            print("%s %s float64 %s: %.3e of max|f| %.3f" % (type(m).__name__, kind, name, err / np.abs(ref).max(), np.abs(ref).max()))
            assert err <= 1e-8 * np.abs(ref).max()
            bound = 1e-8 * np.abs(ref).max()
        else:
            rerr = float(np.abs(PR.evaluate(x, omega, z, ell, coef, draws.scale, dtype=np.float32) - ref).max())
            print("%s %s float32 %s: device %.3e, float32 restatement %.3e (%.2f x); max|v| %.3e"
                  % (type(m).__name__, kind, name, err, rerr, err / rerr, np.abs(coef[:, 2 * L:]).max()))
            assert err <= 4.0 * rerr
            bound = 4.0 * rerr
        if name == "mean":
            perr = float(np.abs(got - pmean).max())
            print("   rows against predict_f's mean: %.3e (bound %.3e)" % (perr, bound))
            assert perr <= bound
    # the same points as an array and as the model's own Data: the same bits
    a = draws(X)
    b = draws.evaluate(object.__getattribute__(m, "X")).cpu().numpy()
    assert a.shape == (S, X.shape[0]) and np.array_equal(a, b)
    assert np.array_equal(draws(X[100:163]), a[:, 100:163])


def test_device_rng_draws_have_the_exact_law_at_their_frequencies():
    """S = 4096 draws with 256 features at 64 points inside the data range, float64 session.  Given omega the draws are
    Gaussian with mean sqrt(k) m A and covariance k pathwise_ref.covariance (no 1 / sqrt(L) term enters): the sample mean
    is within 6 sqrt(v_j / S) of the mean, the sample variance within 6 v_j sqrt(2 / (S - 1)) of v_j.  The same seed gives
    the same bits, another seed other coefficients."""
    m, X = _fitted("lik", "float64")
    S, L = 4096, 256
    draws = m.sample_functions(S, num_features=L, seed=3)
    x = np.linspace(0.5, 15.5, 64)[:, None]
    f = draws(x)
    z, ell, omega = draws.z, draws.lengthscales, draws.omega
    qm, qS = _q_of(m)
    W = _factor(z, ell, "float64")
    k = draws.scale ** 2
    mean = draws.scale * (qm @ R.A_of(W, z, x, ell)).reshape(-1)
    v = k * np.diag(PR.covariance(x, omega, z, ell, W, qS))
    em, ev = np.abs(f.mean(0) - mean) / np.sqrt(v / S), np.abs(f.var(0, ddof=1) - v) / (v * np.sqrt(2.0 / (S - 1)))
    print("device RNG: sample mean within %.2f standard errors, sample variance within %.2f; v in [%.3g, %.3g]"
          % (em.max(), ev.max(), v.min(), v.max()))
    assert f.shape == (S, 64) and em.max() <= 6.0 and ev.max() <= 6.0
    again, other = m.sample_functions(S, num_features=L, seed=3), m.sample_functions(S, num_features=L, seed=4)
    assert np.array_equal(again.coef, draws.coef) and np.array_equal(again.omega, draws.omega)
    assert np.array_equal(again(x), f)
    assert not np.array_equal(other.coef, draws.coef)


def test_pathwise_draws_refuses_what_it_does_not_cover():
    m, X = _fitted("lik", "float64")
    q = object.__getattribute__(m, "u")
    with pytest.raises(NotImplementedError, match="one latent function"):
        m.gp.pathwise_draws((np.zeros((2, 32)), np.eye(32)), 3)
    for bad in (dict(omega=np.zeros((8, 1)), w=np.zeros((3, 16))),                                 # eps missing
                dict(omega=np.zeros((8, 1)), w=np.zeros((3, 16)), eps=np.zeros((3, 31))),          # eps [S, M - 1]
                dict(omega=np.zeros((8, 2)), w=np.zeros((3, 16)), eps=np.zeros((3, 32))),          # omega [L, d + 1]
                np.zeros((3, 16))):
        with pytest.raises(ValueError, match="noise"):
            m.gp.pathwise_draws(q, 3, num_features=8, noise=bad)
    with pytest.raises(ValueError):
        m.gp.pathwise_draws(q, 0)
    with pytest.raises(ValueError):
        m.sample_functions(2, num_features=8)(np.zeros((4, 2)))

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    Z = SR.problem(SR.BERNOULLI)[2]
    prior = (np.zeros((1, 32)), np.eye(32))
    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.pathwise_draws(prior, 3)
    with pytest.raises(NotImplementedError, match="one expert"):
        Other(Z=np.stack([Z, Z]), kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))), dtype="float64").gp.pathwise_draws(prior, 3)
