"""The exact GP's log marginal likelihood, its gradient and ExactGPR.fit_hyper on the GPU, against the dense float64
algebra and the same-probe numpy estimator of tests/exact_mll_ref.py (pinned on the host by tests/test_exact_mll_cpu.py).

Bounds are stated in the SUM OF THE MAGNITUDES OF THE TERMS (`mag` of exact_mll_ref.mll_dense): for the value
1/2 sum_c |y_c . alpha_c| + P/2 |logdet K^| + N P / 2 log 2 pi, for a gradient component 1/2 sum_c |alpha_c^T dK^ alpha_c| +
P/2 |tr K^^-1 dK^|.  float64 at tol 1e-6: 1e-5 of it (the restatement reaches 1e-7 at that tolerance: the 100 x margin
the test of alpha uses).  float32 at the default tol 1e-3: F32_FACTOR x tol of it.  Every figure is printed before it is
asserted."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.gp import exact
from henbun_amd.models import ExactGPR

import exact_gp_ref as E
import exact_mll_ref as R

pytestmark = pytest.mark.gpu

ELL, K_VAR, NOISE = np.array([0.5, 0.7]), 1.3, 0.05      # the small case: N = 48, P = 2
F32_FACTOR = 1.0     # float32 errors at tol 1e-3 are asserted below F32_FACTOR x 1e-3 x magnitude: about 10 x the worst seen, 0.13
_REF = {}


class Host(hb.model.Model):
    def setUp(self, kern):
        self.gp = hb.gp.GP(kern=kern)


def _gp(X, Y, ell, dtype):
    """(model, its GP) with a UnitRBF kernel of len(ell) lengthscales"""
    m = Host(kern=hb.gp.kernels.UnitRBF(np.array(ell, dtype=np.float64)), dtype=dtype)
    return m, m.gp


def _small(rank):
    """(X, Y [48, 2], C, orthogonal probes Z [48, 48], mll_dense) of the small case, once per rank."""
    if ("small", rank) not in _REF:
        X, Y, _, _, _ = E.plane_case(48)
        Y = np.concatenate([Y, np.cos(X[:, :1])], axis=1)
        C = E.factor(X, ELL, rank) if rank else None
        Z = R.orthogonal_probes(R.precond_dense(X, C, K_VAR, NOISE))
        _REF[("small", rank)] = (X, Y, C, Z, R.mll_dense(X, Y, ELL, K_VAR, NOISE))
    return _REF[("small", rank)]


def _plane():
    """(X, Y, ell, k_var, noise_var, Z [16, 300] Gaussian with covariance P_ at rank 64, mll_dense, mll_estimate at tol 1e-6)
    of plane_case(300), once."""
    if "plane" not in _REF:
        X, Y, ell, k_var, noise_var = E.plane_case(300)
        C = E.factor(X, ell, 64)
        Z = np.random.default_rng(6).standard_normal((16, 300)) @ np.linalg.cholesky(R.precond_dense(X, C, k_var, noise_var)).T
        _REF["plane"] = (X, Y, ell, k_var, noise_var, Z, R.mll_dense(X, Y, ell, k_var, noise_var),
                         R.mll_estimate(X, Y, ell, k_var, noise_var, Z, C, tol=1e-6))
    return _REF["plane"]


def _ratios(value, grad, ref_value, ref_grad, mag):
    """error / magnitude of the value and of every gradient component -> dict of floats"""
    out = dict(value=abs(value - ref_value) / mag["value"])
    for k in ("lengthscales", "k_var", "noise_var"):
        out[k] = float(np.max(np.abs(np.asarray(grad[k]) - ref_grad[k]) / mag[k]))
    return out


# ---------------------------------------------------------------- the recording PCG steps
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_recording_steps_log_alpha_and_beta_and_move_nothing_else(dtype):
    """hb_pcg_update_coef / hb_pcg_direction_coef on random vectors [4, 3001], row 1 converged, at iteration 1 of a log of 3:
    alpha and beta within 1e-12 relative of numpy on the same inputs, x, r, p, rz, rr bitwise those of the non-recording
    entries, the converged row and every other row of the log still NaN."""
    dt, npdt = (torch.float64, np.float64) if dtype == "float64" else (torch.float32, np.float32)
    rng = np.random.default_rng(11)
    S, N = 4, 3001
    x, r, p, Ap, w = (rng.standard_normal((S, N)).astype(npdt) for _ in range(5))
    Ap = (Ap + 3.0 * p).astype(npdt)
    rz, thr = rng.uniform(1.0, 2.0, S), np.full(S, 10.0)
    rr = (r.astype(np.float64) ** 2).sum(1)
    thr[1] = 2.0 * rr[1]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    f64 = lambda a: a.astype(np.float64)
    live = np.array([0, 2, 3])
    nan_log = lambda: torch.full((6, S), float("nan"), dtype=torch.float64, device="cuda")

    plain, rec, log = (up(x), up(r), up(rr)), (up(x), up(r), up(rr)), nan_log()
    H.pcg_update(plain[0], plain[1], up(p), up(Ap), up(rz), plain[2], up(thr))
    H.pcg_update(rec[0], rec[1], up(p), up(Ap), up(rz), rec[2], up(thr), coef=log, it=1)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, rec))
    lg = log.cpu().numpy()
    alpha = rz / (f64(p) * f64(Ap)).sum(1)
    print("%s alpha: %.3e relative" % (dtype, np.abs(lg[2, live] / alpha[live] - 1).max()))
    assert np.abs(lg[2, live] / alpha[live] - 1).max() <= 1e-12
    assert np.isnan(lg[2, 1]) and np.isnan(np.delete(lg, 2, axis=0)).all()
    xr, rref, _ = E.pcg_update(f64(x), f64(r), f64(p), f64(Ap), rz, rr, thr)
    assert np.abs(rec[0].cpu().numpy() - xr).max() <= 4 * np.finfo(npdt).eps * np.abs(xr).max()

    for wv, first in ((w, False), (None, False), (w, True)):
        plain, rec, log = (up(p), up(rz)), (up(p), up(rz)), nan_log()
        wd = None if wv is None else up(wv)
        H.pcg_direction(up(r), wd, plain[0], plain[1], up(rr), up(thr), wscale=1.3, zscale=0.7, first=first)
        H.pcg_direction(up(r), wd, rec[0], rec[1], up(rr), up(thr), wscale=1.3, zscale=0.7, first=first, coef=log, it=1)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(plain, rec))
        lg = log.cpu().numpy()
        _, rzr = E.pcg_direction(f64(r), None if wv is None else f64(wv), f64(p), rz, rr, thr, 1.3, 0.7, first)
        if first:
            assert np.array_equal(lg[3, live], np.zeros(3))                       # beta of a first step is 0, stored as such
        else:
            beta = rzr / rz
            print("%s beta (w %s): %.3e relative" % (dtype, wv is not None, np.abs(lg[3, live] / beta[live] - 1).max()))
            assert np.abs(lg[3, live] / beta[live] - 1).max() <= 1e-12
        assert np.isnan(lg[3, 1]) and np.isnan(np.delete(lg, 3, axis=0)).all()
    with pytest.raises(ValueError, match="coef"):
        H.pcg_update(rec[0], rec[0], rec[0], rec[0], up(rz), up(rr), up(thr), coef=nan_log(), it=3)


def test_a_recorded_solve_is_the_same_solve():
    """plane_case(300), float64, rank 64: pcg_solve(record=True) returns the bits of record=False, the same counts, and a log
    of `iterations` rows whose NaNs mark where the row stopped; record=False carries no log."""
    X, Y, ell, k_var, noise_var = E.plane_case(300)
    m, gp = _gp(X, Y, ell, "float64")
    sess, Xd, Yt, elld, tol, precond = gp._exact_inputs("test", X, Y, noise_var, k_var, 64, None)
    B = torch.cat([Yt, 2.0 * Yt, torch.zeros_like(Yt)]).contiguous()
    x0, i0 = exact.pcg_solve(sess, Xd, elld, k_var, noise_var, B, precond, tol, 1000)
    x1, i1 = exact.pcg_solve(sess, Xd, elld, k_var, noise_var, B, precond, tol, 1000, record=True)
    assert torch.equal(x0, x1) and i0["iterations"] == i1["iterations"] and i0["restarts"] == i1["restarts"] == 0
    assert "coef" not in i0 and "rz0" not in i0
    coef, steps = i1["coef"], i1["lanczos_steps"]
    print("recorded solve: %d iterations, lanczos_steps %r, rz0 %r" % (i1["iterations"], steps, i1["rz0"]))
    assert coef.shape == (i1["iterations"], 2, 3) and steps.tolist() == [i1["iterations"], i1["iterations"], 0]
    assert np.all(coef[:, 0, :2] > 0) and np.isnan(coef[:, :, 2]).all() and i1["rz0"][2] == 0.0
    assert abs(i1["rz0"][1] / i1["rz0"][0] - 4.0) <= 1e-12 and np.abs(coef[:, 0, 1] / coef[:, 0, 0] - 1).max() <= 1e-9


# ---------------------------------------------------------------- value and gradient
@pytest.mark.parametrize("rank", [0, 16])
def test_float64_orthogonal_probes_against_the_dense_algebra(rank):
    """N = 48, P = 2, probes sqrt(N) chol(P_)^T with P_ from exact_gp_ref.factor, tol 1e-6: the estimator is then exact up
    to the solves, and the value and every gradient component are within 1e-5 of their terms' magnitudes of mll_dense."""
    X, Y, C, Z, (ref, gref, mag) = _small(rank)
    m, gp = _gp(X, Y, ELL, "float64")
    value, grad, info = gp.log_marginal_likelihood_and_grad(X, Y, NOISE, k_var=K_VAR, precond_rank=rank, tol=1e-6, probes=Z)
    rat = _ratios(value, grad, ref, gref, mag)
    print("float64 rank %d (used %d): value %.6f (dense %.6f), %d iterations, logdet %.6f; error / magnitude %r"
          % (rank, info["precond_rank"], value, ref, info["iterations"], info["logdet"], rat))
    assert info["precond_rank"] == rank and info["num_probes"] == 48 and info["lanczos_steps"].shape == (48,)
    assert grad["lengthscales"].shape == (2,) and grad["lengthscales"].dtype == np.float64
    assert all(v <= 1e-5 for v in rat.values())
    only = gp.log_marginal_likelihood(X, Y, NOISE, k_var=K_VAR, precond_rank=rank, tol=1e-6, probes=Z)
    assert only == value


def test_float64_gaussian_probes_against_the_same_probe_estimator():
    """plane_case(300), 16 injected Gaussian probes, rank 64: value and gradient equal exact_mll_ref.mll_estimate on the
    same probes within 1e-5 of the terms' magnitudes; the two solves may stop an iteration apart, so the steps each
    probe contributed are within 2 of the restatement's."""
    X, Y, ell, k_var, noise_var, Z, (_, _, mag), (ref, gref, rinfo) = _plane()
    m, gp = _gp(X, Y, ell, "float64")
    value, grad, info = gp.log_marginal_likelihood_and_grad(X, Y, noise_var, k_var=k_var, precond_rank=64, probes=Z)
    rat = _ratios(value, grad, ref, gref, mag)
    print("float64 same-probe estimator: value %.6f (numpy %.6f), logdet %.6f (numpy %.6f), steps %r (numpy %r); error / "
          "magnitude %r" % (value, ref, info["logdet"], rinfo["logdet"], info["lanczos_steps"], rinfo["lanczos_steps"], rat))
    assert np.abs(info["lanczos_steps"] - rinfo["lanczos_steps"]).max() <= 2
    assert abs(info["logdet_precond"] - rinfo["logdet_precond"]) <= 1e-8 * abs(rinfo["logdet_precond"])
    assert all(v <= 1e-5 for v in rat.values())


def test_float32_at_its_default_tolerance():
    """The same two cases in a float32 session at tol 1e-3: errors against mll_dense (orthogonal probes, rank 0 and rank
    16) and against mll_estimate (Gaussian probes, rank 64) below F32_FACTOR x tol x magnitude.
    The orthogonal probes must have the covariance of the preconditioner THE SESSION builds, and a float32 session does not
    take the pivots of exact_gp_ref.factor: with ell = (0.5, 0.7) on [0, 5]^2 the conditional variances of far-apart points
    round to exactly 1 in float32 and tie to the lowest index (pivots 0, 1, 2, 16, ... where float64 takes 0, 1, 13, 33,
    ...) -- both valid factors.  So the small case at rank 16 reads the float32 session's pivots (hb_sgp_select) and builds P_ in
    numpy float64 along them (exact_mll_ref.factor_along); the reference stays mll_dense.  (With probes from the float64
    pivots the float32 estimate is off by 258 / 144 / 239 / 52 x tol x magnitude -- value, lengthscales, k_var, noise_var --
    and the numpy estimator given the same mismatched factor reproduces those figures to four digits: the probes, not the
    arithmetic.)  Observed on MI355X, error / (tol x magnitude), value / lengthscales / k_var / noise_var: small rank 0 0.0016 / 0.048 /
    0.014 / 0.015, rank 16 0.0008 / 0.040 / 0.036 / 0.13, plane 0.0014 / 0.095 / 0.11 / 0.062; F32_FACTOR = 1.0 is about 10 x the worst."""
    worst = {}
    dev32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    for rank in (0, 16):
        X, Y, _, Z, (ref, gref, mag) = _small(rank)          # rank 0: no factor, P_ = I, Z = sqrt(N) I
        m, gp = _gp(X, Y, ELL, "float32")
        C, idx = None, None
        if rank:
            idx = H.sgp_select(dev32(X), dev32(ELL), rank)[0].cpu().numpy()
            C = R.factor_along(X, ELL, idx)
            Z = R.orthogonal_probes(R.precond_dense(X, C, K_VAR, NOISE))
        value, grad, info = gp.log_marginal_likelihood_and_grad(X, Y, NOISE, k_var=K_VAR, precond_rank=rank, probes=Z)
        worst["small rank %d" % rank] = _ratios(value, grad, ref, gref, mag)
        print("float32 small rank %d: pivots %r, %d iterations, %d restarts, rank used %d, logdet %.6f (dense %.6f), "
              "logdet_precond %.6f (numpy %.6f), steps %r"
              % (rank, idx, info["iterations"], info["restarts"], info["precond_rank"], info["logdet"],
                 np.linalg.slogdet(E.dense(X, ELL, K_VAR, NOISE))[1], info["logdet_precond"],
                 R.logdet_precond(C, K_VAR, NOISE, 48), info["lanczos_steps"]))
        assert info["precond_rank"] == rank
        assert abs(info["logdet_precond"] - R.logdet_precond(C, K_VAR, NOISE, 48)) <= 1e-3
    X, Y, ell, k_var, noise_var, Z, (_, _, mag), (ref, gref, rinfo) = _plane()
    m, gp = _gp(X, Y, ell, "float32")
    value, grad, info = gp.log_marginal_likelihood_and_grad(X, Y, noise_var, k_var=k_var, precond_rank=64, probes=Z)
    worst["plane"] = _ratios(value, grad, ref, gref, mag)
    print("float32 plane: %d iterations, %d restarts, steps %r (numpy at 1e-6: %r)"
          % (info["iterations"], info["restarts"], info["lanczos_steps"], rinfo["lanczos_steps"]))
    for name, rat in worst.items():
        print("float32 %s: error / (tol x magnitude) %r" % (name, {k: v / 1e-3 for k, v in rat.items()}))
    assert all(v <= F32_FACTOR * 1e-3 for rat in worst.values() for v in rat.values())


def test_default_probes_are_a_function_of_the_seed():
    """Device-drawn probes: two evaluations with one seed are bitwise equal, another seed gives another estimate, and 16
    probes land within the estimator's spread of the dense value (|error| <= 0.1 of the value's magnitude: the spread seen
    with 16 probes is a few nats in hundreds)."""
    X, Y, ell, k_var, noise_var, _, (ref, _, mag), _ = _plane()
    m, gp = _gp(X, Y, ell, "float64")
    a = gp.log_marginal_likelihood_and_grad(X, Y, noise_var, k_var=k_var, seed=3)
    b = gp.log_marginal_likelihood_and_grad(X, Y, noise_var, k_var=k_var, seed=3)
    c = gp.log_marginal_likelihood(X, Y, noise_var, k_var=k_var, seed=4)
    d = gp.log_marginal_likelihood(X, Y, noise_var, k_var=k_var, seed=3, precond_rank=0, num_probes=8)
    print("seeded probes: %.4f, %.4f (seed 4), %.4f (no preconditioner, 8 probes); dense %.4f" % (a[0], c, d, ref))
    assert a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in a[1]) and c != a[0]
    assert max(abs(a[0] - ref), abs(c - ref), abs(d - ref)) <= 0.1 * mag["value"]


# ---------------------------------------------------------------- the model
def test_fit_hyper_climbs_the_marginal_likelihood():
    """plane_case(300) from ell = 1.5, k_var = 0.3, var = 0.5, 40 steps at lr 0.05, float64: 41 finite trace entries, and the
    DENSE log marginal likelihood at the final parameters is at least 50 nats above the one at the start.  (The numpy
    restatement's own ascent -- exact_mll_ref.adam_ascent, same transforms, steps and rate -- climbs 243.2 nats, from
    -209.06 to 34.12, on the dense objective, and as far on mll_estimate with 16 fixed probes at rank 64.)"""
    X, Y, _, _, _ = E.plane_case(300)
    m = ExactGPR(X=X, Y=Y, dtype="float64")
    m.gp.kern.lengthscales = np.ones(1) * 1.5
    m.k_var = np.ones(1) * 0.3
    m.var = np.ones(1) * 0.5
    start = R.mll_dense(X, Y, np.array([1.5]), 0.3, 0.5)[0]
    trace = m.fit_hyper(40, lr=0.05)
    ell, k_var, var = (np.ravel(v.value).astype(np.float64) for v in m._hyper_variables().values())
    end = R.mll_dense(X, Y, ell, float(k_var[0]), float(var[0]))[0]
    print("fit_hyper: trace %.3f -> %.3f, dense %.3f -> %.3f (+%.3f); ell %.4f k_var %.4f var %.4f"
          % (trace[0], trace[-1], start, end, end - start, ell[0], k_var[0], var[0]))
    assert trace.shape == (41,) and np.all(np.isfinite(trace))
    assert end - start >= 50.0
    assert m.posterior is not None and m.posterior.info["converged"]
    assert m.posterior.k_var == float(k_var[0]) and m.posterior.noise_var == float(var[0])


def test_the_objective_refuses_what_it_does_not_cover():
    X, Y, _, _, _ = E.plane_case(48)
    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Host(kern=hb.gp.kernels.UnitMatern32(np.ones(1)), dtype="float64").gp.log_marginal_likelihood(X, Y, 0.01)
    host = Host(kern=hb.gp.kernels.UnitRBF(np.ones(1)), dtype="float64")
    with pytest.raises(ValueError, match="probes"):
        host.gp.log_marginal_likelihood(X, Y, 0.01, probes=np.ones((3, 47)))
    with pytest.raises(ValueError, match="num_probes"):
        host.gp.log_marginal_likelihood(X, Y, 0.01, num_probes=0)
    with pytest.raises(hb.gp.NotConverged):
        host.gp.log_marginal_likelihood(X, Y, 0.01, precond_rank=0, max_iter=2)
