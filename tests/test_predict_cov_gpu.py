"""SparseGP.predict_f(full_cov=True) and predict_f_samples on the MI355X: hb_sgp_predict_cov (fp32 MFMA kernel, fp64 loop)
against an fp64 reference written here from the definition,

    A = Lm^-1 K(z, x),  u ~ N(m, S S^T):
    cov_p = A^T S_p S_p^T A + K(x, x) - A^T A + jitter I   ('fullrank')
          = A^T S_p S_p^T A + diag(|1 - colsum A^2|)       ('diagonal')
          = A^T S_p S_p^T A                                ('neglected'),

with Lm and K from henbun_oracle; bitwise symmetry; diag(cov) against predict_f's var; the generic composition; joint
draws against their mean and covariance; the full size (n = 8192, M = 512) with its memory bound; the SVGP helpers."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
import henbun_oracle as O
from henbun_amd import graph as G
from henbun_amd.models import SVGP, svgp_data
from parity import observe, rel_err, tile_err
from test_predict_gpu import G_, N_, _build, _values

pytestmark = pytest.mark.gpu
tf = hb.tf
FUSED = "fused predictive covariance"
JIT = 1e-3


def _factors(x, z, ell, mu, sq, scale, packed, q, jitter):
    """fp64 (A_e, S_ep) per expert / latent function, from henbun_oracle's Gram (difference form) and Cholesky."""
    shape = list(q._shape)
    P, M = shape[-2], shape[-1]
    E = z.shape[0] if z.ndim == 3 else 1
    z3 = z.reshape(E, M, -1)
    ell2 = ell.reshape(E, -1) if ell.ndim == 2 else np.broadcast_to(ell, (E, ell.size))
    if q.q_shape == "diagonal":
        s = scale * np.exp(sq).reshape(E, P, M)
    else:
        S = scale * (O.vec_to_tri(O.T(sq)).numpy() if packed else np.tril(sq))
    xt = O.T(x)
    out = []
    for e in range(E):
        zt, lt = O.T(z3[e]), O.T(ell2[e])
        Lm = O.kern_cholesky(zt, lt, jitter, K=O.rbf_K_difference)
        A = torch.linalg.solve_triangular(Lm, O.rbf_K_difference(zt, xt, lt), upper=False).numpy()
        Ss = [np.diag(s[e, p]) if q.q_shape == "diagonal" else S[(e * P + p) * M:(e * P + p + 1) * M, :] for p in range(P)]
        out.append((A, Ss, lt))
    return out


def reference_cov(x, z, ell, mu, sq, scale, packed, q, mode, jitter, rows=None):
    """fp64 covariance [E?, P, n, n] (or its rows `rows`) from the definition."""
    E = z.shape[0] if z.ndim == 3 else 1
    res = []
    for A, Ss, lt in _factors(x, z, ell, mu, sq, scale, packed, q, jitter):
        Ar = A if rows is None else A[:, rows]
        n, nr = A.shape[1], Ar.shape[1]
        per = []
        for Sp in Ss:
            C, Cr = Sp.T @ A, Sp.T @ Ar
            cov = Cr.T @ C
            eye = np.eye(n)[rows] if rows is not None else np.eye(n)
            if mode == "fullrank":
                xr = x if rows is None else x[rows]
                cov = cov + O.rbf_K_difference(O.T(xr), O.T(x), lt).numpy() - Ar.T @ A + jitter * eye
            elif mode == "diagonal":
                cov = cov + eye * np.abs(1.0 - (Ar * Ar).sum(0))[:, None]
            per.append(cov)
        res.append(np.stack(per))
    res = np.stack(res)
    return res if z.ndim == 3 else res[0]


def _plan(m, q, x, mode, fused=True, jitter=JIT, chol=False):
    """(mean, var, cov, notes) of one plan (cholesky(cov) in it too when `chol`: plan.check() then covers it)."""
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = jitter
    cfg.runtime.fused_predict = fused
    with hb.settings.temp_settings(cfg):
        xs = G.as_tensor(x)
        with m.tf_mode():
            mean, var = m.gp.predict_f(xs, q, q_shape=mode)
            mean2, cov = m.gp.predict_f(xs, q, q_shape=mode, full_cov=True)
            outs = [mean, var, cov] + ([G.cholesky(cov)] if chol else [])
        assert mean2 is mean
        plan = m._session.make_plan(outs)
        plan.run()
        plan.check()
        notes = [e for e in plan.explain if e[0].startswith(FUSED)]
        return plan.value(plan.outputs[0]), plan.value(plan.outputs[1]), plan.value(plan.outputs[2]), notes


CASES = [
    dict(d=1, M=64, n=333, E=1, P=1, cls=N_, qs="diagonal", packed=False, mode="fullrank"),
    dict(d=2, M=512, n=1001, E=1, P=3, cls=N_, qs="diagonal", packed=False, mode="diagonal"),
    dict(d=3, M=64, n=1001, E=4, P=1, cls=G_, qs="diagonal", packed=False, mode="neglected"),
    dict(d=1, M=512, n=2049, E=1, P=1, cls=N_, qs="fullrank", packed=False, mode="fullrank"),
    dict(d=2, M=64, n=333, E=1, P=1, cls=N_, qs="fullrank", packed=True, mode="diagonal"),
    dict(d=1, M=64, n=1001, E=4, P=3, cls=G_, qs="diagonal", packed=False, mode="fullrank"),
    dict(d=3, M=512, n=333, E=1, P=1, cls=G_, qs="fullrank", packed=False, mode="neglected"),
]


# fp32 bounds per case, <= 10x the values observed on the MI355X (rel, tile, diag-vs-var):
#   rel  1.1e-5 9.7e-6 4.3e-6 6.7e-5 1.2e-5 7.9e-6 8.4e-6;  tile 7.7e-6 8.8e-6 5.8e-6 1.8e-4 6.2e-6 1.0e-5 1.5e-5;
#   diag 2.4e-7 1.4e-6 5.1e-7 2.0e-6 6.7e-7 3.4e-7 1.6e-6
TOL_REL = [1e-4, 9e-5, 4e-5, 6e-4, 1e-4, 7e-5, 8e-5]
TOL_TILE = [7e-5, 8e-5, 5e-5, 1.5e-3, 6e-5, 1e-4, 1.5e-4]
TOL_DIAG = [2e-6, 1e-5, 5e-6, 2e-5, 6e-6, 3e-6, 1.5e-5]
# fused against the generic composition (cases 0, 3, 4, 5), observed rel 4.4e-6 3.5e-5 1.9e-6 4.6e-6,
# tile 4.9e-6 8.9e-5 2.7e-6 5.7e-6
TOL_GEN = {0: (4e-5, 4.5e-5), 3: (1e-4, 8e-4), 4: (1.8e-5, 2.5e-5), 5: (4e-5, 5e-5)}


def _sym(c):
    return np.array_equal(c, np.swapaxes(c, -1, -2))


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_fused_cov_fp32_and_fp64_match_the_definition(ci):
    case = CASES[ci]
    mode = case["mode"]
    m, q, x = _build("float32", case)
    mean, var, cov, notes = _plan(m, q, x, mode, chol=mode == "fullrank")
    assert notes and all(e[2] for e in notes), notes
    lead = ((case["E"],) if case["E"] > 1 else ()) + (case["P"], case["n"], case["n"])
    assert cov.shape == lead and _sym(cov)
    z, ell, mu, sq, scale, packed = _values(m, q)
    ref = reference_cov(x.astype(np.float32).astype(np.float64), z, ell, mu, sq, scale, packed, q, mode, JIT)
    # fp32 against fp64: dominated by the fp32 factorisation of Kmm + jitter I that A is formed from (as for predict_f);
    # tile_err: a wrong mirrored or edge tile reads ~1
    observe("predict cov fp32 rel case %d" % ci, rel_err(cov, ref), TOL_REL[ci])
    observe("predict cov fp32 tile case %d" % ci, tile_err(cov, ref), TOL_TILE[ci])
    # diag(cov) against predict_f's var from the same plan (same A, different summation order)
    observe("predict cov fp32 diag-vs-var case %d" % ci, rel_err(np.diagonal(cov, axis1=-2, axis2=-1), var), TOL_DIAG[ci])
    m64, q64, _ = _build("float64", case)
    mean64, var64, cov64, _ = _plan(m64, q64, x, mode, chol=mode == "fullrank")
    assert _sym(cov64)
    z, ell, mu, sq, scale, packed = _values(m64, q64)
    ref = reference_cov(x, z, ell, mu, sq, scale, packed, q64, mode, JIT)
    assert rel_err(cov64, ref) <= 1e-9, rel_err(cov64, ref)
    assert rel_err(np.diagonal(cov64, axis1=-2, axis2=-1), var64) <= 1e-12


@pytest.mark.parametrize("ci", [0, 3, 4, 5])
def test_fused_cov_agrees_with_the_generic_composition(ci):
    case = dict(CASES[ci], n=300)
    m, q, x = _build("float32", case, seed=3)
    _, _, fc, notes = _plan(m, q, x, case["mode"])
    assert notes and all(e[2] for e in notes)
    _, _, gc, notes = _plan(m, q, x, case["mode"], fused=False)
    assert not notes
    # the same factor W (the composition's L^-1 K is the trinv node the moments read); only the sums differ
    observe("predict cov fused-vs-generic case %d" % ci, rel_err(fc, gc), TOL_GEN[ci][0])
    observe("predict cov fused-vs-generic tile case %d" % ci, tile_err(fc, gc), TOL_GEN[ci][1])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("qs, mode", [("fullrank", "fullrank"), ("diagonal", "diagonal")])
def test_joint_draws_have_the_predicted_mean_and_covariance(dtype, qs, mode):
    case = dict(d=1, M=64, n=48, E=1, P=1, cls=N_, qs=qs, packed=False, mode=mode)
    m, q, x = _build(dtype, case, seed=5)
    mean, _, cov, _ = _plan(m, q, x, mode)
    S = 20000
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = JIT
    with hb.settings.temp_settings(cfg):
        with m.tf_mode():
            f = m.gp.predict_f_samples(x, q, S, q_shape=mode)
            _, cov_t = m.gp.predict_f(x, q, q_shape=mode, full_cov=True)
        plan = m._session.make_plan([f, cov_t])
    plan.run()
    plan.check()
    d1 = np.array(plan.value(plan.outputs[0]), dtype=np.float64, copy=True)
    plan.run()
    plan.check()
    d2 = np.array(plan.value(plan.outputs[0]), dtype=np.float64, copy=True)
    assert d1.shape == (1, S, 48) and not np.array_equal(d1, d2)
    assert q._draw is None
    d1, mean, cov = d1[0], mean[0].astype(np.float64), cov[0].astype(np.float64)
    v = np.diagonal(cov)
    z_mean = np.abs(d1.mean(0) - mean) / np.sqrt(v / S)
    assert z_mean.max() < 5.0, z_mean.max()
    # each entry of the sample covariance has standard deviation sqrt((C_ii C_jj + C_ij^2) / (S - 1)); 6 of them over
    # the 1176 distinct entries
    scov = np.cov(d1, rowvar=False)
    sd = np.sqrt((v[:, None] * v[None, :] + cov * cov) / (S - 1))
    z_cov = np.abs(scov - cov) / sd
    assert z_cov.max() < 6.0, z_cov.max()


@pytest.mark.parametrize("qs, mode", [("diagonal", "fullrank"), ("fullrank", "diagonal")])
def test_full_size_and_memory(qs, mode):
    """fp32, n = 8192, M = 512: 64 random rows against fp64; the peak extra device memory is cov plus the predicted
    workspace (plus the small moments / factorisation buffers)."""
    case = dict(d=1, M=512, n=8192, E=1, P=1, cls=N_, qs=qs, packed=False, mode=mode)
    m, q, x = _build("float32", case, seed=11)
    n, M = 8192, 512
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = JIT
    with hb.settings.temp_settings(cfg):
        with m.tf_mode():
            _, cov_t = m.gp.predict_f(x, q, q_shape=mode, full_cov=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        plan = m._session.make_plan([cov_t])
        plan.run()
        plan.check()
        torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    ws = hb.hip_ops.sgp_predict_cov_ws_elems(torch.float32, 1, n, M, 1, 0 if qs == "diagonal" else 1) * 4
    small = 16 * 2 ** 20          # x, the Gram / factor / inverse of z and its fragment images, mean / var, q's factor
    assert rise <= n * n * 4 + ws + small, (rise / 2 ** 20, (n * n * 4 + ws) / 2 ** 20)
    notes = [e for e in plan.explain if e[0].startswith(FUSED)]
    assert notes and all(e[2] for e in notes)
    cov = plan.value(plan.outputs[0])
    assert _sym(cov)
    rows = np.sort(np.random.RandomState(0).choice(n, 64, replace=False))
    z, ell, mu, sq, scale, packed = _values(m, q)
    ref = reference_cov(x.astype(np.float32).astype(np.float64), z, ell, mu, sq, scale, packed, q, mode, JIT, rows=rows)
    # observed: rel 7.1e-5 / 7.1e-5, tile 8.0e-5 / 1.6e-4 (diagonal / full-rank S)
    observe("predict cov full size rel " + qs, rel_err(cov[:, rows], ref), 6e-4)
    observe("predict cov full size tile " + qs, tile_err(cov[:, rows], ref), 7e-4 if qs == "diagonal" else 1.5e-3)


def test_svgp_full_cov_and_draws():
    np.random.seed(0)
    X, Y, Z = svgp_data(3000, 48, 0)
    m = SVGP(X=X, Y=Y, Z=Z, dtype="float64")
    m.ELBO().compile(optimizer=tf.train.AdamOptimizer(0.01))
    m.ELBO().optimize(maxiter=100, minibatch_size=512)
    xs = np.linspace(0, 24, 50)[:, None]
    fm, fv = m.predict_f(xs)
    cm, cov = m.predict_f(xs, full_cov=True)
    assert cm.shape == (1, 50) and cov.shape == (1, 50, 50) and _sym(cov)
    assert np.array_equal(cm, fm)
    assert rel_err(np.diagonal(cov, axis1=-2, axis2=-1), fv) <= 1e-12
    s = m._session
    k_var = float(s.read_value(object.__getattribute__(m, "k_var"))[0])
    q = object.__getattribute__(m, "u")
    z, ell, mu, sq, scale, packed = _values(m, q)
    ref = reference_cov(xs, z, ell, mu, sq, scale, packed, q, "diagonal", hb.settings.numerics.jitter_level)
    assert rel_err(cov, ref * k_var) <= 1e-10
    S = 4000
    f = m.predict_f_samples(xs, S)
    assert f.shape == (S, 50)
    z_mean = np.abs(f.mean(0) - fm[0]) / np.sqrt(fv[0] / S)
    assert z_mean.max() < 5.0, z_mean.max()
    assert np.abs(f.var(0, ddof=1) / fv[0] - 1.0).max() < 6.0 * np.sqrt(2.0 / (S - 1))
