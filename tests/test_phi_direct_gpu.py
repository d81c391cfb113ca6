"""hb_sgp_bwd_phi_f32 and the planner pairing that uses it.

The Cholesky VJP's first product, Phisym(L^T tril(Lbar)) with Lbar = -tril(W^T Abar A^T), equals Phisym(-Abar A^T)
(tests/test_phi_direct_cpu.py): the sparse-GP backward leaves the fragment-major image of Abar instead of Kbar's, the
Lbar contraction kernels form Abar A^T, and the finish pass writes Phisym -- both triangles -- where it wrote Lbar.

Kernel level: the result against the float64 value formed from the device's own A and v; ubar / zbar / ellbar bit for bit
those of hb_sgp_bwd_f32; determinism.  Model level: the ledger entry, one product fewer in the plan, both gradients
against the float64 oracle, and the three shapes of graph that must keep the unpaired path."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
import henbun_oracle as O

from henbun_amd import graph as G
from henbun_amd.models import SVGP, svgp_data
from parity import observe, tile_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
PASS = G.PHI_DIRECT


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).cuda().contiguous()


def host(t):
    return t.detach().double().cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("E,M,n,d,P", [(1, 96, 70, 2, 3),       # three row tiles (an odd count), a ragged last strip
                                       (1, 128, 257, 1, 1),     # nine strips, one column in the last
                                       (2, 64, 96, 1, 1),       # batched
                                       (8, 512, 2048, 1, 1)])   # pairs * E >= 256 and nS >= 64: sgp_lbar_lds_kernel
def test_phi_kernel_against_fp64_and_the_unpaired_backward(H, E, M, n, d, P):
    rng = np.random.RandomState(11 + M + n)
    z = np.cumsum(1.5 * (0.75 + 0.5 * rng.rand(E, M, 1)), axis=1) * np.ones((1, 1, d))
    if d > 1:
        z = z + 0.3 * rng.randn(E, M, d)
    ell = np.exp(0.1 * rng.randn(E, d))
    x = z[0][rng.randint(0, M, n)] + 0.7 * rng.randn(n, d)       # one x shared by the experts
    u, eps, fbar = rng.randn(E, P, M), rng.randn(E, n), rng.randn(E, P, n)
    if E == 1:
        z, ell, u, eps, fbar = z[0], ell[0], u[0], eps[0], fbar[0]
    K = H.gram_fwd(dev(z), dev(z), dev(ell), diag_add=0.1).reshape((E, M, M) if E > 1 else (M, M))
    frag = torch.zeros(2 * E * M * M, dtype=F32, device="cuda")
    L, W, info = H.cholesky_inverse(K, frag=frag)
    assert not info.cpu().numpy().any()
    assert H.sgp_strip_path(E, n, M, d, P, H.PREC_NATIVE) and H.sgp_bwd_phi_supported(E, n, M, d, P)
    args = (dev(x), dev(z), dev(ell), W.reshape(K.shape), dev(u))
    a_frag = torch.zeros(H.sgp_frag_elems(E, n, M), dtype=F32, device="cuda")
    f, A, v, _ = H.sgp_fwd(*args, eps_in=dev(eps), wfrag=frag, a_frag=a_frag)      # row-major A as well: the reference's operand
    bargs = (dev(eps), None, v, dev(fbar))
    Lb, ub, zb, lb, _ = H.sgp_bwd(*(args + bargs), wfrag=frag, a_frag=a_frag)
    nan = lambda t: torch.full_like(t, float("nan"))
    outs = (nan(Lb), nan(ub), nan(zb), nan(lb))
    Phi, ub2, zb2, lb2 = H.sgp_bwd_phi(args[0], args[1], args[2], args[3], args[4], dev(eps), v, dev(fbar), frag, a_frag, out=outs)
    torch.cuda.synchronize()
    # the other gradients do not know which image the strip kernel stored
    assert torch.equal(ub2, ub) and torch.equal(zb2, zb) and torch.equal(lb2, lb)
    # float64 reference from the device's own A and v:  Abar = u^T fbar + A diag(c),  c = -eps sign(v) / sqrt|v| * sum_p fbar_p
    Ad, vd = host(A).reshape(E, M, n), host(v).reshape(E, n)
    ud, fd, ed = np.reshape(u, (E, P, M)), np.reshape(fbar, (E, P, n)), np.reshape(eps, (E, n))
    ud, fd, ed = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (ud, fd, ed))
    c = np.where(np.abs(vd) > 0, -ed * np.sign(vd) / np.sqrt(np.maximum(np.abs(vd), 1e-300)) * fd.sum(1), 0.0)
    Abar = np.einsum("epm,epn->emn", ud, fd) + Ad * c[:, None, :]
    Q = -np.einsum("emn,ekn->emk", Abar, Ad)
    i, j = np.indices((M, M))
    ref = 0.5 * Q[:, np.maximum(i, j), np.minimum(i, j)]
    got = host(Phi).reshape(E, M, M)
    assert np.isfinite(got).all() and np.array_equal(got, np.transpose(got, (0, 2, 1)))
    # the n-deep fp32 sum that test_fp32_parity_gpu.py bounds by 1e-5 as Lbar
    observe("phi_direct/Phi[E%d,M%d,n%d,d%d,P%d]" % (E, M, n, d, P), tile_err(got, ref), 1e-5)
    # determinism: the same call again, into fresh buffers
    Phi2, ub3, zb3, lb3 = H.sgp_bwd_phi(args[0], args[1], args[2], args[3], args[4], dev(eps), v, dev(fbar), frag, a_frag)
    assert torch.equal(Phi2.reshape(Phi.shape), Phi) and torch.equal(ub3, ub) and torch.equal(zb3, zb) and torch.equal(lb3, lb)


# ------------------------------------------------------------------------------------------------ model level
NAMES = [("model.gp.z", "z"), ("model.gp.kern.lengthscales", "ell_raw"), ("model.u.q_mu", "q_mu"),
         ("model.u.q_sqrt", "q_sqrt"), ("model.k_var", "k_var_raw"), ("model.var", "var_raw")]
# the bounds tests/test_model_gpu.py::test_cfg2_full_size_properties_fp32 applies at jitter 1e-4
BOUND_ELBO = 5e-5
BOUND = {"model.gp.z": 1e-2, "model.gp.kern.lengthscales": 1.5e-3, "model.u.q_mu": 1.8e-3, "model.u.q_sqrt": 1.6e-3,
         "model.k_var": 2e-5, "model.var": 1e-4}
JITTER = 1e-4
N, M, MB = 20000, 128, 512      # the data set and seed of the test the bounds come from; M and the minibatch reduced


def make_svgp(dtype, seed=0):
    np.random.seed(seed)
    rng = np.random.RandomState(seed)
    X, Y, Z = svgp_data(N, M, seed)
    eps = rng.randn(N)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape="diagonal", residual="diagonal", eps=eps, dtype=dtype)
    m.gp.kern.lengthscales = np.ones(1) * 0.9
    m.k_var = np.ones(1) * 1.3
    m.var = np.ones(1) * 0.4
    u = rng.randn(M)
    m.u.inject_noise(u)
    idx = rng.randint(0, N, MB)
    return m, (X, Y, Z, eps, u, idx)


def oracle(m, data):
    X, Y, Z, eps, u, idx = data
    sess = m._session
    params = {"z": O.T(sess.read_raw(m.gp.z)), "ell_raw": O.T(sess.read_raw(m.gp.kern.lengthscales)),
              "q_mu": O.T(sess.read_raw(m.u.q_mu)).reshape(1, M), "q_sqrt": O.T(sess.read_raw(m.u.q_sqrt)),
              "k_var_raw": O.T(sess.read_raw(m.k_var)), "var_raw": O.T(sess.read_raw(m.var))}
    fn = lambda p: O.svgp_elbo(p, O.T(X[idx]), O.T(Y[idx]), float(X.shape[0]), O.T(u), O.T(eps[idx]), jitter=JITTER,
                               q_shape="diagonal", residual="diagonal")
    val, ref = O.grads_of(fn, params)
    return val.item(), {k: t.numpy() for k, t in ref.items()}


def settings_with(**numerics):
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = JITTER
    for k, v in numerics.items():
        setattr(cfg.numerics, k, v)
    return hb.settings.temp_settings(cfg)


def ledger(plan):
    return [e for e in plan.explain if e[0] == PASS]


def n_products(plan):
    return sum(1 for s in plan.steps if plan.step_labels.get(id(s)) == "matmul")


@pytest.fixture(scope="module")
def fp32_case(H):
    """The fp32 model, its float64 oracle, and the gradient step with the pairing on and off (same model, same point)."""
    with settings_with():
        m, data = make_svgp("float32")
        opt = m.ELBO()
        opt.compile()
        res = {}
        for on in (1, 0):
            H.debug_set("sgp_phi_direct", on)      # read when the plan is built
            try:
                v, g = opt.gradients(minibatch_size=MB, indices=data[5])
                plan = opt.last_plan
            finally:
                H.debug_clear()
            plan.run()                             # the same plan once more
            res[on] = dict(val=v, grads=g, ledger=ledger(plan), products=n_products(plan), again=float(plan.value(plan.outputs[0])))
        ref_val, ref = oracle(m, data)
    return m, opt, data, res, ref_val, ref


def test_ledger_reports_the_pairing_and_the_plan_loses_one_product(fp32_case):
    _, _, _, res, _, _ = fp32_case
    on, off = res[1], res[0]
    assert len(on["ledger"]) == 1 and on["ledger"][0][2], on["ledger"]
    assert len(off["ledger"]) == 1 and not off["ledger"][0][2] and "sgp_phi_direct" in off["ledger"][0][3], off["ledger"]
    assert on["products"] == off["products"] - 1, (on["products"], off["products"])
    assert on["again"] == on["val"] and off["again"] == off["val"]       # a second run of the same plan: the same bits


def test_paired_step_against_the_oracle_and_the_unpaired_step(fp32_case):
    _, _, _, res, ref_val, ref = fp32_case
    on, off = res[1], res[0]
    assert on["val"] == off["val"], "the forward is untouched: the ELBO must be bit-identical"
    observe("phi_direct/model/ELBO", abs(on["val"] - ref_val) / abs(ref_val), BOUND_ELBO)
    for mine, theirs in NAMES:
        e_on = tile_err(on["grads"][mine], ref[theirs])
        e_off = tile_err(off["grads"][mine], ref[theirs])
        print("phi_direct/model %-28s paired %.3e   unpaired %.3e" % (mine, e_on, e_off))
        observe("phi_direct/model/unpaired/" + mine, e_off, BOUND[mine])
        observe("phi_direct/model/paired/" + mine, e_on, BOUND[mine])
        # the direct form drops two cond(L)-amplified products: it should be closer; the factor covers rounding luck at M = 128
        observe("phi_direct/model/paired_vs_unpaired/" + mine, e_on, 2.0 * e_off + 1e-6)


def _check_fp32_level(tag, val, grads, ref_val, ref):
    observe(tag + "ELBO", abs(val - ref_val) / abs(ref_val), BOUND_ELBO)
    for mine, theirs in NAMES:
        observe(tag + mine, tile_err(grads[mine], ref[theirs]), BOUND[mine])


def test_fp64_session_keeps_the_unpaired_path():
    with settings_with():
        m, data = make_svgp("float64")
        opt = m.ELBO()
        opt.compile()
        val, grads = opt.gradients(minibatch_size=MB, indices=data[5])
        led = ledger(opt.last_plan)
        ref_val, ref = oracle(m, data)
    assert len(led) == 1 and not led[0][2], led
    assert abs(val - ref_val) <= 1e-5 * abs(ref_val)
    for mine, theirs in NAMES:      # the bar of test_model_gpu.py::test_svgp_fp64_elbo_and_gradient_parity
        a, b = np.asarray(grads[mine], dtype=np.float64).reshape(-1), ref[theirs].reshape(-1)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), mine


def test_bf16x3_session_keeps_the_unpaired_path():
    with settings_with(contraction="bf16x3"):
        m, data = make_svgp("float32")
        opt = m.ELBO()
        opt.compile()
        val, grads = opt.gradients(minibatch_size=MB, indices=data[5])
        led = ledger(opt.last_plan)
        ref_val, ref = oracle(m, data)
    assert len(led) == 1 and not led[0][2], led
    _check_fp32_level("phi_direct/model/bf16x3/", val, grads, ref_val, ref)


def test_lbar_as_a_plan_output_keeps_the_unpaired_path(fp32_case):
    """The same fp32 step with Lbar itself requested: it has a reader besides the Cholesky VJP, so it must be formed."""
    m, opt, data, res, ref_val, ref = fp32_case
    with settings_with():
        sess = m._session
        obj = opt._trace(MB)
        leaves, names = [], []
        for v in m.get_variables(opt._collection):
            if v.is_parameter and v._leaf not in leaves:
                leaves.append(v._leaf)
                names.append(v.long_name)
        grads = G.gradients(obj, leaves)
        outs = [obj] + [g for g in grads if g is not None]
        sg = [nd for nd in G.topo_order(outs) if nd.op == "sgp_grad"]
        assert len(sg) == 1
        plan = sess.make_plan(outs + [sg[0].outputs[0]], minibatch=MB)
        plan.set_indices(data[5])
        plan.run()
        plan.check()
    led = ledger(plan)
    assert len(led) == 1 and not led[0][2] and "plan output" in led[0][3], led
    assert n_products(plan) == res[0]["products"]
    got = {nme: plan.value(g).astype(np.float64) for nme, g in zip(names, grads) if g is not None}
    _check_fp32_level("phi_direct/model/lbar_output/", float(plan.value(obj)), got, ref_val, ref)
    Lbar = plan.value(sg[0].outputs[0])
    assert np.isfinite(Lbar).all() and np.all(np.triu(Lbar.reshape(M, M), 1) == 0) and np.abs(Lbar).max() > 0
    # ... and it is the unpaired step, bit for bit
    assert float(plan.value(obj)) == res[0]["val"]
    for nme in got:
        assert np.array_equal(got[nme], res[0]["grads"][nme]), nme
