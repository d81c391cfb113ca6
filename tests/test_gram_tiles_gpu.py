"""Tiles mode of the Gram VJP inside the product that computes Kbar (hb_matmul_gram_vjp_tiles_f32) and the fold of its tile
partials (hb_gram_tiles_fold_f32), and the planner pairing that puts the fold at the head of the step's last serial chain.

Kernel level: S, Xbar and ellbar against tests/gram_ref.py in float64 and against hb_matmul followed by the one-pass
symmetric hb_gram_bwd, with the error measure and bound of test_kernels_gpu.py's
test_gram_vjp_inside_the_product_that_computes_kbar (max |a - b| / max |a| <= 2e-5; S keeps its bits); one case leaves S
unstored; determinism.  Model level (the sizes of tests/test_phi_direct_gpu.py): objective, gradients, ledger, launches,
captured against eager, hoisted chain against plain chain."""
import numpy as np
import pytest
import torch

import gram_ref as GR
import henbun_amd as hb
import test_phi_direct_gpu as PD
from henbun_amd import graph as G
from parity import observe, rel_err, tile_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
BOUND = 2e-5      # test_gram_vjp_inside_the_product_that_computes_kbar's; it observed <= 3e-6


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).cuda().contiguous()


def host(t):
    return t.detach().double().cpu().numpy()


def _case(H, B, M, d, dl):
    rng = np.random.RandomState(B * 1000 + M + d)
    X = dev(np.sort(rng.uniform(0, 8.0, (M, d)), axis=-2))
    ell = dev(0.7 + rng.rand(dl))
    Wl = dev(np.tril(rng.randn(M, M)) / np.sqrt(M))
    P = rng.randn(M, M)
    P = dev(P + P.T)
    T1 = H.matmul(Wl, P, transA=True)                      # W^T P
    return X, ell, Wl, T1


def _tiles(H, T1, Wl, X, ell, M, d, dl, store):
    S = torch.full((M, M), float("nan"), dtype=F32, device="cuda") if store else None
    xb, lb = torch.full_like(X, float("nan")), torch.full_like(ell, float("nan"))
    part = torch.full((H.matmul_gram_vjp_ws_elems(1, M, d),), float("nan"), dtype=F32, device="cuda")
    H.matmul_gram_vjp_tiles(T1, Wl, S, False, False, X, 0, ell, 0, dl, d, part)
    H.gram_tiles_fold(part, 1, M, d, dl, xb, lb)
    torch.cuda.synchronize()
    return S, xb, lb, part


@pytest.mark.parametrize("B,M,d,dl,store", [(1, 128, 1, 1, True), (1, 128, 2, 2, False), (1, 256, 3, 1, True), (1, 256, 4, 4, True)])
def test_tiles_mode_against_fp64_and_the_two_launch_path(H, B, M, d, dl, store):
    """M = K = 128 is the smallest in-workgroup split-K product (16 tiles, four per row); 256 gives eight tiles per row and,
    with d = 3 / 4, two outputs per thread of the one-workgroup fold.  T random and W lower triangular: S = T W is symmetric
    to rounding only.  store=False: C == NULL, S is never written."""
    X, ell, Wl, T1 = _case(H, B, M, d, dl)
    assert H.matmul_gram_vjp_tiles_ok(M, M, B, d, F32)
    S0 = H.matmul(T1, Wl)                                  # (W^T P) W
    xb0, lb0 = torch.empty_like(X), torch.empty_like(ell)
    ws = torch.empty(M * d, dtype=F32, device="cuda")
    H.gram_bwd_raw(H.KERN_RBF | H.KERN_KBAR_SYMMETRIC, X, 0, X, 0, ell, 0, dl, S0, xb0, xb0, lb0, 1, M, M, d, ws)
    S1, xb1, lb1, part = _tiles(H, T1, Wl, X, ell, M, d, dl, store)
    assert torch.isfinite(part).all() and torch.isfinite(xb1).all() and torch.isfinite(lb1).all()
    # float64: the product, and the VJP of the device's own S (what the epilogue held in registers)
    Sref = host(T1) @ host(Wl)
    (gx, gx2, gl), _ = GR.gram_vjp(GR.RBF, host(X)[None], host(X)[None], host(ell)[None], host(S0)[None])
    gl = gl.sum(0) if dl == d else gl.sum(keepdims=True).reshape(1)
    tag = "gram_tiles/kernel[M%d,d%d,dl%d]/" % (M, d, dl)
    print(tag, "S %.3e  Xbar %.3e %.3e  ellbar %.3e %.3e" % (rel_err(S0, Sref), rel_err(xb1, (gx + gx2)[0]), rel_err(xb1, xb0),
                                                          rel_err(lb1, gl), rel_err(lb1, lb0)))
    if store:
        assert torch.equal(S1, S0)                         # the product keeps its bits
        observe(tag + "S/fp64", rel_err(S1, Sref), BOUND)
    observe(tag + "Xbar/fp64", rel_err(xb1, (gx + gx2)[0]), BOUND)
    observe(tag + "ellbar/fp64", rel_err(lb1, gl), BOUND)
    observe(tag + "Xbar/two_launches", rel_err(xb1, xb0), BOUND)
    observe(tag + "ellbar/two_launches", rel_err(lb1, lb0), BOUND)


def test_tiles_rule_refuses_what_the_fold_cannot_take(H):
    assert H.matmul_gram_vjp_tiles_ok(512, 512, 1, 1, F32) and H.matmul_gram_vjp_ws_elems(1, 512, 1) == 16384
    assert not H.matmul_gram_vjp_tiles_ok(128, 128, 1, 5, F32)          # d = 5
    assert not H.matmul_gram_vjp_tiles_ok(512, 512, 8, 1, F32)          # the batched benchmark shape: 131072 partials
    assert H.matmul_gram_vjp_tiles_ok(128, 128, 16, 1, F32) and not H.matmul_gram_vjp_tiles_ok(128, 128, 17, 1, F32)


def test_tiles_mode_is_deterministic(H):
    M, d, dl = 256, 3, 1
    X, ell, Wl, T1 = _case(H, 1, M, d, dl)
    _, xa, la, pa = _tiles(H, T1, Wl, X, ell, M, d, dl, True)
    _, xb, lb, pb = _tiles(H, T1, Wl, X, ell, M, d, dl, False)
    assert torch.equal(pa, pb) and torch.equal(xa, xb) and torch.equal(la, lb)


# ------------------------------------------------------------------------------------------------ model level
def _ledger(plan):
    return [e for e in plan.explain if e[0] == G.GRAM_TILES]


def _launches(plan):
    """Launches of one run of the plan, from its step list: one per step, and one more for a serial chain whose first member
    is a "tail" step -- such a step issues its own kernel (the Gram VJP: gram_bwd_side_kernel) in front of the chain and only
    its last small launch joins it.  (plan.steps itself counts the gram_grad step in both forms.)"""
    n = 0
    for s in plan.steps:
        members = plan.chain_members.get(id(s))
        n += 1 + (1 if members and plan.chain_kind.get(id(members[0])) == "tail" else 0)
    return n


@pytest.fixture(scope="module")
def fp32_case(H):
    with PD.settings_with():
        m, data = PD.make_svgp("float32")
        opt = m.ELBO()
        opt.compile()
        res = {}
        for on in (1, 0):
            H.debug_set("gram_vjp_tiles", on)      # read when the plan is built
            try:
                v, g = opt.gradients(minibatch_size=PD.MB, indices=data[5])
                plan = opt.last_plan
            finally:
                H.debug_clear()
            plan.run()
            res[on] = dict(val=v, grads=g, ledger=_ledger(plan), launches=_launches(plan),
                           labels=[plan.step_labels.get(id(s), "other") for s in plan.steps], again=float(plan.value(plan.outputs[0])))
        ref_val, ref = PD.oracle(m, data)
    return res, ref_val, ref


def test_ledger_reports_the_pairing_and_the_step_loses_a_launch(fp32_case):
    res, _, _ = fp32_case
    on, off = res[1], res[0]
    assert len(on["ledger"]) == 1 and on["ledger"][0][2], on["ledger"]
    assert len(off["ledger"]) == 1 and not off["ledger"][0][2] and "gram_vjp_tiles" in off["ledger"][0][3], off["ledger"]
    assert on["launches"] == off["launches"] - 1, (on["labels"], off["labels"])
    assert on["again"] == on["val"] and off["again"] == off["val"]


def test_step_with_the_tile_fold_against_the_oracle_and_the_switched_off_step(fp32_case):
    res, ref_val, ref = fp32_case
    on, off = res[1], res[0]
    assert on["val"] == off["val"], "the forward is untouched: the ELBO must be bit-identical"
    observe("gram_tiles/model/ELBO", abs(on["val"] - ref_val) / abs(ref_val), PD.BOUND_ELBO)
    for mine, theirs in PD.NAMES:
        e_on, e_off = tile_err(on["grads"][mine], ref[theirs]), tile_err(off["grads"][mine], ref[theirs])
        print("gram_tiles/model %-28s on %.3e   off %.3e" % (mine, e_on, e_off))
        observe("gram_tiles/model/off/" + mine, e_off, PD.BOUND[mine])
        observe("gram_tiles/model/on/" + mine, e_on, PD.BOUND[mine])
        if mine not in ("model.gp.z", "model.gp.kern.lengthscales"):     # only these two pass through the Gram VJP
            assert np.array_equal(np.asarray(on["grads"][mine]), np.asarray(off["grads"][mine])), mine


_TRAINED = {}      # (capture, hoist) -> the parameters after three steps


@pytest.mark.parametrize("capture,hoist", [(True, 1), (False, 1), (True, 0)])
def test_training_steps_agree_captured_eager_and_with_the_plain_chain(H, capture, hoist):
    """Three Adam steps with the fold at the head of the update's chain: replayed from a captured graph, launched eagerly,
    and with the chain generated in its plain form (every job loads after its barrier; no LDS hand-off) -- the same
    arithmetic in the same order, so the same parameters bit for bit."""
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = PD.JITTER
    cfg.runtime.graph_capture = capture
    with hb.settings.temp_settings(cfg):
        m, data = PD.make_svgp("float32")
        opt = m.ELBO()
        opt.compile()
        H.debug_set("chain_hoist", hoist)
        try:
            opt.optimize(maxiter=3, minibatch_size=PD.MB, indices=data[5])
            plan = opt.last_plan
            torch.cuda.synchronize()
        finally:
            H.debug_clear()
        assert len(_ledger(plan)) == 1 and _ledger(plan)[0][2]
        assert any(l.startswith("chain[gram_grad+") for l in (plan.step_labels.get(id(s), "") for s in plan.steps))
        theta = m._session.theta.clone()
    assert torch.isfinite(theta).all()
    _TRAINED[(capture, hoist)] = theta
    first = next(iter(_TRAINED.values()))
    assert torch.equal(theta, first), (capture, hoist)
