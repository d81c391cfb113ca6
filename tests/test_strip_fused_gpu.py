"""Forward and Kbar column strips in one launch (sgp_fwd_kbar_strip_kernel).

hb_sgp_fwd_gauss_kbar_f32 followed by hb_sgp_bwd_phi_rest_f32 against hb_sgp_fwd_gauss_f32 followed by hb_sgp_bwd_phi_f32
on the same inputs and the same RNG state.  No operation of either parent kernel changes and none is reordered, so every
output is held to bits: A_frag, f, v, eps_out, dmu, fbar, head_part, Abar_frag, ubar, zbar, ellbar, Phi and the advanced
RNG state.  The images and the strip partials are filled with NaN before each run so that an unwritten element shows.

Shapes (M, n, d), P = 1: one strip and two tiles; a last strip with ONE live pair of columns; nT = 6, d = 2 and a ragged
last strip; 37 strips; the benchmark's M; and an odd tile count (the middle tile is taken once by each walk).
n = 33 -- a last strip with one live column -- is outside both calls: the finishing pass inside the forward kernel, which
carries the head, works on pairs of columns and is served for even n only (tests/test_form_rules_cpu.py, 'n odd'), so
hb_sgp_fwd_gauss_f32 itself refuses it; that case is held to exactly this refusal, and (64, 34, 1) is the ragged strip.

Model level: the reduced SVGP of tests/test_gram_tiles_gpu.py, ten Adam steps with the switch on and off."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
import test_phi_direct_gpu as PD
from henbun_amd import graph as G

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).cuda().contiguous()


def nans(n):
    return torch.full((int(n),), float("nan"), dtype=F32, device="cuda")


_INPUTS = {}


def inputs(H, M, n, d):
    key = (M, n, d)
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.RandomState(5 + M + n)
    z = np.cumsum(1.5 * (0.75 + 0.5 * rng.rand(M, 1)), axis=0) * np.ones((1, d))
    if d > 1:
        z = z + 0.3 * rng.randn(M, d)
    ell = np.exp(0.1 * rng.randn(d))
    x = z[rng.randint(0, M, n)] + 0.7 * rng.randn(n, d)
    u, y = rng.randn(1, M), rng.randn(n)
    K = H.gram_fwd(dev(z), dev(z), dev(ell), diag_add=0.1).reshape(M, M)
    frag = torch.zeros(2 * M * M, dtype=F32, device="cuda")
    L, W, info = H.cholesky_inverse(K, frag=frag)
    assert info.item() == 0
    res = dict(x=dev(x), z=dev(z), ell=dev(ell), W=W.reshape(M, M), u=dev(u), frag=frag, y=dev(y), var=dev([0.4]), scale=dev([1.3]))
    _INPUTS[key] = res
    return res


def run(H, c, M, n, d, fused, bws=None):
    """One forward + backward; the noise is drawn in the kernel from a generator seeded the same way each time."""
    rng = H.Rng(1234, nlanes=max((n + 1) // 2, 64))
    units = H.sgp_head_units(c["x"], c["z"], c["u"], H.PREC_NATIVE, True, True, rng)
    assert units == (n + 31) // 32
    fe = H.sgp_frag_elems(1, n, M)
    o = dict(f=nans(n).reshape(1, n), v=nans(n), eps=nans(n), dmu=nans(n), fbar=nans(n), part=nans(3 * units),
             a_frag=nans(fe), abar_frag=nans(fe), Phi=nans(M * M).reshape(M, M), ubar=nans(M).reshape(1, M),
             zbar=nans(M * d).reshape(M, d), ellbar=nans(d))
    head = dict(y=c["y"], var=c["var"], scale=c["scale"], post=2.5, dmu=o["dmu"], fbar=o["fbar"], part=o["part"], units=units)
    bout = (o["Phi"], o["ubar"], o["zbar"], o["ellbar"])
    if fused:
        if bws is None:
            bws = nans(H.sgp_ws_elems(1, n, M, d, 1))
        H.sgp_fwd_gauss_kbar(c["x"], c["z"], c["ell"], c["W"], c["u"], c["frag"], o["a_frag"], o["abar_frag"], bws, head, rng=rng,
                             out=(o["f"], o["v"], o["eps"]))
        H.sgp_bwd_phi_rest(o["a_frag"], o["abar_frag"], bws, (1, n, M, d, 1), d, bout)
    else:
        H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], rng=rng, out=(o["f"], None, o["v"], o["eps"]), wfrag=c["frag"],
                  a_frag=o["a_frag"], skip_a=True, head=head)
        H.sgp_bwd_phi(c["x"], c["z"], c["ell"], c["W"], c["u"], o["eps"], o["v"], o["fbar"].reshape(1, n), c["frag"], o["a_frag"],
                      out=bout, abar_frag=o["abar_frag"])
    torch.cuda.synchronize()
    o["rng"] = rng.state.clone()
    return o, bws


HELD = ["a_frag", "f", "v", "eps", "dmu", "fbar", "part", "abar_frag", "ubar", "zbar", "ellbar", "Phi", "rng"]
SHAPES = [(64, 32, 1), (64, 34, 1), (192, 70, 2), (128, 1184, 1), (512, 2048, 1), (96, 64, 1)]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == F32 else t


@pytest.mark.parametrize("M,n,d", SHAPES)
def test_fused_pair_keeps_every_bit_of_the_two_launches(H, M, n, d):
    c = inputs(H, M, n, d)
    rng = H.Rng(1234, nlanes=max((n + 1) // 2, 64))
    assert H.sgp_fwd_kbar_supported(c["x"], c["z"], c["u"], H.PREC_NATIVE, True, True, rng)
    ref, _ = run(H, c, M, n, d, False)
    got, bws = run(H, c, M, n, d, True)
    for k in HELD:
        assert not torch.isnan(ref[k].float()).any() if k != "rng" else True, k   # the reference writes every element too
        same = torch.equal(bits(got[k]), bits(ref[k]))
        if not same:
            diff = (got[k].double() - ref[k].double()).abs()
            print("strip_fused[M%d,n%d,d%d] %s: %d elements differ, max |diff| %.3e" % (M, n, d, k, int((bits(got[k]) != bits(ref[k])).sum()),
                                                                                        float(torch.nan_to_num(diff, nan=float("inf")).max())))
        assert same, k
    # twice on one workspace (what a replayed plan does): the same bits again
    again, _ = run(H, c, M, n, d, True, bws=bws)
    for k in HELD:
        assert torch.equal(bits(again[k]), bits(got[k])), k


def test_odd_n_is_outside_the_head_and_so_outside_the_fused_call(H):
    """(64, 33, 1): the forward that carries the head needs an even n, so there is no two-launch reference to hold to."""
    c = inputs(H, 64, 34, 1)
    x33 = c["x"][:33].contiguous()
    rng = H.Rng(1, nlanes=64)
    assert H.sgp_head_units(x33, c["z"], c["u"], H.PREC_NATIVE, True, True, rng) == 0
    assert not H.sgp_fwd_kbar_supported(x33, c["z"], c["u"], H.PREC_NATIVE, True, True, rng)


# ------------------------------------------------------------------------------------------------ model level
def _ledger(plan, name):
    return [e for e in plan.explain if e[0] == name]


# launches a step issues beyond its first: the two-launch backward is strip kernel + contraction + finish, its rest is two
_EXTRA = {"sgp_grad": 2, "sgp_grad_rest": 1}


def _launches(plan):
    """Launches of one run of the plan, counted from its step list as tests/test_gram_tiles_gpu.py counts them, with the
    launches inside the sparse-GP backward steps spelled out."""
    n = 0
    for s in plan.steps:
        members = plan.chain_members.get(id(s))
        n += 1 + (1 if members and plan.chain_kind.get(id(members[0])) == "tail" else 0)
        for m in (members or [s]):
            n += _EXTRA.get(plan.step_labels.get(id(m), "other"), 0)
    return n


def _train(H, on, steps=10, make=None):
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = PD.JITTER
    with hb.settings.temp_settings(cfg):
        m, data = (make or PD.make_svgp)("float32")
        opt = m.ELBO()
        opt.compile()
        H.debug_set("sgp_fwd_kbar", on)      # read when the plan is built
        try:
            opt.optimize(maxiter=steps, minibatch_size=PD.MB, indices=data[5])
            plan = opt.last_plan
            torch.cuda.synchronize()
        finally:
            H.debug_clear()
        theta = m._session.theta.clone()
    labels = [plan.step_labels.get(id(s), "other") for s in plan.steps]
    return dict(theta=theta, fused=_ledger(plan, G.FWD_KBAR), phi=_ledger(plan, G.PHI_DIRECT), launches=_launches(plan), labels=labels)


@pytest.fixture(scope="module")
def trained(H):
    return {on: _train(H, on) for on in (1, 0)}


def test_ten_adam_steps_are_bit_identical_with_the_switch_on_and_off(trained):
    on, off = trained[1], trained[0]
    assert torch.isfinite(on["theta"]).all()
    assert torch.equal(on["theta"], off["theta"])


def test_ledger_and_launch_count(trained):
    on, off = trained[1], trained[0]
    assert len(on["fused"]) == 1 and on["fused"][0][2], on["fused"]
    assert len(off["fused"]) == 1 and not off["fused"][0][2] and "sgp_fwd_kbar" in off["fused"][0][3], off["fused"]
    for r in (on, off):
        assert len(r["phi"]) == 1 and r["phi"][0][2], r["phi"]
    assert any("sgp+kbar" in l for l in on["labels"]) and any("sgp_grad_rest" in l for l in on["labels"]), on["labels"]
    assert not any("sgp+kbar" in l or "sgp_grad_rest" in l for l in off["labels"]), off["labels"]
    assert on["launches"] == off["launches"] - 1, (on["labels"], off["labels"])


def _make_svgp_3d(dtype, seed=0):
    """PD.make_svgp with three input dimensions (the first is PD's own)."""
    from henbun_amd.models import SVGP

    np.random.seed(seed)     # (as PD.make_svgp: the model's own initial values come from the global generator)
    rng = np.random.RandomState(seed)
    X, Y, Z = PD.svgp_data(PD.N, PD.M, seed)
    X = np.concatenate([X.reshape(PD.N, -1), 0.3 * rng.randn(PD.N, 2)], axis=1)
    Z = np.concatenate([Z.reshape(PD.M, -1), 0.3 * rng.randn(PD.M, 2)], axis=1)
    eps = rng.randn(PD.N)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape="diagonal", residual="diagonal", eps=eps, dtype=dtype)
    m.gp.kern.lengthscales = np.ones(1) * 0.9
    m.k_var = np.ones(1) * 1.3
    m.var = np.ones(1) * 0.4
    m.u.inject_noise(rng.randn(PD.M))
    return m, (X, Y, Z, eps, None, rng.randint(0, PD.N, PD.MB))


def test_three_input_dimensions_keep_the_two_launch_plan(H):
    on, off = (_train(H, s, steps=1, make=_make_svgp_3d) for s in (1, 0))
    assert len(on["fused"]) == 1 and not on["fused"][0][2] and "d > 2" in on["fused"][0][3], on["fused"]
    assert on["labels"] == off["labels"] and on["launches"] == off["launches"]
    assert torch.equal(on["theta"], off["theta"])
