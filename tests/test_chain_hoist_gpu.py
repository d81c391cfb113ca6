"""The hoisted form of a serial chain on the device: one load phase, LDS slots and windows between the jobs
(csrc/jit.hip, chain_source_hoist) must return the bits of the same calls made one by one, and of the plain chain
(hb_debug_set("chain_hoist", 0))."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, svgp_data

pytestmark = pytest.mark.gpu
tf = hb.tf

R, NB = 70, 37      # rows of the lengthscale fold (two waves, no multiple of 64); units of the likelihood fold


def _tail(n, dtype, mode, runs=1, bad_info=False, over=False):
    """lengthscale fold -> likelihood fold -> gradient program -> Adam -> transform program [-> a program over the three
    sums and the value next to them].  mode: "alone" (every call a launch of its own), 0 / 1 (one chain, chain_hoist)."""
    if not H.ewise_jit_enabled():
        pytest.skip("hiprtc is not loadable in this process")
    E = H.EW
    gen = torch.Generator().manual_seed(7 + n)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype).cuda()
    b = dict(part_ell=rnd(R), ellbar=rnd(1), part_ll=rnd(3 * NB), stats=rnd(4), va=rnd(R), vb=rnd(R), g=rnd(n), theta=rnd(n),
             m=0.1 * rnd(n), v=(0.1 * rnd(n)) ** 2, tr=rnd(2), st2=rnd(4))
    b["t"] = torch.tensor([3], dtype=torch.int64).cuda()
    b["info"] = torch.tensor([0, 5 if bad_info else 0], dtype=torch.int32).cuda()
    b["fail"] = torch.zeros(2, dtype=torch.int64).cuda()
    g, theta, stats = b["g"], b["theta"], b["stats"]
    z2 = [[0.0, 0.0]]
    grad = H.EwiseProgram([[E["MUL"], 6, 4, 0, 0], [E["MUL"], 7, 5, 2, 0], [E["ADD"], 8, 6, 7, 0], [E["MUL"], 9, 0, 3, 0],
                           [E["ADD"], 10, 1, 2, 0], [E["MUL"], 11, 8, 3, 0]], z2 * 6,
                          [b["ellbar"], stats[0:1], stats[1:2], stats[2:3], b["va"], b["vb"]], [[0, 0]] * 4 + [[1, 0]] * 2,
                          [g[5:5 + R], g[1:2], g[2:3], g[3:4]], [8, 9, 10, 11 + H.EW_PROG_SUM], [[1, 0], [0, 0], [0, 0], [0, 0]], [R, 1])
    trail = H.EwiseProgram([[E["SOFTPLUS"], 3, 2, 0, 0], [E["MUL"], 4, 0, 1, 0]], z2 * 2,
                           [theta[n - 3:n - 2], theta[n - 2:n - 1], theta[n - 1:n]], [[0]] * 3, [b["tr"][0:1], b["tr"][1:2]], [3, 4],
                           [[0], [0]], [1])
    prog_over = H.EwiseProgram([[E["ADD"], 1, 0, 0, 0]], z2, [stats], [[1]], [b["st2"]], [1], [[1]], [4]) if over else None
    if mode != "alone":
        H.debug_set("chain_hoist", mode)
    try:
        for _ in range(runs):
            if mode != "alone":
                H.chain_begin()
            H.gram_ell_fold(b["part_ell"], R, 1, 1, 1, b["ellbar"])
            H.gauss_ll_fold(b["part_ll"], NB, stats[0:1], stats[1:2], stats[2:3])
            grad.launch()
            H.adam_step(theta, g, b["m"], b["v"], b["t"], lr=1e-2, gscale=-1.0, tick=True, info=b["info"], fail=b["fail"])
            trail.launch()
            if over:
                prog_over.launch()
            if mode != "alone":
                H.chain_end()
        torch.cuda.synchronize()
    finally:
        H.chain_discard()
        H.debug_clear()
    return {k: v.clone() for k, v in b.items()}


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [143, 1027, 4096])
def test_hoisted_chain_returns_the_bits_of_the_separate_calls_and_of_the_plain_chain(n, dtype):
    """n: one partial pass of the workgroup, more than 1024 parameters (two per thread), the chain's admission limit."""
    alone, hoisted = _tail(n, dtype, "alone"), _tail(n, dtype, 1)
    _same(alone, hoisted)
    _same(_tail(n, dtype, 0), hoisted)
    assert hoisted["t"].item() == 4 and not torch.equal(hoisted["theta"], _tail(n, dtype, "alone", runs=0)["theta"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_second_run_of_the_chain_loads_what_the_first_one_stored(dtype):
    alone, hoisted = _tail(1027, dtype, "alone", runs=2), _tail(1027, dtype, 1, runs=2)
    _same(alone, hoisted)
    _same(_tail(1027, dtype, 0, runs=2), hoisted)
    assert hoisted["t"].item() == 5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_blocked_step_keeps_the_parameters_and_the_transforms_of_the_old_ones(dtype):
    start = _tail(143, dtype, "alone", runs=0)
    alone, hoisted = _tail(143, dtype, "alone", bad_info=True), _tail(143, dtype, 1, bad_info=True)
    _same(alone, hoisted)
    _same(_tail(143, dtype, 0, bad_info=True), hoisted)
    for k in ("theta", "m", "v", "t"):
        assert torch.equal(hoisted[k], start[k]), k
    assert hoisted["fail"].tolist() == [4, 5]
    th = start["theta"].double()
    want = torch.stack([torch.nn.functional.softplus(th[-1]), th[-3] * th[-2]])
    assert torch.allclose(hoisted["tr"].double(), want, rtol=1e-5 if dtype == torch.float32 else 1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_range_that_partly_overlaps_earlier_outputs_takes_the_plain_path(dtype):
    alone, hoisted = _tail(143, dtype, "alone", over=True), _tail(143, dtype, 1, over=True)
    _same(alone, hoisted)
    _same(_tail(143, dtype, 0, over=True), hoisted)
    assert torch.equal(hoisted["st2"], hoisted["stats"] + hoisted["stats"])


def _svgp_theta(dtype, hoist=None, chains=True):
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 1e-5
    cfg.runtime.serial_chains = chains
    np.random.seed(5)
    rng = np.random.RandomState(5)
    X, Y, Z = svgp_data(2048, 64, 5)
    if hoist is not None:
        H.debug_set("chain_hoist", hoist)
    try:
        with hb.settings.temp_settings(cfg):
            m = SVGP(X=X, Y=Y, Z=Z, q_shape="diagonal", residual="diagonal", eps=rng.randn(2048), dtype=dtype)
            m.u.inject_noise(rng.randn(64))
            idx = rng.randint(0, 2048, 256)
            opt = m.ELBO()
            opt.compile(optimizer=tf.train.AdamOptimizer(0.01))
            opt.optimize(maxiter=5, minibatch_size=256, indices=idx)
            torch.cuda.synchronize()
            return m._session.theta.clone()
    finally:
        H.debug_clear()


def test_svgp_parameters_after_five_steps_are_the_same_bits_with_and_without_the_hoist():
    for dtype in ("float32", "float64"):
        assert torch.equal(_svgp_theta(dtype, hoist=0), _svgp_theta(dtype, hoist=1)), dtype
    # ... and agree with the step run without serial chains to the bound of test_svgp_adam_trajectory_matches_oracle
    a, b = _svgp_theta("float64", hoist=1).cpu().numpy(), _svgp_theta("float64", chains=False).cpu().numpy()
    assert np.abs(a - b).max() / np.abs(b).max() <= 1e-6
