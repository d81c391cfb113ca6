"""The references of tests/step_ref.py against independent float64 evaluations (torch autograd on the CPU, the oracle's
AdamTF), and the launcher arithmetic restated there against the properties the shapes of tests/test_step_kernels_gpu.py
rely on: which row chunks of the encoder's backward are empty, which wave walks two tiles, whether the finish kernel
runs its 16-partial round and its tail, which full-rank / Adam / reduction form a size reaches."""
import numpy as np
import pytest
import torch

import henbun_oracle as O
import step_ref as SR

T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
TACT = {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}


def _close(a, b, rtol=1e-10):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=0)


# ------------------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("name", ["sigmoid", "relu", "tanh"])
@pytest.mark.parametrize("adj", ["both", "x", "kl"])
def test_encoder_reference_against_autograd(name, adj):
    rng = np.random.RandomState(3)
    n, din, hid = 96, 32, 128
    y, u = rng.randn(n, din), rng.randn(n, SR.L)
    w0, b0 = rng.randn(din, hid) / np.sqrt(din), 0.1 * rng.randn(hid)
    w1, b1 = rng.randn(hid, 2 * SR.L) / np.sqrt(hid), 0.1 * rng.randn(2 * SR.L)
    xbar = rng.randn(n, SR.L) if adj != "kl" else None
    klbar = np.array([-0.7]) if adj != "x" else None
    f = SR.encoder_fwd(y, w0, b0, w1, b1, name, u)
    tw0, tb0, tw1, tb1 = [T(a).clone().requires_grad_(True) for a in (w0, b0, w1, b1)]
    o = TACT[name](T(y) @ tw0 + tb0) @ tw1 + tb1
    mu, s = o[:, :SR.L], o[:, SR.L:]
    x = mu + torch.exp(s) * T(u)
    kl = -0.5 * (2 * s + T(u) ** 2 - x ** 2).sum()
    _close(f["o"], o.detach().numpy())
    _close(f["x"], x.detach().numpy())
    _close(f["kl"], kl.item())
    loss = (x * T(xbar)).sum() if xbar is not None else 0.0
    loss = loss + (float(klbar[0]) * kl if klbar is not None else 0.0)
    loss.backward()
    got = SR.encoder_vjp(y, w0, b0, w1, name, f["o"][:, SR.L:], u, f["x"], xbar, klbar)
    for g, t in zip(got, (tw0, tb0, tw1, tb1)):
        _close(g, t.grad.numpy())


def test_sigmoid_reference_is_finite_and_exact_in_saturation():
    v = np.array([-800.0, -40.0, 0.0, 40.0, 800.0])
    h = SR.act("sigmoid", v)
    assert np.all(np.isfinite(h)) and h[0] == 0.0 and h[2] == 0.5 and h[4] == 1.0
    _close(h[1], np.exp(-40.0) / (1.0 + np.exp(-40.0)), 1e-15)


# ---------------------------------------------------------------------------------------------------- full-rank sampler
@pytest.mark.parametrize("rows,size", [(1, 1), (5, 7), (2, 65)])
@pytest.mark.parametrize("adj", ["both", "x", "kl"])
def test_fullrank_reference_against_autograd(rows, size, adj):
    rng = np.random.RandomState(rows + size)
    mu, u = rng.randn(rows, size), rng.randn(rows, size)
    S = 0.3 * rng.randn(rows, size, size) + np.eye(size)
    S[:, 0, 0] = -np.abs(S[:, 0, 0])                   # log S_kk^2: the sign of the diagonal does not matter
    xbar = rng.randn(rows, size) if adj != "kl" else None
    klbar = np.array([1.3]) if adj != "x" else None
    tm, tS = T(mu).requires_grad_(True), T(S).requires_grad_(True)
    tx = O.sample_fullrank(tm, tS, T(u))
    tkl = O.kl_normal(tS, T(u), tx, "fullrank")
    x, kl, xs, ks = SR.fullrank_fwd(mu, S, u)
    _close(x, tx.detach().numpy())
    _close(kl, tkl.item())
    assert np.all(xs >= np.abs(x) - 1e-15) and ks >= abs(kl)
    loss = ((tx * T(xbar)).sum() if xbar is not None else 0.0) + (float(klbar[0]) * tkl if klbar is not None else 0.0)
    gm, gS = torch.autograd.grad(loss, [tm, tS])
    mb, Sb = SR.fullrank_vjp(S, u, x, xbar, klbar)
    _close(mb, gm.numpy())
    _close(Sb, gS.numpy())
    assert np.all(np.triu(Sb, 1) == 0)
    # the packed twin: the same numbers in tril_indices order; NaN above the diagonal of the dense S changes nothing
    Sp = SR.tri_pack(S)
    xp, klp = SR.fullrank_fwd(mu, Sp, u, packed=True)[:2]
    assert np.array_equal(xp, x) and klp == kl
    mbp, Sbp = SR.fullrank_vjp(Sp, u, x, xbar, klbar, packed=True)
    assert np.array_equal(mbp, mb) and np.array_equal(Sbp, SR.tri_pack(Sb)) and np.array_equal(SR.tri_unpack(Sbp, size), Sb)
    Sn = np.where(np.triu(np.ones((size, size), bool), 1), np.nan, S)
    assert np.array_equal(SR.fullrank_fwd(mu, Sn, u)[0], x) and np.array_equal(SR.fullrank_vjp(Sn, u, x, xbar, klbar)[1], Sb)


# ------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_reference_against_the_oracle_over_several_steps():
    rng = np.random.RandomState(0)
    n, hp = 300, dict(lr=0.05, b1=0.8, b2=0.95, eps=1e-3)
    th = rng.randn(n)
    ref = O.T(th.copy())
    opt = O.AdamTF([ref], **hp)
    m, v, t = np.zeros(n), np.zeros(n), 0
    for _ in range(7):
        g = rng.randn(n) * 10.0 ** rng.uniform(-6, 2, n)
        opt.step([O.T(-0.25 * g)])                      # the oracle has no gscale: it is handed the scaled gradient
        th, m, v, t = SR.adam_step(th, g, m, v, t, gscale=-0.25, **hp)
    assert t == opt.t == 7
    _close(th, ref.numpy(), 1e-12)
    _close(m, opt.m[0].numpy(), 1e-12)
    _close(v, opt.v[0].numpy(), 1e-12)


def test_adam_reference_separates_the_two_epsilon_placements():
    """With the GPU test's hyper-parameters and small gradients the TF-1 rule, the rule with epsilon under the root, and a
    rule that forgets gscale^2 in v differ by O(1) of the step: the GPU tolerances cannot confuse them."""
    g, m, v = np.array([1e-5]), np.array([0.0]), np.array([0.0])
    hp = dict(lr=0.05, b1=0.8, b2=0.95, eps=1e-3, gscale=-0.25)
    th1, m1, v1, _ = SR.adam_step(np.zeros(1), g, m, v, 7, **hp)
    lr_t = 0.05 * np.sqrt(1 - 0.95 ** 8) / (1 - 0.8 ** 8)
    under_root = -lr_t * m1 / np.sqrt(v1 + 1e-3)
    assert abs(under_root - th1) > 0.5 * abs(th1)
    g2 = np.array([1.0])
    th2, m2, v2, _ = SR.adam_step(np.zeros(1), g2, m, v, 7, **hp)
    no_gs2 = -lr_t * m2 / (np.sqrt(0.05 * g2 * g2) + 1e-3)
    assert abs(no_gs2 - th2) > 0.5 * abs(th2)


# ------------------------------------------------------------------------------------------------------------ reductions
def test_reduction_reference():
    x = -1.0 - np.random.RandomState(0).rand(3, 5, 4)
    assert np.array_equal(SR.reduce_mid(x, "max"), np.max(x, 1)) and np.all(SR.reduce_mid(x, "max") < 0)
    _close(SR.reduce_mid(x, "sum"), np.einsum("krc->kc", x), 1e-14)
    assert np.array_equal(SR.reduce_mid(np.zeros((2, 0, 3)), "sum"), np.zeros((2, 3)))


# ------------------------------------------------------------------------------------------ the shapes reach their paths
def test_encoder_backward_chunk_partition_of_the_gpu_shapes():
    # n = 160: one chunk, wave 0 walks two tiles (one requested ahead), the others one
    for hid in (128, 256):
        p = SR.mlp2_bwd_partition(160, hid)
        assert len(p) == 1 and [len(w) for w in p[0]] == [2, 1, 1, 1] and p[0][0] == [0, 4]
    # n = 32 / 96: one chunk, three / one idle waves
    assert [len(w) for w in SR.mlp2_bwd_partition(32, 128)[0]] == [1, 0, 0, 0]
    assert [len(w) for w in SR.mlp2_bwd_partition(96, 256)[0]] == [1, 1, 1, 0]
    # n = 800: 25 tiles in 6 chunks of 5; chunk 5 starts at tile 25 and is empty; fewer than 16 chunks: scalar tail only
    for hid in (128, 256):
        p = SR.mlp2_bwd_partition(800, hid)
        assert len(p) == 6 and [sum(len(w) for w in c) for c in p] == [5, 5, 5, 5, 5, 0]
        assert [len(w) for w in p[0]] == [2, 1, 1, 1]
    # n = 2208: 69 tiles in 17 chunks of 5: a 16-partial round and one tail partial; chunks 14, 15, 16 are empty
    for hid in (128, 256):
        p = SR.mlp2_bwd_partition(2208, hid)
        sizes = [sum(len(w) for w in c) for c in p]
        assert len(p) == 17 and 16 <= len(p) < 32 and sizes == [5] * 13 + [4, 0, 0, 0]
    # n = 2176: 68 tiles in 17 full chunks of 4: the partial that the tail adds after the 16-partial round is not a zero one
    for hid in (128, 256):
        p = SR.mlp2_bwd_partition(2176, hid)
        assert len(p) == 17 and [sum(len(w) for w in c) for c in p] == [4] * 17
    # every tile is owned exactly once, whatever n
    for n in (32, 96, 160, 800, 2208, 4096, 32768):
        for hid in (128, 256):
            tiles = sorted(t for c in SR.mlp2_bwd_partition(n, hid) for w in c for t in w)
            assert tiles == list(range(n // 32)) and len(SR.mlp2_bwd_partition(n, hid)) <= 128


def test_encoder_forward_second_trip_needs_more_than_131072_rows():
    assert SR.mlp2_fwd_trips(131072) == (1024, 1) and SR.mlp2_fwd_trips(131104) == (1024, 2)
    assert SR.mlp2_fwd_trips(160) == (2, 1) and SR.mlp2_fwd_trips(32768)[1] == 1


def test_fullrank_forms_of_the_gpu_shapes():
    F = SR.fullrank_fwd_form
    assert F(1, 1)[0] == F(5, 7)[0] == F(3, 64)[0] == "thread"
    assert F(3, 65) == ("wave", 1, 1)
    assert F(64, 128) == ("wave", 1, 1) and F(65, 128) == ("wave", 3, 2)      # 8192 is the limit; past it the grid is capped
    assert F(1, 1024) == ("wave", 1, 1) and F(1, 1025) == ("wave", 3, 1)


def test_adam_forms_of_the_gpu_sizes():
    forms = {(n, eb, off): SR.adam_form(n, eb, off * eb) for n in (1, 255, 2048, 2049, 2051, 4099) for eb in (4, 8) for off in (0, 1)}
    assert all(forms[(n, eb, off)] == ("block", 0) for n in (1, 255, 2048) for eb in (4, 8) for off in (0, 1))
    assert all(forms[(n, eb, 1)] == ("scalar", 0) for n in (2049, 2051, 4099) for eb in (4, 8))
    assert {forms[(n, 4, 0)] for n in (2049, 2051, 4099)} == {("vec", 1), ("vec", 3)}
    assert {forms[(n, 8, 0)] for n in (2049, 2051, 4099)} == {("vec", 1)}


def test_reduction_splits_of_the_gpu_shapes():
    R = SR.reduce_split
    assert R(1, 16384, 1) == ("rows", 1) and R(1, 16385, 1) == ("rows", 4)
    assert R(63, 16385, 1) == ("rows", 4) and R(64, 16385, 1) == ("rows", 1) and R(3, 40000, 1) == ("rows", 9)
    assert R(1, 2048, 3) == ("cols", 1) and R(1, 2049, 3) == ("cols", 4)
    assert R(1, 2049, 64) == ("cols", 4) and R(1, 2049, 65) == ("cols", 4)      # one and two column blocks
    assert R(2, 2049, 4000) == ("cols", 4)       # 126 blocks: the last count below 128 with K1 = 2
    assert R(127, 2049, 1) == ("rows", 1)        # K2 == 1 takes the row kernel whatever R
    assert R(3, 5000, 70) == ("cols", 9)
    # no split leaves a chunk empty: ceil(R / S) (S - 1) < R
    for K1, Rr, K2 in [(1, 16385, 1), (63, 16385, 1), (3, 40000, 1), (1, 2049, 3), (2, 2049, 4000), (3, 5000, 70)]:
        S = R(K1, Rr, K2)[1]
        assert -(-Rr // S) * (S - 1) < Rr
