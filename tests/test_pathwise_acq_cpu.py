"""Batch acquisition from function draws without a device: the numpy restatement tests/pathwise_acq_ref.py and the host
loop henbun_amd/gp/_host.py::greedy_batch, driven by numpy callables over a matrix of values F [S, n], and the argument
refusals of PathwiseDraws.acquisition / acquisition_argmax / select_batch, which are decided before anything is launched.

The one bound, q (2S + 4) 2^-53 joint for |sum of the gains - joint|: a gain is a sum of S non-negative doubles, each a
rounded difference, divided by S -- relative error at most (S + 1) 2^-53 to first order whatever the order of the sum;
joint likewise; the q gains are added with q - 1 more roundings.  Exact arithmetic makes the two equal (the gains
telescope: max(f - b, 0) = max(b, f) - b), so their difference is at most q (S + 2) 2^-53 joint + (S + 1) 2^-53 joint,
inside the bound.  Everything else is exact.  Every figure is printed before it is asserted."""
import types

import numpy as np
import pytest
import torch

from henbun_amd.gp import _host, sparse

import pathwise_acq_ref as AR

S, N = 17, 60


def _values(seed=0, S=S, n=N):
    """F [S, n]: smooth-ish rows of mixed sign and scale, and a scalar incumbent that some entries of every row beat."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((S, n)) * rng.uniform(0.5, 2.0, (S, 1)) + rng.standard_normal((1, n))
    return F, float(np.quantile(F, 0.8))


def _host_batch(F, b0, q, kind="ei", largest=True):
    """_host.greedy_batch over the columns of F with the restatement's acquisition as the arg-max."""
    def argmax_fn(b):
        a = AR.mc_acq(F, b, kind, largest)
        j = int(np.argmax(a))
        return j, a[j], j

    sign = 1.0 if largest else -1.0
    return _host.greedy_batch(argmax_fn, lambda j: F[:, j], np.broadcast_to(np.asarray(b0, np.float64), (F.shape[0],)), q, sign)


def test_mc_acq_by_hand():
    """Two draws, three columns, per-draw incumbents: every entry worked out by hand, both kinds, both directions; a NaN
    makes its column NaN and no other."""
    F = np.array([[1.0, 3.0, -2.0], [0.5, 0.0, 4.0]])
    b = np.array([2.0, 0.5])
    assert np.array_equal(AR.mc_acq(F, b, "ei"), [0.0, 0.5, 1.75])
    assert np.array_equal(AR.mc_acq(F, b, "pi"), [0.0, 0.5, 0.5])
    assert np.array_equal(AR.mc_acq(F, b, "ei", largest=False), [0.5, 0.25, 2.0])
    assert np.array_equal(AR.mc_acq(F, b, "pi", largest=False), [0.5, 0.5, 0.5])
    assert np.array_equal(AR.pi_count(F, b), [0, 1, 1])
    F[1, 1] = np.nan
    a = AR.mc_acq(F, b, "ei")
    assert np.isnan(a[1]) and a[0] == 0.0 and a[2] == 1.75
    assert AR.joint(np.array([[1.0, 3.0], [0.5, 4.0]]), b) == 0.5 * (1.0 + 3.5)
    with pytest.raises(ValueError):
        AR.mc_acq(F, b, "ucb")


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("kind", ["ei", "pi"])
def test_host_loop_is_the_restatement(kind, largest):
    """_host.greedy_batch and the restatement's greedy_batch pick the same columns with the same gains and end at the
    same incumbents, bit for bit; the gains never increase (exactly: the incumbents only rise and a sum of rounded
    non-negative terms is monotone in every term); a chosen column is worth exactly 0 afterwards."""
    F, b0 = _values(1)
    picks, gains, b = _host_batch(F, b0, 6, kind, largest)
    ridx, rgains, rb = AR.greedy_batch(F, b0, 6, kind, largest)
    idx = [i for i, _ in picks]
    print("greedy %s largest=%s: columns %s gains %s" % (kind, largest, idx, gains))
    assert len(idx) == 6 and len(set(idx)) == 6
    assert np.array_equal(idx, ridx) and np.array_equal(gains, rgains) and np.array_equal(b, rb)
    assert gains.dtype == np.float64 and np.all(np.diff(gains) <= 0.0) and np.all(gains > 0.0)
    assert np.all(AR.mc_acq(F, b, kind, largest)[idx] == 0.0)
    assert np.all(b >= b0) if largest else np.all(b <= b0)


@pytest.mark.parametrize("largest", [True, False])
def test_gains_sum_to_the_joint_improvement(largest):
    """sum of the gains against joint() of the chosen columns under the ORIGINAL incumbent, q = 1 .. 8."""
    F, b0 = _values(2)
    b0 = b0 if largest else float(np.quantile(F, 0.2))
    for q in (1, 2, 5, 8):
        picks, gains, _ = _host_batch(F, b0, q, "ei", largest)
        idx = [i for i, _ in picks]
        jt = AR.joint(F[:, idx], b0, largest)
        bound = q * (2 * S + 4) * 2.0 ** -53 * jt
        print("q=%d largest=%s: sum of gains %.17g, joint %.17g, difference %.3e, bound %.3e" % (q, largest, gains.sum(), jt, abs(gains.sum() - jt), bound))
        assert len(idx) == q and jt > 0.0
        assert abs(float(np.sum(gains)) - jt) <= bound


def test_early_stop_at_gain_zero():
    """Three columns improve on the incumbent and one of them dominates the other two in every draw: after it nothing
    improves, so a batch of 5 ends with 1 point; an incumbent above everything ends it with none; the restatement agrees."""
    F = -np.abs(_values(3)[0])
    F[:, 7], F[:, 20], F[:, 41] = 1.0, 2.0, 1.5
    picks, gains, b = _host_batch(F, 0.0, 5)
    assert [i for i, _ in picks] == [20] and np.array_equal(gains, [2.0]) and np.all(b == 2.0)
    assert np.array_equal(AR.greedy_batch(F, 0.0, 5)[0], [20])
    picks, gains, b = _host_batch(F, 10.0, 5)
    assert picks == [] and gains.shape == (0,) and np.all(b == 10.0)
    calls = []

    def nothing(b):
        calls.append(1)
        return -1, -np.inf, None

    picks, gains, _ = _host.greedy_batch(nothing, None, np.zeros(3), 4, 1.0)
    assert picks == [] and len(calls) == 1


def test_scalar_and_per_draw_incumbents_agree():
    F, b0 = _values(4)
    for kind in ("ei", "pi"):
        assert np.array_equal(AR.mc_acq(F, b0, kind), AR.mc_acq(F, np.full(S, b0), kind))
    a, b = _host_batch(F, b0, 4), _host_batch(F, np.full(S, b0), 4)
    assert [i for i, _ in a[0]] == [i for i, _ in b[0]] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("kind", ["ei", "pi"])
def test_smallest_mirrors_the_negated_values(kind):
    """largest=False on F with incumbents b is largest=True on -F with -b, bit for bit (negation is exact)."""
    F, b0 = _values(5)
    b = np.random.default_rng(6).uniform(-1.0, 0.0, S)
    assert np.array_equal(AR.mc_acq(F, b, kind, largest=False), AR.mc_acq(-F, -b, kind, largest=True))
    lo, hi = _host_batch(F, b, 4, kind, False), _host_batch(-F, -b, 4, kind, True)
    assert [i for i, _ in lo[0]] == [i for i, _ in hi[0]] and np.array_equal(lo[1], hi[1]) and np.array_equal(lo[2], -hi[2])


# ------------------------------------------------------------------------------------------------ refusals
def _draws(S=5, L=4, M=3, d=2):
    """A PathwiseDraws over host tensors: enough for everything that is decided before a launch."""
    sess = types.SimpleNamespace(torch=torch, device="cpu", np_dtype=np.float64, torch_dtype=torch.float64, H=None)
    return sparse.PathwiseDraws(sess, torch.zeros(L, d, dtype=torch.float64), torch.zeros(S, 2 * L + M, dtype=torch.float64),
                                torch.zeros(M, d, dtype=torch.float64), torch.ones(1, dtype=torch.float64), 1.0)


def test_acquisition_refuses_bad_arguments():
    """Another kind, a best that is neither a scalar nor [S], a non-finite scalar, an empty X, X of another width: ValueError
    from each of the three methods, before the session's kernels are touched (the stub session has none)."""
    draws = _draws()
    X = np.zeros((7, 2))
    for fn, extra in ((draws.acquisition, {}), (draws.acquisition_argmax, {}), (draws.select_batch, dict(q=2))):
        name = fn.__name__
        for kw in (dict(kind="ucb"), dict(kind="EI"), dict(best=np.zeros(4)), dict(best=np.zeros((5, 1))), dict(best=np.nan),
                   dict(best=np.inf)):
            args = dict(dict(best=0.0, **extra), **kw)
            with pytest.raises(ValueError, match=name):
                fn(X, **args)
        with pytest.raises(ValueError, match=name):
            fn(np.zeros((0, 2)), **dict(best=0.0, **extra))
        with pytest.raises(ValueError):
            fn(np.zeros((7, 3)), **dict(best=0.0, **extra))


def test_select_batch_refuses_bad_arguments():
    """q < 1, steps < 0, lr <= 0, malformed bounds, and steps > 0 with 'pi'."""
    draws = _draws()
    X = np.zeros((7, 2))
    for kw in (dict(q=0), dict(q=-3), dict(q=2, steps=-1), dict(q=2, lr=0.0), dict(q=2, bounds=(np.zeros(1), np.ones(1))),
               dict(q=2, bounds=(np.ones(2), np.zeros(2))), dict(q=2, kind="pi", steps=3)):
        with pytest.raises(ValueError, match="select_batch"):
            draws.select_batch(X, best=0.0, **kw)
