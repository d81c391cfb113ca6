"""The host helpers the eager GP routes share (henbun_amd/gp/_host.py) and the argument checks of gp/sparse.py, without a
device: the chunk rule of the float64 walks, the scalar value of the collapsed bound against the numpy restatement, and
every refusal that is decided before the session is touched.  The refusals that need device data in flight (X, Y, z
shapes that do not match, a factorisation that fails) stay with the GPU tests test_*_refuses_what_it_does_not_cover."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import henbun_amd as hb
from henbun_amd.gp import _host, sparse

import optimal_q_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("M, align, rows", [(32, 1, 32768), (512, 1, 32768), (600, 1, 27962), (600, 32, 27936), (1024, 1, 16384),
                                            (1 << 20, 1, 32)])
def test_f64_chunk_rows(M, align, rows):
    """min(32768, max(32, 2^24 // M)) rounded down to `align`, evaluated by hand.  M = 600 is the smallest kind of M at
    which the statistics walk (align 1) and the ELBO-gradient walk (align 32) cut at different rows: the chunks' sums are
    added in chunk order, so the two rules were NOT unified."""
    assert _host.f64_chunk_rows(M, align) == rows


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
@pytest.mark.parametrize("P", [1, 2])
def test_collapsed_value_against_the_restatement(P, residual):
    """Both association orders -- yy, quad per column (collapsed_bound) and summed over the columns beforehand (the gradient
    route) -- against optimal_q_ref.collapsed_bound, quad and logdet formed in numpy from the same Lambda the way the
    restatement forms them, so the inputs are the same doubles and only the order of the sum differs.
    Bound: the value is the sum of T1 = N P / 2 log(2 pi s2), T2 = sum yy / (2 s2), T3 = sum quad / 2, T4 = P / 2 logdet
    and T5 = P k (N - a2sum) / (2 s2).  Either order reaches it in at most 8 rounded operations past the inputs (the
    products and quotients inside a term, the P - 1 additions over the columns, four additions of terms), each with a
    relative error of at most eps / 2 on a partial result no larger than S = sum |T_i|: |difference of two orders| <=
    2 * 8 * (eps / 2) * S = 8 eps S."""
    rng = np.random.RandomState(P)
    M, N, s2, k = 8, 50, 0.4, 1.3
    A = 0.3 * rng.randn(M, N)
    Y = rng.randn(N, P)
    Phi, b, yy, a2sum = A @ A.T, (A @ Y).T, (Y ** 2).sum(0), float(np.trace(A @ A.T))
    L = np.linalg.cholesky(np.eye(M) + (k / s2) * Phi)
    t = np.linalg.solve(L, (np.sqrt(k) * b / s2).T)
    quad, logdet = (t * t).sum(0), 2.0 * float(np.log(np.diag(L)).sum())
    ref = R.collapsed_bound(Phi, b, yy, a2sum, N, s2, k, residual)
    terms = [0.5 * N * P * np.log(2 * np.pi * s2), yy.sum() / (2 * s2), 0.5 * quad.sum(), 0.5 * P * logdet,
             P * k * (N - a2sum) / (2 * s2) if residual == "diagonal" else 0.0]
    bound = 8 * np.finfo(np.float64).eps * sum(abs(x) for x in terms)
    per_column = _host.collapsed_value(N, P, s2, k, yy, quad, logdet, a2sum, residual)
    summed = _host.collapsed_value(N, P, s2, k, float(yy.sum()), float(quad.sum()), logdet, a2sum, residual)
    print("collapsed_value P=%d %s: ref %.17g, per column %+.3e, summed %+.3e, bound %.3e"
          % (P, residual, ref, per_column - ref, summed - ref, bound))
    assert isinstance(per_column, float) and isinstance(summed, float)
    assert abs(per_column - ref) <= bound and abs(summed - ref) <= bound
    if P == 1:
        assert per_column == summed       # one column: nothing to associate differently


class _Holder(hb.model.Model):
    def setUp(self, gp):
        self.gp = gp


def _sparse(kern, Z=np.linspace(0, 1, 4)[:, None]):
    return hb.gp.SparseGP(kern=kern, z=Z)


def test_rbf_model_inputs_refuses_before_the_session_is_touched():
    K = hb.gp.kernels
    for gp in (hb.gp.GP(kern=K.UnitRBF(np.ones(1))), _sparse(K.UnitRBF(np.ones(1)))):          # outside a Model
        with pytest.raises(ValueError, match="part of a Model"):
            _host.rbf_model_inputs(gp, "who")
    X, Y = np.zeros((5, 1)), np.zeros((5, 1))
    other = _Holder(gp=_sparse(K.UnitMatern52(np.ones(1))))
    batched = _Holder(gp=_sparse(K.UnitRBF(np.ones((2, 1))), np.zeros((2, 4, 1))))
    batched_ell = _Holder(gp=hb.gp.GP(kern=K.UnitRBF(np.ones((2, 1)))))
    with pytest.raises(NotImplementedError, match="UnitRBF"):
        _host.rbf_model_inputs(other.gp, "who")
    with pytest.raises(NotImplementedError, match="one expert"):
        _host.rbf_model_inputs(batched_ell.gp, "who")
    # the public routes reach the same refusals, with no device: none of these models ever opens one
    for m, what in ((other, "UnitRBF"), (batched, "one expert")):
        for route in (lambda g: g.statistics(X, Y), lambda g: g.select_inducing(X), lambda g: g.collapsed_bound_and_grad(X, Y, 0.1),
                      lambda g: g.natgrad_q(X, Y, hb.likelihoods.Bernoulli()), lambda g: g.condition(X, Y, 0.1),
                      lambda g: g.pathwise_draws((np.zeros((1, 4)), np.eye(4)), 2)):
            with pytest.raises(NotImplementedError, match=what):
                route(m.gp)
        assert not m._session._ready
    with pytest.raises(NotImplementedError, match="one expert"):
        batched_ell.gp.log_marginal_likelihood(X, Y, 0.1)


def test_check_lik_inputs_refusals():
    lik, M = hb.likelihoods.Bernoulli(), 4
    Y1, Y2, q = np.zeros((5, 1)), np.zeros((5, 2)), (np.zeros((1, 4)), np.eye(4))
    check = lambda **kw: sparse._check_lik_inputs(*[{**dict(who="who", name="q", likelihood=lik, k_var=1.0, residual="diagonal",
                                                           q=q, Yd=Y1, M=M), **kw}[k]
                                                    for k in ("who", "name", "likelihood", "k_var", "residual", "q", "Yd", "M")])
    m0, S0 = check(q=([[0, 1, 2, 3]], np.eye(4, dtype=np.float32)))
    assert m0.dtype == S0.dtype == np.float64 and m0.shape == (1, 4) and check(q=None) is None
    assert S0.shape == (1, 4, 4)                                            # the one block of a one-latent q
    # the block-shaped q of a likelihood over C = 3 latent functions
    lik3, Y3 = hb.likelihoods.Softmax(3, nodes=np.zeros((2, 3))), np.zeros((5, 1))
    m3, S3 = check(likelihood=lik3, Yd=Y3, q=(np.zeros((3, 4), dtype=np.float32), [np.eye(4)] * 3))
    assert m3.dtype == S3.dtype == np.float64 and m3.shape == (3, 4) and S3.shape == (3, 4, 4)
    assert check(likelihood=lik3, Yd=Y3, q=None) is None
    with pytest.raises(NotImplementedError, match="mean-field"):
        check(likelihood=lik3, Yd=Y3, q=(np.zeros((3, 4)), np.ones((3, 4))))
    with pytest.raises(ValueError, match=r"q = \(m \[3, 4\], S \[3, 4, 4\]\) expected"):
        check(likelihood=lik3, Yd=Y3, q=(np.zeros((3, 5)), np.stack([np.eye(5)] * 3)))     # M of another z
    with pytest.raises(ValueError, match=r"q = \(m \[3, M\], S \[3, M, M\]\) expected"):
        check(likelihood=lik3, Yd=Y3, q=q)                                  # the one-latent shape
    with pytest.raises(ValueError, match="labels"):
        check(likelihood=lik3, Yd=Y3 + 3.0)
    with pytest.raises(NotImplementedError, match="fullrank"):
        check(residual="fullrank")
    with pytest.raises(ValueError, match="residual"):
        check(residual="dense")
    with pytest.raises(NotImplementedError, match="mean-field"):
        check(q=(np.zeros((1, 4)), np.ones(4)))
    with pytest.raises(ValueError, match="expected"):
        check(q=(np.zeros((1, 3)), np.eye(4)))
    with pytest.raises(ValueError, match="expected"):
        check(q=(np.zeros((1, 4)), np.eye(5)))
    with pytest.raises(NotImplementedError, match="one latent function"):
        check(Yd=Y2)
    with pytest.raises(TypeError, match="Likelihood"):
        check(likelihood="bernoulli")
    with pytest.raises(ValueError, match="k_var"):
        check(k_var=0.0)


def test_the_helpers_import_where_no_gpu_is_visible():
    code = ("import os, sys; os.environ['HIP_VISIBLE_DEVICES'] = ''; os.environ['CUDA_VISIBLE_DEVICES'] = ''; "
            "sys.path.insert(0, %r); import henbun_amd.gp._host, henbun_amd.gp.sparse; "
            "print(henbun_amd.gp._host.f64_chunk_rows(600, 32))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "27936", out.stderr


def test_the_shared_idioms_are_written_once():
    """The factorise-and-raise read-back and the upload expression occur in _host.py only."""
    pats = [re.compile(r"info\.cpu\(\)"), re.compile(r"as_tensor\(np\.ascontiguousarray")]
    gp_dir = os.path.join(ROOT, "henbun_amd", "gp")
    files = [os.path.join(gp_dir, f) for f in sorted(os.listdir(gp_dir)) if f.endswith(".py")] + [os.path.join(ROOT, "henbun_amd", "models.py")]
    hits = {}
    for path in files:
        with open(path) as f:
            text = f.read()
        n = [len(p.findall(text)) for p in pats]
        if any(n):
            hits[os.path.basename(path)] = n
    assert hits == {"_host.py": [1, 1]}
