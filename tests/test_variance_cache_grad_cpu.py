"""Input gradients of the exact GP's cached predictive on the host: the numpy restatement the GPU tests lean on
(tests/variance_cache_grad_ref.py) agrees with central differences; hb_gram_predict_grad is declared, bound and validates
its arguments before any launch; the ExactPosterior methods built on it reject malformed calls before they reach the
device.  No HIP kernel runs here."""
import numpy as np
import pytest

import variance_cache_grad_ref as VG
import variance_cache_ref as VC

NEW = {"hb_gram_predict_grad_f32": 26, "hb_gram_predict_grad_f64": 26, "hb_gram_predict_grad_ws_elems": 5}
H_STEP = 1e-6
_BUILT = {}


# ---------------------------------------------------------------- the restatement against central differences
def _built():
    """The 48-point case with a rank-16 cache: (Xnew, X, ell, V = [alpha; R_c], k_var), computed once and left unchanged."""
    if not _BUILT:
        import exact_gp_ref as E

        X, ell, k_var, noise_var, Xnew = VC.square_case(48, 2.0)
        Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * np.random.default_rng(1).standard_normal((48, 1))
        alpha = np.linalg.solve(E.dense(X, ell, k_var, noise_var), Y).T
        cache = VC.build(X, ell, k_var, noise_var, rank=16)
        assert cache["rank"] == 16
        _BUILT["case"] = (Xnew, X, ell, np.concatenate([alpha, cache["Rc"]]), k_var)
    return _BUILT["case"]


def _central(f, x):
    """[n, d] central differences of f(x) -> [n] with step H_STEP, every point moved at once (a column's value depends on
    its own point alone)."""
    g = np.empty(x.shape)
    for k in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[k] = H_STEP
        g[:, k] = (f(x + e) - f(x - e)) / (2.0 * H_STEP)
    return g


def test_moment_gradients_agree_with_central_differences():
    """dmean and dvar within 1e-7 max|gradient| of central differences at h = 1e-6: the truncation, h^2 |f'''| / 6 ~ 1e-12,
    and the round-off, 2^-53 |f| / h ~ 1e-10, are both far below it.  No variance is clamped (asserted)."""
    x, x2, ell, V, k_var = _built()
    t, u = VG.products(x, x2, ell, V, scale=k_var)
    mean, var, dmean, dvar, raw = VG.moments_grad(t, u, 1, k_var)
    assert raw.min() > 0.0
    fd_mean = _central(lambda z: VG.products(z, x2, ell, V[:1], scale=k_var)[0][0], x)
    fd_var = _central(lambda z: k_var - VG.ordered_q(VG.products(z, x2, ell, V, scale=k_var)[0], 1), x)
    for name, got, fd in (("dmean", dmean[0], fd_mean), ("dvar", dvar, fd_var)):
        err, size = np.abs(got - fd).max(), np.abs(fd).max()
        print("%s: max |restatement - central difference| %.3e, max |gradient| %.3e, min variance %.3e" % (name, err, size, raw.min()))
        assert size > 1e-3 and err <= 1e-7 * size


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("kind", ["ei", "pi", "ucb"])
def test_acquisition_gradient_agrees_with_central_differences(kind, largest):
    """dval within 1e-7 max|gradient| of central differences of the value.  best is the 0.7 (0.3) quantile of the mean and
    var_floor = 1e-9 lies below every variance, at the points and a step away from them: nothing is clamped (asserted)."""
    x, x2, ell, V, k_var = _built()
    t, u = VG.products(x, x2, ell, V, scale=k_var)
    best = float(np.quantile(t[0], 0.7 if largest else 0.3))
    kw = dict(best=best, param=1.5 if kind == "ucb" else 0.01, largest=largest, var_floor=1e-9)
    val, dval, clamped = VG.acquisition_grad(kind, t, u, k_var, **kw)
    assert not clamped.any() and (k_var - VG.ordered_q(t, 1)).min() > 10.0 * kw["var_floor"]

    def value(z):
        tz, uz = VG.products(z, x2, ell, V, scale=k_var)
        v, _, c = VG.acquisition_grad(kind, tz, uz, k_var, **kw)
        assert not c.any()
        return v

    fd = _central(value, x)
    err, size = np.abs(dval - fd).max(), np.abs(fd).max()
    print("%s largest=%s: max |restatement - central difference| %.3e, max |gradient| %.3e" % (kind, largest, err, size))
    assert size > 1e-3 and err <= 1e-7 * size


def test_clamped_variance_passes_no_gradient():
    x, x2, ell, V, k_var = _built()
    t, u = VG.products(x, x2, ell, V, scale=k_var)
    _, var, _, dvar, raw = VG.moments_grad(t, u, 1, 0.0)
    assert np.all(raw < 0.0) and np.all(var == 0.0) and np.all(dvar == 0.0)
    _, dval, clamped = VG.acquisition_grad("ucb", t, u, 0.0, param=2.0, var_floor=1e-6)
    assert clamped.all() and np.array_equal(dval, u[0])
    assert np.all(VG.moments_grad(t[:1], u[:1], 1, k_var)[3] == 0.0)      # no cache rows


# ---------------------------------------------------------------- C ABI
def test_gram_predict_grad_is_declared_and_bound():
    import os

    import henbun_amd as hb
    from henbun_amd import _build, _lib, hip_ops as H
    from henbun_amd.models import ExactGPR

    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    sigs = _lib.parse_prototypes(header)
    lib = _lib.lib()
    for name, nargs in NEW.items():
        assert name in _lib.declared_symbols() and name + "(" in header
        assert len(sigs[name][1]) == nargs and len(lib.raw(name).argtypes) == nargs
    assert lib.raw("hb_version")() == 2 and _lib.constants()["HB_ABI_VERSION"] == 2
    assert "gram_predict_grad" in _build.SOURCES
    assert callable(H.gram_predict_grad) and callable(H.gram_predict_grad_ws_elems)
    assert all(callable(getattr(hb.gp.ExactPosterior, k)) for k in ("predict_grad", "maximise"))
    import inspect

    assert "grad" in inspect.signature(hb.gp.ExactPosterior.acquisition).parameters
    assert inspect.signature(ExactGPR.suggest).parameters["steps"].default == 0


def test_workspace_size():
    """1 + d times the partials of hb_gram_predict (min(chunks, 16) S n, rounded up to 8 bytes) and, beyond 16 chunks,
    1 + d times S n doubles; no arg-max partials."""
    from henbun_amd import _lib

    lib = _lib.lib()
    chunk = lib.raw("hb_gram_matvec_chunk")()
    ws = lib.raw("hb_gram_predict_grad_ws_elems")
    for nbytes in (4, 8):
        per = 8 // nbytes
        assert ws(0, 100, 2, 3, nbytes) == 0 and ws(100, 100, 0, 3, nbytes) == 0
        assert ws(300, chunk, 2, 17, nbytes) == 3 * 17 * 300
        assert ws(1, 1, 1, 1, nbytes) == 2 * (2 if nbytes == 4 else 1)
        assert ws(300, chunk + 1, 5, 17, nbytes) == 6 * 2 * 17 * 300
        assert ws(257, 16 * chunk + 1, 2, 3, nbytes) == 3 * (16 * 3 * 257 + 3 * 257 * per)
        assert ws(100000, 10 ** 9, 4, 64, nbytes) == ws(100000, 100000, 4, 64, nbytes)
        assert ws(300, chunk, 2, 17, nbytes) * nbytes % 8 == 0


ORDER = ("kind", "x", "x2", "ell", "dl", "V", "P", "scale", "prior", "acq", "best", "param", "largest", "var_floor", "mean", "var",
         "val", "dmean", "dvar", "dval", "n", "N", "d", "S", "ws")


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(S=0), "extents"),
    (dict(N=0), "extents"),
    (dict(d=0), "extents"),
    (dict(n=-1), "extents"),
    (dict(P=0), "mean rows"),
    (dict(P=3), "mean rows"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(V=None), "NULL"),
    (dict(x2=None), "NULL"),
    (dict(x=None), "NULL"),
    (dict(acq=0, P=2), "one latent function"),
    (dict(acq=7, P=1), "unknown acquisition"),
    (dict(acq=-1, val=16), "need an acquisition"),
    (dict(acq=-1, dval=16), "need an acquisition"),
    (dict(acq=-1, mean=None, var=None, dmean=None, dvar=None), "at least one"),
    (dict(acq=0, P=1, mean=None, var=None, dmean=None, dvar=None), "at least one"),
    (dict(acq=0, P=1, var_floor=-1.0), "var_floor"),
    (dict(acq=0, P=1, best=float("nan")), "best"),
    (dict(prior=float("nan")), "prior"),
    (dict(d=4 * 65535 + 1, dl=1), "too large"),
    (dict(ws=None), "workspace"),
    (dict(ws=8), "aligned"),
])
def test_gram_predict_grad_rejects_bad_arguments(suffix, bad, word):
    """(the pointers are small integers: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(kind=0, x=16, x2=16, ell=16, dl=1, V=16, P=2, scale=1.0, prior=1.0, acq=-1, best=0.0, param=0.0, largest=1,
             var_floor=0.0, mean=16, var=16, val=None, dmean=16, dvar=16, dval=None, n=100, N=40, d=1, S=2, ws=16)
    a.update(bad)
    rc = lib.raw("hb_gram_predict_grad" + suffix)(*[a[k] for k in ORDER], None)
    assert rc < 0 and word in lib.last_error() and "hb_gram_predict_grad" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_no_columns_is_not_an_error_and_not_a_launch(suffix):
    from henbun_amd import _lib

    rc = _lib.lib().raw("hb_gram_predict_grad" + suffix)(0, None, 16, 16, 1, 16, 1, 1.0, 1.0, -1, 0.0, 0.0, 1, 0.0, 16, 16, None, 16,
                                                         16, None, 0, 40, 1, 2, None, None)
    assert rc == 0


# ---------------------------------------------------------------- the Python layers, before the device
def test_wrapper_rejects_operands_that_are_not_on_the_device():
    """Where gram_predict raises without a GPU, gram_predict_grad does."""
    import torch

    from henbun_amd import hip_ops as H

    x, x2, ell, V = torch.ones(5, 2), torch.ones(7, 2), torch.ones(1), torch.ones(3, 7)
    for call in (H.gram_predict, H.gram_predict_grad):
        with pytest.raises(ValueError, match="GPU"):
            call(x, x2, ell, V)


def _posterior(P=1, N=7):
    """An ExactPosterior over host tensors and no session: enough for every check that precedes the device."""
    import torch

    import henbun_amd as hb

    return hb.gp.ExactPosterior(None, torch.ones(N, 2), torch.ones(P, N), torch.ones(1), 1.0, 0.1, torch.ones(P, N), None, {}, 1e-6, 10)


def test_posterior_methods_reject_malformed_calls_before_the_device():
    """Without a cache: ValueError naming build_cache.  Two outputs: acquisition(grad=True) and maximise are defined for
    one latent function only (predict_grad is not an acquisition: it returns the gradients of all P means)."""
    post = _posterior()
    X = np.ones((3, 2))
    with pytest.raises(ValueError, match="build_cache"):
        post.predict_grad(X)
    with pytest.raises(ValueError, match="build_cache"):
        post.acquisition(X, "ei", best=0.0, grad=True)
    with pytest.raises(ValueError, match="build_cache"):
        post.maximise(X, "ucb", param=2.0)
    with pytest.raises(ValueError, match="kind must be one of"):
        post.maximise(X, "thompson", best=0.0)
    with pytest.raises(ValueError, match="incumbent"):
        post.maximise(X, "ei")
    two = _posterior(P=2)
    with pytest.raises(ValueError, match="build_cache"):
        two.predict_grad(X)
    with pytest.raises(NotImplementedError, match="one latent function only"):
        two.acquisition(X, "ei", best=0.0, grad=True)
    with pytest.raises(NotImplementedError, match="one latent function only"):
        two.maximise(X, "ei", best=0.0)
