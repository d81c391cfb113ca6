"""The exact GP's cached predictive variance on the host: hb_gram_predict is declared, bound and validates its arguments
before any launch; the ExactPosterior methods built on it reject malformed calls before they reach the device; and the
numpy restatement the GPU tests lean on (tests/variance_cache_ref.py) has the properties the cache is used for -- an upper
bound of the exact variance that falls as the basis grows and meets it once the selection is exhausted.  No HIP kernel
runs here."""
import numpy as np
import pytest

import variance_cache_ref as VC

NEW = {"hb_gram_predict_f32": 25, "hb_gram_predict_f64": 25, "hb_gram_predict_ws_elems": 4}


# ---------------------------------------------------------------- C ABI
def test_gram_predict_is_declared_and_bound():
    import os

    import henbun_amd as hb
    from henbun_amd import _lib, hip_ops as H
    from henbun_amd.models import ExactGPR

    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    sigs = _lib.parse_prototypes(header)
    lib = _lib.lib()
    for name, nargs in NEW.items():
        assert name in _lib.declared_symbols() and name + "(" in header
        assert len(sigs[name][1]) == nargs and len(lib.raw(name).argtypes) == nargs
    assert lib.raw("hb_version")() == 2 and _lib.constants()["HB_ABI_VERSION"] == 2
    assert callable(H.gram_predict) and callable(H.gram_predict_ws_elems) and H.GRAM_PREDICT_WS_BYTES == 1 << 30
    assert all(callable(getattr(hb.gp.ExactPosterior, k)) for k in ("build_cache", "acquisition", "argmax"))
    assert hasattr(hb.gp, "VarianceCache") and callable(ExactGPR.suggest)


def test_workspace_size():
    """Partials of min(chunks, 16) chunks -- one chunk included, and rounded up to 8 bytes --, S n doubles beyond 16 chunks,
    a double and a long per 256 columns."""
    from henbun_amd import _lib

    lib = _lib.lib()
    chunk = lib.raw("hb_gram_matvec_chunk")()
    ws = lib.raw("hb_gram_predict_ws_elems")
    for nbytes in (4, 8):
        per = 8 // nbytes
        assert ws(0, 100, 3, nbytes) == 0
        assert ws(300, chunk, 17, nbytes) == 17 * 300 + 2 * per * 2
        assert ws(1, 1, 1, nbytes) == (2 if nbytes == 4 else 1) + 2 * per
        assert ws(300, chunk + 1, 17, nbytes) == 2 * 17 * 300 + 2 * per * 2
        assert ws(257, 16 * chunk + 1, 3, nbytes) == 16 * 3 * 257 + 3 * 257 * per + 2 * per * 2
        assert ws(100000, 10 ** 9, 64, nbytes) == ws(100000, 100000, 64, nbytes)


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
    (dict(acq=-1, val=1), "need an acquisition"),
    (dict(acq=-1, best_idx=1), "need an acquisition"),
    (dict(acq=-1, mean=None, var=None), "at least one"),
    (dict(acq=0, P=1, mean=None, var=None), "at least one"),
    (dict(acq=0, P=1, var_floor=-1.0), "var_floor"),
    (dict(acq=0, P=1, best=float("nan")), "best"),
    (dict(acq=0, P=1, best_idx=1, n=0), "candidate"),
    (dict(prior=float("nan")), "prior"),
    (dict(ws=None), "workspace"),
    (dict(ws=8), "aligned"),
])
def test_gram_predict_rejects_bad_arguments(suffix, bad, word):
    """(the pointers are small integers: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(kind=0, x=16, x2=16, ell=16, dl=1, V=16, P=2, scale=1.0, prior=1.0, acq=-1, best=0.0, param=0.0, largest=1,
             var_floor=0.0, mean=16, var=16, val=None, best_val=None, best_idx=None, n=100, N=40, d=1, S=2, ws=16)
    a.update(bad)
    rc = lib.raw("hb_gram_predict" + suffix)(*[a[k] for k in ("kind", "x", "x2", "ell", "dl", "V", "P", "scale", "prior", "acq", "best",
                                                              "param", "largest", "var_floor", "mean", "var", "val", "best_val",
                                                              "best_idx", "n", "N", "d", "S", "ws")], None)
    assert rc < 0 and word in lib.last_error() and "hb_gram_predict" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_no_columns_is_not_an_error_and_not_a_launch(suffix):
    from henbun_amd import _lib

    rc = _lib.lib().raw("hb_gram_predict" + suffix)(0, None, 16, 16, 1, 16, 1, 1.0, 1.0, -1, 0.0, 0.0, 1, 0.0, 16, 16, None, None,
                                                    None, 0, 40, 1, 2, None, None)
    assert rc == 0


# ---------------------------------------------------------------- the Python layers, before the device
def test_wrapper_rejects_operands_that_are_not_on_the_device():
    import torch

    from henbun_amd import hip_ops as H

    x, x2, ell, V = torch.ones(5, 2), torch.ones(7, 2), torch.ones(1), torch.ones(3, 7)
    with pytest.raises(ValueError, match="GPU"):
        H.gram_predict(x, x2, ell, V)


def _posterior(P=1, N=7):
    """An ExactPosterior over host tensors and no session: enough for every check that precedes the device."""
    import torch

    import henbun_amd as hb

    return hb.gp.ExactPosterior(None, torch.ones(N, 2), torch.ones(P, N), torch.ones(1), 1.0, 0.1, torch.ones(P, N), None, {}, 1e-6, 10)


def test_posterior_methods_reject_malformed_calls_before_the_device():
    post = _posterior()
    X = np.ones((3, 2))
    assert post.cache_info is None
    with pytest.raises(ValueError, match="build_cache"):
        post.predict_f(X, var="cache")
    with pytest.raises(ValueError, match="build_cache"):
        post.predict_y(X, var="cache")
    with pytest.raises(ValueError, match="'cache'"):
        post.predict_f(X, var="love")
    with pytest.raises(ValueError, match="kind must be one of"):
        post.acquisition(X, "thompson", best=0.0)
    with pytest.raises(ValueError, match="kind must be one of"):
        post.argmax(X, "thompson", best=0.0)
    with pytest.raises(ValueError, match="incumbent"):
        post.acquisition(X, "ei")
    with pytest.raises(ValueError, match="build_cache"):
        post.acquisition(X, "ei", best=0.0)
    with pytest.raises(ValueError, match="build_cache"):
        post.argmax(X, "ucb", param=2.0)
    with pytest.raises(ValueError, match="build_cache"):
        post.cache_basis
    with pytest.raises(ValueError, match="rank"):
        post.build_cache(rank=0)
    with pytest.raises(ValueError, match="threshold"):
        post.build_cache(threshold=-1.0)
    two = _posterior(P=2)
    for call in (two.acquisition, two.argmax):
        with pytest.raises(NotImplementedError, match="one latent function only"):
            call(X, "ei", best=0.0)


# ---------------------------------------------------------------- the restatement
CASES = {"n48": (48, 2.0), "n600": (600, 5.0)}
_BUILT = {}


def _built(name):
    """(case, v_exact, {rank asked: (cache, v_cache)}): computed once, shared by the tests below and left unchanged."""
    if name not in _BUILT:
        case = VC.square_case(*CASES[name])
        X, ell, k_var, noise_var, Xnew = case
        caches = {}
        for rank in (16, 64, 128, 256):
            c = VC.build(X, ell, k_var, noise_var, rank=rank)
            caches[rank] = (c, VC.v_cache(c, X, ell, k_var, Xnew))
        _BUILT[name] = (case, VC.v_exact(X, ell, k_var, noise_var, Xnew), caches)
    return _BUILT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cached_variance_is_an_upper_bound_that_falls_with_the_rank(name):
    (X, ell, k_var, noise_var, Xnew), ve, caches = _built(name)
    vs = {}
    for rank, (c, v) in caches.items():
        print("%s rank %d -> %d: min(v_cache - v_exact) %.3e, max %.3e, cond(T) %.3e, jitter %.1e"
              % (name, rank, c["rank"], (v - ve).min(), (v - ve).max(), c["cond"], c["jitter"]))
        assert c["rank"] == min(rank, c["rank"]) and c["jitter"] == VC.JITTER
        assert np.all(v >= 0.0) and np.all(v <= k_var)
        assert np.all(v >= ve - 1e-12)
        vs[rank] = v
    assert np.all(vs[16] >= vs[64] - 1e-12) and np.all(vs[64] >= vs[128] - 1e-12)   # nested bases
    assert np.all(vs[128] >= vs[256] - 1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_exhausted_selection_gives_the_exact_variance(name):
    """The float32 selection at threshold 0 stops by itself (rank 256 asked): the cache then is the exact variance to
    1e-5 k_var.  Measured with this restatement: 6.3e-9 at rank 34 (48 points), 1.3e-6 at rank 139 (600 points)."""
    (X, ell, k_var, noise_var, Xnew), ve, caches = _built(name)
    c, v = caches[256]
    print("%s: exhausted at rank %d, max(v_cache - v_exact) %.3e" % (name, c["rank"], (v - ve).max()))
    assert c["rank"] < min(256, X.shape[0])
    assert (v - ve).max() <= 1e-5 * k_var


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bound_depends_on_the_span_of_the_basis_alone(name):
    """Rows permuted and rescaled span the same space: v_cache to 1e-9.  A basis handed in is taken as it is."""
    (X, ell, k_var, noise_var, Xnew), _, caches = _built(name)
    c, v = caches[64]
    rng = np.random.default_rng(5)
    C2 = (c["C"] * rng.uniform(0.1, 10.0, (c["rank"], 1)))[rng.permutation(c["rank"])]
    c2 = VC.build(X, ell, k_var, noise_var, C=C2)
    assert c2["rank"] == c["rank"]
    assert np.abs(VC.v_cache(c2, X, ell, k_var, Xnew) - v).max() <= 1e-9


def test_float32_cache_rows_keep_the_bound_to_product_rounding():
    """R_c rounded once to float32, as a float32 session holds it: each entry moves by at most 2^-24 of itself, a product
    t_s = R_c[s] . k* by at most 2^-24 (|R_c[s]| . k*), the sum of squares by 2 |t_s| times that, summed over s: the bound
    holds up to that much (some 1e-7 k_var here)."""
    (X, ell, k_var, noise_var, Xnew), ve, _ = _built("n600")
    for rank in (64, 256):
        c = VC.build(X, ell, k_var, noise_var, rank=rank, rc_dtype=np.float32)
        v = VC.v_cache(c, X, ell, k_var, Xnew)
        t = VC.products(c, X, ell, k_var, Xnew)
        mag = VC.products(dict(Rc=np.abs(c["Rc"])), X, ell, k_var, Xnew)
        slack = 2.0 ** -23 * (np.abs(t) * mag).sum(0) + 1e-12
        print("rank %d -> %d, float32 R_c: min(v_cache - v_exact) %.3e, largest slack %.3e, max|R_c| %.3f"
              % (rank, c["rank"], (v - ve).min(), slack.max(), np.abs(c["Rc"]).max()))
        assert np.all(v >= ve - slack)


def test_tails_are_those_of_acq_ref():
    import acq_ref as AR

    mean, var = np.array([0.1, -0.4, 1.2]), np.array([0.3, 0.0, 0.05])
    for kind in ("ei", "pi", "ucb"):
        want = AR.tail(kind, mean, var, 0.5, 0.01, 1.0, False, 1e-6)[0]
        assert np.array_equal(VC.acquisition(kind, mean, var, 0.5, 0.01, False, 1e-6), want)
