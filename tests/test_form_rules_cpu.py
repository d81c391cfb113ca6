"""The form and size rules of the native library, asked on the host (no kernel runs here): the answers for the benchmark
shapes and at every boundary of a rule are pinned as literals -- taken from tools/form_rules_table.py's table of the
build before the rules moved into one decision function -- and the exports a planner asks agree with the `hip_ops`
names that wrap them.

One answer tuple per case: (sgp_strip_path, hb_sgp_head_units, hb_sgp_rider_supported, sgp_bwd_phi_supported,
hb_sgp_ws_elems, sgp_predict_fused [fp32, diagonal S], sgp_frag_elems, cholesky_persistent_shape [fp32],
cholesky_ws_elems [fp32])."""
import pytest
import torch

from henbun_amd import _lib
from henbun_amd import hip_ops as H

F32, F64 = torch.float32, torch.float64


def _answers(E, n, M, d, P, prec=0, wf=1, draw=0, lanes=0):
    raw = _lib.lib().raw
    return (int(H.sgp_strip_path(E, n, M, d, P, prec)),
            int(raw("hb_sgp_head_units")(E, n, M, d, P, prec, wf, draw, lanes)),
            int(raw("hb_sgp_rider_supported")(E, n, M, d, P, prec, wf, draw, lanes)),
            int(H.sgp_bwd_phi_supported(E, n, M, d, P)),
            int(raw("hb_sgp_ws_elems")(E, n, M, d, P)),
            int(H.sgp_predict_fused(F32, E, n, M, d, P, H.SGP_S_DIAG, wf)),
            int(H.sgp_frag_elems(E, n, M, prec)),
            int(H.cholesky_persistent_shape(E, M, F32)),
            int(H.cholesky_ws_elems(E, M, F32)))


# the four benchmark shapes (cfg4 runs no sparse GP: M = 0), then the two sides of every boundary
PINNED = [
    ('cfg2', {'E': 1, 'n': 8192, 'M': 512, 'd': 1, 'P': 1}, (1, 256, 1, 1, 8397312, 1, 4194304, 1, 262496)),
    ('cfg3', {'E': 1, 'n': 16384, 'M': 1024, 'd': 1, 'P': 1}, (0, 0, 0, 0, 33571840, 0, 16777216, 1, 1049696)),
    ('cfg4', {'E': 1, 'n': 32768, 'M': 0, 'd': 1, 'P': 1}, (0, 0, 0, 0, 32768, 0, 0, 0, 1)),
    ('cfg5', {'E': 8, 'n': 65536, 'M': 512, 'd': 1, 'P': 1}, (1, 16384, 1, 1, 67637248, 1, 268435456, 1, 2099328)),
    ('cfg5 bf16x3', {'E': 8, 'n': 65536, 'M': 512, 'd': 1, 'P': 1, 'prec': 1}, (1, 0, 0, 1, 67637248, 1, 402653184, 1, 2099328)),
    ('M=32', {'E': 1, 'n': 1024, 'M': 32, 'd': 1, 'P': 1}, (1, 32, 0, 1, 33824, 1, 32768, 0, 1024)),
    ('M=48', {'E': 1, 'n': 1024, 'M': 48, 'd': 1, 'P': 1}, (0, 0, 0, 0, 74800, 0, 49152, 0, 2304)),
    ('M=512', {'E': 1, 'n': 1024, 'M': 512, 'd': 1, 'P': 1}, (1, 32, 1, 1, 8390144, 1, 524288, 1, 262496)),
    ('M=544', {'E': 1, 'n': 1024, 'M': 544, 'd': 1, 'P': 1}, (0, 0, 0, 0, 9471520, 0, 557056, 0, 295936)),
    ('d=2', {'E': 1, 'n': 1024, 'M': 64, 'd': 2, 'P': 1}, (1, 32, 1, 1, 132224, 1, 65536, 1, 4192)),
    ('d=3', {'E': 1, 'n': 1024, 'M': 64, 'd': 3, 'P': 1}, (1, 32, 0, 1, 132288, 1, 65536, 1, 4192)),
    ('d=4', {'E': 1, 'n': 1024, 'M': 64, 'd': 4, 'P': 1}, (1, 32, 0, 1, 132352, 1, 65536, 1, 4192)),
    ('d=5', {'E': 1, 'n': 1024, 'M': 64, 'd': 5, 'P': 1}, (0, 0, 0, 0, 132416, 0, 65536, 1, 4192)),
    ('P=2', {'E': 1, 'n': 1024, 'M': 64, 'd': 1, 'P': 2}, (1, 0, 0, 1, 132160, 1, 65536, 1, 4192)),
    ('P=4', {'E': 1, 'n': 1024, 'M': 64, 'd': 1, 'P': 4}, (1, 0, 0, 1, 132160, 1, 65536, 1, 4192)),
    ('P=5', {'E': 1, 'n': 1024, 'M': 64, 'd': 1, 'P': 5}, (0, 0, 0, 0, 132160, 0, 65536, 1, 4192)),
    ('n odd', {'E': 1, 'n': 33, 'M': 64, 'd': 1, 'P': 1}, (1, 0, 0, 1, 131169, 1, 4096, 1, 4192)),
    ('no wfrag', {'E': 1, 'n': 1024, 'M': 64, 'd': 1, 'P': 1, 'wf': 0}, (1, 0, 0, 1, 132160, 0, 65536, 1, 4192)),
    ('lanes short', {'E': 2, 'n': 1024, 'M': 64, 'd': 1, 'P': 1, 'draw': 1, 'lanes': 1023}, (1, 0, 0, 1, 264320, 1, 131072, 1, 8288)),
    ('lanes exact', {'E': 2, 'n': 1024, 'M': 64, 'd': 1, 'P': 1, 'draw': 1, 'lanes': 1024}, (1, 64, 1, 1, 264320, 1, 131072, 1, 8288)),
]
SWITCHED = [
    ('sgp_no_strip', 1, 'cfg2', (0, 0, 0, 0, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_no_strip', 1, 'cfg5', (0, 0, 0, 0, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_force_strip', 1, 'cfg2', (1, 256, 1, 1, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_force_strip', 1, 'cfg5', (1, 16384, 1, 1, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_tiled_crossover', 1, 'cfg2', (1, 256, 1, 1, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_tiled_crossover', 1, 'cfg5', (0, 0, 0, 0, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_strip_form2', 1, 'cfg2', (1, 0, 0, 1, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_strip_form2', 1, 'cfg5', (1, 0, 0, 1, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_no_fused_finish', 1, 'cfg2', (1, 0, 0, 1, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_no_fused_finish', 1, 'cfg5', (1, 0, 0, 1, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_form16', 1, 'cfg2', (1, 256, 1, 1, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_form16', 1, 'cfg5', (1, 16384, 1, 1, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_early', 0, 'cfg2', (1, 256, 0, 1, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_early', 0, 'cfg5', (1, 16384, 0, 1, 67637248, 1, 268435456, 1, 2099328)),
    ('sgp_phi_direct', 0, 'cfg2', (1, 256, 1, 0, 8397312, 1, 4194304, 1, 262496)),
    ('sgp_phi_direct', 0, 'cfg5', (1, 16384, 1, 0, 67637248, 1, 268435456, 1, 2099328)),
]


@pytest.fixture(autouse=True)
def _switches_cleared():
    H.debug_clear()
    yield
    H.debug_clear()


@pytest.mark.parametrize("name, kw, want", PINNED, ids=[p[0] for p in PINNED])
def test_rule_answers_for_benchmark_and_boundary_shapes(name, kw, want):
    assert _answers(**kw) == want


@pytest.mark.parametrize("key, value, cfg, want", SWITCHED, ids=["%s-%s" % (s[0], s[2]) for s in SWITCHED])
def test_rule_answers_with_each_switch_flipped(key, value, cfg, want):
    """Each diagnostic switch the form rules read, flipped alone, at the cfg2 and cfg5 shapes."""
    H.debug_set(key, value)
    assert _answers(**{p[0]: p[1] for p in PINNED}[cfg]) == want


def test_sizes_and_shape_rules_a_planner_once_restated():
    """Literals worked out from the expressions the planner carried: (5 if bf16x3 else 2) B M^2; M, N % 32 == 0,
    K % 128 == 0, 128 <= K <= 4096, at most 1024 tiles; B (M/32)^2 32 2 d."""
    assert H.cholesky_frag_elems(1, 512, False) == 524288 and H.cholesky_frag_elems(1, 1024, False) == 2097152
    assert H.cholesky_frag_elems(8, 512, True) == 10485760 and H.cholesky_frag_elems(1, 0, True) == 0
    wgk = {(512, 512, 512, 1): True, (1024, 1024, 1024, 1): True, (512, 512, 512, 8): False, (512, 512, 8192, 1): False,
           (512, 512, 4096, 1): True, (48, 512, 512, 1): False, (512, 48, 512, 1): False, (512, 512, 64, 1): False,
           (512, 512, 128, 1): True, (512, 512, 192, 1): False, (32, 32, 128, 1024): True, (32, 32, 128, 1025): False}
    for a, want in wgk.items():
        assert H.matmul_wgk_shape(*a) is want, a
    assert H.matmul_gram_vjp_ws_elems(1, 512, 1) == 16384 and H.matmul_gram_vjp_ws_elems(2, 64, 3) == 1536
    assert (H.MATUTIL_BAND, H.MATUTIL_ADD_EYE, H.MATUTIL_PHI, H.MATUTIL_SYM, H.MATUTIL_SYMLOW) == (0, 1, 2, 3, 4)


def test_new_exports_agree_with_the_names_that_wrap_them():
    raw = _lib.lib().raw
    for _, kw, _ in PINNED:
        E, n, M, d, P = (kw[k] for k in "EnMdP")
        for dt, sk, wf in ((F32, H.SGP_S_DIAG, 1), (F32, H.SGP_S_TRIL, 1), (F32, H.SGP_S_DIAG, 0), (F64, H.SGP_S_DIAG, 1)):
            assert bool(raw("hb_sgp_predict_fused")(E, n, M, d, P, sk, wf, 4 if dt == F32 else 8)) == H.sgp_predict_fused(dt, E, n, M, d, P, sk, wf)
        for prec in (H.PREC_NATIVE, H.PREC_BF16X3):
            assert raw("hb_sgp_frag_elems")(E, n, M, prec) == H.sgp_frag_elems(E, n, M, prec)
            assert raw("hb_cholesky_frag_elems")(E, M, prec) == H.cholesky_frag_elems(E, M, bool(prec)) == (5 if prec else 2) * E * M * M
        assert bool(raw("hb_matmul_wgk_shape")(M, M, M, E)) == H.matmul_wgk_shape(M, M, M, E)
        assert raw("hb_matmul_gram_vjp_ws_elems")(E, M, d) == H.matmul_gram_vjp_ws_elems(E, M, d)
    # a full-rank S is fused only for one latent function of one expert
    assert H.sgp_predict_fused(F32, 1, 1024, 64, 1, 1, H.SGP_S_TRIL, True) and not H.sgp_predict_fused(F32, 2, 1024, 64, 1, 1, H.SGP_S_TRIL, True)
