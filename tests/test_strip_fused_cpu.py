"""hb_sgp_fwd_kbar_supported, asked on the host (no kernel runs): 1 where the likelihood head rides in the forward strip
kernel (hb_sgp_head_units > 0), the backward is Phi-direct (hb_sgp_bwd_phi_supported), d <= 2 -- the dimensions the fused
kernel is built for --, the call has at most 512 strips of 32 columns, and the switch sgp_fwd_kbar is not 0.  The
answers below are written down by hand from that rule; every answer tests/test_form_rules_cpu.py pins must stand as it
is, with the new switch either way."""
import pytest

import test_form_rules_cpu as FR
from henbun_amd import _lib
from henbun_amd import hip_ops as H


def _supported(E, n, M, d, P, prec=0, wf=1, draw=0, lanes=0):
    return int(_lib.lib().raw("hb_sgp_fwd_kbar_supported")(E, n, M, d, P, prec, wf, draw, lanes))


@pytest.fixture(autouse=True)
def _switches_cleared():
    H.debug_clear()
    yield
    H.debug_clear()


BY_HAND = [
    ("cfg2", dict(E=1, n=8192, M=512, d=1, P=1), 1),
    ("cfg5", dict(E=8, n=65536, M=512, d=1, P=1), 0),            # 16384 strips: beyond 512 the two launches measured faster
    ("512 strips", dict(E=2, n=8192, M=512, d=1, P=1), 1),
    ("513 strips", dict(E=1, n=16416, M=512, d=1, P=1), 0),
    ("M % 64 != 0", dict(E=1, n=1024, M=96, d=1, P=1), 1),      # an odd tile count: both walks take the middle tile once
    ("M % 32 != 0", dict(E=1, n=1024, M=48, d=1, P=1), 0),      # no column-strip form at all
    ("d = 2", dict(E=1, n=1024, M=64, d=2, P=1), 1),
    ("d = 3", dict(E=1, n=1024, M=64, d=3, P=1), 0),            # head and Phi-direct both served; the fused kernel is not built
    ("P = 2", dict(E=1, n=1024, M=64, d=1, P=2), 0),            # no head with two latent functions
    ("bf16x3", dict(E=8, n=65536, M=512, d=1, P=1, prec=1), 0),
    ("no Wfrag", dict(E=1, n=1024, M=64, d=1, P=1, wf=0), 0),
    ("n odd", dict(E=1, n=33, M=64, d=1, P=1), 0),              # the finishing pass in the forward kernel works on pairs
    ("lanes short", dict(E=2, n=1024, M=64, d=1, P=1, draw=1, lanes=1023), 0),
    ("lanes exact", dict(E=2, n=1024, M=64, d=1, P=1, draw=1, lanes=1024), 1),
]


@pytest.mark.parametrize("name, kw, want", BY_HAND, ids=[c[0] for c in BY_HAND])
def test_answers_written_down_by_hand(name, kw, want):
    assert _supported(**kw) == want
    # the rule's two library-side premises, where the answer is yes
    if want:
        assert _lib.lib().raw("hb_sgp_head_units")(kw["E"], kw["n"], kw["M"], kw["d"], kw["P"], kw.get("prec", 0), kw.get("wf", 1),
                                                   kw.get("draw", 0), kw.get("lanes", 0)) > 0
        assert H.sgp_bwd_phi_supported(kw["E"], kw["n"], kw["M"], kw["d"], kw["P"])


@pytest.mark.parametrize("key, value", [("sgp_fwd_kbar", 0), ("sgp_phi_direct", 0), ("sgp_no_fused_finish", 1), ("sgp_strip_form2", 1),
                                        ("sgp_no_strip", 1)])
def test_switches_that_take_a_premise_away(key, value):
    assert _supported(E=1, n=8192, M=512, d=1, P=1) == 1
    H.debug_set(key, value)
    assert _supported(E=1, n=8192, M=512, d=1, P=1) == 0


def test_the_switch_can_be_set_back():
    H.debug_set("sgp_fwd_kbar", 0)
    H.debug_set("sgp_fwd_kbar", 1)
    assert _supported(E=1, n=8192, M=512, d=1, P=1) == 1


@pytest.mark.parametrize("switch", [None, 0, 1])
def test_every_pinned_answer_of_the_form_rules_is_unchanged(switch):
    if switch is not None:
        H.debug_set("sgp_fwd_kbar", switch)
    for name, kw, want in FR.PINNED:
        assert FR._answers(**kw) == want, name
    for key, value, cfg, want in FR.SWITCHED:
        H.debug_set(key, value)
        assert FR._answers(**{p[0]: p[1] for p in FR.PINNED}[cfg]) == want, (key, cfg)
        H.debug_set(key, 1 - value)     # (each of these switches is 0 / 1: back to its default)


def test_wrapper_agrees_with_the_export():
    import torch

    x, z, u = torch.zeros(1024, 1), torch.zeros(64, 1), torch.zeros(1, 64)
    assert H.sgp_fwd_kbar_supported(x, z, u, H.PREC_NATIVE, True, False, None) is True
    assert H.sgp_fwd_kbar_supported(x, z, u, H.PREC_NATIVE, False, False, None) is False
    assert H.sgp_fwd_kbar_supported(x.double(), z.double(), u.double(), H.PREC_NATIVE, True, False, None) is False
    assert H.sgp_ws_elems(1, 1024, 64, 1, 1) == _lib.lib().raw("hb_sgp_ws_elems")(1, 1024, 64, 1, 1)
