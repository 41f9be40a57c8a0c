"""CPU (no GPU needed): the float64 closed form of the HardNet criterion and its gradient (tests/hardnet_reference.py) and the torch
restatement reproduce tests/golden/hardnet_loss.npz, which autograd through the REAL reference wrote with its HardNet switch flipped
(tests/golden/make_golden_hardnet_loss.py), and the cases of tests/test_gpu_hardnet_loss.py hold what they are meant to hold.  That
pins the closed form, so the GPU tests can use it at shapes that have no fixture.  The library's side that needs no device: the
exported symbols, the workspace size query against its layout, and the `mining` switch of descriptor_loss."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load
import val_step_reference as R
import hardnet_reference as H

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_closed_form_and_restatement_reproduce_the_reference_fixture():
    f = load("hardnet_loss")
    d0, d1, assign = f["desc0"], f["desc1"], f["assign"]
    assert d0.shape == d1.shape == (3, 256, 40) and assign.shape == (3, 41, 41) and f["grad0_f64"].shape == (3, 256, 40)
    g = assign[:, :-1, :-1]
    assert ((g > 0.3).sum(axis=2) > 1).any() and ((g > 0.3).sum(axis=1) > 1).any() and (g == np.float32(0.2)).any()
    cf = H.closed_form(d0, d1, assign)
    assert H.max_err(f["grad0_f64"], f["grad1_f64"], cf) <= 1e-12
    assert cf["V"] == int(f["V"]) and cf["live"] == int(f["live"]) and 0 < cf["live"] < cf["V"]
    assert cf["loss"] == float(f["loss"]) and cf["hardest_positive"] == float(f["hp"]) and cf["hardest_negative"] == float(f["hn"])
    pos, neg = H.reference_order(cf)
    assert np.array_equal(pos, f["pos"]) and np.array_equal(neg, f["neg"])
    assert H.selection_gap(d0, d1, assign) >= R.MIN_MARGIN
    for loop in (False, True):
        t0, t1 = H.torch_grads(d0, d1, assign, torch.float64, anchor_loop=loop)
        assert H.max_err(t0, t1, cf) <= 1e-12
    out = H.torch_criterion(*(torch.tensor(x, dtype=torch.float64) for x in (d0, d1, assign)))
    assert float(out[0]) == float(f["loss"]) and float(out[1]) == float(f["hp"]) and float(out[2]) == float(f["hn"])
    assert out[3] == int(f["V"])
    t0, t1 = H.torch_grads(d0, d1, assign, torch.float32)
    assert H.max_err(t0, t1, cf) <= H.FACTOR * float(f["ref_f32_err"])


def test_closed_form_on_a_single_pair():
    """n = 1 with a match: V counts both anchors, the loss is exactly 0, hardest_negative is 10000 and nothing has a gradient"""
    d0 = np.zeros((1, 256, 1), np.float32)
    d0[0, :16] = 0.25
    d1 = d0.copy()
    d1[0, :2] = -0.25
    assign = np.zeros((1, 2, 2), np.float32)
    assign[0, 0, 0] = 1.0
    cf = H.closed_form(d0, d1, assign)
    assert cf["V"] == 2 and cf["live"] == 0 and cf["loss"] == 0.0 and cf["hardest_negative"] == 10000.0 and cf["hardest_positive"] == 0.5
    assert not cf["grad0"].any() and not cf["grad1"].any()
    assign[0, 0, 0] = 0.0
    cf = H.closed_form(d0, d1, assign)
    assert cf["V"] == 0 and np.isnan(cf["loss"]) and np.isnan(cf["hardest_negative"])


def test_exact_family_holds_its_variants():
    for variant in H.EXACT_VARIANTS:
        d0, d1, assign = H.exact_case(variant)
        cf = H.closed_form(d0, d1, assign)
        V = cf["V"]
        assert V >= 4 and V & (V - 1) == 0, (variant, V)
        # every number on the way is a small dyadic rational: float32 holds the float64 result
        for k in ("grad0", "grad1", "G"):
            assert np.array_equal(cf[k].astype(np.float32).astype(np.float64), cf[k]), (variant, k)
        assert np.array_equal((2 - 2 * R.dots(d0, d1, np.float32)).astype(np.float64), 2 - 2 * R.dots(d0, d1, np.float64))
        t0, t1 = H.torch_grads(d0, d1, assign, torch.float32)
        assert H.max_err(t0, t1, cf) == 0, variant
    one = lambda v: (H.closed_form(*H.exact_case(v)), 2 - 2 * R.dots(*H.exact_case(v)[:2], np.float64)[0], H.exact_case(v)[2][0])
    cf, dist, asg = one("tied_positives")
    w = 1.0 / cf["V"]
    assert dist[0, 0] == dist[0, 1] == 0.5 and asg[0, 0] == asg[0, 1] == 1 and cf["arg"][0, 0] == 0
    assert cf["G"][0, 0, 0] == 2 * w and cf["G"][0, 0, 1] == w and cf["G"][0, 0, 2] == -3 * w      # row anchor: +w at the first index alone
    cf, dist, asg = one("tied_minima")
    w = 1.0 / cf["V"]
    assert dist[0, 1] == dist[0, 2] == 0.75 and cf["G"][0, 0, 1] == cf["G"][0, 0, 2] == -w and cf["G"][0, 0, 0] == 2 * w
    cf, dist, asg = one("own_equals_cross")
    w = 1.0 / cf["V"]
    assert dist[0, 1] == dist[0, 2] == dist[1, 0] == dist[2, 0] == 0.75
    assert cf["G"][0, 0, 1] == cf["G"][0, 0, 2] == cf["G"][0, 1, 0] == cf["G"][0, 2, 0] == -w / 2 and cf["G"][0, 0, 0] == 2 * w
    cf, dist, asg = one("claimed_by_rows_and_columns")
    w = 1.0 / cf["V"]
    assert cf["G"][0, 0, 1] == -4 * w and cf["G"][0, 0, 0] == 2 * w and cf["G"][0, 1, 1] == 2 * w and cf["G"][0, 1, 0] == 0
    cf, dist, asg = one("relu_at_zero")
    assert cf["pos"][0, 0] == 0.5 and cf["neg"][0, 0] == 1.5 and not cf["alive"][0, 0] and not cf["G"][0, 0].any()
    cf, dist, asg = one("no_unmatched")
    assert cf["neg"][0, 0] == 10000.0 and cf["neg"][0, 24] == 10000.0 and not cf["alive"][0, 0] and not cf["G"][0, 0].any()
    cf, dist, asg = one("middle_assign")
    w = 1.0 / cf["V"]
    assert asg[0, 1] == np.float32(0.2) and dist[0, 1] == 0.25 and cf["neg"][0, 0] == 0.75 and cf["G"][0, 0, 1] == 0 and cf["G"][0, 0, 2] == -2 * w
    d0, d1, assign = H.exact_case("combined")
    cf = H.closed_form(d0, d1, assign)
    assert d0.shape == (2, 256, 70) and cf["V"] == 32 and 0 < cf["live"] < cf["V"] and cf["hardest_negative"] == 0.75


@pytest.mark.parametrize("B,n,extra", H.EDGE_CASES)
def test_generated_cases_select_the_same_in_any_float32_order(B, n, extra):
    d0, d1, assign = H.edge_case(B, n, extra)
    assert R.margins(d0, d1, assign, 0.7) >= R.MIN_MARGIN
    assert H.selection_gap(d0, d1, assign) >= R.MIN_MARGIN
    cf = H.closed_form(d0, d1, assign)
    assert cf["V"] > 0 and (cf["live"] > 0) == (n > 1)
    if extra:
        g = assign[:, :-1, :-1] > R.MATCH
        assert (g.sum(axis=2) > 1).any()
    t0, t1 = H.torch_grads(d0, d1, assign, torch.float64)
    assert H.max_err(t0, t1, cf) <= 1e-15 * max(H.grad_max(cf), 1e-3)


def align(x, a=256):
    return (x + a - 1) // a * a


def test_workspace_query_is_the_layouts_sum():
    from linetr_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in ("linetr_hardnet_loss_grad_workspace_bytes", "linetr_hardnet_loss_grad"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in nat.EXPORTS and hasattr(L, name), name
    for B, n in ((1, 1), (3, 40), (2, 250), (32, 250), (1, 32768), (65535, 7)):
        rows = align(B * n * 4)
        # result block | dots | two norm vectors | seven per-line records of 2n entries | the slack every layout ends in
        want = align(40) + align(B * n * n * 4) + 2 * rows + 7 * 2 * rows + 256
        assert L.linetr_hardnet_loss_grad_workspace_bytes(B, n) == want, (B, n)
    for B, n in ((0, 40), (3, 0), (-1, 5), (65536, 4), (2, 32769)):
        assert L.linetr_hardnet_loss_grad_workspace_bytes(B, n) == 0, (B, n)


def test_descriptor_loss_refuses_an_unknown_mining():
    import linetr_amd.evaluations as E
    assert E.descriptor_loss().mining == "semi-hard" and E.descriptor_loss(mining="hardnet").mining == "hardnet"
    with pytest.raises(ValueError, match="mining"):
        E.descriptor_loss(mining="bogus")
