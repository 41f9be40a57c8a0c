"""CPU (no GPU needed): the float64 closed form of the criterion's gradient (tests/loss_grad_reference.py) reproduces
tests/golden/loss_grad.npz, which autograd through the REAL reference wrote (tests/golden/make_golden_loss_grad.py), and the cases of
tests/test_gpu_loss_grad.py hold what they are meant to hold.  That pins the closed form, so the GPU tests can use it at shapes that
have no fixture."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load
import val_step_reference as R
import loss_grad_reference as LG

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_closed_form_reproduces_the_reference_fixture():
    g, f = load("val_step"), load("loss_grad")
    cf = LG.closed_form(g["desc0"], g["desc1"], g["assign"])
    assert f["grad0_f64"].shape == f["grad1_f64"].shape == (3, 256, 40)
    scale = max(np.abs(f["grad0_f64"]).max(), np.abs(f["grad1_f64"]).max())
    assert LG.max_err(f["grad0_f64"], f["grad1_f64"], cf) <= 1e-15 * scale
    assert cf["V"] == int(f["V"]) == len(g["anchor_rows"]) and np.array_equal(cf["rows"], g["anchor_rows"])
    assert abs(cf["loss"] - float(g["loss"])) <= float(g["ref_err_f64"])
    # anchors of a row and of a column regularly select the same entry: fewer distinct entries than 2 V
    assert np.count_nonzero(cf["G"]) < 2 * cf["V"]
    assert LG.selection_gap(g["desc0"], g["desc1"], g["assign"]) >= R.MIN_MARGIN
    # the torch restatement differentiates to the same gradient, with and without the row loop
    for loop in (False, True):
        t0, t1 = LG.torch_grads(g["desc0"], g["desc1"], g["assign"], torch.float64, row_loop=loop)
        assert LG.max_err(t0, t1, cf) <= 1e-15 * scale
    t0, t1 = LG.torch_grads(g["desc0"], g["desc1"], g["assign"], torch.float32)
    assert LG.max_err(t0, t1, cf) <= LG.FACTOR * float(f["ref_f32_err"])


def test_closed_form_splits_ties_and_takes_the_first_negative():
    d0, d1, assign = LG.exact_case("tied_positives")
    cf = LG.closed_form(d0, d1, assign)
    w = 1.0 / cf["V"]
    assert cf["V"] == 4 and cf["ties"][0, 0] == 2
    assert cf["G"][0, 0, 0] == cf["G"][0, 0, 1] == w / 2 and cf["G"][0, 0, 2] == -w
    d0, d1, assign = LG.exact_case("tied_negatives")
    cf = LG.closed_form(d0, d1, assign)
    dist = 2 - 2 * R.dots(d0, d1, np.float64)[0]
    assert dist[0, 1] == dist[0, 2] == 0.75 and cf["neg_index"][0, 0] == 1
    assert cf["G"][0, 0, 0] == w and cf["G"][0, 0, 1] == -w and cf["G"][0, 0, 2] == 0


def test_exact_family_holds_its_variants():
    for variant in LG.EXACT_VARIANTS:
        d0, d1, assign = LG.exact_case(variant)
        cf = LG.closed_form(d0, d1, assign)
        V = cf["V"]
        assert V >= 4 and V & (V - 1) == 0, (variant, V)
        # every number on the way is a small dyadic rational: float32 holds the float64 result
        for k in ("grad0", "grad1", "G"):
            assert np.array_equal(cf[k].astype(np.float32).astype(np.float64), cf[k])
        assert np.array_equal((2 - 2 * R.dots(d0, d1, np.float32)).astype(np.float64), 2 - 2 * R.dots(d0, d1, np.float64))
        t0, t1 = LG.torch_grads(d0, d1, assign, torch.float32)
        assert LG.max_err(t0, t1, cf) == 0
    w = 0.25
    G = LG.closed_form(*LG.exact_case("claimed_twice"))
    assert G["G"][0, 0, 0] == 2 * w and G["G"][0, 0, 1] == -w and G["G"][0, 1, 0] == -w and G["neg_index"][0, 16 + 0] == 1
    d0, d1, assign = LG.exact_case("strict_window")
    G, dist = LG.closed_form(d0, d1, assign), 2 - 2 * R.dots(d0, d1, np.float64)[0]
    assert dist[0, 0] == 0.5 and dist[0, 1] == 0.5 and dist[0, 2] == 1.0 and assign[0, 0, 1] == 0 and assign[0, 0, 2] == 0
    assert G["G"][0, 0, 1] == 0 and G["G"][0, 0, 2] == 0 and G["G"][0, 0, 3] == -w
    assert dist[1, 4] == 0.5 and assign[0, 1, 4] == 1 and G["ties"][0, 1] == 0 and not G["G"][0, 1].any()      # nothing but the two bounds
    d0, d1, assign = LG.exact_case("middle_assign")
    G, dist = LG.closed_form(d0, d1, assign), 2 - 2 * R.dots(d0, d1, np.float64)[0]
    assert assign[0, 0, 1] == np.float32(0.2) and dist[0, 1] == dist[0, 2] == 0.75 and G["G"][0, 0, 1] == 0 and G["G"][0, 0, 2] == -w
    assert assign[0, 0, 4] == np.float32(0.3) and dist[0, 3] > dist[0, 0] and dist[0, 4] > dist[0, 0] and G["G"][0, 0, 0] == w
    assert G["G"][0, 0, 3] == 0 and G["G"][0, 0, 4] == 0
    d0, d1, assign = LG.exact_case("combined")
    assert d0.shape == (2, 256, 70) and LG.closed_form(d0, d1, assign)["V"] == 16


@pytest.mark.parametrize("B,n", LG.EDGE_CASES)
def test_generated_cases_select_the_same_in_any_float32_order(B, n):
    d0, d1, assign = LG.edge_case(B, n)
    assert R.margins(d0, d1, assign, LG.NN_THRESH) >= R.MIN_MARGIN
    assert LG.selection_gap(d0, d1, assign) >= R.MIN_MARGIN
    cf = LG.closed_form(d0, d1, assign)
    assert (cf["V"] == 0) == (n == 1)
    if cf["V"]:
        t0, t1 = LG.torch_grads(d0, d1, assign, torch.float64)
        assert LG.max_err(t0, t1, cf) <= 1e-15 * LG.grad_max(cf)


def test_library_exports_and_header_declares_the_entry_points():
    from linetr_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in ("linetr_desc_loss_grad_workspace_bytes", "linetr_desc_loss_grad"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in nat.EXPORTS and hasattr(L, name), name
    assert L.linetr_desc_loss_grad_workspace_bytes(0, 40) == 0 and L.linetr_desc_loss_grad_workspace_bytes(3, 0) == 0
    assert L.linetr_desc_loss_grad_workspace_bytes(3, 40) >= 3 * 40 * 40 * 4
