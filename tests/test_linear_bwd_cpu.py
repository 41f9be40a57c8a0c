"""CPU (no GPU needed): the float64 closed forms of tests/linear_bwd_reference.py reproduce tests/golden/head_bwd.npz (+ head_bwd_dw.npz),
which autograd through the REAL reference's final_proj + F.normalize wrote (tests/golden/make_golden_head_bwd.py); the torch
restatement (the yardstick) reproduces it within the bar; the premises of the case families of tests/test_gpu_linear_bwd.py hold for
every committed seed; linetr_amd.train_ops imports and handles its shapes."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load
import val_step_reference as R
import loss_grad_reference as LG
import linear_bwd_reference as LB

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEAD_KEYS = ("line_desc", "dx", "dW", "db")


def chunk_rows():
    from linetr_amd import _native as nat
    return int(nat.lib().linetr_linear_backward_chunk_rows())


def head_fixture():
    f, w = load("head_bwd"), load("head_bwd_dw")
    fix = {**{k: f[k] for k in f.files}, **{k: w[k] for k in w.files}}
    rows = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, 256)
    fix["rows"] = {"x": rows(fix["x"]), "g": rows(fix["upstream"]), "W": fix["weight"][:, :, 0], "b": fix["bias"]}
    for p in ("f32", "f64"):
        fix["rows"][p] = {"line_desc": rows(fix[f"line_desc_{p}"]), "dx": rows(fix[f"dx_{p}"]), "dW": fix[f"dW_{p}"][:, :, 0], "db": fix[f"db_{p}"]}
    return fix


def test_closed_form_reproduces_the_reference_fixture():
    fix = head_fixture()
    r = fix["rows"]
    assert fix["x"].shape == fix["upstream"].shape == (2, 256, 33) and fix["weight"].shape == (256, 256, 1)
    assert all(fix[k].dtype == np.float32 for k in ("x", "weight", "bias", "upstream"))
    cf = LB.head_closed_form(r["x"], r["W"], r["b"], r["g"])
    cf["line_desc"] = cf["d"]
    for k in HEAD_KEYS:
        ref = r["f64"][k]
        # float64 rounding: a few hundred terms per element, each product rounded once
        assert np.abs(cf[k] - ref).max() <= 1e-13 * np.abs(ref).max(), k
    # the layer's closed form on the fixture's gy gives the same three gradients
    lay = LB.layer_closed_form(r["x"], r["W"], r["b"], cf["gy"])
    for k in ("dx", "dW", "db"):
        assert np.array_equal(lay[k], cf[k])
    assert cf["norm"].min() > LB.NORM_CLEAR * LB.EPS


def test_yardstick_reproduces_the_fixture_within_the_bar():
    fix = head_fixture()
    r = fix["rows"]
    t64, t32 = (LB.torch_head(r["x"], r["W"], r["b"], r["g"], dt) for dt in (torch.float64, torch.float32))
    for k, tk in zip(HEAD_KEYS, ("d", "dx", "dW", "db")):
        ref = r["f64"][k]
        assert np.abs(t64[tk] - ref).max() <= 1e-13 * np.abs(ref).max(), k
        ref_err = np.abs(r["f32"][k].astype(np.float64) - ref).max()             # the reference's own float32 run
        assert np.abs(t32[tk] - ref).max() <= LB.bar_of(ref_err, np.abs(ref).max()), k
    cf = LB.head_closed_form(r["x"], r["W"], r["b"], r["g"])
    assert np.abs(t64["gy"] - cf["gy"]).max() <= 1e-13 * np.abs(cf["gy"]).max()


def test_normalisation_below_eps_is_what_autograd_gives():
    """a row with y = 0 exactly, and one with 0 < |y| < eps: gy = g / eps in torch and in the closed form"""
    rs = np.random.RandomState(0)
    x = rs.standard_normal((3, 256))
    x[0] = 0.0
    x[1] *= 1e-16
    W, b, g = rs.standard_normal((256, 256)) / 16, np.zeros(256), rs.standard_normal((3, 256))
    cf, t64 = LB.head_closed_form(x, W, b, g), LB.torch_head(x, W, b, g, torch.float64)
    assert cf["norm"][0] == 0 and 0 < cf["norm"][1] < LB.EPS and cf["norm"][2] > 1
    assert np.array_equal(cf["gy"][:2], g[:2] / LB.EPS) and not cf["d"][0].any()
    assert np.abs(t64["gy"] - cf["gy"])[:2].max() <= 1e-15 * np.abs(cf["gy"]).max()
    assert np.abs(t64["gy"] - cf["gy"])[2].max() <= 1e-13


def test_case_lists_hold_every_row_edge():
    Rc = chunk_rows()
    assert Rc >= 64 and Rc % 32 == 0
    full = [r for r, N, K in LB.CASES if (N, K) == LB.FULL_NK]
    assert full == LB.ROW_EDGES and set(LB.ROW_EDGES) >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 250, 257, "Rc-1", "Rc", "Rc+1", "2Rc+1"}
    assert {(N, K) for _, N, K in LB.CASES} == {(64, 32), (256, 256), (256, 512), (512, 512), (1024, 256), (256, 1024)}
    reduced = [r for r, N, K in LB.CASES if (N, K) != LB.FULL_NK]
    assert set(reduced) == set(LB.ROW_EDGES)                                    # every row edge is there
    for nk in LB.OTHER_NK:
        assert "2Rc+1" in LB.REDUCED[nk] and len(LB.REDUCED[nk]) < len(LB.ROW_EDGES) // 2
    assert len({(LB.resolve_rows(r, Rc), N, K) for r, N, K in LB.CASES}) >= len(LB.CASES) - 1      # (Rc + 1 may be 257)


@pytest.mark.parametrize("rows,N,K", LB.CASES)
def test_exact_family_is_exact_in_float32(rows, N, K):
    rows = LB.resolve_rows(rows, chunk_rows())
    x, W, b, g, mask = LB.exact_case(rows, N, K)
    for a in (x, W, b, g, mask):
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a))
    assert LB.exact_partial_sum_bound(x, W, b, g) < 2 ** 24                      # every partial sum, in any order, is an exact integer
    for m, relu in ((None, False), (mask, True)):
        cf = LB.layer_closed_form(x, W, b, g, m, relu)
        for k in ("y", "dx", "dW", "db"):
            assert np.array_equal(cf[k], np.round(cf[k])) and np.abs(cf[k]).max() < 2 ** 24
    assert np.array_equal(mask, LB.layer_closed_form(x, W, b, g, None, True)["y"].astype(np.float32))
    if rows > 1:
        assert 0 < np.count_nonzero(mask > 0) < mask.size                       # the mask passes some entries and stops some


@pytest.mark.parametrize("rows,N,K", LB.CASES)
def test_normal_family_premises(rows, N, K):
    rows = LB.resolve_rows(rows, chunk_rows())
    x, W, b, g, mask = LB.normal_case(rows, N, K)
    cf = LB.layer_closed_form(x, W, b, g, mask, True)
    assert np.array_equal(mask > 0, cf["pre"].astype(np.float32) > 0)            # float32 rounding keeps the sign of every entry
    t64 = LB.torch_layer(x, W, b, g, torch.float64, relu=True)
    for k in ("y", "dx", "dW", "db"):
        assert np.abs(t64[k] - cf[k]).max() <= 1e-12 * max(np.abs(cf[k]).max(), 1.0), k
    if (N, K) == LB.FULL_NK:                                                     # the head runs on these
        assert LB.head_closed_form(x, W, b, g)["norm"].min() > LB.NORM_CLEAR * LB.EPS


def test_relu_surface_case_is_clear_of_zero():
    x, W, b, g = LB.relu_surface_case()
    cf = LB.layer_closed_form(x, W, b, g, None, True)
    t32 = LB.torch_layer(x, W, b, g, torch.float32, relu=True)
    bar = LB.bar_of(np.abs(t32["y"] - cf["y"]).max(), np.abs(cf["y"]).max())
    assert np.abs(cf["pre"]).min() > 2 * bar


def test_head_surface_case_has_surviving_anchors():
    W, b, x0, x1, assign, d0, d1 = LB.head_surface_case()
    cf0 = LB.head_closed_form(x0.transpose(0, 2, 1).reshape(-1, 256), W[:, :, 0], b, np.zeros((3 * 65, 256)))
    assert np.abs(cf0["d"].reshape(3, 65, 256).transpose(0, 2, 1) - d0).max() <= 1e-6     # line_desc is the generator's case
    grads, loss, V, e0, e1 = LB.torch_head_surface(torch.float64)
    assert V > 0 and np.isfinite(loss) and all(np.abs(v).max() > 0 for v in grads.values())
    assert R.margins(e0, e1, assign, LG.NN_THRESH) >= R.MIN_MARGIN and LG.selection_gap(e0, e1, assign) >= R.MIN_MARGIN
    assert V == LG.closed_form(d0, d1, assign)["V"]


def test_train_ops_imports_and_handles_shapes():
    from linetr_amd import train_ops as T
    from linetr_amd.engine import Engine
    conv_w, lin_w = torch.zeros(64, 32, 1), torch.zeros(64, 32)
    assert T.as_rows_weight(conv_w).shape == (64, 32) and T.as_rows_weight(conv_w).data_ptr() == conv_w.data_ptr()
    assert T.as_rows_weight(lin_w) is lin_w
    assert T.check_pointwise_shapes(torch.zeros(2, 32, 5), conv_w, torch.zeros(64)) == (64, 32)
    assert T.check_pointwise_shapes(torch.zeros(10, 32), lin_w) == (64, 32)
    for bad in ((torch.zeros(2, 5, 32), conv_w, None), (torch.zeros(10, 31), lin_w, None), (torch.zeros(10, 32), lin_w, torch.zeros(63)),
                (torch.zeros(10, 32), torch.zeros(64, 32, 3), None)):
        with pytest.raises(ValueError):
            T.check_pointwise_shapes(*bad)
    head = T.DescriptorHead()
    assert sorted(head.state_dict()) == ["final_proj.bias", "final_proj.weight"]
    assert head.state_dict()["final_proj.weight"].shape == (256, 256, 1)
    sd = {"final_proj.weight": torch.randn(256, 256, 1), "final_proj.bias": torch.randn(256), "klenc.other": torch.zeros(1)}
    loaded = T.DescriptorHead.from_line_transformer(sd)
    assert torch.equal(loaded.final_proj.weight, sd["final_proj.weight"]) and torch.equal(loaded.final_proj.bias, sd["final_proj.bias"])
    # [B, C, n] views: served through the transposed [B*n, C] rows, without a copy where the rows already exist
    eng = Engine.__new__(Engine)
    eng.device, eng._h = torch.device("cpu"), None
    x = torch.arange(2 * 8 * 3, dtype=torch.float32).reshape(2, 8, 3)
    rows, B, n = eng._act_rows(x, 8, "x")
    assert (B, n) == (2, 3) and rows.shape == (6, 8) and rows.is_contiguous() and torch.equal(rows[4], x[1, :, 1])
    back = Engine._like_input(rows, B, n)
    assert back.shape == x.shape and torch.equal(back, x) and back.data_ptr() == rows.data_ptr()
    again, _, _ = eng._act_rows(back, 8, "x")
    assert again.data_ptr() == rows.data_ptr()                                  # the transposed view of rows: no copy
    wide = torch.zeros(6, 12)
    strided, B2, n2 = eng._act_rows(wide[:, :8], 8, "x")
    assert B2 is None and strided.data_ptr() == wide.data_ptr() and strided.stride(0) == 12
    assert eng._act_rows(wide[:, :8], 8, "x", strided=False)[0].is_contiguous()
    assert eng._act_rows(torch.zeros(6, 13)[:, :8], 8, "x")[0].stride(0) == 8   # a stride that is no multiple of 4: copied
    with pytest.raises(ValueError):
        eng._act_rows(torch.zeros(2, 7, 3), 8, "x")
    assert eng._weight_2d(conv_w).shape == (64, 32)


def test_library_exports_and_header_declares_the_entry_points():
    from linetr_amd import _native as nat
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in ("linetr_linear_backward_chunk_rows", "linetr_linear_backward_workspace_bytes", "linetr_linear_forward", "linetr_linear_backward",
                 "linetr_head_backward_workspace_bytes", "linetr_head_forward", "linetr_head_backward"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in nat.EXPORTS and hasattr(L, name), name
    assert "#define LINETR_ABI_VERSION 6" in hdr
    Rc = L.linetr_linear_backward_chunk_rows()
    for bad in ((0, 256, 256), (10, 100, 256), (10, 256, 48), (10, 2048, 256), (10, 256, 2048)):
        assert L.linetr_linear_backward_workspace_bytes(*bad) == 0
    one, two = L.linetr_linear_backward_workspace_bytes(Rc, 256, 512), L.linetr_linear_backward_workspace_bytes(Rc + 1, 256, 512)
    assert one >= 256 * 512 * 4 + 256 * 4 and two >= 2 * (256 * 512 * 4 + 256 * 4) and two > one
    assert L.linetr_head_backward_workspace_bytes(0) == 0
    assert L.linetr_head_backward_workspace_bytes(100) >= 100 * 256 * 4 + L.linetr_linear_backward_workspace_bytes(100, 256, 256)
