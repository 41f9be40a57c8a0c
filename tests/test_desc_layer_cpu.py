"""CPU (no GPU needed): the references of tests/test_gpu_desc_layer.py are what they claim to be.  The torch restatement of the
reference's unfolded LineDescriptiveEncoder (tests/desc_layer_reference.py) reproduces tests/golden/desc_layer.npz, which autograd
through the REAL reference wrote (tests/golden/make_golden_desc_layer.py); the float64 closed forms of the three kernel pairs equal
float64 autograd; the FOLDED graph (CLS row only, key projection folded into u, value projection after the pooling) in float32 sits
inside the bar of the unfolded module -- worst error / bar 0.17 over the four cases below --, and a planted mistake in each
formula falls outside it; the header declares the new entry points and the built library exports them."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load
import desc_layer_reference as DL

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY_POINTS = ("linetr_cls_pool_train_forward", "linetr_cls_pool_train_backward", "linetr_layer_norm_forward", "linetr_layer_norm_backward",
                "linetr_layer_norm_backward_workspace_bytes", "linetr_gelu_forward", "linetr_gelu_backward")
FOLD_CASES = ((2, 33, 2, 1.0), (2, 33, 22, 1.0), (2, 33, 42, 1.0), (2, 33, 22, 4.0))      # (B, L, S, weight scale)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1.0)


def test_restatement_reproduces_the_fixture():
    f = load("desc_layer")
    assert os.path.getsize(os.path.join(HERE, "golden", "desc_layer.npz")) < 1 << 20
    assert sorted(f["state_dict_keys"].tolist()) == sorted(DL.SHAPES)
    assert f["out"].shape == (2, 5, 256) and f["d_desc"].shape == (2, 5, 22, 256) and f["out"].dtype == np.float64
    ref64, ref32 = DL.module_refs(*DL.FIXTURE_SHAPE)
    for key, val in ref64.items():
        want, mine32 = f[key], ref32[key]
        if key in DL.MATRICES:
            assert want.shape == val[::7, ::5].shape
            val, mine32 = val[::7, ::5], mine32[::7, ::5]
        yard = float(f[f"{key}_f32_err"])
        bar = DL.FACTOR * max(yard, 2.0 ** -23 * np.abs(want).max())
        assert np.abs(val - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), key      # the float64 runs agree to rounding
        assert 0 < yard < 1e-4 and np.abs(mine32 - want).max() <= bar, key                # and the float32 run sits inside the bar
    assert np.abs(f["slf_attn.w_ks.bias"]).max() < 1e-14 < float(f["slf_attn.w_ks.bias_f32_err"])     # zero in exact arithmetic, noise in float32


@pytest.mark.parametrize("family", DL.POOL_FAMILIES)
def test_pooling_closed_form_equals_float64_autograd(family):
    for L, S in ((1, 1), (2, 2), (5, 22), (3, 65)):
        c = DL.pool_case(family, L, S)
        ag = DL.pool_torch(c["x"][c["check"]], c["u"][c["check"]], c["dpooled"][c["check"]], torch.float64)
        for key in DL.POOL_OUTPUTS:
            assert rel(c["ref64"][key], ag[key]) <= 1e-12, (family, L, S, key)
    # S = 1: the softmax is 1, pooled is the row itself and no gradient reaches u
    c = DL.pool_case("normal", 3, 1)
    assert np.array_equal(c["ref64"]["pooled"], np.repeat(c["x"].astype(np.float64), 4, axis=1)) and not c["ref64"]["du"].any()
    # peaky: one token's score is +-40 against a field of a few units
    c = DL.pool_case("peaky", 4, 22)
    s = np.einsum("lhc,ltc->lht", c["u"].astype(np.float64), c["x"].astype(np.float64))
    assert np.abs(np.abs(s).max(axis=2) - 40.0).max() < 1e-3


@pytest.mark.parametrize("family", DL.LN_FAMILIES)
@pytest.mark.parametrize("residual", (False, True))
def test_layer_norm_closed_form_equals_float64_autograd(family, residual):
    c = DL.ln_case(family, 5, residual)
    ag = DL.ln_torch(c["a"], c["r"], c["gamma"], c["beta"], c["g"], torch.float64)
    for key in DL.LN_OUTPUTS:
        assert rel(c["ref64"][key], ag[key]) <= (1e-7 if family == "offset" else 1e-11), (family, key)      # (offset: 4096 x rounding in the mean)
    v = c["a"].astype(np.float64) + (c["r"] if residual else 0.0)
    if family == "offset":
        assert np.allclose(np.abs(v.mean(axis=1)) / v.std(axis=1), 4096.0, rtol=0.2)
    if family == "constant":
        assert not v.std(axis=1).any() and np.isfinite(c["ref64"]["dx"]).all()
        assert np.abs(c["ref64"]["y"] - c["beta"].astype(np.float64)).max() == 0.0


def test_gelu_closed_form_equals_float64_autograd():
    for family in DL.GELU_FAMILIES:
        c = DL.gelu_case(family)
        ag = DL.gelu_torch(c["z"], c["g"], torch.float64)
        for key in ("y", "dz"):
            assert np.abs(c["ref64"][key] - ag[key]).max() <= 1e-14 * max(np.abs(ag[key]).max(), 1.0), (family, key)
    z = np.abs(DL.gelu_case("small")["z"])
    assert z.max() < 1e-3 and 4.0 <= np.abs(DL.gelu_case("large")["z"]).min() and np.abs(DL.gelu_case("large")["z"]).max() <= 12.0


def fold_ratios(case, mistake=None):
    B, L, S, scale = case
    sd, desc, g = DL.module_case(B, L, S, DL.FIXTURE_SEED + 1, scale)
    ref64, ref32 = DL.module_refs(B, L, S, True, DL.FIXTURE_SEED + 1, scale)
    return DL.ratios(DL.run_layer(sd, desc, g, torch.float32, folded=True, mistake=mistake), ref64, ref32)


@pytest.mark.parametrize("case", FOLD_CASES)
def test_folded_float32_graph_sits_inside_the_bar(case):
    rows = fold_ratios(case)
    print(f"desc_layer folded float32 {case}: worst error / bar {DL.worst(rows):.3f}")
    assert len(rows) == 18 and not DL.failures(rows), DL.failures(rows)


def test_planted_mistakes_fall_outside_the_bar():
    # the 1/8 dropped from the folded graph
    assert DL.failures(fold_ratios(FOLD_CASES[1], mistake="no_scale"))
    # delta omitted from the pooling's backward; the LayerNorm backward without its xhat term; the tanh GELU
    c = DL.pool_case("normal", 5, 22)
    bad = DL.pool_closed_form(c["x"], c["u"], c["dpooled"], mistake="no_delta")
    assert DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("dx",))) and DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("du",)))
    assert not DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("pooled", "lse")))
    c = DL.ln_case("normal", 5, True)
    bad = DL.ln_closed_form(c["a"], c["r"], c["gamma"], c["beta"], c["g"], mistake="no_xhat")
    assert DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("dx",)))
    for family in ("unit", "large"):
        c = DL.gelu_case(family)
        bad = DL.gelu_closed_form(c["z"], c["g"], mistake="tanh")
        assert DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("y",))) and DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("dz",))), family


def test_header_declares_and_library_exports_the_entry_points():
    from linetr_amd import _native as nat
    with open(os.path.join(os.path.dirname(HERE), "include", "linetr_hip.h")) as fh:
        header = fh.read()
    L = nat.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in nat.EXPORTS and hasattr(L, name), name
    per_chunk = 2 * 256 * 4
    assert L.linetr_layer_norm_backward_workspace_bytes(0, 256) >= 0 and L.linetr_layer_norm_backward_workspace_bytes(1, 256) >= per_chunk
    assert L.linetr_layer_norm_backward_workspace_bytes(5, 128) == 0 and L.linetr_layer_norm_backward_workspace_bytes(-1, 256) == 0
    assert L.linetr_abi_version() == 6
