"""CPU: pins the references and the bar of the BatchNorm backward unit tests (bn_bwd_cases.py) before a GPU is involved.

ref64 agrees with torch's float64 autograd through relu(F.batch_norm) to 1e-12; the CPU statement of the kernels' arithmetic
(bn_bwd_cases.kernel_model) stays inside the bar on every case of the list and keeps the exact properties, and three planted mistakes
applied to it do not stay inside -- so the bar is neither unreachable nor loose; the library exports the four entry points and the header
declares them."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bn_bwd_cases as BB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = BB.layer_cases()
SMALL = [k for k in KEYS if not BB.is_big(k)]
NAMES = ("linetr_bn_forward_workspace_bytes", "linetr_bn_forward", "linetr_bn_backward_workspace_bytes", "linetr_bn_backward")


def test_the_list_holds_every_family_width_and_edge():
    assert {k[0] for k in KEYS} == set(BB.FAMILIES)
    for C in BB.CHANNELS:
        assert {k[2] for k in KEYS if k[1] == C and k[6] == (C,) * 4 and k[4] == BB.TRAIN} >= set(BB.ROWS)
        for t in range(4):                                     # z, y, g, dz each at C, C + 4 and 2 C
            assert {k[6][t] for k in KEYS if k[1] == C} == {C, C + 4, 2 * C}, (C, t)
    for fam in BB.PLAIN:
        assert {k[1] for k in KEYS if k[0] == fam} >= set(BB.CHANNELS), fam
    assert {k[2] for k in KEYS if BB.is_big(k)} == set(BB.BIG_ROWS) and {k[2] for k in KEYS if k[2] == 1}
    assert any(k[4] == BB.EVAL for k in KEYS) and any(not k[3] for k in KEYS)
    assert {BB.n_chunks(r) for r in BB.ROWS + BB.BIG_ROWS} >= {1, 2, 4, 5, 511, 512}


@pytest.mark.parametrize("family", BB.FAMILIES)
def test_ref64_is_torchs_float64_autograd(family):
    """the formulae against autograd through relu(F.batch_norm) in double, with the case's mask: 1e-12 of the largest entry"""
    for key in SMALL:
        if key[0] != family or key[2] == 1:
            continue
        c = BB.layer_case(*key)
        C = c["C"]
        z, gamma, beta = (c[k].double().requires_grad_() for k in ("z", "gamma", "beta"))
        with torch.enable_grad():
            y = F.batch_norm(z, c["running"][:C].double(), c["running"][C:].double(), gamma, beta, c["mode"] == BB.TRAIN, 0.1, BB.EPS)
            if c["relu"]:
                y = y * (c["y_in"] > 0)                    # the case's mask (the float32 forward's), not the float64 one
            y.backward(c["g"].double())
        for k, t in (("dz", z.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
            ref = c["ref64"][k]
            assert (t - ref).abs().max().item() <= 1e-12 * max(ref.abs().max().item(), 1.0), (key, k)
        if c["relu"]:                                      # and the two forwards open the same activations but for roundings at 0
            assert ((c["y64"] > 0) != (c["y_in"] > 0)).float().mean().item() < 1e-3, key


def check_model(key):
    c = BB.layer_case(*key)
    got = BB.kernel_model(c)
    rows = BB.backward_errors(got, c)
    bad = [f"{key}: {m}" for m in BB.failures(rows)] + [f"{key}: {m}" for m in BB.exact_failures(got, c)]
    bad += [f"{key}: {m}" for m in BB.failures(BB.saved_errors(dict(save_mean=got["mean"], save_invstd=got["invstd"]), c))]
    return bad, BB.worst(rows)


@pytest.mark.parametrize("family", BB.FAMILIES)
def test_kernel_model_is_inside_the_bar(family):
    bad = []
    for key in SMALL:
        if key[0] == family:
            b, w = check_model(key)
            bad += b
            print(f"bn_bwd model {key}: worst unit {w[0]} err {w[2]:.3e} bar {w[3]:.3e}")
    assert not bad, "\n".join(bad)


def test_kernel_model_is_inside_the_bar_at_many_rows():
    bad = []
    for key in KEYS:
        if BB.is_big(key):
            bad += check_model(key)[0]
    assert not bad, "\n".join(bad)


def _pick(family, C):
    """the ReLU case of the list in training mode with that family and width that has the most rows"""
    return max((k for k in SMALL if k[0] == family and k[1] == C and k[3] and k[4] == BB.TRAIN), key=lambda k: k[2])


PLANTED = [(m, _pick(f, C)) for m in ("no_mask", "no_dgamma", "unbiased_n") for f, C in (("workload", 4), ("workload", 256), ("integer", 100), ("offset", 512))]


@pytest.mark.parametrize("mistake,key", PLANTED)
def test_planted_mistake_is_outside_the_bar(mistake, key):
    """the same model with one mistake: a tile of dz leaves the bar (and, for the dropped mask, dgamma and dbeta too), while the clean
    model stays inside"""
    c = BB.layer_case(*key)
    assert not BB.failures(BB.backward_errors(BB.kernel_model(c), c))
    failed = [r for r in BB.backward_errors(BB.kernel_model(c, mistake), c) if not r[2] <= r[3]]
    assert any(isinstance(r[0], int) for r in failed), (mistake, key, "no tile of dz left the bar")
    if mistake == "no_mask":
        assert {r[0] for r in failed} >= {"dgamma", "dbeta"}, (mistake, key)


def test_library_exports_and_header_declares_the_entry_points():
    from linetr_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in NAMES:
        assert name in nat.ABI and re.search(r"\b%s\(" % name, header), name
    assert "#define LINETR_ABI_VERSION 6" in header
    L = nat.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.linetr_bn_forward_workspace_bytes(8000, 512) > 0 and L.linetr_bn_backward_workspace_bytes(8000, 512) > 0
    for rows, C in ((64, 0), (64, 2), (64, 34), (64, 516), ((1 << 30) + 1, 64)):     # shapes the entry points refuse
        assert L.linetr_bn_forward_workspace_bytes(rows, C) == 0 and L.linetr_bn_backward_workspace_bytes(rows, C) == 0, (rows, C)
