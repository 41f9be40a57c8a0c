"""CPU (no GPU needed): the references of tests/test_gpu_keyline.py are what they claim to be.  The torch restatement of the reference's
positional encoders, KeylineEncoder and LineTransformer (tests/keyline_reference.py) reproduces tests/golden/keyline.npz and
keyline_matrices.npz, which autograd through the REAL reference wrote (tests/golden/make_golden_keyline.py); the float64 closed forms of
the two new kernel pairs equal float64 autograd, and a planted mistake in each falls outside the bar; the header declares the new entry
points and the built library exports them; train_ops exposes the new surface with the reference's key set."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import load
import keyline_reference as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY_POINTS = ("linetr_input_layer_forward", "linetr_input_layer_backward", "linetr_input_layer_backward_workspace_bytes",
                "linetr_input_layer_chunk_rows", "linetr_token_assemble_forward", "linetr_token_assemble_backward",
                "linetr_token_assemble_backward_workspace_bytes")
NEW_NAMES = ("input_linear", "assemble_tokens", "LinePositionalEncoder", "WordPositionalEncoder", "KeylineEncoder", "TrainableLineTransformer")
# conv biases in front of a BatchNorm: their gradient is zero in exact arithmetic
CANCELLED = tuple(f"klenc.{enc}_position_enc.encoder.{i}.bias" for enc in ("line", "word") for i in (0, 3, 6, 9))


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1.0)


def test_restatement_reproduces_the_fixture():
    f, fm = load("keyline"), load("keyline_matrices")
    for stem in ("keyline", "keyline_matrices"):
        assert os.path.getsize(os.path.join(HERE, "golden", stem + ".npz")) < 1 << 20
    B, n, S = KR.FIXTURE_SHAPE
    assert f["line_desc.0"].shape == (B, 256, n) and f["d_desc.0"].shape == (B, n, S, 256) and f["line_desc.0"].dtype == np.float64
    ref64, ref32 = KR.model_refs()
    keys = f["state_dict_keys"].tolist()
    assert sum(1 for k in keys if "running" not in k and "num_batches" not in k) == 153 and sum(1 for k in keys if k.endswith("running_mean")) == 15
    grads = [k for k in keys if "running" not in k and "num_batches" not in k]
    stored = ["line_desc.0", "line_desc.1", "d_desc.0"] + [g + ".0" for g in grads] + \
             [f"after.{k}.{c}" for k in keys if "running" in k for c in range(KR.FIXTURE_CALLS)]
    n_matrices = 0
    for name in stored:
        key = name.rsplit(".", 1)[0]
        val, mine32 = ref64[name], ref32[name]
        if KR.is_matrix(key, val):
            want, val, mine32, tol = fm[name].astype(np.float64), KR.sub_grid(key, val), KR.sub_grid(key, mine32), 2.0 ** -24
            n_matrices += 1
        else:
            want, tol = f[name], 1e-12
        assert want.shape == val.shape, name
        yard = float(f[name + "_f32_err"])
        bar = KR.FACTOR * max(yard, 2.0 ** -23 * np.abs(want).max())
        assert np.abs(val - want).max() <= tol * max(np.abs(want).max(), 1.0), name      # the float64 runs agree to rounding (of the storage)
        assert 0 < yard < 1e-3 and np.abs(mine32 - want).max() <= bar, name               # and the float32 run sits inside the bar
    assert n_matrices == len(fm.files) == 59      # 2 x 5 + 6 + 7 x 6 + 1
    for c in range(KR.FIXTURE_CALLS):
        for k in keys:
            if k.endswith("num_batches_tracked"):
                assert int(f[f"after.{k}.{c}"]) == c + 1 == int(ref64[f"after.{k}.{c}"]), k
    # the second call moves the buffers on and nothing else
    moved = "after.klenc.line_position_enc.encoder.1.running_mean"
    assert np.array_equal(ref64["line_desc.0"], ref64["line_desc.1"]) and not np.array_equal(f[moved + ".0"], f[moved + ".1"])
    # zero in exact arithmetic, noise in float32: under the same bar as everything else
    for key in CANCELLED:
        assert np.abs(f[key + ".0"]).max() < 1e-12 < float(f[key + ".0_f32_err"]), key
    assert np.abs(f["klenc.cls_token.0"]).max() > 1e-3


def test_a_planted_mistake_in_the_restatement_is_caught():
    f = load("keyline")
    wrong = KR.run_model(torch.float64, calls=1, mistake="no_word_position")
    bar = KR.FACTOR * max(float(f["line_desc.0_f32_err"]), 2.0 ** -23 * np.abs(f["line_desc.0"]).max())
    assert np.abs(wrong["line_desc.0"] - f["line_desc.0"]).max() > 100 * bar


def test_input_layer_closed_form_equals_float64_autograd():
    for Kin, N, rows in ((1, 4, 1), (3, 32, 7), (5, 32, 300), (8, 64, 65)):
        c = KR.il_case(Kin, N, rows)
        ag = KR.il_torch(c["x"], c["W"], c["b"], c["g"], torch.float64)
        for key in KR.IL_OUTPUTS:
            assert rel(c["ref64"][key], ag[key]) <= 1e-12, (Kin, N, rows, key)
        wrong = KR.il_closed_form(c["x"], c["W"], c["b"], c["g"], mistake="db_mean")
        if rows > 1:
            assert KR.failures(KR.ratios(wrong, c["ref64"], c["ref32"], ("db",)))
        assert not KR.failures(KR.ratios(c["ref32"], c["ref64"], c["ref32"]))
    # integer data: float32 holds every result exactly
    c = KR.il_case(5, 32, 515, integer=True)
    for key in KR.IL_OUTPUTS:
        assert np.array_equal(c["ref64"][key], c["ref64"][key].astype(np.float32)) and np.array_equal(c["ref64"][key], c["ref32"][key]), key


@pytest.mark.parametrize("family", KR.TA_FAMILIES)
def test_token_assembly_closed_form_equals_float64_autograd(family):
    for L, S in ((1, 1), (3, 2), (9, 21)):
        c = KR.ta_case(family, L, S)
        ag = KR.ta_torch(c["desc"], c["pos"], c["cls"], c["dx"], torch.float64)
        for key in KR.TA_OUTPUTS:
            assert rel(c["ref64"][key], ag[key]) <= 1e-12, (family, L, S, key)
        assert np.array_equal(c["ref64"]["x"][:, 1:].astype(np.float32), c["desc"] + c["pos"]) or family != "integer"
        wrong = KR.ta_closed_form(c["desc"], c["pos"], c["cls"], c["dx"], mistake="dcls_all_slots")
        assert KR.failures(KR.ratios(wrong, c["ref64"], c["ref32"], ("dcls",))), (family, L, S)
    if family == "sentinel":
        c = KR.ta_case(family, 9, 21)
        assert np.abs(c["ref64"]["dcls"]).max() < 100 and np.abs(c["ref64"]["dtok"]).min() == KR.SENTINEL


def test_header_declares_and_library_exports_the_entry_points():
    from linetr_amd import _native as nat
    hdr = open(os.path.join(HERE, "..", "include", "linetr_hip.h")).read()
    L = nat.lib()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in nat.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define LINETR_ABI_VERSION 6\b", hdr) and L.linetr_abi_version() == 6
    chunk = L.linetr_input_layer_chunk_rows()
    assert 16 <= chunk <= 4096
    # the workspace grows by one partial [Kin + 1][N] per chunk, and a refused shape has none
    ws = L.linetr_input_layer_backward_workspace_bytes
    assert ws(chunk, 32, 3) == ws(1, 32, 3) < ws(chunk + 1, 32, 3) and ws(10 * chunk, 64, 8) - ws(chunk, 64, 8) >= 9 * 9 * 64 * 4
    assert ws(5, 30, 3) == ws(5, 68, 3) == ws(5, 32, 0) == ws(5, 32, 9) == ws(-1, 32, 3) == 0
    wt = L.linetr_token_assemble_backward_workspace_bytes
    assert wt(-1) == 0 and wt(1) > 0 and wt(4096) - wt(1) >= 1024


def test_train_ops_exposes_the_surface_with_the_references_keys():
    from linetr_amd import train_ops as T
    for name in NEW_NAMES:
        assert hasattr(T, name), name
    f = load("keyline")
    model = T.TrainableLineTransformer()
    assert sorted(model.state_dict()) == sorted(f["state_dict_keys"].tolist())
    sd, _, _ = KR.model_case()
    model.load_state_dict(KR.tensors(sd), strict=True)                      # the reference's shapes
    ref = KR.Model()
    ref.load_state_dict(model.state_dict(), strict=True)                     # and back
    assert len(list(model.parameters())) == 153
    with pytest.raises(ValueError):
        T.LinePositionalEncoder(256, [30, 64, 128, 256])
    with pytest.raises(ValueError):
        T.WordPositionalEncoder(256, [32, 64, 100, 256])
    enc = T.WordPositionalEncoder.from_line_transformer(KR.tensors(sd))
    assert torch.equal(enc.encoder[12].weight, torch.from_numpy(sd["klenc.word_position_enc.encoder.12.weight"]))
    kl = T.KeylineEncoder.from_line_transformer(model)
    assert torch.equal(kl.cls_token, model.klenc.cls_token) and len(kl.desc_layers) == 1
    # empty klines: the reference's default return, on any device
    out = model({"klines": torch.empty(0)})
    assert out["line_desc"].shape == (1, 256, 0) and out["sublines"].shape == (1, 0, 2, 2)
