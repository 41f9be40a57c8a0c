"""CPU (no GPU needed): the float64 closed form of tests/sig_attn_bwd_reference.py equals float64 autograd through the torch statement
on rows (attn_rows), reproduces tests/golden/sig_attn_bwd.npz (which autograd through the REAL reference's attention() wrote:
tests/golden/make_golden_sig_attn_bwd.py) and, where the reference checkout is at hand, autograd through the reference's own attention()
and MultiHeadedAttention in double; the premises of the GPU suite's exact properties hold; the built library exports the entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import load
import sig_attn_bwd_reference as SA

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("LINETR_REFERENCE", "/root/reference")
GRADS = ("o", "dq", "dk", "dv")


def rel(a, b):
    """relative to the output's largest magnitude, or to 1 where the output is a difference of O(1) terms that cancel (the planted
    family's dq and dk, ~1e-13: P is one-hot and dP - delta vanishes; n = 1, where they are exactly 0)"""
    return np.abs(a - b).max() / max(np.abs(b).max(), 1.0)


def fixture_rows(f, key):
    """[2, 64, 4, 33] of the fixture -> [66, 4, 64] rows (image after image)"""
    return SA.from_call_shape(torch.from_numpy(f[key])).numpy()


def fixture_closed_form(f):
    n = f["q"].shape[3]
    parts = [SA.closed_form_image(*(fixture_rows(f, key)[i * n:(i + 1) * n] for key in ("q", "k", "v", "dO"))) for i in range(f["q"].shape[0])]
    return {key: np.concatenate([p[key] for p in parts]) for key in GRADS}


@pytest.mark.parametrize("family", SA.FAMILIES)
def test_closed_form_equals_float64_autograd(family):
    c = SA.case(family, (0, 1, 2, 33, 0, 65, 129, 0))
    for i in c["check"]:
        a, b = int(c["cu"][i]), int(c["cu"][i + 1])
        if a == b:
            continue
        ag = SA.torch_image(*(t[a:b].numpy() for t in (c["q"], c["k"], c["v"], c["dO"])), torch.float64)
        for key in SA.OUTPUTS:
            assert rel(c["ref64"][key][a:b], ag[key]) <= 1e-12, (family, i, key)


def test_fixture_agrees_with_the_closed_form():
    f = load("sig_attn_bwd")
    assert f["q"].shape == (2, 64, 4, 33) and f["q"].dtype == np.float32 and f["dq"].dtype == np.float64
    assert os.path.getsize(os.path.join(HERE, "golden", "sig_attn_bwd.npz")) < 1 << 20
    cf = fixture_closed_form(f)
    for key in GRADS:
        want = fixture_rows(f, key)
        assert rel(cf[key], want) <= 1e-12, key                                   # the reference's own float64 run
        yard = float(f[f"{key}_f32_err"])                                          # the reference's own float32 run against it
        assert 0 < yard < 1e-5 and np.abs(cf[key] - want).max() <= yard, key


def test_closed_form_equals_the_reference_in_double(tmp_path):
    if not os.path.exists(os.path.join(REFERENCE, "models", "line_transformer.py")):
        pytest.skip("the reference checkout is not present")
    cases = {}
    for i, shared in enumerate((False, True)):
        sd, x, src, g = SA.mha_case(shared=shared)
        cases.update({f"mha{i}.{key}": val for key, val in sd.items()})
        cases.update({f"mha{i}.query": x, f"mha{i}.source": src, f"mha{i}.g": g, f"mha{i}.shared": np.array(shared)})
    np.savez(tmp_path / "in.npz", **cases)
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_sig_attn_bwd.py"), "--double", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], check=True, cwd=str(tmp_path))
    got = np.load(tmp_path / "out.npz")
    assert sorted(got["state_dict_keys"].tolist()) == sorted(SA.MHA_KEYS)
    f = load("sig_attn_bwd")
    cf = fixture_closed_form(f)
    for key in GRADS:
        assert rel(cf[key], SA.from_call_shape(torch.from_numpy(got[f"attn.{key}"])).numpy()) <= 1e-12, key
    for i, shared in enumerate((False, True)):
        sd, x, src, g = SA.mha_case(shared=shared)
        mine = SA.torch_mha(sd, x, src, g, torch.float64, shared=shared)
        for key, val in mine.items():
            assert rel(val, got[f"mha{i}.{key}"]) <= 1e-12, (shared, key)


def test_premises_of_the_exact_properties():
    # n = 1: P = 1, o = v, dP = delta, so dq = dk = 0 and dv = dO
    c = SA.case("normal", (1,))
    assert np.array_equal(c["ref64"]["dv"], c["dO"].double().numpy()) and not c["ref64"]["dq"].any() and not c["ref64"]["dk"].any()
    # equal (k = 0): every P is 1 / n, dq = dS k / 8 = 0 and every dv row is the column mean of dO
    for n in SA.POW2:
        c = SA.case("equal", (n,), integer_dO=True)
        dO = c["dO"].double().numpy()
        assert not c["k"].any() and np.array_equal(dO, np.round(dO)) and not c["ref64"]["dq"].any()
        assert np.abs(c["ref64"]["dv"] - dO.sum(axis=0) / n).max() <= 1e-13                       # (float64's own exp(-log n) is 1 / n to 1e-16)
        assert (n & (n - 1)) == 0 and SA.pow2_premise(n) < 0.3
    assert SA.pow2_premise(32) > 0.3 and SA.pow2_premise(256) > 0.5                              # why POW2 is not every power of two
    # planted: P is near one-hot, so dv is almost a scatter of dO rows
    c = SA.case("planted", (65,))
    q, k = c["q"].double().numpy(), c["k"].double().numpy()
    for h in range(4):
        S = (q[:, h] * 0.125) @ k[:, h].T
        P = np.exp(S - S.max(axis=1, keepdims=True))
        P /= P.sum(axis=1, keepdims=True)
        assert P.max(axis=1).min() > 0.99
    # sentinel: the images of one parity hold +-1e4 in every input and in dO; the others are the compared ones
    c = SA.case("sentinel", (0, 33, 65, 2, 0))
    assert c["check"] == [1, 3] and all(float(t[33:98].abs().min()) == SA.SENTINEL for t in (c["q"], c["k"], c["v"], c["dO"]))
    # the ragged batch holds every size the issue lists, an empty image first, in the middle and last
    counts = SA.ragged_counts()
    assert sorted(n for n in counts if n) == sorted(SA.SIZES) and counts[0] == counts[-1] == 0 and counts.count(0) == 3
    for edge in (32, 64, 128):
        assert {edge - 1, edge, edge + 1} <= set(SA.SIZES)


def test_library_exports_the_attention_entry_points():
    from linetr_amd import _native as nat
    L = nat.lib()
    for name in ("linetr_sig_attention_forward", "linetr_sig_attention_backward", "linetr_sig_attention_backward_workspace_bytes"):
        assert name in nat.EXPORTS and hasattr(L, name), name
    assert L.linetr_sig_attention_backward_workspace_bytes(0) >= 0 and L.linetr_sig_attention_backward_workspace_bytes(769) >= 769 * 16
    assert L.linetr_sig_attention_backward_workspace_bytes(-1) == 0
