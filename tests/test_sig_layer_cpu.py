"""CPU: pins tests/sig_layer_reference.py -- the restatement of the reference's AttentionalPropagation and SelfAttentionalLayer that the GPU
tests compare against -- to the real reference through tests/golden/sig_layer.npz and sig_layer_stack.npz (made by
tests/golden/make_golden_sig_layer.py from the reference's own modules), checks the state_dict names and shapes of the native modules
against the reference's, and asserts the premises of the GPU test of the whole signature network: every anchor of the planted ground
truth has a semi-hard negative that float32 cannot exchange for another, and one SGD step lowers the float64 loss."""
import numpy as np
import torch

from helpers import load
import loss_grad_reference as LG
import sig_layer_reference as SL


def check_fixture(f, got):
    stored = [k for k in f.files if k != "state_dict_keys" and not k.endswith("_f32_err")]
    assert sorted(stored) == sorted(got), set(stored) ^ set(got)
    for key in stored:
        want, have = f[key], got[key]
        if have.ndim == 3 and have.shape[2] == 1:
            have = have[::7, ::5, 0]                                   # a weight matrix: the stored sub-grid
        assert have.shape == want.shape and have.dtype == want.dtype, key
        if want.dtype == np.int64:
            assert np.array_equal(have, want), key
            continue
        assert np.abs(have - want).max() <= 1e-10 * max(np.abs(want).max(), 1.0), (key, np.abs(have - want).max())
        assert float(f[key + "_f32_err"]) >= 0.0


def test_layer_restatement_reproduces_the_reference():
    f = load("sig_layer")
    sd, x, source, g = SL.layer_case(*SL.FIXTURE_SHAPE)
    check_fixture(f, SL.run_layer(sd, x, source, g, torch.float64))
    assert int(f["after.mlp.1.num_batches_tracked"]) == 1
    # the float32 yardstick the fixture carries is the restatement's own, to the digits float32 noise leaves
    r64, r32 = SL.layer_refs(*SL.FIXTURE_SHAPE)
    for key in ("delta", "dx", "mlp.1.weight", "mlp.0.weight"):
        ours, theirs = np.abs(r32[key] - r64[key]).max(), float(f[key + "_f32_err"])
        assert 0.25 * theirs <= ours <= 4.0 * theirs, (key, ours, theirs)


def test_stack_restatement_reproduces_the_reference():
    f = load("sig_layer_stack")
    sd, x, g = SL.stack_case()
    check_fixture(f, SL.run_stack(sd, 2, x, g, torch.float64))


def test_state_dict_key_sets_are_the_references():
    layer_keys, stack_keys = list(load("sig_layer")["state_dict_keys"]), list(load("sig_layer_stack")["state_dict_keys"])
    assert sorted(SL.LAYER_SHAPES) == sorted(layer_keys) and sorted(SL.Layer().state_dict()) == sorted(layer_keys)
    assert sorted(SL.Stack(2).state_dict()) == sorted(stack_keys)
    assert all(tuple(t.shape) == SL.LAYER_SHAPES[k] for k, t in SL.Layer().state_dict().items())
    # the restatement saves what it loaded
    sd = SL.layer_case(*SL.FIXTURE_SHAPE)[0]
    mod = SL.Layer()
    mod.load_state_dict(SL.tensors(sd), strict=True)
    assert all(np.array_equal(mod.state_dict()[k].numpy(), sd[k]) for k in sd)


def test_native_modules_carry_the_references_state_dict():
    from linetr_amd.train_ops import AttentionalPropagation, SelfAttentionalLayer
    layer_keys, stack_keys = list(load("sig_layer")["state_dict_keys"]), list(load("sig_layer_stack")["state_dict_keys"])
    layer = AttentionalPropagation()
    assert sorted(layer.state_dict()) == sorted(layer_keys)
    assert all(tuple(t.shape) == SL.LAYER_SHAPES[k] for k, t in layer.state_dict().items())
    assert not bool(layer.mlp[3].bias.any())                           # the reference zeroes the last bias
    assert sorted(SelfAttentionalLayer(256, ["self", "self"]).state_dict()) == sorted(stack_keys)
    assert len(SelfAttentionalLayer().layers) == 7
    # a reference `selfattn.*` state dict loads with strict=True; another prefix in the same dict is ignored
    sd, _, _ = SL.stack_case()
    full = {"selfattn." + k: v for k, v in SL.tensors(sd).items()}
    full["final_proj.weight"] = torch.zeros(256, 256, 1)
    stack = SelfAttentionalLayer.from_line_transformer(full)
    assert len(stack.layers) == 2 and all(torch.equal(stack.state_dict()[k], t) for k, t in SL.tensors(sd).items())
    one = AttentionalPropagation.from_line_transformer(full, layer=1)
    assert torch.equal(one.mlp[1].weight, torch.from_numpy(sd["layers.1.mlp.1.weight"]))
    for bad in (lambda: AttentionalPropagation(128, 4), lambda: AttentionalPropagation(256, 8)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("another width or head count must be refused")


def test_premises_of_the_network_test():
    """the planted ground truth gives every one of the 2 B n anchors a semi-hard negative; the float64 gap between the chosen negative and
    the runner-up is a thousand times the descriptors' float32 error, so float32 picks the same ones; one SGD step of NET_LR lowers the loss"""
    r64, r32 = SL.network_refs()
    assert r64["V"] == r32["V"] == 2 * SL.NET_B * SL.NET_N
    assert np.isfinite(r64["loss"]) and r64["loss_after"] < r64["loss"] - 0.01, (r64["loss"], r64["loss_after"])
    assert abs(r32["loss"] - r64["loss"]) <= 1e-6
    stack, head = SL.build_network(torch.float64)
    _, _, _, x0, x1, assign = SL.network_case()
    with torch.no_grad():
        d64 = [torch.nn.functional.normalize(head(stack(torch.tensor(x, dtype=torch.float64))), dim=1).numpy() for x in (x0, x1)]
    stack, head = SL.build_network(torch.float32)
    with torch.no_grad():
        d32 = [torch.nn.functional.normalize(head(stack(torch.tensor(x))), dim=1).numpy() for x in (x0, x1)]
    err = max(np.abs(a - b).max() for a, b in zip(d32, d64))
    gap = LG.selection_gap(d64[0], d64[1], assign)
    assert gap >= 1000 * err, (gap, err)
    assert all(np.isfinite(v).all() for v in r64.values() if isinstance(v, np.ndarray))
