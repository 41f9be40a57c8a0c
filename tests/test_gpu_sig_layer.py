"""GPU: the signature layer and its stack composed of native pieces under autograd (linetr_amd.train_ops.AttentionalPropagation /
SelfAttentionalLayer: MultiHeadedAttention, pointwise_linear, batch_norm_relu), and the signature network under the descriptor head and
the criterion, against the stock-torch restatement of tests/sig_layer_reference.py in float64 -- which tests/test_sig_layer_cpu.py pins
to the real reference through tests/golden/sig_layer*.npz.

The bar of a tensor is 8 x max(float32 restatement's error against float64, 2^-23 max |float64|); outputs, input gradients, every
parameter's .grad and the BatchNorm running statistics each have their own.  Measured on the MI355X: profiles/sig_layer_errors.txt."""
import numpy as np
import pytest
import torch

from helpers import load
import sig_layer_reference as SL

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def native_layer(sd, train=True):
    from linetr_amd.train_ops import AttentionalPropagation
    mod = AttentionalPropagation.from_line_transformer({"selfattn.layers.0." + k: v for k, v in SL.tensors(sd).items()}).cuda()
    return mod.train(train)


def native_stack(sd):
    from linetr_amd.train_ops import SelfAttentionalLayer
    return SelfAttentionalLayer.from_line_transformer({"selfattn." + k: v for k, v in SL.tensors(sd).items()}).cuda().train()


def collect(mod, out):
    """gradients and buffers of a native module under the restatement's keys, as CPU arrays"""
    for key, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, key
        out[key] = p.grad.cpu().numpy()
    for key, b in mod.state_dict().items():
        if "running_" in key or key.endswith("num_batches_tracked"):
            out["after." + key] = b.cpu().numpy()
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def check(got, ref64, ref32, label):
    assert sorted(got) == sorted(ref64), set(got) ^ set(ref64)
    for key, r in ref64.items():
        if r.dtype == np.int64:
            assert np.array_equal(got[key], r), (label, key, got[key], r)
    rows = SL.ratios(got, ref64, ref32)
    for key, e, b in rows:
        print(f"sig_layer {label} {key}: err {e:.3e} bar {b:.3e} ratio {e / b if b else 0.0:.3f}")
    assert all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in got.values())
    assert not SL.failures(rows), (label, SL.failures(rows))


def run_native_layer(sd, x, source, g, train=True):
    mod = native_layer(sd, train)
    xt = dev(x).requires_grad_()
    st = xt if source is None else dev(source).requires_grad_()
    with torch.enable_grad():
        delta, prob = mod(xt, st)
        assert prob is None and delta.shape == x.shape and delta.grad_fn is not None
        delta.backward(dev(g))
    out = {"delta": delta, "dx": xt.grad}
    if source is not None:
        out["d_source"] = st.grad
    return collect(mod, out)


@pytest.mark.parametrize("B,n", SL.LAYER_SHAPES_TESTED)
def test_layer_forward_and_backward(B, n):
    """one AttentionalPropagation in .train(): delta, dx, d_source, all fourteen parameter gradients, the running statistics and
    num_batches_tracked after the call.  [3, 256, 129] crosses the attention's 128-row tile; [2, 256, 1]: one sub-line per item (the
    attention's P is 1) and a BatchNorm over two rows."""
    sd, x, source, g = SL.layer_case(B, n)
    ref64, ref32 = SL.layer_refs(B, n)
    check(run_native_layer(sd, x, source, g), ref64, ref32, f"layer [{B}, 256, {n}]")


def test_layer_on_itself():
    """layer(x, x): x feeds the three projections and the concatenation; autograd adds their gradients"""
    sd, x, _, g = SL.layer_case(2, 33, shared=True)
    ref64, ref32 = SL.layer_refs(2, 33, shared=True)
    check(run_native_layer(sd, x, None, g), ref64, ref32, "layer(x, x)")


def test_layer_in_eval_mode():
    """.eval(): the running statistics normalise and stay; the backward is the eval-mode one"""
    sd, x, source, g = SL.layer_case(2, 33)
    ref64, ref32 = SL.layer_refs(2, 33, train=False)
    got = run_native_layer(sd, x, source, g, train=False)
    check(got, ref64, ref32, "layer eval")
    assert np.array_equal(got["after.mlp.1.running_mean"], sd["mlp.1.running_mean"]) and int(got["after.mlp.1.num_batches_tracked"]) == 0


def test_layer_against_the_fixture():
    """the real reference's numbers (tests/golden/sig_layer.npz): outputs, 1-D gradients, the weight gradients on the stored sub-grid"""
    f = load("sig_layer")
    sd, x, source, g = SL.layer_case(*SL.FIXTURE_SHAPE)
    got = run_native_layer(sd, x, source, g)
    for key in (k for k in f.files if k != "state_dict_keys" and not k.endswith("_f32_err")):
        ref, have = f[key], got[key]
        if have.ndim == 3 and have.shape[2] == 1:
            have = have[::7, ::5, 0]
        if ref.dtype == np.int64:
            assert np.array_equal(have, ref), key
            continue
        bar = SL.FACTOR * max(float(f[key + "_f32_err"]), 2.0 ** -23 * np.abs(ref).max())
        err = np.abs(have.astype(np.float64) - ref).max()
        assert have.shape == ref.shape and err <= bar, (key, err, bar)


def test_two_layer_stack():
    sd, x, g = SL.stack_case()
    ref64, ref32 = SL.stack_refs()
    mod = native_stack(sd)
    xt = dev(x).requires_grad_()
    with torch.enable_grad():
        y = mod(xt)
        assert y.shape == x.shape and y.transpose(1, 2).is_contiguous()          # rows behind the [B, 256, n] view
        y.backward(dev(g))
    check(collect(mod, {"out": y, "dx": xt.grad}), ref64, ref32, "stack of two")


def run_native_network(lr=None):
    """loss.backward() through seven layers + DescriptorHead + descriptor_loss; with lr: one plain SGD step and the loss after it"""
    import linetr_amd.evaluations as E
    from linetr_amd.train_ops import DescriptorHead
    sd, W, b, x0, x1, assign = SL.network_case()
    stack = native_stack(sd)
    head = DescriptorHead.from_line_transformer({"final_proj.weight": torch.from_numpy(W), "final_proj.bias": torch.from_numpy(b)}).cuda()
    crit = E.descriptor_loss()
    a0, a1 = dev(x0).requires_grad_(), dev(x1).requires_grad_()
    target = {"mat_assign_sublines": dev(assign)}
    with torch.enable_grad():
        loss = crit({"line_desc0": head(stack(a0)), "line_desc1": head(stack(a1))}, target)[0]
        loss.backward()
    out = {"loss": float(loss.detach()), "V": crit.last["count"], "dx0": a0.grad.cpu().numpy(), "dx1": a1.grad.cpu().numpy()}
    for key, p in stack.named_parameters():
        assert p.grad is not None, key
        out[key] = p.grad.cpu().numpy()
    for key, p in head.named_parameters():
        assert p.grad is not None, key
        out[key] = p.grad.cpu().numpy()
    if lr is not None:
        with torch.no_grad():
            for p in list(stack.parameters()) + list(head.parameters()):
                p -= lr * p.grad
            out["loss_after"] = float(crit({"line_desc0": head(stack(a0.detach())), "line_desc1": head(stack(a1.detach()))}, target)[0])
    return out


def test_loss_backward_fills_the_signature_network():
    """seven layers + head + criterion at B = 2, n = 33 with the planted ground truth: the loss, the anchors, the gradient of both inputs
    and of all 7 x 14 + 2 parameters; a second run gives the same bits; one SGD step lowers the loss as it does in float64 on the CPU"""
    ref64, ref32 = SL.network_refs()
    got = run_native_network(lr=SL.NET_LR)
    again = run_native_network()
    assert got["V"] == ref64["V"] and abs(got["loss"] - ref64["loss"]) <= 8 * max(abs(ref32["loss"] - ref64["loss"]), 2.0 ** -23 * ref64["loss"])
    arrays = lambda d: {k: v for k, v in d.items() if isinstance(v, np.ndarray)}
    assert len(arrays(got)) == 2 + 7 * 14 + 2
    for key, v in arrays(got).items():
        assert again[key].tobytes() == v.tobytes(), key
    assert again["loss"] == got["loss"]
    check(arrays(got), arrays(ref64), arrays(ref32), "network")
    print(f"sig_layer network: loss {got['loss']:.6f} -> {got['loss_after']:.6f} after one SGD step (float64: {ref64['loss']:.6f} -> {ref64['loss_after']:.6f})")
    assert got["loss_after"] < got["loss"] - 0.01 and abs(got["loss_after"] - ref64["loss_after"]) <= 1e-4
