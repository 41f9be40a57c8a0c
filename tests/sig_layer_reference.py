"""The signature layer and its stack (AttentionalPropagation and SelfAttentionalLayer of the reference, models/line_transformer.py:139-183)
restated in stock torch, with the reference's state_dict names; seeded weights and inputs; the runs whose float64 results are the
references of tests/test_gpu_sig_layer.py and whose float32 results give its bars; the signature network with the descriptor head and
the criterion on top.  tests/test_sig_layer_cpu.py pins the restatement to the real reference through tests/golden/sig_layer.npz.
Test infrastructure only (tools/sig_layer_report.py reuses it).

    layer    message = merge(attention(proj0(x), proj1(source), proj2(source)))        (channel c of a projection is (d, h) = (c // 4, c % 4))
             delta = conv3(relu(bn(conv0(cat([x, message])))))                          conv0: 512 -> 512, bn over all B n positions, conv3: 512 -> 256
    stack    x <- x + layer(x, x), layer after layer

The bar of a tensor, in the project's form:  max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

FACTOR = 8
D = 256
LAYER_SHAPES = {"attn.merge.weight": (D, D, 1), "attn.merge.bias": (D,), "attn.proj.0.weight": (D, D, 1), "attn.proj.0.bias": (D,),
                "attn.proj.1.weight": (D, D, 1), "attn.proj.1.bias": (D,), "attn.proj.2.weight": (D, D, 1), "attn.proj.2.bias": (D,),
                "mlp.0.weight": (2 * D, 2 * D, 1), "mlp.0.bias": (2 * D,), "mlp.1.weight": (2 * D,), "mlp.1.bias": (2 * D,),
                "mlp.1.running_mean": (2 * D,), "mlp.1.running_var": (2 * D,), "mlp.1.num_batches_tracked": (),
                "mlp.3.weight": (D, 2 * D, 1), "mlp.3.bias": (D,)}
BUFFERS = ("mlp.1.running_mean", "mlp.1.running_var", "mlp.1.num_batches_tracked")
PARAMS = tuple(k for k in LAYER_SHAPES if k not in BUFFERS)
MATRICES = tuple(k for k in PARAMS if len(LAYER_SHAPES[k]) == 3)
VECTORS = tuple(k for k in PARAMS if len(LAYER_SHAPES[k]) == 1)


def layer_state_dict(rs):
    """one layer's state dict drawn from the np.random.RandomState `rs`, in LAYER_SHAPES' order: weights N(0, 1 / K), biases in
    (-0.5, 0.5), the BatchNorm weight in (0.5, 1.5) and bias N(0, 0.3^2) -- away from 1 and 0 --, running statistics away from 0 and 1"""
    sd = {}
    for key, shape in LAYER_SHAPES.items():
        if key.endswith("num_batches_tracked"):
            sd[key] = np.array(0, dtype=np.int64)
        elif key.endswith("running_var") or key == "mlp.1.weight":
            sd[key] = rs.uniform(0.5, 1.5, shape).astype(np.float32)
        elif key.endswith("running_mean") or key == "mlp.1.bias":
            sd[key] = (0.3 * rs.standard_normal(shape)).astype(np.float32)
        elif len(shape) == 3:
            sd[key] = (rs.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        else:
            sd[key] = rs.uniform(-0.5, 0.5, shape).astype(np.float32)
    return sd


def stack_state_dict(rs, n_layers):
    return {f"layers.{i}.{key}": val for i in range(n_layers) for key, val in layer_state_dict(rs).items()}


def tensors(sd, dtype=None):
    """a NumPy state dict as torch tensors (floating entries at `dtype` when given)"""
    out = {}
    for key, val in sd.items():
        t = torch.from_numpy(np.array(val))
        out[key] = t.to(dtype) if dtype is not None and t.is_floating_point() else t
    return out


class Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.merge = nn.Conv1d(D, D, 1)
        self.proj = nn.ModuleList([nn.Conv1d(D, D, 1) for _ in range(3)])

    def forward(self, query, key, value):
        B = query.shape[0]
        q, k, v = (conv(t).reshape(B, 64, 4, -1) for conv, t in zip(self.proj, (query, key, value)))
        prob = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) * 0.125, dim=-1)
        return self.merge(torch.einsum("bhnm,bdhm->bdhn", prob, v).reshape(B, D, -1))


class Layer(nn.Module):
    def __init__(self):
        super().__init__()
        self.attn = Attention()
        self.mlp = nn.Sequential(nn.Conv1d(2 * D, 2 * D, 1), nn.BatchNorm1d(2 * D), nn.ReLU(), nn.Conv1d(2 * D, D, 1))

    def forward(self, x, source):
        return self.mlp(torch.cat([x, self.attn(x, source, source)], dim=1))


class Stack(nn.Module):
    def __init__(self, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([Layer() for _ in range(n_layers)])

    def forward(self, x):
        for layer in self.layers:
            x = x + layer(x, x)
        return x


def _np64(t):
    return t.detach().double().cpu().numpy()


def _collect(module, out):
    """gradients of every parameter, and the buffers after the call, under their state_dict names"""
    for key, p in module.named_parameters():
        out[key] = _np64(p.grad)
    for key, b in module.named_buffers():
        out["after." + key] = b.detach().cpu().numpy().astype(np.float64 if b.is_floating_point() else np.int64)
    return out


def run_layer(sd, x, source, upstream, dtype, train=True, device="cpu"):
    """One layer differentiated by torch at `dtype`; source None: the layer on (x, x).  dict of float64 arrays: delta, dx, d_source
    (absent for source None), the parameter gradients under their names, after.<buffer>."""
    mod = Layer().to(dtype)
    mod.load_state_dict(tensors(sd, dtype), strict=True)
    mod = mod.to(device).train(train)
    xt = torch.tensor(x, dtype=dtype, device=device, requires_grad=True)
    st = xt if source is None else torch.tensor(source, dtype=dtype, device=device, requires_grad=True)
    with torch.enable_grad():
        delta = mod(xt, st)
        delta.backward(torch.tensor(upstream, dtype=dtype, device=device))
    out = {"delta": _np64(delta), "dx": _np64(xt.grad)}
    if source is not None:
        out["d_source"] = _np64(st.grad)
    return _collect(mod, out)


def run_stack(sd, n_layers, x, upstream, dtype, train=True, device="cpu"):
    """The stack differentiated by torch at `dtype`: out, dx, the parameter gradients, after.<buffer>"""
    mod = Stack(n_layers).to(dtype)
    mod.load_state_dict(tensors(sd, dtype), strict=True)
    mod = mod.to(device).train(train)
    xt = torch.tensor(x, dtype=dtype, device=device, requires_grad=True)
    with torch.enable_grad():
        y = mod(xt)
        y.backward(torch.tensor(upstream, dtype=dtype, device=device))
    return _collect(mod, {"out": _np64(y), "dx": _np64(xt.grad)})


def bar_of(ref32, ref64):
    return FACTOR * max(np.abs(ref32 - ref64).max(), 2.0 ** -23 * np.abs(ref64).max())


def ratios(got, ref64, ref32):
    """[(tensor, max |got - ref64|, bar)] over the floating tensors of ref64 (`got` must carry every one of them)"""
    rows = []
    for key, r64 in ref64.items():
        if r64.dtype != np.float64:
            continue
        g = np.asarray(got[key], dtype=np.float64)
        assert g.shape == r64.shape, (key, g.shape, r64.shape)
        rows.append((key, np.abs(g - r64).max(), bar_of(ref32[key], r64)))
    return rows


def failures(rows):
    return [f"{key}: error {e:.3e} > bar {b:.3e} (x{e / b if b else float('inf'):.2f})" for key, e, b in rows if not e <= b]


# ---- the cases -------------------------------------------------------------------------------------------------------------------

LAYER_SHAPES_TESTED = ((2, 33), (3, 129), (2, 1))       # (B, n): the fixture's; across the attention's 128-row tile; one sub-line per item
FIXTURE_SEED, FIXTURE_SHAPE = 31, (2, 33)


@functools.lru_cache(maxsize=None)
def layer_case(B, n, seed=FIXTURE_SEED, shared=False):
    """(state dict, x, source or None, upstream): seeded; (2, 33, FIXTURE_SEED) is what tests/golden/make_golden_sig_layer.py draws"""
    rs = np.random.RandomState(seed)
    sd = layer_state_dict(rs)
    x = rs.standard_normal((B, D, n)).astype(np.float32)
    source = rs.standard_normal((B, D, n)).astype(np.float32)
    upstream = rs.standard_normal((B, D, n)).astype(np.float32)
    return sd, x, (None if shared else source), upstream


@functools.lru_cache(maxsize=None)
def stack_case(n_layers=2, B=2, n=33, seed=FIXTURE_SEED + 1):
    rs = np.random.RandomState(seed)
    sd = stack_state_dict(rs, n_layers)
    x = rs.standard_normal((B, D, n)).astype(np.float32)
    upstream = rs.standard_normal((B, D, n)).astype(np.float32)
    return sd, x, upstream


@functools.lru_cache(maxsize=None)
def layer_refs(B, n, train=True, shared=False):
    sd, x, source, g = layer_case(B, n, shared=shared)
    return run_layer(sd, x, source, g, torch.float64, train), run_layer(sd, x, source, g, torch.float32, train)


@functools.lru_cache(maxsize=None)
def stack_refs():
    sd, x, g = stack_case()
    return run_stack(sd, 2, x, g, torch.float64), run_stack(sd, 2, x, g, torch.float32)


# ---- the signature network under the head and the criterion ---------------------------------------------------------------------------

NET_LAYERS, NET_B, NET_N, NET_SEED, NET_INPUT_SEED, NET_LR = 7, 2, 33, 77, 5, 0.05


@functools.lru_cache(maxsize=None)
def network_case(B=NET_B, n=NET_N):
    """Seven layers + final_proj, two views of B items of n sub-lines (the tests': 2 of 33) with a planted ground truth: view 1 holds view 0's
    sub-lines in another order with noise, the sub-lines of an item share a component (so that an anchor's negatives lie within the
    criterion's margin of its positive: every anchor has a semi-hard negative), and mat_assign_sublines [B, n+1, n+1] matches each
    sub-line to itself.  The layers'
    last convolutions are drawn eight times smaller than layer_state_dict draws them, so that seven residual layers keep the features'
    scale.  Returns (stack state dict, head weight [256,256,1], head bias [256], x0, x1 [B,256,n], assign)."""
    rs = np.random.RandomState(NET_SEED)
    sd = stack_state_dict(rs, NET_LAYERS)
    for i in range(NET_LAYERS):
        sd[f"layers.{i}.mlp.3.weight"] = (sd[f"layers.{i}.mlp.3.weight"] / 8).astype(np.float32)
        sd[f"layers.{i}.mlp.3.bias"] = (sd[f"layers.{i}.mlp.3.bias"] / 8).astype(np.float32)
    W = (rs.standard_normal((D, D, 1)) / 16).astype(np.float32)
    b = rs.uniform(-0.05, 0.05, D).astype(np.float32)
    rs = np.random.RandomState(NET_INPUT_SEED)
    x0 = (rs.standard_normal((B, D, 1)) + 0.5 * rs.standard_normal((B, D, n))).astype(np.float32)
    x1 = np.empty_like(x0)
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    for i in range(B):
        perm = rs.permutation(n)
        x1[i] = x0[i][:, perm] + 0.5 * rs.standard_normal((D, n)).astype(np.float32)
        assign[i, perm, np.arange(n)] = 1.0          # sub-line perm[j] of view 0 is sub-line j of view 1
    return sd, W, b, x0, x1, assign


def build_network(dtype, device="cpu"):
    sd, W, b, _, _, _ = network_case()
    stack = Stack(NET_LAYERS).to(dtype)
    stack.load_state_dict(tensors(sd, dtype), strict=True)
    head = nn.Conv1d(D, D, 1).to(dtype)
    head.load_state_dict(tensors({"weight": W, "bias": b}, dtype))
    return stack.to(device).train(), head.to(device)


def network_loss(stack, head, x0, x1, assign):
    """the criterion (loss_grad_reference.torch_criterion) on normalize(final_proj(stack(x))) of both views: (loss, V)"""
    import loss_grad_reference as LG
    d0, d1 = (F.normalize(head(stack(x)), p=2, dim=1) for x in (x0, x1))
    loss, _, _, V = LG.torch_criterion(d0, d1, assign)
    return loss, V


def run_network(dtype, device="cpu", sgd_lr=None):
    """loss.backward() through the network at `dtype`.  dict: loss, V, dx0, dx1, the gradients of the stack's parameters under their names and
    of the head under final_proj.*; with `sgd_lr` also loss_after: the loss of a second forward after one plain SGD step."""
    _, _, _, x0, x1, assign = network_case()
    stack, head = build_network(dtype, device)
    a0, a1 = (torch.tensor(x, dtype=dtype, device=device, requires_grad=True) for x in (x0, x1))
    at = torch.tensor(assign, dtype=dtype, device=device)
    with torch.enable_grad():
        loss, V = network_loss(stack, head, a0, a1, at)
        loss.backward()
    out = {"loss": float(loss.detach()), "V": int(V), "dx0": _np64(a0.grad), "dx1": _np64(a1.grad)}
    for key, p in stack.named_parameters():
        out[key] = _np64(p.grad)
    for key, p in head.named_parameters():
        out["final_proj." + key] = _np64(p.grad)
    if sgd_lr is not None:
        with torch.no_grad():
            for p in list(stack.parameters()) + list(head.parameters()):
                p -= sgd_lr * p.grad
            out["loss_after"] = float(network_loss(stack, head, a0.detach(), a1.detach(), at)[0])
    return out


@functools.lru_cache(maxsize=None)
def network_refs():
    return run_network(torch.float64, sgd_lr=NET_LR), run_network(torch.float32)
