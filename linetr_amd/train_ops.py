"""Differentiable native layers: torch.autograd.Functions on top of the exact-fp32 kernels of csrc/lt_linbwd.h and csrc/lt_attnbwd.h, the
BatchNorm kernels of csrc/lt_bnbwd.h, the pooling / LayerNorm / GELU kernels of csrc/lt_descbwd.h and the input-layer / token-assembly
kernels of csrc/lt_posbwd.h, and the signature network, the descriptive layer, the positional encoders and the whole network composed
of them.

    pointwise_linear(x, weight, bias=None, relu=False)   y = act(x W^T + b): Conv1d(k=1) ([N, K, 1] weight, x [B, K, n]) or Linear
                                                         ([N, K] weight, x [rows, K]) on the UNFOLDED state_dict weight, with the
                                                         data, weight and bias gradients native (Engine.linear_forward / _backward)
    DescriptorHead                                       line_desc = F.normalize(final_proj(x), p=2, dim=1)
                                                         (models/line_transformer.py:245-246 of the reference), forward and backward
                                                         native (Engine.head_forward / head_backward)
    signature_attention(query, key, value)               the reference's attention() (:132-136), softmax(q^T k / 8) v per item and head, on
                                                         its [B, 64, 4, n] call shape, without the n x n `prob`; flash-style backward
                                                         (Engine.sig_attention_forward / _backward)
    MultiHeadedAttention                                 the reference's module (:139-154): three projections, attention, merge, with its
                                                         state_dict; every gradient native
    batch_norm_relu(z, bn, relu=True)                    relu?(bn(z)) for an nn.BatchNorm1d `bn`, on batch statistics in .train() (the running
                                                         statistics and num_batches_tracked move as torch moves them) and on the running
                                                         ones in .eval(); dz, dgamma and dbeta native (Engine.bn_forward / bn_backward)
    AttentionalPropagation                               the reference's signature layer (:157-166): attn(x, source, source), cat, Conv1d(512,
                                                         512), BatchNorm1d(512), ReLU, Conv1d(512, 256), with its state_dict
    SelfAttentionalLayer                                 the reference's stack (:168-183): kline_desc + delta, layer after layer
    gelu(x)                                              F.gelu in its erf form, from the saved pre-activation (Engine.gelu_forward / _backward)
    residual_layer_norm(a, residual, ln)                 ln(a + residual) for an nn.LayerNorm(256) `ln`; the data gradient (of a and of the
                                                         residual), dgamma and dbeta native (Engine.layer_norm_forward / _backward)
    cls_token_pool(x, u)                                 the CLS query row's softmax-weighted mean of the S tokens of every segment and head,
                                                         x [L, S, 256], u [L, 4, 256]; dx and du native (Engine.cls_pool_forward / _backward)
    LineDescriptiveEncoder                               the reference's descriptive layer (:75-91) with its state_dict, in the folded form:
                                                         only the CLS row KeylineEncoder reads is computed; every gradient native
    cls_token_pool(x, u, dropout), residual_layer_norm(a, residual, ln, dropout, site), seed_dropout(seed)
                                                         training-time dropout at the reference's three places, the masks a pure function
                                                         of (seed, call, site, element) that the kernels of csrc/lt_dropout.h generate in the
                                                         forward and again in the backward (Engine.cls_pool_dropout_* / layer_norm_dropout_*)

With linetr_amd.evaluations.descriptor_loss on top of a DescriptorHead on top of a SelfAttentionalLayer, `loss.backward()` fills every
gradient of the signature network -- the eight attention parameters, the two convolutions and the BatchNorm weight and bias of every layer,
the head, and the input features' .grad -- on the device.  Every contraction, softmax, normalisation and reduction in it, forward and
backward, is a native kernel.  What torch still does: data movement (cat, permute / transpose, views, the gather of the attention's
parameters into head-major order and its scatter back, copies of the running statistics into and out of their packed pair), the residual
add kline_desc + delta, the increment of num_batches_tracked, and autograd's own sums where one tensor feeds several consumers (x feeds the
attention's three projections, the concatenation and the residual) -- single float32 adds, as in the reference.  The tensors must live on
a HIP device (there is no CPU path).  The descriptive layer underneath trains the same way: in LineDescriptiveEncoder torch gathers the
per-head slices of the key and value weights, stacks and concatenates the heads, scales q by the exact 1/8 and adds the gradients of the
CLS rows (which feed the query, the tokens and the residual); the rest is native.

    input_linear(x, weight, bias)                        z = x W^T + b for the narrow first layer of a positional encoder (1 <= Kin <= 8 inputs,
                                                         N % 4 == 0, 4 <= N <= 64 outputs): dW and db native, no gradient for x
                                                         (Engine.input_layer_forward / _backward)
    assemble_tokens(desc, pos, cls_token)                the token rows of the descriptive layer, x[:, 0] = cls_token, x[:, 1:] = desc + pos; the
                                                         gradient of desc and pos (one tensor) and of cls_token native
                                                         (Engine.assemble_tokens_forward / _backward)
    LinePositionalEncoder, WordPositionalEncoder         the reference's encoders (:40-73) with their state_dict: input_linear, then
                                                         batch_norm_relu / pointwise_linear per layer, on [rows, C] rows
    KeylineEncoder                                       the reference's module (:93-130): both encoders, assemble_tokens, the last descriptive layer
    TrainableLineTransformer                             the reference's LineTransformer (:185-249) under its full key set, on its input dict:
                                                         klenc, selfattn, final_proj + normalize; `loss.backward()` fills all 153 gradients

With these the training surface is complete: every layer of the model the reference's train.py trains has a native backward.  In the
encoders and their glue torch makes the key-line normalisation, the mid-point, the concatenation of the 3 / 5 input columns, the reshapes
(no gradient flows there) and the final add klines_pos + cls_out^T.

The line behind loss.backward() is native too: linetr_amd.optim.Adam (optim.py; csrc/lt_adam.h) steps all 153 parameters in one launch, in
the arithmetic of torch.optim.Adam's single-tensor path.  What torch still does in optimizer.step(): it keeps the 153 step counters (0-d
float32 CPU tensors, as in torch's state_dict) and adds 1 to each, makes a non-contiguous .grad contiguous, allocates the two moments of
a parameter at its first step, and bumps the parameters' version counters; zero_grad() is torch's."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from ._shapes import as_rows_weight, check_pointwise_shapes  # noqa: F401  (the layer's shape rules; Engine.linear_forward applies them too)
from .evaluations import _engine

HEADS, DH, D = 4, 64, 256


class _PointwiseLinear(torch.autograd.Function):
    """y = act(x W^T + b).  Saved for the backward: x, W and, with ReLU, the output itself -- the mask (nothing is recomputed)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        check_pointwise_shapes(x, weight, bias)       # (before an engine is looked up: a bad shape is a ValueError on any device)
        y = _engine(x.device).linear_forward(x, weight, bias, relu)
        ctx.relu = bool(relu)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, y = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        dx, dW, db = _engine(x.device).linear_backward(x, weight, grad_out, mask=y if ctx.relu else None, need=need)
        return dx, dW, db, None


def pointwise_linear(x, weight, bias=None, relu=False):
    """y = relu?(x W^T + b), differentiable with respect to x, weight and bias; y in x's layout ([B, N, n] or [rows, N])"""
    return _PointwiseLinear.apply(x, weight, bias, relu)


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight, bias)
        return _engine(x.device).head_forward(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_desc):
        x, weight, bias = ctx.saved_tensors
        return _engine(x.device).head_backward(x, weight, bias, grad_desc, need=tuple(ctx.needs_input_grad[:3]))


class DescriptorHead(nn.Module):
    """final_proj + F.normalize of the reference's LineTransformer: pre-head features [B, 256, n] -> line_desc [B, 256, n].
    Its state_dict holds `final_proj.weight` [256, 256, 1] and `final_proj.bias` [256], the reference's names."""

    def __init__(self, descriptor_dim=256):
        super().__init__()
        if descriptor_dim != 256:
            raise ValueError("the native head is 256 -> 256")
        self.final_proj = nn.Conv1d(descriptor_dim, descriptor_dim, kernel_size=1, bias=True)

    @classmethod
    def from_line_transformer(cls, model) -> "DescriptorHead":
        """the head of a LineTransformer (this package's or the reference's), or of its state_dict: a copy of its final_proj"""
        sd = model if isinstance(model, dict) else model.state_dict()
        head = cls()
        head.load_state_dict({k: sd[k] for k in ("final_proj.weight", "final_proj.bias")})
        return head.to(sd["final_proj.weight"].device)

    def forward(self, x):
        return _Head.apply(x, self.final_proj.weight, self.final_proj.bias)


class _SigAttnRows(torch.autograd.Function):
    """softmax(q k^T / 8) v on head-major rows [N, 256] (column h*64 + d), one image of cu_sub = one softmax domain.  Saved for the
    backward: q, k, v, the message and lse [N, 4]; P is recomputed from them, nothing else is."""

    @staticmethod
    def forward(ctx, q, k, v, cu_sub):
        o, lse = _engine(q.device).sig_attention_forward(q, k, v, cu_sub)
        ctx.save_for_backward(q, k, v, o, lse, cu_sub)
        ctx.mark_non_differentiable(lse)
        return o, lse

    @staticmethod
    def backward(ctx, grad_o, _grad_lse):
        q, k, v, o, lse, cu_sub = ctx.saved_tensors
        dq, dk, dv = _engine(q.device).sig_attention_backward(q, k, v, o, lse, grad_o, cu_sub, need=tuple(ctx.needs_input_grad[:3]))
        return dq, dk, dv, None


def _item_offsets(B: int, n: int, device) -> torch.Tensor:
    """cu_sub of B items of n positions each, on the device"""
    return torch.arange(B + 1, dtype=torch.int32, device=device) * n


def signature_attention(query, key, value):
    """The reference's attention(query, key, value) (models/line_transformer.py:132-136) on its call shape: query, key, value
    [B, 64, 4, n] (channel d, head h, position), every item its own softmax domain; returns the message [B, 64, 4, n].  The n x n `prob`
    is not returned (it is never formed).  Differentiable with respect to all three inputs; the backward recomputes P from q, k and the
    saved lse.  The tensors are brought to the kernels' head-major rows [B n, 256] and the message back by torch copies (permute +
    contiguous): data movement only, no arithmetic."""
    if query.dim() != 4 or tuple(query.shape[1:3]) != (DH, HEADS) or key.shape != query.shape or value.shape != query.shape:
        raise ValueError(f"query, key and value must share the shape [B, {DH}, {HEADS}, n], got {tuple(query.shape)}, {tuple(key.shape)}, "
                         f"{tuple(value.shape)}")
    B, n = int(query.shape[0]), int(query.shape[3])
    rows = lambda t: t.permute(0, 3, 2, 1).reshape(B * n, D)            # [B, n, h, d] -> head-major rows
    o, _ = _SigAttnRows.apply(rows(query), rows(key), rows(value), _item_offsets(B, n, query.device))
    return o.view(B, n, HEADS, DH).permute(0, 3, 2, 1)


class MultiHeadedAttention(nn.Module):
    """The reference's MultiHeadedAttention (models/line_transformer.py:139-154): message = merge(attention(proj[0](query),
    proj[1](key), proj[2](value))).  Its state_dict has the reference's names and shapes: merge.weight / .bias and proj.{0,1,2}.weight /
    .bias, [256, 256, 1] and [256].  The projections and the merge are pointwise_linear, the attention is the native Function.  The
    reference splits a projection's channel c into (d, h) = (c // 4, c % 4); the kernels read head-major rows (column h*64 + d).  That
    permutation is applied to the PARAMETERS -- the rows of proj[i].weight / .bias and the columns of merge.weight are gathered, which
    autograd differentiates as a scatter into the parameter's gradient -- so the projections write head-major rows, the attention reads
    them in place and no activation is copied or touched by torch arithmetic."""

    def __init__(self, num_heads: int = HEADS, d_model: int = D):
        super().__init__()
        if num_heads != HEADS or d_model != D:
            raise ValueError(f"the native attention is {HEADS} heads of {DH} channels ({D} in all), got {num_heads} heads, d_model {d_model}")
        self.merge = nn.Conv1d(D, D, kernel_size=1)                                            # (names and shapes: the reference's state_dict)
        self.proj = nn.ModuleList(nn.Conv1d(D, D, kernel_size=1) for _ in range(3))
        c = torch.arange(D)
        self.register_buffer("_head_major", (c % DH) * HEADS + c // DH, persistent=False)    # head-major column h*64 + d <- reference channel d*4 + h

    @classmethod
    def from_line_transformer(cls, model, layer: int = 0) -> "MultiHeadedAttention":
        """the attention of signature layer `layer` of a LineTransformer (this package's or the reference's), or of its state_dict: a copy"""
        sd = model if isinstance(model, dict) else model.state_dict()
        prefix = f"selfattn.layers.{int(layer)}.attn."
        own = cls()
        own.load_state_dict({k: torch.as_tensor(sd[prefix + k]) for k in own.state_dict()})
        ref = sd[prefix + "merge.weight"]
        return own.to(ref.device) if isinstance(ref, torch.Tensor) else own

    def forward(self, query, key, value):
        """query, key, value [B, 256, n] -> (message [B, 256, n], None): the reference returns the n x n prob second, which is never
        formed here."""
        if query.dim() != 3 or int(query.shape[1]) != D or key.shape != query.shape or value.shape != query.shape:
            raise ValueError(f"query, key and value must share the shape [B, {D}, n], got {tuple(query.shape)}, {tuple(key.shape)}, "
                             f"{tuple(value.shape)}")
        B, n = int(query.shape[0]), int(query.shape[2])
        hm = self._head_major

        def head_major_rows(layer, x):      # the layer with its output channels gathered head-major: the [B n, 256] rows the kernel wrote, a view
            return pointwise_linear(x, layer.weight[hm], layer.bias[hm]).transpose(1, 2).reshape(B * n, D)

        o, _ = _SigAttnRows.apply(head_major_rows(self.proj[0], query), head_major_rows(self.proj[1], key), head_major_rows(self.proj[2], value),
                                  _item_offsets(B, n, query.device))
        return pointwise_linear(o.view(B, n, D).transpose(1, 2), self.merge.weight[:, hm], self.merge.bias), None


class _BatchNormRelu(torch.autograd.Function):
    """y = relu?(batch_norm(z)).  Saved for the backward: z, the statistics float64 [mean | invstd], gamma and, with ReLU, the output
    itself -- the mask (nothing is recomputed)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, momentum, eps, training, relu):
        y, save = _engine(z.device).bn_forward(z, gamma, beta, running_mean, running_var, momentum, eps, training, relu)
        ctx.training, ctx.relu = bool(training), bool(relu)
        ctx.save_for_backward(z, y if relu else None, save, gamma)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        z, y, save, gamma = ctx.saved_tensors
        dz, dgamma, dbeta = _engine(z.device).bn_backward(z, y, grad_out, save, gamma, ctx.training, need=tuple(ctx.needs_input_grad[:3]))
        return dz, dgamma, dbeta, None, None, None, None, None, None


def batch_norm_relu(z, bn: nn.BatchNorm1d, relu: bool = True):
    """relu?(bn(z)) as torch computes it for z [B, C, n] or [rows, C], differentiable with respect to z, bn.weight and bn.bias; y in z's
    layout.  bn.training: batch statistics (mean and biased variance over all B n positions), bn.running_mean / running_var moved in
    place with bn.momentum and the unbiased variance, num_batches_tracked incremented; a single value per channel raises torch's
    ValueError.  bn.eval(): the running statistics, nothing moves.  Refused: momentum=None (the cumulative average) and affine=False."""
    if not isinstance(bn, nn.BatchNorm1d):
        raise TypeError(f"batch_norm_relu takes an nn.BatchNorm1d, got {type(bn).__name__}")
    if not bn.affine or bn.momentum is None:
        raise ValueError("batch_norm_relu: affine=False and momentum=None (a cumulative moving average) have no native kernel")
    C_ = int(bn.num_features)
    if z.dim() not in (2, 3) or int(z.shape[1]) != C_:
        raise ValueError(f"z must be [B, {C_}, n] or [rows, {C_}], got {tuple(z.shape)}")
    training = bn.training or bn.running_mean is None          # (track_running_stats=False: batch statistics in either mode, as torch)
    if training and z.numel() // C_ <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {z.size()}")
    tracked = bn.training and bn.running_mean is not None
    if tracked and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BatchNormRelu.apply(z, bn.weight, bn.bias, bn.running_mean if tracked or not training else None,
                                bn.running_var if tracked or not training else None, float(bn.momentum), float(bn.eps), training, relu)


def _sub_state_dict(model, prefix):
    """the entries of a model's (or a state_dict's) state dict under `prefix`, the prefix cut off, as tensors"""
    sd = model if isinstance(model, dict) else model.state_dict()
    return {k[len(prefix):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(prefix)}


def _device_of(sub):
    ref = next(iter(sub.values()))
    return ref.device


class AttentionalPropagation(nn.Module):
    """The reference's AttentionalPropagation (models/line_transformer.py:157-166): delta = mlp(cat([x, attn(x, source, source)])) with
    mlp = Conv1d(512, 512) -> BatchNorm1d(512) -> ReLU -> Conv1d(512, 256).  Its state_dict has the reference's names and shapes: attn.*
    (MultiHeadedAttention), mlp.0.weight / .bias, mlp.1.weight / .bias / .running_mean / .running_var / .num_batches_tracked, mlp.3.weight /
    .bias.  `mlp` is the reference's nn.Sequential and holds the parameters; it is never called: the two convolutions are
    pointwise_linear and the normalisation with its activation is batch_norm_relu, which follows .train() / .eval() through mlp[1].
    The concatenation is made of rows ([B, n, 512], x beside the message), so that every layer reads and writes [B n, C] rows behind
    the [B, C, n] view and no activation is copied between the kernels."""

    def __init__(self, feature_dim: int = D, num_heads: int = HEADS):
        super().__init__()
        if feature_dim != D:
            raise ValueError(f"the native signature layer is {D} channels wide, got {feature_dim}")
        self.attn = MultiHeadedAttention(num_heads, feature_dim)
        self.mlp = nn.Sequential(nn.Conv1d(2 * D, 2 * D, kernel_size=1), nn.BatchNorm1d(2 * D), nn.ReLU(), nn.Conv1d(2 * D, D, kernel_size=1))
        nn.init.constant_(self.mlp[-1].bias, 0.0)

    @classmethod
    def from_line_transformer(cls, model, layer: int = 0) -> "AttentionalPropagation":
        """signature layer `layer` of a LineTransformer (this package's or the reference's), or of its state_dict: a copy"""
        sub = _sub_state_dict(model, f"selfattn.layers.{int(layer)}.")
        own = cls()
        own.load_state_dict(sub, strict=True)
        return own.to(_device_of(sub))

    def forward(self, x, source):
        """x, source [B, 256, n] -> (delta [B, 256, n], None): the reference returns the n x n prob second, which is never formed here."""
        message, _ = self.attn(x, source, source)
        rows = torch.cat([x.transpose(1, 2), message.transpose(1, 2)], dim=2)         # [B, n, 512]: data movement only
        z = pointwise_linear(rows.transpose(1, 2), self.mlp[0].weight, self.mlp[0].bias)
        y = batch_norm_relu(z, self.mlp[1], relu=True)
        return pointwise_linear(y, self.mlp[3].weight, self.mlp[3].bias), None


class SelfAttentionalLayer(nn.Module):
    """The reference's SelfAttentionalLayer (models/line_transformer.py:168-183): kline_desc <- kline_desc + layer(kline_desc, kline_desc)
    for every layer; state_dict layers.<i>.* as AttentionalPropagation names them.  The input is brought to rows once (a copy: data
    movement), after which the residual adds keep the [B n, 256] rows behind the [B, 256, n] view from layer to layer."""

    def __init__(self, feature_dim: int = D, layer_names=("self",) * 7):
        super().__init__()
        self.layers = nn.ModuleList(AttentionalPropagation(feature_dim, HEADS) for _ in range(len(layer_names)))
        self.names = list(layer_names)

    @classmethod
    def from_line_transformer(cls, model) -> "SelfAttentionalLayer":
        """the signature network of a LineTransformer (this package's or the reference's), or of its state_dict: a copy"""
        sub = _sub_state_dict(model, "selfattn.")
        n_layers = 1 + max(int(k.split(".")[1]) for k in sub)
        own = cls(D, ["self"] * n_layers)
        own.load_state_dict(sub, strict=True)
        return own.to(_device_of(sub))

    def forward(self, kline_desc):
        """kline_desc [B, 256, n] -> [B, 256, n] (the transposed view of [B n, 256] rows)"""
        if kline_desc.dim() != 3 or int(kline_desc.shape[1]) != D:
            raise ValueError(f"kline_desc must be [B, {D}, n], got {tuple(kline_desc.shape)}")
        kline_desc = kline_desc.transpose(1, 2).contiguous().transpose(1, 2)
        for layer in self.layers:
            delta, _ = layer(kline_desc, kline_desc)
            kline_desc = kline_desc + delta
        return kline_desc


# ---- the line descriptive layer ----------------------------------------------------------------------------------------------------

class _Gelu(torch.autograd.Function):
    """y = gelu(z), erf form.  Saved for the backward: the pre-activation z."""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return _engine(z.device).gelu_forward(z.reshape(-1, z.shape[-1])).view(z.shape)

    @staticmethod
    def backward(ctx, grad_out):
        z, = ctx.saved_tensors
        return _engine(z.device).gelu_backward(z.reshape(-1, z.shape[-1]), grad_out.reshape(-1, z.shape[-1])).view(z.shape)


def gelu(x):
    """F.gelu(x) in its erf form, 0.5 x (1 + erf(x / sqrt 2)), differentiable; x [..., C] with C a multiple of 4 up to 4096"""
    if x.dim() < 1 or int(x.shape[-1]) % 4 or not 4 <= int(x.shape[-1]) <= 4096:
        raise ValueError(f"x must be [..., C] with C a multiple of 4 up to 4096, got {tuple(x.shape)}")
    return _Gelu.apply(x)


class DropoutState(NamedTuple):
    """What the masks of one training forward are a pure function of: a 64-bit seed, the 32-bit index of the forward, the probability.
    (The generator and its counter layout: include/linetr_hip.h, LinetrDropout.)"""
    seed: int
    call: int
    p: float


def _native_dropout(dropout):
    """a DropoutState (or any (seed, call, p)) as the engine's LinetrDropout; 0 <= p < 1, else ValueError"""
    from ._native import Dropout
    seed, call, p = dropout
    return Dropout.make(seed, call, p)


class _ResidualLayerNorm(torch.autograd.Function):
    """y = LayerNorm(a + residual), or with `drop` (a native Dropout, else None) y = LayerNorm(r a + residual), r the factors of `site`.
    Saved for the backward: a, the residual, the rows' float32 mean | rstd, gamma and the dropout state itself -- the mask is generated
    again, not stored."""

    @staticmethod
    def forward(ctx, a, residual, gamma, beta, eps, drop, site):
        eng = _engine(a.device)
        y, stats = (eng.layer_norm_forward(a, residual, gamma, beta, eps) if drop is None else
                    eng.layer_norm_dropout_forward(a, residual, gamma, beta, drop, site, eps))
        ctx.drop, ctx.site = drop, site
        ctx.save_for_backward(a, residual, stats, gamma)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        a, residual, stats, gamma = ctx.saved_tensors
        eng, need = _engine(a.device), ctx.needs_input_grad
        need_a, need_r = need[0], residual is not None and need[1]
        if ctx.drop is None:                         # one data gradient, of a and of the residual alike
            dx, dgamma, dbeta = eng.layer_norm_backward(a, residual, stats, gamma, grad_out, need=(need_a or need_r, need[2], need[3]))
            da, dr = dx if need_a else None, dx if need_r else None
        else:
            da, dr, dgamma, dbeta = eng.layer_norm_dropout_backward(a, residual, stats, gamma, grad_out, ctx.drop, ctx.site,
                                                                    need=(need_a, need_r, need[2], need[3]))
        return da, dr, dgamma, dbeta, None, None, None


def residual_layer_norm(a, residual, ln: nn.LayerNorm, dropout=None, site=None):
    """ln(a + residual) for an nn.LayerNorm(256) `ln`, as the reference's `q += residual; q = self.layer_norm(q)`; a, residual
    [rows, 256] (residual may be None).  Differentiable with respect to a, residual, ln.weight and ln.bias.  With `dropout` (a
    DropoutState) and `site` (1: behind fc, 2: behind w_2) it is ln(dropout(a) + residual) as the reference's train mode computes it, the
    mask generated in the kernels, forward and backward.  Refused: an `ln` without affine parameters or of another width."""
    if not isinstance(ln, nn.LayerNorm):
        raise TypeError(f"residual_layer_norm takes an nn.LayerNorm, got {type(ln).__name__}")
    if tuple(ln.normalized_shape) != (D,) or ln.weight is None or ln.bias is None:
        raise ValueError(f"residual_layer_norm: the native kernel is an affine LayerNorm({D}), got normalized_shape {tuple(ln.normalized_shape)}"
                         f"{'' if ln.weight is not None and ln.bias is not None else ' without weight and bias'}")
    if a.dim() != 2 or int(a.shape[1]) != D or (residual is not None and residual.shape != a.shape):
        raise ValueError(f"a and residual must be [rows, {D}], got {tuple(a.shape)} and {None if residual is None else tuple(residual.shape)}")
    if dropout is None:
        return _ResidualLayerNorm.apply(a, residual, ln.weight, ln.bias, float(ln.eps), None, None)
    if site not in (1, 2):
        raise ValueError(f"residual_layer_norm: dropout needs its site, 1 (behind fc) or 2 (behind w_2), got {site!r}")
    return _ResidualLayerNorm.apply(a, residual, ln.weight, ln.bias, float(ln.eps), _native_dropout(dropout), int(site))


class _ClsTokenPool(torch.autograd.Function):
    """pooled[l, h] = sum_t softmax_t(u[l, h] . x[l, t]) x[l, t].  Saved for the backward: x, u, pooled and lse [L, 4]; the softmax is
    recomputed from them."""

    @staticmethod
    def forward(ctx, x, u):
        pooled, lse = _engine(x.device).cls_pool_forward(x, u)
        ctx.save_for_backward(x, u, pooled, lse)
        return pooled

    @staticmethod
    def backward(ctx, grad_pooled):
        x, u, pooled, lse = ctx.saved_tensors
        return _engine(x.device).cls_pool_backward(x, u, pooled, lse, grad_pooled, need=tuple(ctx.needs_input_grad[:2]))


class _ClsTokenPoolDropout(torch.autograd.Function):
    """a = softmax_t(u[l, h] . x[l, t]) r[l, h, t];  pooled[l, h] = sum_t a_t x[l, t];  kept[l, h] = sum_t a_t.  Saved for the backward: x, u,
    pooled, kept, lse and the dropout state itself -- softmax and mask are made again, not stored."""

    @staticmethod
    def forward(ctx, x, u, drop):
        pooled, kept, lse = _engine(x.device).cls_pool_dropout_forward(x, u, drop)
        ctx.drop = drop
        ctx.save_for_backward(x, u, pooled, kept, lse)
        return pooled, kept

    @staticmethod
    def backward(ctx, grad_pooled, grad_kept):
        x, u, pooled, kept, lse = ctx.saved_tensors
        return (*_engine(x.device).cls_pool_dropout_backward(x, u, pooled, lse, kept, grad_pooled, grad_kept, ctx.drop,
                                                              need=tuple(ctx.needs_input_grad[:2])), None)


def cls_token_pool(x, u, dropout=None):
    """The CLS query row's attention over the S tokens of each segment, in the folded form: x [L, S, 256] token rows (slot 0: the CLS
    token), u [L, 4, 256] with u[l, h] = Wk_h^T (q_lh / 8); returns pooled [L, 4, 256], the softmax-weighted mean of the tokens per
    head.  Differentiable with respect to x and u.  With `dropout` (a DropoutState) the softmax weights go through the reference's
    attention dropout (site 0) and the result is (pooled, kept): kept [L, 4] is what is left of the weights' sum, the factor of the
    value bias behind the pooling; both are differentiable."""
    if x.dim() != 3 or int(x.shape[2]) != D or not 1 <= int(x.shape[1]) <= 256 or tuple(u.shape) != (int(x.shape[0]), HEADS, D):
        raise ValueError(f"x must be [L, S, {D}] with 1 <= S <= 256 and u [L, {HEADS}, {D}], got {tuple(x.shape)} and {tuple(u.shape)}")
    if dropout is None:
        return _ClsTokenPool.apply(x, u)
    return _ClsTokenPoolDropout.apply(x, u, _native_dropout(dropout))


class _CancelledBias(torch.autograd.Function):
    """Ties a parameter that cancels out of the forward into the graph: the output is `y` itself, and the parameter's gradient is a
    tensor of exact zeros."""

    @staticmethod
    def forward(ctx, y, bias):
        ctx.save_for_backward(bias)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, grad_y):
        bias, = ctx.saved_tensors
        return grad_y, torch.zeros_like(bias) if ctx.needs_input_grad[1] else None


class _Linears(nn.Module):
    """a holder of nn.Linear / nn.LayerNorm parameters under the reference's names; never called"""


class LineDescriptiveEncoder(nn.Module):
    """The reference's LineDescriptiveEncoder (models/line_transformer.py:75-91) = MultiHeadAttention + FeedForward
    (models/line_attention.py:23-94), with its state_dict names and shapes: slf_attn.w_qs / w_ks / w_vs / fc (.weight [256, 256],
    .bias [256]), slf_attn.layer_norm, pos_ffn.w_1 ([1024, 256]), pos_ffn.w_2 ([256, 1024]), pos_ffn.layer_norm (both eps 1e-6).

    KeylineEncoder reads only the CLS row enc_output[:, :, 0, :] of the layer's output (:128), so only the CLS query row is computed,
    in the folded form: q = w_qs(x_0);  u_h = Wk_h^T (q_h / 8);  pooled = cls_token_pool(x, u);  o_h = Wv_h pooled_h +
    bv_h (the weights sum to 1);  y = LN1(fc(o) + x_0);  out = LN2(w_2(gelu(w_1(y))) + y).  The output and every gradient -- of the
    parameters and of desc, slot 0 included -- are those of the reference's row 0; token rows 1 .. S-1 of its output are not made.
    The key bias adds one constant per (segment, head) to the scores, which the softmax cancels: slf_attn.w_ks.bias.grad is a tensor of
    exact zeros, the exact value of what float32 autograd through the reference leaves as noise of about 1e-6."""

    def __init__(self, d_feature: int = D, n_heads: int = HEADS, n_att_layers: int = 1, d_inner: int = 1024, dropout: float = 0.0):
        super().__init__()
        if d_feature != D or n_heads != HEADS or d_inner % 64 or not 64 <= d_inner <= 1024:
            raise ValueError(f"the native descriptive layer is {D} wide with {HEADS} heads and d_inner a multiple of 64 up to 1024, got "
                             f"{d_feature}, {n_heads}, {d_inner}")
        self.dropout = float(dropout)
        self._dropout_state = None               # (seed, call) once seed_dropout() was called: plain Python, not in the state_dict
        self.slf_attn, self.pos_ffn = _Linears(), _Linears()
        for name in ("w_qs", "w_ks", "w_vs", "fc"):
            setattr(self.slf_attn, name, nn.Linear(D, D, bias=True))
        self.slf_attn.layer_norm = nn.LayerNorm(D, eps=1e-6)
        self.pos_ffn.w_1 = nn.Linear(D, d_inner)
        self.pos_ffn.w_2 = nn.Linear(d_inner, D)
        self.pos_ffn.layer_norm = nn.LayerNorm(D, eps=1e-6)

    @classmethod
    def from_line_transformer(cls, model, layer: int = -1) -> "LineDescriptiveEncoder":
        """descriptive layer `layer` (default: the last, the only one whose output KeylineEncoder reads) of a LineTransformer (this
        package's or the reference's), or of its state_dict: a copy"""
        sd = model if isinstance(model, dict) else model.state_dict()
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("klenc.desc_layers."))
        sub = _sub_state_dict(sd, f"klenc.desc_layers.{int(layer) % n_layers}.")
        own = cls(d_inner=int(sub["pos_ffn.w_1.weight"].shape[0]))
        own.load_state_dict(sub, strict=True)
        return own.to(_device_of(sub))

    def seed_dropout(self, seed: int, call: int = 0):
        """Switches training-time dropout on: from now on a train-mode forward with `dropout != 0` draws its masks from (seed, call) and
        then increments `call`, so that consecutive forwards -- the two views of one step -- draw different masks.  A 64-bit seed, a
        32-bit call index (it wraps)."""
        self.set_dropout_state((seed, call))
        return self

    def dropout_state(self):
        """(seed, call) of the next training forward, or None for a module that was never seeded: what a checkpoint keeps beside the
        state_dict (it is no tensor and not part of it)"""
        return self._dropout_state

    def set_dropout_state(self, state):
        """dropout_state()'s inverse: (seed, call), or None to go back to refusing"""
        if state is not None:
            seed, call = (int(v) for v in state)
            if not 0 <= seed < 1 << 64 or not 0 <= call < 1 << 32:
                raise ValueError(f"dropout state {state!r}: a 64-bit seed and a 32-bit call index")
            state = (seed, call)
        self._dropout_state = state

    def _next_dropout(self):
        """the DropoutState of this training forward (None: no dropout); advances the call index"""
        if not self.training or self.dropout == 0.0:
            return None
        if self._dropout_state is None:
            raise RuntimeError(
                "linetr_amd.train_ops.LineDescriptiveEncoder in train mode with dropout "
                f"{self.dropout}: the masks of training-time dropout (the reference's nn.Dropout(0.1), models/line_attention.py:18,70,90) "
                "are a function of a seed, and randomness is never drawn implicitly.  Call `seed_dropout(seed)` first, set `dropout = 0.0` "
                "to run the deterministic train-mode forward, or call .eval()")
        seed, call = self._dropout_state
        self._dropout_state = (seed, (call + 1) & 0xffffffff)
        return DropoutState(seed, call, self.dropout)

    def forward(self, desc, slf_attn_mask=None):
        """desc [B, L, S, 256] (slot 0 of every segment: the CLS token) -> (cls_out [B, L, 256], None).  cls_out is row 0 of the
        reference's output, enc_output[:, :, 0, :], the only row KeylineEncoder reads; the reference's second result, the S x S attention
        map, is never formed.  `slf_attn_mask` is accepted and ignored: the reference's mask acts on QUERY rows, and the CLS row is never
        masked, so row 0 attends to all S keys whatever the mask holds.  In train mode with `dropout != 0` the three
        dropouts of the reference act on row 0 (training-time dropout): the value bias is then scaled by what the attention dropout kept."""
        if desc.dim() != 4 or int(desc.shape[3]) != D or not 1 <= int(desc.shape[2]) <= 256:
            raise ValueError(f"desc must be [B, L, S, {D}] with 1 <= S <= 256, got {tuple(desc.shape)}")
        drop = self._next_dropout()
        B, L, S = (int(v) for v in desc.shape[:3])
        att, ffn = self.slf_attn, self.pos_ffn
        x = desc.reshape(B * L, S, D)
        x0 = x[:, 0].contiguous()                                                            # the CLS rows: the query and the residual
        q = pointwise_linear(x0, att.w_qs.weight, att.w_qs.bias) * 0.125                     # (a power of two: exact)
        head = lambda h: slice(h * DH, (h + 1) * DH)
        u = torch.stack([pointwise_linear(q[:, head(h)], att.w_ks.weight[head(h)].t()) for h in range(HEADS)], dim=1)
        if drop is None:
            pooled = cls_token_pool(x, u)
            o = torch.cat([pointwise_linear(pooled[:, h], att.w_vs.weight[head(h)], att.w_vs.bias[head(h)]) for h in range(HEADS)], dim=1)
        else:
            pooled, kept = cls_token_pool(x, u, drop)
            o = torch.cat([pointwise_linear(pooled[:, h], att.w_vs.weight[head(h)]) + kept[:, h:h + 1] * att.w_vs.bias[head(h)]
                           for h in range(HEADS)], dim=1)
        y = residual_layer_norm(pointwise_linear(o, att.fc.weight, att.fc.bias), x0, att.layer_norm, drop, 1 if drop is not None else None)
        hidden = gelu(pointwise_linear(y, ffn.w_1.weight, ffn.w_1.bias))
        out = residual_layer_norm(pointwise_linear(hidden, ffn.w_2.weight, ffn.w_2.bias), y, ffn.layer_norm, drop, 2 if drop is not None else None)
        if att.w_ks.bias.requires_grad and torch.is_grad_enabled():
            out = _CancelledBias.apply(out, att.w_ks.bias)
        return out.view(B, L, D), None


# ---- the positional encoders, KeylineEncoder and the whole network ------------------------------------------------------------------

class _InputLinear(torch.autograd.Function):
    """z = x W^T + b for the narrow first layer of an encoder.  Saved for the backward: x and the weight (for its shape)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if ctx.needs_input_grad[0]:
            raise RuntimeError("linetr_amd.train_ops.input_linear has no gradient with respect to x: the coordinates, scores and angles the "
                               "positional encoders read are inputs of the network, not functions of a parameter (detach them)")
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return _engine(x.device).input_layer_forward(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        dW, db = _engine(x.device).input_layer_backward(x, weight, grad_out, need=(ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]))
        return None, dW, db


def input_linear(x, weight, bias=None):
    """z = x W^T + b for x [rows, Kin] with 1 <= Kin <= 8 and a weight [N, Kin] or [N, Kin, 1] with N % 4 == 0, 4 <= N <= 64: the first
    layer of a positional encoder, too narrow for the GEMM of pointwise_linear.  Differentiable with respect to weight and bias; an x
    that requires a gradient raises."""
    check_pointwise_shapes(x, weight, bias)
    if x.dim() != 2:
        raise ValueError(f"x must be [rows, Kin], got {tuple(x.shape)}")
    return _InputLinear.apply(x, weight, bias)


class _AssembleTokens(torch.autograd.Function):
    """x[:, 0] = cls, x[:, 1:] = desc + pos.  Nothing is saved but the shape of the cls token."""

    @staticmethod
    def forward(ctx, desc, pos, cls_token):
        ctx.cls_shape = tuple(cls_token.shape)
        return _engine(desc.device).assemble_tokens_forward(desc, pos, cls_token)

    @staticmethod
    def backward(ctx, grad_x):
        need = ctx.needs_input_grad
        dtok, dcls = _engine(grad_x.device).assemble_tokens_backward(grad_x, need=(need[0] or need[1], need[2]))
        return dtok if need[0] else None, dtok if need[1] else None, dcls.view(ctx.cls_shape) if dcls is not None else None


def assemble_tokens(desc, pos, cls_token):
    """The token rows the descriptive layer reads (models/line_transformer.py:116-121 of the reference): desc, pos [L, S, 256] with
    1 <= S <= 255 and cls_token (256 values, any shape) -> x [L, S + 1, 256], x[:, 0] = cls_token and x[:, 1:] = desc + pos.
    Differentiable with respect to all three (the gradient of desc and of pos is one tensor)."""
    if desc.dim() != 3 or int(desc.shape[2]) != D or not 1 <= int(desc.shape[1]) <= 255 or pos.shape != desc.shape or cls_token.numel() != D:
        raise ValueError(f"desc and pos must share the shape [L, S, {D}] with 1 <= S <= 255 and cls_token hold {D} values, got "
                         f"{tuple(desc.shape)}, {tuple(pos.shape)} and {tuple(cls_token.shape)}")
    return _AssembleTokens.apply(desc, pos, cls_token)


def _mlp_holder(channels):
    """the reference's MLP(channels) (models/line_transformer.py:9-20): Conv1d(k=1) [-> BatchNorm1d -> ReLU] per layer, none behind the last"""
    layers = []
    for i in range(1, len(channels)):
        layers.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            layers += [nn.BatchNorm1d(channels[i]), nn.ReLU()]
    return nn.Sequential(*layers)


class _PositionalEncoder(nn.Module):
    """What the two encoders share: `encoder`, the reference's nn.Sequential, holds the parameters and the BatchNorm buffers under the
    reference's names and is never called; rows [rows, n_in] go through input_linear, batch_norm_relu and then pointwise_linear /
    batch_norm_relu per further layer, all on [rows, C] rows."""
    N_IN = 0

    def __init__(self, feature_dim: int, layers):
        super().__init__()
        widths = [int(v) for v in layers] + [int(feature_dim)]
        ok = len(widths) >= 2 and widths[0] % 4 == 0 and 4 <= widths[0] <= 64
        ok = ok and all(n % 64 == 0 and k % 32 == 0 and n <= 1024 for k, n in zip(widths[:-1], widths[1:]))
        if not ok:
            raise ValueError(f"the native encoder takes a first width that is a multiple of 4 in 4 .. 64 and then widths that are multiples of "
                             f"64 up to 1024 (each one's input a multiple of 32), got layers {list(layers)} and feature_dim {feature_dim}")
        self.feature_dim = int(feature_dim)
        self.encoder = _mlp_holder([self.N_IN] + widths)
        nn.init.constant_(self.encoder[-1].bias, 0.0)

    @classmethod
    def _from(cls, model, prefix):
        sub = _sub_state_dict(model, prefix)
        convs = sorted((int(k.split(".")[1]), int(v.shape[0])) for k, v in sub.items() if k.endswith(".weight") and v.dim() == 3)
        own = cls(convs[-1][1], [n for _, n in convs[:-1]])
        own.load_state_dict(sub, strict=True)
        return own.to(_device_of(sub))

    def _rows(self, x):
        enc = self.encoder
        y = batch_norm_relu(input_linear(x, enc[0].weight, enc[0].bias), enc[1], relu=True)
        for i in range(3, len(enc) - 1, 3):
            y = batch_norm_relu(pointwise_linear(y, enc[i].weight, enc[i].bias), enc[i + 1], relu=True)
        return pointwise_linear(y, enc[-1].weight, enc[-1].bias)


class LinePositionalEncoder(_PositionalEncoder):
    """The reference's LinePositionalEncoder (models/line_transformer.py:40-50) with its state_dict (encoder.{0,1,3,4,..}.*): the
    mid-point, response and angle of every sub-line -> [B, feature_dim, n].  Torch makes the mid-point and the concatenation of the five
    input columns (no gradient flows there); every layer, forward and backward, is native."""
    N_IN = 5

    @classmethod
    def from_line_transformer(cls, model) -> "LinePositionalEncoder":
        """the line encoder of a LineTransformer (this package's or the reference's), or of its state_dict: a copy"""
        return cls._from(model, "klenc.line_position_enc.")

    def forward(self, klines, responses, angles):
        """klines [B, n, 2, 2], responses [B, n, 1], angles [B, n, 2] -> [B, feature_dim, n] (the transposed view of [B n, C] rows)"""
        B, n = int(klines.shape[0]), int(klines.shape[1])
        mid_points = (klines[:, :, 0] + klines[:, :, 1]) / 2.
        rows = torch.cat([mid_points, responses, angles], dim=2).reshape(B * n, self.N_IN)
        return self._rows(rows).view(B, n, self.feature_dim).transpose(1, 2)


class WordPositionalEncoder(_PositionalEncoder):
    """The reference's WordPositionalEncoder (models/line_transformer.py:52-73) with its state_dict: the position and score of every
    token -> [B, n, S, feature_dim].  One row per token, B n S of them: BatchNorm's statistics run over all of them, as the reference's
    do over its [B n, C, S] tensor."""
    N_IN = 3

    @classmethod
    def from_line_transformer(cls, model) -> "WordPositionalEncoder":
        """the word encoder of a LineTransformer (this package's or the reference's), or of its state_dict: a copy"""
        return cls._from(model, "klenc.word_position_enc.")

    def forward(self, words_in_line, scores_in_line):
        """words_in_line [B, n, S, 2], scores_in_line [B, n, S, 1] -> [B, n, S, feature_dim]"""
        B, n, S = (int(v) for v in words_in_line.shape[:3])
        rows = torch.cat([words_in_line, scores_in_line], dim=-1).reshape(B * n * S, self.N_IN)
        return self._rows(rows).view(B, n, S, self.feature_dim)


class KeylineEncoder(nn.Module):
    """The reference's KeylineEncoder (models/line_transformer.py:93-130) with its state_dict: line_position_enc.*, word_position_enc.*,
    desc_layers.<i>.* and cls_token [1, 1, 1, 256].  sentence = line_position_enc(..) + desc_layer(cat(cls, desc + word_position_enc(..)))
    [:, :, 0]^T.  The reference feeds every descriptive layer the same `desc` and reads only the last one's output, so only the last is
    computed (the others get no gradient there either).  The sum desc + pos and the CLS slot are assemble_tokens; the final sum is a
    torch add, like the signature network's residual."""

    def __init__(self, feature_dim: int = D, mlp_layers=(32, 64, 128, 256), n_heads: int = HEADS, n_att_layers: int = 1, d_inner: int = 1024,
                 dropout: float = 0.0):
        super().__init__()
        if feature_dim != D or int(n_att_layers) < 1:
            raise ValueError(f"the native KeylineEncoder is {D} wide with at least one descriptive layer, got {feature_dim}, {n_att_layers}")
        self.feature_dim = D
        self.line_position_enc = LinePositionalEncoder(D, list(mlp_layers))
        self.word_position_enc = WordPositionalEncoder(D, list(mlp_layers))
        self.desc_layers = nn.ModuleList(LineDescriptiveEncoder(D, n_heads, n_att_layers, d_inner, dropout=dropout) for _ in range(int(n_att_layers)))
        self.cls_token = nn.Parameter(torch.randn(1, 1, 1, D))

    @classmethod
    def from_line_transformer(cls, model) -> "KeylineEncoder":
        """the klenc of a LineTransformer (this package's or the reference's), or of its state_dict: a copy"""
        sub = _sub_state_dict(model, "klenc.")
        widths = sorted((int(k.split(".")[2]), int(v.shape[0])) for k, v in sub.items()
                        if k.startswith("line_position_enc.") and k.endswith(".weight") and v.dim() == 3)
        n_layers = 1 + max(int(k.split(".")[1]) for k in sub if k.startswith("desc_layers."))
        own = cls(D, [n for _, n in widths[:-1]], HEADS, n_layers, int(sub["desc_layers.0.pos_ffn.w_1.weight"].shape[0]))
        own.load_state_dict(sub, strict=True)
        return own.to(_device_of(sub))

    def seed_dropout(self, seed: int, call: int = 0):
        """LineDescriptiveEncoder.seed_dropout of the layer that is computed, the last one"""
        self.desc_layers[-1].seed_dropout(seed, call)
        return self

    def dropout_state(self):
        return self.desc_layers[-1].dropout_state()

    def set_dropout_state(self, state):
        self.desc_layers[-1].set_dropout_state(state)

    def forward(self, klines, resp, angle, pnt, desc, score, mask=None):
        """klines [B, n, 2, 2], resp [B, n, 1], angle [B, n, 2], pnt [B, n, S, 2], desc [B, n, S, 256], score [B, n, S, 1] -> sentence
        [B, 256, n].  `mask` is accepted and ignored, as in LineDescriptiveEncoder."""
        if desc.dim() != 4 or int(desc.shape[3]) != D or not 1 <= int(desc.shape[2]) <= 255:
            raise ValueError(f"desc must be [B, n, S, {D}] with 1 <= S <= 255, got {tuple(desc.shape)}")
        B, n, S = (int(v) for v in desc.shape[:3])
        klines_pos = self.line_position_enc(klines, resp, angle)
        pos = self.word_position_enc(pnt, score)
        tokens = assemble_tokens(desc.reshape(B * n, S, D), pos.reshape(B * n, S, D), self.cls_token)
        cls_out, _ = self.desc_layers[-1](tokens.view(B, n, S + 1, D), mask)
        return klines_pos + cls_out.transpose(1, 2)


class TrainableLineTransformer(nn.Module):
    """The network the reference's train.py trains (LineTransformer, models/line_transformer.py:185-249) with a native backward: klenc
    (KeylineEncoder), selfattn (SelfAttentionalLayer) and final_proj, under the reference's full key set -- load_state_dict(strict=True)
    works in both directions with the reference's model.  forward(data) takes the reference's dict and returns it with `line_desc`
    [B, 256, n] carrying the autograd graph; with linetr_amd.evaluations.descriptor_loss on top, `loss.backward()` fills every
    parameter's .grad and desc_sublines.grad.  The key-line normalisation is torch without a gradient; the coordinates, responses,
    angles and scores are inputs only (one that requires a gradient raises).  `config` is merged over default_config; a `dropout` other
    than 0 runs in train mode once seed_dropout(seed) was called and raises before (LineDescriptiveEncoder: randomness is never drawn
    implicitly).  linetr_amd.LineTransformer, the inference model, is another class and stays as it is."""
    default_config = {"image_shape": [480, 640], "descriptor_dim": D, "keyline_encoder": [32, 64, 128, 256], "n_heads": HEADS,
                      "n_line_descriptive_layers": 1, "d_inner": 1024, "n_signature_layers": 7, "dropout": 0.0}
    _INPUTS = ("sublines", "resp_sublines", "angle_sublines", "pnt_sublines", "score_sublines")

    def __init__(self, config=None):
        super().__init__()
        self.config = c = {**self.default_config, **(config or {})}
        self.image_shape = c["image_shape"]
        if c["descriptor_dim"] != D:
            raise ValueError(f"the native network is {D} wide, got descriptor_dim {c['descriptor_dim']}")
        self.klenc = KeylineEncoder(D, c["keyline_encoder"], c["n_heads"], c["n_line_descriptive_layers"], c["d_inner"], dropout=c["dropout"])
        self.selfattn = SelfAttentionalLayer(D, ["self"] * int(c["n_signature_layers"]))
        self.final_proj = nn.Conv1d(D, D, kernel_size=1, bias=True)

    @classmethod
    def from_line_transformer(cls, model, **config) -> "TrainableLineTransformer":
        """a copy of a LineTransformer (this package's or the reference's), or of its state_dict"""
        sd = {k: torch.as_tensor(v) for k, v in (model if isinstance(model, dict) else model.state_dict()).items()}
        enc = sorted((int(k.split(".")[3]), int(v.shape[0])) for k, v in sd.items()
                     if k.startswith("klenc.line_position_enc.encoder.") and k.endswith(".weight") and v.dim() == 3)
        own = cls({"keyline_encoder": [n for _, n in enc[:-1]],
                   "n_line_descriptive_layers": 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("klenc.desc_layers.")),
                   "d_inner": int(sd["klenc.desc_layers.0.pos_ffn.w_1.weight"].shape[0]),
                   "n_signature_layers": 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("selfattn.layers.")), **config})
        own.load_state_dict(sd, strict=True)
        return own.to(sd["final_proj.weight"].device)

    def seed_dropout(self, seed: int, call: int = 0):
        """Switches training-time dropout on (LineDescriptiveEncoder.seed_dropout of klenc's last descriptive layer): with `dropout` 0.1
        in the config and a seed, .train() runs the reference's recipe; every forward draws its own masks.  Checkpoint
        dropout_state() beside the state_dict and hand it to set_dropout_state() to resume."""
        self.klenc.seed_dropout(seed, call)
        return self

    def dropout_state(self):
        return self.klenc.dropout_state()

    def set_dropout_state(self, state):
        self.klenc.set_dropout_state(state)

    def _normalize(self, klines, pnt):
        """normalize_keylines of the reference (:22-38): (x - centre) / (0.7 max(width, height)) on both end points and on the tokens"""
        height, width = self.image_shape[-2:]
        size = klines.new_tensor([float(width), float(height)])
        center, scaling = size / 2, size.max() * 0.7
        return (klines - center) / scaling, (pnt - center) / scaling

    @staticmethod
    def default_ret():
        """the reference's return for an input without lines (:284-291)"""
        return {"klines": torch.empty((1, 0, 2, 2)), "sublines": torch.empty((1, 0, 2, 2)), "line_desc": torch.empty((1, 256, 0)),
                "mat_klines2sublines": torch.empty((1, 0, 0))}

    def forward(self, data):
        if len(data["klines"]) == 0:
            return self.default_ret()
        if torch.is_grad_enabled():
            asked = [k for k in self._INPUTS if data[k].requires_grad]
            if asked:
                raise RuntimeError(f"linetr_amd.train_ops.TrainableLineTransformer has no gradient with respect to {', '.join(asked)}: of the "
                                   "network's inputs only desc_sublines is differentiated")
        with torch.no_grad():
            klines, pnt = self._normalize(data["sublines"], data["pnt_sublines"])
        sentence = self.klenc(klines, data["resp_sublines"], data["angle_sublines"], pnt, data["desc_sublines"], data["score_sublines"],
                              data["mask_sublines"])
        data.update({"line_desc": _Head.apply(self.selfattn(sentence), self.final_proj.weight, self.final_proj.bias)})
        return data
