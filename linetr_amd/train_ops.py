"""Differentiable native layers: torch.autograd.Functions on top of the exact-fp32 kernels of csrc/lt_linbwd.h and csrc/lt_attnbwd.h.

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

With linetr_amd.evaluations.descriptor_loss on top of a DescriptorHead, `loss.backward()` fills head.final_proj.weight.grad, .bias.grad
and the pre-head features' .grad on the device, with no torch arithmetic between the criterion's gradient and them; a
MultiHeadedAttention's `message.backward(g)` fills its eight parameters' and its inputs' .grad the same way.  The tensors must live on a
HIP device (there is no CPU path).  Of the signature layer the BatchNorm backward, the concatenated MLP and the residual are not here, nor
is the descriptive layer."""
from __future__ import annotations

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
