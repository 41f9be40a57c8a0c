"""Differentiable native layers: torch.autograd.Functions on top of the exact-fp32 kernels of csrc/lt_linbwd.h.

    pointwise_linear(x, weight, bias=None, relu=False)   y = act(x W^T + b): Conv1d(k=1) ([N, K, 1] weight, x [B, K, n]) or Linear
                                                         ([N, K] weight, x [rows, K]) on the UNFOLDED state_dict weight, with the
                                                         data, weight and bias gradients native (Engine.linear_forward / _backward)
    DescriptorHead                                       line_desc = F.normalize(final_proj(x), p=2, dim=1)
                                                         (models/line_transformer.py:245-246 of the reference), forward and backward
                                                         native (Engine.head_forward / head_backward)

With linetr_amd.evaluations.descriptor_loss on top of a DescriptorHead, `loss.backward()` fills head.final_proj.weight.grad, .bias.grad
and the pre-head features' .grad on the device, with no torch arithmetic between the criterion's gradient and them.  The tensors must live
on a HIP device (there is no CPU path).  The backward of the folded forward stages (attention, LayerNorm, BatchNorm) is not here."""
from __future__ import annotations

import torch
from torch import nn

from .evaluations import _engine


def as_rows_weight(weight: torch.Tensor) -> torch.Tensor:
    """a Conv1d(k=1) [N, K, 1] or a Linear [N, K] weight as its [N, K] matrix (a view)"""
    if weight.dim() == 3 and weight.shape[2] == 1:
        return weight[:, :, 0]
    if weight.dim() != 2:
        raise ValueError(f"a point-wise weight must be [N, K] or [N, K, 1], got {tuple(weight.shape)}")
    return weight


def check_pointwise_shapes(x, weight, bias=None):
    """(N, K) of the layer; raises ValueError where x / bias do not fit the weight: x is [B, K, n] or [rows, K]"""
    N, K = (int(v) for v in as_rows_weight(weight).shape)
    if x.dim() not in (2, 3) or int(x.shape[1]) != K:
        raise ValueError(f"x must be [B, {K}, n] or [rows, {K}] for a [{N}, {K}] weight, got {tuple(x.shape)}")
    if bias is not None and bias.numel() != N:
        raise ValueError(f"bias must hold {N} elements, got {tuple(bias.shape)}")
    return N, K


class _PointwiseLinear(torch.autograd.Function):
    """y = act(x W^T + b).  Saved for the backward: x, W and, with ReLU, the output itself -- the mask (nothing is recomputed)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        check_pointwise_shapes(x, weight, bias)
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
