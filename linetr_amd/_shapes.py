"""What engine.py, its training / debug surfaces and train_ops.py share and none of them owns: the descriptor width, the address of
an optional tensor and the shape rules of a point-wise layer.  Imports nothing of the package (every one of them imports it)."""
from __future__ import annotations

import torch

D = 256


def ptr(t):
    """the device address of an optional tensor (None stays None: a NULL pointer at the C ABI)"""
    return t.data_ptr() if t is not None else None


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
