"""The training and evaluation surface of Engine (a mixin: engine.py declares `class Engine(_TrainSurface, _DebugSurface)` and holds
the helpers used here -- _call, _f32, _workspace, _host_stage, _event, _await_stage): ground truth, the validation step, the criterion with
its gradient, and forward / backward of the layers that have a native backward (csrc/linetr_train.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._shapes import D, as_rows_weight, check_pointwise_shapes, ptr


class _TrainSurface:
    def assign_from_matches(self, lmatches: torch.Tensor, n: int) -> torch.Tensor:
        """train.py:176-183 on the device (linetr_assign_from_matches): the loader's lmatches [B, M, 2] (rows whose first entry is -1
        are padding) -> mat_assign_sublines [B, n+1, n+1] float32."""
        lm = lmatches.to(device=self.device, dtype=torch.int32).contiguous()
        B, M = int(lm.shape[0]), int(lm.shape[1])
        assign = torch.empty((B, n + 1, n + 1), dtype=torch.float32, device=self.device)
        self._call("linetr_assign_from_matches", lm.data_ptr(), B, M, int(n), assign.data_ptr())
        return assign

    def _criterion_args(self, who, desc0, desc1, assign, lmatches):
        """What val_step and loss_step (`who`) take, checked and brought to what the criterion kernels read: the two descriptor sets as
        [B*n, 256] rows, B, n0, n1 and mat_assign_sublines [B, n+1, n+1] (made from `lmatches` where that is what was given)."""
        if (assign is None) == (lmatches is None):
            raise ValueError(f"{who}: give exactly one of assign / lmatches")
        d0, B0, _ = self._act_rows(desc0, D, "line descriptors", strided=False)
        d1, B1, _ = self._act_rows(desc1, D, "line descriptors", strided=False)
        B = int((assign if assign is not None else lmatches).shape[0])
        if B <= 0 or any(b is not None and b != B for b in (B0, B1)) or d0.shape[0] % B or d1.shape[0] % B:
            raise ValueError(f"{who}: the descriptors and the ground truth disagree about the batch size")
        n0, n1 = int(d0.shape[0]) // B, int(d1.shape[0]) // B
        if assign is None:
            assign = self.assign_from_matches(lmatches, n0)
        else:
            assign = self._f32(assign)
            if n0 == n1 and tuple(assign.shape) != (B, n0 + 1, n0 + 1):
                raise ValueError(f"{who}: assign must be [{B}, {n0 + 1}, {n0 + 1}], got {tuple(assign.shape)}")
        return d0, d1, B, n0, n1, assign

    def val_step(self, desc0, desc1, assign=None, lmatches=None, nn_thresh=0.7, mutual=True):
        """The reference's validation step after the forward, in one native call (linetr_val_step): descriptor_loss
        (evaluations/criteria.py), nn_matcher_batches (evaluations/matcher.py) and the precision / recall / F1 of
        evaluations/evaluate_pr.py.  desc0 / desc1: [B, 256, n] or [B*n, 256] (then `assign` / `lmatches` gives B); the ground truth is
        either `assign` [B, n+1, n+1] (mat_assign_sublines) or the loader's `lmatches` [B, M, 2].  One host wait.  Returns a dict:
        loss, hardest_positive, hardest_negative (float; NaN when count == 0), count, TP / FP / FN / TN (int32 [B]), precision /
        recall / f1 (float64 [B]) and the device tensors row_pos, row_neg [B, 2n] (row_neg -1: no anchor, or no semi-hard negative)
        and match01 [B, n]."""
        d0, d1, B, n0, n1, assign = self._criterion_args("val_step", desc0, desc1, assign, lmatches)
        n = n0
        offs = (C.c_int64 * 4)()
        out_bytes = int(self._L.linetr_val_step_output_bytes(B, offs))
        ws = self._workspace("val_step", max(int(self._L.linetr_val_step_workspace_bytes(B, n)), 256))
        stage, *gen = self._host_stage(out_bytes)
        row_pos = torch.empty((B, 2 * n), dtype=torch.float32, device=self.device)
        row_neg = torch.empty((B, 2 * n), dtype=torch.float32, device=self.device)
        match01 = torch.empty((B, n), dtype=torch.int32, device=self.device)
        self._call("linetr_val_step", d0.data_ptr(), n0, d1.data_ptr(), n1, assign.data_ptr(), B, float(nn_thresh), int(bool(mutual)),
                   row_pos.data_ptr(), row_neg.data_ptr(), match01.data_ptr(), stage.data_ptr(), stage.numel(), ws.data_ptr(), ws.numel())
        self._await_stage("val_step", self._event(), *gen)
        host = stage.numpy()
        scalars = host[offs[0]:offs[0] + 24].view(np.float64)
        counts = host[offs[2]:offs[2] + 16 * B].view(np.int32).reshape(B, 4).copy()
        scores = host[offs[3]:offs[3] + 24 * B].view(np.float64).reshape(B, 3).copy()
        return {"loss": float(scalars[0]), "hardest_positive": float(scalars[1]), "hardest_negative": float(scalars[2]),
                "count": int(host[offs[1]:offs[1] + 8].view(np.int64)[0]),
                "TP": counts[:, 0], "FP": counts[:, 1], "FN": counts[:, 2], "TN": counts[:, 3],
                "precision": scores[:, 0], "recall": scores[:, 1], "f1": scores[:, 2],
                "row_pos": row_pos, "row_neg": row_neg, "match01": match01}

    def loss_step(self, desc0, desc1, assign=None, lmatches=None, upstream=None):
        """descriptor_loss AND its gradient with respect to both descriptor sets in one native call (linetr_desc_loss_grad): what
        `loss.backward()` leaves in line_desc0.grad / line_desc1.grad when the reference's criterion (evaluations/criteria.py) is
        differentiated by torch.  Inputs as val_step takes them; `upstream`: the gradient arriving at the loss, a one-element float32
        device tensor (read on the device: no host wait for it), default 1.  One host wait.  Returns a dict: loss, hardest_positive,
        hardest_negative (float; NaN when count == 0), count, and the device tensors grad0 / grad1 in the shape of desc0 / desc1
        ([B, 256, n] inputs: the transposed view of the [B*n, 256] rows the kernels write); count == 0: both all zero.
        Like val_step, every call uses the engine's one cached workspace whatever the stream: calls from two streams are safe only
        because each ends in its host wait before it returns."""
        d0, d1, B, n0, n1, assign = self._criterion_args("loss_step", desc0, desc1, assign, lmatches)
        n = n0
        if upstream is not None:
            upstream = self._f32(upstream.detach().reshape(-1))
            if upstream.numel() != 1:
                raise ValueError("loss_step: upstream must hold one element")
        ws = self._workspace("loss_step", max(int(self._L.linetr_desc_loss_grad_workspace_bytes(B, n)), 256))
        stage, *gen = self._host_stage(32)
        grad0, grad1 = torch.empty_like(d0), torch.empty_like(d1)
        self._call("linetr_desc_loss_grad", d0.data_ptr(), n0, d1.data_ptr(), n1, assign.data_ptr(), B, ptr(upstream), grad0.data_ptr(),
                   grad1.data_ptr(), stage.data_ptr(), stage.numel(), ws.data_ptr(), ws.numel())
        self._await_stage("loss_step", self._event(), *gen)
        host = stage.numpy()
        scalars = host[:24].view(np.float64)
        grad0, grad1 = (g.view(B, n, D).transpose(1, 2) if d.dim() == 3 else g for g, d in ((grad0, desc0), (grad1, desc1)))
        return {"loss": float(scalars[0]), "hardest_positive": float(scalars[1]), "hardest_negative": float(scalars[2]),
                "count": int(host[24:32].view(np.int64)[0]), "grad0": grad0, "grad1": grad1}

    def hardnet_step(self, desc0, desc1, assign=None, lmatches=None, upstream=None, need_grad=True, rows=False):
        """The reference's HardNet criterion (descriptor_loss.compute_distances_hardnet under its forward, evaluations/criteria.py:126-192)
        and, with `need_grad`, its gradient with respect to both descriptor sets in one native call (linetr_hardnet_loss_grad): the
        hardest positive of every anchor line against the hardest negative of that line and of its positive's line.  Inputs and
        `upstream` as loss_step takes them.  One host wait.  Returns a dict: loss, hardest_positive, hardest_negative (float; NaN when
        count == 0; hardest_negative may be 10000), count, live (the anchors with pos - neg + 1 > 0); with need_grad the device tensors
        grad0 / grad1 in the shape of desc0 / desc1 (need_grad=False: the value-only call, the same scalars bit for bit, no gradient
        kernel); with `rows` the device tensors row_pos, row_neg [B, 2n] float32 and row_arg [B, 2n] int32 (row_neg and row_arg -1
        where the line is no anchor).  The engine's one cached workspace, as loss_step."""
        d0, d1, B, n0, n1, assign = self._criterion_args("hardnet_step", desc0, desc1, assign, lmatches)
        n = n0
        if upstream is not None:
            upstream = self._f32(upstream.detach().reshape(-1))
            if upstream.numel() != 1:
                raise ValueError("hardnet_step: upstream must hold one element")
        ws = self._workspace("hardnet_step", max(int(self._L.linetr_hardnet_loss_grad_workspace_bytes(B, n)), 256))
        stage, *gen = self._host_stage(40)
        grad0, grad1 = (torch.empty_like(d0), torch.empty_like(d1)) if need_grad else (None, None)
        row_pos = row_neg = row_arg = None
        if rows:
            row_pos, row_neg = (torch.empty((B, 2 * n), dtype=torch.float32, device=self.device) for _ in range(2))
            row_arg = torch.empty((B, 2 * n), dtype=torch.int32, device=self.device)
        self._call("linetr_hardnet_loss_grad", d0.data_ptr(), n0, d1.data_ptr(), n1, assign.data_ptr(), B, ptr(upstream), ptr(grad0),
                   ptr(grad1), ptr(row_pos), ptr(row_neg), ptr(row_arg), stage.data_ptr(), stage.numel(), ws.data_ptr(), ws.numel())
        self._await_stage("hardnet_step", self._event(), *gen)
        host = stage.numpy()
        scalars, counts = host[:24].view(np.float64), host[24:40].view(np.int64)
        res = {"loss": float(scalars[0]), "hardest_positive": float(scalars[1]), "hardest_negative": float(scalars[2]),
               "count": int(counts[0]), "live": int(counts[1])}
        if need_grad:
            res["grad0"], res["grad1"] = (g.view(B, n, D).transpose(1, 2) if d.dim() == 3 else g
                                          for g, d in ((grad0, desc0), (grad1, desc1)))
        if rows:
            res.update(row_pos=row_pos, row_neg=row_neg, row_arg=row_arg)
        return res

    # ------------------------------------------------------------------ backward of the 1x1 layers and the descriptor head
    def _act_rows(self, t: torch.Tensor, width: int, what: str, strided=True):
        """Activations as the point-wise layers read them: a float32 [rows, width] tensor whose rows are `stride(0)` floats apart
        (a multiple of 4, 16-byte aligned; anything else is copied).  Accepts [B, width, n] (contiguous, or the transposed view of
        [B*n, width] rows: no copy then) or the rows themselves.  Returns (rows, B or None, n or None)."""
        t = t.detach()
        if t.dim() == 3:
            if int(t.shape[1]) != width:
                raise ValueError(f"{what} must be [B, {width}, n] or [rows, {width}], got {tuple(t.shape)}")
            B, n = int(t.shape[0]), int(t.shape[2])
            return self._f32(t.transpose(1, 2)).view(B * n, width), B, n
        if t.dim() != 2 or int(t.shape[1]) != width:
            raise ValueError(f"{what} must be [B, {width}, n] or [rows, {width}], got {tuple(t.shape)}")
        ok = (strided and t.device == self.device and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) >= width
              and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)
        return (t if ok else self._f32(t)), None, None

    @staticmethod
    def _like_input(rows: torch.Tensor, B, n):
        """[B*n, C] rows back in the shape of a [B, C, n] input (the transposed view), or the rows of a 2-D input"""
        return rows if B is None else rows.view(B, n, rows.shape[1]).transpose(1, 2)

    def _weight_2d(self, weight: torch.Tensor) -> torch.Tensor:
        """a Conv1d(k=1) [N, K, 1] or a Linear [N, K] weight as [N, K] float32 on the device"""
        return self._f32(as_rows_weight(weight.detach()))

    def _stream_workspace(self, tag: str, nbytes: int) -> torch.Tensor:
        """the cached workspace of `tag` for the current stream (these calls return without a host wait: one per stream)"""
        return self._workspace(f"{tag}:{torch.cuda.current_stream(self.device).cuda_stream}", max(int(nbytes), 256))

    def linear_forward(self, x, weight, bias=None, relu=False) -> torch.Tensor:
        """A point-wise linear layer (Conv1d(k=1) / Linear) on the unfolded weight, by exact-fp32 MFMA (linetr_linear_forward):
        y = act(x W^T + b).  x: [B, K, n] or [rows, K]; weight [N, K] or [N, K, 1]; y in x's layout ([B, N, n] inputs: the transposed
        view of the [B*n, N] rows the kernel writes).  No host wait."""
        N, K = check_pointwise_shapes(x, weight, bias)
        W = self._weight_2d(weight)
        xr, B, n = self._act_rows(x, K, "x")
        b = self._f32(bias.detach().reshape(-1)) if bias is not None else None
        y = torch.empty((xr.shape[0], N), dtype=torch.float32, device=self.device)
        self._call("linetr_linear_forward", xr.data_ptr(), xr.stride(0), W.data_ptr(), ptr(b), int(xr.shape[0]), N, K, int(bool(relu)),
                   y.data_ptr(), N)
        return self._like_input(y, B, n)

    def linear_backward(self, x, weight, grad_out, mask=None, need=(True, True, True)):
        """The layer's backward (linetr_linear_backward): (dx, dW, db) for the gradient `grad_out` arriving at y = act(x W^T + b);
        `mask`: the layer's own post-ReLU output (the gradient passes where it is > 0), None for no activation.  dx in x's layout, dW in
        the weight's shape, db [N]; `need` = which of the three to compute (the others are None).  Deterministic; no host wait."""
        W = self._weight_2d(weight)
        N, K = int(W.shape[0]), int(W.shape[1])
        xr, B, n = self._act_rows(x, K, "x")
        g, _, _ = self._act_rows(grad_out, N, "grad_out", strided=mask is None)
        m = self._act_rows(mask, N, "mask", strided=False)[0] if mask is not None else None
        rows = int(xr.shape[0])
        if int(g.shape[0]) != rows or (m is not None and int(m.shape[0]) != rows):
            raise ValueError("linear_backward: x, grad_out and mask disagree about the number of rows")
        dx = torch.empty_strided((rows, K), (xr.stride(0), 1), dtype=torch.float32, device=self.device) if need[0] else None
        dW = torch.empty((N, K), dtype=torch.float32, device=self.device) if need[1] else None
        db = torch.empty((N,), dtype=torch.float32, device=self.device) if need[2] else None
        ws = self._stream_workspace("linear_bwd", self._L.linetr_linear_backward_workspace_bytes(rows, N, K))
        self._call("linetr_linear_backward", xr.data_ptr(), xr.stride(0), W.data_ptr(), g.data_ptr(), g.stride(0), ptr(m), rows, N, K, ptr(dx),
                   ptr(dW), ptr(db), ws.data_ptr(), ws.numel())
        return (self._like_input(dx, B, n) if dx is not None else None, dW.view(weight.shape) if dW is not None else None, db)

    def _head_args(self, x, weight, bias):
        W = self._weight_2d(weight)
        if tuple(W.shape) != (D, D) or bias is None or bias.numel() != D:
            raise ValueError(f"the descriptor head is final_proj: a [{D}, {D}] weight and a [{D}] bias")
        xr, B, n = self._act_rows(x, D, "x", strided=False)
        return xr, W, self._f32(bias.detach().reshape(-1)), B, n

    def head_forward(self, x, weight, bias) -> torch.Tensor:
        """The descriptor head (models/line_transformer.py:245-246; linetr_head_forward): line_desc = F.normalize(final_proj(x), dim=1),
        one kernel.  x: the pre-head features [B, 256, n] or [rows, 256]; line_desc in x's layout.  No host wait."""
        xr, W, b, B, n = self._head_args(x, weight, bias)
        desc = torch.empty_like(xr)
        self._call("linetr_head_forward", xr.data_ptr(), W.data_ptr(), b.data_ptr(), int(xr.shape[0]), desc.data_ptr())
        return self._like_input(desc, B, n)

    def head_backward(self, x, weight, bias, grad_desc, need=(True, True, True)):
        """The head's backward (linetr_head_backward): (dx, dW, db) for the gradient `grad_desc` arriving at line_desc, as torch autograd
        differentiates F.normalize(final_proj(x)).  Shapes and `need` as linear_backward.  Deterministic; no host wait."""
        xr, W, b, B, n = self._head_args(x, weight, bias)
        g = self._act_rows(grad_desc, D, "grad_desc", strided=False)[0]
        rows = int(xr.shape[0])
        if int(g.shape[0]) != rows:
            raise ValueError("head_backward: x and grad_desc disagree about the number of rows")
        dx = torch.empty_like(xr) if need[0] else None
        dW = torch.empty((D, D), dtype=torch.float32, device=self.device) if need[1] else None
        db = torch.empty((D,), dtype=torch.float32, device=self.device) if need[2] else None
        ws = self._stream_workspace("head_bwd", self._L.linetr_head_backward_workspace_bytes(rows))
        self._call("linetr_head_backward", xr.data_ptr(), W.data_ptr(), b.data_ptr(), g.data_ptr(), rows, ptr(dx), ptr(dW), ptr(db),
                   ws.data_ptr(), ws.numel())
        return (self._like_input(dx, B, n) if dx is not None else None, dW.view(weight.shape) if dW is not None else None, db)

    # ------------------------------------------------------------------ neighbour-line attention for training
    def _cu_sub_dev(self, cu_sub) -> torch.Tensor:
        """sub-line offsets [n_images + 1] as an int32 tensor on the device (a device tensor is taken as it is: no host wait)"""
        cu = cu_sub if isinstance(cu_sub, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(cu_sub, dtype=np.int32)))
        cu = cu.detach().reshape(-1)
        if cu.numel() < 2:
            raise ValueError("cu_sub must hold n_images + 1 >= 2 offsets")
        if cu.device != self.device or cu.dtype != torch.int32 or not cu.is_contiguous():
            cu = cu.to(device=self.device, dtype=torch.int32).contiguous()
        return cu

    def _attn_rows(self, named, N=None):
        """head-major [N, 256] rows as the attention kernels read them: strided row views pass as they are, anything else is copied"""
        rows = [self._act_rows(t, D, name)[0] for name, t in named]
        N = int(rows[0].shape[0]) if N is None else N
        for (name, _), r in zip(named, rows):
            if r.dim() != 2 or int(r.shape[0]) != N:
                raise ValueError(f"{name} must be [{N}, {D}] head-major rows, got {tuple(r.shape)}")
        return rows, N

    def sig_attention_forward(self, q, k, v, cu_sub):
        """The neighbour-line attention softmax(q^T k / 8) v of models/line_transformer.py:132-136 with its softmax statistics
        (linetr_sig_attention_forward; exact-fp32 MFMA).  q, k, v: head-major rows [N, 256] (column h*64 + d), q UNSCALED; each may be a
        strided row view, e.g. a column block of one [N, 768] buffer.  cu_sub [n_images + 1]: one image is one softmax domain (a device
        int32 tensor is read in place).  Returns (message [N, 256] head-major, lse [N, 4] = m + log l).  No host wait."""
        (qr, kr, vr), N = self._attn_rows((("q", q), ("k", k), ("v", v)))
        cu = self._cu_sub_dev(cu_sub)
        msg = torch.empty((N, D), dtype=torch.float32, device=self.device)
        lse = torch.empty((N, 4), dtype=torch.float32, device=self.device)
        if N == 0:                                   # (an empty tensor has no address to hand over)
            return msg, lse
        self._call("linetr_sig_attention_forward", qr.data_ptr(), qr.stride(0), kr.data_ptr(), kr.stride(0), vr.data_ptr(), vr.stride(0),
                   cu.data_ptr(), cu.numel() - 1, N, msg.data_ptr(), D, lse.data_ptr())
        return msg, lse

    def sig_attention_backward(self, q, k, v, o, lse, grad_out, cu_sub, need=(True, True, True)):
        """The attention's backward (linetr_sig_attention_backward): (dq, dk, dv) [N, 256] head-major for the gradient `grad_out` arriving at
        the message `o`; q, k, v, o, lse as sig_attention_forward took and returned them.  P is recomputed from q, k and lse; nothing n x n
        is stored.  `need` = which of the three to compute (the others are None).  Deterministic; no host wait."""
        (qr, kr, vr, orow, g), N = self._attn_rows((("q", q), ("k", k), ("v", v), ("o", o), ("grad_out", grad_out)))
        ls = self._f32(lse.detach())
        if tuple(ls.shape) != (N, 4):
            raise ValueError(f"lse must be [{N}, 4], got {tuple(ls.shape)}")
        cu = self._cu_sub_dev(cu_sub)
        dq, dk, dv = (torch.empty((N, D), dtype=torch.float32, device=self.device) if n else None for n in need)
        if N == 0:
            return dq, dk, dv
        ws = self._stream_workspace("sig_attn_bwd", self._L.linetr_sig_attention_backward_workspace_bytes(N))
        self._call("linetr_sig_attention_backward", qr.data_ptr(), qr.stride(0), kr.data_ptr(), kr.stride(0), vr.data_ptr(), vr.stride(0),
                   orow.data_ptr(), orow.stride(0), ls.data_ptr(), g.data_ptr(), g.stride(0), cu.data_ptr(), cu.numel() - 1, N, ptr(dq), D,
                   ptr(dk), D, ptr(dv), D, ws.data_ptr(), ws.numel())
        return dq, dk, dv

    # ------------------------------------------------------------------ BatchNorm (+ ReLU) for training
    def bn_forward(self, z, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True, relu=True):
        """torch.nn.BatchNorm1d (+ ReLU) out of place (linetr_bn_forward): y = relu?((z - mean) invstd gamma + beta) with the batch's mean
        and biased variance (`training`) or the running ones.  z: [B, C, n] (the transposed view of [B*n, C] rows: no copy) or
        [rows, C], rows may be strided; gamma, beta [C].  running_mean / running_var [C]: float32 device tensors, updated IN PLACE in
        training mode (both or neither), required and only read otherwise.  Returns (y in z's layout, save: float64 [2 C] mean | invstd,
        what bn_backward takes).  No host wait."""
        C_ = int(gamma.numel())
        zr, B, n = self._act_rows(z, C_, "z")
        rows = int(zr.shape[0])
        if (running_mean is None) != (running_var is None) or (not training and running_mean is None):
            raise ValueError("bn_forward: running_mean and running_var come together, and eval mode needs them")
        run = None
        if running_mean is not None:
            for t in (running_mean, running_var):
                if t.device != self.device or t.dtype != torch.float32 or tuple(t.shape) != (C_,):
                    raise ValueError(f"bn_forward: the running statistics must be float32 [{C_}] tensors on {self.device}")
            run = torch.cat([running_mean.detach(), running_var.detach()])
        y = torch.empty((rows, C_), dtype=torch.float32, device=self.device)
        save = torch.empty((2 * C_,), dtype=torch.float64, device=self.device)
        if rows == 0:
            return self._like_input(y, B, n), save.zero_()
        ws = self._stream_workspace("bn_fwd", self._L.linetr_bn_forward_workspace_bytes(rows, C_))
        self._call("linetr_bn_forward", zr.data_ptr(), zr.stride(0), rows, C_, self._f32(gamma.detach().reshape(-1)).data_ptr(),
                   self._f32(beta.detach().reshape(-1)).data_ptr(), float(eps), float(momentum), ptr(run), int(not training), int(bool(relu)),
                   y.data_ptr(), C_, save.data_ptr(), ws.data_ptr(), ws.numel())
        if training and run is not None:
            with torch.no_grad():
                running_mean.copy_(run[:C_])
                running_var.copy_(run[C_:])
        return self._like_input(y, B, n), save

    def bn_backward(self, z, y, grad_out, save, gamma, training=True, need=(True, True, True)):
        """The layer's backward (linetr_bn_backward): (dz, dgamma, dbeta) for the gradient `grad_out` arriving at y; z and save as
        bn_forward took and returned them, y: the layer's own post-ReLU output (the mask y > 0), None for no activation.  dz in z's
        layout; `need` = which of the three to compute (the others are None).  Deterministic; no host wait."""
        C_ = int(gamma.numel())
        zr, B, n = self._act_rows(z, C_, "z")
        g = self._act_rows(grad_out, C_, "grad_out")[0]
        m = self._act_rows(y, C_, "y")[0] if y is not None else None
        rows = int(zr.shape[0])
        if int(g.shape[0]) != rows or (m is not None and int(m.shape[0]) != rows):
            raise ValueError("bn_backward: z, grad_out and y disagree about the number of rows")
        if save.device != self.device or save.dtype != torch.float64 or tuple(save.shape) != (2 * C_,) or not save.is_contiguous():
            raise ValueError(f"bn_backward: save must be the float64 [{2 * C_}] tensor bn_forward returned")
        dz = torch.empty((rows, C_), dtype=torch.float32, device=self.device) if need[0] else None
        dgamma, dbeta = (torch.empty((C_,), dtype=torch.float32, device=self.device) if k else None for k in need[1:3])
        if rows == 0:
            return (self._like_input(dz, B, n) if dz is not None else None, dgamma.zero_() if dgamma is not None else None,
                    dbeta.zero_() if dbeta is not None else None)
        ws = self._stream_workspace("bn_bwd", self._L.linetr_bn_backward_workspace_bytes(rows, C_))
        self._call("linetr_bn_backward", zr.data_ptr(), zr.stride(0), ptr(m), m.stride(0) if m is not None else 0, g.data_ptr(), g.stride(0),
                   save.data_ptr(), self._f32(gamma.detach().reshape(-1)).data_ptr(), rows, C_, int(not training), ptr(dz), C_, ptr(dgamma),
                   ptr(dbeta), ws.data_ptr(), ws.numel())
        return self._like_input(dz, B, n) if dz is not None else None, dgamma, dbeta

    # ------------------------------------------------------------------ the descriptive layer for training: CLS pooling, LayerNorm, GELU
    def _rows_of(self, t, shape, what, strided=True):
        """a float32 2-D device tensor of exactly `shape` as the kernels read it (strided rows pass as they are, anything else is copied)"""
        if t.dim() != 2 or tuple(int(v) for v in t.shape) != tuple(shape):
            raise ValueError(f"{what} must be {list(shape)}, got {tuple(t.shape)}")
        return self._act_rows(t, int(shape[1]), what, strided=strided)[0]

    def _pool_args(self, x, u):
        if x.dim() != 3 or int(x.shape[2]) != D or not 1 <= int(x.shape[1]) <= 256:
            raise ValueError(f"x must be [L, S, {D}] token rows with 1 <= S <= 256, got {tuple(x.shape)}")
        L, S = int(x.shape[0]), int(x.shape[1])
        if tuple(u.shape) != (L, 4, D):
            raise ValueError(f"u must be [{L}, 4, {D}], got {tuple(u.shape)}")
        return self._f32(x.detach()).view(L * S, D), self._f32(u.detach()).view(L, 4 * D), L, S

    def _cls_pool_fwd(self, x, u, drop=None):
        """cls_pool_forward (`drop` None: kept is None) and cls_pool_dropout_forward: (pooled, kept, lse)"""
        xr, ur, L, S = self._pool_args(x, u)
        pooled = torch.empty((L, 4, D), dtype=torch.float32, device=self.device)
        lse = torch.empty((L, 4), dtype=torch.float32, device=self.device)
        kept = torch.empty_like(lse) if drop is not None else None
        if L == 0:                                   # (an empty tensor has no address to hand over)
            return pooled, kept, lse
        if drop is None:
            self._call("linetr_cls_pool_train_forward", xr.data_ptr(), D, ur.data_ptr(), 4 * D, L, S, pooled.data_ptr(), lse.data_ptr())
        else:
            self._call("linetr_cls_pool_dropout_forward", xr.data_ptr(), D, ur.data_ptr(), 4 * D, L, S, C.byref(drop), pooled.data_ptr(),
                       kept.data_ptr(), lse.data_ptr())
        return pooled, kept, lse

    def _cls_pool_bwd(self, x, u, pooled, lse, grad_pooled, need, drop=None, kept=None, grad_kept=None):
        """cls_pool_backward (`drop` None) and cls_pool_dropout_backward: (dx, du)"""
        xr, ur, L, S = self._pool_args(x, u)
        pr = self._rows_of(pooled.detach().reshape(L, 4 * D), (L, 4 * D), "pooled", strided=False)
        gr = self._rows_of(grad_pooled.detach().reshape(L, 4 * D), (L, 4 * D), "grad_pooled", strided=False)
        ls = self._rows_of(lse.detach(), (L, 4), "lse", strided=False)
        if drop is not None:
            kp = self._rows_of(kept.detach(), (L, 4), "kept", strided=False)
            gk = self._rows_of(grad_kept.detach(), (L, 4), "grad_kept", strided=False) if grad_kept is not None else None
        dx = torch.empty((L, S, D), dtype=torch.float32, device=self.device) if need[0] else None
        du = torch.empty((L, 4, D), dtype=torch.float32, device=self.device) if need[1] else None
        if L == 0:
            return dx, du
        if drop is None:
            self._call("linetr_cls_pool_train_backward", xr.data_ptr(), D, ur.data_ptr(), 4 * D, pr.data_ptr(), ls.data_ptr(), gr.data_ptr(), L, S,
                       ptr(dx), D, ptr(du), 4 * D)
        else:
            self._call("linetr_cls_pool_dropout_backward", xr.data_ptr(), D, ur.data_ptr(), 4 * D, pr.data_ptr(), ls.data_ptr(), kp.data_ptr(),
                       gr.data_ptr(), ptr(gk), L, S, C.byref(drop), ptr(dx), D, ptr(du), 4 * D)
        return dx, du

    def cls_pool_forward(self, x, u):
        """The CLS row's attention pooling of the descriptive layer in its folded form (linetr_cls_pool_train_forward): per segment l and
        head h, p = softmax_t(u[l, h] . x[l, t]) and pooled[l, h] = sum_t p_t x[l, t].  x [L, S, 256] token rows (slot 0: the CLS token),
        u [L, 4, 256] = Wk_h^T (q_h / 8).  Returns (pooled [L, 4, 256], lse [L, 4]).  No host wait."""
        pooled, _, lse = self._cls_pool_fwd(x, u)
        return pooled, lse

    def cls_pool_backward(self, x, u, pooled, lse, grad_pooled, need=(True, True)):
        """The pooling's backward (linetr_cls_pool_train_backward): (dx [L, S, 256], du [L, 4, 256]) for the gradient `grad_pooled`
        arriving at pooled; x, u, pooled, lse as cls_pool_forward took and returned them.  p is recomputed from x, u and lse.  `need` =
        which of the two to compute (the other is None).  Deterministic; no host wait."""
        return self._cls_pool_bwd(x, u, pooled, lse, grad_pooled, need)
    def _ln_args(self, who, a, residual, gamma):
        if a.dim() != 2 or int(a.shape[1]) != D or int(gamma.numel()) != D:
            raise ValueError(f"{who}: the native LayerNorm is over rows of {D}, got {tuple(a.shape)} and {int(gamma.numel())} weights")
        ar = self._act_rows(a, D, "a")[0]
        rr = self._rows_of(residual.detach(), a.shape, "residual") if residual is not None else None
        return ar, rr, self._f32(gamma.detach().reshape(-1)), int(ar.shape[0])

    def _ln_fwd(self, who, a, residual, gamma, beta, eps, drop=None, site=None):
        """layer_norm_forward (`drop` None) and layer_norm_dropout_forward: (y, stats)"""
        ar, rr, gm, rows = self._ln_args(who, a, residual, gamma)
        y = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=self.device)
        if rows == 0:
            return y, stats
        dropout = () if drop is None else (C.byref(drop), int(site))
        self._call("linetr_" + who, ar.data_ptr(), ar.stride(0), ptr(rr), rr.stride(0) if rr is not None else 0, gm.data_ptr(),
                   self._f32(beta.detach().reshape(-1)).data_ptr(), float(eps), rows, D, *dropout, y.data_ptr(), D, stats.data_ptr())
        return y, stats

    def _ln_bwd(self, who, a, residual, stats, gamma, grad_out, need, drop=None, site=None):
        """layer_norm_backward (`drop` None: da is None and dresidual is its dx) and layer_norm_dropout_backward:
        (da, dresidual, dgamma, dbeta); `need` = which of the four"""
        ar, rr, gm, rows = self._ln_args(who, a, residual, gamma)
        g = self._rows_of(grad_out.detach(), (rows, D), "grad_out")
        st = self._rows_of(stats.detach(), (rows, 2), "stats", strided=False)
        da, dr = (torch.empty((rows, D), dtype=torch.float32, device=self.device) if k else None for k in need[:2])
        dgamma, dbeta = (torch.empty((D,), dtype=torch.float32, device=self.device) if k else None for k in need[2:4])
        if rows == 0:
            return da, dr, dgamma.zero_() if dgamma is not None else None, dbeta.zero_() if dbeta is not None else None
        ws = self._stream_workspace("layer_norm_bwd", self._L.linetr_layer_norm_backward_workspace_bytes(rows, D))
        grads = (ptr(dr), D) if drop is None else (C.byref(drop), int(site), ptr(da), D, ptr(dr), D)
        self._call("linetr_" + who, ar.data_ptr(), ar.stride(0), ptr(rr), rr.stride(0) if rr is not None else 0, st.data_ptr(), gm.data_ptr(),
                   g.data_ptr(), g.stride(0), rows, D, *grads, ptr(dgamma), ptr(dbeta), ws.data_ptr(), ws.numel())
        return da, dr, dgamma, dbeta

    def layer_norm_forward(self, a, residual, gamma, beta, eps=1e-6):
        """y = LayerNorm(a + residual) gamma + beta over rows of 256 (linetr_layer_norm_forward); a, residual [rows, 256] (rows may be
        strided; residual may be None), the add one float32 add.  Returns (y [rows, 256], stats [rows, 2] float32: mean | rstd, what
        layer_norm_backward takes).  No host wait."""
        return self._ln_fwd("layer_norm_forward", a, residual, gamma, beta, eps)

    def layer_norm_backward(self, a, residual, stats, gamma, grad_out, need=(True, True, True)):
        """The layer's backward (linetr_layer_norm_backward): (dx, dgamma, dbeta) for the gradient `grad_out` arriving at y; dx [rows, 256]
        is the gradient of a and of the residual alike.  `need` = which of the three to compute (the others are None).  Deterministic;
        no host wait."""
        return self._ln_bwd("layer_norm_backward", a, residual, stats, gamma, grad_out, (False, *need))[1:]

    # ------------------------------------------------------------------ the same with training-time dropout (csrc/lt_dropout.h)
    @staticmethod
    def dropout(seed: int, call: int, p: float) -> nat.Dropout:
        """The LinetrDropout of (seed, call, p): threshold = floor(p 2^32), scale = float32(1 / (1 - p)); 0 <= p < 1, else ValueError.  The
        masks are a pure function of it, the site and the element: a backward takes the one its forward took."""
        return nat.Dropout.make(seed, call, p)

    def dropout_factors(self, drop: nat.Dropout, site: int, rows: int, inner: int) -> torch.Tensor:
        """The factors a dropout kernel applies (linetr_dropout_factors): [rows, inner, 4] float32, `scale` or 0.  Site 0: [segment, token,
        head]; sites 1 / 2: [row, column / 4, column % 4].  Stateless.  No host wait."""
        out = torch.empty((int(rows), int(inner), 4), dtype=torch.float32, device=self.device)
        if out.numel():
            self._call("linetr_dropout_factors", C.byref(drop), int(site), int(rows), int(inner), out.data_ptr())
        return out

    def cls_pool_dropout_forward(self, x, u, drop: nat.Dropout):
        """cls_pool_forward with dropout on the softmax weights (site 0; linetr_cls_pool_dropout_forward): a = p r, pooled = sum_t a_t x_t,
        kept = sum_t a_t.  Returns (pooled [L, 4, 256], kept [L, 4], lse [L, 4]).  No host wait."""
        return self._cls_pool_fwd(x, u, drop)

    def cls_pool_dropout_backward(self, x, u, pooled, lse, kept, grad_pooled, grad_kept, drop: nat.Dropout, need=(True, True)):
        """The backward of cls_pool_dropout_forward (linetr_cls_pool_dropout_backward): (dx, du) for the gradients arriving at pooled and
        at kept (`grad_kept` None: none arrives); `drop`: what the forward took -- the masks are generated again.  Deterministic; no
        host wait."""
        return self._cls_pool_bwd(x, u, pooled, lse, grad_pooled, need, drop, kept, grad_kept)

    def layer_norm_dropout_forward(self, a, residual, gamma, beta, drop: nat.Dropout, site: int, eps=1e-6):
        """y = LayerNorm(r a + residual) with r the factors of `site` (1 or 2; linetr_layer_norm_dropout_forward).  Returns (y, stats) as
        layer_norm_forward.  No host wait."""
        return self._ln_fwd("layer_norm_dropout_forward", a, residual, gamma, beta, eps, drop, site)

    def layer_norm_dropout_backward(self, a, residual, stats, gamma, grad_out, drop: nat.Dropout, site: int, need=(True, True, True, True)):
        """The backward of layer_norm_dropout_forward (linetr_layer_norm_dropout_backward): (da, dresidual, dgamma, dbeta) with dresidual =
        dv and da = r dv, the masks generated again from `drop` and `site`.  `need` = which of the four to compute (the others are
        None).  Deterministic; no host wait."""
        return self._ln_bwd("layer_norm_dropout_backward", a, residual, stats, gamma, grad_out, need, drop, site)

    def _gelu_rows(self, z, what):
        if z.dim() != 2 or int(z.shape[1]) % 4 or not 4 <= int(z.shape[1]) <= 4096:
            raise ValueError(f"{what} must be [rows, C] with C a multiple of 4 up to 4096, got {tuple(z.shape)}")
        return self._act_rows(z, int(z.shape[1]), what)[0]

    def gelu_forward(self, z) -> torch.Tensor:
        """F.gelu(z), erf form, on rows [rows, C] (linetr_gelu_forward).  No host wait."""
        zr = self._gelu_rows(z, "z")
        y = torch.empty(tuple(zr.shape), dtype=torch.float32, device=self.device)
        if zr.numel():
            self._call("linetr_gelu_forward", zr.data_ptr(), zr.stride(0), int(zr.shape[0]), int(zr.shape[1]), y.data_ptr(), int(zr.shape[1]))
        return y

    def gelu_backward(self, z, grad_out) -> torch.Tensor:
        """dz = grad_out (Phi(z) + z phi(z)) from the pre-activation z (linetr_gelu_backward).  No host wait."""
        zr = self._gelu_rows(z, "z")
        g = self._rows_of(grad_out.detach(), zr.shape, "grad_out")
        dz = torch.empty(tuple(zr.shape), dtype=torch.float32, device=self.device)
        if zr.numel():
            self._call("linetr_gelu_backward", zr.data_ptr(), zr.stride(0), g.data_ptr(), g.stride(0), int(zr.shape[0]), int(zr.shape[1]),
                       dz.data_ptr(), int(zr.shape[1]))
        return dz

    # ------------------------------------------------------------------ the positional encoders' input layer and the token assembly
    def _narrow_rows(self, x, Kin, what):
        """the encoders' input [rows, Kin] as the input-layer kernels read it: float32 on the device, unit column stride, any row
        stride and alignment (anything else is copied)"""
        x = x.detach()
        if x.dim() != 2 or int(x.shape[1]) != Kin:
            raise ValueError(f"{what} must be [rows, {Kin}], got {tuple(x.shape)}")
        ok = x.device == self.device and x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) >= Kin
        return x if ok else self._f32(x)

    @staticmethod
    def _input_layer_shape(weight):
        W = as_rows_weight(weight.detach())
        N, Kin = int(W.shape[0]), int(W.shape[1])
        if not 1 <= Kin <= 8 or N % 4 or not 4 <= N <= 64:
            raise ValueError(f"the native input layer takes 1 <= Kin <= 8 inputs and N % 4 == 0, 4 <= N <= 64 outputs, got a weight {tuple(weight.shape)}")
        return W, N, Kin

    def input_layer_forward(self, x, weight, bias=None) -> torch.Tensor:
        """The first layer of a positional encoder, Conv1d(Kin -> N, k = 1) with 1 <= Kin <= 8 and N % 4 == 0, 4 <= N <= 64, which is no
        GEMM (linetr_input_layer_forward): z = x W^T + b.  x [rows, Kin] (rows may be strided, any alignment); weight [N, Kin] or
        [N, Kin, 1]; returns z [rows, N].  No host wait."""
        W, N, Kin = self._input_layer_shape(weight)
        W = self._f32(W)
        xr = self._narrow_rows(x, Kin, "x")
        b = self._f32(bias.detach().reshape(-1)) if bias is not None else None
        if b is not None and b.numel() != N:
            raise ValueError(f"bias must hold {N} values, got {tuple(bias.shape)}")
        rows = int(xr.shape[0])
        z = torch.empty((rows, N), dtype=torch.float32, device=self.device)
        if rows:
            self._call("linetr_input_layer_forward", xr.data_ptr(), xr.stride(0), W.data_ptr(), ptr(b), rows, N, Kin, z.data_ptr(), N)
        return z

    def input_layer_backward(self, x, weight, grad_out, need=(True, True)):
        """The layer's backward (linetr_input_layer_backward): (dW in the weight's shape, db [N]) for the gradient `grad_out` [rows, N]
        arriving at z; there is no dx (the encoders' inputs never require a gradient).  `need` = which of the two to compute (the other
        is None).  Deterministic; no host wait."""
        _, N, Kin = self._input_layer_shape(weight)
        xr = self._narrow_rows(x, Kin, "x")
        rows = int(xr.shape[0])
        g = self._rows_of(grad_out.detach(), (rows, N), "grad_out")
        dW = torch.empty((N, Kin), dtype=torch.float32, device=self.device) if need[0] else None
        db = torch.empty((N,), dtype=torch.float32, device=self.device) if need[1] else None
        if rows == 0:
            return dW.zero_().view(weight.shape) if dW is not None else None, db.zero_() if db is not None else None
        ws = self._stream_workspace("input_layer_bwd", self._L.linetr_input_layer_backward_workspace_bytes(rows, N, Kin))
        self._call("linetr_input_layer_backward", xr.data_ptr(), xr.stride(0), g.data_ptr(), g.stride(0), rows, N, Kin, ptr(dW), ptr(db),
                   ws.data_ptr(), ws.numel())
        return dW.view(weight.shape) if dW is not None else None, db

    def _token_args(self, who, desc, pos):
        if desc.dim() != 3 or int(desc.shape[2]) != D or not 1 <= int(desc.shape[1]) <= 255 or pos.shape != desc.shape:
            raise ValueError(f"{who}: desc and pos must share the shape [L, S, {D}] with 1 <= S <= 255, got {tuple(desc.shape)} and {tuple(pos.shape)}")
        return self._f32(desc.detach()), self._f32(pos.detach()), int(desc.shape[0]), int(desc.shape[1])

    def assemble_tokens_forward(self, desc, pos, cls_token) -> torch.Tensor:
        """The token rows of the descriptive layer (linetr_token_assemble_forward): x [L, S + 1, 256] with x[:, 0] = cls_token and
        x[:, 1:] = desc + pos (one float32 add).  desc, pos [L, S, 256], 1 <= S <= 255; cls_token: 256 values.  No host wait."""
        d, p, L, S = self._token_args("assemble_tokens_forward", desc, pos)
        cls = self._f32(cls_token.detach().reshape(-1))
        if cls.numel() != D:
            raise ValueError(f"cls_token must hold {D} values, got {tuple(cls_token.shape)}")
        x = torch.empty((L, S + 1, D), dtype=torch.float32, device=self.device)
        if L:                                        # (an empty tensor has no address to hand over)
            self._call("linetr_token_assemble_forward", d.data_ptr(), p.data_ptr(), cls.data_ptr(), L, S, x.data_ptr())
        return x

    def assemble_tokens_backward(self, grad_x, need=(True, True)):
        """The assembly's backward (linetr_token_assemble_backward), one pass over grad_x [L, S + 1, 256]: (dtok [L, S, 256] = grad_x[:, 1:]
        as contiguous rows -- the gradient of desc and of pos alike --, dcls [256] = the sum of grad_x[:, 0]).  `need` = which of the two
        to compute (the other is None).  Deterministic; no host wait."""
        if grad_x.dim() != 3 or int(grad_x.shape[2]) != D or not 2 <= int(grad_x.shape[1]) <= 256:
            raise ValueError(f"grad_x must be [L, S + 1, {D}] with 1 <= S <= 255, got {tuple(grad_x.shape)}")
        g = self._f32(grad_x.detach())
        L, S = int(g.shape[0]), int(g.shape[1]) - 1
        dtok = torch.empty((L, S, D), dtype=torch.float32, device=self.device) if need[0] else None
        dcls = torch.empty((D,), dtype=torch.float32, device=self.device) if need[1] else None
        if L == 0:
            return dtok, dcls.zero_() if dcls is not None else None
        ws = self._stream_workspace("token_assemble_bwd", self._L.linetr_token_assemble_backward_workspace_bytes(L))
        self._call("linetr_token_assemble_backward", g.data_ptr(), L, S, ptr(dtok), ptr(dcls), ws.data_ptr(), ws.numel())
        return dtok, dcls

    # ------------------------------------------------------------------ the optimizer step and the gradient norm (csrc/lt_adam.h)
    def _adam_table(self, who, grads, rest=None):
        """The host table (nat.ADAM_TENSOR_DTYPE records) of `grads` and, for the step, of `rest` = (params, exp_avgs, exp_avg_sqs):
        contiguous float32 tensors on the engine's device, every one of a row the size of its gradient.  Returns (table, n_total)."""
        lists = [list(grads)] + ([list(r) for r in rest] if rest is not None else [])
        if not lists[0] or any(len(l) != len(lists[0]) for l in lists):
            raise ValueError(f"{who}: the tensor lists must be non-empty and equally long")
        table = np.zeros(len(lists[0]), dtype=nat.ADAM_TENSOR_DTYPE)
        sizes = [t.numel() for t in lists[0]]
        dev, f32, strided = self.device, torch.float32, torch.strided
        for name, column in zip(("g", "p", "m", "v"), lists):
            for t in column:                                 # (the host cost of a step is this loop: 4 x 153 tensors for the model)
                if t.dtype is not f32 or t.device != dev or t.layout is not strided or not t.is_contiguous():
                    raise ValueError(f"{who}: every tensor must be a contiguous float32 tensor on {self.device}")
            table[name] = [t.data_ptr() for t in column]
            if name != "g" and [t.numel() for t in column] != sizes:
                raise ValueError(f"{who}: a parameter, its gradient and its two moments must hold equally many elements")
        table["n"] = sizes
        return table, sum(sizes)

    def adam_step(self, params, grads, exp_avgs, exp_avg_sqs, steps, *, lr, betas, eps, weight_decay, decoupled=False, grad_scale=None):
        """One Adam step over every tensor of the lists in ONE native call (linetr_adam_step), the functional form, like
        torch.optim._functional.adam: params, exp_avgs and exp_avg_sqs are updated in place in the arithmetic of torch's single-tensor path
        (include/linetr_hip.h); grads are only read.  `steps`: the step count of each parameter AFTER this step (Python numbers; the bias
        corrections are made here in double, per tensor).  `grad_scale`: a one-element float32 device tensor every gradient is multiplied
        by on the way in (grad_norm's scale), read on the device.  The tensors are written through raw pointers: their autograd version
        counters do not move (linetr_amd.optim.Adam moves them).  No host wait."""
        table, n_total = self._adam_table("adam_step", grads, (params, exp_avgs, exp_avg_sqs))
        steps = list(steps)
        if len(steps) != len(table):
            raise ValueError("adam_step: one step count per parameter")
        if isinstance(lr, torch.Tensor):
            raise ValueError("adam_step: a tensor lr is not supported")
        corr = [nat.adam_bias_corrections(lr, betas[0], betas[1], s) for s in steps]
        table["step_size"] = [c[0] for c in corr]
        table["bc2_sqrt"] = [c[1] for c in corr]
        hyper = nat.AdamHyper(float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(lr), int(bool(decoupled)))
        if grad_scale is not None:
            if grad_scale.device != self.device or grad_scale.dtype != torch.float32 or grad_scale.numel() != 1:
                raise ValueError(f"adam_step: grad_scale must be a one-element float32 tensor on {self.device}")
        ws = self._stream_workspace("adam_step", self._L.linetr_adam_workspace_bytes(len(table), n_total))
        self._call("linetr_adam_step", table.ctypes.data, len(table), C.byref(hyper), ptr(grad_scale), ws.data_ptr(), ws.numel())

    def grad_norm(self, grads, max_norm=float("inf")):
        """The L2 norm of all `grads` together and the coefficient of torch.nn.utils.clip_grad_norm_ (linetr_grad_norm): (norm: a float64
        scalar tensor, scale: a float32 one-element tensor = min(1, max_norm / (norm + 1e-6))), both on the device.  Deterministic: float64
        sums in a fixed order.  No host wait."""
        table, n_total = self._adam_table("grad_norm", grads)
        with torch.cuda.device(self.device):
            norm = torch.empty((), dtype=torch.float64, device=self.device)
            scale = torch.empty((1,), dtype=torch.float32, device=self.device)
        ws = self._stream_workspace("grad_norm", self._L.linetr_grad_norm_workspace_bytes(len(table), n_total))
        self._call("linetr_grad_norm", table.ctypes.data, len(table), float(max_norm), norm.data_ptr(), scale.data_ptr(), ws.data_ptr(), ws.numel())
        return norm, scale

    # ------------------------------------------------------------------ fixed-size training samples (csrc/lt_fixedsize.h)
    FIXED_SIZE_SHAPES = (("klines", ("M", 2, 2)), ("length_klines", ("M",)), ("angles", ("M", 2)), ("sublines", ("M", 2, 2)),
                         ("pnt_sublines", ("M", "T", 2)), ("mask_sublines", ("M", "S", 1)), ("resp_sublines", ("M", 1)),
                         ("angle_sublines", ("M", 2)), ("desc_sublines", ("M", "T", D)), ("score_sublines", ("M", "T", 1)),
                         ("mat_klines2sublines", ("M", "M")))
    _FIXED_SIZE_FIELDS = ("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "desc", "score", "mat")

    @classmethod
    def fixed_size_shapes(cls, B, max_sublines, max_tokens):
        """{key: shape} of the float32 tensors fixed_size_batch returns"""
        dims = {"M": int(max_sublines), "T": int(max_tokens), "S": int(max_tokens) + 1}
        return {k: (int(B), *(dims.get(d, d) for d in sh)) for k, sh in cls.FIXED_SIZE_SHAPES}

    def fixed_size_batch(self, recs, cu_k, cu_n, dense_desc, dense_score, *, max_sublines, token_distance, max_tokens, min_length=16,
                         resize=(640, 480), seed=None, pseudo_lines=None, dense_layout="nchw", align_corners=False, clip_shape=None,
                         out=None):
        """Fixed-size training samples of a batch in one native call (linetr_fixed_size): the 'klines' branch of the reference's
        conv_fixed_size (dataloaders/utils/util_lines.py:695-766) applied to what `preprocess` returns for each image, without the
        per-image tensors ever existing.  recs, cu_k, cu_n: the pre-filter's (prefilter / pack_many); dense maps as tokenize takes
        them; clip_shape: tokenize's, for the real lines.

        Image b with num_slns < max_sublines is padded with max_sublines - num_slns tokenised pseudo lines, clipped as the dataset
        builder clips them: `resize` = conf['data']['resize'] reaches line_tokenizer as (height, width).  The lines are
        `pseudo_lines[b]` = {'klines', 'length_klines', 'angles'} (float64, as find_line_attributes returns them; None or absent
        where none is needed), or, with pseudo_lines=None, util_lines.make_pseudo_lines + find_line_attributes with the Philox stream
        of (seed, b) -- seed None is 0.  Every pseudo line must make exactly one sub-line.  An image with num_slns >= max_sublines
        is cut to its first max_sublines sub-lines; more key-lines than max_sublines is refused, as the reference raises.  An image
        with no line at all is all pseudo lines (the reference raises there).

        Returns a dict of device tensors under the reference's key names with leading axis B (fixed_size_shapes), num_klns /
        num_slns (int64 [B], the counts before padding or truncation) and 'pseudo_lines': the host float64 dicts used, one per
        image (None where none was needed).  `out`: float32 device tensors to write into instead of new ones.  No host wait."""
        from . import util_lines
        cu_k32, cu_n32 = (np.ascontiguousarray(c, dtype=np.int32) for c in (cu_k, cu_n))
        B = len(cu_k32) - 1
        M, T = int(max_sublines), int(max_tokens)
        if B < 1 or len(cu_n32) != B + 1:
            raise ValueError("fixed_size_batch: cu_k and cu_n must hold B + 1 >= 2 prefix sums")
        # (linetr_fixed_size takes float32 maps only: a half map is upcast, as every map of another type is)
        dense_desc, dense_score, H, W, nhwc = self._dense_maps(dense_desc, dense_score, B, dense_layout, in_place=False)
        n_add = np.maximum(M - np.diff(cu_n32).astype(np.int64), 0)
        if pseudo_lines is None:
            pseudo_lines = [util_lines.find_line_attributes(util_lines.make_pseudo_lines(int(n), resize, seed=seed or 0, image=b), min_length, M)
                            if n else None for b, n in enumerate(n_add)]
        pseudo_lines = list(pseudo_lines) + [None] * (B - len(pseudo_lines))
        if len(pseudo_lines) != B:
            raise ValueError(f"fixed_size_batch: {len(pseudo_lines)} pseudo-line sets for {B} images")
        counts = [0 if p is None else len(p["klines"]) for p in pseudo_lines]
        cu_p = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(counts, out=cu_p[1:])
        precs = np.zeros(max(int(cu_p[-1]), 1), dtype=nat.REC_DTYPE)
        n_out = C.c_int32()
        for b, p in enumerate(pseudo_lines):
            if counts[b]:
                kl, ln, an = (np.ascontiguousarray(p[k], dtype=np.float64) for k in ("klines", "length_klines", "angles"))
                nat.check(self._L.linetr_pack_lines(nat.np_ptr(kl), nat.np_ptr(ln), nat.np_ptr(an), counts[b], float(token_distance), T, b, 0, 0,
                                                    nat.np_ptr(precs[cu_p[b]:cu_p[b + 1]]), C.byref(n_out)), self._L)
        shapes = self.fixed_size_shapes(B, M, T)
        f = dict(dtype=torch.float32, device=self.device)
        if out is None:
            out = {k: torch.empty(sh, **f) for k, sh in shapes.items()}
        for k, sh in shapes.items():
            t = out[k]
            if tuple(t.shape) != sh or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"fixed_size_batch: out['{k}'] must be a contiguous float32 {sh} tensor on {self.device}")
        counts_dev = torch.empty((2, B), dtype=torch.int32, device=self.device)
        K = int(cu_k32[-1])
        d_recs = torch.from_numpy(np.ascontiguousarray(recs[:K]).view(np.uint8).reshape(-1).copy()).to(self.device) if K else None
        d_precs = torch.from_numpy(precs.view(np.uint8).reshape(-1)).to(self.device) if int(cu_p[-1]) else None
        ct = nat.Tokens()
        for field, key in zip(self._FIXED_SIZE_FIELDS, shapes):
            setattr(ct, field, out[key].data_ptr())
        ws = self._stream_workspace("fixed_size", self._L.linetr_fixed_size_workspace_bytes(B, H, W, int(nhwc)))
        clip = (int(clip_shape[0]), int(clip_shape[1])) if clip_shape is not None else (0, 0)
        self._call("linetr_fixed_size", ptr(d_recs), nat.np_ptr(cu_k32), nat.np_ptr(cu_n32), ptr(d_precs), nat.np_ptr(precs), nat.np_ptr(cu_p), B, M, T,
                   float(token_distance), dense_desc.data_ptr(), dense_score.data_ptr(), H, W, clip[0], clip[1], int(resize[0]), int(resize[1]),
                   int(bool(align_corners)), int(nhwc), ct, counts_dev[0].data_ptr(), counts_dev[1].data_ptr(), ws.data_ptr(), ws.numel())
        res = {k: out[k] for k in shapes}
        res["num_klns"], res["num_slns"] = counts_dev[0].to(torch.int64), counts_dev[1].to(torch.int64)
        res["pseudo_lines"] = pseudo_lines
        return res

    def line_ground_truth(self, lines0, lines1, H, *, thres_reprojected=3, thres_angdiff=2, min_overlap_ratio=0.3, max_matches=None,
                          counts=None, dustbin=True, directions=False, projected=False):
        """The ground truth of homography pairs in one native call (linetr_gt_assign): what the reference's dataset builder computes
        per pair with find_line_matches / calculate_line_overlaps in both directions (dataloaders/build_homography_dataset.py:210-237,
        dataloaders/utils/util_lines.py:67-171).

        lines0 [B, n0, 2, 2] / lines1 [B, n1, 2, 2] (or [n, 2, 2] for one pair; then H is [3, 3]): the sub-lines' end points, torch or
        NumPy.  float32 on both sides computes as the reference does; float64 on either side selects the float64 instance.  H [B, 3, 3]
        takes image-0 pixels to image-1 pixels; its inverse is np.linalg.inv(H), as in the builder.  `counts` = (count0 [B], count1 [B]):
        the valid prefix of each item.  max_matches (M) defaults to the builder's int(max_sublines * 1.5) with max_sublines = n0; an item
        with more pairs than that makes the call run once more with room for all of them (0: no list, `found` only).  Returns a dict of device tensors:
        assign [B, n0 + 1, n1 + 1] float32 (`dustbin`; what val_step(assign=...) takes) or [B, n0, n1], lmatches [B, M, 2] int32 with -1
        behind each list, found [B] int32; with `directions` match_dir [B, 2, n0, n1] uint8 and overlap_dir [B, 2, n0, n1] (direction 1
        as [i][j]); with `projected` proj0 / proj1.  One host wait (the list sizes)."""
        def arr(x):
            return x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        l0, l1 = arr(lines0), arr(lines1)
        Hm = np.asarray(H.detach().cpu() if isinstance(H, torch.Tensor) else H, dtype=np.float64)
        if l0.dim() == 3 and l1.dim() == 3 and Hm.shape == (3, 3):
            l0, l1, Hm = l0[None], l1[None], Hm[None]
        if l0.dim() != 4 or l1.dim() != 4 or tuple(l0.shape[2:]) != (2, 2) or tuple(l1.shape[2:]) != (2, 2) or l0.shape[0] != l1.shape[0]:
            raise ValueError(f"line_ground_truth: lines must be [B, n, 2, 2], got {tuple(l0.shape)} and {tuple(l1.shape)}")
        B, n0, n1 = int(l0.shape[0]), int(l0.shape[1]), int(l1.shape[1])
        if Hm.shape != (B, 3, 3):
            raise ValueError(f"line_ground_truth: H must be [{B}, 3, 3], got {Hm.shape}")
        dt = torch.float64 if torch.float64 in (l0.dtype, l1.dtype) else torch.float32
        l0, l1 = (t.to(device=self.device, dtype=dt).contiguous() for t in (l0, l1))
        Hd = torch.from_numpy(np.stack([Hm, np.linalg.inv(Hm)], axis=1).reshape(B, 2, 9)).to(self.device)
        c0 = c1 = None
        if counts is not None:
            c0, c1 = (arr(c).to(device=self.device, dtype=torch.int32).contiguous() for c in counts)
            if tuple(c0.shape) != (B,) or tuple(c1.shape) != (B,):
                raise ValueError("line_ground_truth: counts must be two arrays of B entries")
        M = int(n0 * 1.5) if max_matches is None else int(max_matches)
        pad = int(bool(dustbin))
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):     # a heads-only engine has no handle: the current device is used
            assign = new((B, n0 + pad, n1 + pad), torch.float32)
            found = new((B,), torch.int32)
            mdir = new((B, 2, n0, n1), torch.uint8) if directions else None
            odir = new((B, 2, n0, n1), dt) if directions else None
            p0, p1 = (new((B, n0, 2, 2), dt), new((B, n1, 2, 2), dt)) if projected else (None, None)
            ws = self._workspace("gt_assign", int(self._L.linetr_gt_assign_workspace_bytes(B, n0, n1)))
            while True:
                lm = new((B, M, 2), torch.int32)
                self._call("linetr_gt_assign", int(dt == torch.float64), l0.data_ptr(), n0, l1.data_ptr(), n1, Hd.data_ptr(), B, ptr(c0), ptr(c1),
                           float(thres_reprojected), float(thres_angdiff), float(min_overlap_ratio), pad, assign.data_ptr(), lm.data_ptr(), M,
                           found.data_ptr(), ptr(mdir), ptr(odir), ptr(p0), ptr(p1), ws.data_ptr(), ws.numel())
                most = int(found.max())
                if most <= M or M == 0:          # (max_matches = 0: no list is wanted, `found` alone)
                    break
                M = most                         # once more with room for every pair
        out = {"assign": assign, "lmatches": lm, "found": found}
        if directions:
            out["match_dir"], out["overlap_dir"] = mdir, odir
        if projected:
            out["proj0"], out["proj1"] = p0, p1
        return out
