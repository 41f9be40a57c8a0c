"""The reference's evaluation names on top of Engine.val_step (linetr_val_step, csrc/lt_valstep.h), Engine.loss_step
(linetr_desc_loss_grad, csrc/lt_lossgrad.h) and Engine.hardnet_step (linetr_hardnet_loss_grad, csrc/lt_hardnet.h):

    descriptor_loss      evaluations/criteria.py:35-192     differentiable with respect to line_desc0 / line_desc1: loss.backward()
                                                            reaches whatever torch graph produced them (the gradient of the
                                                            criterion is native; no gradient is taken where none is asked for);
                                                            mining="hardnet": compute_distances_hardnet (:126-171), the switch the
                                                            reference keeps as a commented line of forward (:175-176)
    nn_matcher_batches   evaluations/matcher.py:51-102
    Evaluate_PR          evaluations/evaluate_pr.py:3-35
    Result, AverageMeter evaluations/metric.py:7-112        the interface train.py and its logger use; no save_matching_image
                                                            (no cv2 here)

Loss, matcher and scores are computed on the device from one set of dot products; the descriptors must live on a HIP device
(there is no CPU path)."""
from __future__ import annotations

import numpy as np
import torch

from .engine import Engine

_engines = {}


def _engine(device) -> Engine:
    """one weight-free Engine per device (val_step needs no model)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("linetr_amd.evaluations needs descriptors on a HIP device (torch device 'cuda:N'); there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    eng = _engines.get(device)
    if eng is None:
        eng = _engines[device] = Engine.heads_only(device)
    return eng


def _on_device(desc0, desc1):
    """(desc0, desc1) as device tensors: NumPy arrays (what Result.evaluate of the reference hands the matcher) go to the current HIP device"""
    if not isinstance(desc0, torch.Tensor):
        dev = torch.device("cuda", torch.cuda.current_device())
        desc0, desc1 = torch.as_tensor(np.asarray(desc0), device=dev), torch.as_tensor(np.asarray(desc1), device=dev)
    return desc0, desc1


def _require_anchors(res, mining="semi-hard"):
    if res["count"] == 0:     # the reference stacks an empty list (criteria.py:117, :148)
        what = "no anchor has a semi-hard negative" if mining == "semi-hard" else "no line has a positive"
        raise RuntimeError(f"descriptor_loss: {what} (stack expects a non-empty TensorList)")


MININGS = ("semi-hard", "hardnet")


class _DescriptorLossGrad(torch.autograd.Function):
    """(loss, hardest_positive, hardest_negative) = criterion(desc0, desc1): forward is Engine.loss_step (mining "semi-hard") or
    Engine.hardnet_step (mining "hardnet"), which also leaves d loss / d desc for an upstream of 1; backward scales them by the gradient
    arriving at the loss (on the device: nothing is waited for).  The two hardest values are not differentiable.  The gradients live in
    the graph only: `owner.last` gets the scalars."""

    @staticmethod
    def forward(ctx, desc0, desc1, assign, owner, mining="semi-hard"):
        eng = _engine(desc0.device)
        res = eng.loss_step(desc0, desc1, assign=assign) if mining == "semi-hard" else eng.hardnet_step(desc0, desc1, assign=assign)
        owner.last = {k: res[k] for k in ("loss", "hardest_positive", "hardest_negative", "count")}
        _require_anchors(res, mining)
        ctx.save_for_backward(res["grad0"], res["grad1"])
        loss, hp, hn = (torch.tensor(res[k], dtype=torch.float32, device=desc0.device) for k in ("loss", "hardest_positive", "hardest_negative"))
        ctx.mark_non_differentiable(hp, hn)
        return loss, hp, hn

    @staticmethod
    def backward(ctx, grad_loss, _grad_hp, _grad_hn):
        grad0, grad1 = ctx.saved_tensors
        return (grad_loss * grad0 if ctx.needs_input_grad[0] else None, grad_loss * grad1 if ctx.needs_input_grad[1] else None,
                None, None, None)


class descriptor_loss(torch.nn.Module):
    """forward(pred, target) -> (loss, hardest_positive, hardest_negative): 0-dim float32 tensors on the descriptors' device.
    pred: 'line_desc0', 'line_desc1' [B, 256, n]; target: 'mat_assign_sublines' [B, n+1, n+1].
    With grad enabled and a descriptor set that requires grad, `loss` carries a grad_fn (Engine.loss_step: value and gradient from one
    selection); the two hardest values never do (the reference never differentiates them).  Otherwise nothing carries one.
    mining: "semi-hard" (the default: the reference's compute_distances) or "hardnet" (its compute_distances_hardnet, through
    Engine.hardnet_step: with a gradient under autograd, the value-only call otherwise)."""

    def __init__(self, mining="semi-hard"):
        super().__init__()
        if mining not in MININGS:
            raise ValueError(f"descriptor_loss: mining must be one of {MININGS}, got {mining!r}")
        self.margin = 0.5
        self.mining = mining

    def forward(self, pred, target):
        desc0, desc1 = pred["line_desc0"], pred["line_desc1"]
        assign = target["mat_assign_sublines"]
        if torch.is_grad_enabled() and (desc0.requires_grad or desc1.requires_grad):
            return _DescriptorLossGrad.apply(desc0, desc1, assign, self, self.mining)
        with torch.no_grad():
            if self.mining == "semi-hard":
                res = _engine(desc0.device).val_step(desc0, desc1, assign=assign)
            else:
                res = _engine(desc0.device).hardnet_step(desc0, desc1, assign=assign, need_grad=False)
            self.last = res
            _require_anchors(res, self.mining)
            return tuple(torch.tensor(res[k], dtype=torch.float32, device=desc0.device)
                         for k in ("loss", "hardest_positive", "hardest_negative"))


def _with_dustbins(match01: np.ndarray, n: int) -> np.ndarray:
    """match01 [B, n] -> the reference's float64 [B, n+1, n+1] matrix (matcher.py:92-100): 1 at every match, at (row, n) of every
    unmatched row, at (n, column) of every unmatched column, and in the corner."""
    B = match01.shape[0]
    mat = np.zeros((B, n + 1, n + 1))
    for b in range(B):
        rows = np.nonzero(match01[b] >= 0)[0]
        cols = match01[b][rows]
        mat[b, rows, cols] = 1
        mat[b, np.delete(np.arange(n + 1), rows), -1] = 1
        mat[b, -1, np.delete(np.arange(n + 1), cols)] = 1
        mat[b, -1, -1] = 1
    return mat


def nn_matcher_batches(desc0, desc1, nn_thresh, is_mutual_NN=False):
    """The float64 [B, n+1, n+1] match matrix with dustbins.  Cost: this is a whole val_step against an all-zero ground truth (the
    dot products are the bulk of it; the selection and the counts of an empty ground truth ride along and are thrown away), plus
    one [B, n] copy to the host.  A caller that also wants the loss or the scores should call Engine.val_step once instead."""
    desc0, desc1 = _on_device(desc0, desc1)
    B, _, n = desc0.shape
    eng = _engine(desc0.device)
    res = eng.val_step(desc0, desc1, assign=torch.zeros((B, n + 1, n + 1), dtype=torch.float32, device=desc0.device),
                       nn_thresh=nn_thresh, mutual=is_mutual_NN)
    return _with_dustbins(eng.to_host(res["match01"])[0], n)


class Evaluate_PR:
    """precision / recall / F1 per item from 0/1 prediction and ground-truth matrices (host side; Result.evaluate gets the same
    numbers from the device without building the matrices)"""

    def __init__(self, args=None):
        self.args = args
        self.eps = 1e-5

    def calc_TFPN(self, score, score_gt):
        """one item: score [n, n] 0/1 predictions, score_gt [n, n] ground truth (> 0) -> TP, FP, FN, TN over the rows"""
        gt = np.asarray(score_gt) > 0
        pred = np.asarray(score) > 0
        has_gt, has_pred = gt.any(axis=1), pred.any(axis=1)
        TP = int((pred & gt).any(axis=1).sum())
        TN = int((~has_gt & ~has_pred).sum())
        return TP, int((~has_gt).sum()) - TN, int(has_gt.sum()) - TP, TN

    def get_precision_recall(self, score, score_gt):
        rows = []
        for s, g in zip(score, score_gt):
            TP, FP, FN, _ = self.calc_TFPN(s, g)
            p, r = (TP / (TP + other + self.eps) * 100.0 for other in (FP, FN))
            rows.append((p, r, 2 * p * r / (p + r) if p + r else 0.0))
        return tuple(list(col) for col in zip(*rows)) if rows else ([], [], [])


class Result:
    """The scores of one batch: .precision / .recall / .f1_score hold one entry per item after evaluate()."""

    def __init__(self, mode, args):
        self.mode, self.args = mode, args
        self.nn_thresh = args.nn_thresh
        self._set([], [], [])

    def _set(self, precision, recall, f1_score, gpu_time=0, loss=0):
        self.precision, self.recall, self.f1_score = precision, recall, f1_score
        self.gpu_time, self.loss = gpu_time, loss

    def set_to_worst(self):
        self._set([], [], [])

    def set_to_worst_for_logger(self):
        self._set([0], [0], [0])

    def update(self, precision, recall, f1_score, gpu_time, loss):
        self._set([precision], [recall], [f1_score], gpu_time, loss)

    def evaluate(self, pred, batch_data, loss=0, batch_idx=0):
        """precision / recall / F1 of the batch from ONE val_step (matcher and counts on the device)"""
        desc0, desc1 = pred["line_desc0"], pred["line_desc1"]
        res = _engine(desc0.device).val_step(desc0, desc1, assign=batch_data["mat_assign_sublines"], nn_thresh=self.nn_thresh,
                                             mutual=self.args.mutual_nn)
        for name, key in (("precision", "precision"), ("recall", "recall"), ("f1_score", "f1")):
            getattr(self, name).extend(float(v) for v in res[key])
        self.loss = loss
        return pred


class AverageMeter:
    """Running per-item means over the batches of an epoch (the interface train.py uses: update(result, gpu_time, n), average(),
    reset()).  Totals live in one dict; the three scores are sums over items, time and loss are weighted by the batch size."""

    _SCORES = ("precision", "recall", "f1_score")

    def __init__(self, args):
        self.args = args
        self.reset()

    def reset(self):
        self.count = 0.0
        self._totals = dict.fromkeys(self._SCORES + ("gpu_time", "loss"), 0.0)

    def update(self, result, gpu_time, n=1):
        self.count += n
        for key in self._SCORES:
            self._totals[key] += float(np.sum(getattr(result, key)))
        self._totals["gpu_time"] += n * gpu_time
        self._totals["loss"] += n * result.loss

    def average(self):
        mean = Result("test", self.args)
        if self.count > 0:
            mean.update(*(self._totals[key] / self.count for key in self._SCORES + ("gpu_time", "loss")))
        return mean
