"""The optimizer of the reference's training iteration (train.py:82 `torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=wd)`,
:193-195 `optimizer.zero_grad(); loss.backward(); optimizer.step()`) with a native step: one launch of csrc/lt_adam.h per parameter
group updates every parameter of it, in the arithmetic of torch's single-tensor path (include/linetr_hip.h has the order).

    Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, decoupled_weight_decay=False, max_grad_norm=None)

A torch.optim.Optimizer: param groups, zero_grad, hooks and schedulers work as they do there, and state_dict() / load_state_dict() are
interchangeable with torch.optim.Adam in both directions (per parameter `step`, a float32 scalar on the CPU, `exp_avg`, `exp_avg_sq`;
the param groups carry torch's full key set).  There is no CPU path: the parameters must be contiguous float32 tensors on one HIP
device."""
from __future__ import annotations

import torch

from .evaluations import _engine

# torch's options this class does not implement: anything but these values is refused, at construction and at load
_UNSUPPORTED = {"amsgrad": False, "maximize": False, "capturable": False, "differentiable": False}


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (coupled L2 weight decay; `decoupled_weight_decay=True`: AdamW's) on the native step.

    step(closure=None): one Engine.adam_step per parameter group, no host wait.  State is created lazily per parameter, as torch creates
    it; a parameter whose .grad is None is skipped and keeps its own step count; a non-contiguous .grad is made contiguous by torch; a
    sparse one raises RuntimeError, as in torch.  After the step every updated parameter's autograd version counter has advanced, as
    after an in-place torch update (the kernel writes through raw pointers).

    max_grad_norm: clip the global L2 norm of all gradients of all groups to it, as torch.nn.utils.clip_grad_norm_ in front of the step
    would: Engine.grad_norm runs first and its device scalar min(1, max_norm / (norm + 1e-6)) multiplies every gradient on its way into
    the update.  .grad itself is NOT rewritten.  The norm of the last step stays in `last_grad_norm`, a float64 device tensor (None
    without max_grad_norm).

    ValueError, at construction and at load_state_dict: amsgrad, maximize, capturable, differentiable; a tensor lr; a parameter that is
    not a contiguous float32 tensor on the one HIP device of the others.  `foreach` and `fused` choose among torch's own
    implementations and are ignored."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, decoupled_weight_decay=False, max_grad_norm=None,
                 amsgrad=False, maximize=False, capturable=False, differentiable=False, foreach=None, fused=None):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._device = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=capturable, differentiable=differentiable, fused=None, decoupled_weight_decay=bool(decoupled_weight_decay))
        self._check_group(defaults)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------ refusals
    @staticmethod
    def _check_group(group):
        """the hyper-parameters of one group (or of the defaults)"""
        for key, value in _UNSUPPORTED.items():
            if group.get(key, value) != value:
                raise ValueError(f"linetr_amd.optim.Adam does not implement {key}={group[key]!r}")
        lr, betas = group["lr"], group["betas"]
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("linetr_amd.optim.Adam takes lr and betas as Python numbers, not tensors")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= group["eps"]:
            raise ValueError(f"Invalid epsilon value: {group['eps']}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= group["weight_decay"]:
            raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")

    def _check_params(self, params):
        for p in params:
            if (not isinstance(p, torch.Tensor) or p.device.type != "cuda" or p.dtype != torch.float32 or p.layout != torch.strided
                    or not p.is_contiguous()):
                raise ValueError("linetr_amd.optim.Adam: every parameter must be a contiguous float32 tensor on a HIP device (torch device "
                                 f"'cuda:N'; there is no CPU path), got {getattr(p, 'dtype', type(p))} on {getattr(p, 'device', None)}")
            if self._device is None:
                self._device = p.device
            elif p.device != self._device:
                raise ValueError(f"linetr_amd.optim.Adam: parameters on {self._device} and {p.device} (one device per optimizer)")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            self._check_params(group["params"])
        except ValueError:
            self.param_groups.pop()
            raise

    def load_state_dict(self, state_dict):
        for group in state_dict["param_groups"]:
            self._check_group({**self.defaults, **group})
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for key, value in self.defaults.items():          # (a state_dict of an older torch may lack the younger keys)
                group.setdefault(key, value)
        for p, state in self.state.items():
            if not state:
                continue
            step = state["step"]
            state["step"] = (step.detach() if isinstance(step, torch.Tensor) else torch.tensor(float(step))).to(device="cpu", dtype=torch.float32)
            for key in ("exp_avg", "exp_avg_sq"):
                state[key] = state[key].to(device=p.device, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, steps = [], [], [], [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.zeros((), dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                params.append(p)
                grads.append(g if g.is_contiguous() else g.contiguous())
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                steps.append(state["step"])
            if params:
                work.append((group, params, grads, exp_avgs, exp_avg_sqs, steps))
        if not work:
            return loss
        eng = _engine(self._device)
        scale = None
        if self.max_grad_norm is not None:
            self.last_grad_norm, scale = eng.grad_norm([g for w in work for g in w[2]], self.max_grad_norm)
        for group, params, grads, exp_avgs, exp_avg_sqs, steps in work:
            self._check_group(group)                          # (a scheduler or the caller may have written into the group)
            # the counts after this step, in float32 as torch counts them (one stack, one add: the steps are 0-d CPU tensors)
            eng.adam_step(params, grads, exp_avgs, exp_avg_sqs, (torch.stack(steps) + 1).tolist(), lr=group["lr"], betas=group["betas"],
                          eps=group["eps"], weight_decay=group["weight_decay"], decoupled=group["decoupled_weight_decay"], grad_scale=scale)
            torch._foreach_add_(steps, 1)
            torch.autograd.graph.increment_version(params)
        return loss
