#!/usr/bin/env python3
"""Generate tests/golden/loss_grad.npz: the gradient of the REAL reference's descriptor_loss (evaluations/criteria.py) with respect
to line_desc0 / line_desc1, by torch autograd, on the inputs already frozen in tests/golden/val_step.npz.

Run in the build container only (needs /root/reference), on the CPU, after make_golden_val_step.py:

    python tests/golden/make_golden_loss_grad.py

Same harness as make_golden_val_step.py (cv2 stub; the reference's packages first on the path).  Only data is written:
grad0_f64 / grad1_f64 [3,256,40] from the reference run in float64, V, and ref_f32_err = the largest difference between the
reference's own float32 gradients and those -- the yardstick of tests/test_gpu_loss_grad.py."""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")   # FIRST on the path: `evaluations` must be the reference's package, not this repo's shim

import numpy as np  # noqa: E402
import torch  # noqa: E402

import evaluations as _ref_eval  # noqa: E402
assert _ref_eval.__file__.startswith("/root/reference/"), _ref_eval.__file__
from evaluations.criteria import descriptor_loss  # noqa: E402  (reference)


def reference_grads(fix, dtype):
    desc0 = torch.tensor(fix["desc0"], dtype=dtype, requires_grad=True)
    desc1 = torch.tensor(fix["desc1"], dtype=dtype, requires_grad=True)
    crit = descriptor_loss()
    pred, target = {"line_desc0": desc0, "line_desc1": desc1}, {"mat_assign_sublines": torch.tensor(fix["assign"], dtype=dtype)}
    with torch.no_grad():
        V = len(crit.compute_distances(pred, target)[0])
    loss, hp, hn = crit(pred, target)
    loss.backward()
    return desc0.grad.double().numpy(), desc1.grad.double().numpy(), V


def main():
    fix = np.load(os.path.join(HERE, "val_step.npz"))
    g0, g1, V = reference_grads(fix, torch.float64)
    h0, h1, V32 = reference_grads(fix, torch.float32)
    assert V == V32 == len(fix["anchor_rows"])
    err = max(np.abs(h0 - g0).max(), np.abs(h1 - g1).max())
    path = os.path.join(HERE, "loss_grad.npz")
    np.savez_compressed(path, grad0_f64=g0, grad1_f64=g1, V=np.int64(V), ref_f32_err=np.float64(err))
    print(f"V = {V}, max |grad| {max(np.abs(g0).max(), np.abs(g1).max()):.3e}, "
          f"ref_f32_err {err:.2e}, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
