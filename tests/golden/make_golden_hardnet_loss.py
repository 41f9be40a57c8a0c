#!/usr/bin/env python3
"""Generate tests/golden/hardnet_loss.npz: the REAL reference's descriptor_loss (evaluations/criteria.py) with its HardNet mining
switched on -- `crit.compute_distances = crit.compute_distances_hardnet` on the instance, which is forward's commented line
(:175-176) flipped -- and its gradient with respect to line_desc0 / line_desc1 by torch autograd.

Run in the build container only (needs /root/reference), on the CPU:

    python tests/golden/make_golden_hardnet_loss.py

Same harness as make_golden_loss_grad.py (cv2 stub; the reference's packages first on the path).  Only data is written: the inputs
(desc0, desc1 [3,256,40], assign [3,41,41]: unit vectors, matched copies at noise 1/16, second positives on some rows and columns, some
0.2 overlaps, rows without a match), loss / hp / hn / V and pos / neg per anchor from the reference run in float64, grad0_f64 /
grad1_f64, ref_f32_err = the largest difference between the reference's own float32 gradients and those, and ref_f32_val_err = the
same for its pos / neg -- the yardsticks of tests/test_gpu_hardnet_loss.py."""
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

B, N, SEED = 3, 40, 5


def inputs():
    rs = np.random.RandomState(SEED)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    desc0, desc1 = np.zeros((B, N, 256)), np.zeros((B, N, 256))
    assign = np.zeros((B, N + 1, N + 1), np.float32)
    for b in range(B):
        desc0[b] = unit(rs.standard_normal((N, 256)))
        perm = rs.permutation(N)
        desc1[b, perm] = unit(desc0[b] + rs.standard_normal((N, 256)) / 16.0)
        kind = rs.randint(0, 10, N)                       # 0: no match at all, 1: overlap 0.2, else a match
        for a in range(N):
            if kind[a] == 1:
                assign[b, a, perm[a]] = 0.2
            elif kind[a] >= 2:
                assign[b, a, perm[a]] = 1.0
                if a % 5 == 0:                            # a second positive on this row and on the column of the next row's copy
                    assign[b, a, perm[(a + 1) % N]] = 1.0
    to = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1).astype(np.float32))
    return to(desc0), to(desc1), assign


def reference_run(desc0, desc1, assign, dtype):
    d0 = torch.tensor(desc0, dtype=dtype, requires_grad=True)
    d1 = torch.tensor(desc1, dtype=dtype, requires_grad=True)
    crit = descriptor_loss()
    crit.compute_distances = crit.compute_distances_hardnet
    pred, target = {"line_desc0": d0, "line_desc1": d1}, {"mat_assign_sublines": torch.tensor(assign, dtype=dtype)}
    with torch.no_grad():
        pos, neg = crit.compute_distances_hardnet(pred, target)
    loss, hp, hn = crit(pred, target)
    loss.backward()
    return {"loss": loss.item(), "hp": hp.item(), "hn": hn.item(), "pos": pos.double().numpy(), "neg": neg.double().numpy(),
            "grad0": d0.grad.double().numpy(), "grad1": d1.grad.double().numpy()}


def main():
    # torch.max(dim) on the CPU returns the FIRST index of equal maxima: the rule the native selection and the closed form follow
    tie = torch.tensor([[0.0, 0.5, 0.25, 0.5], [0.75, 0.0, 0.75, 0.75]], dtype=torch.float64)
    assert torch.max(tie, dim=1).indices.tolist() == [1, 0], "torch.max(dim) no longer returns the first of equal maxima"
    assert torch.max(tie.float(), dim=1).indices.tolist() == [1, 0]
    desc0, desc1, assign = inputs()
    g = assign[:, :-1, :-1]
    assert ((g > 0.3).sum(axis=2) > 1).any() and ((g > 0.3).sum(axis=1) > 1).any()          # second positives on rows and on columns
    assert (g == np.float32(0.2)).any() and (~(g > 0.3).any(axis=2)).any()                  # 0.2 overlaps, rows without a match
    r64, r32 = reference_run(desc0, desc1, assign, torch.float64), reference_run(desc0, desc1, assign, torch.float32)
    V = len(r64["pos"])
    live = int((r64["pos"] - r64["neg"] + 1 > 0).sum())
    assert V == len(r32["pos"]) and 0 < live < V                                            # a mix of live and dead anchors
    err = max(np.abs(r32["grad0"] - r64["grad0"]).max(), np.abs(r32["grad1"] - r64["grad1"]).max())
    val_err = max(np.abs(r32["pos"] - r64["pos"]).max(), np.abs(r32["neg"] - r64["neg"]).max())
    path = os.path.join(HERE, "hardnet_loss.npz")
    np.savez_compressed(path, desc0=desc0, desc1=desc1, assign=assign, loss=np.float64(r64["loss"]), hp=np.float64(r64["hp"]),
                        hn=np.float64(r64["hn"]), V=np.int64(V), live=np.int64(live), pos=r64["pos"], neg=r64["neg"],
                        grad0_f64=r64["grad0"], grad1_f64=r64["grad1"], ref_f32_err=np.float64(err), ref_f32_val_err=np.float64(val_err))
    print(f"V = {V}, live = {live}, loss {r64['loss']:.6f}, max |grad| {max(np.abs(r64['grad0']).max(), np.abs(r64['grad1']).max()):.3e}, "
          f"ref_f32_err {err:.2e}, ref_f32_val_err {val_err:.2e}, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
