#!/usr/bin/env python3
"""Generate tests/golden/val_step.npz by running the REAL reference's descriptor_loss, nn_matcher_batches and Evaluate_PR
(evaluations/criteria.py, matcher.py, evaluate_pr.py) on seeded clustered descriptors (tests/val_step_reference.py:clustered_case).

Run in the build container only (needs /root/reference), on the CPU:

    python tests/golden/make_golden_val_step.py

Same harness as make_golden.py (cv2 stub; the reference's packages first on the path).  Only data is written.  Before saving it
asserts that the case is worth freezing -- enough surviving anchors, some dropped ones, and every compare a selection depends on at
least 1e-5 (about 40 float32 spacings) away from flipping in float64 -- and moves on to the next seed otherwise."""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))           # val_step_reference
sys.path.insert(0, "/root/reference")   # FIRST on the path: `evaluations` must be the reference's package, not this repo's shim

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_grad_enabled(False)

import evaluations as _ref_eval  # noqa: E402
assert _ref_eval.__file__.startswith("/root/reference/"), _ref_eval.__file__
from evaluations.criteria import descriptor_loss  # noqa: E402  (reference)
from evaluations.matcher import nn_matcher_batches  # noqa: E402  (reference)
from evaluations.evaluate_pr import Evaluate_PR  # noqa: E402  (reference)

import val_step_reference as R  # noqa: E402

B, N, NN_THRESH = 3, 40, 0.7


def attempt(seed):
    desc0, desc1, assign = R.clustered_case(seed, B, N)
    crit = descriptor_loss()
    pred = {"line_desc0": torch.from_numpy(desc0), "line_desc1": torch.from_numpy(desc1)}
    target = {"mat_assign_sublines": torch.from_numpy(assign)}
    pos, neg = crit.compute_distances(pred, target)
    loss, hp, hn = crit(pred, target)
    pos, neg = pos.numpy(), neg.numpy()
    f64 = R.descriptor_loss(desc0, desc1, assign, np.float64)
    anchors = int((f64["row_pos"] > 0).sum())
    assert len(pos) >= 20, f"V = {len(pos)}"
    assert anchors - len(f64["rows"]) >= 3, f"{anchors - len(f64['rows'])} anchors dropped"
    margin = R.margins(desc0, desc1, assign, NN_THRESH)
    assert margin >= R.MIN_MARGIN, f"margin {margin:.2e}"
    assert len(f64["rows"]) == len(pos), "the float64 selection differs from the reference's"
    # position by position the float64 survivors carry the reference's values (to a few float32 spacings; the margins above are 40):
    # the stored row indices are the reference's survivors, in its order
    assert np.abs(pos - f64["pos"]).max() <= 1e-5 and np.abs(neg - f64["neg"]).max() <= 1e-5, "float64 survivors are not the reference's"
    out = {"desc0": desc0, "desc1": desc1, "assign": assign, "nn_thresh": np.float64(NN_THRESH), "seed": np.int64(seed),
           "loss": loss.numpy(), "hardest_positive": hp.numpy(), "hardest_negative": hn.numpy(),
           "dists_pos_final": pos, "dists_neg_final": neg, "anchor_rows": f64["rows"].astype(np.int64),
           "ref_err_f64": np.float64(max(np.abs(pos - f64["pos"]).max(), np.abs(neg - f64["neg"]).max())),
           "min_margin": np.float64(margin)}
    gt = assign[:, :-1, :-1]
    for mutual in (True, False):
        mat = nn_matcher_batches(desc0, desc1, NN_THRESH, is_mutual_NN=mutual)
        p, r, f = Evaluate_PR(None).get_precision_recall(mat[:, :-1, :-1], gt)
        tag = "mutual" if mutual else "oneway"
        out[f"mat_nn_{tag}"] = mat
        out[f"prf_{tag}"] = np.array([p, r, f], np.float64).T
        out[f"tfpn_{tag}"] = np.array([Evaluate_PR(None).calc_TFPN(mat[b, :-1, :-1], gt[b]) for b in range(B)], np.int32)
    return out


def main():
    for seed in range(100, 200):
        try:
            out = attempt(seed)
        except AssertionError as e:
            print(f"seed {seed}: {e}")
            continue
        path = os.path.join(HERE, "val_step.npz")
        np.savez_compressed(path, **out)
        print(f"seed {seed}: V = {len(out['dists_pos_final'])}, margin {out['min_margin']:.2e}, ref_err_f64 {out['ref_err_f64']:.2e}, "
              f"{os.path.getsize(path)} bytes -> {path}")
        return
    raise SystemExit("no seed qualified")


if __name__ == "__main__":
    main()
