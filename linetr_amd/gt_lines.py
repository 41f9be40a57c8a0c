"""find_line_matches / calculate_line_overlaps of the reference's dataloaders/utils/util_lines.py (:67-171) with its signatures and
return types, computed by the native ground-truth kernel (linetr_gt_assign, csrc/lt_gtassign.h) instead of two Python loops over
every pair of lines; line_ground_truth is the fused step of its dataset builder (dataloaders/build_homography_dataset.py:210-237).

There is no CPU path: a HIP device is required, like everywhere else in this package.  (No top-level `dataloaders` package is
shipped: it would shadow the reference's own when the library is dropped into its checkout -- import these names from here.)"""
from __future__ import annotations

import numpy as np

_engine = None


def _eng():
    global _engine
    if _engine is None:
        from .engine import Engine
        _engine = Engine.heads_only("cuda")
    return _engine


def _one_direction(lines0, lines1, thres_reprojected=3, thres_angdiff=2):
    """direction 0 of the native call for reference lines `lines0` and ALREADY projected `lines1` (identity homography: a point
    passes through the projection unchanged), as NumPy arrays: (match [n0, n1] uint8, overlap [n0, n1])"""
    l0, l1 = np.asarray(lines0), np.asarray(lines1)
    if l0.dtype != np.float32 or l1.dtype != np.float32:           # anything but the reference's float32: float64 geometry
        l0, l1 = l0.astype(np.float64), l1.astype(np.float64)
    res = _eng().line_ground_truth(l0.reshape(-1, 2, 2), l1.reshape(-1, 2, 2), np.eye(3), thres_reprojected=thres_reprojected,
                                   thres_angdiff=thres_angdiff, max_matches=0, dustbin=False, directions=True)
    return res["match_dir"][0, 0].cpu().numpy(), res["overlap_dir"][0, 0].cpu().numpy()


def find_line_matches(lines0, lines1, thres_reprojected, thres_angdiff):
    """util_lines.py:67-114: mat_line_match [n0, n1] float64, 1 where lines1[i1] (already projected into lines0's frame) matches
    the reference line lines0[i0]."""
    if len(lines0) == 0 or len(lines1) == 0:
        return np.zeros((len(lines0), len(lines1)))
    return _one_direction(lines0, lines1, thres_reprojected, thres_angdiff)[0].astype(np.float64)


def calculate_line_overlaps(lines0, lines1, matches_sublines):
    """util_lines.py:116-171: (mat_overlap [n0, n1] float64 holding the overlap ratio at the listed pairs and 0 elsewhere, overlaps
    [len(matches_sublines)] float64) -- a gather of the dense matrix the kernel computes."""
    pairs = np.asarray(matches_sublines, dtype=np.int64).reshape(-1, 2)
    mat_overlap = np.zeros((len(lines0), len(lines1)))
    if len(pairs) == 0:
        return mat_overlap, np.zeros(0)
    overlaps = _one_direction(lines0, lines1)[1][pairs[:, 0], pairs[:, 1]].astype(np.float64)
    mat_overlap[pairs[:, 0], pairs[:, 1]] = overlaps
    return mat_overlap, overlaps


def line_ground_truth(lines0, lines1, H, **kw):
    """The builder's lines 210-237 for a batch of pairs in one call: Engine.line_ground_truth on a weight-free engine."""
    return _eng().line_ground_truth(lines0, lines1, H, **kw)
