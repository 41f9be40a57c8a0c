#!/usr/bin/env python3
"""Generate tests/golden/gt_assign.npz by running the REAL reference's find_line_matches and calculate_line_overlaps
(dataloaders/utils/util_lines.py:67-171) the way its dataset builder does (dataloaders/build_homography_dataset.py:222-234) on
the seeded homography case of tests/gt_assign_reference.py, once on float32 arrays (the reference as executed: its sub-lines are
float32 tensors) and once on float64 arrays.

Run in the build container only (needs /root/reference), on the CPU:

    python tests/golden/make_golden_gt_assign.py

Same harness as make_golden_val_step.py (cv2 stub; the reference's packages first on the path).  cv2 itself is not installed, so the
projected lines come from the restatement's `project` (the builder's lines 214-218 are the one step this fixture does not pin).
The builder evaluates calc_overlap only where both directions matched, which its "lines apart" branch (ratio 0) cannot reach except by
a rounding accident; so calculate_line_overlaps also runs, as a caller of the function alone would run it, on the list EXTRA of one
further pair per row, most of them lines far apart.
Only data is written.  Before saving it asserts that the case is worth freezing -- every overlap branch hit, an asymmetric match, an
assignment in (0, 0.3], no angle compare inside the band, the restatement equal to the reference's output bit for bit -- and
moves on to the next seed otherwise.  (The last one does fail for some seeds: the reference squares float32 SCALARS with `** 2`,
which NumPy hands to libm's powf; where x * x is an exact tie between two float32 values powf may round the other way.)"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))     # workloads
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))           # gt_assign_reference
sys.path.insert(0, "/root/reference")   # FIRST on the path: `dataloaders` must be the reference's package

import numpy as np  # noqa: E402

import dataloaders.utils.util_lines as _ref_lines  # noqa: E402
assert _ref_lines.__file__.startswith("/root/reference/"), _ref_lines.__file__
from dataloaders.utils.util_lines import find_line_matches, calculate_line_overlaps  # noqa: E402  (reference)

import gt_assign_reference as R  # noqa: E402

B, N0, N1 = 3, 48, 40
TAGS = {np.float32: "f32", np.float64: "f64"}
EXTRA = np.array([(i, (7 * i + 3) % N1) for i in range(N0)])


def builder(klns0, klns1, klns0_projected, klns1_projected):
    """build_homography_dataset.py:222-234, as written"""
    mat_matches0 = find_line_matches(klns0, klns1_projected, R.THRES_REPROJECTED, R.THRES_ANGDIFF)
    mat_matches1 = find_line_matches(klns1, klns0_projected, R.THRES_REPROJECTED, R.THRES_ANGDIFF)
    mat_matches1 = mat_matches1.T
    b_matches = (np.logical_and(mat_matches0 > 0, mat_matches1 > 0))

    lmatches0 = np.array(np.where(b_matches)).T
    lmatches1 = np.zeros_like(lmatches0)
    lmatches1[:, 0], lmatches1[:, 1] = lmatches0[:, 1], lmatches0[:, 0]
    mat_overlap0, overlaps0 = calculate_line_overlaps(klns0, klns1_projected, lmatches0)
    mat_overlap1, overlaps1 = calculate_line_overlaps(klns1, klns0_projected, lmatches1)
    mat_overlap1 = mat_overlap1.T
    mat_assign_sublines = np.where(mat_overlap0 > mat_overlap1, mat_overlap0, mat_overlap1)
    lmatches = np.array(np.where(mat_assign_sublines > R.MIN_OVERLAP)).T
    return mat_matches0, mat_matches1, mat_overlap0, mat_overlap1, mat_assign_sublines, lmatches


def branches(ref, oth, pairs):
    """which of calc_overlap's branches the matched pairs take (float64 geometry is enough to classify)"""
    hit = set()
    for i, j in pairs:
        l0, l1 = ref[i].astype(np.float64), oth[j].astype(np.float64)
        d = lambda p, q: float(np.hypot(*(q - p)))
        len0, len1 = d(l0[0], l0[1]), d(l1[0], l1[1])
        sp = d(l0[0], l1[0]) < len0 and d(l0[1], l1[0]) < len0
        ep = d(l0[0], l1[1]) < len0 and d(l0[1], l1[1]) < len0
        far = max(d(l0[0], l1[0]), d(l0[1], l1[0]), d(l0[0], l1[1]), d(l0[1], l1[1])) > len0 + len1
        hit.add("both" if sp and ep else "sp" if sp else "ep" if ep else "apart" if far else "touching")
    return hit


def attempt(seed):
    out = {"seed": np.int64(seed)}
    for dtype, tag in TAGS.items():
        lines0, lines1, H = R.case(seed, B, N0, N1, dtype)
        keep = {k: [] for k in ("proj0", "proj1", "match0", "match1", "overlap0", "overlap1", "assign")}
        lms, hit, extra0, extra1 = [], set(), [], []
        asym = low = mid = one = 0
        for b in range(B):
            proj0, proj1 = R.project(lines0[b], H[b]), R.project(lines1[b], np.linalg.inv(H[b]))
            m0, m1, ov0, ov1, assign, lm = builder(lines0[b], lines1[b], proj0, proj1)
            mine = R.ground_truth(lines0[b], lines1[b], H[b])
            assert mine["margin"] >= R.BAND[dtype], f"{tag}: an angle compare {mine['margin']:.2e} degrees from flipping"
            both = (m0 > 0) & (m1 > 0)
            assert np.array_equal(mine["match0"], m0 > 0) and np.array_equal(mine["match1"], m1 > 0), f"{tag}: matches differ"
            assert np.array_equal(np.where(both, mine["overlap0"], 0).astype(np.float64), ov0), f"{tag}: overlap0 differs"
            assert np.array_equal(np.where(both, mine["overlap1"], 0).astype(np.float64), ov1), f"{tag}: overlap1 differs"
            assert np.array_equal(mine["assign"].astype(np.float64), assign), f"{tag}: assign differs"
            assert np.array_equal(mine["lmatches"], lm), f"{tag}: lmatches differ"
            _, ex0 = calculate_line_overlaps(lines0[b], proj1, EXTRA)
            _, ex1 = calculate_line_overlaps(lines1[b], proj0, EXTRA[:, ::-1])
            assert np.array_equal(mine["overlap0"][EXTRA[:, 0], EXTRA[:, 1]].astype(np.float64), ex0), f"{tag}: extra overlap0 differs"
            assert np.array_equal(mine["overlap1"][EXTRA[:, 0], EXTRA[:, 1]].astype(np.float64), ex1), f"{tag}: extra overlap1 differs"
            extra0.append(ex0); extra1.append(ex1)
            pairs = np.concatenate([np.array(np.where(both)).T, EXTRA])
            hit |= branches(lines0[b], proj1, pairs) | branches(lines1[b], proj0, pairs[:, ::-1])
            asym += int(((m0 > 0) != (m1 > 0)).sum())
            low += int(((assign > 0) & (assign <= R.MIN_OVERLAP)).sum())
            mid += int(((assign > R.MIN_OVERLAP) & (assign < 1)).sum())
            one += int((assign == 1).sum())
            for k, v in zip(keep, (proj0, proj1, m0, m1, ov0, ov1, assign)):
                keep[k].append(v)
            lms.append(lm)
        assert hit == {"both", "sp", "ep", "apart", "touching"}, f"{tag}: overlap branches hit: {sorted(hit)}"
        assert asym >= 1 and low >= 1 and mid >= 1 and one >= 1, f"{tag}: asymmetric {asym}, (0, 0.3] {low}, (0.3, 1) {mid}, 1: {one}"
        out[f"lines0_{tag}"], out[f"lines1_{tag}"], out["H"] = lines0, lines1, H
        for k, v in keep.items():
            out[f"{k}_{tag}"] = np.stack(v)
        out["extra_pairs"], out[f"extra_overlap0_{tag}"], out[f"extra_overlap1_{tag}"] = EXTRA, np.stack(extra0), np.stack(extra1)
        M = int(N0 * 1.5)
        assert max(len(lm) for lm in lms) <= M
        out[f"lmatches_{tag}"] = R.padded_list(lms, M).astype(np.float64)      # (the builder's lmatches_ret is a float64 array)
        out[f"found_{tag}"] = np.array([len(lm) for lm in lms], np.int32)
        print(f"seed {seed} {tag}: asymmetric {asym}, assign = 1: {one}, (0.3, 1): {mid}, (0, 0.3]: {low}, found {out[f'found_{tag}'].tolist()}")
    differ = int((out["assign_f32"].astype(np.float32) != out["assign_f64"].astype(np.float32)).sum())
    print(f"seed {seed}: {differ} entries of assign differ between the dtypes after rounding to float32")
    return out


def main():
    for seed in range(11, 111):
        try:
            out = attempt(seed)
        except AssertionError as e:
            print(f"seed {seed}: {e}")
            continue
        path = os.path.join(HERE, "gt_assign.npz")
        np.savez_compressed(path, **out)
        print(f"seed {seed}: {os.path.getsize(path)} bytes -> {path}")
        return
    raise SystemExit("no seed qualified")


if __name__ == "__main__":
    main()
