"""NumPy restatement of the ground-truth line assignment of a homography pair (the reference's dataset builder,
dataloaders/build_homography_dataset.py:210-237, with find_line_matches / calculate_line_overlaps of
dataloaders/utils/util_lines.py:67-171), vectorised over every pair of lines, in float32 or float64, and the seeded case the
fixture (tests/golden/gt_assign.npz) and the GPU tests are built from.  Test infrastructure only.

Every scalar operation is the reference's, in its order and in the arrays' dtype (the reference's `sublines` are float32 tensors, so
NumPy computes every scalar in float32): `x * x` stands for `x ** 2`, divide and square root are correctly rounded, thresholds that
are Python numbers take the dtype of the value they are compared with.  tests/test_gt_assign_fixture_cpu.py pins this file to the
reference's output bit for bit.

The one step that is NOT the reference's code is the projection: cv2.perspectiveTransform is restated from its documented
arithmetic (double accumulation, w = x m6 + y m7 + m8, w = w != 0 ? 1 / w : 0, X = (x m0 + y m1 + m2) w, cast to the input type)."""
import math

import numpy as np

from workloads import synth

THRES_REPROJECTED, THRES_ANGDIFF, MIN_OVERLAP = 3, 2, 0.3
# An entry may differ between two correct implementations only where atan2 decides: the angle difference within this many degrees of
# the threshold, or of the wrap of `% 180` (the same compare seen from the other side).  A few ulp of a ~3 rad atan2 result in
# degrees (float32: 180 * 2^-23 = 2e-5; float64: 4e-14), times a safety factor of about 30.
BAND = {np.float32: 1e-3, np.float64: 1e-9}
# the (n0, n1) shapes of tests/test_gpu_gt_assign.py::test_edges (tile edges of the 64-column ballot words and the 16-row blocks, one
# shape with several words per row) and their seeds, chosen on the CPU by the band premise alone (test_band_premise)
EDGE_CASES = {(1, 1): 3, (1, 65): 3, (63, 64): 3, (64, 64): 3, (65, 63): 3, (129, 250): 3}
EDGE_B = 3


def project(lines, m):
    """[..., 2] points of dtype T through the 3x3 float64 matrix `m`, as cv2.perspectiveTransform orders it."""
    m = np.asarray(m, np.float64).reshape(9)
    x, y = lines[..., 0].astype(np.float64), lines[..., 1].astype(np.float64)
    w = x * m[6] + y * m[7] + m[8]
    with np.errstate(divide="ignore"):
        w = np.where(w != 0, 1.0 / w, 0.0)
    out = np.stack([(x * m[0] + y * m[1] + m[2]) * w, (x * m[3] + y * m[4] + m[5]) * w], axis=-1)
    return out.astype(lines.dtype)


def line_angles(lines):
    """util_lines.py:84-85 for every line [n, 2, 2]: degrees(arctan2(dx, dy))"""
    return np.degrees(np.arctan2(lines[:, 1, 0] - lines[:, 0, 0], lines[:, 1, 1] - lines[:, 0, 1]))


def _pp(p, q):
    """calc_distance_point_point(p, q) (util_lines.py:15-21)"""
    dx, dy = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1]
    return np.sqrt(dx * dx + dy * dy)


def _pl(pt, ln):
    """calc_distance_point_line(pt, ln) (util_lines.py:5-13)"""
    x0, y0 = pt[..., 0], pt[..., 1]
    x1, y1, x2, y2 = ln[..., 0, 0], ln[..., 0, 1], ln[..., 1, 0], ln[..., 1, 1]
    a, b = y2 - y1, x2 - x1
    return np.abs(a * x0 - b * y0 + x2 * y1 - y2 * x1) / np.sqrt(a * a + b * b)


def direction(ref, oth, thres_reprojected=THRES_REPROJECTED, thres_angdiff=THRES_ANGDIFF):
    """find_line_matches(ref, oth, ..) and calc_overlap(ref[i], oth[j]) for EVERY pair.  ref [n, 2, 2], oth [m, 2, 2], one dtype.
    Returns (match [n, m] bool, overlap [n, m] dtype, margin [n, m] float64): margin = how far the pair's angle compare is from
    flipping, in degrees (inf where the pair never reaches the compare)."""
    T = ref.dtype.type
    r, o = ref[:, None], oth[None, :]
    with np.errstate(all="ignore"):
        d0, d1 = _pl(o[:, :, 0], r), _pl(o[:, :, 1], r)
        far = (d0 > T(thres_reprojected)) & (d1 > T(thres_reprojected))
        diff = np.abs(line_angles(oth)[None, :] - line_angles(ref)[:, None])
        ang = diff % T(180)
        len0, len1 = _pp(r[:, :, 0], r[:, :, 1]), _pp(o[:, :, 0], o[:, :, 1])
        s0s1, e0s1 = _pp(r[:, :, 0], o[:, :, 0]), _pp(r[:, :, 1], o[:, :, 0])
        s0e1, e0e1 = _pp(r[:, :, 0], o[:, :, 1]), _pp(r[:, :, 1], o[:, :, 1])
        sp_on = (s0s1 < len0) & (e0s1 < len0)
        ep_on = (s0e1 < len0) & (e0e1 < len0)
        dmax = np.maximum(np.maximum(s0s1, e0s1), np.maximum(s0e1, e0e1))
        lsum = len0 + len1
        apart = ~sp_on & ~ep_on & (dmax > lsum)
        match = ~far & ~(ang > T(thres_angdiff)) & ~apart
        ov = np.where(sp_on & ep_on, len1 / len0,
                      np.where(sp_on, np.where(s0e1 > e0e1, e0s1 / len0, s0s1 / len0),
                               np.where(ep_on, np.where(s0s1 > e0s1, e0e1 / len0, s0e1 / len0),
                                        np.where(dmax <= lsum, T(1), T(0)))))
        d64 = diff.astype(np.float64)
        margin = np.minimum(np.abs(ang.astype(np.float64) - thres_angdiff), np.minimum(np.abs(d64 - 180), np.abs(d64 - 360)))
    return match, ov.astype(ref.dtype), np.where(far | np.isnan(margin), np.inf, margin)


def ground_truth(lines0, lines1, H, thres_reprojected=THRES_REPROJECTED, thres_angdiff=THRES_ANGDIFF, min_overlap=MIN_OVERLAP,
                 count0=None, count1=None):
    """One item.  lines0 [n0, 2, 2], lines1 [n1, 2, 2] of one dtype, H [3, 3] float64 (image 0 -> image 1).  Everything is indexed
    [i][j] (direction 1 transposed); rows >= count0 and columns >= count1 hold 0 / no match."""
    n0, n1 = len(lines0), len(lines1)
    proj0, proj1 = project(lines0, H), project(lines1, np.linalg.inv(H))
    m0, ov0, g0 = direction(lines0, proj1, thres_reprojected, thres_angdiff)
    m1, ov1, g1 = (a.T for a in direction(lines1, proj0, thres_reprojected, thres_angdiff))
    valid = (np.arange(n0)[:, None] < (n0 if count0 is None else count0)) & (np.arange(n1)[None, :] < (n1 if count1 is None else count1))
    m0, m1 = m0 & valid, m1 & valid
    ov0, ov1 = np.where(valid, ov0, 0).astype(lines0.dtype), np.where(valid, ov1, 0).astype(lines0.dtype)
    assign = np.where(m0 & m1, np.where(ov0 > ov1, ov0, ov1), 0).astype(lines0.dtype)
    lm = np.array(np.where(assign.astype(np.float64) > min_overlap)).T          # (the reference's matrix is float64)
    return {"proj0": proj0, "proj1": proj1, "match0": m0, "match1": m1, "overlap0": ov0, "overlap1": ov1, "assign": assign,
            "lmatches": lm.astype(np.int32).reshape(-1, 2), "margin": float(np.where(valid, np.minimum(g0, g1), np.inf).min())}


def batch_truth(lines0, lines1, H, counts=None, **kw):
    """ground_truth per item of [B, n, 2, 2] batches, stacked (lmatches: a list)."""
    items = [ground_truth(lines0[b], lines1[b], H[b], count0=None if counts is None else counts[0][b],
                          count1=None if counts is None else counts[1][b], **kw) for b in range(len(lines0))]
    out = {k: np.stack([it[k] for it in items]) for k in items[0] if k not in ("lmatches", "margin")}
    out["lmatches"] = [it["lmatches"] for it in items]
    out["margin"] = min(it["margin"] for it in items)
    return out


def padded_list(lmatches, M):
    """[B][M][2] int32: every item's list cut at M, -1 behind it (build_homography_dataset.py:236-237)"""
    out = np.full((len(lmatches), M, 2), -1, np.int32)
    for b, lm in enumerate(lmatches):
        out[b, :min(len(lm), M)] = lm[:M]
    return out


def _egcd(a, b):
    if b == 0:
        return (1, 0) if a >= 0 else (-1, 0)
    x, y = _egcd(b, a % b)
    return y, x - (a // b) * y


def zero_w_point(H):
    """H with m6, m7 moved to multiples of 2^-24 (with coprime numerators; m8 = 1) and an integer point (x, y), exact in float32,
    for which x m6 + y m7 + m8 is EXACTLY 0 in double arithmetic: every product and sum is an integer times 2^-24."""
    H = np.array(H, np.float64) / H[2, 2]
    a, b, c = int(round(H[2, 0] * 2 ** 24)), int(round(H[2, 1] * 2 ** 24)), 2 ** 24
    a += a == 0
    while math.gcd(a, b) != 1:
        b += 1
    x, y = (v * -c for v in _egcd(a, b))
    k = round(x / b) if b else 0              # the solution with the smallest |x|
    x, y = x - k * b, y + k * a
    assert a * x + b * y == -c and max(abs(x), abs(y)) <= 2 ** 24
    H[2, 0], H[2, 1] = a / 2 ** 24, b / 2 ** 24
    assert float(x) * H[2, 0] + float(y) * H[2, 1] + H[2, 2] == 0.0
    return H, (float(x), float(y))


ZERO_LENGTH_COL, ZERO_W_ROW = 7, 5


def case(seed, B, n0, n1, dtype):
    """B items from synth.homography_pair(seed + b, max(n0, n1), strength=0.3), the first n0 / n1 sub-lines of each side.  Image-1
    line j is perturbed by j % 6:
      0 untouched | 1 shifted 0-5 px along its normal (crosses the 3 px test) | 2 slid along itself by up to +-1.3 lengths (one end
      point inside; none inside but touching; disjoint) | 3 scaled 0.2-2.5 about its midpoint (both inside; containing) | 4 rotated
      +-4 degrees about its midpoint (crosses the 2 degree test) | 5 end points swapped and rotated by +-0.2-1 degree (lands on
      either side of the wrap of % 180, not on it).
    Column ZERO_LENGTH_COL is a zero-length line; end point 1 of row ZERO_W_ROW projects with w = 0 (zero_w_point).
    Returns lines0 [B, n0, 2, 2], lines1 [B, n1, 2, 2] in `dtype` (built in float64, then cast) and H [B, 3, 3] float64."""
    n = max(n0, n1)
    L0, L1, Hs = [], [], []
    for b in range(B):
        r0, r1, m, _ = synth.homography_pair(seed + b, n, strength=0.3)
        rs = np.random.RandomState(seed + b + 1000)
        l0 = r0[:n0, :4].reshape(-1, 2, 2).copy()
        l1 = r1[:n1, :4].reshape(-1, 2, 2).copy()
        for j in range(len(l1)):
            s, e = l1[j, 0].copy(), l1[j, 1].copy()
            d = e - s
            ln = math.hypot(*d)
            u, mid = d / ln, (s + e) / 2
            nrm = np.array([-u[1], u[0]])
            kind = j % 6
            if kind == 1:
                off = nrm * rs.uniform(0, 5)
                s, e = s + off, e + off
            elif kind == 2:
                off = d * rs.uniform(-1.3, 1.3)
                s, e = s + off, e + off
            elif kind == 3:
                f = rs.uniform(0.2, 2.5)
                s, e = mid - d * f / 2, mid + d * f / 2
            elif kind in (4, 5):
                t = math.radians(rs.uniform(-4, 4) if kind == 4 else rs.uniform(0.2, 1) * rs.choice([-1, 1]))
                rot = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
                s, e = mid + rot @ (s - mid), mid + rot @ (e - mid)
                if kind == 5:
                    s, e = e, s
            l1[j, 0], l1[j, 1] = s, e
        if len(l1) > ZERO_LENGTH_COL:
            l1[ZERO_LENGTH_COL, 1] = l1[ZERO_LENGTH_COL, 0]
        m, pt = zero_w_point(m)
        if len(l0) > ZERO_W_ROW:
            l0[ZERO_W_ROW, 1] = pt
        L0.append(l0); L1.append(l1); Hs.append(m)
    return np.stack(L0).astype(dtype), np.stack(L1).astype(dtype), np.stack(Hs)
