"""The reference's validation step restated in NumPy, in this project's own words, at a chosen precision (float32: what the
reference computes; float64: the yardstick the GPU tests measure against), and the seeded clustered inputs the fixture
(tests/golden/make_golden_val_step.py) and the GPU tests share.  Test infrastructure only.

    descriptor_loss   evaluations/criteria.py:59-124,173-192
    matcher           evaluations/matcher.py:51-102
    counts / scores   evaluations/evaluate_pr.py:10-35
"""
import numpy as np

MATCH, MARGIN, MASKED = 0.3, 0.5, 10000.0
FP32_SPACING = 2.4e-7          # spacing of float32 just below 4 (distances lie in 0..4)
MIN_MARGIN = 1e-5              # ~40 spacings: a decision with this margin in float64 is the same in any float32 summation order


def dots(desc0, desc1, dtype):
    """<d0[b,:,a], d1[b,:,c]> [B,n,n]; desc [B,256,n]"""
    a, b = np.asarray(desc0, dtype), np.asarray(desc1, dtype)
    return np.matmul(a.transpose(0, 2, 1), b)


def anchor_rows(desc0, desc1, assign, dtype):
    """(row_pos, row_neg) [B,2n] in `dtype`: rows 0..n-1 of an item are the rows of D = 2 - 2 dot, rows n..2n-1 those of D^T.
    row_neg is -1 where the row is no anchor (pos <= 0) or has no semi-hard negative."""
    dt = np.dtype(dtype).type
    g = np.asarray(assign)[:, :-1, :-1]
    dist = dt(2) - dt(2) * dots(desc0, desc1, dtype)
    dist = np.concatenate([dist, dist.transpose(0, 2, 1)], axis=1)                  # [B,2n,n]
    match = np.concatenate([g > MATCH, (g > MATCH).transpose(0, 2, 1)], axis=1)
    unmatch = np.concatenate([g <= 0, (g <= 0).transpose(0, 2, 1)], axis=1)
    pos = np.where(match, dist, dt(0)).max(axis=2).astype(dtype)
    pos = np.maximum(pos, dt(0))
    cand = np.where(unmatch, dist, dt(MASKED)).astype(dtype)
    window = (cand > pos[..., None]) & (cand < (pos + dt(MARGIN))[..., None]) & (pos > 0)[..., None]
    neg = np.where(window, cand, dt(np.inf)).min(axis=2)
    return pos, np.where(np.isfinite(neg), neg, dt(-1)).astype(dtype)


def descriptor_loss(desc0, desc1, assign, dtype):
    """dict: loss, hardest_positive, hardest_negative (NaN when no anchor survives), rows (flat index b*2n + r of every survivor, in
    the reference's order), pos / neg of the survivors, row_pos / row_neg [B,2n]"""
    dt = np.dtype(dtype).type
    row_pos, row_neg = anchor_rows(desc0, desc1, assign, dtype)
    rows = np.nonzero(row_neg.reshape(-1) > 0)[0]
    pos, neg = row_pos.reshape(-1)[rows], row_neg.reshape(-1)[rows]
    out = {"rows": rows, "pos": pos, "neg": neg, "row_pos": row_pos, "row_neg": row_neg}
    if len(rows) == 0:
        out.update(loss=np.nan, hardest_positive=np.nan, hardest_negative=np.nan)
    else:
        out.update(loss=np.maximum(pos - neg + dt(1), dt(0)).mean(dtype=dtype), hardest_positive=pos.max(), hardest_negative=neg.min())
    return out


def scores(desc0, desc1, dtype):
    """the matcher's clipped squared distances [B,n,n]"""
    a, b = np.asarray(desc0, dtype), np.asarray(desc1, dtype)
    sq0, sq1 = np.square(a).sum(axis=1)[:, :, None], np.square(b).sum(axis=1)[:, None, :]
    return ((sq0 + sq1) - np.dtype(dtype).type(2) * dots(desc0, desc1, dtype)).clip(min=0)


def matcher(desc0, desc1, nn_thresh, mutual, dtype):
    """match01 [B,n] int32, -1 = no match"""
    sc = scores(desc0, desc1, dtype)
    B, n, _ = sc.shape
    idx = sc.argmin(axis=2)
    keep = np.take_along_axis(sc, idx[..., None], axis=2)[..., 0] < nn_thresh
    if mutual:
        back = sc.argmin(axis=1)
        keep &= np.take_along_axis(back, idx, axis=1) == np.arange(n)[None]
    return np.where(keep, idx, -1).astype(np.int32)


def with_dustbins(match01):
    """the [B,n+1,n+1] float64 matrix of matcher.py:92-100"""
    B, n = match01.shape
    mat = np.zeros((B, n + 1, n + 1))
    for b in range(B):
        free_rows, free_cols = np.ones(n + 1, bool), np.ones(n + 1, bool)
        for a in np.nonzero(match01[b] >= 0)[0]:
            mat[b, a, match01[b, a]] = 1
            free_rows[a] = free_cols[match01[b, a]] = False
        mat[b, free_rows, n] = 1
        mat[b, n, free_cols] = 1
    return mat


def counts(match01, assign):
    """[B,4] TP, FP, FN, TN"""
    gt = np.asarray(assign)[:, :-1, :-1] > 0
    B, n = match01.shape
    out = np.zeros((B, 4), np.int32)
    for b in range(B):
        has_gt, has_pred = gt[b].any(axis=1), match01[b] >= 0
        hit = has_pred & gt[b][np.arange(n), np.maximum(match01[b], 0)]
        tp, tn = int(hit.sum()), int((~has_gt & ~has_pred).sum())
        out[b] = tp, int((~has_gt).sum()) - tn, int(has_gt.sum()) - tp, tn
    return out


def prf(cnt, eps=1e-5):
    """[B,3] precision, recall, f1 (float64)"""
    tp, fp, fn = (cnt[:, i].astype(np.float64) for i in range(3))
    p, r = tp / (tp + fp + eps) * 100.0, tp / (tp + fn + eps) * 100.0
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(p + r == 0, 0.0, 2 * p * r / (p + r))
    return np.stack([p, r, f], axis=1)


def margins(desc0, desc1, assign, nn_thresh):
    """The smallest float64 margin of every compare a selection depends on: pos > 0, neg > pos, neg < pos + 0.5 (for every unmatched
    entry of every anchor row), the first-versus-second gap of every row and column argmin, score < nn_thresh."""
    g = np.asarray(assign)[:, :-1, :-1]
    dist = 2.0 - 2.0 * dots(desc0, desc1, np.float64)
    worst = np.inf
    for d, m, u in ((dist, g > MATCH, g <= 0), (dist.transpose(0, 2, 1), (g > MATCH).transpose(0, 2, 1), (g <= 0).transpose(0, 2, 1))):
        has = m.any(axis=2)
        top = np.where(m, d, -np.inf).max(axis=2)
        if has.any():
            worst = min(worst, np.abs(top[has]).min())
        anchors = has & (top > 0)
        for b, r in zip(*np.nonzero(anchors)):
            v = d[b, r][u[b, r]]
            if len(v):
                worst = min(worst, np.abs(v - top[b, r]).min(), np.abs(v - (top[b, r] + MARGIN)).min())
    sc = scores(desc0, desc1, np.float64)
    n = sc.shape[1]
    for axis in (2, 1):
        s = np.sort(sc, axis=axis)
        if n > 1:
            worst = min(worst, (np.take(s, 1, axis=axis) - np.take(s, 0, axis=axis)).min())
    worst = min(worst, np.abs(sc.min(axis=2) - nn_thresh).min())
    return float(worst)


def clustered_case(seed, B, n, n_centres=6):
    """Seeded inputs with semi-hard negatives: desc0 [B,256,n] = L2-normalised (one of n_centres unit centres + noise), the last
    min(3, n // 8) sub-lines of an item on centres of their own (their anchors find no semi-hard negative); desc1 = a permuted,
    noisier copy; assign [B,n+1,n+1] from the permutation: 1.0, a few 0.2 (neither match nor unmatch), some rows without a match."""
    rs = np.random.RandomState(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    lonely = min(3, n // 8)
    desc0, desc1 = np.zeros((B, n, 256)), np.zeros((B, n, 256))
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    for b in range(B):
        centres = unit(rs.standard_normal((n_centres + lonely, 256)))
        which = rs.randint(0, n_centres, n)
        if lonely:
            which[n - lonely:] = n_centres + np.arange(lonely)
        desc0[b] = unit(centres[which] + 0.5 * rs.standard_normal((n, 256)) / 16.0)
        perm = rs.permutation(n)
        desc1[b, perm] = unit(desc0[b] + 0.25 * rs.standard_normal((n, 256)) / 16.0)
        kind = rs.randint(0, 10, n)                       # 0: no match at all, 1: overlap 0.2, else a match
        if lonely:
            kind[n - lonely:] = 2
        for a in range(n):
            if kind[a] == 1:
                assign[b, a, perm[a]] = 0.2
            elif kind[a] >= 2:
                assign[b, a, perm[a]] = 1.0
    return (np.ascontiguousarray(desc0.transpose(0, 2, 1).astype(np.float32)),
            np.ascontiguousarray(desc1.transpose(0, 2, 1).astype(np.float32)), assign)
