"""The gradient of the reference's descriptor_loss (evaluations/criteria.py:59-124,173-192, taken through torch autograd) with respect
to line_desc0 / line_desc1, restated from its formulas: a float64 closed form in NumPy (the yardstick of tests/test_gpu_loss_grad.py),
a torch restatement of the criterion (what autograd differentiates: its float32 error is the bar, and it carries a gradient on to the
weights of a graph in front of the descriptors), and the cases the tests and tools/loss_grad_report.py share.  Test infrastructure
only.

    D = 2 - 2 <d0[a], d1[c]>; anchor rows: the n rows of D, then the n rows of D^T
    pos_r = amax_c(D[r, c] [assign > 0.3]), an anchor iff pos_r > 0
    neg_r = the FIRST smallest v = (assign <= 0 ? D : 10000) with pos_r < v < pos_r + 0.5; no such entry: the row is dropped
    loss = mean over the V survivors of relu(pos - neg + 1);  w = upstream / V
    dD: + w / ties at every entry tied at the positive (amax's backward splits evenly), - w at the negative's index
    grad0[a] = -2 sum_c dD[a, c] d1[c]        grad1[c] = -2 sum_a dD[a, c] d0[a]
"""
import numpy as np

import val_step_reference as R

FACTOR = 4          # the bar: FACTOR x the float32 autograd error of the same case, floored at two float32 spacings of max |gradient|


def closed_form(desc0, desc1, assign, upstream=1.0):
    """float64.  dict: grad0, grad1 [B,256,n]; G [B,n,n] = d loss / d D; V; loss; rows (flat index b*2n + r of every survivor, the
    reference's order); ties, neg_index [B,2n] (0 / -1 where the row gives no gradient)"""
    d0, d1 = np.asarray(desc0, np.float64), np.asarray(desc1, np.float64)
    B, _, n = d0.shape
    g = np.asarray(assign)[:, :-1, :-1]
    dist = 2.0 - 2.0 * R.dots(d0, d1, np.float64)
    G = np.zeros((B, n, n))
    pos_all, neg_all, ties_all, idx_all = [], [], [], []
    for side in (0, 1):                                          # the rows of D, then the rows of D^T
        Ds, gs = (dist, g) if side == 0 else (dist.transpose(0, 2, 1), g.transpose(0, 2, 1))
        match, unmatch = gs > R.MATCH, gs <= 0
        pos = np.maximum(np.where(match, Ds, 0.0).max(axis=2), 0.0)
        cand = np.where(unmatch, Ds, R.MASKED)
        window = (cand > pos[..., None]) & (cand < (pos + R.MARGIN)[..., None]) & (pos > 0)[..., None]
        masked = np.where(window, cand, np.inf)
        idx = masked.argmin(axis=2)                              # NumPy's argmin: the first of equal minima
        neg = np.take_along_axis(masked, idx[..., None], axis=2)[..., 0]
        live = np.isfinite(neg) & (pos - np.where(np.isfinite(neg), neg, 0.0) + 1.0 > 0)       # relu's strict > 0
        tied = match & (Ds == pos[..., None]) & live[..., None]
        ties = tied.sum(axis=2)
        share = tied / np.maximum(ties, 1)[..., None]
        share[live, idx[live]] -= 1.0
        G += share if side == 0 else share.transpose(0, 2, 1)
        pos_all.append(pos); neg_all.append(np.where(np.isfinite(neg), neg, -1.0))
        ties_all.append(ties); idx_all.append(np.where(live, idx, -1))
    pos, neg = np.concatenate(pos_all, axis=1), np.concatenate(neg_all, axis=1)
    rows = np.nonzero(neg.reshape(-1) > 0)[0]
    V = len(rows)
    if V:
        G *= float(upstream) / V
    p, q = pos.reshape(-1)[rows], neg.reshape(-1)[rows]
    return {"grad0": -2.0 * np.matmul(d1, G.transpose(0, 2, 1)), "grad1": -2.0 * np.matmul(d0, G), "G": G, "V": V, "rows": rows,
            "loss": np.maximum(p - q + 1.0, 0.0).mean() if V else np.nan,
            "ties": np.concatenate(ties_all, axis=1), "neg_index": np.concatenate(idx_all, axis=1)}


def selection_gap(desc0, desc1, assign):
    """What val_step_reference.margins does not look at and a gradient depends on, in float64 over the surviving anchors: the gap between
    the two smallest semi-hard entries (which index the negative is) and between the two largest matched entries (whether the positive
    is tied).  inf when no anchor has two of either."""
    g = np.asarray(assign)[:, :-1, :-1]
    dist = 2.0 - 2.0 * R.dots(desc0, desc1, np.float64)
    worst = np.inf
    for Ds, gs in ((dist, g), (dist.transpose(0, 2, 1), g.transpose(0, 2, 1))):
        match = gs > R.MATCH
        pos = np.maximum(np.where(match, Ds, 0.0).max(axis=2), 0.0)
        cand = np.where(gs <= 0, Ds, R.MASKED)
        window = (cand > pos[..., None]) & (cand < (pos + R.MARGIN)[..., None]) & (pos > 0)[..., None]
        for b, r in zip(*np.nonzero(window.any(axis=2))):
            v = np.sort(cand[b, r][window[b, r]])
            m = np.sort(Ds[b, r][match[b, r]])
            if len(v) > 1:
                worst = min(worst, v[1] - v[0])
            if len(m) > 1:
                worst = min(worst, m[-1] - m[-2])
    return float(worst)


def torch_criterion(desc0, desc1, assign, row_loop=False):
    """The criterion on torch tensors of any floating dtype and device, differentiable: (loss, hardest_positive, hardest_negative, V).
    row_loop: pick every anchor's negative in a Python loop over the anchor rows, as the reference does (what a training step pays
    without a native criterion); otherwise one masked argmin (torch returns the first of equal minima, as the loop's argmin does)."""
    import torch
    g = assign[:, :-1, :-1]
    dist = 2 - 2 * torch.einsum("bdn,bdm->bnm", desc0, desc1)
    both = torch.cat([dist, dist.transpose(1, 2)], dim=1)
    match = torch.cat([g > R.MATCH, (g > R.MATCH).transpose(1, 2)], dim=1)
    unmatch = torch.cat([g <= 0, (g <= 0).transpose(1, 2)], dim=1)
    pos = torch.amax(torch.where(match, both, torch.zeros_like(both)), dim=2).reshape(-1)
    cand = torch.where(unmatch, both, torch.full_like(both, R.MASKED)).reshape(-1, both.shape[2])
    anchors = torch.nonzero(pos > 0)[:, 0]
    pos, cand = pos[anchors], cand[anchors]
    window = (cand > pos[:, None]) & (cand < pos[:, None] + R.MARGIN)
    if row_loop:
        kept, negs = [], []
        for i in range(len(pos)):
            inside = cand[i][window[i]]
            if len(inside):
                kept.append(i)
                negs.append(inside[torch.argmin(inside)])
        if not kept:
            raise RuntimeError("no anchor has a semi-hard negative")
        pos, neg = pos[kept], torch.stack(negs)
    else:
        kept = window.any(dim=1)
        if not bool(kept.any()):
            raise RuntimeError("no anchor has a semi-hard negative")
        masked = torch.where(window, cand, torch.full_like(cand, float("inf")))
        neg = torch.gather(cand, 1, masked.argmin(dim=1, keepdim=True))[:, 0][kept]
        pos = pos[kept]
    return torch.relu(pos - neg + 1).mean(), pos.max().detach(), neg.min().detach(), len(pos)


def torch_grads(desc0, desc1, assign, dtype, row_loop=False):
    """autograd through torch_criterion on the CPU at `dtype`: (grad0, grad1) [B,256,n] as float64 arrays"""
    import torch
    a = torch.tensor(np.asarray(desc0), dtype=dtype, requires_grad=True)
    b = torch.tensor(np.asarray(desc1), dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        torch_criterion(a, b, torch.tensor(np.asarray(assign), dtype=dtype), row_loop)[0].backward()
    return a.grad.double().numpy(), b.grad.double().numpy()


def bar_of(yardstick_err, grad_max):
    """FACTOR x the reference-precision error of the case, floored at two float32 spacings of its largest gradient magnitude"""
    return max(FACTOR * float(yardstick_err), 2 * float(np.spacing(np.float32(grad_max))))


def max_err(got0, got1, ref):
    return max(np.abs(np.asarray(got0, np.float64) - ref["grad0"]).max(), np.abs(np.asarray(got1, np.float64) - ref["grad1"]).max())


def grad_max(ref):
    return max(np.abs(ref["grad0"]).max(), np.abs(ref["grad1"]).max())


# ---- generated cases: (B, n) -> seed of val_step_reference.clustered_case, chosen on the CPU so that every compare a selection
# depends on is MIN_MARGIN away from flipping (tests/test_loss_grad_cpu.py asserts it)
EDGE_SEEDS = {(1, 1): 0, (3, 1): 0, (1, 2): 20, (3, 2): 4, (1, 63): 0, (3, 63): 0, (1, 64): 0, (3, 64): 0, (1, 65): 0, (3, 65): 0,
              (1, 129): 0, (3, 129): 0, (2, 250): 3}
EDGE_CASES = [(B, n) for n in (1, 2, 63, 64, 65, 129) for B in (1, 3)] + [(2, 250)]
NN_THRESH = 0.7          # margins() also looks at the matcher's compares; the criterion has none of them


def edge_case(B, n):
    return R.clustered_case(EDGE_SEEDS[(B, n)], B, n)


# ---- the exact family: descriptors with 16 entries of +-0.25 on a 16-channel support of their own group.  Inside a group
# D = (number of differing signs) / 4, across groups D = 2 (never inside a window: every pos is 0.5); every product and sum below is
# exact in float32 and V is a power of two, so the gradients must equal the closed form bit for bit.
# A group: (row sign flips, column sign flips, {(row, column): assign}).
FILLER = ([()], [(0, 1), (0, 1, 2)], {(0, 0): 1.0})          # one surviving row anchor: pos 0.5, neg 0.75
GROUPS = {
    # two columns tied at the positive of row 0: each w / 2
    "tied_positives": [([()], [(0, 1), (0, 1), (0, 1, 2)], {(0, 0): 1.0, (0, 1): 1.0})],
    # two equal semi-hard negatives: the first column alone gets -w
    "tied_negatives": [([()], [(0, 1), (0, 1, 2), (0, 1, 2)], {(0, 0): 1.0})],
    # (0, 0) is the positive of row anchor 0 AND of column anchor 0 (whose negative is row 1): 2w
    "claimed_twice": [([(), (3,)], [(0, 1), (0, 1, 2)], {(0, 0): 1.0})],
    # unmatched entries exactly at pos (column 1) and at pos + 0.5 (column 2) are no negatives; the second group's anchor has nothing else
    "strict_window": [([()], [(0, 1), (2, 3), (0, 1, 2, 3), (0, 1, 2)], {(0, 0): 1.0}),
                      ([()], [(0, 1), (2, 3), (0, 1, 2, 3)], {(0, 0): 1.0})],
    # assign 0.2 in front of the negative (no unmatch), 0.25 and exactly 0.3 on larger distances (no match)
    "middle_assign": [([()], [(0, 1), (0, 1, 2), (0, 1, 2), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5)],
                       {(0, 0): 1.0, (0, 1): 0.2, (0, 3): 0.25, (0, 4): np.float32(0.3)})],
}
EXACT_VARIANTS = list(GROUPS) + ["combined"]


def _item(groups, n, perm_seed=None):
    rows, cols, entries = [], [], []
    for gi, (rflips, cflips, asg) in enumerate(groups):
        def vec(flips):
            x = np.zeros(256, np.float32)
            x[16 * gi:16 * gi + 16] = 0.25
            x[[16 * gi + f for f in flips]] = -0.25
            return x
        r0, c0 = len(rows), len(cols)
        rows += [vec(f) for f in rflips]
        cols += [vec(f) for f in cflips]
        entries += [(r0 + r, c0 + c, v) for (r, c), v in asg.items()]
    assert len(groups) <= 16 and max(len(rows), len(cols)) <= n
    pr, pc = (np.arange(n), np.arange(n)) if perm_seed is None else (np.random.RandomState(perm_seed).permutation(n),
                                                                      np.random.RandomState(perm_seed + 1).permutation(n))
    d0, d1, assign = np.zeros((n, 256), np.float32), np.zeros((n, 256), np.float32), np.zeros((n + 1, n + 1), np.float32)
    for i, x in enumerate(rows):
        d0[pr[i]] = x
    for i, x in enumerate(cols):
        d1[pc[i]] = x
    for r, c, v in entries:
        assign[pr[r], pc[c]] = v
    return d0.T.copy(), d1.T.copy(), assign


def exact_case(variant):
    """(desc0, desc1 [B,256,n], assign [B,n+1,n+1]) with V a power of two.  A named variant: B = 1, its groups first (indices as in
    GROUPS), fillers up to V = 4.  'combined': B = 2, n = 70 (two tiles), every variant plus fillers in item 0, fillers in item 1, rows and
    columns scattered by a fixed permutation; V = 16."""
    if variant == "combined":
        every = [g for v in GROUPS.values() for g in v]
        items = [_item(every + [FILLER] * 2, 70, perm_seed=3), _item([FILLER] * 8, 70, perm_seed=5)]
    else:
        groups = GROUPS[variant]
        own = closed_form(*(x[None] for x in _item(groups, 8)))["V"]
        items = [_item(groups + [FILLER] * (4 - own), 16)]
    return tuple(np.stack([it[k] for it in items]) for k in range(3))
