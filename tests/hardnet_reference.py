"""The reference's HardNet criterion (descriptor_loss.compute_distances_hardnet under its forward, evaluations/criteria.py:126-192,
taken through torch autograd) restated from its formulas: a float64 closed form in NumPy (the yardstick of
tests/test_gpu_hardnet_loss.py), a vectorised torch restatement (what autograd differentiates: its float32 error is the bar where the
reference is absent, and it carries a gradient on to the weights of a graph in front of the descriptors), and the cases the tests and
tools/hardnet_loss_report.py share.  Test infrastructure only.

    D = 2 - 2 <d0[a], d1[c]>; cand = (assign <= 0 ? D : 10000); rowmin = min over a row of cand, colmin over a column
    2n anchor lines per item: the n rows of D, then its n columns
    pos_r = max(0, largest D with assign > 0.3 on the line), an anchor iff pos_r > 0; p_r the FIRST index attaining it
    neg_r = min(own, cross): own the minimum of the anchor's line, cross the minimum of the line of the other direction through p_r
    loss = mean over the V anchors of relu(pos - neg + 1);  w = upstream / V;  live iff pos - neg + 1 > 0
    dD: + w at (r, p_r) only; - w to the own line if own < cross, to the cross line if own > cross, w / 2 each if equal; on a line the
        share is split evenly over the unmatched entries equal to its minimum; entries valued 10000 carry nothing
    grad0[a] = -2 sum_c dD[a, c] d1[c]        grad1[c] = -2 sum_a dD[a, c] d0[a]
"""
import numpy as np

import val_step_reference as R
import loss_grad_reference as LG

FACTOR = LG.FACTOR      # the bar is the project's own rule: loss_grad_reference.bar_of
bar_of, max_err, grad_max = LG.bar_of, LG.max_err, LG.grad_max


def _lines(dist, g):
    """per direction (the rows of D, then its columns): (D, match, unmatch) with the anchor lines along axis 1"""
    match, unmatch = g > R.MATCH, g <= 0
    t = lambda x: x.transpose(0, 2, 1)
    return ((dist, match, unmatch), (t(dist), t(match), t(unmatch)))


def closed_form(desc0, desc1, assign, upstream=1.0):
    """float64.  dict: grad0, grad1 [B,256,n]; G [B,n,n] = d loss / d D; V; live; loss, hardest_positive, hardest_negative (NaN when
    V == 0); pos [B,2n]; neg, arg [B,2n] (-1 where the line is no anchor); alive [B,2n] bool"""
    d0, d1 = np.asarray(desc0, np.float64), np.asarray(desc1, np.float64)
    B, _, n = d0.shape
    g = np.asarray(assign)[:, :-1, :-1]
    dist = 2.0 - 2.0 * R.dots(d0, d1, np.float64)
    cand = np.where(g <= 0, dist, R.MASKED)
    mins = (cand.min(axis=2), cand.min(axis=1))                  # rowmin, colmin [B,n]
    G = np.zeros((B, n, n))
    pos, neg = np.zeros((B, 2 * n)), np.full((B, 2 * n), -1.0)
    arg, alive = np.full((B, 2 * n), -1, np.int64), np.zeros((B, 2 * n), bool)
    for side, (Ds, ms, us) in enumerate(_lines(dist, g)):
        Gs = np.zeros((B, n, n))                                  # in this direction's orientation: [anchor line][index along it]
        for b in range(B):
            for r in range(n):
                vals = np.where(ms[b, r], Ds[b, r], 0.0)
                p = int(vals.argmax())                            # NumPy's argmax: the first of equal maxima
                pos[b, side * n + r] = max(vals[p], 0.0)
                if not vals[p] > 0:
                    continue
                own, cross = mins[side][b, r], mins[1 - side][b, p]
                lo = min(own, cross)
                neg[b, side * n + r], arg[b, side * n + r] = lo, p
                if not vals[p] - lo + 1.0 > 0:                    # relu's strict > 0
                    continue
                alive[b, side * n + r] = True
                Gs[b, r, p] += 1.0
                to_own = 1.0 if own < cross else 0.0 if own > cross else 0.5
                ties = us[b, r] & (Ds[b, r] == own)
                if to_own and ties.any():
                    Gs[b, r, ties] -= to_own / ties.sum()
                ties = us[b, :, p] & (Ds[b, :, p] == cross)
                if to_own < 1 and ties.any():
                    Gs[b, ties, p] -= (1.0 - to_own) / ties.sum()
        G += Gs if side == 0 else Gs.transpose(0, 2, 1)
    anchors = arg >= 0
    V = int(anchors.sum())
    if V:
        G *= float(upstream) / V
    p, q = pos[anchors], neg[anchors]
    return {"grad0": -2.0 * np.matmul(d1, G.transpose(0, 2, 1)), "grad1": -2.0 * np.matmul(d0, G), "G": G, "V": V, "live": int(alive.sum()),
            "loss": np.maximum(p - q + 1.0, 0.0).mean() if V else np.nan, "hardest_positive": p.max() if V else np.nan,
            "hardest_negative": q.min() if V else np.nan, "pos": pos, "neg": neg, "arg": arg, "alive": alive}


def reference_order(cf):
    """(pos, neg) of the V anchors in the reference's order: the row anchors of every item, then the column anchors of every item"""
    n = cf["pos"].shape[1] // 2
    parts = [(cf["pos"][:, s], cf["neg"][:, s], cf["arg"][:, s] >= 0) for s in (slice(0, n), slice(n, 2 * n))]
    return np.concatenate([p[m] for p, _, m in parts]), np.concatenate([q[m] for _, q, m in parts])


def selection_gap(desc0, desc1, assign):
    """The smallest float64 margin of every decision the selection and its gradient depend on: pos > 0 on every line with a match, the
    first versus the second matched maximum of an anchor, the first versus the second cand minimum of every line, |own - cross| of every
    live anchor and |pos - neg + 1| of every anchor.  inf where nothing is decided."""
    g = np.asarray(assign)[:, :-1, :-1]
    dist = 2.0 - 2.0 * R.dots(desc0, desc1, np.float64)
    cf = closed_form(desc0, desc1, assign)
    B, n = g.shape[:2]
    cand = np.where(g <= 0, dist, R.MASKED)
    mins = (cand.min(axis=2), cand.min(axis=1))
    worst = np.inf
    for side, (Ds, ms, us) in enumerate(_lines(dist, g)):
        for b in range(B):
            for r in range(n):
                m = np.sort(Ds[b, r][ms[b, r]])
                if len(m):
                    worst = min(worst, abs(m[-1]))
                if len(m) > 1 and m[-1] > 0:
                    worst = min(worst, m[-1] - m[-2])
                v = np.sort(Ds[b, r][us[b, r]])
                if len(v) > 1:
                    worst = min(worst, v[1] - v[0])
                l = side * n + r
                if cf["arg"][b, l] >= 0:
                    worst = min(worst, abs(cf["pos"][b, l] - cf["neg"][b, l] + 1.0))
                    if cf["alive"][b, l]:
                        worst = min(worst, abs(mins[side][b, r] - mins[1 - side][b, cf["arg"][b, l]]))
    return float(worst)


def torch_criterion(desc0, desc1, assign, anchor_loop=False):
    """The criterion on torch tensors of any floating dtype and device, differentiable: (loss, hardest_positive, hardest_negative, V).
    The positive's index is the first of equal maxima on any device (computed, not left to torch.max).  anchor_loop: every anchor's
    negative from a Python loop over the anchors with three tiny torch calls each (two amin, one min), as the reference does -- what a
    training step pays without a native criterion; otherwise two amin over the whole matrix, a gather and one element-wise min."""
    import torch
    g = assign[:, :-1, :-1]
    n = g.shape[1]
    dist = 2 - 2 * torch.einsum("bdn,bdm->bnm", desc0, desc1)
    match, unmatch = g > R.MATCH, g <= 0
    cand = torch.where(unmatch, dist, torch.full_like(dist, R.MASKED))
    index = torch.arange(n, device=dist.device)
    pos_all, neg_all = [], []
    for flip in (False, True):
        Ds, ms, cs = (x.transpose(1, 2) if flip else x for x in (dist, match, cand))
        vals = torch.where(ms, Ds, torch.zeros_like(Ds))
        top = vals.detach().amax(dim=2, keepdim=True)
        first = torch.where(vals.detach() == top, index, n).amin(dim=2)                   # [B,n] the first index of the maximum
        pos = torch.gather(vals, 2, first[..., None])[..., 0]
        anchors = pos > 0
        if anchor_loop:
            negs = [torch.min(torch.amin(cs[b, a]), torch.amin(cs[b, :, p]))
                    for (b, a), p in zip(torch.nonzero(anchors).tolist(), first[anchors].tolist())]
            neg = torch.stack(negs) if negs else pos[anchors]
        else:
            neg = torch.min(cs.amin(dim=2), torch.gather(cs.amin(dim=1), 1, first))[anchors]
        pos_all.append(pos[anchors]); neg_all.append(neg)
    pos, neg = torch.cat(pos_all), torch.cat(neg_all)
    if len(pos) == 0:
        raise RuntimeError("no line has a positive")
    return torch.relu(pos - neg + 1).mean(), pos.max().detach(), neg.min().detach(), len(pos)


def torch_grads(desc0, desc1, assign, dtype, anchor_loop=False):
    """autograd through torch_criterion on the CPU at `dtype`: (grad0, grad1) [B,256,n] as float64 arrays"""
    import torch
    a = torch.tensor(np.asarray(desc0), dtype=dtype, requires_grad=True)
    b = torch.tensor(np.asarray(desc1), dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        torch_criterion(a, b, torch.tensor(np.asarray(assign), dtype=dtype), anchor_loop)[0].backward()
    return a.grad.double().numpy(), b.grad.double().numpy()


# ---- generated cases: (B, n, extra) -> seed of edge_case, chosen on the CPU so that every decision is MIN_MARGIN away from flipping
# (tests/test_hardnet_loss_cpu.py asserts it).  extra: second positives on some rows and columns, so the first of two matched maxima
# is picked away from ties.
WIDTHS = (1, 2, 63, 64, 65, 129)
EDGE_CASES = [(B, n, False) for n in WIDTHS for B in (1, 3)] + [(2, 250, False)] + [(1, n, True) for n in WIDTHS[1:] + (250,)]
EDGE_SEEDS = {(1, 1, False): 0, (3, 1, False): 0, (1, 2, False): 20, (3, 2, False): 4, (1, 63, False): 0, (3, 63, False): 0,
              (1, 64, False): 0, (3, 64, False): 0, (1, 65, False): 0, (3, 65, False): 0, (1, 129, False): 0, (3, 129, False): 0,
              (2, 250, False): 3, (1, 2, True): 20, (1, 63, True): 0, (1, 64, True): 0, (1, 65, True): 0, (1, 129, True): 1,
              (1, 250, True): 4}


def edge_case(B, n, extra=False, seed=None):
    d0, d1, assign = R.clustered_case(EDGE_SEEDS[(B, n, extra)] if seed is None else seed, B, n)
    if extra:
        rs = np.random.RandomState(1000 + n)
        for b in range(B):
            for a in rs.choice(n, max(1, n // 8), replace=False):
                free = np.nonzero(assign[b, a, :n] == 0)[0]
                if len(free):
                    assign[b, a, rs.choice(free)] = 1.0
    return d0, d1, assign


# ---- the exact family: the +-0.25 sign-flip descriptors of loss_grad_reference (inside a group D = differing signs / 4, across groups
# and against the zero padding D = 2), every share a dyadic rational and V a power of two, so the gradients must equal the closed form
# bit for bit.  No positive exceeds 1 where a line's minimum is the 2 of the padding, so the many entries tied there carry nothing.
# A group: (row sign flips, column sign flips, {(row, column): assign}[, sealed pairs]); a sealed pair's row and column hold 0.2 at
# every other entry: no unmatched entry on either line.
FILLER2 = ([()], [(0, 1), (0, 1, 2)], {(0, 0): 1.0})                                 # 2 anchors: pos 0.5, neg 0.75
FILLER3 = ([()], [(0, 1), (0,), (0, 1, 2)], {(0, 0): 1.0, (0, 1): 1.0})              # 3 anchors
GROUPS = {
    # two columns tied at the positive of row 0: the first alone gets the row anchor's +w
    "tied_positives": [([()], [(0, 1), (0, 1), (0, 1, 2)], {(0, 0): 1.0, (0, 1): 1.0})],
    # two equal row minima: w / 2 each, from the row anchor (own line) and from the column anchor (cross line)
    "tied_minima": [([()], [(0, 1), (0, 1, 2), (0, 1, 2)], {(0, 0): 1.0})],
    # own == cross = 0.75, two entries tied on each line: w / 4 to each of the four, from either anchor
    "own_equals_cross": [([(), (3,), (4,)], [(0, 1), (0, 1, 2), (0, 1, 2)], {(0, 0): 1.0})],
    # (0, 1) is the negative of both row anchors and of both column anchors: -4w
    "claimed_by_rows_and_columns": [([(), (5, 6)], [(0, 1), (0, 1, 2)], {(0, 0): 1.0, (1, 1): 1.0})],
    # pos 0.5, neg 1.5: pos - neg + 1 == 0 exactly, no gradient
    "relu_at_zero": [([()], [(0, 1), (0, 1, 2, 3, 4, 5)], {(0, 0): 1.0})],
    # no unmatched entry on the anchor's row or its positive's column: neg 10000, dead
    "no_unmatched": [([()], [(0, 1), (0, 1, 2)], {(0, 0): 1.0}, [(0, 0)])],
    # assign 0.2 on the smallest distance of the row: neither a match nor a negative
    "middle_assign": [([()], [(0, 1), (0,), (0, 1, 2)], {(0, 0): 1.0, (0, 1): 0.2})],
}
EXACT_VARIANTS = list(GROUPS) + ["combined"]


def _item(groups, n, perm_seed=None):
    plain = [g[:3] for g in groups]
    d0, d1, assign = LG._item(plain, n, perm_seed)
    pr, pc = (np.arange(n), np.arange(n)) if perm_seed is None else (np.random.RandomState(perm_seed).permutation(n),
                                                                      np.random.RandomState(perm_seed + 1).permutation(n))
    r0 = c0 = 0
    for g in groups:
        for r, c in (g[3] if len(g) > 3 else ()):
            a, b = pr[r0 + r], pc[c0 + c]
            keep = assign[a, b]
            assign[a, :n], assign[:n, b] = 0.2, 0.2
            assign[a, b] = keep
        r0, c0 = r0 + len(g[0]), c0 + len(g[1])
    return d0, d1, assign


def _fillers(own):
    """fillers that bring `own` anchors to a power of two >= 4"""
    for total in (4, 8, 16, 32, 64):
        rest = total - own
        if rest >= 0 and rest != 1:
            return [FILLER3] * (rest % 2) + [FILLER2] * ((rest - 3 * (rest % 2)) // 2)
    raise ValueError(own)


def exact_case(variant):
    """(desc0, desc1 [B,256,n], assign [B,n+1,n+1]) with V a power of two.  A named variant: B = 1, n = 24, its groups first (indices as
    in GROUPS), then fillers.  'combined': B = 2, n = 70 (two tiles), every variant plus fillers in item 0, fillers in item 1, rows and
    columns scattered by a fixed permutation."""
    count = lambda groups, n: closed_form(*(x[None] for x in _item(groups, n)))["V"]
    if variant == "combined":
        every = [g for v in GROUPS.values() for g in v]
        every = every + _fillers(count(every, 70) + 8)
        items = [_item(every, 70, perm_seed=3), _item([FILLER2] * 4, 70, perm_seed=5)]
    else:
        groups = GROUPS[variant]
        items = [_item(groups + _fillers(count(groups, 24)), 24)]
    return tuple(np.stack([it[k] for it in items]) for k in range(3))
