"""The backward of a point-wise linear layer (Conv1d(k=1) / Linear, Y = act(X W^T + b)) and of the descriptor head
(models/line_transformer.py:245-246 of the reference: F.normalize(final_proj(x), p=2, dim=1)), restated from their formulas: a float64
closed form in NumPy (the reference of tests/test_gpu_linear_bwd.py), a torch restatement (what autograd differentiates: its float32
error is the bar) and the cases the tests and tools/linear_bwd_report.py share.  Test infrastructure only.

    rows-major: x [rows, K], W [N, K], b [N], g [rows, N] (the gradient arriving at the output), mask [rows, N] (the post-ReLU output)
    layer:  pre = x W^T + b;  y = relu?(pre);  g' = g [mask > 0];  dx = g' W;  dW = g'^T x;  db = column sums of g'
    head:   y = x W^T + b;  c = max(|y|, 1e-12);  d = y / c;  gy = (g - d (d . g)) / c where |y| >= 1e-12, g / 1e-12 elsewhere;
            dx = gy W;  dW = gy^T x;  db = column sums of gy
"""
import numpy as np

FACTOR = 4          # the bar: FACTOR x the float32 autograd error of the same case, floored at two float32 spacings of max |output|
EPS = 1e-12         # F.normalize's eps
NORM_CLEAR = 1e3    # the normal family keeps every |y| this factor away from EPS


def layer_closed_form(x, W, b, g, mask=None, relu=False):
    """float64.  dict: pre, y, dx, dW, db.  `mask`: the gradient passes where it is > 0 (None: everywhere)"""
    x, W, g = (np.asarray(a, np.float64) for a in (x, W, g))
    pre = x @ W.T + (0.0 if b is None else np.asarray(b, np.float64))
    gm = g if mask is None else np.where(np.asarray(mask) > 0, g, 0.0)
    return {"pre": pre, "y": np.maximum(pre, 0.0) if relu else pre, "dx": gm @ W, "dW": gm.T @ x, "db": gm.sum(axis=0)}


def head_closed_form(x, W, b, g):
    """float64.  dict: y, d, gy, dx, dW, db, norm"""
    x, W, b, g = (np.asarray(a, np.float64) for a in (x, W, b, g))
    y = x @ W.T + b
    norm = np.sqrt((y * y).sum(axis=1, keepdims=True))
    c = np.maximum(norm, EPS)
    d = y / c
    gy = np.where(norm >= EPS, (g - d * (d * g).sum(axis=1, keepdims=True)) / c, g / EPS)
    return {"y": y, "d": d, "gy": gy, "dx": gy @ W, "dW": gy.T @ x, "db": gy.sum(axis=0), "norm": norm[:, 0]}


def torch_layer(x, W, b, g, dtype, relu=False):
    """F.linear (+ F.relu) and autograd on the CPU at `dtype`: dict y, dx, dW, db as float64 arrays"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
    xt, Wt, bt = t(x), t(W), (t(b) if b is not None else None)
    with torch.enable_grad():
        y = F.linear(xt, Wt, bt)
        y = F.relu(y) if relu else y
        y.backward(torch.tensor(np.asarray(g), dtype=dtype))
    out = {"y": y.detach(), "dx": xt.grad, "dW": Wt.grad}
    if bt is not None:
        out["db"] = bt.grad
    return {k: v.double().numpy() for k, v in out.items()}


def torch_head(x, W, b, g, dtype):
    """F.normalize(F.linear(x, W, b), p=2, dim=1) and autograd on the CPU at `dtype`: dict d, gy, dx, dW, db as float64 arrays"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
    xt, Wt, bt = t(x), t(W), t(b)
    with torch.enable_grad():
        y = F.linear(xt, Wt, bt)
        y.retain_grad()
        d = F.normalize(y, p=2, dim=1)
        d.backward(torch.tensor(np.asarray(g), dtype=dtype))
    return {k: v.double().numpy() for k, v in (("d", d.detach()), ("gy", y.grad), ("dx", xt.grad), ("dW", Wt.grad), ("db", bt.grad))}


def bar_of(yardstick_err, out_max):
    """FACTOR x the reference-precision error of the output, floored at two float32 spacings of its largest magnitude"""
    return max(FACTOR * float(yardstick_err), 2 * float(np.spacing(np.float32(out_max))))


def bars(yard, ref, keys):
    """{key: (bar, yardstick error)} of the outputs `keys`: yard the float32 torch results, ref the float64 closed form"""
    out = {}
    for k in keys:
        err = np.abs(yard[k] - ref[k]).max()
        out[k] = (bar_of(err, np.abs(ref[k]).max()), float(err))
    return out


# ---- shapes.  Row edges: one row, the 32-row MFMA block, the 64-row tile, two tiles, the flagship's n = 250, and the chunk of the weight
# gradient's row reduction (Rc = linetr_linear_backward_chunk_rows(), asked of the library when a test runs).
ROW_EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 250, 257, "Rc-1", "Rc", "Rc+1", "2Rc+1"]
FULL_NK = (256, 256)
OTHER_NK = [(64, 32), (256, 512), (512, 512), (1024, 256), (256, 1024)]
# the other (N, K): every row edge once, dealt out in turn, and the two-chunk case with each
REDUCED = {nk: sorted(set(ROW_EDGES[i::len(OTHER_NK)] + ["2Rc+1"]), key=str) for i, nk in enumerate(OTHER_NK)}
CASES = [(r, *FULL_NK) for r in ROW_EDGES] + [(r, *nk) for nk in OTHER_NK for r in REDUCED[nk]]


def resolve_rows(r, chunk_rows):
    return {"Rc-1": chunk_rows - 1, "Rc": chunk_rows, "Rc+1": chunk_rows + 1, "2Rc+1": 2 * chunk_rows + 1}.get(r, r)


def case_seed(rows, N, K):
    return (rows * 7919 + N * 31 + K) % 100003


# ---- the exact family: integers in -3 .. 3.  |any partial sum| <= 9 max(K, N, rows) + 3 < 2^24, so float32 holds every partial sum
# of every contraction in any order, and the results must equal the float64 closed form bit for bit.
EXACT_MAX = 3


def exact_case(rows, N, K):
    """(x, W, b, g, mask) float32, integer-valued; mask: relu(pre) of the case itself (about half the entries pass)"""
    rs = np.random.RandomState(case_seed(rows, N, K))
    draw = lambda *shape: rs.randint(-EXACT_MAX, EXACT_MAX + 1, size=shape).astype(np.float32)
    x, W, b, g = draw(rows, K), draw(N, K), draw(N), draw(rows, N)
    mask = np.maximum(x.astype(np.float64) @ W.T.astype(np.float64) + b, 0.0).astype(np.float32)
    return x, W, b, g, mask


def exact_partial_sum_bound(x, W, b, g):
    """the largest sum of |products| (+ |bias|) of any output element of the four contractions: an upper bound of every partial sum"""
    ax, aW, ag = np.abs(x).astype(np.float64), np.abs(W).astype(np.float64), np.abs(g).astype(np.float64)
    return max((ax @ aW.T + np.abs(b)).max(), (ag @ aW).max(), (ag.T @ ax).max(), ag.sum(axis=0).max())


# ---- the normal family
def normal_case(rows, N, K, seed=None):
    """(x, W, b, g, mask) float32: unit-variance features and upstream, W ~ N(0, 1 / K) (unit-variance outputs), b ~ N(0, 0.01);
    mask: relu(pre) of the case itself, rounded to float32"""
    rs = np.random.RandomState(case_seed(rows, N, K) if seed is None else seed)
    x = rs.standard_normal((rows, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rs.standard_normal(N)).astype(np.float32)
    g = rs.standard_normal((rows, N)).astype(np.float32)
    mask = np.maximum(x.astype(np.float64) @ W.T.astype(np.float64) + b, 0.0).astype(np.float32)
    return x, W, b, g, mask


# the autograd-surface test of pointwise_linear with relu=True: [B, K, n] features.  Seeds chosen on the CPU so that no pre-activation
# lies within twice the bar of 0 (tests/test_linear_bwd_cpu.py asserts it): the library's own mask is then the float64 one.
RELU_SURFACE = {"B": 2, "n": 33, "N": 64, "K": 32, "seed": 1}


def relu_surface_case():
    c = RELU_SURFACE
    x, W, b, g, _ = normal_case(c["B"] * c["n"], c["N"], c["K"], seed=c["seed"])
    return x, W, b, g


# ---- descriptor_loss(DescriptorHead(x)): pre-head features whose descriptors are a clustered case of the loss gradient's generator.
# W = Q (orthogonal), x = Q^T (s d - b) with a scale s per position, so final_proj(x) = s d and line_desc = d up to rounding.
def head_surface_case(dtype=np.float64):
    """(W [256,256,1], b [256], x0, x1 [B,256,n], assign, desc0, desc1) -- B = 3, n = 65 of loss_grad_reference.edge_case"""
    import loss_grad_reference as LG
    d0, d1, assign = LG.edge_case(3, 65)
    rs = np.random.RandomState(23)
    Q, _ = np.linalg.qr(rs.standard_normal((256, 256)))
    b = 0.05 * rs.standard_normal(256)
    feats = []
    for d in (d0, d1):
        s = rs.uniform(0.5, 2.0, size=(d.shape[0], 1, d.shape[2]))
        feats.append(np.einsum("oc,bon->bcn", Q, s * d.astype(np.float64) - b[None, :, None]))
    W32, b32, x0, x1 = Q.astype(np.float32), b.astype(np.float32), feats[0].astype(np.float32), feats[1].astype(np.float32)
    return W32[:, :, None].astype(dtype), b32.astype(dtype), x0.astype(dtype), x1.astype(dtype), assign, d0, d1


def torch_head_surface(dtype):
    """the graph normalize(conv1d(x)) -> criterion on the CPU at `dtype`: (dict x0, x1, W, b of gradients as float64 arrays, loss, V,
    desc0, desc1 as float64 arrays)"""
    import torch
    import torch.nn.functional as F
    import loss_grad_reference as LG
    W, b, x0, x1, assign, _, _ = head_surface_case()
    t = lambda a: torch.tensor(a, dtype=dtype, requires_grad=True)
    Wt, bt, a0, a1 = t(W), t(b), t(x0), t(x1)
    with torch.enable_grad():
        e0, e1 = (F.normalize(F.conv1d(a, Wt, bt), p=2, dim=1) for a in (a0, a1))
        loss, _, _, V = LG.torch_criterion(e0, e1, torch.tensor(assign, dtype=dtype))
        loss.backward()
    grads = {"x0": a0.grad, "x1": a1.grad, "W": Wt.grad, "b": bt.grad}
    return ({k: v.double().numpy() for k, v in grads.items()}, float(loss.detach()), V, e0.detach().double().numpy(),
            e1.detach().double().numpy())
