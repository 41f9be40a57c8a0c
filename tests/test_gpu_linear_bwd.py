"""GPU: the native backward of a point-wise linear layer and of the descriptor head (csrc/lt_linbwd.h; linetr_linear_forward /
_backward, linetr_head_forward / _backward; Engine.linear_* / head_*; linetr_amd.train_ops) against the float64 closed forms that
tests/test_linear_bwd_cpu.py pins to autograd through the reference (tests/linear_bwd_reference.py, tests/golden/head_bwd.npz).

The bar of an output is 4 x the float32 torch autograd error of the SAME case against float64 (torch on the CPU), floored at two
float32 spacings of the output's largest magnitude; the exact family must match bit for bit.
Measured on the MI355X: profiles/linear_bwd_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load
import linear_bwd_reference as LB

pytestmark = pytest.mark.gpu
E_ARG = -1
LAYER_KEYS = ("y", "dx", "dW", "db")
HEAD_KEYS = ("d", "gy", "dx", "dW", "db")


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def L():
    from linetr_amd import _native as nat
    return nat.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


def run_layer(eng, x, W, b, g, mask, relu):
    """forward and backward through the Engine: dict y, dx, dW, db as arrays"""
    xd, Wd = dev(x), dev(W)
    y = eng.linear_forward(xd, Wd, dev(b) if b is not None else None, relu=relu)
    dx, dW, db = eng.linear_backward(xd, Wd, dev(g), mask=dev(mask) if mask is not None else None)
    return {k: v.cpu().numpy() for k, v in (("y", y), ("dx", dx), ("dW", dW), ("db", db))}


def run_head(L, x, W, b, g, want=(True, True, True)):
    """the raw entry points: dict d, gy (read back from the head of the workspace), dx, dW, db"""
    rows = x.shape[0]
    xd, Wd, bd, gd = dev(x), dev(W), dev(b), dev(g)
    d = torch.full_like(xd, float("nan"))
    dx, dW, db = torch.full_like(xd, float("nan")), torch.full((256, 256), float("nan"), device="cuda"), torch.full((256,), float("nan"), device="cuda")
    ws = torch.empty(L.linetr_head_backward_workspace_bytes(rows), dtype=torch.uint8, device="cuda")
    assert L.linetr_head_forward(None, xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), rows, d.data_ptr(), stream()) == 0
    assert L.linetr_head_backward(None, xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), gd.data_ptr(), rows, ptr(dx if want[0] else None),
                                  ptr(dW if want[1] else None), ptr(db if want[2] else None), ws.data_ptr(), ws.numel(), stream()) == 0
    torch.cuda.synchronize()
    gy = ws[:rows * 256 * 4].view(torch.float32).view(rows, 256)
    return {k: v.cpu().numpy() for k, v in (("d", d), ("gy", gy), ("dx", dx), ("dW", dW), ("db", db))}


def check_bars(got, ref, yard, keys, label):
    worst = 0.0
    for k, (bar, yerr) in LB.bars(yard, ref, keys).items():
        err = np.abs(got[k].astype(np.float64) - ref[k]).max()
        worst = max(worst, err / bar)
        print(f"linear_bwd {label} {k}: err {err:.3e}, yardstick {yerr:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert err <= bar, (label, k, err, bar)
    return worst


@pytest.mark.parametrize("rows,N,K", LB.CASES)
def test_exact_family_is_bit_equal(eng, L, rows, N, K):
    rows = LB.resolve_rows(rows, L.linetr_linear_backward_chunk_rows())
    x, W, b, g, mask = LB.exact_case(rows, N, K)
    for m, relu in ((None, False), (mask, True)):
        cf, got = LB.layer_closed_form(x, W, b, g, m, relu), run_layer(eng, x, W, b, g, m, relu)
        for k in LAYER_KEYS:
            assert got[k].shape == cf[k].shape and np.array_equal(got[k], cf[k].astype(np.float32)), (k, relu)


@pytest.mark.parametrize("rows,N,K", LB.CASES)
def test_normal_family_within_the_bar(eng, L, rows, N, K):
    label = f"rows={rows} N={N} K={K}"
    rows = LB.resolve_rows(rows, L.linetr_linear_backward_chunk_rows())
    x, W, b, g, mask = LB.normal_case(rows, N, K)
    yard = LB.torch_layer(x, W, b, g, torch.float32)
    check_bars(run_layer(eng, x, W, b, g, None, False), LB.layer_closed_form(x, W, b, g), yard, LAYER_KEYS, label)
    # with the mask (the case's own post-ReLU output, handed in): the yardstick is autograd through F.relu
    yard = LB.torch_layer(x, W, b, g, torch.float32, relu=True)
    check_bars(run_layer(eng, x, W, b, g, mask, True), LB.layer_closed_form(x, W, b, g, mask, True), yard, LAYER_KEYS, label + " relu")


@pytest.mark.parametrize("rows", LB.ROW_EDGES)
def test_head_within_the_bar(L, rows):
    label = f"head rows={rows}"
    rows = LB.resolve_rows(rows, L.linetr_linear_backward_chunk_rows())
    x, W, b, g, _ = LB.normal_case(rows, 256, 256)
    cf = LB.head_closed_form(x, W, b, g)
    assert cf["norm"].min() > LB.NORM_CLEAR * LB.EPS
    check_bars(run_head(L, x, W, b, g), cf, LB.torch_head(x, W, b, g, torch.float32), HEAD_KEYS, label)


def test_head_fixture(eng):
    f, w = load("head_bwd"), load("head_bwd_dw")
    x, W, b, g = dev(f["x"]), dev(f["weight"]), dev(f["bias"]), dev(f["upstream"])
    desc = eng.head_forward(x, W, b)
    dx, dW, db = eng.head_backward(x, W, b, g)
    assert desc.shape == dx.shape == x.shape and dW.shape == (256, 256, 1) and db.shape == (256,)
    got = {"line_desc": desc, "dx": dx, "dW": dW, "db": db}
    for k, v in got.items():
        src = w if k == "dW" else f
        ref = src[f"{k}_f64"]
        bar = LB.bar_of(np.abs(src[f"{k}_f32"].astype(np.float64) - ref).max(), np.abs(ref).max())
        err = np.abs(v.cpu().double().numpy() - ref).max()
        print(f"linear_bwd head fixture {k}: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert err <= bar, (k, err, bar)


def test_row_strides_larger_than_the_width(eng, L):
    """x (and dx) in a [rows, K + 12] block, g and y in [rows, N + 4] blocks: the same bits as the dense call; the padding is untouched"""
    rows, N, K = 129, 256, 256
    x, W, b, g, mask = LB.exact_case(rows, N, K)
    cf = LB.layer_closed_form(x, W, b, g)
    Wd, bd = dev(W), dev(b)
    xw, gw = torch.full((rows, K + 12), 7.0, device="cuda"), torch.full((rows, N + 4), 7.0, device="cuda")
    xw[:, :K], gw[:, :N] = dev(x), dev(g)
    yw, dxw = torch.full((rows, N + 4), 7.0, device="cuda"), torch.full((rows, K + 12), 7.0, device="cuda")
    dW, db = torch.empty((N, K), device="cuda"), torch.empty((N,), device="cuda")
    ws = torch.empty(L.linetr_linear_backward_workspace_bytes(rows, N, K), dtype=torch.uint8, device="cuda")
    assert L.linetr_linear_forward(None, xw.data_ptr(), K + 12, Wd.data_ptr(), bd.data_ptr(), rows, N, K, 0, yw.data_ptr(), N + 4, stream()) == 0
    # (d_dx shares x's stride)
    assert L.linetr_linear_backward(None, xw.data_ptr(), K + 12, Wd.data_ptr(), gw.data_ptr(), N + 4, None, rows, N, K, dxw.data_ptr(),
                                    dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(yw[:, :N].cpu().numpy(), cf["y"].astype(np.float32)) and (yw[:, N:] == 7.0).all()
    assert np.array_equal(dxw[:, :K].cpu().numpy(), cf["dx"].astype(np.float32)) and (dxw[:, K:] == 7.0).all()
    assert np.array_equal(dW.cpu().numpy(), cf["dW"].astype(np.float32)) and np.array_equal(db.cpu().numpy(), cf["db"].astype(np.float32))
    # the Engine takes a strided view as it is
    y = eng.linear_forward(xw[:, :K], Wd, bd)
    dx, dW2, db2 = eng.linear_backward(xw[:, :K], Wd, gw[:, :N])
    assert dx.stride(0) == K + 12 and torch.equal(y, yw[:, :N]) and torch.equal(dx, dxw[:, :K]) and torch.equal(dW2, dW) and torch.equal(db2, db)


def test_zero_row_takes_the_eps_branch(L):
    """a row with y = 0 exactly (zero features, zero bias): d = 0 and gy = g / 1e-12, as clamp_min's backward leaves it"""
    x, W, _, g, _ = LB.normal_case(65, 256, 256)
    x[40] = 0.0
    b = np.zeros(256, np.float32)
    got = run_head(L, x, W, b, g)
    assert not got["d"][40].any() and np.array_equal(got["gy"][40], g[40] / np.float32(1e-12))
    cf = LB.head_closed_form(x, W, b, g)
    others = np.arange(65) != 40
    yard = LB.torch_head(x[others], W, b, g[others], torch.float32)
    for k in ("d", "gy"):
        bar = LB.bar_of(np.abs(yard[k] - cf[k][others]).max(), np.abs(cf[k][others]).max())
        assert np.abs(got[k][others] - cf[k][others]).max() <= bar, k
    assert np.isfinite(got["dx"]).all() and np.isfinite(got["dW"]).all() and np.isfinite(got["db"]).all()


def test_two_calls_give_identical_bits(eng, L):
    Rc = L.linetr_linear_backward_chunk_rows()
    x, W, b, g, mask = LB.normal_case(2 * Rc + 1, 256, 512)
    a, c = run_layer(eng, x, W, b, g, mask, True), run_layer(eng, x, W, b, g, mask, True)
    for k in LAYER_KEYS:
        assert a[k].tobytes() == c[k].tobytes(), k
    x, W, b, g, _ = LB.normal_case(2 * Rc + 1, 256, 256)
    h0, h1 = run_head(L, x, W, b, g), run_head(L, x, W, b, g)
    for k in HEAD_KEYS:
        assert h0[k].tobytes() == h1[k].tobytes(), k
    # another stream, other work in between
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run_layer(eng, x, W, b, g, None, False)
    side.synchronize()
    m = run_layer(eng, x, W, b, g, None, False)
    for k in LAYER_KEYS:
        assert s[k].tobytes() == m[k].tobytes(), k


def test_null_outputs_are_honoured(eng, L):
    x, W, b, g, mask = LB.normal_case(129, 256, 256)
    full = run_layer(eng, x, W, b, g, mask, True)
    xd, Wd, gd, md = dev(x), dev(W), dev(g), dev(mask)
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (False, False, False)):
        dx, dW, db = eng.linear_backward(xd, Wd, gd, mask=md, need=need)
        for k, v, n in (("dx", dx, need[0]), ("dW", dW, need[1]), ("db", db, need[2])):
            assert (v is not None) == n and (v is None or np.array_equal(v.cpu().numpy(), full[k])), (need, k)
    nobias = eng.linear_forward(xd, Wd, None, relu=False).cpu().numpy()          # d_b = NULL
    assert np.array_equal(nobias, eng.linear_forward(xd, Wd, torch.zeros(256, device="cuda")).cpu().numpy())
    every = run_head(L, x, W, b, g)
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        some = run_head(L, x, W, b, g, want)
        for k, n in zip(("dx", "dW", "db"), want):
            assert np.array_equal(some[k], every[k]) if n else np.isnan(some[k]).all(), (want, k)


def test_argument_errors(L):
    rows, N, K = 70, 256, 256
    x, W, b, g = (torch.zeros(s, device="cuda") for s in ((rows, K), (N, K), (N,), (rows, N)))
    y, dx, dW, db = torch.full((rows, N), 7.0, device="cuda"), torch.full((rows, K), 7.0, device="cuda"), torch.full((N, K), 7.0, device="cuda"), torch.full((N,), 7.0, device="cuda")
    ws = torch.empty(L.linetr_linear_backward_workspace_bytes(rows, N, K), dtype=torch.uint8, device="cuda")
    hws = torch.empty(L.linetr_head_backward_workspace_bytes(rows), dtype=torch.uint8, device="cuda")

    def fwd(x_=x, ldx=K, W_=W, b_=b, rows_=rows, N_=N, K_=K, act=0, y_=y, ldy=N):
        return L.linetr_linear_forward(None, ptr(x_), ldx, ptr(W_), ptr(b_), rows_, N_, K_, act, ptr(y_), ldy, stream())

    def bwd(x_=x, ldx=K, W_=W, g_=g, ldg=N, m_=None, rows_=rows, N_=N, K_=K, dx_=dx, dW_=dW, db_=db, ws_=ws, nbytes=None):
        return L.linetr_linear_backward(None, ptr(x_), ldx, ptr(W_), ptr(g_), ldg, ptr(m_), rows_, N_, K_, ptr(dx_), ptr(dW_), ptr(db_),
                                        ptr(ws_), ws.numel() if nbytes is None else nbytes, stream())

    def hbwd(x_=x, W_=W, b_=b, g_=g, rows_=rows, ws_=hws, nbytes=None):
        return L.linetr_head_backward(None, ptr(x_), ptr(W_), ptr(b_), ptr(g_), rows_, ptr(dx), ptr(dW), ptr(db), ptr(ws_),
                                      hws.numel() if nbytes is None else nbytes, stream())

    off = lambda t: t.view(-1)[1:]                                               # 4 bytes past a 16-byte boundary
    refused = [fwd(x_=None), fwd(W_=None), fwd(y_=None), fwd(rows_=0), fwd(N_=96), fwd(N_=2048), fwd(K_=48), fwd(K_=2048), fwd(act=2),
               fwd(ldx=K - 4), fwd(ldx=K + 2), fwd(ldy=N + 1), fwd(x_=off(x)), fwd(y_=off(y)), fwd(W_=off(W)),
               bwd(x_=None), bwd(W_=None), bwd(g_=None), bwd(rows_=0), bwd(rows_=-5), bwd(N_=32), bwd(K_=16), bwd(ldx=K - 4), bwd(ldg=N + 3),
               bwd(g_=off(g)), bwd(m_=off(g)), bwd(dx_=off(dx)), bwd(dW_=off(dW)), bwd(ws_=None), bwd(nbytes=ws.numel() - 1),
               bwd(nbytes=L.linetr_linear_backward_workspace_bytes(rows, N, K) - 1),
               hbwd(x_=None), hbwd(W_=None), hbwd(b_=None), hbwd(g_=None), hbwd(rows_=0), hbwd(ws_=None),
               hbwd(nbytes=L.linetr_head_backward_workspace_bytes(rows) - 1),
               L.linetr_head_forward(None, ptr(x), ptr(W), None, rows, ptr(y), stream()),
               L.linetr_head_forward(None, ptr(x), ptr(W), ptr(b), 0, ptr(y), stream()),
               L.linetr_head_forward(None, ptr(x), ptr(W), ptr(b), rows, None, stream())]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_last_error()
    torch.cuda.synchronize()
    for t in (y, dx, dW, db):
        assert (t == 7.0).all()                                                  # nothing was launched
    assert fwd() == 0 and bwd() == 0 and hbwd() == 0 and bwd(dx_=None, dW_=None, db_=None, ws_=None, nbytes=0) == 0
    torch.cuda.synchronize()
    for t in (y, dx, dW, db):
        assert not t.any()


def test_autograd_surface_of_pointwise_linear(eng):
    from linetr_amd.train_ops import pointwise_linear
    c = LB.RELU_SURFACE
    x, W, b, g = LB.relu_surface_case()
    to_bcn = lambda a, C_: np.ascontiguousarray(a.reshape(c["B"], c["n"], C_).transpose(0, 2, 1))
    cf = LB.layer_closed_form(x, W, b, g, None, True)
    cf = LB.layer_closed_form(x, W, b, g, cf["y"], True)                        # the float64 mask
    yard = LB.torch_layer(x, W, b, g, torch.float32, relu=True)
    xt, Wt, bt = dev(to_bcn(x, c["K"])).requires_grad_(), dev(W[:, :, None]).requires_grad_(), dev(b).requires_grad_()
    with torch.enable_grad():
        y = pointwise_linear(xt, Wt, bt, relu=True)                              # Conv1d: [B, K, n] features, [N, K, 1] weight
        assert y.shape == (c["B"], c["N"], c["n"]) and y.grad_fn is not None
        y.backward(dev(to_bcn(g, c["N"])))
    assert xt.grad.shape == xt.shape and Wt.grad.shape == Wt.shape and bt.grad.shape == bt.shape
    rows_of = lambda t, C_: t.detach().transpose(1, 2).reshape(-1, C_).cpu().numpy()
    got = {"y": rows_of(y, c["N"]), "dx": rows_of(xt.grad, c["K"]), "dW": Wt.grad[:, :, 0].cpu().numpy(), "db": bt.grad.cpu().numpy()}
    check_bars(got, cf, yard, LAYER_KEYS, "pointwise_linear relu surface")
    # Linear: [rows, K] features, [N, K] weight, no bias, no activation; only the weight requires grad
    W2 = dev(W).requires_grad_()
    with torch.enable_grad():
        pointwise_linear(dev(x), W2).backward(dev(g))
    lin = LB.layer_closed_form(x, W, None, g)
    yard = LB.torch_layer(x, W, None, g, torch.float32)
    check_bars({"dW": W2.grad.cpu().numpy()}, lin, yard, ("dW",), "pointwise_linear linear surface")


def test_loss_backward_reaches_the_head(eng):
    """descriptor_loss(DescriptorHead(x)).backward() against the same graph in torch float64: features, weight and bias gradients"""
    import linetr_amd.evaluations as E
    from linetr_amd.train_ops import DescriptorHead
    W, b, x0, x1, assign, _, _ = LB.head_surface_case(np.float32)
    head = DescriptorHead.from_line_transformer({"final_proj.weight": torch.from_numpy(W), "final_proj.bias": torch.from_numpy(b)}).cuda()
    a0, a1 = dev(x0).requires_grad_(), dev(x1).requires_grad_()
    crit = E.descriptor_loss()
    with torch.enable_grad():
        pred = {"line_desc0": head(a0), "line_desc1": head(a1)}
        assert pred["line_desc0"].shape == a0.shape and pred["line_desc0"].grad_fn is not None
        loss = crit(pred, {"mat_assign_sublines": dev(assign)})[0]
        loss.backward()
    ref, ref_loss, V, _, _ = LB.torch_head_surface(torch.float64)
    yard = LB.torch_head_surface(torch.float32)[0]
    assert crit.last["count"] == V and abs(float(loss.detach()) - ref_loss) <= 1e-5
    got = {"x0": a0.grad, "x1": a1.grad, "W": head.final_proj.weight.grad, "b": head.final_proj.bias.grad}
    assert all(v is not None and v.shape == r.shape for v, r in zip(got.values(), ref.values()))
    check_bars({k: v.cpu().numpy() for k, v in got.items()}, ref, yard, tuple(ref), "descriptor_loss(DescriptorHead)")
    # frozen features: only the head's parameters get a gradient
    head.zero_grad(set_to_none=True)
    with torch.enable_grad():
        crit({"line_desc0": head(dev(x0)), "line_desc1": head(dev(x1))}, {"mat_assign_sublines": dev(assign)})[0].backward()
    assert torch.equal(head.final_proj.weight.grad, got["W"]) and torch.equal(head.final_proj.bias.grad, got["b"])


def test_directional_derivative_in_float32(eng):
    """gradcheck's idea at float32: for f = <c, head(x; W, b)> the central difference along a random direction of (x, W, b) against
    <gradient, direction>.  h = 2^-7.  The difference quotient carries the rounding of f (about 1e-7 per element of d, summed in
    float64 over 5 x 256 elements weighted by |c| ~ 1: some 4e-6, over 2 h: 3e-4) and h^2 / 6 times a third derivative of order
    |direction|^3 (a few 1e-4); the tolerance is 1e-2 of |gradient| |direction|, an order above both."""
    rows = 5
    rs = np.random.RandomState(3)
    x, W, b, c, _ = LB.normal_case(rows, 256, 256, seed=77)
    unit = lambda a: (a / np.sqrt((a * a).sum())).astype(np.float32)
    vx, vW, vb = unit(rs.standard_normal(x.shape)), unit(rs.standard_normal(W.shape)), unit(rs.standard_normal(b.shape))
    dx, dW, db = (t.cpu().double().numpy() for t in eng.head_backward(dev(x), dev(W), dev(b), dev(c)))
    analytic = (dx * vx).sum() + (dW * vW).sum() + (db * vb).sum()
    h = np.float32(2.0 ** -7)
    at = lambda p, v, s: dev((p + np.float32(s) * h * v).astype(np.float32))
    f = lambda s: (eng.head_forward(at(x, vx, s), at(W, vW, s), at(b, vb, s)).cpu().double().numpy() * c).sum()
    numeric = (f(1) - f(-1)) / (2.0 * float(h))
    scale = np.sqrt((dx ** 2).sum() + (dW ** 2).sum() + (db ** 2).sum()) * np.sqrt(3.0)
    print(f"linear_bwd directional: analytic {analytic:.6e}, numeric {numeric:.6e}, scale {scale:.3e}")
    assert abs(analytic - numeric) <= 1e-2 * scale
