"""GPU: the native gradient of the triplet criterion (linetr_desc_loss_grad, csrc/lt_lossgrad.h; Engine.loss_step; the autograd-aware
linetr_amd.evaluations.descriptor_loss) against autograd through the reference (tests/golden/loss_grad.npz) and the float64 closed
form that tests/test_loss_grad_cpu.py pins to it (tests/loss_grad_reference.py).

The bar for a gradient is 4 x the float32 autograd error of the SAME case against float64 (the fixture's ref_f32_err; torch on the CPU
through the restatement elsewhere), floored at two float32 spacings of the case's largest gradient magnitude; the exact family must
match bit for bit.  Measured on the MI355X: profiles/loss_grad_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load
import val_step_reference as R
import loss_grad_reference as LG

pytestmark = pytest.mark.gpu
E_ARG = -1


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def fix():
    g, f = load("val_step"), load("loss_grad")
    return {**{k: g[k] for k in g.files}, **{k: f[k] for k in f.files}}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def step(eng, d0, d1, assign, upstream=None):
    res = eng.loss_step(dev(d0), dev(d1), assign=dev(assign), upstream=upstream)
    assert res["grad0"].shape == d0.shape and res["grad1"].shape == d1.shape
    res["grad0"], res["grad1"] = res["grad0"].cpu().numpy(), res["grad1"].cpu().numpy()
    return res


def check_bar(res, cf, yardstick, label):
    err, bar = LG.max_err(res["grad0"], res["grad1"], cf), LG.bar_of(yardstick, LG.grad_max(cf))
    print(f"loss_grad {label}: err {err:.3e}, yardstick {yardstick:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
    assert err <= bar, (label, err, bar)


def test_fixture(eng, fix):
    d0, d1, assign = fix["desc0"], fix["desc1"], fix["assign"]
    res = step(eng, d0, d1, assign)
    assert res["count"] == int(fix["V"])
    val = eng.val_step(dev(d0), dev(d1), assign=dev(assign))
    for k in ("loss", "hardest_positive", "hardest_negative"):
        assert np.float64(res[k]).tobytes() == np.float64(val[k]).tobytes(), k
    assert res["count"] == val["count"]
    cf = {"grad0": fix["grad0_f64"], "grad1": fix["grad1_f64"]}
    check_bar(res, cf, float(fix["ref_f32_err"]), "fixture B=3 n=40")


@pytest.mark.parametrize("B,n", LG.EDGE_CASES)
def test_tile_edges(eng, B, n):
    d0, d1, assign = LG.edge_case(B, n)
    cf = LG.closed_form(d0, d1, assign)
    res = step(eng, d0, d1, assign)
    assert res["count"] == cf["V"]
    if n == 1:
        assert cf["V"] == 0 and not res["grad0"].any() and not res["grad1"].any() and np.isnan(res["loss"])
        return
    val = eng.val_step(dev(d0), dev(d1), assign=dev(assign))
    assert np.float64(res["loss"]).tobytes() == np.float64(val["loss"]).tobytes()
    t0, t1 = LG.torch_grads(d0, d1, assign, torch.float32)
    check_bar(res, cf, LG.max_err(t0, t1, cf), f"B={B} n={n}")


def exact_equal(res, cf):
    return all(np.array_equal(res[k], cf[k].astype(np.float32)) for k in ("grad0", "grad1"))


@pytest.mark.parametrize("variant", LG.EXACT_VARIANTS)
def test_exact_family_is_bit_equal(eng, variant):
    d0, d1, assign = LG.exact_case(variant)
    cf = LG.closed_form(d0, d1, assign)
    res = step(eng, d0, d1, assign)
    assert res["count"] == cf["V"] and res["loss"] == cf["loss"]
    assert exact_equal(res, cf)
    assert not np.signbit(res["grad0"][res["grad0"] == 0]).any()             # zeros are +0


def test_upstream(eng):
    d0, d1, assign = LG.exact_case("combined")
    unit = step(eng, d0, d1, assign)                                         # d_upstream = NULL
    one = step(eng, d0, d1, assign, upstream=torch.tensor([1.0], device="cuda"))
    three = step(eng, d0, d1, assign, upstream=torch.tensor(3.0, device="cuda"))
    for k in ("grad0", "grad1"):
        assert np.array_equal(unit[k], one[k]) and np.array_equal(three[k], np.float32(3) * unit[k]) and unit[k].any()
    assert exact_equal(three, LG.closed_form(d0, d1, assign, upstream=3.0))
    assert three["loss"] == unit["loss"]


def raw_call(L, d0, d1, assign, B, n, g0, g1, host, ws, *, n1=None, ws_bytes=None, d0p=True, up=None, stream=None):
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    return L.linetr_desc_loss_grad(None, d0.data_ptr() if d0p else None, n, d1.data_ptr(), n if n1 is None else n1, assign.data_ptr(), B,
                                   up.data_ptr() if up is not None else None, g0.data_ptr() if g0 is not None else None,
                                   g1.data_ptr() if g1 is not None else None, host.data_ptr(), host.numel(), ws.data_ptr(),
                                   ws.numel() if ws_bytes is None else ws_bytes, st)


def rows_of(x):
    """[B,256,n] -> device rows [B*n,256]"""
    return dev(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, 256))


def test_outputs_fully_written(eng):
    from linetr_amd import _native as nat
    L = nat.lib()
    d0, d1, assign = LG.exact_case("combined")
    B, n = d0.shape[0], d0.shape[2]
    cf = LG.closed_form(d0, d1, assign)
    r0, r1, asg = rows_of(d0), rows_of(d1), dev(assign)
    ws = torch.empty(L.linetr_desc_loss_grad_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    host = torch.zeros(32, dtype=torch.uint8).pin_memory()
    g0, g1 = torch.full_like(r0, float("nan")), torch.full_like(r1, float("nan"))
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host, ws) == 0
    torch.cuda.synchronize()
    got0, got1 = (g.cpu().numpy().reshape(B, n, 256).transpose(0, 2, 1) for g in (g0, g1))
    assert not np.isnan(got0).any() and not np.isnan(got1).any()
    assert np.array_equal(got0, cf["grad0"].astype(np.float32)) and np.array_equal(got1, cf["grad1"].astype(np.float32))
    idle0, idle1 = ~cf["G"].any(axis=2), ~cf["G"].any(axis=1)                 # rows of D / columns of D no anchor selected
    assert idle0.sum() > B * n // 2 and idle1.sum() > B * n // 2
    assert not got0.transpose(0, 2, 1)[idle0].any() and not got1.transpose(0, 2, 1)[idle1].any()
    assert host.numpy()[24:32].view(np.int64)[0] == cf["V"] and host.numpy()[:8].view(np.float64)[0] == cf["loss"]
    # one side alone: the side asked for is the same
    only1 = torch.full_like(r1, float("nan"))
    assert raw_call(L, r0, r1, asg, B, n, None, only1, host, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(only1, g1)
    before = g0.clone()
    assert raw_call(L, r0, r1, asg, B, n, g0, None, host, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(g0, before)


def test_no_surviving_anchor(eng):
    B, n = 2, 5
    d = np.zeros((B, 256, n), np.float32)
    d[:, :4] = 0.5
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    assign[:, np.arange(n), np.arange(n)] = 1
    res = eng.loss_step(dev(d), dev(d), assign=dev(assign))
    assert res["count"] == 0 and np.isnan(res["loss"]) and not res["grad0"].any() and not res["grad1"].any()
    from linetr_amd.evaluations import descriptor_loss
    with pytest.raises(RuntimeError, match="no anchor has a semi-hard negative"), torch.enable_grad():
        descriptor_loss()({"line_desc0": dev(d).requires_grad_(), "line_desc1": dev(d)}, {"mat_assign_sublines": dev(assign)})


def test_deterministic_and_stream_independent(eng, fix):
    d0, d1, assign = dev(fix["desc0"]), dev(fix["desc1"]), dev(fix["assign"])
    runs = [eng.loss_step(d0, d1, assign=assign) for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(eng.loss_step(d0, d1, assign=assign))
    side.synchronize()
    for r in runs[1:]:
        for k, v in runs[0].items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, r[k]), k
            else:
                assert np.array_equal(np.float64(v), np.float64(r[k]), equal_nan=True), k


def test_layouts_and_lmatches(eng, fix):
    d0, d1, assign = dev(fix["desc0"]), dev(fix["desc1"]), dev(fix["assign"])
    a = eng.loss_step(d0, d1, assign=assign)
    assert a["grad0"].shape == d0.shape
    rows0, rows1 = d0.transpose(1, 2).contiguous(), d1.transpose(1, 2).contiguous()
    b = eng.loss_step(rows0.view(-1, 256), rows1.view(-1, 256), assign=assign)
    assert b["grad0"].shape == (3 * 40, 256) and b["grad0"].is_contiguous()
    assert torch.equal(b["grad0"].view(3, 40, 256).transpose(1, 2), a["grad0"]) and torch.equal(b["grad1"].view(3, 40, 256).transpose(1, 2), a["grad1"])
    c = eng.loss_step(rows0.transpose(1, 2), rows1.transpose(1, 2), assign=assign)          # the transposed view this build's forward returns
    assert torch.equal(c["grad0"], a["grad0"]) and c["loss"] == a["loss"]
    ones = (fix["assign"][:, :-1, :-1] == 1.0)
    lm = np.full((3, 60, 2), -1, np.int32)
    for i in range(3):
        r, cc = np.nonzero(ones[i])
        lm[i, :len(r), 0], lm[i, :len(r), 1] = r, cc
    only_ones = np.zeros_like(fix["assign"])
    only_ones[:, :-1, :-1][ones] = 1.0
    x, y = eng.loss_step(d0, d1, lmatches=dev(lm)), eng.loss_step(d0, d1, assign=dev(only_ones))
    assert x["count"] == y["count"] and x["loss"] == y["loss"] and torch.equal(x["grad0"], y["grad0"]) and torch.equal(x["grad1"], y["grad1"])


def graph_case(dtype, device):
    """desc = normalize(W @ x) for both images, from clustered inputs of 24 channels: (W, x0, x1, assign)"""
    d0, d1, assign = LG.edge_case(3, 65)
    rs = np.random.RandomState(11)
    P = rs.standard_normal((24, 256)) / 16.0                        # inputs: a fixed projection of the clustered descriptors
    W = rs.standard_normal((256, 24))
    t = lambda a: torch.tensor(a, dtype=dtype, device=device)
    return t(W).requires_grad_(), t(np.einsum("cd,bdn->bcn", P, d0)), t(np.einsum("cd,bdn->bcn", P, d1)), t(assign)


def test_autograd_surface(eng, fix):
    import linetr_amd.evaluations as E
    crit = E.descriptor_loss()
    W, x0, x1, assign = graph_case(torch.float32, "cuda")
    with torch.enable_grad():
        pred = {"line_desc0": F.normalize(W @ x0, dim=1), "line_desc1": F.normalize(W @ x1, dim=1)}
        loss, hp, hn = crit(pred, {"mat_assign_sublines": assign})
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == W.device and loss.grad_fn is not None
        assert hp.grad_fn is None and hn.grad_fn is None and not hp.requires_grad and not hn.requires_grad
        loss.backward()
        once = W.grad.clone()
        W.grad = None
        pred = {"line_desc0": F.normalize(W @ x0, dim=1), "line_desc1": F.normalize(W @ x1, dim=1)}
        (2 * crit(pred, {"mat_assign_sublines": assign})[0]).backward()
    assert torch.equal(W.grad, 2 * once)
    # the same graph through the float64 restatement on the CPU; the yardstick: the same in float32
    grads = {}
    for dtype in (torch.float64, torch.float32):
        Wc, c0, c1, asg = graph_case(dtype, "cpu")
        with torch.enable_grad():
            d0c, d1c = F.normalize(Wc @ c0, dim=1), F.normalize(Wc @ c1, dim=1)
            if dtype == torch.float64:
                assert R.margins(d0c.detach().numpy(), d1c.detach().numpy(), asg.numpy(), LG.NN_THRESH) >= R.MIN_MARGIN
                assert LG.selection_gap(d0c.detach().numpy(), d1c.detach().numpy(), asg.numpy()) >= R.MIN_MARGIN
            out = LG.torch_criterion(d0c, d1c, asg)
            out[0].backward()
        grads[dtype] = Wc.grad.double().numpy()
        if dtype == torch.float64:
            assert out[3] == crit.last["count"] and abs(float(loss.detach()) - float(out[0].detach())) <= 1e-6
    ref = grads[torch.float64]
    err, bar = np.abs(once.cpu().double().numpy() - ref).max(), LG.bar_of(np.abs(grads[torch.float32] - ref).max(), np.abs(ref).max())
    print(f"loss_grad autograd W.grad: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
    assert err <= bar
    # one side alone requires grad: the other gets none
    a, b = dev(fix["desc0"]).requires_grad_(), dev(fix["desc1"])
    with torch.enable_grad():
        crit({"line_desc0": a, "line_desc1": b}, {"mat_assign_sublines": dev(fix["assign"])})[0].backward()
    assert b.grad is None and torch.equal(a.grad, eng.loss_step(a, b, assign=dev(fix["assign"]))["grad0"])


def test_no_grad_paths_are_todays(eng, fix):
    import linetr_amd.evaluations as E
    crit = E.descriptor_loss()
    d0, d1, target = dev(fix["desc0"]), dev(fix["desc1"]), {"mat_assign_sublines": dev(fix["assign"])}
    val = eng.val_step(d0, d1, assign=target["mat_assign_sublines"])
    want = [torch.tensor(val[k], dtype=torch.float32, device=d0.device) for k in ("loss", "hardest_positive", "hardest_negative")]
    with torch.enable_grad():
        plain = crit({"line_desc0": d0, "line_desc1": d1}, target)                       # nothing requires grad
        with torch.no_grad():
            off = crit({"line_desc0": d0.clone().requires_grad_(), "line_desc1": d1}, target)
        on = crit({"line_desc0": d0.clone().requires_grad_(), "line_desc1": d1}, target)
    for out in (plain, off):
        for t, w in zip(out, want):
            assert t.grad_fn is None and not t.requires_grad and t.dim() == 0 and torch.equal(t, w)
    assert on[0].grad_fn is not None and all(torch.equal(t, w) for t, w in zip(on, want))


def test_argument_errors(eng, fix):
    from linetr_amd import _native as nat
    L = nat.lib()
    B, n = 3, 40
    r0, r1, asg = rows_of(fix["desc0"]), rows_of(fix["desc1"]), dev(fix["assign"])
    ws = torch.empty(L.linetr_desc_loss_grad_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    host = torch.zeros(32, dtype=torch.uint8).pin_memory()
    g0, g1 = torch.full_like(r0, 7.0), torch.full_like(r1, 7.0)
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host, ws, n1=n - 1) == E_ARG
    assert raw_call(L, r0, r1, asg, 0, n, g0, g1, host, ws) == E_ARG
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host, ws, d0p=False) == E_ARG
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host, ws, ws_bytes=ws.numel() - 1) == E_ARG
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host[:31], ws) == E_ARG
    torch.cuda.synchronize()
    assert (g0 == 7.0).all() and (g1 == 7.0).all() and not host.numpy().any()          # nothing was launched
    with pytest.raises(nat.NativeError, match="error -1"):
        eng.loss_step(dev(fix["desc0"]), dev(fix["desc1"][:, :, :39]), assign=asg)
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host, ws) == 0
    torch.cuda.synchronize()
    assert not (g0 == 7.0).any() and host.numpy().any()
