"""GPU: the native HardNet criterion, value and gradient (linetr_hardnet_loss_grad, csrc/lt_hardnet.h; Engine.hardnet_step;
linetr_amd.evaluations.descriptor_loss(mining="hardnet")) against autograd through the reference with its HardNet switch flipped
(tests/golden/hardnet_loss.npz) and the float64 closed form that tests/test_hardnet_loss_cpu.py pins to it (tests/hardnet_reference.py).

The bar for a gradient is the project's own rule (loss_grad_reference.bar_of): 4 x the float32 autograd error of the SAME case
against float64 (the fixture's ref_f32_err; torch on the CPU through the restatement elsewhere), floored at two float32 spacings of
the case's largest gradient magnitude; the exact family must match bit for bit.  The bar for values (pos, neg, the scalars) is
val_step's rule: the reference's own float32 error on the fixture's data, doubled (2 x max(ref_f32_val_err, 2.4e-7)).  Measured on the
MI355X: profiles/hardnet_loss_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load
import val_step_reference as R
import hardnet_reference as H

pytestmark = pytest.mark.gpu
E_ARG = -1
VALUE_BAR = 2 * max(float(load("hardnet_loss")["ref_f32_val_err"]), R.FP32_SPACING)
SCALARS = ("loss", "hardest_positive", "hardest_negative")


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def fix():
    f = load("hardnet_loss")
    return {k: f[k] for k in f.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def step(eng, d0, d1, assign, upstream=None):
    res = eng.hardnet_step(dev(d0), dev(d1), assign=dev(assign), upstream=upstream, rows=True)
    assert res["grad0"].shape == d0.shape and res["grad1"].shape == d1.shape
    for k in ("grad0", "grad1", "row_pos", "row_neg", "row_arg"):
        res[k] = res[k].cpu().numpy()
    return res


def bits(res):
    return [np.float64(res[k]).tobytes() for k in SCALARS] + [res["count"], res["live"]]


def check_selection(res, cf, label):
    """the selection is the float64 closed form's; the values are within VALUE_BAR of it"""
    assert res["count"] == cf["V"] and res["live"] == cf["live"], label
    assert np.array_equal(res["row_arg"], cf["arg"]), label                   # integer-exact: anchors and the first index of each positive
    errs = {"row_pos": np.abs(res["row_pos"] - cf["pos"]).max(), "row_neg": np.abs(res["row_neg"] - cf["neg"]).max()}
    if cf["V"]:
        errs.update(hardest_positive=abs(res["hardest_positive"] - cf["hardest_positive"]),
                    hardest_negative=abs(res["hardest_negative"] - cf["hardest_negative"]), loss=abs(res["loss"] - cf["loss"]))
    print(f"hardnet values {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bar {VALUE_BAR:.3e})")
    assert all(v <= VALUE_BAR for v in errs.values()), (label, errs)


def check_bar(res, cf, yardstick, label):
    err, bar = H.max_err(res["grad0"], res["grad1"], cf), H.bar_of(yardstick, H.grad_max(cf))
    print(f"hardnet_loss {label}: err {err:.3e}, yardstick {yardstick:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
    assert err <= bar, (label, err, bar)


def test_fixture(eng, fix):
    d0, d1, assign = fix["desc0"], fix["desc1"], fix["assign"]
    res = step(eng, d0, d1, assign)
    cf = H.closed_form(d0, d1, assign)
    assert res["count"] == int(fix["V"]) and res["live"] == int(fix["live"])
    for k, ref in zip(SCALARS, ("loss", "hp", "hn")):
        assert abs(res[k] - float(fix[ref])) <= VALUE_BAR, (k, res[k], float(fix[ref]))
    check_selection(res, cf, "fixture B=3 n=40")
    pos, neg = H.reference_order({"pos": res["row_pos"].astype(np.float64), "neg": res["row_neg"].astype(np.float64), "arg": res["row_arg"]})
    assert np.abs(pos - fix["pos"]).max() <= VALUE_BAR and np.abs(neg - fix["neg"]).max() <= VALUE_BAR
    value_only = eng.hardnet_step(dev(d0), dev(d1), assign=dev(assign), need_grad=False)
    assert bits(res) == bits(value_only) and "grad0" not in value_only
    check_bar(res, {"grad0": fix["grad0_f64"], "grad1": fix["grad1_f64"]}, float(fix["ref_f32_err"]), "fixture B=3 n=40")


@pytest.mark.parametrize("B,n,extra", H.EDGE_CASES)
def test_tile_edges(eng, B, n, extra):
    d0, d1, assign = H.edge_case(B, n, extra)
    cf = H.closed_form(d0, d1, assign)
    res = step(eng, d0, d1, assign)
    label = f"B={B} n={n}" + (" extra positives" if extra else "")
    check_selection(res, cf, label)
    if n == 1:                                                               # one pair: anchors without a negative
        assert cf["V"] > 0 and res["loss"] == 0.0 and res["hardest_negative"] == 10000.0 and res["live"] == 0
        assert not res["grad0"].any() and not res["grad1"].any()
        return
    t0, t1 = H.torch_grads(d0, d1, assign, torch.float32)
    check_bar(res, cf, H.max_err(t0, t1, cf), label)


def exact_equal(res, cf):
    return all(np.array_equal(res[k], cf[k].astype(np.float32)) for k in ("grad0", "grad1"))


@pytest.mark.parametrize("variant", H.EXACT_VARIANTS)
def test_exact_family_is_bit_equal(eng, variant):
    d0, d1, assign = H.exact_case(variant)
    cf = H.closed_form(d0, d1, assign)
    res = step(eng, d0, d1, assign)
    assert res["count"] == cf["V"] and res["live"] == cf["live"] and res["loss"] == cf["loss"]
    assert res["hardest_positive"] == cf["hardest_positive"] and res["hardest_negative"] == cf["hardest_negative"]
    assert np.array_equal(res["row_arg"], cf["arg"]) and np.array_equal(res["row_pos"], cf["pos"]) and np.array_equal(res["row_neg"], cf["neg"])
    assert exact_equal(res, cf)
    assert res["grad0"].any() == bool(cf["live"]) and not np.signbit(res["grad0"][res["grad0"] == 0]).any()      # zeros are +0
    assert not np.signbit(res["grad1"][res["grad1"] == 0]).any()


def test_single_pair(eng):
    """n = 1 with a match: V counts both anchors, loss exactly 0, hardest_negative 10000, all gradients zero"""
    d0 = np.zeros((2, 256, 1), np.float32)
    d0[:, :16] = 0.25
    d1 = d0.copy()
    d1[:, :2] = -0.25
    assign = np.zeros((2, 2, 2), np.float32)
    assign[:, 0, 0] = 1.0
    res = step(eng, d0, d1, assign)
    assert res["count"] == 4 and res["live"] == 0 and res["loss"] == 0.0 and res["hardest_positive"] == 0.5
    assert res["hardest_negative"] == 10000.0 and not res["grad0"].any() and not res["grad1"].any()
    assert np.array_equal(res["row_neg"], np.full((2, 2), 10000.0, np.float32)) and not res["row_arg"].any()


def test_upstream(eng):
    d0, d1, assign = H.exact_case("combined")
    unit = step(eng, d0, d1, assign)                                         # d_upstream = NULL
    one = step(eng, d0, d1, assign, upstream=torch.tensor([1.0], device="cuda"))
    three = step(eng, d0, d1, assign, upstream=torch.tensor(3.0, device="cuda"))
    for k in ("grad0", "grad1"):
        assert np.array_equal(unit[k], one[k]) and np.array_equal(three[k], np.float32(3) * unit[k]) and unit[k].any()
    assert exact_equal(three, H.closed_form(d0, d1, assign, upstream=3.0))
    assert bits(three) == bits(unit)


def raw_call(L, d0, d1, assign, B, n, g0, g1, host, ws, *, n1=None, ws_bytes=None, d0p=True, up=None, rows=(None, None, None), hostp=True,
             wsp=True, asgp=True):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    return L.linetr_hardnet_loss_grad(None, d0.data_ptr() if d0p else None, n, d1.data_ptr(), n if n1 is None else n1,
                                      assign.data_ptr() if asgp else None, B, p(up), p(g0), p(g1), p(rows[0]), p(rows[1]), p(rows[2]),
                                      host.data_ptr() if hostp else None, host.numel(), ws.data_ptr() if wsp else None,
                                      ws.numel() if ws_bytes is None else ws_bytes, st)


def rows_of(x):
    """[B,256,n] -> device rows [B*n,256]"""
    return dev(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, 256))


def guarded(shape, dtype, fill):
    """a device tensor of `shape` inside a larger one filled with `fill`: (the whole, the view)"""
    count = int(np.prod(shape))
    whole = torch.full((count + 512,), fill, dtype=dtype, device="cuda")
    return whole, whole[256:256 + count].view(shape)


def test_outputs_fully_written_and_nothing_beyond(eng):
    from linetr_amd import _native as nat
    L = nat.lib()
    d0, d1, assign = H.exact_case("combined")
    B, n = d0.shape[0], d0.shape[2]
    cf = H.closed_form(d0, d1, assign)
    r0, r1, asg = rows_of(d0), rows_of(d1), dev(assign)
    need = L.linetr_hardnet_loss_grad_workspace_bytes(B, n)
    ws_whole = torch.full((need + 1024,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = ws_whole[512:512 + need]
    host = torch.zeros(40, dtype=torch.uint8).pin_memory()
    nan = float("nan")
    (w0, g0), (w1, g1) = guarded((B * n, 256), torch.float32, nan), guarded((B * n, 256), torch.float32, nan)
    (wp, rp), (wn, rn), (wa, ra) = guarded((B, 2 * n), torch.float32, nan), guarded((B, 2 * n), torch.float32, nan), guarded((B, 2 * n), torch.int32, -77)
    assert raw_call(L, r0, r1, asg, B, n, g0, g1, host, ws, rows=(rp, rn, ra)) == 0
    torch.cuda.synchronize()
    for whole, view in ((w0, g0), (w1, g1), (wp, rp), (wn, rn)):
        assert not torch.isnan(view).any() and torch.isnan(whole[:256]).all() and torch.isnan(whole[256 + view.numel():]).all()
    assert (wa[:256] == -77).all() and (wa[256 + ra.numel():] == -77).all()
    assert (ws_whole[:512] == 0x5A).all() and (ws_whole[512 + need:] == 0x5A).all()
    got0, got1 = (g.cpu().numpy().reshape(B, n, 256).transpose(0, 2, 1) for g in (g0, g1))
    assert np.array_equal(got0, cf["grad0"].astype(np.float32)) and np.array_equal(got1, cf["grad1"].astype(np.float32))
    assert np.array_equal(ra.cpu().numpy(), cf["arg"]) and np.array_equal(rp.cpu().numpy(), cf["pos"]) and np.array_equal(rn.cpu().numpy(), cf["neg"])
    idle0, idle1 = ~cf["G"].any(axis=2), ~cf["G"].any(axis=1)                 # rows of D / columns of D nothing selected
    assert idle0.sum() > B * n // 2 and idle1.sum() > B * n // 2
    assert not got0.transpose(0, 2, 1)[idle0].any() and not got1.transpose(0, 2, 1)[idle1].any()
    out = host.numpy()
    assert out[24:40].view(np.int64).tolist() == [cf["V"], cf["live"]] and out[:24].view(np.float64).tolist() == [cf[k] for k in SCALARS]
    # one side alone: the side asked for is the same, the other is left alone; both NULL: the value-only call, the scalars' bits
    only1 = torch.full_like(g1, nan)
    assert raw_call(L, r0, r1, asg, B, n, None, only1, host, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(only1, g1)
    before, scalars = g0.clone(), out.tobytes()
    host.zero_()
    assert raw_call(L, r0, r1, asg, B, n, None, None, host, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(g0, before) and host.numpy().tobytes() == scalars


def test_no_anchor(eng):
    B, n = 2, 5
    d = np.zeros((B, 256, n), np.float32)
    d[:, :4] = 0.5
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    assign[:, 0, 1] = 0.2                                                    # neither a match nor an unmatch
    res = step(eng, d, 0.5 * d, assign)
    assert res["count"] == 0 and res["live"] == 0 and all(np.isnan(res[k]) for k in SCALARS)
    assert not res["grad0"].any() and not res["grad1"].any() and (res["row_arg"] == -1).all() and (res["row_neg"] == -1).all()
    assign[:, np.arange(n), np.arange(n)] = 1                                # matches at distance 0: pos is not > 0
    res = step(eng, d, d, assign)
    assert res["count"] == 0 and np.isnan(res["loss"]) and not res["grad0"].any()
    from linetr_amd.evaluations import descriptor_loss
    crit = descriptor_loss(mining="hardnet")
    with pytest.raises(RuntimeError, match="stack expects a non-empty TensorList"), torch.enable_grad():
        crit({"line_desc0": dev(d).requires_grad_(), "line_desc1": dev(d)}, {"mat_assign_sublines": dev(assign)})
    with pytest.raises(RuntimeError, match="stack expects a non-empty TensorList"), torch.no_grad():
        crit({"line_desc0": dev(d), "line_desc1": dev(d)}, {"mat_assign_sublines": dev(assign)})


def test_deterministic(eng, fix):
    d0, d1, assign = dev(fix["desc0"]), dev(fix["desc1"]), dev(fix["assign"])
    runs = [eng.hardnet_step(d0, d1, assign=assign, rows=True) for _ in range(2)]
    big = [eng.hardnet_step(*(dev(x) for x in H.edge_case(2, 250)[:2]), assign=dev(H.edge_case(2, 250)[2])) for _ in range(2)]
    for a, b in ((runs[0], runs[1]), (big[0], big[1])):
        for k, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, b[k]), k
            else:
                assert np.array_equal(np.float64(v), np.float64(b[k]), equal_nan=True), k


def test_argument_errors(eng, fix):
    from linetr_amd import _native as nat
    L = nat.lib()
    B, n = 3, 40
    r0, r1, asg = rows_of(fix["desc0"]), rows_of(fix["desc1"]), dev(fix["assign"])
    ws = torch.empty(L.linetr_hardnet_loss_grad_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    host = torch.zeros(40, dtype=torch.uint8).pin_memory()
    g0, g1 = torch.full_like(r0, 7.0), torch.full_like(r1, 7.0)
    call = lambda *a, **k: raw_call(L, r0, r1, asg, *a, **k)
    assert call(B, n, g0, g1, host, ws, n1=n - 1) == E_ARG
    assert call(0, n, g0, g1, host, ws) == E_ARG and call(-1, n, g0, g1, host, ws) == E_ARG
    assert call(B, 0, g0, g1, host, ws) == E_ARG
    assert call(65536, n, g0, g1, host, ws) == E_ARG and call(B, 32769, g0, g1, host, ws) == E_ARG
    assert call(B, n, g0, g1, host, ws, d0p=False) == E_ARG and call(B, n, g0, g1, host, ws, asgp=False) == E_ARG
    assert call(B, n, g0, g1, host, ws, hostp=False) == E_ARG and call(B, n, g0, g1, host, ws, wsp=False) == E_ARG
    assert call(B, n, g0, g1, host, ws, ws_bytes=ws.numel() - 1) == E_ARG
    assert call(B, n, g0, g1, host[:39], ws) == E_ARG
    torch.cuda.synchronize()
    assert (g0 == 7.0).all() and (g1 == 7.0).all() and not host.numpy().any()          # nothing was launched
    with pytest.raises(nat.NativeError, match="error -1"):
        eng.hardnet_step(dev(fix["desc0"]), dev(fix["desc1"][:, :, :39]), assign=asg)
    with pytest.raises(ValueError, match="upstream"):
        eng.hardnet_step(dev(fix["desc0"]), dev(fix["desc1"]), assign=asg, upstream=torch.ones(2, device="cuda"))
    assert call(B, n, g0, g1, host, ws) == 0
    torch.cuda.synchronize()
    assert not (g0 == 7.0).any() and host.numpy().any()


def test_autograd_surface(eng, fix):
    """descriptor_loss(mining="hardnet") under autograd behind a DescriptorHead: final_proj.weight.grad against the torch restatement"""
    import linetr_amd.evaluations as E
    from linetr_amd.train_ops import DescriptorHead
    crit = E.descriptor_loss(mining="hardnet")
    d0, d1, assign = H.edge_case(3, 65)
    rs = np.random.RandomState(11)
    state = {"final_proj.weight": rs.standard_normal((256, 256, 1)) / 16.0, "final_proj.bias": 0.01 * rs.standard_normal(256)}

    def run(dtype, device, native):
        head = DescriptorHead() if native else None
        w = torch.tensor(state["final_proj.weight"], dtype=dtype, device=device, requires_grad=True)
        b = torch.tensor(state["final_proj.bias"], dtype=dtype, device=device, requires_grad=True)
        x0, x1, asg = (torch.tensor(x, dtype=dtype, device=device) for x in (d0, d1, assign))
        with torch.enable_grad():
            if native:
                head.final_proj.weight.data.copy_(w.detach())
                head.final_proj.bias.data.copy_(b.detach())
                head = head.cuda()
                out = [head(x) for x in (x0, x1)]
                res = crit({"line_desc0": out[0], "line_desc1": out[1]}, {"mat_assign_sublines": asg})
                res[0].backward()
                return res, head.final_proj.weight.grad.detach().double().cpu().numpy().reshape(256, 256), out
            out = [F.normalize(F.conv1d(x, w, b), p=2, dim=1) for x in (x0, x1)]
            res = H.torch_criterion(out[0], out[1], asg)
            res[0].backward()
            return res, w.grad.double().numpy().reshape(256, 256), out

    (loss, hp, hn), got, _ = run(torch.float32, "cuda", True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.grad_fn is not None
    assert hp.grad_fn is None and hn.grad_fn is None and not hp.requires_grad and not hn.requires_grad
    ref_out, ref, descs = run(torch.float64, "cpu", False)
    _, f32, _ = run(torch.float32, "cpu", False)
    a, b = (x.detach().numpy() for x in descs)
    assert H.selection_gap(a, b, assign) >= R.MIN_MARGIN
    assert ref_out[3] == crit.last["count"] and abs(float(loss.detach()) - float(ref_out[0].detach())) <= VALUE_BAR
    err, bar = np.abs(got - ref).max(), H.bar_of(np.abs(f32 - ref).max(), np.abs(ref).max())
    print(f"hardnet_loss autograd final_proj.weight.grad: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
    assert err <= bar
    # one side alone requires grad: the other gets none; an upstream factor scales the gradient
    x, y, asg = dev(fix["desc0"]).requires_grad_(), dev(fix["desc1"]), dev(fix["assign"])
    with torch.enable_grad():
        (2 * crit({"line_desc0": x, "line_desc1": y}, {"mat_assign_sublines": asg})[0]).backward()
    assert y.grad is None and torch.equal(x.grad, 2 * eng.hardnet_step(x, y, assign=asg)["grad0"])


def test_no_grad_path_is_the_value_only_call(eng, fix):
    import linetr_amd.evaluations as E
    crit = E.descriptor_loss(mining="hardnet")
    d0, d1, target = dev(fix["desc0"]), dev(fix["desc1"]), {"mat_assign_sublines": dev(fix["assign"])}
    val = eng.hardnet_step(d0, d1, assign=target["mat_assign_sublines"], need_grad=False)
    want = [torch.tensor(val[k], dtype=torch.float32, device=d0.device) for k in SCALARS]
    with torch.enable_grad():
        plain = crit({"line_desc0": d0, "line_desc1": d1}, target)                       # nothing requires grad
        with torch.no_grad():
            off = crit({"line_desc0": d0.clone().requires_grad_(), "line_desc1": d1}, target)
        assert "grad0" not in crit.last and crit.last["count"] == int(fix["V"])
        on = crit({"line_desc0": d0.clone().requires_grad_(), "line_desc1": d1}, target)
    for out in (plain, off):
        for t, w in zip(out, want):
            assert t.grad_fn is None and not t.requires_grad and t.dim() == 0 and torch.equal(t, w)
    assert on[0].grad_fn is not None and all(torch.equal(t, w) for t, w in zip(on, want))


def test_training_step(eng):
    """one step of TrainableLineTransformer on two views at B = 2 under the HardNet criterion with the native Adam"""
    import keyline_reference as KR
    import linetr_amd.evaluations as E
    from linetr_amd.optim import Adam
    from linetr_amd.train_ops import TrainableLineTransformer
    sd, v0, v1, assign = KR.loss_case()
    mod = TrainableLineTransformer({})
    mod.load_state_dict(KR.tensors(sd), strict=True)
    mod = mod.cuda().train()
    crit = E.descriptor_loss(mining="hardnet")
    params = list(mod.parameters())
    opt = Adam(params, lr=1e-3)
    before = [p.detach().clone() for p in params]
    a, b = KR.data_tensors(v0, torch.float32, "cuda"), KR.data_tensors(v1, torch.float32, "cuda")
    with torch.enable_grad():
        loss = crit({"line_desc0": mod(a)["line_desc"], "line_desc1": mod(b)["line_desc"]}, {"mat_assign_sublines": dev(assign)})[0]
        loss.backward()
    assert assign.shape[0] == 2 and len(params) == 153 and np.isfinite(float(loss.detach())) and crit.last["count"] > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert sum(bool(p.grad.any()) for p in params) > 100
    opt.step()
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert sum(not torch.equal(p, q) for p, q in zip(params, before)) > 100


def test_default_mining_is_unchanged(eng):
    """descriptor_loss() without arguments still returns loss_step's bits on the semi-hard fixture"""
    import linetr_amd.evaluations as E
    g = load("val_step")
    d0, d1, asg = dev(g["desc0"]), dev(g["desc1"]), dev(g["assign"])
    want = eng.loss_step(d0, d1, assign=asg)
    for crit in (E.descriptor_loss(), E.descriptor_loss(mining="semi-hard")):
        x = d0.clone().requires_grad_()
        with torch.enable_grad():
            out = crit({"line_desc0": x, "line_desc1": d1}, {"mat_assign_sublines": asg})
            out[0].backward()
        for t, k in zip(out, SCALARS):
            assert torch.equal(t, torch.tensor(want[k], dtype=torch.float32, device="cuda")), k
        assert torch.equal(x.grad, want["grad0"]) and crit.last["count"] == want["count"]
        with torch.no_grad():
            off = crit({"line_desc0": d0, "line_desc1": d1}, {"mat_assign_sublines": asg})
        assert all(torch.equal(t, torch.tensor(want[k], dtype=torch.float32, device="cuda")) for t, k in zip(off, SCALARS))
