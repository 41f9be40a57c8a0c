"""GPU: the native Adam step and the gradient norm that can feed it (csrc/lt_adam.h; linetr_adam_step, linetr_grad_norm; Engine.adam_step /
grad_norm; linetr_amd.optim.Adam) against the float64 restatement of tests/adam_cases.py, which tests/test_adam_cpu.py pins to
torch.optim.Adam in float64.

The bar of an output tensor is 8 x max(error of torch.optim.Adam(foreach=False) in float32 on the CPU on the SAME case against float64,
2^-23 max |float64|), for p', m', v' and for the update p' - p; an all-zero float64 result must be met exactly; the exact properties and
every value outside a tensor must hold bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import adam_cases as AC
import keyline_reference as KR

pytestmark = pytest.mark.gpu
E_ARG = -1
SIZES = AC.ragged_sizes(AC.CHUNK, AC.THREADS)
TOTAL = sum(SIZES)


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def nat():
    from linetr_amd import _native
    return _native


@pytest.fixture(scope="module")
def L(nat):
    return nat.lib()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the cases' arrays are read-only)


def check(label, got, case, scale=None, refs=None):
    ref64, ref32 = refs if refs is not None else AC.refs_of(case, scale)
    rows = AC.ratios(got, case["p"], ref64, ref32)
    print(f"adam {label}: " + ", ".join(f"{k} {AC.ratio(e, b):.3f}" for k, e, b in rows) + "  (error / bar)")
    assert not AC.failures(rows), (label, AC.failures(rows))
    return rows


def step_kwargs(case):
    h = case["hyper"]
    return dict(lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], decoupled=h["decoupled_weight_decay"])


def split(flat, sizes):
    """device tensors of `sizes` elements each, cut out of the flat array"""
    out, at = [], 0
    for n in sizes:
        out.append(dev(flat[at:at + n]))
        at += n
    return out


def joined(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


def run_plain(eng, case, sizes, scale=None, **override):
    """the case cut into ordinary (allocator-aligned) tensors of `sizes`, one call: {p, m, v} flat"""
    t = {k: split(case[k], sizes) for k in "pgmv"}
    eng.adam_step(t["p"], t["g"], t["m"], t["v"], [case["step"]] * len(sizes), grad_scale=scale, **{**step_kwargs(case), **override})
    return {k: joined(t[k]) for k in "pmv"}


# ---- edges: one ragged table -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", AC.FAMILIES)
def test_ragged_table(eng, family):
    """tensors of 0 .. 2 chunks + 5 elements in ONE call, each of p, g, m, v carved out of a flat buffer between sentinels: 16-byte aligned,
    at float offsets 1, 2, 3, and with the alignments mixed inside one tensor"""
    for step in AC.steps_of(family):
        case = AC.make_case(family, step, TOTAL)
        refs = AC.refs(family, step, TOTAL)
        outs = {}
        for label, offsets in AC.ALIGNMENTS.items():
            outs[label] = AC.run_ragged(eng, case, SIZES, offsets)
            check(f"{family} step {step} {label}", outs[label], case, refs=refs)
        for label, out in outs.items():                     # one arithmetic on both paths: the vector and the scalar one give the same bits
            assert all(out[k].tobytes() == outs["aligned"][k].tobytes() for k in "pmv"), (family, step, label)


def test_many_tensors(eng):
    """1 000 tensors of 1 .. 9 elements in one call: more entries than any fixed-size search or table a kernel might assume"""
    sizes = [i % 9 + 1 for i in range(1000)]
    case = AC.make_case("wd", 10, sum(sizes))
    out = AC.run_ragged(eng, case, sizes, {"p": (0, 1, 2, 3), "g": (0, 1, 2, 3), "m": (0, 1, 2, 3), "v": (0, 1, 2, 3)})
    check("1000 tensors", out, case, refs=AC.refs("wd", 10, sum(sizes)))
    assert all(out[k].tobytes() == run_plain(eng, case, sizes)[k].tobytes() for k in "pmv")


def test_model_shapes_three_steps(eng):
    """the model's own 153 shapes for 3 steps with seeded gradients, each step against the float64 restatement started from the device's
    own float32 state of the step before: one-step errors, so the bar applies as it is"""
    shapes = AC.model_shapes()
    sizes = [int(np.prod(s)) for s in shapes]
    rs = AC._rs("model shapes")
    total = sum(sizes)
    assert total == 5683776
    state = {"p": split((0.05 * rs.standard_normal(total)).astype(np.float32), sizes),
             "m": [torch.zeros(n, device="cuda") for n in sizes], "v": [torch.zeros(n, device="cuda") for n in sizes]}
    hyper = dict(lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-4, decoupled_weight_decay=False)
    for step in (1, 2, 3):
        g = (rs.standard_normal(total) * 10.0 ** rs.uniform(-6, 0, total)).astype(np.float32)
        case = {"step": step, "hyper": hyper, "g": g, **{k: joined(state[k]) for k in "pmv"}}
        eng.adam_step(state["p"], split(g, sizes), state["m"], state["v"], [step] * len(sizes), **step_kwargs(case))
        check(f"153 model tensors, step {step}", {k: joined(state[k]) for k in "pmv"}, case)


# ---- exact properties --------------------------------------------------------------------------------------------------------------

def test_one_call_equals_one_call_per_tensor(eng):
    case = AC.make_case("wd", 10, TOTAL)
    together = run_plain(eng, case, SIZES)
    t = {k: split(case[k], SIZES) for k in "pgmv"}
    for i in range(len(SIZES)):
        eng.adam_step([t["p"][i]], [t["g"][i]], [t["m"][i]], [t["v"][i]], [10], **step_kwargs(case))
    for k in "pmv":
        assert joined(t[k]).tobytes() == together[k].tobytes(), k
    again = run_plain(eng, case, SIZES)
    for k in "pmv":
        assert again[k].tobytes() == together[k].tobytes(), k


def test_grad_scale_is_a_rounded_product(eng):
    case = AC.make_case("model", 10, TOTAL)
    plain = run_plain(eng, case, SIZES)
    one = run_plain(eng, case, SIZES, scale=torch.ones(1, device="cuda"))
    for k in "pmv":
        assert one[k].tobytes() == plain[k].tobytes(), k
    s = np.float32(0.3137)
    scaled = run_plain(eng, case, SIZES, scale=dev(np.array([s])))
    pre = dict(case, g=s * case["g"])
    assert pre["g"].dtype == np.float32
    want = run_plain(eng, pre, SIZES)
    for k in "pmv":
        assert scaled[k].tobytes() == want[k].tobytes(), k
    check("grad scale 0.3137", scaled, case, scale=s)


def test_no_weight_decay_ignores_decoupled(eng):
    case = AC.make_case("model", 2, TOTAL)
    a, b = run_plain(eng, case, SIZES, decoupled=False), run_plain(eng, case, SIZES, decoupled=True)
    for k in "pmv":
        assert a[k].tobytes() == b[k].tobytes(), k


def test_zero_lr_and_zero_inputs(eng):
    case = AC.make_case("model", 10, TOTAL)
    out = run_plain(eng, case, SIZES, lr=0.0)
    assert out["p"].tobytes() == case["p"].tobytes()
    assert (out["m"] != case["m"]).mean() > 0.9 and (out["v"] != case["v"]).mean() > 0.9
    for step in AC.STEPS:
        case = AC.make_case("zeros", step, TOTAL)
        out = run_plain(eng, case, SIZES)
        for k in "pmv":
            assert out[k].tobytes() == case[k].tobytes(), (step, k)           # 0 / (0 + eps) = 0: no NaN


def test_one_nan_stays_where_it_is(eng):
    case = AC.make_case("wd", 10, TOTAL)
    clean = run_plain(eng, case, SIZES)
    at = sum(SIZES[:-2]) + 4097                              # inside the second chunk of a two-chunk tensor
    g = case["g"].copy()
    g[at] = np.nan
    out = run_plain(eng, dict(case, g=g), SIZES)
    for k in "pmv":
        assert np.isnan(out[k][at]), k
        rest = np.arange(TOTAL) != at
        assert out[k][rest].tobytes() == clean[k][rest].tobytes(), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_step_refusals(L, nat):
    n = 70
    t = {k: [torch.full((n,), 7.0, device="cuda"), torch.full((3,), 7.0, device="cuda")] for k in "pgmv"}
    ws = torch.zeros(int(L.linetr_adam_workspace_bytes(2, n + 3)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0 and L.linetr_adam_workspace_bytes(0, 1) == 0 and L.linetr_adam_workspace_bytes(65537, 1) == 0
    assert L.linetr_adam_workspace_bytes(1, -1) == 0
    good_hyper = dict(betas=AC.BETAS, eps=AC.EPS, weight_decay=0.0, lr=AC.LR, decoupled_weight_decay=False)
    byte = lambda tensor, off: tensor.data_ptr() + off

    def call(edit=None, hyper=None, n_tensors=2, table=True, hyp=True, wsp=ws.data_ptr(), ws_bytes=ws.numel(), scale=None):
        tab = AC.table_of(nat, t, step_size=1e-3, bc2_sqrt=0.5)
        if edit:
            edit(tab)
        h = AC.hyper_of(nat, {**good_hyper, **(hyper or {})})
        return L.linetr_adam_step(None, tab.ctypes.data if table else None, n_tensors, C.byref(h) if hyp else None, scale, wsp, ws_bytes, AC.stream())

    def field(i, key, value):
        return lambda tab: tab[key].__setitem__(i, 0 if value is None else value)

    nan, inf = float("nan"), float("inf")
    refused = {"null table": call(table=False), "null hyper": call(hyp=False), "no tensors": call(n_tensors=0), "negative count": call(n_tensors=-1),
               "too many tensors": call(n_tensors=65537), "n < 0": call(field(1, "n", -1))}
    for key in "pgmv":
        refused[f"null {key}"] = call(field(0, key, None))
        refused[f"misaligned {key}"] = call(field(1, key, byte(t[key][1], 2)))
    for a, b in (("p", "g"), ("p", "m"), ("p", "v"), ("g", "m"), ("g", "v"), ("m", "v")):
        refused[f"{a} == {b}"] = call(field(0, a, t[b][0].data_ptr()))
    for i, name in enumerate(("beta1", "beta2")):
        for bad in (1.0, -0.1, 1.5, nan):
            betas = list(AC.BETAS)
            betas[i] = bad
            refused[f"{name} {bad}"] = call(hyper={"betas": tuple(betas)})
    for bad in (-1.0, inf, nan):
        refused[f"eps {bad}"] = call(hyper={"eps": bad})
        refused[f"weight_decay {bad}"] = call(hyper={"weight_decay": bad})
    for bad in (inf, -inf, nan):
        refused[f"step_size {bad}"] = call(field(1, "step_size", bad))
    for bad in (0.0, -0.5, 1.5, nan, inf):
        refused[f"bc2_sqrt {bad}"] = call(field(0, "bc2_sqrt", bad))
    refused["null workspace"] = call(wsp=None)
    refused["misaligned workspace"] = call(wsp=ws.data_ptr() + 16, ws_bytes=ws.numel() - 16)
    refused["short workspace"] = call(ws_bytes=ws.numel() - 1)
    refused["misaligned scale"] = call(scale=byte(t["p"][0], 2))
    assert all(code == E_ARG for code in refused.values()), {k: v for k, v in refused.items() if v != E_ARG}
    assert L.linetr_last_error()
    # a table of no elements at all is no error and launches nothing; n = 0 entries may carry any pointers
    assert call(lambda tab: tab["n"].fill(0)) == 0
    torch.cuda.synchronize()
    for key in "pgmv":
        for tensor in t[key]:
            assert (tensor == 7.0).all(), key
    assert not ws.any()
    assert call() == 0                                       # the unedited call is accepted
    torch.cuda.synchronize()
    assert not (t["p"][0] == 7.0).any() and (t["g"][0] == 7.0).all()


def test_grad_norm_refusals(L, nat):
    g = [torch.full((70,), 7.0, device="cuda"), torch.full((3,), 7.0, device="cuda")]
    out = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    scale = torch.full((4,), 7.0, device="cuda")
    ws = torch.zeros(int(L.linetr_grad_norm_workspace_bytes(2, 73)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > L.linetr_adam_workspace_bytes(2, 73) > 0 and L.linetr_grad_norm_workspace_bytes(0, 1) == 0

    def call(edit=None, n_tensors=2, table=True, max_norm=1.0, norm=out.data_ptr(), sc=scale.data_ptr(), wsp=ws.data_ptr(), ws_bytes=ws.numel()):
        tab = AC.table_of(nat, {"g": g})
        if edit:
            edit(tab)
        return L.linetr_grad_norm(None, tab.ctypes.data if table else None, n_tensors, max_norm, norm, sc, wsp, ws_bytes, AC.stream())

    refused = {"null table": call(table=False), "no tensors": call(n_tensors=0), "too many tensors": call(n_tensors=65537),
               "n < 0": call(lambda tab: tab["n"].__setitem__(0, -5)), "null g": call(lambda tab: tab["g"].__setitem__(0, 0)),
               "misaligned g": call(lambda tab: tab["g"].__setitem__(1, g[1].data_ptr() + 2)), "negative max_norm": call(max_norm=-1.0),
               "nan max_norm": call(max_norm=float("nan")), "null norm": call(norm=None), "null scale": call(sc=None),
               "misaligned norm": call(norm=out.data_ptr() + 4), "misaligned scale": call(sc=scale.data_ptr() + 2), "null workspace": call(wsp=None),
               "misaligned workspace": call(wsp=ws.data_ptr() + 16, ws_bytes=ws.numel() - 16), "short workspace": call(ws_bytes=ws.numel() - 1)}
    assert all(code == E_ARG for code in refused.values()), {k: v for k, v in refused.items() if v != E_ARG}
    assert L.linetr_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (scale == 7.0).all() and not ws.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert abs(float(out[0]) - 7.0 * np.sqrt(73.0)) <= 2.0 ** -40 * 60 and (out[1:] == 7.0).all() and (scale[1:] == 7.0).all()


# ---- the gradient norm -------------------------------------------------------------------------------------------------------------

def expected_scale(norm64, max_norm):
    return np.float32(min(1.0, max_norm / (norm64 + 1e-6)))


def norm_checks(eng, label, views, flat):
    norm64 = float(np.sqrt((flat.astype(np.float64) ** 2).sum()))
    results = []
    for max_norm in (float("inf"), 2.0 * norm64, 0.5 * norm64, 1e-3):
        norm, scale = eng.grad_norm(views, max_norm)
        assert norm.dtype == torch.float64 and norm.is_cuda and scale.dtype == torch.float32 and scale.is_cuda
        got, s = float(norm), scale.cpu().numpy()[0]
        assert abs(got - norm64) <= 2.0 ** -40 * norm64, (label, got, norm64)
        want = expected_scale(norm64, max_norm)
        assert abs(float(s) - float(want)) <= float(np.spacing(want)), (label, max_norm, s, want)
        if max_norm >= 2.0 * norm64:
            assert s == np.float32(1.0), (label, max_norm, s)
        results.append((got, s))
    again = eng.grad_norm(views, 1e-3)
    assert float(again[0]) == results[-1][0] and again[1].cpu().numpy()[0] == results[-1][1]
    assert len({r[0] for r in results}) == 1                 # the norm does not depend on max_norm
    print(f"grad norm {label}: |gpu - float64| / float64 = {abs(results[0][0] - norm64) / norm64 if norm64 else 0.0:.2e} (allowed 2^-40 = 9.1e-13)")
    return results[0][0]


def test_grad_norm_ragged_and_model(eng):
    for family in ("model", "wide"):
        case = AC.make_case(family, 1, TOTAL)
        norms = []
        for label, offsets in AC.ALIGNMENTS.items():
            buf = AC.Carved(SIZES, offsets["g"]).fill(case["g"])
            norms.append(norm_checks(eng, f"{family} ragged {label}", buf.views, case["g"]))
            assert buf.values().tobytes() == case["g"].tobytes()
        assert len(set(norms)) == 1                          # one order of summation whatever the alignment
    sizes = [int(np.prod(s)) for s in AC.model_shapes()]
    rs = AC._rs("model norm")
    g = (rs.standard_normal(sum(sizes)) * 10.0 ** rs.uniform(-6, 0, sum(sizes))).astype(np.float32)
    norm_checks(eng, "153 model tensors", split(g, sizes), g)
    zeros = [torch.zeros(n, device="cuda") for n in (5, 0, 4097)]
    for max_norm in (float("inf"), 1.0, 0.0):
        norm, scale = eng.grad_norm(zeros, max_norm)
        assert float(norm) == 0.0 and float(scale) == (1.0 if max_norm > 0 else 0.0)
    norm, scale = eng.grad_norm([torch.zeros(0, device="cuda")], 1.0)
    assert float(norm) == 0.0 and float(scale) == 1.0        # a table of no elements


# ---- linetr_amd.optim.Adam ---------------------------------------------------------------------------------------------------------

def flat_case(params_before, grads, exp_avgs, exp_avg_sqs, step, **hyper):
    flat = lambda ts: joined(ts) if ts is not None else np.zeros(sum(p.numel() for p in params_before), np.float32)
    base = dict(lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=0.0, decoupled_weight_decay=False)
    return {"p": flat(params_before), "g": flat(grads), "m": flat(exp_avgs), "v": flat(exp_avg_sqs), "step": step, "hyper": {**base, **hyper}}


def per_tensor_rows(names, sizes, got, case, refs):
    """the bar per parameter: the flat case's references (AC.refs_of) sliced parameter by parameter (the update is element-wise)"""
    ref64, ref32 = refs
    rows, at = [], 0
    for name, n in zip(names, sizes):
        sl = slice(at, at + n)
        rows += [(f"{name}.{k}", e, b) for k, e, b in AC.ratios({k: got[k][sl] for k in "pmv"}, case["p"][sl], {k: v[sl] for k, v in ref64.items()},
                                                                  {k: v[sl] for k, v in ref32.items()})]
        at += n
    return rows


def snapshot(opt, params):
    return {"p": [p.detach().clone() for p in params], "m": [opt.state[p]["exp_avg"].clone() for p in params],
            "v": [opt.state[p]["exp_avg_sq"].clone() for p in params]}


def model_and_loss():
    import linetr_amd.evaluations as E
    from linetr_amd.train_ops import TrainableLineTransformer
    sd, v0, v1, assign = KR.loss_case()
    mod = TrainableLineTransformer({})
    mod.load_state_dict(KR.tensors(sd), strict=True)
    mod = mod.cuda().train()
    crit = E.descriptor_loss()
    target = {"mat_assign_sublines": dev(assign)}

    def backward():
        d0, d1 = KR.data_tensors(v0, torch.float32, "cuda"), KR.data_tensors(v1, torch.float32, "cuda")
        with torch.enable_grad():
            loss = crit({"line_desc0": mod(d0)["line_desc"], "line_desc1": mod(d1)["line_desc"]}, target)[0]
            loss.backward()
        return float(loss.detach())
    return mod, backward


def test_optimizer_steps_the_model_as_torch_does():
    """TrainableLineTransformer on two views under descriptor_loss at B = 2, n = 33, S = 21: one backward, then the native step against the
    float64 restatement and against torch.optim.Adam(foreach=False) on a deep copy fed the same gradients; then a second iteration"""
    from linetr_amd.optim import Adam
    mod, backward = model_and_loss()
    names = [k for k, _ in mod.named_parameters()]
    params = list(mod.parameters())
    sizes = [p.numel() for p in params]
    assert len(params) == 153
    extra = torch.nn.Parameter(torch.randn(5, device="cuda"))       # never gets a gradient
    hyper = dict(lr=1e-3, weight_decay=1e-4)
    opt = Adam(params + [extra], **hyper)
    backward()
    twin = copy.deepcopy(mod)
    assert all(q is not p and torch.equal(q, p) for p, q in zip(params, twin.parameters()))
    theirs = torch.optim.Adam(twin.parameters(), foreach=False, **hyper)
    for p, q in zip(params, twin.parameters()):
        assert p.grad is not None
        q.grad = p.grad.clone()
    before = [p.detach().clone() for p in params]
    grads = [p.grad.clone() for p in params]
    versions = [p._version for p in params]
    extra_bits, extra_version = extra.detach().cpu().numpy().tobytes(), extra._version
    opt.step()
    theirs.step()
    case = flat_case(before, grads, None, None, 1, **hyper)
    got = {"p": joined(params), "m": joined([opt.state[p]["exp_avg"] for p in params]), "v": joined([opt.state[p]["exp_avg_sq"] for p in params])}
    torchs = {"p": joined(list(twin.parameters())), "m": joined([theirs.state[q]["exp_avg"] for q in twin.parameters()]),
              "v": joined([theirs.state[q]["exp_avg_sq"] for q in twin.parameters()])}
    refs = AC.refs_of(case)
    rows, rows_torch = per_tensor_rows(names, sizes, got, case, refs), per_tensor_rows(names, sizes, torchs, case, refs)
    print(f"adam optimizer on the model, step 1: native worst error / bar {AC.worst(rows):.3f}, torch on the GPU {AC.worst(rows_torch):.3f} "
          f"({len(rows)} rows)")
    assert len(rows) == 153 * 4 and not AC.failures(rows), AC.failures(rows)[:8]
    assert not AC.failures(rows_torch), AC.failures(rows_torch)[:8]
    assert all(p._version > v for p, v in zip(params, versions))
    assert [g.cpu().numpy().tobytes() for g in grads] == [p.grad.cpu().numpy().tobytes() for p in params]
    assert extra.detach().cpu().numpy().tobytes() == extra_bits and extra._version == extra_version and extra not in opt.state
    for p in params:
        st = opt.state[p]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
        assert float(st["step"]) == 1.0 and st["exp_avg"].shape == p.shape
    # the second iteration: zero_grad() drops the gradients, the backward allocates new ones
    snap = snapshot(opt, params)
    opt.zero_grad()
    assert all(p.grad is None for p in params)
    backward()
    opt.step()
    case = flat_case(snap["p"], [p.grad for p in params], snap["m"], snap["v"], 2, **hyper)
    got = {"p": joined(params), "m": joined([opt.state[p]["exp_avg"] for p in params]), "v": joined([opt.state[p]["exp_avg_sq"] for p in params])}
    rows = per_tensor_rows(names, sizes, got, case, AC.refs_of(case))
    print(f"adam optimizer on the model, step 2: native worst error / bar {AC.worst(rows):.3f}")
    assert not AC.failures(rows), AC.failures(rows)[:8]
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params)


SMALL_SHAPES = ((5,), (300, 7), (4097,), (2, 3, 4))


def small_params(seed):
    rs = AC._rs("optimizer", seed)
    return [torch.nn.Parameter(dev((0.05 * rs.standard_normal(s)).astype(np.float32))) for s in SMALL_SHAPES]


def set_grads(params, seed):
    rs = AC._rs("grads", seed)
    for p in params:
        p.grad = dev((rs.standard_normal(tuple(p.shape)) * 10.0 ** rs.uniform(-4, 0, tuple(p.shape))).astype(np.float32))


def check_optimizer_step(label, opt, params, seed, scale=None):
    """one more step of `opt` with seeded gradients against the restatement from the state it has now, group by group"""
    set_grads(params, seed)
    groups = []
    for group in opt.param_groups:
        ps = [p for p in group["params"] if p.grad is not None]
        steps = {float(opt.state[p]["step"]) if p in opt.state and opt.state[p] else 0.0 for p in ps}
        assert len(steps) == 1
        has = bool(steps.pop())
        groups.append((group, ps, [p.detach().clone() for p in ps], [p.grad.clone() for p in ps],
                       [opt.state[p]["exp_avg"].clone() for p in ps] if has else None, [opt.state[p]["exp_avg_sq"].clone() for p in ps] if has else None,
                       float(opt.state[ps[0]]["step"]) + 1 if has else 1.0))
    opt.step()
    for i, (group, ps, before, grads, ms, vs, step) in enumerate(groups):
        case = flat_case(before, grads, ms, vs, step, lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"],
                         decoupled_weight_decay=group["decoupled_weight_decay"])
        got = {"p": joined(ps), "m": joined([opt.state[p]["exp_avg"] for p in ps]), "v": joined([opt.state[p]["exp_avg_sq"] for p in ps])}
        check(f"{label}, group {i}, step {int(step)}", got, case, scale=scale)


def test_state_moves_between_torch_and_native():
    from linetr_amd.optim import Adam
    hyper = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-3)
    # torch -> native
    a = small_params(1)
    theirs = torch.optim.Adam(a, foreach=False, **hyper)
    for i in range(3):
        set_grads(a, i)
        theirs.step()
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    mine = Adam(b)
    mine.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert {k: v for k, v in mine.param_groups[0].items() if k != "params"} == {k: v for k, v in theirs.param_groups[0].items() if k != "params"}
    for p, q in zip(a, b):
        for key in ("exp_avg", "exp_avg_sq"):
            assert mine.state[q][key].cpu().numpy().tobytes() == theirs.state[p][key].cpu().numpy().tobytes() and mine.state[q][key].is_cuda
        assert float(mine.state[q]["step"]) == float(theirs.state[p]["step"]) == 3.0
        assert mine.state[q]["step"].device.type == "cpu" and mine.state[q]["step"].dtype == torch.float32
    check_optimizer_step("after torch's state", mine, b, 7)
    # native -> torch
    sd = mine.state_dict()
    fresh = Adam(small_params(8), weight_decay=1e-2, decoupled_weight_decay=True).state_dict()["param_groups"][0]
    torchs = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], weight_decay=1e-2, decoupled_weight_decay=True).state_dict()["param_groups"][0]
    assert fresh == {**torchs, "params": [0, 1, 2, 3]} and sorted(sd["param_groups"][0]) == sorted(torchs)
    assert (fresh["amsgrad"], fresh["maximize"], fresh["foreach"], fresh["capturable"], fresh["differentiable"], fresh["fused"],
            fresh["decoupled_weight_decay"]) == (False, False, None, False, False, None, True)
    c = [torch.nn.Parameter(p.detach().clone()) for p in b]
    back = torch.optim.Adam(c)
    back.load_state_dict(copy.deepcopy(sd))
    for p, q in zip(b, c):
        for key in ("exp_avg", "exp_avg_sq"):
            assert back.state[q][key].cpu().numpy().tobytes() == mine.state[p][key].cpu().numpy().tobytes()
        assert float(back.state[q]["step"]) == 4.0
    set_grads(c, 9)
    back.step()                                              # raises nothing
    assert all(float(back.state[q]["step"]) == 5.0 for q in c)


def test_two_param_groups_and_decoupled_decay():
    from linetr_amd.optim import Adam
    ps = small_params(2)
    opt = Adam([{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.1}, {"params": ps[2:]}], lr=1e-3)
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 1e-3] and [g["weight_decay"] for g in opt.param_groups] == [0.1, 0]
    for seed in (3, 4):
        check_optimizer_step("two groups", opt, ps, seed)
    ps = small_params(3)
    opt = Adam(ps, weight_decay=1e-2, decoupled_weight_decay=True)
    assert opt.param_groups[0]["decoupled_weight_decay"] is True
    for seed in (5, 6):
        check_optimizer_step("decoupled", opt, ps, seed)
    # a closure is evaluated with gradients enabled and its loss returned
    calls = []

    def closure():
        calls.append(torch.is_grad_enabled())
        return torch.tensor(3.5)
    assert float(opt.step(closure)) == 3.5 and calls == [True]


def test_max_grad_norm():
    from linetr_amd.optim import Adam
    probe = small_params(4)
    set_grads(probe, 11)
    norm64 = float(np.sqrt((joined([p.grad for p in probe]).astype(np.float64) ** 2).sum()))
    for max_norm, clipped in ((0.25 * norm64, True), (4.0 * norm64, False)):
        ps = small_params(4)
        opt = Adam(ps, max_grad_norm=max_norm)
        assert opt.last_grad_norm is None
        scale = expected_scale(norm64, max_norm)
        assert (scale < 1) == clipped
        check_optimizer_step(f"max_grad_norm {'below' if clipped else 'above'} the norm", opt, ps, 11, scale=scale)
        assert opt.last_grad_norm.dtype == torch.float64 and opt.last_grad_norm.is_cuda
        assert abs(float(opt.last_grad_norm) - norm64) <= 2.0 ** -40 * norm64
        set_grads(probe, 11)                                 # .grad itself is not rewritten
        assert all(p.grad.cpu().numpy().tobytes() == q.grad.cpu().numpy().tobytes() for p, q in zip(ps, probe))


def test_optimizer_refusals():
    from linetr_amd.optim import Adam
    good = small_params(5)
    with pytest.raises(ValueError, match="contiguous"):
        Adam([torch.nn.Parameter(torch.zeros(4, 6, device="cuda").t())])
    with pytest.raises(ValueError, match="float32"):
        Adam([torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float64))])
    with pytest.raises(ValueError, match="HIP device"):
        Adam(good + [torch.nn.Parameter(torch.zeros(4))])
    for option in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=option):
            Adam(good, **{option: True})
        sd = Adam(good).state_dict()
        sd["param_groups"][0][option] = True
        with pytest.raises(ValueError, match=option):
            Adam(good).load_state_dict(sd)
    with pytest.raises(ValueError, match="tensor"):
        Adam(good, lr=torch.tensor(1e-3, device="cuda"))
    opt = Adam(good)
    with pytest.raises(ValueError, match="tensor"):
        opt.add_param_group({"params": small_params(6), "lr": torch.tensor(1e-3)})
    assert len(opt.param_groups) == 1
    sd = opt.state_dict()
    sd["param_groups"][0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(ValueError, match="tensor"):
        opt.load_state_dict(sd)
    bits = [p.detach().cpu().numpy().tobytes() for p in good]
    good[0].grad = torch.sparse_coo_tensor(torch.tensor([[0, 2]], device="cuda"), torch.ones(2, device="cuda"), (5,))
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert [p.detach().cpu().numpy().tobytes() for p in good] == bits
    # a non-contiguous gradient is made contiguous by torch
    ps = [torch.nn.Parameter(torch.zeros(6, 4, device="cuda"))]
    opt = Adam(ps)
    ps[0].grad = torch.ones(4, 6, device="cuda").t()
    assert not ps[0].grad.is_contiguous()
    opt.step()
    assert torch.allclose(ps[0].detach(), torch.full((6, 4), -1e-3, device="cuda"), rtol=1e-5)
