"""GPU: training-time dropout of the line descriptive layer (csrc/lt_dropout.h; linetr_dropout_factors, linetr_cls_pool_dropout_*,
linetr_layer_norm_dropout_*; Engine.cls_pool_dropout_* / layer_norm_dropout_* / dropout_factors; train_ops.cls_token_pool /
residual_layer_norm with a DropoutState, LineDescriptiveEncoder.seed_dropout and what forwards it) against the host restatement of the
generator, the float64 closed forms with host masks and the masked restatement of the reference's unfolded module that
tests/test_dropout_cpu.py pins to autograd through the reference (tests/dropout_reference.py, tests/golden/desc_layer_dropout.npz).

The bar of a tensor is 8 x max(float32 CPU autograd error of the SAME case with the SAME masks against float64, 2^-23 max |float64|); the
generator, the p = 0 identities and the exact properties must hold bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load
import desc_layer_reference as DL
import dropout_reference as DR

pytestmark = pytest.mark.gpu
E_ARG = -1


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(got, c, keys, label):
    rows = DL.ratios(got, c["ref64"], c["ref32"], keys)
    print(f"dropout {label}: " + ", ".join(f"{key} {e / b if b else 0.0:.3f}" for key, e, b in rows) + "  (error / bar)")
    assert not DL.failures(rows), (label, DL.failures(rows))


# ---- the generator -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("site", (0, 1, 2))
def test_factors_equal_the_host_table(L, nat, eng, site):
    for seed in (DR.SEED, DR.BIG_SEED):
        for call in (0, 7):
            for p in (0.0,) + DR.P_VALUES:
                for rows in (1, 5):
                    for inner in (1, 22, 64):
                        got = DR.factors_launch(L, nat, seed, call, site, rows, inner, p)
                        assert got.tobytes() == DR.factors(seed, call, site, rows, inner, p).tobytes(), (seed, call, p, rows, inner)
    # the Engine makes the same state from (seed, call, p) and the same table
    drop = eng.dropout(DR.BIG_SEED, 7, 0.1)
    mine = DR.drop_struct(nat, DR.BIG_SEED, 7, 0.1)
    assert (drop.seed, drop.call, drop.threshold, drop.scale) == (mine.seed, mine.call, mine.threshold, mine.scale)
    assert eng.dropout_factors(drop, site, 5, 22).cpu().numpy().tobytes() == DR.factors(DR.BIG_SEED, 7, site, 5, 22, 0.1).tobytes()
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            eng.dropout(1, 0, bad)


def test_factors_argument_errors(L, nat):
    out = torch.full((64, 4), 7.0, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = DR.drop_struct(nat, 1, 0, 0.1)

    def call(drop=good, site=0, rows=4, inner=4, o=out.data_ptr()):
        return L.linetr_dropout_factors(None, C.byref(drop) if drop is not None else None, site, rows, inner, o, st())

    refused = [call(site=-1), call(site=3), call(rows=-1), call(rows=1 << 31), call(rows=1 << 40), call(inner=0), call(inner=1 << 31), call(drop=None),
               call(o=None), call(o=out.view(-1)[1:].data_ptr()), call(drop=nat.Dropout(1, 0, 0, 0.5)), call(drop=nat.Dropout(1, 0, 0, float("inf"))),
               call(drop=nat.Dropout(1, 0, 0, float("nan"))), call(rows=(1 << 31) - 1, inner=1 << 20)]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_last_error()
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                    # nothing was launched


# ---- CLS token pooling with dropout ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", DR.POOL_S)
def test_pooling_within_the_bar(L, nat, S):
    """forward and both gradients against float64 with host masks at every L around a block's four segments; padded strides give the
    same bits; a (segment, head) that lost all its tokens is exact zeros"""
    for family in DR.POOL_FAMILIES:
        for n_seg in DR.POOL_L:
            for p in DR.P_VALUES:
                c = DR.pool_case(family, n_seg, S, p)
                got = DR.pool_launch(L, nat, c)
                check(got, c, DR.POOL_OUTPUTS, f"pool {family} L={n_seg} S={S} p={p}")
                assert all(np.isfinite(got[key]).all() for key in DR.POOL_OUTPUTS)
                gone = DR.all_dropped(c["seed"], c["call"], n_seg, S, p)
                assert not got["pooled"][gone].any() and not got["kept"][gone].any()
                wide = DR.pool_launch(L, nat, c, ldx=260, ldu=1028)
                for key in DR.POOL_OUTPUTS:
                    assert got[key].tobytes() == wide[key].tobytes(), (family, n_seg, S, p, key)


@pytest.mark.parametrize("S", (1, 2, 3))
def test_all_dropped_heads_are_exact_zeros(L, nat, S):
    """seed 2026, call 0, p = 0.5, L = 9: the pairs that lost every token give pooled = 0 and kept = 0 exactly, and a gradient that arrives
    at them alone reaches neither x nor u; no NaN anywhere"""
    c = dict(DR.pool_case("normal", 9, S, 0.5))
    gone = DR.all_dropped(DR.SEED, 0, 9, S, 0.5)
    assert 0 < gone.sum() < 36
    got = DR.pool_launch(L, nat, c)
    assert not got["pooled"][gone].any() and not got["kept"][gone].any() and (got["kept"][~gone] > 0).all()
    assert all(np.isfinite(got[key]).all() for key in DR.POOL_OUTPUTS)
    c["dpooled"], c["dkept"] = c["dpooled"] * gone[:, :, None], c["dkept"] * gone
    only = DR.pool_launch(L, nat, c)
    assert not only["dx"].any() and not only["du"].any()


def test_pooling_without_dropout_has_the_bits_of_the_plain_kernels(L, nat):
    for family, n_seg, S in (("normal", 5, 23), ("peaky", 9, 22), ("normal", 3, 1), ("normal", 4, 7)):
        c = DR.pool_case(family, n_seg, S, 0.0)
        plain = DL.pool_launch(L, DL.pool_case(family, n_seg, S))
        for dkept in (False, True):
            cz = dict(c, dkept=np.zeros_like(c["dkept"]))
            got = DR.pool_launch(L, nat, cz, dkept=dkept)
            for key in DL.POOL_OUTPUTS:
                assert got[key].tobytes() == plain[key].tobytes(), (family, n_seg, S, dkept, key)
        # kept = sum of the weights the plain kernel normalises: 1 to the bar (exactly 1 only where that sum is), and a gradient
        # arriving at it is within the bar too
        check(DR.pool_launch(L, nat, c), c, DR.POOL_OUTPUTS, f"pool {family} L={n_seg} S={S} p=0")


def test_pooling_need_masks_and_the_engine(L, nat, eng):
    c = DR.pool_case("normal", 9, 23, 0.1)
    a, b = DR.pool_launch(L, nat, c), DR.pool_launch(L, nat, c)
    for key in DR.POOL_OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), key
    for need in ((True, False), (False, True), (False, False)):
        some = DR.pool_launch(L, nat, c, need=need)
        for key, n in zip(("dx", "du"), need):
            assert (key in some) == n and (not n or some[key].tobytes() == a[key].tobytes()), (need, key)
    # another call index draws other masks
    other = DR.pool_launch(L, nat, DR.pool_case("normal", 9, 23, 0.1, call=1))
    assert other["pooled"].tobytes() != a["pooled"].tobytes() and other["lse"].tobytes() == a["lse"].tobytes()
    # the Engine and the autograd surface
    from linetr_amd.train_ops import DropoutState, cls_token_pool
    drop = eng.dropout(c["seed"], c["call"], c["p"])
    x, u = dev(c["x"]), dev(c["u"])
    pooled, kept, lse = eng.cls_pool_dropout_forward(x, u, drop)
    dx, du = eng.cls_pool_dropout_backward(x, u, pooled, lse, kept, dev(c["dpooled"]), dev(c["dkept"]), drop)
    for key, t in (("pooled", pooled), ("kept", kept), ("lse", lse), ("dx", dx), ("du", du)):
        assert t.cpu().numpy().tobytes() == a[key].tobytes(), key
    xt, ut = x.clone().requires_grad_(), u.clone().requires_grad_()
    with torch.enable_grad():
        pl, kp = cls_token_pool(xt, ut, DropoutState(c["seed"], c["call"], c["p"]))
        torch.autograd.backward([pl, kp], [dev(c["dpooled"]), dev(c["dkept"])])
    assert torch.equal(pl.detach(), pooled) and torch.equal(kp.detach(), kept) and torch.equal(xt.grad, dx) and torch.equal(ut.grad, du)
    e = eng.cls_pool_dropout_forward(x[:0], u[:0], drop)
    assert [tuple(t.shape) for t in e] == [(0, 4, 256), (0, 4), (0, 4)]


def test_pooling_argument_errors(L, nat):
    n, S = 6, 3
    z = lambda *s: torch.zeros(s, device="cuda")
    x, u, pooled, lse, kept, g, gk = z(n * S, 256), z(n, 1024), z(n, 1024), z(n, 4), z(n, 4), z(n, 1024), z(n, 4)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((n, 1024), (n, 4), (n, 4), (n * S, 256), (n, 1024))]
    po, ko, lo, dx, du = outs
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]
    good = DR.drop_struct(nat, 1, 0, 0.1)
    ref = lambda d: C.byref(d) if d is not None else None

    def fwd(x_=x, ldx=256, u_=u, ldu=1024, L_=n, S_=S, d=good, p_=po, k_=ko, l_=lo):
        return L.linetr_cls_pool_dropout_forward(None, ptr(x_), ldx, ptr(u_), ldu, L_, S_, ref(d), ptr(p_), ptr(k_), ptr(l_), st())

    def bwd(x_=x, ldx=256, u_=u, ldu=1024, p_=pooled, l_=lse, k_=kept, g_=g, gk_=gk, L_=n, S_=S, d=good, dx_=dx, lddx=256, du_=du, lddu=1024):
        return L.linetr_cls_pool_dropout_backward(None, ptr(x_), ldx, ptr(u_), ldu, ptr(p_), ptr(l_), ptr(k_), ptr(g_), ptr(gk_), L_, S_, ref(d),
                                                  ptr(dx_), lddx, ptr(du_), lddu, st())

    bad = nat.Dropout(1, 0, 0, 0.5)
    refused = [fwd(S_=0), fwd(S_=257), fwd(L_=-1), fwd(ldx=252), fwd(ldx=258), fwd(ldu=1020), fwd(ldu=1026), fwd(x_=None), fwd(u_=None), fwd(p_=None),
               fwd(k_=None), fwd(l_=None), fwd(d=None), fwd(d=bad), fwd(x_=off(x)), fwd(u_=off(u)), fwd(p_=off(po)), fwd(k_=off(ko)), fwd(l_=off(lo)),
               bwd(S_=0), bwd(S_=257), bwd(L_=-1), bwd(ldx=252), bwd(ldu=1026), bwd(lddx=257), bwd(lddu=512), bwd(x_=None), bwd(u_=None), bwd(p_=None),
               bwd(l_=None), bwd(k_=None), bwd(g_=None), bwd(d=None), bwd(d=bad), bwd(x_=off(x)), bwd(k_=off(kept)), bwd(gk_=off(gk)), bwd(g_=off(g)),
               bwd(dx_=off(dx)), bwd(du_=off(du))]
    assert refused == [E_ARG] * len(refused), refused
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    assert bwd(dx_=None, lddx=0, du_=None, lddu=0) == 0 and fwd(L_=0) == 0 and bwd(L_=0) == 0 and bwd(gk_=None) == 0 and fwd() == 0
    torch.cuda.synchronize()
    assert not po.any() and not dx.any() and not du.any()                        # x = 0: zeros everywhere


# ---- LayerNorm with dropout --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("site", (1, 2))
def test_layer_norm_within_the_bar_and_its_identities(L, nat, site, residual):
    for rows in DR.LN_ROWS:
        for p in DR.P_VALUES:
            c = DR.ln_case(rows, residual, site, p)
            got = DR.ln_launch(L, nat, c)
            check(got, c, [k for k in DR.LN_OUTPUTS if k in c["ref64"]], f"layer_norm site {site} residual={residual} rows={rows} p={p}")
            wide = DR.ln_launch(L, nat, c, ld=260)
            for key in DR.LN_OUTPUTS:
                assert got[key].tobytes() == wide[key].tobytes(), (rows, p, key)
            # the plain kernels on the pre-masked input: the same bits in everything, dr = their dx; da = dr * factor
            masked = dict(DL.ln_case("normal", rows, residual), a=c["a"] * c["fac"])
            plain = DL.ln_launch(L, masked)
            for key, theirs in (("y", "y"), ("mean", "mean"), ("rstd", "rstd"), ("dr", "dx"), ("dgamma", "dgamma"), ("dbeta", "dbeta")):
                assert got[key].tobytes() == plain[theirs].tobytes(), (rows, p, key)
            assert got["da"].tobytes() == (got["dr"] * c["fac"]).tobytes(), (rows, p)
            assert (got["da"][c["fac"] == 0] == 0).all()
        # p = 0: today's entry points
        c0 = DR.ln_case(rows, residual, site, 0.0)
        got, plain = DR.ln_launch(L, nat, c0), DL.ln_launch(L, DL.ln_case("normal", rows, residual))
        for key, theirs in (("y", "y"), ("mean", "mean"), ("rstd", "rstd"), ("da", "dx"), ("dr", "dx"), ("dgamma", "dgamma"), ("dbeta", "dbeta")):
            assert got[key].tobytes() == plain[theirs].tobytes(), (rows, key)


def test_layer_norm_need_masks_engine_and_argument_errors(L, nat, eng):
    c = DR.ln_case(65, True, 2, 0.1)
    got = DR.ln_launch(L, nat, c)
    for need in ((True, False, False, False), (False, True, False, False), (False, False, True, True), (True, True, False, False)):
        some = DR.ln_launch(L, nat, c, need=need)
        for key, n in zip(("da", "dr", "dgamma", "dbeta"), need):
            assert (key in some) == n and (not n or some[key].tobytes() == got[key].tobytes()), (need, key)
    from linetr_amd.train_ops import DropoutState, residual_layer_norm
    drop = eng.dropout(c["seed"], c["call"], c["p"])
    a, r, g, gamma, beta = (dev(c[k]) for k in ("a", "r", "g", "gamma", "beta"))
    y, stats = eng.layer_norm_dropout_forward(a, r, gamma, beta, drop, 2)
    da, dr, dgamma, dbeta = eng.layer_norm_dropout_backward(a, r, stats, gamma, g, drop, 2)
    for key, t in (("y", y), ("_stats", stats), ("da", da), ("dr", dr), ("dgamma", dgamma), ("dbeta", dbeta)):
        assert t.cpu().numpy().tobytes() == got[key].tobytes(), key
    ln = torch.nn.LayerNorm(256, eps=DR.EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(gamma)
        ln.bias.copy_(beta)
    at, rt = a.clone().requires_grad_(), r.clone().requires_grad_()
    with torch.enable_grad():
        out = residual_layer_norm(at, rt, ln, DropoutState(c["seed"], c["call"], c["p"]), 2)
        out.backward(g)
    assert torch.equal(out.detach(), y) and torch.equal(at.grad, da) and torch.equal(rt.grad, dr) and torch.equal(ln.weight.grad, dgamma)
    with pytest.raises(ValueError):
        residual_layer_norm(at, rt, ln, DropoutState(1, 0, 0.1), None)
    with pytest.raises(ValueError):
        residual_layer_norm(at, rt, ln, DropoutState(1, 0, 1.0), 1)
    # the C entry points refuse what the plain ones refuse, and a bad site or state
    rows = 6
    z = lambda *s: torch.zeros(s, device="cuda")
    a, r, g, stats, gamma, beta = z(rows, 256), z(rows, 256), z(rows, 256), z(rows, 2), z(256), z(256)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((rows, 256), (rows, 2), (rows, 256), (rows, 256), (256,), (256,))]
    y, so, da, dr, dgamma, dbeta = outs
    need = L.linetr_layer_norm_backward_workspace_bytes(rows, 256)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]
    good = DR.drop_struct(nat, 1, 0, 0.1)
    ref = lambda d: C.byref(d) if d is not None else None

    def fwd(a_=a, lda=256, r_=r, ldr=256, eps=1e-6, rows_=rows, C_=256, d=good, site=1, y_=y, ldy=256, s_=so):
        return L.linetr_layer_norm_dropout_forward(None, ptr(a_), lda, ptr(r_), ldr, ptr(gamma), ptr(beta), eps, rows_, C_, ref(d), site, ptr(y_), ldy,
                                                   ptr(s_), st())

    def bwd(a_=a, lda=256, r_=r, ldr=256, g_=g, ldg=256, rows_=rows, C_=256, d=good, site=1, da_=da, ldda=256, dr_=dr, lddr=256, dg=dgamma, ws_=ws,
            nbytes=None):
        return L.linetr_layer_norm_dropout_backward(None, ptr(a_), lda, ptr(r_), ldr, ptr(stats), ptr(gamma), ptr(g_), ldg, rows_, C_, ref(d), site,
                                                    ptr(da_), ldda, ptr(dr_), lddr, ptr(dg), ptr(dbeta), ptr(ws_), ws.numel() if nbytes is None else nbytes,
                                                    st())

    refused = [fwd(site=-1), fwd(site=3), fwd(d=None), fwd(d=nat.Dropout(1, 0, 0, 0.0)), fwd(C_=128), fwd(rows_=-1), fwd(eps=0.0), fwd(lda=252),
               fwd(ldr=258), fwd(ldy=255), fwd(a_=None), fwd(y_=None), fwd(s_=None), fwd(a_=off(a)), fwd(r_=off(r)), fwd(y_=off(y)),
               bwd(site=-1), bwd(site=3), bwd(d=None), bwd(C_=260), bwd(rows_=-1), bwd(lda=252), bwd(ldr=2), bwd(ldg=258), bwd(ldda=254), bwd(lddr=257),
               bwd(a_=None), bwd(g_=None), bwd(ws_=None), bwd(a_=off(a)), bwd(da_=off(da)), bwd(dr_=off(dr)), bwd(nbytes=need - 1)]
    assert refused == [E_ARG] * len(refused), refused
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    assert fwd(r_=None, ldr=0) == 0 and bwd(da_=None, ldda=0) == 0 and bwd(dr_=None, lddr=0) == 0 and fwd(rows_=0) == 0 and fwd(site=0) == 0
    torch.cuda.synchronize()


# ---- the module under autograd -----------------------------------------------------------------------------------------------------

def build(sd, train=True, **kw):
    from linetr_amd.train_ops import LineDescriptiveEncoder
    mod = LineDescriptiveEncoder(**kw)
    mod.load_state_dict(DL.tensors(sd), strict=True)
    return mod.cuda().train(train)


def run_native(mod, desc, upstream, state=(DR.SEED, 0)):
    """dict out, d_desc and every parameter's .grad (CPU float32 arrays) of one forward + backward from the dropout state `state`"""
    for p in mod.parameters():
        p.grad = None
    if state is not None:
        mod.set_dropout_state(state)
    xt = dev(desc).requires_grad_()
    with torch.enable_grad():
        out, attn = mod(xt)
        assert attn is None and out.shape == desc.shape[:2] + (256,) and out.grad_fn is not None
        out.backward(dev(upstream))
    got = {"out": out.detach(), "d_desc": xt.grad, **{key: p.grad for key, p in mod.named_parameters()}}
    assert all(t is not None for t in got.values()), [key for key, t in got.items() if t is None]
    return {key: t.cpu().numpy() for key, t in got.items()}


@pytest.mark.parametrize("p", DR.P_VALUES)
def test_module_against_the_fixture(eng, p):
    f = load("desc_layer_dropout")
    sd, desc, g = DL.module_case(*DL.FIXTURE_SHAPE)
    mod = build(sd, dropout=p).seed_dropout(int(f["seed"]), int(f["call"]))
    got = run_native(mod, desc, g, state=None)
    worst = 0.0
    for key in ["out", "d_desc"] + list(DL.SHAPES):
        ref, val = f[DR.fixture_key(key, p)], DR.fixture_grid(key, got[key].astype(np.float64))
        bar = DL.FACTOR * max(float(f[DR.fixture_key(key, p) + "_f32_err"]), 2.0 ** -23 * np.abs(ref).max())
        err = np.abs(val - ref).max()
        worst = max(worst, err / bar)
        print(f"dropout fixture p={p} {key}: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert val.shape == ref.shape and err <= bar, (key, err, bar)
    print(f"dropout fixture p={p}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("shape", DR.MODULE_SHAPES)
def test_module_against_the_restatement(eng, shape):
    sd, desc, g = DL.module_case(*shape)
    ref64, ref32 = DR.module_refs(*shape, 0.1)
    mod = build(sd, dropout=0.1)
    got = run_native(mod, desc, g)
    rows = DL.ratios(got, ref64, ref32)
    print(f"dropout module {shape} p=0.1: worst error / bar {DL.worst(rows):.3f}; value bias "
          f"{[e / b for k, e, b in rows if k == 'slf_attn.w_vs.bias'][0]:.3f}")
    assert len(rows) == 18 and not DL.failures(rows), DL.failures(rows)
    kb = mod.slf_attn.w_ks.bias.grad
    assert kb is not None and kb.shape == (256,) and not kb.any()                # the key bias: still exact zeros
    assert np.abs(got["slf_attn.w_vs.bias"]).max() > 0
    again = run_native(mod, desc, g)                                              # the same state twice: identical bytes
    for key, val in got.items():
        assert val.tobytes() == again[key].tobytes(), key


def test_module_state_and_calls(eng):
    from linetr_amd.train_ops import KeylineEncoder
    sd, desc, g = DL.module_case(*DL.FIXTURE_SHAPE)
    mod = build(sd, dropout=0.1)
    assert mod.dropout_state() is None
    with pytest.raises(RuntimeError, match="dropout.*seed_dropout|seed_dropout.*dropout"):
        mod(dev(desc))                                                            # unseeded: randomness is never drawn implicitly
    assert mod.seed_dropout(DR.SEED) is mod and mod.dropout_state() == (DR.SEED, 0)
    x = dev(desc)
    # eval: no dropout, no call consumed, the bits of the dropout = 0 module
    plain = build(sd, train=False)(x)[0]
    assert torch.equal(mod.eval()(x)[0], plain) and mod.dropout_state() == (DR.SEED, 0)
    mod.train()
    # two forwards, then two backwards: each backward uses the masks of its own forward
    x0, x1 = x.clone().requires_grad_(), x.clone().requires_grad_()
    with torch.enable_grad():
        o0, o1 = mod(x0)[0], mod(x1)[0]
        assert mod.dropout_state() == (DR.SEED, 2) and not torch.equal(o0, o1)
        o1.backward(dev(g))
        o0.backward(dev(g))
    for call, (o, xt) in enumerate(((o0, x0), (o1, x1))):
        alone = run_native(mod, desc, g, state=(DR.SEED, call))
        assert alone["out"].tobytes() == o.detach().cpu().numpy().tobytes() and alone["d_desc"].tobytes() == xt.grad.cpu().numpy().tobytes(), call
    # dropout = 0 with a seed: today's bits, no call consumed
    zero = build(sd, dropout=0.0).seed_dropout(5, 9)
    assert torch.equal(zero(x)[0], build(sd)(x)[0]) and zero.dropout_state() == (5, 9)
    # the call index wraps; the state round-trips; bad states are refused
    mod.set_dropout_state((DR.BIG_SEED, 0xffffffff))
    mod(x)
    assert mod.dropout_state() == (DR.BIG_SEED, 0)
    mod.set_dropout_state(None)
    assert mod.dropout_state() is None
    for bad in ((-1, 0), (1 << 64, 0), (1, 1 << 32)):
        with pytest.raises(ValueError):
            mod.set_dropout_state(bad)
    # KeylineEncoder forwards to the layer that is computed, the last one
    enc = KeylineEncoder(n_att_layers=2, dropout=0.1).seed_dropout(3, 4)
    assert enc.dropout_state() == (3, 4) == enc.desc_layers[-1].dropout_state() and enc.desc_layers[0].dropout_state() is None


# ---- the whole model on two views under the criterion -------------------------------------------------------------------------------

def native_model(sd, train=True, **config):
    import keyline_reference as KR
    from linetr_amd.train_ops import TrainableLineTransformer
    mod = TrainableLineTransformer(config)
    mod.load_state_dict(KR.tensors(sd), strict=True)
    return mod.cuda().train(train)


def run_native_loss(mod, state):
    import keyline_reference as KR
    import linetr_amd.evaluations as E
    sd, v0, v1, assign = KR.loss_case()
    for p in mod.parameters():
        p.grad = None
    mod.set_dropout_state(state)
    crit = E.descriptor_loss()
    d0, d1 = KR.data_tensors(v0, torch.float32, "cuda"), KR.data_tensors(v1, torch.float32, "cuda")
    with torch.enable_grad():
        desc0, desc1 = mod(d0)["line_desc"], mod(d1)["line_desc"]
        loss = crit({"line_desc0": desc0, "line_desc1": desc1}, {"mat_assign_sublines": dev(assign)})[0]
        loss.backward()
    out = {"loss": float(loss.detach()), "V": crit.last["count"], "d_desc0": d0["desc_sublines"].grad.cpu().numpy(),
           "d_desc1": d1["desc_sublines"].grad.cpu().numpy(), "_line_desc0": desc0.detach().cpu().numpy()}
    for key, p in mod.named_parameters():
        assert p.grad is not None, key
        out[key] = p.grad.cpu().numpy()
    return out


def test_model_on_two_views_under_the_criterion(eng):
    """TrainableLineTransformer with dropout 0.1, seeded, at B = 2, n = 33, S = 21 under descriptor_loss against the float64 model built of
    keyline_reference's pieces with the masked layer in the place of its descriptive layer: view 0 draws call 0, view 1 call 1"""
    import keyline_reference as KR
    sd, v0, _, _ = KR.loss_case()
    ref64, ref32 = DR.loss_refs()
    mod = native_model(sd, dropout=DR.MODEL_P)
    with pytest.raises(RuntimeError, match="dropout"):
        mod(KR.data_tensors(v0, torch.float32, "cuda"))                           # unseeded still raises
    assert mod.seed_dropout(DR.SEED) is mod and mod.dropout_state() == (DR.SEED, 0)
    got = run_native_loss(mod, (DR.SEED, 0))
    assert mod.dropout_state() == (DR.SEED, 2)
    assert got["V"] == ref64["V"] and abs(got["loss"] - ref64["loss"]) <= 8 * max(abs(ref32["loss"] - ref64["loss"]), 2.0 ** -23 * ref64["loss"])
    arrays = lambda d: {k: v for k, v in d.items() if isinstance(v, np.ndarray) and not k.startswith("_")}
    assert len(arrays(got)) == 2 + 153 and sorted(arrays(got)) == sorted(arrays(ref64))
    rows = DL.ratios(arrays(got), arrays(ref64), arrays(ref32))
    vb = [e / b for k, e, b in rows if k.endswith("slf_attn.w_vs.bias")]
    print(f"dropout two views under the criterion: worst error / bar {DL.worst(rows):.3f}; value bias {vb[0]:.3f}")
    assert not DL.failures(rows), DL.failures(rows)
    assert not got["klenc.desc_layers.0.slf_attn.w_ks.bias"].any()
    # the same state again: identical bits; another call: other descriptors; eval: the dropout = 0 model's bits
    again = run_native_loss(mod, (DR.SEED, 0))
    for key, val in got.items():
        assert (val.tobytes() == again[key].tobytes()) if isinstance(val, np.ndarray) else val == again[key], key
    assert run_native_loss(mod, (DR.SEED, 1))["_line_desc0"].tobytes() != got["_line_desc0"].tobytes()
    data = lambda: KR.data_tensors(v0, torch.float32, "cuda", grad=False)
    plain = native_model(sd, train=False)
    plain.load_state_dict(mod.state_dict(), strict=True)                          # (the BatchNorm buffers moved in the training forwards)
    assert torch.equal(mod.eval()(data())["line_desc"], plain(data())["line_desc"])
