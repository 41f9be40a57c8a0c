"""GPU: the native backward of the line descriptive layer -- CLS token pooling, LayerNorm with a residual and GELU, each forward and
backward (csrc/lt_descbwd.h; linetr_cls_pool_train_*, linetr_layer_norm_*, linetr_gelu_*; Engine.cls_pool_* / layer_norm_* / gelu_*;
linetr_amd.train_ops.cls_token_pool / residual_layer_norm / gelu / LineDescriptiveEncoder) against the float64 closed forms and the
restatement of the reference's unfolded module that tests/test_desc_layer_cpu.py pins to autograd through the reference
(tests/desc_layer_reference.py, tests/golden/desc_layer.npz).

The bar of a tensor is 8 x max(float32 CPU autograd error of the SAME case against float64, 2^-23 max |float64|); the exact properties
must hold bit for bit.  Measured on the MI355X: profiles/desc_layer_gpu_tests.txt, profiles/desc_layer_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load
import desc_layer_reference as DL

pytestmark = pytest.mark.gpu
E_ARG = -1


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


def check(got, c, keys, label, pick=None):
    """every tensor of `keys` within its bar (`pick`: the compared leading indices of what the launch returned)"""
    got = {key: got[key][pick] if pick is not None else got[key] for key in keys}
    rows = DL.ratios(got, c["ref64"], c["ref32"], keys)
    print(f"desc_layer {label}: " + ", ".join(f"{key} {e / b if b else 0.0:.3f}" for key, e, b in rows) + "  (error / bar)")
    assert not DL.failures(rows), (label, DL.failures(rows))


# ---- CLS token pooling -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", DL.POOL_S)
@pytest.mark.parametrize("family", DL.POOL_FAMILIES)
def test_pooling_within_the_bar(L, family, S):
    """forward and both gradients against float64 at every L around a block's four segments; padded strides give the same bits"""
    for n_seg in DL.POOL_L:
        c = DL.pool_case(family, n_seg, S)
        got = DL.pool_launch(L, c)
        check(got, c, DL.POOL_OUTPUTS, f"pool {family} L={n_seg} S={S}", pick=c["check"])
        wide = DL.pool_launch(L, c, ldx=260, ldu=1028)
        for key in DL.POOL_OUTPUTS:
            assert got[key][c["check"]].tobytes() == wide[key][c["check"]].tobytes(), (family, n_seg, S, key)


def test_pooling_of_one_token_is_exact(L):
    """S = 1: p = 1, so pooled is the token row in all four heads and du = 0 (delta and dp are the same sum), bit for bit"""
    c = DL.pool_case("normal", 5, 1)
    got = DL.pool_launch(L, c)
    assert np.array_equal(got["pooled"], np.repeat(c["x"], 4, axis=1)) and not got["du"].any()
    assert not DL.failures(DL.ratios(got, c["ref64"], c["ref32"], ("dx",)))


def test_pooling_two_calls_and_need_masks_give_identical_bits(L, eng):
    c = DL.pool_case("normal", 11, 23)
    a, b = DL.pool_launch(L, c), DL.pool_launch(L, c)
    for key in DL.POOL_OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), key
    for need in ((True, False), (False, True)):
        some = DL.pool_launch(L, c, need=need, saved=a["_dev"])
        for key, n in zip(("dx", "du"), need):
            assert (key in some) == n and (not n or some[key].tobytes() == a[key].tobytes()), (need, key)
    none = DL.pool_launch(L, c, need=(False, False), saved=a["_dev"])
    assert "dx" not in none and "du" not in none
    # the Engine, on another stream
    x, u, g = dev(c["x"]), dev(c["u"]), dev(c["dpooled"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pooled, lse = eng.cls_pool_forward(x, u)
        dx, du = eng.cls_pool_backward(x, u, pooled, lse, g)
        only = eng.cls_pool_backward(x, u, pooled, lse, g, need=(False, True))
    side.synchronize()
    for key, t in (("pooled", pooled), ("lse", lse), ("dx", dx), ("du", du)):
        assert t.cpu().numpy().tobytes() == a[key].tobytes(), key
    assert only[0] is None and torch.equal(only[1], du)
    e = eng.cls_pool_forward(x[:0], u[:0])
    assert e[0].shape == (0, 4, 256) and e[1].shape == (0, 4)
    assert [t.shape for t in eng.cls_pool_backward(x[:0], u[:0], e[0], e[1], g[:0])] == [(0, 23, 256), (0, 4, 256)]


def test_pooling_argument_errors(L):
    n, S = 6, 3
    z = lambda *s: torch.zeros(s, device="cuda")
    x, u, pooled, lse, g = z(n * S, 256), z(n, 1024), z(n, 1024), z(n, 4), z(n, 1024)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((n, 1024), (n, 4), (n * S, 256), (n, 1024))]
    po, lo, dx, du = outs
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]                                               # 4 bytes past a 16-byte boundary

    def fwd(x_=x, ldx=256, u_=u, ldu=1024, L_=n, S_=S, p_=po, l_=lo):
        return L.linetr_cls_pool_train_forward(None, ptr(x_), ldx, ptr(u_), ldu, L_, S_, ptr(p_), ptr(l_), st())

    def bwd(x_=x, ldx=256, u_=u, ldu=1024, p_=pooled, l_=lse, g_=g, L_=n, S_=S, dx_=dx, lddx=256, du_=du, lddu=1024):
        return L.linetr_cls_pool_train_backward(None, ptr(x_), ldx, ptr(u_), ldu, ptr(p_), ptr(l_), ptr(g_), L_, S_, ptr(dx_), lddx, ptr(du_), lddu,
                                                st())

    refused = [fwd(S_=0), fwd(S_=257), fwd(S_=-1), fwd(L_=-1), fwd(ldx=252), fwd(ldx=258), fwd(ldu=1020), fwd(ldu=1026), fwd(x_=None), fwd(u_=None),
               fwd(p_=None), fwd(l_=None), fwd(x_=off(x)), fwd(u_=off(u)), fwd(p_=off(po)), fwd(l_=off(lo)),
               bwd(S_=0), bwd(S_=257), bwd(L_=-1), bwd(ldx=252), bwd(ldx=258), bwd(ldu=1020), bwd(ldu=1026), bwd(lddx=252), bwd(lddx=257),
               bwd(lddu=512), bwd(lddu=1030), bwd(x_=None), bwd(u_=None), bwd(p_=None), bwd(l_=None), bwd(g_=None), bwd(x_=off(x)),
               bwd(u_=off(u)), bwd(p_=off(pooled)), bwd(l_=off(lse)), bwd(g_=off(g)), bwd(dx_=off(dx)), bwd(du_=off(du))]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    # legal: absent outputs (their strides are not read), no segments
    assert bwd(dx_=None, lddx=0, du_=None, lddu=0) == 0 and fwd(L_=0) == 0 and bwd(L_=0) == 0
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not po.any() and not dx.any() and not du.any()                        # x = 0: zeros everywhere
    assert torch.allclose(lo, torch.full((n, 4), float(np.log(3.0)), device="cuda"), rtol=0, atol=1e-6)       # all scores 0: lse = log S


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------

def ln_chunk_rows(L):
    """rows per partial row of the parameter-gradient reduction, read off the workspace size"""
    base = L.linetr_layer_norm_backward_workspace_bytes(1, 256)
    return next(r for r in range(1, 4097) if L.linetr_layer_norm_backward_workspace_bytes(r + 1, 256) > base)


@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("family", DL.LN_FAMILIES)
def test_layer_norm_within_the_bar(L, family, residual):
    chunk = ln_chunk_rows(L)
    assert 4 <= chunk <= 1024
    for rows in sorted({1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 5}):
        c = DL.ln_case(family, rows, residual)
        got = DL.ln_launch(L, c)
        check(got, c, DL.LN_OUTPUTS, f"layer_norm {family} residual={residual} rows={rows}")
        wide = DL.ln_launch(L, c, ld=260)
        for key in DL.LN_OUTPUTS:
            assert got[key].tobytes() == wide[key].tobytes(), (family, rows, key)
        if family == "constant":
            assert np.array_equal(got["y"], np.broadcast_to(c["beta"], (rows, 256))) and np.isfinite(got["dx"]).all()


def test_layer_norm_exact_properties(L):
    chunk = ln_chunk_rows(L)
    rows = 2 * chunk + 3
    # gamma = 0: dx is exactly 0
    c = DL.ln_case("normal", rows, True, zero_gamma=True)
    got = DL.ln_launch(L, c)
    assert not got["dx"].any() and np.array_equal(got["y"], np.broadcast_to(c["beta"], (rows, 256)))
    # integer g: dbeta is exact
    c = DL.ln_case("normal", rows, True, integer_g=True)
    got = DL.ln_launch(L, c)
    assert np.array_equal(got["dbeta"], c["g"].astype(np.float64).sum(axis=0).astype(np.float32))
    # two calls and every need mask give the same bits
    again = DL.ln_launch(L, c)
    for key in DL.LN_OUTPUTS:
        assert got[key].tobytes() == again[key].tobytes(), key
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        some = DL.ln_launch(L, c, need=need)
        for key, n in zip(("dx", "dgamma", "dbeta"), need):
            assert (key in some) == n and (not n or some[key].tobytes() == got[key].tobytes()), (need, key)


def test_layer_norm_argument_errors(L, eng):
    rows = 70
    z = lambda *s: torch.zeros(s, device="cuda")
    a, r, g, stats, gamma, beta = z(rows, 256), z(rows, 256), z(rows, 256), z(rows, 2), z(256), z(256)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((rows, 256), (rows, 2), (rows, 256), (256,), (256,))]
    y, so, dx, dgamma, dbeta = outs
    need = L.linetr_layer_norm_backward_workspace_bytes(rows, 256)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]

    def fwd(a_=a, lda=256, r_=r, ldr=256, gm=gamma, bt=beta, eps=1e-6, rows_=rows, C_=256, y_=y, ldy=256, s_=so):
        return L.linetr_layer_norm_forward(None, ptr(a_), lda, ptr(r_), ldr, ptr(gm), ptr(bt), eps, rows_, C_, ptr(y_), ldy, ptr(s_), st())

    def bwd(a_=a, lda=256, r_=r, ldr=256, s_=stats, gm=gamma, g_=g, ldg=256, rows_=rows, C_=256, dx_=dx, lddx=256, dg=dgamma, db=dbeta, ws_=ws,
            nbytes=None):
        return L.linetr_layer_norm_backward(None, ptr(a_), lda, ptr(r_), ldr, ptr(s_), ptr(gm), ptr(g_), ldg, rows_, C_, ptr(dx_), lddx, ptr(dg),
                                            ptr(db), ptr(ws_), ws.numel() if nbytes is None else nbytes, st())

    refused = [fwd(C_=128), fwd(C_=512), fwd(C_=0), fwd(rows_=-1), fwd(eps=0.0), fwd(lda=252), fwd(ldr=258), fwd(ldy=255), fwd(a_=None), fwd(gm=None),
               fwd(bt=None), fwd(y_=None), fwd(s_=None), fwd(a_=off(a)), fwd(r_=off(r)), fwd(gm=off(gamma)), fwd(bt=off(beta)), fwd(y_=off(y)),
               fwd(s_=off(so)),
               bwd(C_=128), bwd(C_=260), bwd(rows_=-1), bwd(lda=252), bwd(ldr=2), bwd(ldg=258), bwd(lddx=254), bwd(a_=None), bwd(s_=None), bwd(gm=None),
               bwd(g_=None), bwd(ws_=None), bwd(a_=off(a)), bwd(r_=off(r)), bwd(s_=off(stats)), bwd(gm=off(gamma)), bwd(g_=off(g)), bwd(dx_=off(dx)),
               bwd(dg=off(dgamma)), bwd(db=off(dbeta)), bwd(ws_=off(ws)), bwd(nbytes=need - 1), bwd(nbytes=0)]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_layer_norm_backward_workspace_bytes(rows, 128) == 0
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    # legal: no residual (its stride is not read), no parameter gradients and then no workspace, no rows
    assert fwd(r_=None, ldr=0) == 0 and bwd(r_=None, ldr=0, dg=None, db=None, ws_=None, nbytes=0) == 0 and fwd(rows_=0) == 0
    assert bwd(rows_=0, dx_=None) == 0
    torch.cuda.synchronize()
    assert not dgamma.any() and not dbeta.any() and not y.any() and not dx.any()        # a = 0, beta = 0; no rows: zero sums
    # the surface refuses another width and an `ln` without parameters
    from linetr_amd.train_ops import residual_layer_norm
    with pytest.raises(ValueError):
        residual_layer_norm(z(4, 128), None, torch.nn.LayerNorm(128).cuda())
    with pytest.raises(ValueError):
        residual_layer_norm(z(4, 256), None, torch.nn.LayerNorm(256, elementwise_affine=False).cuda())
    with pytest.raises(ValueError):
        eng.layer_norm_forward(z(4, 128), None, z(128), z(128))


# ---- GELU --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", DL.GELU_FAMILIES)
def test_gelu_within_the_bar_of_its_family(L, family):
    c = DL.gelu_case(family)
    got = DL.gelu_launch(L, c["z"], c["g"])
    check(got, c, ("y", "dz"), f"gelu {family}")
    wide = DL.gelu_launch(L, c["z"], c["g"], ld=1028)
    assert got["y"].tobytes() == wide["y"].tobytes() and got["dz"].tobytes() == wide["dz"].tobytes()


def test_gelu_at_its_ends_and_argument_errors(L):
    z = np.array([[0.0, -0.0, 30.0, -30.0]], np.float32)
    g = np.array([[3.0, -5.0, 7.0, 11.0]], np.float32)
    got = DL.gelu_launch(L, z, g)
    assert got["y"].tobytes() == np.array([[0.0, -0.0, 30.0, -0.0]], np.float32).tobytes()
    assert np.array_equal(got["dz"], np.array([[1.5, -2.5, 7.0, 0.0]], np.float32))
    zt, gt = dev(np.zeros((3, 8), np.float32)), dev(np.zeros((3, 8), np.float32))
    out = torch.full((3, 8), 7.0, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    off = lambda t: t.view(-1)[1:].data_ptr()
    p = lambda t: t.data_ptr()
    refused = [L.linetr_gelu_forward(None, p(zt), 8, 3, 6, p(out), 8, st()), L.linetr_gelu_forward(None, p(zt), 8, 3, 0, p(out), 8, st()),
               L.linetr_gelu_forward(None, p(zt), 8, 3, 4100, p(out), 4100, st()), L.linetr_gelu_forward(None, p(zt), 4, 3, 8, p(out), 8, st()),
               L.linetr_gelu_forward(None, p(zt), 8, 3, 8, p(out), 10, st()), L.linetr_gelu_forward(None, None, 8, 3, 8, p(out), 8, st()),
               L.linetr_gelu_forward(None, p(zt), 8, 3, 8, None, 8, st()), L.linetr_gelu_forward(None, off(zt), 8, 2, 8, p(out), 8, st()),
               L.linetr_gelu_forward(None, p(zt), 8, -1, 8, p(out), 8, st()), L.linetr_gelu_backward(None, p(zt), 8, None, 8, 3, 8, p(out), 8, st()),
               L.linetr_gelu_backward(None, p(zt), 8, p(gt), 6, 3, 8, p(out), 8, st()), L.linetr_gelu_backward(None, p(zt), 8, off(gt), 8, 2, 8, p(out), 8, st()),
               L.linetr_gelu_backward(None, p(zt), 8, p(gt), 8, 3, 8, off(out), 8, st())]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_gelu_forward(None, p(zt), 8, 0, 8, p(out), 8, st()) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- the module under autograd -----------------------------------------------------------------------------------------------------

def build(sd, train=True, **kw):
    from linetr_amd.train_ops import LineDescriptiveEncoder
    mod = LineDescriptiveEncoder(**kw)
    mod.load_state_dict(DL.tensors(sd), strict=True)
    return mod.cuda().train(train)


def run_native(mod, desc, upstream, mask=None):
    """dict out, d_desc and every parameter's .grad (CPU float32 arrays) of one forward + backward"""
    for p in mod.parameters():
        p.grad = None
    xt = dev(desc).requires_grad_()
    with torch.enable_grad():
        out, attn = mod(xt, mask)
        assert attn is None and out.shape == desc.shape[:2] + (256,) and out.grad_fn is not None
        out.backward(dev(upstream))
    got = {"out": out.detach(), "d_desc": xt.grad, **{key: p.grad for key, p in mod.named_parameters()}}
    assert all(t is not None for t in got.values()), [key for key, t in got.items() if t is None]
    return {key: t.cpu().numpy() for key, t in got.items()}


def test_module_against_the_fixture(eng):
    f = load("desc_layer")
    sd, desc, g = DL.module_case(*DL.FIXTURE_SHAPE)
    mod = build(sd)
    assert sorted(mod.state_dict()) == sorted(f["state_dict_keys"].tolist())
    assert all(tuple(t.shape) == DL.SHAPES[key] for key, t in mod.state_dict().items())
    got = run_native(mod, desc, g)
    worst = 0.0
    for key in ["out", "d_desc"] + list(DL.SHAPES):
        ref, val = f[key], got[key].astype(np.float64)
        val = val[::7, ::5] if key in DL.MATRICES else val
        bar = DL.FACTOR * max(float(f[f"{key}_f32_err"]), 2.0 ** -23 * np.abs(ref).max())
        err = np.abs(val - ref).max()
        worst = max(worst, err / bar)
        print(f"desc_layer fixture {key}: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert val.shape == ref.shape and err <= bar, (key, err, bar)
    print(f"desc_layer fixture: worst error / bar {worst:.3f}")
    # the key bias: exact zeros, not None
    kb = mod.slf_attn.w_ks.bias.grad
    assert kb is not None and kb.shape == (256,) and not kb.any()
    # the same bits on two calls; a mask of ones and a mask with zeros at padded slots change nothing
    again = run_native(mod, desc, g)
    B, n, S = DL.FIXTURE_SHAPE
    ones = torch.ones(B, n, S, S, device="cuda")
    padded = ones.clone()
    padded[:, :, 15:, :] = 0
    padded[:, :, :, 15:] = 0
    for other in (again, run_native(mod, desc, g, ones), run_native(mod, desc, g, padded)):
        for key, val in got.items():
            assert val.tobytes() == other[key].tobytes(), key
    # from_line_transformer reads klenc.desc_layers.<i>.* of a state_dict: the last layer by default
    from linetr_amd.train_ops import LineDescriptiveEncoder
    full = {f"klenc.desc_layers.{i}.{key}": torch.from_numpy(val) * (i + 1) for i in range(2) for key, val in sd.items()}
    last, first = LineDescriptiveEncoder.from_line_transformer(full), LineDescriptiveEncoder.from_line_transformer(full, layer=0)
    assert sorted(last.state_dict()) == sorted(DL.SHAPES)
    for key, val in sd.items():
        assert torch.equal(first.state_dict()[key], torch.from_numpy(val)) and torch.equal(last.state_dict()[key], torch.from_numpy(val) * 2)


@pytest.mark.parametrize("shape,train", [(DL.MODULE_SHAPES[0], True), (DL.MODULE_SHAPES[1], True), (DL.FIXTURE_SHAPE, False)])
def test_module_against_the_restatement(eng, shape, train):
    sd, desc, g = DL.module_case(*shape)
    ref64, ref32 = DL.module_refs(*shape, train)
    got = run_native(build(sd, train), desc, g)
    rows = DL.ratios(got, ref64, ref32)
    print(f"desc_layer module {shape} train={train}: worst error / bar {DL.worst(rows):.3f}")
    assert len(rows) == 18 and not DL.failures(rows), DL.failures(rows)
    assert not got["slf_attn.w_ks.bias"].any()


def test_module_refusals(eng):
    from linetr_amd.train_ops import LineDescriptiveEncoder, cls_token_pool, gelu
    sd, desc, g = DL.module_case(*DL.MODULE_SHAPES[0])
    mod = build(sd, dropout=0.1)
    with pytest.raises(RuntimeError, match="dropout"):
        mod(dev(desc))
    assert mod.eval()(dev(desc))[0].shape == (1, 1, 256)                       # dropout is the identity in eval mode
    with pytest.raises(ValueError):
        LineDescriptiveEncoder(d_feature=128)
    with pytest.raises(ValueError):
        LineDescriptiveEncoder(n_heads=8)
    with pytest.raises(ValueError):
        build(sd)(torch.zeros(1, 2, 3, 128, device="cuda"))
    with pytest.raises(ValueError):
        build(sd)(torch.zeros(1, 2, 257, 256, device="cuda"))
    with pytest.raises(RuntimeError, match="HIP device"):
        build(sd).cpu()(torch.from_numpy(desc))                               # the tensors must be on the device
    with pytest.raises(ValueError):
        cls_token_pool(torch.zeros(2, 3, 256, device="cuda"), torch.zeros(2, 4, 128, device="cuda"))
    with pytest.raises(ValueError):
        gelu(torch.zeros(2, 6, device="cuda"))


def test_layer_under_the_signature_network_and_the_head(eng):
    """LineDescriptiveEncoder -> klines_pos + cls_out^T -> a two-layer SelfAttentionalLayer -> DescriptorHead -> a seeded upstream: every
    .grad, d_desc included, against the float64 restatement"""
    from linetr_amd.train_ops import DescriptorHead, SelfAttentionalLayer
    import sig_layer_reference as SL
    sd, stack_sd, W, b, desc, pos, upstream = DL.tail_case()
    layer = build(sd)
    stack = SelfAttentionalLayer(256, ["self", "self"])
    stack.load_state_dict(SL.tensors(stack_sd), strict=True)
    head = DescriptorHead()
    head.load_state_dict({"final_proj.weight": torch.from_numpy(W), "final_proj.bias": torch.from_numpy(b)})
    stack, head = stack.cuda().train(), head.cuda()
    xt, pt = dev(desc).requires_grad_(), dev(pos).requires_grad_()
    with torch.enable_grad():
        cls_out, _ = layer(xt)
        line_desc = head(stack(pt + cls_out.transpose(1, 2)))
        line_desc.backward(dev(upstream))
    got = {"line_desc": line_desc.detach(), "d_desc": xt.grad, "d_pos": pt.grad}
    for prefix, mod in (("desc.", layer), ("stack.", stack), ("final_proj.", head.final_proj)):
        got.update({prefix + key: p.grad for key, p in mod.named_parameters()})
    assert all(t is not None for t in got.values())
    ref64, ref32 = DL.tail_refs()
    assert sorted(got) == sorted(ref64)
    rows = DL.ratios({key: t.cpu().numpy() for key, t in got.items()}, ref64, ref32)
    print(f"desc_layer under the signature network: worst error / bar {DL.worst(rows):.3f}")
    assert not DL.failures(rows), DL.failures(rows)
