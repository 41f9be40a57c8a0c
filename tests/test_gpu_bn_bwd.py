"""GPU: BatchNorm (+ ReLU) for training -- the forward that keeps z and the statistics, and the backward (csrc/lt_bntrain.h, lt_bnbwd.h;
linetr_bn_forward / linetr_bn_backward; Engine.bn_forward / bn_backward; linetr_amd.train_ops.batch_norm_relu) -- against the float64
formulae that tests/test_bn_bwd_cases_cpu.py pins to torch's float64 autograd.

Cases, input families, references and the bar -- max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per 64-row tile of
dz (and of y) and per vector dgamma / dbeta, a property of the CPU references alone -- are in bn_bwd_cases.py.  The exact properties
hold bit for bit: two calls, gamma = 0, fully masked channels, integer g, and the forward against linetr_debug_bn_train on the same input.
Measured on the MI355X: profiles/bn_bwd_errors.txt."""
import ctypes as C

import pytest
import torch

import bn_cases as BC
import bn_bwd_cases as BB
from attn_cases import MARKER

pytestmark = pytest.mark.gpu
E_ARG = -1
KEYS = BB.layer_cases()
SMALL = [k for k in KEYS if not BB.is_big(k)]
BIG = [k for k in KEYS if BB.is_big(k)]


@pytest.fixture(scope="module")
def L():
    from linetr_amd import _native as nat
    return nat.lib()


@pytest.fixture(scope="module")
def train_eng():
    from linetr_amd.engine import Engine
    return Engine(BC.chain_state_dict("calibrated", BC.CHAIN_WIDTHS[0])[0], "cuda:0", keyline_encoder=list(BC.CHAIN_WIDTHS[0]), bn_batch_stats=True)


def check_case(L, key, train_eng=None):
    """forward (y inside bn_cases' bar, the saved statistics against float64, train mode: the running statistics; with `train_eng`: y
    and the running statistics bit for bit against linetr_debug_bn_train) and the backward on the forward's own saved statistics"""
    c = BB.layer_case(*key)
    rows, Cn = c["rows"], c["C"]
    fwd = BB.launch_forward(L, c)
    bad = [f"{key} y: {m}" for m in BB.failures(BB.forward_errors(fwd["y"], c))]
    bad += [f"{key}: {m}" for m in BB.failures(BB.saved_errors(fwd, c))]
    if c["mode"] == BB.TRAIN:
        bad += [f"{key}: {m}" for m in BB.failures(BC.stat_errors(fwd, c["fwd64"], c["fwd32"], ("run_mean", "run_var")))]
        if train_eng is not None and c["relu"]:
            ref, _ = BC.launch_layer(train_eng, dict(rows=rows, C=Cn, ld=c["strides"][0], z=c["z"], gamma=c["gamma"], beta=c["beta"],
                                                     running=c["running"], momentum=c["momentum"]))
            for k in ("y", "run_mean", "run_var"):
                if not torch.equal(fwd[k], ref[k]):
                    bad.append(f"{key}: {k} differs from linetr_debug_bn_train's")
    got = BB.launch_backward(L, c, save=fwd["_save"])
    errs = BB.backward_errors(got, c)
    w = BB.worst(errs)
    print(f"bn_bwd {key}: worst unit {w[0]} err {w[2]:.3e} bar {w[3]:.3e} ratio {w[2] / w[3] if w[3] else 0.0:.3f}")
    bad += [f"{key}: {m}" for m in BB.failures(errs)] + [f"{key}: {m}" for m in BB.exact_failures(got, c)]
    if not all(bool(torch.isfinite(t).all()) for t in got.values()):
        bad.append(f"{key}: a result is not finite")
    return bad


@pytest.mark.parametrize("family", BB.FAMILIES)
def test_layer(L, train_eng, family):
    """Every C in (4, 100, 252, 256, 260, 512) at rows around the chunking's edges, every row stride of z, y, g and dz ('sentinel':
    +-1e4 between and behind the rows, bit-unchanged afterwards), with and without ReLU, training and eval mode, one row."""
    bad = []
    for key in SMALL:
        if key[0] == family:
            bad += check_case(L, key, train_eng)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("rows", BB.BIG_ROWS)
def test_layer_many_rows(L, rows):
    """32 767 / 32 769 rows: 511 chunks, and 512 of which the last seven own no row and must write zero partials"""
    bad = []
    for key in BIG:
        if key[2] == rows:
            bad += check_case(L, key)
    assert not bad, "\n".join(bad)


def test_two_calls_and_need_masks_give_identical_bits(L):
    twice = [k for k in SMALL if k[2] in (129, 333)][::3]
    assert len(twice) >= 6
    for key in twice:
        c = BB.layer_case(*key)
        a, b = BB.launch_forward(L, c), BB.launch_forward(L, c)
        for k in ("y", "run_mean", "run_var", "save_mean", "save_invstd"):
            assert torch.equal(a[k], b[k]), (key, k)
        ga, gb = BB.launch_backward(L, c, save=a["_save"]), BB.launch_backward(L, c, save=b["_save"])
        for k in ("dz", "dgamma", "dbeta"):
            assert torch.equal(ga[k], gb[k]), (key, k)
        for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
            some = BB.launch_backward(L, c, save=a["_save"], need=need)
            for k, n in zip(("dz", "dgamma", "dbeta"), need):
                assert (some[k] is not None) == n and (not n or torch.equal(some[k], ga[k])), (key, need, k)


def test_refusals(L):
    """what the entry points are not written for is refused with LINETR_E_ARG and a message before anything is launched"""
    rows, Cn, ld = 70, 32, 64
    dev = "cuda"
    mk = lambda *s: torch.full(s, MARKER, dtype=torch.float32, device=dev)
    z, y, g, dz = mk(rows, ld), mk(rows, ld), mk(rows, ld), mk(rows, ld)
    gamma, beta, running, dgamma, dbeta = torch.ones(Cn, device=dev), torch.zeros(Cn, device=dev), mk(2 * Cn), mk(Cn), mk(Cn)
    save = torch.full((2 * Cn,), MARKER, dtype=torch.float64, device=dev)
    need_f, need_b = L.linetr_bn_forward_workspace_bytes(rows, Cn), L.linetr_bn_backward_workspace_bytes(rows, Cn)
    ws = torch.empty(max(need_f, need_b) + 64, dtype=torch.uint8, device=dev)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]

    def fwd(z_=z, ldz=ld, rows_=rows, C_=Cn, gamma_=gamma, beta_=beta, eps=1e-5, mom=0.1, run_=running, mode=0, relu=1, y_=y, ldy=ld, save_=save,
            ws_=ws, nbytes=None):
        return L.linetr_bn_forward(None, p(z_), ldz, rows_, C_, p(gamma_), p(beta_), eps, mom, p(run_), mode, relu, p(y_), ldy, p(save_), p(ws_),
                                   ws.numel() if nbytes is None else nbytes, st())

    def bwd(z_=z, ldz=ld, y_=y, ldy=ld, g_=g, ldg=ld, save_=save, gamma_=gamma, rows_=rows, C_=Cn, mode=0, dz_=dz, lddz=ld, dgamma_=dgamma,
            dbeta_=dbeta, ws_=ws, nbytes=None):
        return L.linetr_bn_backward(None, p(z_), ldz, p(y_), ldy, p(g_), ldg, p(save_), p(gamma_), rows_, C_, mode, p(dz_), lddz, p(dgamma_),
                                    p(dbeta_), p(ws_), ws.numel() if nbytes is None else nbytes, st())

    refused = [fwd(C_=34, ldz=36, ldy=36), fwd(C_=516, ldz=516, ldy=516), fwd(C_=0), fwd(C_=2), fwd(ldz=28), fwd(ldz=34), fwd(ldy=28), fwd(ldy=30),
               fwd(z_=off(z)), fwd(y_=off(y)), fwd(gamma_=off(gamma)), fwd(run_=off(running)), fwd(save_=save.view(torch.float32)[1:]), fwd(ws_=off(ws)),
               fwd(z_=None), fwd(gamma_=None), fwd(beta_=None), fwd(y_=None), fwd(save_=None), fwd(ws_=None), fwd(run_=None, mode=1), fwd(mode=2),
               fwd(mode=-1), fwd(relu=2), fwd(eps=0.0), fwd(eps=float("nan")), fwd(mom=-0.1), fwd(mom=1.5), fwd(nbytes=need_f - 1), fwd(nbytes=0),
               fwd(rows_=(1 << 30) + 1),
               bwd(C_=34, ldz=36, ldy=36, ldg=36, lddz=36), bwd(C_=516), bwd(C_=0), bwd(ldz=28), bwd(ldy=34), bwd(ldg=0), bwd(lddz=30),
               bwd(z_=off(z)), bwd(y_=off(y)), bwd(g_=off(g)), bwd(dz_=off(dz)), bwd(dgamma_=off(dgamma)), bwd(dbeta_=off(dbeta)), bwd(gamma_=off(gamma)),
               bwd(save_=save.view(torch.float32)[1:]), bwd(ws_=off(ws)), bwd(z_=None), bwd(g_=None), bwd(save_=None), bwd(gamma_=None), bwd(ws_=None),
               bwd(mode=2), bwd(nbytes=need_b - 1), bwd(nbytes=0), bwd(rows_=(1 << 30) + 1)]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_last_error()
    torch.cuda.synchronize()
    for t in (y, dz, dgamma, dbeta, running, save):
        assert bool((t == MARKER).all())                                         # nothing was launched
    # legal and nothing runs: no rows; absent outputs (their strides are not read)
    assert fwd(rows_=0) == 0 and fwd(rows_=-3) == 0 and bwd(rows_=0) == 0 and bwd(dz_=None, lddz=0, dgamma_=None, dbeta_=None) == 0
    torch.cuda.synchronize()
    for t in (y, dz, dgamma, dbeta, running, save):
        assert bool((t == MARKER).all())
    # the same buffers are served when nothing is wrong; running = NULL: no update; y = NULL: no mask
    z.normal_()
    g.normal_()
    assert fwd(run_=None) == 0 and bwd() == 0 and bwd(y_=None, ldy=0) == 0
    torch.cuda.synchronize()
    assert bool((running == MARKER).all()) and bool((y[:, Cn:] == MARKER).all()) and not bool((y[:, :Cn] == MARKER).any())
    assert bool((dz[:, Cn:] == MARKER).all()) and bool(torch.isfinite(dz[:, :Cn]).all()) and bool(torch.isfinite(save).all())


# ---- the Engine and the autograd surface ------------------------------------------------------------------------------------------

def _torch_run(bn_state, z, g, dtype, training, relu):
    """relu?(nn.BatchNorm1d(z)) differentiated by torch on the CPU at `dtype`: dict y, dz, dgamma, dbeta, running_mean, running_var"""
    Cn = z.shape[1]
    bn = torch.nn.BatchNorm1d(Cn).to(dtype)
    bn.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in bn_state.items()})
    bn.train(training)
    zt = z.to(dtype).clone().requires_grad_()
    with torch.enable_grad():
        y = bn(zt)
        y = torch.relu(y) if relu else y
        y.backward(g.to(dtype))
    return dict(y=y.detach(), dz=zt.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean.clone(),
                running_var=bn.running_var.clone(), tracked=int(bn.num_batches_tracked))


@pytest.mark.parametrize("shape,training,relu", [((2, 256, 33), True, True), ((3, 512, 129), True, True), ((2, 512, 1), True, True),
                                                 ((65, 100), True, False), ((2, 256, 33), False, True), ((70, 512), False, False)])
def test_batch_norm_relu_against_torch(shape, training, relu):
    """batch_norm_relu under autograd against nn.BatchNorm1d (+ relu) on the same tensors: float64 torch is the reference, float32
    torch gives the bar, per tensor; the running statistics and num_batches_tracked move as torch's"""
    from linetr_amd.train_ops import batch_norm_relu
    gen = BC._gen("batch_norm_relu", shape, training, relu)
    Cn = shape[1]
    z, g = 2.0 * torch.randn(shape, generator=gen) + 0.5, torch.randn(shape, generator=gen)
    state = dict(weight=0.5 + torch.rand(Cn, generator=gen), bias=0.3 * torch.randn(Cn, generator=gen), running_mean=0.5 * torch.randn(Cn, generator=gen),
                 running_var=0.5 + torch.rand(Cn, generator=gen), num_batches_tracked=torch.tensor(3))
    ref64, ref32 = _torch_run(state, z, g, torch.float64, training, relu), _torch_run(state, z, g, torch.float32, training, relu)
    bn = torch.nn.BatchNorm1d(Cn)
    bn.load_state_dict(state)
    bn = bn.cuda().train(training)
    zt = z.cuda().requires_grad_()
    with torch.enable_grad():
        y = batch_norm_relu(zt, bn, relu=relu)
        assert y.shape == z.shape and y.grad_fn is not None
        y.backward(g.cuda())
    got = dict(y=y.detach(), dz=zt.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var)
    if relu:          # the premise of comparing backwards: the three forwards open the same activations
        assert torch.equal(got["y"].cpu() > 0, ref64["y"] > 0) and torch.equal(ref32["y"] > 0, ref64["y"] > 0)
    assert int(bn.num_batches_tracked) == ref64["tracked"] == (4 if training else 3)
    for k, t in got.items():
        r64, r32 = ref64[k], ref32[k].double()
        bar = BB.FACTOR * max((r32 - r64).abs().max().item(), 2.0 ** -23 * r64.abs().max().item())
        err = (t.cpu().double() - r64).abs().max().item()
        print(f"batch_norm_relu {shape} training={training} {k}: err {err:.3e} bar {bar:.3e} ratio {err / bar if bar else 0.0:.3f}")
        assert t.shape == r64.shape and err <= bar, (k, err, bar)
    if not training:
        assert torch.equal(bn.running_mean.cpu(), state["running_mean"]) and torch.equal(bn.running_var.cpu(), state["running_var"])
    # only z requires a gradient: the same dz
    bn2 = torch.nn.BatchNorm1d(Cn)
    bn2.load_state_dict(state)
    bn2 = bn2.cuda().train(training).requires_grad_(False)
    z2 = z.cuda().requires_grad_()
    with torch.enable_grad():
        batch_norm_relu(z2, bn2, relu=relu).backward(g.cuda())
    assert torch.equal(z2.grad, zt.grad) and bn2.weight.grad is None


def test_batch_norm_relu_refusals():
    from linetr_amd.train_ops import batch_norm_relu
    z = torch.randn(1, 8, 1, device="cuda")
    bn = torch.nn.BatchNorm1d(8).cuda()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        batch_norm_relu(z, bn)
    assert int(bn.num_batches_tracked) == 0
    assert batch_norm_relu(z, bn.eval()).shape == z.shape                       # eval mode takes a single value
    for bad in (torch.nn.BatchNorm1d(8, momentum=None), torch.nn.BatchNorm1d(8, affine=False)):
        with pytest.raises(ValueError):
            batch_norm_relu(torch.randn(4, 8, device="cuda"), bad.cuda())
    with pytest.raises(ValueError):
        batch_norm_relu(torch.randn(4, 12, device="cuda"), bn)
    with pytest.raises(TypeError):
        batch_norm_relu(torch.randn(4, 8, device="cuda"), torch.nn.LayerNorm(8).cuda())


def test_engine_takes_strided_rows_and_the_transposed_view():
    """[B, C, n] as the transposed view of rows and a column block of a wider buffer go through without a copy and give the bits of the
    contiguous rows"""
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    gen = BC._gen("engine bn")
    B, Cn, n = 2, 64, 37
    rows = torch.randn((B * n, Cn), generator=gen).cuda()
    g = torch.randn((B * n, Cn), generator=gen).cuda()
    gamma, beta = (0.5 + torch.rand(Cn, generator=gen)).cuda(), torch.randn(Cn, generator=gen).cuda()
    y0, save0 = eng.bn_forward(rows, gamma, beta)
    d0 = eng.bn_backward(rows, y0, g, save0, gamma)
    view = rows.view(B, n, Cn).transpose(1, 2)
    y1, save1 = eng.bn_forward(view, gamma, beta)
    assert y1.shape == (B, Cn, n) and y1.transpose(1, 2).is_contiguous() and torch.equal(y1.transpose(1, 2).reshape(B * n, Cn), y0)
    d1 = eng.bn_backward(view, y1, g.view(B, n, Cn).transpose(1, 2), save1, gamma)
    assert torch.equal(d1[0].transpose(1, 2).reshape(B * n, Cn), d0[0]) and torch.equal(d1[1], d0[1]) and torch.equal(d1[2], d0[2])
    wide = torch.zeros((B * n, 3 * Cn), device="cuda")
    wide[:, Cn:2 * Cn] = rows
    y2, save2 = eng.bn_forward(wide[:, Cn:2 * Cn], gamma, beta)
    assert torch.equal(y2, y0) and torch.equal(save2, save0)
    rm, rv = torch.zeros(Cn, device="cuda"), torch.ones(Cn, device="cuda")
    eng.bn_forward(rows, gamma, beta, rm, rv, momentum=1.0)
    assert torch.allclose(rm, rows.mean(dim=0), atol=1e-5) and torch.allclose(rv, rows.var(dim=0), rtol=1e-4)
