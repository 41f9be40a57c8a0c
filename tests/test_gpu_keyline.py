"""GPU: the native backward of the positional encoders and of KeylineEncoder's glue, and the whole network under autograd -- the encoders'
input layer and the token assembly, each forward and backward (csrc/lt_posbwd.h; linetr_input_layer_*, linetr_token_assemble_*;
Engine.input_layer_* / assemble_tokens_*; linetr_amd.train_ops.input_linear / assemble_tokens / LinePositionalEncoder /
WordPositionalEncoder / KeylineEncoder / TrainableLineTransformer) against the float64 closed forms and the restatement of the reference's
modules that tests/test_keyline_cpu.py pins to autograd through the reference (tests/keyline_reference.py, tests/golden/keyline.npz,
tests/golden/keyline_matrices.npz).

The bar of a tensor is 8 x max(float32 CPU autograd error of the SAME case against float64, 2^-23 max |float64|); the exact properties
must hold bit for bit.  Measured on the MI355X: profiles/keyline_gpu_tests.txt, profiles/keyline_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load
import keyline_reference as KR

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


@pytest.fixture(autouse=True)
def grad_enabled():
    """every test here differentiates, whatever grad mode an earlier test of the session left behind"""
    with torch.enable_grad():
        yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(got, ref64, ref32, label, keys=None):
    rows = KR.ratios(got, ref64, ref32, keys)
    print(f"keyline {label}: worst error / bar {KR.worst(rows):.3f} over {len(rows)} tensors")
    assert not KR.failures(rows), (label, KR.failures(rows))
    return rows


# ---- the encoders' input layer -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", KR.IL_N)
@pytest.mark.parametrize("Kin", KR.IL_KIN)
def test_input_layer_within_the_bar(L, Kin, N):
    """forward and both gradients against float64 at every row count around a chunk; x misaligned and strided between sentinels; padded
    strides of z and g give the same bits"""
    chunk = L.linetr_input_layer_chunk_rows()
    worst = 0.0
    for rows in KR.il_rows(chunk):
        c = KR.il_case(Kin, N, rows)
        got = KR.il_launch(L, c)
        rws = KR.ratios(got, c["ref64"], c["ref32"], KR.IL_OUTPUTS)
        worst = max(worst, KR.worst(rws))
        assert not KR.failures(rws), (Kin, N, rows, KR.failures(rws))
        wide = KR.il_launch(L, c, ldx=Kin, ld=N + 4, shift=0)
        for key in KR.IL_OUTPUTS:
            assert got[key].tobytes() == wide[key].tobytes(), (Kin, N, rows, key)
    print(f"keyline input layer Kin={Kin} N={N}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("Kin", KR.IL_KIN)
def test_input_layer_is_exact_on_integers_and_repeatable(L, Kin):
    chunk = L.linetr_input_layer_chunk_rows()
    for N in KR.IL_N:
        for rows in KR.il_rows(chunk):
            c = KR.il_case(Kin, N, rows, integer=True)
            got = KR.il_launch(L, c)
            for key in KR.IL_OUTPUTS:
                assert np.array_equal(got[key], c["ref64"][key].astype(np.float32)), (Kin, N, rows, key)
    c = KR.il_case(Kin, 32, 2 * chunk + 3)
    a, b = KR.il_launch(L, c), KR.il_launch(L, c)
    for key in KR.IL_OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), key
    for need in ((True, False), (False, True), (False, False)):
        some = KR.il_launch(L, c, need=need)
        for key, n in zip(("dW", "db"), need):
            assert (key in some) == n and (not n or some[key].tobytes() == a[key].tobytes()), (need, key)


def test_input_layer_engine_and_autograd(eng):
    from linetr_amd.train_ops import input_linear
    c = KR.il_case(5, 32, 300)
    raw = KR.il_launch(eng._L, c)
    x, W, b, g = dev(c["x"]), dev(c["W"][:, :, None]).requires_grad_(), dev(c["b"]).requires_grad_(), dev(c["g"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = input_linear(x, W, b)
        z.backward(g)
        only = eng.input_layer_backward(x, W, g, need=(False, True))
    side.synchronize()
    assert W.grad.shape == (32, 5, 1) and only[0] is None and torch.equal(only[1], b.grad)
    for key, t in (("z", z.detach()), ("dW", W.grad[:, :, 0]), ("db", b.grad)):
        assert t.cpu().numpy().tobytes() == raw[key].tobytes(), key
    assert eng.input_layer_forward(x[:0], W, b).shape == (0, 32) and not eng.input_layer_backward(x[:0], W, g[:0])[0].any()
    with pytest.raises(RuntimeError, match="no gradient with respect to x"):
        input_linear(x.clone().requires_grad_(), W, b)
    with pytest.raises(ValueError):
        input_linear(x, dev(np.zeros((30, 5), np.float32)), None)
    with pytest.raises(ValueError):
        input_linear(dev(np.zeros((4, 9), np.float32)), dev(np.zeros((32, 9), np.float32)), None)


def test_input_layer_argument_errors(L):
    rows, N, Kin = 70, 32, 3
    z_ = lambda *s: torch.zeros(s, device="cuda")
    x, W, b, g = z_(rows, Kin), z_(N, Kin), z_(N), z_(rows, N)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((rows, N), (N, Kin), (N,))]
    z, dW, db = outs
    need = L.linetr_input_layer_backward_workspace_bytes(rows, N, Kin)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]                                               # 4 bytes past a 16-byte boundary
    odd = lambda t: t.view(torch.uint8).view(-1)[2:]                             # 2 bytes past: not even a float's alignment

    def fwd(x_=x, ldx=Kin, W_=W, b_=b, rows_=rows, N_=N, K_=Kin, z_=z, ldz=N):
        return L.linetr_input_layer_forward(None, ptr(x_), ldx, ptr(W_), ptr(b_), rows_, N_, K_, ptr(z_), ldz, st())

    def bwd(x_=x, ldx=Kin, g_=g, ldg=N, rows_=rows, N_=N, K_=Kin, dW_=dW, db_=db, ws_=ws, nbytes=None):
        return L.linetr_input_layer_backward(None, ptr(x_), ldx, ptr(g_), ldg, rows_, N_, K_, ptr(dW_), ptr(db_), ptr(ws_),
                                             ws.numel() if nbytes is None else nbytes, st())

    refused = [fwd(K_=0), fwd(K_=9), fwd(N_=0), fwd(N_=30), fwd(N_=68), fwd(rows_=-1), fwd(ldx=2), fwd(ldz=28), fwd(ldz=34), fwd(x_=None), fwd(W_=None),
               fwd(z_=None), fwd(z_=off(z)), fwd(x_=odd(x)), fwd(W_=odd(W)), fwd(b_=odd(b)),
               bwd(K_=0), bwd(K_=9), bwd(N_=30), bwd(N_=68), bwd(rows_=-1), bwd(ldx=2), bwd(ldg=28), bwd(ldg=34), bwd(x_=None), bwd(g_=None), bwd(ws_=None),
               bwd(g_=off(g)), bwd(ws_=off(ws)), bwd(x_=odd(x)), bwd(dW_=odd(dW)), bwd(db_=odd(db)), bwd(nbytes=need - 1), bwd(nbytes=0)]
    assert refused == [E_ARG] * len(refused), refused
    assert b"1 <= Kin <= 8" in L.linetr_last_error() or b"workspace" in L.linetr_last_error()
    assert fwd(K_=9) == E_ARG and b"1 <= Kin <= 8" in L.linetr_last_error() and b"4 <= N <= 64" in L.linetr_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    # legal: x and the small tensors at any float alignment, no bias, no gradients wanted (then no workspace), no rows
    assert fwd(x_=off(x), rows_=rows - 1) == 0 and fwd(b_=None) == 0 and bwd(dW_=None, db_=None, ws_=None, nbytes=0) == 0 and fwd(rows_=0) == 0
    assert bwd(rows_=0) == 0
    torch.cuda.synchronize()
    assert not z.any() and not dW.any() and not db.any()                         # x = 0, no bias; no rows: zero sums


# ---- the token assembly ------------------------------------------------------------------------------------------------------------

def ta_segs_per_block(L):
    """segments per partial row of the cls gradient's reduction, read off the workspace size"""
    base = L.linetr_token_assemble_backward_workspace_bytes(1)
    return next(n for n in range(1, 4097) if L.linetr_token_assemble_backward_workspace_bytes(n + 1) > base)


@pytest.mark.parametrize("S", KR.TA_S)
@pytest.mark.parametrize("family", KR.TA_FAMILIES)
def test_token_assembly(L, family, S):
    per_block = ta_segs_per_block(L)
    assert 2 <= per_block <= 256
    worst = 0.0
    for n_seg in KR.ta_segments(per_block):
        c = KR.ta_case(family, n_seg, S)
        got = KR.ta_launch(L, c)
        assert got["x"][:, 1:].tobytes() == (c["desc"] + c["pos"]).tobytes(), (family, n_seg, S)            # one float32 add
        assert np.array_equal(got["x"][:, 0], np.broadcast_to(c["cls"], (n_seg, 256)))
        assert got["dtok"].tobytes() == np.ascontiguousarray(c["dx"][:, 1:]).tobytes()                       # a copy
        if family == "integer":
            assert np.array_equal(got["dcls"], c["ref64"]["dcls"].astype(np.float32))
        rws = KR.ratios(got, c["ref64"], c["ref32"], ("dcls",))                                                # (sentinel: nothing of the token slots leaks)
        worst = max(worst, KR.worst(rws))
        assert not KR.failures(rws), (family, n_seg, S, KR.failures(rws))
    print(f"keyline token assembly {family} S={S}: dcls worst error / bar {worst:.3f}")


def test_token_assembly_two_calls_need_masks_engine_and_autograd(L, eng):
    from linetr_amd.train_ops import assemble_tokens
    c = KR.ta_case("normal", 2 * ta_segs_per_block(L) + 3, 21)
    a, b = KR.ta_launch(L, c), KR.ta_launch(L, c)
    for key in KR.TA_OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), key
    for need in ((True, False), (False, True), (False, False)):
        some = KR.ta_launch(L, c, need=need)
        for key, n in zip(("dtok", "dcls"), need):
            assert (key in some) == n and (not n or some[key].tobytes() == a[key].tobytes()), (need, key)
    desc, pos, cls = dev(c["desc"]).requires_grad_(), dev(c["pos"]).requires_grad_(), dev(c["cls"]).view(1, 1, 1, 256).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = assemble_tokens(desc, pos, cls)
        x.backward(dev(c["dx"]))
    side.synchronize()
    assert cls.grad.shape == (1, 1, 1, 256) and torch.equal(desc.grad, pos.grad)
    for key, t in (("x", x.detach()), ("dtok", desc.grad), ("dcls", cls.grad.view(-1))):
        assert t.cpu().numpy().tobytes() == a[key].tobytes(), key
    assert eng.assemble_tokens_forward(desc[:0], pos[:0], cls).shape == (0, 22, 256)
    empty = eng.assemble_tokens_backward(x[:0].detach())
    assert empty[0].shape == (0, 21, 256) and not empty[1].any()
    with pytest.raises(ValueError):
        assemble_tokens(desc, pos[:, :20], cls)
    with pytest.raises(ValueError):
        assemble_tokens(torch.zeros(2, 256, 256, device="cuda"), torch.zeros(2, 256, 256, device="cuda"), cls)


def test_token_assembly_argument_errors(L):
    n, S = 11, 3
    z = lambda *s: torch.zeros(s, device="cuda")
    desc, pos, cls, dx = z(n * S, 256), z(n * S, 256), z(256), z(n * (S + 1), 256)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((n * (S + 1), 256), (n * S, 256), (256,))]
    x, dtok, dcls = outs
    need = L.linetr_token_assemble_backward_workspace_bytes(n)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    off = lambda t: t.view(-1)[1:]

    def fwd(d_=desc, p_=pos, c_=cls, L_=n, S_=S, x_=x):
        return L.linetr_token_assemble_forward(None, ptr(d_), ptr(p_), ptr(c_), L_, S_, ptr(x_), st())

    def bwd(dx_=dx, L_=n, S_=S, dt_=dtok, dc_=dcls, ws_=ws, nbytes=None):
        return L.linetr_token_assemble_backward(None, ptr(dx_), L_, S_, ptr(dt_), ptr(dc_), ptr(ws_), ws.numel() if nbytes is None else nbytes, st())

    refused = [fwd(S_=0), fwd(S_=256), fwd(S_=-1), fwd(L_=-1), fwd(L_=(1 << 24) + 1), fwd(d_=None), fwd(p_=None), fwd(c_=None), fwd(x_=None),
               fwd(d_=off(desc)), fwd(p_=off(pos)), fwd(c_=off(cls)), fwd(x_=off(x)),
               bwd(S_=0), bwd(S_=256), bwd(L_=-1), bwd(dx_=None), bwd(ws_=None), bwd(dx_=off(dx)), bwd(dt_=off(dtok)), bwd(dc_=off(dcls)), bwd(ws_=off(ws)),
               bwd(nbytes=need - 1), bwd(nbytes=0)]
    assert refused == [E_ARG] * len(refused), refused
    assert fwd(S_=256) == E_ARG and b"1 <= S <= 255" in L.linetr_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    # legal: no cls gradient and then no workspace, nothing wanted, no segments
    assert bwd(dc_=None, ws_=None, nbytes=0) == 0 and bwd(dt_=None, dc_=None, ws_=None, nbytes=0) == 0 and fwd(L_=0) == 0 and bwd(L_=0) == 0
    torch.cuda.synchronize()
    assert (x == 7.0).all() and not dtok.any() and not dcls.any()                # dx = 0; no segments: a zero sum


# ---- the encoders under autograd ---------------------------------------------------------------------------------------------------

def native_encoder(kind, sd, train):
    from linetr_amd import train_ops as T
    mod = (T.LinePositionalEncoder if kind == "line" else T.WordPositionalEncoder)(256, [32, 64, 128, 256])
    mod.load_state_dict(KR.tensors(sd), strict=True)
    return mod.cuda().train(train)


@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("kind,shape", [(k, s) for k, shapes in KR.ENCODER_SHAPES.items() for s in shapes])
def test_encoder_against_the_restatement(eng, kind, shape, train):
    """output, every .grad, the running statistics and num_batches_tracked after the call, in .train() and in .eval()"""
    sd, inputs, upstream = KR.encoder_case(kind, shape)
    ref64, ref32 = KR.encoder_refs(kind, shape, train)
    mod = native_encoder(kind, sd, train)
    with torch.enable_grad():
        out = mod(*(dev(a) for a in inputs))
        assert out.shape == upstream.shape
        out.backward(dev(upstream))
    got = KR.collect(mod, {"out": out.detach().double().cpu().numpy()})
    rows = check(got, ref64, ref32, f"{kind} encoder {shape} train={train}")
    assert len(rows) == 1 + 18 + 8
    for key, val in ref64.items():
        if val.dtype == np.int64:
            assert np.array_equal(got[key], val) and int(val) == int(train), key


def test_encoder_refusals(eng):
    from linetr_amd import train_ops as T
    for bad in ([30, 64, 128, 256], [32, 64, 100, 256], [128, 64], [32, 2048]):
        with pytest.raises(ValueError):
            T.LinePositionalEncoder(256, bad)
    sd, inputs, _ = KR.encoder_case("word", (1, 1, 2))
    mod = native_encoder("word", sd, True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        mod(dev(inputs[0][:, :, :1]), dev(inputs[1][:, :, :1]))                # a single token in the whole batch
    with pytest.raises(RuntimeError, match="no gradient with respect to x"):
        mod(dev(inputs[0]).requires_grad_(), dev(inputs[1]))


# ---- the whole model ---------------------------------------------------------------------------------------------------------------

def native_model(sd, train=True, **config):
    from linetr_amd.train_ops import TrainableLineTransformer
    mod = TrainableLineTransformer(config)
    mod.load_state_dict(KR.tensors(sd), strict=True)
    return mod.cuda().train(train)


def run_fixture_calls(mod):
    sd, inputs, upstream = KR.model_case()
    return KR.run_calls(mod, lambda: KR.data_tensors(inputs, torch.float32, "cuda"), dev(upstream), forward=lambda data: mod(data)["line_desc"])


def test_model_against_the_fixture(eng):
    """both calls of the fixture: line_desc, desc_sublines.grad, all 153 parameter gradients, all 15 BatchNorms' buffers"""
    f, fm = load("keyline"), load("keyline_matrices")
    sd, inputs, upstream = KR.model_case()
    mod = native_model(sd)
    assert sorted(mod.state_dict()) == sorted(f["state_dict_keys"].tolist())
    got = run_fixture_calls(mod)
    rows = KR.fixture_ratios(got, f, fm)
    grads = [name for name, _, _ in rows if not name.startswith(("after.", "line_desc", "d_desc"))]
    stats = [name for name, _, _ in rows if name.startswith("after.")]
    assert len(grads) == 153 and len(stats) == 15 * 2 * KR.FIXTURE_CALLS and len(rows) == 153 + len(stats) + 3
    groups = {"line_desc": ("line_desc",), "d_desc": ("d_desc",), "encoders": ("klenc.line_position_enc", "klenc.word_position_enc"),
              "cls_token": ("klenc.cls_token",), "desc_layer": ("klenc.desc_layers",), "signature": ("selfattn",), "head": ("final_proj",),
              "running statistics": ("after.",)}
    for label, prefixes in groups.items():
        print(f"keyline fixture {label}: worst error / bar {KR.worst([r for r in rows if r[0].startswith(prefixes)]):.3f}")
    assert not KR.failures(rows), KR.failures(rows)
    for c in range(KR.FIXTURE_CALLS):
        for key in f["state_dict_keys"].tolist():
            if key.endswith("num_batches_tracked"):
                assert int(got[f"after.{key}.{c}"]) == c + 1, key
    # the second call: the same bits in everything but the buffers
    for name, val in got.items():
        if name.endswith(".1") and not name.startswith("after."):
            assert val.tobytes() == got[name[:-2] + ".0"].tobytes(), name
    # a fresh model gives the same bits again
    again = run_fixture_calls(native_model(sd))
    for name, val in got.items():
        assert val.tobytes() == again[name].tobytes(), name
    # from_line_transformer copies a model, or a state dict, key for key
    from linetr_amd.train_ops import TrainableLineTransformer
    copy = TrainableLineTransformer.from_line_transformer(mod)
    assert all(torch.equal(v, copy.state_dict()[k]) for k, v in mod.state_dict().items()) and next(copy.parameters()).is_cuda


def run_native_loss(lr=None):
    import linetr_amd.evaluations as E
    sd, v0, v1, assign = KR.loss_case()
    mod = native_model(sd)
    crit = E.descriptor_loss()
    d0, d1 = KR.data_tensors(v0, torch.float32, "cuda"), KR.data_tensors(v1, torch.float32, "cuda")
    target = {"mat_assign_sublines": dev(assign)}
    with torch.enable_grad():
        loss = crit({"line_desc0": mod(d0)["line_desc"], "line_desc1": mod(d1)["line_desc"]}, target)[0]
        loss.backward()
    out = {"loss": float(loss.detach()), "V": crit.last["count"], "d_desc0": d0["desc_sublines"].grad.cpu().numpy(),
           "d_desc1": d1["desc_sublines"].grad.cpu().numpy()}
    for key, p in mod.named_parameters():
        assert p.grad is not None, key
        out[key] = p.grad.cpu().numpy()
    if lr is not None:
        with torch.no_grad():
            for p in mod.parameters():
                p -= lr * p.grad
            out["line_desc_eval"] = mod.eval()(KR.data_tensors(v0, torch.float32, "cuda", grad=False))["line_desc"].cpu().numpy()
    return out


def test_loss_backward_fills_the_whole_network():
    """the model on two views under descriptor_loss at B = 2, n = 33, S = 21 with a planted ground truth: the loss, the anchors, the gradient
    of both views' desc_sublines and of all 153 parameters; a second run gives the same bits; one SGD step followed by an .eval() forward
    agrees with the same step taken by the restatement"""
    ref64, ref32 = KR.loss_refs()
    got = run_native_loss(lr=KR.LOSS_LR)
    again = run_native_loss()
    assert got["V"] == ref64["V"] and abs(got["loss"] - ref64["loss"]) <= 8 * max(abs(ref32["loss"] - ref64["loss"]), 2.0 ** -23 * ref64["loss"])
    arrays = lambda d: {k: v for k, v in d.items() if isinstance(v, np.ndarray)}
    assert len(arrays(got)) == 2 + 153 + 1
    for key, v in arrays(again).items():
        assert got[key].tobytes() == v.tobytes(), key
    assert again["loss"] == got["loss"]
    rows = check(arrays(got), arrays(ref64), arrays(ref32), "two views under the criterion")
    cls = [r for r in rows if r[0] == "klenc.cls_token"]
    assert np.abs(got["klenc.cls_token"]).max() > 1e-4 and len(cls) == 1
    print(f"keyline cls_token.grad: max |.| {np.abs(got['klenc.cls_token']).max():.3e}, error / bar {cls[0][1] / cls[0][2]:.3f}; "
          f"eval forward after one SGD step: error / bar {KR.worst([r for r in rows if r[0] == 'line_desc_eval']):.3f}")


def test_model_refusals_and_the_empty_return(eng):
    sd, inputs, _ = KR.model_case()
    mod = native_model(sd, dropout=0.1)
    with pytest.raises(RuntimeError, match="dropout"):
        mod(KR.data_tensors(inputs, torch.float32, "cuda"))
    out = mod.eval()(KR.data_tensors(inputs, torch.float32, "cuda", grad=False))          # dropout is the identity in eval mode
    assert out["line_desc"].shape == (2, 256, 5)
    mod = native_model(sd)
    ret = mod({"klines": torch.empty((0, 2, 2), device="cuda")})
    assert sorted(ret) == ["klines", "line_desc", "mat_klines2sublines", "sublines"] and ret["line_desc"].shape == (1, 256, 0)
    data = KR.data_tensors(inputs, torch.float32, "cuda")
    data["pnt_sublines"].requires_grad_()
    with pytest.raises(RuntimeError, match="pnt_sublines"):
        mod(data)
    one = {k: (v[:1, :1] if k != "klines" else v[:1]) for k, v in KR.data_tensors(inputs, torch.float32, "cuda").items()}
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        mod(one)                                                                        # a single line in the whole batch
    from linetr_amd.train_ops import KeylineEncoder, TrainableLineTransformer
    with pytest.raises(ValueError):
        KeylineEncoder(128)
    with pytest.raises(ValueError):
        TrainableLineTransformer({"descriptor_dim": 128})
