"""GPU: the neighbour-line attention's forward with statistics and its backward (csrc/lt_attnbwd.h; linetr_sig_attention_forward /
_backward; Engine.sig_attention_*; linetr_amd.train_ops.signature_attention / MultiHeadedAttention) against the float64 closed form that
tests/test_sig_attn_bwd_cpu.py pins to autograd through the reference (tests/sig_attn_bwd_reference.py, tests/golden/sig_attn_bwd.npz).

The bar of an output of an image is 8 x max(float32 CPU autograd error of the SAME image against float64, 2^-23 max |float64|); the
exact properties must hold bit for bit.  Measured on the MI355X: profiles/sig_attn_bwd_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load
import attn_cases as AC
import sig_attn_bwd_reference as SA

pytestmark = pytest.mark.gpu
E_ARG = -1
GRADS = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def model_eng():
    from linetr_amd.engine import Engine
    return Engine(AC.state_dict_t("calibrated")[0], "cuda:0")


@pytest.fixture(scope="module")
def L():
    from linetr_amd import _native as nat
    return nat.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_ratios(got, c, label):
    rows = SA.image_ratios(got, c)
    for key in SA.OUTPUTS:
        worst = max((e / b for _, _, k, e, b in rows if k == key and b > 0), default=0.0)      # (b = 0: dq, dk of one sub-line, exactly 0)
        print(f"sig_attn_bwd {label} {key}: worst error / bar {worst:.3f}")
    assert rows and not SA.failures(rows), SA.failures(rows)


@pytest.mark.parametrize("family", SA.FAMILIES)
def test_ragged_batch_within_the_bar(L, model_eng, family):
    """every tile edge in one var-len batch; q | k | v as column blocks of one buffer and as three buffers with ld = 260 give the same
    bits; the message has the bits of sig_attn_kernel (kernel 0 of linetr_debug_sig_attention) on pre-scaled q"""
    c = SA.case(family, SA.ragged_counts())
    got = SA.launch(L, c, "packed")
    check_ratios(got, c, family)
    apart = SA.launch(L, c, "apart")
    for key in SA.OUTPUTS:
        assert got[key].tobytes() == apart[key].tobytes(), (family, key)
    msg, used = AC.launch(model_eng, 0, AC.qkv_case(family, SA.ragged_counts()))
    assert used == 0 and msg.numpy().tobytes() == got["o"].tobytes()


def test_one_sub_line_is_exact(L):
    """n = 1: P = 1, so dq = dk = 0 and dv = dO, bit for bit (images of one sub-line between others)"""
    c = SA.case("normal", (1, 33, 1, 0, 1))
    got = SA.launch(L, c)
    dO = AC.to_kernel_layout(c["dO"]).numpy()
    for r in (0, 34, 35):
        assert not got["dq"][r].any() and not got["dk"][r].any() and np.array_equal(got["dv"][r], dO[r]), r
        assert np.array_equal(got["o"][r], AC.to_kernel_layout(c["v"]).numpy()[r])


@pytest.mark.parametrize("n", SA.POW2)
def test_equal_family_is_exact(L, n):
    """k = 0: dq is exactly 0; n a power of two (tests/sig_attn_bwd_reference.py: pow2_premise) and integer dO: every dv row of an
    (image, head) is the column sum of dO / n"""
    c = SA.case("equal", (n, 0, n), integer_dO=True)
    got = SA.launch(L, c)
    assert not got["dq"].any()
    dO = AC.to_kernel_layout(c["dO"]).numpy()
    for a in (0, n):
        want = (dO[a:a + n].astype(np.float64).sum(axis=0) / n).astype(np.float32)
        assert np.array_equal(got["dv"][a:a + n], np.broadcast_to(want, (n, 256))), (n, a)
    assert not SA.failures(SA.image_ratios(got, c))


def test_equal_family_dq_is_zero_at_every_size(L):
    c = SA.case("equal", SA.ragged_counts())
    assert not SA.launch(L, c)["dq"].any()


def test_two_calls_and_need_masks_give_identical_bits(L, eng):
    c = SA.case("normal", (65, 0, 257, 129))
    a, b = SA.launch(L, c), SA.launch(L, c)
    for key in SA.OUTPUTS:
        assert a[key].tobytes() == b[key].tobytes(), key
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        some = SA.launch(L, c, need=need, saved=a["_dev"])
        for key, n in zip(GRADS, need):
            assert (key in some) == n and (not n or some[key].tobytes() == a[key].tobytes()), (need, key)
    # the Engine: strided column blocks of one buffer as they are, another stream, other work in between
    N = int(c["cu"][-1])
    qkv = torch.cat([AC.to_kernel_layout(c[k]) for k in ("q", "k", "v")], dim=1).cuda()
    g = AC.to_kernel_layout(c["dO"]).cuda()
    cu = dev(c["cu"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o, lse = eng.sig_attention_forward(qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], cu)
        dq, dk, dv = eng.sig_attention_backward(qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], o, lse, g, cu)
    side.synchronize()
    assert o.shape == (N, 256) and lse.shape == (N, 4)
    for key, t in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert t.cpu().numpy().tobytes() == a[key].tobytes(), key
    only = eng.sig_attention_backward(qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], o, lse, g, c["cu"], need=(False, False, True))
    assert only[0] is None and only[1] is None and torch.equal(only[2], dv)


def test_argument_errors(L):
    N, n_img = 70, 2
    z = lambda *s: torch.zeros(s, device="cuda")
    q, k, v, o, g, lse = z(N, 256), z(N, 256), z(N, 256), z(N, 256), z(N, 256), z(N, 4)
    cu = dev(np.array([0, 33, 70], np.int32))
    outs = [torch.full((N, 256), 7.0, device="cuda") for _ in range(4)] + [torch.full((N, 4), 7.0, device="cuda")]
    msg, dq, dk, dv, lse_out = outs
    need = L.linetr_sig_attention_backward_workspace_bytes(N)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def fwd(q_=q, ldq=256, k_=k, ldk=256, v_=v, ldv=256, cu_=cu, n_=n_img, N_=N, o_=msg, ldo=256, lse_=lse_out):
        return L.linetr_sig_attention_forward(None, ptr(q_), ldq, ptr(k_), ldk, ptr(v_), ldv, ptr(cu_), n_, N_, ptr(o_), ldo, ptr(lse_), st())

    def bwd(q_=q, ldq=256, k_=k, ldk=256, v_=v, ldv=256, o_=o, ldo=256, lse_=lse, g_=g, ldg=256, cu_=cu, n_=n_img, N_=N, dq_=dq, lddq=256,
            dk_=dk, lddk=256, dv_=dv, lddv=256, ws_=ws, nbytes=None):
        return L.linetr_sig_attention_backward(None, ptr(q_), ldq, ptr(k_), ldk, ptr(v_), ldv, ptr(o_), ldo, ptr(lse_), ptr(g_), ldg, ptr(cu_),
                                               n_, N_, ptr(dq_), lddq, ptr(dk_), lddk, ptr(dv_), lddv, ptr(ws_),
                                               ws.numel() if nbytes is None else nbytes, st())

    off = lambda t: t.view(-1)[1:]                                               # 4 bytes past a 16-byte boundary
    refused = [fwd(q_=None), fwd(k_=None), fwd(v_=None), fwd(cu_=None), fwd(o_=None), fwd(lse_=None), fwd(ldq=252), fwd(ldk=258), fwd(ldv=0),
               fwd(ldo=255), fwd(q_=off(q)), fwd(k_=off(k)), fwd(v_=off(v)), fwd(o_=off(msg)), fwd(lse_=off(lse_out)), fwd(n_=0), fwd(n_=-1),
               fwd(n_=4097), fwd(N_=-1),
               bwd(q_=None), bwd(k_=None), bwd(v_=None), bwd(o_=None), bwd(lse_=None), bwd(g_=None), bwd(cu_=None), bwd(ws_=None),
               bwd(ldq=252), bwd(ldk=258), bwd(ldv=128), bwd(ldo=254), bwd(ldg=257), bwd(lddq=252), bwd(lddk=2), bwd(lddv=259),
               bwd(q_=off(q)), bwd(k_=off(k)), bwd(v_=off(v)), bwd(o_=off(o)), bwd(lse_=off(lse)), bwd(g_=off(g)), bwd(dq_=off(dq)),
               bwd(dk_=off(dk)), bwd(dv_=off(dv)), bwd(ws_=off(ws)), bwd(n_=0), bwd(n_=4097), bwd(N_=-2), bwd(nbytes=need - 1), bwd(nbytes=0)]
    assert refused == [E_ARG] * len(refused), refused
    assert L.linetr_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 7.0).all()                                                  # nothing was launched
    # legal: absent outputs (their strides are not read), images of no sub-lines, a batch of no rows
    assert fwd() == 0 and bwd() == 0 and bwd(dq_=None, lddq=0, dk_=None, lddk=0, dv_=None, lddv=0) == 0
    empty = dev(np.array([0, 0, 0], np.int32))
    assert fwd(cu_=empty, N_=0) == 0 and bwd(cu_=empty, N_=0) == 0
    torch.cuda.synchronize()
    for t in (msg, dq, dk, dv):
        assert not t.any()                                                       # v = 0 and dO = 0: zeros everywhere
    assert torch.allclose(lse_out[:33], torch.full((33, 4), float(np.log(33.0)), device="cuda"), rtol=0, atol=1e-6)   # all scores 0: lse = log n


def check_against(got, ref64, ref32, label):
    worst = 0.0
    for key, val in got.items():
        bar, err = SA.bar_of(ref32[key], ref64[key]), np.abs(val.astype(np.float64) - ref64[key]).max()
        worst = max(worst, err / bar)
        print(f"sig_attn_bwd {label} {key}: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert val.shape == ref64[key].shape and err <= bar, (label, key, err, bar)
    return worst


def test_signature_attention_against_the_fixture(eng):
    from linetr_amd.train_ops import signature_attention
    f = load("sig_attn_bwd")
    q, k, v = (dev(f[key]).requires_grad_() for key in ("q", "k", "v"))
    with torch.enable_grad():
        o = signature_attention(q, k, v)
        assert o.shape == (2, 64, 4, 33) and o.grad_fn is not None
        o.backward(dev(f["dO"]))
    for key, t in (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        ref = f[key]
        bar = SA.FACTOR * max(float(f[f"{key}_f32_err"]), 2.0 ** -23 * np.abs(ref).max())
        err = np.abs(t.cpu().double().numpy() - ref).max()
        print(f"sig_attn_bwd fixture {key}: err {err:.3e}, bar {bar:.3e}, err/bar {err / bar:.3f}")
        assert t.shape == ref.shape and err <= bar, (key, err, bar)
    # only value requires a gradient
    v2 = dev(f["v"]).requires_grad_()
    with torch.enable_grad():
        signature_attention(dev(f["q"]), dev(f["k"]), v2).backward(dev(f["dO"]))
    assert torch.equal(v2.grad, v.grad)


@pytest.mark.parametrize("shared", (False, True))
def test_multi_headed_attention_module(eng, shared):
    """message, input gradients and the eight parameter gradients against float64 autograd of the module on rows (torch_mha)"""
    from linetr_amd.train_ops import MultiHeadedAttention
    sd, x, src, g = SA.mha_case(shared=shared)
    mod = MultiHeadedAttention.from_line_transformer({"selfattn.layers.1.attn." + key: torch.from_numpy(val) for key, val in sd.items()}, layer=1).cuda()
    assert sorted(mod.state_dict()) == sorted(SA.MHA_KEYS)
    assert all(tuple(t.shape) == ((256, 256, 1) if key.endswith("weight") else (256,)) for key, t in mod.state_dict().items())
    xt = dev(x).requires_grad_()
    st = xt if shared else dev(src).requires_grad_()
    with torch.enable_grad():
        msg, prob = mod(xt, st, st)
        assert prob is None and msg.shape == x.shape and msg.grad_fn is not None
        msg.backward(dev(g))
    got = {"message": msg.detach(), "d_query": xt.grad, **{key: p.grad for key, p in mod.named_parameters()}}
    if not shared:
        got["d_source"] = st.grad
    assert all(t is not None for t in got.values())
    ref64, ref32 = SA.torch_mha(sd, x, src, g, torch.float64, shared), SA.torch_mha(sd, x, src, g, torch.float32, shared)
    assert sorted(got) == sorted(ref64)
    check_against({key: t.cpu().numpy() for key, t in got.items()}, ref64, ref32, f"MultiHeadedAttention shared={shared}")


def test_module_refuses_other_shapes():
    from linetr_amd.train_ops import MultiHeadedAttention, signature_attention
    for heads, width in ((8, 256), (4, 128), (2, 256)):
        with pytest.raises(ValueError):
            MultiHeadedAttention(heads, width)
    with pytest.raises(ValueError):
        signature_attention(torch.zeros(1, 32, 8, 5, device="cuda"), torch.zeros(1, 32, 8, 5, device="cuda"), torch.zeros(1, 32, 8, 5, device="cuda"))
