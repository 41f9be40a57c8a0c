"""GPU: the SuperPoint head kernels (lt_producer.h: sp_desc_head_kernel and sp_score_head_kernel, NCHW and row form) alone against
float64 at the block edges of their grids -- the vector path with a ragged last block included --, bit-exact families, sentinels
behind the inputs and markers behind the outputs; and the refusal of pointers that are not 16-byte aligned by every entry point whose
kernels access them with 16-byte vectors.  Cases, references and the bar: tests/sample_cases.py."""
import numpy as np
import pytest
import torch

import sample_cases as S
from attn_cases import MARKER
from linetr_amd import _native as nat
from workloads import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
D = 256


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


def test_heads_every_shape_form_and_output_set(eng):
    """every head case through Engine.superpoint_heads and Engine.superpoint_heads_rows (row stride = row length and + 3), score only /
    NHWC only / NCHW only / all three; the row forms and the NHWC output bit-equal to the NCHW form's; the `sentinel` family through
    the C ABI: nothing outside the requested outputs is written"""
    rows = S.sweep_heads(eng)
    assert {r[1] for r in rows} >= {"normal", "onehot", "onehot65", "sentinel", "sentinel/markers", "normal/forms", "normal/layouts"}
    print("\n" + "\n".join(S.worst_lines(rows)))
    bad = S.failures(rows)
    assert not bad, "\n".join(bad[:20])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def marked(n, device="cuda:0"):
    """n marker floats with room for a view one float further on"""
    return torch.full((n + 4,), MARKER, dtype=torch.float32, device=device)


def off(t, on):
    """the tensor's address, one float further on when `on`"""
    return t.data_ptr() + (4 if on else 0)


def refused(L, code):
    assert code == nat.E_ARG, code
    assert "16-byte" in L.linetr_last_error().decode()


def untouched(*outs):
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == MARKER).all()), "a refused call wrote to an output"


def test_heads_refuse_misaligned_pointers(eng):
    L, st = eng._L, eng._stream()
    B, Hc, Wc = 1, 4, 8
    HW = Hc * Wc
    sl, dr = torch.zeros(65 * HW + 4, device="cuda"), torch.zeros(D * HW + 4, device="cuda")
    s, a, b = marked(64 * HW), marked(D * HW), marked(D * HW)
    for which in ("sl", "dr", "s", "a", "b"):
        refused(L, L.linetr_superpoint_heads(None, off(sl, which == "sl"), off(dr, which == "dr"), B, Hc, Wc, off(s, which == "s"),
                                             off(a, which == "a"), off(b, which == "b"), st))
    for which in ("s", "a", "b"):           # the rows are read scalar-wise: only the outputs are constrained
        refused(L, L.linetr_superpoint_heads_rows(None, off(sl, True), 65, off(dr, True), D, B, Hc, Wc, off(s, which == "s"),
                                                  off(a, which == "a"), off(b, which == "b"), st))
    untouched(s, a, b)
    assert L.linetr_superpoint_heads_rows(None, off(sl, True), 65, off(dr, True), D, B, Hc, Wc, off(s, False), off(a, False), off(b, False), st) == 0
    torch.cuda.synchronize()
    assert not bool((s[:64 * HW] == MARKER).any()) and not bool((a[:D * HW] == MARKER).any()) and bool((s[64 * HW:] == MARKER).all())


def test_samplers_refuse_misaligned_pointers(eng):
    L, st = eng._L, eng._stream()
    Hc, Wc, n = 4, 8, 4
    pts = torch.rand(n, 2, device="cuda") * 30
    dd = torch.zeros(Hc * Wc * D + 4, device="cuda")
    cu = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    out, ws = marked(n * D), marked(Hc * Wc * D + 64)
    for nhwc, which in ((1, "dd"), (1, "out"), (1, "ws"), (0, "out"), (0, "ws")):
        refused(L, L.linetr_sample_descriptors(None, pts.data_ptr(), n, off(dd, which == "dd"), Hc, Wc, 0, nhwc, off(out, which == "out"),
                                               off(ws, which == "ws"), ws.numel() * 4 - 16, st))
    for nhwc, which in ((1, "dd"), (1, "ws"), (0, "ws")):
        refused(L, L.linetr_point_descriptors(None, pts.data_ptr(), cu.data_ptr(), 1, n, off(dd, which == "dd"), Hc, Wc, 0, nhwc, out.data_ptr(),
                                              off(ws, which == "ws"), ws.numel() * 4 - 16, st))
    untouched(out, ws)


def token_setup(eng):
    """records of a few lines on two 64 x 96 images, their maps, and marker-filled token tensors"""
    from test_gpu_tokenizer_fuzz import BORDER, MIN_LEN, fuzz_lines
    H, W, T = 64, 96, 3
    lines = [fuzz_lines(4100 + i, 6, 8, T, hw=(H, W)) for i in range(2)]
    recs, cu_k, cu_n = eng.prefilter(lines, H, W, remove_borders=BORDER, min_length=MIN_LEN, max_keylines=-1, token_distance=8, max_tokens=T)
    K, N = int(cu_k[-1]), int(cu_n[-1])
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    dd = torch.zeros(2 * (H // 8) * (W // 8) * D + 4, device="cuda")
    ds = torch.zeros(2 * H * W, device="cuda")
    sizes = dict(klines=K * 4, length=K, angles=K * 2, sublines=N * 4, pnt=N * T * 2, mask=N * (T + 1), resp=N, angle_sub=N * 2, desc=N * T * D,
                 score=N * T)
    bufs = {k: marked(v) for k, v in sizes.items()}
    s2l = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    return dict(H=H, W=W, T=T, K=K, N=N, recs=recs, cu_n=np.ascontiguousarray(cu_n, dtype=np.int32), d_recs=d_recs, dd=dd, ds=ds, bufs=bufs, s2l=s2l)


def tokens_of(bufs, desc_off):
    t = nat.Tokens()
    for k, v in bufs.items():
        setattr(t, k, off(v, desc_off and k == "desc"))
    return t


def test_tokenize_refuses_misaligned_pointers(eng):
    L, st = eng._L, eng._stream()
    c = token_setup(eng)
    need = L.linetr_tokenize_workspace_bytes(2, c["H"], c["W"], c["N"])
    ws = marked(need // 4 + 64)
    for nhwc, which in ((1, "dd"), (1, "desc"), (1, "ws"), (0, "desc"), (0, "ws")):
        refused(L, L.linetr_tokenize(None, c["d_recs"].data_ptr(), c["K"], c["N"], 8.0, c["T"], off(c["dd"], which == "dd"), c["ds"].data_ptr(), 2,
                                     c["H"], c["W"], 0, 0, 0, nhwc, tokens_of(c["bufs"], which == "desc"), c["s2l"].data_ptr(),
                                     off(ws, which == "ws"), need, st))
    untouched(ws, *c["bufs"].values())
    assert bool((c["s2l"] == -7).all())


def test_describe_refuses_misaligned_pointers():
    from linetr_amd.engine import Engine
    eng = Engine(synth.calibrated_state_dict(), "cuda:0", image_shape=[64, 96])
    L, st = eng._L, eng._stream()
    c = token_setup(eng)
    n_real = int(c["recs"]["n_tok"][:c["K"]].sum())
    need = L.linetr_describe_workspace_bytes(eng._h, 2, c["H"], c["W"], c["N"], n_real)
    ws, ld = marked(need // 4 + 64), marked(c["N"] * D)
    args = lambda nhwc, which: (eng._h, c["d_recs"].data_ptr(), c["K"], c["N"], n_real, nat.np_ptr(c["cu_n"]), None, 2, 8.0, c["T"],
                                off(c["dd"], which == "dd"), c["ds"].data_ptr(), c["H"], c["W"], 0, nhwc, tokens_of(c["bufs"], which == "desc"),
                                c["s2l"].data_ptr(), ld.data_ptr(), off(ws, which == "ws"), need)
    for nhwc, which in ((1, "dd"), (1, "desc"), (1, "ws"), (0, "desc"), (0, "ws")):
        refused(L, L.linetr_describe(*args(nhwc, which), st))
        refused(L, L.linetr_describe_submit(*args(nhwc, which), 0, 2, st))
    untouched(ws, ld, *c["bufs"].values())
    assert bool((c["s2l"] == -7).all())
    eng.close()


# ---- the Python wrappers keep accepting any view ---------------------------------------------------------------------------------

def shifted(t):
    """the same values as a contiguous view one float into its storage: data_ptr() % 16 == 4"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_wrappers_accept_views_at_odd_offsets(eng):
    case = S.head_case("normal", (4, 8), 3)
    sl, dr = case["logits"].cuda(), case["raw"].cuda()
    want = eng.superpoint_heads(sl, dr, nhwc=True, nchw=True)
    got = eng.superpoint_heads(shifted(sl), shifted(dr), nhwc=True, nchw=True)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    sc = S.sampler_case("border", (7, 9), False)
    pts = sc["points"].cuda()
    for layout in ("nhwc", "nchw"):
        m = S._layout(sc["dense"], layout)[0].cuda()
        want = eng.sample_descriptors(pts, m, dense_layout=layout)
        assert torch.equal(want, eng.sample_descriptors(shifted(pts), shifted(m), dense_layout=layout))
    from test_gpu_tokenizer_fuzz import BORDER, MIN_LEN, fuzz_lines
    dense, score = S.tokenize_maps()
    lines = [fuzz_lines(4200 + i, 6, 8, 3, hw=S.TOK_HW) for i in range(3)]
    pre = eng.prefilter(lines, *S.TOK_HW, remove_borders=BORDER, min_length=MIN_LEN, max_keylines=-1, token_distance=8, max_tokens=3)
    for layout in ("nhwc", "nchw"):
        m, s = S._layout(dense, layout).cuda(), score.cuda()
        a = eng.tokenize(*pre, m, s, token_distance=8, max_tokens=3, dense_layout=layout)
        b = eng.tokenize(*pre, shifted(m), shifted(s), token_distance=8, max_tokens=3, dense_layout=layout)
        assert torch.equal(a.desc, b.desc) and torch.equal(a.score, b.score) and torch.equal(a.pnt, b.pnt)
    kps = eng.superpoint_keypoints(score.cuda(), S._layout(dense, "nhwc").cuda(), nms_radius=4, keypoint_threshold=0.005, remove_borders=4,
                                   max_keypoints=-1, dense_layout="nhwc")
    kps2 = eng.superpoint_keypoints(shifted(score.cuda()), shifted(S._layout(dense, "nhwc").cuda()), nms_radius=4, keypoint_threshold=0.005,
                                    remove_borders=4, max_keypoints=-1, dense_layout="nhwc")
    assert sum(int(d.shape[1]) for d in kps[2]) > 0 and all(torch.equal(a, b) for a, b in zip(kps[2], kps2[2]))
