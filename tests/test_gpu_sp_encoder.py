"""GPU: the native SuperPoint encoder (lt_spconv.h, linetr_sp.hip) -- every layer alone through linetr_sp_conv3x3 / linetr_sp_conv1a
against float64 at the tile's edges, the whole chain against the float64 restatement and the reference-generated fixture, the rows
entry point of the dense-map producer, and the `native_encoder` switches of FusedHeadSuperPoint and Matching.
Cases, references and the bar: sp_encoder_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sp_encoder_cases as S
from test_gpu_producer import _Helpers, _StandInSuperPoint
from workloads import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def tile(eng):
    return eng.sp_conv_tile()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared cases are read-only arrays


def guarded(shape, row_floats, fill=None, value=S.SENTINEL):
    """A tensor of `shape` between two guard regions of SPARE_ROWS rows (rounded up to 16 bytes) holding `value`; -> (whole buffer,
    the view, guard length).  fill: NumPy contents of the view (default: `value` everywhere)."""
    n = int(np.prod(shape))
    guard = -(-S.SPARE_ROWS * row_floats // 4) * 4
    buf = torch.full((2 * guard + n,), value, dtype=torch.float32, device="cuda")
    view = buf[guard:guard + n].view(*shape)
    if fill is not None:
        view.copy_(torch.from_numpy(np.array(fill, order="C")))
    return buf, view, guard


def guards_intact(buf, guard, value):
    n = buf.numel()
    return bool((buf[:guard] == value).all()) and bool((buf[n - guard:] == value).all())


def run_layer(eng, x, w, b, pool):
    """x [B,H,W,cin] NumPy through linetr_sp_conv3x3 between sentinel guards -> NumPy output; the output guards must be untouched"""
    B, H, W, cin = x.shape
    cout = w.shape[0]
    _, xv, _ = guarded(x.shape, W * cin, fill=x)
    oshape = (B, H // 2, W // 2, cout) if pool else (B, H, W, cout)
    obuf, ov, og = guarded(oshape, max(oshape[2], 1) * cout, value=S.MARKER)
    packed = eng.sp_conv3x3_pack(dev(w))
    # (an empty output -- pooling a single row or column -- still gets the address it would start at: torch gives an empty view none)
    eng.sp_conv3x3(xv, packed, dev(b), pool=pool, out=ov if ov.numel() else obuf[og:])
    torch.cuda.synchronize()
    assert guards_intact(obuf, og, S.MARKER), "the kernel wrote outside its output"
    return ov.cpu().numpy()


@pytest.mark.parametrize("pool", (0, 1))
@pytest.mark.parametrize("family", ("normal", "integers"))
@pytest.mark.parametrize("cin,cout", S.PAIRS)
def test_layer_alone_at_tile_edges(eng, tile, cin, cout, family, pool):
    worst = 0.0
    for H, W, B in S.sizes(*tile):
        x, w, b, r32, r64 = S.layer_case(family, cin, cout, B, H, W)
        if pool:
            r32, r64 = S.pool_ref(r32), S.pool_ref(r64)
        y = run_layer(eng, x, w, b, pool)
        assert y.shape == r64.shape, (H, W, B)
        if y.size == 0:                       # pooling a single row or column: nothing to write, nothing launched
            continue
        if family == "integers":
            assert np.array_equal(y.astype(np.float64), r64), (H, W, B)
        else:
            err, bar = np.abs(y - r64).max(), S.bar(r32, r64)
            worst = max(worst, err / bar)
            print(f"conv3x3 {cin}->{cout} pool={pool} B={B} {H}x{W}: error {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
            assert err <= bar, (H, W, B, err, bar)
    print(f"conv3x3 {cin}->{cout} pool={pool} {family}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("cin,cout", S.PAIRS)
def test_one_hot_taps_and_corners(eng, tile, cin, cout):
    H, W = tile[0] + 1, tile[1] + 1
    for tap in range(9):
        for corner in range(4):
            x, w, b = S.one_hot_inputs(cin, cout, H, W, tap, corner)
            pool = (tap + corner) % 2
            r64 = S.conv_ref(x, w, b, torch.float64)
            y = run_layer(eng, x, w, b, pool)
            assert np.array_equal(y.astype(np.float64), S.pool_ref(r64) if pool else r64), (tap, corner, pool)


@pytest.mark.parametrize("cin,cout", S.PAIRS)
def test_relu_of_all_negative_preactivations_is_exact_zero(eng, tile, cin, cout):
    H, W = tile[0] + 1, 2 * tile[1] + 1
    x, w, b, _, r64 = S.layer_case("negative", cin, cout, 3, H, W)
    pre = S.conv_ref(x, w, b, torch.float64, relu=False)
    assert pre.max() < 0 and not r64.any()
    for pool in (0, 1):
        y = run_layer(eng, x, w, b, pool)
        assert not y.any() and not np.signbit(y).any()


def test_layer_is_deterministic(eng, tile):
    x, w, b, _, _ = S.layer_case("normal", 128, 512, 3, 2 * tile[0] + 1, tile[1] + 1)
    for pool in (0, 1):
        assert np.array_equal(run_layer(eng, x, w, b, pool), run_layer(eng, x, w, b, pool))


@pytest.mark.parametrize("family", ("normal", "integers"))
def test_conv1a_alone(eng, tile, family):
    for H, W, B in S.sizes(*tile):
        img, w, b = S.conv1a_inputs(family, B, H, W)
        r32, r64 = S.conv1a_ref(img, w, b, torch.float32), S.conv1a_ref(img, w, b, torch.float64)
        _, iv, _ = guarded(img.shape, W, fill=img)
        obuf, ov, og = guarded((B, H, W, 64), W * 64, value=S.MARKER)
        eng.sp_conv1a(iv, dev(w), dev(b), out=ov)
        torch.cuda.synchronize()
        assert guards_intact(obuf, og, S.MARKER)
        y = ov.cpu().numpy()
        if family == "integers":
            assert np.array_equal(y.astype(np.float64), r64), (H, W, B)
        else:
            err, bar = np.abs(y - r64).max(), S.bar(r32, r64)
            print(f"conv1a B={B} {H}x{W}: error {err:.3e} bar {bar:.3e}")
            assert err <= bar, (H, W, B)


def test_refusals_leave_the_outputs_untouched(eng):
    """every LINETR_E_ARG condition of the header: status -1, nothing launched, the output still holds its marker"""
    import linetr_amd._native as nat
    L = eng._L
    st = eng._stream()
    x = torch.zeros(1, 4, 4, 64, device="cuda")
    w = torch.zeros(128 * 9 * 512, device="cuda")
    bias = torch.zeros(512, device="cuda")
    y = torch.full((1 * 4 * 4 * 512 + 8,), S.MARKER, device="cuda")
    img = torch.zeros(1, 1, 8, 8, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    ok = dict(x=p(x), B=1, H=4, W=4, cin=64, w=p(w), b=p(bias), cout=64, pool=0, y=p(y))

    def conv(**kw):
        a = {**ok, **kw}
        return L.linetr_sp_conv3x3(None, a["x"], a["B"], a["H"], a["W"], a["cin"], a["w"], a["b"], a["cout"], a["pool"], a["y"], st)
    bad = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(cin=32), dict(cin=256), dict(cout=65), dict(cin=128, cout=64), dict(pool=2),
           dict(pool=-1), dict(x=None), dict(w=None), dict(b=None), dict(y=None), dict(x=p(x, 4)), dict(w=p(w, 8)), dict(b=p(bias, 4)),
           dict(y=p(y, 4))]
    for kw in bad:
        assert conv(**kw) == nat.E_ARG, kw
    assert L.linetr_sp_conv3x3_pack_bytes(32, 64) == 0 and L.linetr_sp_conv3x3_pack_bytes(64, 64) == 64 * 64 * 9 * 4
    assert L.linetr_sp_conv3x3_pack(p(w), 32, 64, p(y), st) == nat.E_ARG
    assert L.linetr_sp_conv3x3_pack(None, 64, 64, p(y), st) == nat.E_ARG
    assert L.linetr_sp_conv3x3_pack(p(w), 64, 64, p(y, 4), st) == nat.E_ARG
    w1, b1 = torch.zeros(64 * 9, device="cuda"), torch.zeros(64, device="cuda")
    for args in ((p(img), 0, 8, 8, p(w1), p(b1), p(y)), (p(img), 1, 0, 8, p(w1), p(b1), p(y)), (None, 1, 8, 8, p(w1), p(b1), p(y)),
                 (p(img, 4), 1, 8, 8, p(w1), p(b1), p(y)), (p(img), 1, 8, 8, None, p(b1), p(y)), (p(img), 1, 8, 8, p(w1), p(b1), p(y, 4))):
        assert L.linetr_sp_conv1a(None, *args, st) == nat.E_ARG, args
    # the whole encoder
    sd = {k: dev(v) for k, v in synth.superpoint_state_dict(0).items()}
    enc = eng._sp_encoder(sd)
    need = L.linetr_sp_encoder_workspace_bytes(1, 8, 8)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    sc, de = y, torch.full((256 + 8,), S.MARKER, device="cuda")
    fw = lambda e=enc, im=p(img), B=1, H=8, W=8, s=p(sc), d=p(de), f=None, wsp=p(ws), nb=need: \
        L.linetr_sp_encoder_forward(e, im, B, H, W, s, d, f, wsp, nb, st)
    for kw in (dict(e=None), dict(B=0), dict(H=7), dict(W=7), dict(im=None), dict(s=None), dict(d=None), dict(wsp=None), dict(im=p(img, 4)),
               dict(s=p(sc, 4)), dict(d=p(de, 4)), dict(f=p(sc, 4)), dict(wsp=p(ws, 4)), dict(nb=need - 1)):
        assert fw(**kw) == nat.E_ARG, kw
    fresh = C.c_void_p()
    assert L.linetr_sp_encoder_create(0, C.byref(fresh)) == 0
    assert fw(e=fresh) == nat.E_ARG                            # no weights yet
    L.linetr_sp_encoder_destroy(fresh)
    assert L.linetr_superpoint_heads_rows(None, p(sc), 64, None, 0, 1, 1, 1, p(de), None, None, st) == nat.E_ARG       # stride < 65
    torch.cuda.synchronize()
    assert bool((y == S.MARKER).all()) and bool((de == S.MARKER).all())
    assert fw() == 0 and conv() == 0                           # and the accepted calls do run
    torch.cuda.synchronize()
    assert not bool((y == S.MARKER).all())


# ---- the whole chain -------------------------------------------------------------------------------------------------------------

def rows_as_nchw(rows, shape):
    B, Hc, Wc = shape
    return rows.reshape(B, Hc, Wc, -1).permute(0, 3, 1, 2).contiguous()


def encode(eng, image, sd):
    score, desc, shape, feat = eng.superpoint_encode(dev(image), {k: dev(v) for k, v in sd.items()}, return_feat=True)
    return rows_as_nchw(score, shape).cpu().numpy(), rows_as_nchw(desc, shape).cpu().numpy(), feat.cpu().numpy(), shape


def check_chain(eng, image, sd, r32, r64, tag):
    score, desc, feat, shape = encode(eng, image, sd)
    errs = {}
    for key, have in (("feat", feat), ("score_logits", score), ("desc_raw", desc)):
        assert have.shape == r64[key].shape, (tag, key, have.shape, r64[key].shape)
        err, bar = np.abs(have - r64[key]).max(), S.bar(r32[key], r64[key])
        print(f"{tag} {key}: max|ref64| {np.abs(r64[key]).max():.3f} error {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        assert err <= bar, (tag, key, err, bar)
        errs[key] = err
    return score, desc, errs


def test_chain_on_the_reference_fixture(eng):
    g = np.load(os.path.join(GOLD, "superpoint_heads.npz"))
    sd = synth.superpoint_state_dict(int(g["weights_seed"]))
    r32, r64 = S.chain_ref(g["image"], sd, torch.float32), S.chain_ref(g["image"], sd, torch.float64)
    score, desc, _ = check_chain(eng, g["image"], sd, r32, r64, "fixture 64x96")
    for key, have in (("score_logits", score), ("desc_raw", desc)):      # the reference's own float32 run, transposed back
        room = S.bar(r32[key], r64[key]) + np.abs(r32[key] - r64[key]).max()
        err = np.abs(have.astype(np.float64) - g[key]).max()
        print(f"fixture {key}: error against the reference's run {err:.3e} room {room:.3e}")
        assert err <= room


def test_chain_on_an_odd_size(eng):
    """72 x 104 -> 36 x 52 -> 18 x 26 -> 9 x 13 cells: no multiple of the tile in cells, odd at the last level; 70 x 100 floors at
    two levels (35 x 50 -> 17 x 25 -> 8 x 12)"""
    for H, W in ((72, 104), (70, 100)):
        image, sd, r32, r64 = S.chain_case(H, W)
        check_chain(eng, image, sd, r32, r64, f"{H}x{W}")


def test_heads_rows_equal_heads_bit_for_bit(eng):
    image, sd, _, _ = S.chain_case(72, 104)
    score_rows, desc_rows, shape = eng.superpoint_encode(dev(image), {k: dev(v) for k, v in sd.items()})
    assert score_rows.stride(0) == 68 and tuple(score_rows.shape) == (2 * 9 * 13, 65)
    a = eng.superpoint_heads_rows(score_rows, desc_rows, shape, nhwc=True, nchw=True)
    b = eng.superpoint_heads(rows_as_nchw(score_rows, shape), rows_as_nchw(desc_rows, shape), nhwc=True, nchw=True)
    for x, y, name in zip(a, b, ("dense_score", "nhwc", "nchw")):
        assert x.shape == y.shape and torch.equal(x, y), name
    only = eng.superpoint_heads_rows(None, desc_rows, shape, nhwc=True)
    assert only[0] is None and only[2] is None and torch.equal(only[1], a[1])


def standin(seed=0):
    sp = _StandInSuperPoint()
    sp.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(seed).items()})
    sp = sp.cuda().eval()
    for p in sp.parameters():
        p.requires_grad_(False)
    return sp


def test_wrapper_native_encoder(eng):
    from linetr_amd.superpoint import FusedHeadSuperPoint
    g = np.load(os.path.join(GOLD, "superpoint_heads.npz"))
    sp = standin(int(g["weights_seed"]))
    image = {"image": dev(g["image"])}
    default = FusedHeadSuperPoint(sp, helpers=_Helpers)
    native = FusedHeadSuperPoint(sp, helpers=_Helpers, native_encoder=True)
    a, b = default(image), native(image)
    assert set(a) == set(b)
    for key in a:
        assert type(a[key]) is type(b[key]), key
        if torch.is_tensor(a[key]):
            assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and not b[key].requires_grad, key
    # the bar, propagated through the heads: the float64 / float32 restatement of softmax and normalize on the chain's references
    sd = synth.superpoint_state_dict(int(g["weights_seed"]))
    r32, r64 = S.chain_ref(g["image"], sd, torch.float32), S.chain_ref(g["image"], sd, torch.float64)
    h32, h64 = S.heads_ref(r32["score_logits"], r32["desc_raw"], torch.float32), S.heads_ref(r64["score_logits"], r64["desc_raw"], torch.float64)
    for key, i in (("dense_score", 0), ("dense_descriptor", 1)):
        bar = S.bar(h32[i], h64[i])
        e64 = np.abs(b[key].cpu().numpy() - h64[i]).max()
        eab = (a[key] - b[key]).abs().max().item()
        print(f"wrapper {key}: native vs float64 {e64:.3e}, native vs torch path {eab:.3e}, bar {bar:.3e}")
        assert e64 <= bar and eab <= bar, key
    assert torch.equal(b["dense_descriptor_nhwc"], b["dense_descriptor"].permute(0, 2, 3, 1))
    # the key-point branch is the wrapped module's own, on the native path's own maps: equality is exact
    kps, scs, descs = native._keypoints(b["dense_score"], b["dense_descriptor"], 64, 96)
    for i in range(2):
        assert torch.equal(kps[i], b["keypoints"][i]) and kps[i].shape[0] > 50
        assert torch.equal(scs[i], b["scores"][i]) and torch.equal(descs[i], b["descriptors"][i])


def test_weight_cache_sees_an_in_place_edit(eng):
    from linetr_amd.superpoint import FusedHeadSuperPoint
    g = np.load(os.path.join(GOLD, "superpoint_heads.npz"))
    sp = standin(0)
    native = FusedHeadSuperPoint(sp, helpers=_Helpers, native_encoder=True)
    image = {"image": dev(g["image"])}
    before = native(image)["dense_descriptor"].clone()
    assert torch.equal(before, native(image)["dense_descriptor"])           # cached weights: same bits
    with torch.no_grad():
        sp.conv3a.weight.mul_(-1.0)
    after = native(image)["dense_descriptor"]
    sd = {k: v.detach().cpu().numpy() for k, v in sp.state_dict().items()}
    r32, r64 = S.chain_ref(g["image"], sd, torch.float32), S.chain_ref(g["image"], sd, torch.float64)
    h32, h64 = S.heads_ref(r32["score_logits"], r32["desc_raw"], torch.float32), S.heads_ref(r64["score_logits"], r64["desc_raw"], torch.float64)
    assert (after - before).abs().max().item() > 1e-2
    assert np.abs(after.cpu().numpy() - h64[1]).max() <= S.bar(h32[1], h64[1])


def test_requires_grad_under_enabled_grad_raises(eng):
    from linetr_amd.superpoint import FusedHeadSuperPoint
    sp = standin(0)
    sp.conv2b.bias.requires_grad_(True)
    native = FusedHeadSuperPoint(sp, helpers=_Helpers, native_encoder=True)
    image = {"image": torch.rand(1, 1, 16, 16, device="cuda")}
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference only"):
            native(image)
    with torch.no_grad():
        out = native(image)
    assert not out["dense_score"].requires_grad and out["dense_score"].shape == (1, 16, 16)


def test_batch_above_the_workspace_cap_is_chunked(eng):
    image, sd, _, _ = S.chain_case(72, 104, B=5)
    w = {k: dev(v) for k, v in sd.items()}
    img = dev(image)
    whole = eng.superpoint_encode(img, w, return_feat=True)
    per_image = eng._L.linetr_sp_encoder_workspace_bytes(1, 72, 104)
    calls = []
    lib = eng._L
    real = lib.linetr_sp_encoder_forward

    class Spy:           # counts the native calls without changing them
        def __getattr__(self, name):
            if name == "linetr_sp_encoder_forward":
                return lambda *a: (calls.append(a[2]), real(*a))[1]
            return getattr(lib, name)
    eng._L = Spy()
    try:
        parts = eng.superpoint_encode(img, w, max_workspace_bytes=2 * per_image + 1, return_feat=True)
        tiny = eng.superpoint_encode(img, w, max_workspace_bytes=1)
    finally:
        eng._L = lib
    assert calls == [2, 2, 1] + [1] * 5
    for a, b in zip(whole, parts):
        assert a == b if isinstance(a, tuple) else torch.equal(a, b)
    assert torch.equal(whole[0], tiny[0]) and torch.equal(whole[1], tiny[1])
    odd = torch.rand(3, 1, 9, 9, device="cuda")              # 81 pixels: images 1 and 2 start off a 16-byte boundary
    a, b = eng.superpoint_encode(odd, w), eng.superpoint_encode(odd, w, max_workspace_bytes=1)
    assert a[2] == b[2] == (3, 1, 1) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_matching_native_encoder(monkeypatch):
    """Matching with config['native_encoder'] on the asset pair's grey images end to end: same keys and dtypes as the default; line
    matches agree on every row whose argmin margin exceeds 4x the measured difference of the two line-distance matrices."""
    import sys
    import types
    from test_gpu_dropin import LT_CFG, FakeLSD
    from linetr_amd.superpoint import FusedHeadSuperPoint

    class SuperPoint(_StandInSuperPoint):
        def __init__(self, config):
            super().__init__()
            self.config = {**self.config, "nn_threshold": 0.7, "max_keypoints": 1024, **config}
            self.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(0).items()})
            for p in self.parameters():
                p.requires_grad_(False)

    mod = types.ModuleType("models.superpoint")
    mod.SuperPoint = SuperPoint
    for fn in ("simple_nms", "remove_borders", "top_k_keypoints", "sample_descriptors"):
        setattr(mod, fn, getattr(_Helpers, fn))
    SuperPoint.__module__ = "models.superpoint"
    monkeypatch.setitem(sys.modules, "models.superpoint", mod)
    from models.matching import Matching
    g = np.load(os.path.join(GOLD, "asset_pair.npz"))
    gi = np.load(os.path.join(GOLD, "asset_pair_images.npz"))
    imgs = [dev(gi[k].astype(np.float32) / 255.0)[None, None] for k in ("gray0", "gray1")]
    preds = []
    for native in (False, True):
        cfg = {"auto_min_length": True, "linetransformer": {**LT_CFG}}
        if native:
            cfg["native_encoder"] = True
        mt = Matching(cfg, lsd=FakeLSD([g["lines0"], g["lines1"]]))
        assert isinstance(mt.superpoint, FusedHeadSuperPoint) and mt.superpoint.native_encoder == native
        mt.linetransformer.load_state_dict(synth.to_torch_state_dict(synth.calibrated_state_dict()))
        mt = mt.eval().to("cuda")
        with torch.no_grad():
            preds.append(mt({"image0": imgs[0], "image1": imgs[1]}))
    a, b = preds
    assert set(a) == set(b)
    for key in a:
        assert type(a[key]) is type(b[key]), key
        if torch.is_tensor(a[key]):
            assert a[key].dtype == b[key].dtype, key
    for s in "01":
        assert a["dense_score" + s].shape == b["dense_score" + s].shape == (1, 480, 640)
        print("image", s, "dense descriptor difference", (a["dense_descriptor" + s] - b["dense_descriptor" + s]).abs().max().item(),
              "key points", a["keypoints" + s][0].shape[0], b["keypoints" + s][0].shape[0])
    da, db = a["matching_scores_l"][0].numpy().astype(np.float64), b["matching_scores_l"][0].numpy().astype(np.float64)
    ma, mb = a["matches_l"][0].numpy(), b["matches_l"][0].numpy()
    assert da.shape == db.shape and ma.shape == mb.shape
    err = np.abs(da - db).max()
    margin = 4 * err
    thr = LT_CFG["nn_threshold"]
    two = np.sort(da, axis=1)[:, :2]
    col_two = np.sort(da, axis=0)[:2]
    col_tight = (col_two[1] - col_two[0]) < margin
    excused = ((two[:, 1] - two[:, 0]) < margin) | col_tight[da.argmin(axis=1)] | (np.abs(two[:, 0] - thr) < margin)
    differ = np.any(ma != mb, axis=1)
    print("line-distance difference", err, "rows", len(differ), "differing rows", int(differ.sum()), "excused rows", int(excused.sum()))
    assert not np.any(differ & ~excused)
