"""GPU: the photometric kernels (linetr_photometric / linetr_gaussian_blur, csrc/lt_photometric.h) between sentinel guards against the NumPy
restatement (tests/photometric_reference.py) on the cases of tests/photometric_cases.py: the exact stages bit for bit, the noise on seeds
with no pixel near a rounding boundary, float32 sums under their derived bars with the excused rule for what is quantised behind them, the
shade, batches, refusals, determinism and the Python surface."""
import json
import os

import numpy as np
import pytest
import torch

import photometric_cases as PC
import photometric_reference as R
from linetr_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD, MARKER = 64, -777.25
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def yaml_config():
    with open(os.path.join(ROOT, "tests", "golden", "homography_photometric.json")) as fh:
        return json.load(fh)


class Guarded:
    """a tensor carved out of a sentinel-filled pool, `shift` floats off the pool's natural alignment"""

    def __init__(self, shape, shift=0, fill=None):
        n = int(np.prod(shape))
        self.pool = torch.full((n + 2 * GUARD + shift,), MARKER, dtype=torch.float32, device="cuda")
        self.t = self.pool[GUARD + shift:GUARD + shift + n].view(shape)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)))

    def guards_intact(self):
        return bool((self.pool[:self.lo] == MARKER).all()) and bool((self.pool[self.hi:] == MARKER).all())

    def untouched(self):
        return bool((self.pool == MARKER).all())


def run_photo(eng, x, params, seed=PC.SEED, first=0, q=False, shift=0):
    """x [B,1,H,W] float32 through one native call into a guarded output (input and output `shift` floats off alignment)"""
    src = Guarded(x.shape, shift, fill=x)
    dst = Guarded(x.shape, shift)
    out = eng.photometric(src.t, R.to_records(params, nat.PHOTO_PARAMS_DTYPE), seed, quantise_out=q, out=dst.t, first=first)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.t.data_ptr() and dst.guards_intact() and src.guards_intact()
    o = dst.t.cpu().numpy()
    assert not (o == MARKER).any() and np.array_equal(src.t.cpu().numpy(), x)
    return o


def run_blur(eng, x, ksize, sigma, quantise, shift=0):
    src = Guarded(x.shape, shift, fill=x)
    dst = Guarded(x.shape, shift)
    eng.gaussian_blur(src.t, ksize, sigma, quantise=quantise, out=dst.t)
    torch.cuda.synchronize()
    assert dst.guards_intact() and src.guards_intact()
    o = dst.t.cpu().numpy()
    assert not (o == MARKER).any()
    return o


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def levels_of(out):
    """the levels of an output level / 255 (float32): exact for every integer level"""
    return np.rint(out.astype(np.float64) * 255.0)


def test_tiles_of_the_case_table_are_the_kernels(eng):
    t = eng.photometric_tile()
    assert (t["point"], t["row"], t["col"], t["max_radius"]) == (PC.POINT_TILE, PC.ROW_TILE, PC.COL_TILE, PC.MAX_RADIUS)


@pytest.mark.parametrize("shape", PC.POINT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_stages_and_noise_are_bit_exact(eng, shape):
    """stages 0, 1, 2, 4, 5 (integer-valued kernels) and the identity: zero differing elements; the Gaussian noise on seeds with no pixel
    inside the band: identity as well; every case also off the 16-byte alignment (the scalar loads give what the 16-byte loads give)"""
    H, W = shape
    for name in (*PC.EXACT, *PC.NOISE):
        c = PC.point_case(name, H, W)
        want = f32(c["ref"]["out"])
        for shift in (0, 1):
            got = run_photo(eng, c["x"][None, None], [c["p"]], shift=shift)[0, 0]
            assert same_bits(got, want), (name, shift, int((got != want).sum()))
    # all stages disabled: rint(255 x) / 255 bit for bit
    x = PC.point_case("identity", H, W)["x"]
    got = run_photo(eng, x[None, None], [R.make_params()])[0, 0]
    assert same_bits(got, (np.rint(255.0 * x.astype(np.float64)) / 255.0).astype(np.float32))
    # impulse positions and polarities are the host table's
    c = PC.point_case("impulse", H, W)
    words, pol = R.impulse_table(PC.SEED, 0, H, W)
    hit = words < np.uint32(PC.THR)
    got = levels_of(run_photo(eng, c["x"][None, None], [c["p"]])[0, 0])
    assert np.array_equal(got[hit], np.where(pol, 255.0, 0.0)[hit]) and np.array_equal(got[~hit], np.rint(255.0 * c["x"].astype(np.float64))[~hit])


@pytest.mark.parametrize("shape", PC.POINT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_blur_with_real_kernels(eng, shape):
    """every K: the quantised float32 sums against the float64 correlation under the excused rule, and against the restatement of the
    kernel's own order (float32 products and sums, unfused), which must be the same bits"""
    H, W = shape
    for name in PC.MOTION_REAL:
        c = PC.point_case(name, H, W)
        got = run_photo(eng, c["x"][None, None], [c["p"]])[0, 0]
        R.check_discrete(levels_of(got), R.quantise(c["ref"]["pre_motion"]), c["excused"], PC.SHARE, f"{name} {H}x{W} vs float64")
        assert same_bits(got, f32(c["ref"]["out"])), name


@pytest.mark.parametrize("shape", PC.BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gaussian_blur_alone(eng, shape):
    H, W = shape
    for ksize, sigma in PC.BLUR_KSIZES:
        c = PC.blur_case(H, W, ksize, sigma, False)
        got = run_blur(eng, c["x"][None, None], ksize, sigma, False, shift=ksize % 4 == 1)[0, 0]
        err = np.abs(got.astype(np.float64) - c["ref"])
        print(f"blur {H}x{W} ksize {ksize}: error / bar = {err.max() / max(c['bar'], 1e-300):.3f}" if c["bar"] else f"blur {H}x{W} ksize 1: {int((err != 0).sum())} differ")
        assert np.all(err <= c["bar"] + 2.0 ** -24 * np.abs(c["ref"])), (ksize, float(err.max()), c["bar"])     # + the float32 rounding of the result
        cq = PC.blur_case(H, W, ksize, sigma, True)
        gq = run_blur(eng, cq["x"][None, None], ksize, sigma, True)[0, 0]
        R.check_discrete(gq, R.quantise(cq["ref"]), cq["excused"], PC.SHARE, f"blur {H}x{W} ksize {ksize} quantised")


def test_gaussian_blur_batches_channels_and_the_chain(eng):
    """B = 4 (two carrier launches) x C = 3 with a ksize and sigma per image; stage 6 inside linetr_photometric equals the blur alone
    on the levels; an image without the stage passes through"""
    B, Cn, H, W = 4, 3, 33, 70
    x = np.stack([PC.blur_input(H + b, W, False)[:H] for b in range(B * Cn)]).reshape(B, Cn, H, W)
    ks, sg = np.array([1, 9, 31, 5], np.int32), np.array([0.0, 2.5, 0.0, 0.0])
    got = run_blur(eng, x, ks, sg, False)
    for b in range(B):
        ref = R.blur(x[b], int(ks[b]), float(sg[b]))
        err = np.abs(got[b].astype(np.float64) - ref)
        assert np.all(err <= PC.blur_bar(int(ks[b]), 255.0) + 2.0 ** -24 * np.abs(ref)), b
    assert same_bits(got[0], x[0])
    # in the chain: levels -> quantised blur -> / 255
    xs = np.stack([PC.image(("chain", b), H, W) for b in range(3)])[:, None]
    params = [R.make_params(R.BRIGHTNESS | R.BLUR, d=7, blur_ksize=9, blur_sigma=2.5), R.make_params(R.BRIGHTNESS, d=7),
              R.make_params(R.BLUR | R.SHADE, blur_ksize=5, t=0.0, shade_ksize=3)]
    out = run_photo(eng, xs, params)
    lev = R.quantise(R.quantise(255.0 * xs.astype(np.float64)) + 7.0)
    alone = run_blur(eng, lev.astype(np.float32), np.array([9, 1, 5], np.int32), np.array([2.5, 0.0, 0.0]), True)
    assert same_bits(levels_of(out)[0], alone[0].astype(np.float64)) and same_bits(levels_of(out)[1], lev[1])
    assert same_bits(levels_of(out)[2], run_blur(eng, R.quantise(255.0 * xs[2:3].astype(np.float64)).astype(np.float32), 5, 0.0, True)[0].astype(np.float64))


@pytest.mark.parametrize("shape", PC.SHADE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shade(eng, shape):
    H, W = shape
    for i, (kind, t, ksize, q) in enumerate(PC.SHADE):
        c = PC.shade_case(H, W, i)
        got = run_photo(eng, c["x"][None, None], [c["p"]], q=bool(q), shift=i % 2)[0, 0]
        ref = c["ref"]
        what = f"shade {H}x{W} {kind} t={t} ksize={ksize} q={q}"
        if t == 0.0 or kind == "none" or ksize == 1:
            assert same_bits(got, f32(ref["out"])), what          # nothing float32 in the way: the input levels (or an exact mask)
            continue
        if q:
            n_diff, _ = R.check_discrete(levels_of(got), np.floor(ref["shaded"]), c["excused"], PC.SHARE, what)
            assert np.all((got == f32(ref["out"])) | (levels_of(got) != np.floor(ref["shaded"]))), what
        else:
            err = np.abs(got.astype(np.float64) - ref["out"])
            bar = PC.shade_out_bar(ref, c["bar"])
            print(f"{what}: error / bar = {(err / np.maximum(bar, 1e-300)).max():.3f}")
            assert np.all(err <= bar), (what, float(err.max()))


@pytest.mark.parametrize("case", ((3, 33, 65, 0), (2 * PC.CARRY + 1, 20, 67, 5)), ids=("B3", "B7"))
def test_batches_equal_their_images_alone(eng, case):
    """different parameters per image (image 1 with every stage disabled), more images than one carrier launch takes, W % 4 != 0 on a base
    one float off: every image equals the restatement with its own key (seed, first + b) and the same image run alone; two calls give the
    same bits"""
    B, H, W, first = case
    c = PC.batch_case(B, H, W, first)
    got = run_photo(eng, c["x"], c["params"], first=first, shift=1)
    again = run_photo(eng, c["x"], c["params"], first=first, shift=0)
    assert same_bits(got, again)
    for b in range(B):
        p, ref = c["params"][b], c["refs"][b]
        alone = run_photo(eng, c["x"][b:b + 1], [p], first=first + b)
        assert same_bits(alone[0], got[b]), b
        assert same_bits(levels_of(run_photo(eng, c["x"][b:b + 1], [{**p, "stages": p["stages"] & ~R.SHADE}], first=first + b))[0, 0], ref["level"]), b
        if p["stages"] & R.SHADE:
            bar = PC.shade_out_bar(ref, abs(p["t"]) * ref["level"] / 255.0 * PC.mask_bar(p["shade_ksize"], ref["mask_blur"]))
            assert np.all(np.abs(got[b, 0].astype(np.float64) - ref["out"]) <= bar), b
        else:
            assert same_bits(got[b, 0], f32(ref["out"])), b
    assert same_bits(got[1, 0], (np.rint(255.0 * c["x"][1, 0].astype(np.float64)) / 255.0).astype(np.float32))
    other = run_photo(eng, c["x"], c["params"], seed=PC.SEED + 1, first=first)
    assert not same_bits(other, got) and same_bits(other[1], got[1])          # another seed: other bits, except where nothing is drawn


def test_refusals_launch_nothing(eng):
    L = eng._L
    B, H, W = 2, 8, 12
    src = torch.full((B, 1, H, W), 0.5, device="cuda")
    dst = Guarded((B, 1, H, W))
    need = L.linetr_photometric_workspace_bytes(B, 1, H, W)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    good = R.to_records([R.make_params(R.SHADE, ellipses=[(3, 3, 2.5, 1.5, 1, 0)], t=0.3, shade_ksize=5)] * B, nat.PHOTO_PARAMS_DTYPE)

    def photo(src_p=src.data_ptr(), B=B, H=H, W=W, params=good, seed=1, first=0, q=0, dst_p=dst.t.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=need):
        return L.linetr_photometric(None, src_p, B, H, W, nat.np_ptr(params) if params is not None else None, seed, first, q, dst_p, ws_p, ws_bytes, None)

    def planted(**fields):
        p = good.copy()
        for k, v in fields.items():
            p[1][k] = v
        return dict(params=p)
    bad = [dict(src_p=None), dict(dst_p=None), dict(ws_p=None), dict(params=None), dict(B=0), dict(H=0), dict(W=0), dict(seed=1 << 32), dict(q=2),
           dict(dst_p=src.data_ptr()), dict(src_p=src.data_ptr() + 2), dict(ws_p=ws.data_ptr() + 16), planted(stages=128), planted(K=2),
           planted(blur_ksize=4), planted(shade_ksize=2 * PC.MAX_RADIUS + 3), planted(n_ellipses=21), planted(alpha=np.nan), planted(sigma=-1.0)]
    for kw in bad:
        assert photo(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    assert photo(ws_bytes=need - 1) == nat.E_WORKSPACE
    ks, sg = np.array([3, 2 * PC.MAX_RADIUS + 1], np.int32), np.array([0.0, 1.5])

    def blur(src_p=src.data_ptr(), B=B, Cn=1, H=H, W=W, ks=ks, sg=sg, q=0, dst_p=dst.t.data_ptr(), ws_p=ws.data_ptr(), ws_bytes=need):
        return L.linetr_gaussian_blur(None, src_p, B, Cn, H, W, nat.np_ptr(ks), nat.np_ptr(sg), q, dst_p, ws_p, ws_bytes, None)
    for kw in (dict(src_p=None), dict(B=0), dict(Cn=0), dict(q=3), dict(ks=np.array([3, 2 * PC.MAX_RADIUS + 3], np.int32)), dict(ks=np.array([2, 3], np.int32)),
               dict(sg=np.array([-1.0, 0.0])), dict(dst_p=src.data_ptr())):
        assert blur(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    assert blur(ws_bytes=need - 1) == nat.E_WORKSPACE
    torch.cuda.synchronize()
    assert dst.untouched() and bool((src == 0.5).all()) and not bool(ws.any())
    with pytest.raises(RuntimeError, match="HIP device"):
        eng.photometric(src.cpu(), good, 1)
    with pytest.raises(ValueError):
        eng.photometric(src, good[:1], 1)
    with pytest.raises(nat.NativeError, match="ksize"):
        eng.gaussian_blur(src, 4)
    # and the same calls, unbroken, are served
    assert photo() == 0 and dst.guards_intact()
    torch.cuda.synchronize()
    assert not (dst.t == MARKER).any()
    assert blur() == 0
    torch.cuda.synchronize()
    assert bool(((dst.t - 0.5).abs() < 1e-5).all()) and dst.guards_intact()


def test_surface_on_the_reference_config(eng, yaml_config):
    """ImgAugTransform / customizedTransform on the reference's yaml dict: float and uint8 inputs of the accepted shapes, the same seed gives
    the same bits and another seed other bits, the two classes in turn equal the one-call chain, and augmented_views is the augmentation
    followed by homography_views"""
    from linetr_amd import homography, photometric as P
    from workloads import synth
    H, W = 60, 80
    x = PC.image("surface", H, W)
    xd = torch.from_numpy(x).cuda()
    aug, cus = P.ImgAugTransform(**yaml_config), P.customizedTransform()
    a = aug(xd, seed=11)
    assert a.shape == (H, W) and a.dtype == torch.float32 and torch.equal(a, aug(xd, seed=11)) and not torch.equal(a, aug(xd, seed=12))
    assert torch.equal(aug(xd[:, :, None], seed=11)[:, :, 0], a) and torch.equal(aug(xd[None, None], seed=11)[0, 0], a)
    lv = a.double() * 255
    assert bool((lv - lv.round()).abs().max() < 1e-4) and float(a.min()) >= 0 and float(a.max()) <= 1
    u8 = torch.from_numpy(np.rint(x * 255).astype(np.uint8)).cuda()
    assert torch.equal(aug(u8, seed=11), aug(u8.float() / 255, seed=11))
    s = cus(a, seed=11, **yaml_config)
    assert s.shape == (H, W) and torch.equal(s, cus(a, seed=11, **yaml_config)) and not torch.equal(s, cus(a, seed=12, **yaml_config))
    chain = P.augment(xd, yaml_config, seed=11, quantise_out=False)
    assert torch.equal(chain, s)                                     # the levels pass between the two classes exactly
    params = eng.photometric_params(yaml_config, 1, H, W, 11)
    ref = R.augment(x, R.sample(R.config_stages(yaml_config), 11, 0, 1, H, W)[0], 11, 0)
    assert same_bits(levels_of(a.cpu().numpy()), ref["level"]) and int(params["n_ellipses"][0]) == 20
    off = P.ImgAugTransform(photometric={"enable": False})
    assert same_bits(off(xd, seed=3).cpu().numpy(), (np.rint(255.0 * x.astype(np.float64)) / 255.0).astype(np.float32))
    assert torch.equal(cus(a, seed=3, photometric={"enable": True, "params": {"additive_shade": False}}), a)
    with pytest.raises(RuntimeError, match="HIP device"):
        aug(xd.cpu(), seed=1)
    # a pair
    batch = torch.stack([xd, xd.flip(0)])[:, None].contiguous()
    m = np.stack([synth.pixel_homography(np.random.RandomState(5 + b), H, W, strength=0.5) for b in range(2)])
    i0, i1, valid = P.augmented_views(batch, m, yaml_config, seed=21)
    want0 = P.augment(batch, yaml_config, seed=21)
    want1, want_valid = homography.homography_views(want0, m)
    assert torch.equal(i0, want0) and torch.equal(i1, want1) and torch.equal(valid, want_valid)
    assert torch.equal(i0[1], P.augment(batch[1:], yaml_config, seed=21, first=1)[0])
    lv = i0.double() * 255
    assert bool((lv - lv.round()).abs().max() < 1e-4)                # quantise_out: levels, as the builder's uint8 image


def test_pair_augmented_and_detected_on_the_device_trains(yaml_config):
    """augmented_views -> detect_batch -> Engine.prefilter -> fixed-size samples -> one training iteration up to the Adam step (the line
    detector's end-to-end test with the photometric stage in front)"""
    import keyline_reference as KR
    import linetr_amd.evaluations as E
    from test_gpu_producer import _Helpers, _StandInSuperPoint
    from workloads import synth
    from linetr_amd import homography as HG, photometric as P
    from linetr_amd.engine import Engine
    from linetr_amd.frontends.line_detector import LSD
    from linetr_amd.optim import Adam
    from linetr_amd.superpoint import FusedHeadSuperPoint
    from linetr_amd.train_ops import TrainableLineTransformer
    H, W = 480, 640
    pre = dict(remove_borders=8, min_length=16, max_keylines=-1, token_distance=8, max_tokens=21)
    gi = np.load(os.path.join(ROOT, "tests", "golden", "asset_pair_images.npz"))
    clean = torch.from_numpy(gi["gray0"].astype(np.float32) / 255.0)[None, None].cuda()
    m = synth.pixel_homography(np.random.RandomState(31), H, W, strength=0.5)
    image0, image1, valid1 = P.augmented_views(clean, m[None], yaml_config, seed=77)
    assert not torch.equal(image0, clean) and image0.shape == clean.shape and float(image0.min()) >= 0 and float(image0.max()) <= 1
    rows, offsets = LSD({}).detect_batch(torch.cat([image0, image1]))
    print(f"augmented pair: {offsets[1]} lines in the image, {offsets[2] - offsets[1]} in its view")
    assert offsets[1] > 30 and offsets[2] - offsets[1] > 15
    eng = Engine.heads_only("cuda:0")
    sp = _StandInSuperPoint()
    sp.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(0).items()})
    sp = FusedHeadSuperPoint(sp.cuda().eval(), helpers=_Helpers, native_encoder=True)
    with torch.no_grad():
        preds = [sp({"image": im}) for im in (image0, image1)]
    views = []
    for i, p in enumerate(preds):
        single = eng.prefilter([rows[offsets[i]:offsets[i + 1]]], H, W, valid_masks=[None if i == 0 else HG.prefilter_mask(valid1, 0)], **pre)
        r, k, n = (np.array(v, copy=True) for v in single)
        views.append(eng.fixed_size_batch(r, k, n, p["dense_descriptor"], p["dense_score"], max_sublines=300, token_distance=8, max_tokens=21, seed=3 + i))
    gt = eng.line_ground_truth(views[0]["sublines"], views[1]["sublines"], m[None])
    mod = TrainableLineTransformer({})
    mod.load_state_dict(KR.tensors(KR.loss_case()[0]), strict=True)
    mod = mod.cuda().train()
    params = list(mod.parameters())
    opt = Adam(params, lr=1e-3)
    crit = E.descriptor_loss()
    with torch.enable_grad():
        loss = crit({"line_desc0": mod(views[0])["line_desc"], "line_desc1": mod(views[1])["line_desc"]}, {"mat_assign_sublines": gt["assign"]})[0]
        loss.backward()
    before = [p.detach().clone() for p in params]
    opt.step()
    moved = sum(not torch.equal(p.detach(), q) for p, q in zip(params, before))
    print(f"augmented pair: loss {float(loss):.6f}, {int(gt['found'].sum())} ground-truth pairs, {moved} tensors moved by the step")
    assert np.isfinite(float(loss)) and int(gt["found"].sum()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params) and moved > 0
