"""GPU: the Python surface of the homography views (linetr_amd/homography.py): the reference-signature functions against the real
reference's outputs (tests/golden/warp.npz), homography_views on a real image through the native front end, and one training
iteration on a pair made on the device."""
import os

import numpy as np
import pytest
import torch

import keyline_reference as KR
import warp_reference as R
from test_gpu_producer import _Helpers, _StandInSuperPoint
from workloads import synth

pytestmark = pytest.mark.gpu

HW = (480, 640)
PRE = dict(remove_borders=8, min_length=16, max_keylines=-1, token_distance=8, max_tokens=21)


@pytest.fixture(scope="module")
def g():
    return R.fixture()


@pytest.fixture(scope="module")
def image0():
    gi = np.load(os.path.join(R.GOLDEN, "asset_pair_images.npz"))
    return torch.from_numpy(gi["gray0"].astype(np.float32) / 255.0)[None, None].cuda()


@pytest.fixture(scope="module")
def superpoint():
    from linetr_amd.superpoint import FusedHeadSuperPoint
    sp = _StandInSuperPoint()
    sp.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(0).items()})
    sp = sp.cuda().eval()
    for p in sp.parameters():
        p.requires_grad_(False)
    return FusedHeadSuperPoint(sp, helpers=_Helpers, native_encoder=True)


def check_case(g, c, bilinear, nearest, mask):
    """[B,C,H,W] / [B,H,W] NumPy results against the fixture's under the bars of tests/test_gpu_warp.py"""
    B, C, H, W = R.SHAPES[c]
    pix = R.normalised_to_pixel(g[f"mat_{c}"], H, W)
    for b in range(B):
        _, max_tap = R.warp(g[f"img_{c}"][b], pix[b], "bilinear")
        err = np.abs(bilinear[b].astype(np.float64) - g[f"bilinear_{c}"][b])
        assert np.all(err <= float(g[f"ref_dev_{c}"]) + R.BILINEAR_BAR * max_tap[None]), (c, b, float(err.max()))
        ex = R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_REF)
        R.check_discrete(nearest[b], g[f"nearest_{c}"][b], ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} nearest")
        R.check_discrete(mask[b], g[f"mask_{c}"][b].astype(np.float32), ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} mask")


@pytest.mark.parametrize("c", range(len(R.SHAPES)))
def test_reference_signature_functions_against_the_fixture(g, c):
    from linetr_amd import homography as HG
    B, C, H, W = R.SHAPES[c]
    img, mat = torch.from_numpy(g[f"img_{c}"]).cuda(), torch.from_numpy(g[f"mat_{c}"])
    out = {mode: HG.inv_warp_image_batch(img, mat, "cuda:0", mode) for mode in ("bilinear", "nearest")}
    mask = HG.compute_valid_mask((H, W), mat, "cuda:0", erosion_radius=0)
    for t in (*out.values(), mask):
        assert t.dtype == torch.float32 and t.device.type == "cuda"
    assert tuple(out["bilinear"].shape) == (B, C, H, W) and tuple(mask.shape) == (B, H, W)
    check_case(g, c, out["bilinear"].cpu().numpy(), out["nearest"].cpu().numpy(), mask.cpu().numpy())
    # matrices on the device, and the eroded mask: the square element on the un-eroded one
    assert torch.equal(HG.inv_warp_image_batch(img, mat.cuda(), "cuda:0"), out["bilinear"])
    eroded = HG.compute_valid_mask((H, W), mat, "cuda:0", erosion_radius=2)
    assert eroded.dtype == torch.float32 and np.array_equal(eroded.cpu().numpy(), R.erode(mask.cpu().numpy(), 2).astype(np.float32))


def test_single_image_inputs_of_the_reference(g):
    """the reference's 2-D and 3-D image inputs and a single 3x3 matrix (utils.py:335-338, 353-370)"""
    from linetr_amd import homography as HG
    c = 0
    B, C, H, W = R.SHAPES[c]
    img, mat = torch.from_numpy(g[f"img_{c}"]).cuda(), torch.from_numpy(g[f"mat_{c}"])
    batch = HG.inv_warp_image_batch(img, mat, "cuda:0")
    for b in range(B):
        two = HG.inv_warp_image_batch(img[b, 0], mat[b], "cuda:0")                     # [H,W], [3,3]
        three = HG.inv_warp_image_batch(img[b, 0][:, :, None], mat[b][None], "cuda:0")   # [H,W,1], [1,3,3]
        assert tuple(two.shape) == (1, 1, H, W) and torch.equal(two[0, 0], batch[b, 0]) and torch.equal(three, two)
        flat = HG.inv_warp_image(img[b, 0], mat[b], "cuda:0", "nearest")
        assert tuple(flat.shape) == (H, W) and torch.equal(flat, HG.inv_warp_image_batch(img[b:b + 1], mat[b], "cuda:0", "nearest")[0, 0])
    # scale_homography is the builder's formula (build_homography_dataset.py:123-127) in float64
    hn = g[f"mat_{c}"].astype(np.float64)
    trans = np.array([[2. / W, 0., -1.], [0., 2. / H, -1.], [0., 0., 1.]])
    scaled = HG.scale_homography(hn, (H, W), shift=(-1, -1))
    assert scaled.dtype == np.float64 and np.array_equal(scaled, np.linalg.inv(trans) @ hn @ trans)
    one = HG.compute_valid_mask((H, W), mat[1], "cuda:0")
    assert tuple(one.shape) == (1, H, W) and torch.equal(one[0], HG.compute_valid_mask((H, W), mat, "cuda:0")[1])


def lines_of_asset():
    return np.load(os.path.join(R.GOLDEN, "asset_pair.npz"))["lines0"]


def test_identity_view_is_the_image_and_everything_behind_it(image0, superpoint):
    from linetr_amd import homography as HG
    from linetr_amd.engine import Engine
    image1, valid1 = HG.homography_views(image0, np.eye(3)[None], erosion_radius=0)
    assert image1.dtype == torch.float32 and valid1.dtype == torch.uint8 and valid1.device == image0.device
    assert torch.equal(image1, image0) and image1.data_ptr() != image0.data_ptr()
    assert tuple(valid1.shape) == (1, *HW) and bool((valid1 == 1).all())
    eng = Engine(synth.calibrated_state_dict(), "cuda:0")
    lines = lines_of_asset()
    off = np.array([0, len(lines)], np.int32)
    outs = []
    with torch.no_grad():
        for im in (image0, image1):
            pred = superpoint({"image": im})
            tb, desc = eng.describe_lines(lines, off, pred["dense_descriptor"], pred["dense_score"], want_tokens=True, **PRE)
            outs.append((pred, tb, desc))
    (p0, tb0, d0), (p1, tb1, d1) = outs
    for key in ("dense_score", "dense_descriptor", "dense_descriptor_nhwc"):
        assert torch.equal(p0[key], p1[key]), key
    assert torch.equal(p0["keypoints"][0], p1["keypoints"][0]) and torch.equal(p0["descriptors"][0], p1["descriptors"][0])
    for key in ("klines", "sublines", "pnt", "mask", "resp", "angle_sub", "desc", "score"):
        assert torch.equal(getattr(tb0, key), getattr(tb1, key)), key
    assert tb0.N > 200 and torch.equal(d0, d1)


def test_pair_made_on_the_device_trains(image0, superpoint):
    """a pixel_homography(strength=0.5) view: the mask against the restatement, the pre-filter fed by it, and one training iteration"""
    import linetr_amd.evaluations as E
    from linetr_amd import homography as HG
    from linetr_amd.engine import Engine
    from linetr_amd.optim import Adam
    from linetr_amd.train_ops import TrainableLineTransformer
    H, W = HW
    m = synth.pixel_homography(np.random.RandomState(31), H, W, strength=0.5)
    image1, valid1 = HG.homography_views(image0, m[None], erosion_radius=2)
    # ---- the mask
    inv = np.linalg.inv(m)
    want_mask = R.erode(R.valid_mask(inv, H, W), 2)
    ex = R.near_rounding_boundary(inv, H, W, R.EXCUSE_F64)
    ex_wide = R.erode(~ex, 2) == 0                                # a pixel whose 5 x 5 window holds an excused one
    R.check_discrete(valid1[0].cpu().numpy(), want_mask, ex_wide, 25 * R.EXCUSE_F64_SHARE, "eroded mask of the view")
    assert 0.5 < want_mask.mean() < 0.98
    want_img, max_tap = R.warp(image0[0].cpu().numpy(), inv, "bilinear")
    assert np.all(np.abs(image1[0].cpu().numpy() - want_img) <= R.BILINEAR_BAR * max_tap[None])
    # ---- the pre-filter: image 0's lines seen through m, and fresh lines all over image 1
    eng = Engine.heads_only("cuda:0")
    lines0 = lines_of_asset()
    ends = synth.warp_points(m, lines0[:, :4].reshape(-1, 2, 2)).astype(np.float32).astype(np.float64)
    warped = np.concatenate([ends.reshape(-1, 4), np.float32(np.hypot(*(ends[:, 1] - ends[:, 0]).T))[:, None].astype(np.float64),
                             np.zeros((len(ends), 1))], axis=1)
    # at strength 0.5 the invalid area hugs the border the pre-filter removes anyway, and a line goes only when BOTH its end points
    # are invalid (models/line_process.py:76-80): plant lines between two invalid pixels inside the border band, 18 to 40 px apart
    ys, xs = np.nonzero(want_mask[12:H - 12, 12:W - 12] == 0)
    assert len(ys) > 1000
    pts = np.stack([xs + 12.0, ys + 12.0], axis=1)
    planted = []
    for i in np.random.RandomState(5).permutation(len(pts))[:20]:
        d = np.linalg.norm(pts - pts[i], axis=1)
        j = int(np.flatnonzero((d >= 18) & (d <= 40))[0])
        planted.append([*pts[i], *pts[j], float(np.float32(d[j])), 0.0])
    planted = np.asarray(planted)
    lines1 = np.concatenate([warped, synth.synth_lines(77, 60, H, W), planted])
    host_mask = HG.prefilter_mask(valid1, 0)
    assert host_mask.dtype == np.float64 and host_mask.shape == HW
    got = eng.prefilter([lines1], H, W, valid_masks=[host_mask], **PRE)
    want = eng.prefilter([lines1], H, W, valid_masks=[want_mask.astype(np.float64)], **PRE)
    free = eng.prefilter([lines1], H, W, **PRE)
    recs1, cu_k1, cu_n1 = (np.array(v, copy=True) for v in got)
    assert np.array_equal(recs1, np.array(want[0])) and np.array_equal(cu_n1, want[2])
    print(f"pre-filter: {int(free[1][1])} lines without the mask, {int(cu_k1[1])} with it")
    assert 100 < cu_k1[1] <= free[1][1] - 20
    recs0, cu_k0, cu_n0 = (np.array(v, copy=True) for v in eng.prefilter([lines0], H, W, **PRE))
    # ---- one training iteration on the pair
    M = 300
    with torch.no_grad():
        preds = [superpoint({"image": im}) for im in (image0, image1)]
    views = [eng.fixed_size_batch(r, k, n, p["dense_descriptor"], p["dense_score"], max_sublines=M, token_distance=8, max_tokens=21, seed=3 + i)
             for i, ((r, k, n), p) in enumerate(zip(((recs0, cu_k0, cu_n0), (recs1, cu_k1, cu_n1)), preds))]
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
    found = int(gt["found"].sum())
    print(f"pair made on the device: loss {float(loss):.6f}, {found} ground-truth pairs, {moved} tensors moved by the step")
    assert np.isfinite(float(loss)) and found > 20
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params) and moved > 0
    assert all(bool(torch.isfinite(p).all()) for p in params)
