"""GPU: SuperPoint's key-point branch in native calls (Engine.superpoint_keypoints: linetr_superpoint_keypoints +
linetr_point_descriptors) against the fixtures frozen from the real reference and against the torch restatement of the branch
(test_gpu_producer._Helpers, pinned to the fixtures by test_keypoints_fixtures_cpu.py).  Key points and scores must be EQUAL, in
order; descriptors within DESC_TOL."""
import os

import numpy as np
import pytest
import torch

from test_gpu_producer import _Helpers, _StandInSuperPoint
from workloads import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DESC_TOL = 1e-6       # unit vectors; the bound of the same sampler against the same kind of fixture (test_gpu_line_process.py):
                      # the taps are torch's CPU kernel's bit for bit, only the 256-term norm is summed in another order


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


def reference(score, r, thr, border, k=-1):
    """The branch in torch on the device, per image: [(xy [n,2], val [n], row-major candidates before the top-k)].  The top-k is a
    stable descending sort (ties to the lower row-major index)."""
    B, H, W = score.shape
    nms = _Helpers.simple_nms(score, r)
    out = []
    for b in range(B):
        rc = torch.nonzero(nms[b] > thr)
        val = nms[b][rc[:, 0], rc[:, 1]]
        rc, val = _Helpers.remove_borders(rc, val, border, H, W)
        n_cand = int(rc.shape[0])
        if 0 <= k < n_cand:
            v = val.cpu().numpy()
            order = torch.from_numpy(np.lexsort((np.arange(n_cand), -v.astype(np.float64)))[:k].copy()).to(rc.device)
            rc, val = rc[order], val[order]
        out.append((rc.flip(1).float().cpu().numpy(), val.cpu().numpy(), n_cand))
    return out


def check_equal(eng, score, r, thr, border, k=-1, tag=""):
    kps, scs, descs = eng.superpoint_keypoints(score, None, nms_radius=r, keypoint_threshold=thr, remove_borders=border, max_keypoints=k)
    assert descs is None and len(kps) == len(scs) == score.shape[0]
    want = reference(score, r, thr, border, k)
    for b, (xy, val, _) in enumerate(want):
        have_xy, have_v = kps[b].cpu().numpy(), scs[b].cpu().numpy()
        assert have_xy.shape == xy.shape and have_v.shape == val.shape, (tag, b, have_xy.shape, xy.shape)
        assert np.array_equal(have_xy, xy), (tag, b)
        assert np.array_equal(have_v, val), (tag, b)
    return want


def family(name, B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if name == "uniform":
        return torch.rand(B, H, W, device="cuda", generator=g)
    if name == "normal":        # negative scores: suppressed zeros beat negative neighbours
        return torch.randn(B, H, W, device="cuda", generator=g)
    if name == "quantised":     # plateaus
        return torch.floor(torch.rand(B, H, W, device="cuda", generator=g) * 16) / 16
    if name == "constant":
        return torch.full((B, H, W), 0.25, device="cuda")
    return torch.zeros(B, H, W, device="cuda")


def sample_desc_ok(have, want):
    return have.shape == want.shape and np.abs(have - want).max() <= DESC_TOL


def test_reference_fixture_without_topk(eng):
    g = np.load(os.path.join(GOLD, "superpoint_heads.npz"))
    score = torch.from_numpy(g["dense_score"]).cuda()
    nchw = torch.from_numpy(g["dense_descriptor"]).cuda()
    for layout, dd in (("nchw", nchw), ("nhwc", nchw.permute(0, 2, 3, 1).contiguous())):
        kps, scs, descs = eng.superpoint_keypoints(score, dd, nms_radius=4, keypoint_threshold=0.005, remove_borders=4, max_keypoints=-1,
                                                   align_corners=False, dense_layout=layout)
        for b in range(2):
            assert np.array_equal(kps[b].cpu().numpy(), g[f"keypoints{b}"])
            assert np.array_equal(scs[b].cpu().numpy(), g[f"scores{b}"])
            d = descs[b].cpu().numpy()
            print(layout, b, "descriptor max-abs error", np.abs(d - g[f"descriptors{b}"]).max())
            assert sample_desc_ok(d, g[f"descriptors{b}"])


def test_reference_fixture_topk_on_real_image_statistics(eng):
    g = np.load(os.path.join(GOLD, "asset_pair.npz"))
    score = torch.from_numpy(np.concatenate([g["dense_score0"], g["dense_score1"]])).cuda()
    dd = torch.from_numpy(np.concatenate([g["dense_descriptor0"], g["dense_descriptor1"]])).cuda()
    kps, scs, descs = eng.superpoint_keypoints(score, dd, nms_radius=4, keypoint_threshold=0.005, remove_borders=4, max_keypoints=1024,
                                               align_corners=False, dense_layout="nchw")
    for b in range(2):
        assert np.array_equal(kps[b].cpu().numpy(), g[f"keypoints{b}"])
        d = descs[b].cpu().numpy()
        print(b, "descriptor max-abs error", np.abs(d - g[f"descriptors{b}"]).max())
        assert d.shape == (256, 1024) and sample_desc_ok(d, g[f"descriptors{b}"])
        xy = kps[b].long()
        assert torch.equal(scs[b], score[b][xy[:, 1], xy[:, 0]])


FAMILIES = ("uniform", "normal", "quantised", "constant", "zero")


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 37, 53), (3, 480, 640)])
def test_exact_against_torch_full_cross(eng, B, H, W):
    for fam in FAMILIES:
        score = family(fam, B, H, W, 11)
        for r in (0, 1, 4, 8):
            for border in (0, 4, 8):
                check_equal(eng, score, r, 0.005, border, tag=(fam, r, border))


@pytest.mark.parametrize("B,H,W", [(2, 960, 1280), (128, 480, 640)])
def test_exact_against_torch_large(eng, B, H, W):
    for fam in ("uniform", "quantised"):
        check_equal(eng, family(fam, B, H, W, 12), 4, 0.005, 4, tag=fam)


def test_capacity_retry_on_ties(eng):
    """more key points than a tie-free map can hold: the detector reports the count and runs once more"""
    want = check_equal(eng, family("quantised", 1, 64, 96, 11), 4, 0.005, 0)
    assert want[0][2] > -(-64 // 5) * -(-96 // 5)
    want = check_equal(eng, family("constant", 1, 40, 56, 11), 4, 0.005, 0)
    assert want[0][2] == 40 * 56


def test_threshold_is_strict_and_float32(eng):
    score = family("uniform", 2, 64, 96, 13) * 0.02
    base = reference(score, 4, 0.005, 4)
    thr = float(np.sort(base[0][1])[len(base[0][1]) // 2])           # a kept point's own score: '>' drops it
    want = check_equal(eng, score, 4, thr, 4)
    assert want[0][2] < base[0][2] and thr not in want[0][1]
    score = family("uniform", 2, 64, 96, 13) * 0.004                  # everything below the threshold, then isolated peaks
    above = np.nextafter(np.float32(0.005), np.float32(1))
    score[:, ::9, ::9] = float(np.float32(0.005))                     # float32(0.005) in the map, threshold 0.005: not kept
    score[:, 4::9, 4::9] = float(above)                               # one ulp above: kept
    want = check_equal(eng, score, 1, 0.005, 0)
    for _, v, n_cand in want:
        assert n_cand == len(range(4, 64, 9)) * len(range(4, 96, 9)) and np.all(v == above)


@pytest.mark.parametrize("k", [1, 7, 64, 1024, 4096])
def test_topk_tie_contract(eng, k):
    for (B, H, W) in ((2, 64, 96), (2, 480, 640)):
        score = family("quantised", B, H, W, 14)
        want = check_equal(eng, score, 4, 0.005, 4, k=k)
        for xy, val, n_cand in want:
            assert len(val) == min(k, n_cand)
            if n_cand <= k:                                           # untouched: row-major order
                idx = xy[:, 1] * W + xy[:, 0]
                assert np.all(np.diff(idx) > 0)


def test_bad_arguments(eng):
    score = torch.rand(1, 16, 16, device="cuda")
    for kw in ({"max_keypoints": 4097}, {"nms_radius": 9}, {"max_keypoints": 0}, {"nms_radius": -1}, {"keypoint_threshold": -0.1}):
        with pytest.raises(ValueError):
            eng.superpoint_keypoints(score, None, **kw)


def test_empty_and_odd_shapes(eng):
    score = torch.rand(3, 32, 48, device="cuda")
    dd = torch.nn.functional.normalize(torch.randn(3, 4, 6, 256, device="cuda"), dim=-1)
    kps, scs, descs = eng.superpoint_keypoints(score, dd, keypoint_threshold=2.0)
    for b in range(3):
        assert kps[b].shape == (0, 2) and scs[b].shape == (0,) and descs[b].shape == (256, 0)
    kps, scs, descs = eng.superpoint_keypoints(score[:0], dd[:0])
    assert kps == [] and scs == [] and descs == []
    score[1] = 0.0                                                    # one empty image in a batch of three
    kps, scs, descs = eng.superpoint_keypoints(score, dd)
    assert kps[1].shape == (0, 2) and descs[1].shape == (256, 0) and kps[0].shape[0] > 0 and kps[2].shape[0] > 0
    want = reference(score, 4, 0.005, 4)
    for b in range(3):
        assert np.array_equal(kps[b].cpu().numpy(), want[b][0])
        assert descs[b].shape == (256, kps[b].shape[0])
    kps, scs, descs = eng.superpoint_keypoints(score)                 # score only
    assert descs is None and np.array_equal(kps[2].cpu().numpy(), want[2][0])


def test_descriptor_placement(eng):
    """var-len batch with uneven counts: every image's block equals the image run alone and Engine.sample_descriptors, bit for bit"""
    g = torch.Generator(device="cuda").manual_seed(15)
    score = torch.rand(3, 120, 160, device="cuda", generator=g)
    score[1, :, 40:] = 0.0
    score[2, 30:, :] = 0.0
    dd = torch.nn.functional.normalize(torch.randn(3, 15, 20, 256, device="cuda", generator=g), dim=-1)
    for align in (False, True):
        kps, scs, descs = eng.superpoint_keypoints(score, dd, align_corners=align)
        counts = [int(k.shape[0]) for k in kps]
        assert len(set(counts)) == 3 and min(counts) > 64
        for b in range(3):
            k1, s1, d1 = eng.superpoint_keypoints(score[b:b + 1], dd[b:b + 1], align_corners=align)
            assert torch.equal(k1[0], kps[b]) and torch.equal(s1[0], scs[b]) and torch.equal(d1[0], descs[b])
            rows = eng.sample_descriptors(kps[b], dd[b], align_corners=align, dense_layout="nhwc")
            assert torch.equal(rows.t(), descs[b])
            assert (descs[b].norm(dim=0) - 1).abs().max().item() < 1e-6


def test_repeatable(eng):
    score = family("uniform", 3, 480, 640, 11)
    dd = torch.nn.functional.normalize(torch.randn(3, 60, 80, 256, device="cuda"), dim=-1)
    runs = [eng.superpoint_keypoints(score, dd, max_keypoints=k) for k in (-1, -1, -1, 1024, 1024, 1024)]
    for first, others in ((runs[0], runs[1:3]), (runs[3], runs[4:])):
        for other in others:
            for part_a, part_b in zip(first, other):
                assert all(torch.equal(a, b) for a, b in zip(part_a, part_b))


def _standin(seed):
    sp = _StandInSuperPoint()
    sp.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(seed).items()})
    return sp.cuda().eval()


def test_wrapper_native_keypoints():
    from linetr_amd.superpoint import FusedHeadSuperPoint
    g = np.load(os.path.join(GOLD, "superpoint_heads.npz"))
    sp = _standin(int(g["weights_seed"]))
    image = {"image": torch.from_numpy(g["image"]).cuda()}
    default = FusedHeadSuperPoint(sp, helpers=_Helpers)
    native = FusedHeadSuperPoint(sp, helpers=_Helpers, native_keypoints=True, align_corners=True)     # _Helpers samples with True
    default(image)                                       # (the convolution library settles on its kernels during the first call)
    a, b = default(image), native(image)
    assert set(a) == set(b)
    for key in a:
        assert type(a[key]) is type(b[key]), key
    assert isinstance(b["keypoints"], list) and isinstance(b["scores"], tuple) and isinstance(b["descriptors"], list)
    if not torch.equal(a["dense_score"], b["dense_score"]):          # convolutions that differ from run to run: the native branch
        kps, scs, descs = native._keypoints_native(a["dense_score"], a["dense_descriptor_nhwc"])      # on the default run's own maps
        b = {"keypoints": kps, "scores": scs, "descriptors": descs}
    for i in range(2):
        assert torch.equal(a["keypoints"][i], b["keypoints"][i]) and a["keypoints"][i].shape[0] > 50
        assert torch.equal(a["scores"][i], b["scores"][i])
        err = (a["descriptors"][i] - b["descriptors"][i]).abs().max().item()
        print(i, "wrapper descriptor max-abs difference", err)
        assert b["descriptors"][i].shape == a["descriptors"][i].shape and err <= DESC_TOL


def test_matching_native_keypoints(monkeypatch):
    """Matching with config['native_keypoints'] against the default on the synthetic pair of test_matching_wraps_the_host_superpoint:
    same key points and line matches; point matches equal except on rows whose decision margin lies inside 4 x the measured
    difference of the two distance matrices, and those are at most 2 % of the rows."""
    import sys
    import types
    from test_gpu_dropin import LT_CFG, FakeLSD
    from linetr_amd.superpoint import FusedHeadSuperPoint

    class SuperPoint(_StandInSuperPoint):
        def __init__(self, config):
            super().__init__()
            self.config = {**self.config, "nn_threshold": 0.7, **config}
            self.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(0).items()})

    mod = types.ModuleType("models.superpoint")
    mod.SuperPoint = SuperPoint
    for fn in ("simple_nms", "remove_borders", "top_k_keypoints", "sample_descriptors"):
        setattr(mod, fn, getattr(_Helpers, fn))
    SuperPoint.__module__ = "models.superpoint"
    monkeypatch.setitem(sys.modules, "models.superpoint", mod)
    from models.matching import Matching
    lines = [synth.synth_lines(61, 80, 96, 128, 17.0, 60.0, margin=9.0), synth.synth_lines(62, 80, 96, 128, 17.0, 60.0, margin=9.0)]
    rs = np.random.RandomState(1)
    imgs = [torch.from_numpy(rs.rand(1, 1, 96, 128).astype(np.float32)).cuda() for _ in range(2)]
    preds = []
    for native in (False, True):
        cfg = {"auto_min_length": True, "linetransformer": {**LT_CFG}}
        if native:
            cfg["native_keypoints"] = True
        mt = Matching(cfg, lsd=FakeLSD(lines))
        assert isinstance(mt.superpoint, FusedHeadSuperPoint) and mt.superpoint.native_keypoints == native
        mt.superpoint.align_corners = True               # the stand-in module's sample_descriptors uses align_corners=True
        mt.linetransformer.load_state_dict(synth.to_torch_state_dict(synth.calibrated_state_dict()))
        mt = mt.eval().to("cuda")
        if not preds:
            mt.superpoint({"image": imgs[0]})            # (the convolution library settles on its kernels during the first call)
        preds.append(mt({"image0": imgs[0], "image1": imgs[1]}))
    a, b = preds
    assert set(a) == set(b)
    for s in "01":
        assert torch.equal(a["dense_score" + s], b["dense_score" + s]), "the convolutions are not repeatable: nothing to compare"
        assert torch.equal(a["keypoints" + s][0], b["keypoints" + s][0]) and a["keypoints" + s][0].shape[0] > 100
        assert torch.equal(a["scores" + s][0], b["scores" + s][0])
    assert torch.equal(a["matches_l"], b["matches_l"])
    da, db = a["matching_scores_p"][0].numpy().astype(np.float64), b["matching_scores_p"][0].numpy().astype(np.float64)
    ma, mb = a["matches_p"][0].numpy(), b["matches_p"][0].numpy()
    err = np.abs(da - db).max()
    bar = 4 * err
    two = np.sort(da, axis=1)[:, :2]
    col_two = np.sort(da, axis=0)[:2]
    col_tight = (col_two[1] - col_two[0]) < bar          # per column
    best = da.argmin(axis=1)
    excused = ((two[:, 1] - two[:, 0]) < bar) | col_tight[best] | (np.abs(two[:, 0] - 0.7) < bar)
    differ = np.any(ma != mb, axis=1)
    print("point-distance difference", err, "excused rows", int(excused.sum()), "of", len(excused), "differing rows", int(differ.sum()))
    assert not np.any(differ & ~excused)
    assert excused.sum() <= 0.02 * len(excused)
