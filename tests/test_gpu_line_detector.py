"""GPU: the native line segment detector (csrc/lt_linedet.h) against its NumPy restatement (tests/line_detector_reference.py): the
labelling kernels alone on planted bucket maps between sentinels, the gradient kernel alone, the whole call on drawn scenes (counts, order
and integer moments exact, rows under a derived bar), capacity, determinism, refusals, and the Python surface up to Matching and one
training iteration on a pair whose pixels never leave the device.

The bar of the rows, 1e-6 * 2^octave px: the inputs of the fit are exact integers and the moments of inertia carry the restatement's bits
(no FMA contraction in det_fit_kernel); what differs is atan2 / sin / cos to a few ulp and contraction in the projections, about 1e-15
relative on extents of at most 2048 px: 1e-6 leaves six orders of magnitude."""
import os

import numpy as np
import pytest
import torch

import line_detector_cases as LC
import line_detector_reference as R
from linetr_amd import _native as nat

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 64
ROW_BAR = 1e-6


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def scenes():
    """name -> (image, rows, debug rows, counts per octave) of the restatement; computed once, never changed"""
    out = {}
    for name in LC.SCENE_NAMES:
        img = LC.scene(name)
        rows, regions, _ = R.detect(img, want_debug=True)
        out[name] = (img, rows, R.kept_debug_rows(regions), np.bincount(rows[:, 5].astype(int), minlength=2))
    return out


class Guarded:
    """an output tensor carved out of a sentinel-filled pool"""

    def __init__(self, shape, dtype, marker):
        n = int(np.prod(shape))
        self.pool = torch.full((n + 2 * GUARD,), marker, dtype=dtype, device="cuda")
        self.t = self.pool[GUARD:GUARD + n].view(shape)
        self.marker, self.n = marker, n

    def guards_intact(self):
        return bool((self.pool[:GUARD] == self.marker).all()) and bool((self.pool[GUARD + self.n:] == self.marker).all())

    def untouched(self):
        return bool((self.pool == self.marker).all())


def raw_detect(eng, images, capacity, debug=True, **config):
    """one linetr_detect_lines call into guarded buffers: (rows [B,cap,6], debug rows [B,cap,10] or None, counts [B,n_oct]) as NumPy,
    after checking the guards and that nothing beyond the reported rows was written"""
    img = eng._detect_images(images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images)).cuda())
    B, H, W = img.shape
    cfg = eng.detect_config(**config)
    rows = Guarded((B, max(capacity, 1), 6), torch.float64, -777.25)
    dbg = Guarded((B, max(capacity, 1), 10), torch.int64, -777) if debug else None
    counts = torch.full((B * cfg.n_octaves + 16,), -5, dtype=torch.int32).pin_memory()
    ws = torch.empty(max(eng._L.linetr_detect_lines_workspace_bytes(B, H, W, cfg.n_octaves), 256), dtype=torch.uint8, device="cuda")
    code = eng._L.linetr_detect_lines(None, img.data_ptr(), int(img.dtype != torch.uint8), B, H, W, nat.C.byref(cfg), capacity, rows.t.data_ptr(),
                                      counts.data_ptr(), dbg.t.data_ptr() if debug else None, ws.data_ptr(), ws.numel(), None)
    nat.check(code, eng._L)
    torch.cuda.synchronize()
    assert rows.guards_intact() and (dbg is None or dbg.guards_intact())
    c = counts.numpy()
    assert np.all(c[B * cfg.n_octaves:] == -5)
    c = c[:B * cfg.n_octaves].reshape(B, cfg.n_octaves).copy()
    r, d = rows.t.cpu().numpy(), dbg.t.cpu().numpy() if debug else None
    for b in range(B):
        n = min(int(c[b].sum()), capacity)
        assert not (r[b, :n] == -777.25).any() and (r[b, n:] == -777.25).all(), b
        assert d is None or (d[b, n:] == -777).all()
    return r, d, c


def check_against_restatement(r, d, c, b, want_rows, want_dbg, want_counts):
    n = len(want_rows)
    assert np.array_equal(c[b], want_counts), (c[b], want_counts)
    got = r[b, :n]
    assert np.array_equal(got[:, 5], want_rows[:, 5])                                  # octaves and, with the labels below, the order
    assert np.array_equal(d[b, :n], want_dbg)                                          # octave, partition, label, n and the six moments
    err = np.abs(got[:, :5] - want_rows[:, :5]) / np.exp2(want_rows[:, 5:6])
    worst = float(err.max()) if n else 0.0
    assert worst <= ROW_BAR, worst
    return worst


def test_tile_of_the_case_table_is_the_kernels(eng):
    assert eng.detect_tile() == LC.TILE
    T = LC.T
    assert {(T - 1, T - 1), (T, T), (T + 1, T + 1), (1, 1)} <= set(LC.label_sizes())


@pytest.mark.parametrize("pattern", sorted(LC.PATTERNS))
def test_labelling_alone_is_exact(eng, pattern):
    """every size of the table, B = 3 with different maps, the output between sentinels"""
    for H, W in LC.label_sizes():
        maps = np.stack([LC.PATTERNS[pattern](H, W), LC.random_map(H, W, 3 + H * W), LC.PATTERNS[pattern](H, W)[::-1, ::-1]])
        out = Guarded((3, H, W), torch.int32, -9)
        res = eng.detect_debug_labels(torch.from_numpy(np.ascontiguousarray(maps)).cuda(), out=out.t)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.t.data_ptr() and out.guards_intact()
        got = out.t.cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], R.label_regions(maps[b])), (pattern, H, W, b)


def test_labelling_of_long_paths_across_many_tiles(eng):
    T = LC.T
    H, W = 5 * T + 7, 6 * T + 3
    maps = np.stack([LC.serpentine(H, W), LC.spiral(H, W), LC.tile_corner(H, W)])
    got = eng.detect_debug_labels(torch.from_numpy(maps).cuda()).cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b], R.label_regions(maps[b])), b
    assert set(np.unique(got[0])) == {-1, 0} and set(np.unique(got[1])) == {-1, 0}


def test_gradient_and_buckets_alone_are_exact(eng):
    for H, W in LC.gradient_sizes():
        imgs = np.stack([LC.random_image(H, W, 11 + H + 3 * W), LC.random_image(H, W, 12 + H + 3 * W)])
        pyr = [R.pyramid(im, 2) for im in imgs]
        for octave in (0, 1):
            m2, a, b = (t.cpu().numpy() for t in eng.detect_debug_gradient(torch.from_numpy(imgs).cuda(), octave=octave, grad_threshold=200000))
            for i in range(2):
                q = pyr[i][octave]
                if min(q.shape) < 2:
                    assert m2.shape == (2, 0, 0)
                    continue
                wm2, wa, wb = R.gradient(q, 200000)
                assert np.array_equal(m2[i], wm2) and np.array_equal(a[i], wa) and np.array_equal(b[i], wb), (H, W, octave, i)
                assert (H, W) != (33, 47) or (0 < (wa >= 0).mean() < 1)
    # the pairs next to every bucket boundary, planted as gradients (twice each pair: a sum gx + gy is always even)
    pairs = [p for p in LC.boundary_pairs() if abs(p[0]) + abs(p[1]) <= 255]
    img = LC.planted_gradient_image(pairs)
    m2, a, b = (t.cpu().numpy()[0] for t in eng.detect_debug_gradient(torch.from_numpy(img).cuda(), n_octave=1, grad_threshold=1))
    wm2, wa, wb = R.gradient(img, 1)
    assert np.array_equal(m2, wm2) and np.array_equal(a, wa) and np.array_equal(b, wb)
    for j, p in enumerate(pairs):
        assert (int(a[1, 8 * j + 1]), int(b[1, 8 * j + 1])) == LC.bucket_by_bigint(*p), p


@pytest.mark.parametrize("name", LC.SCENE_NAMES)
def test_whole_call_on_a_drawn_scene(eng, scenes, name):
    img, rows, dbg, counts = scenes[name]
    r, d, c = raw_detect(eng, img[None], 64)
    worst = check_against_restatement(r, d, c, 0, rows, dbg, counts)
    print(f"{name}: {len(rows)} lines, worst row deviation {worst:.3e} px (bar {ROW_BAR:.0e})")
    err = LC.edge_errors(r[0, :len(rows)], LC.scene_edges(name))
    assert err.max() <= 1.5 * LC.EDGE_ERROR_MEASURED <= LC.EDGE_BAR_CEILING


def test_whole_call_on_a_batch_of_different_scenes(eng, scenes):
    imgs = np.stack([scenes[n][0] for n in LC.SCENE_NAMES])
    r, d, c = raw_detect(eng, imgs, 40)
    for b, n in enumerate(LC.SCENE_NAMES):
        check_against_restatement(r, d, c, b, *scenes[n][1:])
    # the Python surface gives the same rows, concatenated
    rows, offsets = eng.detect_lines(torch.from_numpy(imgs).cuda())
    assert rows.dtype == np.float64 and offsets.dtype == np.int32 and offsets.tolist() == np.cumsum([0] + [len(scenes[n][1]) for n in LC.SCENE_NAMES]).tolist()
    for b in range(3):
        assert np.array_equal(rows[offsets[b]:offsets[b + 1]], r[b, :offsets[b + 1] - offsets[b]])


def test_three_octaves_of_an_odd_sized_image(eng, scenes):
    img = scenes["more"][0][:171, :233]
    cfg = {"n_octave": 3, "min_region_size": 8, "density": 0.5}
    rows, regions, _ = R.detect(img, cfg, want_debug=True)
    assert set(rows[:, 5]) == {0.0, 1.0, 2.0}
    assert min(abs(x["fill"] / 0.5 - 1) for reg in regions for x in reg) > 1e-9
    r, d, c = raw_detect(eng, img[None], 128, **cfg)
    check_against_restatement(r, d, c, 0, rows, R.kept_debug_rows(regions), np.bincount(rows[:, 5].astype(int), minlength=3))


def test_flat_and_noise_images(eng):
    H, W = 70, 90
    flat = np.full((2, H, W), 123, np.uint8)
    r, d, c = raw_detect(eng, flat, 16)
    assert c.sum() == 0
    noise = np.random.RandomState(4).randint(0, 256, size=(2, H, W)).astype(np.uint8)
    r, d, c = raw_detect(eng, noise, 16)                               # the default settings: whatever is found equals the restatement
    for b in range(2):
        rows, regions, _ = R.detect(noise[b], want_debug=True)
        assert c[b].sum() == len(rows)
    cfg = {"min_region_size": 4, "density": 0.0, "grad_threshold": 1, "n_octave": 1}
    r, d, c = raw_detect(eng, noise, 2048, **cfg)
    for b in range(2):
        rows, regions, _ = R.detect(noise[b], cfg, want_debug=True)
        print(f"noise image {b}: {len(rows)} lines at min_region_size 4, density 0")
        assert len(rows) > 50
        check_against_restatement(r, d, c, b, rows, R.kept_debug_rows(regions), np.array([len(rows)]))
    for shape in ((1, 1), (1, 40), (40, 1), (2, 2), (3, 2)):
        r, d, c = raw_detect(eng, np.zeros((1, *shape), np.uint8), 4, n_octave=4)
        assert c.shape == (1, 4) and c.sum() == 0


def test_capacity_smaller_than_the_count(eng, scenes):
    img, rows, dbg, counts = scenes["bars"]
    full, _, _ = raw_detect(eng, img[None], 64)
    for cap in (7, 1, 0):
        r, d, c = raw_detect(eng, img[None], cap)                      # raw_detect checks the guards and that nothing lies beyond
        assert np.array_equal(c[0], counts)                            # the true count
        assert np.array_equal(r[0, :cap], full[0, :cap]) and np.array_equal(d[0, :cap], dbg[:cap])
    got, offsets = eng.detect_lines(torch.from_numpy(img).cuda(), capacity=7)      # the Python surface runs once more with room for all
    assert offsets.tolist() == [0, len(rows)] and np.array_equal(got, full[0, :len(rows)])


def test_two_calls_give_identical_bytes_and_float_input_equals_uint8(eng, scenes):
    imgs = np.stack([scenes[n][0] for n in LC.SCENE_NAMES])
    a = raw_detect(eng, imgs, 40)
    b = raw_detect(eng, imgs, 40)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    as_float = ((imgs.astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    assert np.array_equal(R.quantise(as_float), imgs)
    f = raw_detect(eng, as_float, 40)
    for x, y in zip(a, f):
        assert x.tobytes() == y.tobytes()
    # truncation, as the reference's astype('uint8'): a float image between two grey levels is the lower one
    low = ((imgs.astype(np.float64) + 0.9) / 255.0).astype(np.float32)
    assert np.array_equal(R.quantise(low), imgs) and raw_detect(eng, low, 40)[0].tobytes() == a[0].tobytes()


def test_refusals_launch_nothing(eng, scenes):
    L = eng._L
    img = torch.from_numpy(scenes["bars"][0][None]).cuda()
    B, H, W = img.shape
    rows = Guarded((B, 64, 6), torch.float64, -777.25)
    counts = torch.full((64,), -5, dtype=torch.int32).pin_memory()
    need = L.linetr_detect_lines_workspace_bytes(B, H, W, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def detect(img_p=img.data_ptr(), is_float=0, B=B, H=H, W=W, cfg={}, no_cfg=False, cap=64, rows_p=rows.t.data_ptr(), counts_p=counts.data_ptr(),
               ws_p=ws.data_ptr(), ws_bytes=need):
        c = eng.detect_config(**cfg)
        return L.linetr_detect_lines(None, img_p, is_float, B, H, W, None if no_cfg else nat.C.byref(c), cap, rows_p, counts_p, None, ws_p, ws_bytes, None)
    bad = [dict(B=0), dict(B=-2), dict(H=0), dict(W=0), dict(H=2049), dict(W=2049), dict(cfg={"n_octave": 0}), dict(cfg={"scale": 1}),
           dict(cfg={"scale": 3}), dict(no_cfg=True), dict(img_p=None), dict(rows_p=None), dict(counts_p=None), dict(ws_p=None),
           dict(ws_bytes=need - 1), dict(rows_p=rows.t.data_ptr() + 4), dict(img_p=img.data_ptr() + 1, is_float=1), dict(cap=-1)]
    for kw in bad:
        assert detect(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    torch.cuda.synchronize()
    assert rows.untouched() and bool((counts == -5).all()) and not bool(ws.any())
    with pytest.raises(nat.NativeError, match="outside 1..2048"):
        eng.detect_lines(torch.zeros((1, 4, 2049), dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.NativeError, match="scale"):
        eng.detect_lines(img, scale=4)
    with pytest.raises(RuntimeError, match="HIP device"):
        eng.detect_lines(img.cpu())
    assert detect() == 0                                               # and the same call, unbroken, is served
    torch.cuda.synchronize()
    assert int(counts[:2].sum()) == len(scenes["bars"][1]) and rows.guards_intact()


def test_lsd_surface_agrees_with_itself(eng, scenes):
    from linetr_amd.frontends.line_detector import LSD
    from linetr_amd.line_process import keylines_to_array
    lsd = LSD({})
    imgs = np.stack([scenes[n][0] for n in LC.SCENE_NAMES])
    as_float = torch.from_numpy(((imgs.astype(np.float64) + 0.5) / 255.0).astype(np.float32)).cuda()
    rows, offsets = lsd.detect_batch(as_float[:, None])
    assert offsets.tolist() == np.cumsum([0] + [len(scenes[n][1]) for n in LC.SCENE_NAMES]).tolist()
    for b, name in enumerate(LC.SCENE_NAMES):
        want = rows[offsets[b]:offsets[b + 1]]
        assert np.abs(want - scenes[name][1]).max() <= ROW_BAR * 2
        from_host = lsd.detect(imgs[b])                                # a uint8 ndarray
        from_dev = lsd.detect(torch.from_numpy(imgs[b]).cuda())        # a uint8 device tensor
        for shape in ((1, 1, *imgs[b].shape), (1, *imgs[b].shape), imgs[b].shape):
            kl = lsd.detect_torch(as_float[b].reshape(shape))
            assert np.array_equal(keylines_to_array(kl), want)
        assert np.array_equal(keylines_to_array(from_host), want) and np.array_equal(keylines_to_array(from_dev), want)
        k = from_host[len(from_host) - 1]
        assert k.octave == 1 and k.class_id == len(want) - 1 and k.sPointInOctaveX == k.startPointX / 2 and k.numOfPixels == int(k.lineLength) + 1
        assert abs(np.hypot(k.endPointX - k.startPointX, k.endPointY - k.startPointY) - 2 * k.lineLength) < 1e-9 and 0 < k.response <= 1
    one = LSD({"n_octave": 1}).detect(imgs[0])
    assert len(one) == int((scenes["bars"][1][:, 5] == 0).sum()) and all(k.octave == 0 for k in one)


def _standin_superpoint_module(monkeypatch):
    import sys
    import types
    from test_gpu_producer import _Helpers, _StandInSuperPoint
    from workloads import synth

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


def test_matching_constructs_and_runs_without_injection(monkeypatch):
    """Matching(config) with neither lsd= nor superpoint=: the host project's SuperPoint module (a seeded stand-in) and THIS package's
    detector; the asset pair's images go in, the reference's keys come out"""
    from test_gpu_dropin import LT_CFG
    from workloads import synth
    from linetr_amd.frontends.line_detector import LSD
    _standin_superpoint_module(monkeypatch)
    from models.matching import Matching
    gi = np.load(os.path.join(GOLD, "asset_pair_images.npz"))
    imgs = [torch.from_numpy(gi[k].astype(np.float32) / 255.0)[None, None].cuda() for k in ("gray0", "gray1")]
    cfg = {"auto_min_length": True, "linetransformer": {**LT_CFG}}
    mt = Matching(cfg)
    assert type(mt.lsd) is LSD and mt.lsd.config == LSD.default_config
    mt.linetransformer.load_state_dict(synth.to_torch_state_dict(synth.calibrated_state_dict()))
    mt = mt.eval().to("cuda")
    with torch.no_grad():
        own = mt({"image0": imgs[0], "image1": imgs[1]})
    # models/matching.py:19-86: SuperPoint's dict and the line dict of models/line_process.py:182-196 + line_transformer.py:247 per image,
    # and the four matcher entries
    per_image = ("keypoints", "scores", "descriptors", "dense_score", "dense_descriptor", "klines", "length_klines", "angles", "sublines",
                 "pnt_sublines", "mask_sublines", "resp_sublines", "angle_sublines", "desc_sublines", "score_sublines", "mat_klines2sublines",
                 "line_desc")
    want_keys = {k + s for k in per_image for s in "01"} | {"matches_p", "matching_scores_p", "matches_l", "matching_scores_l"}
    assert want_keys <= set(own), want_keys - set(own)
    assert own["line_desc0"].shape[1] == 256 and own["klines0"].shape[-2:] == (2, 2)
    n0, n1 = own["matching_scores_l"].shape[-2:]
    print(f"Matching on the asset pair with the native detector: {n0} x {n1} lines, {int((own['matches_l'][0] >= 0).sum())} match entries")
    assert n0 > 50 and n1 > 50 and bool(torch.isfinite(own["matching_scores_l"]).all())


def test_pair_detected_on_the_device_trains():
    """homography_views -> detect_batch -> Engine.prefilter -> one training iteration; no pixel is copied to the host"""
    import keyline_reference as KR
    import linetr_amd.evaluations as E
    from test_gpu_producer import _Helpers, _StandInSuperPoint
    from workloads import synth
    from linetr_amd import homography as HG
    from linetr_amd.engine import Engine
    from linetr_amd.frontends.line_detector import LSD
    from linetr_amd.optim import Adam
    from linetr_amd.superpoint import FusedHeadSuperPoint
    from linetr_amd.train_ops import TrainableLineTransformer
    H, W = 480, 640
    pre = dict(remove_borders=8, min_length=16, max_keylines=-1, token_distance=8, max_tokens=21)
    gi = np.load(os.path.join(GOLD, "asset_pair_images.npz"))
    image0 = torch.from_numpy(gi["gray0"].astype(np.float32) / 255.0)[None, None].cuda()
    m = synth.pixel_homography(np.random.RandomState(31), H, W, strength=0.5)
    image1, valid1 = HG.homography_views(image0, m[None], erosion_radius=2)
    pair = torch.cat([image0, image1])
    to_host = []
    real_cpu = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (to_host.append(tuple(self.shape)), real_cpu(self, *a, **k))[1]
    try:
        rows, offsets = LSD({}).detect_batch(pair)
    finally:
        torch.Tensor.cpu = real_cpu
    assert to_host == [(int(offsets[-1]), 6)]                          # exactly the rows came back, nothing else
    print(f"detected on the device: {offsets[1]} lines in the image, {offsets[2] - offsets[1]} in its view")
    assert offsets[1] == 186 and offsets[2] - offsets[1] > 50
    eng = Engine.heads_only("cuda:0")
    recs, cu_k, cu_n = (np.array(v, copy=True) for v in
                        eng.prefilter(rows, H, W, offsets=offsets, valid_masks=[None, HG.prefilter_mask(valid1, 0)], **pre))
    assert cu_k[1] > 50 and cu_k[2] - cu_k[1] > 30
    sp = _StandInSuperPoint()
    sp.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(0).items()})
    sp = FusedHeadSuperPoint(sp.cuda().eval(), helpers=_Helpers, native_encoder=True)
    with torch.no_grad():
        preds = [sp({"image": im}) for im in (image0, image1)]
    views = []
    for i, p in enumerate(preds):
        # the same image alone: the records of a one-image batch, as fixed_size_batch takes them
        single = eng.prefilter([rows[offsets[i]:offsets[i + 1]]], H, W, valid_masks=[None if i == 0 else HG.prefilter_mask(valid1, 0)], **pre)
        r, k, n = (np.array(v, copy=True) for v in single)
        assert k.tolist() == [0, cu_k[i + 1] - cu_k[i]] and n.tolist() == [0, cu_n[i + 1] - cu_n[i]]
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
    found = int(gt["found"].sum())
    print(f"pair detected on the device: loss {float(loss):.6f}, {found} ground-truth pairs, {moved} tensors moved by the step")
    assert np.isfinite(float(loss)) and found > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params) and moved > 0
