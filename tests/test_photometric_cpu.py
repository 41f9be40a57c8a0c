"""CPU (no GPU needed): the photometric augmentation's restatement (tests/photometric_reference.py) against scipy, the statistics of its
generator, the host sampler of the library against the restatement, the C ABI (entry points, struct layouts, workspace layout, refusals
before any device call) and the premises of the GPU cases (tests/photometric_cases.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import photometric_cases as PC
import photometric_reference as R
from linetr_amd import _native as nat

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_POINTS = ("linetr_photometric_sample", "linetr_photometric_workspace_bytes", "linetr_photometric", "linetr_gaussian_blur",
                "linetr_photometric_tile")


@pytest.fixture(scope="module")
def L():
    return nat.lib()


@pytest.fixture(scope="module")
def yaml_config():
    with open(os.path.join(ROOT, "tests", "golden", "homography_photometric.json")) as fh:
        return json.load(fh)


def test_philox_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        assert tuple(int(v) for v in R.philox4x32_10(counter, key)) == want


@pytest.mark.parametrize("n", (1, 2, 3, 8, 41))
def test_blur_equals_scipy_mirror_along_each_axis(n):
    """scipy's mode='mirror' is reflect-101 with repeated reflection; radii below, at and far beyond the extent, and extent 1"""
    rs = np.random.RandomState(n)
    a = rs.standard_normal((n, 5)) * 40
    for ksize in (1, 3, 2 * n - 1, 2 * n + 1, 2 * n + 3, 31, 351):
        if ksize < 1:
            continue
        taps = R.gaussian_taps(ksize, 0.0).astype(np.float64)
        for arr, axis in ((a, 0), (a.T.copy(), 1)):
            got = R.correlate1d(arr, taps, axis)
            want = ndi.correlate1d(arr, taps, axis=axis, mode="mirror")
            assert np.abs(got - want).max() <= 1e-12 * 40 * 10, (n, ksize, axis)
    idx = np.arange(-400, 400)
    for extent in (1, 2, 3, 7):
        want = ndi.correlate1d(np.arange(extent, dtype=np.float64), [1.0], mode="mirror")       # identity; the index map by hand:
        period = max(2 * (extent - 1), 1)
        by_hand = [min(v % period, period - v % period) if extent > 1 else 0 for v in idx]
        assert R.reflect101(idx, extent).tolist() == by_hand and want.tolist() == list(range(extent))


def test_gaussian_taps_are_normalised_and_symmetric():
    for ksize, sigma in ((1, 0.0), (3, 0.0), (9, 2.5), (351, 0.0)):
        t = R.gaussian_taps(ksize, sigma)
        assert t.dtype == np.float32 and len(t) == ksize and np.array_equal(t, t[::-1]) and abs(float(t.astype(np.float64).sum()) - 1.0) < ksize * 2.0 ** -24
    assert R.gaussian_taps(1)[0] == 1.0


def test_stage0_rounding_equals_the_reference_truncation_on_all_grey_values():
    """the builder feeds gray / 255. (float64) and truncates (img * 255).astype(uint8); the device rounds 255 x of the float32 image"""
    k = np.arange(256)
    ours = np.rint(255.0 * (k / 255.0).astype(np.float32).astype(np.float64))
    theirs = ((k / 255.0) * 255).astype(np.uint8)
    assert np.array_equal(ours, k) and np.array_equal(theirs, k)


def test_normals_and_impulse_share_within_sampling_error():
    H, W = 1000, 1000
    z = R.normals(PC.SEED, 3, H, W)
    n = z.size
    assert abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs(np.mean(z ** 4) - 3.0) <= 5.0 * np.sqrt(96.0 / n)          # and the tails: the fourth moment, variance 96 / n
    for a, b in ((z[:, 0::4], z[:, 1::4]), (z[:, 0::4], z[:, 2::4]), (z[:, 2::4], z[:, 3::4])):      # the members of a group are uncorrelated
        assert abs(np.mean(a * b)) <= 5.0 / np.sqrt(a.size)
    words, pol = R.impulse_table(PC.SEED, 3, H, W)
    for p in (0.0035, 0.1):
        thr = int(p * 4294967296.0)
        share = np.mean(words < np.uint32(thr))
        assert abs(share - thr / 4294967296.0) <= 5.0 * np.sqrt(p * (1 - p) / n)
    assert abs(pol.mean() - 0.5) <= 5.0 * 0.5 / np.sqrt(n)


def test_entry_points_are_declared_bound_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in nat.EXPORTS and hasattr(L, name), name
    assert "#define LINETR_ABI_VERSION 6" in hdr and L.linetr_abi_version() == 6
    for name, value in (("BRIGHTNESS", R.BRIGHTNESS), ("CONTRAST", R.CONTRAST), ("NOISE", R.NOISE), ("IMPULSE", R.IMPULSE), ("MOTION", R.MOTION),
                        ("BLUR", R.BLUR), ("SHADE", R.SHADE), ("MAX_KSIZE", R.MAX_KSIZE), ("MAX_ELLIPSES", R.MAX_ELLIPSES)):
        assert re.search(r"#define LINETR_PHOTO_%s %d\b" % (name, value), hdr), name
    assert set(nat.PHOTO_STAGES.values()) == {1, 2, 4, 8, 16, 32, 64}


def test_struct_layouts_match_the_header(L):
    """sizes and offsets as the C compiler lays the header's structs out (natural alignment), the ctypes mirrors and the NumPy record"""
    P = nat.PhotoParams
    want = dict(stages=0, d=4, alpha=8, sigma=16, thr=24, K=28, weights=32, blur_ksize=228, blur_sigma=232, n_ellipses=240, ellipse=248, t=1208,
                shade_ksize=1216)
    assert C.sizeof(P) == 1224 and {k: getattr(P, k).offset for k in want} == want
    assert nat.PHOTO_PARAMS_DTYPE.itemsize == 1224 and {k: nat.PHOTO_PARAMS_DTYPE.fields[k][1] for k in want} == want
    Cf = nat.PhotoConfig
    want_c = dict(stages=0, max_abs_change=4, strength_range=8, stddev_range=24, prob_range=40, max_kernel_size=56, nb_ellipses=60, blur_sigma=64,
                  transparency_range=72, kernel_size_range=88)
    assert C.sizeof(Cf) == 96 and {k: getattr(Cf, k).offset for k in want_c} == want_c
    # the header declares the fields in this order with these types
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    body = re.search(r"typedef struct LinetrPhotoParams \{(.*?)\} LinetrPhotoParams;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+)(\[[^;]*)?;", body, re.M)
    assert [f[1] for f in fields] == list(want), fields
    body_c = re.search(r"typedef struct LinetrPhotoConfig \{(.*?)\} LinetrPhotoConfig;", hdr, re.S).group(1)
    assert [f[1] for f in re.findall(r"^\s*(\w+)\s+(\w+)(\[[^;]*)?;", body_c, re.M)] == list(want_c)


def test_tile_constants_are_the_case_table(L):
    v = [C.c_int32() for _ in range(8)]
    assert L.linetr_photometric_tile(*(C.byref(x) for x in v)) == 0
    v = [x.value for x in v]
    assert (tuple(v[0:3]), tuple(v[3:5]), tuple(v[5:7]), v[7]) == (PC.POINT_TILE, PC.ROW_TILE, PC.COL_TILE, PC.MAX_RADIUS)
    assert 2 * PC.MAX_RADIUS + 1 == R.MAX_KSIZE
    assert L.linetr_photometric_tile(None, *(C.byref(x) for x in [C.c_int32() for _ in range(7)])) == nat.E_ARG


def config_struct(flat):
    c = nat.PhotoConfig()
    for k, v in flat.items():
        if isinstance(v, tuple):
            getattr(c, k)[:] = v
        else:
            setattr(c, k, v)
    return c


def sample_native(L, flat, seed, first, B, H, W):
    out = np.zeros(B, nat.PHOTO_PARAMS_DTYPE)
    code = L.linetr_photometric_sample(C.byref(config_struct(flat)), seed, first, B, H, W, nat.np_ptr(out))
    return code, out


def ulps(a, b, dtype):
    """|a - b| in units of the spacing at b"""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), np.finfo(dtype).tiny)).astype(np.float64)


@pytest.mark.parametrize("variant", ("yaml", "defaults_k7_blur", "shade_only", "nothing"))
def test_sampler_equals_the_restatement_and_respects_the_ranges(L, yaml_config, variant):
    """Field for field.  Integers, thresholds, ranges and axes are equal; a value that went through cos / sin (the ellipses' c and s, the
    motion weights) may sit one unit in the last place from NumPy's libm (the two need not round a transcendental the same way)."""
    cfg = json.loads(json.dumps(yaml_config))
    prm = cfg["photometric"]["params"]
    if variant == "defaults_k7_blur":
        prm["motion_blur"]["max_kernel_size"] = 7
        prm["additive_shade"] = {}                              # customizedTransform's own defaults
        prm["GaussianBlur"] = {"sigma": 1.7}
    elif variant == "shade_only":
        cfg["photometric"]["params"] = {"additive_shade": prm["additive_shade"]}
    elif variant == "nothing":
        cfg["photometric"]["enable"] = False
    flat = R.config_stages(cfg)
    from linetr_amd.photometric import photo_config
    mine = photo_config(cfg)
    assert bytes(mine) == bytes(config_struct(flat))            # the package reads the dict as the restatement does
    B, H, W, first = 64, 120, 160, 5
    code, got = sample_native(L, flat, PC.SEED, first, B, H, W)
    assert code == 0, L.linetr_last_error()
    want = R.sample(flat, PC.SEED, first, B, H, W)
    rec = R.to_records(want, nat.PHOTO_PARAMS_DTYPE)
    for k in ("stages", "d", "alpha", "sigma", "thr", "K", "blur_ksize", "blur_sigma", "n_ellipses", "t", "shade_ksize"):
        assert np.array_equal(got[k], rec[k]), k
    assert np.array_equal(got["ellipse"][..., :4], rec["ellipse"][..., :4])
    assert ulps(got["ellipse"][..., 4:], rec["ellipse"][..., 4:], np.float64).max() <= 1
    assert ulps(got["weights"], rec["weights"], np.float32).max() <= 1
    # the ranges of the configuration
    st = flat["stages"]
    assert np.all((got["stages"] & ~st) == 0) and np.all((got["stages"] | R.MOTION) == (st | R.MOTION))
    if st & R.BRIGHTNESS:
        assert np.abs(got["d"]).max() <= flat["max_abs_change"] and got["d"].min() < -25 and got["d"].max() > 25
    if st & R.CONTRAST:
        assert got["alpha"].min() >= flat["strength_range"][0] and got["alpha"].max() < flat["strength_range"][1]
    if st & R.NOISE:
        assert got["sigma"].min() >= flat["stddev_range"][0] and got["sigma"].max() < flat["stddev_range"][1]
    if st & R.IMPULSE:
        assert got["thr"].max() <= int(flat["prob_range"][1] * 4294967296.0)
    if st & R.MOTION:
        on = (got["stages"] & R.MOTION) != 0
        assert 0.25 * B < on.sum() < 0.75 * B and set(got["K"][on]) == set(range(3, flat["max_kernel_size"] + 1, 2)) and np.all(got["K"][~on] == 1)
        for p in got[on]:
            w = p["weights"].astype(np.float64)
            assert abs(w[:p["K"] ** 2].sum() - 1) < 1e-6 and w.min() >= 0 and not w[p["K"] ** 2:].any() and w[(p["K"] ** 2) // 2] == w.max()
    else:
        assert np.all(got["K"] == 1) and np.all(got["weights"][:, 0] == 1)
    if st & R.BLUR:
        assert np.all(got["blur_ksize"] == 5) and np.all(got["blur_sigma"] == 1.7)
    if st & R.SHADE:
        lo, hi = flat["kernel_size_range"]
        assert np.all(got["shade_ksize"] % 2 == 1) and got["shade_ksize"].min() >= lo and got["shade_ksize"].max() <= hi
        assert got["t"].min() >= flat["transparency_range"][0] and got["t"].max() < flat["transparency_range"][1]
        e = got["ellipse"]
        rad = np.maximum(e[..., 2], e[..., 3])
        assert np.all(got["n_ellipses"] == 20) and e[..., 2:4].min() >= int(min(H, W) / 4 / 5) and e[..., 2:4].max() <= min(H, W) / 4
        assert np.all(e[..., 0] >= rad) and np.all(e[..., 0] < W - rad) and np.all(e[..., 1] >= rad) and np.all(e[..., 1] < H - rad)
        assert np.allclose(e[..., 4] ** 2 + e[..., 5] ** 2, 1.0, atol=1e-15) and e[..., 4:].min() >= 0
    else:
        assert not got["n_ellipses"].any() and np.all(got["shade_ksize"] == 1)
    # an image's values do not depend on the batch it is drawn in
    code, alone = sample_native(L, flat, PC.SEED, first + 9, 1, H, W)
    assert code == 0 and alone[0].tobytes() == got[9].tobytes()
    code, other = sample_native(L, flat, PC.SEED + 1, first, B, H, W)
    assert code == 0 and (variant == "nothing" or other.tobytes() != got.tobytes())


def test_sampler_refusals(L, yaml_config):
    flat = R.config_stages(yaml_config)
    out = np.zeros(2, nat.PHOTO_PARAMS_DTYPE)
    ok = dict(cfg=flat, seed=1, first=0, B=2, H=64, W=64)

    def call(**kw):
        a = {**ok, **kw}
        return L.linetr_photometric_sample(C.byref(config_struct(a["cfg"])) if a["cfg"] is not None else None, a["seed"], a["first"], a["B"], a["H"],
                                           a["W"], nat.np_ptr(out) if a.get("out", True) else None)
    bad = [dict(cfg=None), dict(out=False), dict(B=0), dict(H=0), dict(W=-1), dict(first=-1), dict(seed=1 << 32), dict(H=19), dict(W=19),
           dict(cfg={**flat, "stages": 128}), dict(cfg={**flat, "max_abs_change": 256}), dict(cfg={**flat, "strength_range": (1.5, 0.3)}),
           dict(cfg={**flat, "stddev_range": (-1.0, 2.0)}), dict(cfg={**flat, "prob_range": (0.0, 1.5)}), dict(cfg={**flat, "max_kernel_size": 9}),
           dict(cfg={**flat, "max_kernel_size": 2}), dict(cfg={**flat, "nb_ellipses": 21}), dict(cfg={**flat, "kernel_size_range": (100, 400)}),
           dict(cfg={**flat, "kernel_size_range": (100, 100)}), dict(cfg={**flat, "transparency_range": (float("nan"), 1.0)}),
           dict(cfg={**flat, "stages": flat["stages"] | R.BLUR, "blur_sigma": 0.0}), dict(cfg={**flat, "stages": flat["stages"] | R.BLUR, "blur_sigma": 80.0})]
    for kw in bad:
        assert call(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    assert not out.view(np.uint8).any()
    assert call() == 0 and call(H=20, W=20) == 0
    assert call(H=8, W=8, cfg={**flat, "stages": flat["stages"] & ~R.SHADE}) == 0          # without the shade any size is served


def layout_bytes(B, Cn, H, W):
    """the layout function restated: 256-byte aligned segments: the table, two tap rows of 352 floats per image, three plane sets"""
    up = lambda v: (v + 255) // 256 * 256
    return up(B * 1224) + up(B * 2 * 352 * 4) + 3 * up(B * Cn * H * W * 4)


def test_workspace_query_equals_the_layout(L):
    for shape in ((1, 1, 1, 1), (3, 1, 33, 65), (32, 1, 480, 640), (7, 3, 20, 67), (65535, 1, 1, 1)):
        assert L.linetr_photometric_workspace_bytes(*shape) == layout_bytes(*shape), shape
    for shape in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, -1), (65536, 1, 4, 4), (256, 256, 4, 4), (1, 1, 32769, 4), (1, 1, 4, 32769),
                  (1, 2, 32768, 32768)):
        assert L.linetr_photometric_workspace_bytes(*shape) == 0, shape


def test_refusals_come_before_any_device_call(L):
    """Host buffers stand in for device memory: every one of these calls must return before it reaches a launch (the checks come first,
    so no device is needed) and must leave the buffers as they were."""
    B, H, W = 2, 8, 12
    need = L.linetr_photometric_workspace_bytes(B, 1, H, W)
    pool = np.zeros(need + 512, np.uint8)
    off = (-pool.ctypes.data) % 256
    ws = pool.ctypes.data + off
    src, dst = np.full((B, 1, H, W), 0.5, np.float32), np.full((B, 1, H, W), -7.0, np.float32)
    good = R.to_records([R.make_params(R.SHADE | R.MOTION | R.BLUR, K=3, weights=PC.int_kernel(3), blur_ksize=3, ellipses=[(3, 3, 2.5, 1.5, 1, 0)], t=0.3,
                                       shade_ksize=5)] * B, nat.PHOTO_PARAMS_DTYPE)

    def photo(src_p=src.ctypes.data, B=B, H=H, W=W, params=good, seed=1, first=0, q=0, dst_p=dst.ctypes.data, ws_p=ws, ws_bytes=need):
        return L.linetr_photometric(None, src_p, B, H, W, nat.np_ptr(params) if params is not None else None, seed, first, q, dst_p, ws_p, ws_bytes, None)

    def planted(**fields):
        p = good.copy()
        for k, v in fields.items():
            if k == "ellipse":
                p[1]["ellipse"][0] = v
            elif k == "weight":
                p[1]["weights"][3] = v
            else:
                p[1][k] = v
        return dict(params=p)
    bad = [dict(src_p=None), dict(dst_p=None), dict(ws_p=None), dict(params=None), dict(B=0), dict(H=0), dict(W=0), dict(B=65536), dict(H=32769),
           dict(seed=1 << 32), dict(first=-1), dict(first=(1 << 31) - 1), dict(q=2), dict(q=-1), dict(dst_p=src.ctypes.data), dict(src_p=src.ctypes.data + 2),
           dict(dst_p=dst.ctypes.data + 1), dict(ws_p=ws + 16),
           planted(stages=128), planted(d=256), planted(d=-256), planted(alpha=np.nan), planted(sigma=-1.0), planted(sigma=np.inf), planted(t=np.inf),
           planted(K=2), planted(K=9), planted(K=0), planted(weight=np.nan), planted(blur_ksize=4), planted(blur_ksize=353), planted(blur_ksize=0),
           planted(shade_ksize=352), planted(shade_ksize=353), planted(shade_ksize=-1), planted(blur_sigma=-0.5), planted(blur_sigma=np.nan),
           planted(n_ellipses=21), planted(n_ellipses=-1), planted(ellipse=(3, 3, 0.0, 1, 1, 0)), planted(ellipse=(3, 3, 1, -1.0, 1, 0)),
           planted(ellipse=(np.nan, 3, 1, 1, 1, 0)), planted(ellipse=(3, 3, 1, 1, np.inf, 0))]
    for kw in bad:
        assert photo(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    assert photo(ws_bytes=need - 1) == nat.E_WORKSPACE and "workspace too small" in L.linetr_last_error().decode()
    ks, sg = np.array([3, 5], np.int32), np.array([0.0, 1.5])

    def blur(src_p=src.ctypes.data, B=B, Cn=1, H=H, W=W, ks=ks, sg=sg, q=0, dst_p=dst.ctypes.data, ws_p=ws, ws_bytes=need):
        return L.linetr_gaussian_blur(None, src_p, B, Cn, H, W, nat.np_ptr(ks) if ks is not None else None, nat.np_ptr(sg) if sg is not None else None, q,
                                      dst_p, ws_p, ws_bytes, None)
    bad = [dict(src_p=None), dict(dst_p=None), dict(ws_p=None), dict(ks=None), dict(sg=None), dict(B=0), dict(Cn=0), dict(H=-1), dict(W=0), dict(q=2),
           dict(ks=np.array([3, 4], np.int32)), dict(ks=np.array([353, 3], np.int32)), dict(ks=np.array([3, 0], np.int32)),
           dict(sg=np.array([0.0, -1.0])), dict(sg=np.array([np.nan, 1.0])), dict(dst_p=src.ctypes.data), dict(dst_p=dst.ctypes.data + 2), dict(ws_p=ws + 128)]
    for kw in bad:
        assert blur(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    assert blur(ws_bytes=need - 1) == nat.E_WORKSPACE
    assert blur(Cn=2, ws_bytes=need) == nat.E_WORKSPACE          # the layout grows with C
    assert np.all(dst == -7.0) and np.all(src == 0.5) and not pool.any()


def test_premises_of_the_point_cases():
    """no pixel of a noise case within NOISE_BAND of a rounding boundary (the GPU test demands identity); the real-valued motion kernels'
    excused share under SHARE; the exact kernels are integer-valued"""
    for name, p in PC.EXACT.items():
        assert np.array_equal(p["weights"], np.rint(p["weights"])), name
    total_impulses = 0
    for H, W in PC.POINT_SHAPES:
        for name in (*PC.EXACT, *PC.NOISE, *PC.MOTION_REAL):
            c = PC.point_case(name, H, W)
            assert c["n_noise_band"] == 0, (name, H, W)
            assert c["excused"].sum() <= PC.SHARE * H * W, (name, H, W, int(c["excused"].sum()))
        a, _ = R.impulse_table(PC.SEED, 0, H, W)
        total_impulses += int((a < np.uint32(PC.THR)).sum())
    assert total_impulses > 500
    for B, H, W, first in BATCHES:
        assert PC.batch_case(B, H, W, first)["n_noise_band"] == 0


BATCHES = ((3, 33, 65, 0), (2 * PC.CARRY + 1, 20, 67, 5))


def test_premises_of_the_blur_and_shade_cases():
    for H, W in PC.BLUR_SHAPES:
        for ksize, sigma in PC.BLUR_KSIZES:
            c = PC.blur_case(H, W, ksize, sigma, True)
            assert c["excused"].sum() <= PC.SHARE * H * W, (H, W, ksize, int(c["excused"].sum()))
    assert any(k // 2 >= 8 for k, _ in PC.BLUR_KSIZES) and (8, 8) in PC.BLUR_SHAPES                   # radius >= extent
    assert {k // 2 for k, _ in PC.BLUR_KSIZES} >= {PC.MAX_RADIUS - 1, PC.MAX_RADIUS}
    kinds = {s[0] for s in PC.SHADE}
    assert kinds == {"axis", "rotated", "clipped", "overlap", "cover", "none", "twenty"} and {s[1] for s in PC.SHADE} >= {-0.5, 0.5, 0.8, 0.0}
    for H, W in PC.SHADE_SHAPES:
        for i in range(len(PC.SHADE)):
            c = PC.shade_case(H, W, i)
            assert c["form_gap"] > PC.FORM_BAND, (H, W, i)
            assert c["excused"].sum() <= PC.SHARE * H * W, (H, W, i, int(c["excused"].sum()))
            if PC.SHADE[i][1] == 0.0:
                assert np.array_equal(c["ref"]["out"], c["ref"]["level"] / 255.0)
    # the planted ellipses do what their names say (on a shape with room)
    H, W = 65, 129
    m = {k: R.ellipse_mask(PC.ellipses(k, H, W), H, W) for k in kinds}
    assert not m["none"].any() and m["cover"].all() and 0 < m["axis"].mean() < 255 and m["clipped"][0].any() and m["clipped"][-1].any()
    assert m["clipped"][:, 0].any() and m["clipped"][:, -1].any()
    a, b = (R.ellipse_mask([e], H, W) for e in PC.ellipses("overlap", H, W))
    assert (a * b).any() and (a != b).any()
