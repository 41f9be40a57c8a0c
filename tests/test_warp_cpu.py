"""CPU: the float64 restatement of the homography views (tests/warp_reference.py) against the real reference's outputs
(tests/golden/warp.npz, written by tests/golden/make_golden_warp.py), its square erosion against scipy, the pixel / normalised
conversions of linetr_amd.homography, and the refusals of the two entry points that come before any device call."""
import os
import re

import numpy as np
import pytest
import torch

import warp_reference as R
from linetr_amd import _native as nat
from linetr_amd import homography as HG

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def g():
    return R.fixture()


def test_fixture_holds_the_cases_of_the_restatement(g):
    assert tuple(map(tuple, g["shapes"])) == R.SHAPES
    for c, shape in enumerate(R.SHAPES):
        B, C, H, W = shape
        assert g[f"img_{c}"].shape == shape and g[f"img_{c}"].dtype == np.float32
        assert g[f"mat_{c}"].shape == (B, 3, 3) and g[f"mat_{c}"].dtype == np.float32
        assert g[f"bilinear_{c}"].shape == shape and g[f"nearest_{c}"].shape == shape
        assert g[f"mask_{c}"].shape == (B, H, W) and g[f"mask_{c}"].dtype == np.uint8
        assert 0.05 < g[f"mask_{c}"].mean() < 0.95            # the views leave the image and stay in it
    assert os.path.getsize(os.path.join(R.GOLDEN, "warp.npz")) < 1000000


@pytest.mark.parametrize("c", range(len(R.SHAPES)))
def test_restatement_equals_the_reference(g, c):
    B, C, H, W = R.SHAPES[c]
    img = g[f"img_{c}"]
    pix = R.normalised_to_pixel(g[f"mat_{c}"], H, W)
    dev = 0.0
    for b in range(B):
        want, max_tap = R.warp(img[b], pix[b], "bilinear")
        dev = max(dev, float(np.abs(g[f"bilinear_{c}"][b] - want).max()))
        ex = R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_REF)
        near = R.warp(img[b], pix[b], "nearest")[0].astype(np.float32)
        R.check_discrete(g[f"nearest_{c}"][b], near, ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} nearest")
        R.check_discrete(g[f"mask_{c}"][b], R.valid_mask(pix[b], H, W), ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} mask")
        # a nearest sample is a copy, and it is zero exactly where the mask is zero or the copied pixel is
        assert np.all((near != 0).any(axis=0) <= (R.valid_mask(pix[b], H, W) != 0))
    print(f"case {c}: reference bilinear - float64 = {dev:.3e} (stored {float(g[f'ref_dev_{c}']):.3e})")
    assert dev == float(g[f"ref_dev_{c}"]) and dev <= 2e-5      # float32 coordinates: 6 roundings * 160 px * 2^-24 * |gradient| <= 1


def test_restatement_on_exact_geometry():
    rs = np.random.RandomState(3)
    img = rs.randint(1, 200, size=(2, 9, 13)).astype(np.float64)
    eye = np.eye(3)
    out, tap = R.warp(img, eye)
    assert np.array_equal(out, img) and np.array_equal(R.valid_mask(eye, 9, 13), np.ones((9, 13), np.uint8))
    shift = np.array([[1.0, 0, 3], [0, 1.0, -2], [0, 0, 1]])          # dst (x, y) reads src (x + 3, y - 2)
    want = np.zeros_like(img)
    want[:, 2:, :10] = img[:, :7, 3:]
    for mode in ("bilinear", "nearest"):
        assert np.array_equal(R.warp(img, shift, mode)[0], want)
    assert np.array_equal(R.valid_mask(shift, 9, 13), (want[0] != 0).astype(np.uint8))
    half = np.array([[1.0, 0, 0.5], [0, 1.0, 0], [0, 0, 1]])
    want = np.concatenate([(img[:, :, :-1] + img[:, :, 1:]) / 2, img[:, :, -1:] / 2], axis=2)
    assert np.array_equal(R.warp(img, half)[0], want)
    # half to even: 0.5 -> 0, 1.5 -> 2, .., 11.5 -> 12, 12.5 -> 12
    assert np.array_equal(R.warp(img, half, "nearest")[0][:, :, :4], img[:, :, [0, 2, 2, 4]])
    # w' == 0 on column 4, negative w' to its left: finite positions are sampled, the pole is not
    pole = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -4.0]])
    v = R.valid_mask(pole, 9, 13)
    sx, _ = R.source_positions(pole, 9, 13)
    assert not np.isfinite(sx[:, 4]).any() and v[:, 4].sum() == 0 and np.isfinite(R.warp(img, pole)[0]).all()
    assert v[0, 3] == 0 and sx[0, 3] == -3.0 and v[0, 5] == 1 and sx[0, 5] == 5.0 and v[0, 0] == 1      # 0 / -4 = -0 rounds to pixel 0
    huge = np.diag([1e300, 1e300, 1.0])
    assert R.valid_mask(huge, 9, 13).sum() == 1 and np.isfinite(R.warp(img, huge)[0]).all()


@pytest.mark.parametrize("radius", [0, 1, 2, 8])
def test_square_erosion_equals_scipy(radius):
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(10 + radius)
    for shape, p in (((37, 53), 0.02), ((5, 7), 0.05), ((1, 1), 0.5), ((64, 96), 0.002), ((3, 40), 0.03)):
        mask = (rs.uniform(size=shape) >= p).astype(np.uint8)
        want = ndi.binary_erosion(mask, structure=np.ones((2 * radius + 1,) * 2), border_value=1).astype(np.uint8)
        assert np.array_equal(R.erode(mask, radius), want), (shape, radius)
    batch = (rs.uniform(size=(3, 20, 30)) >= 0.01).astype(np.uint8)
    assert np.array_equal(R.erode(batch, radius), np.stack([R.erode(m, radius) for m in batch]))


def test_conversions_of_the_python_surface():
    rs = np.random.RandomState(5)
    m = rs.standard_normal((4, 3, 3))
    assert np.array_equal(HG.normalised_to_pixel(m, 48, 64), R.normalised_to_pixel(m, 48, 64))
    assert HG.normalised_to_pixel(torch.from_numpy(m[0].astype(np.float32)), 48, 64).dtype == np.float64
    # the normalised corners are the pixel corners
    pix = HG.normalised_to_pixel(np.eye(3), 33, 67)[0]
    assert np.allclose(pix, np.eye(3), atol=1e-15)
    p = HG.normalised_to_pixel(m[1], 33, 67)[0]
    corner = p @ np.array([66.0, 32.0, 1.0])
    want = m[1] @ np.array([1.0, 1.0, 1.0])
    assert np.allclose(corner[:2] / corner[2], (want[:2] / want[2] + 1) / 2 * np.array([66.0, 32.0]), rtol=1e-12)
    assert np.isfinite(HG.normalised_to_pixel(np.eye(3), 1, 1)).all()
    # scale_homography: the builder's formula (build_homography_dataset.py:123-127) in float64
    H, W = 480, 640
    trans = np.array([[2. / W, 0., -1.], [0., 2. / H, -1.], [0., 0., 1.]])
    for shift, t in (((-1, -1), trans), ((0.5, -2), np.array([[2. / W, 0., 0.5], [0., 2. / H, -2.], [0., 0., 1.]]))):
        got = HG.scale_homography(m[2], (H, W), shift=shift)
        assert got.dtype == np.float64 and np.array_equal(got, np.linalg.inv(t) @ m[2] @ t)
    assert HG.scale_homography(m, (H, W)).shape == (4, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        HG.inv_warp_image_batch(torch.zeros(1, 1, 4, 4), torch.eye(3))
    with pytest.raises(RuntimeError, match="HIP device"):
        HG.homography_views(torch.zeros(1, 1, 4, 4), np.eye(3))
    with pytest.raises(RuntimeError):
        HG.compute_valid_mask((4, 4), torch.eye(3))


def test_header_declares_and_library_exports_the_entry_points():
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in ("linetr_warp_images", "linetr_warp_tile", "linetr_mask_erode"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in nat.EXPORTS and hasattr(L, name), name
    assert "#define LINETR_ABI_VERSION 6" in hdr and L.linetr_abi_version() == 6
    t = [nat.C.c_int32() for _ in range(4)]
    assert L.linetr_warp_tile(*(nat.C.byref(v) for v in t)) == 0 and all(v.value > 0 for v in t)
    assert L.linetr_warp_tile(None, None, None, None) == nat.E_ARG


def test_refusals_come_before_any_device_call():
    """no pointer below is ever dereferenced on the device: every call is refused on its arguments alone"""
    L = nat.lib()
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(3), (2, 3, 3)))
    src, dst, val = 0x10000, 0x20000, 0x30000

    def warp(src=src, B=2, C=1, H=8, W=8, mat=eye, mode=0, dst=dst, val=val):
        return L.linetr_warp_images(None, src, B, C, H, W, nat.np_ptr(mat) if mat is not None else None, mode, dst, val, None)
    for kw, text in ((dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(mat=None), b"null"), (dict(B=0), b"bad shape"),
                     (dict(C=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-1), b"bad shape"), (dict(mode=2), b"mode"),
                     (dict(mode=-1), b"mode"), (dict(C=32768, H=256, W=256), b"2^31"), (dict(H=32768, W=32768, C=2), b"2^31"),
                     (dict(H=40000), b"2^31"), (dict(dst=src), b"in-place"), (dict(src=src + 2), b"aligned")):
        assert warp(**kw) == nat.E_ARG and text in L.linetr_last_error(), kw
    for bad in (np.nan, np.inf, -np.inf):
        m = eye.copy()
        m[1, 2, 0] = bad
        assert warp(mat=m) == nat.E_ARG and b"matrix 1" in L.linetr_last_error()

    def erode(mask=src, B=2, H=8, W=8, radius=2, out=dst):
        return L.linetr_mask_erode(None, mask, B, H, W, radius, out, None)
    for kw, text in ((dict(mask=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"bad shape"), (dict(H=0), b"bad shape"),
                     (dict(W=0), b"bad shape"), (dict(radius=-1), b"radius"), (dict(radius=9), b"radius"), (dict(out=src), b"in-place"),
                     (dict(out=src + 64), b"in-place"), (dict(W=40000), b"2^31"), (dict(B=70000), b"above")):
        assert erode(**kw) == nat.E_ARG and text in L.linetr_last_error(), kw
