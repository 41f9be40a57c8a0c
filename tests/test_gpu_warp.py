"""GPU: the homography-view kernels alone (linetr_warp_images / linetr_mask_erode, csrc/lt_warp.h) between sentinel guards: bit-exact
geometries on integer-valued images, every shape of tests/warp_cases.py, the float64 restatement (tests/warp_reference.py) and the real
reference's outputs (tests/golden/warp.npz) under derived bars, degenerate matrices, the erosion, refusals and determinism."""
import numpy as np
import pytest
import torch

import warp_cases as WC
import warp_reference as R
from linetr_amd import _native as nat

pytestmark = pytest.mark.gpu

GUARD, MARKER, MARKER_U8 = 64, -777.25, 0xA5


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def g():
    return R.fixture()


class Guarded:
    """an output tensor carved out of a sentinel-filled pool, `shift` elements off the pool's natural alignment"""

    def __init__(self, shape, dtype, marker, shift=0):
        n = int(np.prod(shape))
        self.pool = torch.full((n + 2 * GUARD + shift,), marker, dtype=dtype, device="cuda")
        self.t = self.pool[GUARD + shift:GUARD + shift + n].view(shape)
        self.marker, self.lo, self.hi = marker, GUARD + shift, GUARD + shift + n

    def guards_intact(self):
        return bool((self.pool[:self.lo] == self.marker).all()) and bool((self.pool[self.hi:] == self.marker).all())

    def untouched(self):
        return bool((self.pool == self.marker).all())


def run_warp(eng, img, mats, mode, shift=0):
    """one native call into guarded outputs; returns (dst, valid) as NumPy after checking the guards and that every element was written"""
    B, C, H, W = img.shape
    dst = Guarded((B, C, H, W), torch.float32, MARKER, shift)
    val = Guarded((B, H, W), torch.uint8, MARKER_U8, shift)
    src = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    out, v = eng.warp_images(src, mats, mode=mode, return_valid=True, out=dst.t, out_valid=val.t)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.t.data_ptr() and v.data_ptr() == val.t.data_ptr()
    assert dst.guards_intact() and val.guards_intact()
    o, vv = dst.t.cpu().numpy(), val.t.cpu().numpy()
    assert not (o == MARKER).any() and set(np.unique(vv)) <= {0, 1}
    return o, vv


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_tiles_of_the_case_table_are_the_kernels(eng):
    assert eng.warp_tiles() == (WC.WARP_TILE, WC.ERODE_TILE)
    assert WC.WARP_TILE in WC.SHAPES and (WC.WARP_TILE[0] + 1, WC.WARP_TILE[1] + 1) in WC.SHAPES


@pytest.mark.parametrize("shape", WC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_geometries_are_bit_exact(eng, shape):
    """identity, integer translation, 180 degrees and half a pixel on integer-valued images: gray single images, and C = 3, B = 3
    with a different matrix per image"""
    H, W = shape
    img1 = WC.int_images(100 + H, 1, 1, H, W)
    for kind in WC.KINDS:
        m, want = WC.exact_case(kind, img1[0])
        got, valid = run_warp(eng, img1, m[None], "bilinear")
        assert same_bits(got[0], want), kind
        assert np.array_equal(valid[0], R.valid_mask(m, H, W)), kind
        if kind != "half":
            got_n, valid_n = run_warp(eng, img1, m[None], "nearest")
            assert same_bits(got_n[0], want) and np.array_equal(valid_n, valid), kind
            assert np.array_equal(valid[0] != 0, want[0] != 0), kind           # images are >= 1: a copied pixel is a valid one
    img3 = WC.int_images(200 + W, 3, 3, H, W)
    for rotation in range(4):
        mats, want, kinds = WC.exact_batch(rotation, img3)
        got, valid = run_warp(eng, img3, mats, "bilinear", shift=rotation % 2)      # odd rotations: outputs off the 16-byte alignment
        assert same_bits(got, want), kinds
        assert np.array_equal(valid, np.stack([R.valid_mask(m, H, W) for m in mats])), kinds


@pytest.mark.parametrize("c", range(len(R.SHAPES)))
def test_fixture_homographies_against_float64_and_the_reference(eng, g, c):
    B, C, H, W = R.SHAPES[c]
    pix = R.normalised_to_pixel(g[f"mat_{c}"], H, W)
    # ---- random images against the float64 restatement
    rnd = (np.random.RandomState(300 + c).standard_normal((B, C, H, W)) * 50).astype(np.float32)
    got, valid = run_warp(eng, rnd, pix, "bilinear")
    got_n, valid_n = run_warp(eng, rnd, pix, "nearest")
    assert np.array_equal(valid, valid_n)
    worst = 0.0
    for b in range(B):
        want, max_tap = R.warp(rnd[b], pix[b], "bilinear")
        err = np.abs(got[b].astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(R.BILINEAR_BAR * max_tap[None], 1e-300)).max()))
        assert np.all(err <= R.BILINEAR_BAR * max_tap[None]), (b, float(err.max()))
        ex = R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_F64)
        R.check_discrete(got_n[b], R.warp(rnd[b], pix[b], "nearest")[0].astype(np.float32), ex, R.EXCUSE_F64_SHARE, f"case {c} image {b} nearest vs f64")
        R.check_discrete(valid[b], R.valid_mask(pix[b], H, W), ex, R.EXCUSE_F64_SHARE, f"case {c} image {b} valid vs f64")
    print(f"case {c}: bilinear error / bar vs float64 = {worst:.3f}")
    # ---- the fixture's images against the reference's own outputs
    img = g[f"img_{c}"]
    got, valid = run_warp(eng, img, pix, "bilinear")
    got_n, _ = run_warp(eng, img, pix, "nearest")
    ref_dev = float(g[f"ref_dev_{c}"])
    for b in range(B):
        _, max_tap = R.warp(img[b], pix[b], "bilinear")
        err = np.abs(got[b].astype(np.float64) - g[f"bilinear_{c}"][b])
        assert np.all(err <= ref_dev + R.BILINEAR_BAR * max_tap[None]), (b, float(err.max()), ref_dev)
        ex = R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_REF)
        R.check_discrete(got_n[b], g[f"nearest_{c}"][b], ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} nearest vs reference")
        R.check_discrete(valid[b], g[f"mask_{c}"][b], ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} valid vs reference")


def test_degenerate_geometry_gives_zeros_and_no_error(eng):
    """the contract of the four matrices of warp_cases.degenerate_matrices, one call per mode"""
    names, mats = WC.degenerate_matrices()
    H, W = 33, 67
    img = WC.int_images(7, len(mats), 1, H, W)
    for mode in ("bilinear", "nearest"):
        got, valid = run_warp(eng, img, mats, mode)
        assert np.isfinite(got).all()
        for b, name in enumerate(names):
            want, max_tap = R.warp(img[b], mats[b], mode)
            want_valid = R.valid_mask(mats[b], H, W)
            # integers in, exact arithmetic: the pole, the huge and the outside matrix give the restatement's positions bit for bit
            ex = R.near_rounding_boundary(mats[b], H, W, R.EXCUSE_F64) if name == "horizon" else np.zeros((H, W), bool)
            assert ex.sum() <= R.EXCUSE_F64_SHARE * H * W, name
            ok = ~ex[None]
            assert np.all(np.abs(got[b] - want)[ok] <= R.BILINEAR_BAR * max_tap[None][ok]), (name, mode)
            assert np.all((got[b] == 0)[(want == 0) & ok]), (name, mode)
            assert np.array_equal(valid[b][~ex], want_valid[~ex]), name
            if mode == "nearest":
                assert np.all(got[b][0][(want_valid == 0) & ~ex] == 0), name
        sx, _ = R.source_positions(mats[3], H, W)
        assert not np.isfinite(sx[:, 4]).any() and valid[3][:, 4].sum() == 0 and np.all(got[3][0][:, 4] == 0)      # the pole
        assert valid[2].sum() == 0 and not got[2].any()                                                          # all outside
        assert valid[1].sum() == 1 and valid[1][0, 0] == 1                                                       # 1e300: only the origin maps to itself
        assert 0 < valid[0].sum() < H * W


@pytest.mark.parametrize("shape", WC.EROSION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_erosion_equals_the_restatement(eng, shape):
    H, W = shape
    B = 3
    masks = WC.erosion_masks(40 + H, B, H, W)
    src = torch.from_numpy(masks).cuda()
    for radius in WC.EROSION_RADII:
        for shift in (0, 1):
            out = Guarded((B, H, W), torch.uint8, MARKER_U8, shift)
            res = eng.erode_mask(src, radius, out=out.t)
            torch.cuda.synchronize()
            assert res.data_ptr() == out.t.data_ptr() and out.guards_intact()
            want = R.erode(masks, radius)
            assert np.array_equal(out.t.cpu().numpy(), want), (radius, shift)
    assert np.array_equal(eng.erode_mask(src[0], 1).cpu().numpy(), R.erode(masks[0], 1))      # a [H,W] mask


def test_refusals_launch_nothing(eng):
    L = eng._L
    B, C, H, W = 2, 2, 8, 12
    src = torch.ones((B, C, H, W), device="cuda")
    dst = Guarded((B, C, H, W), torch.float32, MARKER)
    val = Guarded((B, H, W), torch.uint8, MARKER_U8)
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(3), (B, 3, 3)))

    def warp(src_p=src.data_ptr(), B=B, C=C, H=H, W=W, mat=eye, mode=0, dst_p=dst.t.data_ptr(), val_p=val.t.data_ptr()):
        return L.linetr_warp_images(None, src_p, B, C, H, W, nat.np_ptr(mat) if mat is not None else None, mode, dst_p, val_p, None)
    bad = [dict(src_p=None), dict(dst_p=None), dict(mat=None), dict(B=0), dict(B=-1), dict(C=0), dict(H=0), dict(W=0), dict(mode=2),
           dict(mode=-1), dict(C=1 << 15, H=256, W=256), dict(H=1 << 15, W=1 << 15, C=2), dict(dst_p=src.data_ptr())]
    for entry in (np.nan, np.inf, -np.inf):
        m = eye.copy()
        m[1].flat[4] = entry
        bad.append(dict(mat=m))
    for kw in bad:
        assert warp(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    torch.cuda.synchronize()
    assert dst.untouched() and val.untouched() and bool((src == 1).all())
    with pytest.raises(ValueError):
        eng.warp_images(src, eye, mode="bicubic")
    with pytest.raises(RuntimeError, match="HIP device"):
        eng.warp_images(src.cpu(), eye)
    with pytest.raises(ValueError):
        eng.warp_images(src, eye[:1].repeat(3, axis=0))
    mask = torch.ones((B, H, W), dtype=torch.uint8, device="cuda")
    out = Guarded((B, H, W), torch.uint8, MARKER_U8)

    def erode(mask_p=mask.data_ptr(), B=B, H=H, W=W, radius=2, out_p=out.t.data_ptr()):
        return L.linetr_mask_erode(None, mask_p, B, H, W, radius, out_p, None)
    for kw in (dict(mask_p=None), dict(out_p=None), dict(B=0), dict(H=0), dict(W=-3), dict(radius=-1), dict(radius=9),
               dict(out_p=mask.data_ptr()), dict(W=1 << 16)):
        assert erode(**kw) == nat.E_ARG and L.linetr_last_error(), kw
    torch.cuda.synchronize()
    assert out.untouched() and bool((mask == 1).all())
    with pytest.raises(nat.NativeError, match="radius"):
        eng.erode_mask(mask, 9)
    with pytest.raises(RuntimeError, match="HIP device"):
        eng.erode_mask(mask.cpu(), 1)
    # and the same calls, unbroken, are served
    assert warp() == 0 and erode() == 0
    torch.cuda.synchronize()
    assert bool((dst.t == 1).all()) and bool((val.t == 1).all()) and bool((out.t == 1).all()) and dst.guards_intact() and out.guards_intact()


def test_two_calls_give_identical_bits(eng, g):
    c = 1
    B, C, H, W = R.SHAPES[c]
    pix = R.normalised_to_pixel(g[f"mat_{c}"], H, W)
    img = g[f"img_{c}"]
    first = {}
    for mode in ("bilinear", "nearest"):
        a, va = run_warp(eng, img, pix, mode)
        b, vb = run_warp(eng, img, pix, mode, shift=1)          # and the scalar stores write what the 16-byte stores write
        assert same_bits(a, b) and same_bits(va, vb)
        first[mode] = a
    src = torch.from_numpy(img).cuda()
    assert same_bits(eng.warp_images(src, pix).cpu().numpy(), first["bilinear"])          # without a mask the image is the same
    assert same_bits(eng.warp_images(src, pix[0])[0].cpu().numpy(), first["bilinear"][0])   # one matrix for the whole batch
    m = torch.from_numpy(WC.erosion_masks(9, 2, 70, 131)).cuda()
    assert torch.equal(eng.erode_mask(m, 2), eng.erode_mask(m, 2))
