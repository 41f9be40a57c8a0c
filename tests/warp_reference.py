"""Float64 NumPy restatement of the homography views (linetr_warp_images / linetr_mask_erode; the reference's
dataloaders/utils/utils.py:317-351 inv_warp_image_batch and :677-704 compute_valid_mask in PIXEL coordinates), the excused rule of its
discrete outputs and the fixture tests/golden/warp.npz.  Pinned to the real reference's outputs by tests/test_warp_cpu.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ((3, 1, 33, 67), (3, 3, 48, 64), (2, 1, 120, 160))          # the fixture's image batches [B,C,H,W]
# A discrete output (nearest sample, valid bit) of the REFERENCE may differ from the float64 restatement where the float64 source
# coordinate lies within EXCUSE_REF px of a rounding boundary (k + 1/2; the image edge of a nearest sample is the boundary at -1/2
# or extent - 1/2): the reference's coordinates are float32, about six roundings at magnitude <= 640 are 6 * 640 * 2^-24 = 2.3e-4 px,
# 1e-3 leaves a 4x margin.  At most EXCUSE_REF_SHARE of a case's pixels may be excused.
EXCUSE_REF, EXCUSE_REF_SHARE = 1e-3, 0.02
# The native kernel computes the position in float64 like the restatement (a few ulps apart): 1e-9 px, at most 0.1 % of the pixels.
EXCUSE_F64, EXCUSE_F64_SHARE = 1e-9, 0.001
BILINEAR_BAR = 1e-6          # |native - float64| <= BILINEAR_BAR * max|tap| per pixel: at most eight float32 roundings of 2^-24 = 4.8e-7


def fixture():
    return np.load(os.path.join(GOLDEN, "warp.npz"))


def normalised_to_pixel(mat, height, width):
    """the reference's normalised matrices (linspace(-1, 1, W), align_corners=True) as pixel matrices, float64"""
    mat = np.asarray(mat, dtype=np.float64).reshape(-1, 3, 3)
    sx, sy = (width - 1) / 2.0, (height - 1) / 2.0
    to_pix = np.array([[sx, 0.0, sx], [0.0, sy, sy], [0.0, 0.0, 1.0]])
    to_norm = np.array([[1.0 / sx if sx else 0.0, 0.0, -1.0], [0.0, 1.0 / sy if sy else 0.0, -1.0], [0.0, 0.0, 1.0]])
    return to_pix @ mat @ to_norm


def source_positions(m, H, W):
    """(sx, sy) [H,W] float64: where destination pixel (x, y) reads the source, (x' / w', y' / w') as x' * (1 / w'); may be non-finite"""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(all="ignore"):
        xs = m[0, 0] * x + m[0, 1] * y + m[0, 2]
        ys = m[1, 0] * x + m[1, 1] * y + m[1, 2]
        inv = 1.0 / (m[2, 0] * x + m[2, 1] * y + m[2, 2])
        return xs * inv, ys * inv


def _finite(sx, sy):
    return np.isfinite(sx) & np.isfinite(sy)


def _clamped(s, extent, fin):
    """the position moved into [-2, extent + 1] (every position outside (-1, extent) has all its taps outside the image)"""
    return np.clip(np.where(fin, s, -2.0), -2.0, extent + 1.0)


def valid_mask(m, H, W):
    """uint8 [H,W]: 1 where the nearest (half to even) source pixel lies inside the image"""
    sx, sy = source_positions(m, H, W)
    fin = _finite(sx, sy)
    xn, yn = np.rint(_clamped(sx, W, fin)), np.rint(_clamped(sy, H, fin))
    return (fin & (xn >= 0) & (xn <= W - 1) & (yn >= 0) & (yn <= H - 1)).astype(np.uint8)


def warp(img, m, mode="bilinear"):
    """img [C,H,W] through the pixel matrix m (destination -> source), zero padding, everything in float64.
    Returns (out [C,H,W] float64, max_tap [H,W]: the largest |tap| a pixel's result was made of)."""
    img = np.asarray(img, dtype=np.float64)
    C, H, W = img.shape
    sx, sy = source_positions(m, H, W)
    fin = _finite(sx, sy)
    sx, sy = _clamped(sx, W, fin), _clamped(sy, H, fin)
    out = np.zeros((C, H, W))
    max_tap = np.zeros((H, W))

    def tap(xi, yi):
        ok = fin & (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        xc, yc = np.clip(xi, 0, W - 1).astype(np.int64), np.clip(yi, 0, H - 1).astype(np.int64)
        return np.where(ok[None], img[:, yc, xc], 0.0)
    if mode == "nearest":
        v = tap(np.rint(sx), np.rint(sy))
        return v, np.abs(v).max(axis=0)
    assert mode == "bilinear"
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    for dx, dy, w in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        v = tap(x0 + dx, y0 + dy)
        out += v * w[None]
        max_tap = np.maximum(max_tap, np.abs(v).max(axis=0))
    return out, max_tap


def near_rounding_boundary(m, H, W, tol):
    """bool [H,W]: the float64 source coordinate lies within tol px of a rounding boundary k + 1/2 in x or in y (non-finite
    positions: never)"""
    sx, sy = source_positions(m, H, W)
    fin = _finite(sx, sy)
    with np.errstate(all="ignore"):
        dx = np.abs(np.abs(sx - np.floor(sx)) - 0.5)
        dy = np.abs(np.abs(sy - np.floor(sy)) - 0.5)
    big = np.abs(sx) + np.abs(sy) > 1e6          # far outside: no decision hangs on the fraction
    return fin & ~big & ((dx <= tol) | (dy <= tol))


def erode(mask, radius):
    """binary erosion of [..., H, W] by the (2 radius + 1)^2 square of ones, outside counting as set; uint8 0 / 1"""
    m = (np.asarray(mask) != 0)
    r = int(radius)
    H, W = m.shape[-2:]
    pad = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(r, r), (r, r)], constant_values=True)
    out = np.ones_like(m)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= pad[..., dy:dy + H, dx:dx + W]
    return out.astype(np.uint8)


def check_discrete(got, want, excused, share, what):
    """every non-excused pixel equal, the excused share under its cap; returns (differing, excused) counts"""
    got, want = np.asarray(got), np.asarray(want)
    ex = np.broadcast_to(excused, got.shape)
    differ = got != want
    n_ex = int(np.count_nonzero(excused))
    print(f"{what}: {int(differ.sum())} of {differ.size} differ, {n_ex} of {excused.size} pixels excused")
    assert n_ex <= share * excused.size, (what, n_ex, excused.size)
    assert not np.any(differ & ~ex), (what, int((differ & ~ex).sum()))
    return int(differ.sum()), n_ex
