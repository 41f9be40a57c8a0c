"""The unit cases of the homography-view kernels (linetr_warp_images / linetr_mask_erode): shapes, exact geometries, degenerate
matrices, erosion masks.  NumPy only; tests/test_gpu_warp.py and tools/warp_report.py run them on the device."""
import numpy as np

# the kernels' tiles (rows, columns), csrc/lt_warp.h: WARP_TH x WARP_TW and ERODE_TH x ERODE_TW; asserted against linetr_warp_tile
WARP_TILE = (16, 64)
ERODE_TILE = (32, 64)
WARP_PX = 4            # consecutive x per thread: 16-byte stores where W % 4 == 0, scalar stores otherwise

# (H, W): a single pixel, smaller than a thread's run, row tails with W % 4 != 0, several tiles, exactly one warp tile, one pixel
# beyond it in each direction
SHAPES = ((1, 1), (5, 7), (33, 67), (64, 64), WARP_TILE, (WARP_TILE[0] + 1, WARP_TILE[1] + 1))
KINDS = ("identity", "translation", "flip", "half")


def int_images(seed, B, C, H, W):
    """integer-valued float32 images in 1 .. 250: every bilinear result of the exact cases is exact in float32"""
    return np.random.RandomState(seed).randint(1, 251, size=(B, C, H, W)).astype(np.float32)


def exact_case(kind, img, variant=0):
    """(matrix [3,3] destination -> source in pixels, expected [C,H,W] float32, exact in both modes unless kind == 'half') for one
    image [C,H,W]; `variant` varies the translation / the axis of the half pixel"""
    C, H, W = img.shape
    want = np.zeros_like(img)
    if kind == "identity":
        return np.eye(3), img.copy()
    if kind == "translation":                       # dst (x, y) reads src (x + tx, y + ty)
        tx, ty = ((2, -1), (-3, 2), (1, 3))[variant % 3]
        ys, xs = np.broadcast_arrays(np.arange(H)[:, None] + ty, np.arange(W)[None, :] + tx)
        ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
        want = np.where(ok[None], img[:, np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)], np.float32(0))
        return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]]), want
    if kind == "flip":                              # 180 degrees about the centre
        return np.array([[-1.0, 0, W - 1], [0, -1.0, H - 1], [0, 0, 1.0]]), img[:, ::-1, ::-1].copy()
    assert kind == "half"                           # half a pixel: the exact means of neighbours, the last one with the zero outside
    if variant % 2 == 0:
        nxt = np.concatenate([img[:, :, 1:], np.zeros((C, H, 1), np.float32)], axis=2)
        return np.array([[1.0, 0, 0.5], [0, 1.0, 0], [0, 0, 1.0]]), (img + nxt) * np.float32(0.5)
    nxt = np.concatenate([img[:, 1:, :], np.zeros((C, 1, W), np.float32)], axis=1)
    return np.array([[1.0, 0, 0], [0, 1.0, 0.5], [0, 0, 1.0]]), (img + nxt) * np.float32(0.5)


def exact_batch(rotation, img):
    """a batch [B,C,H,W] in which image i gets kind (rotation + i) % 4: a different matrix per image.  Returns (mats [B,3,3],
    expected [B,C,H,W], kinds)."""
    kinds = [KINDS[(rotation + i) % 4] for i in range(len(img))]
    pairs = [exact_case(k, im, variant=i) for i, (k, im) in enumerate(zip(kinds, img))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), kinds


def degenerate_matrices():
    """four destination -> source matrices no index may be derived from carelessly (names, [4,3,3]): the horizon w' = 0 crosses the
    image between pixels (huge finite positions on both sides, negative w' behind it); entries of 1e300 (finite positions far
    beyond any integer); every pixel maps outside; w' == 0 exactly on the pixels of column 4 (non-finite positions)"""
    names = ("horizon", "huge", "outside", "pole")
    mats = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0313717, 0.0171931, -1.0]],
                     [[1e300, 1e300, 0.0], [1e300, -1e300, 0.0], [0.0, 0.0, 1.0]],
                     [[1.0, 0.0, 1000.0], [0.0, 1.0, -1000.0], [0.0, 0.0, 1.0]],
                     [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, -4.0]]])
    return names, mats


def erosion_masks(seed, B, H, W):
    """uint8 [B,H,W]: image 0 random with a few holes, image 1 all set but single-pixel holes on every border, in every corner and
    on both sides of every tile edge, further images random at other densities; values 1 and (sparsely) other non-zero bytes"""
    rs = np.random.RandomState(seed)
    m = np.ones((B, H, W), np.uint8)
    m[0] = rs.uniform(size=(H, W)) >= 0.01
    if B > 1:
        th, tw = ERODE_TILE
        ys = sorted({0, H - 1, H // 2} | {y for e in range(th, H, th) for y in (e - 1, e)})
        xs = sorted({0, W - 1, W // 2} | {x for e in range(tw, W, tw) for x in (e - 1, e)})
        for y in ys:
            m[1][y, xs] = 0
    for b in range(2, B):
        m[b] = rs.uniform(size=(H, W)) >= 0.002 * b
    m[(rs.uniform(size=m.shape) < 0.1) & (m != 0)] = 255                  # non-zero is set
    return m


EROSION_SHAPES = ((70, 131), (64, 128), (3, 5), (20, 30), (1, 1), (33, 64))     # > 1 tile with tails; exact tiles; smaller than the
EROSION_RADII = (0, 1, 2, 8)                                                     # element; smaller than a tile; one pixel; W % 4 == 0
