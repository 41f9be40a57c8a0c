"""Cases of the line-detector tests: drawn scenes with known edges, planted bucket maps for the labelling kernels, gradient pairs next to
the bucket boundaries, and the sizes that walk the kernels' tile.  Everything is generated deterministically; nothing is read from disk."""
import numpy as np

TILE = (32, 32)                  # linetr_detect_tile: cells per tile of the gradient and labelling kernels
T = TILE[0]
SCENE_SHAPE = (240, 320)
BACKGROUND, FOREGROUND = 40, 200
EDGE_BAR_CEILING = 3.0           # px: the end-point bar may in no case exceed this
# worst end-point error of the restatement on SCENES (profiles/line_detector_errors.txt); the tests' bar is 1.5 x this value
EDGE_ERROR_MEASURED = 1.917
SHIFT = (6, 10)                  # (dx, dy), even: the pyramid samples the same pixels

# bars: (angle in degrees, centre x, centre y, length, width); they do not cross and stay away from the border
SCENES = {
    "bars": [(0.0, 70, 25, 90, 10), (90.0, 25, 130, 90, 10), (45.0, 100, 110, 90, 10), (21.0, 220, 60, 90, 10), (75.0, 200, 160, 90, 10)],
    "more": [(135.0, 80, 80, 100, 10), (10.0, 220, 40, 120, 10), (110.0, 250, 150, 100, 10), (30.0, 100, 185, 100, 14)],
}
NEGATIVE_OF = {"dark": "bars"}      # a third scene: dark bars on a bright ground
SCENE_NAMES = ("bars", "more", "dark")


def _coverage(shape, bar, sub=4):
    """share of each pixel (a unit square around its centre) inside the bar, from sub x sub samples"""
    ang, cx, cy, length, width = bar
    H, W = shape
    c, s = np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
    offs = (np.arange(sub) + 0.5) / sub - 0.5
    ys = (np.arange(H)[:, None] + offs[None, :]).reshape(-1)
    xs = (np.arange(W)[:, None] + offs[None, :]).reshape(-1)
    px, py = xs[None, :] - cx, ys[:, None] - cy
    inside = (np.abs(px * c + py * s) <= length / 2) & (np.abs(py * c - px * s) <= width / 2)
    return inside.reshape(H, sub, W, sub).mean(axis=(1, 3))


def scene(name):
    """uint8 [H, W]"""
    bars = SCENES[NEGATIVE_OF.get(name, name)]
    cov = np.zeros(SCENE_SHAPE)
    for bar in bars:
        cov = np.maximum(cov, _coverage(SCENE_SHAPE, bar))
    img = np.floor(BACKGROUND + (FOREGROUND - BACKGROUND) * cov + 0.5).astype(np.uint8)
    return (255 - img).astype(np.uint8) if name in NEGATIVE_OF else img


def scene_edges(name):
    """[E,2,2] the two long edges of every bar as ((x0, y0), (x1, y1))"""
    out = []
    for ang, cx, cy, length, width in SCENES[NEGATIVE_OF.get(name, name)]:
        c, s = np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
        for side in (-1, 1):
            ox, oy = cx - side * s * width / 2, cy + side * c * width / 2
            out.append(((ox - c * length / 2, oy - s * length / 2), (ox + c * length / 2, oy + s * length / 2)))
    return np.asarray(out)


def shifted(img, shift=SHIFT, fill=BACKGROUND):
    dx, dy = shift
    out = np.full_like(img, fill)
    out[dy:, dx:] = img[:img.shape[0] - dy, :img.shape[1] - dx]
    return out


def edge_errors(rows, edges):
    """for every edge the smaller, over the octave-0 lines, of the larger of its two end-point distances (either direction)"""
    r = rows[rows[:, 5] == 0]
    a, b = r[:, None, 0:2], r[:, None, 2:4]
    e0, e1 = edges[None, :, 0], edges[None, :, 1]
    d = lambda p, q: np.sqrt(((p - q) ** 2).sum(-1))      # noqa: E731
    worst = np.minimum(np.maximum(d(a, e0), d(b, e1)), np.maximum(d(a, e1), d(b, e0)))
    return worst.min(axis=0) if len(r) else np.full(len(edges), np.inf)


# ---- gradient pairs next to the bucket boundaries -------------------------------------------------------------------------------------------

CONVERGENTS = [(12, 5), (29, 12), (70, 29)]          # v / u -> sqrt 2 - 1 from both sides: next to partition B's boundary


def octant_images(u, v):
    """the eight images of (u, v) under the symmetries of the square"""
    return sorted({(a, b) for x, y in ((u, v), (v, u)) for a in (x, -x) for b in (y, -y)})


def boundary_pairs():
    pairs = []
    for u, v in CONVERGENTS:
        pairs += octant_images(u, v)
    for n in (1, 2, 7, 100, 8160):
        pairs += octant_images(n, n)                 # gx == gy: partition A's boundary
        pairs += octant_images(n, 0)                 # a zero component
        pairs += octant_images(n, n - 1) if n > 1 else []
    for u in (5, 12, 29, 169, 408, 985, 5741):      # every integer next to u (sqrt 2 - 1)
        for v in range(max(0, int(u * 0.41421356) - 1), int(u * 0.41421356) + 3):
            pairs += octant_images(u, v)
    return sorted(set(pairs) - {(0, 0)})


def bucket_by_bigint(gx, gy):
    """(A, B) with Python integers and exact comparisons of squares: the angle's 45-degree sector, and its 22.5-degree-offset sector"""
    gx, gy = int(gx), int(gy)
    if gx > 0 and gy >= 0:
        k, u, v = 0, gx, gy
    elif gx <= 0 and gy > 0:
        k, u, v = 1, gy, -gx
    elif gx < 0 and gy <= 0:
        k, u, v = 2, -gx, -gy
    else:
        k, u, v = 3, -gy, gx
    a = 2 * k + (1 if v >= u else 0)
    # tan(theta) < sqrt 2 - 1  <=>  v + u < sqrt 2 u  <=>  (u + v)^2 < 2 u^2; and the mirror image for theta > 67.5 degrees
    b = 2 * k if (u + v) ** 2 < 2 * u * u else (2 * k + 2 if (u + v) ** 2 < 2 * v * v else 2 * k + 1)
    return a, b % 8


def planted_gradient_image(pairs):
    """A uint8 image whose cell (8 j + 1, 1) has gradient 2 * pairs[j] exactly (gx + gy is even for every image, so odd sums cannot be
    planted; buckets only depend on the direction).  Four pixels at the corners of the cell's 4 x 4 support carry the pair."""
    img = np.zeros((4, 8 * len(pairs)), dtype=np.uint8)
    for j, (gx, gy) in enumerate(pairs):
        p, m = gx + gy, gx - gy                # 2 gx = a + b - c - d, 2 gy = -a + b - c + d with b - c = p, a - d = m
        assert abs(p) <= 255 and abs(m) <= 255
        x = 8 * j
        img[3, x + 3], img[0, x] = max(p, 0), max(-p, 0)
        img[0, x + 3], img[3, x] = max(m, 0), max(-m, 0)
    return img


# ---- planted bucket maps for the labelling kernels ----------------------------------------------------------------------------------------------

def label_sizes():
    s = [1, T - 1, T, T + 1]
    return [(h, w) for h in s for w in s] + [(1, 3 * T + 5), (3 * T + 5, 1), (2 * T + 3, 3 * T + 1)]


def serpentine(H, W, bucket=3):
    """a one-cell-wide path: full even rows joined alternately at the right and the left end"""
    m = np.full((H, W), -1, np.int8)
    m[0::2] = bucket
    for k, r in enumerate(range(1, H, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = bucket
    return m


def spiral(H, W, bucket=5):
    """a one-cell-wide square spiral with a one-cell gap"""
    m = np.full((H, W), -1, np.int8)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    first = True
    while top <= bottom and left <= right:
        m[top, (left if first else max(left - 2, 0)):right + 1] = bucket
        m[top:bottom + 1, right] = bucket
        if bottom - top >= 2 and right - left >= 2:
            m[bottom, left:right + 1] = bucket
            m[top + 2:bottom + 1, left] = bucket
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        first = False
    return m


def checkerboard(H, W):
    """every cell its own region: no two 8-neighbours share a bucket"""
    y, x = np.mgrid[0:H, 0:W]
    return ((x % 2) + 2 * (y % 2)).astype(np.int8)


def diagonal_touch(H, W):
    """2 x 2 blocks of one bucket that touch only at their corners (one region through the diagonals), the rest unused"""
    y, x = np.mgrid[0:H, 0:W]
    return np.where(((x // 2) + (y // 2)) % 2 == 0, 1, -1).astype(np.int8)


def one_apart(H, W):
    """vertical stripes of one bucket, one unused column between them: separate regions"""
    m = np.full((H, W), -1, np.int8)
    m[:, 0::2] = 2
    return m


def tile_corner(H, W):
    """a 2 x 2 region on every tile corner inside the map, plus single cells diagonally across the corner"""
    m = np.full((H, W), -1, np.int8)
    for y in range(T, H, T):
        for x in range(T, W, T):
            m[y - 1:y + 1, x - 1:x + 1] = 6
            if y + 1 < H and x + 1 < W:
                m[y + 1, x + 1] = 6
            if y >= 2 and x + 1 < W:
                m[y - 2, x + 1] = 6
    return m


def random_map(H, W, seed, p_unused=0.3, n_buckets=3):
    rs = np.random.RandomState(seed)
    m = rs.randint(0, n_buckets, size=(H, W)).astype(np.int8)
    m[rs.uniform(size=(H, W)) < p_unused] = -1
    return m


PATTERNS = {"serpentine": serpentine, "spiral": spiral, "checkerboard": checkerboard, "diagonal_touch": diagonal_touch, "one_apart": one_apart,
            "tile_corner": tile_corner, "random": lambda H, W: random_map(H, W, 17 + H + W)}


def gradient_sizes():
    """pixel sizes whose cell maps are the label sizes, and one odd size that goes through two octaves"""
    s = [2, T, T + 1, T + 2]
    return [(h, w) for h in s for w in s] + [(33, 47), (1, 9), (9, 1)]


def random_image(H, W, seed):
    """uint8: smooth blobs plus noise, so that used and unused cells both occur"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 100 * np.sin(x / 3.0 + rs.uniform(0, 6)) * np.cos(y / 4.0 + rs.uniform(0, 6))
    return np.clip(base + rs.normal(0, 12, size=(H, W)), 0, 255).astype(np.uint8)
