"""The line segment detector of csrc/lt_linedet.h restated in NumPy: integers up to the region moments, float64 in the fit.  Nothing here
imports the package; the CPU tests pin it to scipy.ndimage.label and to Python's big integers, the GPU tests compare the kernels with it.

Pixel centres sit at the integers.  Cell (x, y) is the 2 x 2 block of pixels x..x+1, y..y+1; its linear index is y * (W - 1) + x."""
import numpy as np

DEFAULTS = {"n_octave": 2, "scale": 2, "grad_threshold": 28160, "min_region_size": 16, "density": 0.6}
MIN_REGION = 4          # the smallest min_region_size the native call takes
MAX_DIM = 2048


def reflect101(i, n):
    """index i of an axis of n samples under reflect-101 (.. 2 1 | 0 1 2 .. n-1 | n-2 ..), for any i"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def quantise(image):
    """octave 0: a uint8 image as it is; a float image in [0,1] as uint8(image * 255), float32 multiply, truncation"""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image
    v = image.astype(np.float32) * np.float32(255.0)
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)


def _separable(q, taps, ys, xs):
    """sum_ij taps[i] taps[j] q[ys[:, i], xs[:, j]] in int64"""
    q = q.astype(np.int64)
    rows = sum(int(t) * q[ys[:, i], :] for i, t in enumerate(taps))
    return sum(int(t) * rows[:, xs[:, j]] for j, t in enumerate(taps))


def pyramid_next(q):
    H, W = q.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    off = np.arange(-2, 3)[None, :]
    ys = reflect101(2 * np.arange(Ho)[:, None] + off, H)
    xs = reflect101(2 * np.arange(Wo)[:, None] + off, W)
    return ((_separable(q, (1, 4, 6, 4, 1), ys, xs) + 128) >> 8).astype(np.uint8)


def pyramid(image, n_octave):
    out = [quantise(image)]
    for _ in range(1, n_octave):
        out.append(pyramid_next(out[-1]))
    return out


def smooth16(q):
    H, W = q.shape
    off = np.arange(-1, 2)[None, :]
    return _separable(q, (1, 2, 1), reflect101(np.arange(H)[:, None] + off, H), reflect101(np.arange(W)[:, None] + off, W))


def buckets(gx, gy):
    """(A, B) of integer gradients (int64 arrays, not both zero): the angle atan2(gy, gx) in [0, 360) against boundaries at multiples of
    45 degrees (A) and at 22.5 degrees + multiples of 45 (B), by integer tests"""
    gx, gy = np.asarray(gx, dtype=np.int64), np.asarray(gy, dtype=np.int64)
    q0 = (gx > 0) & (gy >= 0)
    q1 = (gx <= 0) & (gy > 0)
    q2 = (gx < 0) & (gy <= 0)
    k = np.where(q0, 0, np.where(q1, 1, np.where(q2, 2, 3)))
    u = np.where(q0, gx, np.where(q1, gy, np.where(q2, -gx, -gy)))
    v = np.where(q0, gy, np.where(q1, -gx, np.where(q2, -gy, gx)))
    a = 2 * k + (v >= u)
    s = (u + v) * (u + v)
    b = np.where(s < 2 * u * u, 2 * k, np.where(s < 2 * v * v, 2 * k + 2, 2 * k + 1)) % 8
    return a.astype(np.int64), b.astype(np.int64)


def gradient(q, grad_threshold):
    """m2 int64 [H-1, W-1], bucket maps int8 (-1 = unused), and w = floor(sqrt(m2))"""
    S = smooth16(q)
    gx = S[:-1, 1:] + S[1:, 1:] - S[:-1, :-1] - S[1:, :-1]
    gy = S[1:, :-1] + S[1:, 1:] - S[:-1, :-1] - S[:-1, 1:]
    m2 = gx * gx + gy * gy
    used = m2 >= grad_threshold
    a, b = buckets(gx, gy)
    return m2, np.where(used, a, -1).astype(np.int8), np.where(used, b, -1).astype(np.int8)


def isqrt(m2):
    w = np.floor(np.sqrt(m2.astype(np.float64))).astype(np.int64)
    w -= w * w > m2
    w += (w + 1) * (w + 1) <= m2
    return w


def label_regions(bk):
    """int64 [H, W]: the smallest linear index among the cells of each 8-connected region of equal buckets; -1 where bk < 0.
    Minimum propagation with pointer jumping: a cell's label is always a cell of its own region."""
    bk = np.asarray(bk)
    H, W = bk.shape
    big = H * W
    used = bk >= 0
    L = np.where(used, np.arange(H * W, dtype=np.int64).reshape(H, W), big)
    K = np.pad(bk.astype(np.int16), 1, constant_values=-2)
    shifts = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    same = [used & (K[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == bk) for dy, dx in shifts]
    while True:
        P = np.pad(L, 1, constant_values=big)
        new = L.copy()
        for (dy, dx), ok in zip(shifts, same):
            nb = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            np.minimum(new, np.where(ok, nb, big), out=new)
        flat = np.append(new.ravel(), big)
        while True:
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        new = flat[:-1].reshape(H, W)
        if np.array_equal(new, L):
            break
        L = new
    return np.where(used, L, -1)


def octave_regions(q, cfg):
    """every candidate region of one octave, in order (A before B, ascending label): dicts with partition, label, the integer moments
    and the float64 fit; plus the maps the debug entry points return"""
    H, W = q.shape
    maps = {"m2": None, "bucket": [None, None], "labels": [None, None]}
    if H < 2 or W < 2:
        return [], maps
    m2, bA, bB = gradient(q, cfg["grad_threshold"])
    lab = [label_regions(bA), label_regions(bB)]
    maps = {"m2": m2, "bucket": [bA, bB], "labels": lab}
    Nc = m2.size
    used = (bA >= 0).ravel()
    flat = [l.ravel() for l in lab]
    size = [np.bincount(f[used], minlength=Nc) for f in flat]
    nA, nB = size[0][flat[0][used]], size[1][flat[1][used]]
    for_a = nA >= nB
    votes = [np.bincount(flat[0][used][for_a], minlength=Nc), np.bincount(flat[1][used][~for_a], minlength=Nc)]
    ys, xs = np.divmod(np.arange(Nc, dtype=np.int64), W - 1)
    w = isqrt(m2.ravel())
    out = []
    for p in (0, 1):
        roots = np.nonzero((size[p] >= cfg["min_region_size"]) & (2 * votes[p] > size[p]))[0]
        for label in roots.tolist():
            cells = flat[p] == label
            x, y, ww = xs[cells], ys[cells], w[cells]
            mom = [int(cells.sum()), int(ww.sum()), int((ww * x).sum()), int((ww * y).sum()), int((ww * x * x).sum()), int((ww * x * y).sum()),
                   int((ww * y * y).sum())]
            n, sw, swx, swy, sxx, sxy, syy = (float(v) for v in mom)
            cx, cy = swx / sw, swy / sw
            ixx, ixy, iyy = sxx / sw - cx * cx, sxy / sw - cx * cy, syy / sw - cy * cy
            theta = 0.5 * np.arctan2(2.0 * ixy, ixx - iyy)
            dx, dy = np.cos(theta), np.sin(theta)
            px, py = x - cx, y - cy
            l, t = px * dx + py * dy, py * dx - px * dy
            lmin, lmax, tmin, tmax = l.min(), l.max(), t.min(), t.max()
            fill = n / ((lmax - lmin + 1.0) * (tmax - tmin + 1.0))
            out.append({"partition": p, "label": label, "moments": mom, "c": (cx, cy), "d": (dx, dy), "l": (lmin, lmax), "t": (tmin, tmax),
                        "fill": fill, "keep": bool(lmax > lmin and not fill < cfg["density"])})
    return out, maps


def detect(image, config=None, want_debug=False):
    """rows [K,6] float64 (startX, startY, endX, endY, lineLength, octave) of one [H, W] image, uint8 or float in [0,1].
    want_debug: also (regions per octave, maps per octave)"""
    cfg = {**DEFAULTS, **(config or {})}
    if cfg["scale"] != 2 or cfg["n_octave"] < 1 or cfg["min_region_size"] < MIN_REGION or cfg["grad_threshold"] < 1:
        raise ValueError(f"unsupported detector config {cfg}")
    image = np.asarray(image)
    if image.ndim != 2 or not (1 <= image.shape[0] <= MAX_DIM and 1 <= image.shape[1] <= MAX_DIM):
        raise ValueError(f"image of shape {image.shape}")
    rows, regions, maps = [], [], []
    for o, q in enumerate(pyramid(image, cfg["n_octave"])):
        reg, mp = octave_regions(q, cfg)
        regions.append(reg)
        maps.append(mp)
        for r in reg:
            if not r["keep"]:
                continue
            (cx, cy), (dx, dy), (lmin, lmax) = r["c"], r["d"], r["l"]
            s = float(2 ** o)
            rows.append([(cx + lmin * dx + 0.5) * s, (cy + lmin * dy + 0.5) * s, (cx + lmax * dx + 0.5) * s, (cy + lmax * dy + 0.5) * s,
                         lmax - lmin, float(o)])
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    return (rows, regions, maps) if want_debug else rows


def kept_debug_rows(regions):
    """int64 [K,10] as the native call's debug rows: octave, partition, label, n, sw, swx, swy, swxx, swxy, swyy of every kept region"""
    out = [[o, r["partition"], r["label"], *r["moments"]] for o, reg in enumerate(regions) for r in reg if r["keep"]]
    return np.asarray(out, dtype=np.int64).reshape(-1, 10)
