"""NumPy float64 restatement of the photometric augmentation (linetr_photometric / linetr_gaussian_blur / linetr_photometric_sample; the
contract is written in linetr_amd/csrc/lt_photometric.h), stage by stage, with Philox4x32-10 in NumPy.  Imports nothing of the package.
Test infrastructure only.

    quantise(v) = rint(clip(v, 0, 255))                     generator key = (seed, image), counter = (x // 4, y, draw, 0)
    0 input       quantise(255 x)                           draws 0 / 1: normals of pixels 0, 1 / 2, 3 of a group of four
    1 brightness  quantise(level + d)                       draw 2: impulse words, draw 3: polarity words
    2 contrast    quantise(127 + alpha (level - 127))       host sampler: counter = (n, 0, 0, 1)
    3 noise       quantise(level + sigma z)
    4 impulse     word < thr -> 255 if polarity & 1 else 0
    5 motion      K x K correlation, reflect-101, float32 products and sums, ky then kx ascending; quantise
    6 blur        separable Gaussian, float32 taps, reflect-101; quantise
    7 shade       clip(level (1 - t m / 255), 0, 255) / 255 with m the blurred ellipse mask; floor first with quantise_out"""
import math

import numpy as np

BRIGHTNESS, CONTRAST, NOISE, IMPULSE, MOTION, BLUR, SHADE = 1, 2, 4, 8, 16, 32, 64
MAX_KSIZE, MAX_ELLIPSES = 351, 20
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
U24 = 2.0 ** -24


# ---- the generator -----------------------------------------------------------------------------------------------------------------

def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcast together), key: two -> the four output words, uint32 arrays"""
    c = [np.asarray(v, np.uint64) for v in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(v)) for v in key]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return [v.astype(np.uint32) for v in c]


def u01(hi, lo):
    """the 53-bit uniform in [0, 1) of two words"""
    return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint32(6)).astype(np.float64)) / 9007199254740992.0


def group_words(seed, image, draw, H, W):
    """the four words of every group of four pixels: uint32 [H, ceil(W / 4), 4]"""
    g = (W + 3) // 4
    w = philox4x32_10((np.arange(g, dtype=np.uint64)[None, :], np.arange(H, dtype=np.uint64)[:, None], draw, 0), (seed, image))
    return np.stack(w, axis=2)


def normals(seed, image, H, W):
    """z [H, W] float64 by Box-Muller: pixels 4 g, 4 g + 1 from draw 0 (cos, sin), 4 g + 2, 4 g + 3 from draw 1"""
    g = (W + 3) // 4
    z = np.empty((H, g, 4))
    for pair in range(2):
        w = group_words(seed, image, pair, H, W)
        u1, u2 = u01(w[..., 0], w[..., 1]), u01(w[..., 2], w[..., 3])
        r, th = np.sqrt(-2.0 * np.log(1.0 - u1)), 6.283185307179586 * u2
        z[..., 2 * pair], z[..., 2 * pair + 1] = r * np.cos(th), r * np.sin(th)
    return z.reshape(H, 4 * g)[:, :W]


def impulse_table(seed, image, H, W):
    """(words, polarity bits) [H, W]: a pixel is replaced iff its word < thr, by 255 if its bit is set else by 0"""
    a = group_words(seed, image, 2, H, W).reshape(H, -1)[:, :W]
    pol = group_words(seed, image, 3, H, W).reshape(H, -1)[:, :W]
    return a, (pol & np.uint32(1)).astype(bool)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------

def quantise(v):
    return np.rint(np.clip(v, 0.0, 255.0))


def reflect101(idx, n):
    """repeated reflection of period 2 (n - 1); n = 1 maps everything to 0"""
    idx = np.asarray(idx, np.int64)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    v = np.mod(idx, period)
    return np.where(v < n, v, period - v)


def gaussian_taps(ksize, sigma=0.0):
    """float32 [ksize]: exp(-(k - r)^2 / (2 sigma^2)) normalised in float64 (the sum taken in ascending order), rounded once"""
    assert ksize % 2 == 1 and 1 <= ksize <= MAX_KSIZE
    r = ksize // 2
    if sigma == 0.0:
        sigma = 0.3 * ((ksize - 1) / 2.0 - 1.0) + 0.8
    scale = -1.0 / (2.0 * sigma * sigma)
    e = np.exp(((np.arange(ksize) - r) ** 2).astype(np.float64) * scale)
    total = 0.0
    for v in e:
        total += float(v)
    return (e / total).astype(np.float32)


def correlate1d(a, taps, axis):
    """float64 direct sums of taps[k] * a[reflect101(i + k - r)] along `axis`"""
    a = np.asarray(a, np.float64)
    n, r = a.shape[axis], len(taps) // 2
    out = np.zeros_like(a)
    for k, t in enumerate(np.asarray(taps, np.float64)):
        out += t * np.take(a, reflect101(np.arange(n) + k - r, n), axis=axis)
    return out


def blur(a, ksize, sigma=0.0):
    """[..., H, W] under the separable Gaussian: rows (along W) first, then columns; float64, not quantised"""
    taps = gaussian_taps(ksize, sigma)
    return correlate1d(correlate1d(a, taps, -1), taps, -2)


def motion_indices(H, W, K):
    r = K // 2
    ys = [reflect101(np.arange(H) + k - r, H) for k in range(K)]
    xs = [reflect101(np.arange(W) + k - r, W) for k in range(K)]
    return ys, xs


def motion_f64(level, weights, K):
    """the K x K correlation in float64 (not quantised): what the float32 sums are measured against"""
    level = np.asarray(level, np.float64)
    H, W = level.shape
    ys, xs = motion_indices(H, W, K)
    w = np.asarray(weights, np.float32)[:K * K].astype(np.float64).reshape(K, K)
    out = np.zeros((H, W))
    for ky in range(K):
        for kx in range(K):
            out += w[ky, kx] * level[np.ix_(ys[ky], xs[kx])]
    return out


def motion_f32(level, weights, K):
    """the same in the kernel's own order and precision: float32 products and sums, ky then kx ascending (not quantised)"""
    level = np.asarray(level, np.float32)
    H, W = level.shape
    ys, xs = motion_indices(H, W, K)
    w = np.asarray(weights, np.float32)[:K * K].reshape(K, K)
    acc = np.zeros((H, W), np.float32)
    for ky in range(K):
        for kx in range(K):
            acc = acc + w[ky, kx] * level[np.ix_(ys[ky], xs[kx])]
    return acc


def ellipse_forms(ellipses, H, W):
    """[n, H, W] float64: ((dx c + dy s) / ax)^2 + ((dy c - dx s) / ay)^2 of every pixel and ellipse"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((len(ellipses), H, W))
    for i, (cx, cy, ax, ay, c, s) in enumerate(np.asarray(ellipses, np.float64).reshape(-1, 6)):
        dx, dy = x - cx, y - cy
        a, b = (dx * c + dy * s) / ax, (dy * c - dx * s) / ay
        out[i] = a * a + b * b
    return out


def ellipse_mask(ellipses, H, W):
    if len(ellipses) == 0:
        return np.zeros((H, W))
    return np.where((ellipse_forms(ellipses, H, W) <= 1.0).any(axis=0), 255.0, 0.0)


# ---- parameters --------------------------------------------------------------------------------------------------------------------

def make_params(stages=0, d=0, alpha=1.0, sigma=0.0, thr=0, K=1, weights=(1.0,), blur_ksize=1, blur_sigma=0.0, ellipses=(), t=0.0, shade_ksize=1):
    w = np.zeros(49, np.float32)
    flat = np.asarray(weights, np.float32).ravel()
    w[:len(flat)] = flat
    return dict(stages=int(stages), d=int(d), alpha=float(alpha), sigma=float(sigma), thr=int(thr), K=int(K), weights=w, blur_ksize=int(blur_ksize),
                blur_sigma=float(blur_sigma), ellipses=np.asarray(ellipses, np.float64).reshape(-1, 6), t=float(t), shade_ksize=int(shade_ksize))


def to_records(params, dtype):
    """a list of make_params dicts as the NumPy records of LinetrPhotoParams (`dtype`: the binding's PHOTO_PARAMS_DTYPE)"""
    rec = np.zeros(len(params), dtype)
    for r, p in zip(rec, params):
        for k in ("stages", "d", "alpha", "sigma", "thr", "K", "weights", "blur_ksize", "blur_sigma", "t", "shade_ksize"):
            r[k] = p[k]
        r["n_ellipses"] = len(p["ellipses"])
        r["ellipse"][:len(p["ellipses"])] = p["ellipses"]
    return rec


def imgaug_blur_ksize(sigma):
    k = 2.6 * sigma if sigma < 3.0 else (3.3 * sigma if sigma < 5.0 else 5.21 * sigma)
    k = int(max(k, 5.0))
    return k + 1 if k % 2 == 0 else k


def config_stages(cfg):
    """the stage bits and the flat fields of LinetrPhotoConfig from the reference's `augmentation` dict (homography.yaml)"""
    ph = cfg["photometric"]
    prm = ph["params"] if ph.get("enable", False) else {}
    out = dict(stages=0, max_abs_change=0, strength_range=(1.0, 1.0), stddev_range=(0.0, 0.0), prob_range=(0.0, 0.0), max_kernel_size=3,
               nb_ellipses=0, blur_sigma=0.0, transparency_range=(0.0, 0.0), kernel_size_range=(1, 2))
    if prm.get("random_brightness"):
        out["stages"] |= BRIGHTNESS
        out["max_abs_change"] = int(prm["random_brightness"]["max_abs_change"])
    if prm.get("random_contrast"):
        out["stages"] |= CONTRAST
        out["strength_range"] = tuple(float(v) for v in prm["random_contrast"]["strength_range"])
    if prm.get("additive_gaussian_noise"):
        out["stages"] |= NOISE
        out["stddev_range"] = tuple(float(v) for v in prm["additive_gaussian_noise"]["stddev_range"])
    if prm.get("additive_speckle_noise"):
        out["stages"] |= IMPULSE
        out["prob_range"] = tuple(float(v) for v in prm["additive_speckle_noise"]["prob_range"])
    if prm.get("motion_blur"):
        out["stages"] |= MOTION
        out["max_kernel_size"] = int(prm["motion_blur"]["max_kernel_size"])
    if prm.get("GaussianBlur"):
        out["stages"] |= BLUR
        out["blur_sigma"] = float(prm["GaussianBlur"]["sigma"])
    if prm.get("additive_shade"):
        sh = prm["additive_shade"]
        out["stages"] |= SHADE
        out["nb_ellipses"] = int(sh.get("nb_ellipses", 20))
        out["transparency_range"] = tuple(float(v) for v in sh.get("transparency_range", (-0.5, 0.8)))
        out["kernel_size_range"] = tuple(int(v) for v in sh.get("kernel_size_range", (250, 350)))
    return out


def sample(flat, seed, first, B, H, W):
    """linetr_photometric_sample restated: `flat` = config_stages(...); a list of B make_params dicts"""
    out = []
    lerp = lambda r, u: r[0] + u * (r[1] - r[0])
    for b in range(B):
        image = first + b

        def draw(n):
            w = philox4x32_10((n, 0, 0, 1), (seed, image))
            return float(u01(w[0], w[1])), float(u01(w[2], w[3]))
        st = flat["stages"]
        p = make_params(stages=st & ~MOTION)
        if st & BLUR:
            p["blur_ksize"], p["blur_sigma"] = imgaug_blur_ksize(flat["blur_sigma"]), flat["blur_sigma"]
        u0, u1 = draw(0)
        if st & BRIGHTNESS:
            p["d"] = int(math.floor(u0 * (2.0 * flat["max_abs_change"] + 1.0))) - flat["max_abs_change"]
        if st & CONTRAST:
            p["alpha"] = lerp(flat["strength_range"], u1)
        u0, u1 = draw(1)
        if st & NOISE:
            p["sigma"] = lerp(flat["stddev_range"], u0)
        if st & IMPULSE:
            p["thr"] = int(min(math.floor(lerp(flat["prob_range"], u1) * 4294967296.0), 4294967295.0))
        u0, u1 = draw(2)
        if (st & MOTION) and u0 < 0.5:
            p["stages"] |= MOTION
            K = 3 + 2 * int(math.floor(u1 * float((flat["max_kernel_size"] - 3) // 2 + 1)))
            r = K // 2
            u0, _ = draw(3)
            theta = math.pi * u0
            ct, sn = math.cos(theta), math.sin(theta)
            w, total = [], 0.0
            for i in range(K):
                for j in range(K):
                    w.append(max(0.0, 1.0 - abs(ct * float(i - r) - sn * float(j - r))))
                    total += w[-1]
            p["K"] = K
            p["weights"][:] = 0
            p["weights"][:K * K] = (np.asarray(w) / total).astype(np.float32)
        if st & SHADE:
            u0, u1 = draw(4)
            p["t"] = lerp(flat["transparency_range"], u0)
            lo, hi = flat["kernel_size_range"]
            ks = lo + int(math.floor(u1 * float(hi - lo)))
            p["shade_ksize"] = ks + 1 if ks % 2 == 0 else ks
            min_dim = float(min(H, W)) / 4.0
            el = []
            for e in range(flat["nb_ellipses"]):
                u0, u1 = draw(5 + 3 * e)
                ax, ay = int(max(u0 * min_dim, min_dim / 5.0)), int(max(u1 * min_dim, min_dim / 5.0))
                rad = max(ax, ay)
                u0, u1 = draw(6 + 3 * e)
                cx, cy = rad + int(math.floor(u0 * float(W - 2 * rad))), rad + int(math.floor(u1 * float(H - 2 * rad)))
                u0, _ = draw(7 + 3 * e)
                ang = (u0 * 90.0) * (math.pi / 180.0)
                el.append((cx, cy, ax, ay, math.cos(ang), math.sin(ang)))
            p["ellipses"] = np.asarray(el, np.float64).reshape(-1, 6)
        out.append(p)
    return out


# ---- the chain ---------------------------------------------------------------------------------------------------------------------

def augment(x, p, seed, image, quantise_out=False, motion="f32"):
    """One image x [H, W] float32 under the parameters p (make_params).  Returns a dict:
        out          float64 [H, W], the output before its rounding to float32
        level        the levels that reach the shade (after stages 0-6)
        pre_noise    level + sigma z before its quantisation (None without the stage)
        pre_motion   the float64 correlation before its quantisation (None without the stage)
        pre_blur     the float64 blur before its quantisation (None without the stage)
        shaded       the clipped shaded level before floor / division (None without the stage); shaded_raw: before the clip
    motion 'f32': stage 5 quantises the kernel's own float32 sums (bit-exact restatement); 'f64': the float64 correlation."""
    x = np.asarray(x, np.float32)
    H, W = x.shape
    st = p["stages"]
    res = dict(pre_noise=None, pre_motion=None, pre_blur=None, shaded=None)
    level = quantise(255.0 * x.astype(np.float64))
    if st & BRIGHTNESS:
        level = quantise(level + float(p["d"]))
    if st & CONTRAST:
        level = quantise(127.0 + p["alpha"] * (level - 127.0))
    if st & NOISE:
        res["pre_noise"] = level + p["sigma"] * normals(seed, image, H, W)
        level = quantise(res["pre_noise"])
    if st & IMPULSE:
        a, pol = impulse_table(seed, image, H, W)
        level = np.where(a < np.uint32(p["thr"]), np.where(pol, 255.0, 0.0), level)
    if st & MOTION:
        res["pre_motion"] = motion_f64(level, p["weights"], p["K"])
        level = quantise(motion_f32(level, p["weights"], p["K"]).astype(np.float64) if motion == "f32" else res["pre_motion"])
    if st & BLUR:
        res["pre_blur"] = blur(level, p["blur_ksize"], p["blur_sigma"])
        level = quantise(res["pre_blur"])
    res["level"] = level
    shaded = level
    if st & SHADE:
        m = blur(ellipse_mask(p["ellipses"], H, W), p["shade_ksize"], 0.0)
        res["mask_blur"] = m
        res["shaded_raw"] = level * (1.0 - p["t"] * m / 255.0)
        shaded = np.clip(res["shaded_raw"], 0.0, 255.0)
        res["shaded"] = shaded
        if quantise_out:
            shaded = np.floor(shaded)
    res["out"] = shaded / 255.0
    return res


def near_half(v, tol):
    """bool: v lies within tol of a rounding boundary k + 1/2 (inside the clip range)"""
    v = np.asarray(v, np.float64)
    return (np.abs(np.abs(v - np.floor(v)) - 0.5) <= tol) & (v > -1.0) & (v < 256.0)


def near_integer(v, tol):
    """bool: v lies within tol of an integer (the boundary of floor)"""
    v = np.asarray(v, np.float64)
    return np.abs(v - np.rint(v)) <= tol


def check_discrete(got, want, excused, share, what, unit=1.0):
    """warp_reference.check_discrete's pattern: every non-excused pixel equal, an excused one at most one level (`unit`) apart, the excused
    share under its cap; returns (differing, excused) counts"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    differ = got != want
    n_ex = int(np.count_nonzero(excused))
    print(f"{what}: {int(differ.sum())} of {differ.size} differ, {n_ex} of {excused.size} pixels excused")
    assert n_ex <= share * excused.size, (what, n_ex, excused.size)
    assert not np.any(differ & ~excused), (what, int((differ & ~excused).sum()))
    assert np.all(np.abs(got - want)[excused] <= unit * (1.0 + 1e-6)), what
    return int(differ.sum()), n_ex
