"""The cases and bars of the photometric kernels' tests (tests/test_photometric_cpu.py checks their premises without a GPU,
tests/test_gpu_photometric.py and tools/photometric_report.py run them).  References are computed once per case (lru_cache) and shared:
do not write to them.

Bars, in levels (u = 2^-24, one float32 rounding):
  motion   K K u 255: the K K products of non-negative weights that sum to 1 round once each (together at most u 255) and the K K - 1
           sums that follow 0 + product once each (partial sums <= 255).
  blur     per pass (n + 2) u max|value| for n = ksize taps: n fused multiply-adds of non-negative terms whose partial sums stay below
           max|value|, and 2 u for device taps that round the other way than NumPy's (exp may differ in the last place: a tap moves by
           2^-23 of itself, the taps sum to 1).  Two passes: 2 (n + 2) u max|value|.  ksize 1 has the single tap 1: bar 0.
  mask     the same two passes on the non-negative mask, relative to the pixel's own blurred value m (partial sums of non-negative terms
           stay below the total): 2 (n + 2) u m.  Where the blurred mask is 0 the bar is 0.
  shade    shaded = level (1 - t m / 255): |t| level / 255 times the mask's bar; the float64 operations add 1e-13 of nothing.  The output
           shaded / 255 is rounded to float32 once: u |out| on top, in output units.
A quantised output that follows a float32 sum is EXCUSED where the restatement's float64 value lies within the bar of a rounding boundary
(k + 1/2 for rint, k for floor); an excused pixel may differ by one level, and at most SHARE of a case's pixels may be excused.
The Gaussian noise is float64 on both sides; the device's log / cos / sin may differ from NumPy's in the last place, about 1e-14 levels
at sigma 10: NOISE_BAND = 1e-9 levels around k + 1/2 is far wider, and the seeds are chosen with no pixel inside it.  The planted
ellipses keep every pixel's form further than FORM_BAND from 1."""
import functools
import math
import zlib

import numpy as np

import photometric_reference as R

POINT_TILE, ROW_TILE, COL_TILE, MAX_RADIUS = (32, 64, 3), (8, 256), (64, 64), 175      # what linetr_photometric_tile must report
CARRY = 3                                                                              # images per carrier launch
SHARE, NOISE_BAND, FORM_BAND = 0.01, 1e-9, 1e-9
SEED = 2026
U = R.U24

TH, TW, HALO = POINT_TILE
# 1 x 1, 1 x W, H x 1; one below, at and one above the tile in both extents; one pixel beyond two tiles; W % 4 != 0
POINT_SHAPES = ((1, 1), (1, 70), (37, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (20, 67))
# the strips of the row pass (8 x 256) and the tiles of the column pass (64 x 64); 8 x 8: radius >= extent at every ksize above 15
BLUR_SHAPES = ((1, 1), (8, 8), (1, 300), (70, 1), (7, 255), (8, 256), (9, 257), (65, 63), (2 * 64 + 1, 2 * 8 + 1), (17, 2 * 256 + 1))
# 1, 3, a given sigma, radius = MAX_RADIUS - 1 and MAX_RADIUS (MAX_RADIUS + 1 = ksize 353 is refused)
BLUR_KSIZES = ((1, 0.0), (3, 0.0), (9, 2.5), (31, 0.0), (2 * MAX_RADIUS - 1, 0.0), (2 * MAX_RADIUS + 1, 0.0))
SHADE_SHAPES = ((1, 1), (1, 70), (37, 1), (33, 65), (65, 129), (70, 257))


def _rs(*tag):
    """a seeded generator named by its arguments (the same in every process, unlike hash())"""
    return np.random.RandomState(zlib.crc32(repr(tag).encode()))


def image(tag, H, W):
    """float32 [H, W] in [0, 1]: every second pixel a grey value k / 255, the others arbitrary floats"""
    rs = _rs("image", tag, H, W)
    a = rs.random_sample((H, W)).astype(np.float32)
    k = (rs.randint(0, 256, (H, W)) / 255.0).astype(np.float32)
    pick = rs.random_sample((H, W)) < 0.5
    return np.where(pick, k, a).astype(np.float32)


def line_kernel(K, theta):
    """the sampler's motion kernel: an anti-aliased line through the centre, normalised in float64, rounded once"""
    r = K // 2
    w = np.array([[max(0.0, 1.0 - abs(math.cos(theta) * (i - r) - math.sin(theta) * (j - r))) for j in range(K)] for i in range(K)])
    return (w / w.sum()).astype(np.float32)


def int_kernel(K):
    """integer-valued kernels that sum to 1: every product and sum is exact in float32 whatever the order"""
    w = np.zeros((K, K), np.float32)
    if K == 1:
        w[0, 0] = 1
    elif K == 3:
        w[0, 2] = 1
    elif K == 5:
        w[0, 0], w[4, 4], w[2, 2] = 1, 1, -1
    else:
        w[0, 6], w[6, 0], w[3, 3], w[0, 0], w[6, 6] = 1, 1, 1, -1, -1
    return w


THR = int(0.1 * 4294967296.0)          # a tenth of the pixels: enough of both polarities on the smallest shapes' neighbours
# the stages that must agree bit for bit
EXACT = {
    "identity": R.make_params(),
    "brighter": R.make_params(R.BRIGHTNESS, d=50),
    "darker": R.make_params(R.BRIGHTNESS, d=-50),
    "flat": R.make_params(R.CONTRAST, alpha=0.3),
    "steep": R.make_params(R.CONTRAST, alpha=1.5),
    "impulse": R.make_params(R.IMPULSE, thr=THR),
    "shift3": R.make_params(R.MOTION, K=3, weights=int_kernel(3)),
    "int5": R.make_params(R.MOTION, K=5, weights=int_kernel(5)),
    "int7": R.make_params(R.MOTION, K=7, weights=int_kernel(7)),
    "motion1": R.make_params(R.MOTION, K=1, weights=int_kernel(1)),
    "all_exact": R.make_params(R.BRIGHTNESS | R.CONTRAST | R.IMPULSE | R.MOTION, d=-17, alpha=1.3, thr=THR // 4, K=5, weights=int_kernel(5)),
}
NOISE = {
    "noise_lo": R.make_params(R.NOISE, sigma=0.75),
    "noise_hi": R.make_params(R.NOISE, sigma=10.0),
    "noise_chain": R.make_params(R.BRIGHTNESS | R.CONTRAST | R.NOISE | R.IMPULSE | R.MOTION, d=21, alpha=0.8, sigma=6.5, thr=THR // 8, K=3,
                                 weights=int_kernel(3)),
}
MOTION_REAL = {f"line{K}": R.make_params(R.MOTION, K=K, weights=line_kernel(K, 0.3 + 0.55 * K)) for K in (1, 3, 5, 7)}


def motion_bar(K):
    return 0.0 if K == 1 else K * K * U * 255.0


def blur_bar(ksize, max_abs):
    return 0.0 if ksize == 1 else 2.0 * (ksize + 2) * U * max_abs


def mask_bar(ksize, m):
    return 0.0 * m if ksize == 1 else 2.0 * (ksize + 2) * U * m


@functools.lru_cache(maxsize=None)
def point_case(name, H, W, image_index=0):
    """restatement of one EXACT / NOISE / MOTION_REAL case on image(name-independent tag): dict with x, p, ref (R.augment) and, for
    the premises, n_noise_band (pixels within NOISE_BAND of a boundary) and excused (motion: within the bar of a boundary)"""
    p = {**EXACT, **NOISE, **MOTION_REAL}[name]
    x = image("point", H, W)
    ref = R.augment(x, p, SEED, image_index)
    n_band = int(R.near_half(ref["pre_noise"], NOISE_BAND).sum()) if ref["pre_noise"] is not None else 0
    excused = R.near_half(ref["pre_motion"], motion_bar(p["K"])) if ref["pre_motion"] is not None else np.zeros((H, W), bool)
    return dict(x=x, p=p, ref=ref, n_noise_band=n_band, excused=excused)


def blur_input(H, W, quantised):
    """levels-like float32 values; the quantised cases stay below 16 so that the bar at ksize 351 (2 * 353 u 16 = 7e-4 levels) keeps the
    expected excused share (twice the bar; a wide blur of a small image puts all its pixels close together) under SHARE"""
    x = image("blur", H, W)
    return (x * (16.0 if quantised else 255.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def blur_case(H, W, ksize, sigma, quantised):
    x = blur_input(H, W, quantised)
    ref = R.blur(x, ksize, sigma)
    bar = blur_bar(ksize, float(np.abs(x).max()))
    return dict(x=x, ref=ref, bar=bar, excused=R.near_half(ref, bar) if quantised else None)


def ellipses(kind, H, W):
    """planted ellipses (cx, cy, ax, ay, c, s); the odd fractions keep every pixel's form away from 1"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    ax, ay = max(W / 4.0, 0.6) + 0.3713, max(H / 5.0, 0.6) + 0.2171
    rot = lambda deg: (math.cos(math.radians(deg)), math.sin(math.radians(deg)))
    if kind == "none":
        return []
    if kind == "axis":
        return [(cx + 0.123, cy - 0.077, ax, ay, 1.0, 0.0)]
    if kind == "rotated":
        return [(cx - 0.31, cy + 0.17, ax, ay * 0.5 + 0.1, *rot(33.0))]
    if kind == "clipped":          # one across every edge of the image
        return [(0.2, cy, ax * 0.6, ay * 0.6, *rot(10.0)), (W - 1.3, cy, ax * 0.5, ay * 0.7, *rot(80.0)), (cx, -0.4, ax * 0.7, ay * 0.5, *rot(45.0)),
                (cx, H - 0.7, ax * 0.4, ay * 0.6, *rot(5.0))]
    if kind == "overlap":
        return [(cx - ax / 3, cy, ax * 0.7, ay * 0.7, *rot(20.0)), (cx + ax / 3, cy + 0.4, ax * 0.7, ay * 0.9, *rot(70.0))]
    if kind == "cover":
        return [(cx, cy, 2.0 * (H + W) + 0.37, 2.0 * (H + W) + 0.91, *rot(12.0))]
    assert kind == "twenty"
    rs = _rs("twenty", H, W)
    return [(rs.uniform(0, W), rs.uniform(0, H), rs.uniform(0.2, 1.0) * ax + 0.0137, rs.uniform(0.2, 1.0) * ay + 0.0211, *rot(rs.uniform(0, 90)))
            for _ in range(R.MAX_ELLIPSES)]


# (ellipses, t, ksize, quantise_out).  t at both ends of the yaml's range and of the reference's default (-0.5, 0.5, 0.8) and t = 0.  The
# quantise_out cases use the yaml's ksize range (101 .. 151) and t away from simple fractions: inside a fully covered region m = 255 and
# shaded = level (1 - t), which for t = 0.5 sits on a floor boundary for every even level -- the restatement's own excused count would
# pass SHARE there, so the range ends run with quantise_out = 0.
SHADE = (("axis", 0.5, 101, 0), ("rotated", -0.5, 151, 0), ("clipped", 0.8, 2 * MAX_RADIUS + 1, 0), ("overlap", 0.37, 125, 1),
         ("cover", -0.2718281, 101, 1), ("none", 0.5, 151, 1), ("twenty", 0.43, 2 * MAX_RADIUS - 1, 0), ("axis", 0.0, 151, 1), ("twenty", -0.413, 149, 1),
         ("rotated", 0.5, 3, 0), ("overlap", -0.5, 1, 0))
SHADE_LEAD = R.make_params(R.BRIGHTNESS | R.CONTRAST, d=12, alpha=1.1)          # exact stages in front of the shade


@functools.lru_cache(maxsize=None)
def shade_case(H, W, i):
    kind, t, ksize, q = SHADE[i]
    el = ellipses(kind, H, W)
    p = dict(SHADE_LEAD)
    p.update(stages=SHADE_LEAD["stages"] | R.SHADE, ellipses=np.asarray(el, np.float64).reshape(-1, 6), t=float(t), shade_ksize=int(ksize))
    x = image("shade", H, W)
    ref = R.augment(x, p, SEED, 0, quantise_out=bool(q))
    forms = R.ellipse_forms(p["ellipses"], H, W) if len(el) else np.full((1, H, W), 2.0)
    bar = abs(t) * ref["level"] / 255.0 * mask_bar(ksize, ref["mask_blur"])          # in levels, per pixel
    # the boundaries of floor inside the clip range: a value clipped to 0 or 255 is exact on both sides
    raw = ref["shaded_raw"]
    excused = (R.near_integer(raw, bar) & (bar > 0) & (raw > -bar) & (raw < 255.0 + bar)) if q else np.zeros((H, W), bool)
    return dict(x=x, p=p, q=int(q), ref=ref, bar=bar, excused=excused, form_gap=float(np.abs(forms - 1.0).min()))


def batch_params(B):
    """B different parameter sets, image 1 with every stage disabled, shade and noise on others"""
    out = []
    for b in range(B):
        if b == 1:
            out.append(R.make_params())
            continue
        K = (1, 3, 5, 7)[b % 4]
        p = R.make_params(R.BRIGHTNESS | R.CONTRAST | R.NOISE | R.IMPULSE | R.MOTION | (R.SHADE if b % 2 == 0 else 0), d=5 * b - 20, alpha=0.6 + 0.1 * b,
                          sigma=1.0 + b, thr=THR // (b + 1), K=K, weights=line_kernel(K, 0.4 * b + 0.2), t=0.1 * b - 0.3, shade_ksize=21 + 10 * (b % 3))
        out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def batch_case(B, H, W, first):
    """a batch whose images differ in everything; refs by R.augment with image = first + b (stage 5 in the kernel's own float32 order)"""
    params = batch_params(B)
    for b, p in enumerate(params):
        if p["stages"] & R.SHADE:
            p["ellipses"] = np.asarray(ellipses(("axis", "twenty", "clipped")[b % 3], H, W), np.float64).reshape(-1, 6)
    xs = np.stack([image(("batch", b), H, W) for b in range(B)])[:, None]
    refs = [R.augment(xs[b, 0], params[b], SEED, first + b) for b in range(B)]
    n_band = sum(int(R.near_half(r["pre_noise"], NOISE_BAND).sum()) for r in refs if r["pre_noise"] is not None)
    return dict(x=xs, params=params, refs=refs, n_noise_band=n_band)


def shade_out_bar(ref, bar_levels):
    """the bar of the float32 output in output units: the shade's bar / 255 and one rounding of the quotient"""
    return bar_levels / 255.0 + U * np.abs(ref["out"])
