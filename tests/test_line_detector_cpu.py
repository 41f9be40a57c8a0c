"""CPU: the NumPy restatement of the line segment detector (tests/line_detector_reference.py) alone -- its labelling against
scipy.ndimage.label, its bucket tests against Python's big integers, its filters against scipy's, drawn scenes with known edges, a
shifted scene, the distance of every region from the density threshold -- and the header, exports and refusals of the native entry points
that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import line_detector_cases as LC
import line_detector_reference as R
from linetr_amd import _native as nat

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_POINTS = ("linetr_detect_lines_workspace_bytes", "linetr_detect_lines", "linetr_detect_tile", "linetr_detect_debug_labels_workspace_bytes",
                "linetr_detect_debug_labels", "linetr_detect_debug_gradient")


@pytest.fixture(scope="module")
def scenes():
    """name -> (image, rows, regions per octave): computed once, never changed"""
    out = {}
    for name in LC.SCENE_NAMES:
        img = LC.scene(name)
        rows, regions, _ = R.detect(img, want_debug=True)
        out[name] = (img, rows, regions)
    return out


def scipy_labels(bk):
    ndi = pytest.importorskip("scipy.ndimage")
    out = np.full(bk.shape, -1, np.int64)
    idx = np.arange(bk.size).reshape(bk.shape)
    for b in np.unique(bk[bk >= 0]):
        lab, n = ndi.label(bk == b, structure=np.ones((3, 3)))
        if n:
            smallest = ndi.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int64)
            out[lab > 0] = smallest[lab[lab > 0] - 1]
    return out


@pytest.mark.parametrize("pattern", sorted(LC.PATTERNS))
def test_labelling_equals_scipy(pattern):
    for H, W in LC.label_sizes():
        bk = LC.PATTERNS[pattern](H, W)
        assert bk.shape == (H, W) and bk.dtype == np.int8
        assert np.array_equal(R.label_regions(bk), scipy_labels(bk)), (pattern, H, W)


def test_planted_patterns_are_what_their_names_say():
    T = LC.T
    H, W = 2 * T + 3, 3 * T + 1
    for name in ("serpentine", "spiral"):
        lab = R.label_regions(LC.PATTERNS[name](H, W))
        assert set(np.unique(lab)) == {-1, 0} and (lab == 0).sum() > 3 * max(H, W), name        # one long region through every tile
    lab = R.label_regions(LC.checkerboard(H, W))
    assert np.array_equal(lab.ravel(), np.arange(H * W))                                          # every cell its own region
    assert set(np.unique(R.label_regions(LC.diagonal_touch(H, W)))) == {-1, 0}                    # joined through corners only
    lab = R.label_regions(LC.one_apart(H, W))
    assert len(np.unique(lab[lab >= 0])) == (W + 1) // 2                                          # one cell apart stays apart
    lab = R.label_regions(LC.tile_corner(H, W))
    assert lab[T, T] == (T - 2) * W + T + 1 and lab[T + 1, T + 1] == lab[T - 1, T - 1]            # across the corner, both diagonals


def test_buckets_next_to_every_boundary_equal_big_integer_arithmetic():
    pairs = LC.boundary_pairs()
    for u, v in LC.CONVERGENTS:
        assert len(set(LC.octant_images(u, v))) == 8 and set(LC.octant_images(u, v)) <= set(pairs)
    assert (7, 7) in pairs and (-100, 100) in pairs and (0, 7) in pairs and (-100, 0) in pairs
    g = np.asarray(pairs, dtype=np.int64)
    a, b = R.buckets(g[:, 0], g[:, 1])
    for (gx, gy), got_a, got_b in zip(pairs, a.tolist(), b.tolist()):
        assert (got_a, got_b) == LC.bucket_by_bigint(gx, gy), (gx, gy)
    # and against the angle itself wherever it is clear of a boundary
    ang = np.degrees(np.arctan2(g[:, 1].astype(float), g[:, 0].astype(float))) % 360.0
    clear_a = np.abs((ang / 45.0) - np.round(ang / 45.0)) > 1e-6
    assert np.array_equal(a[clear_a], np.floor(ang[clear_a] / 45.0).astype(np.int64))
    clear_b = np.abs(((ang - 22.5) / 45.0) - np.round((ang - 22.5) / 45.0)) > 1e-6
    assert np.array_equal(b[clear_b], np.floor(((ang[clear_b] - 22.5) % 360.0) / 45.0 + 1).astype(np.int64) % 8)
    # the convergents straddle sqrt 2 - 1: 5/12 and 29/70 above, 12/29 below
    assert R.buckets(12, 5)[1] == 1 and R.buckets(29, 12)[1] == 0 and R.buckets(70, 29)[1] == 1
    # values at the top of the range stay exact in 64 bit
    big = 2 * 8160
    assert tuple(int(v) for v in R.buckets(big, big)) == LC.bucket_by_bigint(big, big)


def test_planted_gradient_image_carries_the_pairs():
    pairs = [p for p in LC.boundary_pairs() if abs(p[0]) + abs(p[1]) <= 255]
    assert {(70, 29), (-29, 70), (12, -5), (7, 7), (100, 0)} <= set(pairs)
    img = LC.planted_gradient_image(pairs)
    S = R.smooth16(img)
    gx = S[:-1, 1:] + S[1:, 1:] - S[:-1, :-1] - S[1:, :-1]
    gy = S[1:, :-1] + S[1:, 1:] - S[:-1, :-1] - S[:-1, 1:]
    at = 8 * np.arange(len(pairs)) + 1
    assert np.array_equal(np.stack([gx[1, at], gy[1, at]], axis=1), 2 * np.asarray(pairs))
    m2, bA, bB = R.gradient(img, 1)
    for j, (px, py) in enumerate(pairs):
        assert (int(bA[1, at[j]]), int(bB[1, at[j]])) == LC.bucket_by_bigint(px, py)
        assert int(m2[1, at[j]]) == 4 * (px * px + py * py)


def test_filters_equal_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for H, W in ((33, 47), (2, 2), (1, 9), (9, 1), (3, 2), (64, 65)):
        q = LC.random_image(H, W, 5 + H)
        k3 = np.outer([1, 2, 1], [1, 2, 1])
        assert np.array_equal(R.smooth16(q), ndi.correlate(q.astype(np.int64), k3, mode="mirror"))
        k5 = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
        if min(H, W) >= 3:          # scipy's mirror wants the kernel's reach inside the image
            want = ((ndi.correlate(q.astype(np.int64), k5, mode="mirror") + 128) >> 8)[::2, ::2]
            assert np.array_equal(R.pyramid_next(q), want.astype(np.uint8))
        assert R.pyramid_next(q).shape == ((H + 1) // 2, (W + 1) // 2)
    assert np.array_equal(R.reflect101(np.arange(-5, 8), 3), [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1])
    assert np.array_equal(R.reflect101(np.arange(-3, 4), 1), np.zeros(7))
    m2 = np.array([0, 1, 3, 4, 8, 9, 28160, 133171200, 2 ** 31 - 1], dtype=np.int64)
    w = R.isqrt(m2)
    assert np.all(w * w <= m2) and np.all((w + 1) * (w + 1) > m2)
    f = np.array([[0.0, 1.0, 0.5, 0.999, 1.0 / 255, 0.2]], dtype=np.float32)
    assert np.array_equal(R.quantise(f), (f * np.float32(255)).astype(np.uint8)) and R.quantise(f)[0, 1] == 255


def test_small_and_empty_images():
    assert R.detect(np.zeros((1, 1), np.uint8)).shape == (0, 6)
    assert R.detect(np.zeros((1, 40), np.uint8), {"n_octave": 3}).shape == (0, 6)
    assert R.detect(np.full((64, 64), 99, np.uint8), {"n_octave": 8}).shape == (0, 6)            # octaves below 2 x 2 are no error
    for bad in ({"scale": 3}, {"n_octave": 0}, {"min_region_size": 3}, {"grad_threshold": 0}):
        with pytest.raises(ValueError):
            R.detect(np.zeros((8, 8), np.uint8), bad)
    with pytest.raises(ValueError):
        R.detect(np.zeros((2049, 8), np.uint8))


@pytest.mark.parametrize("name", LC.SCENE_NAMES)
def test_every_long_edge_of_a_drawn_scene_is_found(scenes, name):
    img, rows, _ = scenes[name]
    assert img.dtype == np.uint8 and img.shape == LC.SCENE_SHAPE
    err = LC.edge_errors(rows, LC.scene_edges(name))
    print(f"{name}: {len(rows)} lines, worst end-point error per edge {np.round(err, 3)}")
    bar = 1.5 * LC.EDGE_ERROR_MEASURED
    assert bar <= LC.EDGE_BAR_CEILING
    assert err.max() <= bar, (name, err)
    assert set(np.unique(rows[:, 5])) == {0.0, 1.0}
    # lineLength is in pixels of the line's octave
    length = np.hypot(rows[:, 2] - rows[:, 0], rows[:, 3] - rows[:, 1])
    assert np.allclose(length, rows[:, 4] * 2.0 ** rows[:, 5], rtol=1e-12)


def test_scenes_hold_the_asked_orientations():
    angles = sorted(b[0] for b in LC.SCENES["bars"])
    assert angles[0] == 0.0 and 90.0 in angles and 45.0 in angles and any(abs(a - 22.5) <= 2 for a in angles) and any(70 <= a < 90 for a in angles)
    for bars in LC.SCENES.values():
        for ang, cx, cy, length, width in bars:
            reach = (length + width) / 2 + 12
            assert reach <= cx <= LC.SCENE_SHAPE[1] - reach or abs(np.cos(np.deg2rad(ang))) * reach <= min(cx, LC.SCENE_SHAPE[1] - cx)
            assert abs(np.sin(np.deg2rad(ang))) * length / 2 + width / 2 + 12 <= min(cy, LC.SCENE_SHAPE[0] - cy)


def test_shifted_scene_gives_shifted_rows(scenes):
    img, rows, _ = scenes["bars"]
    dx, dy = LC.SHIFT
    got = R.detect(LC.shifted(img))
    want = rows.copy()
    want[:, [0, 2]] += dx
    want[:, [1, 3]] += dy
    assert got.shape == want.shape
    print(f"shifted scene: max deviation {np.abs(got - want).max():.3e} px")
    assert np.abs(got - want).max() <= 1e-9


def test_no_region_lies_at_the_density_threshold(scenes):
    """so the device and the restatement can never disagree on a keep decision"""
    worst = np.inf
    for name, (_, _, regions) in scenes.items():
        for reg in regions:
            for r in reg:
                worst = min(worst, abs(r["fill"] / R.DEFAULTS["density"] - 1.0))
                assert r["l"][1] - r["l"][0] > 1e-9                      # nor at the l_max <= l_min test
    print(f"closest region to the density threshold: {worst:.3e} relative")
    assert worst > 1e-9


def test_debug_rows_and_order(scenes):
    _, rows, regions = scenes["more"]
    dbg = R.kept_debug_rows(regions)
    assert len(dbg) == len(rows) and np.array_equal(dbg[:, 0], rows[:, 5].astype(np.int64))
    key = dbg[:, 0] * 2 ** 40 + dbg[:, 1] * 2 ** 32 + dbg[:, 2]
    assert np.all(np.diff(key) > 0)                                      # octave-major, A before B, ascending label
    assert np.all(dbg[:, 3] >= R.DEFAULTS["min_region_size"]) and np.all(dbg[:, 4:] >= 0) and dbg[:, 4:].max() < 2 ** 58


def test_asset_pair_line_counts():
    g = np.load(os.path.join(ROOT, "tests", "golden", "asset_pair_images.npz"))
    counts = []
    for k in ("gray0", "gray1"):
        rows = R.detect(np.squeeze(g[k]))
        counts.append((len(rows), int((rows[:, 4] * 2.0 ** rows[:, 5] > 16).sum())))
    assert counts == [(186, 131), (177, 131)]


def test_header_declares_and_library_exports_the_entry_points():
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in nat.EXPORTS and hasattr(L, name), name
    assert "#define LINETR_ABI_VERSION 6" in hdr and L.linetr_abi_version() == 6
    assert "typedef struct LinetrDetectConfig" in hdr and nat.C.sizeof(nat.DetectConfig) == 24
    th, tw = nat.C.c_int32(), nat.C.c_int32()
    assert L.linetr_detect_tile(nat.C.byref(th), nat.C.byref(tw)) == 0 and (th.value, tw.value) == LC.TILE
    assert L.linetr_detect_tile(None, None) == nat.E_ARG
    assert L.linetr_detect_lines_workspace_bytes(1, 480, 640, 2) > 0
    assert L.linetr_detect_lines_workspace_bytes(32, 480, 640, 2) >= 32 * L.linetr_detect_lines_workspace_bytes(1, 480, 640, 2) // 2
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 2049, 1), (1, 8, 8, 0), (1, 8, 8, 13)):
        assert L.linetr_detect_lines_workspace_bytes(*bad) == 0, bad


def test_refusals_come_before_any_device_call():
    """no pointer below is ever dereferenced on the device: every call is refused on its arguments alone"""
    from linetr_amd.engine import Engine
    L = nat.lib()
    img, rows, counts, ws = 0x100000, 0x200000, 0x300000, 0x400000
    need = L.linetr_detect_lines_workspace_bytes(2, 16, 16, 2)

    def detect(img=img, is_float=0, B=2, H=16, W=16, cfg={}, no_cfg=False, cap=8, rows=rows, counts=counts, dbg=None, ws=ws, ws_bytes=need):
        c = Engine.detect_config(**cfg)
        return L.linetr_detect_lines(None, img, is_float, B, H, W, None if no_cfg else nat.C.byref(c), cap, rows, counts, dbg, ws, ws_bytes, None)
    for kw, text in ((dict(B=0), b"B="), (dict(B=-1), b"B="), (dict(H=0), b"outside 1..2048"), (dict(W=2049), b"outside 1..2048"),
                     (dict(H=2049), b"outside 1..2048"), (dict(cfg={"n_octave": 0}), b"n_octaves"), (dict(cfg={"n_octave": 13}), b"n_octaves"),
                     (dict(cfg={"scale": 3}), b"scale"), (dict(cfg={"grad_threshold": 0}), b"grad_threshold"),
                     (dict(cfg={"min_region_size": 3}), b"min_region_size"), (dict(cfg={"density": float("nan")}), b"density"),
                     (dict(cfg={"density": 1.5}), b"density"), (dict(no_cfg=True), b"null"), (dict(img=None), b"null"), (dict(rows=None), b"null"),
                     (dict(counts=None), b"null"), (dict(ws=None), b"null"), (dict(ws_bytes=need - 1), b"workspace too small"),
                     (dict(ws_bytes=0), b"workspace too small"), (dict(cap=-1), b"capacity"), (dict(is_float=2), b"images_are_float"),
                     (dict(rows=rows + 4), b"misaligned rows"), (dict(img=img + 2, is_float=1), b"misaligned rows"),
                     (dict(dbg=0x500004), b"misaligned rows"), (dict(ws=ws + 8), b"misaligned rows")):
        assert detect(**kw) == nat.E_ARG and text in L.linetr_last_error(), (kw, L.linetr_last_error())

    def labels(bk=img, B=2, H=5, W=7, out=rows, ws=ws, ws_bytes=4096):
        return L.linetr_detect_debug_labels(None, bk, B, H, W, out, ws, ws_bytes, None)
    for kw in (dict(bk=None), dict(out=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=2049), dict(ws_bytes=2 * 5 * 7 * 4 - 1), dict(out=rows + 2)):
        assert labels(**kw) == nat.E_ARG and L.linetr_last_error(), kw

    def grad(img=img, B=2, H=16, W=16, cfg={}, octave=0, m2=rows, a=counts, b=counts + 4096, ws=ws, ws_bytes=need):
        c = Engine.detect_config(**cfg)
        return L.linetr_detect_debug_gradient(None, img, 0, B, H, W, nat.C.byref(c), octave, m2, a, b, ws, ws_bytes, None)
    for kw in (dict(img=None), dict(m2=None), dict(a=None), dict(b=None), dict(ws=None), dict(B=0), dict(H=0), dict(octave=2), dict(octave=-1),
               dict(ws_bytes=need - 1), dict(cfg={"scale": 1})):
        assert grad(**kw) == nat.E_ARG and L.linetr_last_error(), kw


def test_python_surface_without_a_device():
    from linetr_amd.engine import Engine
    from linetr_amd.frontends.line_detector import LSD, KeyLine
    from linetr_amd.matching import _frontend
    lsd = _frontend("line_detector", "LSD", {"n_octave": 1})
    assert isinstance(lsd, LSD) and lsd.config == {**LSD.default_config, "n_octave": 1}
    assert LSD.default_config["n_octave"] == 2 and LSD.default_config["scale"] == 2
    assert {k: LSD.default_config[k] for k in R.DEFAULTS} == R.DEFAULTS == Engine.DETECT_DEFAULTS
    with pytest.raises(ValueError):
        LSD({"scale": 4})
    with pytest.raises(ValueError):
        LSD({"threshold": 4})
    with pytest.raises(RuntimeError, match="HIP device"):
        lsd.detect_torch(torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError):
        Engine.detect_config(octaves=2)
    kl = KeyLine([2.0, 4.0, 10.0, 10.0, 5.0, 1.0], 3, 320.0)
    assert (kl.startPointX, kl.startPointY, kl.endPointX, kl.endPointY, kl.lineLength, kl.octave) == (2.0, 4.0, 10.0, 10.0, 5.0, 1)
    assert (kl.sPointInOctaveX, kl.ePointInOctaveY, kl.numOfPixels, kl.class_id, kl.pt) == (1.0, 5.0, 6, 3, (6.0, 7.0))
    assert kl.response == 5.0 / 320.0 and abs(kl.angle - np.arctan2(6.0, 8.0)) < 1e-15
    from linetr_amd.line_process import keylines_to_array
    assert np.array_equal(keylines_to_array([kl]), [[2.0, 4.0, 10.0, 10.0, 5.0, 1.0]])
