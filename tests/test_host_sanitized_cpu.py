"""CPU: the HOST half of the library under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer.

The other CPU suites reach the host code through ctypes, at -O3, with NumPy arrays as buffers: an over-read of a caller's buffer lands
in the neighbouring heap and nothing notices.  Here tests/host_driver/host_driver.cpp, a program of its own, is linked against the
library's translation units compiled from source with the host side instrumented (tests/host_driver_build.py), hands the C ABI heap
allocations of exactly the documented sizes and runs as a child process; any sanitizer report or non-zero exit fails the test with the
report in the message.  What the sanitized run computed is then checked against the same independent references the other CPU suites
use, under their rules (the oracle's pre-filter, fixed_size_reference, the float64 restatements of the folds, photometric_reference's
sampler, the pinned workspace tables): a clean run of a wrong answer does not pass.  Nothing is compared with the unsanitized .so.

Nothing is preloaded and no interpreter is instrumented; the executables carry their sanitizer's runtime.  The module skips itself,
before anything is compiled, where a HIP device is visible (the driver is for hosts without one) or hipcc is missing."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest


def _why_not():
    try:
        import torch
        if torch.cuda.is_available():
            return "a HIP device is visible: the sanitized host driver runs on hosts without one"
    except Exception:
        pass
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        return "hipcc not found"
    return None


if _why_not():
    pytest.skip(_why_not(), allow_module_level=True)

import host_driver_build as HB                                    # noqa: E402
import photometric_cases as PHC                                   # noqa: E402
import photometric_reference as PR                                # noqa: E402
import prepare_cases as PC                                        # noqa: E402
import fixed_size_reference as FR                                 # noqa: E402
import test_photometric_cpu as TPH                                # noqa: E402
import test_prepare_cpu as TP                                     # noqa: E402
import test_workspace_layouts_cpu as TW                           # noqa: E402
from helpers import BASE_CFG, load                                # noqa: E402
from linetr_amd import _native as nat                             # noqa: E402
from oracle import linetr_oracle as O                             # noqa: E402
from workloads import synth                                       # noqa: E402

E_ARG, E_ASSERT, E_WORKSPACE, E_CAPACITY = -1, -4, -5, -6         # LinetrStatus (include/linetr_hip.h)
REPORT = re.compile(r"Sanitizer|runtime error|terminate called|LeakSanitizer")


@pytest.fixture(scope="module")
def asan():
    return HB.build("asan")


@pytest.fixture(scope="module")
def tsan():
    return HB.build("tsan")


def run_driver(exe, command, directory, env=None, timeout=300):
    r = subprocess.run([exe, command, str(directory)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout,
                       env={**os.environ, **(env or {})})
    assert r.returncode == 0 and not REPORT.search(r.stderr), f"host_driver {command}: exit {r.returncode}\n{r.stderr[-6000:]}\n{r.stdout[-1000:]}"
    assert f"host_driver {command}: ok" in r.stdout
    return r


# ---- prefilter -------------------------------------------------------------------------------------------------------------------------

def _pf_case(ident, images, hw, cfg, masks=None, expect=0):
    """images: a list of [K_i, 6] arrays; masks: None or a list of (array or None)"""
    return dict(id=ident, images=[np.ascontiguousarray(r, np.float64).reshape(-1, 6) for r in images], hw=hw, cfg=cfg,
                masks=masks or [None] * len(images), expect=expect)


def _fixture_case(name):
    g = load(name)
    cfg = dict(BASE_CFG)
    for k in g.files:
        if k.startswith("cfg_"):
            cfg[k[4:]] = g[k].item()
    return _pf_case(name, [g["lines"]], tuple(int(v) for v in g["hw"]), cfg)


def prefilter_cases():
    hw = (480, 640)
    cases = [_pf_case(f"random{seed}", [synth.synth_lines(seed, 200, *hw, len_lo=5.0)], hw, BASE_CFG) for seed in (11, 12, 77)]
    cases += [_fixture_case(n) for n in ("tiny_default", "tiny_max3", "tiny_noborder", "tiny_float_td")]
    g = load("tiny_validmask")
    ghw = tuple(int(v) for v in g["hw"])
    vm = np.ones(ghw)
    vm[:, :int(g["valid_mask_cols"])] = 0
    cases.append(_pf_case("tiny_validmask", [g["lines"]], ghw, BASE_CFG, [vm]))
    # lineLength beyond the geometric length: the reference's AssertionError
    cases.append(_pf_case("assertion", [np.array([[100.0, 100.0, 150.0, 100.0, 200.0, 0.0], [10.0, 10.0, 300.0, 10.0, 20.0, 0.0]])], ghw, BASE_CFG,
                          expect=E_ASSERT))
    cases.append(_pf_case("no_lines", [np.zeros((0, 6))], hw, BASE_CFG))
    cases.append(_pf_case("no_images", [], hw, BASE_CFG))
    # end points that graze width - border - 0.001 and height - border - 0.001 from both sides, and the border itself; every value a
    # float32 (the detector's type, and what the oracle's key-line objects hold), so the neighbours are float32 neighbours
    b, (H, W), f32 = 8, hw, np.float32
    below = lambda v: float(np.nextafter(f32(v), f32(0)))
    graze = [[100.0, 100.0, below(W - b - 0.001), 100.0], [100.0, 120.0, float(f32(W - b - 0.0005)), 120.0], [100.0, 140.0, W - b, 140.0],
             [100.0, 160.0, below(W - b), 160.0], [200.0, 100.0, 200.0, below(H - b - 0.001)], [220.0, 100.0, 220.0, below(H - b)],
             [float(b), float(b), 100.0, float(b)], [below(b), 50.0, 100.0, 50.0], [float(f32(W - b - 0.0005)), 300.0, below(W - b - 0.001), 200.0]]
    rows = [[*l, float(f32(0.9 * np.hypot(l[2] - l[0], l[3] - l[1]))), 0.0] for l in graze]
    cases.append(_pf_case("grazing", [np.array(rows)], hw, BASE_CFG))
    short = synth.synth_lines(5, 30, *hw, len_lo=5.0, len_hi=15.0)                  # every line below min_length
    half = np.ones(hw)
    half[:, :320] = 0
    cases.append(_pf_case("three", [synth.synth_lines(21, 60, *hw), np.zeros((0, 6)), short], hw, BASE_CFG, [None, None, half]))
    imgs = [synth.synth_lines(300 + i, 60, *hw) for i in range(32)]
    for i, idx in ((1, (3, 11, 17, 40)), (4, (0, 59))):                             # equal lengths: images 1 and 4 are reported
        imgs[i][list(idx), 4] = 18.0 + i
    imgs[4][30:40, 4] = 25.0
    imgs[5], imgs[9] = np.zeros((0, 6)), short
    for max_k in (-1, 50):
        cases.append(_pf_case(f"pool{max_k}", imgs, hw, dict(BASE_CFG, max_keylines=max_k), [half if i in (2, 9, 30) else None for i in range(32)]))
    return cases


def write_prefilter_cases(d, cases):
    rows = []
    for c in cases:
        cat = np.concatenate(c["images"]) if c["images"] else np.zeros((0, 6))
        off = np.concatenate([[0], np.cumsum([len(r) for r in c["images"]])]).astype(np.int32)
        cat.astype(np.float64).tofile(d / f"{c['id']}_lines.bin")
        off.tofile(d / f"{c['id']}_off.bin")
        for i, m in enumerate(c["masks"]):
            if m is not None:
                np.ascontiguousarray(m, np.float64).tofile(d / f"{c['id']}_vm{i}.bin")
        cfg = c["cfg"]
        rows.append(" ".join([c["id"], str(len(c["images"])), str(c["hw"][0]), str(c["hw"][1]), str(int(cfg["remove_borders"])),
                              repr(float(cfg["min_length"])), str(int(cfg["max_keylines"])), repr(float(cfg["token_distance"])),
                              str(int(cfg["max_tokens"])), str(c["expect"])]))
    (d / "cases.txt").write_text("\n".join(rows) + "\n")


def oracle_image(rows, hw, cfg, vm, tied):
    """the oracle's pre-filter; an image with equal lengths under the tie rule the header documents (a stable ascending sort, reversed)"""
    if len(rows) == 0:
        return dict(klines=np.zeros((0, 2, 2)), length_klines=np.zeros(0), angles=np.zeros((0, 2)))
    lines = O.cv2_to_arrays(synth.array_to_keylines(rows))
    lines = O.drop_border_lines(lines, cfg["remove_borders"], hw[0], hw[1], vm)
    if not tied:
        return O.keep_long_lines(lines, cfg["min_length"], cfg["max_keylines"])
    sel = lines["length_klines"] > cfg["min_length"]
    kl, ln = lines["klines"][sel], lines["length_klines"][sel]
    order = np.argsort(ln, kind="stable")[::-1][:cfg["max_keylines"]]
    return dict(klines=kl[order], length_klines=ln[order], angles=O.line_angles(kl[order]) if len(order) else np.zeros((0, 2)))


def check_records(recs, cu_k, cu_n, tied, images, hw, cfg, masks, where):
    td, T = float(cfg["token_distance"]), int(cfg["max_tokens"])
    assert cu_k[0] == 0 and cu_n[0] == 0 and len(recs) == cu_k[-1], where
    for i, rows in enumerate(images):
        ref = oracle_image(rows.copy(), hw, cfg, masks[i], i in tied)
        r = recs[cu_k[i]:cu_k[i + 1]]
        assert len(r) == len(ref["klines"]), (where, i, len(r), len(ref["klines"]))
        if len(r) == 0:
            assert cu_n[i + 1] == cu_n[i], (where, i)
            continue
        assert np.array_equal(r["sp"], ref["klines"][:, 0]) and np.array_equal(r["ep"], ref["klines"][:, 1]), (where, i)
        assert np.array_equal(r["length"], ref["length_klines"]), (where, i)
        assert np.abs(r["angle"] - ref["angles"]).max() < 1e-15, (where, i)
        ntok = np.ceil(ref["length_klines"] / td).astype(int)
        assert np.array_equal(r["n_tok"], ntok) and np.array_equal(r["n_sub"], -(-ntok // T)), (where, i)
        assert cu_n[i + 1] - cu_n[i] == r["n_sub"].sum(), (where, i)
        assert np.array_equal(r["first_sub"], cu_n[i] + np.cumsum(r["n_sub"]) - r["n_sub"]), (where, i)
        assert (r["image"] == i).all() and np.array_equal(r["line_local"], np.arange(len(r))), (where, i)
        # which images hold equal lengths among their candidates: the library's report against the filtered lengths
        lines = O.drop_border_lines(O.cv2_to_arrays(synth.array_to_keylines(rows.copy())), cfg["remove_borders"], hw[0], hw[1], masks[i])
        ln = lines["length_klines"][lines["length_klines"] > cfg["min_length"]]
        assert (len(np.unique(ln)) != len(ln)) == (i in tied), (where, i)
    assert np.array_equal(recs["first_tok"], np.cumsum(recs["n_tok"]) - recs["n_tok"]), where


def test_prefilter_every_thread_setting_against_the_oracle(asan, tmp_path):
    cases = prefilter_cases()
    outputs = {}
    for threads in ("0", "1", "3", "100"):                          # the pool's size comes from the child's environment (100: clamped)
        d = tmp_path / f"threads{threads}"
        d.mkdir()
        write_prefilter_cases(d, cases)
        run_driver(asan, "prefilter", d, env={"LINETR_HOST_THREADS": threads})
        outputs[threads] = {p.name: p.read_bytes() for p in sorted(d.iterdir()) if re.search(r"_(recs|cu_k|cu_n|tied)\.bin$", p.name)}
    first = outputs["0"]
    assert len(first) == 4 * sum(c["expect"] == 0 for c in cases)
    for threads, out in outputs.items():
        assert out.keys() == first.keys() and all(out[k] == first[k] for k in first), f"LINETR_HOST_THREADS={threads} gives other bytes"
    seen_tied = set()
    for c in cases:
        if c["expect"]:
            continue
        recs = np.frombuffer(first[c["id"] + "_recs.bin"], nat.REC_DTYPE)
        cu_k, cu_n = (np.frombuffer(first[c["id"] + f"_{k}.bin"], np.int32) for k in ("cu_k", "cu_n"))
        tied = set(np.frombuffer(first[c["id"] + "_tied.bin"], np.int32).tolist())
        assert len(cu_k) == len(cu_n) == len(c["images"]) + 1
        check_records(recs, cu_k, cu_n, tied, c["images"], c["hw"], c["cfg"], c["masks"], c["id"])
        seen_tied |= {(c["id"], i) for i in tied}
    assert {("pool-1", 1), ("pool-1", 4), ("pool50", 1), ("pool50", 4)} <= seen_tied
    # the special-line fixtures carry the reference's own output
    for name in ("tiny_default", "tiny_max3", "tiny_noborder", "tiny_float_td", "tiny_validmask"):
        g = load(name)
        recs = np.frombuffer(first[name + "_recs.bin"], nat.REC_DTYPE)
        assert np.array_equal(recs["sp"].astype(np.float32), g["klines"][0][:, 0]), name
        if name != "tiny_validmask":                                 # (that fixture keeps the key-lines alone)
            assert np.frombuffer(first[name + "_cu_n.bin"], np.int32)[1] == g["sublines"].shape[1], name
            assert np.array_equal(recs["length"].astype(np.float32), g["length_klines"][0]), name


# ---- pseudo lines ------------------------------------------------------------------------------------------------------------------------

PSEUDO = (("a", 0, 0, 40, (640, 480), 16.0, 250), ("b", 7, 3, 25, (640, 480), 16.0, 250), ("c", 123456789, 31, 17, (320, 240), 16.0, 250),
          ("none", 1, 0, 0, (640, 480), 16.0, 250), ("cut0", 5, 1, 12, (640, 480), 16.0, 0), ("cut3", 5, 1, 12, (640, 480), 16.0, 3),
          ("beyond", 5, 1, 12, (640, 480), 16.0, 13), ("minus1", 5, 1, 12, (640, 480), 16.0, -1), ("minus40", 5, 1, 12, (640, 480), 16.0, -40),
          ("long", 9, 2, 30, (200, 180), 70.0, 30))


def write_pseudo_cases(d):
    (d / "cases.txt").write_text("".join(f"{i} {seed} {image} {n} {float(s[0])!r} {float(s[1])!r} {ml!r} {cut}\n" for i, seed, image, n, s, ml, cut in PSEUDO))


def test_pseudo_lines_against_the_restatement(asan, tmp_path):
    write_pseudo_cases(tmp_path)
    run_driver(asan, "pseudo", tmp_path)
    for ident, seed, image, n, shape, ml, cut in PSEUDO:
        want = FR.make_pseudo_lines(seed, image, n, shape, ml)
        got = np.fromfile(tmp_path / f"{ident}_lines.bin", np.float64)
        assert got.tobytes() == want.tobytes(), ident
        attrs = FR.find_line_attributes(want, ml, cut)
        k = int(np.fromfile(tmp_path / f"{ident}_n.bin", np.int32)[0])
        assert k == len(attrs["klines"]), (ident, k)
        for name, key, per in (("klines", "klines", 4), ("length", "length_klines", 1), ("angles", "angles", 2)):
            assert np.fromfile(tmp_path / f"{ident}_{name}.bin", np.float64)[:k * per].tobytes() == attrs[key].tobytes(), (ident, name)


# ---- weight preparation ------------------------------------------------------------------------------------------------------------------

PREPARE = tuple(c for c in PC.CONFIGS if c[3] or c[1] in (0, 1, 7))


def write_prepare_case(d, weights, n_layers, widths, training):
    sd = PC.config_state_dict(weights, n_layers, widths)[0]
    names = [k for k in sd if not k.endswith("num_batches_tracked")]
    (d / "names.txt").write_text("\n".join(names) + "\n")
    for i, k in enumerate(names):
        np.ascontiguousarray(sd[k], np.float32).tofile(d / f"t{i}.bin")              # the driver gives each tensor an allocation of its own
    (d / "cfg.bin").write_bytes(bytes(PC.model_config(**PC.config_kwargs(n_layers, widths, training))))


@pytest.mark.parametrize("weights,n_layers,widths,training", PREPARE)
def test_prepare_against_the_float64_restatements(asan, tmp_path, monkeypatch, weights, n_layers, widths, training):
    write_prepare_case(tmp_path, weights, n_layers, widths, training)
    run_driver(asan, "prepare", tmp_path)
    mine = PC.Prepared(np.fromfile(tmp_path / "image.bin", np.float32), np.fromfile(tmp_path / "table.bin", nat.PREPARED_ENTRY_DTYPE))
    # the existing suite's checks, with the sanitized run's image in the place of the shared library's
    monkeypatch.setattr(PC, "prepared", lambda *a, **k: mine)
    if training:
        TP.test_training_mode_configuration(weights, n_layers, widths, training)
    else:
        TP.test_folds_against_the_restatement(weights, n_layers)
        if n_layers == 7:
            TP.test_pooling_constants_and_encoders_against_float64(weights)
    t, end = mine.table, 0                                                             # placement, as test_table_layout walks it
    for r in t[:-2]:
        assert int(r["offset"]) == (end + 63) // 64 * 64, r["name"]
        end = int(r["offset"]) + int(r["rows"]) * int(r["cols"])
    assert end == mine.arena_floats() and [r["name"] for r in t[-2:]] == [b"c_tok", b"s_cls"]


# ---- photometric sampler -----------------------------------------------------------------------------------------------------------------

def photo_variants():
    import json
    with open(os.path.join(TPH.ROOT, "tests", "golden", "homography_photometric.json")) as fh:     # the yaml_config fixture's file
        base = json.load(fh)
    out = {}
    for variant in ("yaml", "defaults_k7_blur", "shade_only", "nothing"):
        cfg = json.loads(json.dumps(base))
        prm = cfg["photometric"]["params"]
        if variant == "defaults_k7_blur":
            prm["motion_blur"]["max_kernel_size"] = 7
            prm["additive_shade"] = {}
            prm["GaussianBlur"] = {"sigma": 1.7}
        elif variant == "shade_only":
            cfg["photometric"]["params"] = {"additive_shade": prm["additive_shade"]}
        elif variant == "nothing":
            cfg["photometric"]["enable"] = False
        out[variant] = PR.config_stages(cfg)
    return out


PHOTO_SHAPE = (64, 120, 160, 5)                                     # B, H, W, first


def write_photo_cases(tmp_path):
    B, H, W, first = PHOTO_SHAPE
    variants = photo_variants()
    rows = []
    for name, flat in variants.items():
        (tmp_path / f"{name}_cfg.bin").write_bytes(bytes(TPH.config_struct(flat)))
        (tmp_path / f"{name}1_cfg.bin").write_bytes(bytes(TPH.config_struct(flat)))
        rows += [f"{name} {PHC.SEED} {first} {B} {H} {W} 0", f"{name}1 {PHC.SEED} {first + 9} 1 {H} {W} 0"]
    flat = variants["yaml"]
    refused = {"r_batch0": (flat, 1, 0, 0, 64, 64), "r_h19": (flat, 1, 0, 2, 19, 64), "r_first": (flat, 1, -1, 2, 64, 64), "r_seed": (flat, 1 << 32, 0, 2, 64, 64),
               "r_ellipses": ({**flat, "nb_ellipses": 21}, 1, 0, 2, 64, 64), "r_kernel": ({**flat, "max_kernel_size": 9}, 1, 0, 2, 64, 64),
               "r_nan": ({**flat, "transparency_range": (float("nan"), 1.0)}, 1, 0, 2, 64, 64)}
    for name, (f, seed, fst, b, h, w) in refused.items():
        (tmp_path / f"{name}_cfg.bin").write_bytes(bytes(TPH.config_struct(f)))
        rows.append(f"{name} {seed} {fst} {b} {h} {w} {E_ARG}")
    (tmp_path / "cases.txt").write_text("\n".join(rows) + "\n")
    return variants


def test_photometric_sampler_against_the_restatement(asan, tmp_path):
    B, H, W, first = PHOTO_SHAPE
    variants = write_photo_cases(tmp_path)
    run_driver(asan, "photo", tmp_path)
    for name, flat in variants.items():
        got = np.fromfile(tmp_path / f"{name}_params.bin", nat.PHOTO_PARAMS_DTYPE)
        rec = PR.to_records(PR.sample(flat, PHC.SEED, first, B, H, W), nat.PHOTO_PARAMS_DTYPE)
        assert len(got) == B
        for k in ("stages", "d", "alpha", "sigma", "thr", "K", "blur_ksize", "blur_sigma", "n_ellipses", "t", "shade_ksize"):
            assert np.array_equal(got[k], rec[k]), (name, k)
        assert np.array_equal(got["ellipse"][..., :4], rec["ellipse"][..., :4]), name
        assert TPH.ulps(got["ellipse"][..., 4:], rec["ellipse"][..., 4:], np.float64).max() <= 1, name
        assert TPH.ulps(got["weights"], rec["weights"], np.float32).max() <= 1, name
        alone = np.fromfile(tmp_path / f"{name}1_params.bin", nat.PHOTO_PARAMS_DTYPE)
        assert len(alone) == 1 and alone[0].tobytes() == got[9].tobytes(), name                # an image's values do not depend on its batch


# ---- size queries ------------------------------------------------------------------------------------------------------------------------

def _up(v):
    return (v + 255) // 256 * 256


# Exact restatements (Python integers) of the layouts whose wrapped answers started this suite; None: a shape the restatement does
# not cover.  The header promises the exact number for every size that can be formed, below 2^56 bytes, and 0 beyond: so the answer is
# the restated one, or 0 where that is at or beyond 2^56, and never anything else.  PM_ROWS and the 88-byte pair record: lt_match.h.
PM_ROWS, PAIR_DESC = 16, 88
_c0 = lambda *v: [max(x, 0) for x in v]


def _scratch_ints(k0, k1):
    return 2 * k0 + 2 * k1 + 1 + 2 * (-(-max(k0, 1) // PM_ROWS)) * k1 + 8


def _match_bytes(P, s, k):
    return None if min(P, s, k) < 0 else _up(P * PAIR_DESC) + _up(s * 4) + _up((6 * k + 2 * (s // PM_ROWS + 1) + 9 * P) * 4) + 256


def _distmat_bytes(n0, n1):
    n0, n1 = _c0(n0, n1)
    return 256 + _up(n0 * 4) + _up(max(n1, 1) * 4) + _up(n0 * max(n1, 1) * 4) + _up(_scratch_ints(n0, n1) * 4)


def _points_bytes(n0, n1):
    n0, n1 = _c0(n0, n1)
    return _up(n0 * 1024) + _up(max(n1, 1) * 1024) + _up(n0 * 4) + _up(max(n1, 1) * 4) + _up(_match_bytes(1, n0 * n1, n0 + n1))


def _keypoints_bytes(B, H, W, cap):
    B, H, W, cap = _c0(B, H, W, cap)
    if H * W > 2 ** 31 - 1 or B * H > 2 ** 31 - 1:
        return 0                                                    # refused by the entry point, says the header
    return _up(B * H * (-(-W // 32)) * 4) + _up(B * H * 4) + _up(B * cap * 8) + 256


EXACT = {
    "linetr_match_workspace_bytes": lambda P, s, s2, k: _match_bytes(P, s, k),
    "linetr_match_distmat_workspace_bytes": _distmat_bytes,
    "linetr_pool_distmat_workspace_bytes": lambda k0, k1: _up(_scratch_ints(*_c0(k0, k1)) * 4) + 256,
    "linetr_match_points_workspace_bytes": _points_bytes,
    "linetr_superpoint_keypoints_workspace_bytes": _keypoints_bytes,
    "linetr_sample_descriptors_workspace_bytes": lambda hc, wc, nhwc: None if min(hc, wc) < 0 else 0 if nhwc else _up(hc * wc * 1024),
    "linetr_point_descriptors_workspace_bytes": lambda b, hc, wc, nhwc: 0 if nhwc else _up(max(b, 0) * max(hc, 0) * max(wc, 0) * 1024),
    "linetr_tokenize_workspace_bytes": lambda n, h, w, N: None if min(n, h, w) < 0 else _up(n * (h // 8) * (w // 8) * 1024) + _up(max(N, 1) * 4) + 256,
    "linetr_sp_encoder_workspace_bytes": lambda b, h, w: 0 if not (1 <= b <= 65535 and 8 <= h <= 32768 and 8 <= w <= 32768)
    else _up(b * h * w * 256) + _up(b * (h // 2) * (w // 2) * 256),
    "linetr_match_distmat_f64_workspace_bytes": lambda n0, n1: _up(max(n0, 0) * 8) + _up(max(n0, 0) * 4) + _up(max(n1, 1) * 4) + 256,
}
HOLDABLE = 1 << 56
# dense_is_nhwc: a switch between two layouts, not a count (a channel-last map needs no copy)
FLAG = {"linetr_sample_descriptors_workspace_bytes": 2, "linetr_point_descriptors_workspace_bytes": 3, "linetr_fixed_size_workspace_bytes": 3}


def _parse(path):
    out = []
    for line in path.read_text().splitlines():
        lhs, rhs = line.split(" = ")
        name, *args = lhs.split()
        vals = [int(v) for v in rhs.split()]
        out.append((name, tuple(int(a) for a in args), vals[0], tuple(vals[1:])))
    return out


NEGATIVE_POINTS = ((-1, 5), (5, -1), (-3, -3))
PHOTO_LAYOUT_SHAPES = ((1, 1, 1, 1), (3, 1, 33, 65), (32, 1, 480, 640), (7, 3, 20, 67), (65535, 1, 1, 1))


def write_query_calls(tmp_path):
    calls = [(n, a) for n, a, _ in TW.SIZES] + [("linetr_pair_tail_output_bytes", a) for a, _, _ in TW.TAIL_OUTPUT]
    calls += [("linetr_pair_tail_workspace_bytes", a) for a, _ in TW.TAIL_WORKSPACE]
    for (n0, n1), _ in TW.POINTS:
        calls += [("linetr_match_points_workspace_bytes", (n0, n1)), ("linetr_match_workspace_bytes", (1, n0 * n1, 0, n0 + n1))]
    for n0, n1 in NEGATIVE_POINTS:
        calls += [("linetr_match_points_workspace_bytes", (n0, n1)), ("linetr_match_points_workspace_bytes", (max(n0, 0), max(n1, 0)))]
    calls += [("linetr_photometric_workspace_bytes", s) for s in PHOTO_LAYOUT_SHAPES]
    (tmp_path / "calls.txt").write_text("".join(f"{n} {' '.join(str(v) for v in a)}\n" for n, a in calls))
    return calls


def test_size_queries_pinned_tables_and_edges(asan, tmp_path):
    calls = write_query_calls(tmp_path)
    run_driver(asan, "queries", tmp_path)
    got = _parse(tmp_path / "calls_out.txt")
    assert [(n, a) for n, a, _, _ in got] == [(n, tuple(a)) for n, a in calls]
    it = iter(got)
    # tests/test_workspace_layouts_cpu.py's tables, under its rules
    assert len(TW.SIZES) + len(TW.TAIL_OUTPUT) + len(TW.TAIL_WORKSPACE) + len(TW.POINTS) >= 60
    for name, args, want in TW.SIZES:
        assert next(it)[2] == want, (name, args)
    for args, want, want_offs in TW.TAIL_OUTPUT:
        _, _, v, offs = next(it)
        assert v == want and offs == want_offs, args
    for args, before in TW.TAIL_WORKSPACE:
        v = next(it)[2]
        assert before - TW.TAIL_SLACK < v <= before and (v == before or (args[0] and args[1])), (args, v, before)
    for (n0, n1), before in TW.POINTS:
        v, floor = next(it)[2], 1024 * (n0 + n1) + next(it)[2]
        assert v % 256 == 0 and floor <= v <= before, ((n0, n1), floor, v, before)
    for _ in NEGATIVE_POINTS:
        assert next(it)[2] == next(it)[2]
    for shape in PHOTO_LAYOUT_SHAPES:                                       # tests/test_photometric_cpu.py's restated layout
        assert next(it)[2] == TPH.layout_bytes(*shape), shape
    # the edges: nothing negative, nothing below the base shape's answer once an argument grew, the restated layouts exact
    edges = _parse(tmp_path / "edges_out.txt")
    assert len(edges) > 4000 and len({n for n, _, _, _ in edges}) == 32
    base = {}
    for name, args, v, offs in edges:
        if name not in base:
            base[name] = (args, v)
            assert v > 0, (name, args)
        bargs, bv = base[name]
        assert v >= 0 and all(o >= 0 for o in offs), (name, args, v, offs)
        assert all(a <= b for a, b in zip(offs, offs[1:])) and (not offs or offs[-1] <= v), (name, args, v, offs)
        if all(a >= b for a, b in zip(args, bargs)) and (name not in FLAG or args[FLAG[name]] == bargs[FLAG[name]]):
            assert v == 0 or v >= bv, (name, args, v, bv)
        if name in EXACT:
            exact = EXACT[name](*args)
            if exact is not None:
                assert v == exact or (v == 0 and exact >= HOLDABLE), (name, args, v, exact)
    assert {n for n in EXACT} <= set(base)
    tiles = {l.split()[0]: tuple(int(v) for v in l.split()[1:]) for l in (tmp_path / "tiles_out.txt").read_text().splitlines()}
    assert tiles["linetr_photometric_tile"] == (*PHC.POINT_TILE, *PHC.ROW_TILE, *PHC.COL_TILE, PHC.MAX_RADIUS)
    assert all(v > 0 for t in tiles.values() for v in t) and tiles["linetr_abi_version"] == (6,) and tiles["linetr_pipeline_max_slots"][0] >= 1
    assert set(tiles) == {"linetr_warp_tile", "linetr_photometric_tile", "linetr_detect_tile", "linetr_sp_conv3x3_tile", "linetr_pipeline_max_slots", "linetr_abi_version"}


# ---- refusals and malformed arguments ----------------------------------------------------------------------------------------------------

def _rows(path):
    out = []
    for line in path.read_text().splitlines():
        name, code, *msg = line.split(" ", 2)
        out.append((name, int(code), msg[0] if msg else ""))
    return out


def test_refusals_decided_before_any_device_call(asan, tmp_path):
    run_driver(asan, "refusals", tmp_path)
    rows = _rows(tmp_path / "refusals_out.txt")
    assert len(rows) >= 60 and len({n for n, _, _ in rows}) == len(rows)
    assert all(code in (E_ARG, E_WORKSPACE, E_CAPACITY) and msg for _, code, msg in rows), rows
    short = [(n, c, m) for n, c, m in rows if n.endswith("/short")]
    assert len(short) == 11 and all(c == E_WORKSPACE and "workspace too small" in m for _, c, m in short), short
    assert not any("hip" in m.lower() and "failed" in m for _, _, m in rows), "a refusal that reached the HIP runtime"
    for kind in ("null_", "misaligned_", "/negative", "/short"):
        assert sum(kind in n for n, _, _ in rows) >= 4, kind
    # the photometric, view, detector and training units: the refusals that read the caller's HOST tables, each table an exact-size
    # allocation with the planted entry last
    rows = _rows(tmp_path / "refusals_tables_out.txt")
    assert len(rows) >= 200 and len({n for n, _, _ in rows}) == len(rows)
    assert all(code in (E_ARG, E_WORKSPACE) and msg for _, code, msg in rows), rows
    assert not any("hip" in m.lower() and "failed" in m for _, _, m in rows), "a refusal that reached the HIP runtime"
    by_entry = {}
    for n, c, m in rows:
        by_entry.setdefault(n.split("/")[0], []).append((n.split("/")[1], c, m))
    assert set(by_entry) == {"photometric", "gaussian_blur", "warp_images", "mask_erode", "detect_lines", "detect_debug_labels", "adam_step", "grad_norm",
                             "fixed_size", "val_step", "desc_loss_grad", "gt_assign", "linear_backward", "head_backward", "bn_forward", "bn_backward",
                             "layer_norm_backward", "input_layer_backward", "token_assemble_backward", "linear_forward", "head_forward",
                             "sig_attention_forward", "sig_attention_backward", "cls_pool_train_forward", "cls_pool_train_backward", "layer_norm_forward",
                             "gelu_forward", "gelu_backward", "input_layer_forward", "token_assemble_forward", "dropout_factors", "cls_pool_dropout_forward",
                             "cls_pool_dropout_backward", "layer_norm_dropout_forward", "layer_norm_dropout_backward"}
    takes_workspace = {"photometric", "gaussian_blur", "detect_lines", "detect_debug_labels", "adam_step", "grad_norm", "fixed_size", "val_step", "desc_loss_grad",
                       "gt_assign", "linear_backward", "head_backward", "bn_forward", "bn_backward", "layer_norm_backward", "input_layer_backward",
                       "token_assemble_backward", "sig_attention_backward", "layer_norm_dropout_backward"}
    for entry, cases in by_entry.items():                           # a workspace one byte short wherever one is taken; every message names its entry point
        assert entry not in takes_workspace or any(k == "short" and "too small" in m for k, _, m in cases), entry
        assert all(m.startswith(entry + ":") for _, _, m in cases), (entry, cases)
    # a planted last entry is refused BY NAME: the whole table in front of it was read
    last = {"photometric": "image 4", "gaussian_blur": "image 4", "warp_images": "matrix 4", "adam_step": "tensor 5", "grad_norm": "tensor 5",
            "fixed_size": "image 2"}
    for entry, where in last.items():
        planted = [m for k, _, m in by_entry[entry] if k.startswith("last_")]
        assert planted and all(where in m for m in planted), (entry, planted)


def test_malformed_arguments_are_refused_with_a_code_and_a_message(asan, tmp_path):
    run_driver(asan, "malformed", tmp_path)
    rows = {n: (c, m) for n, c, m in _rows(tmp_path / "malformed_out.txt")}
    assert len(rows) >= 70
    for name in ("batch/offsets_decreasing", "batch/offsets_negative", "batch/offsets_overlapping", "single/negative_lines", "single/records_null",
                 "batch/records_null", "batch/capacity_negative", "batch/threads_negative", "batch/border_negative", "batch/height_negative",
                 "batch/width_negative", "batch/border_negative_with_mask", "batch/token_distance_0", "batch/token_distance_negative",
                 "batch/token_distance_nan", "batch/max_tokens_0", "line/length_inf", "line/octave_inf", "prepare/name_null"):
        assert rows[name][0] == E_ARG and rows[name][1], (name, rows[name])
    for name in ("batch/well_formed", "batch/max_keylines_int_min", "single/max_keylines_int_min", "line/x_nan", "line/x_inf", "line/length_nan",
                 "line/octave_nan"):
        assert rows[name] == (0, ""), (name, rows[name])
    assert rows["pack/end_point_nan"][0] == rows["pack/longer_than_the_segment"][0] == E_ASSERT


# ---- threads -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ("asan", "tsan"))
def test_four_caller_threads_share_the_pool(flavour, request, tmp_path):
    exe = request.getfixturevalue(flavour)
    run_driver(exe, "threads", tmp_path, env={"LINETR_HOST_THREADS": "8"})
    # thread 0's result (its n_threads = 1 answer, which every pooled round equalled byte for byte) against the oracle
    rows = np.fromfile(tmp_path / "thread0_lines.bin", np.float64).reshape(32, 40, 6)
    recs = np.fromfile(tmp_path / "thread0_recs.bin", nat.REC_DTYPE)
    cu_k = np.fromfile(tmp_path / "thread0_cu_k.bin", np.int32)
    cfg = dict(BASE_CFG, max_keylines=512)
    tied = {i for i in range(32) if i % 4 == 0 or i == 1}
    for i in range(32):
        ref = oracle_image(rows[i].copy(), (480, 640), cfg, None, i in tied)
        r = recs[cu_k[i]:cu_k[i + 1]]
        assert len(r) == len(ref["klines"]) and np.array_equal(r["sp"], ref["klines"][:, 0]) and np.array_equal(r["ep"], ref["klines"][:, 1]), i
        assert np.array_equal(r["length"], ref["length_klines"]) and (r["image"] == i).all(), i
    assert cu_k[-1] == len(recs) > 32 * 20
