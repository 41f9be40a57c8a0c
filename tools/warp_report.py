"""Measured error and time of the homography views (csrc/lt_warp.h through linetr_warp_images / linetr_mask_erode) -- writes
profiles/warp_errors.txt and profiles/warp_bench.txt:

    python tools/warp_report.py [--out-dir profiles] [--calls 20]

Errors: every unit case of tests/test_gpu_warp.py (tests/warp_cases.py, tests/golden/warp.npz) as error / bar or as a count of
differing elements.
Time: B = 32 images of 480 x 640 at C = 1 and C = 3.  The native warp with its valid mask, the native erosion (radius 2), and the
reference's torch recipe (dataloaders/utils/utils.py:317-351, 677-704: meshgrid + matmul + grid_sample for the image + grid_sample of
ones in 'nearest' mode for the mask, its host erosion replaced by max_pool2d on the negated mask) on the same device in the same
process, alternating call by call; each call between two HIP events, the median of `calls` calls after warm-up.  The recipe is
given its source coordinates ONCE for both grid_sample calls (the reference computes them twice).  Every call works on the next of
several buffer sets that together exceed the 256 MB Infinity Cache, so the rates are HBM rates.  No time is fixed in advance; the one
bar is that the native warp + mask is not slower than the recipe it replaces."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import warp_cases as WC  # noqa: E402
import warp_reference as R  # noqa: E402
from workloads import synth  # noqa: E402

HW = (480, 640)
STREAM_TBS = 6.3          # the streaming rate DESIGN.md section 4 uses for this device, TB/s
CACHE_BYTES = 256 << 20


def errors(eng):
    import test_gpu_warp as T
    g = R.fixture()
    out = []
    for H, W in WC.SHAPES:
        img1, img3 = WC.int_images(100 + H, 1, 1, H, W), WC.int_images(200 + W, 3, 3, H, W)
        diff = 0
        for kind in WC.KINDS:
            m, want = WC.exact_case(kind, img1[0])
            for mode in ("bilinear",) + (("nearest",) if kind != "half" else ()):
                got, valid = T.run_warp(eng, img1, m[None], mode)
                diff += int((got[0] != want).sum()) + int((valid[0] != R.valid_mask(m, H, W)).sum())
        for rotation in range(4):
            mats, want, _ = WC.exact_batch(rotation, img3)
            got, valid = T.run_warp(eng, img3, mats, "bilinear", shift=rotation % 2)
            diff += int((got != want).sum()) + int((valid != np.stack([R.valid_mask(m, H, W) for m in mats])).sum())
        out.append(f"exact geometries {H:3d} x {W:3d} (identity, translation, 180 degrees, half pixel; C = 1 and B = C = 3)   differing elements: {diff}")
    for c, (B, C, H, W) in enumerate(R.SHAPES):
        pix = R.normalised_to_pixel(g[f"mat_{c}"], H, W)
        rnd = (np.random.RandomState(300 + c).standard_normal((B, C, H, W)) * 50).astype(np.float32)
        got, valid = T.run_warp(eng, rnd, pix, "bilinear")
        got_n, _ = T.run_warp(eng, rnd, pix, "nearest")
        ratio, d_near, d_valid, n_ex = 0.0, 0, 0, 0
        for b in range(B):
            want, max_tap = R.warp(rnd[b], pix[b], "bilinear")
            err = np.abs(got[b].astype(np.float64) - want)
            ratio = max(ratio, float((err / np.maximum(R.BILINEAR_BAR * max_tap[None], 1e-300)).max()))
            d_near += int((got_n[b] != R.warp(rnd[b], pix[b], "nearest")[0].astype(np.float32)).sum())
            d_valid += int((valid[b] != R.valid_mask(pix[b], H, W)).sum())
            n_ex += int(R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_F64).sum())
        out.append(f"fixture homographies {B} x {C} x {H:3d} x {W:3d} vs float64    bilinear error / ({R.BILINEAR_BAR:g} max|tap|) = {ratio:.3f}   nearest differing: "
                   f"{d_near}   valid differing: {d_valid}   pixels within {R.EXCUSE_F64:g} px of a rounding boundary: {n_ex}")
        img = g[f"img_{c}"]
        got, valid = T.run_warp(eng, img, pix, "bilinear")
        got_n, _ = T.run_warp(eng, img, pix, "nearest")
        ref_dev = float(g[f"ref_dev_{c}"])
        ratio, d_near, d_valid, n_ex = 0.0, 0, 0, 0
        for b in range(B):
            _, max_tap = R.warp(img[b], pix[b], "bilinear")
            err = np.abs(got[b].astype(np.float64) - g[f"bilinear_{c}"][b])
            ratio = max(ratio, float((err / (ref_dev + R.BILINEAR_BAR * max_tap[None])).max()))
            ex = R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_REF)
            d_near += int(((got_n[b] != g[f"nearest_{c}"][b]) & ~ex[None]).sum())
            d_valid += int(((valid[b] != g[f"mask_{c}"][b]) & ~ex).sum())
            n_ex += int(ex.sum())
        out.append(f"fixture homographies {B} x {C} x {H:3d} x {W:3d} vs the reference  bilinear error / (ref_dev {ref_dev:.2e} + bar) = {ratio:.3f}   non-excused "
                   f"differing: nearest {d_near}, valid {d_valid}   excused ({R.EXCUSE_REF:g} px): {n_ex} of {B * H * W} = {100.0 * n_ex / (B * H * W):.2f} % (cap 2 %)")
    names, mats = WC.degenerate_matrices()
    H, W = 33, 67
    img = WC.int_images(7, len(mats), 1, H, W)
    for mode in ("bilinear", "nearest"):
        got, valid = T.run_warp(eng, img, mats, mode)
        for b, name in enumerate(names):
            want, max_tap = R.warp(img[b], mats[b], mode)
            ex = R.near_rounding_boundary(mats[b], H, W, R.EXCUSE_F64) if name == "horizon" else np.zeros((H, W), bool)
            err = np.where(ex[None], 0.0, np.abs(got[b] - want))
            ratio = float((err / np.maximum(R.BILINEAR_BAR * max_tap[None], 1e-300)).max())
            out.append(f"degenerate {name:8s} {mode:8s}  finite: {bool(np.isfinite(got[b]).all())}   valid pixels {int(valid[b].sum()):4d} (restatement "
                       f"{int(R.valid_mask(mats[b], H, W).sum()):4d})   error / bar = {ratio:.3f}   non-zero where the restatement is zero: {int(((got[b] != 0) & (want == 0) & ~ex[None]).sum())}")
    for H, W in WC.EROSION_SHAPES:
        masks = WC.erosion_masks(40 + H, 3, H, W)
        src = torch.from_numpy(masks).cuda()
        diff = {r: int((eng.erode_mask(src, r).cpu().numpy() != R.erode(masks, r)).sum()) for r in WC.EROSION_RADII}
        out.append(f"erosion 3 x {H:3d} x {W:3d}   differing elements at radius " + ", ".join(f"{r}: {d}" for r, d in diff.items()))
    return ("# every unit case of tests/test_gpu_warp.py: exact cases and the erosion as the number of differing elements, the float64 restatement\n"
            "# (tests/warp_reference.py) and the real reference's outputs (tests/golden/warp.npz) as error / bar; written by tools/warp_report.py on "
            + torch.cuda.get_device_name(0) + "\n" + "\n".join(out) + "\n")


def torch_recipe(img, mat, ones, radius):
    """inv_warp_image_batch + compute_valid_mask of the reference on the device, coordinates computed once"""
    B, _, H, W = img.shape
    dev = img.device
    cells = torch.stack(torch.meshgrid(torch.linspace(-1, 1, W, device=dev), torch.linspace(-1, 1, H, device=dev), indexing="ij"), dim=2)
    cells = cells.transpose(0, 1).contiguous().view(-1, 2)
    pts = torch.cat((cells, torch.ones((cells.shape[0], 1), device=dev)), dim=1)
    wp = (mat.view(B * 3, 3) @ pts.transpose(0, 1)).view(B, 3, -1).transpose(2, 1)
    coords = (wp[:, :, :2] / wp[:, :, 2:]).view(B, H, W, 2)
    warped = F.grid_sample(img, coords, mode="bilinear", align_corners=True)
    mask = F.grid_sample(ones, coords, mode="nearest", align_corners=True)
    return warped, -F.max_pool2d(-mask, 2 * radius + 1, 1, radius)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def bench(eng, calls):
    from linetr_amd import homography as HG
    H, W = HW
    B, radius = 32, 2
    rs = np.random.RandomState(5)
    norm = np.stack([np.linalg.inv(synth.sample_homography(rs, **synth.HOMOGRAPHY_PARAMS)) for _ in range(B)])
    pix = HG.normalised_to_pixel(norm, H, W)
    mat_dev = torch.from_numpy(norm.astype(np.float32)).cuda()
    lines = []
    for C in (1, 3):
        algo = float(B * H * W * (8 * C + 1))
        n_sets = int(CACHE_BYTES // algo) + 2
        g = torch.Generator(device="cuda").manual_seed(C)
        sets = [dict(img=torch.rand((B, C, H, W), generator=g, device="cuda"), out=torch.empty((B, C, H, W), device="cuda"),
                     valid=torch.empty((B, H, W), dtype=torch.uint8, device="cuda"), eroded=torch.empty((B, H, W), dtype=torch.uint8, device="cuda"))
                for _ in range(n_sets)]
        ones = torch.ones((B, 1, H, W), device="cuda")
        sides = {"warp": lambda s: eng.warp_images(s["img"], pix, return_valid=True, out=s["out"], out_valid=s["valid"]),
                 "erode": lambda s: eng.erode_mask(s["valid"], radius, out=s["eroded"]),
                 "torch": lambda s: torch_recipe(s["img"], mat_dev, ones, radius)}
        # the two paths compute the same view (the recipe's coordinates are float32)
        a = sides["warp"](sets[0])[0]
        sides["erode"](sets[0])
        b, mb = sides["torch"](sets[0])
        dev_img = float((a - b).abs().max())
        dev_mask = float((sets[0]["eroded"].float() != mb[:, 0]).float().mean())
        events = {k: [] for k in sides}
        for i in range(3 + calls):
            for k, fn in sides.items():
                s = sets[i % n_sets]
                ev = timed(lambda: fn(s))
                if i >= 3:
                    events[k].append(ev)
        torch.cuda.synchronize()
        ms = {k: float(np.median([x.elapsed_time(y) for x, y in v])) for k, v in events.items()}
        spread = {k: (min(x.elapsed_time(y) for x, y in v), max(x.elapsed_time(y) for x, y in v)) for k, v in events.items()}
        frac = algo / (ms["warp"] * 1e-3) / (STREAM_TBS * 1e12)
        verdict = "the native warp + mask is not slower" if ms["warp"] <= ms["torch"] else "the native warp + mask IS SLOWER than the recipe"
        lines += [f"C = {C}: B = {B} images of {C} x {H} x {W}, {n_sets} buffer sets in turn ({n_sets * algo / 1e6:.0f} MB > the Infinity Cache)",
                  f"  linetr_warp_images, bilinear, with the valid mask      {ms['warp']:8.4f} ms  [{spread['warp'][0]:.4f} .. {spread['warp'][1]:.4f}]",
                  f"  linetr_mask_erode, radius {radius}                           {ms['erode']:8.4f} ms  [{spread['erode'][0]:.4f} .. {spread['erode'][1]:.4f}]",
                  f"  torch recipe (meshgrid + matmul + 2 grid_sample + max_pool2d)  {ms['torch']:8.4f} ms  [{spread['torch'][0]:.4f} .. {spread['torch'][1]:.4f}]"
                  f"   recipe / native warp + mask {ms['torch'] / ms['warp']:.2f}, recipe / (native warp + mask + erosion) {ms['torch'] / (ms['warp'] + ms['erode']):.2f}: {verdict}",
                  f"  algorithmic bytes of the warp (input once, output once, mask once): {algo / 1e6:.1f} MB = {algo / (STREAM_TBS * 1e12) * 1e3:.4f} ms at {STREAM_TBS} TB/s"
                  f" -> achieved {algo / (ms['warp'] * 1e-3) / 1e12:.2f} TB/s = {100 * frac:.1f} % of it; the erosion moves {2.0 * B * H * W / 1e6:.1f} MB"
                  f" -> {2.0 * B * H * W / (ms['erode'] * 1e-3) / 1e12:.2f} TB/s",
                  f"  native against the recipe on the same batch: max |image difference| {dev_img:.2e} (float32 coordinates there), eroded masks differ on {100 * dev_mask:.3f} % of the pixels"]
        del sets
    return (f"# homography views at the dataset builder's size; ms per call between two HIP events, median of {calls} calls after 3 warm-up calls, the three\n"
            "# sides alternating call by call (min .. max in brackets); same GPU, same process; homographies drawn with workloads.synth.sample_homography\n"
            f"# (HOMOGRAPHY_PARAMS); written by tools/warp_report.py on {torch.cuda.get_device_name(0)}\n" + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("warp_errors.txt", lambda: errors(eng)), ("warp_bench.txt", lambda: bench(eng, args.calls))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
