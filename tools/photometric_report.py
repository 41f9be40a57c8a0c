"""Measured error and time of the photometric augmentation (csrc/lt_photometric.h through linetr_photometric / linetr_gaussian_blur) -- writes
profiles/photometric_errors.txt and profiles/photometric_bench.txt:

    python tools/photometric_report.py [--out-dir profiles] [--calls 20] [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/photometric_report.py --chain-only

Errors: every unit case of tests/test_gpu_photometric.py (tests/photometric_cases.py) as a count of differing elements or as error / bar,
with the excused share of what is quantised behind a float32 sum.
Time: B = 32 images of 480 x 640 with parameters drawn from the reference's homography.yaml (tests/golden/homography_photometric.json) by
the host sampler.  The native chain, the chain at the shade's largest kernel (ksize 351), the Gaussian blur alone, and the same chain
written in plain torch on the same device (randn / rand / F.conv2d), alternating call by call; each call between two HIP events, the
median of `calls` calls after warm-up.  Every call works on the next of several buffer sets that together exceed the 256 MB Infinity
Cache.  The time of each launch comes from a kernel trace taken in a run of its own (--chain-only under rocprofv3) and is read from
--kernel-stats; without it the file says so.  No time or share is fixed in advance."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import photometric_cases as PC  # noqa: E402
import photometric_reference as R  # noqa: E402

HW, B = (480, 640), 32
STREAM_TBS = 6.3          # the streaming rate DESIGN.md section 4 uses for this device, TB/s
CACHE_BYTES = 256 << 20
BYTES_PER_PIXEL = 24      # point kernel: read 4, write 4; row pass: write 4 (the mask is never read); column pass: read 4 + 4, write 4


def yaml_config():
    with open(os.path.join(ROOT, "tests", "golden", "homography_photometric.json")) as fh:
        return json.load(fh)


def errors(eng):
    import test_gpu_photometric as T
    out = []
    for H, W in PC.POINT_SHAPES:
        diff = 0
        for name in (*PC.EXACT, *PC.NOISE):
            c = PC.point_case(name, H, W)
            for shift in (0, 1):
                diff += int((T.run_photo(eng, c["x"][None, None], [c["p"]], shift=shift)[0, 0] != T.f32(c["ref"]["out"])).sum())
        out.append(f"exact stages and noise {H:3d} x {W:3d} ({len(PC.EXACT)} exact cases, {len(PC.NOISE)} noise cases, aligned and one float off)   differing elements: {diff}")
    for H, W in PC.POINT_SHAPES:
        parts = []
        for name in PC.MOTION_REAL:
            c = PC.point_case(name, H, W)
            got = T.run_photo(eng, c["x"][None, None], [c["p"]])[0, 0]
            d64 = int((T.levels_of(got) != R.quantise(c["ref"]["pre_motion"])).sum())
            d32 = int((got != T.f32(c["ref"]["out"])).sum())
            parts.append(f"{name}: {d64} differ from float64 ({int(c['excused'].sum())} excused), {d32} from the float32 order")
        out.append(f"motion blur, real kernels {H:3d} x {W:3d} ({H * W} pixels)   " + "; ".join(parts))
    for H, W in PC.BLUR_SHAPES:
        parts = []
        for ksize, sigma in PC.BLUR_KSIZES:
            c = PC.blur_case(H, W, ksize, sigma, False)
            err = np.abs(T.run_blur(eng, c["x"][None, None], ksize, sigma, False)[0, 0].astype(np.float64) - c["ref"])
            cq = PC.blur_case(H, W, ksize, sigma, True)
            dq = int((T.run_blur(eng, cq["x"][None, None], ksize, sigma, True)[0, 0] != R.quantise(cq["ref"])).sum())
            ratio = f"{(err / (c['bar'] + R.U24 * np.abs(c['ref']))).max():.3f}" if ksize > 1 else f"exact ({int((err != 0).sum())} differ)"
            parts.append(f"ksize {ksize}: {ratio}, quantised {dq} differ ({int(cq['excused'].sum())} excused)")
        out.append(f"Gaussian blur alone {H:3d} x {W:3d} ({H * W} pixels)   error / bar " + "; ".join(parts))
    for H, W in PC.SHADE_SHAPES:
        parts = []
        for i, (kind, t, ksize, q) in enumerate(PC.SHADE):
            c = PC.shade_case(H, W, i)
            got = T.run_photo(eng, c["x"][None, None], [c["p"]], q=bool(q), shift=i % 2)[0, 0]
            if q:
                parts.append(f"{kind} t={t} k={ksize} floor: {int((T.levels_of(got) != np.floor(c['ref']['shaded'])).sum())} differ ({int(c['excused'].sum())} excused)")
            else:
                err = np.abs(got.astype(np.float64) - c["ref"]["out"])
                parts.append(f"{kind} t={t} k={ksize}: {(err / np.maximum(PC.shade_out_bar(c['ref'], c['bar']), 1e-300)).max():.3f}")
        out.append(f"shade {H:3d} x {W:3d} ({H * W} pixels)   error / bar " + "; ".join(parts))
    return ("# every unit case of tests/test_gpu_photometric.py against the NumPy restatement (tests/photometric_reference.py): exact cases as the number of\n"
            "# differing elements, float32 sums as error / bar (bars: tests/photometric_cases.py), quantised results behind a float32 sum as differing\n"
            f"# and excused pixels (cap {100 * PC.SHARE:g} % of a case); written by tools/photometric_report.py on " + torch.cuda.get_device_name(0) + "\n"
            + "\n".join(out) + "\n")


def gauss_kernel(ksize, dev):
    return torch.from_numpy(R.gaussian_taps(ksize, 0.0)).to(dev)


def torch_chain(x, prm, masks, taps, gen):
    """the same chain in plain torch on the device: per-batch tensors of the drawn values, randn / rand for the per-pixel randomness,
    F.conv2d with reflect padding for the motion kernel and for the two passes of the mask's blur (one ksize for the batch)"""
    q = lambda v: v.clamp(0, 255).round()
    lev = q(255.0 * x)
    lev = q(lev + prm["d"])
    lev = q(127.0 + prm["alpha"] * (lev - 127.0))
    lev = q(lev + prm["sigma"] * torch.randn(x.shape, device=x.device, generator=gen))
    hit = torch.rand(x.shape, device=x.device, generator=gen) < prm["p"]
    lev = torch.where(hit, torch.where(torch.rand(x.shape, device=x.device, generator=gen) < 0.5, 255.0, 0.0), lev)
    Bn = x.shape[0]
    mo = F.conv2d(F.pad(lev.view(1, Bn, *x.shape[2:]), (1, 1, 1, 1), mode="reflect"), prm["w3"], groups=Bn).view_as(lev)
    lev = torch.where(prm["motion"], q(mo), lev)
    r = taps.numel() // 2
    m = F.conv2d(F.pad(masks, (r, r, 0, 0), mode="reflect"), taps.view(1, 1, 1, -1))
    m = F.conv2d(F.pad(m, (0, 0, r, r), mode="reflect"), taps.view(1, 1, -1, 1))
    return (lev * (1.0 - prm["t"] * m / 255.0)).clamp(0, 255).floor() / 255.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def bench_setup(eng):
    from linetr_amd import _native as nat
    H, W = HW
    params = eng.photometric_params(yaml_config(), B, H, W, seed=7)
    big = params.copy()
    big["shade_ksize"] = R.MAX_KSIZE
    algo = float(B * H * W * BYTES_PER_PIXEL)
    n_sets = int(CACHE_BYTES // (B * H * W * 8)) + 2
    g = torch.Generator(device="cuda").manual_seed(1)
    sets = [dict(img=torch.rand((B, 1, H, W), generator=g, device="cuda"), out=torch.empty((B, 1, H, W), device="cuda")) for _ in range(n_sets)]
    return nat, params, big, algo, n_sets, sets


def chain_only(eng, calls):
    """the native chain alone, for a kernel trace"""
    _, params, big, _, n_sets, sets = bench_setup(eng)
    for i in range(calls):
        s = sets[i % n_sets]
        eng.photometric(s["img"], params, 7, quantise_out=True, out=s["out"])
    torch.cuda.synchronize()


def kernel_stats(path):
    """{kernel name: (calls, average microseconds)} of the photometric kernels from rocprofv3's *kernel_stats.csv under `path`"""
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                if "photo_" in name:
                    out[name] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3)
    return out


def bench(eng, calls, stats_path):
    nat, params, big, algo, n_sets, sets = bench_setup(eng)
    H, W = HW
    dev = sets[0]["img"].device
    col = lambda k, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(params[k])).to(dev).to(dt).view(B, 1, 1, 1)
    motion = (params["stages"] & R.MOTION) != 0
    w3 = np.zeros((B, 1, 3, 3), np.float32)
    w3[:, 0, 1, 1] = 1.0
    w3[motion, 0] = params["weights"][motion, :9].reshape(-1, 3, 3)
    prm = dict(d=col("d"), alpha=col("alpha"), sigma=col("sigma"), p=(col("thr", torch.float64) / 4294967296.0).float(), t=col("t"),
               w3=torch.from_numpy(w3).to(dev), motion=torch.from_numpy(motion).to(dev).view(B, 1, 1, 1))
    masks = torch.from_numpy(np.stack([R.ellipse_mask(params["ellipse"][b][:params["n_ellipses"][b]], H, W) for b in range(B)]).astype(np.float32)).to(dev)[:, None]
    k_mid = int(np.median(params["shade_ksize"])) | 1
    taps = gauss_kernel(k_mid, dev)
    gen = torch.Generator(device="cuda").manual_seed(2)
    ks = np.full(B, k_mid, np.int32)
    sides = {"chain": lambda s: eng.photometric(s["img"], params, 7, quantise_out=True, out=s["out"]),
             "chain351": lambda s: eng.photometric(s["img"], big, 7, quantise_out=True, out=s["out"]),
             "blur": lambda s: eng.gaussian_blur(s["img"], ks, 0.0, out=s["out"]),
             "blur351": lambda s: eng.gaussian_blur(s["img"], R.MAX_KSIZE, 0.0, out=s["out"]),
             "torch": lambda s: torch_chain(s["img"], prm, masks, taps, gen)}
    # the same computation: without the two random stages and with one shade ksize the two chains must agree up to rounding boundaries
    det = params.copy()
    det["stages"] &= ~(R.NOISE | R.IMPULSE)
    det["shade_ksize"] = k_mid
    a = eng.photometric(sets[0]["img"], det, 7, quantise_out=True)
    b = torch_chain(sets[0]["img"], {**prm, "sigma": torch.zeros_like(prm["sigma"]), "p": torch.zeros_like(prm["p"])}, masks, taps, gen)
    agree = (float(((a - b).abs() <= 0.5 / 255).float().mean()), float(((a - b).abs() <= 1.5 / 255).float().mean()), float((a - b).abs().max()) * 255)
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
    share = lambda k, nbytes: f"{nbytes / (ms[k] * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms[k] * 1e-3) / (STREAM_TBS * 1e12):.1f} % of {STREAM_TBS} TB/s"
    row = lambda label, k: f"  {label:66s} {ms[k]:8.4f} ms  [{spread[k][0]:.4f} .. {spread[k][1]:.4f}]"
    blur_bytes = float(B * H * W * 16)
    lines = [f"B = {B} images of 1 x {H} x {W}, {n_sets} buffer sets in turn ({n_sets * B * H * W * 8 / 1e6:.0f} MB of inputs and outputs > the Infinity Cache)",
             f"parameters: linetr_photometric_sample on the yaml, seed 7: motion blur on {int(motion.sum())} of {B} images, shade ksize "
             f"{int(params['shade_ksize'].min())} .. {int(params['shade_ksize'].max())}, 20 ellipses per image; {-(-B // PC.CARRY)} carrier launches + 3 kernels per call",
             row("linetr_photometric, the yaml's chain, quantise_out", "chain"),
             row("linetr_photometric, the same with every shade ksize = 351", "chain351"),
             row(f"linetr_gaussian_blur alone, ksize {k_mid} (2 launches + carriers)", "blur"),
             row("linetr_gaussian_blur alone, ksize 351", "blur351"),
             row(f"the chain in plain torch (randn, rand, conv2d; one shade ksize {k_mid}, masks given)", "torch")
             + f"   torch / native = {ms['torch'] / ms['chain']:.2f}",
             f"algorithmic bytes of the chain, {BYTES_PER_PIXEL} B per pixel (point kernel 4 + 4, row pass 0 + 4, column pass 4 + 4 + 4): {algo / 1e6:.1f} MB = "
             f"{algo / (STREAM_TBS * 1e12) * 1e3:.4f} ms at {STREAM_TBS} TB/s -> the chain achieves {share('chain', algo)}; at ksize 351 {share('chain351', algo)}",
             f"the blur alone moves 16 B per pixel ({blur_bytes / 1e6:.1f} MB): {share('blur', blur_bytes)}; at ksize 351 {share('blur351', blur_bytes)}",
             f"native against torch without the two random stages, one shade ksize: {100 * agree[0]:.3f} % of the pixels equal, {100 * agree[1]:.3f} % within one "
             f"level, largest difference {agree[2]:.1f} levels (float32 levels and another summation order there)",
             "(the torch chain is given its masks; the native chain builds them in the row pass.  The torch chain takes one shade ksize for the batch.)"]
    if stats_path:
        st = kernel_stats(stats_path)
        lines.append("per launch, from a kernel trace of the yaml's native chain alone (rocprofv3 --kernel-trace --stats, a run of its own; average microseconds [min .. max], calls):")
        for name, (n, avg, lo, hi) in sorted(st.items()):
            lines.append(f"  {name[:110]:110s} {avg:9.1f} us  [{lo:.1f} .. {hi:.1f}]  x {n}")
        lines.append(f"  at ksize 351 the chain takes {ms['chain351'] - ms['chain']:.4f} ms more than at the yaml's sizes: the two passes of the mask's blur are all that differs")
    else:
        lines.append("per launch: not measured (take a kernel trace of --chain-only and pass --kernel-stats)")
    return (f"# photometric augmentation at the dataset builder's size; ms per call between two HIP events, median of {calls} calls after 3 warm-up calls, the\n"
            f"# sides alternating call by call (min .. max in brackets); same GPU, same process; written by tools/photometric_report.py on {torch.cuda.get_device_name(0)}\n"
            + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--chain-only", action="store_true")
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    if args.chain_only:
        chain_only(eng, args.calls)
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("photometric_errors.txt", lambda: errors(eng)), ("photometric_bench.txt", lambda: bench(eng, args.calls, args.kernel_stats))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
