"""Measured error and time of the native line segment detector (csrc/lt_linedet.h through linetr_detect_lines) -- writes
profiles/line_detector_errors.txt and profiles/line_detector_bench.txt:

    python tools/line_detector_report.py [--out-dir profiles] [--calls 10]

Errors: every unit case of tests/test_gpu_line_detector.py (tests/line_detector_cases.py) against the NumPy restatement
(tests/line_detector_reference.py) as a number of differing elements or as error / bar, and the restatement's end-point error on the drawn scenes.
Time: B = 32 images of 480 x 640 (the asset pair's two photographs in turn), two octaves, the default settings: the whole call between two
HIP events (median of `calls` calls after warm-up) and every kernel class from the library's own profiler, with the algorithmic bytes each
launch is charged in linetr_det.hip.  No speed bar is set: there is no parent implementation and no OpenCV to race."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import line_detector_cases as LC  # noqa: E402
import line_detector_reference as R  # noqa: E402

STREAM_TBS = 6.3          # the streaming rate DESIGN.md section 4 uses for this device, TB/s
PROTOTYPE_COUNTS = (186, 177)


def asset_images():
    g = np.load(os.path.join(ROOT, "tests", "golden", "asset_pair_images.npz"))
    return [np.squeeze(g[k]) for k in ("gray0", "gray1")]


def errors(eng):
    import test_gpu_line_detector as T
    out = []
    for name, make in sorted(LC.PATTERNS.items()):
        diff = 0
        for H, W in LC.label_sizes() + [(5 * LC.T + 7, 6 * LC.T + 3)]:
            maps = np.stack([make(H, W), LC.random_map(H, W, 3 + H * W), make(H, W)[::-1, ::-1]])
            got = eng.detect_debug_labels(torch.from_numpy(np.ascontiguousarray(maps)).cuda()).cpu().numpy()
            diff += sum(int((got[b] != R.label_regions(maps[b])).sum()) for b in range(3))
        out.append(f"labelling alone, {name:15s} {len(LC.label_sizes()) + 1} sizes from 1 x 1 to {5 * LC.T + 7} x {6 * LC.T + 3}, B = 3   differing labels: {diff}")
    diff = 0
    for H, W in LC.gradient_sizes():
        imgs = np.stack([LC.random_image(H, W, 11 + H + 3 * W), LC.random_image(H, W, 12 + H + 3 * W)])
        for octave in (0, 1):
            got = [t.cpu().numpy() for t in eng.detect_debug_gradient(torch.from_numpy(imgs).cuda(), octave=octave, grad_threshold=200000)]
            for i in range(2):
                q = R.pyramid(imgs[i], 2)[octave]
                if min(q.shape) >= 2:
                    diff += sum(int((a[i] != b).sum()) for a, b in zip(got, R.gradient(q, 200000)))
    out.append(f"m2 and both bucket maps, {len(LC.gradient_sizes())} sizes x 2 octaves x 2 random images   differing elements: {diff}")
    pairs = [p for p in LC.boundary_pairs() if abs(p[0]) + abs(p[1]) <= 255]
    img = LC.planted_gradient_image(pairs)
    got = [t.cpu().numpy()[0] for t in eng.detect_debug_gradient(torch.from_numpy(img).cuda(), n_octave=1, grad_threshold=1)]
    diff = sum(int((a != b).sum()) for a, b in zip(got, R.gradient(img, 1)))
    wrong = sum((int(got[1][1, 8 * j + 1]), int(got[2][1, 8 * j + 1])) != LC.bucket_by_bigint(*p) for j, p in enumerate(pairs))
    out.append(f"{len(pairs)} planted gradient pairs next to the bucket boundaries   differing elements: {diff}   buckets unlike big-integer arithmetic: {wrong}")
    worst_edge = 0.0
    for name in LC.SCENE_NAMES:
        scene = LC.scene(name)
        rows, regions, _ = R.detect(scene, want_debug=True)
        dbg = R.kept_debug_rows(regions)
        r, d, c = T.raw_detect(eng, scene[None], 64)
        n = len(rows)
        err = float((np.abs(r[0, :n, :5] - rows[:, :5]) / np.exp2(rows[:, 5:6])).max()) if int(c.sum()) == n else float("inf")
        edge = LC.edge_errors(rows, LC.scene_edges(name))
        worst_edge = max(worst_edge, float(edge.max()))
        fill = min(abs(x["fill"] / R.DEFAULTS["density"] - 1) for reg in regions for x in reg)
        out.append(f"scene {name:5s} {n:3d} lines (restatement {n}, device {int(c.sum())})   differing debug integers (octave, partition, label, n, moments): "
                   f"{int((d[0, :n] != dbg).sum()) if int(c.sum()) == n else -1}   row error / bar = {err:.3e} / {T.ROW_BAR:.0e} px = {err / T.ROW_BAR:.2e}"
                   f"   end-point error of the worst edge {edge.max():.3f} px / bar {1.5 * LC.EDGE_ERROR_MEASURED:.3f} px   closest region to the density threshold {fill:.2e}")
    out.append(f"worst end-point error over the scenes: {worst_edge:.3f} px (tests/line_detector_cases.py EDGE_ERROR_MEASURED = {LC.EDGE_ERROR_MEASURED}; the tests' bar "
               f"is 1.5 x that = {1.5 * LC.EDGE_ERROR_MEASURED:.3f} px, ceiling {LC.EDGE_BAR_CEILING} px)")
    base = LC.scene("bars")
    got, want = R.detect(LC.shifted(base)), R.detect(base)
    want[:, [0, 2]] += LC.SHIFT[0]
    want[:, [1, 3]] += LC.SHIFT[1]
    out.append(f"restatement on the scene shifted by {LC.SHIFT}: max row deviation {np.abs(got - want).max():.3e} px / bar 1e-9")
    return ("# every unit case of tests/test_gpu_line_detector.py against the NumPy restatement (tests/line_detector_reference.py); written by\n"
            "# tools/line_detector_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(out) + "\n")


def bench(eng, calls):
    B, (H, W) = 32, (480, 640)
    photos = asset_images()
    batch = torch.from_numpy(np.stack([photos[b % 2] for b in range(B)])).cuda()
    rows, offsets = eng.detect_lines(batch)
    counts = np.diff(offsets)
    want = [len(R.detect(p)) for p in photos]
    eng.set_profiling(True)
    for _ in range(2):
        eng.detect_lines(batch)
    before = {e["name"]: e for e in eng.get_profile()}
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.detect_lines(batch)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    after = {e["name"]: e for e in eng.get_profile()}
    eng.set_profiling(False)
    lines = [f"B = {B} images of {H} x {W} uint8 (the asset pair's two photographs in turn), two octaves, default settings; workspace "
             f"{eng._L.linetr_detect_lines_workspace_bytes(B, H, W, 2) / 1e6:.0f} MB",
             f"lines on the asset pair: {counts[0]} / {counts[1]} (restatement {want[0]} / {want[1]}, the NumPy + scipy prototype {PROTOTYPE_COUNTS[0]} / "
             f"{PROTOTYPE_COUNTS[1]}); {int((rows[:, 4] * 2.0 ** rows[:, 5] > 16).sum()) // (B // 2)} of a pair's are longer than 16 px",
             f"Engine.detect_lines, whole call with its synchronisation and the copy of the rows: {np.median(times):.3f} ms  [{min(times):.3f} .. {max(times):.3f}]"
             " (profiler events on)", "per kernel class, per call (library profiler; algorithmic bytes as charged in linetr_det.hip):"]
    total_ms = 0.0
    for name, e in after.items():
        if not name.startswith("det_"):
            continue
        p = before.get(name, dict(calls=0, ms=0.0, bytes=0.0))
        if e["calls"] < p["calls"]:
            p = dict(calls=0, ms=0.0, bytes=0.0)
        n = max(e["calls"] - p["calls"], 1)
        ms, byts = (e["ms"] - p["ms"]) / calls, (e["bytes"] - p["bytes"]) / calls
        total_ms += ms
        rate = byts / (ms * 1e-3) / 1e12 if ms > 0 and byts > 0 else 0.0
        lines.append(f"  {name:18s} {n // calls:2d} launches  {ms:8.4f} ms   {byts / 1e6:8.1f} MB   {rate:5.2f} TB/s = {100 * rate / STREAM_TBS:5.1f} % of {STREAM_TBS} TB/s")
    lines.append(f"  sum of the kernels {total_ms:.4f} ms")
    return (f"# the native line segment detector at the dataset builder's size; ms between two HIP events, median of {calls} calls after warm-up (min .. max in\n"
            f"# brackets); written by tools/line_detector_report.py on {torch.cuda.get_device_name(0)}.  No speed bar: no parent implementation and no OpenCV to race.\n"
            + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    from workloads import synth
    eng = Engine(synth.calibrated_state_dict(), "cuda:0")          # a handle: the per-kernel profiler lives there
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("line_detector_errors.txt", lambda: errors(eng)), ("line_detector_bench.txt", lambda: bench(eng, args.calls))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
