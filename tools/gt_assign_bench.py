"""Time the native ground-truth line assignment (linetr_gt_assign, csrc/lt_gtassign.h) at cfg4's shape and, where a checkout of the
reference is at hand, the two Python functions it replaces on ONE pair of the same inputs on the same host.
    python tools/gt_assign_bench.py [--pairs 1024] [--lines 250] [--reps 20] [--reference DIR] [--no-write]
Per instance (float32, float64), with and without the match list: median and p10 / p90 of HIP-event times around the call alone
(outputs and workspace allocated once), and the bytes the call must write -- assign [B][n+1][n+1] float32, plus the list and its
ballot words -- over that time, against the HBM figures of DESIGN section 4.  Writes profiles/gt_assign_bench.txt."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.set_grad_enabled(False)
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.3e12


def inputs(B, n, dtype):
    """B seeded homography pairs of n sub-lines a side: four distinct seeds, tiled (the arithmetic does not depend on the values)"""
    import gt_assign_reference as R
    l0, l1, H = R.case(11, min(B, 4), n, n, dtype)
    reps = -(-B // len(l0))
    return tuple(np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B]) for a in (l0, l1, H))


def reference_seconds(ref_dir, l0, l1, H):
    """the reference's builder lines 222-232 for one pair: find_line_matches x 2, calculate_line_overlaps x 2"""
    import types
    import gt_assign_reference as R
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref_dir)
    from dataloaders.utils.util_lines import find_line_matches, calculate_line_overlaps
    p0, p1 = R.project(l0, H), R.project(l1, np.linalg.inv(H))
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        m0 = find_line_matches(l0, p1, 3, 2)
        m1 = find_line_matches(l1, p0, 3, 2).T
        lm = np.array(np.where((m0 > 0) & (m1 > 0))).T
        calculate_line_overlaps(l0, p1, lm)
        calculate_line_overlaps(l1, p0, lm[:, ::-1])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--lines", type=int, default=250)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference", default=None, help="a checkout of the reference (dataloaders/utils/util_lines.py)")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    from linetr_amd import _native as nat
    L = nat.lib()
    B, n = args.pairs, args.lines
    M = int(n * 1.5)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"linetr_gt_assign, {B} pairs x {n} x {n} sub-lines, M = {M}; HIP-event time of the call, median of {args.reps} (p10 p90)"]
    for dtype in (np.float32, np.float64):
        l0, l1, H = inputs(B, n, dtype)
        d0, d1 = torch.from_numpy(l0).cuda(), torch.from_numpy(l1).cuda()
        dH = torch.from_numpy(np.stack([H, np.linalg.inv(H)], axis=1).reshape(B, 2, 9)).cuda()
        assign = torch.empty((B, n + 1, n + 1), dtype=torch.float32, device="cuda")
        lm = torch.empty((B, M, 2), dtype=torch.int32, device="cuda")
        found = torch.empty(B, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L.linetr_gt_assign_workspace_bytes(B, n, n)), dtype=torch.uint8, device="cuda")
        for with_list in (False, True):
            def call():
                nat.check(L.linetr_gt_assign(None, int(dtype == np.float64), d0.data_ptr(), n, d1.data_ptr(), n, dH.data_ptr(), B, None, None,
                                             3.0, 2.0, 0.3, 1, assign.data_ptr(), lm.data_ptr() if with_list else None, M,
                                             found.data_ptr() if with_list else None, None, None, None, None, ws.data_ptr(), ws.numel(), st), L)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            q = np.percentile(times, [50, 10, 90])
            written = B * (n + 1) * (n + 1) * 4 + (B * (n * ((n + 63) // 64) * 8 + M * 8 + 4) if with_list else 0)
            rate = written / (q[0] * 1e-3)
            lines.append(f"{np.dtype(dtype).name:8s} {'assign + list' if with_list else 'assign only  '}  {q[0]:8.3f} ms (p10 {q[1]:.3f} p90 {q[2]:.3f})  "
                         f"writes {written / 1e6:7.1f} MB = {rate / 1e12:5.2f} TB/s: {100 * rate / HBM_MEASURED:5.1f} % of the measured "
                         f"{HBM_MEASURED / 1e12:.1f} TB/s, {100 * rate / HBM_PEAK:5.1f} % of the {HBM_PEAK / 1e12:.1f} TB/s peak"
                         + (f"  (matches per pair: {found.float().mean().item():.1f})" if with_list else ""))
            print(lines[-1], flush=True)
    if args.reference:
        for dtype in (np.float32, np.float64):
            l0, l1, H = inputs(1, n, dtype)
            sec = reference_seconds(args.reference, l0[0], l1[0], H[0])
            lines.append(f"reference, same host CPU, ONE pair of the same inputs, {np.dtype(dtype).name}: {sec:.3f} s "
                         f"(x {B} pairs = {sec * B / 60:.1f} min, extrapolated, not run)")
            print(lines[-1], flush=True)
    else:
        lines.append("reference: no checkout given (--reference DIR): not timed on this host")
        print(lines[-1])
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "gt_assign_bench.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
