"""Time SuperPoint's key-point branch: the native call (Engine.superpoint_keypoints) against the per-image torch path it replaces
(FusedHeadSuperPoint._keypoints with torch helpers), alternating on identical seeded maps in one process.
    python tools/keypoints_bench.py [--reps 20] [--sizes 128x480x640,2x480x640,16x960x1280] [--no-write]
Per workload (each with max_keypoints -1 and 1024): median and p10 / p90 of HIP-event times around a call that ends in a
synchronise, the host waits per batch (Event.synchronize / Tensor.cpu / nonzero counted), and for the native side the compulsory
bytes -- score map once, bit mask, 4 taps x 1 KiB + 1 KiB per key point -- over 6.3 TB/s: the HBM floor of the CALL, not a kernel's
share of peak.  Also prints the descriptors' largest error against the two reference fixtures.  Writes profiles/keypoints_bench.txt
and profiles/keypoints_errors.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_grad_enabled(False)
HBM = 6.3e12


class Helpers:
    """torch restatement of the branch's helpers (what the wrapped module supplies)"""

    @staticmethod
    def simple_nms(scores, r):
        pool = lambda t: torch.nn.functional.max_pool2d(t, 2 * r + 1, 1, r)
        keep = scores == pool(scores)
        for _ in range(2):
            near = pool(keep.float()) > 0
            rest = scores.masked_fill(near, 0.0)
            keep = keep | ((rest == pool(rest)) & ~near)
        return scores * keep

    @staticmethod
    def remove_borders(rc, val, b, h, w):
        ok = (rc[:, 0] >= b) & (rc[:, 0] < h - b) & (rc[:, 1] >= b) & (rc[:, 1] < w - b)
        return rc[ok], val[ok]

    @staticmethod
    def top_k_keypoints(rc, val, n):
        if n >= rc.shape[0]:
            return rc, val
        best = torch.topk(val, n).indices
        return rc[best], val[best]

    @staticmethod
    def sample_descriptors(xy, dense, cell=8):
        bsz, ch, hc, wc = dense.shape
        span = torch.tensor([wc * cell - cell / 2 - 0.5, hc * cell - cell / 2 - 0.5], device=xy.device, dtype=xy.dtype)
        grid = ((xy - cell / 2 + 0.5) / span) * 2 - 1
        got = torch.nn.functional.grid_sample(dense, grid.view(bsz, 1, -1, 2), mode="bilinear", align_corners=False)
        return torch.nn.functional.normalize(got.reshape(bsz, ch, -1), p=2, dim=1)


class WaitCounter:
    """counts the calls that make the host wait for the device"""

    def __init__(self):
        self.n = 0

    def __enter__(self):
        self.saved = (torch.cuda.Event.synchronize, torch.Tensor.cpu, torch.nonzero)
        ev, cpu, nz = self.saved

        def bump(fn):
            def wrapped(*a, **k):
                self.n += 1
                return fn(*a, **k)
            return wrapped
        torch.cuda.Event.synchronize, torch.Tensor.cpu, torch.nonzero = bump(ev), bump(cpu), bump(nz)
        return self

    def __exit__(self, *exc):
        torch.cuda.Event.synchronize, torch.Tensor.cpu, torch.nonzero = self.saved


def parse_sizes(text):
    return [tuple(int(v) for v in item.split("x")) for item in text.split(",")]


def fixture_errors(eng, out):
    gold = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(gold, "superpoint_heads.npz"))
    _, _, d = eng.superpoint_keypoints(torch.from_numpy(g["dense_score"]).cuda(), torch.from_numpy(g["dense_descriptor"]).cuda(),
                                       dense_layout="nchw")
    out.append("superpoint_heads.npz  descriptor max-abs error  " + "  ".join(
        f"{np.abs(d[b].cpu().numpy() - g[f'descriptors{b}']).max():.3e}" for b in range(2)))
    g = np.load(os.path.join(gold, "asset_pair.npz"))
    _, _, d = eng.superpoint_keypoints(torch.from_numpy(np.concatenate([g["dense_score0"], g["dense_score1"]])).cuda(),
                                       torch.from_numpy(np.concatenate([g["dense_descriptor0"], g["dense_descriptor1"]])).cuda(),
                                       max_keypoints=1024, dense_layout="nchw")
    out.append("asset_pair.npz        descriptor max-abs error  " + "  ".join(
        f"{np.abs(d[b].cpu().numpy() - g[f'descriptors{b}']).max():.3e}" for b in range(2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="128x480x640,2x480x640,16x960x1280")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    sizes = parse_sizes(args.sizes)
    if args.reps < 1 or any(len(s) != 3 or min(s) < 1 or s[1] % 8 or s[2] % 8 for s in sizes):
        ap.error("sizes are BxHxW with H and W multiples of 8; reps >= 1")
    from linetr_amd.engine import Engine
    from linetr_amd.superpoint import FusedHeadSuperPoint
    eng = Engine.heads_only("cuda:0")
    lines = []
    for B, H, W in sizes:
        g = torch.Generator(device="cuda").manual_seed(B * 7 + H)
        # score statistics of a softmax over 65 channels: most pixels near 1/65 and below, sparse peaks
        score = torch.rand(B, H, W, device="cuda", generator=g) ** 8 * 0.3
        nhwc = torch.nn.functional.normalize(torch.randn(B, H // 8, W // 8, 256, device="cuda", generator=g), dim=-1)
        nchw = nhwc.permute(0, 3, 1, 2).contiguous()
        for k in (-1, 1024):
            cfg = {"nms_radius": 4, "keypoint_threshold": 0.005, "remove_borders": 4, "max_keypoints": k}
            parent = FusedHeadSuperPoint.__new__(FusedHeadSuperPoint)
            torch.nn.Module.__init__(parent)
            parent._fn, parent.config = Helpers, cfg
            sides = {"native": lambda: eng.superpoint_keypoints(score, nhwc, nms_radius=4, keypoint_threshold=0.005, remove_borders=4,
                                                                max_keypoints=k, align_corners=False, dense_layout="nhwc"),
                     "parent": lambda: parent._keypoints(score, nchw, H, W)}
            times = {name: [] for name in sides}
            waits = {}
            for name, fn in sides.items():
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                with WaitCounter() as wc:
                    out = fn()
                waits[name] = wc.n
                if name == "native":
                    n_kp = sum(int(t.shape[0]) for t in out[0])
            for _ in range(args.reps):                     # alternate the two sides
                for name, fn in sides.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            floor_bytes = B * H * W * 4 + B * H * ((W + 31) // 32) * 4 + n_kp * 5 * 1024
            q = {name: np.percentile(v, [50, 10, 90]) for name, v in times.items()}
            lines.append(f"{B:4d} x {H} x {W}  k={k:5d}  key points {n_kp:8d}  "
                         f"native {q['native'][0]:8.3f} ms (p10 {q['native'][1]:.3f} p90 {q['native'][2]:.3f}, {waits['native']} host wait(s))  "
                         f"parent {q['parent'][0]:8.3f} ms (p10 {q['parent'][1]:.3f} p90 {q['parent'][2]:.3f}, {waits['parent']} host waits)  "
                         f"x{q['parent'][0] / q['native'][0]:.1f}  HBM floor of the call {floor_bytes / 1e6:.1f} MB = {floor_bytes / HBM * 1e3:.4f} ms")
            print(lines[-1], flush=True)
    errors = []
    fixture_errors(eng, errors)
    print("\n".join(errors))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        open(os.path.join(ROOT, "profiles", "keypoints_bench.txt"), "w").write("\n".join(lines) + "\n")
        open(os.path.join(ROOT, "profiles", "keypoints_errors.txt"), "w").write("\n".join(errors) + "\n")


if __name__ == "__main__":
    main()
