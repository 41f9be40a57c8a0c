#!/usr/bin/env python3
"""Errors and timings of the native SuperPoint encoder on the GPU:  python tools/sp_encoder_report.py [--out DIR] [--quick]

  DIR/sp_encoder_errors.txt   every unit case of tests/sp_encoder_cases.py as error / bar (the bar is a property of the CPU references
                              alone: 8 x max(|ref32 - ref64|, 2^-23 max|ref64|)), then the chain cases
  DIR/sp_encoder_bench.txt    per layer at 480 x 640: time and fraction of the 157 TF exact-fp32 matrix peak; then the whole native
                              encoder + heads against FusedHeadSuperPoint.encode + superpoint_heads (torch / MIOpen, the path of the
                              default configuration) in the same process, alternating, at B = 2 and B = 16

Timing: every shape is warmed up, each sample is one HIP-event pair around `inner` back-to-back calls, the median and the 10th / 90th
percentile of the samples are reported.  No GPU: the tool fails.  DIR defaults to profiles/."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sp_encoder_cases as S  # noqa: E402
from linetr_amd.engine import Engine  # noqa: E402
from workloads import synth  # noqa: E402

PEAK_F32_MATRIX = 157.3e12       # v_mfma_f32_32x32x2_f32: 256 FLOP / clk / CU x 256 CUs x 2.4 GHz
# the encoder's layers at full resolution: name, Cin, Cout, pool, resolution divisor of the INPUT
LAYERS = (("conv1b", 64, 64, 1, 1), ("conv2a", 64, 64, 0, 2), ("conv2b", 64, 64, 1, 2), ("conv3a", 64, 128, 0, 4),
          ("conv3b", 128, 128, 1, 4), ("conv4a", 128, 128, 0, 8), ("conv4b", 128, 128, 0, 8), ("convPa|convDa", 128, 512, 0, 8))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def timed(fn, warmup, samples, inner):
    """median, p10, p90 in ms of `samples` HIP-event windows of `inner` calls each"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return tuple(float(np.percentile(out, q)) for q in (50, 10, 90))


def errors(eng, lines):
    TH, TW = eng.sp_conv_tile()
    lines.append(f"# unit cases through linetr_sp_conv3x3, tile {TH} x {TW}: error / bar (max |gpu - ref64| over the bar of the CPU references)")
    for cin, cout in S.PAIRS:
        for pool in (0, 1):
            for H, W, B in S.sizes(TH, TW):
                for family in ("normal", "integers"):
                    x, w, b, r32, r64 = S.layer_case(family, cin, cout, B, H, W)
                    if pool:
                        r32, r64 = S.pool_ref(r32), S.pool_ref(r64)
                    if r64.size == 0:
                        lines.append(f"conv3x3 {cin:3d}->{cout:3d} pool={pool} B={B} {H:2d}x{W:2d} {family:8s} empty output")
                        continue
                    y = eng.sp_conv3x3(dev(x), eng.sp_conv3x3_pack(dev(w)), dev(b), pool=bool(pool)).cpu().numpy()
                    err, bar = np.abs(y - r64).max(), S.bar(r32, r64)
                    lines.append(f"conv3x3 {cin:3d}->{cout:3d} pool={pool} B={B} {H:2d}x{W:2d} {family:8s} error {err:.3e} bar {bar:.3e} "
                                 f"ratio {err / bar:.3f}" + ("  (bit-equal)" if np.array_equal(y.astype(np.float64), r64) else ""))
    for H, W, B in S.sizes(TH, TW):
        img, w, b = S.conv1a_inputs("normal", B, H, W)
        r32, r64 = S.conv1a_ref(img, w, b, torch.float32), S.conv1a_ref(img, w, b, torch.float64)
        y = eng.sp_conv1a(dev(img), dev(w), dev(b)).cpu().numpy()
        err, bar = np.abs(y - r64).max(), S.bar(r32, r64)
        lines.append(f"conv1a B={B} {H:2d}x{W:2d} normal   error {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    lines.append("# the whole chain (linetr_sp_encoder_forward, seed-0 weights) against the float64 restatement")
    for H, W in ((64, 96), (72, 104), (70, 100)):
        image, sd, r32, r64 = S.chain_case(H, W)
        score, desc, shape, feat = eng.superpoint_encode(dev(image), {k: dev(v) for k, v in sd.items()}, return_feat=True)
        nchw = lambda rows: rows.reshape(*shape, -1).permute(0, 3, 1, 2).cpu().numpy()
        for key, have in (("feat", feat.cpu().numpy()), ("score_logits", nchw(score)), ("desc_raw", nchw(desc))):
            err, bar = np.abs(have - r64[key]).max(), S.bar(r32[key], r64[key])
            lines.append(f"chain {H}x{W} {key:12s} max|ref64| {np.abs(r64[key]).max():7.3f} |ref32-ref64| {np.abs(r32[key] - r64[key]).max():.3e} "
                         f"error {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")


def bench(eng, lines, quick):
    from linetr_amd.superpoint import FusedHeadSuperPoint
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_producer import _StandInSuperPoint
    H, W = (480, 640)
    warm, samples = (2, 5) if quick else (5, 20)
    g = torch.Generator(device="cuda").manual_seed(0)
    sd = {k: dev(v) for k, v in synth.superpoint_state_dict(0).items()}
    lines.append(f"# per layer at {H} x {W}, B = 2: linetr_sp_conv3x3 alone; median ms (p10 p90), achieved TFLOP/s, fraction of the "
                 f"{PEAK_F32_MATRIX / 1e12:.0f} TF exact-fp32 matrix peak (the MFMA bound; every layer is above the HBM ridge)")
    B = 2
    total = 0.0
    for name, cin, cout, pool, div in LAYERS:
        h, w = H // div, W // div
        x = torch.randn(B, h, w, cin, device="cuda", generator=g)
        if name.startswith("convPa"):
            wt = torch.cat([sd["convPa.weight"], sd["convDa.weight"]])
            bias = torch.cat([sd["convPa.bias"], sd["convDa.bias"]])
        else:
            wt, bias = sd[name + ".weight"], sd[name + ".bias"]
        packed = eng.sp_conv3x3_pack(wt)
        out = torch.empty((B, h // 2, w // 2, cout) if pool else (B, h, w, cout), device="cuda")
        flop = 2.0 * B * h * w * 9 * cin * cout
        ms, lo, hi = timed(lambda: eng.sp_conv3x3(x, packed, bias, pool=bool(pool), out=out), warm, samples, 5)
        total += ms
        lines.append(f"{name:14s} {cin:3d}->{cout:3d} pool={pool} {h:3d}x{w:3d}  {flop / 1e9:7.2f} GFLOP  {ms:8.4f} ms ({lo:.4f} {hi:.4f})  "
                     f"{flop / ms / 1e9:6.1f} TFLOP/s  {flop / ms / 1e-3 / PEAK_F32_MATRIX:6.1%} of peak")
    img = torch.rand(B, 1, H, W, device="cuda", generator=g)
    o1 = torch.empty(B, H, W, 64, device="cuda")
    ms, lo, hi = timed(lambda: eng.sp_conv1a(img, sd["conv1a.weight"], sd["conv1a.bias"], out=o1), warm, samples, 5)
    by = B * H * W * 65 * 4.0
    lines.append(f"{'conv1a':14s}   1-> 64 pool=0 {H}x{W}  direct kernel, HBM-bound: {by / 1e6:.1f} MB  {ms:8.4f} ms ({lo:.4f} {hi:.4f})  "
                 f"{by / ms / 1e9:.2f} TB/s")
    lines.append(f"sum of the eight 3x3 layers' medians: {total:.4f} ms for B = {B}")

    lines.append("# whole encoder + heads, native (superpoint_encode + superpoint_heads_rows) against the torch / MIOpen path "
                 "(FusedHeadSuperPoint.encode + superpoint_heads), same process, alternating windows; median ms (p10 p90)")
    sp = _StandInSuperPoint()
    sp.load_state_dict({k: v.cpu() for k, v in sd.items()})
    sp = sp.cuda().eval()
    for p in sp.parameters():
        p.requires_grad_(False)
    wrap = FusedHeadSuperPoint(sp, engine=eng)
    params = dict(sp.named_parameters())
    for B in (2, 16):
        img = torch.rand(B, 1, H, W, device="cuda", generator=g)

        def native():
            s, d, shape = eng.superpoint_encode(img, params)
            return eng.superpoint_heads_rows(s, d, shape, nhwc=True, nchw=False)

        def parent():
            with torch.no_grad():
                s, d = wrap.encode(img)
            return eng.superpoint_heads(s, d, nhwc=True, nchw=False)
        a, b = native(), parent()
        diff = max((a[0] - b[0]).abs().max().item(), (a[1] - b[1]).abs().max().item())
        n_t, p_t = [], []
        for _ in range(3):                         # alternate the two sides
            n_t.append(timed(native, warm, samples // 2 + 1, 2))
            p_t.append(timed(parent, warm, samples // 2 + 1, 2))
        n_ms, p_ms = sorted(n_t)[1], sorted(p_t)[1]
        flop = B * 52.0e9 * (H * W) / (480 * 640)
        lines.append(f"B = {B:2d}  native {n_ms[0]:8.3f} ms ({n_ms[1]:.3f} {n_ms[2]:.3f}) = {flop / n_ms[0] / 1e9:5.1f} TFLOP/s end to end   "
                     f"torch/MIOpen {p_ms[0]:8.3f} ms ({p_ms[1]:.3f} {p_ms[2]:.3f})   native / torch time ratio {n_ms[0] / p_ms[0]:.2f}   "
                     f"max dense-map difference {diff:.2e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--quick", action="store_true", help="fewer samples")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sp_encoder_report needs the GPU: nothing is measured on a CPU")
    os.makedirs(args.out, exist_ok=True)
    torch.set_grad_enabled(False)
    eng = Engine.heads_only("cuda:0")
    for name, fn in (("sp_encoder_errors.txt", lambda ls: errors(eng, ls)), ("sp_encoder_bench.txt", lambda ls: bench(eng, ls, args.quick))):
        lines = ["# tools/sp_encoder_report.py" + (" --quick" if args.quick else "")]
        fn(lines)
        with open(os.path.join(args.out, name), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
