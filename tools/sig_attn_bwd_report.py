"""Measured error and time of the neighbour-line attention's forward with statistics and backward (csrc/lt_attnbwd.h through
linetr_sig_attention_forward / _backward and Engine.sig_attention_*) -- writes profiles/sig_attn_bwd_errors.txt and
profiles/sig_attn_bwd_bench.txt:

    python tools/sig_attn_bwd_report.py [--out-dir profiles] [--iters 100]

Errors: the ragged batch of tests/test_gpu_sig_attn_bwd.py (tests/sig_attn_bwd_reference.py) per family: the largest error / bar of every
output over the batch's images and the image size it occurs at (the bar, per image and output: 8 x max(float32 CPU autograd error of the
same image against float64, 2^-23 max |float64|)).
Time: the training shape B = 32, n = 250 -- forward + backward native against torch autograd of the same attention on rows (attn_rows) on the same
GPU in the same process, alternating, `iters` calls per window between two synchronisations, and against the forward kernel alone (the
backward does 2.5 x the forward's contraction work).  No time is fixed in advance."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import attn_cases as AC  # noqa: E402
import sig_attn_bwd_reference as SA  # noqa: E402


def errors(L):
    counts = SA.ragged_counts()
    lines = []
    for family in SA.FAMILIES:
        c = SA.case(family, counts)
        rows = SA.image_ratios(SA.launch(L, c), c)
        cells = []
        for key in SA.OUTPUTS:
            r, n = max(((e / b, n) for _, n, k, e, b in rows if k == key and b > 0), default=(0.0, 0))
            cells.append(f"{key} {r:5.3f} (n = {n})")
        lines.append(f"{family:9s} " + "   ".join(cells))
    return ("# per family: the largest |gpu - float64| / bar of every output over the images of one ragged batch, and the size of the image it occurs\n"
            f"# at; bar = {SA.FACTOR:g} x max(float32 CPU autograd error of the same image against float64, 2^-23 max |float64|)\n"
            f"# image sizes {sorted(n for n in counts if n)} shuffled, an empty image first, in the middle and last ({int(sum(counts))} rows)\n"
            "# written by tools/sig_attn_bwd_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def window(fn, iters):
    """ms per call: `iters` calls between two synchronisations"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def compare(fns, iters, rounds=5):
    for fn in fns:
        fn()                                               # warm every side
    times = [[] for _ in fns]
    for _ in range(rounds):                                # alternating windows
        for t, fn in zip(times, fns):
            t.append(window(fn, iters))
    return [(float(np.median(t)), min(t), max(t)) for t in times]


def bench(eng, iters):
    B, n = 32, 250
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn((B * n, 768), generator=g).cuda()
    dO = torch.randn((B * n, 256), generator=g).cuda()
    q, k, v = qkv[:, :256], qkv[:, 256:512], qkv[:, 512:]
    cu = (torch.arange(B + 1, dtype=torch.int32) * n).cuda()
    o, lse = eng.sig_attention_forward(q, k, v, cu)

    def forward():
        eng.sig_attention_forward(q, k, v, cu)

    def backward():
        eng.sig_attention_backward(q, k, v, o, lse, dO, cu)

    def both():
        forward()
        backward()

    # the same rows as contiguous [B, n, 4, 64] tensors for torch
    rows = lambda t: t.reshape(B, n, 4, 64).contiguous()
    qt, kt, vt = (rows(t).requires_grad_() for t in (q, k, v))
    gt = rows(dO)

    def torch_both():
        with torch.enable_grad():
            out, _ = SA.attn_rows(qt, kt, vt)
        torch.autograd.grad(out, (qt, kt, vt), gt)

    (f, f0, f1), (b, b0, b1), (fb, fb0, fb1), (t, t0, t1) = compare((forward, backward, both, torch_both), iters)
    return (f"# B = {B}, n = {n} ({B * n} rows, q | k | v column blocks of one [N][768] buffer); ms per call, median of 5 alternating windows of {iters}\n"
            f"# calls each between two device synchronisations (min .. max of the windows in brackets); written by tools/sig_attn_bwd_report.py on\n"
            f"# {torch.cuda.get_device_name(0)}.  Every contraction is exact-fp32 MFMA; the backward does 2.5 x the forward's contraction work\n"
            f"forward with lse (1 launch), native                          {f:8.4f} ms  [{f0:.4f} .. {f1:.4f}]\n"
            f"backward dq, dk, dv (3 launches), native                     {b:8.4f} ms  [{b0:.4f} .. {b1:.4f}]   backward / forward {b / f:.2f}\n"
            f"forward + backward, native                                   {fb:8.4f} ms  [{fb0:.4f} .. {fb1:.4f}]\n"
            f"attn_rows forward + backward, torch autograd (n x n prob)   {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / fb:.2f}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, text in (("sig_attn_bwd_errors.txt", errors(eng._L)), ("sig_attn_bwd_bench.txt", bench(eng, args.iters))):
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
