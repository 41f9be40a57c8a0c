"""Measured error and time of the native criterion gradient (linetr_desc_loss_grad through Engine.loss_step) -- writes
profiles/loss_grad_errors.txt and profiles/loss_grad_bench.txt:

    python tools/loss_grad_report.py [--out-dir profiles] [--iters 20]

Errors: the cases of tests/test_gpu_loss_grad.py (tests/loss_grad_reference.py): max |gpu - float64| over both gradients, the bar
(4 x the float32 autograd error of the same case, floored at two float32 spacings of max |gradient|) and their ratio; the exact family
must show error 0.
Time: the training shape B = 32, n = 250 -- one native call (loss scalars + both gradients, host wait included) against forward +
backward of a torch restatement of the criterion on the same device, with the reference's Python loop over the anchor rows and with
one masked argmin in its place."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import val_step_reference as R  # noqa: E402
import loss_grad_reference as LG  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def errors(eng):
    lines = []

    def line(name, d0, d1, assign, cf, yardstick):
        res = eng.loss_step(dev(d0), dev(d1), assign=dev(assign))
        err = LG.max_err(res["grad0"].cpu().numpy(), res["grad1"].cpu().numpy(), cf)
        bar = LG.bar_of(yardstick, LG.grad_max(cf)) if yardstick is not None else 0.0
        ratio = f"{err / bar:5.3f}" if bar else ("exact" if err == 0 else "NOT EXACT")
        lines.append(f"{name:28s} V {res['count']:5d}  max |grad| {LG.grad_max(cf):.3e}  err {err:.3e}  yardstick "
                     f"{0.0 if yardstick is None else yardstick:.3e}  bar {bar:.3e}  err/bar {ratio}")

    g, f = (np.load(os.path.join(ROOT, "tests", "golden", k + ".npz")) for k in ("val_step", "loss_grad"))
    line("fixture B=3 n=40", g["desc0"], g["desc1"], g["assign"], {"grad0": f["grad0_f64"], "grad1": f["grad1_f64"]}, float(f["ref_f32_err"]))
    for B, n in LG.EDGE_CASES:
        if n == 1:
            continue
        d0, d1, assign = LG.edge_case(B, n)
        cf = LG.closed_form(d0, d1, assign)
        t0, t1 = LG.torch_grads(d0, d1, assign, torch.float32)
        line(f"clustered B={B} n={n}", d0, d1, assign, cf, LG.max_err(t0, t1, cf))
    for variant in LG.EXACT_VARIANTS:
        d0, d1, assign = LG.exact_case(variant)
        line(f"exact {variant}", d0, d1, assign, LG.closed_form(d0, d1, assign), None)
    return ("# max |gpu - float64| over d loss / d line_desc0 and d loss / d line_desc1 per case; yardstick = float32 autograd error of the same\n"
            f"# case against float64 (fixture: the reference's own; clustered: torch on the CPU); bar = max({LG.FACTOR} x yardstick, 2 float32 spacings of max |grad|)\n"
            "# written by tools/loss_grad_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def bench(eng, iters):
    B, n = 32, 250
    d0, d1, assign = (dev(x) for x in R.clustered_case(7, B, n))

    def native():
        eng.loss_step(d0, d1, assign=assign)

    def restated(row_loop):
        def run():
            a, b = d0.clone().requires_grad_(), d1.clone().requires_grad_()
            with torch.enable_grad():
                LG.torch_criterion(a, b, assign, row_loop=row_loop)[0].backward()
        return run

    V = eng.loss_step(d0, d1, assign=assign)["count"]
    t_native = timed(native, iters)
    t_vec = timed(restated(False), iters)
    t_loop = timed(restated(True), max(2, iters // 10))
    return (f"# criterion value + gradient with respect to both descriptor sets at B = {B}, n = {n} (V = {V} of {2 * B * n} anchor rows), median wall\n"
            f"# time of one step with the device idle before and synchronised after; written by tools/loss_grad_report.py on {torch.cuda.get_device_name(0)}\n"
            "# lg_grad_kernel walks the non-zeros of dL/dD (one 1 KB descriptor row load + 4 fmaf per lane each) instead of a dense exact-fp32\n"
            "# MFMA product of the 64 x 64 tile; its cost grows with the non-zeros per row (clustered data: about 1.3 per anchor; a row whose\n"
            "# positives all tie exactly would walk up to n).  The dense MFMA form has not been built or timed.\n"
            f"native Engine.loss_step (4 launches, 1 host wait)             {t_native:9.3f} ms\n"
            f"torch restatement, masked argmin, forward + backward         {t_vec:9.3f} ms   x{t_vec / t_native:.1f}\n"
            f"torch restatement, Python loop over anchor rows, fwd + bwd   {t_loop:9.3f} ms   x{t_loop / t_native:.1f}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, text in (("loss_grad_errors.txt", errors(eng)), ("loss_grad_bench.txt", bench(eng, args.iters))):
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
