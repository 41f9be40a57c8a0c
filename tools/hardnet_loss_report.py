"""Measured error and time of the native HardNet criterion (linetr_hardnet_loss_grad through Engine.hardnet_step) -- writes
profiles/hardnet_loss_errors.txt and profiles/hardnet_loss_bench.txt:

    python tools/hardnet_loss_report.py [--out-dir profiles] [--rounds 30]

Errors: the cases of tests/test_gpu_hardnet_loss.py (tests/hardnet_reference.py): max |gpu - float64| over both gradients, the bar
(4 x the float32 autograd error of the same case, floored at two float32 spacings of max |gradient|) and their ratio; the exact family
must show error 0.
Time: the training shape B = 32, n = 250, device events around each side after warm-up, the sides alternating round by round in one
process, medians: the native call with both gradients and value-only, linetr_desc_loss_grad on the same inputs (the same dots and the
same contraction: the difference is the selection), and forward + backward of the torch restatement on the same device, with the
reference's Python loop over the anchors and vectorised.  Nothing is fixed in advance: the file records what was measured."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import val_step_reference as R  # noqa: E402
import hardnet_reference as H  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def errors(eng):
    lines = []

    def line(name, d0, d1, assign, cf, yardstick):
        res = eng.hardnet_step(dev(d0), dev(d1), assign=dev(assign))
        err = H.max_err(res["grad0"].cpu().numpy(), res["grad1"].cpu().numpy(), cf)
        bar = H.bar_of(yardstick, H.grad_max(cf)) if yardstick is not None else 0.0
        ratio = f"{err / bar:5.3f}" if bar else ("exact" if err == 0 else "NOT EXACT")
        lines.append(f"{name:42s} V {res['count']:5d} live {res['live']:5d}  max |grad| {H.grad_max(cf):.3e}  err {err:.3e}  yardstick "
                     f"{0.0 if yardstick is None else yardstick:.3e}  bar {bar:.3e}  err/bar {ratio}")

    f = np.load(os.path.join(ROOT, "tests", "golden", "hardnet_loss.npz"))
    line("fixture B=3 n=40", f["desc0"], f["desc1"], f["assign"], {"grad0": f["grad0_f64"], "grad1": f["grad1_f64"]}, float(f["ref_f32_err"]))
    for B, n, extra in H.EDGE_CASES:
        if n == 1:
            continue
        d0, d1, assign = H.edge_case(B, n, extra)
        cf = H.closed_form(d0, d1, assign)
        t0, t1 = H.torch_grads(d0, d1, assign, torch.float32)
        line(f"clustered B={B} n={n}" + (" extra positives" if extra else ""), d0, d1, assign, cf, H.max_err(t0, t1, cf))
    for variant in H.EXACT_VARIANTS:
        d0, d1, assign = H.exact_case(variant)
        line(f"exact {variant}", d0, d1, assign, H.closed_form(d0, d1, assign), None)
    return ("# max |gpu - float64| over d loss / d line_desc0 and d loss / d line_desc1 per case; yardstick = float32 autograd error of the same\n"
            f"# case against float64 (fixture: the reference's own; clustered: torch on the CPU); bar = max({H.FACTOR} x yardstick, 2 float32 spacings of max |grad|)\n"
            "# written by tools/hardnet_loss_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def bench(eng, rounds):
    from linetr_amd import _native as nat
    L = nat.lib()
    B, n = 32, 250
    d0, d1, assign = (dev(x) for x in R.clustered_case(7, B, n))
    r0, r1 = (x.transpose(1, 2).contiguous().view(-1, 256) for x in (d0, d1))
    g0, g1 = torch.empty_like(r0), torch.empty_like(r1)
    host = torch.zeros(64, dtype=torch.uint8).pin_memory()
    ws_h = torch.empty(L.linetr_hardnet_loss_grad_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    ws_s = torch.empty(L.linetr_desc_loss_grad_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def hardnet(grads):
        def run():
            rc = L.linetr_hardnet_loss_grad(None, r0.data_ptr(), n, r1.data_ptr(), n, assign.data_ptr(), B, None, g0.data_ptr() if grads else None,
                                            g1.data_ptr() if grads else None, None, None, None, host.data_ptr(), host.numel(), ws_h.data_ptr(),
                                            ws_h.numel(), stream())
            assert rc == 0
        return run

    def semi_hard():
        rc = L.linetr_desc_loss_grad(None, r0.data_ptr(), n, r1.data_ptr(), n, assign.data_ptr(), B, None, g0.data_ptr(), g1.data_ptr(),
                                     host.data_ptr(), host.numel(), ws_s.data_ptr(), ws_s.numel(), stream())
        assert rc == 0

    def restated(anchor_loop):
        def run():
            a, b = d0.clone().requires_grad_(), d1.clone().requires_grad_()
            with torch.enable_grad():
                H.torch_criterion(a, b, assign, anchor_loop=anchor_loop)[0].backward()
        return run

    sides = [("native linetr_hardnet_loss_grad, both gradients (5 launches, 1 copy)", hardnet(True), 1),
             ("native linetr_hardnet_loss_grad, value only (4 launches, 1 copy)", hardnet(False), 1),
             ("native linetr_desc_loss_grad (semi-hard), both gradients (4 launches)", semi_hard, 1),
             ("torch restatement, vectorised, forward + backward", restated(False), 1),
             ("torch restatement, Python loop over the anchors, forward + backward", restated(True), 10)]      # every 10th round: it is slow
    res = eng.hardnet_step(d0, d1, assign=assign)
    for _, fn, every in sides:                                               # warm-up: every shape the timed window uses
        for _ in range(3 if every == 1 else 1):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in sides]
    for r in range(rounds):
        for i, (_, fn, every) in enumerate(sides):
            if r % every:
                continue
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times[i].append(start.elapsed_time(end))
    med = [float(np.median(t)) for t in times]
    text = (f"# HardNet criterion at B = {B}, n = {n} (V = {res['count']} of {2 * B * n} lines are anchors, {res['live']} live): device time between two\n"
            f"# events around one call, the sides alternating round by round in one process after warm-up, medians of {rounds} rounds (the Python\n"
            f"# loop: of {len(times[-1])}); measured, not fixed in advance; written by tools/hardnet_loss_report.py on {torch.cuda.get_device_name(0)}\n"
            "# the two native criteria share val_dot_kernel and the contraction of the gradient kernel: their difference is the selection\n"
            "# (hn_select_kernel reads every entry once; hn_resolve_kernel gathers the cross weights over n anchors per line)\n")
    for (name, _, _), t, ts in zip(sides, med, times):
        text += f"{name:74s} {t:10.3f} ms   (min {min(ts):.3f}, max {max(ts):.3f})   x{t / med[0]:.1f}\n"
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, text in (("hardnet_loss_errors.txt", errors(eng)), ("hardnet_loss_bench.txt", bench(eng, args.rounds))):
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
