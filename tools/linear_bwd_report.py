"""Measured error and time of the native backward of the 1x1 layers and the descriptor head (csrc/lt_linbwd.h through Engine.linear_* /
head_*) -- writes profiles/linear_bwd_errors.txt and profiles/linear_bwd_bench.txt:

    python tools/linear_bwd_report.py [--out-dir profiles] [--iters 200]

Errors: the cases of tests/test_gpu_linear_bwd.py (tests/linear_bwd_reference.py): per case the largest error / bar over its outputs
(the bar: 4 x the float32 torch autograd error of the same case against float64, floored at two float32 spacings of max |output|), and
per family the largest ratio; the exact family must show error 0.
Time: rows = 32 x 250 -- the head's backward and a 512 x 512 layer's backward, each against torch autograd of the same expression on
the same GPU in the same process, alternating, `iters` calls per window between two synchronisations.  No time is fixed in advance."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import linear_bwd_reference as LB  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def worst_ratio(got, ref, yard, keys):
    worst, at = 0.0, ""
    for k, (bar, _) in LB.bars(yard, ref, keys).items():
        r = np.abs(got[k].astype(np.float64) - ref[k]).max() / bar
        if r >= worst:
            worst, at = r, k
    return worst, at


def layer(eng, x, W, b, g, mask, relu):
    xd, Wd = dev(x), dev(W)
    y = eng.linear_forward(xd, Wd, dev(b), relu=relu)
    dx, dW, db = eng.linear_backward(xd, Wd, dev(g), mask=dev(mask) if mask is not None else None)
    return {k: v.cpu().numpy() for k, v in (("y", y), ("dx", dx), ("dW", dW), ("db", db))}


def errors(eng):
    Rc = int(eng._L.linetr_linear_backward_chunk_rows())
    keys = ("y", "dx", "dW", "db")
    lines, family = [], {"exact": 0, "normal": 0.0, "normal, masked": 0.0, "head": 0.0}
    for r, N, K in LB.CASES:
        rows = LB.resolve_rows(r, Rc)
        x, W, b, g, mask = LB.exact_case(rows, N, K)
        wrong = 0
        for m, relu in ((None, False), (mask, True)):
            cf, got = LB.layer_closed_form(x, W, b, g, m, relu), layer(eng, x, W, b, g, m, relu)
            wrong += sum(int(np.count_nonzero(got[k] != cf[k].astype(np.float32))) for k in keys)
        family["exact"] += wrong
        x, W, b, g, mask = LB.normal_case(rows, N, K)
        plain, at0 = worst_ratio(layer(eng, x, W, b, g, None, False), LB.layer_closed_form(x, W, b, g), LB.torch_layer(x, W, b, g, torch.float32), keys)
        masked, at1 = worst_ratio(layer(eng, x, W, b, g, mask, True), LB.layer_closed_form(x, W, b, g, mask, True),
                                  LB.torch_layer(x, W, b, g, torch.float32, relu=True), keys)
        family["normal"], family["normal, masked"] = max(family["normal"], plain), max(family["normal, masked"], masked)
        text = f"rows {rows:4d} N {N:4d} K {K:4d}  exact: {'bit-equal' if not wrong else f'{wrong} WRONG'}  normal err/bar {plain:5.3f} ({at0})  masked err/bar {masked:5.3f} ({at1})"
        if (N, K) == LB.FULL_NK:
            cf = LB.head_closed_form(x, W, b, g)
            xd, Wd, bd, gd = dev(x), dev(W), dev(b), dev(g)
            d = eng.head_forward(xd, Wd, bd)
            dx, dW, db = eng.head_backward(xd, Wd, bd, gd)
            got = {k: v.cpu().numpy() for k, v in (("d", d), ("dx", dx), ("dW", dW), ("db", db))}
            head, at2 = worst_ratio(got, cf, LB.torch_head(x, W, b, g, torch.float32), tuple(got))
            family["head"] = max(family["head"], head)
            text += f"  head err/bar {head:5.3f} ({at2})"
        lines.append(text)
    summary = [f"largest err/bar, {k} family: {v:5.3f}" if k != "exact" else f"exact family: {'bit-equal everywhere' if not v else f'{v} elements WRONG'}"
               for k, v in family.items()]
    return ("# per case: the largest |gpu - float64| / bar over y, dx, dW, db (head: d, dx, dW, db) and the output it occurs at; bar = max("
            f"{LB.FACTOR} x float32 torch\n# autograd error of the same case against float64, 2 float32 spacings of max |output|); chunk rows Rc = {Rc}\n"
            "# written by tools/linear_bwd_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines + summary) + "\n")


def window(fn, iters):
    """ms per call: `iters` calls between two synchronisations"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def compare(native, restated, iters, rounds=5):
    native(), restated()                                   # warm both
    a, b = [], []
    for _ in range(rounds):                                # alternating windows
        a.append(window(native, iters))
        b.append(window(restated, iters))
    return float(np.median(a)), float(np.median(b)), (min(a), max(a)), (min(b), max(b))


def bench(eng, iters):
    rows = 32 * 250
    out = [f"# rows = 32 x 250 = {rows}; ms per call, median of 5 alternating windows of {iters} calls each between two device synchronisations\n"
           f"# (min .. max of the windows in brackets); written by tools/linear_bwd_report.py on {torch.cuda.get_device_name(0)}\n"
           "# every contraction is exact-fp32 MFMA; a bf16x6 form was not built or timed\n"]
    x, W, b, g, _ = (dev(a) for a in LB.normal_case(rows, 256, 256, seed=1))

    def head_native():
        eng.head_backward(x, W, b, g)

    def head_torch():
        xt, Wt, bt = x.clone().requires_grad_(), W.clone().requires_grad_(), b.clone().requires_grad_()
        with torch.enable_grad():
            F.normalize(F.linear(xt, Wt, bt), p=2, dim=1).backward(g)

    n, t, nr, tr = compare(head_native, head_torch, iters)
    out.append(f"head backward 256 x 256 (forward recomputed inside), native   {n:8.4f} ms  [{nr[0]:.4f} .. {nr[1]:.4f}]\n"
               f"F.normalize(F.linear(x)) forward + backward, torch autograd  {t:8.4f} ms  [{tr[0]:.4f} .. {tr[1]:.4f}]   torch / native {t / n:.2f}\n")
    x, W, b, g, mask = (dev(a) for a in LB.normal_case(rows, 512, 512, seed=2))

    def layer_native():
        eng.linear_backward(x, W, g, mask=mask)

    xt, Wt, bt = x.clone().requires_grad_(), W.clone().requires_grad_(), b.clone().requires_grad_()
    with torch.enable_grad():
        yt = F.relu(F.linear(xt, Wt, bt))

    def layer_torch():
        torch.autograd.grad(yt, (xt, Wt, bt), g, retain_graph=True)

    n, t, nr, tr = compare(layer_native, layer_torch, iters)
    out.append(f"layer backward 512 x 512 with ReLU mask (dx, dW, db), native  {n:8.4f} ms  [{nr[0]:.4f} .. {nr[1]:.4f}]\n"
               f"backward of F.relu(F.linear(x)), torch autograd (graph kept) {t:8.4f} ms  [{tr[0]:.4f} .. {tr[1]:.4f}]   torch / native {t / n:.2f}\n")
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, text in (("linear_bwd_errors.txt", errors(eng)), ("linear_bwd_bench.txt", bench(eng, args.iters))):
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
