"""Measured error and time of the BatchNorm forward-for-training / backward kernels (csrc/lt_bnbwd.h through linetr_bn_forward /
linetr_bn_backward) and of the signature layer composed under autograd (linetr_amd.train_ops.AttentionalPropagation /
SelfAttentionalLayer) -- writes profiles/bn_bwd_errors.txt, profiles/sig_layer_errors.txt and profiles/sig_layer_bench.txt:

    python tools/sig_layer_report.py [--out-dir profiles] [--iters 50]

Errors: the cases of tests/test_gpu_bn_bwd.py (tests/bn_bwd_cases.py) per family and unit, and the tensors of tests/test_gpu_sig_layer.py
(tests/sig_layer_reference.py) per run: the largest |gpu - float64| / bar.
Time, at the training shape B = 32, n = 250, native against torch on the same GPU in the same process, alternating windows of `iters`
calls between two synchronisations: BatchNorm + ReLU forward + backward on 8 000 x 512 (and against the bytes it must move at the achievable
HBM rate), one signature layer forward + backward, seven layers + head + criterion forward + backward.  No time is fixed in advance."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bn_bwd_cases as BB  # noqa: E402
import sig_layer_reference as SL  # noqa: E402
from sig_attn_bwd_report import compare  # noqa: E402

HBM_RATE = 6.3e12          # bytes / s a streaming kernel reaches on the MI355X


def bn_errors(L):
    units = ("y", "dz", "dgamma", "dbeta", "saved")
    worst = {(f, u): (0.0, None) for f in BB.FAMILIES for u in units}

    def note(fam, unit, rows, key):
        for _, _, e, b in rows:
            r = e / b if b else (float("inf") if e else 0.0)
            if r > worst[(fam, unit)][0]:
                worst[(fam, unit)] = (r, key)

    for key in BB.layer_cases():
        c = BB.layer_case(*key)
        fwd = BB.launch_forward(L, c)
        got = BB.launch_backward(L, c, save=fwd["_save"])
        note(key[0], "y", BB.forward_errors(fwd["y"], c), key)
        note(key[0], "saved", BB.saved_errors(fwd, c), key)
        rows = BB.backward_errors(got, c)
        note(key[0], "dz", [r for r in rows if isinstance(r[0], int)], key)
        for u in ("dgamma", "dbeta"):
            note(key[0], u, [r for r in rows if r[0] == u], key)
    lines = []
    for f in BB.FAMILIES:
        cells = []
        for u in units:
            r, key = worst[(f, u)]
            cells.append(f"{u} {r:5.3f}" + (f" (C {key[1]}, rows {key[2]})" if key else ""))
        lines.append(f"{f:9s} " + "   ".join(cells))
    return ("# per family and unit: the largest |gpu - float64| / bar over the cases of tests/bn_bwd_cases.py and the case it occurs at; y and dz per\n"
            f"# 64-row tile, dgamma and dbeta per vector, bar = {BB.FACTOR:g} x max(float32 torch error against float64, 2^-23 max |float64|); saved: the\n"
            "# statistics float64 [mean | invstd] against their own bounds (mean 1e-12 relative; invstd: the roundings of the one-pass variance)\n"
            "# written by tools/sig_layer_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def layer_errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_sig_layer as T
    lines = []

    def add(label, got, ref64, ref32):
        rows = SL.ratios(got, {k: v for k, v in ref64.items() if isinstance(v, np.ndarray)}, ref32)
        rows.sort(key=lambda r: -(r[1] / r[2] if r[2] else 0.0))
        lines.append(f"{label}: {len(rows)} tensors, worst " + ", ".join(f"{k} {e / b if b else 0.0:.3f}" for k, e, b in rows[:4]))
        for k, e, b in rows:
            lines.append(f"    {k:44s} err {e:.3e}  bar {b:.3e}  ratio {e / b if b else 0.0:.3f}")

    for B, n in SL.LAYER_SHAPES_TESTED:
        sd, x, source, g = SL.layer_case(B, n)
        add(f"layer [{B}, 256, {n}] train", T.run_native_layer(sd, x, source, g), *SL.layer_refs(B, n))
    sd, x, source, g = SL.layer_case(2, 33)
    add("layer [2, 256, 33] eval", T.run_native_layer(sd, x, source, g, train=False), *SL.layer_refs(2, 33, train=False))
    sd, x, g = SL.stack_case()
    mod = T.native_stack(sd)
    xt = T.dev(x).requires_grad_()
    with torch.enable_grad():
        y = mod(xt)
        y.backward(T.dev(g))
    add("stack of two [2, 256, 33]", T.collect(mod, {"out": y, "dx": xt.grad}), *SL.stack_refs())
    got = T.run_native_network()
    add("seven layers + head + criterion [2, 256, 33]", {k: v for k, v in got.items() if isinstance(v, np.ndarray)}, *SL.network_refs())
    return ("# per run and tensor: |gpu - float64 restatement| / bar, bar = 8 x max(float32 restatement's error against float64, 2^-23 max |float64|)\n"
            "# (tests/sig_layer_reference.py; the runs of tests/test_gpu_sig_layer.py); written by tools/sig_layer_report.py on "
            + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def bench(eng, iters):
    import linetr_amd.evaluations as E
    from linetr_amd.train_ops import AttentionalPropagation, DescriptorHead, SelfAttentionalLayer
    B, n = 32, 250
    rows, C = B * n, 512
    gen = torch.Generator().manual_seed(4)
    out = [f"# B = {B}, n = {n} ({rows} rows); ms per call, median of 5 alternating windows of {iters} calls each between two device synchronisations\n"
           f"# (min .. max of the windows in brackets); both sides float32 on the same GPU in the same process; written by tools/sig_layer_report.py on\n"
           f"# {torch.cuda.get_device_name(0)}\n"]

    # ---- BatchNorm + ReLU, forward + backward
    z, g = (torch.randn((rows, C), generator=gen).cuda() for _ in range(2))
    gamma, beta = (0.5 + torch.rand(C, generator=gen)).cuda(), torch.randn(C, generator=gen).cuda()
    rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()

    def native_bn():
        y, save = eng.bn_forward(z, gamma, beta, rm, rv)
        eng.bn_backward(z, y, g, save, gamma)

    zt, gt, bt = z.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()

    def torch_bn():
        with torch.enable_grad():
            y = F.relu(F.batch_norm(zt, rm, rv, gt, bt, True, 0.1, 1e-5))
        torch.autograd.grad(y, (zt, gt, bt), g)

    (a, a0, a1), (t, t0, t1) = compare((native_bn, torch_bn), iters)
    nbytes = 10 * rows * C * 4                               # forward: z twice, y once; backward: g, y, z twice, dz once
    floor = 1e3 * nbytes / HBM_RATE
    out.append(f"BatchNorm + ReLU forward + backward, {rows} x {C} (6 launches), native   {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]   "
               f"{nbytes / 1e6:.1f} MB at {HBM_RATE / 1e12:.1f} TB/s = {floor:.4f} ms: native / floor {a / floor:.2f}\n"
               f"relu(F.batch_norm) forward + backward, torch autograd                      {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.2f}\n")

    # ---- one signature layer, forward + backward
    sd = SL.layer_state_dict(np.random.RandomState(8))
    x, up = (torch.randn((B, 256, n), generator=gen).cuda() for _ in range(2))
    native = AttentionalPropagation.from_line_transformer({"selfattn.layers.0." + k: v for k, v in SL.tensors(sd).items()}).cuda().train()
    stock = SL.Layer()
    stock.load_state_dict(SL.tensors(sd), strict=True)
    stock = stock.cuda().train()
    xn = x.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_()      # rows behind the view, as the stack hands them on
    xs = x.clone().requires_grad_()

    def native_layer():
        with torch.enable_grad():
            delta, _ = native(xn, xn)
        torch.autograd.grad(delta, [xn] + list(native.parameters()), up)

    def torch_layer():
        with torch.enable_grad():
            delta = stock(xs, xs)
        torch.autograd.grad(delta, [xs] + list(stock.parameters()), up)

    (a, a0, a1), (t, t0, t1) = compare((native_layer, torch_layer), iters)
    out.append(f"one signature layer forward + backward, native                             {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"the restatement (tests/sig_layer_reference.py) by torch                    {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.2f}\n")

    # ---- seven layers + head + criterion, forward + backward
    sd, W, b, x0, x1, assign = SL.network_case(B, n)
    nstack = SelfAttentionalLayer.from_line_transformer({"selfattn." + k: v for k, v in SL.tensors(sd).items()}).cuda().train()
    nhead = DescriptorHead.from_line_transformer({"final_proj.weight": torch.from_numpy(W), "final_proj.bias": torch.from_numpy(b)}).cuda()
    sstack, shead = SL.build_network(torch.float32, "cuda")
    crit = E.descriptor_loss()
    a0_, a1_, at = (torch.from_numpy(v).cuda() for v in (x0, x1, assign))
    nparams, sparams = list(nstack.parameters()) + list(nhead.parameters()), list(sstack.parameters()) + list(shead.parameters())

    def native_net():
        with torch.enable_grad():
            loss = crit({"line_desc0": nhead(nstack(a0_)), "line_desc1": nhead(nstack(a1_))}, {"mat_assign_sublines": at})[0]
        torch.autograd.grad(loss, nparams)

    def torch_net():
        with torch.enable_grad():
            loss, _ = SL.network_loss(sstack, shead, a0_, a1_, at)
        torch.autograd.grad(loss, sparams)

    (a, a0, a1), (t, t0, t1) = compare((native_net, torch_net), max(iters // 5, 4))
    out.append(f"seven layers + head + criterion, both views, forward + backward, native    {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"the restatement + the criterion in torch (one masked argmin)               {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.2f}\n")
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("bn_bwd_errors.txt", lambda: bn_errors(eng._L)), ("sig_layer_errors.txt", layer_errors), ("sig_layer_bench.txt", lambda: bench(eng, args.iters))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
