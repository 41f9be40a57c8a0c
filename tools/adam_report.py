"""Measured error and time of the native Adam step and the gradient norm (csrc/lt_adam.h through linetr_adam_step / linetr_grad_norm,
Engine.adam_step / grad_norm, linetr_amd.optim.Adam) -- writes profiles/adam_errors.txt and profiles/adam_bench.txt:

    python tools/adam_report.py [--out-dir profiles] [--iters 20]

Errors: the cases of tests/test_gpu_adam.py (tests/adam_cases.py): the largest |gpu - float64| / bar per output.
Time, on the model's own 153 tensors (5 683 776 parameters), in one process, alternating windows of `iters` calls between two device
synchronisations: the native step against torch.optim.Adam as the reference constructs it (defaults), with foreach=False and with
fused=True.  Between two timed steps every side streams 512 MB of unrelated memory (a 256 MB buffer read and written), so that the 91 MB of
p, g, m and v do not stay in the 256 MiB Infinity Cache from one step to the next; the same windows with the streaming alone are printed
and subtracted.  The device time of one step is measured behind work queued in front of it (every launch is queued before the device
reaches the first), the host time of one step() call without any wait.  Then the whole training iteration at B = 32, L = 250, S = 21 with
the native and with torch's default optimizer.  No time is fixed in advance."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adam_cases as AC  # noqa: E402
import keyline_reference as KR  # noqa: E402
from sig_attn_bwd_report import compare  # noqa: E402

STEP_BYTES = 7 * 4 * 5683776             # p, g, m, v read; p, m, v written
HBM_TBS = 6.3                            # what a streaming kernel reaches on this part


def errors(eng):
    import test_gpu_adam as T
    lines = []

    def table(title, cases):
        worst = {o: (0.0, None) for o in AC.OUTPUTS}
        count = 0
        for key, rows in cases:
            count += 1
            for o, e, b in rows:
                if AC.ratio(e, b) >= worst[o][0]:
                    worst[o] = (AC.ratio(e, b), key)
        lines.append(f"{title}: {count} cases")
        lines.append("    " + "   ".join(f"{o} {worst[o][0]:5.3f} ({worst[o][1]})" for o in AC.OUTPUTS))

    def ragged(family):
        for step in AC.steps_of(family):
            case, refs = AC.make_case(family, step, T.TOTAL), AC.refs(family, step, T.TOTAL)
            for label, offsets in AC.ALIGNMENTS.items():
                yield f"step {step}, {label}", AC.ratios(AC.run_ragged(eng, case, T.SIZES, offsets), case["p"], *refs)

    for family in AC.FAMILIES:
        table(f"ragged table of {len(T.SIZES)} tensors ({T.TOTAL} elements), {family}", ragged(family))
    sizes = [i % 9 + 1 for i in range(1000)]
    case = AC.make_case("wd", 10, sum(sizes))
    out = AC.run_ragged(eng, case, sizes, {k: (0, 1, 2, 3) for k in "pgmv"})
    table("1 000 tensors of 1 .. 9 elements, wd, step 10", [("one call", AC.ratios(out, case["p"], *AC.refs("wd", 10, sum(sizes))))])

    def model_steps():
        shapes = [int(np.prod(s)) for s in AC.model_shapes()]
        rs = AC._rs("model shapes")
        total = sum(shapes)
        state = {"p": T.split((0.05 * rs.standard_normal(total)).astype(np.float32), shapes),
                 "m": [torch.zeros(n, device="cuda") for n in shapes], "v": [torch.zeros(n, device="cuda") for n in shapes]}
        hyper = dict(lr=AC.LR, betas=AC.BETAS, eps=AC.EPS, weight_decay=1e-4, decoupled_weight_decay=False)
        for step in (1, 2, 3):
            g = (rs.standard_normal(total) * 10.0 ** rs.uniform(-6, 0, total)).astype(np.float32)
            case = {"step": step, "hyper": hyper, "g": g, **{k: T.joined(state[k]) for k in "pmv"}}
            eng.adam_step(state["p"], T.split(g, shapes), state["m"], state["v"], [step] * len(shapes), **T.step_kwargs(case))
            yield f"step {step}", AC.ratios({k: T.joined(state[k]) for k in "pmv"}, case["p"], *AC.refs_of(case))

    table("the model's 153 tensors, seeded gradients, weight_decay 1e-4, each step from the device's own state", model_steps())

    def optimizer_on_the_model():
        from linetr_amd.optim import Adam
        mod, backward = T.model_and_loss()
        names, params = [k for k, _ in mod.named_parameters()], list(mod.parameters())
        sizes = [p.numel() for p in params]
        hyper = dict(lr=1e-3, weight_decay=1e-4)
        opt = Adam(params, **hyper)
        for step in (1, 2):
            opt.zero_grad()
            backward()
            ms = [opt.state[p]["exp_avg"].clone() for p in params] if step > 1 else None
            vs = [opt.state[p]["exp_avg_sq"].clone() for p in params] if step > 1 else None
            case = T.flat_case([p.detach().clone() for p in params], [p.grad for p in params], ms, vs, step, **hyper)
            opt.step()
            got = {"p": T.joined(params), "m": T.joined([opt.state[p]["exp_avg"] for p in params]),
                   "v": T.joined([opt.state[p]["exp_avg_sq"] for p in params])}
            rows = T.per_tensor_rows(names, sizes, got, case, AC.refs_of(case))
            worst = {o: max((r for r in rows if r[0].endswith("." + o)), key=lambda r: AC.ratio(r[1], r[2])) for o in AC.OUTPUTS}
            yield f"step {step}", [(o, worst[o][1], worst[o][2]) for o in AC.OUTPUTS]

    table("linetr_amd.optim.Adam on TrainableLineTransformer under descriptor_loss (B 2, n 33, S 21), worst of 153 parameters", optimizer_on_the_model())
    return ("# per group of cases and output (p', m', v', update = p' - p): the largest |gpu - float64 restatement| / bar and the case it occurs at;\n"
            f"# bar = {AC.FACTOR} x max(|torch.optim.Adam(foreach=False) float32 on the CPU - float64|, 2^-23 max |float64|) (tests/adam_cases.py); torch itself\n"
            "# sits at 0.125 by construction; written by tools/adam_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def bench(eng, iters):
    from linetr_amd.optim import Adam
    shapes = AC.model_shapes()
    gen = torch.Generator().manual_seed(12)
    values = [0.05 * torch.randn(s, generator=gen) for s in shapes]
    grads = [torch.randn(s, generator=gen) * 10.0 ** torch.empty(s).uniform_(-6, 0, generator=gen) for s in shapes]
    flush = torch.zeros(64 * 1024 * 1024, device="cuda")                   # 256 MB: read + written = 512 MB streamed
    busy = torch.randn(8192, 8192, device="cuda")

    def side(make):
        params = [torch.nn.Parameter(v.clone().cuda()) for v in values]
        for p, g in zip(params, grads):
            p.grad = g.clone().cuda()
        return make(params)

    sides = {"native (linetr_amd.optim.Adam)": side(lambda ps: Adam(ps, lr=1e-3, weight_decay=1e-4)),
             "torch.optim.Adam, defaults": side(lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4)),
             "torch.optim.Adam, foreach=False": side(lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4, foreach=False)),
             "torch.optim.Adam, fused=True": side(lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4, fused=True))}

    def flushed(opt):
        def run():
            flush.add_(1.0)
            opt.step()
        return run

    results = compare([lambda: flush.add_(1.0)] + [flushed(opt) for opt in sides.values()], iters)
    (f, f0, f1), rest = results[0], results[1:]
    out = [f"# the model's 153 parameter tensors ({sum(int(np.prod(s)) for s in shapes)} elements, {sum(int(np.prod(s)) <= 2048 for s in shapes)} of them of at most 2 048), lr 1e-3, weight_decay 1e-4, constant\n"
           f"# gradients; ms per call, median of 5 alternating windows of {iters} calls each between two device synchronisations (min .. max of the\n"
           f"# windows in brackets); a call = 512 MB of unrelated memory streamed (a 256 MB buffer read and written) + one step(); all sides float32\n"
           f"# on the same GPU in the same process; written by tools/adam_report.py on {torch.cuda.get_device_name(0)}\n",
           f"{'the streaming alone':38s} {f:8.4f} ms  [{f0:.4f} .. {f1:.4f}]\n"]
    for name, (t, t0, t1) in zip(sides, rest):
        out.append(f"{name:38s} {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   less the streaming {t - f:8.4f} ms\n")
    native, default, fused = rest[0][0], rest[1][0], rest[3][0]
    out.append(f"torch defaults / native {default / native:.2f} (less the streaming {(default - f) / (native - f):.2f}): "
               + ("the native step is not slower than torch's default\n" if native <= default else "the native step is SLOWER than torch's default\n"))

    # the device time of one step: queued behind work, so that no launch waits for the host
    def device_ms(opt, reps=9):
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                torch.mm(busy, busy)
            flush.add_(1.0)
            a.record()
            opt.step()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times)), min(times), max(times)

    def host_ms(opt, reps=20):
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            opt.step()
            times.append(1e3 * (time.perf_counter() - t))
            torch.cuda.synchronize()
        return float(np.median(times)), min(times), max(times)

    out.append(f"\n# one step() alone: device time between two events queued behind three 8192^3 matrix products and the streaming (every launch is\n"
               f"# queued before the device reaches the first; median of 9 [min .. max]); {STEP_BYTES / 1e6:.0f} MB over it beside the {HBM_TBS} TB/s a streaming\n"
               f"# kernel reaches; host time of the step() call, nothing waited for (median of 20 [min .. max])\n")
    alone = {}
    for name, opt in sides.items():
        d, d0, d1 = device_ms(opt)
        h, h0, h1 = host_ms(opt)
        alone[name] = (d, h)
        out.append(f"{name:38s} device {d:8.4f} ms  [{d0:.4f} .. {d1:.4f}]  {STEP_BYTES / d / 1e9:5.2f} TB/s of {HBM_TBS}   host {h:8.4f} ms  [{h0:.4f} .. {h1:.4f}]\n")
    (dn, hn), (df, hf) = alone["native (linetr_amd.optim.Adam)"], alone["torch.optim.Adam, fused=True"]
    out.append(f"torch fused / native per window {fused / native:.2f}" + ("\n" if native <= fused else
               f": fused=True is faster in the windows.  They are bound by the host on both sides (native: host {hn:.3f} ms against device {dn:.3f} ms; "
               f"fused: host {hf:.3f} ms against device {df:.3f} ms), and fused's host path is C++ throughout while the native step() walks its "
               f"{len(shapes)} parameters in Python; on the device the native step takes {dn / df:.2f} of fused's time\n"))
    # the raw call: does the table's way to the device make the host wait for the stream?
    opt = sides["native (linetr_amd.optim.Adam)"]
    params = opt.param_groups[0]["params"]
    args = (params, [p.grad for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params], [5.0] * len(params))
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)

    def raw_host(queued):
        times = []
        for _ in range(9):
            torch.cuda.synchronize()
            for _ in range(3 if queued else 0):
                torch.mm(busy, busy)
            t = time.perf_counter()
            eng.adam_step(*args, **kw)
            times.append(1e3 * (time.perf_counter() - t))
        torch.cuda.synchronize()
        return float(np.median(times))
    idle, queued = raw_host(False), raw_host(True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(3):
        torch.mm(busy, busy)
    torch.cuda.synchronize()
    mm = 1e3 * (time.perf_counter() - t)
    out.append(f"Engine.adam_step host time on an idle stream {idle:.4f} ms, behind {mm:.1f} ms of queued work {queued:.4f} ms: "
               + ("the call does not wait for the stream\n" if queued < idle + 0.25 * mm else "the call WAITS for the stream\n"))
    norm_opt = side(lambda ps: Adam(ps, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0))
    d, d0, d1 = device_ms(norm_opt)
    h, h0, h1 = host_ms(norm_opt)
    out.append(f"{'native with max_grad_norm':38s} device {d:8.4f} ms  [{d0:.4f} .. {d1:.4f}]  (the norm reads 23 MB more)   host {h:8.4f} ms  [{h0:.4f} .. {h1:.4f}]\n")
    del sides, norm_opt, flush, busy

    # ---- the whole iteration: two views forward, descriptor_loss, backward, step
    import linetr_amd.evaluations as E
    from linetr_amd.train_ops import TrainableLineTransformer
    B, n, S = 32, 250, 21
    rs = np.random.RandomState(10)
    sd = KR.model_state_dict(rs)
    v0 = KR.model_inputs(rs, B, n, S)
    v0["desc_sublines"] = (rs.standard_normal((B, 1, 1, 256)) + 0.5 * rs.standard_normal((B, n, 1, 256)) + 0.25 * v0["desc_sublines"]).astype(np.float32)
    v1 = {k: v.copy() for k, v in v0.items()}
    v1["desc_sublines"] += 0.25 * rs.standard_normal((B, n, S, 256)).astype(np.float32)
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    assign[:, np.arange(n), np.arange(n)] = 1.0
    d0, d1 = KR.data_tensors(v0, torch.float32, "cuda", grad=False), KR.data_tensors(v1, torch.float32, "cuda", grad=False)
    target = {"mat_assign_sublines": torch.from_numpy(assign).cuda()}
    crit = E.descriptor_loss()

    def iteration(make):
        mod = TrainableLineTransformer({})
        mod.load_state_dict(KR.tensors(sd), strict=True)
        mod = mod.cuda().train()
        opt = make(mod.parameters())

        def run():
            opt.zero_grad()
            with torch.enable_grad():
                loss = crit({"line_desc0": mod(d0)["line_desc"], "line_desc1": mod(d1)["line_desc"]}, target)[0]
                loss.backward()
            opt.step()
        return run

    (a, a0, a1), (t, t0, t1) = compare((iteration(lambda ps: Adam(ps, lr=1e-3, weight_decay=1e-4)),
                                        iteration(lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4))), max(iters // 4, 2))
    out.append(f"\n# the training iteration (train.py:193-195) at B = {B}, L = {n}, S = {S}: zero_grad, two views forward, descriptor_loss, backward, step;\n"
               f"# ms per iteration, median of 5 alternating windows of {max(iters // 4, 2)} iterations\n"
               f"{'with linetr_amd.optim.Adam':38s} {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"{'with torch.optim.Adam, defaults':38s} {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.3f}\n")
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("adam_errors.txt", lambda: errors(eng)), ("adam_bench.txt", lambda: bench(eng, args.iters))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
