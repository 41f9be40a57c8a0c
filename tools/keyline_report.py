"""Measured error and time of the positional encoders' and the token assembly's training kernels (csrc/lt_posbwd.h through
linetr_input_layer_*, linetr_token_assemble_*), of the encoders and of the whole network composed under autograd
(linetr_amd.train_ops.WordPositionalEncoder / TrainableLineTransformer) -- writes profiles/keyline_errors.txt and profiles/keyline_bench.txt:

    python tools/keyline_report.py [--out-dir profiles] [--iters 20]

Errors: the cases of tests/test_gpu_keyline.py (tests/keyline_reference.py) per kernel pair and output, and the tensors of its module runs:
the largest |gpu - float64| / bar.
Time, at the training shape B = 32, L = 250, S = 21, in the same process, alternating windows of `iters` calls between two
synchronisations: the two kernel pairs alone against the bytes they must move; the word encoder forward + backward, and the whole model
with the criterion on two views forward + backward, against torch autograd through the tests' float32 restatement on the same GPU.  No time
is fixed in advance."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import keyline_reference as KR  # noqa: E402
from sig_attn_bwd_report import compare  # noqa: E402


def _ratio(e, b):
    return e / b if b else (float("inf") if e else 0.0)


def errors(L):
    import test_gpu_keyline as T
    from helpers import load
    lines = []

    def table(title, outputs, cases):
        worst = {o: (0.0, None) for o in outputs}
        for key, got, c in cases:
            for o, e, b in KR.ratios(got, c["ref64"], c["ref32"], outputs):
                if _ratio(e, b) >= worst[o][0]:
                    worst[o] = (_ratio(e, b), key)
        lines.append(title)
        lines.append("    " + "   ".join(f"{o} {worst[o][0]:5.3f} {worst[o][1]}" for o in outputs))

    def il_cases():
        for Kin in KR.IL_KIN:
            for N in KR.IL_N:
                for rows in KR.il_rows(L.linetr_input_layer_chunk_rows()):
                    c = KR.il_case(Kin, N, rows)
                    yield f"(Kin {Kin}, N {N}, rows {rows})", KR.il_launch(L, c), c

    def ta_cases(family):
        for S in KR.TA_S:
            for n_seg in KR.ta_segments(T.ta_segs_per_block(L)):
                c = KR.ta_case(family, n_seg, S)
                yield f"(L {n_seg}, S {S})", KR.ta_launch(L, c), c

    table("input layer (linetr_input_layer_forward / _backward)", KR.IL_OUTPUTS, il_cases())
    for family in KR.TA_FAMILIES:
        table(f"token assembly (linetr_token_assemble_forward / _backward), {family}: x and dtok are exact copies / one add", ("dcls",), ta_cases(family))

    def add(label, rows, full=True):
        rows = sorted(rows, key=lambda r: -_ratio(r[1], r[2]))
        lines.append(f"{label}: {len(rows)} tensors, worst " + ", ".join(f"{k} {_ratio(e, b):.3f}" for k, e, b in rows[:4]))
        for k, e, b in rows if full else rows[:12]:
            lines.append(f"    {k:60s} err {e:.3e}  bar {b:.3e}  ratio {_ratio(e, b):.3f}")

    for kind, shapes in KR.ENCODER_SHAPES.items():
        for shape in shapes:
            for train in (True, False):
                sd, inputs, upstream = KR.encoder_case(kind, shape)
                mod = T.native_encoder(kind, sd, train)
                with torch.enable_grad():
                    out = mod(*(T.dev(a) for a in inputs))
                    out.backward(T.dev(upstream))
                got = KR.collect(mod, {"out": out.detach().double().cpu().numpy()})
                add(f"{kind} encoder {list(shape)} {'train' if train else 'eval'}", KR.ratios(got, *KR.encoder_refs(kind, shape, train)))
    sd, _, _ = KR.model_case()
    add(f"TrainableLineTransformer against the fixture {list(KR.FIXTURE_SHAPE)}, {KR.FIXTURE_CALLS} calls",
        KR.fixture_ratios(T.run_fixture_calls(T.native_model(sd)), load("keyline"), load("keyline_matrices")), full=False)
    ref64, ref32 = KR.loss_refs()
    got = T.run_native_loss(lr=KR.LOSS_LR)
    arrays = lambda d: {k: v for k, v in d.items() if isinstance(v, np.ndarray)}
    lines.append(f"two views under descriptor_loss {list(KR.LOSS_SHAPE)}: loss {got['loss']:.7f} (float64 {ref64['loss']:.7f}, float32 CPU {ref32['loss']:.7f}), "
                 f"V {got['V']} (float64 {ref64['V']})")
    add("TrainableLineTransformer on two views under descriptor_loss", KR.ratios(arrays(got), arrays(ref64), arrays(ref32)), full=False)
    return ("# per kernel pair and output: the largest |gpu - float64| / bar over the cases of tests/test_gpu_keyline.py and the case it occurs at;\n"
            "# per module run and tensor: |gpu - float64 restatement| / bar (the fixture: |gpu - the reference's float64 run| / its stored bar).\n"
            "# bar = 8 x max(float32 CPU autograd error against float64, 2^-23 max |float64|) (tests/keyline_reference.py); the twelve worst tensors\n"
            "# of the whole-model runs are listed; written by tools/keyline_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def bench(eng, iters):
    import test_gpu_keyline as T
    import linetr_amd.evaluations as E
    import loss_grad_reference as LG
    B, n, S = 32, 250, 21
    segs, toks = B * n, B * n * S
    gen = torch.Generator().manual_seed(8)
    rand = lambda *s: torch.randn(s, generator=gen).cuda()
    out = [f"# B = {B}, L = {n}, S = {S} ({segs} segments, {toks} token rows); ms per call, median of 5 alternating windows of {iters} calls each\n"
           f"# between two device synchronisations (min .. max of the windows in brackets); both sides float32 on the same GPU in the same process;\n"
           f"# written by tools/keyline_report.py on {torch.cuda.get_device_name(0)}\n"]

    # ---- the two kernel pairs alone
    x, W, b, g = rand(toks, 3), rand(32, 3), rand(32), rand(toks, 32)
    (f, f0, f1), (bw, b0, b1) = compare((lambda: eng.input_layer_forward(x, W, b), lambda: eng.input_layer_backward(x, W, g)), iters * 5)
    nbytes = 4.0 * toks * (32 + 3)
    out.append(f"input layer 3 -> 32 forward      {f:8.4f} ms  [{f0:.4f} .. {f1:.4f}]   {nbytes / 1e6:.1f} MB -> {nbytes / f / 1e9:.2f} TB/s\n"
               f"input layer 3 -> 32 backward     {bw:8.4f} ms  [{b0:.4f} .. {b1:.4f}]   {nbytes / 1e6:.1f} MB (g and x read) -> {nbytes / bw / 1e9:.2f} TB/s   (two launches)\n")
    desc, pos, cls, dx = rand(segs, S, 256), rand(segs, S, 256), rand(256), rand(segs, S + 1, 256)
    (f, f0, f1), (bw, b0, b1) = compare((lambda: eng.assemble_tokens_forward(desc, pos, cls), lambda: eng.assemble_tokens_backward(dx)), iters * 5)
    fb, bb = 4.0 * segs * 256 * (3 * S + 1), 4.0 * segs * 256 * (2 * S + 1)
    out.append(f"token assembly forward           {f:8.4f} ms  [{f0:.4f} .. {f1:.4f}]   {fb / 1e6:.0f} MB -> {fb / f / 1e9:.2f} TB/s\n"
               f"token assembly backward          {bw:8.4f} ms  [{b0:.4f} .. {b1:.4f}]   {bb / 1e6:.0f} MB (dx read, dtok written) -> {bb / bw / 1e9:.2f} TB/s   (two launches)\n")
    del desc, pos, dx

    # ---- the word encoder forward + backward
    rs = np.random.RandomState(10)
    sd = KR.encoder_state_dict(rs, 3)
    native = T.native_encoder("word", sd, True)
    stock = KR.WordEncoder()
    stock.load_state_dict(KR.tensors(sd), strict=True)
    stock = stock.cuda().train()
    pnt, score, up = torch.rand((B, n, S, 2), generator=gen).cuda() - 0.5, torch.rand((B, n, S, 1), generator=gen).cuda(), rand(B, n, S, 256)

    def side(mod):
        def run():
            with torch.enable_grad():
                y = mod(pnt, score)
            torch.autograd.grad(y, list(mod.parameters()), up)
        return run

    (a, a0, a1), (t, t0, t1) = compare((side(native), side(stock)), iters)
    verdict = "the native encoder is faster" if a < t else "the native encoder is NOT faster than the torch graph"
    out.append(f"WordPositionalEncoder forward + backward, native                              {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"the restatement (tests/keyline_reference.py) by torch autograd                {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.2f}: "
               f"{verdict}\n")
    del pnt, score, up

    # ---- the whole model with the criterion on two views
    sd = KR.model_state_dict(rs)
    v0 = KR.model_inputs(rs, B, n, S)
    v0["desc_sublines"] = (rs.standard_normal((B, 1, 1, 256)) + 0.5 * rs.standard_normal((B, n, 1, 256)) + 0.25 * v0["desc_sublines"]).astype(np.float32)
    v1 = {k: v.copy() for k, v in v0.items()}
    v1["desc_sublines"] += 0.25 * rs.standard_normal((B, n, S, 256)).astype(np.float32)
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    assign[:, np.arange(n), np.arange(n)] = 1.0
    d0, d1 = KR.data_tensors(v0, torch.float32, "cuda"), KR.data_tensors(v1, torch.float32, "cuda")
    at = T.dev(assign)
    native = T.native_model(sd)
    stock = KR.Model()
    stock.load_state_dict(KR.tensors(sd), strict=True)
    stock = stock.cuda().train()
    crit = E.descriptor_loss()
    leaves = lambda mod: [d0["desc_sublines"], d1["desc_sublines"]] + list(mod.parameters())

    def native_step():
        with torch.enable_grad():
            loss = crit({"line_desc0": native(d0)["line_desc"], "line_desc1": native(d1)["line_desc"]}, {"mat_assign_sublines": at})[0]
        torch.autograd.grad(loss, leaves(native))

    def torch_step():
        with torch.enable_grad():
            loss = LG.torch_criterion(stock(d0), stock(d1), at)[0]
        torch.autograd.grad(loss, leaves(stock))

    (a, a0, a1), (t, t0, t1) = compare((native_step, torch_step), max(iters // 4, 2))
    verdict = "the native step is faster" if a < t else "the native step is NOT faster than the torch graph"
    out.append(f"TrainableLineTransformer + descriptor_loss on two views, forward + backward   {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"the restatement + the criterion in torch (one masked argmin) by autograd      {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.2f}: "
               f"{verdict}\n")
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("keyline_errors.txt", lambda: errors(eng._L)), ("keyline_bench.txt", lambda: bench(eng, args.iters))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
