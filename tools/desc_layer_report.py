"""Measured error and time of the descriptive layer's training kernels (csrc/lt_descbwd.h through linetr_cls_pool_train_*,
linetr_layer_norm_*, linetr_gelu_*) and of the layer composed under autograd (linetr_amd.train_ops.LineDescriptiveEncoder) -- writes
profiles/desc_layer_errors.txt and profiles/desc_layer_bench.txt:

    python tools/desc_layer_report.py [--out-dir profiles] [--iters 20]

Errors: the cases of tests/test_gpu_desc_layer.py (tests/desc_layer_reference.py) per kernel, family and output, and the tensors of its
module runs: the largest |gpu - float64| / bar.
Time, at the training shape B = 32, L = 250, S = 22, in the same process, alternating windows of `iters` calls between two
synchronisations: the native layer forward + backward against torch autograd through the tests' float32 restatement of the UNFOLDED module
on the same GPU, and the two pooling kernels alone against the bytes they must move.  No time is fixed in advance."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import desc_layer_reference as DL  # noqa: E402
from sig_attn_bwd_report import compare  # noqa: E402


def _ratio(e, b):
    return e / b if b else (float("inf") if e else 0.0)


def kernel_errors(L):
    import test_gpu_desc_layer as T
    lines = []

    def table(title, families, outputs, cases):
        worst = {(f, o): (0.0, None) for f in families for o in outputs}
        for fam, key, got, c, pick in cases:
            got = {o: got[o][pick] if pick is not None else got[o] for o in outputs}
            for o, e, b in DL.ratios(got, c["ref64"], c["ref32"], outputs):
                if _ratio(e, b) >= worst[(fam, o)][0]:
                    worst[(fam, o)] = (_ratio(e, b), key)
        lines.append(title)
        for f in families:
            lines.append(f"    {f:9s} " + "   ".join(f"{o} {worst[(f, o)][0]:5.3f} {worst[(f, o)][1]}" for o in outputs))

    def pool_cases():
        for fam in DL.POOL_FAMILIES:
            for S in DL.POOL_S:
                for n_seg in DL.POOL_L:
                    c = DL.pool_case(fam, n_seg, S)
                    yield fam, f"(L {n_seg}, S {S})", DL.pool_launch(L, c), c, c["check"]

    def ln_cases():
        chunk = T.ln_chunk_rows(L)
        for fam in DL.LN_FAMILIES:
            for residual in (False, True):
                for rows in sorted({1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 5}):
                    c = DL.ln_case(fam, rows, residual)
                    yield fam, f"(rows {rows}{', residual' if residual else ''})", DL.ln_launch(L, c), c, None

    def gelu_cases():
        for fam in DL.GELU_FAMILIES:
            c = DL.gelu_case(fam)
            yield fam, "", DL.gelu_launch(L, c["z"], c["g"]), c, None

    table("CLS token pooling (linetr_cls_pool_train_forward / _backward)", DL.POOL_FAMILIES, DL.POOL_OUTPUTS, pool_cases())
    table("LayerNorm with a residual (linetr_layer_norm_forward / _backward)", DL.LN_FAMILIES, DL.LN_OUTPUTS, ln_cases())
    table("GELU (linetr_gelu_forward / _backward), one bar per magnitude family", DL.GELU_FAMILIES, ("y", "dz"), gelu_cases())

    def add(label, got, ref64, ref32):
        rows = DL.ratios(got, ref64, ref32)
        rows.sort(key=lambda r: -_ratio(r[1], r[2]))
        lines.append(f"{label}: {len(rows)} tensors, worst " + ", ".join(f"{k} {_ratio(e, b):.3f}" for k, e, b in rows[:4]))
        for k, e, b in rows:
            lines.append(f"    {k:44s} err {e:.3e}  bar {b:.3e}  ratio {_ratio(e, b):.3f}")

    for shape, train in ((DL.FIXTURE_SHAPE, True), (DL.MODULE_SHAPES[0], True), (DL.MODULE_SHAPES[1], True), (DL.FIXTURE_SHAPE, False)):
        sd, desc, g = DL.module_case(*shape)
        add(f"LineDescriptiveEncoder {list(shape) + [256]} {'train' if train else 'eval'}", T.run_native(T.build(sd, train), desc, g),
            *DL.module_refs(*shape, train))
    return ("# per kernel, family and output: the largest |gpu - float64| / bar over the cases of tests/test_gpu_desc_layer.py and the case it occurs at;\n"
            "# per module run and tensor: |gpu - float64 restatement of the unfolded module| / bar.  bar = 8 x max(float32 CPU autograd error against\n"
            "# float64, 2^-23 max |float64|) (tests/desc_layer_reference.py); written by tools/desc_layer_report.py on " + torch.cuda.get_device_name(0)
            + "\n" + "\n".join(lines) + "\n")


def bench(eng, iters):
    import test_gpu_desc_layer as T
    B, n, S = 32, 250, 22
    segs = B * n
    gen = torch.Generator().manual_seed(6)
    out = [f"# B = {B}, L = {n}, S = {S} ({segs} segments, {segs * S} token rows); ms per call, median of 5 alternating windows of {iters} calls each\n"
           f"# between two device synchronisations (min .. max of the windows in brackets); both sides float32 on the same GPU in the same process;\n"
           f"# written by tools/desc_layer_report.py on {torch.cuda.get_device_name(0)}\n"]

    # ---- the pooling kernels alone
    x = torch.randn((segs, S, 256), generator=gen).cuda()
    u = (torch.randn((segs, 4, 256), generator=gen) / 16).cuda()
    g = torch.randn((segs, 4, 256), generator=gen).cuda()
    pooled, lse = eng.cls_pool_forward(x, u)
    (f, f0, f1), (b, b0, b1) = compare((lambda: eng.cls_pool_forward(x, u), lambda: eng.cls_pool_backward(x, u, pooled, lse, g)), iters * 5)
    fb = 4.0 * segs * (S * 256 + 2 * 1024 + 4)
    bb = 4.0 * segs * (2 * S * 256 + 4 * 1024 + 4)
    out.append(f"CLS token pooling forward   {f:8.4f} ms  [{f0:.4f} .. {f1:.4f}]   {fb / 1e6:.0f} MB -> {fb / f / 1e9:.2f} TB/s\n"
               f"CLS token pooling backward  {b:8.4f} ms  [{b0:.4f} .. {b1:.4f}]   {bb / 1e6:.0f} MB (x read, dx written) -> {bb / b / 1e9:.2f} TB/s\n")

    # ---- the layer forward + backward, native (folded) against the unfolded restatement run by torch
    sd = DL.state_dict(np.random.RandomState(9))
    native = T.build(sd)
    stock = DL.Layer()
    stock.load_state_dict(DL.tensors(sd), strict=True)
    stock = stock.cuda().train()
    desc = torch.randn((B, n, S, 256), generator=gen).cuda()
    up = torch.randn((B, n, 256), generator=gen).cuda()
    dn, ds = desc.clone().requires_grad_(), desc.clone().requires_grad_()

    def native_layer():
        with torch.enable_grad():
            y, _ = native(dn)
        torch.autograd.grad(y, [dn] + list(native.parameters()), up)

    def torch_layer():
        with torch.enable_grad():
            y = stock(ds)[:, :, 0]
        torch.autograd.grad(y, [ds] + list(stock.parameters()), up)

    (a, a0, a1), (t, t0, t1) = compare((native_layer, torch_layer), iters)
    verdict = "the native layer is faster" if a < t else "the native layer is NOT faster than the unfolded torch graph"
    out.append(f"LineDescriptiveEncoder forward + backward, native (folded, CLS row only)     {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"the unfolded restatement (tests/desc_layer_reference.py) by torch autograd   {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / a:.2f}: "
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
    for name, make in (("desc_layer_errors.txt", lambda: kernel_errors(eng._L)), ("desc_layer_bench.txt", lambda: bench(eng, args.iters))):
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
