"""Measured error and cost of training-time dropout in the descriptive layer (csrc/lt_dropout.h through linetr_cls_pool_dropout_*,
linetr_layer_norm_dropout_*; LineDescriptiveEncoder.seed_dropout) -- writes profiles/dropout_errors.txt and profiles/dropout_bench.txt:

    python tools/dropout_report.py [--out-dir profiles] [--iters 20]

Errors: the cases of tests/test_gpu_dropout.py (tests/dropout_reference.py) per kernel and output and the tensors of its module and model
runs: the largest |gpu - float64| / bar.
Time, at the training shape B = 32, L = 250, S = 22, in the same process, alternating windows of `iters` calls between two
synchronisations: the two dropout pooling kernels beside their plain twins, the layer forward + backward at p = 0.1 against p = 0 and
against stock torch through the unfolded module with nn.Dropout(0.1), and the model + criterion step at p = 0.1 against p = 0.  No time is
fixed in advance."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

import desc_layer_reference as DL  # noqa: E402
import dropout_reference as DR  # noqa: E402
import keyline_reference as KR  # noqa: E402
from sig_attn_bwd_report import compare  # noqa: E402


def _ratio(e, b):
    return e / b if b else (float("inf") if e else 0.0)


def errors(L, nat):
    import test_gpu_dropout as T
    lines = []

    def table(title, groups, outputs, cases):
        worst = {(f, o): (0.0, None) for f in groups for o in outputs}
        for group, key, got, c in cases:
            keys = [o for o in outputs if o in c["ref64"]]
            for o, e, b in DL.ratios(got, c["ref64"], c["ref32"], keys):
                if _ratio(e, b) >= worst[(group, o)][0]:
                    worst[(group, o)] = (_ratio(e, b), key)
        lines.append(title)
        for f in groups:
            lines.append(f"    {f:18s} " + "   ".join(f"{o} {worst[(f, o)][0]:5.3f} {worst[(f, o)][1]}" for o in outputs))

    def pool_cases():
        for fam in DR.POOL_FAMILIES:
            for p in (0.0,) + DR.P_VALUES:
                for S in DR.POOL_S:
                    for n_seg in DR.POOL_L:
                        c = DR.pool_case(fam, n_seg, S, p)
                        yield f"{fam} p={p}", f"(L {n_seg}, S {S})", DR.pool_launch(L, nat, c), c

    def ln_cases():
        for site in (1, 2):
            for p in DR.P_VALUES:
                for residual in (False, True):
                    for rows in DR.LN_ROWS:
                        c = DR.ln_case(rows, residual, site, p)
                        yield f"site {site} p={p}", f"(rows {rows}{', residual' if residual else ''})", DR.ln_launch(L, nat, c), c

    table("CLS token pooling with dropout (linetr_cls_pool_dropout_forward / _backward)",
          [f"{fam} p={p}" for fam in DR.POOL_FAMILIES for p in (0.0,) + DR.P_VALUES], DR.POOL_OUTPUTS, pool_cases())
    table("LayerNorm with dropout and a residual (linetr_layer_norm_dropout_forward / _backward)",
          [f"site {site} p={p}" for site in (1, 2) for p in DR.P_VALUES], DR.LN_OUTPUTS, ln_cases())

    def add(label, got, ref64, ref32):
        rows = DL.ratios(got, ref64, ref32)
        rows.sort(key=lambda r: -_ratio(r[1], r[2]))
        lines.append(f"{label}: {len(rows)} tensors, worst " + ", ".join(f"{k} {_ratio(e, b):.3f}" for k, e, b in rows[:4]))
        for k, e, b in rows:
            lines.append(f"    {k:58s} err {e:.3e}  bar {b:.3e}  ratio {_ratio(e, b):.3f}")

    for shape in DR.MODULE_SHAPES:
        for p in DR.P_VALUES:
            sd, desc, g = DL.module_case(*shape)
            add(f"LineDescriptiveEncoder {list(shape) + [256]} train, dropout {p}", T.run_native(T.build(sd, dropout=p), desc, g), *DR.module_refs(*shape, p))
    sd = KR.loss_case()[0]
    got = T.run_native_loss(T.native_model(sd, dropout=DR.MODEL_P), (DR.SEED, 0))
    ref64, ref32 = DR.loss_refs()
    arrays = lambda d: {k: v for k, v in d.items() if isinstance(v, np.ndarray) and not k.startswith("_")}
    lines.append(f"TrainableLineTransformer + descriptor_loss on two views, dropout {DR.MODEL_P}: loss {got['loss']:.7f} against {ref64['loss']:.7f} "
                 f"(float32 CPU {ref32['loss']:.7f}), anchors {got['V']} / {ref64['V']}")
    add(f"TrainableLineTransformer {list(KR.LOSS_SHAPE)} two views under the criterion, dropout {DR.MODEL_P}", arrays(got), arrays(ref64), arrays(ref32))
    return ("# per kernel, case group and output: the largest |gpu - float64| / bar over the cases of tests/test_gpu_dropout.py and the case it occurs at;\n"
            "# per module run and tensor: |gpu - float64 restatement of the unfolded module with the same masks| / bar.  bar = 8 x max(float32 CPU\n"
            "# autograd error against float64, 2^-23 max |float64|) (tests/dropout_reference.py); written by tools/dropout_report.py on "
            + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


class _StockLayer(DL.Layer):
    """desc_layer_reference.Layer with nn.Dropout at the reference's three places: stock torch, its own device generator"""

    def __init__(self, p):
        super().__init__()
        self.d0, self.d1, self.d2 = nn.Dropout(p), nn.Dropout(p), nn.Dropout(p)

    def forward(self, desc, mask=None):
        import torch.nn.functional as F
        att, ffn = self.slf_attn, self.pos_ffn
        B, L, S, _ = desc.shape
        q, k, v = (w(desc).view(B, L, S, 4, 64).transpose(2, 3) for w in (att.w_qs, att.w_ks, att.w_vs))
        o = torch.matmul(self.d0(torch.softmax(torch.matmul(q / 8.0, k.transpose(3, 4)), dim=-1)), v).transpose(2, 3).contiguous().view(B, L, S, 256)
        y = att.layer_norm(self.d1(att.fc(o)) + desc)
        return ffn.layer_norm(self.d2(ffn.w_2(F.gelu(ffn.w_1(y)))) + y)


def bench(eng, iters):
    import test_gpu_dropout as T
    import linetr_amd.evaluations as E
    B, n, S = 32, 250, 22
    segs = B * n
    gen = torch.Generator().manual_seed(6)
    out = [f"# B = {B}, L = {n}, S = {S} ({segs} segments, {segs * S} token rows); ms per call, median of 5 alternating windows of {iters} calls each\n"
           f"# between two device synchronisations (min .. max of the windows in brackets); every pair in the same process on the same GPU;\n"
           f"# written by tools/dropout_report.py on {torch.cuda.get_device_name(0)}\n"]

    # ---- the pooling kernels: dropout beside plain
    x = torch.randn((segs, S, 256), generator=gen).cuda()
    u = (torch.randn((segs, 4, 256), generator=gen) / 16).cuda()
    g = torch.randn((segs, 4, 256), generator=gen).cuda()
    gk = torch.randn((segs, 4), generator=gen).cuda()
    drop = eng.dropout(DR.SEED, 0, 0.1)
    pooled, lse = eng.cls_pool_forward(x, u)
    dpooled, kept, dlse = eng.cls_pool_dropout_forward(x, u, drop)
    (f, f0, f1), (fd, fd0, fd1), (b, b0, b1), (bd, bd0, bd1) = compare(
        (lambda: eng.cls_pool_forward(x, u), lambda: eng.cls_pool_dropout_forward(x, u, drop), lambda: eng.cls_pool_backward(x, u, pooled, lse, g),
         lambda: eng.cls_pool_dropout_backward(x, u, dpooled, dlse, kept, g, gk, drop)), iters * 5)
    fb = 4.0 * segs * (S * 256 + 2 * 1024 + 4)
    bb = 4.0 * segs * (2 * S * 256 + 4 * 1024 + 4)
    out.append(f"CLS token pooling forward               {f:8.4f} ms  [{f0:.4f} .. {f1:.4f}]   {fb / f / 1e9:.2f} TB/s\n"
               f"CLS token pooling forward, p = 0.1      {fd:8.4f} ms  [{fd0:.4f} .. {fd1:.4f}]   {(fb + 16.0 * segs) / fd / 1e9:.2f} TB/s   dropout / plain {fd / f:.3f}\n"
               f"CLS token pooling backward              {b:8.4f} ms  [{b0:.4f} .. {b1:.4f}]   {bb / b / 1e9:.2f} TB/s\n"
               f"CLS token pooling backward, p = 0.1     {bd:8.4f} ms  [{bd0:.4f} .. {bd1:.4f}]   {(bb + 32.0 * segs) / bd / 1e9:.2f} TB/s   dropout / plain {bd / b:.3f}\n")
    del x, u, g, pooled, dpooled

    # ---- the layer forward + backward: p = 0.1 against p = 0 and against stock torch with nn.Dropout(0.1)
    sd = DL.state_dict(np.random.RandomState(9))
    plain, dropped = T.build(sd), T.build(sd, dropout=0.1).seed_dropout(DR.SEED)
    stock = _StockLayer(0.1)
    stock.load_state_dict(DL.tensors(sd), strict=True)
    stock = stock.cuda().train()
    desc = torch.randn((B, n, S, 256), generator=gen).cuda()
    up = torch.randn((B, n, 256), generator=gen).cuda()

    def layer(mod, row0):
        leaf = desc.clone().requires_grad_()

        def run():
            with torch.enable_grad():
                y = mod(leaf)
                y = y[:, :, 0] if row0 else y[0]
            torch.autograd.grad(y, [leaf] + list(mod.parameters()), up)
        return run

    (a, a0, a1), (d, d0, d1), (t, t0, t1) = compare((layer(plain, False), layer(dropped, False), layer(stock, True)), iters)
    out.append(f"LineDescriptiveEncoder forward + backward, native, dropout 0                     {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"LineDescriptiveEncoder forward + backward, native, dropout 0.1 (seeded)          {d:8.4f} ms  [{d0:.4f} .. {d1:.4f}]   p = 0.1 / p = 0 {d / a:.3f}\n"
               f"the unfolded module with nn.Dropout(0.1) at its three places by torch autograd   {t:8.4f} ms  [{t0:.4f} .. {t1:.4f}]   torch / native {t / d:.2f}\n")
    del desc, up

    # ---- the model + criterion step: p = 0.1 against p = 0
    S = 21
    rs = np.random.RandomState(10)
    sd = KR.model_state_dict(rs)
    v0 = KR.model_inputs(rs, B, n, S)
    v0["desc_sublines"] = (rs.standard_normal((B, 1, 1, 256)) + 0.5 * rs.standard_normal((B, n, 1, 256)) + 0.25 * v0["desc_sublines"]).astype(np.float32)
    v1 = {k: v.copy() for k, v in v0.items()}
    v1["desc_sublines"] += 0.25 * rs.standard_normal((B, n, S, 256)).astype(np.float32)
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    assign[:, np.arange(n), np.arange(n)] = 1.0
    d0_, d1_ = KR.data_tensors(v0, torch.float32, "cuda"), KR.data_tensors(v1, torch.float32, "cuda")
    at = T.dev(assign)
    crit = E.descriptor_loss()

    def step(mod):
        def run():
            with torch.enable_grad():
                loss = crit({"line_desc0": mod(d0_)["line_desc"], "line_desc1": mod(d1_)["line_desc"]}, {"mat_assign_sublines": at})[0]
            torch.autograd.grad(loss, [d0_["desc_sublines"], d1_["desc_sublines"]] + list(mod.parameters()))
        return run

    (a, a0, a1), (d, d0, d1) = compare((step(T.native_model(sd)), step(T.native_model(sd, dropout=0.1).seed_dropout(DR.SEED))), max(iters // 4, 2))
    out.append(f"TrainableLineTransformer + descriptor_loss on two views (S = {S}), dropout 0       {a:8.4f} ms  [{a0:.4f} .. {a1:.4f}]\n"
               f"TrainableLineTransformer + descriptor_loss on two views (S = {S}), dropout 0.1     {d:8.4f} ms  [{d0:.4f} .. {d1:.4f}]   p = 0.1 / p = 0 {d / a:.3f}\n")
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=("errors", "bench"), default=None)
    args = ap.parse_args()
    from linetr_amd import _native as nat
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    os.makedirs(args.out_dir, exist_ok=True)
    for name, make in (("dropout_errors.txt", lambda: errors(eng._L, nat)), ("dropout_bench.txt", lambda: bench(eng, args.iters))):
        if args.only and not name.startswith("dropout_" + args.only):
            continue
        text = make()
        with open(os.path.join(args.out_dir, name), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
