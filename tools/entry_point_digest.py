"""One SHA-256 per case over every output tensor's bytes of the entry points that run the exact-fp32 attention tile (sig_attn_tile),
the BatchNorm forward (lt_bntrain.h) and the descriptive layer's pooling and LayerNorm, plain and with dropout (lt_descbwd.h,
lt_dropout.h): the companion of tools/kernel_isa_diff.py for a refactor that DOES move instructions and must not move a bit.  On the
GPU box, once in the parent's tree and once in this one, both built; the two listings must be equal line for line (diff them):
    python tools/entry_point_digest.py > listing.txt
Cases and launch helpers are the unit tests' (tests/*_cases.py, tests/*_reference.py); the cases their is_big() names are left out and
the descriptive layer runs at the unit tests' small sizes, so a run takes seconds.
profiles/*_digest.txt record its listings."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attn_cases as AC  # noqa: E402
import bn_bwd_cases as BB  # noqa: E402
import bn_cases as BC  # noqa: E402
import desc_layer_reference as DL  # noqa: E402
import dropout_reference as DR  # noqa: E402
import sig_attn_bwd_reference as SA  # noqa: E402
from helpers import load, train_mode_batches  # noqa: E402
from workloads import synth  # noqa: E402

torch.set_grad_enabled(False)


def line(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t).tobytes())
    print(f"{name:70s} {h.hexdigest()}")


def parities(family):
    return (0, 1) if family == "sentinel" else (0,)


def main():
    from linetr_amd import _native as nat
    from linetr_amd.engine import Engine
    from models.line_process import line_tokenizer
    from models.line_transformer import LineTransformer
    L = nat.lib()
    eng = Engine(AC.state_dict_t("calibrated")[0], "cuda:0")
    for family in AC.FAMILIES:          # linetr_debug_sig_attention, kernel 0: tests/test_gpu_attention.py's batches
        for par in parities(family):
            line(f"sig_attn ragged {family} parity {par}", AC.launch(eng, 0, AC.qkv_case(family, AC.ragged_counts(0), parity=par))[0])
    for family in ("normal", "planted"):
        for n in AC.counts_for(0):
            line(f"sig_attn alone {family} n {n}", AC.launch(eng, 0, AC.qkv_case(family, (n,)))[0])
    for family in SA.FAMILIES:          # linetr_sig_attention_forward: tests/test_gpu_sig_attn_bwd.py's batch, both layouts
        for layout in ("packed", "apart"):
            got = SA.launch(L, SA.case(family, SA.ragged_counts()), layout, need=(False, False, False))
            line(f"sig_attention_forward {family} {layout}", got["o"], got["lse"])
    widths = BC.CHAIN_WIDTHS[0]
    eng = Engine(BC.chain_state_dict("calibrated", widths)[0], "cuda:0", keyline_encoder=list(widths), bn_batch_stats=True)
    for key in BC.layer_cases():        # linetr_debug_bn_train, one layer
        if not BC.is_big(key):
            got = BC.launch_layer(eng, BC.layer_case(*key))[0]
            line(f"debug_bn_train {key}", *(got[k] for k in ("y", "run_mean", "run_var", "mean", "var", "alpha", "beta2")))
    for key in BB.layer_cases():        # linetr_bn_forward, train and eval mode
        if not BB.is_big(key):
            got = BB.launch_forward(L, BB.layer_case(*key))
            line(f"bn_forward {key}", *(got[k] for k in ("y", "save_mean", "save_invstd", "run_mean", "run_var")))
    g = load("train_mode")              # linetr_forward_train: the module in train mode on the fixture's two batches
    nl = int(g["n_desc_layers"])
    m = LineTransformer({"mode": "train", "max_keylines": -1, "min_length": 16, "token_distance": 8, "nn_threshold": 0.8,
                         "n_line_descriptive_layers": nl})
    m.load_state_dict(synth.to_torch_state_dict(synth.calibrated_state_dict(nl)), strict=True)
    m = m.to("cuda").eval()
    hw = tuple(int(v) for v in g["hw"])
    pre = lambda rows, pred: m.preprocess(synth.array_to_keylines(rows), (1, 1, *hw), pred)
    tok = lambda lines, pred: line_tokenizer(lines, 8, 21, pred, (640, 480))
    batches = train_mode_batches(g, pre, tok, to_dev=lambda t: t.cuda())
    m.train()
    m.dropout = 0.0
    for c, batch in enumerate(batches):
        desc = m(batch)["line_desc"]
        line(f"forward_train call {c}", desc, *(v for k, v in sorted(m.state_dict().items()) if "running_" in k))
    desc_layer(L, nat)


POOL_L, POOL_S = (1, 4, 5, 9), (1, 2, 3, 4, 5, 22, 23)      # the edges of CP_SEGS = 4, CP_TOK = 4 and CP_TOK_B = 2 (csrc/lt_descbwd.h)
LN_ROWS = (1, 4, 5, 31, 32, 33, 65)                         # the edges of LN_ROWS = 4 and LN_CHUNK = 32
DROP_P = (0.0, 0.1, 0.5)


def desc_layer(L, nat):
    """The eight pooling / LayerNorm entry points of the descriptive layer, plain and with dropout, and linetr_dropout_factors, on the
    unit tests' cases (tests/desc_layer_reference.py, tests/dropout_reference.py) at their own small sizes; then the module."""
    take = lambda got, keys: [got[k] for k in keys]
    for l in POOL_L:                    # linetr_cls_pool_train_forward / _backward
        for s in POOL_S:
            line(f"cls_pool_train L {l} S {s}", *take(DL.pool_launch(L, DL.pool_case("normal", l, s)), DL.POOL_OUTPUTS))
    line("cls_pool_train peaky L 5 S 22", *take(DL.pool_launch(L, DL.pool_case("peaky", 5, 22)), DL.POOL_OUTPUTS))
    line("cls_pool_train padded L 5 S 23", *take(DL.pool_launch(L, DL.pool_case("normal", 5, 23), ldx=260, ldu=1028), DL.POOL_OUTPUTS))
    for rows in LN_ROWS:                # linetr_layer_norm_forward / _backward
        for residual in (False, True):
            line(f"layer_norm rows {rows} residual {residual}", *take(DL.ln_launch(L, DL.ln_case("normal", rows, residual)), DL.LN_OUTPUTS))
    line("layer_norm padded rows 33", *take(DL.ln_launch(L, DL.ln_case("normal", 33, True), ld=260), DL.LN_OUTPUTS))
    for p in DROP_P:
        for site, rows, inner in ((0, 9, 23), (1, 65, 64), (2, 65, 64)):        # linetr_dropout_factors
            line(f"dropout_factors p {p} site {site}", DR.factors_launch(L, nat, DR.SEED, 3, site, rows, inner, p))
        for l in POOL_L:                # linetr_cls_pool_dropout_forward / _backward
            for s in POOL_S:
                line(f"cls_pool_dropout p {p} L {l} S {s}", *take(DR.pool_launch(L, nat, DR.pool_case("normal", l, s, p)), DR.POOL_OUTPUTS))
        line(f"cls_pool_dropout p {p} padded L 5 S 23",
             *take(DR.pool_launch(L, nat, DR.pool_case("normal", 5, 23, p), ldx=260, ldu=1028), DR.POOL_OUTPUTS))
        for site in (1, 2):             # linetr_layer_norm_dropout_forward / _backward
            for rows in LN_ROWS:
                for residual in (False, True):
                    got = DR.ln_launch(L, nat, DR.ln_case(rows, residual, site, p))
                    line(f"layer_norm_dropout p {p} site {site} rows {rows} residual {residual}", *take(got, DR.LN_OUTPUTS))
            line(f"layer_norm_dropout p {p} site {site} padded rows 33",
                 *take(DR.ln_launch(L, nat, DR.ln_case(33, True, site, p), ld=260), DR.LN_OUTPUTS))
    from linetr_amd.train_ops import LineDescriptiveEncoder
    sd, desc, upstream = DL.module_case(2, 5, 22)       # LineDescriptiveEncoder, forward + backward: unseeded without dropout, seeded with
    for p, state in ((0.0, None), (0.1, (DR.SEED, 0))):
        mod = LineDescriptiveEncoder(dropout=p)
        mod.load_state_dict(DL.tensors(sd), strict=True)
        mod = mod.cuda().train()
        mod.set_dropout_state(state)
        x = torch.from_numpy(desc).cuda().requires_grad_()
        with torch.enable_grad():
            out = mod(x)[0]
            out.backward(torch.from_numpy(upstream).cuda())
        line(f"LineDescriptiveEncoder (2, 5, 22) dropout {p}", out.detach(), x.grad, *(prm.grad for _, prm in sorted(mod.named_parameters()) if prm.grad is not None))


if __name__ == "__main__":
    main()
