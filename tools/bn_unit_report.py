"""Measured error of the train-mode BatchNorm kernels (lt_bntrain.h) against float64, as a fraction of the unit tests' bar
(tests/bn_cases.py: bar = 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per 64-row tile of y and per statistics vector).  Runs the
cases of tests/test_gpu_bn_train.py through linetr_debug_bn_train and writes profiles/bn_unit_errors.txt:

    python tools/bn_unit_report.py [--out profiles/bn_unit_errors.txt]

One line per (entry, family, unit): compared units, the largest error / bar ratio and the case it was measured on."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import bn_cases as BC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_unit_errors.txt"))
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from linetr_amd.engine import Engine
    engines = {}

    def engine(weights="calibrated", widths=BC.CHAIN_WIDTHS[0]):
        if (weights, widths) not in engines:
            engines[(weights, widths)] = Engine(BC.chain_state_dict(weights, widths)[0], "cuda:0", keyline_encoder=list(widths), bn_batch_stats=True)
        return engines[(weights, widths)]

    stat = collections.OrderedDict()          # (entry, family, unit) -> [units, worst ratio, where]

    def note(entry, family, rows, where):
        for r in rows:
            unit = "y tile" if isinstance(r[0], int) else r[0].split()[-1]
            s = stat.setdefault((entry, family, unit), [0, 0.0, ""])
            s[0] += 1
            ratio = r[2] / r[3] if r[3] else (float("inf") if r[2] else 0.0)
            if ratio >= s[1]:
                s[1], s[2] = ratio, f"{where}, unit {r[0]}: err {r[2]:.3e}, bar {r[3]:.3e}"

    for key in BC.layer_cases():
        case = BC.layer_case(*key)
        got, nb = BC.launch_layer(engine(), case)
        fam = key[0] + (f" {key[5]:g}" if key[0] == "offset" else "") + (", 1 row" if key[3] == 1 else ", >= 32767 rows" if BC.is_big(key) else "")
        note("bn_train_layer", fam, BC.layer_errors(got, case), f"C {key[1]} ld {key[2]} rows {key[3]} momentum {key[4]:g} chunks {nb}")
    for widths in BC.CHAIN_WIDTHS:
        for enc in ("word", "line"):
            for weights in BC.CHAIN_WEIGHTS:
                for rows in BC.CHAIN_ROWS:
                    case = BC.chain_case(enc, weights, widths, rows)
                    got = BC.launch_chain(engine(weights, widths), case)[0]
                    note(f"pos_encoder_bn {enc}", "-".join(str(w) for w in widths), BC.chain_errors(got, case), f"{weights} rows {rows}")
    lines = [f"{k:20s} {f:26s} {u:9s} units {s[0]:6d}  max err/bar {s[1]:6.3f}  ({s[2]})" for (k, f, u), s in stat.items() if s[0]]
    text = (f"# max |gpu - float64| / bar of the train-mode BatchNorm kernels per input family; bar = {BC.FACTOR:g} * max(max |ref32 - ref64|, 2^-23 max |ref64|)\n"
            "# per 64-row tile of y and per statistics vector (batch mean, batch var, running mean, running var, alpha; the chains: per layer);\n"
            "# '1 row': y against 4 x 2^-24 (|z alpha| + |beta|), bn_cases.single_row_errors\n"
            "# written by tools/bn_unit_report.py\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
