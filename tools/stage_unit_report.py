"""Measured error of the descriptive layer's tail and of the line-signature network, each run alone through linetr_debug_stage, against
float64, as a fraction of the unit tests' bar (tests/stage_cases.py: bar = 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per tensor /
per image and tensor, every step judged from the device's own input to it).  Runs the cases of tests/test_gpu_stages.py and writes
profiles/stage_unit_errors.txt:

    python tools/stage_unit_report.py [--out profiles/stage_unit_errors.txt]

One line per (stage, weights, depth, precision, plan, family, tensor): compared units, the largest error / bar ratio and the unit it
was measured on; then the largest ratio per stage and precision."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import stage_cases as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_unit_errors.txt"))
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from linetr_amd.engine import Engine
    engines = {}

    def engine(weights, L=7):
        if (weights, L) not in engines:
            engines[(weights, L)] = Engine(S.weights_t(weights, L)[0], "cuda:0", n_sig_layers=L)
        return engines[(weights, L)]

    lines, top = [], collections.defaultdict(float)

    def emit(stage, prec, what, rows):
        """rows of the error measure, grouped by tensor (the taps of all layers as one)"""
        by = collections.defaultdict(list)
        for w, u, n, e, b in rows:
            by["x_out" if w.startswith("x_out") else w].append((w, u, n, e, b))
        for tensor in sorted(by):
            w, u, n, e, b = max(by[tensor], key=lambda r: r[3] / r[4])
            top[(stage, prec)] = max(top[(stage, prec)], e / b)
            lines.append(f"{stage:4s} {what:58s} {tensor:9s} units {len(by[tensor]):3d}  max err/bar {e / b:6.3f}"
                         f"  ({w} [{u}], {n} rows: err {e:.3e}, bar {b:.3e})")

    def sig(eng, weights, L, prec, plan, cases, what):
        eng.set_precision(prec)
        try:
            for fam in sorted({c["family"] for c in cases}):
                rows, used = [], None
                for c in (c for c in cases if c["family"] == fam):
                    desc, taps, used = S.launch_sig(eng, c, plan)
                    rows += S.sig_errors(desc, taps, c, weights, L)
                emit("sig", prec, f"{weights}/L{L} {prec:6s} {what} -> {S.PLAN_NAMES[used]:15s} {fam}", rows)
        finally:
            eng.set_precision("bf16x6")

    for weights in S.WEIGHTS:
        eng = engine(weights)
        for prec in ("f32", "bf16x6"):
            eng.set_precision(prec)
            try:
                for fam in S.TAIL_FAMILIES:
                    rows = []
                    for N in S.TAIL_N:
                        c = S.tail_case(fam, N)
                        rows += [(w, f"N={N}", n, e, b) for w, _, n, e, b in S.tail_errors(S.launch_tail(eng, c), c, weights)]
                    emit("tail", prec, f"{weights} {prec:6s} {fam}", rows)
            finally:
                eng.set_precision("bf16x6")
    for weights in S.WEIGHTS:
        for L in (7, 2):
            for prec, plans in S.FORCED.items():
                for plan in plans:
                    sig(engine(weights, L), weights, L, prec, plan, S.sig_cases(), "forced")
    for counts, _ in S.DISPATCH:
        for prec in ("bf16x6", "f32"):
            sig(engine("calibrated"), "calibrated", 7, prec, -1, [S.sig_case("normal", counts)], f"{len(counts)} images, max {max(counts)}")
    for L in S.DEPTHS:
        for prec in ("bf16x6", "f32"):
            sig(engine("calibrated", L), "calibrated", L, prec, -1, [S.sig_case("normal", S.SIG_COUNTS)], "depth")
    lines.append("")
    for (stage, prec), v in sorted(top.items()):
        lines.append(f"{stage:4s} {prec:6s} largest err/bar: {v:.3f}")
    text = (f"# max |gpu - float64| / bar of the descriptive tail and the signature network run alone (linetr_debug_stage), MI355X;\n"
            f"# bar = {S.FACTOR:g} * max(max |ref32 - ref64|, 2^-23 max |ref64|), every step judged from the device's own input to it\n"
            "# written by tools/stage_unit_report.py\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
