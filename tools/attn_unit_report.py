"""Measured error of every signature-attention kernel against float64, as a fraction of the unit tests' bar
(tests/attn_cases.py: bar = 8 max(max |ref32 - ref64|, 2^-23 max |v|) per image).  Runs the cases of tests/test_gpu_attention.py
through linetr_debug_sig_attention and writes profiles/attn_unit_errors.txt:

    python tools/attn_unit_report.py [--out profiles/attn_unit_errors.txt]

One line per (kernel, batch shape, input family): compared images, the largest error / bar ratio and the image it was measured
on; then per kernel the number of (count, family) cases and the largest ratio overall."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import attn_cases as A  # noqa: E402

SEED_WEIGHTS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_unit_errors.txt"))
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    engines = {w: Engine(A.state_dict_t(w)[0], "cuda:0") for w in ("calibrated", SEED_WEIGHTS)}
    eng = engines["calibrated"]
    lines, cases, worst = [], collections.Counter(), collections.defaultdict(float)

    def run(e, kernel, shape, family, case, ld=768):
        gpu, used = A.launch(e, kernel, case, ld)
        rows = A.image_errors(gpu, case)
        if not rows:
            return None
        i, n, err, bar = max(rows, key=lambda r: r[2] / r[3])
        cases[used] += len(rows)
        worst[used] = max(worst[used], err / bar)
        return used, shape, family, len(rows), err / bar, n, err, bar

    def emit(rs):
        rs = [r for r in rs if r]
        if not rs:
            return
        used, shape, family = rs[0][:3]
        best = max(rs, key=lambda r: r[4])
        lines.append(f"{A.KERNELS[used]:16s} {shape:22s} {family:10s} images {sum(r[3] for r in rs):4d}  max err/bar {best[4]:6.3f}"
                     f"  (n = {best[5]}: err {best[6]:.3e}, bar {best[7]:.3e})")

    par = lambda f: (0, 1) if f == "sentinel" else (0,)
    for kernel in (0, 1, 2, 3):
        for family in A.FAMILIES:
            emit([run(eng, kernel, "ragged", family, A.qkv_case(family, A.ragged_counts(kernel), parity=p)) for p in par(family)])
        for family in ("normal", "planted"):
            emit([run(eng, kernel, "one image alone", family, A.qkv_case(family, (n,))) for n in A.counts_for(kernel)])
    for family in A.FAMILIES:
        emit([run(eng, 1, "ragged, row stride 1024", family, A.qkv_case(family, A.ragged_counts(1), parity=p), ld=1024)
              for p in par(family)])
    emit([run(eng, -1, "16 x 599 (dispatcher)", "normal", A.qkv_case("normal", (599,) * 16))])
    for weights in ("calibrated", SEED_WEIGHTS):
        for layer in (0, 6):
            for family in A.Z_FAMILIES:
                emit([run(engines[weights], 4, f"ragged, {weights}/L{layer}", family,
                          A.z_case(family, A.ragged_counts(4), weights, layer, parity=p)) for p in par(family)])
    for weights, layer in (("calibrated", 0), (SEED_WEIGHTS, 6)):
        emit([run(engines[weights], 4, f"alone, {weights}/L{layer}", "normal", A.z_case("normal", (n,), weights, layer))
              for n in A.counts_for(4)])
    emit([run(eng, -1, "64 x 199 (dispatcher)", "normal", A.z_case("normal", (199,) * 64, "calibrated", 0))])
    lines.append("")
    for k in sorted(cases):
        lines.append(f"{A.KERNELS[k]:16s} (count, family) cases compared: {cases[k]:4d}   largest err/bar: {worst[k]:.3f}")
    text = (f"# max |gpu - float64| / bar per signature-attention kernel; bar = {A.FACTOR:g} * max(max |ref32 - ref64|, 2^-23 max |v|) per image\n"
            "# written by tools/attn_unit_report.py\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
