"""Measured error of the front-end kernels -- the token MLP's launches and the CLS-pooling kernels -- against float64, as a fraction
of the unit tests' bar (tests/front_cases.py: bar = 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per 64-row tile / per sub-line,
vector columns and p_0 separately).  Runs the cases of tests/test_gpu_front.py through linetr_debug_tok_mlp / linetr_debug_cls_pool
and writes profiles/front_unit_errors.txt:

    python tools/front_unit_report.py [--out profiles/front_unit_errors.txt]

One line per (kernel, family): compared units, the largest error / bar ratio and the case it was measured on; then which families'
bar includes the kernel-order float32 reference (front_cases.KERNEL_ORDER)."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import front_cases as FC  # noqa: E402
from attn_cases import state_dict_t  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "front_unit_errors.txt"))
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    engines = {w: Engine(state_dict_t(w)[0], "cuda:0") for w in FC.WEIGHTS}
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    stat = collections.OrderedDict()          # (kernel, family, column) -> [units, worst ratio, where]

    def note(kernel, family, col, rows, where):
        s = stat.setdefault((kernel, family, col), [0, 0.0, ""])
        for r in rows:
            s[0] += 1
            ratio = r[2] / r[3] if r[3] else float("inf")
            if ratio >= s[1]:
                s[1], s[2] = ratio, f"{where}, unit {r[0]}: err {r[2]:.3e}, bar {r[3]:.3e}"

    for family in FC.MLP_FAMILIES:
        for w in FC.WEIGHTS:
            for variant, enc in ((0, "word"), (1, "line")):
                for mb, rows in [(0, r) for r in FC.MLP_ROWS] + list(FC.MLP_WALK) + [(0, 64 * cu + 1)]:
                    case = FC.mlp_case(enc, w, family, rows)
                    got, used = FC.launch_mlp(engines[w], variant, **{enc: case}, max_blocks=mb)
                    note(FC.VARIANTS[used], family, "tile", FC.tile_errors(got[enc], case), f"{w} rows {rows} max_blocks {mb}")
            pairs = [(2, 0, p) for p in FC.DUAL_PAIRS] + [(3, 0, p) for p in FC.DUAL_PAIRS]
            pairs += [(3, mb, p) for mb in (1, 2, 3) for p in ((193, 449), (449, 64), (65, 321))]
            pairs += [(4, 0, (r, r)) for r in (1, 65, 257, 4378)]
            for variant, mb, (rw, rl) in pairs:
                word, line = FC.mlp_case("word", w, family, rw), FC.mlp_case("line", w, family, rl)
                got, used = FC.launch_mlp(engines[w], variant, word, line, mb)
                for enc, case in (("word", word), ("line", line)):
                    note(FC.VARIANTS[used], family, "tile", FC.tile_errors(got[enc], case), f"{w} {enc} rows {rw}+{rl} max_blocks {mb}")
    for family in FC.POOL_FAMILIES:
        variants = {"sentinel": [dict(parity=0), dict(parity=1)], "border": [dict(align_corners=False), dict(align_corners=True)]}
        for i, s in enumerate(FC.pool_shapes()):
            for w in FC.WEIGHTS if i % 4 == 0 else FC.WEIGHTS[:1]:
                for kw in variants.get(family, [dict()]):
                    case = FC.pool_case(family, *s, weights=w, **kw)
                    for kernel in (0, 1, 2, 3):
                        got, used = FC.launch_pool(engines[w], kernel, case)
                        rows = FC.subline_errors(got, case)
                        for col in ("vec", "p0", "zeros"):
                            note(FC.POOL_KERNELS[used], family, col, [r for r in rows if r[1] == col], f"{w} T {s[0]} N {s[1]} images {s[2]}")
    for m in FC.MAPS:
        for n_img in (1, 3):
            case = FC.pool_case("normal", 21, 33, n_img, hw_cells=m)
            got, _ = FC.launch_pool(engines["calibrated"], 3, case, nhwc=False)
            rows = FC.subline_errors(got, case)
            for col in ("vec", "p0"):
                note("nchw_to_nhwc + split4", "normal", col, [r for r in rows if r[1] == col], f"map {m[0]}x{m[1]} images {n_img}")
    lines = [f"{k:26s} {f:9s} {c:5s} units {s[0]:6d}  max err/bar {s[1]:6.3f}  ({s[2]})" for (k, f, c), s in stat.items() if s[0]]
    order = sorted(FC.KERNEL_ORDER)
    lines += ["", "families whose bar includes the kernel-order float32 reference (front_cases.KERNEL_ORDER): "
              + (", ".join(f"{k}/{f}" for k, f in order) if order else "none")]
    text = (f"# max |gpu - float64| / bar per front-end kernel and input family; bar = {FC.FACTOR:g} * max(max |ref32 - ref64|, 2^-23 max |ref64|)\n"
            "# per 64-row tile (token MLP) / per sub-line, vector columns and p_0 separately (CLS pooling)\n"
            "# written by tools/front_unit_report.py\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
