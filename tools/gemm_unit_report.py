"""Measured error of every GEMM tile against float64, as a fraction of the unit tests' bar (tests/gemm_cases.py), and the number of
bit mismatches of the `exact` / `onehot` families, which must be 0.  Runs the shape grids of tests/test_gpu_gemm_tiles.py through
linetr_debug_gemm_case and writes profiles/gemm_unit_errors.txt:

    python tools/gemm_unit_report.py [--out profiles/gemm_unit_errors.txt]

One line per (precision mode, tile, family): cases, the largest error / bar ratio and the shape it was measured on."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import gemm_cases as G  # noqa: E402

EPILOGUES = [(0, False), (1, True), (3, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_unit_errors.txt"))
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    from workloads import synth
    eng = Engine(synth.make_state_dict(0), "cuda:0")
    lines, total_bad, worst_all = [], 0, 0.0
    for mode in G.MODES:
        eng.set_precision(mode)
        for tile in G.tiles_of(mode) + ((G.WS,) if mode == "bf16x6" else ()):
            ws = tile == G.WS
            n_exact = bad = 0
            for M, N, K in G.shape_grid(tile, mode):
                for family in ("exact", "onehot"):
                    p = G.problem(family, M, N, K)
                    for act, res in (EPILOGUES if not ws else [(0, False), (1, False)]):
                        for strided in (False, True):
                            Y, used = G.launch(eng, p, tile, act=act, residual=res, strided=strided)
                            assert used == tile, (used, tile)
                            bad += G.mismatches(Y, G.references(p, act, res)[0])[0]
                            n_exact += 1
            total_bad += bad
            lines.append(f"{mode:7s} {tile:9s} exact+onehot cases {n_exact:4d}  elements that differ from float64: {bad}")
            for family in ("normal", "sentinel"):
                worst, n = (0.0, None, 0.0, 0.0), 0
                for M, N, K in G.shape_grid(tile, mode):
                    p = G.problem(family, M, N, K)
                    for act in ((0, 1) if ws else (0, 1, 2, 3)):
                        Y, used = G.launch(eng, p, tile, act=act, residual=not ws, strided=family == "sentinel")
                        r64, r32 = G.references(p, act, not ws)
                        err, bar = (Y.double() - r64).abs().max().item(), G.bar(mode, r64, r32)
                        n += 1
                        if err / bar >= worst[0]:
                            worst = (err / bar, (M, N, K, act), err, bar)
                worst_all = max(worst_all, worst[0])
                lines.append(f"{mode:7s} {tile:9s} {family:8s}     cases {n:4d}  max err/bar {worst[0]:6.3f}  (M, N, K, act = {worst[1]}: "
                             f"err {worst[2]:.3e}, bar {worst[3]:.3e})")
    lines += ["", f"exact / onehot elements that differ from float64, all tiles and modes: {total_bad}", f"largest err/bar: {worst_all:.3f}"]
    text = (f"# GEMM tiles alone against float64.  bar: f32 / bf16x6 {G.FACTOR:g} * max(max |ref32 - ref64|, 2^-23 max |ref64|) per case; "
            f"f16x3 {G.TWO_PLANE_TOL['f16x3']:g}, bf16x3 {G.TWO_PLANE_TOL['bf16x3']:g} of max |ref64|\n"
            "# written by tools/gemm_unit_report.py\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
