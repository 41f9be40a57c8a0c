"""Measured error of the kernels that read and write the dense maps -- the descriptor samplers (sample_desc_kernel, sp_kp_desc_kernel)
and the SuperPoint heads (sp_desc_head_kernel, sp_score_head_kernel, NCHW and row form) -- against float64, as a fraction of the unit
tests' bar (tests/sample_cases.py: bar = 8 max(max |ref32 - ref64|, 2^-23 max |ref64|) per case, per image where a call has several).
Runs the sweeps of tests/test_gpu_sampler.py and tests/test_gpu_heads_edges.py and writes profiles/sampler_unit_errors.txt:

    python tools/sampler_unit_report.py [--out profiles/sampler_unit_errors.txt]

One line per (kernel, family, map): compared units, the largest error / bar ratio and the case it was measured on.  Families with a
'/' are exact properties, reported against a bar of 0 (a ratio of 0 means they hold): zero vectors where every tap is outside the map,
NCHW-fed against NHWC-fed results, row form against NCHW form, key-point blocks against linetr_sample_descriptors, markers."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import sample_cases as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_unit_errors.txt"))
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    torch.set_grad_enabled(False)
    eng = Engine.heads_only("cuda:0")
    lines = [f"# error / bar per kernel, family and map (tests/sample_cases.py, FACTOR = {S.FACTOR:g})"]
    bad = []
    for title, sweep in (("linetr_sample_descriptors", S.sweep_sample_descriptors), ("linetr_point_descriptors", S.sweep_point_descriptors),
                         ("linetr_prefilter_batch + linetr_tokenize", S.sweep_tokenize),
                         ("linetr_superpoint_heads / linetr_superpoint_heads_rows", S.sweep_heads)):
        rows = sweep(eng)
        lines += ["", f"## {title}: {len(rows)} units"] + S.worst_lines(rows)
        bad += S.failures(rows)
    lines += ["", f"units over their bar: {len(bad)}"] + bad
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
