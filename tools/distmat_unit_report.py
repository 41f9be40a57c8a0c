"""Measured error of the entry points that take an existing distance matrix against float64 (tests/distmat_cases.py: the cases of
tests/test_gpu_distmat.py, run through the C ABI) -- writes profiles/distmat_unit_errors.txt:

    python tools/distmat_unit_report.py [--out profiles/distmat_unit_errors.txt]

One line per (entry point, family): cases, the largest error and its reference bar (8 x the error of NumPy's own float32 product on the
case), the largest error / bar ratio, the largest error / entry-wise bound ratio over all entries, and the case the bar ratio was
measured on; the matcher lines count the rows that differ from the rules.  The exact families must show error 0 / 0 rows."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import distmat_cases as DC  # noqa: E402
from match_cases import pool_matrix  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distmat_unit_errors.txt"))
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    raw = DC.Raw(Engine.heads_only("cuda:0"))
    stat = collections.OrderedDict()          # (entry point, family) -> [cases, max err, its bar, worst err / bar, worst err / bound, where]
    lines = []

    def note(entry, family, name, ref, dk):
        s = stat.setdefault((entry, family), [0, 0.0, 0.0, 0.0, 0.0, ""])
        fin = np.isfinite(ref["ref64"])
        err = np.abs(dk.astype(np.float64) - ref["ref64"])[fin]
        s[0] += 1
        if not err.size:
            return
        s[4] = max(s[4], float((err / np.maximum(ref["bound"][fin], 1e-300)).max()))
        ratio = err.max() / ref["bar"] if ref["bar"] else (0.0 if err.max() == 0 else float("inf"))
        if ratio >= s[3]:
            s[1], s[2], s[3], s[5] = float(err.max()), ref["bar"], ratio, name

    for dtype in ("f32", "f64"):
        for mutual in (True, False):
            rows = bad = 0
            for c in DC.match_cases(dtype):
                _, m01, _ = raw.match(c["d"], c["thr"], mutual)
                rows += len(m01)
                bad += int((m01 != DC.match_want(c, mutual)).sum())
            entry = "linetr_match_distmat" + ("_f64" if dtype == "f64" else "")
            lines.append(f"{entry:44s} {'mutual' if mutual else 'one-way':13s} cases {len(DC.match_cases(dtype)):4d}  rows {rows:5d}  rows that differ from the rules {bad}")
    for family in ("exact", "normal"):
        for p in DC.pool_cases(family):
            _, dk, _ = raw.pool(p["D"], p["s0"], p["k0"], p["s1"], p["k1"])
            note("linetr_pool_distmat", family, p["name"], DC.pool_reference(family, p["c0"], p["c1"]), dk)
    for c0, c1 in DC.tokeniser_shapes():
        p = DC.pool_case("normal", c0, c1)
        _, dk, word, _ = raw.dense(p["D"], pool_matrix(c0, np.float32), pool_matrix(c1, np.float32))
        note("linetr_pool_distmat_dense", f"tokeniser (verdict {word})", p["name"], DC.pool_reference("normal", c0, c1), dk)
    for side in (0, 1):
        for name in DC.mutation_names():
            c = DC.dense_mutation_case(side, name)
            _, dk, word, _ = raw.dense(c["D"], c["A0"], c["A1"])
            note("linetr_pool_distmat_dense", f"mutated A{side}", c["name"] + f" (verdict {word})", c, dk)
    for c in DC.as_given_cases():
        _, dk, word, _ = raw.dense(c["D"], c["A0"], c["A1"])
        note("linetr_pool_distmat_dense", "as given", c["name"] + f" (verdict {word})", c, dk)
    lines += [f"{k:44s} {f:22s} cases {s[0]:4d}  max err {s[1]:.3e}  bar {s[2]:.3e}  err/bar {s[3]:5.3f}  max err/entry-wise bound {s[4]:6.4f}  ({s[5]})"
              for (k, f), s in stat.items()]
    text = (f"# max |gpu - float64| per entry point and family; bar = {DC.FACTOR:g} x max |NumPy float32 product - float64| per case;\n"
            "# entry-wise bound: (s0 + s1 + 2) 2^-24 max|D| over the entry's segment (pooled), (n0 + n1 + 2) 2^-24 (|A0| |D| |A1|^T) (as given)\n"
            "# (tests/distmat_cases.py); written by tools/distmat_unit_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
