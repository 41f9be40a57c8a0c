"""Measured error of the matcher's kernels against float64 (tests/match_cases.py: the cases of tests/test_gpu_match_kernels.py, run
through linetr_debug_match) -- writes profiles/match_unit_errors.txt:

    python tools/match_unit_report.py [--out profiles/match_unit_errors.txt]

One line per (path, family): compared pairs, the largest error and its reference bar (8 max(max |ref32 - ref64|, 2^-23 max |Dk|)), the
largest error / bar ratio, the largest error / forward bound ratio over all entries, and the case the bar ratio was measured on.
The exact families must show error 0."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import match_cases as MC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_unit_errors.txt"))
    args = ap.parse_args()
    from linetr_amd.engine import Engine
    eng = Engine.heads_only("cuda:0")
    stat = collections.OrderedDict()          # (path, family) -> [pairs, max err, its bar, worst err / bar, worst err / bound, where]

    def note(name, case, res, **force):
        s = stat.setdefault((name, case["family"]), [0, 0.0, 0.0, 0.0, 0.0, ""])
        for i in case["check"]:
            err, bar, rb = MC.measure(MC.case_reference(case, i), res[i][0])
            s[0] += 1
            s[4] = max(s[4], rb)
            if bar and err / bar >= s[3]:
                s[1], s[2], s[3], s[5] = err, bar, err / bar, f"{case['name']} pair {i}" + (f" {force}" if force else "")

    def run(name, case, path, **force):
        ln = MC.Launcher(eng, case)
        thr, mutual = MC.case_thresholds(case)[0]
        res, used = ln.run(path, thr, mutual, **force)
        assert used == path
        note(name, case, res, **force)

    for family in MC.FAMILIES:
        for case in MC.single_cases(family):
            for path in MC.legal_paths(case):
                run(MC.PATHS[path], case, path)
        for case in MC.pool_forced_cases(family):
            for sg in (0, 1):
                for cd in (0, 1):
                    run(f"three_launch seg1_global={sg} cache_dk={cd}", case, 0, seg1_global=sg, cache_dk=cd)
        for P, dt in ((8, -1), (9, -1), (2, 1)):
            for variant in (0, 1):
                run(f"three_launch batch P={P}" + (" device table forced" if dt == 1 else ""), MC.batch_case(family, P, variant), 0, device_table=dt)
    lines = [f"{k:52s} {f:13s} pairs {s[0]:4d}  max err {s[1]:.3e}  bar {s[2]:.3e}  err/bar {s[3]:5.3f}  max err/forward bound {s[4]:6.4f}  ({s[5]})"
             for (k, f), s in stat.items()]
    text = (f"# max |gpu - float64| of Dk per matcher path and input family; bar = {MC.FACTOR:g} * max(max |ref32 - ref64|, 2^-23 max |Dk|) per pair;\n"
            "# forward bound per entry: 2 * 256 * 2^-24 (|a|.|b|) + 4 * 2^-24 pooled like Dk, + (s0 + s1 + 2) * 2^-24 * 4 (tests/match_cases.py)\n"
            "# written by tools/match_unit_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
