"""What the host sanitizers say about the library's host code, before and after -- writes profiles/host_sanitized_findings.txt:

    python tools/host_sanitized_report.py [--parent REV] [--out profiles/host_sanitized_findings.txt] [--keep DIR]

The driver of tests/test_host_sanitized_cpu.py (tests/host_driver/host_driver.cpp) is linked twice: against linetr_amd/csrc and include/
as commit REV has them (default: HEAD~1, exported with `git archive` into a temporary directory), and against the working tree.  Every
command runs on the inputs the test writes, under AddressSanitizer + UndefinedBehaviorSanitizer and, for `threads`, under ThreadSanitizer.
The parent's build lets a UB report pass (one run lists every site, and the file says so above the list); the working tree is run with
the test's own builds, where a UB report ends the run.  A report is one line: kind, file:line of the first frame inside this project, command.  Wall times of the builds
and of the test are measured here.  CPU only: nothing runs on a device and nothing is preloaded."""
import argparse
import os
import pathlib
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_driver_build as HB  # noqa: E402
import test_host_sanitized_cpu as T  # noqa: E402

COMMANDS = ("prefilter", "pseudo", "prepare", "photo", "queries", "refusals", "malformed", "threads")


def write_inputs(command, d):
    if command == "prefilter":
        T.write_prefilter_cases(d, T.prefilter_cases())
    elif command == "pseudo":
        T.write_pseudo_cases(d)
    elif command == "prepare":
        T.write_prepare_case(d, *T.PREPARE[1])
    elif command == "photo":
        T.write_photo_cases(d)
    elif command == "queries":
        T.write_query_calls(d)


def findings(stderr, command, root):
    """[(kind, file:line, command)] of a run's standard error; `root`: where that build's sources lie"""
    out = []
    where = lambda path: os.path.relpath(path, root) if path.startswith(root) else path
    for m in re.finditer(r"^(\S+?):(\d+):\d+: runtime error: ([^\n]*)", stderr, re.M):
        kind = "signed integer overflow" if "signed integer overflow" in m.group(3) else m.group(3)[:60]
        out.append((f"UBSan {kind}", f"{where(m.group(1))}:{m.group(2)}", command))
    for m in re.finditer(r"(ERROR: AddressSanitizer|WARNING: ThreadSanitizer|ERROR: LeakSanitizer): ([^\n(]*)(.*?)(?=\n\n|\Z)", stderr, re.S):
        frame = re.search(r"#\d+ \S+ in (\S+) (%s[^\s:]*):(\d+)" % re.escape(root), m.group(3))
        out.append((f"{m.group(1).split()[-1]} {m.group(2).strip()}", f"{where(frame.group(2))}:{frame.group(3)} ({frame.group(1)})" if frame else "(no frame in this project)", command))
    m = re.search(r"terminate called after throwing an instance of '([^']*)'\s*what\(\):\s*([^\n]*)", stderr)
    if m:
        out.append((f"abort: {m.group(1)} leaves an extern \"C\" function", f"what(): {m.group(2).strip()}", command))
    return out


def run_all(exes, work, root):
    """every command under the ASan + UBSan build; threads under the TSan build too -> (findings, [(command, flavour, exit status)])"""
    found, status = [], []
    for command in COMMANDS:
        for flavour in (("asan", "tsan") if command == "threads" else ("asan",)):
            d = pathlib.Path(work) / f"{command}_{flavour}"
            d.mkdir(parents=True)
            write_inputs(command, d)
            r = subprocess.run([exes[flavour], command, str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900,
                               env={**os.environ, "LINETR_HOST_THREADS": "8"})
            status.append((command, flavour, r.returncode))
            found += findings(r.stderr, command, root)
            for line in r.stderr.splitlines():
                if line.startswith("host_driver MISMATCH"):
                    found.append(("driver check", line[len("host_driver MISMATCH: "):][:150], command))
    seen, unique = set(), []
    for f in found:
        if f not in seen:
            seen.add(f)
            unique.append(f)
    return unique, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD~1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_sanitized_findings.txt"))
    ap.add_argument("--keep", default=None, help="directory for the parent's export and objects (default: a temporary one)")
    ap.add_argument("--skip-test", action="store_true")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="host_sanitized_")
    os.makedirs(tmp, exist_ok=True)
    parent = os.path.join(tmp, "parent")
    os.makedirs(parent, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, "linetr_amd/csrc", "include"], stdout=subprocess.PIPE, check=True).stdout
    subprocess.run(["tar", "-x", "-C", parent], input=tar, check=True)
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.parent], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    lines = ["Host code under AddressSanitizer + UndefinedBehaviorSanitizer and ThreadSanitizer (tools/host_sanitized_report.py).",
             "One line per report: kind | file:line of the first frame in this project | driver command.", ""]
    times = {}
    exes_parent = {}
    for flavour, build_as in (("asan", "asan_all"), ("tsan", "tsan")):
        t0 = time.time()
        exes_parent[flavour] = HB.build(build_as, csrc=os.path.join(parent, "linetr_amd", "csrc"), out_dir=os.path.join(tmp, f"parent_{build_as}"))
        times[f"parent {build_as}"] = time.time() - t0
    found, status = run_all(exes_parent, os.path.join(tmp, "run_parent"), parent + os.sep)
    lines.append(f"== the driver linked against commit {rev} (the parent): {len(found)} reports")
    lines.append("(this run alone uses a build in which a UB report does not end the process, so that one run lists every site: `queries` therefore exits 0")
    lines.append(" below although it reports; under the test's own build, where a UB report is fatal, it stops at the first site with a non-zero status)")
    lines += [f"{k} | {w} | {c}" for k, w, c in found]
    lines.append("exit status per command: " + ", ".join(f"{c}[{f}] {s}" for c, f, s in status))
    lines.append("")
    exes = {}
    for flavour in ("asan", "tsan"):
        force = not a.skip_test                                      # a build from nothing, so that its time means something
        t0 = time.time()
        exes[flavour] = HB.build(flavour, force=force)
        times[f"working tree {flavour}" + (" (from nothing)" if force else " (incremental)")] = time.time() - t0
    found, status = run_all(exes, os.path.join(tmp, "run_head"), ROOT + os.sep)
    lines.append(f"== the driver linked against the working tree: {len(found)} reports")
    lines += [f"{k} | {w} | {c}" for k, w, c in found]
    lines.append("exit status per command: " + ", ".join(f"{c}[{f}] {s}" for c, f, s in status))
    lines.append("")
    if not a.skip_test:
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_host_sanitized_cpu.py"), "-q", "-rs"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        times["tests/test_host_sanitized_cpu.py (both builds present)"] = time.time() - t0
        lines.append("pytest tests/test_host_sanitized_cpu.py -q -rs: " + r.stdout.strip().splitlines()[-1])
    lines.append(f"wall time on this host ({os.cpu_count()} CPUs, at most {HB.MAX_JOBS} compilers at a time):")
    lines += [f"  {k}: {v:.0f} s" for k, v in times.items()]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
