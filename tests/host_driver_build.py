"""Builds tests/host_driver/host_driver.cpp against the library's translation units with the HOST side under a sanitizer, for
tests/test_host_sanitized_cpu.py and tools/host_sanitized_report.py.  A plain module: no conftest, no pytest settings.

Two flavours: "asan" (AddressSanitizer + UndefinedBehaviorSanitizer, a UB report is fatal) and "tsan" (ThreadSanitizer).  Every
linetr_amd/csrc/linetr_*.hip is compiled in full with linetr_amd.build.CFLAGS as they are plus -g and the flavour's -Xarch_host flags,
so only the host half is instrumented: the device code objects are what the product ships, nothing is preloaded, and the executable
carries its sanitizer's runtime itself.  Objects go to linetr_amd/csrc/build/san_<flavour>/ and are recompiled only when a file they
include changed (hipcc's -MD files, as linetr_amd/build.py does); at most 16 compilers run at a time.

`csrc` may name another checkout's linetr_amd/csrc (the report links the same driver against the parent commit's sources); its objects
go to `out_dir`."""
from __future__ import annotations

import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from linetr_amd import build as LB  # noqa: E402

DRIVER = os.path.join(ROOT, "tests", "host_driver", "host_driver.cpp")
FLAVOURS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
    "tsan": ["-fsanitize=thread"],
    # for the findings report alone: UB reports do not end the run, so one run lists every site
    "asan_all": ["-fsanitize=address,undefined"],
}
MAX_JOBS = 16


def san_dir(flavour):
    return os.path.join(LB.OBJ, f"san_{flavour}")


def _host_flags(flavour):
    out = []
    for f in FLAVOURS[flavour]:
        out += ["-Xarch_host", f]
    return out


def _cxx(hipcc):
    """the clang++ that hipcc drives (hipcc itself compiles every source as HIP)"""
    real = os.path.dirname(os.path.realpath(hipcc))
    for cand in (os.path.join(real, "amdclang++"), os.path.join(real, "..", "lib", "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("no clang++ beside " + hipcc)


def _stale(obj, dfile, base):
    if not os.path.exists(obj):
        return True
    deps = LB._deps(dfile)
    if deps is None:
        return True
    t = os.path.getmtime(obj)
    for d in deps:
        p = d if os.path.isabs(d) else os.path.join(base, d)
        if not os.path.exists(p) or os.path.getmtime(p) > t:
            return True
    return False


def build(flavour, csrc=None, out_dir=None, verbose=False, force=False):
    """-> path of the sanitized driver executable"""
    csrc = os.path.abspath(csrc or LB.CSRC)
    out_dir = os.path.abspath(out_dir or san_dir(flavour))
    os.makedirs(out_dir, exist_ok=True)
    hipcc = LB._hipcc()
    include = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    flags = [*LB.CFLAGS, "-g", *_host_flags(flavour)]
    units = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith("linetr_") and f.endswith(".hip"))
    jobs, objs = [], []
    for src in [*units, DRIVER]:
        stem = os.path.splitext(os.path.basename(src))[0]
        obj = os.path.join(out_dir, stem + ".o")
        dfile = obj[:-2] + ".d"
        objs.append(obj)
        if force or _stale(obj, dfile, os.path.dirname(src)):
            if src == DRIVER:       # plain C++ over the C ABI: the toolchain's clang++, no device pass; the same sanitizer, given directly
                jobs.append([_cxx(hipcc), "-O1", "-g", "-std=c++17", "-Wall", *FLAVOURS[flavour], "-I", include, "-MD", "-MF", dfile, "-c", src, "-o", obj])
            else:
                jobs.append([hipcc, *flags, "-MD", "-MF", dfile, "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, cwd=os.path.dirname(cmd[-3]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stdout[-4000:]))

    exe = os.path.join(out_dir, "host_driver")
    if jobs or not os.path.exists(exe):
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), MAX_JOBS))) as ex:
            list(ex.map(run, jobs))
        link = [hipcc, "--offload-arch=gfx950", *FLAVOURS[flavour], "-pthread", "-o", exe, *objs, "-ldl"]
        if verbose:
            print(" ".join(link), flush=True)
        r = subprocess.run(link, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise RuntimeError("%s\n%s" % (" ".join(link), r.stdout[-4000:]))
    return exe


if __name__ == "__main__":
    for fl in (sys.argv[1:] or ["asan", "tsan"]):
        t0 = time.time()
        print(build(fl, verbose=True), "%.0f s" % (time.time() - t0))
