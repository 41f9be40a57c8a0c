"""Gates and measurements of the ragged describe path (linetr_prefilter_ragged / linetr_describe_ragged, Engine.describe_ragged,
Matching.forward / forward_batch on images of different sizes):

    python tools/ragged_describe_report.py --isa PARENT_TREE      CPU only: writes profiles/ragged_describe_isa.txt
    python tools/ragged_describe_report.py [--iters 5]            on the GPU: profiles/ragged_describe_errors.txt and _bench.txt

ISA gate: tools/kernel_isa_diff.py of PARENT_TREE (a checkout of the parent commit) against this tree; the kernels the uniform entry
points launch are expected unchanged, and every one that is not is named in the file.
Errors: every case of tests/test_gpu_describe_ragged.py (cases and bars: tests/ragged_cases.py), as error / bar or as a count of
differing elements -- the lines the tests print, and their verdict.
Time, ms per call, median of 5 alternating windows of `iters` calls between two device synchronisations, same GPU, same process:
  (a) 32 pairs alternating 480 x 640 / 960 x 1280 (64 images, each with the reference's auto_min_length values of its shape) through ONE
      Engine.describe_ragged call, against linetr_describe image by image on the same records and maps (the only route without it);
  (b) 64 equal 480 x 640 pairs (128 images) through Engine.describe_ragged against one Engine.describe call;
  (c) Matching.forward on tests/golden/mixed_size_pair.npz: the fused ragged call against the per-image path it took before (the path
      this tree still takes when the fused call declines; forced here by making it decline).
No time is fixed in advance."""
import argparse
import contextlib
import io
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

UNIFORM_KERNELS = ("line_fill_kernel", "tokenize_kernel", "nchw_to_nhwc_kernel", "sample_desc_kernel", "cls_pool_online_kernel")


def isa(parent, out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_isa_diff.py"), parent, ROOT], capture_output=True, text=True)
    names = subprocess.run(["c++filt"], input=r.stdout, capture_output=True, text=True).stdout
    moved = sorted({k for line in names.split("\n") if line.startswith("  differs:") for k in UNIFORM_KERNELS if k in line})
    # what the compiler made of every kernel that moved, parent -> tree (product build)
    import re
    import kernel_isa_diff as K
    (a, _), (b, _) = K.tree_kernels(parent, False), K.tree_kernels(ROOT, False)
    meta = lambda t, f: re.search(r"\.%s:\s+(\S+)" % f, t).group(1)
    instr = lambda t: sum(1 for ln in t.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))
    res = []
    for sym in sorted(k for k in set(a) & set(b) if a[k] != b[k]):
        dem = subprocess.run(["c++filt", sym.split(":")[-1]], capture_output=True, text=True).stdout.strip().split("(")[0]
        res.append(f"  {dem}: " + ", ".join(f"{f} {meta(a[sym], f)} -> {meta(b[sym], f)}" for f in
                                         ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"))
                   + f", instructions {instr(a[sym])} -> {instr(b[sym])}")
    text = ("# tools/kernel_isa_diff.py of the parent commit against this tree (symbols demangled); exit status " + str(r.returncode) + "\n"
            "# 'one side': the new ragged kernels.  'differs': a kernel both trees have whose text is not the same.\n"
            "# kernels of the uniform entry points (linetr_tokenize / linetr_describe) whose instructions moved: "
            + (", ".join(moved) if moved else "none") + "\n" + names + r.stderr
            + "# resources of the kernels that differ, parent -> tree\n" + "\n".join(res) + "\n")
    with open(os.path.join(out_dir, "ragged_describe_isa.txt"), "w") as f:
        f.write(text)
    print(text)


def errors(eng):
    import torch
    import pytest
    import test_gpu_describe_ragged as T
    mp = pytest.MonkeyPatch()
    cases = [(f"equal sizes, 3 x (64 x 96), {'NHWC' if n else 'NCHW'}, align_corners {a}: every output against linetr_describe",
              lambda n=n, a=a: T.test_equal_sizes_equal_linetr_describe_bit_for_bit(eng, n, a)) for n in (False, True) for a in (0, 1)]
    cases += [(f"{name}, {'NHWC' if n else 'NCHW'}: against linetr_describe image by image",
               lambda ids=ids, n=n: T.test_ragged_equals_linetr_describe_image_by_image(eng, ids, n))
              for name, ids in (("B = 1", (3,)), ("B = 2", (1, 5)), ("B = 9", tuple(range(9)))) for n in (False, True)]
    cases += [("above 2048 sub-lines (one wave per sub-line), NHWC, align_corners 1", lambda: T.test_many_sub_lines_take_the_one_wave_per_sub_line_kernel(eng))]
    cases += [(f"the nine images against the oracle, {'NHWC' if n else 'NCHW'}", lambda n=n: T.test_against_the_oracle_through_the_engine(eng, n)) for n in (False, True)]
    cases += [("Matching.forward_batch, golden pair + the pair swapped", T.test_forward_batch_of_mixed_sizes_against_the_real_reference),
              ("Matching.forward, golden pair, fused", lambda: T.test_forward_of_a_mixed_size_pair_takes_the_fused_path(mp)),
              ("refusals", lambda: T.test_refusals_leave_everything_untouched(eng)),
              ("two calls, same bytes", lambda: T.test_two_calls_give_the_same_bytes(eng))]
    lines = []
    for name, fn in cases:
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                fn()
            verdict = "every assertion holds (token tensors: 0 differing elements)"
        except AssertionError as e:
            verdict = f"FAILS: {e}"
        finally:
            mp.undo()
        lines.append(f"{name}: {verdict}")
        lines += ["    " + ln for ln in buf.getvalue().split("\n") if ln.strip()]
    return ("# every case of tests/test_gpu_describe_ragged.py; tokeniser tensors as counts of differing elements, descriptors as error / bar\n"
            "# (tests/ragged_cases.py); written by tools/ragged_describe_report.py on " + torch.cuda.get_device_name(0) + "\n" + "\n".join(lines) + "\n")


def bench(eng, iters):
    import numpy as np
    import torch
    import ragged_cases as rc
    from helpers import load
    from sig_attn_bwd_report import compare
    from workloads import synth
    T = 21
    sizes = {(480, 640): (8.0, 16.0), (960, 1280): (16.0, 32.0)}
    base = {hw: [tuple(torch.from_numpy(m).cuda() for m in synth.synth_dense_maps_np(1200 + i, *hw)) for i in range(2)] for hw in sizes}

    def batch(shapes):
        rows = [synth.synth_lines(1300 + i, 200, *hw) for i, hw in enumerate(shapes)]
        maps = [base[hw][i % 2] for i, hw in enumerate(shapes)]
        kw = dict(remove_borders=8, max_keylines=-1, max_tokens=T)
        recs, cu_k, cu_n = eng.prefilter_ragged(rows, shapes, min_length=[sizes[hw][1] for hw in shapes], token_distance=[sizes[hw][0] for hw in shapes], **kw)
        recs = recs.copy()
        dds, dss, tds = [m[0][0] for m in maps], [m[1][0] for m in maps], [sizes[hw][0] for hw in shapes]
        ragged = lambda: eng.describe_ragged(recs, cu_k, cu_n, dds, dss, token_distance=tds, max_tokens=T)
        per = []
        for i, hw in enumerate(shapes):
            r, ck, cn = eng.prefilter([rows[i]], *hw, min_length=sizes[hw][1], token_distance=sizes[hw][0], **kw)
            per.append((r.copy(), ck, cn, maps[i][0], maps[i][1], sizes[hw][0]))
        by_image = lambda: [eng.describe(r, ck, cn, dd, ds, token_distance=td, max_tokens=T) for r, ck, cn, dd, ds, td in per]
        return recs, cu_k, cu_n, ragged, by_image, maps

    out = []
    # (a)
    shapes = [hw for _ in range(32) for hw in sizes]
    recs, cu_k, cu_n, ragged, by_image, _ = batch(shapes)
    ld = ragged()[1]
    err = max(float((ld[int(cu_n[i]):int(cu_n[i + 1])] - one[1]).abs().max()) for i, one in enumerate(by_image()))
    (a, a0, a1), (b, b0, b1) = compare((ragged, by_image), iters)
    out.append(f"(a) 32 pairs of 480 x 640 + 960 x 1280, {int(cu_k[-1])} key-lines, {int(cu_n[-1])} sub-lines, NCHW maps, records on the host\n"
               f"    Engine.describe_ragged, one call for the 64 images            {a:9.3f} ms  [{a0:.3f} .. {a1:.3f}]\n"
               f"    Engine.describe image by image (64 calls)                     {b:9.3f} ms  [{b0:.3f} .. {b1:.3f}]   image by image / ragged {b / a:.2f}\n"
               f"    max |line_desc ragged - image by image| {err:.2e} / {rc.DESC_BATCH_BAR:.0e}")
    # (b)
    shapes = [(480, 640)] * 128
    recs, cu_k, cu_n, ragged, _, maps = batch(shapes)
    dd, ds = torch.cat([m[0] for m in maps]), torch.cat([m[1] for m in maps])
    uniform = lambda: eng.describe(recs, cu_k, cu_n, dd, ds, token_distance=8.0, max_tokens=T)
    same = torch.equal(ragged()[1], uniform()[1])
    (a, a0, a1), (b, b0, b1) = compare((ragged, uniform), iters)
    inside = "inside" if b0 <= a <= b1 else "OUTSIDE"
    out.append(f"(b) 64 equal pairs of 480 x 640, {int(cu_k[-1])} key-lines, {int(cu_n[-1])} sub-lines, NCHW maps, records on the host\n"
               f"    Engine.describe_ragged                                        {a:9.3f} ms  [{a0:.3f} .. {a1:.3f}]\n"
               f"    Engine.describe (linetr_describe)                             {b:9.3f} ms  [{b0:.3f} .. {b1:.3f}]   ragged / uniform {a / b:.3f}: "
               f"the ragged median lies {inside} the min .. max of linetr_describe's own windows\n"
               f"    line_desc of the two calls bit-identical: {same}")
    # (c)
    import test_gpu_describe_ragged as TT
    from models.matching import Matching
    g = load("mixed_size_pair")
    imgs = {s: torch.zeros(1, 1, *(int(v) for v in g["hw" + s]), device="cuda") for s in "01"}
    mt = TT.matching(g)
    seeds, sets = [int(g["map_seed0"]), int(g["map_seed1"])], [g["lines0"], g["lines1"]]
    sp_maps = {}

    class CachedSuperPoint(rc.FakeSuperPoint):          # the maps are made once: the timed call is the line branch and the matchers
        def __call__(self, data):
            key = tuple(data["image"].shape)
            if key not in sp_maps:
                self.seeds = [seeds[0 if key[-1] == int(g["hw0"][1]) else 1]]
                sp_maps[key] = rc.FakeSuperPoint.__call__(self, data)
            return sp_maps[key]

    class CyclicLSD:
        i = 0

        def detect_torch(self, image):
            CyclicLSD.i += 1
            return synth.array_to_keylines(sets[(CyclicLSD.i - 1) % 2])
    mt.superpoint, mt.lsd = CachedSuperPoint([]), CyclicLSD()
    pair = lambda: mt({"image0": imgs["0"], "image1": imgs["1"]})
    fused_path = Matching._describe_fused_ragged

    def per_image_path():
        Matching._describe_fused_ragged = lambda self, *a: None
        try:
            return pair()
        finally:
            Matching._describe_fused_ragged = fused_path
    same = np.array_equal(pair()["matches_l"].numpy(), per_image_path()["matches_l"].numpy())
    (a, a0, a1), (b, b0, b1) = compare((pair, per_image_path), iters * 4)
    out.append(f"(c) Matching.forward on tests/golden/mixed_size_pair.npz (480 x 640 + 960 x 1280; dense maps cached, detector rows given)\n"
               f"    fused: linetr_prefilter_ragged + linetr_describe_ragged       {a:9.3f} ms  [{a0:.3f} .. {a1:.3f}]\n"
               f"    image by image (the path taken before; fused call declined)   {b:9.3f} ms  [{b0:.3f} .. {b1:.3f}]   image by image / fused {b / a:.2f}\n"
               f"    matches_l of the two paths identical: {same}")
    return (f"# ms per call, median of 5 alternating windows of {iters} calls ((c): {iters * 4}) between two device synchronisations (min .. max of the\n"
            f"# windows in brackets); same GPU, same process; written by tools/ragged_describe_report.py on {torch.cuda.get_device_name(0)}\n" + "\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--isa", metavar="PARENT_TREE")
    ap.add_argument("--only", choices=("errors", "bench"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.isa:
        return isa(args.isa, args.out_dir)
    import torch
    from linetr_amd.engine import Engine
    from workloads import synth
    torch.set_grad_enabled(False)
    eng = Engine(synth.calibrated_state_dict(), "cuda:0")
    for name, make in (("errors", lambda: errors(eng)), ("bench", lambda: bench(eng, args.iters))):
        if args.only in (None, name):
            text = make()
            with open(os.path.join(args.out_dir, f"ragged_describe_{name}.txt"), "w") as f:
                f.write(text)
            print(text)


if __name__ == "__main__":
    main()
