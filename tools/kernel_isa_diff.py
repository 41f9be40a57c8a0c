"""Do two source trees compile to the same kernels?  The gate of a refactor that must not move an instruction (no GPU needed).
    python tools/kernel_isa_diff.py PARENT_TREE HEAD_TREE [-v]
Both trees are compiled with tools/resource_table.py's compile step, once as the product (linetr_amd/csrc/linetr_*.hip) and once as
the experiments build (-DLINETR_EXPERIMENTS, experiments/csrc/linetr_*.hip included).  Per kernel symbol it compares the text from the
kernel's label to .end_amdhsa_kernel and the kernel's metadata entry, and per device function that was not inlined its text, with
comments, the numbers of local labels (renumbered in order of appearance) and the per-compile __hip_cuid symbol masked.  Prints one line per build and the symbols that differ or exist on one side
only (-v: a unified diff of each differing kernel); exit status 1 if there are any.  A symbol that changed translation unit is compared all
the same and listed as moved.  profiles/*_refactor_isa.txt record its results."""
import difflib
import re
import sys

from resource_table import compile_asm


def _mask(text):
    text = re.sub(r"\s*;.*", "", text)
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid", text)
    labels = {}
    text = re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), text)
    return "\n".join(ln.rstrip() for ln in text.split("\n") if ln.strip())


def kernels(asm):
    """{symbol: masked text} of one translation unit's device assembly: every kernel (its text and its metadata entry) and, under
    "fn:" + symbol, every device function that was not inlined (a kernel's own text does not contain the text of what it calls)"""
    meta = {re.search(r"\.name:\s+(\S+)", it).group(1): it
            for it in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", asm, flags=re.S)}
    out = {}
    for sym in re.findall(r"^\s*\.type\s+(\S+),@function", asm, flags=re.M):
        end = r"^\s*\.end_amdhsa_kernel" if sym in meta else r"^\.Lfunc_end\d+:"
        m = re.search(r"^%s:.*?%s" % (re.escape(sym), end), asm, flags=re.S | re.M)
        if m is None:
            raise RuntimeError("no text for " + sym)
        out[sym if sym in meta else "fn:" + sym] = _mask(m.group(0) + "\n" + meta.get(sym, ""))
    if set(meta) - set(out):
        raise RuntimeError("kernels without text: " + ", ".join(sorted(set(meta) - set(out))))
    return out


def tree_kernels(root, experiments):
    """({key: masked text}, {symbol: its unit(s)}) of a tree.  A symbol with ONE text in the tree -- it exists in one translation unit,
    or several units instantiate the same template alike -- is keyed by the symbol alone and listed in the second map, so that a
    kernel which moves between units is still compared; one whose copies differ keeps "unit:" in front."""
    units = {stem: kernels(asm) for stem, asm in compile_asm(root, experiments).items()}
    holders = {}
    for stem, syms in sorted(units.items()):
        for sym in syms:
            holders.setdefault(sym, []).append(stem)
    one_text = {sym for sym, stems in holders.items() if len({units[stem][sym] for stem in stems}) == 1}
    out = {(sym if sym in one_text else stem + ":" + sym): text for stem, syms in units.items() for sym, text in syms.items()}
    return out, {sym: " + ".join(holders[sym]) for sym in one_text}


def compare(a, b):
    """(symbols in both, those of them that differ, symbols on one side only)"""
    both = sorted(set(a) & set(b))
    return both, [s for s in both if a[s] != b[s]], sorted(set(a) ^ set(b))


def main():
    verbose = "-v" in sys.argv
    parent, head = [a for a in sys.argv[1:] if a != "-v"]
    bad = 0
    for name, experiments in (("product", False), ("experiments", True)):
        (a, unit_a), (b, unit_b) = tree_kernels(parent, experiments), tree_kernels(head, experiments)
        both, differing, single = compare(a, b)
        nk = lambda syms: sum("fn:" not in s for s in syms)
        print(f"{name:12s} kernels parent {nk(a):<4d} head {nk(b):<4d} compared {nk(both):<4d} differing {nk(differing):<4d} "
              f"only in one build {nk(single)}")
        print(f"{'':12s} device functions that are not inlined: parent {len(a) - nk(a)} head {len(b) - nk(b)} compared {len(both) - nk(both)} "
              f"differing {len(differing) - nk(differing)} only in one build {len(single) - nk(single)}")
        for s in differing:
            print("  differs:  " + s)
            if verbose:
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[s].split("\n"), b[s].split("\n"), "parent", "head", lineterm="", n=2))
        for s in single:
            print("  one side: " + s)
        for s in both:
            if unit_a.get(s, unit_b.get(s)) != unit_b.get(s):
                print(f"  moved:    {s}  {unit_a[s]} -> {unit_b[s]}")
        bad += len(differing) + len(single)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
