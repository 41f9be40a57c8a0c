"""GPU: every kernel of the matcher (linetr_amd/csrc/lt_match.h) alone, through linetr_debug_match, against the float64 restatement of
models/line_process.py:198-201, models/line_transformer.py:277-282 and models/nn_matcher.py:3-31 at its tile edges.  Cases,
references and bars: tests/match_cases.py (its premises: tests/test_match_cases_cpu.py); the measured errors live in
profiles/match_unit_errors.txt (tools/match_unit_report.py), never here."""
import numpy as np
import pytest
import torch

import match_cases as MC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GRIDS = {"dist": MC.dist_cases, "pool": MC.pool_cases, "cache_edge": MC.cache_edge_cases, "fused": MC.fused_cases, "ident": MC.ident_cases}
_first = {}      # (case name, path) -> the results of the case's first run on that path


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


def first_run(eng, case, path):
    key = (case["name"], path)
    if key not in _first:
        _first[key] = MC.run_and_check(eng, case, path)
    return _first[key]


def same(a, b, dk_bits=True):
    """two run_and_check results: identical match01 (and Dk bits) at every threshold and pair"""
    return all(np.array_equal(a[t][i][1], b[t][i][1]) and (not dk_bits or np.array_equal(a[t][i][0].view(np.uint32), b[t][i][0].view(np.uint32)))
               for t in a for i in a[t])


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("path,grid", [(p, g) for p in (0, 1) for g in sorted(GRIDS)] + [(2, "ident")])
def test_single_pair_path_against_float64(eng, path, grid, family):
    """One path on every single-pair case of a grid that it serves: Dk against float64 (bit for bit in the exact families, inside the
    reference bar and the forward bound otherwise), match01 against the rules."""
    cases = [c for c in GRIDS[grid](family) if path in MC.legal_paths(c)]
    assert len(cases) >= 2
    fails = [f for c in cases for f in first_run(eng, c, path)[1]]
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("family", MC.FAMILIES)
def test_paths_agree(eng, family):
    """For every single pair, the paths that serve it give identical match01 -- and identical Dk bits in the exact families.
    Identity maps forced through pair_match_fused_kernel<false> equal <true> bit for bit in every family."""
    bad = []
    for c in MC.single_cases(family):
        runs = {p: first_run(eng, c, p)[0] for p in MC.legal_paths(c)}
        for p in runs:
            if not same(runs[0], runs[p], dk_bits=MC._base(family) in MC.EXACT):
                bad.append(f"{c['name']}: path {p} differs from the three launches")
        if 2 in runs and not same(runs[1], runs[2]):
            bad.append(f"{c['name']}: identity maps through <false> differ from <true>")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("family", ("exact_clip", "normal"))
@pytest.mark.parametrize("seg1_global,cache_dk", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pool_kernel_switches(eng, family, seg1_global, cache_dk):
    """pair_seg1_kernel + the workspace segment table, and the pooled rows read back from Dk instead of LDS, at ordinary sizes."""
    fails = []
    for c in MC.pool_forced_cases(family) + MC.cache_edge_cases(family)[:1]:
        res, f = MC.run_and_check(eng, c, 0, seg1_global=seg1_global, cache_dk=cache_dk)
        fails += f
        if not same(res, first_run(eng, c, 0)[0]):
            fails.append(f"{c['name']}: differs from the matcher's own switches")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("P,device_table", [(8, -1), (9, -1), (2, 1), (8, 1)])
def test_batches(eng, family, P, device_table):
    """Heterogeneous batches through the inline pair table (P = 8) and the device-resident one (P = 9, or forced), pairs without
    key-lines first, in the middle and last; 'sentinel': the other parity's pairs hold +-1e4."""
    fails = []
    for variant in (0, 1):
        for parity in ((0, 1) if family == "sentinel" else (0,)):
            c = MC.batch_case(family, P, variant, parity)
            res, f = MC.run_and_check(eng, c, 0, device_table=device_table)
            fails += f
            for (thr, mutual), r in res.items():      # a pair without key-lines on a side: no Dk, match01 all -1
                for i, d in enumerate(MC.layout(c)["dims"]):
                    if d[1] * d[3] == 0 and not (r[i][1] == -1).all():
                        fails.append(f"{c['name']} pair {i}: match01 of an empty pair is not -1")
    assert not fails, "\n".join(fails[:20])


def test_slot_hygiene(eng):
    """The one-launch cases again in reverse order on one stream, large and small alternating: every result is bit-identical to
    its first run (the kernel leaves its scratch slot clean)."""
    todo = [(c, p) for fam in ("exact_clip", "normal") for c in MC.fused_cases(fam) + MC.ident_cases(fam) for p in MC.legal_paths(c) if p]
    firsts = [first_run(eng, c, p)[0] for c, p in todo]
    bad = [f"{c['name']} path {p}" for (c, p), f in list(zip(todo, firsts))[::-1] if not same(MC.run_and_check(eng, c, p)[0], f)]
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("family", ("exact_clip", "exact_lattice", "normal"))
def test_point_matcher_transpose(eng, family):
    """transpose_cn_kernel in front of the matcher (linetr_match_points on [256, n] descriptors) at its 32 x 32 tile edges."""
    fails = []
    for i, (n0, n1) in enumerate(MC.POINTS_N):
        c = MC._single("points", family, (1,) * n0, (1,) * n1, 40 + i)
        p, ref = MC.case_pairs(c)[0], MC.case_reference(c, 0)
        for thr, mutual in MC.case_thresholds(c):
            dist, m01 = eng.match_points(torch.from_numpy(np.ascontiguousarray(p["d0"].T)).cuda(), torch.from_numpy(np.ascontiguousarray(p["d1"].T)).cuda(), thr, mutual)
            torch.cuda.synchronize()
            fails += [f"{c['name']}: {f}" for f in MC.check_pair(family, ref, dist.cpu().numpy(), m01.cpu().numpy(), thr, mutual)]
    assert not fails, "\n".join(fails[:20])


def test_dispatch_table(eng):
    """path = -1 is the matcher's own choice: one pair with n1 <= 1024 takes the one-launch kernel named by its counts, n1 = 1025 and
    every batch the three launches -- reported without a launch and by a real run alike."""
    assert eng.match_path([[200, 200, 210, 210]]) == 2 and eng.match_path([[1024, 1024, 1024, 1024]]) == 2
    assert eng.match_path([[230, 200, 210, 210]]) == 1 and eng.match_path([[200, 200, 211, 210]]) == 1 and eng.match_path([[1500, 900, 1024, 1000]]) == 1
    assert eng.match_path([[200, 200, 1025, 1025]]) == 0 and eng.match_path([[230, 200, 1025, 1000]]) == 0
    assert eng.match_path([[200, 200, 210, 210]] * 2) == 0 and eng.match_path([[5, 5, 0, 0]]) == 0
    for c, want in ((MC.ident_cases("normal")[5], 2), (MC.fused_cases("normal")[5], 1), (MC.batch_case("normal", 2), 0)):
        ln = MC.Launcher(eng, c)
        thr, mutual = MC.case_thresholds(c)[0]
        res, used = ln.run(-1, thr, mutual)
        assert used == want == eng.match_path(MC.layout(c)["dims"])
        if len(c["specs"]) == 1:
            assert same({0: res}, {0: first_run(eng, c, want)[0][(thr, mutual)]})


def test_refusals_leave_the_outputs_untouched(eng):
    from linetr_amd._native import NativeError
    fused, ident, batch = MC.fused_cases("normal")[5], MC.ident_cases("normal")[5], MC.batch_case("normal", 9)
    big = MC._single("refuse", "normal", (1,) * 5, (1,) * 1025, refused=True)
    wide = MC.cache_edge_cases("normal")[1]

    def refused(case, path, match, **kw):
        ln = MC.Launcher(eng, case)
        with pytest.raises(NativeError, match=match):
            ln.run(path, 1.0, True, **kw)
        torch.cuda.synchronize()
        assert bool((ln.dk == MC.MARKER).all()) and bool((ln.m01 == MC.MARKER_I).all())
        return ln

    refused(batch, 1, "one pair")
    refused(batch, 2, "one pair")
    refused(big, 1, "beyond the one-launch")
    refused(big, 2, "beyond the one-launch")
    refused(fused, 2, "one sub-line per key-line")
    refused(wide, 0, "row cache", cache_dk=1)
    huge = MC._single("refuse", "normal", (1,) * 3, (1,) * 12001, refused=True)      # one past PM_MAX_K1: no LDS segment table
    refused(huge, 0, "segment table", seg1_global=0)
    refused(batch, 0, "inline pair table", device_table=0)
    refused(fused, 1, "path 0 only", cache_dk=0)
    refused(fused, -1, "path 0 only", seg1_global=1)
    refused(fused, 3, "path must be")
    ln = MC.Launcher(eng, ident)
    L, t = ln.L, ln.t
    ln.dk.fill_(MC.MARKER)
    ln.m01.fill_(MC.MARKER_I)
    args = lambda **o: {**dict(path=2, dims=L["dims"], desc0=t["d0"], off_n0=L["off_n0"], s2l0=t["s0"], desc1=t["d1"], off_n1=L["off_n1"], s2l1=t["s1"],
                               thr=1.0, mutual=True, dk=ln.dk, off_dk=L["off_dk"][:-1], m01=ln.m01, off_k0=L["off_k0"][:-1]), **o}
    with pytest.raises(NativeError, match="null tensor"):
        eng.debug_match(**args(desc1=None))
    with pytest.raises(NativeError, match="null tensor"):
        eng.debug_match(**args(m01=None))
    with pytest.raises(NativeError, match="misaligned"):
        eng.debug_match(**args(desc0=t["d0"].view(-1)[1:]))
    with pytest.raises(NativeError, match="bad dims"):
        eng.debug_match(**args(dims=np.array([[3, 5, 4, 4]], dtype=np.int32)))
    torch.cuda.synchronize()
    assert bool((ln.dk == MC.MARKER).all()) and bool((ln.m01 == MC.MARKER_I).all())
