"""CPU: the premises of the matcher's unit tests (match_cases.py; the GPU side is tests/test_gpu_match_kernels.py): the exact families
are exact, ties and clipped zeros occur where the tests rely on them, the thresholds sit on the lattice, the grids hold the tile
edges of every kernel of linetr_amd/csrc/lt_match.h, and a NumPy model with one deliberate mistake fails the checks the kernels must
pass."""
import numpy as np
import pytest

import match_cases as MC

BASES = ("exact_clip", "exact_lattice", "normal")
GRIDS = ("dist", "pool", "cache_edge", "fused", "ident")


def _refs(family):
    return [(c, MC.case_reference(c, 0)) for c in MC.single_cases(family)]


@pytest.mark.parametrize("family", sorted(MC.EXACT))
def test_exact_families_are_exact(family):
    """The float32 chain in two summation orders and float32 pooling all equal float64, and float64 itself is a float32 number."""
    cases = list(MC.single_cases(family)) + [MC.batch_case(family, P, v) for P in (8, 9, 2) for v in (0, 1)]
    for c in cases:
        for i, p in enumerate(MC.case_pairs(c)):
            r = MC.case_reference(c, i)
            assert np.array_equal(r["ref64"].astype(np.float32).astype(np.float64), r["ref64"]), c["name"]
            assert np.array_equal(r["ref32"].astype(np.float64), r["ref64"]), c["name"]
            assert np.array_equal(MC.dk32(p, order=-1).astype(np.float64), r["ref64"]), c["name"]
            D = (2.0 - 2.0 * (p["d0"].astype(np.float64) @ p["d1"].astype(np.float64).T)).clip(min=0)        # float64 D, float32 pooling
            t = MC._pool32(D.astype(np.float32), p["c0"])
            assert np.array_equal(MC._pool32(np.ascontiguousarray(t.T), p["c1"]).T.astype(np.float64), r["ref64"]), c["name"]
            assert set(p["c0"]) | set(p["c1"]) <= {1, 2, 4}


def _ties(r64, axis):
    m = r64.min(axis=axis, keepdims=True)
    return int(((r64 == m).sum(axis=axis) > 1).sum())


def test_ties_and_the_clip_occur_where_the_tests_rely_on_them():
    refs = _refs("exact_clip")
    rows = sum(r["ref64"].shape[0] for _, r in refs)
    cols = sum(r["ref64"].shape[1] for _, r in refs)
    assert 0.10 <= sum(_ties(r["ref64"], 1) for _, r in refs) / rows <= 0.90          # the tie scale: tied row minima ...
    assert 0.10 <= sum(_ties(r["ref64"], 0) for _, r in refs) / cols <= 0.90          # ... and tied column minima
    for grid in ("dist", "pool", "fused", "ident"):
        mine = [(c, r) for c, r in refs if c["grid"] == grid]
        assert any((r["ref64"] == 0).any() for _, r in mine), grid                      # the clip: dot > 1
        assert any(_ties(r["ref64"], 1) for _, r in mine) and any(_ties(r["ref64"], 0) for _, r in mine), grid
    # a column whose minimum occurs in several 16-row chunks (the packed atomicMin / the partials merged in chunk order) and a row
    # whose minimum occurs in both halves of the columns (the row argmin combined across gridDim.y in the identity kernel)
    for grid in ("pool", "ident"):
        cross = 0
        for c, r in refs:
            d = r["ref64"]
            if c["grid"] != grid or d.shape[0] <= 16:
                continue
            hit = d == d.min(axis=0, keepdims=True)
            cross += int((np.add.reduceat(hit, np.arange(0, d.shape[0], 16), axis=0).astype(bool).sum(axis=0) > 1).sum())
        assert cross > 0, grid
    split = 0
    for c, r in refs:
        d = r["ref64"]
        if c["grid"] == "ident" and d.shape[1] > 128:
            n_ct = -(-d.shape[1] // 16)
            per = -(-n_ct // -(-n_ct // 8)) * 16                                        # columns per block of the identity kernel
            hit = d == d.min(axis=1, keepdims=True)
            split += int((np.add.reduceat(hit, np.arange(0, d.shape[1], per), axis=1).astype(bool).sum(axis=1) > 1).sum())
    assert split > 0
    assert not any((r["ref64"] == 0).any() for _, r in _refs("exact_lattice"))          # the other scale never clips
    lat = np.concatenate([r["ref64"].ravel() for c, r in _refs("exact_lattice") if c["grid"] == "ident"])
    assert 0.5 < lat.min() and lat.max() < 3.5 and np.array_equal(lat * 128, np.round(lat * 128))   # a 2^-7 lattice around 2, far from the clip


@pytest.mark.parametrize("family", BASES)
def test_thresholds_sit_on_values_of_dk(family):
    for c in MC.single_cases(family) + tuple(MC.batch_case(family, P) for P in (8, 9, 2)):
        i = next(i for i in c["check"] if MC.case_reference(c, i)["ref64"].size)
        dk = MC.case_reference(c, i)["ref64"].astype(np.float32)
        thr = MC.case_thresholds(c)
        assert all(np.float32(t) == t for t, _ in thr) and {m for _, m in thr} == {True, False}
        if family == "normal" and len(c["specs"]) == 1:      # no decision within 2 x the bar: paths inside the bar agree on match01
            assert MC.near_ties(MC.case_reference(c, i), thr) == 0, c["name"]
            assert 0 < (dk.min(axis=1) < thr[0][0]).sum() < max(2, dk.shape[0]) or dk.shape[0] == 1, c["name"]   # and the threshold still bites
        if family in MC.EXACT:
            v = np.float32(thr[0][0])
            assert (dk == v).any() and (dk.min(axis=1) == v).any(), c["name"]
            assert {t for t, _ in thr} == {float(v), float(np.nextafter(v, np.float32(np.inf)))}
            want = [MC.nn_rules(dk, t, m) for t, m in thr]
            assert not np.array_equal(want[2], want[3]), c["name"]                      # the threshold bites: one-sided, v against nextafter(v)


def test_grids_contain_the_tile_edges():
    d = set(MC.dist_shapes())
    assert d >= {(n, n) for n in (1, 31, 32, 33, 63, 64, 65, 129)} | {(1, 129), (129, 1), (33, 65), (65, 33), (63, 65), (65, 63), (31, 32), (32, 31)}
    for fam in BASES:
        assert {(c["specs"][0][0], c["specs"][0][1]) for c in MC.dist_cases(fam)} and \
            {(sum(c["specs"][0][0]), sum(c["specs"][0][1])) for c in MC.dist_cases(fam)} == d
    shapes = MC.pool_shapes()
    assert {k0 for k0, _ in shapes} >= {1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 79, 80, 81, 143, 144, 145, 257}
    assert {k1 for _, k1 in shapes} == {1, 15, 16, 17, 63, 64, 65, 255, 256, 257}
    for k0 in {k0 for k0, _ in shapes}:
        assert len({k1 for a, k1 in shapes if a == k0}) >= 2, k0
    assert {min(16, k0) * k1 for k0, k1 in shapes} >= {256, 1024, 1040}                 # the 256 x 4 element pass of pair_pool_kernel
    assert {-(-k0 // 16) for k0, _ in shapes} >= {1, 2, 3, 4, 5, 8, 9}                   # pair_final_kernel: 4-chunk loop + remainder
    assert [len(c["specs"][0][1]) for c in MC.cache_edge_cases("normal")] == [896, 897]
    assert len(MC.pool_forced_cases("normal")) >= 5 and {len(c["specs"][0][0]) > 16 for c in MC.pool_forced_cases("normal")} == {True, False}
    for fam in BASES:
        f = MC.fused_cases(fam)
        assert {sum(c["specs"][0][1]) for c in f} == {1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1024}
        assert {len(c["specs"][0][0]) for c in f} == {1, 15, 16, 17, 33}
        assert {-(-sum(c["specs"][0][1]) // 16) for c in f} >= {8, 9, 16, 17}          # the two-tile switch and the second trip
        starts, straddle, owns = set(), False, set()
        for c in f:
            c0 = np.asarray(c["specs"][0][0])
            cu = np.concatenate([[0], np.cumsum(c0)])
            for b in range(0, len(c0), 16):
                lo, hi = int(cu[b]), int(cu[min(b + 16, len(c0))])
                starts.add(lo % 16)
                owns.add(hi - lo)
                inner = cu[b:min(b + 16, len(c0)) + 1]
                straddle |= any((s - lo) // 16 != (e - 1 - lo) // 16 for s, e in zip(inner[:-1], inner[1:]))
        assert starts - {0} and straddle and 64 in owns, fam
        if fam == "normal":
            assert any(3 in c["specs"][0][0] for c in f) and any(3 in c["specs"][0][1] for c in f)
        i = MC.ident_cases(fam)
        assert {sum(c["specs"][0][1]) for c in i} == {1, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1023, 1024}
        assert {len(c["specs"][0][0]) for c in i} == {1, 15, 16, 17, 33, 257}
        assert all(MC.legal_paths(c) == (0, 1, 2) for c in i) and all(MC.legal_paths(c) == (0, 1) for c in f if sum(c["specs"][0][1]) > 1)
    assert {n for p in MC.POINTS_N for n in p} == {1, 31, 32, 33, 65}


def test_batches_and_caps():
    for fam in MC.FAMILIES:
        for P in (8, 9, 2):
            for v in (0, 1):
                c = MC.batch_case(fam, P, v)
                dims = MC.layout(c)["dims"]
                assert len(dims) == P <= MC.MAX_P and dims.max() <= MC.MAX_N
                where = [] if P < 3 else [0, P // 2, P - 1]
                assert all(dims[i, 1] * dims[i, 3] == 0 and dims[i, 1] + dims[i, 3] > 0 for i in where)
                assert P < 3 or ((dims[where][:, 3] == 0).any() and (dims[where][:, 1] == 0).any())
                full = [i for i in range(P) if i not in where]
                assert len({tuple(dims[i]) for i in full}) == len(full)                      # heterogeneous
                L = MC.layout(c)
                assert P < 3 or all(any(o % 2 for o in L[k][1:]) for k in ("off_n0", "off_dk", "off_k0"))  # offsets: multiples of nothing
        assert {(MC.layout(MC.batch_case(fam, 9, v))["dims"][0, 3] == 0) for v in (0, 1)} == {True, False}
        for c in MC.single_cases(fam):
            assert MC.layout(c)["dims"].max() <= MC.MAX_N
    s = MC.batch_case("sentinel", 9, 0, 1)
    assert [i % 2 for i in s["check"]] == [0] * len(s["check"]) and all(np.abs(p["d0"]).min() == MC.SENTINEL for p in MC.case_pairs(s) if p["sentinel"] and p["n0"])


def test_rules_are_the_oracles_and_ref32_sits_inside_both_bars():
    for c in MC.pool_cases("exact_clip")[::5] + MC.pool_cases("normal")[::5] + (MC.batch_case("normal", 9),):
        for i in c["check"]:
            r = MC.case_reference(c, i)
            for thr, mutual in MC.case_thresholds(c):
                assert np.array_equal(MC.nn_rules(r["ref64"], thr, mutual), MC.oracle_rules(r["ref64"], thr, mutual))
            assert MC.check_pair(c["base"], r, r["ref32"], MC.oracle_rules(r["ref32"] if c["base"] == "normal" else r["ref64"], 1.5, True), 1.5, True) == []
    for c, r in _refs("normal"):
        err = np.abs(r["ref32"].astype(np.float64) - r["ref64"])
        assert err.max() <= r["bar"] / MC.FACTOR and (err <= r["bound"] / 4).all(), c["name"]


def _model_fails(case, drop_k=None, plus=0, **rule):
    """Does the NumPy float32 model with one mistake fail the case's checks at any of its thresholds?"""
    p, r = MC.case_pairs(case)[0], MC.case_reference(case, 0)
    dk = MC.dk32(p, drop_k=drop_k, plus=plus) if drop_k is not None or plus else r["ref32"]
    return any(MC.check_pair(case["base"], r, dk, MC.nn_rules(dk, thr, mutual, **rule), thr, mutual) for thr, mutual in MC.case_thresholds(case))


def _some(cases, n=4):
    return list(cases[:n]) + list(cases[-n:])


@pytest.mark.parametrize("family", BASES)
def test_a_model_with_one_mistake_fails(family):
    by_grid = {g: [c for c in MC.single_cases(family) if c["grid"] == g] for g in GRIDS}
    for g, cases in by_grid.items():
        assert not any(_model_fails(c) for c in _some(cases)), g                               # the model itself passes
        for c in _some(cases):
            big = MC.layout(c)["dims"][0, 0] * MC.layout(c)["dims"][0, 2] >= 16 or family == "normal"
            assert _model_fails(c, drop_k=128) or not big, (g, c["name"], "a K step of 4 channels dropped")
            assert _model_fails(c, plus=1), (g, c["name"], "weight 1 / (count + 1)")
            if family in MC.EXACT:
                assert _model_fails(c, le=True), (g, c["name"], "<= at the threshold")
    if family == "exact_clip":       # ties: every grid has a case where the last minimum is not the first ...
        for g in ("dist", "pool", "fused", "ident"):
            assert any(_model_fails(c, last=True) for c in by_grid[g]), (g, "last-index argmin")
        for g in ("pool", "ident"):  # ... and one where a column's minimum occurs in several 16-row chunks
            assert any(_model_fails(c, merge="reverse") for c in by_grid[g]), (g, "columns merged in reverse chunk order")
    if family == "exact_lattice":
        assert any(_model_fails(c, last=True) for c in by_grid["ident"]) and any(_model_fails(c, merge="reverse") for c in by_grid["ident"] + by_grid["pool"])
    if family == "normal":           # four dropped channels exceed the forward bound almost everywhere
        c = by_grid["ident"][-1]
        r = MC.case_reference(c, 0)
        err = np.abs(MC.dk32(MC.case_pairs(c)[0], drop_k=128).astype(np.float64) - r["ref64"])
        assert (err > r["bound"]).mean() > 0.99
