"""CPU: the premises of the distance-matrix entry points' unit tests (distmat_cases.py; the GPU side is tests/test_gpu_distmat.py): every
edge group of the matcher cases holds its plant where the kernels' reductions change hands and tells the rules from each mutated rule
set, the exact pooling family is exact, the bars are properties of the references alone, the sizes hold every edge the kernels have,
and every mutation of a tokeniser's matrix sets its bit and -- one-ulp weights apart -- moves the answer far from
what pooling by a map would give."""
import numpy as np
import pytest

import distmat_cases as DC
from match_cases import pool_matrix

DTYPES = ("f32", "f64")


def _tags(case):
    return {p[0] for p in case["plants"]}


@pytest.mark.parametrize("dtype", DTYPES)
def test_matcher_sizes(dtype):
    shapes = {(c["n0"], c["n1"]) for c in DC.match_cases(dtype)}
    n0s, n1s = (DC.MATCH32_N0, DC.MATCH32_N1) if dtype == "f32" else (DC.MATCH64_N0, DC.MATCH64_N1)
    assert {s[0] for s in shapes} >= set(n0s) and {s[1] for s in shapes} >= set(n1s)
    for n0 in n0s:
        assert sum(s[0] == n0 for s in shapes) >= 2
    for n1 in n1s:
        assert sum(s[1] == n1 for s in shapes) >= 2
    if dtype == "f32":
        assert {(3, 12000), (3, 12001)} <= shapes
    assert max(a * b for a, b in shapes) <= 257 * 897 and max(b for _, b in shapes) <= 12001


@pytest.mark.parametrize("dtype", DTYPES)
def test_matcher_values_and_plants(dtype):
    """The matrices hold the values the tests are about, and every plant is what its tag says: the row's / column's minimum, tied
    across the named edge, the first of the tied entries being the answer."""
    tags = set()
    for c in DC.match_cases(dtype):
        d, thr = c["d"], c["thr"]
        assert not np.isnan(d).any()
        if d.size > 3000:
            for v in (DC.VALS32 if dtype == "f32" else (-1e-12, 0.0, 0.25, 0.8, 0.8 + 1e-12, 0.8 - 1e-12, 1.0, 4.0, np.inf)):
                assert (d == v).any() and (np.signbit(d) & (d == 0)).any(), (c["name"], v)
        dm = d.astype(np.float64).clip(min=0)
        mutual, oneway = DC.match_want(c, True), DC.match_want(c, False)
        for tag, kind, rows, cols in c["plants"]:
            tags.add(tag)
            r = rows[0]
            if kind == "row":
                assert (np.flatnonzero(dm[r] == dm[r].min()) == np.array(cols if tag != "merge" else cols[1:])).all(), (c["name"], tag)
                assert np.argmin(dm[:, cols[0]]) == r and np.argmin(dm[:, cols[-1]]) == r
                first = cols[0] if tag != "merge" else cols[1]
                assert mutual[r] == first and oneway[r] == first
                if tag == "merge":
                    assert np.float32(d[r, cols[0]]) == np.float32(d[r, cols[1]]) and d[r, cols[0]] > d[r, cols[1]]
                    assert DC.match_want(c, True, "as_f32")[r] == cols[0]
                else:
                    assert DC.match_want(c, True, "last")[r] == cols[-1] and DC.match_want(c, False, "no_clip")[r] == cols[1]
                    if tag == "s64":
                        assert np.all(np.diff(cols) == 64)
                    if tag == "l63":
                        assert cols == (63, 64)
            elif kind == "col":
                col = cols[0]
                assert tuple(np.flatnonzero(dm[:, col] == dm[:, col].min())) == rows and rows[1] == rows[0] + 1
                assert rows[0] % 16 == 15 or (dtype == "f64" and rows[0] == 3)
                assert oneway[rows[0]] == col and oneway[rows[1]] == col and mutual[rows[0]] == col and mutual[rows[1]] == -1
                assert DC.match_want(c, True, "last")[rows[0]] == -1 and DC.match_want(c, True, "no_clip")[rows[0]] == -1
            elif kind == "thr":
                assert dm[r].min() == thr and (dm[r] == thr).sum() >= 1 and mutual[r] == -1 and oneway[r] == -1
                assert DC.match_want(c, False, "le")[r] == (c["n1"] - 1) // 2
            else:
                assert np.isinf(d[r]).all() and (d[r] > 0).all() and mutual[r] == -1 and oneway[r] == -1
    want = set(DC.ROW_TAGS) | set(DC.COL_TAGS) | {"thr", "inf"}
    assert tags == (want - {"merge", "r3"} if dtype == "f32" else want - {"last"})


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_edge_group_tells_the_rules_from_every_mutation(dtype):
    """For every edge group, every mutated rule set (last-index argmin, `<=` at the threshold, no mutual check, no clip; f64: the
    matrix rounded to float32 first) differs from the rules on at least one case of the group.  Otherwise the group proves nothing."""
    cases = DC.match_cases(dtype)
    muts = DC.MUTATIONS32 if dtype == "f32" else DC.MUTATIONS64
    differs = {(c["name"], m): any((DC.match_want(c, mu) != DC.match_want(c, mu, m)).any() for mu in (True, False)) for c in cases for m in muts}
    for tag in sorted(set().union(*(_tags(c) for c in cases))):
        for m in muts:
            assert any(differs[(c["name"], m)] for c in cases if tag in _tags(c)), (tag, m)
    if dtype == "f32":     # the sizes on either side of a switch, each on its own
        for n1 in (896, 897, 12000, 12001):
            for m in ("last", "no_clip"):
                assert any(differs[(c["name"], m)] for c in cases if c["n1"] == n1), (n1, m)


def test_matcher_threshold_values():
    assert DC.THR32_BELOW < DC.THR32 < DC.THR32_ABOVE and float(DC.THR32) > 0.8
    assert np.float64(0.8) < DC.THR64 < np.float64(0.8) + 2e-12 and float(np.float32(DC.THR64)) > DC.THR64
    assert np.float64(0.8) + 1e-12 == DC.THR64          # base value + jitter lands on the threshold exactly


# ---------------------------------------------------------------------------------------------------------------- pooling by maps
def test_exact_family_is_exact():
    """NumPy's float32 product in both association orders and a sequential float32 segmented sum all equal float64, which is a
    float32 number."""
    for p in DC.pool_cases("exact"):
        r = DC.pool_reference("exact", p["c0"], p["c1"])
        assert set(p["c0"]) | set(p["c1"]) <= {1, 2, 4}
        assert np.array_equal(r["ref64"].astype(np.float32).astype(np.float64), r["ref64"]), p["name"]
        assert np.array_equal(r["ref32"].astype(np.float64), r["ref64"]) and r["own"] == 0.0
        A0, A1 = pool_matrix(p["c0"], np.float32), pool_matrix(p["c1"], np.float32)
        assert np.array_equal((A0 @ (p["D"] @ A1.T)).astype(np.float64), r["ref64"])
        assert np.array_equal(p["D"] * 16, np.round(p["D"] * 16)) and p["D"].min() >= 0 and p["D"].max() <= 4


def test_normal_family_bars_come_from_the_references():
    for p in DC.pool_cases("normal"):
        r = DC.pool_reference("normal", p["c0"], p["c1"])
        assert r["bar"] == DC.FACTOR * r["own"]
        assert (r["bound"] > 0).all() and r["bound"].max() <= (5 + 5 + 2) * DC.U24 * 4
        assert set(p["c0"]) | set(p["c1"]) <= {1, 2, 3, 4, 5}
        # NumPy's own float32 product stays inside the forward bound: the bound is one a float32 evaluation can meet
        assert (np.abs(r["ref32"].astype(np.float64) - r["ref64"]) <= r["bound"]).all(), p["name"]
    counts = set().union(*(set(p["c0"]) | set(p["c1"]) for p in DC.pool_cases("normal")))
    assert {3, 5} <= counts                                  # 1 / count rounds


@pytest.mark.parametrize("family", ("exact", "normal"))
def test_pool_sizes(family):
    cases = DC.pool_cases(family)
    k0s, k1s = {p["k0"] for p in cases}, {p["k1"] for p in cases}
    assert {1, 15, 16, 17, 33} <= k0s and {896, 897, 12000, 12001} <= k1s
    assert {(p["k0"], p["k1"]) for p in cases} >= {(2, 12000), (2, 12001)}
    tails = {min(16, p["k0"] - i0) * p["k1"] for p in cases for i0 in range(0, p["k0"], 16)}      # rows x k1 of a block
    assert {1023, 1024, 1025, 2047, 2049} <= tails
    assert {256, 257, 513} <= {p["n0"] for p in cases} and {256, 257, 513} <= {p["n1"] for p in cases}
    big = 4 if family == "exact" else 5
    for side in ("0", "1"):
        assert any(p["s" + side][255] == p["s" + side][256] for p in cases if p["n" + side] > 256)            # a key-line across 255 | 256
        assert {1, big} <= {p["c" + side][-1] for p in cases}
    assert max(p["n0"] * p["n1"] for p in cases) <= 2 ** 20 and max(p["n1"] for p in cases) <= 12001
    assert all(p["n0"] <= 3 for p in cases if p["n1"] > 8000)


# ---------------------------------------------------------------------------------------------------------------- pooling by matrices
def test_verdict_rules_on_tokeniser_matrices():
    for c0, c1 in DC.tokeniser_shapes():
        assert DC.expected_verdict(pool_matrix(c0, np.float32), pool_matrix(c1, np.float32)) == 0
    ns = {sum(c) for pair in DC.tokeniser_shapes() for c in pair}
    assert set(DC.TOKENISER_N) <= ns
    straddle = [c for pair in DC.tokeniser_shapes() for c in pair if sum(c) > 257]
    assert straddle and all(np.repeat(np.arange(len(c)), c)[254] == np.repeat(np.arange(len(c)), c)[257] for c in straddle)
    assert set(range(1, 6)) <= set(DC.mut_counts())
    # the weight is the float64 quotient rounded once
    assert all(pool_matrix((c,), np.float32)[0, 0] == np.float32(1.0 / c) for c in range(1, 6))


# (an emptied row 0 leaves the order of the map intact -- an empty column reads as key-line 0 -- and shows in bits 1 and 4: the bit-2
# check in front of key-line 0 is merge_row0's)
WANT_BIT = {"second": 1, "emptycol": 1, "swap_rows": 2, "empty_last_row": 2, "empty_row0": 5, "merge_last_row": 2, "merge_row0": 2,
            "ulp_up": 4, "ulp_down": 4, "negated": 4, "nan": 4}
EXACTLY = {"empty_row0": 5, "empty_last_row": 7, "swap_rows": 2, "merge_last_row": 2, "merge_row0": 2, "ulp_up": 4, "ulp_down": 4, "negated": 4, "nan": 4,
           "second@255": 1, "second@256": 1, f"second@{DC.MUT_N - 1}": 1}


@pytest.mark.parametrize("side", (0, 1))
def test_every_mutation_sets_its_bit_and_moves_the_answer(side):
    clean = DC.dense_mutation_case(side, None)
    assert clean["verdict"] == 0
    cm = DC.mut_counts()
    m_map = np.repeat(np.arange(len(cm)), cm)
    assert m_map[254] == m_map[257] and sum(cm) == DC.MUT_N
    for name in DC.mutation_names():
        c = DC.dense_mutation_case(side, name)
        kind = name.partition("@")[0]
        A, A_clean = (c["A0"], clean["A0"]) if side == 0 else (c["A1"], clean["A1"])
        assert (c["A1"] if side == 0 else c["A0"]).tobytes() == (clean["A1"] if side == 0 else clean["A0"]).tobytes()      # one side alone
        assert c["verdict"] & WANT_BIT[kind], name
        for key, bits in EXACTLY.items():
            if name == key or kind == key:
                assert c["verdict"] == bits, (name, c["verdict"])
        changed = np.argwhere(~((A == A_clean) | (np.isnan(A) & np.isnan(A_clean))))
        if DC.is_ulp(name):
            assert len(changed) == 1
            w, w0 = A[tuple(changed[0])], A_clean[tuple(changed[0])]
            assert w0 in (np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(2)))
            continue
        if name.endswith("straddle_last"):
            assert len(changed) == 1 and changed[0][1] == 257
        # the premise: pooled by a map -- the sanitised one or the matrix's own -- the answer would be far from the product as given
        K, N = A.shape
        maps = {"sanitised": DC.sanitised_map(K, N), "own": m_map}
        k_o = len(DC.OTHER_COUNTS)
        m_o = np.repeat(np.arange(k_o), DC.OTHER_COUNTS)
        far = 100 * max(c["bar"], float(np.nanmax(c["bound"])))
        for label, m in maps.items():
            alt = DC.pooled_by_map(c["D"], m, K, m_o, k_o) if side == 0 else DC.pooled_by_map(c["D"], m_o, k_o, m, K)
            with np.errstate(invalid="ignore"):
                gap = np.abs(alt - c["ref64"])
            assert np.isnan(gap).any() or gap.max() > far, (name, label, float(np.nanmax(gap)), far)


def test_as_given_shapes():
    cases = DC.as_given_cases()
    shapes = {(c["A1"].shape[0], c["A1"].shape[1]) for c in cases}
    assert {k for k, _ in shapes} >= set(DC.AS_GIVEN_K1) and {n for _, n in shapes} >= set(DC.AS_GIVEN_N1)
    assert any(c["A0"].shape[0] > c["A0"].shape[1] and c["verdict"] == 1 for c in cases)
    assert any(c["A1"].shape[0] > c["A1"].shape[1] and c["A0"].shape[0] <= c["A0"].shape[1] and c["verdict"] == 1 for c in cases)
    assert all(c["verdict"] != 0 for c in cases)
    for c in cases:      # the entry-wise bound is one NumPy's own float32 product meets
        assert (np.abs(c["ref32"].astype(np.float64) - c["ref64"]) <= c["bound"]).all(), c["name"]
