"""GPU: the entry points that take a distance matrix that already exists -- linetr_match_distmat, linetr_match_distmat_f64,
linetr_pool_distmat, linetr_pool_distmat_dense (linetr_amd/csrc/linetr_match.hip; kernels in lt_match.h) -- alone, through the C ABI on
marked buffers, against the float64 restatement of models/nn_matcher.py:3-31 and models/line_transformer.py:277-282 at their edges.
Cases, references and bars: tests/distmat_cases.py (its premises: tests/test_distmat_cases_cpu.py); the measured errors live in
profiles/distmat_unit_errors.txt (tools/distmat_unit_report.py), never here."""
import numpy as np
import pytest
import torch

import distmat_cases as DC
from linetr_amd._native import E_ARG, E_WORKSPACE
from match_cases import MARKER, MARKER_I, pool_matrix

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def raw():
    from linetr_amd.engine import Engine
    return DC.Raw(Engine.heads_only("cuda:0"))


# ---------------------------------------------------------------------------------------------------------------- the matcher rules
@pytest.mark.parametrize("mutual", (True, False))
@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_match_distmat_is_the_rules(raw, dtype, mutual):
    """match01 equals nn_rules on the float64 of the same matrix, entry for entry, on every case: ties planted where the lane strides,
    the wave tie-break, the 16-row chunks, pair_final_kernel's groups of four chunks, the f64 kernels' row quads and second blocks
    change hands; +-0, negatives, the threshold and its neighbours, +inf.  Guards intact, the matrix untouched."""
    fails = []
    for c in DC.match_cases(dtype):
        code, m01, _ = raw.match(c["d"], c["thr"], mutual)
        assert code == 0, c["name"]
        want = DC.match_want(c, mutual)
        if not np.array_equal(m01, want):
            bad = np.flatnonzero(m01 != want)
            planted = {r: t for t, _, rows, _ in c["plants"] for r in rows}
            fails.append(f"{c['name']}: {len(bad)} rows differ, first row {bad[0]}: {m01[bad[0]]} != {want[bad[0]]}"
                         f" (plants hit: {sorted({planted[r] for r in bad if r in planted})})")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_match_distmat_without_columns(raw, dtype):
    """n1 = 0 with n0 > 0 through the C call: every entry is -1 (no pointer to a matrix is needed)"""
    for n0 in (1, 5, 257):
        for mutual in (True, False):
            code, m01, _ = raw.match(np.zeros((n0, 0), dtype), 0.8, mutual, null=("dist",))
            assert code == 0 and (m01 == -1).all()


# ---------------------------------------------------------------------------------------------------------------- pooling by maps
@pytest.mark.parametrize("family", ("exact", "normal"))
def test_pool_distmat_against_float64(raw, family):
    """exact: bit for bit the float64 product; normal: inside FACTOR x NumPy's own float32 error and the per-entry forward bound"""
    fails = []
    for p in DC.pool_cases(family):
        code, dk, _ = raw.pool(p["D"], p["s0"], p["k0"], p["s1"], p["k1"])
        assert code == 0, p["name"]
        fails += [f"{p['name']}: {f}" for f in DC.check_pooled(family, DC.pool_reference(family, p["c0"], p["c1"]), dk)]
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------------------------------------------------------- pooling by matrices
def test_dense_tokeniser_matrices_are_pooled_by_their_maps(raw):
    """verdict 0, Dk bit-identical to linetr_pool_distmat on the maps, inside the bars of the map form"""
    fails = []
    for c0, c1 in DC.tokeniser_shapes():
        p = DC.pool_case("normal", c0, c1)
        code, dk, word, _ = raw.dense(p["D"], pool_matrix(c0, np.float32), pool_matrix(c1, np.float32))
        assert code == 0, p["name"]
        _, by_map, _ = raw.pool(p["D"], p["s0"], p["k0"], p["s1"], p["k1"])
        if word != 0:
            fails.append(f"{p['name']}: verdict {word}")
        if not np.array_equal(dk.view(np.uint32), by_map.view(np.uint32)):
            fails.append(f"{p['name']}: differs from linetr_pool_distmat on the maps")
        fails += [f"{p['name']}: {f}" for f in DC.check_pooled("normal", DC.pool_reference("normal", c0, c1), dk)]
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("side", (0, 1))
def test_dense_mutations_are_multiplied_out_as_given(raw, side):
    """Each mutation of a tokeniser's matrix alone, on A0 only / A1 only: the verdict holds exactly the expected bits and Dk is the
    product as given.  (For all but the one-ulp weights a pooled answer would miss the bar by a factor above 100 -- CPU premise;
    the one-ulp weights are what the verdict read-back is for.)"""
    fails = []
    for name in DC.mutation_names():
        c = DC.dense_mutation_case(side, name)
        code, dk, word, _ = raw.dense(c["D"], c["A0"], c["A1"])
        assert code == 0, c["name"]
        if word != c["verdict"]:
            fails.append(f"{c['name']}: verdict {word}, expected {c['verdict']}")
        fails += [f"{c['name']}: {f}" for f in DC.check_product(c, dk)]
    assert not fails, "\n".join(fails[:20])


def test_dense_as_given_shapes(raw):
    """dense random matrices at k1 = 1, 3, 4, 5 (four waves per block) and n1 around the 64-lane stride and the 256-column block;
    K > N: the verdict is exactly 1 (nothing inspected, the pooling launch skipped)"""
    fails = []
    for c in DC.as_given_cases():
        code, dk, word, _ = raw.dense(c["D"], c["A0"], c["A1"])
        assert code == 0, c["name"]
        if word != c["verdict"]:
            fails.append(f"{c['name']}: verdict {word}, expected {c['verdict']}")
        fails += [f"{c['name']}: {f}" for f in DC.check_product(c, dk)]
    assert not fails, "\n".join(fails[:20])


def test_dense_engine_wrapper_reads_the_verdict_back(raw):
    eng = raw.eng
    clean, ulp = DC.dense_mutation_case(0, None), DC.dense_mutation_case(0, "ulp_up@straddle_last")
    for c in (clean, ulp):
        dk, verdict = eng.pool_distmat_dense(raw.up(c["D"]), raw.up(c["A0"]), raw.up(c["A1"]), return_verdict=True)
        assert verdict == c["verdict"] and not DC.check_product(c, dk.cpu().numpy())
        assert torch.equal(eng.pool_distmat_dense(raw.up(c["D"]), raw.up(c["A0"]), raw.up(c["A1"])), dk)
    dk, verdict = eng.pool_distmat_dense(torch.zeros((0, 7), device="cuda"), torch.zeros((3, 0), device="cuda"), torch.ones((2, 7), device="cuda"), return_verdict=True)
    assert verdict is None and dk.shape == (3, 2) and not dk.any()


def test_dense_empty_inner_dimension(raw):
    """n0 = 0 or n1 = 0: a zero matrix, and the verdict word is not written"""
    rs = np.random.RandomState(3)
    for (k0, n0), (k1, n1) in (((3, 0), (2, 7)), ((3, 5), (4, 0)), ((1, 0), (1, 0))):
        A0, A1 = rs.uniform(-1, 1, (k0, n0)).astype(np.float32), rs.uniform(-1, 1, (k1, n1)).astype(np.float32)
        code, dk, word, _ = raw.dense(rs.uniform(0, 4, (n0, n1)).astype(np.float32), A0, A1)
        assert code == 0 and dk.shape == (k0, k1) and not dk.any() and not np.signbit(dk).any()
        assert word == np.int32(DC.WS_WORD)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(raw):
    """null pointers, a workspace one byte short, k0 > n0 for the map form: the error code, nothing launched.  (linetr_match_distmat
    checks its pointers since the change that added this test: never point this test at an older library.)"""
    c32, c64 = DC.match_case("f32", 17, 64), DC.match_case("f64", 5, 64)
    for c in (c32, c64):
        for kw, want in ((dict(null=("dist",)), E_ARG), (dict(null=("m01",)), E_ARG), (dict(null=("ws",)), E_ARG), (dict(short=1), E_WORKSPACE)):
            code, _, buf = raw.match(c["d"], c["thr"], True, **kw)
            assert code == want and (buf == MARKER_I).all(), (c["name"], kw, code)
    p = DC.pool_case("normal", (2, 3, 1), (1, 5, 2, 2))
    args = (p["D"], p["s0"], p["k0"], p["s1"], p["k1"])
    for kw, want in [(dict(null=(n,)), E_ARG) for n in ("dist", "s0", "s1", "dk", "ws")] + [(dict(short=1), E_WORKSPACE)]:
        code, _, buf = raw.pool(*args, **kw)
        assert code == want and (buf == MARKER).all(), (kw, code)
    code, _, buf = raw.pool(p["D"], p["s0"], p["n0"] + 1, p["s1"], p["k1"])              # k0 > n0
    assert code == E_ARG and (buf == MARKER).all()
    code, _, buf = raw.pool(p["D"], p["s0"], p["k0"], p["s1"], p["n1"] + 1)              # k1 > n1
    assert code == E_ARG and (buf == MARKER).all()
    A0, A1 = pool_matrix(p["c0"], np.float32), pool_matrix(p["c1"], np.float32)
    for kw, want in [(dict(null=(n,)), E_ARG) for n in ("dist", "A0", "A1", "dk", "ws")] + [(dict(short=1), E_WORKSPACE)]:
        code, _, word, buf = raw.dense(p["D"], A0, A1, **kw)
        assert code == want and (buf == MARKER).all() and word == np.int32(DC.WS_WORD), (kw, code)
    torch.cuda.synchronize()
