"""No GPU: the fixed-size sample fixture (tests/golden/fixed_size.npz, the real conv_fixed_size) against its NumPy restatement on
top of the per-image oracle, and the library's host pseudo-line generator against its pure-Python restatement."""
import math

import numpy as np

import fixed_size_reference as R


def test_restated_conv_fixed_size_equals_the_reference_fixture():
    g = R.fixture()
    names = R.cases(g)
    assert len(names) == 8
    for name in names:
        R.check_against_fixture(g, name, R.oracle_case(g, name))


def test_fixture_hits_every_branch():
    g = R.fixture()
    k = {n: int(g[f"{n}_num_klns"][0]) for n in R.cases(g)}
    s = {n: int(g[f"{n}_num_slns"][0]) for n in R.cases(g)}
    M = {n: int(g[f"{n}_M"]) for n in R.cases(g)}
    assert k["pad_stray"] < s["pad_stray"] < M["pad_stray"]
    mat = g["pad_stray_mat_klines2sublines"][0]
    j = k["pad_stray"]                                   # a row behind the key-lines, inside the real columns: the stray diagonal 1
    assert j < s["pad_stray"] and mat[j, j] == 1.0 and mat[:k["pad_stray"], j].sum() == 1.0
    assert k["exact"] == s["exact"] == M["exact"] and int(g["exact_n_pseudo"]) == 0
    assert s["cut_unsplit"] > M["cut_unsplit"] and s["cut_straddle"] > M["cut_straddle"]
    mat = g["cut_straddle_mat_klines2sublines"][0]
    owner = int(np.flatnonzero(mat[:k["cut_straddle"], M["cut_straddle"] - 1])[0])
    assert 0 < mat[owner].sum() < 1.0                    # the cut fell inside this key-line's sub-lines: its row no longer sums to 1
    assert k["klns_eq_max"] == M["klns_eq_max"] < s["klns_eq_max"]
    assert k["mostly_pseudo"] == s["mostly_pseudo"] == 1 and int(g["mostly_pseudo_n_pseudo"]) == 15
    assert s["big_pad"] < 250 < s["big_cut"] and M["big_pad"] == M["big_cut"] == 250


def test_host_generator_equals_its_restatement_bit_for_bit():
    from linetr_amd import util_lines as U
    for seed, image, n, shape in ((0, 0, 40, (640, 480)), (7, 3, 25, (640, 480)), (123456789, 31, 17, (320, 240)), (1, 0, 0, (640, 480))):
        want = R.make_pseudo_lines(seed, image, n, shape)
        got = U.make_pseudo_lines(n, shape, seed=seed, image=image)
        assert got.dtype == np.float64 and got.shape == (n, 2, 2)
        assert got.tobytes() == want.tobytes(), (seed, image)
        assert U.make_pseudo_lines(n, shape, seed=seed, image=image).tobytes() == got.tobytes()
        if n > 5:                                        # a prefix of the same stream, whatever n
            assert U.make_pseudo_lines(5, shape, seed=seed, image=image).tobytes() == got[:5].tobytes()
        a, b = U.find_line_attributes(got, 16, 250), R.find_line_attributes(want, 16, 250)
        for k in ("klines", "length_klines", "angles"):
            assert a[k].dtype == np.float64 and a[k].tobytes() == b[k].tobytes(), (seed, k)
    assert U.make_pseudo_lines(8, (640, 480), seed=1).tobytes() != U.make_pseudo_lines(8, (640, 480), seed=2).tobytes()
    assert U.make_pseudo_lines(8, (640, 480), seed=1, image=0).tobytes() != U.make_pseudo_lines(8, (640, 480), seed=1, image=1).tobytes()


def test_find_line_attributes_swaps_drops_sorts_and_breaks_ties_by_descending_index():
    from linetr_amd import util_lines as U
    lines = np.array([[[100.0, 50.0], [70.0, 10.0]],      # 50 px, end points swapped
                      [[10.0, 10.0], [40.0, 50.0]],       # 50 px: the tie, the later row comes first
                      [[10.0, 10.0], [20.0, 10.0]],       # 10 px: dropped
                      [[30.0, 30.0], [30.0, 130.0]],      # 100 px, vertical: swapped (sp_x < ep_x is false)
                      [[5.0, 5.0], [21.0, 5.0]]])         # exactly min_length: kept
    got = U.find_line_attributes(lines, 16, 250)
    assert got["length_klines"].tolist() == [100.0, 50.0, 50.0, 16.0]
    assert got["klines"].tolist() == [[[30.0, 130.0], [30.0, 30.0]], [[10.0, 10.0], [40.0, 50.0]], [[70.0, 10.0], [100.0, 50.0]],
                                      [[5.0, 5.0], [21.0, 5.0]]]
    want = R.find_line_attributes(lines, 16, 250)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    assert len(U.find_line_attributes(lines, 16, 2)["klines"]) == 2


def test_ten_thousand_generated_lines_are_valid_single_sub_lines():
    from linetr_amd import util_lines as U
    shape, n = (640, 480), 2500
    total = 0
    for image in range(4):
        lines = U.make_pseudo_lines(n, shape, seed=99, image=image)
        assert np.all(lines[:, :, 0] >= 15) and np.all(lines[:, :, 0] <= shape[0] - 15)
        assert np.all(lines[:, :, 1] >= 15) and np.all(lines[:, :, 1] <= shape[1] - 15)
        attrs = U.find_line_attributes(lines, 16, n)
        assert len(attrs["klines"]) == n                 # none shorter than min_length
        ln = attrs["length_klines"]
        assert ln.min() >= 16 and np.all(np.diff(ln) <= 0)
        n_tok = np.ceil(ln / R.TD)
        assert np.all(np.ceil(n_tok / R.T) == 1)         # exactly one sub-line each
        total += n
    assert total == 10000
    stats = []
    R.make_pseudo_lines(99, 0, 400, shape, stats=stats)
    assert max(stats) < 64 and any(a > 0 for a in stats), "the redraw path is exercised and terminates"
    assert math.isclose(float(np.mean(stats)), 0.0, abs_tol=0.5)
