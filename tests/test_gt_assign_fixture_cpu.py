"""CPU: the NumPy restatement of the ground-truth line assignment (tests/gt_assign_reference.py) against the fixture the REAL
reference wrote (tests/golden/gt_assign.npz, tests/golden/make_golden_gt_assign.py), in both dtypes, bit for bit -- which is also
the check that `x * x` stands for NumPy's float32 `** 2` on the fixture's data -- the order and padding of the match list, and the
premise the GPU test rests on: no angle compare of the fixture or of any GPU case lies inside the band in which two correct
arctan2 implementations may disagree, so the GPU test may demand identity."""
import numpy as np
import pytest

from helpers import load
import gt_assign_reference as R

DTYPES = [(np.float32, "f32"), (np.float64, "f64")]


@pytest.fixture(scope="module")
def fix():
    g = load("gt_assign")
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_restatement_equals_the_reference(fix, dtype, tag):
    lines0, lines1, H = fix[f"lines0_{tag}"], fix[f"lines1_{tag}"], fix["H"]
    assert lines0.dtype == dtype and lines0.shape == (3, 48, 2, 2) and lines1.shape == (3, 40, 2, 2)
    # the case builder still builds the fixture's inputs
    again = R.case(int(fix["seed"]), 3, 48, 40, dtype)
    assert all(np.array_equal(a, b) for a, b in zip(again, (lines0, lines1, H)))
    got = R.batch_truth(lines0, lines1, H)
    assert np.array_equal(got["proj0"], fix[f"proj0_{tag}"]) and np.array_equal(got["proj1"], fix[f"proj1_{tag}"])
    assert np.array_equal(got["match0"], fix[f"match0_{tag}"] > 0) and np.array_equal(got["match1"], fix[f"match1_{tag}"] > 0)
    both = got["match0"] & got["match1"]
    for d in ("0", "1"):
        assert np.array_equal(np.where(both, got["overlap" + d], 0).astype(np.float64), fix[f"overlap{d}_{tag}"])
        ex = fix["extra_pairs"]
        assert np.array_equal(got["overlap" + d][:, ex[:, 0], ex[:, 1]].astype(np.float64), fix[f"extra_overlap{d}_{tag}"])
    assert np.array_equal(got["assign"].astype(np.float64), fix[f"assign_{tag}"])
    assert np.array_equal([len(lm) for lm in got["lmatches"]], fix[f"found_{tag}"])
    M = fix[f"lmatches_{tag}"].shape[1]
    assert M == int(48 * 1.5) and np.array_equal(R.padded_list(got["lmatches"], M), fix[f"lmatches_{tag}"])


def test_fixture_holds_what_it_is_meant_to_hold(fix):
    for _, tag in DTYPES:
        m0, m1, a = fix[f"match0_{tag}"] > 0, fix[f"match1_{tag}"] > 0, fix[f"assign_{tag}"]
        assert (m0 != m1).any()                                           # an asymmetric match
        assert ((a > 0) & (a <= 0.3)).any() and ((a > 0.3) & (a < 1)).any() and (a == 1).any()
        assert (fix[f"extra_overlap0_{tag}"] == 0).any() and (fix[f"extra_overlap0_{tag}"] == 1).any()     # apart, touching
        l1, l0 = fix[f"lines1_{tag}"], fix[f"lines0_{tag}"]
        assert np.array_equal(l1[:, R.ZERO_LENGTH_COL, 0], l1[:, R.ZERO_LENGTH_COL, 1])                     # a zero-length line
        assert (fix[f"proj0_{tag}"][:, R.ZERO_W_ROW, 1] == 0).all() and (l0[:, R.ZERO_W_ROW, 1] != 0).any()   # w = 0 projects to (0, 0)
    assert (fix["assign_f32"].astype(np.float32) != fix["assign_f64"].astype(np.float32)).any()             # the dtypes disagree


def test_list_order_and_padding(fix):
    for _, tag in DTYPES:
        lm, found, a = fix[f"lmatches_{tag}"], fix[f"found_{tag}"], fix[f"assign_{tag}"]
        for b in range(len(lm)):
            k = int(found[b])
            assert (lm[b, k:] == -1).all() and (lm[b, :k] >= 0).all()
            flat = lm[b, :k, 0] * a.shape[2] + lm[b, :k, 1]
            assert (np.diff(flat) > 0).all()                                                                # row-major, no repeats
            assert np.array_equal(np.array(np.where(a[b] > 0.3)).T, lm[b, :k])
    cut = R.padded_list([np.arange(10).reshape(5, 2)], 3)
    assert cut.shape == (1, 3, 2) and np.array_equal(cut[0], np.arange(6).reshape(3, 2))


@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_band_premise(fix, dtype, tag):
    """no angle compare within the band: of the fixture, and of every case the GPU test builds"""
    assert R.batch_truth(fix[f"lines0_{tag}"], fix[f"lines1_{tag}"], fix["H"])["margin"] >= R.BAND[dtype]
    for (n0, n1), seed in R.EDGE_CASES.items():
        lines0, lines1, H = R.case(seed, R.EDGE_B, n0, n1, dtype)
        assert R.batch_truth(lines0, lines1, H)["margin"] >= R.BAND[dtype], (n0, n1)


def test_zero_w_point_is_exact():
    from workloads import synth
    for seed in range(5):
        H, (x, y) = R.zero_w_point(synth.pixel_homography(np.random.RandomState(seed), 480, 640, 0.3))
        assert np.float32(x) == x and np.float32(y) == y
        assert x * H[2, 0] + y * H[2, 1] + H[2, 2] == 0.0
        assert (R.project(np.array([[x, y]], np.float32), H) == 0).all()
