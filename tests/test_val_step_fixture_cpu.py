"""CPU (no GPU needed): the NumPy restatement of the reference's validation step (tests/val_step_reference.py) in float32 reproduces
tests/golden/val_step.npz, which the REAL reference wrote (tests/golden/make_golden_val_step.py).  That pins the restatement, so
the GPU tests can use it at shapes that have no fixture."""
import numpy as np

from helpers import load
import val_step_reference as R


def test_float32_restatement_reproduces_the_reference_fixture():
    g = load("val_step")
    d0, d1, assign, thr = g["desc0"], g["desc1"], g["assign"], float(g["nn_thresh"])
    bar = float(g["ref_err_f64"])
    assert R.margins(d0, d1, assign, thr) >= R.MIN_MARGIN
    got = R.descriptor_loss(d0, d1, assign, np.float32)
    assert np.array_equal(got["rows"], g["anchor_rows"])
    assert np.abs(got["pos"] - g["dists_pos_final"]).max() <= bar and np.abs(got["neg"] - g["dists_neg_final"]).max() <= bar
    for k in ("loss", "hardest_positive", "hardest_negative"):
        assert abs(float(got[k]) - float(g[k])) <= bar, k
    for mutual, tag in ((True, "mutual"), (False, "oneway")):
        m01 = R.matcher(d0, d1, thr, mutual, np.float32)
        assert np.array_equal(R.with_dustbins(m01), g[f"mat_nn_{tag}"])
        cnt = R.counts(m01, assign)
        assert np.array_equal(cnt, g[f"tfpn_{tag}"])
        assert np.abs(R.prf(cnt) - g[f"prf_{tag}"]).max() <= 1e-9


def test_float64_restatement_selects_what_the_reference_selected():
    g = load("val_step")
    got = R.descriptor_loss(g["desc0"], g["desc1"], g["assign"], np.float64)
    assert np.array_equal(got["rows"], g["anchor_rows"])
    anchors = int((got["row_pos"] > 0).sum())
    assert len(got["rows"]) >= 20 and anchors - len(got["rows"]) >= 3
    a = g["assign"]
    assert (a == 1.0).any() and (a == np.float32(0.2)).any() and (a[:, :-1, :-1].max(axis=2) == 0).any()
