"""CPU (no GPU needed): the references of tests/test_gpu_dropout.py are what they claim to be.  The NumPy Philox4x32-10 gives the known
answers and keeps the fraction it should; the torch restatement of the UNFOLDED layer with explicit masks reproduces
tests/golden/desc_layer_dropout.npz, which autograd through the REAL reference wrote with its nn.Dropout instances replaced by the same
masks (tests/golden/make_golden_desc_layer_dropout.py); the folded graph with masks equals it in float64, whatever rows 1 .. S-1 of the
masks hold; the float64 closed forms equal float64 autograd; each planted mistake falls outside its bar; small segments do lose all
their tokens at p = 0.5, which is what the exact-zero tests on the device stand on."""
import os

import numpy as np
import pytest
import torch

from helpers import load
import desc_layer_reference as DL
import dropout_reference as DR

HERE = os.path.dirname(os.path.abspath(__file__))


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1.0)


def test_philox_known_answers():
    for counter, key, want in DR.KNOWN_ANSWERS:
        got = DR.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want, (counter, key, [hex(int(w)) for w in got])
    # vectorised over the counter: the same words as one call at a time
    w = DR.words(DR.BIG_SEED, 7, 2, 3, 5)
    for row in range(3):
        for inner in range(5):
            one = DR.philox4x32_10((inner, row, 7, 2), (DR.BIG_SEED & 0xffffffff, DR.BIG_SEED >> 32))
            assert [int(v) for v in one] == [int(v) for v in w[row, inner]]


@pytest.mark.parametrize("site,shape,call", [(0, (4096, 64), 0), (1, (1024, 64), 3), (2, (1024, 64), 3)])
def test_keep_fractions(site, shape, call):
    for p in (0.0,) + DR.P_VALUES:
        T = DR.threshold(p)
        assert T == int(np.floor(p * 2.0 ** 32)) and DR.scale(p) == np.float32(1.0 / (1.0 - p))
        f = DR.factors(DR.SEED, call, site, *shape, p)
        assert f.shape == shape + (4,) and f.dtype == np.float32 and set(np.unique(f).tolist()) <= {0.0, float(DR.scale(p))}
        n, q = f.size, 1.0 - T / 2.0 ** 32
        z = ((f != 0).sum() - n * q) / np.sqrt(n * q * (1.0 - q)) if p else 0.0
        print(f"dropout keep fraction site {site} p={p}: kept {(f != 0).mean():.5f} of {q:.5f}, z = {z:+.2f}")
        assert abs(z) <= 4.0 and (p or f.all())
    # the call, the site and the seed each change the table
    base = DR.factors(DR.SEED, call, site, 16, 64, 0.5)
    for other in (DR.factors(DR.SEED, call + 1, site, 16, 64, 0.5), DR.factors(DR.SEED, call, (site + 1) % 3, 16, 64, 0.5),
                  DR.factors(DR.SEED + (1 << 32), call, site, 16, 64, 0.5)):
        assert 0.3 < (other != base).mean() < 0.7


def test_masked_restatement_reproduces_the_fixture():
    f = load("desc_layer_dropout")
    assert os.path.getsize(os.path.join(HERE, "golden", "desc_layer_dropout.npz")) < 1 << 20
    assert int(f["seed"]) == DR.SEED and int(f["call"]) == 0 and tuple(f["p_values"]) == DR.P_VALUES
    plain = load("desc_layer")
    for p in DR.P_VALUES:
        ref64, ref32 = DR.module_refs(*DL.FIXTURE_SHAPE, p)
        assert len(ref64) == 18
        for key, val in ref64.items():
            want, yard = f[DR.fixture_key(key, p)], float(f[DR.fixture_key(key, p) + "_f32_err"])
            val, mine32 = DR.fixture_grid(key, val), DR.fixture_grid(key, ref32[key])
            assert want.shape == val.shape and want.dtype == np.float64, key
            bar = DL.FACTOR * max(yard, 2.0 ** -23 * np.abs(want).max())
            assert np.abs(val - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), (p, key)        # the float64 runs agree to rounding
            assert 0 < yard < 1e-3 and np.abs(mine32 - want).max() <= bar, (p, key)                  # the float32 run sits inside the bar
        assert np.abs(f[DR.fixture_key("slf_attn.w_ks.bias", p)]).max() < 1e-13                     # still zero in exact arithmetic
        # and dropout is not a detail: the output is far from the fixture without it
        assert np.abs(f[DR.fixture_key("out", p)] - plain["out"]).max() > 0.05


@pytest.mark.parametrize("shape", DR.MODULE_SHAPES[:2] + ((2, 9, 3),))
@pytest.mark.parametrize("p", DR.P_VALUES)
def test_folded_equals_unfolded_in_float64(shape, p):
    sd, desc, g = DL.module_case(*shape)
    unfolded = DR.run_layer(sd, desc, g, torch.float64, p)
    folded = DR.run_layer(sd, desc, g, torch.float64, p, folded=True)
    for key, val in unfolded.items():
        assert rel(folded[key], val) <= 1e-12, (shape, p, key)
    # rows 1 .. S-1 of the three masks never reach row 0
    other = DR.run_layer(sd, desc, g, torch.float64, p, other=DR.OTHER_ROWS_SEED + 1)
    for key, val in unfolded.items():
        assert rel(other[key], val) <= 1e-12, (shape, p, key)
    if shape[2] > 1:
        a, b = DR.masks(*shape, DR.SEED, 0, p), DR.masks(*shape, DR.SEED, 0, p, other=DR.OTHER_ROWS_SEED + 1)
        assert all((x[..., 1:, :] != y[..., 1:, :]).any() and np.array_equal(x[..., 0, :], y[..., 0, :]) for x, y in zip(a, b))


def test_closed_forms_equal_float64_autograd():
    for family in DR.POOL_FAMILIES:
        for L, S in ((1, 1), (3, 2), (5, 22), (9, 3)):
            for p in DR.P_VALUES:
                c = DR.pool_case(family, L, S, p)
                ag = DR.pool_torch(c["x"], c["u"], c["dpooled"], c["dkept"], c["r"], torch.float64)
                for key in DR.POOL_OUTPUTS:
                    assert rel(c["ref64"][key], ag[key]) <= 1e-12, (family, L, S, p, key)
    for residual in (False, True):
        for site in (1, 2):
            c = DR.ln_case(5, residual, site, 0.1)
            ag = DR.ln_torch(c["a"], c["r"], c["gamma"], c["beta"], c["g"], c["fac"], torch.float64)
            assert sorted(ag) == sorted(c["ref64"]) and ("dr" in ag) == residual
            for key, val in ag.items():
                assert rel(c["ref64"][key], val) <= 1e-11, (residual, site, key)
    # p = 0: the factors are all 1 and the closed forms are those without dropout
    c, base = DR.pool_case("normal", 5, 22, 0.0), DL.pool_case("normal", 5, 22)
    assert (c["r"] == 1.0).all() and np.abs(c["ref64"]["kept"] - 1.0).max() < 1e-15
    zero_dkept = DR.pool_closed_form(c["x"], c["u"], c["dpooled"], np.zeros_like(c["dkept"]), c["r"])
    for key in DL.POOL_OUTPUTS:
        assert np.array_equal(zero_dkept[key], base["ref64"][key]), key


def test_planted_mistakes_fall_outside_the_bar():
    # the value bias not scaled by kept: the output, and above all the value bias's own gradient
    sd, desc, g = DL.module_case(*DL.FIXTURE_SHAPE)
    ref64, ref32 = DR.module_refs(*DL.FIXTURE_SHAPE, 0.1)
    good = DL.ratios(DR.run_layer(sd, desc, g, torch.float32, 0.1, folded=True), ref64, ref32)
    print(f"dropout folded float32 {DL.FIXTURE_SHAPE} p=0.1: worst error / bar {DL.worst(good):.3f}")
    assert len(good) == 18 and not DL.failures(good), DL.failures(good)
    bad = DL.ratios(DR.run_layer(sd, desc, g, torch.float32, 0.1, folded=True, mistake="bias_not_kept"), ref64, ref32)
    assert DL.failures([r for r in bad if r[0] == "out"]) and DL.failures([r for r in bad if r[0] == "slf_attn.w_vs.bias"])
    # delta without its dkept kept term
    c = DR.pool_case("normal", 5, 22, 0.1)
    bad = DR.pool_closed_form(c["x"], c["u"], c["dpooled"], c["dkept"], c["r"], mistake="delta_without_kept")
    assert DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("dx",))) and DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("du",)))
    assert not DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("pooled", "kept", "lse")))
    # the residual's gradient scaled by the factors
    c = DR.ln_case(5, True, 1, 0.1)
    bad = DR.ln_closed_form(c["a"], c["r"], c["gamma"], c["beta"], c["g"], c["fac"], mistake="dr_scaled")
    assert DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("dr",))) and not DL.failures(DL.ratios(bad, c["ref64"], c["ref32"], ("da", "y")))


def test_small_segments_lose_all_their_tokens_at_one_half():
    """seed 2026, call 0, p = 0.5, L = 9: (segment, head) pairs all of whose tokens are dropped exist at every small S -- 16, 6 and 3 of
    36 at S = 1, 2, 3 -- and are not the rule; their pooled and kept are exact zeros and nothing reaches x or u through them"""
    for S in (1, 2, 3):
        gone = DR.all_dropped(DR.SEED, 0, 9, S, 0.5)
        print(f"dropout all-dropped pairs at S = {S}: {int(gone.sum())} of {gone.size}")
        assert gone.shape == (9, 4) and 0 < gone.sum() < 36
        c = DR.pool_case("normal", 9, S, 0.5)
        assert not c["ref64"]["pooled"][gone].any() and not c["ref64"]["kept"][gone].any() and np.isfinite(c["ref64"]["dx"]).all()
        # gradients arriving at the all-dropped pairs alone go nowhere
        only = DR.pool_closed_form(c["x"], c["u"], c["dpooled"] * gone[:, :, None], c["dkept"] * gone, c["r"])
        assert not only["du"].any() and not only["dx"].any()
