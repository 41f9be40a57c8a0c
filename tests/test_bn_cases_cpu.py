"""CPU: pins the references and the bar of the train-mode BatchNorm unit tests (bn_cases.py) before a GPU is involved.

ref64 agrees with torch.nn.BatchNorm1d in .double().train() and, for the encoder chains, with the oracle's train-mode restatement
(oracle.linetr_oracle._mlp_train); the CPU statement of the kernels' arithmetic (bn_cases.kernel_model) stays inside the bar on every
case of the list, and three planted mistakes applied to it do not -- so the bar is neither unreachable nor loose; the case list
holds every chunk count and rows-in-parallel class the kernels' host code and loops distinguish."""
import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC
import front_cases as FC
from oracle import linetr_oracle as O

torch.set_grad_enabled(False)

SMALL = [k for k in BC.layer_cases() if not BC.is_big(k)]
BIG = [k for k in BC.layer_cases() if BC.is_big(k)]


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("family", BC.FAMILIES)
def test_ref64_is_torch_batchnorm1d_in_double(family):
    """Output, running mean and running variance to 1e-12 of each tensor's largest entry, on every small case of the family
    (torch refuses rows = 1 in training mode: those cases are pinned by test_single_row_is_the_documented_limit)."""
    bad = []
    for key in SMALL:
        if key[0] != family or key[3] == 1:
            continue
        case = BC.layer_case(*key)
        C = case["C"]
        bn = torch.nn.BatchNorm1d(C, eps=BC.EPS, momentum=case["momentum"]).double().train()
        bn.weight.copy_(case["gamma"]); bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running"][:C]); bn.running_var.copy_(case["running"][C:])
        y = F.relu(bn(case["z"].double()))
        r = case["ref64"]
        for what, a, b in (("y", r["y"], y), ("running mean", r["run_mean"], bn.running_mean), ("running var", r["run_var"], bn.running_var)):
            if not rel(a, b) <= 1e-12:
                bad.append(f"{key} {what}: {rel(a, b):.3e}")
    assert not bad, "\n".join(bad)


def test_single_row_is_the_documented_limit():
    """rows = 1: var = 0, y = relu(beta), running mean moved towards z, running variance towards 0 (unbiased factor taken as 1)"""
    keys = [k for k in SMALL if k[3] == 1]
    assert {k[0] for k in keys} == set(BC.PLAIN)
    for key in keys:
        case = BC.layer_case(*key)
        r, C, m = case["ref64"], case["C"], case["momentum"]
        assert bool((r["var"] == 0).all()) and bool(torch.isfinite(r["y"]).all())
        assert torch.equal(r["y"], F.relu(case["beta"].double())[None])
        assert torch.allclose(r["run_var"], (1 - m) * case["running"][C:].double(), rtol=1e-15, atol=0)
        assert torch.allclose(r["run_mean"], (1 - m) * case["running"][:C].double() + m * case["z"][0].double(), rtol=1e-15, atol=1e-300)


def test_constant_channels_have_no_variance():
    for key in SMALL:
        if key[0] != "constant":
            continue
        case = BC.layer_case(*key)
        c = torch.arange(case["C"])
        flat = (c % 4 == 0) | (c % 4 == 2)
        assert bool((case["ref64"]["var"][flat] == 0).all()), key
        assert torch.equal(case["ref64"]["y"][:, flat], F.relu(case["beta"].double())[flat].expand(case["rows"], -1)), key
        assert bool(torch.isfinite(case["ref32"]["y"]).all())


@pytest.mark.parametrize("enc", ["word", "line"])
@pytest.mark.parametrize("widths", BC.CHAIN_WIDTHS)
def test_chain_ref64_is_the_oracles_train_mode_mlp(enc, widths):
    """oracle._mlp_train runs the encoder to its last linear layer and updates the state dict's running statistics in place: in
    float64 it must give W5 ref64 + b5 and ref64's running statistics, to 1e-12."""
    for weights in BC.CHAIN_WEIGHTS:
        sd64 = {k: v.double() if v.is_floating_point() else v.clone() for k, v in BC.chain_state_dict(weights, widths)[1].items()}
        pre = FC.ENC[enc]
        running = torch.cat([torch.cat([sd64[f"{pre}.{3 * i + 1}.running_mean"], sd64[f"{pre}.{3 * i + 1}.running_var"]]) for i in range(4)])
        for rows in (33, 193):
            inputs = FC._mlp_inputs(enc, "workload", rows, BC._gen("oracle pin", enc, rows))
            feats = FC.enc_features(enc, inputs, torch.float64)
            sd = {k: v.clone() for k, v in sd64.items()}
            ref = BC.chain_reference(sd, enc, feats, running, 0.1, torch.float64)
            out = O._mlp_train(sd, pre, feats, 0.1)
            want = F.linear(ref["y"], sd64[pre + ".12.weight"][:, :, 0], sd64[pre + ".12.bias"])
            assert rel(want, out) <= 1e-12
            got_mean = torch.cat([sd[f"{pre}.{3 * i + 1}.running_mean"] for i in range(4)])
            got_var = torch.cat([sd[f"{pre}.{3 * i + 1}.running_var"] for i in range(4)])
            assert rel(ref["run_mean"], got_mean) <= 1e-12 and rel(ref["run_var"], got_var) <= 1e-12


def _model_ratios(keys):
    bad, top = [], 0.0
    for key in keys:
        case = BC.layer_case(*key)
        rows = BC.layer_errors(BC.kernel_model(case), case)
        bad += [f"{key}: {m}" for m in BC.failures(rows)]
        w = BC.worst(rows)
        top = max(top, w[2] / w[3] if w[3] else 0.0)
    return bad, top


def test_kernel_model_is_inside_the_bar_small():
    bad, top = _model_ratios(SMALL)
    print(f"kernel model, {len(SMALL)} cases: worst error / bar {top:.3f}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("C", BC.BIG_CHANNELS)
def test_kernel_model_is_inside_the_bar_big(C):
    keys = [k for k in BIG if k[1] == C]
    assert len(keys) == len(BC.BIG_ROWS) + 1
    bad, top = _model_ratios(keys)
    print(f"kernel model, C = {C}, {len(keys)} cases: worst error / bar {top:.3f}")
    assert not bad, "\n".join(bad)


PLANTED = [("unbiased_norm", ("workload", 32, 32, 65, 0.1, 0.0)), ("unbiased_norm", ("workload", 100, 100, 257, 0.1, 0.0)),
           ("unbiased_norm", ("workload", 32, 32, 32769, 0.1, 0.0)),
           ("drop_last_chunk", ("workload", 32, 32, 129, 0.1, 0.0)), ("drop_last_chunk", ("workload", 260, 260, 333, 0.1, 0.0)),
           ("drop_last_chunk", ("workload", 32, 32, 32769, 0.1, 0.0)),
           ("float_acc", ("offset", 32, 32, 65, 0.1, 256.0)), ("float_acc", ("offset", 100, 100, 257, 0.1, 4096.0)),
           ("float_acc", ("offset", 512, 512, 333, 0.1, 256.0))]


@pytest.mark.parametrize("mistake,key", PLANTED)
def test_planted_mistake_is_outside_the_bar(mistake, key):
    """the same model with one mistake: y AND at least one statistics vector leave the bar, while the clean model stays inside"""
    case = BC.layer_case(*key)
    assert not BC.failures(BC.layer_errors(BC.kernel_model(case), case))
    rows = BC.layer_errors(BC.kernel_model(case, mistake), case)
    failed = [r for r in rows if not r[2] <= r[3]]
    assert any(isinstance(r[0], int) for r in failed), (mistake, key, "no tile of y left the bar")
    if mistake != "unbiased_norm":            # (that one touches alpha alone among the statistics)
        assert any(r[0] in ("mean", "var") for r in failed), (mistake, key, "the batch statistics stayed inside the bar")
    else:
        assert any(r[0] == "alpha" for r in failed), (mistake, key, "alpha stayed inside the bar")


def test_the_list_holds_every_chunk_and_lane_class():
    keys = BC.layer_cases()
    assert len(set(keys)) == len(keys)
    assert {k[0] for k in keys} == set(BC.FAMILIES) and {k[4] for k in keys} == set(BC.MOMENTA)
    assert {k[5] for k in keys if k[0] == "offset"} == set(BC.RATIOS)
    for C in BC.CHANNELS:
        mine = [k for k in keys if k[1] == C]
        assert set(BC.ROWS) <= {k[3] for k in mine if k[2] == C}                         # every row count at ld = C
        assert {C + 4, 2 * C} <= {k[2] for k in mine}                                    # both wider strides
        assert set(BC.PLAIN) <= {k[0] for k in mine} and set(BC.MOMENTA) <= {k[4] for k in mine}
    # chunk counts: 1 (below 128 rows), 2, 3, 4, 5, 511, 512 with and without empty trailing blocks
    nbs = {BC.n_chunks(k[3]) for k in keys}
    assert {1, 2, 3, 4, 5, 511, 512} <= nbs
    for C in BC.BIG_CHANNELS:
        assert set(BC.BIG_ROWS) <= {k[3] for k in keys if k[1] == C}
    rows = 32769
    chunk = -(-rows // BC.n_chunks(rows))
    assert BC.n_chunks(rows) == 512 and chunk == 65 and 512 - -(-rows // chunk) == 7    # the last seven blocks own no rows
    assert -(-BC.BIG_ROWS[3] // 512) == 193                                              # chunks longer than 64 rows
    # rows in parallel: every rp class, widths that leave lanes without a row (256 % cw != 0), the uneven second channel pass
    rps = {BC.rows_in_parallel(C) for C in BC.CHANNELS}
    assert {rp for _, rp in rps} == {64, 32, 8, 4, 2, 1}
    assert any(256 % cw for cw, _ in rps) and {260, 384, 508} <= set(BC.CHANNELS)
    # a chunk size that rp does not divide, for every rp > 1
    for C in BC.CHANNELS:
        rp = BC.rows_in_parallel(C)[1]
        if rp > 1:
            assert any((-(-k[3] // BC.n_chunks(k[3]))) % rp for k in keys if k[1] == C), C
    assert {k[0] for k in keys if k[3] == 1} >= set(BC.PLAIN)
    assert set(BC.CHAIN_ROWS) == {33, 64, 65, 193, 4378}
    assert {BC.rows_in_parallel(C)[1] for w in BC.CHAIN_WIDTHS for C in w} == {8, 4, 2, 1} and 320 in BC.CHAIN_WIDTHS[1]
