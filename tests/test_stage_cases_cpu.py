"""CPU: the references of the stage unit tests (stage_cases.py) are pinned to the oracle that tests/test_oracle_golden.py pins to the
reference; linetr_create's folds, restated and evaluated in float32, sit well inside every bar of tests/test_gpu_stages.py; and each
of ten planted mistakes in that restatement breaks a bar on at least one of those cases -- so the GPU tests can catch them."""
import pytest
import torch

import front_cases as FC
import stage_cases as S
from oracle import linetr_oracle as O
from workloads import synth

torch.set_grad_enabled(False)


def test_stage_references_are_the_oracles_forward():
    """pool_reference (float64) -> tail reference -> signature reference equals oracle.forward(...)['line_desc'] in float64 to 1e-12 on a
    tokenised image whose sub-lines carry padding, at every depth the GPU tests use."""
    hw = (480, 640)
    dd, ds = synth.synth_dense_maps(11, *hw)
    cfg = dict(min_length=16, token_distance=8, max_tokens=5, remove_borders=8, max_keylines=-1)
    data = O.preprocess(synth.array_to_keylines(synth.synth_lines(5, 14, *hw)), (1, 1, *hw), dd, ds, cfg)
    N, T = data["pnt_sublines"].shape[1:3]
    assert float(data["mask_sublines"].min()) == 0.0 and N > data["klines"].shape[1]
    data64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.items()}
    pnt, score = data["pnt_sublines"][0].reshape(N * T, 2), data["score_sublines"][0].reshape(N * T)
    desc = data["desc_sublines"][0].reshape(N * T, 256)
    line_in = (data["sublines"][0].reshape(N, 4), data["resp_sublines"][0].reshape(N), data["angle_sublines"][0])
    for weights in S.WEIGHTS:
        for L in S.DEPTHS:
            sd64 = S._cast(weights, L, torch.float64)
            want = O.forward(sd64, dict(data64), hw)["line_desc"][0].t()
            a4 = FC.mlp4(sd64, "word", FC.enc_features("word", (pnt, score), torch.float64), torch.float64)
            pooled = FC.pool_reference(sd64, desc, a4, torch.arange(N * T).view(N, T), torch.float64)
            lpos = O._mlp(sd64, FC.ENC["line"], FC.enc_features("line", line_in, torch.float64))
            z0 = S.tail_z(sd64, S.tail_o(sd64, S.tail_att(sd64, pooled)), lpos)
            got, outs = S.sig_chain(sd64, z0, [0, N])
            assert len(outs) == L and float((got - want).abs().max()) < 1e-12, (weights, L)


def _folded_rows(weights, mistake=None):
    """(what, rows of the error measure) of every case of the GPU tests with the folded float32 graph in the device's place"""
    tail_only = mistake in ("ln_eps_1e-5", "fc_bias_without_cls", "b5_not_scaled_by_1_minus_p0", "gelu_tanh")
    if mistake is None or tail_only:
        for c in S.tail_cases():
            yield f"tail {c['family']} N={c['N']}", S.tail_errors(S.folded_tail(c, weights, mistake), c, weights)
    if mistake is None or not tail_only:
        for L in S.DEPTHS:
            for fold_next in (False, True):
                for c in S.sig_cases():
                    desc, taps = S.folded_sig(c, weights, L, fold_next, mistake)
                    yield f"sig L={L} fold_next={fold_next} {c['family']}", S.sig_errors(desc, taps, c, weights, L)


def test_folded_float32_graph_sits_inside_every_bar():
    """The folds restated (float64, rounded once) and evaluated in float32, image by image as the references are, leave the kernels
    headroom.  Measured here: the tail at most 0.13 of its bar, the plain route of the signature network at most 0.23 (under the half
    that was expected of it), the fold_next route up to 0.59 with the seed-3 weights (0.43 calibrated): there the next layer's q/k/v
    are Wqkv z + (Wqkv W2) hid instead of Wqkv (z + W2 hid), two larger terms that partly cancel, and that costs float32 digits at any
    input scale (0.25 .. 2 x tried).  It is a property of that fold, not of a case, so the route is asserted inside its bar only."""
    top = {}
    for weights in S.WEIGHTS:
        for what, rows in _folded_rows(weights):
            assert rows
            top[(weights, what)] = S.worst(rows)
    for k, v in sorted(top.items(), key=lambda kv: -kv[1])[:8]:
        print(f"folded float32 graph: {k[0]} / {k[1]}: worst error / bar {v:.3f}")
    plain = {k: v for k, v in top.items() if "fold_next=True" not in k[1]}
    assert max(plain.values()) < 0.5, max(plain.items(), key=lambda kv: kv[1])
    assert max(top.values()) < 1.0, max(top.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_planted_mistake_breaks_a_bar(mistake):
    """One mistake planted in the restatement of the folds / the graph: at least one case of the GPU tests ends over its bar."""
    worst = max(S.worst(rows) for weights in S.WEIGHTS for _, rows in _folded_rows(weights, mistake))
    print(f"{mistake}: worst error / bar {worst:.1f}")
    assert worst > 1.0, f"{mistake} stays under every bar (worst error / bar {worst:.3f})"


def test_tail_pad_family_is_normal_with_filled_pad_columns_and_cases_cover_the_issue():
    for N in S.TAIL_N:
        a, b = S.tail_case("normal", N), S.tail_case("pad", N)
        assert torch.equal(a["pooled"][:, :, :513], b["pooled"][:, :, :513]) and torch.equal(a["lpos"], b["lpos"])
        assert float(a["pooled"][:, :, 513:].abs().max()) == 0.0 and float(b["pooled"][:, :, 513:].abs().min()) == S.SENTINEL
        e = S.tail_case("p0_ends", N)["pooled"][:, :, 512]
        assert set(e.unique().tolist()) <= {0.0, 1.0} and (N < 2 or len(e.unique()) == 2)
    assert sum(S.SIG_COUNTS) == 165 and S.cu_of(S.SIG_COUNTS)[-1] == 165
    checked = [set(c["check"]) for c in S.sig_cases()]
    assert checked[1] | checked[2] == checked[0] == set(range(5)) and not checked[1] & checked[2]
