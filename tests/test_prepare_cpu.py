"""CPU: the weight preparation (linetr_amd/csrc/lt_prepare.h) against float64 restatements, bit for bit, through linetr_debug_prepare.

linetr_create rewrites the state dict before any kernel sees it: BatchNorm folds, the CLS-only pooling constants, the value path,
the CLS residual in the fc bias, head-major and scaled q/k/v, merge folded into W1, Wnext, Wfin2.  The GPU tests of the stages and of
the front end check those folds only through kernels, under a bar of eight float32 evaluation errors.  Here every prepared tensor is
compared with its restatement (tests/stage_cases.py::folded, tests/front_cases.py::_pool_consts) directly: within one float32 ulp
everywhere and bit-equal in all but 1e-5 of a tensor's elements (prepare_cases.py derives that bar), and every planted mistake
of stage_cases.MISTAKES that changes a prepared tensor lands at least 2^10 ulp outside it.  No device is touched."""
import os
import re

import numpy as np
import pytest
import torch

import bn_cases as BC
import front_cases as FC
import prepare_cases as PC
import stage_cases as SC
from linetr_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the prepared tensor every planted mistake of stage_cases.MISTAKES shows in; the two left out change only the graph
MISTAKE_TENSOR = {"wfin2_bias_without_wfin_b2": "bfin2", "mlp0_bias_without_w1b_bm": "b1m0", "bn_eps_1e-6": "b1m0",
                  "merge_columns_not_permuted": "W1m0", "q_not_scaled": "Wqkv0", "fc_bias_without_cls": "bfc",
                  "b5_not_scaled_by_1_minus_p0": "Watt", "wnext_bias_without_wqkv_b2": "bnext0"}
GRAPH_ONLY = {"gelu_tanh", "ln_eps_1e-5"}
FAR = 2.0 ** 10


def _failures(prep, want):
    """want: {entry name: float32 array}.  -> a line per tensor outside the bar (and prints every figure)"""
    bad = []
    for name, w in want.items():
        worst, differ, allowed = PC.ulp_report(prep[name], w)
        print(f"{name:8s} {w.size:8d} elements  worst {worst:.3f} ulp  not bit-equal {differ} (allowed {allowed})")
        assert prep[name].shape == tuple(w.shape), (name, prep[name].shape, w.shape)
        if not (worst <= 1.0 and differ <= allowed):
            bad.append(f"{name}: worst {worst:.3f} ulp, {differ} of {w.size} elements not bit-equal (allowed {allowed})")
    return bad


@pytest.mark.parametrize("n_layers", SC.DEPTHS)
@pytest.mark.parametrize("weights", SC.WEIGHTS)
def test_folds_against_the_restatement(weights, n_layers):
    """every tensor stage_cases.folded names: Watt / batt, Wfc / bfc, the LayerNorm vectors, Wf1 / Wf2, and per layer Wqkv, W1m / b1m,
    W2, Wnext / bnext, then Wfin and Wfin2 / bfin2"""
    want = {k: v.numpy() for k, v in SC.folded(weights, n_layers).items()}
    prep = PC.prepared(weights, n_layers)
    assert len(want) == 14 + 6 * n_layers + 2 * max(n_layers - 1, 0) + (2 if n_layers else 0)
    assert not _failures(prep, want)
    # and nothing else of the signature network is in the table
    assert {n for n in prep.entries if re.match(r"[Wb](qkv|1m|2|next)\d+$", n)} == {k for k in want if re.search(r"\d$", k) and k[1] != "f"}


def _encoder_restatement(sd_t):
    """the eight BatchNorm-folded layers, W g / sqrt(var + 1e-5) and (b - mean) g / sqrt(var + 1e-5) + beta in float64, rounded once"""
    want = {}
    for enc in ("word", "line"):
        for i in range(4):
            c, b = f"{FC.ENC[enc]}.{3 * i}", f"{FC.ENC[enc]}.{3 * i + 1}"
            g = sd_t[b + ".weight"].double() / torch.sqrt(sd_t[b + ".running_var"].double() + 1e-5)
            want[f"W{enc}{i + 1}"] = (sd_t[c + ".weight"][:, :, 0].double() * g[:, None]).float().numpy()
            want[f"b{enc}{i + 1}"] = ((sd_t[c + ".bias"].double() - sd_t[b + ".running_mean"].double()) * g + sd_t[b + ".bias"].double()).float().numpy()
    return want


def _pool_restatement(sd_t):
    """U_h = Wk_h^T q_h, U2_h = W5^T U_h, c_h = q_h . bk_h, c_tok = U_h . b5 + c_h, s_cls = U_h . cls + c_h (float64, rounded once)"""
    k = FC._pool_consts(sd_t, torch.float64)
    U = torch.einsum("hd,hdc->hc", k["q"], k["Wk"].view(4, 64, 256))
    c = torch.einsum("hd,hd->h", k["q"], k["bk"].view(4, 64))
    return {n: v.float().numpy() for n, v in (("U", U), ("U2", U @ k["W5"]), ("c_tok", U @ k["b5"] + c), ("s_cls", U @ k["cls"] + c))}


@pytest.mark.parametrize("weights", SC.WEIGHTS)
def test_pooling_constants_and_encoders_against_float64(weights):
    sd_t = SC.weights_t(weights, 7)[1]
    prep = PC.prepared(weights, 7)
    assert not _failures(prep, {**_pool_restatement(sd_t), **_encoder_restatement(sd_t)})
    # the line encoder's last layer passes through; the word encoder's is consumed by U2 and Watt and has no entry
    assert np.array_equal(prep["Wline5"], sd_t[FC.ENC["line"] + ".12.weight"][:, :, 0].numpy())
    assert np.array_equal(prep["bline5"], sd_t[FC.ENC["line"] + ".12.bias"].numpy())
    assert "Wword5" not in prep.entries


@pytest.mark.parametrize("weights", SC.WEIGHTS)
def test_table_layout(weights):
    """placement as Arena::put made it: ascending, every entry at a multiple of 64 floats right behind the one before it; a GEMM weight
    is followed by its bias; split-tile images for layers 2-4 of the encoders and the q/k/v projections only"""
    prep = PC.prepared(weights, 2)
    t, end = prep.table, 0
    for i, r in enumerate(t[:-2]):
        assert int(r["offset"]) == (end + 63) // 64 * 64, r["name"]
        end = int(r["offset"]) + int(r["rows"]) * int(r["cols"])
        if r["flags"] & PC.GEMM:
            assert t[i + 1]["name"] == b"b" + r["name"][1:] and t[i + 1]["rows"] == r["rows"] and t[i + 1]["cols"] == 1 and not t[i + 1]["flags"]
    assert end == prep.arena_floats()
    assert [(r["name"], int(r["offset"]), int(r["rows"])) for r in t[-2:]] == [(b"c_tok", end, 4), (b"s_cls", end + 4, 4)]
    assert {r["name"].decode() for r in t if r["flags"] & PC.ST} == {f"W{e}{i}" for e in ("word", "line") for i in (2, 3, 4)} | {"Wqkv0", "Wqkv1"}


@pytest.mark.parametrize("weights", SC.WEIGHTS)
def test_every_planted_mistake_is_far_outside_the_bar(weights):
    assert set(MISTAKE_TENSOR) | GRAPH_ONLY == set(SC.MISTAKES) and not set(MISTAKE_TENSOR) & GRAPH_ONLY
    prep = PC.prepared(weights, 2)
    for mistake, name in MISTAKE_TENSOR.items():
        planted, right = SC.folded(weights, 2, mistake), SC.folded(weights, 2)
        worst = PC.ulp_report(prep[name], planted[name].numpy())[0]
        print(f"{mistake:32s} {name:7s} {worst:.3e} ulp")
        assert PC.inside_bar(prep[name], right[name].numpy()), (mistake, name)
        assert worst >= FAR, (mistake, name, worst)
    for mistake in GRAPH_ONLY:                              # they change no prepared tensor at all
        planted, right = SC.folded(weights, 2, mistake), SC.folded(weights, 2)
        assert all(torch.equal(planted[k], right[k]) for k in right), mistake


@pytest.mark.parametrize("weights,n_layers,widths,training", PC.CONFIGS[-2:])
def test_training_mode_configuration(weights, n_layers, widths, training):
    """bn_batch_stats = 1: the convolutions unfolded, gamma / beta in the slots of the packed statistics (word encoder x4, line encoder
    x4, one per signature layer), each pair placed in front of its convolution"""
    assert training and widths in BC.CHAIN_WIDTHS
    sd_t = PC.config_state_dict(weights, n_layers, widths)[1]
    prep = PC.prepared(weights, n_layers, widths, training)
    names = [r["name"].decode() for r in prep.table]
    bits = lambda name, key: np.array_equal(prep[name].view(np.uint32), sd_t[key].reshape(prep[name].shape).numpy().view(np.uint32))
    slot, channels = 0, []
    for enc in ("word", "line"):
        for i in range(4):
            c, b = f"{FC.ENC[enc]}.{3 * i}", f"{FC.ENC[enc]}.{3 * i + 1}"
            assert bits(f"W{enc}{i + 1}", c + ".weight") and bits(f"b{enc}{i + 1}", c + ".bias"), (enc, i)
            assert bits(f"bn_g{slot}", b + ".weight") and bits(f"bn_b{slot}", b + ".bias"), slot
            assert names.index(f"bn_g{slot}") + 2 == names.index(f"bn_b{slot}") + 1 == names.index(f"W{enc}{i + 1}"), slot
            channels.append(widths[i])
            slot += 1
    want = {}
    for l in range(n_layers):
        s = f"selfattn.layers.{l}."
        assert bits(f"bn_g{slot}", s + "mlp.1.weight") and bits(f"bn_b{slot}", s + "mlp.1.bias"), slot
        assert names.index(f"bn_g{slot}") + 2 == names.index(f"bn_b{slot}") + 1 == names.index(f"Wqkv{l}"), slot
        # the MLP's first layer keeps its own bits where nothing is folded in; merge still is: [W1a | W1b Wm], b1 + W1b bm
        W1, b1 = sd_t[s + "mlp.0.weight"][:, :, 0].double(), sd_t[s + "mlp.0.bias"].double()
        Wm2 = SC._head_major(sd_t[s + "attn.merge.weight"][:, :, 0].double().t().contiguous()).t()
        assert np.array_equal(prep[f"W1m{l}"][:, :256].view(np.uint32), W1[:, :256].float().numpy().view(np.uint32)), l
        want[f"W1m{l}"] = torch.cat([W1[:, :256], W1[:, 256:] @ Wm2], dim=1).float().numpy()
        want[f"b1m{l}"] = (b1 + W1[:, 256:] @ sd_t[s + "attn.merge.bias"].double()).float().numpy()
        channels.append(512)
        slot += 1
    assert not _failures(prep, want)
    assert slot == 8 + n_layers and f"bn_g{slot}" not in prep.entries
    assert [int(prep.entries[f"bn_g{s}"]["rows"]) for s in range(slot)] == [int(prep.entries[f"bn_b{s}"]["rows"]) for s in range(slot)] == channels


def _refused(sd, **model_cfg):
    code, nf, ne, msg = PC.call(sd, None, None, **model_cfg)
    assert (nf, ne) == (-1, -1), "a refused call wrote a size"
    return code, msg


def test_refusals_keep_their_codes_and_texts():
    sd = SC.weights_t("calibrated", 2)[0]
    ok = dict(n_sig_layers=2)
    # a training-mode handle wider than the statistics scratch: before any tensor is looked at
    assert _refused(sd, keyline_encoder=[32, 576, 64, 256], bn_batch_stats=True, **ok) == (
        nat.E_ARG, "create: a training-mode handle (bn_batch_stats = 1) takes keyline_encoder widths up to 512 (got 32, 576, 64, 256)")
    missing = "selfattn.layers.1.attn.merge.bias"
    assert _refused({k: v for k, v in sd.items() if k != missing}, **ok) == (PC.E_WEIGHTS, f"state_dict tensor '{missing}' missing")
    short = {**sd, "final_proj.bias": sd["final_proj.bias"][:255]}
    assert _refused(short, **ok) == (PC.E_WEIGHTS, "state_dict tensor 'final_proj.bias' has 255 elements, expected 256")
    assert _refused(sd, n_sig_layers=3) == (PC.E_WEIGHTS, "state_dict tensor 'selfattn.layers.2.mlp.3.bias' missing")   # the group's last fetch
    assert _refused(sd, descriptor_dim=128, **ok) == (nat.E_ARG, "only descriptor_dim=256 / n_heads=4 are supported")
    assert _refused(sd, n_heads=8, **ok) == (nat.E_ARG, "only descriptor_dim=256 / n_heads=4 are supported")
    assert _refused(sd, d_inner=1000, **ok) == (nat.E_ARG, "bad d_inner / layer counts")
    assert _refused(sd, n_sig_layers=-1) == (nat.E_ARG, "bad d_inner / layer counts")
    assert _refused(sd, keyline_encoder=[32, 64, 100, 256], **ok) == (nat.E_ARG, "keyline_encoder must be [32, 64k, 64k, 256] (got 32,64,100,256)")
    assert _refused(sd, keyline_encoder=[16, 64, 128, 256], **ok) == (nat.E_ARG, "keyline_encoder must be [32, 64k, 64k, 256] (got 16,64,128,256)")


def test_sizes_alone_short_buffers_and_repeatability():
    sd = SC.weights_t(3, 1)[0]
    ref = PC.prepared(3, 1)
    code, nf, ne, _ = PC.call(sd, None, None, n_sig_layers=1)
    assert (code, nf, ne) == (0, ref.image.size, len(ref.table))
    marker = np.float32(-777.25)
    for image_floats, entries in ((nf - 1, ne), (nf, ne - 1)):
        image, table = np.full(image_floats, marker, np.float32), np.zeros(entries, nat.PREPARED_ENTRY_DTYPE)
        code, nf2, ne2, msg = PC.call(sd, image, table, n_sig_layers=1)
        assert code == PC.E_CAPACITY and (nf2, ne2) == (nf, ne) and "do not fit" in msg, msg
        assert (image == marker).all() and not table.view(np.uint8).any()
    again = PC.prepare(sd, n_sig_layers=1)
    assert again.image.tobytes() == ref.image.tobytes() and again.table.tobytes() == ref.table.tobytes()
    # one buffer without the other
    image = np.empty(nf, np.float32)
    assert PC.call(sd, image, None, n_sig_layers=1)[0] == 0 and image.tobytes() == ref.image.tobytes()


def test_accessor_is_bound_declared_and_exported():
    name = "linetr_debug_prepare"
    header = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    proto = re.search(r"\bint %s\(([^()]*)\);" % name, header)
    assert proto and name in nat.ABI and hasattr(nat.lib(), name)
    assert proto.group(1).count(",") + 1 == len(nat.ABI[name][1]) == 11
    names = list(nat.ABI)
    assert names.index(name) == names.index("linetr_debug_stage") + 1          # the binding keeps the header's order
    assert header.index("int linetr_debug_stage(") < proto.start() < header.index("#ifdef LINETR_EXPERIMENTS")
    assert "#define LINETR_ABI_VERSION 6" in header and nat.lib().linetr_abi_version() == 6
    assert "} LinetrPreparedEntry; /* 48 bytes */" in header and nat.PREPARED_ENTRY_DTYPE.itemsize == 48
