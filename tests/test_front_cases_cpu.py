"""CPU: the references and the case generator of the front-end unit tests (front_cases.py) are themselves pinned -- to the oracle
that tests/test_oracle_golden.py pins to the reference -- and the generator is shown to produce what tests/test_gpu_front.py
relies on."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

import front_cases as FC
from attn_cases import state_dict_t
from oracle import linetr_oracle as O
from workloads import synth

torch.set_grad_enabled(False)


def test_pooling_reference_is_the_oracles_cls_row(monkeypatch):
    """pool_reference in float64, extended by the value path Wv_h (dbar + W5 abar + (1 - p_0) b5 + p_0 cls) + bv_h, equals row 0 of
    torch.matmul(att, v) inside oracle.forward run in float64, on a tokenised image whose sub-lines carry padding."""
    hw = (480, 640)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state_dict_t(3)[1].items()}
    dd, ds = synth.synth_dense_maps(11, *hw)
    cfg = dict(min_length=16, token_distance=8, max_tokens=5, remove_borders=8, max_keylines=-1)
    data = O.preprocess(synth.array_to_keylines(synth.synth_lines(5, 14, *hw)), (1, 1, *hw), dd, ds, cfg)
    N, T = data["pnt_sublines"].shape[1:3]
    assert float(data["mask_sublines"].min()) == 0.0 and N > data["klines"].shape[1]   # padding slots, key-lines of several sub-lines
    data64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.items()}
    seen = []
    real = torch.matmul
    monkeypatch.setattr(torch, "matmul", lambda a, b: seen.append(real(a, b)) or seen[-1])
    O.forward(sd64, data64, hw)
    monkeypatch.undo()
    want = seen[1][:, :, 0, :]                                             # [N, 4, 64]: CLS row of att @ v
    pnt, score = data["pnt_sublines"][0].reshape(N * T, 2), data["score_sublines"][0].reshape(N * T)
    desc = data["desc_sublines"][0].reshape(N * T, 256)
    a4 = FC.mlp4(sd64, "word", FC.enc_features("word", (pnt, score), torch.float64), torch.float64)
    pooled = FC.pool_reference(sd64, desc, a4, torch.arange(N * T).view(N, T), torch.float64)
    k = FC._pool_consts(sd64, torch.float64)
    p0 = pooled[:, :, 512:513]
    x = pooled[:, :, :256] + F.linear(pooled[:, :, 256:512], k["W5"]) + (1 - p0) * k["b5"] + p0 * k["cls"]
    got = torch.einsum("nhc,hdc->nhd", x, k["Wv"].view(4, 64, 256)) + k["bv"].view(4, 64)
    assert float((got - want).abs().max()) < 1e-12
    assert float(pooled[:, :, 513:].abs().max()) == 0.0


def test_mlp_reference_is_the_oracles_mlp_without_its_last_layer():
    for enc in ("word", "line"):
        for weights in FC.WEIGHTS:
            sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state_dict_t(weights)[1].items()}
            cut = {k: v for k, v in sd64.items() if not k.startswith(FC.ENC[enc] + ".12.")}
            case = FC.mlp_case(enc, weights, "workload", 65)
            feats = FC.enc_features(enc, case["inputs"], torch.float64)
            assert float((O._mlp(cut, FC.ENC[enc], feats) - case["ref64"]).abs().max()) < 1e-12
            assert O._mlp(cut, FC.ENC[enc], feats).shape == (65, 256)


def _digest():
    h = hashlib.sha256()
    for c in (FC.mlp_case("line", 3, "edge", 33), FC.pool_case("planted", 66, 7, 3, "first"), FC.pool_case("sentinel", 5, 33, 4, "mid", parity=1)):
        for k in ("inputs", "cpnt", "a4", "ref64", "ref32"):
            for t in (c.get(k) if isinstance(c.get(k), tuple) else (c.get(k),)):
                if t is not None:
                    h.update(t.numpy().tobytes())
        if "recs" in c:
            h.update(c["recs"].tobytes() + c["sub2line"].tobytes() + FC.dense_of(c).numpy().tobytes())
    return h.hexdigest()


def test_generator_is_reproducible_across_processes():
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_front_cases_cpu as t; print(t._digest())"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                         env={**os.environ, "PYTHONHASHSEED": "123"}).stdout.strip()
    assert out == _digest()


def test_every_listed_size_appears():
    shapes = FC.pool_shapes()
    assert {s[0] for s in shapes} >= set(FC.POOL_T) and {s[1] for s in shapes} == set(FC.POOL_N)
    assert {s[2] for s in shapes} == {1, 2, 3, 4} and {s[3] for s in shapes} == {None, "first", "mid", "last"}
    for T in FC.POOL_T:
        lines = [ln for s in shapes if s[0] == T for ln in FC.layout(*s)]
        last = {n - (-(-n // T) - 1) * T for _, n in lines}
        assert last >= set(FC.n_valid_list(T)), (T, last)
        assert {-(-n // T) for _, n in lines} >= {1, 2, 5}, T
    for s in shapes:                                        # an image named empty has no line, and the records are consistent
        c = FC.pool_case("equal", *s)
        imgs = set(c["recs"]["image"].tolist())
        if s[3]:
            assert {"first": 0, "mid": s[2] // 2, "last": s[2] - 1}[s[3]] not in imgs
        assert int(c["recs"]["n_sub"].sum()) == s[1] and int(c["recs"]["n_tok"].sum()) == c["first_pad"]
    assert set(FC.MLP_ROWS) >= {1, 63, 64, 65, 257} and {r % 64 for _, r in FC.MLP_WALK} == {0, 1, 63}


def test_planted_key_leads_and_equal_family_has_its_closed_form():
    sd_t = state_dict_t("calibrated")[1]
    modes = set()
    for s in ((66, 9, 2, None), (129, 9, 1, None), (21, 33, 4, "first"), (5, 33, 4, "mid")):
        c = FC.pool_case("planted", *s)
        sc, s0 = FC.pool_scores(sd_t, c["desc"], c["a4"], torch.float64)
        for (n, h), r in c["plan"].items():
            mine = c["keys"][n].unique()
            if r is None:                                   # nobody: every key far below CLS
                if (c["keys"][n] < c["first_pad"]).all() and sc[mine, h].max() > s0[h] - 8:
                    continue                                # (a sub-line without padding in a pad-planted image: nothing planted)
                assert sc[mine, h].max() < s0[h] - 8
                modes.add("nobody")
            else:
                rest = torch.cat([sc[mine[mine != r], h], s0[h:h + 1]])
                assert sc[r, h] > rest.max() + 8, (s, n, h)
                pos = (c["keys"][n] == r).nonzero()[0, 0].item()
                modes.add("pad" if r >= c["first_pad"] else pos if pos in (0, 63, 64, 65) else "last")
    assert modes >= {0, 63, 64, 65, "last", "pad", "nobody"}, modes
    c = FC.pool_case("equal", 65, 9, 2)
    sc, s0 = FC.pool_scores(sd_t, c["desc"], c["a4"], torch.float64)
    p0 = 1.0 / (1.0 + c["T"] * torch.exp(sc[0] - s0))
    u = c["desc"][0].double()
    # (the sampled rows are the map's unit vector up to the float32 rounding of the bilinear sum and its normalisation)
    assert float((c["ref64"][:, :, 512] - p0).abs().max()) < 1e-6 and float(c["ref64"][:, :, 256:512].abs().max()) == 0.0
    assert float((c["ref64"][:, :, :256] - (1 - p0)[None, :, None] * u).abs().max()) < 1e-6


def test_ref32_sits_a_factor_inside_the_bar():
    for fam in FC.MLP_FAMILIES:
        for enc in ("word", "line"):
            c = FC.mlp_case(enc, "calibrated", fam, 193)
            assert all(e <= b / FC.FACTOR for _, _, e, b in FC.tile_errors(c["ref32"], c))
    for fam in FC.POOL_FAMILIES:
        c = FC.pool_case(fam, 66, 9, 2)
        rows = FC.subline_errors(c["ref32"], c)
        assert rows and all(e <= b / FC.FACTOR for _, _, e, b in rows), fam
