"""CPU: what the GPU tests of the native SuperPoint encoder rest on (sp_encoder_cases.py): the float64 restatement of the chain is
pinned to the reference-generated fixture, the exact families are exact, floor pooling is nn.MaxPool2d's, and the packing's index
map is a bijection."""
import os

import numpy as np
import torch

import sp_encoder_cases as S

GOLD = os.path.join(os.path.dirname(__file__), "golden", "superpoint_heads.npz")
TH, TW = 8, 16      # any tile gives valid cases here; the GPU tests ask the library for the kernel's


def test_float64_chain_reproduces_the_reference_fixture():
    """seed-0 weights on the fixture's [2,1,64,96] image: the fixture (the reference's own CPU float32 run) lies within the bar of
    the float64 chain -- in fact within |ref32 - ref64|, 8x inside."""
    from workloads import synth
    g = np.load(GOLD)
    sd = synth.superpoint_state_dict(int(g["weights_seed"]))
    r32, r64 = S.chain_ref(g["image"], sd, torch.float32), S.chain_ref(g["image"], sd, torch.float64)
    for key in ("score_logits", "desc_raw"):
        err = np.abs(g[key].astype(np.float64) - r64[key]).max()
        print(key, "max|ref64|", np.abs(r64[key]).max(), "|ref32-ref64|", np.abs(r32[key] - r64[key]).max(), "fixture error", err,
              "bar", S.bar(r32[key], r64[key]))
        assert g[key].shape == r64[key].shape and err <= S.bar(r32[key], r64[key])
    assert r64["feat"].shape == (2, 8, 12, 128)


def test_exact_families_are_exact_in_float32():
    for cin, cout in S.PAIRS:
        for family in ("integers", "negative"):
            for h, w, b in S.sizes(TH, TW)[::5]:
                _, _, _, r32, r64 = S.layer_case(family, cin, cout, b, h, w)
                assert np.array_equal(r32.astype(np.float64), r64), (family, cin, cout, h, w)
                assert np.abs(r64).max() < 2 ** 24
                if family == "negative":
                    assert not r64.any()
        for tap in range(9):
            for corner in range(4):
                x, w, b = S.one_hot_inputs(cin, cout, TH + 1, TW + 1, tap, corner)
                r32, r64 = S.conv_ref(x, w, b, torch.float32), S.conv_ref(x, w, b, torch.float64)
                assert np.array_equal(r32.astype(np.float64), r64)
                assert np.count_nonzero(x.any(axis=3)) == 1 and np.count_nonzero(w.any(axis=(0, 1))) == 1
    for h, w, b in S.sizes(TH, TW):
        img, wt, bias = S.conv1a_inputs("integers", b, h, w)
        assert np.array_equal(S.conv1a_ref(img, wt, bias, torch.float32).astype(np.float64), S.conv1a_ref(img, wt, bias, torch.float64))


def test_one_hot_response_sits_where_the_tap_puts_it():
    """cross-correlation (no kernel flip): input pixel (y, x) through tap (ky, kx) lands at (y - ky + 1, x - kx + 1)"""
    H, W = TH + 1, TW + 1
    for tap in range(9):
        for corner in range(4):
            x, w, b = S.one_hot_inputs(64, 64, H, W, tap, corner)
            y = S.conv_ref(x, w, np.zeros_like(b), torch.float64, relu=False)[0]
            oy, ox = (H - 1) * (corner >> 1) - tap // 3 + 1, (W - 1) * (corner & 1) - tap % 3 + 1
            hit = np.argwhere(y.any(axis=2))
            if 0 <= oy < H and 0 <= ox < W:
                assert hit.tolist() == [[oy, ox]], (tap, corner)
            else:
                assert hit.size == 0, (tap, corner)


def test_floor_pooling_of_odd_sizes_matches_maxpool2d():
    rs = np.random.RandomState(3)
    for h, w in ((1, 5), (5, 1), (2, 2), (3, 3), (7, 10), (9, 17), (17, 33)):
        y = rs.standard_normal((2, h, w, 4)).astype(np.float32)
        want = torch.nn.MaxPool2d(2, 2)(torch.from_numpy(y).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy() if min(h, w) >= 2 else None
        have = S.pool_ref(y)
        assert have.shape == (2, h // 2, w // 2, 4)
        if want is not None:
            assert np.array_equal(have, want)
            manual = np.maximum(np.maximum(y[:, 0:2 * (h // 2):2, 0:2 * (w // 2):2], y[:, 0:2 * (h // 2):2, 1:2 * (w // 2):2]),
                                np.maximum(y[:, 1:2 * (h // 2):2, 0:2 * (w // 2):2], y[:, 1:2 * (h // 2):2, 1:2 * (w // 2):2]))
            assert np.array_equal(have, manual)


def test_packing_index_map_round_trips():
    rs = np.random.RandomState(0)
    for (cin, cout), k in [(p, 3) for p in S.PAIRS] + [((256, 128), 1), ((256, 256), 1)]:
        w = rs.standard_normal((cout, cin, k, k)).astype(np.float32)
        packed = S.pack_model(w)
        assert not np.isnan(packed).any()                      # every slot written: the map is onto, hence a bijection
        assert np.array_equal(S.unpack_model(packed, cout, cin, k), w)
    # the K order the kernel walks: chunk, then tap, then 8-channel group; 8 consecutive channels of one output channel are adjacent
    assert S.pack_index(0, 0, 0, 9, 64) == 0 and S.pack_index(0, 7, 0, 9, 64) == 7 and S.pack_index(1, 0, 0, 9, 64) == 8
    assert S.pack_index(0, 8, 0, 9, 64) == 64 * 8 and S.pack_index(0, 0, 1, 9, 64) == 4 * 64 * 8 and S.pack_index(0, 32, 0, 9, 64) == 9 * 4 * 64 * 8
