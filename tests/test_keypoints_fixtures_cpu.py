"""No GPU: pins the reference the key-point tests compare against.  The torch restatement of SuperPoint's key-point branch
(test_gpu_producer._Helpers: iterated max-pool NMS, border filter, top-k, bilinear lookup), fed the `dense_score` of the two
fixtures frozen from the real reference, reproduces their key points and scores exactly, and their descriptors with
grid_sample's align_corners=False (the fixtures were made under a torch whose version switch selects False)."""
import os

import numpy as np
import torch

from test_gpu_producer import _Helpers

torch.set_grad_enabled(False)
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def sample(xy, dense, align):
    """_Helpers.sample_descriptors with the grid_sample flag as an argument"""
    bsz, ch, hc, wc = dense.shape
    span = torch.tensor([wc * 8 - 4 - 0.5, hc * 8 - 4 - 0.5], dtype=xy.dtype)
    grid = ((xy - 4 + 0.5) / span) * 2 - 1
    got = torch.nn.functional.grid_sample(dense, grid.view(bsz, 1, -1, 2), mode="bilinear", align_corners=align)
    return torch.nn.functional.normalize(got.reshape(bsz, ch, -1), p=2, dim=1)


def branch(score, dense, r, thr, border, k, align):
    """one image: score [H,W], dense [256,Hc,Wc] -> key points (x, y), scores, descriptors [256,n]"""
    h, w = score.shape
    nms = _Helpers.simple_nms(score[None], r)[0]
    rc = torch.nonzero(nms > thr)
    val = nms[rc[:, 0], rc[:, 1]]
    rc, val = _Helpers.remove_borders(rc, val, border, h, w)
    n_cand = rc.shape[0]
    if k >= 0:
        rc, val = _Helpers.top_k_keypoints(rc, val, k)
    xy = rc.flip(1).float()
    return xy, val, sample(xy[None], dense[None], align)[0], n_cand


def test_heads_fixture_reproduced_by_the_restatement():
    g = np.load(os.path.join(GOLD, "superpoint_heads.npz"))
    for b in range(2):
        xy, val, desc, _ = branch(torch.from_numpy(g["dense_score"][b]), torch.from_numpy(g["dense_descriptor"][b]), 4, 0.005, 4, -1, False)
        assert np.array_equal(xy.numpy(), g[f"keypoints{b}"])
        assert np.array_equal(val.numpy(), g[f"scores{b}"])
        assert np.abs(desc.numpy() - g[f"descriptors{b}"]).max() <= 1e-6
        other = sample(xy[None], torch.from_numpy(g["dense_descriptor"][b])[None], True)[0]
        assert np.abs(other.numpy() - g[f"descriptors{b}"]).max() > 1e-3      # the other flag is clearly not the fixture's


def test_asset_fixture_topk_is_a_stable_descending_sort():
    g = np.load(os.path.join(GOLD, "asset_pair.npz"))
    for b in range(2):
        score = torch.from_numpy(g[f"dense_score{b}"][0])
        xy, val, desc, n_cand = branch(score, torch.from_numpy(g[f"dense_descriptor{b}"][0]), 4, 0.005, 4, 1024, False)
        assert n_cand > 1024
        assert np.array_equal(xy.numpy(), g[f"keypoints{b}"])
        assert np.abs(desc.numpy() - g[f"descriptors{b}"]).max() <= 1e-6
        # the same order from a stable descending sort of the row-major candidates: the native top-k's contract
        xa, va, _, _ = branch(score, torch.from_numpy(g[f"dense_descriptor{b}"][0]), 4, 0.005, 4, -1, False)
        order = np.lexsort((np.arange(len(va)), -va.numpy().astype(np.float64)))[:1024]
        assert np.array_equal(xa.numpy()[order], g[f"keypoints{b}"])
        top = np.sort(va.numpy())[::-1][:1025]
        assert len(np.unique(top)) == 1025                                     # no equal scores at or above the cut
