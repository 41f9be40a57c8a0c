#!/usr/bin/env python3
"""Golden fixture of the fixed-size training samples: the reference's own conv_fixed_size (dataloaders/utils/util_lines.py:670-766,
'klines' branch) on what its preprocess returns, for every branch the native batch call (linetr_fixed_size) has to reproduce.

    python tests/golden/make_golden_fixed_size.py      ->  tests/golden/fixed_size.npz

Runs the REAL reference (same harness as make_golden.py / make_golden_train_mode.py), with np.random.seed set before each call
(make_pseudo_lines draws from the global NumPy generator).  Stored per case: the detector rows and the map seed, the pseudo-line dict
exactly as conv_fixed_size hands it to line_tokenizer (float64, before its in-place clip), and every output key.  desc_sublines is
stored as a float64 sum over the channels for every token (`desc_sum` [M, T]) and in full for every `desc_step`-th row: the
fixture has to stay under the size limit of a committed file.  A case's detector rows are synth.synth_lines(seed, ...) for the first
seed at or behind its base seed whose counts hit the intended branch; the script asserts the branch."""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up the cv2 stub and puts /root/reference first on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, "/root/reference/dataloaders")
from utils import util_lines  # noqa: E402  (reference; numpy / torch / math only)
assert util_lines.__file__.startswith("/root/reference/"), util_lines.__file__
from models.line_process import line_tokenizer  # noqa: E402  (reference)

from workloads import synth  # noqa: E402

HW = (480, 640)
KEYS = G.TENSOR_KEYS + ["desc_sublines"]


def key_line_of(mat, j):
    """key-line that owns sub-line j in an image's mat_klines2sublines [K, N]"""
    return int(np.flatnonzero(mat[:, j])[0])


# name, max_sublines, detector rows, shortest / longest line, base seed, desc_step, branch(num_klns, num_slns, mat, M)
CASES = [
    ("pad_stray", 8, 6, 17.0, 330.0, 500, 1, lambda k, n, mat, M: n < M and k < n),                       # one or more pseudo lines, stray diagonal
    ("exact", 16, 17, 17.0, 167.0, 520, 8, lambda k, n, mat, M: k == M and n == M),                       # n_add == 0: the truncation branch
    ("cut_unsplit", 16, 12, 17.0, 330.0, 540, 4, lambda k, n, mat, M: n > M and k < M and key_line_of(mat, M - 1) != key_line_of(mat, M)),
    ("cut_straddle", 7, 6, 200.0, 330.0, 560, 2, lambda k, n, mat, M: n > M and k < M and key_line_of(mat, M - 1) == key_line_of(mat, M)),
    ("klns_eq_max", 7, 8, 200.0, 330.0, 580, 2, lambda k, n, mat, M: k == M and n > M),
    ("mostly_pseudo", 16, 2, 17.0, 167.0, 600, 8, lambda k, n, mat, M: k == 1 and n == 1),
    ("big_pad", 250, 140, 17.0, 167.0, 401, 62, lambda k, n, mat, M: n < M),                              # the builder's configuration
    ("big_cut", 250, 240, 17.0, 330.0, 403, 62, lambda k, n, mat, M: n > M and k <= M),
]


def conf_for(M):
    return {"data": {"resize": (640, 480)},
            "feature": {"linetr": {"token_distance": 8, "max_tokens": 21, "max_sublines": M, "min_length": 16}}}


def main():
    m = G.ref_model(0)
    arrs = {"hw": np.array(HW), "cases": np.array([c[0] for c in CASES])}
    for name, M, n_rows, lo, hi, base, step, branch in CASES:
        for seed in range(base, base + 20):
            rows = synth.synth_lines(seed, n_rows, *HW, lo, hi)
            dd, ds = synth.synth_dense_maps_np(seed, *HW)
            pred = {"dense_descriptor": torch.from_numpy(dd), "dense_score": torch.from_numpy(ds)}
            kl = m.preprocess(synth.array_to_keylines(rows), (1, 1, *HW), pred, None)
            k, n = int(kl["klines"].shape[1]), int(kl["sublines"].shape[1])
            if branch(k, n, kl["mat_klines2sublines"][0].numpy(), M):
                break
        else:
            raise AssertionError(f"{name}: no seed in {base}..{base + 19} hits the branch")
        captured = []

        def tokenizer(lines, td, T, pred_sp, image_shape):
            captured.append({key: np.array(v, dtype=np.float64, copy=True) for key, v in lines.items()})
            assert tuple(image_shape) == (640, 480)          # conv_fixed_size passes conf['data']['resize'] (width, height)
            return line_tokenizer(lines, td, T, pred_sp, image_shape)
        np.random.seed(2000 + seed)
        fixed = util_lines.conv_fixed_size(kl, copy.deepcopy(conf_for(M)), func_token=tokenizer, pred_sp=pred)
        assert int(fixed["num_klns"]) == k and int(fixed["num_slns"]) == n and fixed["sublines"].shape[1] == M
        assert len(captured) == (1 if n < M else 0)
        n_pseudo = len(captured[0]["klines"]) if captured else 0
        assert n_pseudo == max(M - n, 0)
        print(f"{name}: seed {seed}, M = {M}: {k} key-lines, {n} sub-lines, {n_pseudo} pseudo lines")
        p = f"{name}_"
        arrs.update({p + "seed": seed, p + "M": M, p + "lines": rows, p + "n_pseudo": n_pseudo, p + "desc_step": step,
                     p + "num_klns": fixed["num_klns"].numpy(), p + "num_slns": fixed["num_slns"].numpy()})
        if captured:
            for key, v in captured[0].items():
                arrs[p + "pseudo_" + key] = v
        for key in KEYS:
            v = fixed[key].numpy()
            assert v.shape[0] == 1 and v.shape[1] == M, (key, v.shape)
            if key == "desc_sublines":
                arrs[p + "desc_sum"] = v[0].astype(np.float64).sum(-1)
                arrs[p + "desc_rows"] = v[0, ::step].copy()
            else:
                arrs[p + key] = v.copy()
    G.save("fixed_size", **arrs)
    assert os.path.getsize(os.path.join(HERE, "fixed_size.npz")) < (1 << 20)


if __name__ == "__main__":
    main()
