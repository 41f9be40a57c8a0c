"""Restatements behind the fixed-size sample tests (test infrastructure only): conv_fixed_size's 'klines' branch
(dataloaders/utils/util_lines.py:695-766) in NumPy on top of per-image tokeniser outputs, and the pseudo-line generator of
include/linetr_hip.h (linetr_make_pseudo_lines / linetr_find_line_attributes) over a pure-Python Philox4x32-10."""
import math

import numpy as np
import torch

from helpers import BASE_CFG, load
from oracle import linetr_oracle as O
from workloads import synth

KLINE_KEYS = ("klines", "length_klines", "angles")
SUB_KEYS = ("sublines", "pnt_sublines", "mask_sublines", "resp_sublines", "angle_sublines", "desc_sublines", "score_sublines")
ALL_KEYS = KLINE_KEYS + SUB_KEYS + ("mat_klines2sublines",)
EXACT_KEYS = tuple(k for k in ALL_KEYS if k != "desc_sublines")
RESIZE = (640, 480)              # conf['data']['resize'] of the dataset builder: reaches line_tokenizer as (height, width)
TD, T = 8, 21
DESC_TOL = 1e-6                  # desc_sublines against a reference fixture: tests/test_oracle_golden.py, tests/test_gpu_line_process.py
DESC_SUM_TOL = 256 * DESC_TOL    # a sum over the 256 channels of values each within DESC_TOL


def fixture():
    return load("fixed_size")


def cases(g):
    return [str(c) for c in g["cases"]]


def pseudo_of(g, name):
    """the pseudo-line dict of a case as conv_fixed_size handed it to line_tokenizer, or None"""
    if not int(g[f"{name}_n_pseudo"]):
        return None
    return {k: g[f"{name}_pseudo_{k}"].copy() for k in KLINE_KEYS}


def conv_fixed_size_np(real, pseudo, M):
    """real / pseudo: the tokeniser's dict for the image / for its pseudo lines (arrays with a leading axis of 1; pseudo None when no
    padding is needed).  Returns the fixed-size dict, arrays with a leading axis of 1."""
    real = {k: np.asarray(v) for k, v in real.items() if k in ALL_KEYS}
    num_klns, num_slns = real["klines"].shape[1], real["sublines"].shape[1]
    n_add = M - num_slns
    assert num_klns <= M and (pseudo is not None) == (n_add > 0)
    out = {}
    for k in KLINE_KEYS:
        new = np.zeros((1, M) + real[k].shape[2:], dtype=np.float32)
        new[0, :num_klns] = real[k][0]
        if n_add > 0:
            assert np.asarray(pseudo[k]).shape[1] == n_add
            new[0, num_klns:num_klns + n_add] = np.asarray(pseudo[k])[0]
        out[k] = new
    for k in SUB_KEYS:
        out[k] = np.concatenate([real[k], np.asarray(pseudo[k])], axis=1) if n_add > 0 else real[k][:, :M]
        assert out[k].shape[1] == M, k
    mat = np.eye(M, dtype=np.float32)
    cols = min(num_slns, M)
    mat[:num_klns, :cols] = real["mat_klines2sublines"][0, :num_klns, :cols]
    out["mat_klines2sublines"] = mat[None]
    out["num_klns"], out["num_slns"] = np.array([num_klns]), np.array([num_slns])
    return out


def oracle_case(g, name):
    """the case rebuilt from the fixture's inputs with the per-image oracle (preprocess, and tokenize for the pseudo lines)"""
    hw = tuple(int(v) for v in g["hw"])
    seed, M = int(g[f"{name}_seed"]), int(g[f"{name}_M"])
    dd, ds = (torch.from_numpy(a) for a in synth.synth_dense_maps_np(seed, *hw))
    real = O.preprocess(synth.array_to_keylines(g[f"{name}_lines"]), (1, 1, *hw), dd, ds, dict(BASE_CFG))
    pseudo = pseudo_of(g, name)
    tok = O.tokenize(pseudo, TD, T, dd, ds, RESIZE) if pseudo is not None else None
    return conv_fixed_size_np({k: v.numpy() for k, v in real.items() if torch.is_tensor(v)},
                              {k: v.numpy() for k, v in tok.items() if torch.is_tensor(v)} if tok is not None else None, M)


def check_against_fixture(g, name, got, exact=EXACT_KEYS):
    """`got`: {key: array with leading axis 1}.  array_equal for `exact`, DESC_TOL for the stored desc rows, DESC_SUM_TOL for the sums."""
    for k in exact:
        want = g[f"{name}_{k}"]
        assert got[k].shape == want.shape and got[k].dtype == want.dtype, (name, k, got[k].shape, want.shape)
        assert np.array_equal(got[k], want), (name, k)
    for k in ("num_klns", "num_slns"):
        assert np.array_equal(np.asarray(got[k]).reshape(-1), g[f"{name}_{k}"].reshape(-1)), (name, k)
    desc = got["desc_sublines"][0]
    step = int(g[f"{name}_desc_step"])
    err = float(np.abs(desc[::step] - g[f"{name}_desc_rows"]).max())
    err_sum = float(np.abs(desc.astype(np.float64).sum(-1) - g[f"{name}_desc_sum"]).max())
    print(f"{name}: desc_sublines error {err:.3g} (bar {DESC_TOL:g}), channel sums {err_sum:.3g} (bar {DESC_SUM_TOL:g})")
    assert err <= DESC_TOL and err_sum <= DESC_SUM_TOL, (name, err, err_sum)


# ---- the pseudo-line generator ---------------------------------------------------------------------------------------------

M32 = 0xFFFFFFFF


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11): counter c (4 words), key k (2 words) -> 4 words"""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u01(hi, lo):
    return (float(hi >> 5) * 67108864.0 + float(lo >> 6)) / 9007199254740992.0


def make_pseudo_lines(seed, image, n, shape, min_length=16.0, stats=None):
    """linetr_make_pseudo_lines restated: key (seed, image), counter (line, attempt, draw, 0), 64 attempts, then the fixed line"""
    mask, max_rand = 15.0, 160.0
    area = (shape[0] - min_length - mask, shape[1] - min_length - mask)
    lines = np.zeros((n, 2, 2))
    for i in range(n):
        for attempt in range(64):
            a = philox4x32_10((i, attempt, 0, 0), (seed, image))
            b = philox4x32_10((i, attempt, 1, 0), (seed, image))
            sx, sy = area[0] * u01(a[0], a[1]), area[1] * u01(a[2], a[3])
            ang = 2 * math.pi * u01(b[0], b[1])
            ln = (max_rand - min_length) * u01(b[2], b[3]) + min_length
            ex, ey = sx + ln * math.cos(ang), sy + ln * math.sin(ang)
            l = [min(max(v, mask), s - mask) for v, s in ((sx, shape[0]), (sy, shape[1]), (ex, shape[0]), (ey, shape[1]))]
            dx, dy = l[2] - l[0], l[3] - l[1]
            length = math.sqrt(dx * dx + dy * dy)
            if (not length < min_length) if attempt == 0 else length > min_length:
                break
        else:
            l = [mask, mask, mask + 2 * min_length, mask]
            attempt = 64
        if stats is not None:
            stats.append(attempt)
        lines[i] = np.array(l).reshape(2, 2)
    return lines


def find_line_attributes(lines, min_length, max_sublines):
    """linetr_find_line_attributes restated (util_lines.py:634-668; ties by descending original index)"""
    kept = []
    for l in np.asarray(lines, dtype=np.float64).reshape(-1, 2, 2):
        (sx, sy), (ex, ey) = (l[0], l[1]) if l[0, 0] < l[1, 0] else (l[1], l[0])
        dx, dy = float(ex) - float(sx), float(ey) - float(sy)
        length = math.sqrt(dx * dx + dy * dy)
        if length < min_length:
            continue
        kept.append((length, [[float(sx), float(sy)], [float(ex), float(ey)]]))
    order = sorted(range(len(kept)), key=lambda i: kept[i][0])[::-1][:max_sublines]       # sorted() is stable
    kl = np.array([kept[i][1] for i in order], dtype=np.float64).reshape(-1, 2, 2)
    ang = np.zeros((len(order), 2))
    for r, l in enumerate(kl):
        th = math.atan2(l[1, 0] - l[0, 0], l[1, 1] - l[0, 1])
        if th < 0:
            th += math.pi
        ang[r] = (math.cos(2 * th), math.sin(2 * th))
    return {"klines": kl, "length_klines": np.array([kept[i][0] for i in order], dtype=np.float64), "angles": ang}
