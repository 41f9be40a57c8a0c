"""The fixed-size training samples of the reference's dataset builder (dataloaders/utils/util_lines.py:559-766) under the reference's
function names.  The batch form, one native call for B images straight from line records, is Engine.fixed_size_batch; this module
holds the two host functions behind its pseudo lines (native, float64: linetr_make_pseudo_lines / linetr_find_line_attributes) and
conv_fixed_size for one already tokenised image."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as nat

PSEUDO_MIN_LENGTH = 16          # make_pseudo_lines' own constant (util_lines.py:561), whatever the configuration says
KEYS_PER_SUBLINE = ("sublines", "pnt_sublines", "mask_sublines", "resp_sublines", "angle_sublines", "desc_sublines", "score_sublines")


def make_pseudo_lines(n_left, image_shape, seed=0, image=0):
    """util_lines.py:559-617: n_left random lines [n_left, 2, 2] float64 inside `image_shape` = (extent of x, extent of y), 16 to 160
    px long, end points clipped to [15, extent - 15].  The reference draws from NumPy's reseeded global generator; here the stream
    is Philox4x32-10 with key (seed, image) and counter (line, attempt, draw) (include/linetr_hip.h), so the same (seed, image,
    line) gives the same bits on every call.  A line that ends shorter than 16 px is redrawn, 64 times at the most."""
    lines = np.zeros((int(n_left), 2, 2), dtype=np.float64)
    nat.check(nat.lib().linetr_make_pseudo_lines(int(seed), int(image), int(n_left), float(image_shape[0]), float(image_shape[1]),
                                                 float(PSEUDO_MIN_LENGTH), nat.np_ptr(lines)))
    return lines


def find_line_attributes(klines, min_length, max_sublines):
    """util_lines.py:634-668: end points swapped unless sp_x < ep_x, geometric length, lines shorter than min_length dropped, sorted
    by descending length (equal lengths by descending original index: the native pre-filter's tie rule), cut to max_sublines, angles
    as get_angles.  Returns {'klines' [K,2,2], 'length_klines' [K], 'angles' [K,2]} float64."""
    lines = np.ascontiguousarray(klines, dtype=np.float64).reshape(-1, 2, 2)
    n = len(lines)
    kl, ln, an = np.zeros((n, 2, 2)), np.zeros((n,)), np.zeros((n, 2))
    n_out = C.c_int32()
    nat.check(nat.lib().linetr_find_line_attributes(nat.np_ptr(lines), n, float(min_length), int(max_sublines), nat.np_ptr(kl), nat.np_ptr(ln),
                                                    nat.np_ptr(an), C.byref(n_out)))
    k = n_out.value
    return {"klines": kl[:k].copy(), "length_klines": ln[:k].copy(), "angles": an[:k].copy()}


def conv_fixed_size(object, conf, func_token=None, pred_sp=None, seed=0, pseudo_lines=None):
    """util_lines.py:670-766 for one image: `object` is what LineTransformer.preprocess returned (tensors with a leading axis of 1),
    `conf` the builder's (conf['data']['resize'], conf['feature']['linetr']), `pred_sp` the dense maps.  Pads the sample to
    max_sublines with tokenised pseudo lines or cuts it, rebuilds klines / length_klines / angles / mat_klines2sublines at the fixed
    size and records num_klns / num_slns.  `func_token` is accepted and ignored: the pseudo lines go through the native tokeniser.
    `pseudo_lines`: the float64 dict to pad with instead of the generator's (seed, image 0).  The returned dict also carries
    'pseudo_lines', the dict used (None without padding).  One image's worth of Engine.fixed_size_batch, bit for bit."""
    if "keypoints" in object:
        raise NotImplementedError("conv_fixed_size: the 'keypoints' branch is not part of this package (training never reads it)")
    from . import line_process as lp
    lt = conf["feature"]["linetr"]
    td, T, M, min_length = lt["token_distance"], int(lt["max_tokens"]), int(lt["max_sublines"]), lt["min_length"]
    resize = conf["data"]["resize"]
    kl = dict(object)
    num_klns, num_slns = int(kl["klines"].shape[1]), int(kl["sublines"].shape[1])
    if num_klns > M:
        raise ValueError(f"conv_fixed_size: {num_klns} key-lines, more than max_sublines = {M}")
    dev = kl["sublines"].device
    n_add = M - num_slns
    pseudo = None
    if n_add > 0:
        if pseudo_lines is None:
            pseudo_lines = find_line_attributes(make_pseudo_lines(n_add, resize, seed=seed, image=0), min_length, M)
        used = {k: np.array(pseudo_lines[k], dtype=np.float64, copy=True) for k in ("klines", "length_klines", "angles")}
        pseudo = lp.line_tokenizer(dict(used), td, T, pred_sp, resize)
        if len(used["klines"]) != n_add or int(pseudo["sublines"].shape[1]) != n_add:
            raise ValueError(f"conv_fixed_size: {n_add} pseudo lines of one sub-line each are needed, got {len(used['klines'])} lines "
                             f"making {int(pseudo['sublines'].shape[1])} sub-lines")
        pseudo_lines = used
    else:
        pseudo_lines = None
    out = {}
    for key, tail in (("klines", (2, 2)), ("length_klines", ()), ("angles", (2,))):
        new = torch.zeros((1, M, *tail), dtype=torch.float32, device=dev)
        new[0, :num_klns] = kl[key][0]
        if pseudo is not None:
            new[0, num_klns:num_klns + n_add] = pseudo[key][0]
        out[key] = new
    for key in KEYS_PER_SUBLINE:
        out[key] = torch.cat((kl[key], pseudo[key]), dim=1) if pseudo is not None else kl[key][:, :M]
    k2s = torch.eye(M, dtype=torch.float32, device=dev)
    cols = min(num_slns, M)
    k2s[:num_klns, :cols] = torch.as_tensor(kl["mat_klines2sublines"])[0, :num_klns, :cols]
    out["mat_klines2sublines"] = k2s[None]
    out["num_klns"] = torch.tensor([num_klns])
    out["num_slns"] = torch.tensor([num_slns])
    out["pseudo_lines"] = pseudo_lines
    return out
