#!/usr/bin/env python3
"""Generate tests/golden/desc_layer_dropout.npz: the REAL reference's LineDescriptiveEncoder (models/line_transformer.py:75-91) in .train()
WITH dropout, on the seeded desc [2, 5, 22, 256] of desc_layer.npz with the same upstream arriving at row 0 of its output, differentiated
by torch autograd in float32 and in float64, for p in {0.1, 0.5}.

The reference's three nn.Dropout instances (attributes of its module objects: slf_attn.attention.dropout, slf_attn.dropout,
pos_ffn.dropout) are replaced by tests/dropout_reference.py's Mask modules, which multiply by a fixed mask: query row 0 of each mask is the
factor table of (seed 2026, call 0, site, p) -- the masks this project's kernels generate --, the other rows a second seeded draw.  Torch's
own dropout stream is not involved.

Run where the reference checkout is at hand ($LINETR_REFERENCE names it), on the CPU:

    LINETR_REFERENCE=<checkout> python tests/golden/make_golden_desc_layer_dropout.py

The weights, inputs and masks are NOT stored: tests/desc_layer_reference.py (module_case(*FIXTURE_SHAPE)) and tests/dropout_reference.py
(masks) draw them again.  Only data is written, the float64 run's unless said otherwise, every key with `@p<p>` behind it:
    out [2, 5, 256] (= enc_output[:, :, 0]); d_desc on every second column, [2, 5, 22, 128]; the gradient of every 1-D parameter; of every
    weight matrix W its gradient on desc_layer.npz's sub-grid W[::7, ::5] (dropout_reference.fixture_grid);
    <tensor>_f32_err: max |float32 run - float64 run| over the WHOLE tensor, the float32 yardstick"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.path.abspath(os.environ["LINETR_REFERENCE"])
sys.path.insert(0, REFERENCE)   # FIRST on the path: `models` must be the reference's package
sys.path.append(os.path.dirname(HERE))          # tests/: the two reference files (they import nothing of this repository's packages)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

import models as _ref_models  # noqa: E402
assert _ref_models.__file__.startswith(REFERENCE.rstrip("/") + "/"), _ref_models.__file__
from models.line_transformer import LineDescriptiveEncoder  # noqa: E402  (reference)

import desc_layer_reference as DL  # noqa: E402
import dropout_reference as DR  # noqa: E402


def run(dtype, p):
    sd, desc, g = DL.module_case(*DL.FIXTURE_SHAPE)
    mod = LineDescriptiveEncoder(256, 4, 1, 1024).to(dtype)
    mod.load_state_dict(DL.tensors(sd, dtype), strict=True)
    mod.train()
    assert sum(isinstance(m, nn.Dropout) for m in mod.modules()) == 3
    attn, m1, m2 = (torch.tensor(m, dtype=dtype) for m in DR.masks(*DL.FIXTURE_SHAPE, DR.SEED, 0, p))
    for holder, mask in ((mod.slf_attn.attention, attn), (mod.slf_attn, m1), (mod.pos_ffn, m2)):
        assert isinstance(holder.dropout, nn.Dropout)
        holder.dropout = DR.Mask(mask)
    assert not any(isinstance(m, nn.Dropout) for m in mod.modules())
    xt = torch.tensor(desc, dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        enc, _ = mod(xt, slf_attn_mask=None)
        out = enc[:, :, 0]
        out.backward(torch.tensor(g, dtype=dtype))
    res = {"out": out.detach().double().numpy(), "d_desc": xt.grad.double().numpy()}
    for key, prm in mod.named_parameters():
        res[key] = prm.grad.detach().double().numpy()
    return res


def main():
    out = {"seed": np.int64(DR.SEED), "call": np.int64(0), "p_values": np.array(DR.P_VALUES)}
    for p in DR.P_VALUES:
        f64, f32 = run(torch.float64, p), run(torch.float32, p)
        for key, val in f64.items():
            out[DR.fixture_key(key, p)] = DR.fixture_grid(key, val)
            out[DR.fixture_key(key, p) + "_f32_err"] = np.float64(np.abs(f32[key] - val).max())
            print(f"desc_layer dropout p={p} {key}: max |.| {np.abs(val).max():.3e}, float32 error {np.abs(f32[key] - val).max():.2e}")
    path = os.path.join(HERE, "desc_layer_dropout.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
