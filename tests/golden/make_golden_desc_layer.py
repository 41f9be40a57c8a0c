#!/usr/bin/env python3
"""Generate tests/golden/desc_layer.npz: the REAL reference's LineDescriptiveEncoder (models/line_transformer.py:75-91) in .train() with
p = 0 on each of its nn.Dropout instances, on seeded desc [2, 5, 22, 256] with a seeded upstream arriving at row 0 of its output (the
only row KeylineEncoder reads, :128), differentiated by torch autograd in float32 and in float64.

Run where the reference checkout is at hand ($LINETR_REFERENCE names it), on the CPU:

    LINETR_REFERENCE=<checkout> python tests/golden/make_golden_desc_layer.py

The reference is imported as SURVEY.md Appendix D does (cv2 stub; the reference's packages first on the path).  The weights and inputs are
NOT stored: they are drawn from np.random.RandomState(seed) by tests/desc_layer_reference.py (module_case(*FIXTURE_SHAPE)) and go into the
reference's module through load_state_dict(strict=True); a test draws them again.  Only data is written, the float64 run's unless said
otherwise:
    out [2, 5, 256] (= enc_output[:, :, 0]), d_desc [2, 5, 22, 256] (slot 0 included); the gradient of every 1-D parameter; of every weight
    matrix W its gradient on the sub-grid W[::7, ::5] (the whole matrices would take the file past the size a committed file may have);
    <tensor>_f32_err: max |float32 run - float64 run| over the WHOLE tensor, the float32 yardstick;
    state_dict_keys: the reference module's key set"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.path.abspath(os.environ["LINETR_REFERENCE"])
sys.path.insert(0, REFERENCE)   # FIRST on the path: `models` must be the reference's package
sys.path.append(os.path.dirname(HERE))          # tests/: desc_layer_reference.py (imports nothing of this repository's packages)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

import models as _ref_models  # noqa: E402
assert _ref_models.__file__.startswith(REFERENCE.rstrip("/") + "/"), _ref_models.__file__
from models.line_transformer import LineDescriptiveEncoder  # noqa: E402  (reference)

import desc_layer_reference as DL  # noqa: E402


def run(dtype):
    sd, desc, g = DL.module_case(*DL.FIXTURE_SHAPE)
    mod = LineDescriptiveEncoder(256, 4, 1, 1024).to(dtype)
    mod.load_state_dict(DL.tensors(sd, dtype), strict=True)
    mod.train()
    drops = [m for m in mod.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) == 3
    for m in drops:
        m.p = 0.0
    xt = torch.tensor(desc, dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        enc, attn = mod(xt, slf_attn_mask=None)
        out = enc[:, :, 0]
        out.backward(torch.tensor(g, dtype=dtype))
    assert attn.shape == (desc.shape[0], desc.shape[1], 4, desc.shape[2], desc.shape[2])
    res = {"out": out.detach().double().numpy(), "d_desc": xt.grad.double().numpy()}
    for key, p in mod.named_parameters():
        res[key] = p.grad.detach().double().numpy()
    return res, sorted(mod.state_dict())


def main():
    (f64, keys), (f32, _) = run(torch.float64), run(torch.float32)
    out = {"state_dict_keys": np.array(keys)}
    for key, val in f64.items():
        out[key] = val[::7, ::5] if key in DL.MATRICES else val
        out[key + "_f32_err"] = np.float64(np.abs(f32[key] - val).max())
        print(f"desc_layer {key}: max |.| {np.abs(val).max():.3e}, float32 error {np.abs(f32[key] - val).max():.2e}")
    path = os.path.join(HERE, "desc_layer.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
