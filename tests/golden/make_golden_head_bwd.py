#!/usr/bin/env python3
"""Generate tests/golden/head_bwd.npz and tests/golden/head_bwd_dw.npz: the descriptor head of the REAL reference
(models/line_transformer.py:245-246: its own final_proj, then F.normalize(p=2, dim=1)) on seeded pre-head features, and the gradients
torch autograd gives for a seeded upstream.

Run in the build container only (needs /root/reference), on the CPU:

    python tests/golden/make_golden_head_bwd.py

The reference is imported as SURVEY.md Appendix D does (cv2 stub; the reference's packages first on the path).  Only data is written:
    head_bwd.npz      x [2,256,33], weight [256,256,1], bias [256], upstream [2,256,33] (float32: the inputs of both runs),
                      line_desc, dx, db of the float32 run (_f32) and of the float64 run on the same values (_f64)
    head_bwd_dw.npz   dW_f32, dW_f64 [256,256,1] -- a file of their own: the four 256 x 256 arrays (weight, and the weight
                      gradient at 4 + 8 bytes) do not fit one committed file together with the rest"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")   # FIRST on the path: `models` must be the reference's package

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models as _ref_models  # noqa: E402
assert _ref_models.__file__.startswith("/root/reference/"), _ref_models.__file__
from models.line_transformer import LineTransformer  # noqa: E402  (reference)

B, N_SUB, SEED = 2, 33, 5


def run(model, x, upstream, dtype):
    model = model.to(dtype)
    for p in model.final_proj.parameters():
        p.grad = None
    feat = torch.tensor(x, dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        desc = torch.nn.functional.normalize(model.final_proj(feat), p=2, dim=1)      # line_transformer.py:245-246
        desc.backward(torch.tensor(upstream, dtype=dtype))
    return {"line_desc": desc.detach().numpy(), "dx": feat.grad.numpy(), "dW": model.final_proj.weight.grad.numpy().copy(),
            "db": model.final_proj.bias.grad.numpy().copy()}


def main():
    torch.manual_seed(SEED)
    model = LineTransformer({"mode": "train"}).eval()            # 'train': no weight file is read; seeded initialisation
    with torch.no_grad():
        model.final_proj.bias.uniform_(-0.5, 0.5)                # (Conv1d's own bias bound is 1/16: make the bias matter)
    rs = np.random.RandomState(SEED)
    x = rs.standard_normal((B, 256, N_SUB)).astype(np.float32)
    upstream = rs.standard_normal((B, 256, N_SUB)).astype(np.float32)
    weight = model.final_proj.weight.detach().numpy().copy()
    bias = model.final_proj.bias.detach().numpy().copy()
    assert weight.dtype == np.float32 and weight.shape == (256, 256, 1)
    f32 = run(model, x, upstream, torch.float32)
    f64 = run(model, x, upstream, torch.float64)
    assert np.array_equal(model.final_proj.weight.detach().numpy(), weight.astype(np.float64))
    main_path, dw_path = os.path.join(HERE, "head_bwd.npz"), os.path.join(HERE, "head_bwd_dw.npz")
    np.savez_compressed(main_path, x=x, weight=weight, bias=bias, upstream=upstream,
                        **{f"{k}_f32": f32[k] for k in ("line_desc", "dx", "db")}, **{f"{k}_f64": f64[k] for k in ("line_desc", "dx", "db")})
    np.savez_compressed(dw_path, dW_f32=f32["dW"], dW_f64=f64["dW"])
    for k in ("line_desc", "dx", "dW", "db"):
        print(f"{k}: max |.| {np.abs(f64[k]).max():.3e}, float32 error {np.abs(f32[k] - f64[k]).max():.2e}")
    print(f"{os.path.getsize(main_path)} bytes -> {main_path}\n{os.path.getsize(dw_path)} bytes -> {dw_path}")


if __name__ == "__main__":
    main()
