#!/usr/bin/env python3
"""Generate tests/golden/sig_layer.npz and tests/golden/sig_layer_stack.npz: the REAL reference's AttentionalPropagation and a two-layer
SelfAttentionalLayer (models/line_transformer.py:157-183) in .train(), on seeded input [2, 256, 33] with a seeded upstream, differentiated
by torch autograd in float32 and in float64.

Run where the reference checkout is at hand ($LINETR_REFERENCE names it), on the CPU:

    LINETR_REFERENCE=<checkout> python tests/golden/make_golden_sig_layer.py

The reference is imported as SURVEY.md Appendix D does (cv2 stub; the reference's packages first on the path).  The weights and inputs
are NOT stored: they are drawn from np.random.RandomState(seed) by tests/sig_layer_reference.py (layer_case(2, 33), stack_case()) --
the BatchNorm weight and bias away from 1 and 0 -- and go into the reference's modules through load_state_dict(strict=True); a test draws
them again.  Only data is written, the float64 run's unless said otherwise:
    sig_layer.npz        delta, dx, d_source [2, 256, 33]; the gradient of every 1-D parameter; of every weight matrix W its gradient on the
                         sub-grid W[::7, ::5] (the whole matrices would take the file past the size a committed file may have);
                         after.mlp.1.running_mean / running_var / num_batches_tracked: the buffers after the call;
                         <tensor>_f32_err: max |float32 run - float64 run| over the WHOLE tensor, the float32 yardstick;
                         state_dict_keys: the reference module's key set
    sig_layer_stack.npz  the same for the stack: out, dx, and the gradients / buffers under layers.<i>.<name> -- a file of its own, again for
                         the size"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.path.abspath(os.environ["LINETR_REFERENCE"])
sys.path.insert(0, REFERENCE)   # FIRST on the path: `models` must be the reference's package
sys.path.append(os.path.dirname(HERE))          # tests/: sig_layer_reference.py (imports nothing of this repository's packages)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models as _ref_models  # noqa: E402
assert _ref_models.__file__.startswith(REFERENCE.rstrip("/") + "/"), _ref_models.__file__
from models.line_transformer import AttentionalPropagation, SelfAttentionalLayer  # noqa: E402  (reference)

import sig_layer_reference as SL  # noqa: E402


def collect(mod, out):
    for key, p in mod.named_parameters():
        out[key] = p.grad.detach().double().numpy()
    for key, b in mod.named_buffers():
        out["after." + key] = b.detach().numpy().astype(np.float64 if b.is_floating_point() else np.int64)
    return out


def run_layer(dtype):
    sd, x, source, g = SL.layer_case(*SL.FIXTURE_SHAPE)
    mod = AttentionalPropagation(256, 4).to(dtype)
    mod.load_state_dict(SL.tensors(sd, dtype), strict=True)
    mod.train()
    xt, st = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (x, source))
    with torch.enable_grad():
        delta, prob = mod(xt, st)
        delta.backward(torch.tensor(g, dtype=dtype))
    assert prob.shape == (x.shape[0], 4, x.shape[2], x.shape[2])
    return collect(mod, {"delta": delta.detach().double().numpy(), "dx": xt.grad.double().numpy(), "d_source": st.grad.double().numpy()}), sorted(mod.state_dict())


def run_stack(dtype):
    sd, x, g = SL.stack_case()
    mod = SelfAttentionalLayer(256, ["self", "self"]).to(dtype)
    mod.load_state_dict(SL.tensors(sd, dtype), strict=True)
    mod.train()
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        y = mod(xt)
        y.backward(torch.tensor(g, dtype=dtype))
    return collect(mod, {"out": y.detach().double().numpy(), "dx": xt.grad.double().numpy()}), sorted(mod.state_dict())


def pack(f64, f32, keys):
    out = {"state_dict_keys": np.array(keys)}
    for key, val in f64.items():
        out[key] = val[::7, ::5, 0] if val.ndim == 3 and val.shape[2] == 1 else val
        if val.dtype == np.float64:
            out[key + "_f32_err"] = np.float64(np.abs(f32[key] - val).max())
    return out


def main():
    for name, run in (("sig_layer", run_layer), ("sig_layer_stack", run_stack)):
        (f64, keys), (f32, _) = run(torch.float64), run(torch.float32)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **pack(f64, f32, keys))
        for key, val in f64.items():
            if val.dtype == np.float64:
                print(f"{name} {key}: max |.| {np.abs(val).max():.3e}, float32 error {np.abs(f32[key] - val).max():.2e}")
        print(f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
