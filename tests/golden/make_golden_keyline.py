#!/usr/bin/env python3
"""Generate tests/golden/keyline.npz and keyline_matrices.npz: the REAL reference's LineTransformer({'mode': 'train'}) (models/line_transformer.py:185-249) in .train()
with p = 0 on each of its nn.Dropout instances, on the seeded input dict of B = 2 items of n = 5 sub-lines of S = 21 tokens with a seeded
upstream arriving at line_desc, differentiated by torch autograd in float32 and in float64; forward + backward is run twice per dtype (the
gradients cleared in between), so that the BatchNorm buffers are seen to move on.

Run where the reference checkout is at hand ($LINETR_REFERENCE names it), on the CPU:

    LINETR_REFERENCE=<checkout> python tests/golden/make_golden_keyline.py

The reference is imported as SURVEY.md Appendix D does (cv2 stub; the reference's packages first on the path).  The weights and inputs are
NOT stored: they are drawn from np.random.RandomState(seed) by tests/keyline_reference.py (model_case()) and go into the reference's model
through load_state_dict(strict=True); a test draws them again.  Only data is written, the float64 run's, per call c = 0, 1 under <name>.<c>:
    line_desc [2, 256, 5]; d_desc: the gradient of desc_sublines [2, 5, 21, 256]; the gradient of every 1-D parameter (and of cls_token) in
    full; of every weight matrix W its gradient on the sub-grid W[::7, ::5]; after.<buffer>: every BatchNorm's running_mean, running_var
    and num_batches_tracked after the call;
    <tensor>_f32_err: max |float32 run - float64 run| over the WHOLE tensor, the float32 yardstick;
    state_dict_keys: the reference model's key set.
The gradients of call 1 equal those of call 0 bit for bit (only the buffers differ, and .train() does not read them), so they are stored
once, under .0; the same holds for line_desc, which is stored for both calls all the same.  In float64 all of it takes 2 MB, twice the size
a committed file may have, so it goes into two files: keyline.npz holds everything in float64 but the weight matrices' sub-grids, and
keyline_matrices.npz holds those, rounded to float32 (relative error 2^-24, a sixteenth of the bar's floor)."""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.path.abspath(os.environ["LINETR_REFERENCE"])
sys.path.insert(0, REFERENCE)   # FIRST on the path: `models` must be the reference's package
sys.path.append(os.path.dirname(HERE))          # tests/: keyline_reference.py (imports nothing of this repository's packages)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

import models as _ref_models  # noqa: E402
assert _ref_models.__file__.startswith(REFERENCE.rstrip("/") + "/"), _ref_models.__file__
from models.line_transformer import LineTransformer  # noqa: E402  (reference)

import keyline_reference as KR  # noqa: E402


def run(dtype):
    sd, inputs, upstream = KR.model_case()
    mod = LineTransformer({"mode": "train"}).to(dtype)
    mod.load_state_dict(KR.tensors(sd, dtype), strict=True)
    mod.train()
    drops = [m for m in mod.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) == 3
    for m in drops:
        m.p = 0.0
    assert len(list(mod.parameters())) == 153 and sum(isinstance(m, nn.BatchNorm1d) for m in mod.modules()) == 15
    res = KR.run_calls(mod, lambda: KR.data_tensors(inputs, dtype), torch.tensor(upstream, dtype=dtype),
                       forward=lambda data: mod(data)["line_desc"])
    return res, sorted(mod.state_dict())


def main():
    (f64, keys), (f32, _) = run(torch.float64), run(torch.float32)
    out, matrices = {"state_dict_keys": np.array(keys)}, {}
    for name, val in f64.items():
        key, call = name.rsplit(".", 1)
        if val.dtype != np.float64:
            out[name] = val
            continue
        err = np.abs(f32[name] - val).max()
        if call != "0" and not key.startswith("after.") and key != "line_desc":
            assert np.array_equal(val, f64[key + ".0"]), name            # the same bits as call 0: stored once
            continue
        if KR.is_matrix(key, val):
            matrices[name] = KR.sub_grid(key, val).astype(np.float32)
        else:
            out[name] = val
        out[name + "_f32_err"] = np.float64(err)
        print(f"keyline {name}: max |.| {np.abs(val).max():.3e}, float32 error {err:.2e}")
    for stem, what in (("keyline", out), ("keyline_matrices", matrices)):
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **what)
        print(f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
