#!/usr/bin/env python3
"""Golden fixture for the fused SuperPoint-head producer, from the REAL reference.

    python tests/golden/make_golden_superpoint.py        (build container only: needs /root/reference)

The reference's SuperPoint constructor loads `weights/superpoint_v1.pth`, which is not in the checkout; weights are
data, so `torch.load` is pointed at the seeded state_dict of `workloads.synth.superpoint_state_dict` for the
duration of the constructor.  Forward hooks capture the raw head outputs (convPb / convDb); the fixture holds those
inputs plus everything `SuperPoint.forward` returns.  Only data is written.

torch's CPU softmax / normalize round differently per ATen CPU kernel path (ATEN_CPU_CAPABILITY) and, for softmax, per thread
count.  So superpoint_heads_paths.npz holds, for every path of an x86 build, the dense maps `SuperPoint.forward` computes on ONE thread
from the stored head inputs (hooks hand convPb / convDb's outputs back as the stored arrays), PATH as
torch.backends.cpu.get_cpu_capability() names it.  They differ from the fixture's dense_score / dense_descriptor by a few units in the
last place, so each is stored as those bit differences: ulps_dense_score_<PATH> / ulps_dense_descriptor_<PATH> (int8,
map = (fixture map viewed as int32 + ulps) viewed as float32).  `--kernel-paths` writes only that file.
"""
import os
import subprocess
import sys
import tempfile
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))   # linetr_amd (seeded inputs / weights)
sys.path.insert(0, "/root/reference")   # FIRST on the path: `models` must be the reference's package, not this repo's shim

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_grad_enabled(False)
import models.superpoint as ref_sp  # noqa: E402  (reference)
assert ref_sp.__file__.startswith("/root/reference/"), ref_sp.__file__

from workloads import synth  # noqa: E402


def build(seed, **cfg):
    sd = {k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(seed).items()}
    real_load = torch.load
    torch.load = lambda *a, **k: sd
    try:
        m = ref_sp.SuperPoint(cfg).eval()
    finally:
        torch.load = real_load
    return m


KERNEL_PATHS = ("default", "avx2", "avx512")      # ATEN_CPU_CAPABILITY values of an x86 torch build


def heads_on_stored_inputs(path, out):
    """(run with ATEN_CPU_CAPABILITY set) this process's kernel path, one thread, on the fixture's stored head inputs"""
    g = np.load(path)
    torch.set_num_threads(1)
    m = build(0, max_keypoints=-1, keypoint_threshold=0.005, nms_radius=4, remove_borders=4)
    m.convPb.register_forward_hook(lambda mod, i, o: torch.from_numpy(g["score_logits"]))
    m.convDb.register_forward_hook(lambda mod, i, o: torch.from_numpy(g["desc_raw"]))
    r = m({"image": torch.from_numpy(g["image"])})
    np.savez(out, path=np.str_(torch.backends.cpu.get_cpu_capability()), dense_score=r["dense_score"].numpy(),
             dense_descriptor=r["dense_descriptor"].numpy())


def add_kernel_paths(path):
    fx = np.load(path)
    ulps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for cap in KERNEL_PATHS:
            out = os.path.join(tmp, cap + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--heads", path, out], check=True,
                           env=dict(os.environ, ATEN_CPU_CAPABILITY=cap))
            r = np.load(out)
            name = str(r["path"])
            assert name.lower() == cap, (name, cap)
            for k in ("dense_score", "dense_descriptor"):
                d = r[k].view(np.int32).astype(np.int64) - fx[k].view(np.int32).astype(np.int64)
                assert np.abs(d).max() <= 127, (name, k, np.abs(d).max())
                ulps[f"ulps_{k}_{name}"] = d.astype(np.int8)
    out = os.path.join(HERE, "superpoint_heads_paths.npz")
    np.savez_compressed(out, **ulps)
    print(out, {k: int(np.abs(v).max()) for k, v in ulps.items()})


def main():
    m = build(0, max_keypoints=-1, keypoint_threshold=0.005, nms_radius=4, remove_borders=4)
    cap = {}
    m.convPb.register_forward_hook(lambda mod, i, o: cap.__setitem__("score_logits", o.detach().clone()))
    m.convDb.register_forward_hook(lambda mod, i, o: cap.__setitem__("desc_raw", o.detach().clone()))
    g = torch.Generator().manual_seed(7)
    img = torch.rand(2, 1, 64, 96, generator=g)
    out = m({"image": img})
    fx = {"image": img.numpy(), "score_logits": cap["score_logits"].numpy(), "desc_raw": cap["desc_raw"].numpy(),
          "dense_score": out["dense_score"].numpy(), "dense_descriptor": out["dense_descriptor"].numpy(),
          "weights_seed": np.int64(0)}
    for b in range(2):
        fx[f"keypoints{b}"] = out["keypoints"][b].numpy()
        fx[f"scores{b}"] = out["scores"][b].numpy()
        fx[f"descriptors{b}"] = out["descriptors"][b].numpy()
    path = os.path.join(HERE, "superpoint_heads.npz")
    np.savez_compressed(path, **fx)
    print(path, {k: getattr(v, "shape", None) for k, v in fx.items()})
    add_kernel_paths(path)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--heads"]:
        heads_on_stored_inputs(*sys.argv[2:4])
    elif sys.argv[1:2] == ["--kernel-paths"]:
        add_kernel_paths(os.path.join(HERE, "superpoint_heads.npz"))
    else:
        main()
