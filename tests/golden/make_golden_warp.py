#!/usr/bin/env python3
"""Golden fixture of the homography views: the reference's own inv_warp_image_batch (dataloaders/utils/utils.py:317-351) in both modes
and compute_valid_mask(..., erosion_radius=0) (:677-704) on seeded image batches under homographies drawn with the builder's sampler.

    python tests/golden/make_golden_warp.py      ->  tests/golden/warp.npz

Runs the REAL reference on the CPU (same harness as make_golden.py: cv2 is a stub module, never called at erosion_radius = 0).  Per
case c (tests/warp_reference.py SHAPES): `img_c` float32 [B,C,H,W] (seeded multiples of 1/256 in [0, 1): they compress), `mat_c` the
NORMALISED float32 matrices [B,3,3] handed to the reference (the inverse of workloads.synth.sample_homography(HOMOGRAPHY_PARAMS)),
`bilinear_c` / `nearest_c` its outputs, `mask_c` its valid mask [B,H,W], and `ref_dev_c`: the largest |reference - float64
restatement| of the bilinear output (the reference's float32 grid against tests/warp_reference.py).  The script asserts what
tests/test_warp_cpu.py asserts, so a fixture that would fail there is never written."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up the cv2 stub and puts /root/reference first on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, "/root/reference/dataloaders")
from utils import utils as ref_utils  # noqa: E402  (reference; torch / numpy only on the paths used here)
assert ref_utils.__file__.startswith("/root/reference/"), ref_utils.__file__

sys.path.insert(0, os.path.join(HERE, ".."))
import warp_reference as R  # noqa: E402
from workloads import synth  # noqa: E402

SEED = 4100


def main():
    arrs = {"shapes": np.array(R.SHAPES)}
    for c, (B, C, H, W) in enumerate(R.SHAPES):
        rs = np.random.RandomState(SEED + c)
        img = (rs.randint(0, 256, size=(B, C, H, W)) / 256.0).astype(np.float32)
        mat = np.stack([np.linalg.inv(synth.sample_homography(rs, **synth.HOMOGRAPHY_PARAMS)) for _ in range(B)]).astype(np.float32)
        t_img, t_mat = torch.from_numpy(img), torch.from_numpy(mat)
        out = {mode: ref_utils.inv_warp_image_batch(t_img, t_mat, "cpu", mode).numpy() for mode in ("bilinear", "nearest")}
        mask = ref_utils.compute_valid_mask((H, W), t_mat, "cpu", erosion_radius=0).numpy()
        assert out["bilinear"].shape == (B, C, H, W) and out["bilinear"].dtype == np.float32 and mask.shape == (B, H, W)
        assert mask.dtype == np.float32 and set(np.unique(mask)) <= {0.0, 1.0}
        pix = R.normalised_to_pixel(mat, H, W)
        dev = 0.0
        for b in range(B):
            want, _ = R.warp(img[b], pix[b], "bilinear")
            dev = max(dev, float(np.abs(out["bilinear"][b] - want).max()))
            ex = R.near_rounding_boundary(pix[b], H, W, R.EXCUSE_REF)
            R.check_discrete(out["nearest"][b], R.warp(img[b], pix[b], "nearest")[0].astype(np.float32), ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} nearest")
            R.check_discrete(mask[b], R.valid_mask(pix[b], H, W), ex, R.EXCUSE_REF_SHARE, f"case {c} image {b} mask")
        print(f"case {c} {B}x{C}x{H}x{W}: bilinear deviation of the reference from float64 {dev:.3e}, valid share {mask.mean():.3f}")
        assert dev <= 1e-4
        arrs.update({f"img_{c}": img, f"mat_{c}": mat, f"bilinear_{c}": out["bilinear"], f"nearest_{c}": out["nearest"],
                     f"mask_{c}": mask.astype(np.uint8), f"ref_dev_{c}": np.float64(dev)})
    G.save("warp", **arrs)
    assert os.path.getsize(os.path.join(HERE, "warp.npz")) < 1000000


if __name__ == "__main__":
    main()
