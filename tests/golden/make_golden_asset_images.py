#!/usr/bin/env python3
"""The grey images of the asset pair (make_golden_asset_pair.py: the first pair of the reference's demo list), decoded exactly as that
script decodes them (PIL's "L" conversion) and stored as uint8 [480,640] arrays: the INPUT of SuperPoint for the end-to-end test of the
native encoder (tests/test_gpu_sp_encoder.py), which needs real-image statistics in front of the key-point threshold.  Only data is
written.  Usage: python tests/golden/make_golden_asset_images.py [assets directory]"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
PAIR = ("scannet_0a.png", "scannet_0b.png")

if __name__ == "__main__":
    assets = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/assets"
    gray = [np.asarray(Image.open(os.path.join(assets, n)).convert("L").resize((640, 480)), np.uint8) for n in PAIR]
    assert all(g.shape == (480, 640) for g in gray)
    np.savez_compressed(os.path.join(HERE, "asset_pair_images.npz"), gray0=gray[0], gray1=gray[1])
