"""CPU: the half-precision map surface as far as it shows without a GPU -- the built library exports the new entry point, the header, the
binding and the library agree on the two format constants, the size queries that take `dense_is_nhwc` answer at most their float32
answer for a half format and their own "refused" answer for a format the calls refuse, and the premises of the case tables of
tests/half_map_cases.py hold (sizes on both sides of every block edge, special cells that survive torch's rounding, point sets that
touch every map corner).  The size queries are plain host functions and the library loads without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import half_map_cases as hc
import sample_cases as sc
from linetr_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_constants():
    header = open(os.path.join(ROOT, "include", "linetr_hip.h")).read()
    consts = dict(re.findall(r"#define (LINETR_DENSE_\w+) (0x[0-9a-fA-F]+)", header))
    assert {k: int(v, 16) for k, v in consts.items()} == {"LINETR_DENSE_F16": 0x100, "LINETR_DENSE_BF16": 0x200}
    assert (nat.DENSE_F16, nat.DENSE_BF16) == (0x100, 0x200)
    assert nat.dense_type_bits(torch.float32) == 0 and nat.dense_type_bits(torch.float16) == 0x100
    assert nat.dense_type_bits(torch.bfloat16) == 0x200 and nat.dense_type_bits(torch.float64) is None
    assert re.search(r"\bint linetr_superpoint_heads_typed\(", header) and "linetr_superpoint_heads_typed" in nat.ABI
    exported = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T linetr_superpoint_heads_typed$", exported, flags=re.M)
    assert callable(nat.lib().linetr_superpoint_heads_typed)
    # every dense map parameter of the entry points that accept the bits is a const void*
    for fn in ("linetr_tokenize", "linetr_sample_descriptors", "linetr_describe", "linetr_describe_submit", "linetr_point_descriptors"):
        decl = re.search(r"\bint %s\((.*?)\);" % fn, header, flags=re.S).group(1)
        assert "const void* d_dense_desc" in decl, fn
    assert "const void* d_map" in re.search(r"\bint linetr_debug_cls_pool\((.*?)\);", header, flags=re.S).group(1)


BOTH = nat.DENSE_F16 | nat.DENSE_BF16


@pytest.mark.parametrize("hw", [(4, 8), (63, 65), (1, 1), (60, 80)])
def test_size_queries_with_format_bits(hw):
    L = nat.lib()
    Hc, Wc = hw
    for bits in (nat.DENSE_F16, nat.DENSE_BF16):
        for nhwc in (0, 1):
            f32 = L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, nhwc)
            half = L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, nhwc | bits)
            assert 0 <= half <= f32 and (half > 0) == (f32 > 0), (hw, nhwc, bits, half, f32)
            assert half >= Hc * Wc * 256 * 2 * (1 - nhwc)          # room for the half channel-last copy of an NCHW map
            for B in (1, 3):
                f32 = L.linetr_point_descriptors_workspace_bytes(B, Hc, Wc, nhwc)
                half = L.linetr_point_descriptors_workspace_bytes(B, Hc, Wc, nhwc | bits)
                assert 0 <= half <= f32 and half >= B * Hc * Wc * 256 * 2 * (1 - nhwc), (hw, B, nhwc, bits)
    # what the calls refuse: each query's own convention (0 here; linetr_describe_ragged_workspace_bytes, which needs a handle: -1,
    # tests/test_gpu_half_maps.py)
    for fmt in (BOTH, 1 | BOTH, 0x400, 1 | 0x400, nat.DENSE_F16 | 0x1000):
        assert L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, fmt) == 0, hex(fmt)
        assert L.linetr_point_descriptors_workspace_bytes(2, Hc, Wc, fmt) == 0, hex(fmt)
    # linetr_fixed_size takes float32 maps only: nothing to size for a format it refuses; the float32 answers stand
    for fmt in (nat.DENSE_F16, 1 | nat.DENSE_BF16, BOTH, 0x400):
        assert L.linetr_fixed_size_workspace_bytes(2, Hc * 8, Wc * 8, fmt) == 0, hex(fmt)
    assert L.linetr_fixed_size_workspace_bytes(2, Hc * 8, Wc * 8, 0) > L.linetr_fixed_size_workspace_bytes(2, Hc * 8, Wc * 8, 1) > 0
    # every value below 0x100 means what it meant, the negative ones too: non-zero = NHWC float32
    assert L.linetr_fixed_size_workspace_bytes(2, Hc * 8, Wc * 8, -1) == L.linetr_fixed_size_workspace_bytes(2, Hc * 8, Wc * 8, 1)
    assert L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, -1) == L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, 1) == 0


def test_sizes_straddle_the_block_edges():
    head = [h * w for h, w in hc.HEAD_MAPS]
    assert hc.straddles(head, hc.DESC_BLOCK) and hc.straddles(head, hc.SCORE_BLOCK)           # 32, 33, 35 | 64, 65
    assert any(p % 2 for p in head) and any(p % 4 == 0 for p in head) and 1 in head              # the scalar and the vector path
    sample = [h * w for h, w in hc.SAMPLE_MAPS]
    assert hc.straddles(sample, hc.LAYOUT_TILE) and any(p % 2 for p in sample)                   # 63, 64, 65; odd products
    assert any(p % 4 for p in sample) and any(p % 4 == 0 for p in sample)                        # rows on and off the 8-byte grid
    assert hc.pool_valid_tokens() == [5, 1, 3] and hc.pool_case()["N"] == 3 and hc.POOL_T == 5   # 5 valid; 1 valid + 4 padding
    assert len({int(r["image"]) for r in hc.pool_case()["recs"]}) == hc.POOL_IMAGES == 2


@pytest.mark.parametrize("kind", hc.KINDS)
def test_special_cells_survive_the_round_trip(kind):
    dtype = hc.HALF[kind][0]
    for Hc, Wc in hc.SAMPLE_MAPS:
        m16 = hc.map16(kind, 11, 2, Hc, Wc, special=True)
        assert m16.dtype == dtype and m16.shape == (2, 256, Hc, Wc)
        back = m16.float()
        sub = hc.special_subnormals()
        assert torch.equal(back[0, :, 0, 0], sub)                  # exact in both types
        assert float(back[0, hc.MAX_CHANNEL, Hc - 1, Wc - 1]) == torch.finfo(dtype).max
        assert bool(torch.isfinite(back).all())
        # rounding a rounded map changes nothing: the upcast is exact
        assert torch.equal(back.to(dtype).view(torch.int16), m16.view(torch.int16))
    if kind == "f16":
        sub = hc.special_subnormals()          # k * 2^-24, k = 1 .. 256: below the smallest normal fp16 2^-14 (k = 1024)
        assert float(sub[0]) == 2.0 ** -24 and float(sub.max()) < float(torch.finfo(torch.float16).smallest_normal)


def test_point_sets_touch_every_corner():
    for Hc, Wc in hc.SAMPLE_MAPS:
        pts = hc.sample_points(Hc, Wc)
        assert pts.dtype == torch.float32 and pts.shape[1] == 2
        for align in (False, True):
            gx = sc.grid_coord(pts[:, 0].double(), Wc, align)
            gy = sc.grid_coord(pts[:, 1].double(), Hc, align)
            for cx, cy in ((0, 0), (Wc - 1, 0), (0, Hc - 1), (Wc - 1, Hc - 1)):      # a point whose taps include the corner cell
                near = ((gx - cx).abs() < 1) & ((gy - cy).abs() < 1)
                assert bool(near.any()), (Hc, Wc, align, cx, cy)
            assert bool((gx < -0.5).any() and (gx > Wc - 0.5).any() and (gy < -0.5).any() and (gy > Hc - 0.5).any())     # half a cell outside
        # the two special points hit cells (0, 0) and (Hc - 1, Wc - 1) at weight 1 under align_corners
        sp = hc.special_points(Hc, Wc)
        gx, gy = sc.grid_coord(sp[:, 0], Wc, True), sc.grid_coord(sp[:, 1], Hc, True)
        assert gx.tolist() == [0.0, float(Wc - 1)] and gy.tolist() == [0.0, float(Hc - 1)]
