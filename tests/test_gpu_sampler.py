"""GPU: the two descriptor samplers (lt_token.h: sample_desc_kernel and sp_kp_desc_kernel, both on sample_one) alone against float64,
at the map's edges, on degenerate maps, at the block edges of their grids and with a different map per image.  Cases, references and
the bar: tests/sample_cases.py (its premises: tests/test_sample_cases_cpu.py).  Every test prints the worst error / bar per kernel,
family and map, the figures tools/sampler_unit_report.py writes to profiles/sampler_unit_errors.txt."""
import pytest
import torch

import sample_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


def judge(rows):
    print("\n" + "\n".join(S.worst_lines(rows)))
    bad = S.failures(rows)
    assert not bad, "\n".join(bad[:20])


def test_sample_descriptors_every_map_family_layout(eng):
    """linetr_sample_descriptors: n = 1, 3, 4, 5, 8, 9 and the whole case on every map, family and align_corners value; zero vectors
    exactly zero; the NCHW-fed result bit-identical to the NHWC-fed one"""
    rows = S.sweep_sample_descriptors(eng)
    assert {r[1] for r in rows} >= {"normal", "border", "planted", "border/zero", "border/layouts"}
    judge(rows)


def test_point_descriptors_at_the_count_edges(eng):
    """linetr_point_descriptors through the C ABI: 0, 1, 63, 64, 65, 128, 129 key points per image, the empty image first, in the
    middle and last, sentinels behind key points and maps, markers behind the output; every [256][n_b] block against float64 and,
    bit for bit, against linetr_sample_descriptors of its image; two calls give the same bits"""
    rows = S.sweep_point_descriptors(eng)
    assert {r[1] for r in rows} >= {"counts", "counts/same"}
    judge(rows)


def test_tokenize_samples_and_gathers_in_each_images_own_map(eng):
    """sample_desc_kernel with records and the score gather of tokenize_kernel on three images with different maps, T = 1, 3, 5"""
    judge(S.sweep_tokenize(eng))
