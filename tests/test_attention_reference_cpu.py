"""CPU (no GPU needed): the references the GPU attention unit tests (test_gpu_attention.py) measure against.
oracle.linetr_oracle.sig_attention is the attention forward() runs -- so the golden fixtures of test_oracle_golden.py pin it --
and the layout helpers map the reference's channel order onto the library's."""
import numpy as np
import torch
import torch.nn.functional as F

import attn_cases as A
from helpers import attn_reference, from_reference_layout, to_kernel_layout
from oracle import linetr_oracle as O
from workloads import synth

torch.set_grad_enabled(False)


def test_layout_helpers_on_an_index_ramp():
    """reference channel c = d*4 + h  <->  head-major c' = h*64 + d (linetr_core.hip, signature layers)"""
    ramp = torch.arange(3 * 256, dtype=torch.float32).reshape(3, 256)
    hm = from_reference_layout(ramp)
    for n in range(3):
        for h in range(4):
            for d in range(64):
                assert hm[n, h * 64 + d] == ramp[n, d * 4 + h]
    x = torch.arange(3 * 4 * 64, dtype=torch.float32).reshape(3, 4, 64)
    km = to_kernel_layout(x)
    assert km.shape == (3, 256) and all(km[n, h * 64 + d] == x[n, h, d] for n in range(3) for h in range(4) for d in (0, 1, 63))
    # the two meet: reference rows viewed as [N, dh, heads] (line_transformer.py:151) are to_kernel_layout of their transpose
    assert torch.equal(hm, to_kernel_layout(ramp.reshape(3, 64, 4).transpose(1, 2)))


def test_sig_attention_float32_is_the_formula_forward_ran():
    """Bit-identical to lines :132-136 written out as forward() had them inline, per image and as a [B, N, 256] batch."""
    sd = synth.to_torch_state_dict(synth.calibrated_state_dict())
    z = torch.randn((3, 57, 256), generator=torch.Generator().manual_seed(5))
    for layer in (0, 6):
        a = f"selfattn.layers.{layer}.attn"
        for b in range(3):
            qkv = [F.linear(z[b], sd[f"{a}.proj.{j}.weight"][:, :, 0], sd[f"{a}.proj.{j}.bias"]).view(57, 64, 4) for j in range(3)]
            sc = torch.einsum("ndh,mdh->hnm", qkv[0], qkv[1]) / 64 ** 0.5
            msg = torch.einsum("hnm,mdh->ndh", F.softmax(sc, dim=-1), qkv[2]).reshape(57, 256)
            assert torch.equal(O.sig_attention(sd, layer, z[b]), msg)
        qkv = [F.linear(z.reshape(171, 256), sd[f"{a}.proj.{j}.weight"][:, :, 0], sd[f"{a}.proj.{j}.bias"]).view(3, 57, 64, 4)
               for j in range(3)]
        sc = torch.einsum("bndh,bmdh->bhnm", qkv[0], qkv[1]) / 64 ** 0.5
        msg = torch.einsum("bhnm,bmdh->bndh", F.softmax(sc, dim=-1), qkv[2]).reshape(3, 57, 256)
        assert torch.equal(O.sig_attention(sd, layer, z), msg)


def test_attn_reference_is_the_oracle_attention_on_projected_rows():
    """attn_reference (q/k/v given, kernels 0-3) and the oracle's sig_attention (z given, fused kernel) are the same function:
    project in float64, hand the projections over head-major, compare."""
    sd = synth.to_torch_state_dict(synth.calibrated_state_dict())
    counts = (5, 0, 33, 1)
    cu = A.cu_of(counts)
    z = torch.randn((int(cu[-1]), 256), generator=torch.Generator().manual_seed(6)).double()
    a = "selfattn.layers.2.attn"
    q, k, v = (from_reference_layout(F.linear(z, sd[f"{a}.proj.{j}.weight"][:, :, 0].double(), sd[f"{a}.proj.{j}.bias"].double()))
               .reshape(-1, 4, 64) for j in range(3))
    got = attn_reference(q, k, v, cu, torch.float64)
    for i in range(len(counts)):
        s, e = int(cu[i]), int(cu[i + 1])
        if e > s:
            want = from_reference_layout(O.sig_attention(sd, 2, z[s:e], dtype=torch.float64))
            assert (got[s:e] - want).abs().max().item() < 1e-13


def test_case_generator_is_reproducible_and_inside_its_own_bar():
    """Seeds do not depend on the process (no hash()), every listed count appears, and the float32 reference itself sits a
    factor 8 inside the bar by construction."""
    for kernel in (1, 4):
        c = A.ragged_counts(kernel)
        assert sorted(set(c)) == sorted(A.counts_for(kernel)) and c[0] == 0 and c[-1] == 0 and 0 in c[1:-1]
    case = A.qkv_case("planted", (33, 0, 129))
    assert abs(float(case["q"].double().sum()) - float(A.qkv_case.__wrapped__("planted", (33, 0, 129))["q"].double().sum())) == 0
    sc = torch.einsum("nhd,mhd->hnm", case["q"][:33] * 0.125, case["k"][:33])
    top = sc.topk(2, dim=-1).values
    assert (top[..., 0] - 30).abs().max() < 3 and (top[..., 0] - top[..., 1]).min() > 8
    for family in A.FAMILIES:
        case = A.qkv_case(family, (33, 129, 0))
        rows = A.image_errors(case["ref32"], case)
        assert rows and all(e * A.FACTOR <= b for _, _, e, b in rows)
    assert np.array_equal(case["cu"], [0, 33, 162, 162])
