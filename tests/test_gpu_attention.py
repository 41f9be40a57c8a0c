"""GPU: each of the five signature-attention kernels ALONE (linetr_debug_sig_attention) against a float64 reference of
models/line_transformer.py:132-154, at the sub-line counts where their tiles end.

Kernels (linetr_net.hip: sig_attn_plan): 0 sig_attn_kernel (exact fp32 MFMA), 1 sig_attn_small_kernel (the 4 waves split the KV
range, partial softmaxes merged through LDS), 2 / 3 sig_attn_split_kernel<4> / <8>, 4 sig_qkv_attn_kernel (projection fused in).
Cases, input families and the bar -- max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |v|) per image, a property of the two
CPU references alone -- are in attn_cases.py; the float64 reference of kernel 4 is oracle.linetr_oracle.sig_attention, which
tests/test_oracle_golden.py pins through forward().  tools/attn_unit_report.py runs the same cases and writes the measured
error / bar ratios to profiles/attn_unit_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEED_WEIGHTS = 3           # synth.make_state_dict(3): the second set of projection weights of the fused kernel's cases
E_ARG = -1


@pytest.fixture(scope="module")
def engines():
    from linetr_amd.engine import Engine
    return {w: Engine(A.state_dict_t(w)[0], "cuda:0") for w in ("calibrated", SEED_WEIGHTS)}


@pytest.fixture(scope="module")
def eng(engines):
    return engines["calibrated"]


def check(eng, kernel, case, ld=768, expect_used=None):
    gpu, used = A.launch(eng, kernel, case, ld)
    assert used == (kernel if expect_used is None else expect_used)
    rows = A.image_errors(gpu, case)
    for i, n, e, b in rows:
        print(f"{A.KERNELS[used]} {case['family']} image {i} n={n}: err {e:.3e} bar {b:.3e} ratio {e / b:.3f}")
    return A.failures(rows)


def parities(family):
    return (0, 1) if family == "sentinel" else (0,)


# ---- kernels 0-3: direct q/k/v ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_qkv_kernel_ragged_batch(eng, kernel, family):
    """All counts 0 .. 769 in one shuffled batch (empty images first, in the middle and last).  'sentinel': every other image and
    all memory around the batch hold +-1e4; both parities run, so every count is compared."""
    bad = []
    for par in parities(family):
        bad += check(eng, kernel, A.qkv_case(family, A.ragged_counts(kernel), parity=par))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", ["normal", "planted"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_qkv_kernel_one_image_alone(eng, kernel, family):
    """Every count as a batch of ONE image (grid z = its own tile count, n0 = 0); a batch of one empty image launches nothing."""
    bad = []
    for n in A.counts_for(kernel):
        bad += [f"n = {n}: {m}" for m in check(eng, kernel, A.qkv_case(family, (n,)))]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", A.FAMILIES)
def test_small_kernel_row_stride_1024(eng, family):
    """sig_attn_small_kernel on the folded single-pair layout: q/k/v at column 256 of [N][1024] rows whose first 256 columns
    (x_out) hold sentinels."""
    bad = []
    for par in parities(family):
        bad += check(eng, 1, A.qkv_case(family, A.ragged_counts(1), parity=par), ld=1024)
    assert not bad, "\n".join(bad)


def test_split_kernels_agree_with_each_other(eng):
    """A bonus, not a substitute for the reference: kernels 1, 2, 3 on the same q/k/v agree within the same bar."""
    case = A.qkv_case("normal", A.ragged_counts(1))
    out = {k: A.launch(eng, k, case)[0] for k in (1, 2, 3)}
    bad = []
    for a, b in ((1, 2), (1, 3), (2, 3)):
        bad += [f"{A.KERNELS[a]} vs {A.KERNELS[b]}: {m}" for m in A.failures(A.image_errors(out[a], case, ref=out[b]))]
    assert not bad, "\n".join(bad)


def test_cfg5_batch_takes_split8(eng):
    """16 images x 599 sub-lines (the cfg5 shape): the dispatcher's own choice, which must be sig_attn_split_kernel<8>."""
    bad = check(eng, -1, A.qkv_case("normal", (599,) * 16), expect_used=3)
    assert not bad, "\n".join(bad)


# ---- kernel 4: projection + attention ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", A.Z_FAMILIES)
@pytest.mark.parametrize("layer", [0, 6])
@pytest.mark.parametrize("weights", ["calibrated", SEED_WEIGHTS])
def test_fused_kernel_ragged_batch(engines, weights, layer, family):
    bad = []
    for par in parities(family):
        bad += check(engines[weights], 4, A.z_case(family, A.ragged_counts(4), weights, layer, parity=par))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("weights,layer", [("calibrated", 0), (SEED_WEIGHTS, 6)])
def test_fused_kernel_one_image_alone(engines, weights, layer):
    bad = []
    for n in A.counts_for(4):
        bad += [f"n = {n}: {m}" for m in check(engines[weights], 4, A.z_case("normal", (n,), weights, layer))]
    assert not bad, "\n".join(bad)


def test_cfg3_batch_takes_the_fused_kernel(eng):
    """64 images x 199 sub-lines (the headline shape): the dispatcher's own choice, which must be sig_qkv_attn_kernel."""
    bad = check(eng, -1, A.z_case("normal", (199,) * 64, "calibrated", 0), expect_used=4)
    assert not bad, "\n".join(bad)


# ---- the dispatch table -----------------------------------------------------------------------------------------------------

def uniform(n_images, max_n):
    return A.cu_of([max_n] * n_images)


def ragged(n_images, max_n):
    """max_n in ONE image (not the first), the others short: the choice depends on the largest image only"""
    c = [min(max_n, 1 + (7 * i) % 20) for i in range(n_images)]
    c[n_images // 2] = max_n
    return A.cu_of(c)


DISPATCH = [   # (precision, n_images, max_n, kernel): both sides of every threshold of sig_attn_plan
    ("bf16x6", 15, 256, 1), ("bf16x6", 16, 256, 3),      # n_images * 4 * ceil(max_n / 256) < 64 -> small
    ("bf16x6", 7, 512, 1), ("bf16x6", 8, 512, 3),
    ("bf16x6", 5, 599, 1), ("bf16x6", 6, 599, 3),
    ("bf16x6", 31, 256, 3), ("bf16x6", 32, 256, 4), ("bf16x6", 32, 257, 3),      # fused: n_images * 4 >= 128, max_n <= 256
    ("bf16x6", 16, 128, 2), ("bf16x6", 16, 129, 3),      # split<4> up to 128 sub-lines
    ("bf16x6", 31, 128, 2), ("bf16x6", 32, 128, 4), ("bf16x6", 32, 1, 4), ("bf16x6", 1, 1, 1), ("bf16x6", 64, 199, 4),
    ("bf16x3", 15, 256, 1), ("bf16x3", 32, 128, 2), ("bf16x3", 32, 256, 3), ("bf16x3", 64, 199, 3),      # never fused
    ("f16x3", 15, 256, 1), ("f16x3", 32, 128, 2), ("f16x3", 32, 256, 3), ("f16x3", 64, 199, 3),
    ("f32", 1, 1, 0), ("f32", 2, 199, 0), ("f32", 16, 128, 0), ("f32", 32, 256, 0), ("f32", 64, 199, 0), ("f32", 16, 599, 0),
]


def test_dispatch_table(eng):
    """kernel = -1 with no tensors reports what the forward pass would take and launches nothing.  The fold of the single-pair
    path (N <= 960 with the small kernel) changes which GEMMs run, not the attention kernel: small needs fewer than 16 images,
    fused at least 32, so N = 960 / 961 both take sig_attn_small_kernel."""
    got, want = [], []
    try:
        for prec, n_images, max_n, kernel in DISPATCH:
            eng.set_precision(prec)
            for cu in (uniform(n_images, max_n), ragged(n_images, max_n)):
                got.append((prec, n_images, max_n, eng.sig_attention_kernel(cu)))
                want.append((prec, n_images, max_n, kernel))
        eng.set_precision("bf16x6")
        for cu in (A.cu_of([480, 480]), A.cu_of([480, 481]), A.cu_of([199, 199])):
            got.append(("bf16x6", 2, int(cu[-1]), eng.sig_attention_kernel(cu)))
            want.append(("bf16x6", 2, int(cu[-1]), 1))
    finally:
        eng.set_precision("bf16x6")
    assert got == want


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def raw_call(eng, kernel, layer, x, ld, cu, msg):
    cu = np.ascontiguousarray(cu, dtype=np.int32)
    used = C.c_int32(-1)
    code = eng._L.linetr_debug_sig_attention(eng._h, kernel, layer, x.data_ptr() if x is not None else None, ld, cu.ctypes.data,
                                             len(cu) - 1, msg.data_ptr() if msg is not None else None, C.byref(used), None)
    return code, eng._L.linetr_last_error().decode()


def test_refusals(eng):
    """What a kernel is not written for is refused with LINETR_E_ARG and a message; nothing is launched (the output keeps its
    marker)."""
    cu = A.cu_of([40, 200])
    N = int(cu[-1])
    x = torch.zeros((N + 1, 1024), device="cuda:0")
    msg = torch.full((N, 256), A.MARKER, device="cuda:0")
    cases = [("fused, max_n > 256", 4, 0, 256, A.cu_of([257, 3])),
             ("fused, layer -1", 4, -1, 256, cu), ("fused, layer 7", 4, 7, 256, cu), ("fused, ld_in 768", 4, 0, 768, cu),
             ("sig_attn, ld_in 1024", 0, 0, 1024, cu), ("split<4>, ld_in 1024", 2, 0, 1024, cu),
             ("split<8>, ld_in 1024", 3, 0, 1024, cu), ("small, ld_in 512", 1, 0, 512, cu), ("small, ld_in 256", 1, 0, 256, cu),
             ("kernel 5", 5, 0, 768, cu), ("kernel -2", -2, 0, 768, cu),
             ("cu_sub not monotone", 1, 0, 768, np.array([0, 5, 3])), ("cu_sub[0] != 0", 1, 0, 768, np.array([1, 5]))]
    bad = []
    for what, kernel, layer, ld, c in cases:
        code, text = raw_call(eng, kernel, layer, x, ld, c, msg)
        if code != E_ARG or not text:
            bad.append((what, code, text))
    code, text = raw_call(eng, 1, 0, x[:, 1:], 768, cu, msg)          # 4-byte aligned only
    if code != E_ARG or not text:
        bad.append(("misaligned input", code, text))
    code, text = raw_call(eng, 1, 0, None, 768, cu, msg)
    if code != E_ARG or not text:
        bad.append(("null input", code, text))
    try:
        for prec in ("f32", "bf16x3", "f16x3"):
            eng.set_precision(prec)
            code, text = raw_call(eng, 4, 0, x, 256, cu, msg)
            if code != E_ARG or not text:
                bad.append((f"fused in {prec} mode", code, text))
    finally:
        eng.set_precision("bf16x6")
    torch.cuda.synchronize()
    assert not bad, bad
    assert bool((msg == A.MARKER).all())


def test_training_mode_handle_is_refused():
    from linetr_amd.engine import Engine
    eng = Engine(A.state_dict_t("calibrated")[0], "cuda:0", bn_batch_stats=True)
    x = torch.zeros((8, 768), device="cuda:0")
    msg = torch.full((8, 256), A.MARKER, device="cuda:0")
    for kernel in (-1, 0, 1, 2, 3, 4):
        code, text = raw_call(eng, kernel, 0, x, 768 if kernel != 4 else 256, A.cu_of([8]), msg)
        assert code == E_ARG and text, (kernel, code, text)
    torch.cuda.synchronize()
    assert bool((msg == A.MARKER).all())
