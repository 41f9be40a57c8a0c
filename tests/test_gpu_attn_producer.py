"""GPU: the two forms of sig_qkv_attn_kernel (lt_attn_fused.h) ALONE and through the signature network.

Forced kernel 4 runs a batch whose largest image has at most 224 sub-lines in the producer form -- seven row-owning waves, the
eighth wave the operand ring's only DMA issuer -- and a batch with a larger image in the eight-compute-wave form; forced kernel
4 + LINETR_SIG_EIGHT_WAVES (36) runs the eight-compute-wave form whatever the size.  Checked here: every count at which a wave
tile, a key half or the choice between the forms ends, against the float64 reference and under the bar of attn_cases.py
(8 max(max |ref32 - ref64|, 2^-23 max |v|) per image); the two forms bit for bit against each other; two runs of the producer form
bit for bit; +-1e4 in the neighbouring images and behind the input, a marker behind the output (attn_cases.launch); and the
smallest batch the dispatcher gives to the fused plan, through linetr_debug_stage's signature network, against the same call
with the eight-compute-wave form forced."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_cases as A
import stage_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEED_WEIGHTS = 3
E_ARG = -1
FUSED = A.FUSED
EIGHT = FUSED + 32         # 4 + LINETR_SIG_EIGHT_WAVES
PRODUCER_MAX = 224
# one key half and two; the last full wave, the headline count, the last row of the seventh wave
COUNTS_PRODUCER = (1, 2, 31, 32, 33, 127, 128, 129, 191, 192, 193, 199, 223, 224)
COUNTS_EIGHT = (225, 256)


def producer_batch():
    """every count up to 224, shuffled (so that image offsets are multiples of nothing), with an empty image first, in the middle and last"""
    c = list(COUNTS_PRODUCER)
    np.random.RandomState(224).shuffle(c)
    mid = len(c) // 2
    return tuple([0] + c[:mid] + [0] + c[mid:] + [0])


PRODUCER_BATCH = producer_batch()
# max_n = 256: the whole batch, its images of up to 224 sub-lines included, takes the eight-compute-wave form
MIXED_BATCH = (224, 225, 0, 199, 256, 33, 225, 224, 1)


@pytest.fixture(scope="module")
def engines():
    from linetr_amd.engine import Engine
    return {w: Engine(A.state_dict_t(w)[0], "cuda:0") for w in ("calibrated", SEED_WEIGHTS)}


def launch(eng, kernel, case):
    gpu, used = A.launch(eng, kernel, case)
    assert used == kernel
    return gpu


def against_float64(tag, gpu, case):
    rows = A.image_errors(gpu, case)
    for i, n, e, b in rows:
        print(f"{tag} {case['family']} image {i} n={n}: err {e:.3e} bar {b:.3e} ratio {e / b:.3f}")
    return [f"{tag}: {m}" for m in A.failures(rows)]


def differing_images(a, b, case):
    """compared images whose rows differ in any bit"""
    cu = case["cu"]
    return [(i, int(cu[i + 1] - cu[i])) for i in case["check"] if not torch.equal(a[int(cu[i]):int(cu[i + 1])], b[int(cu[i]):int(cu[i + 1])])]


def parities(family):
    return (0, 1) if family == "sentinel" else (0,)


def run_both_forms(eng, case, producer):
    """kernel 4 twice and kernel 36 once on the case: every output against float64, the three bit-equal.  `producer`: whether kernel 4
    takes the producer form here (only named in the messages: the two forms must agree either way)."""
    form = "producer" if producer else "eight waves by size"
    out, again, eight = launch(eng, FUSED, case), launch(eng, FUSED, case), launch(eng, EIGHT, case)
    bad = against_float64(f"kernel 4 ({form})", out, case) + against_float64("kernel 36", eight, case)
    bad += [f"kernel 4 ({form}): two runs differ in image {i} ({n} sub-lines)" for i, n in differing_images(out, again, case)]
    bad += [f"kernel 4 ({form}) and kernel 36 differ in image {i} ({n} sub-lines)" for i, n in differing_images(out, eight, case)]
    return bad


@pytest.mark.parametrize("family", A.Z_FAMILIES)
@pytest.mark.parametrize("layer", [0, 6])
@pytest.mark.parametrize("weights", ["calibrated", SEED_WEIGHTS])
def test_producer_ragged_batch(engines, weights, layer, family):
    """Every count up to 224 in one shuffled batch with an empty image first, in the middle and last.  'sentinel': every other image and
    the rows behind the batch hold +-1e4; both parities run, so every count is compared."""
    bad = []
    for par in parities(family):
        bad += run_both_forms(engines[weights], A.z_case(family, PRODUCER_BATCH, weights, layer, parity=par), True)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", A.Z_FAMILIES)
@pytest.mark.parametrize("weights,layer", [("calibrated", 0), ("calibrated", 6), (SEED_WEIGHTS, 0), (SEED_WEIGHTS, 6)])
def test_mixed_batch_takes_eight_waves(engines, weights, layer, family):
    """224 and 225 (and 256) in one batch: the largest image decides, the whole batch runs with eight compute waves."""
    bad = []
    for par in parities(family):
        bad += run_both_forms(engines[weights], A.z_case(family, MIXED_BATCH, weights, layer, parity=par), False)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("weights,layer", [("calibrated", 0), (SEED_WEIGHTS, 6)])
def test_one_image_alone(engines, weights, layer):
    """Every count as a batch of ONE image (n0 = 0, the count itself decides the form); a batch of one empty image launches nothing."""
    bad = []
    for n in (0,) + COUNTS_PRODUCER + COUNTS_EIGHT:
        bad += [f"n = {n}: {m}" for m in run_both_forms(engines[weights], A.z_case("normal", (n,), weights, layer), n <= PRODUCER_MAX)]
    assert not bad, "\n".join(bad)


def test_through_the_dispatcher():
    """32 images x 199 sub-lines, the smallest batch sig_attn_plan gives to the fused plan: the signature network by the dispatcher's
    own choice (plan 4, the producer form) and with the eight-compute-wave form forced give the same bits in line_desc and in every
    tap."""
    from linetr_amd.engine import Engine
    eng = Engine(S.weights_t("calibrated", 7)[0], "cuda:0", n_sig_layers=7)
    case = S.sig_case("normal", (199,) * 32)
    desc, taps, used = S.launch_sig(eng, case, -1)
    desc8, taps8, used8 = S.launch_sig(eng, case, EIGHT)
    assert (used, used8) == (FUSED, EIGHT)
    assert bool(torch.isfinite(desc).all()) and float(desc.abs().max()) > 0
    assert torch.equal(desc, desc8) and torch.equal(taps, taps8)


def test_refusals(engines):
    """The eight-compute-wave id is the fused kernel's: refused where kernel 4 is, and no other number above 4 is a kernel."""
    eng = engines["calibrated"]
    cu = A.cu_of([40, 200])
    N = int(cu[-1])
    x = torch.zeros((N + 1, 1024), device="cuda:0")
    msg = torch.full((N, 256), A.MARKER, device="cuda:0")

    def raw(kernel, layer, ld, c):
        c = np.ascontiguousarray(c, dtype=np.int32)
        used = C.c_int32(-1)
        code = eng._L.linetr_debug_sig_attention(eng._h, kernel, layer, x.data_ptr(), ld, c.ctypes.data, len(c) - 1, msg.data_ptr(),
                                                 C.byref(used), None)
        return code, eng._L.linetr_last_error().decode()

    cases = [("36, max_n > 256", EIGHT, 0, 256, A.cu_of([257, 3])), ("36, layer 7", EIGHT, 7, 256, cu), ("36, ld_in 768", EIGHT, 0, 768, cu),
             ("kernel 32", 32, 0, 768, cu), ("kernel 35", 35, 0, 768, cu), ("kernel 37", 37, 0, 256, cu), ("kernel 6", 6, 0, 256, cu)]
    bad = [(what, *r) for what, k, l, ld, c in cases for r in [raw(k, l, ld, c)] if r[0] != E_ARG or not r[1]]
    try:
        eng.set_precision("f32")
        r = raw(EIGHT, 0, 256, cu)
        if r[0] != E_ARG or not r[1]:
            bad.append(("36 in f32 mode", *r))
    finally:
        eng.set_precision("bf16x6")
    torch.cuda.synchronize()
    assert not bad, bad
    assert bool((msg == A.MARKER).all())
