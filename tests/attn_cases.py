"""Case generator and error measure of the signature-attention unit tests (tests/test_gpu_attention.py; reused by
tools/attn_unit_report.py, which writes profiles/attn_unit_errors.txt).  Test infrastructure only.

Every case is a var-len batch (sub-line counts per image, seeded inputs) with two CPU references of the same formula: float64
(`ref64`) and plain float32 torch (`ref32`).  A kernel passes an image when

    max |gpu - ref64|  <=  FACTOR * max( max |ref32 - ref64| ,  2^-23 * max |v| )        (FACTOR = 8)

over that image's rows: the library's contract is that bf16x6 products are fp32-class (~2^-23 per product) and f32 mode is exact
fp32 MFMA, so a kernel may differ from float64 by what ANY fp32 evaluation differs, up to summation order, the log2-unit scaling
of the scores and v_exp_f32 -- the factor 8 is the allowance for those three, and the floor covers images of one sub-line, where
ref32 is exact.  The bar is a property of the references alone, never of a kernel's output."""
import functools
import zlib

import numpy as np
import torch

from helpers import attn_reference, from_reference_layout, to_kernel_layout
from oracle import linetr_oracle as O
from workloads import synth

KERNELS = ("sig_attn", "sig_attn_small", "sig_attn_split4", "sig_attn_split8", "sig_qkv_attn")
FUSED = 4
FACTOR = 8.0
# tile edges of every kernel: 32-row wave tiles and KV chunks, 64-row staged tiles, 128-query blocks / 128-key LDS halves, 256
COUNTS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256)
COUNTS_BIG = (257, 288, 289, 511, 512, 513, 599, 600, 767, 768, 769)      # kernels 0-3 only (the fused kernel ends at 256)
FAMILIES = ("normal", "peaky", "planted", "equal", "sentinel")
Z_FAMILIES = ("normal", "peaky", "sentinel")
SENTINEL = 1.0e4          # magnitude of everything a kernel must not read into an image (finite: a leak shows as a huge error, not NaN)
MARKER = -777.25          # what the output buffer holds before the launch
SPARE_ROWS = 8            # sentinel rows behind the batch's N rows of the input


def counts_for(kernel):
    return COUNTS if kernel == FUSED else COUNTS + COUNTS_BIG


def ragged_counts(kernel, seed=0):
    """Every count the kernel is tested at, shuffled (so that image offsets are multiples of nothing), with an empty image first,
    in the middle and last."""
    c = [n for n in counts_for(kernel) if n > 0]
    np.random.RandomState(1000 + seed + kernel).shuffle(c)
    mid = len(c) // 2
    return tuple([0] + c[:mid] + [0] + c[mid:] + [0])


def cu_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _gen(*key):
    """A CPU generator seeded by the key's text (stable from process to process, unlike hash())."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _sentinel_rows(shape, g):
    return SENTINEL * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


@functools.lru_cache(maxsize=None)
def qkv_case(family, counts, seed=0, parity=0):
    """Direct q/k/v inputs (kernels 0-3): dict with q, k, v [N, 4, 64] float32 (q UNSCALED), cu, ref64 / ref32 [N, 256] head-major
    and `check` = the images whose output is compared (all of them, except the sentinel images of the 'sentinel' family).
      normal    unit-variance normal q, k, v
      peaky     q x 4: |logit| up to ~20
      planted   for every (query, head) one key at a position drawn uniformly over the image has logit 30 (all others stay
                below ~13) and its v row carries a marker of 4 in a channel that depends on the key: a wrong running maximum,
                a wrong rescale when partial softmaxes are merged and a wrong P^T / V^T lane mapping all show
      equal     k = 0: every logit is 0 and the message is the plain mean of the image's v rows
      sentinel  'normal' in the images of one parity; the other images hold +-1e4 in q, k and v"""
    g = _gen(family, counts, seed)
    cu = cu_of(counts)
    N = int(cu[-1])
    q, k, v = (torch.randn((N, 4, 64), generator=g) for _ in range(3))
    check = [i for i in range(len(counts))]
    if family == "peaky":
        q = q * 4
    elif family == "equal":
        k = torch.zeros_like(k)
    elif family == "planted":
        v = 0.1 * v
        q = 0.3 * q
        for i, n in enumerate(counts):
            if n == 0:
                continue
            a = int(cu[i])
            tgt = torch.randint(0, n, (n, 4), generator=g)                   # [query, head] -> key of the same image
            kk = k[a:a + n]                                                    # [n, 4, 64]
            kt = torch.stack([kk[tgt[:, h], h] for h in range(4)], dim=1)      # the planted key of every (query, head)
            q[a:a + n] += 240.0 * kt / (kt * kt).sum(-1, keepdim=True)         # q . k_t / 8 = 30 (+ the 0.3-scaled noise)
            rows = torch.arange(n)
            for h in range(4):
                v[a + rows, h, (3 * rows + h) % 64] += 4.0
    elif family == "sentinel":
        check = [i for i in range(len(counts)) if i % 2 != parity]
        for i, n in enumerate(counts):
            if i % 2 == parity and n:
                a = int(cu[i])
                for t in (q, k, v):
                    t[a:a + n] = _sentinel_rows((n, 4, 64), g)
    elif family != "normal":
        raise ValueError(family)
    ref_cu = cu if family != "sentinel" else None
    if ref_cu is None:      # the sentinel images' own output is not compared: leave them out of the references
        r64, r32 = torch.zeros((N, 256), dtype=torch.float64), torch.zeros((N, 256))
        for i in check:
            a, b = int(cu[i]), int(cu[i + 1])
            one = np.array([0, b - a])
            r64[a:b] = attn_reference(q[a:b], k[a:b], v[a:b], one, torch.float64)
            r32[a:b] = attn_reference(q[a:b], k[a:b], v[a:b], one, torch.float32)
    else:
        r64 = attn_reference(q, k, v, cu, torch.float64)
        r32 = attn_reference(q, k, v, cu, torch.float32)
    return dict(family=family, counts=counts, cu=cu, q=q, k=k, v=v, vmax=to_kernel_layout(v).abs(), ref64=r64, ref32=r32, check=check)


def pack_qkv(case, ld=768, device="cuda:0"):
    """The kernel's input rows [N + SPARE_ROWS, ld] on the device: q / 8 | k | v head-major in the LAST 768 columns of every row,
    everything else -- the columns before them (x_out of the folded single-pair layout, ld = 1024) and the rows behind N -- holds
    sentinels.  Returns (whole buffer, the view to hand to the kernel)."""
    N = int(case["cu"][-1])
    g = _gen(77)
    buf = _sentinel_rows((N + SPARE_ROWS, ld), g)
    buf[:N, ld - 768:] = torch.cat([to_kernel_layout(case["q"] * 0.125), to_kernel_layout(case["k"]), to_kernel_layout(case["v"])], dim=1)
    buf = buf.to(device)
    return buf, buf[:, ld - 768:]


@functools.lru_cache(maxsize=None)
def state_dict_t(weights):
    """'calibrated' or an integer seed of synth.make_state_dict -> (numpy state_dict for Engine, torch state_dict for the oracle)."""
    sd = synth.calibrated_state_dict() if weights == "calibrated" else synth.make_state_dict(int(weights))
    return sd, synth.to_torch_state_dict(sd)


@functools.lru_cache(maxsize=None)
def z_case(family, counts, weights, layer, seed=0, parity=0):
    """Inputs of the fused projection + attention kernel: z rows [N, 256] ('normal': unit variance; 'peaky': x 2, i.e. scores x 4;
    'sentinel': +-1e4 rows in the images of one parity).  References: oracle.linetr_oracle.sig_attention -- the function the CPU
    golden tests pin -- per image, in float64 and in float32, brought to the head-major layout."""
    g = _gen(family, counts, weights, layer, seed)
    cu = cu_of(counts)
    N = int(cu[-1])
    z = torch.randn((N, 256), generator=g)
    check = [i for i in range(len(counts))]
    if family == "peaky":
        z = z * 2
    elif family == "sentinel":
        check = [i for i in range(len(counts)) if i % 2 != parity]
        for i, n in enumerate(counts):
            if i % 2 == parity and n:
                z[int(cu[i]):int(cu[i + 1])] = _sentinel_rows((n, 256), g)
    elif family != "normal":
        raise ValueError(family)
    sd_t = state_dict_t(weights)[1]
    r64, r32, vmax = torch.zeros((N, 256), dtype=torch.float64), torch.zeros((N, 256)), torch.zeros((N, 256))
    a_ = f"selfattn.layers.{layer}.attn.proj.2"
    for i in check:
        a, b = int(cu[i]), int(cu[i + 1])
        if a == b:
            continue
        r64[a:b] = from_reference_layout(O.sig_attention(sd_t, layer, z[a:b], dtype=torch.float64))
        r32[a:b] = from_reference_layout(O.sig_attention(sd_t, layer, z[a:b]))
        vmax[a:b] = torch.nn.functional.linear(z[a:b], sd_t[a_ + ".weight"][:, :, 0], sd_t[a_ + ".bias"]).abs()
    return dict(family=family, counts=counts, cu=cu, z=z, vmax=vmax, ref64=r64, ref32=r32, check=check, weights=weights, layer=layer)


def pack_z(case, device="cuda:0"):
    N = int(case["cu"][-1])
    buf = _sentinel_rows((N + SPARE_ROWS, 256), _gen(78))
    buf[:N] = case["z"]
    buf = buf.to(device)
    return buf, buf


def launch(eng, kernel, case, ld=768):
    """Runs `kernel` (-1: the dispatcher's choice) on the case; returns (message [N, 256] on the CPU, kernel used).  Asserts
    that the spare row behind the output still holds its marker."""
    N = int(case["cu"][-1])
    buf, x = pack_z(case, eng.device) if "z" in case else pack_qkv(case, ld, eng.device)
    out = torch.full((N + 1, 256), MARKER, dtype=torch.float32, device=eng.device)
    msg, used = eng.debug_sig_attention(kernel, x, case["cu"], layer=case.get("layer", 0), out=out[:N])
    torch.cuda.synchronize()
    assert bool((out[N] == MARKER).all()), "the row behind the output was written"
    return msg.cpu(), used


def image_errors(gpu, case, ref=None):
    """[(image, sub-lines, max |gpu - ref64|, bar)] for every compared image with at least one sub-line.  `ref`: compare with this
    tensor instead of ref64 (cross-kernel agreement); the bar stays the references' own."""
    cu = case["cu"]
    want = case["ref64"] if ref is None else ref.double()
    rows = []
    for i in case["check"]:
        a, b = int(cu[i]), int(cu[i + 1])
        if a == b:
            continue
        err = (gpu[a:b].double() - want[a:b]).abs().max().item()
        own = (case["ref32"][a:b].double() - case["ref64"][a:b]).abs().max().item()
        bar = FACTOR * max(own, 2.0 ** -23 * case["vmax"][a:b].max().item())
        rows.append((i, b - a, err, bar))
    return rows


def failures(rows):
    return [f"image {i} ({n} sub-lines): error {e:.3e} > bar {b:.3e} (x{e / b:.1f})" for i, n, e, b in rows if not e <= b]
