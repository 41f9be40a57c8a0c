"""Cases, CPU references and the error bar of the native SuperPoint encoder's tests (test_sp_encoder_cpu.py, test_gpu_sp_encoder.py,
tools/sp_encoder_report.py).  Nothing here touches the GPU.

The bar is a property of the CPU references alone.  Per compared tensor:

    max |gpu - ref64| <= FACTOR * max( max |ref32 - ref64| , 2^-23 * max |ref64| )

ref64 = torch.nn.functional.conv2d / relu / max_pool2d on the CPU in float64 from the state_dict-layout weights, ref32 the same in
float32.  The `integers` and `one-hot` families have exact sums (small integers), so ref32 == ref64 bit for bit and the GPU result
must EQUAL them."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from attn_cases import FACTOR, SENTINEL, SPARE_ROWS  # noqa: F401  (re-exported: the GPU tests take all three from here)
from workloads import synth

MARKER = -777.25                       # what an output buffer holds before the launch
PAIRS = ((64, 64), (64, 128), (128, 128), (128, 256), (128, 512))      # (Cin, Cout) of the 3x3 layers; 128 -> 512 = convPa | convDa
CHAIN = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")
POOL_AFTER = ("conv1b", "conv2b", "conv3b")
CK = 32                                # input channels per staged chunk of the kernel: the packing's outer K index


def bar(ref32, ref64):
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    if ref64.size == 0:
        return 0.0
    return FACTOR * max(np.abs(ref32 - ref64).max(), 2.0 ** -23 * np.abs(ref64).max())


def sizes(TH, TW):
    """(H, W, B): every H of {1, 2, 3, TH-1, TH, TH+1, 2TH+1} and every W of the same set on TW, each H with two W (a cyclic design:
    all 7 H and all 7 W appear twice, against different partners), B alternating 1 / 3."""
    hs = (1, 2, 3, TH - 1, TH, TH + 1, 2 * TH + 1)
    ws = (1, 2, 3, TW - 1, TW, TW + 1, 2 * TW + 1)
    out = []
    for shift in (0, 3):
        for i, h in enumerate(hs):
            out.append((h, ws[(i + shift) % 7], 1 if (i + shift) % 2 == 0 else 3))
    return out


def layer_inputs(family, cin, cout, B, H, W, seed=0):
    """x [B,H,W,cin] channel-last, w [cout,cin,3,3], b [cout] as float32 NumPy arrays.
    normal: He-scaled weights, O(1) activations.  integers: small integers everywhere -- every partial sum is an integer below
    2^24, exact in any order.  negative: integers with non-negative inputs, non-positive weights and negative biases: every
    pre-activation is negative, ReLU gives exact zeros."""
    rs = np.random.RandomState(1000 * cin + cout + 7 * H + 13 * W + B + 100003 * seed)
    if family == "normal":
        x = rs.standard_normal((B, H, W, cin))
        w = rs.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))
        b = rs.standard_normal(cout) * 0.05
    elif family == "integers":
        x = rs.randint(-3, 4, (B, H, W, cin))
        w = rs.randint(-2, 3, (cout, cin, 3, 3))
        b = rs.randint(-4, 5, cout)
    elif family == "negative":
        x = rs.randint(0, 4, (B, H, W, cin))
        w = -rs.randint(0, 3, (cout, cin, 3, 3))
        b = -rs.randint(1, 5, cout)
    else:
        raise ValueError(family)
    return x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def one_hot_inputs(cin, cout, H, W, tap, corner, seed=0):
    """One non-zero pixel (a corner of the image: 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right) and one non-zero tap
    (tap = 3 ky + kx), small integers: a dropped or swapped tap, a flipped kernel or a wrong pad moves or loses the response."""
    rs = np.random.RandomState(17 * tap + corner + 31 * cin + cout + 1009 * seed)
    x = np.zeros((1, H, W, cin), np.float32)
    x[0, (H - 1) * (corner >> 1), (W - 1) * (corner & 1)] = rs.randint(1, 4, cin)
    w = np.zeros((cout, cin, 3, 3), np.float32)
    w[:, :, tap // 3, tap % 3] = rs.randint(-2, 3, (cout, cin))
    b = rs.randint(0, 3, cout).astype(np.float32)
    return x, w, b


def conv_ref(x, w, b, dtype, relu=True):
    """relu(conv3x3(x) + b) before any pooling: x [B,H,W,cin] channel-last NumPy -> [B,H,W,cout] NumPy of `dtype`"""
    t = torch.from_numpy(np.array(x, order="C")).to(dtype).permute(0, 3, 1, 2)      # a copy: the shared cases are read-only arrays
    y = F.conv2d(t, torch.from_numpy(np.array(w)).to(dtype), torch.from_numpy(np.array(b)).to(dtype), stride=1, padding=w.shape[-1] // 2)
    if relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def pool_ref(y):
    """nn.MaxPool2d(2, 2) on a channel-last NumPy map (floors: an odd last row / column is dropped)"""
    t = torch.from_numpy(np.array(y)).permute(0, 3, 1, 2)        # a copy: the shared cases are read-only arrays
    if t.shape[2] < 2 or t.shape[3] < 2:
        return np.zeros((y.shape[0], y.shape[1] // 2, y.shape[2] // 2, y.shape[3]), y.dtype)
    return F.max_pool2d(t, 2, 2).permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def layer_case(family, cin, cout, B, H, W):
    """(x, w, b, ref32, ref64) of one unit case before pooling, computed once and shared (read-only) by every test that needs it"""
    x, w, b = layer_inputs(family, cin, cout, B, H, W)
    out = (x, w, b, conv_ref(x, w, b, torch.float32), conv_ref(x, w, b, torch.float64))
    for a in out:
        a.setflags(write=False)
    return out


def conv1a_inputs(family, B, H, W):
    rs = np.random.RandomState(5 + 7 * H + 13 * W + B)
    if family == "normal":
        img, w, b = rs.rand(B, 1, H, W), rs.standard_normal((64, 1, 3, 3)) * np.sqrt(2.0 / 9), rs.standard_normal(64) * 0.05
    else:
        img, w, b = rs.randint(-3, 4, (B, 1, H, W)), rs.randint(-2, 3, (64, 1, 3, 3)), rs.randint(-4, 5, 64)
    return img.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def conv1a_ref(img, w, b, dtype):
    y = F.relu(F.conv2d(torch.from_numpy(img).to(dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype), padding=1))
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# ---- the whole chain -------------------------------------------------------------------------------------------------------------

def chain_ref(image, sd, dtype):
    """models/superpoint.py:148-160, 188-189 restated: image [B,1,H,W] NumPy, sd = state_dict of NumPy arrays ->
    dict(feat [B,Hc,Wc,128] channel-last, score_logits [B,65,Hc,Wc], desc_raw [B,256,Hc,Wc]) as NumPy of `dtype`."""
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    conv = lambda x, n: F.conv2d(x, p[n + ".weight"], p[n + ".bias"], stride=1, padding=p[n + ".weight"].shape[-1] // 2)
    x = torch.from_numpy(image).to(dtype)
    for n in CHAIN:
        x = F.relu(conv(x, n))
        if n in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    score = conv(F.relu(conv(x, "convPa")), "convPb")
    desc = conv(F.relu(conv(x, "convDa")), "convDb")
    return {"feat": x.permute(0, 2, 3, 1).contiguous().numpy(), "score_logits": score.numpy(), "desc_raw": desc.numpy()}


def heads_ref(score_logits, desc_raw, dtype):
    """models/superpoint.py:161-167, 190-193 restated: (dense_score [B,8Hc,8Wc], dense_descriptor [B,256,Hc,Wc]) as NumPy of `dtype`"""
    s = torch.softmax(torch.from_numpy(np.asarray(score_logits)).to(dtype), 1)[:, :-1]
    B, _, Hc, Wc = s.shape
    s = s.permute(0, 2, 3, 1).reshape(B, Hc, Wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, Hc * 8, Wc * 8)
    d = F.normalize(torch.from_numpy(np.asarray(desc_raw)).to(dtype), p=2, dim=1)
    return s.numpy(), d.numpy()


@functools.lru_cache(maxsize=None)
def chain_case(H, W, B=2, seed=0):
    """(image, state_dict, ref32, ref64) of a seeded image of H x W with seed-0 weights; computed once, read-only"""
    rs = np.random.RandomState(4242 + H * 1000 + W + seed)
    image = rs.rand(B, 1, H, W).astype(np.float32)
    sd = synth.superpoint_state_dict(0)
    return image, sd, chain_ref(image, sd, torch.float32), chain_ref(image, sd, torch.float64)


# ---- NumPy model of the weight packing -------------------------------------------------------------------------------------------

def pack_index(n, c, tap, taps, cout_packed):
    """float offset of w[n][c][tap] in the packed weight (include/linetr_hip.h): [(chunk, tap, 8-channel group)][n][8]"""
    return ((((c // CK) * taps + tap) * 4 + (c % CK) // 8) * cout_packed + n) * 8 + c % 8


def pack_model(w):
    """w [cout,cin,k,k] -> the packed float vector"""
    cout, cin, k, _ = w.shape
    n, c, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(k * k), indexing="ij")
    out = np.full(cout * cin * k * k, np.nan, w.dtype)
    out[pack_index(n, c, tap, k * k, cout).ravel()] = w.reshape(cout, cin, k * k).ravel()
    return out


def unpack_model(packed, cout, cin, k):
    n, c, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(k * k), indexing="ij")
    return packed[pack_index(n, c, tap, k * k, cout)].reshape(cout, cin, k, k)
