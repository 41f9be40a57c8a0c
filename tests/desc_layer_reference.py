"""The line descriptive layer (LineDescriptiveEncoder of the reference, models/line_transformer.py:75-91 = MultiHeadAttention + FeedForward,
models/line_attention.py:23-94) and the three kernel pairs its native backward adds (csrc/lt_descbwd.h), stated from the formulas: float64
closed forms in NumPy (the references of tests/test_gpu_desc_layer.py), a torch statement of the reference's UNFOLDED module (all S query
rows; what autograd differentiates: its float32 error is the bar), the folded graph in stock torch, the seeded cases, the bar and the
launch helpers the tests and tools/desc_layer_report.py share.  Imports nothing of the package.  Test infrastructure only.

    pooling    s = u_h . x_t   p = softmax_t s   pooled_h = sum_t p_t x_t   lse_h = log sum_t exp s_t
               delta_h = dpooled_h . pooled_h   ds = p (dpooled_h . x_t - delta_h)   dx_t = sum_h (p dpooled_h + ds u_h)   du_h = sum_t ds x_t
    LayerNorm  v = a + r   xhat = (v - mean) rstd   y = xhat gamma + beta   gg = g gamma
               dx = rstd (gg - mean_c gg - xhat mean_c (gg xhat))   dgamma = sum_r g xhat   dbeta = sum_r g
    GELU       y = z Phi(z)   dz = g (Phi(z) + z phi(z))

The bar of a tensor, in the project's form:  max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|); ref32 = float32
autograd on the CPU, so the bar is a property of the references alone.  The elementwise GELU has one bar per magnitude family."""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

FACTOR = 8
D, HEADS, DH = 256, 4, 64
SENTINEL = 1.0e4          # magnitude of everything a kernel must not read into a result (finite: a leak shows as a huge error, not NaN)
MARKER = -777.25          # what an output buffer holds before the launch
SPARE_ROWS = 8            # sentinel rows behind the last row of an input
EPS = 1e-6


def bar_of(ref32, ref64):
    return FACTOR * max(np.abs(np.asarray(ref32, np.float64) - ref64).max(), 2.0 ** -23 * np.abs(ref64).max())


def ratios(got, ref64, ref32, keys=None):
    """[(tensor, max |got - ref64|, bar)] over `keys` (default: every float64 tensor of ref64; `got` must carry every one of them)"""
    rows = []
    for key in (keys if keys is not None else [k for k, v in ref64.items() if v.dtype == np.float64]):
        g = np.asarray(got[key], dtype=np.float64)
        assert g.shape == ref64[key].shape, (key, g.shape, ref64[key].shape)
        rows.append((key, np.abs(g - ref64[key]).max(), bar_of(ref32[key], ref64[key])))
    return rows


def failures(rows):
    return [f"{key}: error {e:.3e} > bar {b:.3e} (x{e / b if b else float('inf'):.2f})" for key, e, b in rows if not e <= b]


def worst(rows):
    return max((e / b if b else (0.0 if e == 0 else float("inf")) for _, e, b in rows), default=0.0)


def _rs(*key):
    """a RandomState seeded by the key's text (stable from process to process, unlike hash())"""
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def _sentinels(rs, shape):
    return (SENTINEL * (rs.randint(0, 2, shape) * 2 - 1)).astype(np.float32)


def _np64(t):
    return t.detach().double().cpu().numpy()


# ---- CLS token pooling -------------------------------------------------------------------------------------------------------------

POOL_OUTPUTS = ("pooled", "lse", "dx", "du")
POOL_FAMILIES = ("normal", "peaky", "sentinel")
POOL_S = (1, 2, 3, 21, 22, 23, 42, 63, 64, 65, 255, 256)
POOL_SEGS_PER_BLOCK = 4                        # CP_SEGS of csrc/lt_descbwd.h: one wave per segment, four waves per block
POOL_L = (1, 2, 3, 4, 5, 11)                   # 1, 2; a block's four segments -1 / 0 / +1; three blocks, the last one ragged


def pool_closed_form(x, u, dpooled, mistake=None):
    """float64.  x [L, S, 256], u, dpooled [L, 4, 256] -> dict pooled [L, 4, 256], lse [L, 4], dx [L, S, 256], du [L, 4, 256].
    mistake 'no_delta': the backward without its delta term (a planted error for the CPU suite)"""
    x, u, dpooled = (np.asarray(a, np.float64) for a in (x, u, dpooled))
    s = np.einsum("lhc,ltc->lht", u, x)
    m = s.max(axis=2, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(axis=2, keepdims=True))
    p = np.exp(s - lse)
    pooled = np.einsum("lht,ltc->lhc", p, x)
    delta = np.einsum("lhc,lhc->lh", dpooled, pooled)[:, :, None]
    if mistake == "no_delta":
        delta = 0.0
    ds = p * (np.einsum("lhc,ltc->lht", dpooled, x) - delta)
    return {"pooled": pooled, "lse": lse[:, :, 0], "dx": np.einsum("lht,lhc->ltc", p, dpooled) + np.einsum("lht,lhc->ltc", ds, u),
            "du": np.einsum("lht,ltc->lhc", ds, x)}


def pool_torch(x, u, dpooled, dtype):
    """autograd through the same pooling in torch on the CPU at `dtype`: dict of float64 arrays like pool_closed_form"""
    xt, ut = (torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (x, u))
    with torch.enable_grad():
        s = torch.einsum("lhc,ltc->lht", ut, xt)
        pooled = torch.einsum("lht,ltc->lhc", torch.softmax(s, dim=2), xt)
        pooled.backward(torch.tensor(np.asarray(dpooled), dtype=dtype))
    return {"pooled": _np64(pooled), "lse": _np64(torch.logsumexp(s, dim=2)), "dx": _np64(xt.grad), "du": _np64(ut.grad)}


@functools.lru_cache(maxsize=None)
def pool_case(family, L, S, seed=0):
    """x [L, S, 256], u, dpooled [L, 4, 256] float32 with ref64 (the closed form) and ref32 (float32 autograd) over the segments in
    `check`.  'normal': unit-normal tokens, scores of unit scale.  'peaky': u_h = +-40 x_t / |x_t|^2 for one token t of the segment, so
    that token's score is +40 (it carries the mass) or -40 (it carries none).  'sentinel': every odd segment holds +-1e4 in x, u and
    dpooled; the even ones are the compared ones.  The arrays are shared: do not write to them."""
    rs = _rs("pool", family, L, S, seed)
    x = rs.standard_normal((L, S, D)).astype(np.float32)
    u = (rs.standard_normal((L, HEADS, D)) / 16.0).astype(np.float32)
    dpooled = rs.standard_normal((L, HEADS, D)).astype(np.float32)
    check = list(range(L))
    if family == "peaky":
        for l in range(L):
            for h in range(HEADS):
                t = rs.randint(S)
                sign = 1.0 if (l + h) % 2 == 0 else -1.0
                u[l, h] = (sign * 40.0 * x[l, t].astype(np.float64) / np.square(x[l, t].astype(np.float64)).sum()).astype(np.float32)
    elif family == "sentinel":
        check = list(range(0, L, 2))
        for l in range(1, L, 2):
            x[l], u[l], dpooled[l] = _sentinels(rs, (S, D)), _sentinels(rs, (HEADS, D)), _sentinels(rs, (HEADS, D))
    else:
        assert family == "normal", family
    r64, r32 = pool_closed_form(x[check], u[check], dpooled[check]), pool_torch(x[check], u[check], dpooled[check], torch.float32)
    return dict(family=family, L=L, S=S, x=x, u=u, dpooled=dpooled, check=check, ref64=r64, ref32=r32)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------

LN_OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
LN_FAMILIES = ("normal", "offset", "constant")


def ln_closed_form(a, r, gamma, beta, g, eps=EPS, mistake=None):
    """float64.  a, r (or None), g [rows, 256]; gamma, beta [256].  mistake 'no_xhat': dx without its xhat term (a planted error)"""
    a, gamma, beta, g = (np.asarray(t, np.float64) for t in (a, gamma, beta, g))
    v = a if r is None else a + np.asarray(r, np.float64)
    mean = v.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(np.square(v - mean).mean(axis=1, keepdims=True) + eps)
    xhat = (v - mean) * rstd
    gg = g * gamma
    c2 = 0.0 if mistake == "no_xhat" else (gg * xhat).mean(axis=1, keepdims=True)
    return {"y": xhat * gamma + beta, "mean": mean[:, 0], "rstd": rstd[:, 0], "dx": rstd * (gg - gg.mean(axis=1, keepdims=True) - xhat * c2),
            "dgamma": (g * xhat).sum(axis=0), "dbeta": g.sum(axis=0)}


def ln_torch(a, r, gamma, beta, g, dtype, eps=EPS):
    """autograd through F.layer_norm(a + r) on the CPU at `dtype`"""
    at, gt, bt = (torch.tensor(np.asarray(t), dtype=dtype, requires_grad=True) for t in (a, gamma, beta))
    with torch.enable_grad():
        v = at if r is None else at + torch.tensor(np.asarray(r), dtype=dtype)
        y = F.layer_norm(v, (D,), gt, bt, eps)
        y.backward(torch.tensor(np.asarray(g), dtype=dtype))
    vd = v.detach()
    mean = vd.mean(dim=1)
    rstd = 1.0 / torch.sqrt((vd - mean[:, None]).square().mean(dim=1) + eps)
    return {"y": _np64(y), "mean": _np64(mean), "rstd": _np64(rstd), "dx": _np64(at.grad), "dgamma": _np64(gt.grad), "dbeta": _np64(bt.grad)}


@functools.lru_cache(maxsize=None)
def ln_case(family, rows, residual, seed=0, integer_g=False, zero_gamma=False):
    """a, r (None without `residual`), g [rows, 256], gamma, beta [256] float32 with ref64 / ref32.  'normal': unit normal.  'offset':
    every row of a + r has |mean| / std = 4096.  'constant': every row of a + r is one value (variance 0)."""
    rs = _rs("ln", family, rows, residual, seed, integer_g, zero_gamma)
    a = rs.standard_normal((rows, D)).astype(np.float32)
    r = rs.standard_normal((rows, D)).astype(np.float32) if residual else None
    if family == "offset":
        a = (a + 4096.0 * (1.0 + residual) ** 0.5 * np.where(rs.randint(0, 2, (rows, 1)) > 0, 1.0, -1.0)).astype(np.float32)
    elif family == "constant":
        a = np.repeat(rs.uniform(-3, 3, (rows, 1)), D, axis=1).astype(np.float32)
        r = np.repeat(rs.randint(-4, 5, (rows, 1)), D, axis=1).astype(np.float32) if residual else None
    else:
        assert family == "normal", family
    gamma = np.zeros(D, np.float32) if zero_gamma else rs.uniform(0.5, 1.5, D).astype(np.float32)
    beta = (0.3 * rs.standard_normal(D)).astype(np.float32)
    g = rs.randint(-4, 5, (rows, D)).astype(np.float32) if integer_g else rs.standard_normal((rows, D)).astype(np.float32)
    return dict(family=family, rows=rows, a=a, r=r, gamma=gamma, beta=beta, g=g, ref64=ln_closed_form(a, r, gamma, beta, g),
                ref32=ln_torch(a, r, gamma, beta, g, torch.float32))


# ---- GELU --------------------------------------------------------------------------------------------------------------------------

GELU_FAMILIES = ("small", "unit", "large")            # |z| < 1e-3, about 1, 4 .. 12: one bar each
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def gelu_closed_form(z, g, mistake=None):
    """float64, erf form.  mistake 'tanh': the tanh approximation (a planted error)"""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    if mistake == "tanh":
        k = math.sqrt(2.0 / math.pi)
        t = np.tanh(k * (z + 0.044715 * z ** 3))
        return {"y": 0.5 * z * (1 + t), "dz": g * (0.5 * (1 + t) + 0.5 * z * (1 - t * t) * k * (1 + 3 * 0.044715 * z * z))}
    cdf = 0.5 * _erfc(-z / math.sqrt(2.0))
    return {"y": z * cdf, "dz": g * (cdf + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))}


def gelu_torch(z, g, dtype):
    zt = torch.tensor(np.asarray(z), dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        y = F.gelu(zt)
        y.backward(torch.tensor(np.asarray(g), dtype=dtype))
    return {"y": _np64(y), "dz": _np64(zt.grad)}


@functools.lru_cache(maxsize=None)
def gelu_case(family, rows=5, C=1024, seed=0):
    rs = _rs("gelu", family, rows, C, seed)
    if family == "small":
        z = rs.uniform(-1e-3, 1e-3, (rows, C))
    elif family == "unit":
        z = rs.standard_normal((rows, C))
    else:
        assert family == "large", family
        z = rs.uniform(4.0, 12.0, (rows, C)) * np.where(rs.randint(0, 2, (rows, C)) > 0, 1.0, -1.0)
    z, g = z.astype(np.float32), rs.standard_normal((rows, C)).astype(np.float32)
    return dict(family=family, z=z, g=g, ref64=gelu_closed_form(z, g), ref32=gelu_torch(z, g, torch.float32))


# ---- the module --------------------------------------------------------------------------------------------------------------------

SHAPES = {"slf_attn.w_qs.weight": (D, D), "slf_attn.w_qs.bias": (D,), "slf_attn.w_ks.weight": (D, D), "slf_attn.w_ks.bias": (D,),
          "slf_attn.w_vs.weight": (D, D), "slf_attn.w_vs.bias": (D,), "slf_attn.fc.weight": (D, D), "slf_attn.fc.bias": (D,),
          "slf_attn.layer_norm.weight": (D,), "slf_attn.layer_norm.bias": (D,), "pos_ffn.w_1.weight": (1024, D), "pos_ffn.w_1.bias": (1024,),
          "pos_ffn.w_2.weight": (D, 1024), "pos_ffn.w_2.bias": (D,), "pos_ffn.layer_norm.weight": (D,), "pos_ffn.layer_norm.bias": (D,)}
MATRICES = tuple(k for k, s in SHAPES.items() if len(s) == 2)
VECTORS = tuple(k for k, s in SHAPES.items() if len(s) == 1)
FIXTURE_SHAPE, FIXTURE_SEED = (2, 5, 22), 41
MODULE_SHAPES = ((1, 1, 1), (3, 129, 42))        # (B, L, S) against the restatement: one token in all; several blocks of every kernel
TAIL_SHAPE = (2, 33, 22)


def state_dict(rs, scale=1.0):
    """the layer's state dict drawn from `rs` in SHAPES' order: weights N(0, scale^2 / K), biases in (-0.5, 0.5), the LayerNorm weights
    in (0.5, 1.5) and biases N(0, 0.3^2) -- away from 1 and 0"""
    sd = {}
    for key, shape in SHAPES.items():
        if "layer_norm" in key:
            sd[key] = (rs.uniform(0.5, 1.5, shape) if key.endswith("weight") else 0.3 * rs.standard_normal(shape)).astype(np.float32)
        elif len(shape) == 2:
            sd[key] = (scale * rs.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        else:
            sd[key] = rs.uniform(-0.5, 0.5, shape).astype(np.float32)
    return sd


def tensors(sd, dtype=None):
    return {key: torch.from_numpy(np.array(val)).to(dtype) if dtype is not None else torch.from_numpy(np.array(val)) for key, val in sd.items()}


class _Attention(nn.Module):
    """MultiHeadAttention of models/line_attention.py:23-75 with p = 0 on its dropouts: all S query rows"""

    def __init__(self):
        super().__init__()
        self.w_qs, self.w_ks, self.w_vs, self.fc = (nn.Linear(D, D) for _ in range(4))
        self.layer_norm = nn.LayerNorm(D, eps=EPS)

    def forward(self, x, mask=None, drop_scale=False):
        B, L, S, _ = x.shape
        q, k, v = (w(x).view(B, L, S, HEADS, DH).transpose(2, 3) for w in (self.w_qs, self.w_ks, self.w_vs))
        attn = torch.matmul(q if drop_scale else q / 8.0, k.transpose(3, 4))
        if mask is not None:
            attn = attn.masked_fill(mask.unsqueeze(2) == 0, -1e9)
        o = torch.matmul(torch.softmax(attn, dim=-1), v).transpose(2, 3).contiguous().view(B, L, S, D)
        return self.layer_norm(self.fc(o) + x)


class _FeedForward(nn.Module):
    def __init__(self):
        super().__init__()
        self.w_1, self.w_2 = nn.Linear(D, 1024), nn.Linear(1024, D)
        self.layer_norm = nn.LayerNorm(D, eps=EPS)

    def forward(self, x):
        return self.layer_norm(self.w_2(F.gelu(self.w_1(x))) + x)


class Layer(nn.Module):
    """LineDescriptiveEncoder of models/line_transformer.py:75-91, unfolded, with the reference's state_dict names"""

    def __init__(self):
        super().__init__()
        self.slf_attn, self.pos_ffn = _Attention(), _FeedForward()

    def forward(self, desc, mask=None):
        return self.pos_ffn(self.slf_attn(desc, mask))


def folded_forward(p, desc, mistake=None):
    """The FOLDED graph in stock torch (what linetr_amd.train_ops.LineDescriptiveEncoder composes of native kernels): p = dict of
    parameter tensors, desc [B, L, S, 256] -> cls_out [B, L, 256].  mistake 'no_scale': the 1/8 dropped (a planted error)"""
    B, L, S, _ = desc.shape
    x = desc.reshape(B * L, S, D)
    x0 = x[:, 0]
    q = x0 @ p["slf_attn.w_qs.weight"].T + p["slf_attn.w_qs.bias"]
    if mistake != "no_scale":
        q = q * 0.125
    u = torch.einsum("lhd,hdc->lhc", q.view(-1, HEADS, DH), p["slf_attn.w_ks.weight"].view(HEADS, DH, D))
    pooled = torch.einsum("lht,ltc->lhc", torch.softmax(torch.einsum("lhc,ltc->lht", u, x), dim=2), x)
    o = torch.einsum("lhc,hdc->lhd", pooled, p["slf_attn.w_vs.weight"].view(HEADS, DH, D)).reshape(-1, D) + p["slf_attn.w_vs.bias"]
    y = F.layer_norm(o @ p["slf_attn.fc.weight"].T + p["slf_attn.fc.bias"] + x0, (D,), p["slf_attn.layer_norm.weight"],
                     p["slf_attn.layer_norm.bias"], EPS)
    hidden = F.gelu(y @ p["pos_ffn.w_1.weight"].T + p["pos_ffn.w_1.bias"])
    out = F.layer_norm(hidden @ p["pos_ffn.w_2.weight"].T + p["pos_ffn.w_2.bias"] + y, (D,), p["pos_ffn.layer_norm.weight"],
                       p["pos_ffn.layer_norm.bias"], EPS)
    return out.view(B, L, D)


def run_layer(sd, desc, upstream, dtype, train=True, device="cpu", folded=False, mistake=None):
    """The layer differentiated by torch at `dtype`, the upstream arriving at row 0 of its output: dict out [B, L, 256], d_desc
    [B, L, S, 256] and the parameter gradients under their state_dict names, float64 arrays.  `folded`: through folded_forward (the key
    bias, which it never reads, gets a zero gradient)"""
    mod = Layer().to(dtype)
    mod.load_state_dict(tensors(sd, dtype), strict=True)
    mod = mod.to(device).train(train)
    xt = torch.tensor(desc, dtype=dtype, device=device, requires_grad=True)
    with torch.enable_grad():
        out = folded_forward(dict(mod.named_parameters()), xt, mistake) if folded else mod(xt)[:, :, 0]
        out.backward(torch.tensor(upstream, dtype=dtype, device=device))
    res = {"out": _np64(out), "d_desc": _np64(xt.grad)}
    for key, prm in mod.named_parameters():
        res[key] = _np64(prm.grad) if prm.grad is not None else np.zeros(tuple(prm.shape))
    return res


@functools.lru_cache(maxsize=None)
def module_case(B, L, S, seed=FIXTURE_SEED, scale=1.0):
    """(state dict, desc [B, L, S, 256], upstream [B, L, 256]): seeded; FIXTURE_SHAPE with FIXTURE_SEED is what
    tests/golden/make_golden_desc_layer.py draws"""
    rs = np.random.RandomState(seed)
    sd = state_dict(rs, scale)
    desc = rs.standard_normal((B, L, S, D)).astype(np.float32)
    upstream = rs.standard_normal((B, L, D)).astype(np.float32)
    return sd, desc, upstream


@functools.lru_cache(maxsize=None)
def module_refs(B, L, S, train=True, seed=FIXTURE_SEED, scale=1.0):
    sd, desc, g = module_case(B, L, S, seed, scale)
    return run_layer(sd, desc, g, torch.float64, train), run_layer(sd, desc, g, torch.float32, train)


# ---- the layer under the signature network and the head ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tail_case(seed=FIXTURE_SEED + 2):
    """descriptive layer -> klines_pos + cls_out^T -> a two-layer signature network -> final_proj + normalize -> a seeded upstream, at
    TAIL_SHAPE: (layer state dict, stack state dict, head weight, head bias, desc, klines_pos [B, 256, L], upstream [B, 256, L])"""
    import sig_layer_reference as SL
    B, L, S = TAIL_SHAPE
    rs = np.random.RandomState(seed)
    sd = state_dict(rs)
    stack = SL.stack_state_dict(rs, 2)
    W = (rs.standard_normal((D, D, 1)) / 16).astype(np.float32)
    b = rs.uniform(-0.05, 0.05, D).astype(np.float32)
    desc = rs.standard_normal((B, L, S, D)).astype(np.float32)
    pos = rs.standard_normal((B, D, L)).astype(np.float32)
    upstream = rs.standard_normal((B, D, L)).astype(np.float32)
    return sd, stack, W, b, desc, pos, upstream


def run_tail(dtype, device="cpu"):
    """the composition differentiated by torch at `dtype`: dict line_desc, d_desc, d_pos, desc.<name>, stack.<name>, final_proj.<name>"""
    import sig_layer_reference as SL
    sd, stack_sd, W, b, desc, pos, upstream = tail_case()
    layer, stack, head = Layer().to(dtype), SL.Stack(2).to(dtype), nn.Conv1d(D, D, 1).to(dtype)
    layer.load_state_dict(tensors(sd, dtype), strict=True)
    stack.load_state_dict(SL.tensors(stack_sd, dtype), strict=True)
    head.load_state_dict(tensors({"weight": W, "bias": b}, dtype))
    layer, stack, head = layer.to(device).train(), stack.to(device).train(), head.to(device)
    xt, pt = (torch.tensor(a, dtype=dtype, device=device, requires_grad=True) for a in (desc, pos))
    with torch.enable_grad():
        line_desc = F.normalize(head(stack(pt + layer(xt)[:, :, 0].transpose(1, 2))), p=2, dim=1)
        line_desc.backward(torch.tensor(upstream, dtype=dtype, device=device))
    res = {"line_desc": _np64(line_desc), "d_desc": _np64(xt.grad), "d_pos": _np64(pt.grad)}
    for prefix, mod in (("desc.", layer), ("stack.", stack), ("final_proj.", head)):
        for key, prm in mod.named_parameters():
            res[prefix + key] = _np64(prm.grad)
    return res


@functools.lru_cache(maxsize=None)
def tail_refs():
    return run_tail(torch.float64), run_tail(torch.float32)


# ---- launching (GPU) ---------------------------------------------------------------------------------------------------------------

def _stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inp(rows, ld, rs, device):
    """[n + SPARE_ROWS, ld] of sentinels around the rows [n, width]"""
    rows = np.asarray(rows, np.float32)
    buf = _sentinels(rs, (rows.shape[0] + SPARE_ROWS, ld))
    buf[:rows.shape[0], :rows.shape[1]] = rows
    return torch.from_numpy(buf).to(device)


def _out(n, ld, device, wanted=True):
    return torch.full((n + 1, ld), MARKER, dtype=torch.float32, device=device) if wanted else None


def _take(t, n, width, what):
    """the [n, width] result of an output buffer whose marker row and padding columns must be untouched"""
    assert bool((t[n] == MARKER).all()), f"the row behind {what} was written"
    assert t.shape[1] == width or bool((t[:, width:] == MARKER).all()), f"the padding columns of {what} were written"
    return t[:n, :width].cpu().numpy()


_ptr = lambda t: t.data_ptr() if t is not None else None


def pool_launch(lib, c, ldx=256, ldu=1024, need=(True, True), saved=None, device="cuda:0"):
    """The raw pooling entry points on a pool_case: forward, then backward.  Sentinel rows sit behind every input (and in its padding
    columns), a marker row behind every output.  Returns a dict of CPU arrays pooled, lse, dx, du over ALL L segments (what `need`
    leaves out stays away).  `saved` = (pooled, lse) device tensors of an earlier launch to use instead of running the forward."""
    L, S = c["L"], c["S"]
    rs = _rs("pool launch", ldx, ldu)
    x = _inp(c["x"].reshape(L * S, D), ldx, rs, device)
    u = _inp(c["u"].reshape(L, HEADS * D), ldu, rs, device)
    dp = _inp(c["dpooled"].reshape(L, HEADS * D), HEADS * D, rs, device)
    pooled, lse = _out(L, HEADS * D, device), _out(L, HEADS, device)
    dx, du = _out(L * S, ldx, device, need[0]), _out(L, ldu, device, need[1])
    if saved is None:
        rc = lib.linetr_cls_pool_train_forward(None, x.data_ptr(), ldx, u.data_ptr(), ldu, L, S, pooled.data_ptr(), lse.data_ptr(), _stream())
        assert rc == 0, lib.linetr_last_error()
    else:
        pooled[:L], lse[:L] = saved
    rc = lib.linetr_cls_pool_train_backward(None, x.data_ptr(), ldx, u.data_ptr(), ldu, pooled.data_ptr(), lse.data_ptr(), dp.data_ptr(), L, S,
                                            _ptr(dx), ldx, _ptr(du), ldu, _stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    res = {"pooled": _take(pooled, L, HEADS * D, "pooled").reshape(L, HEADS, D), "lse": _take(lse, L, HEADS, "lse")}
    if dx is not None:
        res["dx"] = _take(dx, L * S, D, "dx").reshape(L, S, D)
    if du is not None:
        res["du"] = _take(du, L, HEADS * D, "du").reshape(L, HEADS, D)
    res["_dev"] = (pooled[:L].clone(), lse[:L].clone())
    return res


def ln_launch(lib, c, ld=256, need=(True, True, True), device="cuda:0"):
    """The raw LayerNorm entry points on an ln_case: forward, then backward; dict of CPU arrays y, mean, rstd, dx, dgamma, dbeta"""
    rows = c["rows"]
    rs = _rs("ln launch", ld)
    a, g = _inp(c["a"], ld, rs, device), _inp(c["g"], ld, rs, device)
    r = _inp(c["r"], ld, rs, device) if c["r"] is not None else None
    gamma, beta = (torch.from_numpy(c[k]).to(device) for k in ("gamma", "beta"))
    y, stats, dx = _out(rows, ld, device), _out(rows, 2, device), _out(rows, ld, device, need[0])
    dgamma, dbeta = (_out(1, D, device, n) for n in need[1:])
    rc = lib.linetr_layer_norm_forward(None, a.data_ptr(), ld, _ptr(r), ld, gamma.data_ptr(), beta.data_ptr(), EPS, rows, D, y.data_ptr(), ld,
                                       stats.data_ptr(), _stream())
    assert rc == 0, lib.linetr_last_error()
    ws = torch.empty(max(int(lib.linetr_layer_norm_backward_workspace_bytes(rows, D)), 16), dtype=torch.uint8, device=device)
    rc = lib.linetr_layer_norm_backward(None, a.data_ptr(), ld, _ptr(r), ld, stats.data_ptr(), gamma.data_ptr(), g.data_ptr(), ld, rows, D, _ptr(dx),
                                        ld, _ptr(dgamma), _ptr(dbeta), ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    st = _take(stats, rows, 2, "stats")
    res = {"y": _take(y, rows, D, "y"), "mean": st[:, 0], "rstd": st[:, 1]}
    for key, t, n in (("dx", dx, rows), ("dgamma", dgamma, 1), ("dbeta", dbeta, 1)):
        if t is not None:
            res[key] = _take(t, n, D, key) if key == "dx" else _take(t, n, D, key)[0]
    return res


def gelu_launch(lib, z, g, ld=None, device="cuda:0"):
    """The raw GELU entry points on z, g [rows, C]: dict of CPU arrays y, dz"""
    rows, C_ = z.shape
    ld = C_ if ld is None else ld
    rs = _rs("gelu launch", ld)
    zt, gt = _inp(z, ld, rs, device), _inp(g, ld, rs, device)
    y, dz = _out(rows, ld, device), _out(rows, ld, device)
    rc = lib.linetr_gelu_forward(None, zt.data_ptr(), ld, rows, C_, y.data_ptr(), ld, _stream())
    assert rc == 0, lib.linetr_last_error()
    rc = lib.linetr_gelu_backward(None, zt.data_ptr(), ld, gt.data_ptr(), ld, rows, C_, dz.data_ptr(), ld, _stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    return {"y": _take(y, rows, C_, "y"), "dz": _take(dz, rows, C_, "dz")}
