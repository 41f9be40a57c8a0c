"""Training-time dropout of the line descriptive layer (csrc/lt_dropout.h; the reference's nn.Dropout at models/line_attention.py:18, :70,
:90), stated from the formulas: Philox4x32-10 and the factor tables in NumPy (what the device generator must equal bit for bit), float64
closed forms of the masked pooling and the masked residual LayerNorm, the UNFOLDED layer in stock torch with explicit masks at the three
places (all S query rows; what tests/golden/desc_layer_dropout.npz pins to the reference's own module), the folded graph with masks, the
seeded cases and the launch helpers of tests/test_gpu_dropout.py and tools/dropout_report.py.  Imports nothing of the package; builds on
tests/desc_layer_reference.py without editing it.  Test infrastructure only.

    generator  key = (seed & 0xffffffff, seed >> 32)   counter = (inner, row, call, site)   a word w keeps iff w >= floor(p 2^32)
               factor r = float32(1 / (1 - p)) or 0;  site 0: row = segment, inner = token, word h = head h;  sites 1, 2: inner = column / 4
    pooling    a = p r   pooled_h = sum_t a_t x_t   kept_h = sum_t a_t   (then o_h = Wv_h pooled_h + kept_h bv_h)
               da_t = dpooled_h . x_t + dkept_h   delta_h = dpooled_h . pooled_h + dkept_h kept_h   ds = p (r da - delta)
               dx_t = sum_h (a dpooled_h + ds u_h)   du_h = sum_t ds x_t
    LayerNorm  v = r a + residual   y = LN(v)   dresidual = dv   da = r dv

The bar of a tensor is desc_layer_reference.bar_of: 8 max(|ref32 - ref64|, 2^-23 |ref64|), ref32 = float32 CPU autograd of the same case
with the same masks."""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import desc_layer_reference as DL

D, HEADS, DH, EPS = DL.D, DL.HEADS, DL.DH, DL.EPS
SEED, BIG_SEED = 2026, (0x9E3779B9 << 32) | 2026          # the fixture's seed; one whose upper key word is not zero
P_VALUES = (0.1, 0.5)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


# ---- the generator -----------------------------------------------------------------------------------------------------------------

def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcast together), key: two -> the four output words, uint32 arrays"""
    c = [np.asarray(v, np.uint64) for v in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(v)) for v in key]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """floor(p 2^32) in double: a word w is kept iff w >= threshold"""
    assert 0.0 <= p < 1.0
    return int(float(p) * 4294967296.0)


def scale(p):
    return np.float32(1.0 / (1.0 - float(p)))


def words(seed, call, site, rows, inner):
    """the words of a site: uint32 [rows, inner, 4]"""
    w = philox4x32_10((np.arange(inner, dtype=np.uint64)[None, :], np.arange(rows, dtype=np.uint64)[:, None], call, site),
                      (seed & 0xffffffff, seed >> 32))
    return np.stack(w, axis=2)


def factors(seed, call, site, rows, inner, p):
    """the factors of a site: float32 [rows, inner, 4], scale(p) or 0"""
    return np.where(words(seed, call, site, rows, inner) >= np.uint32(threshold(p)), scale(p), np.float32(0.0)).astype(np.float32)


def pool_factors(seed, call, L, S, p):
    """site 0 as the pooling reads it: r [L, 4, S] (segment, head, token)"""
    return np.ascontiguousarray(factors(seed, call, 0, L, S, p).transpose(0, 2, 1))


def row_factors(seed, call, site, rows, p):
    """sites 1 / 2 as the LayerNorm reads them: r [rows, 256]"""
    return factors(seed, call, site, rows, D // 4, p).reshape(rows, D)


# ---- masked CLS token pooling ------------------------------------------------------------------------------------------------------

POOL_OUTPUTS = ("pooled", "kept", "lse", "dx", "du")
POOL_FAMILIES = ("normal", "peaky")
POOL_S = (1, 2, 3, 4, 5, 7, 8, 9, 22, 23)          # the chunk edges of CP_TOK = 4 and CP_TOK_B = 2
POOL_L = (1, 3, 4, 5, 9)                           # the edges of CP_SEGS = 4


def pool_closed_form(x, u, dpooled, dkept, r, mistake=None):
    """float64.  x [L, S, 256], u, dpooled [L, 4, 256], dkept [L, 4], r [L, 4, S] -> dict of POOL_OUTPUTS.  mistake 'delta_without_kept':
    delta without its dkept kept term (a planted error)"""
    x, u, dpooled, dkept, r = (np.asarray(a, np.float64) for a in (x, u, dpooled, dkept, r))
    s = np.einsum("lhc,ltc->lht", u, x)
    m = s.max(axis=2, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(axis=2, keepdims=True))
    p = np.exp(s - lse)
    a = p * r
    pooled, kept = np.einsum("lht,ltc->lhc", a, x), a.sum(axis=2)
    delta = np.einsum("lhc,lhc->lh", dpooled, pooled) + (0.0 if mistake == "delta_without_kept" else dkept * kept)
    da = np.einsum("lhc,ltc->lht", dpooled, x) + dkept[:, :, None]
    ds = p * (r * da - delta[:, :, None])
    return {"pooled": pooled, "kept": kept, "lse": lse[:, :, 0], "dx": np.einsum("lht,lhc->ltc", a, dpooled) + np.einsum("lht,lhc->ltc", ds, u),
            "du": np.einsum("lht,ltc->lhc", ds, x)}


def pool_torch(x, u, dpooled, dkept, r, dtype):
    """autograd through the same masked pooling in torch on the CPU at `dtype`"""
    xt, ut = (torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (x, u))
    with torch.enable_grad():
        s = torch.einsum("lhc,ltc->lht", ut, xt)
        a = torch.softmax(s, dim=2) * torch.tensor(np.asarray(r), dtype=dtype)
        pooled, kept = torch.einsum("lht,ltc->lhc", a, xt), a.sum(dim=2)
        torch.autograd.backward([pooled, kept], [torch.tensor(np.asarray(dpooled), dtype=dtype), torch.tensor(np.asarray(dkept), dtype=dtype)])
    return {"pooled": DL._np64(pooled), "kept": DL._np64(kept), "lse": DL._np64(torch.logsumexp(s, dim=2)), "dx": DL._np64(xt.grad),
            "du": DL._np64(ut.grad)}


@functools.lru_cache(maxsize=None)
def pool_case(family, L, S, p, seed=SEED, call=0):
    """desc_layer_reference.pool_case(family, L, S) with a seeded dkept [L, 4] and the factors r [L, 4, S] of (seed, call, p); ref64 the
    closed form, ref32 float32 autograd.  The arrays are shared: do not write to them."""
    base = DL.pool_case(family, L, S)
    dkept = DL._rs("dropout dkept", family, L, S).standard_normal((L, HEADS)).astype(np.float32)
    r = pool_factors(seed, call, L, S, p)
    args = (base["x"], base["u"], base["dpooled"], dkept, r)
    return dict(family=family, L=L, S=S, p=p, seed=seed, call=call, x=base["x"], u=base["u"], dpooled=base["dpooled"], dkept=dkept, r=r,
                ref64=pool_closed_form(*args), ref32=pool_torch(*args, torch.float32))


def all_dropped(seed, call, L, S, p):
    """the (segment, head) pairs all of whose S tokens are dropped: bool [L, 4]"""
    return ~pool_factors(seed, call, L, S, p).any(axis=2)


# ---- masked residual LayerNorm -----------------------------------------------------------------------------------------------------

LN_OUTPUTS = ("y", "mean", "rstd", "da", "dr", "dgamma", "dbeta")
LN_ROWS = (1, 3, 4, 5, 31, 32, 33, 65)             # the edges of LN_ROWS = 4 and LN_CHUNK = 32


def ln_closed_form(a, r, gamma, beta, g, fac, eps=EPS, mistake=None):
    """float64: desc_layer_reference.ln_closed_form on fac a (+ r); dr = its dx, da = fac dx.  Without a residual there is no dr.
    mistake 'dr_scaled': the residual's gradient scaled by the factors too (a planted error)"""
    fac = np.asarray(fac, np.float64)
    base = DL.ln_closed_form(np.asarray(a, np.float64) * fac, r, gamma, beta, g, eps)
    dv = base.pop("dx")
    base["da"] = fac * dv
    if r is not None:
        base["dr"] = fac * dv if mistake == "dr_scaled" else dv
    return base


def ln_torch(a, r, gamma, beta, g, fac, dtype, eps=EPS):
    at, gt, bt = (torch.tensor(np.asarray(t), dtype=dtype, requires_grad=True) for t in (a, gamma, beta))
    rt = torch.tensor(np.asarray(r), dtype=dtype, requires_grad=True) if r is not None else None
    with torch.enable_grad():
        v = at * torch.tensor(np.asarray(fac), dtype=dtype)
        v = v + rt if rt is not None else v
        y = F.layer_norm(v, (D,), gt, bt, eps)
        y.backward(torch.tensor(np.asarray(g), dtype=dtype))
    vd = v.detach()
    mean = vd.mean(dim=1)
    rstd = 1.0 / torch.sqrt((vd - mean[:, None]).square().mean(dim=1) + eps)
    out = {"y": DL._np64(y), "mean": DL._np64(mean), "rstd": DL._np64(rstd), "da": DL._np64(at.grad), "dgamma": DL._np64(gt.grad),
           "dbeta": DL._np64(bt.grad)}
    if rt is not None:
        out["dr"] = DL._np64(rt.grad)
    return out


@functools.lru_cache(maxsize=None)
def ln_case(rows, residual, site, p, seed=SEED, call=3):
    base = DL.ln_case("normal", rows, residual)
    fac = row_factors(seed, call, site, rows, p)
    args = (base["a"], base["r"], base["gamma"], base["beta"], base["g"], fac)
    return dict(rows=rows, site=site, p=p, seed=seed, call=call, a=base["a"], r=base["r"], gamma=base["gamma"], beta=base["beta"], g=base["g"],
                fac=fac, ref64=ln_closed_form(*args), ref32=ln_torch(*args, torch.float32))


# ---- the module --------------------------------------------------------------------------------------------------------------------

MODULE_SHAPES = ((1, 1, 1), (2, 5, 22), (3, 129, 42))
OTHER_ROWS_SEED = 7


def masks(B, L, S, seed, call, p, other=OTHER_ROWS_SEED):
    """The three masks of the UNFOLDED layer, float32: attention [B, L, 4, S, S], behind fc and behind w_2 [B, L, S, 256].  Query row 0 of
    each comes from the factor tables (row = b L + l, the module's segment index); rows 1 .. S-1, which never reach row 0 of the output,
    from a second seeded draw (`other`) with the same probability."""
    rs = np.random.RandomState(other)
    draw = lambda shape: np.where(rs.uniform(size=shape) >= p, scale(p), np.float32(0.0)).astype(np.float32)
    attn, m1, m2 = draw((B, L, HEADS, S, S)), draw((B, L, S, D)), draw((B, L, S, D))
    attn[:, :, :, 0, :] = pool_factors(seed, call, B * L, S, p).reshape(B, L, HEADS, S)
    m1[:, :, 0], m2[:, :, 0] = (row_factors(seed, call, site, B * L, p).reshape(B, L, D) for site in (1, 2))
    return attn, m1, m2


class Mask(nn.Module):
    """what stands in the place of an nn.Dropout: the product with a fixed mask"""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


class MaskedLayer(DL.Layer):
    """desc_layer_reference.Layer (the unfolded LineDescriptiveEncoder, same state_dict) with a fixed mask at each of the reference's three
    dropouts: on softmax(attn), behind fc, behind w_2"""

    def set_masks(self, *masks_of_calls):
        """one (attn, m1, m2) per forward to come, used in turn (the last one again and again)"""
        self.calls, self.i = list(masks_of_calls) if isinstance(masks_of_calls[0], (tuple, list)) else [masks_of_calls], 0
        return self

    def forward(self, desc, mask=None):
        self.m = self.calls[min(self.i, len(self.calls) - 1)]
        self.i += 1
        att, ffn = self.slf_attn, self.pos_ffn
        B, L, S, _ = desc.shape
        q, k, v = (w(desc).view(B, L, S, HEADS, DH).transpose(2, 3) for w in (att.w_qs, att.w_ks, att.w_vs))
        attn = torch.matmul(q / 8.0, k.transpose(3, 4))
        if mask is not None:
            attn = attn.masked_fill(mask.unsqueeze(2) == 0, -1e9)
        o = torch.matmul(torch.softmax(attn, dim=-1) * self.m[0], v).transpose(2, 3).contiguous().view(B, L, S, D)
        y = att.layer_norm(att.fc(o) * self.m[1] + desc)
        return ffn.layer_norm(ffn.w_2(F.gelu(ffn.w_1(y))) * self.m[2] + y)


def folded_forward(p, desc, r0, r1, r2, mistake=None):
    """The FOLDED graph with masks in stock torch (what LineDescriptiveEncoder composes of native kernels in train mode): r0 [B L, 4, S],
    r1, r2 [B L, 256].  mistake 'bias_not_kept': the value bias not scaled by kept (a planted error)"""
    B, L, S, _ = desc.shape
    x = desc.reshape(B * L, S, D)
    x0 = x[:, 0]
    q = (x0 @ p["slf_attn.w_qs.weight"].T + p["slf_attn.w_qs.bias"]) * 0.125
    u = torch.einsum("lhd,hdc->lhc", q.view(-1, HEADS, DH), p["slf_attn.w_ks.weight"].view(HEADS, DH, D))
    a = torch.softmax(torch.einsum("lhc,ltc->lht", u, x), dim=2) * r0
    pooled, kept = torch.einsum("lht,ltc->lhc", a, x), a.sum(dim=2)
    bv = p["slf_attn.w_vs.bias"].view(HEADS, DH)
    o = torch.einsum("lhc,hdc->lhd", pooled, p["slf_attn.w_vs.weight"].view(HEADS, DH, D))
    o = (o + (bv if mistake == "bias_not_kept" else kept[:, :, None] * bv)).reshape(-1, D)
    y = F.layer_norm((o @ p["slf_attn.fc.weight"].T + p["slf_attn.fc.bias"]) * r1 + x0, (D,), p["slf_attn.layer_norm.weight"],
                     p["slf_attn.layer_norm.bias"], EPS)
    hidden = F.gelu(y @ p["pos_ffn.w_1.weight"].T + p["pos_ffn.w_1.bias"])
    out = F.layer_norm((hidden @ p["pos_ffn.w_2.weight"].T + p["pos_ffn.w_2.bias"]) * r2 + y, (D,), p["pos_ffn.layer_norm.weight"],
                       p["pos_ffn.layer_norm.bias"], EPS)
    return out.view(B, L, D)


def run_layer(sd, desc, upstream, dtype, p, seed=SEED, call=0, folded=False, mistake=None, other=OTHER_ROWS_SEED, device="cpu"):
    """The masked layer differentiated by torch at `dtype`, the upstream arriving at row 0 of its output: dict out [B, L, 256], d_desc and
    the parameter gradients, float64 arrays (desc_layer_reference.run_layer's).  `folded`: through folded_forward."""
    B, L, S = desc.shape[:3]
    mod = MaskedLayer().to(dtype)
    mod.load_state_dict(DL.tensors(sd, dtype), strict=True)
    mod = mod.to(device).train()
    xt = torch.tensor(desc, dtype=dtype, device=device, requires_grad=True)
    tt = lambda a: torch.tensor(a, dtype=dtype, device=device)
    with torch.enable_grad():
        if folded:
            out = folded_forward(dict(mod.named_parameters()), xt, tt(pool_factors(seed, call, B * L, S, p)),
                                 tt(row_factors(seed, call, 1, B * L, p)), tt(row_factors(seed, call, 2, B * L, p)), mistake)
        else:
            out = mod.set_masks(*(tt(m) for m in masks(B, L, S, seed, call, p, other)))(xt)[:, :, 0]
        out.backward(tt(upstream))
    res = {"out": DL._np64(out), "d_desc": DL._np64(xt.grad)}
    for key, prm in mod.named_parameters():
        res[key] = DL._np64(prm.grad) if prm.grad is not None else np.zeros(tuple(prm.shape))
    return res


@functools.lru_cache(maxsize=None)
def module_refs(B, L, S, p, seed=SEED, call=0):
    """(float64, float32) of the unfolded masked layer on desc_layer_reference.module_case(B, L, S)"""
    sd, desc, g = DL.module_case(B, L, S)
    return run_layer(sd, desc, g, torch.float64, p, seed, call), run_layer(sd, desc, g, torch.float32, p, seed, call)


def fixture_key(key, p):
    return f"{key}@p{p}"


def fixture_grid(key, val):
    """what tests/golden/desc_layer_dropout.npz keeps of a tensor: weight matrices on desc_layer.npz's sub-grid W[::7, ::5], d_desc on every
    second column (two probabilities of the whole tensor would take the file past the size a committed file may have), the rest whole"""
    return val[::7, ::5] if key in DL.MATRICES else val[..., ::2] if key == "d_desc" else val


# ---- the whole model on two views under the criterion ------------------------------------------------------------------------------

MODEL_P = 0.1


def run_loss(dtype, p=MODEL_P, seed=SEED, call=0, device="cpu"):
    """keyline_reference.run_loss with the masked layer in the place of the model's descriptive layer (an attribute of the module object;
    keyline_reference itself is untouched): loss.backward() through the model on both views of its loss_case at `dtype`; view 0 draws the
    masks of `call`, view 1 those of `call + 1`.  dict: loss, V, d_desc0, d_desc1, every parameter's gradient."""
    import keyline_reference as KR
    sd, v0, v1, assign = KR.loss_case()
    B, n, S = KR.LOSS_SHAPE
    mod = KR.Model().to(dtype)
    mod.klenc.desc_layers[0] = MaskedLayer().to(dtype)
    mod.load_state_dict(KR.tensors(sd, dtype), strict=True)
    mod = mod.to(device).train()
    tt = lambda a: torch.tensor(a, dtype=dtype, device=device)
    mod.klenc.desc_layers[0].set_masks(*[tuple(tt(m) for m in masks(B, n, S + 1, seed, call + view, p)) for view in range(2)])
    d0, d1 = KR.data_tensors(v0, dtype, device), KR.data_tensors(v1, dtype, device)
    with torch.enable_grad():
        loss, V = KR.loss_of(mod, d0, d1, tt(assign))
        loss.backward()
    out = {"loss": float(loss.detach()), "V": int(V), "d_desc0": DL._np64(d0["desc_sublines"].grad), "d_desc1": DL._np64(d1["desc_sublines"].grad)}
    for key, prm in mod.named_parameters():
        out[key] = DL._np64(prm.grad)
    return out


@functools.lru_cache(maxsize=None)
def loss_refs():
    return run_loss(torch.float64), run_loss(torch.float32)


# ---- launching (GPU) ---------------------------------------------------------------------------------------------------------------

def drop_struct(nat, seed, call, p):
    """the LinetrDropout of (seed, call, p), made HERE from the formulas (not by the package): threshold floor(p 2^32), scale float32"""
    return nat.Dropout(seed, call, threshold(p), float(scale(p)))


def factors_launch(lib, nat, seed, call, site, rows, inner, p, device="cuda:0"):
    import ctypes as C
    out = torch.full((rows * inner + 1, 4), DL.MARKER, dtype=torch.float32, device=device)
    rc = lib.linetr_dropout_factors(None, C.byref(drop_struct(nat, seed, call, p)), site, rows, inner, out.data_ptr(), DL._stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    return DL._take(out, rows * inner, 4, "factors").reshape(rows, inner, 4)


def pool_launch(lib, nat, c, ldx=256, ldu=1024, need=(True, True), dkept=True, device="cuda:0"):
    """The raw dropout pooling entry points on a pool_case (or any dict with its keys): forward, then backward, as
    desc_layer_reference.pool_launch lays the buffers out -- sentinel rows behind every input, a marker row behind every output."""
    import ctypes as C
    L, S = c["L"], c["S"]
    rs = DL._rs("dropout pool launch", ldx, ldu)
    x = DL._inp(c["x"].reshape(L * S, D), ldx, rs, device)
    u = DL._inp(c["u"].reshape(L, HEADS * D), ldu, rs, device)
    dp = DL._inp(c["dpooled"].reshape(L, HEADS * D), HEADS * D, rs, device)
    dk = DL._inp(c["dkept"], HEADS, rs, device) if dkept else None
    pooled, kept, lse = DL._out(L, HEADS * D, device), DL._out(L, HEADS, device), DL._out(L, HEADS, device)
    dx, du = DL._out(L * S, ldx, device, need[0]), DL._out(L, ldu, device, need[1])
    drop = drop_struct(nat, c["seed"], c["call"], c["p"])
    rc = lib.linetr_cls_pool_dropout_forward(None, x.data_ptr(), ldx, u.data_ptr(), ldu, L, S, C.byref(drop), pooled.data_ptr(), kept.data_ptr(),
                                             lse.data_ptr(), DL._stream())
    assert rc == 0, lib.linetr_last_error()
    rc = lib.linetr_cls_pool_dropout_backward(None, x.data_ptr(), ldx, u.data_ptr(), ldu, pooled.data_ptr(), lse.data_ptr(), kept.data_ptr(),
                                              dp.data_ptr(), DL._ptr(dk), L, S, C.byref(drop), DL._ptr(dx), ldx, DL._ptr(du), ldu, DL._stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    res = {"pooled": DL._take(pooled, L, HEADS * D, "pooled").reshape(L, HEADS, D), "kept": DL._take(kept, L, HEADS, "kept"),
           "lse": DL._take(lse, L, HEADS, "lse")}
    if dx is not None:
        res["dx"] = DL._take(dx, L * S, D, "dx").reshape(L, S, D)
    if du is not None:
        res["du"] = DL._take(du, L, HEADS * D, "du").reshape(L, HEADS, D)
    return res


def ln_launch(lib, nat, c, ld=256, need=(True, True, True, True), device="cuda:0"):
    """The raw dropout LayerNorm entry points on an ln_case: forward, then backward; dict of CPU arrays (what `need` = (da, dr, dgamma,
    dbeta) leaves out stays away; without a residual dr is still computed where asked for: it is dv)"""
    import ctypes as C
    rows = c["rows"]
    rs = DL._rs("dropout ln launch", ld)
    a, g = DL._inp(c["a"], ld, rs, device), DL._inp(c["g"], ld, rs, device)
    r = DL._inp(c["r"], ld, rs, device) if c["r"] is not None else None
    gamma, beta = (torch.from_numpy(c[k]).to(device) for k in ("gamma", "beta"))
    y, stats = DL._out(rows, ld, device), DL._out(rows, 2, device)
    da, dr = DL._out(rows, ld, device, need[0]), DL._out(rows, ld, device, need[1])
    dgamma, dbeta = (DL._out(1, D, device, n) for n in need[2:])
    drop = drop_struct(nat, c["seed"], c["call"], c["p"])
    rc = lib.linetr_layer_norm_dropout_forward(None, a.data_ptr(), ld, DL._ptr(r), ld, gamma.data_ptr(), beta.data_ptr(), EPS, rows, D, C.byref(drop),
                                               c["site"], y.data_ptr(), ld, stats.data_ptr(), DL._stream())
    assert rc == 0, lib.linetr_last_error()
    ws = torch.empty(max(int(lib.linetr_layer_norm_backward_workspace_bytes(rows, D)), 16), dtype=torch.uint8, device=device)
    rc = lib.linetr_layer_norm_dropout_backward(None, a.data_ptr(), ld, DL._ptr(r), ld, stats.data_ptr(), gamma.data_ptr(), g.data_ptr(), ld, rows, D,
                                                C.byref(drop), c["site"], DL._ptr(da), ld, DL._ptr(dr), ld, DL._ptr(dgamma), DL._ptr(dbeta),
                                                ws.data_ptr(), ws.numel(), DL._stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    st = DL._take(stats, rows, 2, "stats")
    res = {"y": DL._take(y, rows, D, "y"), "mean": st[:, 0], "rstd": st[:, 1], "_stats": st}
    for key, t, n in (("da", da, rows), ("dr", dr, rows), ("dgamma", dgamma, 1), ("dbeta", dbeta, 1)):
        if t is not None:
            res[key] = DL._take(t, n, D, key) if n == rows and key in ("da", "dr") else DL._take(t, n, D, key)[0]
    return res
