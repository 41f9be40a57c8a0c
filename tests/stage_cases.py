"""Cases, references, launches and error measure of the stage unit tests (tests/test_gpu_stages.py, tests/test_stage_cases_cpu.py;
reused by tools/stage_unit_report.py, which writes profiles/stage_unit_errors.txt).  Test infrastructure only.

Two stages from the middle of the forward pass run alone through linetr_debug_stage: the descriptive layer's tail (value projection,
fc + LayerNorm, FFN with GELU, second LayerNorm + line_pos) and the line-signature network (0 .. 7 layers, final projection, L2
norm).  Their references are built from the UNFOLDED torch state dict, in float64 (`ref64`) and in plain float32 torch (`ref32`);
none of the weights the preparation (linetr_amd/csrc/lt_prepare.h, run by linetr_create) derives -- Watt, the fc bias with the CLS
residual, the permuted / scaled q/k/v projections, the BatchNorm and merge folds, Wnext, Wfin2 -- enters them, so the tests check the
kernels on those folds end to end.  The folds themselves are pinned on the CPU: tests/test_prepare_cpu.py compares every prepared
tensor with `folded` below, within one float32 ulp.

TEACHER FORCING.  No bar compounds over layers: the reference of every tensor is computed from the tensor the device itself handed
to that step -- o from the device's att, zA from the device's o, x_out behind layer l from the device's x_out behind layer l - 1
(z0 for l = 0), line_desc from the device's x_out behind layer L - 2 through the last layer and the head.  A tensor passes when

    max |gpu - ref64|  <=  FACTOR * max( max |ref32 - ref64| ,  2^-23 * max |ref64| )        (FACTOR = 8, as attn_cases.py)

per tensor (tail) or per image and tensor (signature network).  The bar is a property of the CPU references alone.

The second half of the file restates the folds of lt_prepare.h (float64, rounded once to float32) and the forward pass's float32 graph
over them, with switches that plant one mistake each: tests/test_stage_cases_cpu.py runs it through the same checks in the device's
place, to show that the cases leave the kernels headroom and that every planted mistake breaks a bar."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from attn_cases import FACTOR, MARKER, SENTINEL, SPARE_ROWS, cu_of, state_dict_t
from oracle import linetr_oracle as O

POOLW = 544
WORD = "klenc.word_position_enc.encoder"
WEIGHTS = ("calibrated", 3)
EPS = 1e-12               # F.normalize's eps
NORM_CLEAR = 1e3          # every compared row keeps |final_proj(x)| this factor away from EPS (as linear_bwd_reference.NORM_CLEAR)
FOLD_NEXT = 8             # LINETR_STAGE_FOLD_NEXT
FUSED = 4
PLAN_NAMES = {0: "sig_attn", 1: "small", 2: "split4", 3: "split8", 4: "fused", 1 + FOLD_NEXT: "small+fold_next"}

TAIL_N = (1, 2, 33, 129, 257)
TAIL_FAMILIES = ("normal", "p0_ends", "pad", "sentinel")
SIG_COUNTS = (0, 1, 2, 33, 129)                 # N = 165
SIG_FAMILIES = ("normal", "sentinel")
FORCED = {"f32": (0,), "bf16x6": (1, 2, 3, 1 + FOLD_NEXT, FUSED)}
DEPTHS = (0, 1, 2, 7)
# (counts, expected plan in bf16x6): the dispatcher's own choice, both sides of sig_attn_plan's rules; every case is 0 in f32
DISPATCH = (((33,), 1 + FOLD_NEXT),
            (tuple(1 + i % 8 for i in range(32)), FUSED),
            (tuple(min(40, 5 + 3 * i) for i in range(16)), 2),
            (tuple(129 if i == 7 else 3 + i for i in range(16)), 3))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _sentinel(shape, g):
    return SENTINEL * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


@functools.lru_cache(maxsize=None)
def weights_t(weights, n_layers=7):
    """(numpy state dict for Engine, torch state dict) of `weights` with the signature layers behind the first n_layers removed"""
    sd, sd_t = state_dict_t(weights)
    keep = lambda k: not k.startswith("selfattn.layers.") or int(k.split(".")[2]) < n_layers
    return {k: v for k, v in sd.items() if keep(k)}, {k: v for k, v in sd_t.items() if keep(k)}


@functools.lru_cache(maxsize=None)
def _cast(weights, n_layers, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in weights_t(weights, n_layers)[1].items()}


def n_layers_of(sd_t):
    n = 0
    while f"selfattn.layers.{n}.attn.merge.weight" in sd_t:
        n += 1
    return n


def _desc_prefix(sd_t):
    n = 0
    while f"klenc.desc_layers.{n}.slf_attn.fc.weight" in sd_t:
        n += 1
    return f"klenc.desc_layers.{n - 1}."


# =================================================================================================================================
# references (unfolded state dict `sd`, already cast to the dtype of the inputs)
# =================================================================================================================================

def tail_att(sd, pooled):
    """att_h = Wv_h (dbar + W5 abar + (1 - p0) b5 + p0 cls) + bv_h from pooled rows [N, 4, 544] = [dbar | abar | p0 | pad] -> [N, 256]
    head-major (models/line_attention.py:55-57: the descriptive heads are head-major)"""
    p = _desc_prefix(sd) + "slf_attn."
    cls, W5, b5 = sd["klenc.cls_token"].reshape(256), sd[WORD + ".12.weight"][:, :, 0], sd[WORD + ".12.bias"]
    pooled = pooled.to(cls.dtype)
    p0 = pooled[:, :, 512:513]
    x = pooled[:, :, :256] + F.linear(pooled[:, :, 256:512], W5) + (1 - p0) * b5 + p0 * cls
    att = torch.einsum("nhc,hdc->nhd", x, sd[p + "w_vs.weight"].view(4, 64, 256)) + sd[p + "w_vs.bias"].view(4, 64)
    return att.reshape(-1, 256)


def tail_o(sd, att):
    """o = LN(fc(att) + cls, 1e-6)  (line_attention.py:36-40; the CLS row's residual is the CLS token)"""
    p = _desc_prefix(sd) + "slf_attn."
    cls = sd["klenc.cls_token"].reshape(256)
    return F.layer_norm(F.linear(att.to(cls.dtype), sd[p + "fc.weight"], sd[p + "fc.bias"]) + cls, (256,), sd[p + "layer_norm.weight"],
                        sd[p + "layer_norm.bias"], 1e-6)


def tail_z(sd, o, lpos):
    """zA = lpos + LN(w_2(gelu(w_1 o)) + o, 1e-6)  (line_attention.py:79-83, line_transformer.py:128)"""
    p = _desc_prefix(sd) + "pos_ffn."
    o = o.to(sd[p + "w_1.weight"].dtype)
    f = F.linear(F.gelu(F.linear(o, sd[p + "w_1.weight"], sd[p + "w_1.bias"])), sd[p + "w_2.weight"], sd[p + "w_2.bias"]) + o
    return lpos.to(o.dtype) + F.layer_norm(f, (256,), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1e-6)


def sig_layer(sd, l, z):
    """one signature layer on ONE image's rows: z + mlp([z ; merge(attention(z))])  (line_transformer.py:132-183), restated with
    the oracle's own pieces"""
    a = f"selfattn.layers.{l}.attn"
    msg = F.linear(O.sig_attention(sd, l, z), sd[f"{a}.merge.weight"][:, :, 0], sd[f"{a}.merge.bias"])
    return z + O._mlp(sd, f"selfattn.layers.{l}.mlp", torch.cat([z, msg], dim=1))


def final_proj(sd, x):
    return F.linear(x, sd["final_proj.weight"][:, :, 0], sd["final_proj.bias"])


def sig_head(sd, x):
    return F.normalize(final_proj(sd, x), p=2, dim=1)          # line_transformer.py:245-246


def sig_chain(sd, z0, cu):
    """the whole signature network from z0, per image -> (line_desc, [x_out behind layer 0 .. L - 1])"""
    z = z0.to(sd["final_proj.bias"].dtype)
    outs = []
    for l in range(n_layers_of(sd)):
        zn = torch.zeros_like(z)
        for i in range(len(cu) - 1):
            a, b = int(cu[i]), int(cu[i + 1])
            if b > a:
                zn[a:b] = sig_layer(sd, l, z[a:b])
        z = zn
        outs.append(z)
    return sig_head(sd, z), outs


# =================================================================================================================================
# cases
# =================================================================================================================================

@functools.lru_cache(maxsize=None)
def tail_case(family, N, seed=0):
    """pooled [N, 4, 544] and lpos [N, 256].  normal: dbar, abar, lpos unit normal, p0 uniform in (0, 1), zeros in the 31 pad columns;
    p0_ends: p0 exactly 0 and exactly 1 in alternating rows; pad: 'normal' with +-1e4 in the pad columns (the same bits must come
    out); sentinel: another draw of 'normal' (every launch has +-1e4 rows behind its inputs and marker rows behind its outputs)"""
    if family not in TAIL_FAMILIES:
        raise ValueError(family)
    g = _gen("tail", "normal" if family == "pad" else family, N, seed)
    pooled = torch.zeros((N, 4, POOLW))
    pooled[:, :, :512] = torch.randn((N, 4, 512), generator=g)
    pooled[:, :, 512] = torch.rand((N, 4), generator=g).clamp(1e-3, 1 - 1e-3)
    lpos = torch.randn((N, 256), generator=g)
    if family == "p0_ends":
        pooled[:, :, 512] = (torch.arange(N) % 2).float()[:, None]
    elif family == "pad":
        pooled[:, :, 513:] = _sentinel((N, 4, POOLW - 513), _gen("pad", N))
    return dict(kind="tail", family=family, N=N, pooled=pooled, lpos=lpos)


@functools.lru_cache(maxsize=None)
def sig_case(family, counts, seed=0, parity=0):
    """z0 [N, 256] unit normal; sentinel: +-1e4 rows in the images of one parity, the others are compared"""
    if family not in SIG_FAMILIES:
        raise ValueError(family)
    g = _gen("sig", family, counts, seed)
    cu = cu_of(counts)
    z0 = torch.randn((int(cu[-1]), 256), generator=g)
    check = list(range(len(counts)))
    if family == "sentinel":
        check = [i for i in range(len(counts)) if i % 2 != parity]
        for i, n in enumerate(counts):
            if i % 2 == parity and n:
                z0[int(cu[i]):int(cu[i + 1])] = _sentinel((n, 256), g)
    return dict(kind="sig", family=family, counts=counts, cu=cu, z0=z0, check=check, N=int(cu[-1]))


def tail_cases():
    return [tail_case(f, N) for f in TAIL_FAMILIES for N in TAIL_N]


def sig_cases(counts=SIG_COUNTS):
    """the batch as 'normal' and as 'sentinel' in both parities, so that every image is compared in a sentinel batch too"""
    return [sig_case("normal", counts), sig_case("sentinel", counts, parity=0), sig_case("sentinel", counts, parity=1)]


# =================================================================================================================================
# launches
# =================================================================================================================================

def _guarded(t, device, tag):
    """t with SPARE_ROWS rows of +-1e4 behind it, on the device"""
    return torch.cat([t, _sentinel((SPARE_ROWS,) + tuple(t.shape[1:]), _gen("guard", tag, t.shape[0]))]).contiguous().to(device)


def launch_tail(eng, case):
    """-> {att, o, zA} [N, 256] on the CPU, after asserting that the marker row behind every output is intact"""
    N = case["N"]
    outs = [torch.full((N + 1, 256), MARKER, dtype=torch.float32, device=eng.device) for _ in range(3)]
    eng.debug_stage("tail", _guarded(case["pooled"], eng.device, "pooled"), _guarded(case["lpos"], eng.device, "lpos"), N, -1, tuple(outs))
    torch.cuda.synchronize()
    res = {}
    for name, o in zip(("att", "o", "zA"), outs):
        o = o.cpu()
        assert bool((o[N] == MARKER).all()), f"{name}: the row behind the output was written"
        res[name] = o[:N]
    return res


def launch_sig(eng, case, plan=-1):
    """-> (line_desc [N, 256], taps [L - 1, N, 256], plan used) on the CPU, after asserting that the sentinel rows behind the input
    and the marker rows behind both outputs are intact"""
    N, L = case["N"], int(eng.cfg["n_sig_layers"])
    nt = max(L - 1, 0)
    z = _guarded(case["z0"], eng.device, "z0")
    before = z.clone()
    desc = torch.full((N + 1, 256), MARKER, dtype=torch.float32, device=eng.device)
    taps = torch.full((nt * N + 1, 256), MARKER, dtype=torch.float32, device=eng.device)
    used = eng.debug_stage("sig", z, None, case["cu"], plan, (desc, taps, None))
    torch.cuda.synchronize()
    assert torch.equal(z, before), "the input rows or the sentinel rows behind them were written"
    desc, taps = desc.cpu(), taps.cpu()
    assert bool((desc[N] == MARKER).all()) and bool((taps[nt * N] == MARKER).all()), "a row behind an output was written"
    return desc[:N], taps[:nt * N].view(nt, N, 256), used


# =================================================================================================================================
# error measure
# =================================================================================================================================

def _row(what, unit, n, got, r64, r32):
    err = (got.double() - r64).abs().max().item()
    bar = FACTOR * max((r32.double() - r64).abs().max().item(), 2.0 ** -23 * r64.abs().max().item())
    return (what, unit, n, err, bar)


def tail_errors(got, case, weights):
    """[(tensor, 'all', N, max |got - ref64|, bar)] of att, o and zA; o is judged from the att that was handed in, zA from the o"""
    sd64, sd32 = _cast(weights, 7, torch.float64), _cast(weights, 7, torch.float32)
    rows = []
    for name, fn in (("att", lambda sd, dt: tail_att(sd, case["pooled"].to(dt))), ("o", lambda sd, dt: tail_o(sd, got["att"].to(dt))),
                     ("zA", lambda sd, dt: tail_z(sd, got["o"].to(dt), case["lpos"].to(dt)))):
        rows.append(_row(name, "all", case["N"], got[name], fn(sd64, torch.float64), fn(sd32, torch.float32)))
    return rows


def sig_errors(desc, taps, case, weights, n_layers):
    """[(tensor, image, sub-lines, max |got - ref64|, bar)] of every tap and of line_desc, for every compared image with at least
    one sub-line: layer l from tap l - 1 as it was handed in (z0 for l = 0), line_desc from tap L - 2 through the last layer and the
    head.  Asserts the premise: every compared row's |final_proj(x)| stays NORM_CLEAR clear of F.normalize's eps."""
    sd64, sd32 = _cast(weights, n_layers, torch.float64), _cast(weights, n_layers, torch.float32)
    cu, rows = case["cu"], []
    for i in case["check"]:
        a, b = int(cu[i]), int(cu[i + 1])
        if a == b:
            continue
        for l in range(n_layers + 1):
            x = case["z0"][a:b] if l == 0 else taps[l - 1][a:b]
            if l == n_layers or l == n_layers - 1:       # the head, behind the last layer where there is one
                step = lambda sd, v: sig_head(sd, sig_layer(sd, l, v) if l < n_layers else v)
                pre = final_proj(sd64, sig_layer(sd64, l, x.double()) if l < n_layers else x.double())
                assert float(pre.norm(dim=1).min()) >= NORM_CLEAR * EPS, "a compared row sits at F.normalize's eps"
                rows.append(_row("line_desc", i, b - a, desc[a:b], step(sd64, x.double()), step(sd32, x.float())))
                break
            rows.append(_row(f"x_out{l}", i, b - a, taps[l][a:b], sig_layer(sd64, l, x.double()), sig_layer(sd32, l, x.float())))
    return rows


def failures(rows):
    return [f"{w} [{u}] ({n} rows): error {e:.3e} > bar {b:.3e} (x{e / b:.1f})" for w, u, n, e, b in rows if not e <= b]


def worst(rows):
    return max((e / b for _, _, _, e, b in rows), default=0.0)


# =================================================================================================================================
# the folds of lt_prepare.h restated (float64, rounded once to float32) and the forward pass's float32 graph over them
# =================================================================================================================================

MISTAKES = ("wfin2_bias_without_wfin_b2", "mlp0_bias_without_w1b_bm", "bn_eps_1e-6", "ln_eps_1e-5", "merge_columns_not_permuted",
            "q_not_scaled", "fc_bias_without_cls", "b5_not_scaled_by_1_minus_p0", "gelu_tanh", "wnext_bias_without_wqkv_b2")


def _head_major(W):
    """rows c = d*4 + h of a projection (line_transformer.py:151) -> c' = h*64 + d"""
    return W.reshape(64, 4, *W.shape[1:]).transpose(0, 1).reshape(W.shape)


@functools.lru_cache(maxsize=None)
def folded(weights, n_layers=7, mistake=None):
    """the weights the preparation (lt_prepare.h) derives, as float32 tensors under its entry names; `mistake`: one of MISTAKES planted.
    tests/test_prepare_cpu.py holds the library's own tensors to these"""
    assert mistake is None or mistake in MISTAKES
    sd = _cast(weights, n_layers, torch.float64)
    f = {}
    p = _desc_prefix(sd)
    cls, W5, b5 = sd["klenc.cls_token"].reshape(256), sd[WORD + ".12.weight"][:, :, 0], sd[WORD + ".12.bias"]
    Wv, bv = sd[p + "slf_attn.w_vs.weight"], sd[p + "slf_attn.w_vs.bias"]
    Watt = torch.zeros((256, POOLW), dtype=torch.float64)
    Watt[:, :256], Watt[:, 256:512] = Wv, Wv @ W5
    Watt[:, 512] = Wv @ (cls if mistake == "b5_not_scaled_by_1_minus_p0" else cls - b5)
    f["Watt"], f["batt"] = Watt, Wv @ b5 + bv
    f["Wfc"] = sd[p + "slf_attn.fc.weight"]
    f["bfc"] = sd[p + "slf_attn.fc.bias"] + (0 if mistake == "fc_bias_without_cls" else cls)
    for k, name in (("ln1g", "slf_attn.layer_norm.weight"), ("ln1b", "slf_attn.layer_norm.bias"), ("Wf1", "pos_ffn.w_1.weight"),
                    ("bf1", "pos_ffn.w_1.bias"), ("Wf2", "pos_ffn.w_2.weight"), ("bf2", "pos_ffn.w_2.bias"),
                    ("ln2g", "pos_ffn.layer_norm.weight"), ("ln2b", "pos_ffn.layer_norm.bias")):
        f[k] = sd[p + name]
    bn_eps = 1e-6 if mistake == "bn_eps_1e-6" else 1e-5
    for l in range(n_layers):
        s = f"selfattn.layers.{l}."
        W = [_head_major(sd[f"{s}attn.proj.{j}.weight"][:, :, 0]) for j in range(3)]
        b = [_head_major(sd[f"{s}attn.proj.{j}.bias"]) for j in range(3)]
        if mistake != "q_not_scaled":
            W[0], b[0] = W[0] * 0.125, b[0] * 0.125
        f[f"Wqkv{l}"], f[f"bqkv{l}"] = torch.cat(W), torch.cat(b)
        Wm, bm = sd[s + "attn.merge.weight"][:, :, 0], sd[s + "attn.merge.bias"]
        Wm2 = Wm if mistake == "merge_columns_not_permuted" else _head_major(Wm.t().contiguous()).t()      # columns to head-major
        g = sd[s + "mlp.1.weight"] / torch.sqrt(sd[s + "mlp.1.running_var"] + bn_eps)
        W1 = sd[s + "mlp.0.weight"][:, :, 0] * g[:, None]
        b1 = (sd[s + "mlp.0.bias"] - sd[s + "mlp.1.running_mean"]) * g + sd[s + "mlp.1.bias"]
        f[f"W1m{l}"] = torch.cat([W1[:, :256], W1[:, 256:] @ Wm2], dim=1)
        f[f"b1m{l}"] = b1 + (0 if mistake == "mlp0_bias_without_w1b_bm" else W1[:, 256:] @ bm)
        f[f"W2{l}"], f[f"b2{l}"] = sd[s + "mlp.3.weight"][:, :, 0], sd[s + "mlp.3.bias"]
    for l in range(n_layers - 1):          # [x_out ; qkv_next] = [[I, W2], [Wqkv, Wqkv W2]] [z ; hid] + [b2 ; Wqkv b2 + bqkv]
        W2, b2, Wq, bq = f[f"W2{l}"], f[f"b2{l}"], f[f"Wqkv{l + 1}"], f[f"bqkv{l + 1}"]
        f[f"Wnext{l}"] = torch.cat([torch.cat([torch.eye(256, dtype=torch.float64), W2], dim=1), torch.cat([Wq, Wq @ W2], dim=1)])
        f[f"bnext{l}"] = torch.cat([b2, bq + (0 if mistake == "wnext_bias_without_wqkv_b2" else Wq @ b2)])
    Wfin, bfin = sd["final_proj.weight"][:, :, 0], sd["final_proj.bias"]
    f["Wfin"], f["bfin"] = Wfin, bfin
    if n_layers:
        W2, b2 = f[f"W2{n_layers - 1}"], f[f"b2{n_layers - 1}"]
        f["Wfin2"] = torch.cat([Wfin, Wfin @ W2], dim=1)
        f["bfin2"] = bfin + (0 if mistake == "wfin2_bias_without_wfin_b2" else Wfin @ b2)
    return {k: v.float().contiguous() for k, v in f.items()}


def _gelu_tanh(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def folded_tail(case, weights, mistake=None):
    """the tail's float32 graph over the folded weights -> {att, o, zA}, every launch fed by the previous one's output"""
    f = folded(weights, 7, mistake)
    ln_eps = 1e-5 if mistake == "ln_eps_1e-5" else 1e-6
    gelu = _gelu_tanh if mistake == "gelu_tanh" else F.gelu
    N = case["N"]
    att = torch.cat([F.linear(case["pooled"][:, h], f["Watt"][64 * h:64 * h + 64], f["batt"][64 * h:64 * h + 64]) for h in range(4)], dim=1)
    o = F.layer_norm(F.linear(att, f["Wfc"], f["bfc"]), (256,), f["ln1g"], f["ln1b"], ln_eps)
    ffn = F.linear(gelu(F.linear(o, f["Wf1"], f["bf1"])), f["Wf2"], f["bf2"]) + o
    zA = F.layer_norm(ffn, (256,), f["ln2g"], f["ln2b"], ln_eps) + case["lpos"]
    assert att.shape == o.shape == zA.shape == (N, 256)
    return {"att": att, "o": o, "zA": zA}


def _attention(qkv, cu):
    """softmax(q k^T) v per image and head on head-major rows [N, 768] whose q is scaled already -> [N, 256] head-major"""
    msg = torch.zeros((qkv.shape[0], 256), dtype=qkv.dtype)
    for i in range(len(cu) - 1):
        a, b = int(cu[i]), int(cu[i + 1])
        if b > a:
            q, k, v = (qkv[a:b, j * 256:(j + 1) * 256].reshape(b - a, 4, 64) for j in range(3))
            msg[a:b] = torch.einsum("hnm,mhd->nhd", torch.softmax(torch.einsum("nhd,mhd->hnm", q, k), dim=-1), v).reshape(b - a, 256)
    return msg


def folded_sig(case, weights, n_layers, fold_next=False, mistake=None):
    """sig_network's float32 graph over the folded weights (plain route, or fold_next: x_out and the next layer's q/k/v out of one
    contraction over [z ; hid]) -> (line_desc, taps [L - 1, N, 256]), as launch_sig returns them"""
    cu, N = case["cu"], case["N"]
    if len(cu) > 2:        # image by image, as the references are evaluated: the images are independent
        desc, taps = torch.zeros((N, 256)), torch.zeros((max(n_layers - 1, 0), N, 256))
        for i in range(len(cu) - 1):
            a, b = int(cu[i]), int(cu[i + 1])
            if b > a:
                one = dict(z0=case["z0"][a:b], cu=cu_of([b - a]), N=b - a)
                desc[a:b], taps[:, a:b] = folded_sig(one, weights, n_layers, fold_next, mistake)
        return desc, taps
    f = folded(weights, n_layers, mistake)
    z, taps, qkv = case["z0"], [], None
    hid = None
    for l in range(n_layers):
        if qkv is None:
            qkv = F.linear(z, f[f"Wqkv{l}"], f[f"bqkv{l}"])
        hid = F.relu(F.linear(torch.cat([z, _attention(qkv, cu)], dim=1), f[f"W1m{l}"], f[f"b1m{l}"]))
        qkv = None
        if l + 1 == n_layers:
            break
        if fold_next:
            zq = F.linear(torch.cat([z, hid], dim=1), f[f"Wnext{l}"], f[f"bnext{l}"])
            z, qkv = zq[:, :256], zq[:, 256:]
        else:
            z = z + F.linear(hid, f[f"W2{l}"], f[f"b2{l}"])
        taps.append(z)
    pre = F.linear(torch.cat([z, hid], dim=1), f["Wfin2"], f["bfin2"]) if n_layers else F.linear(z, f["Wfin"], f["bfin"])
    return F.normalize(pre, p=2, dim=1), (torch.stack(taps) if taps else torch.zeros((0, case["N"], 256)))
