"""Case generator, references and error measure of the front-end unit tests (tests/test_gpu_front.py, tests/test_front_cases_cpu.py;
reused by tools/front_unit_report.py, which writes profiles/front_unit_errors.txt).  Test infrastructure only.

The descriptive layer's front end is the positional encoders' MLP up to its fourth ReLU (lt_tokmlp.h) and the CLS-row attention
pooling (lt_model.h), fed through the NCHW -> NHWC layout pass.  Every case has two CPU references of the same formula, built from
the UNFOLDED state dict -- conv + BatchNorm(eval) + ReLU layer by layer, w_qs / w_ks applied to cls_token and to every key -- in
float64 (`ref64`) and in plain float32 torch (`ref32`); none of the constants the preparation (linetr_amd/csrc/lt_prepare.h, run by
linetr_create) derives -- U, U2, c_tok, s_cls, the folded weights -- enters them, so the tests check the kernels on those constants
end to end.  The constants themselves are pinned on the CPU: tests/test_prepare_cpu.py compares them with a float64 restatement from
`_pool_consts` below, within one float32 ulp.  A kernel passes a unit (a 64-row tile of the MLP; a
sub-line of the pooling, its 512 vector columns and its CLS weight p_0 measured separately) when

    max |gpu - ref64|  <=  FACTOR * max( max |ref32 - ref64| ,  2^-23 * max |ref64| )        (FACTOR = 8, as attn_cases.py)

over that unit.  The bar is a property of the CPU references alone, never of a kernel's output.  KERNEL_ORDER names the families
whose bar also takes a second CPU float32 evaluation written in the kernel's own legitimate operation order (`ref32k`) into the
max; the report says which they are and why."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from attn_cases import FACTOR, MARKER, SENTINEL, SPARE_ROWS, state_dict_t
from linetr_amd import _native as nat
from oracle import linetr_oracle as O

HW = (480, 640)                    # the handle's image_shape: normalize_keylines' centre and scale
POOLW = 544
ENC = {"word": "klenc.word_position_enc.encoder", "line": "klenc.line_position_enc.encoder"}
WEIGHTS = ("calibrated", 3)
# (kind, family) pairs whose bar includes ref32k.  pool / peaky: with |score| near 20 one float32 rounding of a score moves p_0 by
# 20 x 2^-24 of itself, more than the 2^-23 floor, and whether ref32 happens to show that on the four p_0 of a sub-line is luck (it
# differs from host to host with the BLAS); the kernels' error there is the folded score's rounding, which ref32k reproduces on the
# CPU to 10 % (cls_pool_kernel: T = 68, sub-line 2: GPU 6.1e-8, ref32k 5.8e-8, plain bar 4.0e-8).
KERNEL_ORDER = frozenset({("pool", "peaky")})


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _sentinel(shape, g):
    return SENTINEL * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


# =================================================================================================================================
# token MLP
# =================================================================================================================================

MLP_FAMILIES = ("workload", "edge", "wide")
MLP_ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)      # one tile per block
MLP_WALK = tuple((mb, 64 * k + r) for mb in (1, 2, 3) for k in (2, 3, 5, 7) for r in (0, 1, 63))   # (max_blocks, rows)
DUAL_PAIRS = ((1, 1), (65, 1), (1, 65), (4378, 398))
VARIANTS = ("tok_mlp_word", "tok_mlp_line", "tok_mlp_dual", "tok_mlp_seq", "mlp123_gemm_chain")


def enc_features(enc, inputs, dtype):
    """(x - cx, y - cy) / scale, score of the word encoder; (mid x, mid y, response, cos, sin) of the line encoder
    (models/line_transformer.py:22-73), every operation in `dtype`"""
    ctr = torch.tensor([HW[1] / 2.0, HW[0] / 2.0], dtype=dtype)
    scale = torch.tensor(float(max(HW)), dtype=dtype) * 0.7 if dtype == torch.float32 else torch.tensor(448.0, dtype=dtype)
    if enc == "word":
        pnt, score = inputs
        return torch.cat([(pnt.to(dtype) - ctr) / scale, score.to(dtype)[:, None]], dim=1)
    sub, resp, ang = inputs
    sn = (sub.to(dtype).view(-1, 2, 2) - ctr) / scale
    return torch.cat([(sn[:, 0] + sn[:, 1]) / 2.0, resp.to(dtype)[:, None], ang.to(dtype)], dim=1)


def mlp4(sd_t, enc, feats, dtype):
    """The encoder's first four conv + BatchNorm(eval) + ReLU layers (line_transformer.py:9-20) on feature rows, in `dtype`"""
    x = feats
    for i in range(4):
        c, b = f"{ENC[enc]}.{3 * i}", f"{ENC[enc]}.{3 * i + 1}"
        x = F.linear(x, sd_t[c + ".weight"][:, :, 0].to(dtype), sd_t[c + ".bias"].to(dtype))
        x = (x - sd_t[b + ".running_mean"].to(dtype)) / torch.sqrt(sd_t[b + ".running_var"].to(dtype) + 1e-5)
        x = F.relu(x * sd_t[b + ".weight"].to(dtype) + sd_t[b + ".bias"].to(dtype))
    return x


def mlp4_kernel_order(sd_t, enc, feats32):
    """float32 in the kernels' operation order: BatchNorm folded into the convolutions (in float64, rounded once, as
    linetr_create does), layer 1 as bias + one multiply and one add per term, layers 2-4 as float32 products"""
    x = feats32
    for i in range(4):
        c, b = f"{ENC[enc]}.{3 * i}", f"{ENC[enc]}.{3 * i + 1}"
        g = sd_t[b + ".weight"].double() / torch.sqrt(sd_t[b + ".running_var"].double() + 1e-5)
        W = (sd_t[c + ".weight"][:, :, 0].double() * g[:, None]).float()
        bias = ((sd_t[c + ".bias"].double() - sd_t[b + ".running_mean"].double()) * g + sd_t[b + ".bias"].double()).float()
        if i == 0:
            t = bias[None, :].expand(x.shape[0], -1).clone()
            for k in range(x.shape[1]):
                t = t + W[None, :, k] * x[:, k:k + 1]
            x = F.relu(t)
        else:
            x = F.relu(F.linear(x, W, bias))
    return x


def _mlp_inputs(enc, family, rows, g):
    W, H = float(HW[1]), float(HW[0])
    lim = torch.tensor([W - 0.6, H - 0.6])
    npt = 1 if enc == "word" else 2
    if family == "edge":
        choice = torch.tensor([[0.0, 0.0], [W - 0.6, H - 0.6], [W / 2, H / 2]])
        xy = torch.stack([choice[torch.randint(0, 3, (rows, npt), generator=g), a] for a in (0, 1)], dim=-1)      # [rows, npt, 2]
        if npt == 2:
            same = torch.randint(0, 3, (rows,), generator=g) == 0                     # zero-length sub-lines
            xy[same, 1] = xy[same, 0]
        score = torch.randint(0, 2, (rows,), generator=g).float()
        cs = torch.tensor([[0.0, 1.0], [0.0, -1.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 0.0]])[torch.randint(0, 5, (rows,), generator=g)]
    else:
        xy = torch.rand((rows, npt, 2), generator=g) * lim
        if family == "wide":
            xy = (xy - lim / 2) * 8
        score = torch.rand((rows,), generator=g)
        th = torch.rand((rows,), generator=g) * 6.2831853
        cs = torch.stack([torch.cos(th), torch.sin(th)], dim=1)
    if enc == "word":
        return xy.reshape(rows, 2).contiguous(), score
    return xy.reshape(rows, 4).contiguous(), score * 2.0, cs.contiguous()


@functools.lru_cache(maxsize=None)
def mlp_case(enc, weights, family, rows, seed=0):
    """dict: inputs (float32 CPU tensors of `rows` rows), ref64 / ref32 / ref32k [rows, 256]"""
    if family not in MLP_FAMILIES:
        raise ValueError(family)
    g = _gen("mlp", enc, weights, family, rows, seed)
    inputs = _mlp_inputs(enc, family, rows, g)
    sd_t = state_dict_t(weights)[1]
    r64 = mlp4(sd_t, enc, enc_features(enc, inputs, torch.float64), torch.float64)
    f32 = enc_features(enc, inputs, torch.float32)
    return dict(kind="mlp", enc=enc, weights=weights, family=family, rows=rows, inputs=inputs, ref64=r64,
                ref32=mlp4(sd_t, enc, f32, torch.float32), ref32k=mlp4_kernel_order(sd_t, enc, f32))


def pack_mlp(case, device):
    """the case's inputs on the device with SPARE_ROWS rows of +-1e4 behind them, and the marker-filled output [rows + SPARE_ROWS, 256]"""
    g = _gen("guard", case["enc"], case["rows"])
    ins = [torch.cat([t, _sentinel((SPARE_ROWS,) + tuple(t.shape[1:]), g)]).contiguous().to(device) for t in case["inputs"]]
    out = torch.full((case["rows"] + SPARE_ROWS, 256), MARKER, dtype=torch.float32, device=device)
    return ins, out


def launch_mlp(eng, variant, word=None, line=None, max_blocks=0):
    """Runs `variant` on the word and / or line case; returns ({enc: output [rows, 256] on the CPU}, variant used) after asserting
    that the spare rows behind every output still hold the marker."""
    packed = {e: pack_mlp(c, eng.device) for e, c in (("word", word), ("line", line)) if c is not None}
    arg = lambda e, c: None if c is None else (*packed[e][0], c["rows"])
    out = lambda e: packed[e][1] if e in packed else None
    _, _, used = eng.debug_tok_mlp(variant, arg("word", word), arg("line", line), out("word"), out("line"), max_blocks)
    torch.cuda.synchronize()
    res = {}
    for e, c in (("word", word), ("line", line)):
        if c is not None:
            o = packed[e][1].cpu()
            assert bool((o[c["rows"]:] == MARKER).all()), f"{e}: rows behind the output were written"
            res[e] = o[:c["rows"]]
    return res, used


def _bar(case, sl, cols=slice(None)):
    r64, r32 = case["ref64"][sl][..., cols], case["ref32"][sl][..., cols]
    own = (r32.double() - r64).abs().max().item()
    if (case["kind"], case["family"]) in KERNEL_ORDER:
        own = max(own, (case["ref32k"][sl][..., cols].double() - r64).abs().max().item())
    return FACTOR * max(own, 2.0 ** -23 * r64.abs().max().item())


def tile_errors(got, case, ref=None):
    """[(first row of the 64-row tile, rows in it, max |got - ref64|, bar)]; `ref`: compare with this tensor instead (cross-variant
    agreement), the bar stays the references' own"""
    want = case["ref64"] if ref is None else ref.double()
    rows = []
    for a in range(0, case["rows"], 64):
        sl = slice(a, min(a + 64, case["rows"]))
        rows.append((a, sl.stop - a, (got[sl].double() - want[sl]).abs().max().item(), _bar(case, sl)))
    return rows


# =================================================================================================================================
# CLS pooling
# =================================================================================================================================

POOL_T = (1, 2, 3, 4, 5, 21, 41, 62, 63, 64, 65, 66, 67, 68, 127, 128, 129, 200)
POOL_N = (1, 2, 3, 4, 5, 7, 8, 9, 33)
POOL_FAMILIES = ("normal", "peaky", "planted", "equal", "border", "sentinel")
POOL_KERNELS = ("cls_pool", "cls_pool_online", "cls_pool_online_reverse", "cls_pool_online_split4")
MAPS = ((1, 1), (7, 9), (8, 8), (5, 13), (60, 80))           # Hc x Wc: P = 1, 63, 64, 65, 4800


def n_valid_list(T):
    return sorted({1, min(2, T), max(T - 1, 1), T})


def layout(T, N, n_images=1, empty=None):
    """Key-lines [(image, n_tok)] of N sub-lines in all: 1, 2 and 5 sub-lines per key-line in turn (as far as N allows), the last
    sub-line of a key-line holding n_valid = 1, 2, T - 1, T real tokens in turn; spread over n_images images in order, `empty`
    ('first' / 'mid' / 'last' / None) naming the image that gets no line."""
    lines, left, i = [], N, 0
    nv = n_valid_list(T)
    while left > 0:
        n_sub = min((1, 2, 5)[i % 3], left)
        lines.append((n_sub - 1) * T + nv[i % len(nv)])
        left -= n_sub
        i += 1
    imgs = [k for k in range(n_images) if k != {"first": 0, "mid": n_images // 2, "last": n_images - 1, None: -1}[empty]]
    return tuple((imgs[min(j * len(imgs) // len(lines), len(imgs) - 1)], n) for j, n in enumerate(lines))


def pool_shapes():
    """(T, N, n_images, empty) of every pooling case: all T at N = 9 (key-lines of 1, 2, 5 and 1 sub-lines, all four n_valid), and
    all N over 1-4 images, with and without an empty image, at one T below and one above the 64-token chunk"""
    s = [(T, 9, 1 + i % 2, None) for i, T in enumerate(POOL_T)]
    for T in (21, 65):
        for i, N in enumerate(POOL_N):
            n_img = 1 + (i + T) % 4
            s.append((T, N, n_img, (None, "first", "mid", "last")[i % 4] if n_img > 1 else None))
    s += [(5, 33, 4, "mid"), (66, 7, 3, "first"), (66, 5, 2, "last")]
    return tuple(s)


def _pool_consts(sd_t, dtype):
    n = 0
    while f"klenc.desc_layers.{n}.slf_attn.fc.weight" in sd_t:
        n += 1
    p = f"klenc.desc_layers.{n - 1}.slf_attn."
    c = lambda k: sd_t[k].to(dtype)
    cls = c("klenc.cls_token").reshape(256)
    W5 = c(ENC["word"] + ".12.weight")[:, :, 0]
    q = (F.linear(cls, c(p + "w_qs.weight"), c(p + "w_qs.bias")) / 8.0).view(4, 64)
    return dict(cls=cls, W5=W5, b5=c(ENC["word"] + ".12.bias"), q=q, Wk=c(p + "w_ks.weight"), bk=c(p + "w_ks.bias"),
                Wv=c(p + "w_vs.weight"), bv=c(p + "w_vs.bias"))


def pool_scores(sd_t, desc, a4, dtype):
    """(scores [rows, 4] of token rows x_j = desc_j + W5 a4_j + b5, scores [4] of the CLS key): q_h . (Wk_h x + bk_h)"""
    k = _pool_consts(sd_t, dtype)
    x = desc.to(dtype) + F.linear(a4.to(dtype), k["W5"], k["b5"])
    s = torch.einsum("rhd,hd->rh", F.linear(x, k["Wk"], k["bk"]).view(-1, 4, 64), k["q"])
    s0 = torch.einsum("hd,hd->h", F.linear(k["cls"], k["Wk"], k["bk"]).view(4, 64), k["q"])
    return s, s0


def pool_reference(sd_t, desc, a4, keys, dtype):
    """pooled [N, 4, 544] in `dtype`.  desc, a4: [rows, 256]; keys [N, T]: the row of every token slot of every sub-line (a padding
    slot names its image's padding row, so it enters the softmax once per slot, as in the reference's dense tensors)"""
    s, s0 = pool_scores(sd_t, desc, a4, dtype)
    N = keys.shape[0]
    p = torch.softmax(torch.cat([s0.expand(N, 1, 4), s[keys]], dim=1), dim=1)            # [N, T + 1, 4]
    out = torch.zeros((N, 4, POOLW), dtype=dtype)
    out[:, :, :256] = torch.einsum("nth,ntc->nhc", p[:, 1:], desc.to(dtype)[keys])
    out[:, :, 256:512] = torch.einsum("nth,ntc->nhc", p[:, 1:], a4.to(dtype)[keys])
    out[:, :, 512] = p[:, 0]
    return out


def pool_reference_kernel_order(sd_t, desc, a4, keys, first_pad):
    """float32 in the online kernels' operation order (lt_model.h): the score in its folded form u_h . desc_j + (W5^T u_h) . a4_j +
    const_h -- u_h = Wk_h^T q_h and the constants derived HERE from the state dict in float64 and rounded once, as linetr_create does
    --, the softmax in the log2 domain in one pass with a running maximum and rescaled sums, the image's padding key once with its
    multiplicity, one reciprocal at the end"""
    k = _pool_consts(sd_t, torch.float64)
    U = torch.einsum("hd,hdc->hc", k["q"], k["Wk"].view(4, 64, 256))
    c = torch.einsum("hd,hd->h", k["q"], k["bk"].view(4, 64))
    U2, c_tok, s_cls, U = (U @ k["W5"]).float(), (U @ k["b5"] + c).float(), (U @ k["cls"] + c).float(), U.float()
    LOG2E = torch.tensor(1.44269504088896340736, dtype=torch.float32)
    sh_all = ((desc @ U.t() + a4 @ U2.t()) + c_tok) * LOG2E                              # [rows, 4]
    N, T = keys.shape
    nv = (keys < first_pad).sum(dim=1)                                                   # real tokens; the rest name the padding row
    m = (s_cls * LOG2E).expand(N, 4).clone()
    l, w0 = torch.ones((N, 4)), torch.ones((N, 4))
    d, a = torch.zeros((N, 4, 256)), torch.zeros((N, 4, 256))
    for t in range(T):
        mult = torch.where(t < nv, 1.0, torch.where(t == nv, (T - nv).float(), 0.0))   # the padding key once, T - nv fold
        live = (mult > 0)[:, None]
        sh = sh_all[keys[:, t]]
        mn = torch.where(live, torch.maximum(m, sh), m)
        al = torch.exp2(m - mn)
        e = torch.exp2(sh - mn) * mult[:, None]
        l, w0 = l * al + e, w0 * al
        d = d * al[:, :, None] + e[:, :, None] * desc[keys[:, t]][:, None, :]
        a = a * al[:, :, None] + e[:, :, None] * a4[keys[:, t]][:, None, :]
        m = mn
    inv = 1.0 / l
    out = torch.zeros((N, 4, POOLW))
    out[:, :, :256], out[:, :, 256:512], out[:, :, 512] = d * inv[:, :, None], a * inv[:, :, None], w0 * inv
    return out


def sample_rows(cpnt, row_image, dense_nchw, align_corners):
    """desc [rows, 256]: oracle.linetr_oracle.sample_token_desc of every row's coordinate in its image's map, float32"""
    desc = torch.zeros((cpnt.shape[0], 256))
    for i in range(dense_nchw.shape[0]):
        sel = (row_image == i).nonzero()[:, 0]
        if len(sel):
            d = O.sample_token_desc(cpnt[sel].view(1, -1, 1, 2), dense_nchw[i:i + 1], 8, bool(align_corners))
            desc[sel] = d[0].t()
    return desc


@functools.lru_cache(maxsize=None)
def dense_base(n_images, hw_cells, constant=False):
    """the unit-norm NCHW maps every case of this shape shares ('equal': one unit vector in every cell)"""
    g = _gen("map", n_images, hw_cells, constant)
    Hc, Wc = hw_cells
    if constant:
        return F.normalize(torch.randn((1, 256, 1, 1), generator=g), p=2, dim=1).expand(n_images, 256, Hc, Wc).contiguous()
    return F.normalize(torch.randn((n_images, 256, Hc, Wc), generator=g), p=2, dim=1)


def dense_of(case):
    """the case's NCHW maps [n_images, 256, Hc, Wc]: the shared ones, the sentinel images overwritten with +-1e4"""
    dense = dense_base(case["n_images"], (case["Hc"], case["Wc"]), case["family"] == "equal")
    if case["sentinel_images"]:
        dense = dense.clone()
        for i in case["sentinel_images"]:
            dense[i] = _sentinel((256, case["Hc"], case["Wc"]), _gen("sentinel map", case["T"], case["N"], i))
    return dense


@functools.lru_cache(maxsize=160)
def pool_case(family, T, N, n_images=1, empty=None, weights="calibrated", hw_cells=(60, 80), align_corners=False, parity=0, seed=0):
    """One batch for the pooling kernels.  dict with the online kernels' operands (recs, sub2line, cpnt, a4, first_pad; the NCHW
    maps come from dense_of(case)), keys [N, T], ref64 / ref32 / ref32k [N, 4, 544] and `check`, the sub-lines that are compared.  Families:
      normal    a4 = ref32 of the word encoder's MLP on the tokens' coordinates and uniform scores
      peaky     the same scaled so that |score| reaches about 20
      planted   per (sub-line, head) one key leads the rest by 30 -- the first token, the last real token, token 63 / 64 / 65
                (where the sub-line has it) in turn; in every image one head has the image's shared padding key lifted instead, or,
                in every third image, nobody: all its keys 30 below CLS -- by adding multiples of the float64 directions
                W5^T Wk_h^T q_h to the a4 rows; every a4 row carries a marker of 4 in a channel that depends on the row
      equal     a4 = 0 and a constant map: every key has the same score, dbar = (1 - p_0) x the map's unit vector, abar = 0
      border    coordinates at 0, 0.5, 3.4, 3.6 and the clip limits in both axes: one to three taps outside the map
      sentinel  'normal' in the images whose index has not `parity`; the others hold +-1e4 in map, a4 rows and coordinates"""
    if family not in POOL_FAMILIES:
        raise ValueError(family)
    g = _gen("pool", family, T, N, n_images, empty, weights, hw_cells, align_corners, parity, seed)
    sd_t = state_dict_t(weights)[1]
    Hc, Wc = hw_cells
    lines = layout(T, N, n_images, empty)
    K = len(lines)
    recs = np.zeros(K, dtype=nat.REC_DTYPE)
    sub2line, keys, row_image = [], [], []
    n_real = sum(n for _, n in lines)
    first_pad = n_real
    sub = tok = 0
    local = {}
    for k, (img, n_tok) in enumerate(lines):
        n_sub = -(-n_tok // T)
        recs[k]["first_sub"], recs[k]["n_tok"], recs[k]["n_sub"], recs[k]["image"] = sub, n_tok, n_sub, img
        recs[k]["first_tok"], recs[k]["line_local"] = tok, local.get(img, 0)
        local[img] = local.get(img, 0) + 1
        for j in range(n_sub):
            nv = min(T, n_tok - j * T)
            keys.append(list(range(tok + j * T, tok + j * T + nv)) + [first_pad + img] * (T - nv))
            sub2line.append(k)
        row_image += [img] * n_tok
        sub += n_sub
        tok += n_tok
    assert sub == N
    row_image = torch.tensor(row_image + list(range(n_images)))
    keys = torch.tensor(keys, dtype=torch.long)
    rows = n_real + n_images
    lim = torch.tensor([8.0 * Wc - 0.6, 8.0 * Hc - 0.6])
    if family == "border":
        vx = torch.tensor([0.0, 0.5, 3.4, 3.6, float(lim[0])]); vy = torch.tensor([0.0, 0.5, 3.4, 3.6, float(lim[1])])
        cpnt = torch.stack([vx[torch.randint(0, 5, (rows,), generator=g)], vy[torch.randint(0, 5, (rows,), generator=g)]], dim=1)
    else:
        cpnt = torch.rand((rows, 2), generator=g) * lim
    cpnt[n_real:] = 0.0                                                                  # the padding token sits at (0, 0)
    dense = dense_base(n_images, hw_cells, family == "equal")
    desc = sample_rows(cpnt, row_image, dense, align_corners)
    feats = enc_features("word", (cpnt * torch.tensor([HW[1] / lim[0], HW[0] / lim[1]]), torch.rand((rows,), generator=g)), torch.float32)
    a4 = mlp4(sd_t, "word", feats, torch.float32)
    if family == "equal":
        a4 = torch.zeros_like(a4)
    elif family in ("peaky", "planted"):
        k64 = _pool_consts(sd_t, torch.float64)
        dirs = torch.einsum("hd,hdc->hc", k64["q"], k64["Wk"].view(4, 64, 256)) @ k64["W5"]        # [4, 256]: d score_h / d a4
        if family == "peaky":
            a4 = a4 * float(20.0 / (a4.double() @ dirs.t()).abs().max())
        else:
            a4 = 0.1 * a4
            a4[torch.arange(rows), (3 * torch.arange(rows) + 1) % 256] += 4.0
            s, s0 = pool_scores(sd_t, desc, a4, torch.float64)
            lift = torch.zeros((rows, 4), dtype=torch.float64)
            salt = T + N
            plan = {}                                                                    # (sub-line, head) -> planted row or None
            for img in range(n_images):
                subs = [n for n in range(N) if int(recs[sub2line[n]]["image"]) == img]
                if not subs:
                    continue
                hp, nobody = (img + salt) % 4, (img + salt) % 3 == 2
                mine = torch.unique(keys[subs])
                top = torch.maximum(s[mine].max(dim=0).values, s0)
                if nobody:
                    lift[mine, hp] = (s0[hp] - 30.0) - s[mine, hp]
                else:
                    lift[first_pad + img, hp] = top[hp] + 30.0 - s[first_pad + img, hp]
                for n in subs:
                    nv = int((keys[n] < first_pad).sum())
                    for h in range(4):
                        if h == hp:
                            plan[(n, h)] = None if nobody or nv == T else first_pad + img
                            continue
                        want = (0, nv - 1, 63, 64, 65)[(n + h + salt) % 5]
                        r = int(keys[n, want if want < nv else want % nv])
                        lift[r, h] = top[h] + 30.0 - s[r, h]
                        plan[(n, h)] = r
            gram = dirs @ dirs.t()
            a4 = (a4.double() + torch.linalg.solve(gram, lift.t()).t() @ dirs).float()
    check, bad_img = list(range(N)), []
    if family == "sentinel":
        bad_img = [i for i in range(n_images) if i % 2 == parity]
        check = [n for n in range(N) if int(recs[sub2line[n]]["image"]) not in bad_img]
        for i in bad_img:                                   # (their rows are compared nowhere: desc is what the dense kernel is handed)
            sel = row_image == i
            cpnt[sel] = _sentinel((int(sel.sum()), 2), g)
            a4[sel] = _sentinel((int(sel.sum()), 256), g)
            desc[sel] = _sentinel((int(sel.sum()), 256), g)
    case = dict(kind="pool", family=family, T=T, N=N, K=K, n_images=n_images, weights=weights, Hc=Hc, Wc=Wc, align_corners=bool(align_corners),
                recs=recs, sub2line=np.asarray(sub2line, dtype=np.int32), keys=keys, cpnt=cpnt.contiguous(), a4=a4.contiguous(),
                desc=desc, sentinel_images=tuple(bad_img), first_pad=first_pad, check=check, lines=lines)
    if family == "planted":
        case["plan"] = plan
    sel = torch.tensor(check, dtype=torch.long)
    for name, fn in (("ref64", lambda k: pool_reference(sd_t, desc, a4, k, torch.float64)),
                     ("ref32", lambda k: pool_reference(sd_t, desc, a4, k, torch.float32)),
                     ("ref32k", lambda k: pool_reference_kernel_order(sd_t, desc, a4, k, first_pad) if ("pool", family) in KERNEL_ORDER else None)):
        r = fn(keys[sel]) if len(check) else None
        full = None
        if r is not None:
            full = torch.zeros((N, 4, POOLW), dtype=r.dtype)
            full[sel] = r
        case[name] = full
    return case


def launch_pool(eng, kernel, case, nhwc=True):
    """Runs pooling kernel `kernel` (0: on the densely expanded case) on the case; returns (pooled [N, 4, 544] on the CPU, kernel
    used) after asserting that the SPARE_ROWS rows behind the output still hold the marker.  The a4 rows and coordinates carry
    SPARE_ROWS rows of +-1e4 behind the batch's."""
    N, T, dev = case["N"], case["T"], eng.device
    g = _gen("guard", N, T)
    out = torch.full((N + SPARE_ROWS, 4, POOLW), MARKER, dtype=torch.float32, device=dev)
    if kernel == 0:
        flat = case["keys"].reshape(-1)
        a4 = torch.cat([case["a4"][flat], _sentinel((SPARE_ROWS, 256), g)]).to(dev)
        dd = torch.cat([case["desc"][flat], _sentinel((SPARE_ROWS, 256), g)]).to(dev)
        _, used = eng.debug_cls_pool(0, a4, out, N, T, desc_dense=dd)
    else:
        a4 = torch.cat([case["a4"], _sentinel((SPARE_ROWS, 256), g)]).to(dev)
        cp = torch.cat([case["cpnt"], _sentinel((SPARE_ROWS, 2), g)]).to(dev)
        m = dense_of(case) if not nhwc else dense_of(case).permute(0, 2, 3, 1).contiguous()
        recs = torch.from_numpy(case["recs"].view(np.uint8).copy()).to(dev)
        _, used = eng.debug_cls_pool(kernel, a4, out, N, T, recs=recs, sub2line=torch.from_numpy(case["sub2line"]).to(dev), cpnt=cp,
                                     first_pad=case["first_pad"], n_images=case["n_images"], dense_map=m.to(dev), nhwc=nhwc,
                                     Hc=case["Hc"], Wc=case["Wc"], align_corners=case["align_corners"])
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[N:] == MARKER).all()), "rows behind the output were written"
    return o[:N], used


def subline_errors(got, case, ref=None):
    """[(sub-line, 'vec' | 'p0', max |got - ref64|, bar)] for every compared sub-line: its 4 x 512 vector columns and its four CLS
    weights separately, so that the vectors do not set the scale of p_0.  The 31 columns behind p_0 must be exactly zero (reported
    as an error against a bar of 0 otherwise)."""
    want = case["ref64"] if ref is None else ref.double()
    rows = []
    for n in case["check"]:
        sl = slice(n, n + 1)
        for what, cols in (("vec", slice(0, 512)), ("p0", slice(512, 513))):
            rows.append((n, what, (got[sl][..., cols].double() - want[sl][..., cols]).abs().max().item(), _bar(case, sl, cols)))
        z = got[n, :, 513:].abs().max().item()
        if z != 0.0:
            rows.append((n, "zeros", z, 0.0))
    return rows


def failures(rows, what="unit"):
    return [f"{what} {a} ({n}): error {e:.3e} > bar {b:.3e} (x{e / b if b else float('inf'):.1f})" for a, n, e, b in rows if not e <= b]
