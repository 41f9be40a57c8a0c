"""The two positional encoders, KeylineEncoder and the whole LineTransformer of the reference (models/line_transformer.py:9-130, :185-249) and
the two kernel pairs their native backward adds (csrc/lt_posbwd.h), stated from the formulas: float64 closed forms in NumPy (the references of
tests/test_gpu_keyline.py), a restatement of the modules in stock torch with the reference's state_dict names (what autograd differentiates:
its float32 error is the bar), the seeded cases, the bar and the launch helpers the tests and tools/keyline_report.py share.  Imports nothing
of the package (the descriptive layer and the signature stack come from desc_layer_reference.py and sig_layer_reference.py).  Test
infrastructure only.

    input layer     z = x W^T + b     dW = g^T x     db = sum_r g                                  x [rows, Kin], W [N, Kin], g [rows, N]
    token assembly  x[l, 0] = cls     x[l, 1 + t] = desc[l, t] + pos[l, t]     dtok = dx[:, 1:]     dcls = sum_l dx[l, 0]

The bar of a tensor, in the project's form:  max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|); ref32 = float32 autograd on
the CPU, so the bar is a property of the references alone."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import desc_layer_reference as DL
import sig_layer_reference as SL

FACTOR = 8
D = 256
SENTINEL = 1.0e4          # magnitude of everything a kernel must not read into a result (finite: a leak shows as a huge error, not NaN)
MARKER = -777.25          # what an output buffer holds before the launch
SPARE_ROWS = 8            # sentinel rows behind the last row of an input

bar_of, ratios, failures, worst = DL.bar_of, DL.ratios, DL.failures, DL.worst


def _rs(*key):
    """a RandomState seeded by the key's text (stable from process to process, unlike hash())"""
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def _sentinels(rs, shape):
    return (SENTINEL * (rs.randint(0, 2, shape) * 2 - 1)).astype(np.float32)


def _np64(t):
    return t.detach().double().cpu().numpy()


# ---- the encoders' input layer -----------------------------------------------------------------------------------------------------

IL_OUTPUTS = ("z", "dW", "db")
IL_KIN = (1, 3, 5, 8)
IL_N = (4, 32, 64)


def il_rows(chunk):
    """the row counts at which the weight-gradient reduction of chunks of `chunk` rows can go wrong"""
    return (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 3)


def il_closed_form(x, W, b, g, mistake=None):
    """float64.  x [rows, Kin], W [N, Kin], b [N], g [rows, N] -> dict z [rows, N], dW [N, Kin], db [N].
    mistake 'db_mean': the bias gradient averaged over the rows instead of summed (a planted error for the CPU suite)"""
    x, W, b, g = (np.asarray(a, np.float64) for a in (x, W, b, g))
    return {"z": x @ W.T + b, "dW": g.T @ x, "db": g.mean(axis=0) if mistake == "db_mean" else g.sum(axis=0)}


def il_torch(x, W, b, g, dtype):
    """autograd through F.linear on the CPU at `dtype`: dict of float64 arrays like il_closed_form"""
    Wt, bt = (torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (W, b))
    with torch.enable_grad():
        z = F.linear(torch.tensor(np.asarray(x), dtype=dtype), Wt, bt)
        z.backward(torch.tensor(np.asarray(g), dtype=dtype))
    return {"z": _np64(z), "dW": _np64(Wt.grad), "db": _np64(bt.grad)}


@functools.lru_cache(maxsize=None)
def il_case(Kin, N, rows, integer=False, seed=0):
    """x [rows, Kin], W [N, Kin], b [N], g [rows, N] float32 with ref64 (the closed form) and ref32 (float32 autograd).  `integer`: small
    integers everywhere, so that every product and sum is exact in float32 whatever its order.  The arrays are shared: do not write."""
    rs = _rs("input layer", Kin, N, rows, integer, seed)
    if integer:
        x, W, b, g = (rs.randint(-4, 5, s).astype(np.float32) for s in ((rows, Kin), (N, Kin), (N,), (rows, N)))
    else:
        x = rs.uniform(-1, 1, (rows, Kin)).astype(np.float32)
        W = (rs.standard_normal((N, Kin)) / np.sqrt(Kin)).astype(np.float32)
        b = rs.uniform(-0.5, 0.5, N).astype(np.float32)
        g = rs.standard_normal((rows, N)).astype(np.float32)
    return dict(Kin=Kin, N=N, rows=rows, x=x, W=W, b=b, g=g, ref64=il_closed_form(x, W, b, g), ref32=il_torch(x, W, b, g, torch.float32))


# ---- the token assembly ------------------------------------------------------------------------------------------------------------

TA_OUTPUTS = ("x", "dtok", "dcls")
TA_FAMILIES = ("normal", "integer", "sentinel")
TA_S = (1, 2, 21, 41, 255)


def ta_segments(per_block):
    """the segment counts around a block of `per_block` segments, and three blocks with a ragged last one"""
    return (per_block - 1, per_block, per_block + 1, 2 * per_block + 3)


def ta_closed_form(desc, pos, cls, dx, mistake=None):
    """float64.  desc, pos [L, S, 256], cls [256], dx [L, S + 1, 256] -> dict x [L, S + 1, 256], dtok [L, S, 256], dcls [256].
    mistake 'dcls_all_slots': the cls gradient summed over every slot, not slot 0 alone (a planted error)"""
    desc, pos, cls, dx = (np.asarray(a, np.float64) for a in (desc, pos, cls, dx))
    x = np.concatenate([np.broadcast_to(cls, (desc.shape[0], 1, D)), desc + pos], axis=1)
    return {"x": x, "dtok": dx[:, 1:].copy(), "dcls": dx.sum(axis=(0, 1)) if mistake == "dcls_all_slots" else dx[:, 0].sum(axis=0)}


def ta_torch(desc, pos, cls, dx, dtype):
    """autograd through cat(cls, desc + pos) on the CPU at `dtype`; dtok is the gradient of desc (and of pos: asserted equal)"""
    dt, pt, ct = (torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (desc, pos, cls))
    with torch.enable_grad():
        x = torch.cat([ct.view(1, 1, D).expand(dt.shape[0], 1, D), dt + pt], dim=1)
        x.backward(torch.tensor(np.asarray(dx), dtype=dtype))
    assert torch.equal(dt.grad, pt.grad)
    return {"x": _np64(x), "dtok": _np64(dt.grad), "dcls": _np64(ct.grad)}


@functools.lru_cache(maxsize=None)
def ta_case(family, L, S, seed=0):
    """desc, pos [L, S, 256], cls [256], dx [L, S + 1, 256] float32 with ref64 / ref32.  'normal': unit normal.  'integer': small integers
    in dx (every sum exact).  'sentinel': the token slots of dx hold +-1e4 (none of it may reach dcls), its CLS slots unit normal."""
    rs = _rs("token assembly", family, L, S, seed)
    desc, pos = (rs.standard_normal((L, S, D)).astype(np.float32) for _ in range(2))
    cls = rs.standard_normal(D).astype(np.float32)
    dx = rs.standard_normal((L, S + 1, D)).astype(np.float32)
    if family == "integer":
        dx = rs.randint(-4, 5, (L, S + 1, D)).astype(np.float32)
    elif family == "sentinel":
        dx[:, 1:] = _sentinels(rs, (L, S, D))
    else:
        assert family == "normal", family
    return dict(family=family, L=L, S=S, desc=desc, pos=pos, cls=cls, dx=dx, ref64=ta_closed_form(desc, pos, cls, dx),
                ref32=ta_torch(desc, pos, cls, dx, torch.float32))


# ---- the modules, restated ---------------------------------------------------------------------------------------------------------

ENCODER_WIDTHS = (32, 64, 128, 256, 256)
IMAGE_SHAPE = (480, 640)
SIG_LAYERS = 7
INPUT_KEYS = ("sublines", "resp_sublines", "angle_sublines", "pnt_sublines", "desc_sublines", "score_sublines", "mask_sublines", "klines")


def mlp(channels):
    """Conv1d(k = 1) -> BatchNorm1d -> ReLU per layer, the last one a bare Conv1d (the reference's MLP, :9-20)"""
    layers = []
    for i in range(1, len(channels)):
        layers.append(nn.Conv1d(channels[i - 1], channels[i], 1))
        if i < len(channels) - 1:
            layers += [nn.BatchNorm1d(channels[i]), nn.ReLU()]
    return nn.Sequential(*layers)


class LineEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = mlp((5,) + ENCODER_WIDTHS)

    def forward(self, klines, resp, angle):
        mid = (klines[:, :, 0] + klines[:, :, 1]) / 2.
        return self.encoder(torch.cat([mid, resp, angle], dim=2).transpose(1, 2))


class WordEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = mlp((3,) + ENCODER_WIDTHS)

    def forward(self, pnt, score):
        B, n, S = pnt.shape[:3]
        x = torch.cat([pnt, score], dim=-1).transpose(-2, -1).reshape(B * n, 3, S)
        return self.encoder(x).transpose(-1, -2).reshape(B, n, S, D)


class Klenc(nn.Module):
    """KeylineEncoder (:93-130) with one descriptive layer (desc_layer_reference.Layer: all S + 1 query rows)"""

    def __init__(self):
        super().__init__()
        self.line_position_enc, self.word_position_enc = LineEncoder(), WordEncoder()
        self.desc_layers = nn.ModuleList([DL.Layer()])
        self.cls_token = nn.Parameter(torch.zeros(1, 1, 1, D))

    def forward(self, klines, resp, angle, pnt, desc, score, mask=None, mistake=None):
        B, n = desc.shape[:2]
        tokens = desc if mistake == "no_word_position" else desc + self.word_position_enc(pnt, score)
        tokens = torch.cat([self.cls_token.expand(B, n, 1, D), tokens], dim=2)
        return self.line_position_enc(klines, resp, angle) + self.desc_layers[0](tokens, mask)[:, :, 0].transpose(1, 2)


def normalize(klines, pnt, image_shape=IMAGE_SHAPE):
    """(x - centre) / (0.7 max(width, height)) on the end points and on the tokens (:22-38)"""
    size = klines.new_tensor([float(image_shape[1]), float(image_shape[0])])
    return (klines - size / 2) / (size.max() * 0.7), (pnt - size / 2) / (size.max() * 0.7)


class Model(nn.Module):
    """LineTransformer.forward (:225-249) on the reference's input dict; mistake 'no_word_position': desc without its positional sum"""

    def __init__(self, n_layers=SIG_LAYERS):
        super().__init__()
        self.klenc, self.selfattn, self.final_proj = Klenc(), SL.Stack(n_layers), nn.Conv1d(D, D, 1)

    def forward(self, data, mistake=None):
        klines, pnt = normalize(data["sublines"], data["pnt_sublines"])
        s = self.klenc(klines, data["resp_sublines"], data["angle_sublines"], pnt, data["desc_sublines"], data["score_sublines"],
                       data["mask_sublines"], mistake)
        return F.normalize(self.final_proj(self.selfattn(s)), p=2, dim=1)


def encoder_state_dict(rs, n_in, out_scale=1.0):
    """an encoder's state dict (keys encoder.<i>.*) drawn from `rs`: weights N(0, 1 / K), biases in (-0.5, 0.5) -- the last one too, which the
    reference initialises to 0 --, BatchNorm weights in (0.5, 1.5), biases N(0, 0.3^2), running statistics away from 0 and 1"""
    sd, widths = {}, (n_in,) + ENCODER_WIDTHS
    for j in range(1, len(widths)):
        i, last = 3 * (j - 1), j == len(widths) - 1
        scale = out_scale if last else 1.0
        sd[f"encoder.{i}.weight"] = (scale * rs.standard_normal((widths[j], widths[j - 1], 1)) / np.sqrt(widths[j - 1])).astype(np.float32)
        sd[f"encoder.{i}.bias"] = (scale * rs.uniform(-0.5, 0.5, widths[j])).astype(np.float32)
        if not last:
            sd[f"encoder.{i + 1}.weight"] = rs.uniform(0.5, 1.5, widths[j]).astype(np.float32)
            sd[f"encoder.{i + 1}.bias"] = (0.3 * rs.standard_normal(widths[j])).astype(np.float32)
            sd[f"encoder.{i + 1}.running_mean"] = (0.3 * rs.standard_normal(widths[j])).astype(np.float32)
            sd[f"encoder.{i + 1}.running_var"] = rs.uniform(0.5, 1.5, widths[j]).astype(np.float32)
            sd[f"encoder.{i + 1}.num_batches_tracked"] = np.array(0, dtype=np.int64)
    return sd


def model_state_dict(rs, n_layers=SIG_LAYERS):
    """the whole model's state dict under the reference's names.  The signature layers' last convolutions are drawn eight times smaller
    than sig_layer_reference draws them (seven residual layers keep the features' scale), the head as its network_case draws it."""
    sd = {f"klenc.line_position_enc.{k}": v for k, v in encoder_state_dict(rs, 5).items()}
    sd.update({f"klenc.word_position_enc.{k}": v for k, v in encoder_state_dict(rs, 3).items()})
    sd.update({f"klenc.desc_layers.0.{k}": v for k, v in DL.state_dict(rs).items()})
    sd["klenc.cls_token"] = rs.standard_normal((1, 1, 1, D)).astype(np.float32)
    for k, v in SL.stack_state_dict(rs, n_layers).items():
        sd[f"selfattn.{k}"] = (v / 8).astype(np.float32) if ".mlp.3." in k else v
    sd["final_proj.weight"] = (rs.standard_normal((D, D, 1)) / 16).astype(np.float32)
    sd["final_proj.bias"] = rs.uniform(-0.05, 0.05, D).astype(np.float32)
    return sd


def model_inputs(rs, B, n, S):
    """the reference's input dict as float32 / NumPy: pixel coordinates inside a 480 x 640 image, scores and responses in (0, 1), unit
    angle vectors, unit-normal token descriptors, a mask of ones"""
    wh = np.array([IMAGE_SHAPE[1], IMAGE_SHAPE[0]], np.float64)
    ang = rs.uniform(0, 2 * np.pi, (B, n))
    return {"sublines": (rs.uniform(0, 1, (B, n, 2, 2)) * wh).astype(np.float32), "resp_sublines": rs.uniform(0, 1, (B, n, 1)).astype(np.float32),
            "angle_sublines": np.stack([np.cos(ang), np.sin(ang)], axis=2).astype(np.float32),
            "pnt_sublines": (rs.uniform(0, 1, (B, n, S, 2)) * wh).astype(np.float32),
            "desc_sublines": rs.standard_normal((B, n, S, D)).astype(np.float32),
            "score_sublines": rs.uniform(0, 1, (B, n, S, 1)).astype(np.float32),
            "mask_sublines": np.ones((B, n, S + 1, S + 1), np.float32), "klines": np.zeros((B, n, 2, 2), np.float32)}


def tensors(sd, dtype=None, device="cpu"):
    return {k: v.to(device) for k, v in SL.tensors(sd, dtype).items()}


def data_tensors(inputs, dtype=torch.float32, device="cpu", grad=True):
    data = {k: torch.tensor(v, dtype=dtype, device=device) for k, v in inputs.items()}
    data["desc_sublines"].requires_grad_(grad)
    return data


def collect(module, out, prefix=""):
    """gradients of every parameter, and the buffers after the call, under their state_dict names"""
    for key, p in module.named_parameters():
        out[prefix + key] = _np64(p.grad) if p.grad is not None else np.zeros(tuple(p.shape))
    for key, b in module.named_buffers():
        out[prefix + "after." + key] = b.detach().cpu().numpy().astype(np.float64 if b.is_floating_point() else np.int64)
    return out


# -- an encoder alone

ENCODER_SHAPES = {"line": ((1, 2), (3, 129)), "word": ((1, 1, 2), (2, 33, 21))}      # two rows in all (BatchNorm's least); several blocks of every kernel


@functools.lru_cache(maxsize=None)
def encoder_case(kind, shape, seed=61):
    """(state dict, inputs (a tuple of arrays), upstream in the output's shape).

    The smallest shapes hold two rows in all, BatchNorm's least.  With two rows a channel's normalised values are +-d / sqrt(d^2 + eps)
    for the half-difference d of its two inputs, and the backward multiplies the upstream by eps / (d^2 + eps)^1.5.  Under random weights
    some of the up to 256 channels have |d| near sqrt(eps) = 0.003 against |z| of 1 .. 3: they carry the whole gradient, with the relative
    error ulp(z) / d of a difference of two roundings, so a float32 result differs from float64 by what ONE rounding happened to be (the
    float32 error of such a draw was sixty times larger on one host's CPU than on another's) and a factor of 8 between two float32
    results holds or not by chance.  (Two equal rows are no way out: every gradient in front of a BatchNorm is then zero in exact
    arithmetic, the CPU's symmetric arithmetic returns exact zeros, and the bar is 0.)  So the weights of these two cases are made so that
    the rows stay far apart in EVERY channel of every layer: the convolutions behind the first hold |w| (with positive BatchNorm weights,
    row 0's activations then exceed row 1's channel by channel, and a sum of non-negative terms does not cancel), and the first one's
    signs follow x_0 - x_1.  Then |d| is of the order of |z| everywhere, every channel contributes alike, and the case checks what it is
    there for -- every kernel at two rows, one block -- on a function float32 can evaluate."""
    rs = _rs("encoder", kind, shape, seed)
    sd = encoder_state_dict(rs, 5 if kind == "line" else 3)
    full = model_inputs(rs, shape[0], shape[1], shape[2] if kind == "word" else 1)
    klines, pnt = normalize(torch.from_numpy(full["sublines"]), torch.from_numpy(full["pnt_sublines"]))
    if kind == "line":
        inputs, out_shape = (klines.numpy(), full["resp_sublines"], full["angle_sublines"]), (shape[0], D, shape[1])
    else:
        inputs, out_shape = (pnt.numpy(), full["score_sublines"]), tuple(shape) + (D,)
    if int(np.prod(shape)) == 2:
        x = np.concatenate([(inputs[0][:, :, 0] + inputs[0][:, :, 1]) / 2] + list(inputs[1:]) if kind == "line" else inputs, axis=-1).reshape(2, -1)
        for key in [k for k in sd if k.endswith(".weight") and sd[k].ndim == 3]:
            sd[key] = np.abs(sd[key]) * (np.where(x[0] >= x[1], 1.0, -1.0).astype(np.float32)[None, :, None] if key == "encoder.0.weight" else 1.0)
    return sd, inputs, rs.standard_normal(out_shape).astype(np.float32)


def run_encoder(kind, shape, dtype, train=True, device="cpu"):
    """the restated encoder differentiated by torch at `dtype`: out, the parameter gradients, after.<buffer>"""
    sd, inputs, upstream = encoder_case(kind, shape)
    mod = (LineEncoder() if kind == "line" else WordEncoder()).to(dtype)
    mod.load_state_dict(tensors(sd, dtype), strict=True)
    mod = mod.to(device).train(train)
    with torch.enable_grad():
        out = mod(*(torch.tensor(a, dtype=dtype, device=device) for a in inputs))
        out.backward(torch.tensor(upstream, dtype=dtype, device=device))
    return collect(mod, {"out": _np64(out)})


@functools.lru_cache(maxsize=None)
def encoder_refs(kind, shape, train=True):
    return run_encoder(kind, shape, torch.float64, train), run_encoder(kind, shape, torch.float32, train)


# -- the whole model against a seeded upstream (the fixture's case)

FIXTURE_SHAPE, FIXTURE_SEED, FIXTURE_CALLS = (2, 5, 21), 83, 2


def is_matrix(key, val):
    """a weight matrix's gradient ([N, K] or [N, K, 1]), as opposed to line_desc, d_desc, the cls token's gradient and the 1-D ones"""
    return key.endswith(".weight") and np.ndim(val) >= 2


def sub_grid(key, val):
    """what the fixture keeps of a tensor: a weight matrix's sub-grid [::7, ::5], everything else in full"""
    return val[::7, ::5] if is_matrix(key, val) else val


@functools.lru_cache(maxsize=None)
def model_case(shape=FIXTURE_SHAPE, seed=FIXTURE_SEED):
    """(state dict, inputs, upstream [B, 256, n]): seeded; the defaults are what tests/golden/make_golden_keyline.py draws"""
    rs = np.random.RandomState(seed)
    sd = model_state_dict(rs)
    inputs = model_inputs(rs, *shape)
    return sd, inputs, rs.standard_normal((shape[0], D, shape[1])).astype(np.float32)


def run_calls(model, data_of, upstream, calls=FIXTURE_CALLS, forward=None):
    """`calls` times forward + backward of a model in .train() whose gradients are cleared in between (its BatchNorm buffers move on):
    dict line_desc.<c>, d_desc.<c>, <parameter>.<c> and after.<buffer>.<c> per call c"""
    out = {}
    for c in range(calls):
        model.zero_grad(set_to_none=True)
        data = data_of()
        with torch.enable_grad():
            line_desc = forward(data) if forward is not None else model(data)
            line_desc.backward(upstream)
        one = collect(model, {"line_desc": _np64(line_desc), "d_desc": _np64(data["desc_sublines"].grad)})
        out.update({f"{k}.{c}": v for k, v in one.items()})
    return out


def run_model(dtype, shape=FIXTURE_SHAPE, seed=FIXTURE_SEED, calls=FIXTURE_CALLS, device="cpu", mistake=None):
    sd, inputs, upstream = model_case(shape, seed)
    mod = Model().to(dtype)
    mod.load_state_dict(tensors(sd, dtype), strict=True)
    mod = mod.to(device).train()
    return run_calls(mod, lambda: data_tensors(inputs, dtype, device), torch.tensor(upstream, dtype=dtype, device=device), calls,
                     forward=lambda data: mod(data, mistake))


@functools.lru_cache(maxsize=None)
def model_refs(shape=FIXTURE_SHAPE, seed=FIXTURE_SEED):
    return run_model(torch.float64, shape, seed), run_model(torch.float32, shape, seed)


# -- the whole model under the criterion, on two views

LOSS_SHAPE, LOSS_SEED, LOSS_LR = (2, 33, 21), 97, 0.05


@functools.lru_cache(maxsize=None)
def loss_case():
    """(state dict, view 0, view 1, mat_assign_sublines [B, n+1, n+1]) at LOSS_SHAPE with a planted ground truth, as
    sig_layer_reference.network_case plants it: view 1 holds view 0's sub-lines in another order with noise on the token descriptors, the
    sub-lines of an item share a component, and each sub-line is matched to itself"""
    B, n, S = LOSS_SHAPE
    rs = np.random.RandomState(LOSS_SEED)
    sd = model_state_dict(rs)
    v0 = model_inputs(rs, B, n, S)
    v0["desc_sublines"] = (rs.standard_normal((B, 1, 1, D)) + 0.5 * rs.standard_normal((B, n, 1, D)) + 0.25 * v0["desc_sublines"]).astype(np.float32)
    v1 = {k: v.copy() for k, v in v0.items()}
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    for i in range(B):
        perm = rs.permutation(n)
        for k in INPUT_KEYS[:6]:
            v1[k][i] = v0[k][i][perm]
        v1["desc_sublines"][i] += 0.25 * rs.standard_normal((n, S, D)).astype(np.float32)
        assign[i, perm, np.arange(n)] = 1.0
    return sd, v0, v1, assign


def loss_of(model, d0, d1, assign):
    import loss_grad_reference as LG
    loss, _, _, V = LG.torch_criterion(model(d0), model(d1), assign)
    return loss, V


def run_loss(dtype, device="cpu", sgd_lr=None):
    """loss.backward() through the model on both views at `dtype`.  dict: loss, V, d_desc0, d_desc1, every parameter's gradient; with
    `sgd_lr` also after.<buffer>, and loss_eval / line_desc_eval: an .eval() forward of view 0 after one plain SGD step"""
    sd, v0, v1, assign = loss_case()
    mod = Model().to(dtype)
    mod.load_state_dict(tensors(sd, dtype), strict=True)
    mod = mod.to(device).train()
    d0, d1 = data_tensors(v0, dtype, device), data_tensors(v1, dtype, device)
    at = torch.tensor(assign, dtype=dtype, device=device)
    with torch.enable_grad():
        loss, V = loss_of(mod, d0, d1, at)
        loss.backward()
    out = {"loss": float(loss.detach()), "V": int(V), "d_desc0": _np64(d0["desc_sublines"].grad), "d_desc1": _np64(d1["desc_sublines"].grad)}
    for key, p in mod.named_parameters():
        out[key] = _np64(p.grad)
    if sgd_lr is not None:
        with torch.no_grad():
            for p in mod.parameters():
                p -= sgd_lr * p.grad
            mod.eval()
            out["line_desc_eval"] = _np64(mod(data_tensors(v0, dtype, device, grad=False)))
    return out


@functools.lru_cache(maxsize=None)
def loss_refs():
    return run_loss(torch.float64, sgd_lr=LOSS_LR), run_loss(torch.float32, sgd_lr=LOSS_LR)


# ---- launching (GPU) ---------------------------------------------------------------------------------------------------------------

def _stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_ptr = lambda t: t.data_ptr() if t is not None else None
_out, _take = DL._out, DL._take


def il_launch(lib, c, ldx=None, ld=None, need=(True, True), shift=1, device="cuda:0"):
    """The raw input-layer entry points on an il_case: forward, then backward.  x sits in a buffer of row stride `ldx` (default Kin + 3)
    that starts `shift` floats behind a 16-byte boundary, with +-1e4 sentinels beside, in front of and behind its rows; z and g have the
    row stride `ld` (default N), g with sentinels, every output is filled with a marker.  Returns a dict of CPU arrays z, dW, db."""
    rows, N, Kin = c["rows"], c["N"], c["Kin"]
    ldx, ld = Kin + 3 if ldx is None else ldx, N if ld is None else ld
    rs = _rs("il launch", ldx, ld)
    xb = _sentinels(rs, (shift + (rows + SPARE_ROWS) * ldx,))
    xb[shift:shift + rows * ldx].reshape(rows, ldx)[:, :Kin] = c["x"]
    xb = torch.from_numpy(xb).to(device)
    x = xb[shift:]
    g = DL._inp(c["g"], ld, rs, device)
    W, b = torch.from_numpy(c["W"]).to(device), torch.from_numpy(c["b"]).to(device)
    z = _out(rows, ld, device)
    dW, db = _out(N, Kin, device, need[0]), _out(1, N, device, need[1])
    rc = lib.linetr_input_layer_forward(None, x.data_ptr(), ldx, W.data_ptr(), b.data_ptr(), rows, N, Kin, z.data_ptr(), ld, _stream())
    assert rc == 0, lib.linetr_last_error()
    ws = torch.empty(max(int(lib.linetr_input_layer_backward_workspace_bytes(rows, N, Kin)), 16), dtype=torch.uint8, device=device)
    rc = lib.linetr_input_layer_backward(None, x.data_ptr(), ldx, g.data_ptr(), ld, rows, N, Kin, _ptr(dW), _ptr(db), ws.data_ptr(), ws.numel(),
                                         _stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    res = {"z": _take(z, rows, N, "z")}
    if dW is not None:
        res["dW"] = _take(dW, N, Kin, "dW")
    if db is not None:
        res["db"] = _take(db, 1, N, "db")[0]
    return res


def ta_launch(lib, c, need=(True, True), device="cuda:0"):
    """The raw token-assembly entry points on a ta_case: forward, then backward from the case's dx.  Sentinel rows sit behind every
    input, a marker row behind every output.  Returns a dict of CPU arrays x, dtok, dcls."""
    L, S = c["L"], c["S"]
    rs = _rs("ta launch")
    desc, pos = (DL._inp(c[k].reshape(L * S, D), D, rs, device) for k in ("desc", "pos"))
    cls = torch.from_numpy(c["cls"]).to(device)
    dx = DL._inp(c["dx"].reshape(L * (S + 1), D), D, rs, device)
    x, dtok, dcls = _out(L * (S + 1), D, device), _out(L * S, D, device, need[0]), _out(1, D, device, need[1])
    rc = lib.linetr_token_assemble_forward(None, desc.data_ptr(), pos.data_ptr(), cls.data_ptr(), L, S, x.data_ptr(), _stream())
    assert rc == 0, lib.linetr_last_error()
    ws = torch.empty(max(int(lib.linetr_token_assemble_backward_workspace_bytes(L)), 16), dtype=torch.uint8, device=device)
    rc = lib.linetr_token_assemble_backward(None, dx.data_ptr(), L, S, _ptr(dtok), _ptr(dcls), ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, lib.linetr_last_error()
    torch.cuda.synchronize()
    res = {"x": _take(x, L * (S + 1), D, "x").reshape(L, S + 1, D)}
    if dtok is not None:
        res["dtok"] = _take(dtok, L * S, D, "dtok").reshape(L, S, D)
    if dcls is not None:
        res["dcls"] = _take(dcls, 1, D, "dcls")[0]
    return res


def fixture_ratios(got, f, fm):
    """[(tensor, max |got - fixture|, bar)] over everything tests/golden/keyline.npz (`f`) and keyline_matrices.npz (`fm`) hold of run_calls'
    result `got`: the bar is 8 max(the stored float32 error of the WHOLE tensor, 2^-23 max |stored|); a matrix is compared on its sub-grid"""
    rows, in_fm = [], set(fm.files)
    for yard in f.files:
        if not yard.endswith("_f32_err"):
            continue
        name = yard[:-len("_f32_err")]
        key = name.rsplit(".", 1)[0]
        want = fm[name].astype(np.float64) if name in in_fm else f[name]
        val = sub_grid(key, np.asarray(got[name], np.float64)) if name in in_fm else np.asarray(got[name], np.float64)
        assert val.shape == want.shape, (name, val.shape, want.shape)
        rows.append((name, np.abs(val - want).max(), FACTOR * max(float(f[yard]), 2.0 ** -23 * np.abs(want).max())))
    return rows
