"""Case generator, references and error measure of the train-mode BatchNorm unit tests (tests/test_gpu_bn_train.py,
tests/test_bn_cases_cpu.py; reused by tools/bn_unit_report.py, which writes profiles/bn_unit_errors.txt).  Test infrastructure only.

The kernels (lt_bntrain.h: bn_partial_kernel, bn_finalize_kernel, bn_apply_kernel behind bn_train_layer) compute, per channel
over ALL rows of z [rows][C],

    mean, var = the mean and the BIASED variance        y = relu((z - mean) / sqrt(var + 1e-5) * gamma + beta)
    running <- (1 - m) running + m (mean | var * n / (n - 1))        alpha = gamma / sqrt(var + 1e-5)

Every case has two CPU references written from that formula, not from the kernel: `ref64`, all of it in float64 with a two-pass
variance, and `ref32`, torch.nn.functional.batch_norm(..., training=True) in float32 followed by ReLU (its batch statistics read
off a second call with momentum 1).  The encoder chains (linetr_debug_bn_train, which = 0 / 1) are conv -> BatchNorm(batch) -> ReLU
layer by layer from the UNFOLDED state dict, in float64 and in plain float32 torch.  A kernel passes a unit when

    max |gpu - ref64|  <=  FACTOR * max( max |ref32 - ref64| ,  2^-23 * max |ref64| )        (FACTOR = 8, as attn_cases.py)

over that unit: for y the 64-row tiles (and the last partial one), for the statistics each vector on its own -- batch mean, batch
variance, running mean, running variance, alpha.  The bar is a property of the CPU references alone, never of a kernel's output.
No family needs a kernel-order float32 evaluation in its bar: kernel_model() below -- float64 sums chunk by chunk, alpha and beta'
rounded to float32, one multiply and one add -- is the CPU statement of what the kernels do, and test_bn_cases_cpu.py shows that
it stays inside the plain bar on every case of the list while three planted mistakes applied to it do not.

rows = 1: torch refuses a single row in training mode, so both references are the formula itself there (float64 and float32) with
the unbiased factor n / (n - 1) taken as 1, which is what bn_finalize_kernel documents: var = 0, the running variance moved towards
0, and y = relu(beta) -- up to the roundings of z alpha + (beta - mean alpha), which single_row_errors() bounds from the number
format (the formula's own float32 error is zero there, so the bar above would say nothing about that form).

linetr_create takes keyline_encoder [32, 64 k, 64 k, 256] only, so the chain's second width set is (32, 192, 320, 256): 192 leaves
a quarter of bn_partial_kernel's block without rows (256 / 192 = 1 row in parallel, threads 192-255 idle), 320 gives the second
channel pass to 64 of its 256 threads."""
import functools
import zlib

import torch
import torch.nn.functional as F

import front_cases as FC
from attn_cases import FACTOR, MARKER, SENTINEL, SPARE_ROWS, state_dict_t
from workloads import synth

EPS = 1e-5
MAX_BLOCKS = 512
FAMILIES = ("workload", "offset", "constant", "affine", "sentinel")
PLAIN = FAMILIES[:4]                                   # the families that run at ld = C
CHANNELS = (4, 8, 32, 64, 96, 100, 128, 252, 256, 260, 384, 508, 512)
ROWS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 257, 333)
BIG_CHANNELS = (32, 260, 512)
BIG_ROWS = (32767, 32768, 32769, 3 * 32768 + 5)
MOMENTA = (0.0, 0.1, 1.0)
RATIOS = (256.0, 4096.0)                               # |mean| / std of the 'offset' family
CHAIN_ROWS = (33, 64, 65, 193, 4378)
CHAIN_WIDTHS = ((32, 64, 128, 256), (32, 192, 320, 256))
CHAIN_WEIGHTS = ("calibrated", 3)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def n_chunks(rows):
    """row chunks bn_train_layer sums the statistics in"""
    return min(MAX_BLOCKS, max(1, rows // 64))


def rows_in_parallel(C):
    """(cw, rp) of bn_partial_kernel: channels side by side in a block pass, rows in parallel"""
    cw = min(C, 256)
    return cw, 256 // cw


# =================================================================================================================================
# one free-standing layer
# =================================================================================================================================

def layer_cases():
    """Every (family, C, ld, rows, momentum, ratio) the unit tests run, in a fixed order; ratio is 0 outside the 'offset' family.
      grid      every C x every row count at ld = C, the four plain families and the three momenta rotating so that every C meets
                every family and every momentum, and every row count every family
      families  every plain family at every C at 65 and 333 rows (a second chunk; a chunk size of 333 / 5 = 67 that rp = 2, 4, 8
                do not divide)
      strides   'sentinel' at ld = C + 4 and 2 C, every C, at 3, 65, 129 and 200 rows
      big       C in BIG_CHANNELS at 32 767 / 32 768 / 32 769 / 98 309 rows (511, 512, 512 chunks -- at 32 769 the last seven own
                no rows -- and chunks of 193 rows), 'workload' and 'offset' in turn, one of them with ld = C + 4"""
    out = []
    for i, C in enumerate(CHANNELS):
        for j, rows in enumerate(ROWS):
            fam = PLAIN[(i + j) % 4]
            out.append((fam, C, C, rows, MOMENTA[(i + 2 * j) % 3], RATIOS[(i + j) // 4 % 2] if fam == "offset" else 0.0))
    for i, C in enumerate(CHANNELS):
        for j, fam in enumerate(PLAIN):
            for k, rows in enumerate((65, 333)):
                out.append((fam, C, C, rows, MOMENTA[(i + j + k) % 3], RATIOS[(i + k) % 2] if fam == "offset" else 0.0))
    for i, C in enumerate(CHANNELS):
        for j, ld in enumerate((C + 4, 2 * C)):
            for k, rows in enumerate((3, 65, 129, 200)):
                out.append(("sentinel", C, ld, rows, MOMENTA[(i + j + k) % 3], 0.0))
    for i, C in enumerate(BIG_CHANNELS):
        for j, rows in enumerate(BIG_ROWS):
            fam = ("workload", "offset")[(i + j) % 2]
            out.append((fam, C, C, rows, 0.1, RATIOS[j % 2] if fam == "offset" else 0.0))
        out.append(("sentinel", C, C + 4, 32769, 0.1, 0.0))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return tuple(uniq)


def is_big(key):
    return key[3] >= 32767


def formula(z, gamma, beta, running, momentum, dtype):
    """The layer from its formula, every operation in `dtype`, two-pass variance; rows = 1: unbiased factor 1.
    Returns dict(y, mean, var, run_mean, run_var, alpha)."""
    z, gamma, beta, running = z.to(dtype), gamma.to(dtype), beta.to(dtype), running.to(dtype)
    n, C = z.shape
    mean = z.mean(dim=0)
    var = ((z - mean) ** 2).mean(dim=0)
    inv = 1.0 / torch.sqrt(var + EPS)
    y = F.relu((z - mean) * inv * gamma + beta)
    unb = var * (n / (n - 1.0)) if n > 1 else var
    return dict(y=y, mean=mean, var=var, run_mean=(1.0 - momentum) * running[:C] + momentum * mean,
                run_var=(1.0 - momentum) * running[C:] + momentum * unb, alpha=gamma * inv)


def torch32(z, gamma, beta, running, momentum):
    """torch.nn.functional.batch_norm in training mode, float32, + ReLU; the batch statistics from a call with momentum 1"""
    n, C = z.shape
    rm, rv = running[:C].clone(), running[C:].clone()
    y = F.relu(F.batch_norm(z, rm, rv, gamma, beta, True, momentum, EPS))
    bm, bv = torch.zeros(C), torch.zeros(C)
    F.batch_norm(z, bm, bv, None, None, True, 1.0, EPS)
    var = bv * torch.tensor((n - 1.0) / n, dtype=torch.float32)
    return dict(y=y, mean=bm, var=var, run_mean=rm, run_var=rv, alpha=gamma / torch.sqrt(var + EPS))


def _layer_inputs(family, C, rows, ratio, g):
    scale = 0.1 + 2.9 * torch.rand((C,), generator=g)
    shift = scale * torch.randn((C,), generator=g)
    gamma = 0.5 + torch.rand((C,), generator=g)
    beta = 0.5 * torch.randn((C,), generator=g)
    z = torch.randn((rows, C), generator=g)
    if family == "offset":                   # |mean| / std of the SAMPLE is `ratio` at every row count (two rows: shift +- scale)
        sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
        shift = sign * ratio * scale
        if rows > 1:
            z = (z - z.mean(dim=0)) / z.std(dim=0, unbiased=False)
    z = z * scale + shift
    if family == "constant":                 # channel c % 4: 0 constant, 1 constant except in one row, 2 all zero, 3 as 'workload'
        c = torch.arange(C)
        z[:, c % 4 == 0] = shift[c % 4 == 0]
        one = (c % 4 == 1).nonzero()[:, 0]
        z[:, one] = shift[one]
        z[torch.randint(0, rows, (len(one),), generator=g), one] += scale[one]
        z[:, c % 4 == 2] = 0.0
    if family == "affine":                   # gamma: c % 3 = 0 zero, 1 negative, 2 positive; beta large
        c = torch.arange(C)
        gamma = torch.where(c % 3 == 0, torch.zeros(C), torch.where(c % 3 == 1, -(0.5 + 1.5 * torch.rand((C,), generator=g)), gamma))
        beta = 50.0 * torch.randn((C,), generator=g)
    running = torch.cat([torch.randn((C,), generator=g), 0.5 + torch.rand((C,), generator=g)])
    return z.contiguous(), gamma, beta, running


def _layer_case(family, C, ld, rows, momentum, ratio):
    if family not in FAMILIES or (family == "sentinel") != (ld > C):
        raise ValueError((family, C, ld))
    g = _gen("bn", family, C, ld, rows, momentum, ratio)
    z, gamma, beta, running = _layer_inputs(family, C, rows, ratio, g)
    r64 = formula(z, gamma, beta, running, momentum, torch.float64)
    r32 = torch32(z, gamma, beta, running, momentum) if rows > 1 else formula(z, gamma, beta, running, momentum, torch.float32)
    return dict(kind="bn", family=family, C=C, ld=ld, rows=rows, momentum=momentum, ratio=ratio, z=z, gamma=gamma, beta=beta,
                running=running, ref64=r64, ref32=r32)


_small = functools.lru_cache(maxsize=None)(_layer_case)
_large = functools.lru_cache(maxsize=2)(_layer_case)           # up to 98 309 x 512: not kept


def layer_case(family, C, ld, rows, momentum, ratio=0.0):
    """dict: z [rows, C], gamma, beta [C], running [2 C] (float32 CPU tensors, made once per key), ref64 / ref32 as formula() gives them"""
    return (_large if rows >= 32767 else _small)(family, C, ld, rows, momentum, ratio)


def kernel_model(case, mistake=None):
    """What the kernels do, on the CPU: per-channel sum and sum of squares in float64, chunk by chunk in block order (the chunking
    of bn_train_layer); mean, biased variance (clamped at 0), alpha and beta' = beta - mean alpha in float64, both rounded to
    float32; y = max(z alpha + beta', 0) as one float32 multiply and one float32 add; running statistics in float64, rounded once.
    `mistake` plants one: 'unbiased_norm' (the unbiased variance in the normalisation), 'drop_last_chunk' (the last chunk's rows
    never summed), 'float_acc' (float32 accumulators)."""
    z, rows, C, m = case["z"], case["rows"], case["C"], case["momentum"]
    acc = torch.float32 if mistake == "float_acc" else torch.float64
    nb = n_chunks(rows)
    chunk = -(-rows // nb)
    last = (rows - 1) // chunk
    s, q = torch.zeros(C, dtype=acc), torch.zeros(C, dtype=acc)
    for b in range(nb):
        v = z[b * chunk:min((b + 1) * chunk, rows)].to(acc)
        if mistake == "drop_last_chunk" and b == last and nb > 1:
            continue
        s, q = s + v.sum(dim=0), q + (v * v).sum(dim=0)
    n = float(rows)
    mean = s.double() / n
    var = (q.double() / n - mean * mean).clamp_min(0.0)
    unb = var * n / (n - 1.0) if rows > 1 else var
    alpha = case["gamma"].double() / torch.sqrt((unb if mistake == "unbiased_norm" else var) + EPS)
    a32, b32 = alpha.float(), (case["beta"].double() - mean * alpha).float()
    run = case["running"].double()
    return dict(y=F.relu(z * a32 + b32), mean=mean.float(), var=var.float(), run_mean=((1.0 - m) * run[:C] + m * mean).float(),
                run_var=((1.0 - m) * run[C:] + m * unb).float(), alpha=a32)


STAT_UNITS = ("mean", "var", "run_mean", "run_var", "alpha")


def _tile_max(x, rows):
    """[ceil(rows / 64)]: max over each 64-row tile of a per-row maximum"""
    pad = (-rows) % 64
    return F.pad(x, (0, pad)).view(-1, 64).amax(dim=1)


def tile_errors(got_y, ref64_y, ref32_y):
    """[(first row of the 64-row tile, rows in it, max |got - ref64|, bar)]"""
    rows = ref64_y.shape[0]
    err = _tile_max((got_y.double() - ref64_y).abs().amax(dim=1), rows)
    own = _tile_max((ref32_y.double() - ref64_y).abs().amax(dim=1), rows)
    top = _tile_max(ref64_y.abs().amax(dim=1), rows)
    bar = FACTOR * torch.maximum(own, 2.0 ** -23 * top)
    return [(64 * i, min(64, rows - 64 * i), float(err[i]), float(bar[i])) for i in range(len(err))]


def stat_errors(got, ref64, ref32, units=STAT_UNITS):
    """[(unit, its length, max |got - ref64|, bar)] for each statistics vector on its own"""
    out = []
    for u in units:
        if got.get(u) is None:
            continue
        r64 = ref64[u]
        own = (ref32[u].double() - r64).abs().max().item()
        out.append((u, r64.numel(), (got[u].double() - r64).abs().max().item(), FACTOR * max(own, 2.0 ** -23 * r64.abs().max().item())))
    return out


def single_row_errors(got_y, case):
    """rows = 1, where the formula gives y = relu(beta) exactly and the bar would be 2^-23 |beta|: the kernels' documented form
    max(z alpha + beta', 0) with beta' = beta - mean alpha cannot reach that, since alpha = gamma / sqrt(1e-5) multiplies the row
    itself.  Its float32 roundings bound the error per channel by 4 x 2^-24 (|z alpha| + |beta|): alpha rounded (2^-24 |z alpha|),
    the product rounded (the same), beta' rounded and the sum rounded (2^-24 (|beta| + |z alpha|) between them at most twice).
    [(0, 1, max error / bound, 1.0)]: that bound is the bar of the single tile."""
    bound = 4.0 * 2.0 ** -24 * ((case["z"].double() * case["ref64"]["alpha"]).abs() + case["beta"].double().abs())
    return [(0, 1, ((got_y.double() - case["ref64"]["y"]).abs() / bound).max().item(), 1.0)]


def layer_errors(got, case):
    """tile_errors of y (rows = 1: single_row_errors) + stat_errors of the statistics a result dict (the GPU's, or
    kernel_model's) carries"""
    tiles = single_row_errors(got["y"], case) if case["rows"] == 1 else tile_errors(got["y"], case["ref64"]["y"], case["ref32"]["y"])
    return tiles + stat_errors(got, case["ref64"], case["ref32"])


def failures(rows, what="unit"):
    return [f"{what} {a} ({n}): error {e:.3e} > bar {b:.3e} (x{e / b if b else float('inf'):.1f})" for a, n, e, b in rows if not e <= b]


def worst(rows):
    return max(rows, key=lambda r: r[2] / r[3] if r[3] else (float("inf") if r[2] else 0.0))


def pack_layer(case, device):
    """The case on the device: z in a [rows + SPARE_ROWS, ld] buffer whose columns behind C and whose spare rows hold +-1e4
    (returned on the CPU as well, to compare what must stay untouched), gamma, beta, running, and marker-filled batch / affine."""
    rows, C, ld = case["rows"], case["C"], case["ld"]
    g = _gen("guard", C, ld, rows)
    buf = SENTINEL * (torch.randint(0, 2, (rows + SPARE_ROWS, ld), generator=g).float() * 2 - 1)
    buf[:rows, :C] = case["z"]
    dev = lambda t: t.clone().to(device)
    mark = lambda: torch.full((2 * C + SPARE_ROWS,), MARKER, dtype=torch.float32, device=device)
    return dict(host=buf, z=buf.to(device), gamma=dev(case["gamma"]), beta=dev(case["beta"]),
                running=torch.cat([case["running"], torch.full((SPARE_ROWS,), MARKER)]).to(device), batch=mark(), affine=mark())


def launch_layer(eng, case, want_batch=True):
    """Runs the case through linetr_debug_bn_train(which = -1); returns (result dict on the CPU like formula()'s plus 'beta2' =
    beta', number of row chunks) after asserting that every sentinel in and behind z and every marker behind the vectors is
    bit-unchanged (and, for want_batch = False, the whole batch vector)."""
    p = pack_layer(case, eng.device)
    rows, C = case["rows"], case["C"]
    _, nb = eng.debug_bn_train(-1, z=p["z"], rows=rows, channels=C, ld=case["ld"], gamma=p["gamma"], beta=p["beta"],
                               momentum=case["momentum"], running=p["running"], batch=p["batch"] if want_batch else None,
                               affine=p["affine"])
    torch.cuda.synchronize()
    z, run, bat, aff = p["z"].cpu(), p["running"].cpu(), p["batch"].cpu(), p["affine"].cpu()
    assert torch.equal(z[rows:], p["host"][rows:]), "rows behind z were written"
    assert torch.equal(z[:rows, C:], p["host"][:rows, C:]), "columns between the rows of z were written"
    assert bool((run[2 * C:] == MARKER).all()) and bool((aff[2 * C:] == MARKER).all()), "floats behind running / affine were written"
    assert bool((bat[2 * C if want_batch else 0:] == MARKER).all()), "floats behind (or of an absent) batch vector were written"
    assert torch.equal(p["gamma"].cpu(), case["gamma"]) and torch.equal(p["beta"].cpu(), case["beta"])
    got = dict(y=z[:rows, :C].contiguous(), run_mean=run[:C], run_var=run[C:2 * C], alpha=aff[:C], beta2=aff[C:2 * C],
               mean=bat[:C] if want_batch else None, var=bat[C:2 * C] if want_batch else None)
    return got, nb


# =================================================================================================================================
# the encoder chains
# =================================================================================================================================

@functools.lru_cache(maxsize=None)
def chain_state_dict(weights, widths):
    """(numpy state dict for Engine, torch state dict) of `weights` ('calibrated' or a seed) at the encoder widths `widths`; the
    calibrated weights exist at the reference's widths only, the other set takes the seed-0 weights in their place"""
    if tuple(widths) == CHAIN_WIDTHS[0]:
        return state_dict_t(weights)
    sd = synth.make_state_dict(0 if weights == "calibrated" else int(weights), enc=tuple(widths))
    return sd, synth.to_torch_state_dict(sd)


def chain_reference(sd_t, enc, feats, running, momentum, dtype):
    """conv -> BatchNorm(batch statistics) -> ReLU of the encoder's four layers on feature rows, every operation in `dtype`
    (float32: torch's batch_norm).  Returns dict(y [rows, e3], mean / var / run_mean / run_var packed layer after layer)."""
    x = feats
    packs = {k: [] for k in ("mean", "var", "run_mean", "run_var")}
    off = 0
    for i in range(4):
        c, b = f"{FC.ENC[enc]}.{3 * i}", f"{FC.ENC[enc]}.{3 * i + 1}"
        x = F.linear(x, sd_t[c + ".weight"][:, :, 0].to(dtype), sd_t[c + ".bias"].to(dtype))
        C = x.shape[1]
        run = running[off:off + 2 * C]
        fn = (lambda *a: formula(*a, torch.float64)) if dtype == torch.float64 else torch32
        r = fn(x, sd_t[b + ".weight"], sd_t[b + ".bias"], run, momentum)
        for k in packs:
            packs[k].append(r[k])
        x = r["y"]
        off += 2 * C
    return dict(y=x, **{k: torch.cat(v) for k, v in packs.items()})


@functools.lru_cache(maxsize=None)
def chain_case(enc, weights, widths, rows, momentum=0.1):
    """One encoder in training mode on `rows` 'workload' rows of front_cases (its own first-layer inputs): inputs, the running
    statistics before the call packed [layer][mean | var] -> 2 sum(widths) floats, ref64 / ref32 as chain_reference gives them."""
    g = _gen("bn chain", enc, weights, widths, rows, momentum)
    inputs = FC._mlp_inputs(enc, "workload", rows, g)
    sd_t = chain_state_dict(weights, widths)[1]
    running = torch.cat([torch.cat([0.2 * torch.randn((C,), generator=g), 0.5 + torch.rand((C,), generator=g)]) for C in widths])
    r64 = chain_reference(sd_t, enc, FC.enc_features(enc, inputs, torch.float64), running, momentum, torch.float64)
    r32 = chain_reference(sd_t, enc, FC.enc_features(enc, inputs, torch.float32), running, momentum, torch.float32)
    return dict(kind="chain", enc=enc, weights=weights, widths=tuple(widths), rows=rows, momentum=momentum, inputs=inputs,
                running=running, ref64=r64, ref32=r32)


def unpack_stats(running, batch, widths):
    """packed [layer][mean | var] vectors -> dict(run_mean, run_var, mean, var), each the layers' vectors one after the other"""
    out = {k: [] for k in ("run_mean", "run_var", "mean", "var")}
    off = 0
    for C in widths:
        out["run_mean"].append(running[off:off + C]); out["run_var"].append(running[off + C:off + 2 * C])
        out["mean"].append(batch[off:off + C]); out["var"].append(batch[off + C:off + 2 * C])
        off += 2 * C
    return {k: torch.cat(v) for k, v in out.items()}


def launch_chain(eng, case):
    """Runs the case through linetr_debug_bn_train(which = 0 / 1); returns (dict(y, run_mean, run_var, mean, var) on the CPU, the
    packed running and batch vectors as the library wrote them, number of row chunks) after asserting that the spare rows behind the
    output and the floats behind the statistics still hold the marker."""
    rows, widths, dev = case["rows"], case["widths"], eng.device
    g = _gen("guard", case["enc"], rows)
    ins = [torch.cat([t, FC._sentinel((SPARE_ROWS,) + tuple(t.shape[1:]), g)]).contiguous().to(dev) for t in case["inputs"]]
    out = torch.full((rows + SPARE_ROWS, widths[3]), MARKER, dtype=torch.float32, device=dev)
    n = 2 * sum(widths)
    running = torch.cat([case["running"], torch.full((SPARE_ROWS,), MARKER)]).to(dev)
    batch = torch.full((n + SPARE_ROWS,), MARKER, dtype=torch.float32, device=dev)
    which = 0 if case["enc"] == "word" else 1
    _, nb = eng.debug_bn_train(which, **{case["enc"]: (*ins, rows)}, out=out, momentum=case["momentum"], running=running, batch=batch)
    torch.cuda.synchronize()
    o, run, bat = out.cpu(), running.cpu(), batch.cpu()
    assert bool((o[rows:] == MARKER).all()), "rows behind the output were written"
    assert bool((run[n:] == MARKER).all()) and bool((bat[n:] == MARKER).all()), "floats behind the statistics were written"
    return dict(y=o[:rows], **unpack_stats(run[:n], bat[:n], widths)), run[:n], bat[:n], nb


def chain_errors(got, case):
    """tile_errors of the encoder's output; the four statistics, every LAYER's vector a unit of its own"""
    rows = tile_errors(got["y"], case["ref64"]["y"], case["ref32"]["y"])
    off = 0
    for i, C in enumerate(case["widths"]):
        sl = slice(off, off + C)
        cut = lambda d: {k: v[sl] for k, v in d.items() if k != "y"}
        rows += [(f"layer {i} {u}", n, e, b) for u, n, e, b in stat_errors(cut(got), cut(case["ref64"]), cut(case["ref32"]),
                                                                          ("mean", "var", "run_mean", "run_var"))]
        off += C
    return rows
