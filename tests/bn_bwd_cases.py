"""Case generator, references and error measure of the BatchNorm forward-for-training / backward unit tests (tests/test_gpu_bn_bwd.py,
tests/test_bn_bwd_cases_cpu.py; reused by tools/sig_layer_report.py, which writes profiles/bn_bwd_errors.txt).  Test infrastructure only.

The kernels (csrc/lt_bntrain.h behind linetr_bn_forward, csrc/lt_bnbwd.h behind linetr_bn_backward) compute, per channel over ALL rows of z [rows][C],

    forward    mean, var = the mean and the BIASED variance;  invstd = 1 / sqrt(var + eps);  y = relu?((z - mean) invstd gamma + beta)
    backward   g' = g where y > 0 else 0 (y is an INPUT: the layer's own output; without ReLU g' = g);  xhat = (z - mean) invstd
               dbeta = sum_r g'     dgamma = sum_r g' xhat     dz = gamma invstd (g' - dbeta / n - xhat dgamma / n)
    eval mode  mean, var = the running statistics;  dz = gamma invstd g', dgamma and dbeta as above

Every backward case has two CPU references: `ref64`, the formulae above in float64 (two-pass variance), and `ref32`, torch autograd
through relu(F.batch_norm(z, ..., training)) in float32.  The backward's y input IS ref32's forward output, so that the three -- ref64,
ref32 and the kernels -- differentiate through the same mask (an activation within a rounding of 0 would otherwise open or close with
the precision, which is no property of a backward).  rows = 1: torch refuses a single row in training mode, so ref32 is the formula in
float32 there, with y = relu(beta) exactly and dz = 0.  A result passes a unit when

    max |gpu - ref64|  <=  FACTOR * max( max |ref32 - ref64| ,  2^-23 * max |ref64| )        (FACTOR = 8, as bn_cases.py)

over that unit: for dz the 64-row tiles, for dgamma and dbeta each vector on its own.  The bar is a property of the CPU references alone.
The forward of a case is checked by the bars of bn_cases.py (y per tile, the running statistics per vector) and bit for bit against
linetr_debug_bn_train.

Families: bn_cases.py's `workload`, `offset` (|mean| / std = 256, 4096: z - mean must be formed before rounding), `constant` (channels
without variance: invstd = 316), `affine` (gamma zero and negative, large beta), `sentinel` (row strides beyond C, +-1e4 between and
behind the rows), and two of this file: `integer` (g holds small integers: the float64 sums of dbeta are exact, so dbeta is checkable bit
for bit) and `masked` (every fifth channel has y <= 0 in every row: its dgamma, dbeta and dz are exactly 0)."""
import functools

import torch
import torch.nn.functional as F

import bn_cases as BC
from attn_cases import FACTOR, MARKER, SENTINEL, SPARE_ROWS

EPS = BC.EPS
FAMILIES = BC.FAMILIES + ("integer", "masked")
PLAIN = ("workload", "offset", "constant", "affine", "integer", "masked")
CHANNELS = (4, 100, 252, 256, 260, 512)
ROWS = (2, 3, 63, 64, 65, 129, 257, 333)
BIG_ROWS = (32767, 32769)
BIG_C = 32
TRAIN, EVAL = 0, 1


def strides_of(C):
    """(ldz, ldy, ldg, lddz) combinations: every tensor meets C, C + 4 and 2 C, next to others that differ from it"""
    a, b, c = C, C + 4, 2 * C
    return ((b, a, a, a), (a, b, a, a), (a, a, b, a), (a, a, a, b), (c, b, a, c), (b, c, c, a), (a, c, b, b), (c, a, c, c))


def layer_cases():
    """Every (family, C, rows, relu, mode, ratio, strides) the unit tests run, in a fixed order; strides = (ldz, ldy, ldg, lddz).
      grid      every C x every row count at ld = C, the six plain families rotating so that every C and every row count meets every
                family; relu off in every fifth case (never in 'masked'); 'offset' alternates its two ratios
      eval      every C at 3, 65 and 333 rows in eval mode, 'workload', 'affine', 'integer' and 'masked' in turn
      strides   'sentinel' at the eight stride combinations of strides_of(C), every C, rows 3 / 65 / 129 in turn, one of them in eval mode
      one row   C = 4 and 256 (the C ABI only: torch and batch_norm_relu refuse it)
      big       C = 32 at 32 767 and 32 769 rows (511 chunks; 512 of which the last seven own no row), 'workload' and 'offset'"""
    out = []
    n = 0
    for i, C in enumerate(CHANNELS):
        for j, rows in enumerate(ROWS):
            fam = PLAIN[(i + j) % 6]
            relu = fam == "masked" or n % 5 != 4
            out.append((fam, C, rows, relu, TRAIN, BC.RATIOS[(i + j) // 6 % 2] if fam == "offset" else 0.0, (C,) * 4))
            n += 1
    for i, C in enumerate(CHANNELS):
        for j, rows in enumerate((3, 65, 333)):
            out.append((("workload", "affine", "integer", "masked")[(i + j) % 4], C, rows, True, EVAL, 0.0, (C,) * 4))
    for i, C in enumerate(CHANNELS):
        for j, st in enumerate(strides_of(C)):
            out.append(("sentinel", C, (3, 65, 129)[(i + j) % 3], j % 4 != 3, EVAL if j == 5 else TRAIN, 0.0, st))
    for C in (4, 256):
        out.append(("workload", C, 1, True, TRAIN, 0.0, (C,) * 4))
    for j, rows in enumerate(BIG_ROWS):
        out.append((("workload", "offset")[j], BIG_C, rows, True, TRAIN, 4096.0 if j else 0.0, (BIG_C,) * 4))
        out.append((("offset", "workload")[j], BIG_C, rows, True, TRAIN, 0.0 if j else 256.0, (BIG_C,) * 4))
    assert len(set(out)) == len(out)
    return tuple(out)


def is_big(key):
    return key[2] >= 32767


def forward64(z, gamma, beta, running, mode):
    """float64: (mean, invstd, pre-activation) of the layer; eval mode: the running statistics"""
    z, gamma, beta = z.double(), gamma.double(), beta.double()
    C = z.shape[1]
    if mode == EVAL:
        mean, var = running[:C].double(), running[C:].double()
    else:
        mean = z.mean(dim=0)
        var = ((z - mean) ** 2).mean(dim=0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    return mean, invstd, (z - mean) * invstd * gamma + beta


def backward_formula(z, y, g, gamma, mean, invstd, mode, dtype=torch.float64):
    """The backward from its formulae, every operation in `dtype`; y None: no mask.  Returns dict(dz, dgamma, dbeta)."""
    z, g, gamma, mean, invstd = (t.to(dtype) for t in (z, g, gamma, mean, invstd))
    n = z.shape[0]
    gm = g if y is None else torch.where(y > 0, g, torch.zeros_like(g))
    xhat = (z - mean) * invstd
    dbeta, dgamma = gm.sum(dim=0), (gm * xhat).sum(dim=0)
    dz = gamma * invstd * gm if mode == EVAL else gamma * invstd * (gm - dbeta / n - xhat * dgamma / n)
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta)


def torch32(z, g, gamma, beta, running, momentum, relu, mode):
    """torch autograd through relu?(F.batch_norm(z, ..., training)) in float32.  Returns (y, dict(dz, dgamma, dbeta))."""
    C = z.shape[1]
    zt, gt, bt = (t.clone().requires_grad_() for t in (z, gamma, beta))
    rm, rv = running[:C].clone(), running[C:].clone()
    with torch.enable_grad():
        y = F.batch_norm(zt, rm, rv, gt, bt, mode == TRAIN, momentum, EPS)
        if relu:
            y = F.relu(y)
        y.backward(g)
    return y.detach(), dict(dz=zt.grad, dgamma=gt.grad, dbeta=bt.grad)


def _case(family, C, rows, relu, mode, ratio, strides):
    if family not in FAMILIES or (family == "sentinel") != (max(strides) > C):
        raise ValueError((family, C, strides))
    gen = BC._gen("bn_bwd", family, C, rows, relu, mode, ratio, strides)
    base = family if family in BC.PLAIN else "workload"
    z, gamma, beta, running = BC._layer_inputs(base, C, rows, ratio, gen)
    momentum = 0.1
    g = torch.randint(-4, 5, (rows, C), generator=gen).float() if family == "integer" else torch.randn((rows, C), generator=gen)
    if mode == EVAL:                         # running statistics near the batch's, so that the activations keep their scale
        running = torch.cat([z.mean(dim=0) + 0.1 * torch.randn((C,), generator=gen),
                             z.var(dim=0, unbiased=False) * (0.5 + torch.rand((C,), generator=gen)) + 1e-3])
    if family == "masked":                   # |xhat| <= sqrt(rows) and gamma <= 1.5: beta = -100 closes the channel in every row
        beta = torch.where(torch.arange(C) % 5 == 0, torch.full((C,), -100.0), beta)
        if mode == EVAL:
            running[:C] = z.mean(dim=0)
            running[C:] = z.var(dim=0, unbiased=False) + 1e-3
    if rows > 1:
        y32, r32 = torch32(z, g, gamma, beta, running, momentum, relu, mode)
    else:                                    # the formula in float32: mean = the row, var = 0
        mean, invstd = z[0].clone(), torch.full((C,), 1.0) / torch.sqrt(torch.tensor(EPS, dtype=torch.float32))
        y32 = (z - mean) * invstd * gamma + beta
        y32 = F.relu(y32) if relu else y32
        r32 = backward_formula(z, y32 if relu else None, g, gamma, mean, invstd, mode, torch.float32)
    y_in = y32 if relu else None
    mean, invstd, pre = forward64(z, gamma, beta, running, mode)
    r64 = backward_formula(z, y_in, g, gamma, mean, invstd, mode)
    fwd64 = BC.formula(z, gamma, beta, running, momentum, torch.float64) if mode == TRAIN else None
    fwd32 = None if mode == EVAL else BC.torch32(z, gamma, beta, running, momentum) if rows > 1 else BC.formula(z, gamma, beta, running, momentum, torch.float32)
    return dict(kind="bn_bwd", family=family, C=C, rows=rows, relu=relu, mode=mode, ratio=ratio, strides=strides, momentum=momentum,
                z=z, g=g, gamma=gamma, beta=beta, running=running, y_in=y_in, y32=y32, y64=F.relu(pre) if relu else pre, mean=mean,
                invstd=invstd, ref64=r64, ref32=r32, fwd64=fwd64, fwd32=fwd32)


_small = functools.lru_cache(maxsize=None)(_case)
_large = functools.lru_cache(maxsize=2)(_case)


def layer_case(*key):
    """dict: z, g [rows, C], gamma, beta [C], running [2 C], y_in (the backward's mask input, None without ReLU): float32 CPU tensors made
    once per key; mean, invstd (float64); ref64 / ref32 = dict(dz, dgamma, dbeta); y64 / y32 the forward's output in float64 and as torch
    gives it; fwd64 / fwd32 = bn_cases.formula's / torch32's dict (train mode: the running statistics' references)"""
    return (_large if is_big(key) else _small)(*key)


def n_chunks(rows):
    return BC.n_chunks(rows)


def kernel_model(case, mistake=None):
    """What the kernels do, on the CPU.  The saved statistics as the forward leaves them: float64 sums of z and z^2 chunk by chunk in
    block order, mean = s / n, var = q / n - mean^2 clamped at 0, invstd = 1 / sqrt(var + eps) (eval: the running statistics).  The
    backward: g' from the mask y > 0; sum g' and sum g' (z - mean) in float64 chunk by chunk (z - mean against the float64 mean); dbeta
    = fl(s), dgamma = fl(q invstd); k1 = fl(gamma invstd), k2 = fl(k1 s / n), k3 = fl(k1 invstd^2 q / n) as float32;
    dz = k1 g' - k2 - k3 fl(z - mean), four float32 operations, each rounded.  `mistake` plants one: 'no_mask' (g' = g), 'no_dgamma'
    (the xhat dgamma / n term dropped), 'unbiased_n' (n - 1 where the backward divides by n).
    Returns dict(dz, dgamma, dbeta, mean, invstd)."""
    z, g, rows, C, mode = case["z"], case["g"], case["rows"], case["C"], case["mode"]
    nb = n_chunks(rows)
    chunk = -(-rows // nb)
    n = float(rows)
    if mode == EVAL:
        mean, invstd = case["running"][:C].double(), 1.0 / torch.sqrt(case["running"][C:].double() + float(torch.tensor(EPS, dtype=torch.float32)))
    else:
        s, q = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        for b in range(nb):
            v = z[b * chunk:min((b + 1) * chunk, rows)].double()
            s, q = s + v.sum(dim=0), q + (v * v).sum(dim=0)
        mean = s / n
        var = (q / n - mean * mean).clamp_min(0.0)
        invstd = 1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))
    gm = g if case["y_in"] is None or mistake == "no_mask" else torch.where(case["y_in"] > 0, g, torch.zeros_like(g))
    d64 = z.double() - mean
    s, q = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for b in range(nb):
        sl = slice(b * chunk, min((b + 1) * chunk, rows))
        s, q = s + gm[sl].double().sum(dim=0), q + (gm[sl].double() * d64[sl]).sum(dim=0)
    div = n - 1.0 if mistake == "unbiased_n" else n
    k1 = (case["gamma"].double() * invstd).float()
    zero = torch.zeros(C)
    k2 = zero if mode == EVAL else (k1.double() * s / div).float()
    k3 = zero if mode == EVAL or mistake == "no_dgamma" else (k1.double() * invstd * invstd * q / div).float()
    dz = k1 * gm if mode == EVAL else k1 * gm - k2 - k3 * d64.float()
    return dict(dz=dz, dgamma=(q * invstd).float(), dbeta=s.float(), mean=mean, invstd=invstd)


UNITS = ("dgamma", "dbeta")


def backward_errors(got, case):
    """[(unit, its size, max |got - ref64|, bar)]: dz per 64-row tile (keyed by its first row), then dgamma and dbeta each as a vector;
    what `got` does not carry is left out"""
    out = []
    if got.get("dz") is not None:
        out += BC.tile_errors(got["dz"], case["ref64"]["dz"], case["ref32"]["dz"])
    return out + BC.stat_errors(got, case["ref64"], case["ref32"], UNITS)


def forward_errors(y, case):
    """y per 64-row tile against the float64 forward with torch's float32 forward as the yardstick (one row: bn_cases.single_row_errors)"""
    if case["rows"] == 1:
        return BC.single_row_errors(y, dict(z=case["z"], beta=case["beta"], ref64=dict(alpha=case["gamma"].double() * case["invstd"], y=case["y64"])))
    return BC.tile_errors(y, case["y64"], case["y32"])


def saved_errors(fwd, case):
    """[(unit, C, worst |got - ref| / allowed, 1.0)] of the saved statistics.  mean: 1e-12 of the largest |mean|.  invstd: the kernels
    form var = q / n - mean^2 from two float64 sums of n terms, each addition rounding once, so var carries at most n 2^-52 (mean^2 + var)
    and invstd = (var + eps)^-1/2 half of that relative to var + eps; eval mode has no sum: 4 roundings.  eps crosses the C ABI as a
    float32, 2.5e-13 from the references' 1e-5: half of that relative to var + eps as well."""
    n = case["rows"]
    mean, invstd = case["mean"], case["invstd"]
    tol_mean = 1e-12 * max(mean.abs().max().item(), 1e-30)
    rel = 2.0 ** -52 * (4.0 if case["mode"] == EVAL else 4.0 + n * (mean * mean * invstd * invstd + 1.0))
    rel = rel + 0.5 * abs(float(torch.tensor(EPS, dtype=torch.float32)) - EPS) * invstd * invstd
    return [("save_mean", case["C"], ((fwd["save_mean"] - mean).abs() / tol_mean).max().item(), 1.0),
            ("save_invstd", case["C"], ((fwd["save_invstd"] - invstd).abs() / (rel * invstd)).max().item(), 1.0)]


failures, worst = BC.failures, BC.worst


def exact_failures(got, case):
    """the exact properties of a result dict (the GPU's, or kernel_model's): gamma = 0 -> dz == 0; a channel that is closed in every row
    -> dgamma == dbeta == 0 and dz == 0; 'integer' -> dbeta equal to the float64 reference's, bit for bit"""
    bad = []
    zero_gamma = case["gamma"] == 0
    if got.get("dz") is not None and bool(zero_gamma.any()) and bool((got["dz"][:, zero_gamma] != 0).any()):
        bad.append("gamma = 0 but dz != 0")
    if case["y_in"] is not None:
        closed = (case["y_in"] <= 0).all(dim=0)
        if case["family"] == "masked" and not bool(closed[::5].all()):
            bad.append("the case itself: a 'masked' channel is open somewhere")
        for k in ("dz", "dgamma", "dbeta"):
            if got.get(k) is not None and bool((got[k][..., closed] != 0).any()):
                bad.append(f"a fully masked channel has a non-zero {k}")
    if case["family"] == "integer" and got.get("dbeta") is not None and not torch.equal(got["dbeta"], case["ref64"]["dbeta"].float()):
        bad.append("integer g: dbeta differs from the exact sum")
    return bad


# =================================================================================================================================
# launching (GPU)
# =================================================================================================================================

def _guarded(t, rows, C, ld, gen, device):
    """t [rows, C] inside a [rows + SPARE_ROWS, ld] buffer of +-1e4; returns (device buffer, its CPU image)"""
    buf = SENTINEL * (torch.randint(0, 2, (rows + SPARE_ROWS, ld), generator=gen).float() * 2 - 1)
    if t is not None:
        buf[:rows, :C] = t
    return buf.to(device), buf


def _check_guards(name, dev_buf, host, rows, C, written):
    got = dev_buf.cpu()
    assert torch.equal(got[rows:], host[rows:]), f"rows behind {name} were written"
    assert torch.equal(got[:rows, C:], host[:rows, C:]), f"columns between the rows of {name} were written"
    if not written:
        assert torch.equal(got, host), f"{name} is an input and was written"
    return got[:rows, :C].contiguous()


def launch_forward(L, case, device="cuda:0"):
    """linetr_bn_forward on the case (z at ldz, y at ldy, guards around both).  Returns dict(y, run_mean, run_var, save_mean,
    save_invstd) on the CPU after asserting that every guard and every marker behind the vectors is bit-unchanged."""
    import ctypes as C_
    rows, C, mode = case["rows"], case["C"], case["mode"]
    ldz, ldy = case["strides"][0], case["strides"][1]
    gen = BC._gen("bn_bwd guard fwd", C, rows, case["strides"])
    z, z_host = _guarded(case["z"], rows, C, ldz, gen, device)
    y, y_host = _guarded(None, rows, C, ldy, gen, device)
    gamma, beta = case["gamma"].to(device), case["beta"].to(device)
    running = torch.cat([case["running"], torch.full((SPARE_ROWS,), MARKER)]).to(device)
    save = torch.full((2 * C + SPARE_ROWS,), MARKER, dtype=torch.float64, device=device)
    ws = torch.empty(max(int(L.linetr_bn_forward_workspace_bytes(rows, C)), 16), dtype=torch.uint8, device=device)
    rc = L.linetr_bn_forward(None, z.data_ptr(), ldz, rows, C, gamma.data_ptr(), beta.data_ptr(), EPS, case["momentum"], running.data_ptr(), mode,
                             int(case["relu"]), y.data_ptr(), ldy, save.data_ptr(), ws.data_ptr(), ws.numel(),
                             C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.linetr_last_error()
    torch.cuda.synchronize()
    _check_guards("z", z, z_host, rows, C, written=False)
    yv = _check_guards("y", y, y_host, rows, C, written=True)
    run, sv = running.cpu(), save.cpu()
    assert bool((run[2 * C:] == MARKER).all()) and bool((sv[2 * C:] == MARKER).all()), "floats behind running / save were written"
    assert torch.equal(gamma.cpu(), case["gamma"]) and torch.equal(beta.cpu(), case["beta"])
    if mode == EVAL:
        assert torch.equal(run[:2 * C], case["running"]), "eval mode moved the running statistics"
    return dict(y=yv, run_mean=run[:C], run_var=run[C:2 * C], save_mean=sv[:C], save_invstd=sv[C:2 * C], _save=save[:2 * C].clone())


def launch_backward(L, case, save=None, need=(True, True, True), device="cuda:0"):
    """linetr_bn_backward on the case with y = case['y_in'] and the statistics `save` (a float64 [2 C] device tensor; default: the
    float64 references' mean | invstd).  Returns dict(dz, dgamma, dbeta) on the CPU (what `need` leaves out is None) after the guard checks."""
    import ctypes as C_
    rows, C, mode = case["rows"], case["C"], case["mode"]
    ldz, ldy, ldg, lddz = case["strides"]
    gen = BC._gen("bn_bwd guard bwd", C, rows, case["strides"])
    z, z_host = _guarded(case["z"], rows, C, ldz, gen, device)
    g, g_host = _guarded(case["g"], rows, C, ldg, gen, device)
    y, y_host = _guarded(case["y_in"], rows, C, ldy, gen, device) if case["y_in"] is not None else (None, None)
    dz, dz_host = _guarded(None, rows, C, lddz, gen, device) if need[0] else (None, None)
    vec = lambda on: torch.full((C + SPARE_ROWS,), MARKER, dtype=torch.float32, device=device) if on else None
    dgamma, dbeta = vec(need[1]), vec(need[2])
    if save is None:
        save = torch.cat([case["mean"], case["invstd"]]).to(device)
    gamma = case["gamma"].to(device)
    ws = torch.empty(max(int(L.linetr_bn_backward_workspace_bytes(rows, C)), 16), dtype=torch.uint8, device=device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = L.linetr_bn_backward(None, z.data_ptr(), ldz, ptr(y), ldy, g.data_ptr(), ldg, save.data_ptr(), gamma.data_ptr(), rows, C, mode, ptr(dz),
                              lddz, ptr(dgamma), ptr(dbeta), ws.data_ptr(), ws.numel(), C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.linetr_last_error()
    torch.cuda.synchronize()
    _check_guards("z", z, z_host, rows, C, written=False)
    _check_guards("g", g, g_host, rows, C, written=False)
    if y is not None:
        _check_guards("y", y, y_host, rows, C, written=False)
    out = dict(dz=_check_guards("dz", dz, dz_host, rows, C, written=True) if need[0] else None, dgamma=None, dbeta=None)
    for k, t in (("dgamma", dgamma), ("dbeta", dbeta)):
        if t is not None:
            host = t.cpu()
            assert bool((host[C:] == MARKER).all()), f"floats behind {k} were written"
            out[k] = host[:C]
    return out
