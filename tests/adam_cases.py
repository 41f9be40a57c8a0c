"""Cases, the float64 restatement and the bars of the native Adam step (csrc/lt_adam.h; linetr_adam_step, linetr_grad_norm;
Engine.adam_step / grad_norm; linetr_amd.optim.Adam) -- shared by tests/test_adam_cpu.py, tests/test_gpu_adam.py and tools/adam_report.py.

The reference's optimizer IS torch.optim.Adam (train.py:82), so no fixture is needed: the yardstick of a case is torch.optim.Adam(foreach=
False) in float32 on the CPU on the same inputs, and the truth is the float64 restatement below, which tests/test_adam_cpu.py pins to
torch.optim.Adam in float64.

The bar of an output tensor is FACTOR x max(|torch float32 - float64|, 2^-23 max |float64|), for p', m', v' AND for the update p' - p.  The
update is formed in float64, where the difference of two float32 numbers is exact, and its floor is relative to max |update|: without it a
0.1 % error in an lr-sized update hides under the rounding of p.  An all-zero float64 result has the bar 0: it must be met exactly."""
import ctypes as C
import functools
import zlib

import numpy as np
import torch

FACTOR = 8
N_CPU = 4099
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
STEPS = (1, 2, 10, 1000, 1000000)
FAMILIES = ("model", "zero_p", "wide", "eps_dominated", "zeros", "fresh", "wd", "wd_cancel", "decoupled")
OUTPUTS = ("p", "m", "v", "update")
DEFECTS = ("bias corrections of step - 1", "no second bias correction", "beta2 in the first moment", "eps under the root",
           "eps before the division by bc2_sqrt", "coupled and decoupled decay swapped")
SENTINEL = 12345.0
CHUNK, THREADS = 4096, 256          # AD_CHUNK, AD_THREADS of csrc/lt_adam.h (tests/test_adam_cpu.py reads them there)


def steps_of(family):
    return (1,) if family == "fresh" else STEPS


def all_cases():
    return [(family, step) for family in FAMILIES for step in steps_of(family)]


def _rs(*key):
    """a RandomState seeded by the key's text (stable from process to process, unlike hash())"""
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


@functools.lru_cache(maxsize=None)
def make_case(family, step, n=N_CPU):
    """{p, g, m, v: float32 [n]; hyper: the keyword arguments of the optimizer; step: the count AFTER the step}"""
    rs = _rs("adam", family, n)                        # (one draw per family: its steps share the inputs)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    N = lambda: rs.standard_normal(n)
    hyper = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled_weight_decay=False)
    p, g, m, v = 0.05 * N(), N() * 10.0 ** rs.uniform(-6, 0, n), 1e-2 * N(), 1e-4 * N() ** 2
    if family == "zero_p":
        p = np.zeros(n)
    elif family == "wide":
        mag = 10.0 ** np.linspace(-12, 6, n)
        g = mag * np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)
        m = 0.5 * mag * N()
        v = mag ** 2 * rs.uniform(0.5, 1.5, n)
    elif family == "eps_dominated":
        p, g, m, v = np.zeros(n), 1e-9 * N(), 1e-9 * N(), 1e-18 * N() ** 2
    elif family == "zeros":
        g, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
    elif family == "fresh":
        m, v = np.zeros(n), np.zeros(n)
    elif family == "wd":
        hyper["weight_decay"] = 1e-2
    elif family == "wd_cancel":
        hyper["weight_decay"] = 1e-2
        g = -1e-2 * f32(p).astype(np.float64) * (1 + 1e-6 * N())
    elif family == "decoupled":
        hyper.update(weight_decay=1e-2, decoupled_weight_decay=True)
    elif family != "model":
        raise KeyError(family)
    case = {"family": family, "step": int(step), "hyper": hyper, "p": f32(p), "g": f32(g), "m": f32(m), "v": f32(v)}
    for key in "pgmv":
        case[key].setflags(write=False)
    return case


def corrections(lr, betas, step):
    """(step_size, bc2_sqrt) in double, as torch's _single_tensor_adam makes them"""
    step = float(step)
    bias_correction1 = 1 - betas[0] ** step
    bias_correction2 = 1 - betas[1] ** step
    return lr / bias_correction1, bias_correction2 ** 0.5


def adam_f64(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled_weight_decay, scale=None):
    """one Adam step in float64, the textbook form; returns {p, m, v}"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if scale is not None:
        g = np.float64(scale) * g
    if weight_decay != 0:
        if decoupled_weight_decay:
            p = p * (1 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    step_size, bc2_sqrt = corrections(lr, betas, step)
    p = p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps)
    return {"p": p, "m": m, "v": v}


def _fma32(a, b, c):
    """fmaf on float32 arrays, through float64 (the product is exact there; the sum is rounded twice, rarely differently)"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def adam_f32(p, g, m, v, step, lr, betas, eps, weight_decay, decoupled_weight_decay, scale=None, defect=None):
    """The order written in include/linetr_hip.h, in float32 NumPy, one rounding per operation; `defect`: one of DEFECTS planted."""
    assert defect is None or defect in DEFECTS, defect
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    if defect == "coupled and decoupled decay swapped":
        decoupled_weight_decay = not decoupled_weight_decay
    if scale is not None:
        g = f(scale) * g
    if weight_decay != 0:
        if decoupled_weight_decay:
            p = p * f(1 - lr * weight_decay)
        else:
            g = _fma32(f(weight_decay), p, g)
    b1 = betas[1] if defect == "beta2 in the first moment" else betas[0]
    m = _fma32(f(1 - b1), g - m, m)
    v = _fma32(f(1 - betas[1]) * g, g, f(betas[1]) * v)
    step_size, bc2_sqrt = corrections(lr, betas, step - 1 if defect == "bias corrections of step - 1" and step > 1 else step)
    if defect == "bias corrections of step - 1" and step == 1:
        step_size, bc2_sqrt = corrections(lr, betas, 2)          # (step 0 has no correction at all: the neighbour on the other side)
    step_size, bc2_sqrt = f(step_size), f(bc2_sqrt)
    if defect == "no second bias correction":
        bc2_sqrt = f(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if defect == "eps under the root":
            d = np.sqrt(v + f(eps)) / bc2_sqrt
        elif defect == "eps before the division by bc2_sqrt":
            d = (np.sqrt(v) + f(eps)) / bc2_sqrt
        else:
            d = np.sqrt(v) / bc2_sqrt + f(eps)
        p = _fma32(-step_size, m / d, p)
    return {"p": p, "m": m, "v": v}


def torch_adam(case, dtype, foreach=False, cls=torch.optim.Adam):
    """torch's optimizer on the CPU on the case, with its state planted: {p, m, v} as NumPy arrays of `dtype`"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    p = torch.nn.Parameter(t(case["p"]))
    p.grad = t(case["g"])
    opt = cls([p], foreach=foreach, **case["hyper"])
    opt.state[p] = {"step": torch.tensor(float(case["step"] - 1)), "exp_avg": t(case["m"]), "exp_avg_sq": t(case["v"])}
    opt.step()
    assert float(opt.state[p]["step"]) == case["step"]
    return {"p": p.detach().numpy().copy(), "m": opt.state[p]["exp_avg"].numpy().copy(), "v": opt.state[p]["exp_avg_sq"].numpy().copy()}


def with_update(out, p0):
    """the outputs in float64 with the update p' - p (exact in float64 for float32 operands)"""
    out = {k: np.asarray(out[k], dtype=np.float64) for k in ("p", "m", "v")}
    out["update"] = out["p"] - np.asarray(p0, dtype=np.float64)
    return out


def refs_of(case, scale=None):
    """(float64 restatement, torch float32 yardstick), each with the update; a scale enters both as the scaled gradient"""
    ref64 = with_update(adam_f64(case["p"], case["g"], case["m"], case["v"], case["step"], scale=scale, **case["hyper"]), case["p"])
    yard = dict(case)
    if scale is not None:
        yard["g"] = np.float32(scale) * case["g"]
    return ref64, with_update(torch_adam(yard, torch.float32), case["p"])


@functools.lru_cache(maxsize=None)
def refs(family, step, n=N_CPU):
    return refs_of(make_case(family, step, n))


def bar_of(ref32, ref64):
    return FACTOR * max(np.abs(ref32 - ref64).max(initial=0.0), 2.0 ** -23 * np.abs(ref64).max(initial=0.0))


def ratios(got, p0, ref64, ref32):
    """[(output, max |got - float64|, bar)] over OUTPUTS; got: {p, m, v} of any float type"""
    got = with_update(got, p0)
    return [(k, float(np.abs(got[k] - ref64[k]).max(initial=0.0)), float(bar_of(ref32[k], ref64[k]))) for k in OUTPUTS]


def failures(rows):
    return [f"{key}: error {e:.3e} > bar {b:.3e} (x{e / b if b else float('inf'):.2f})" for key, e, b in rows if not e <= b]


def ratio(e, b):
    return e / b if b else (0.0 if e == 0 else float("inf"))


def worst(rows):
    return max((ratio(e, b) for _, e, b in rows), default=0.0)


# ---- tables on the device ----------------------------------------------------------------------------------------------------------

def ragged_sizes(chunk, threads):
    """one ragged table: nothing, the scalar tail's lengths, the block, the vector loop's trip, the chunk and its neighbours, two chunks"""
    C_, T = chunk, threads
    return [0, 1, 2, 3, 4, 5, 7, T - 1, T, 4 * T, 4 * T + 1, C_ - 1, C_, C_ + 1, 2 * C_ - 1, 2 * C_ + 5]


MODEL_KEYS = 153


def model_shapes():
    """the shapes of the model's 153 parameters, in named_parameters() order (needs no device)"""
    from linetr_amd.train_ops import TrainableLineTransformer
    shapes = [tuple(p.shape) for p in TrainableLineTransformer().parameters()]
    assert len(shapes) == MODEL_KEYS
    return shapes


class Carved:
    """`sizes` float32 tensors carved out of ONE flat device buffer, four sentinels apart: tensor i starts at a multiple of four floats
    plus offsets[i % len(offsets)] (0: 16-byte aligned).  views: the tensors; fill(arrays) writes them; untouched(): every sentinel has its
    bits."""

    def __init__(self, sizes, offsets=(0,), device="cuda"):
        at, self.spans = 4, []
        for i, n in enumerate(sizes):
            at = (at + 3) // 4 * 4 + offsets[i % len(offsets)]
            self.spans.append((at, at + n))
            at += n + 4
        self.host = np.full(at + 8, SENTINEL, dtype=np.float32)
        self.flat = torch.from_numpy(self.host.copy()).to(device)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[a:b] for a, b in self.spans]

    def fill(self, flat_values):
        """the tensors' values, one after the other, from one flat array"""
        at = 0
        for a, b in self.spans:
            self.host[a:b] = flat_values[at:at + b - a]
            at += b - a
        assert at == len(flat_values)
        self.flat.copy_(torch.from_numpy(self.host))
        return self

    def values(self):
        """the tensors' values back as one flat array, after asserting that nothing between them changed"""
        now = self.flat.cpu().numpy()
        keep = np.ones(len(now), dtype=bool)
        for a, b in self.spans:
            keep[a:b] = False
        assert now[keep].tobytes() == self.host[keep].tobytes(), "a value outside the tensors was written"
        return np.concatenate([now[a:b] for a, b in self.spans]) if self.spans else now[:0]


def table_of(nat, views, step_size=0.0, bc2_sqrt=1.0):
    """a host table of LinetrAdamTensor records over views = {p, g, m, v: lists of 1-D device tensors} (a missing key: NULL pointers);
    hand tab.ctypes.data to the library"""
    tab = np.zeros(len(views["g"]), dtype=nat.ADAM_TENSOR_DTYPE)
    for key in views:
        tab[key] = [t.data_ptr() if t.numel() else 0 for t in views[key]]
    tab["n"] = [t.numel() for t in views["g"]]
    tab["step_size"], tab["bc2_sqrt"] = step_size, bc2_sqrt
    return tab


def hyper_of(nat, hyper):
    return nat.AdamHyper(hyper["betas"][0], hyper["betas"][1], hyper["eps"], hyper["weight_decay"], hyper["lr"], int(hyper["decoupled_weight_decay"]))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_ragged(eng, case, sizes, offsets, scale=None):
    """The case (n = sum(sizes)) cut into `sizes` tensors, p / g / m / v each carved out of its own flat buffer at offsets[which][...],
    through Engine.adam_step in ONE call; returns {p, m, v} flat after asserting every sentinel, and that g kept its bits."""
    bufs = {k: Carved(sizes, offsets[k]).fill(case[k]) for k in "pgmv"}
    eng.adam_step(bufs["p"].views, bufs["g"].views, bufs["m"].views, bufs["v"].views, [case["step"]] * len(sizes), lr=case["hyper"]["lr"],
                  betas=case["hyper"]["betas"], eps=case["hyper"]["eps"], weight_decay=case["hyper"]["weight_decay"],
                  decoupled=case["hyper"]["decoupled_weight_decay"], grad_scale=scale)
    out = {k: bufs[k].values() for k in "pgmv"}
    assert out["g"].tobytes() == case["g"].tobytes(), "the gradient was written"
    return out


ALIGNMENTS = {"aligned": {k: (0,) for k in "pgmv"}, "offset 1": {k: (1,) for k in "pgmv"}, "offset 2": {k: (2,) for k in "pgmv"},
              "offset 3": {k: (3,) for k in "pgmv"}, "mixed": {"p": (0,), "g": (0, 1, 2, 3), "m": (0, 0, 2), "v": (0,)}}
