"""The neighbour-line attention softmax(q^T k / 8) v (models/line_transformer.py:132-136 of the reference) and its backward, stated
from the formulas: a float64 closed form in NumPy (the reference of tests/test_gpu_sig_attn_bwd.py), a torch statement of the attention on rows
and of the module around it (what autograd differentiates: its float32 error is the bar), the cases, the bar and the launch helper the
tests and tools/sig_attn_bwd_report.py share.  Test infrastructure only.

    per image and head, rows [n, 64]:  S = (q / 8) k^T;  lse = log sum_j exp S;  P = exp(S - lse);  o = P v
    delta = rowsum(dO * o);  dV = P^T dO;  dP = dO v^T;  dS = P * (dP - delta);  dK = dS^T (q / 8);  dQ = (dS k) / 8

The bar is the attention suite's (tests/attn_cases.py, FACTOR = 8), per image and output:
    max |gpu - ref64|  <=  8 * max( max |ref32 - ref64| ,  2^-23 * max |ref64| )
ref32 = float32 autograd on the CPU; the bar is a property of the references alone."""
import functools

import numpy as np
import torch

import attn_cases as AC

FACTOR = AC.FACTOR
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
FAMILIES = AC.FAMILIES
# every tile edge of the kernels -1 / 0 / +1 (32-row chunks, 64-row staged tiles, 128-row blocks), the training size 250, 256, and sizes
# of several blocks with a ragged tail
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 250, 255, 256, 257, 599, 769)
POW2 = (2, 4, 8, 16)            # see pow2_premise
SENTINEL, MARKER, SPARE_ROWS = AC.SENTINEL, AC.MARKER, AC.SPARE_ROWS


def ragged_counts(seed=0):
    """SIZES shuffled (image offsets are multiples of nothing), with an empty image first, in the middle and last"""
    c = list(SIZES)
    np.random.RandomState(2000 + seed).shuffle(c)
    mid = len(c) // 2
    return tuple([0] + c[:mid] + [0] + c[mid:] + [0])


# ---- the closed form -------------------------------------------------------------------------------------------------------------

def closed_form_image(q, k, v, dO):
    """float64.  q, k, v, dO [n, 4, 64] of ONE image (q unscaled) -> dict o, dq, dk, dv [n, 4, 64], lse [n, 4]"""
    q, k, v, dO = (np.asarray(a, np.float64) for a in (q, k, v, dO))
    out = {key: np.zeros(q.shape) for key in ("o", "dq", "dk", "dv")}
    out["lse"] = np.zeros(q.shape[:2])
    for h in range(q.shape[1]):
        qs = q[:, h] * 0.125
        S = qs @ k[:, h].T
        m = S.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(S - m).sum(axis=1, keepdims=True))
        P = np.exp(S - lse)
        o = P @ v[:, h]
        delta = np.diag(dO[:, h] @ o.T)[:, None]          # (the product that forms dP below: at n = 1, where o = v, dP - delta is exactly 0)
        dS = P * (dO[:, h] @ v[:, h].T - delta)
        out["o"][:, h], out["lse"][:, h] = o, lse[:, 0]
        out["dv"][:, h] = P.T @ dO[:, h]
        out["dk"][:, h] = dS.T @ qs
        out["dq"][:, h] = (dS @ k[:, h]) * 0.125
    return out


def attn_rows(q, k, v):
    """softmax(q k^T / 8) v on rows, in helpers.attn_reference's terms but differentiable: q, k, v [..., n, 4, 64] (q unscaled; the 1/8
    is a power of two, so exact), one softmax domain per leading index and head.  Returns (message [..., n, 4, 64], scores [..., 4, n, n])"""
    sc = torch.einsum("...nhd,...mhd->...hnm", q * 0.125, k)
    return torch.einsum("...hnm,...mhd->...nhd", torch.softmax(sc, dim=-1), v), sc


def from_call_shape(x):
    """the reference's call shape [B, 64, 4, n] (channel, head, position) -> rows [B * n, 4, 64], item after item"""
    return x.permute(0, 3, 2, 1).reshape(-1, 4, 64)


def torch_image(q, k, v, dO, dtype):
    """autograd through attn_rows on the CPU at `dtype`, one image of rows [n, 4, 64]: dict of float64 arrays like closed_form_image"""
    qt, kt, vt = (torch.as_tensor(np.asarray(a)).to(dtype).clone().requires_grad_() for a in (q, k, v))
    with torch.enable_grad():
        o, sc = attn_rows(qt, kt, vt)
        o.backward(torch.as_tensor(np.asarray(dO)).to(dtype))
    res = {key: x.detach().double().numpy() for key, x in (("o", o), ("dq", qt.grad), ("dk", kt.grad), ("dv", vt.grad))}
    res["lse"] = torch.logsumexp(sc.detach(), dim=-1).T.double().numpy()                     # [4, n] -> [n, 4]
    return res


# ---- the cases -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(family, counts, seed=0, parity=0, integer_dO=False):
    """A var-len batch: q, k, v of attn_cases.qkv_case(family, counts) and a unit-normal dO [N, 4, 64] (`integer_dO`: integers -4 .. 4;
    'sentinel': +-1e4 in the images of `parity`, like q, k, v), with ref64 (the closed form) and ref32 (float32 autograd), dicts of
    [N, 4, 64] / [N, 4] arrays over the images in `check`.  The tensors are shared: do not write to them."""
    base = AC.qkv_case(family, counts, seed, parity)
    g = AC._gen("sig_attn_bwd", family, counts, seed, integer_dO)
    N = int(base["cu"][-1])
    dO = torch.randint(-4, 5, (N, 4, 64), generator=g).float() if integer_dO else torch.randn((N, 4, 64), generator=g)
    cu = base["cu"]
    if family == "sentinel":
        for i, n in enumerate(counts):
            if i % 2 == parity and n:
                dO[int(cu[i]):int(cu[i + 1])] = AC._sentinel_rows((n, 4, 64), g)
    shape = {key: (N, 4) if key == "lse" else (N, 4, 64) for key in OUTPUTS}
    ref64, ref32 = ({key: np.zeros(shape[key]) for key in OUTPUTS} for _ in range(2))
    for i in base["check"]:
        a, b = int(cu[i]), int(cu[i + 1])
        if a == b:
            continue
        args = [t[a:b].numpy() for t in (base["q"], base["k"], base["v"], dO)]
        r64, r32 = closed_form_image(*args), torch_image(*args, torch.float32)
        for key in OUTPUTS:
            ref64[key][a:b], ref32[key][a:b] = r64[key], r32[key]
    return dict(family=family, counts=counts, cu=cu, q=base["q"], k=base["k"], v=base["v"], dO=dO, ref64=ref64, ref32=ref32, check=base["check"])


def bar_of(ref32, ref64):
    return FACTOR * max(np.abs(ref32 - ref64).max(), 2.0 ** -23 * np.abs(ref64).max())


def image_ratios(got, c):
    """[(image, sub-lines, output, max |got - ref64|, bar)] over the compared images with at least one sub-line; got: dict of arrays"""
    rows = []
    for i in c["check"]:
        a, b = int(c["cu"][i]), int(c["cu"][i + 1])
        if a == b:
            continue
        for key in OUTPUTS:
            if key not in got:
                continue
            r64 = c["ref64"][key][a:b]
            err = np.abs(got[key][a:b].astype(np.float64).reshape(r64.shape) - r64).max()
            rows.append((i, b - a, key, err, bar_of(c["ref32"][key][a:b], r64)))
    return rows


def failures(rows):
    return [f"image {i} ({n} sub-lines) {key}: error {e:.3e} > bar {b:.3e} (x{e / b:.2f})" for i, n, key, e, b in rows if not e <= b]


def pow2_premise(n):
    """The `equal` family's exact property needs P = expf(0 - logf(n)) = 1 / n EXACTLY.  float32(log n) = log n + e, and
    exp(-(log n + e)) = (1 - e) / n rounds to 1 / n only while |e| stays inside half the relative spacing below a power of two, 2^-25.
    For n = 2^k, k = 1 .. 10, e comes out as 1.9e-9 k (float32(ln 2) is 1.9e-9 above ln 2, and the nearest float32 of k ln 2 happens to
    be k times it): a correctly rounded expf gives 1 / n up to n = 128 and 1 / n less one spacing from 256 on.  The device's expf is
    good to one spacing, not correctly rounded, so the property is asserted only where |e| is well inside, below 0.3 x 2^-25:
    n = 2, 4, 8, 16.  Returns |e| / 2^-25."""
    return abs(float(np.float32(np.log(np.float64(n)))) - np.log(np.float64(n))) * 2.0 ** 25


# ---- the module ------------------------------------------------------------------------------------------------------------------

MHA_KEYS = ("merge.weight", "merge.bias", "proj.0.weight", "proj.0.bias", "proj.1.weight", "proj.1.bias", "proj.2.weight", "proj.2.bias")


def mha_case(B=2, n=65, seed=11, shared=False):
    """seeded state_dict (the reference's names and shapes), query and key = value (or one tensor for all three) [B, 256, n], upstream g"""
    rs = np.random.RandomState(seed)
    sd = {}
    for name in ("merge", "proj.0", "proj.1", "proj.2"):
        sd[name + ".weight"] = (rs.standard_normal((256, 256, 1)) / 16.0).astype(np.float32)
        sd[name + ".bias"] = rs.uniform(-0.5, 0.5, 256).astype(np.float32)
    x = rs.standard_normal((B, 256, n)).astype(np.float32)
    src = x if shared else rs.standard_normal((B, 256, n)).astype(np.float32)
    g = rs.standard_normal((B, 256, n)).astype(np.float32)
    return sd, x, src, g


def torch_mha(sd, query, source, g, dtype, shared=False):
    """The module on rows, differentiated by autograd on the CPU at `dtype`: the three projections and the merge are linear layers on the
    rows [B, n, 256] of query / source (key = value = source; `shared`: the query tensor itself), a projection's channel c is (d, h) =
    (c // 4, c % 4), and attn_rows sits between them.  dict message, d_query, d_source (absent when shared) and the eight parameter
    gradients under their state_dict names, float64 arrays"""
    p = {key: torch.tensor(val, dtype=dtype, requires_grad=True) for key, val in sd.items()}
    qt = torch.tensor(query, dtype=dtype, requires_grad=True)
    st = qt if shared else torch.tensor(source, dtype=dtype, requires_grad=True)
    B, _, n = qt.shape

    def layer(name, rows):
        return rows @ p[name + ".weight"][:, :, 0].T + p[name + ".bias"]

    def heads(rows):                       # [B, n, 256] with c = d * 4 + h -> [B, n, 4, 64]
        return rows.reshape(B, n, 64, 4).transpose(2, 3)

    with torch.enable_grad():
        xq, xs = qt.transpose(1, 2), st.transpose(1, 2)
        o, _ = attn_rows(heads(layer("proj.0", xq)), heads(layer("proj.1", xs)), heads(layer("proj.2", xs)))
        msg = layer("merge", o.transpose(2, 3).reshape(B, n, 256)).transpose(1, 2)
        msg.backward(torch.tensor(g, dtype=dtype))
    out = {"message": msg.detach(), "d_query": qt.grad, **{key: t.grad for key, t in p.items()}}
    if not shared:
        out["d_source"] = st.grad
    return {key: val.double().numpy() for key, val in out.items()}


# ---- launching (GPU) ---------------------------------------------------------------------------------------------------------------

def _rows(t):
    return AC.to_kernel_layout(t)


def launch(L, c, layout="packed", need=(True, True, True), device="cuda:0", forward=True, saved=None):
    """The raw entry points on the case.  layout 'packed': q | k | v are column blocks of one [N + SPARE_ROWS, 768] buffer and every
    other tensor has the row stride 256; 'apart': three buffers and every other tensor with the row stride 260.  Sentinel rows sit behind
    row N of every input (and in the padding columns), a marker row behind every output, asserted untouched.  Returns a dict of CPU
    arrays o, lse, dq, dk, dv (what `need` leaves out stays away).  `saved` = (o, lse) device tensors of an earlier launch to use instead of
    running the forward."""
    import ctypes as C
    N = int(c["cu"][-1])
    g = AC._gen("sig_attn_bwd launch", layout)
    ld = 256 if layout == "packed" else 260

    def inp(t):          # [N + SPARE_ROWS, ld] of sentinels around the rows
        buf = AC._sentinel_rows((N + SPARE_ROWS, ld), g)
        buf[:N, :256] = _rows(t)
        return buf.to(device)

    if layout == "packed":
        qkv = AC._sentinel_rows((N + SPARE_ROWS, 768), g)
        qkv[:N] = torch.cat([_rows(c["q"]), _rows(c["k"]), _rows(c["v"])], dim=1)
        qkv = qkv.to(device)
        q, k, v, ldq = qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], 768
    else:
        q, k, v, ldq = inp(c["q"]), inp(c["k"]), inp(c["v"]), ld
    dO = inp(c["dO"])
    new = lambda cols: torch.full((N + 1, cols), MARKER, dtype=torch.float32, device=device)
    o, lse = new(ld), new(4)
    dq, dk, dv = (new(ld) if n else None for n in need)
    cu = torch.from_numpy(np.asarray(c["cu"], dtype=np.int32)).to(device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None
    if saved is None:
        rc = L.linetr_sig_attention_forward(None, q.data_ptr(), ldq, k.data_ptr(), ldq, v.data_ptr(), ldq, cu.data_ptr(), len(c["cu"]) - 1, N,
                                            o.data_ptr(), ld, lse.data_ptr(), st)
        assert rc == 0, L.linetr_last_error()
    else:
        o[:N, :256], lse[:N] = saved
    ws = torch.empty(max(int(L.linetr_sig_attention_backward_workspace_bytes(N)), 16), dtype=torch.uint8, device=device)
    rc = L.linetr_sig_attention_backward(None, q.data_ptr(), ldq, k.data_ptr(), ldq, v.data_ptr(), ldq, o.data_ptr(), ld, lse.data_ptr(),
                                         dO.data_ptr(), ld, cu.data_ptr(), len(c["cu"]) - 1, N, ptr(dq), ld, ptr(dk), ld, ptr(dv), ld,
                                         ws.data_ptr(), ws.numel(), st)
    assert rc == 0, L.linetr_last_error()
    torch.cuda.synchronize()
    res = {}
    for key, t in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        if t is None:
            continue
        assert bool((t[N] == MARKER).all()), f"the row behind {key} was written"
        assert t.shape[1] <= 256 or bool((t[:, 256:] == MARKER).all()), f"the padding columns of {key} were written"
        res[key] = t[:N, :256].cpu().numpy() if key != "lse" else t[:N].cpu().numpy()
    res["_dev"] = (o[:N, :256].clone(), lse[:N].clone())
    return res
