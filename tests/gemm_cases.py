"""Case generator and error measures of the GEMM tile unit tests (tests/test_gpu_gemm_tiles.py; reused by
tools/gemm_unit_report.py, which writes profiles/gemm_unit_errors.txt).  Test infrastructure only.

A case is one problem  Y_g = norm(act([A_g | A2_g] W_g^T + b_g) (+ R)) (+ add2)  with seeded CPU inputs and two CPU references of the
same formula, float64 (`ref64`) and plain float32 torch (`ref32`).  Input families:

  exact     every entry of A, A2, W, bias and R is an integer in [-8, 8] times 2^-2, taken from a hash of its (row, column): such
            values sit wholly in the first bf16 plane and in fp16, every product is an integer times 2^-4 and with K <= 1024 every
            partial sum stays below 2^12 -- exact in fp32 in ANY summation order.  So every tile in every precision mode must equal
            float64 BIT FOR BIT (activation none / ReLU / the distance epilogue, residual, A2, groups), and two swapped rows, columns
            or K tiles change the result.  `exact_is_exact` checks the premise on the CPU: ref32 == ref64.
  onehot    A row m is a single 1 at column (7 m + 3) % K, W is `exact`: Y reproduces the selected column of W, so a failure names
            the lane and the K position that went wrong.  Bit for bit as well.
  normal    unit-variance A, W / sqrt(K).  Bar for f32 and bf16x6 (fp32-class arithmetic, DESIGN section 4, as in attn_cases.py):
                max |gpu - ref64| <= 8 max(max |ref32 - ref64|, 2^-23 max |ref64|)     per case;
            for the two-plane modes the tolerances tests/test_gpu_gemm.py states: 4e-6 (f16x3) and 3e-5 (bf16x3) of max |ref64|.
            The bars are properties of the references and the formats, never of a kernel's output.
  sentinel  `normal` values; the rows behind M of A, A2 and R, the columns behind K / N of the row-strided views and every second
            group's operands hold +-1e4 and Y holds a marker: nothing outside the [M, N] views of the compared groups may change.

`launch` puts EVERY family into buffers with sentinel surroundings and a marked output; `normal` only differs from `sentinel` in using
tight (contiguous) views."""
import functools
import zlib

import numpy as np
import torch

FACTOR = 8.0
TWO_PLANE_TOL = {"f16x3": 4e-6, "bf16x3": 3e-5}
MODES = ("f32", "bf16x6", "bf16x3", "f16x3")
SENTINEL = 1.0e4
MARKER = -777.25
SPARE_ROWS = 3
LN_EPS = 1e-6
M_CAP, N_CAP, K_CAP = 769, 768, 1024

# (BM, BN) of every tile the product can launch, by name (Engine.GEMM_SPLIT_TILES / GEMM_F32_TILES / GEMM_WS)
SPLIT_TILES = {"32x32k4": (32, 32), "112x256": (112, 256), "128x64": (128, 64), "256x128": (256, 128), "128x256": (128, 256),
               "64x256": (64, 256), "128x128": (128, 128), "128x128s": (128, 128), "64x64": (64, 64), "64x128": (64, 128)}
F32_TILES = {"128x64": (128, 64), "128x128": (128, 128), "64x128": (64, 128)}
WS = "ws64x256"
K_GRID = (32, 64, 96, 128, 160, 544)          # 1 .. 5 K tiles (shorter than, equal to and one past every prefetch depth) and 17
K_GRID_SMALL = (128, 160, 256, 544)           # 32x32k4 is dispatched from K = 128; 4 waves below K = 256, 8 waves from there (or 4
                                              # waves with one staging buffer at 257 .. 512 blocks: small_blocks())


def small_blocks(M, N):
    """blocks of the K-split kernel's grid (one per 32 x 32 tile)"""
    return -(-M // 32) * (N // 32)


def tiles_of(mode):
    """names of the tiles that run alone in this precision mode (112x256: the two-plane modes, as the dispatcher uses it)"""
    if mode == "f32":
        return tuple(F32_TILES)
    return tuple(t for t in SPLIT_TILES if t != "112x256" or mode != "bf16x6")


def tile_dims(tile, mode):
    return (F32_TILES if mode == "f32" else SPLIT_TILES)[tile]


def n_unit(tile, mode):
    """the smallest N the tile runs at and the step of its N grid: the launchers give every N % 128 != 0 to the 128x64 tile (the
    K-split kernel keeps its 32-wide tiles; the entry point takes N % 64 == 0)"""
    BN = tile_dims(tile, mode)[1]
    return 64 if tile in ("128x64", "32x32k4") else max(BN, 128)


def count_shape(BM, BN, want, unit=64):
    """(M, N) with ceil(M / BM) * (N / BN) == want tiles inside the caps and a ragged last row tile.  Where `want` cannot be
    factored inside the caps: for 7 the largest count below 8 (fewer tiles than XCDs), for 17 the smallest count above 16 that is
    no multiple of 8 (more than two tiles per XCD, with a remainder) -- the properties xcd_tile() is tested for."""
    max_r = -(-M_CAP // BM)
    cols = [n // BN for n in range(unit, N_CAP + 1, unit)]
    for t in [want] + ([6, 5, 4, 3, 2] if want < 8 else [t for t in range(want + 1, 64) if t % 8]):
        for c in cols:
            if t % c == 0 and 1 < t // c <= max_r:
                return (t // c - 1) * BM + 1, c * BN
    raise ValueError((BM, BN, want))


def shape_grid(tile, mode):
    """[(M, N, K)]: the smallest shapes at which the tile can still go wrong.  M in {1, BM - 1, BM, BM + 1, 2 BM + 1} and one M each
    for 7, 8, 9 and 17 tiles; N in {BN, 2 BN, 3 BN} (in legal multiples of 64); K over the K grid.  Not the cross product: every M,
    every N and every K occurs, each K with a ragged M, each M with rotating N and K."""
    if tile == WS:
        return [(M, 256, 128) for M in (1, 63, 64, 65, 129)]
    BM, BN = tile_dims(tile, mode)
    ks = K_GRID_SMALL if tile == "32x32k4" else K_GRID
    bn = n_unit(tile, mode)
    ns = [n for n in (bn, 2 * bn, 3 * bn) if n <= N_CAP]
    ms = [1, BM - 1, BM, BM + 1, 2 * BM + 1]
    if tile == "112x256":
        ms = [1, 111, 112, 113, 225]
    out = []
    for i, M in enumerate(ms):
        out.append((M, ns[i % len(ns)], ks[i % len(ks)]))
    for want in (7, 8, 9, 17):
        M, N = count_shape(BM, BN, want, bn)
        out.append((M, N, ks[(want + 1) % len(ks)]))
    for i, K in enumerate(ks):
        out.append((BM + 1 if i % 2 else 2 * BM + 1, ns[(i + 1) % len(ns)], K))
    for N in ns:
        out.append((BM + 1, N, 96 if tile != "32x32k4" else 160))
    if tile == "32x32k4":
        # 257 .. 512 blocks at K >= 256: the 4-wave variant with ONE staging buffer (gemm_split_small_launch); 14 x 24 = 336 blocks
        out += [(417, 768, 256), (417, 768, 544)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen and s[0] <= M_CAP and s[1] <= N_CAP:
            seen.add(s)
            uniq.append(s)
    return uniq


def _hash_quarters(rows, cols, salt):
    """[rows, cols] float32 of integers in [-8, 8] times 2^-2 from a hash of (row, column, salt)"""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    m = np.uint64(0xFFFFFFFF)
    h = (r * np.uint64(2654435761) + c * np.uint64(40503) + np.uint64(salt) * np.uint64(2246822519) + np.uint64(12345)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & m
    h ^= h >> np.uint64(16)
    return torch.from_numpy(((h % np.uint64(17)).astype(np.int64) - 8).astype(np.float32) * 0.25)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def sentinel_block(shape, g):
    return SENTINEL * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


@functools.lru_cache(maxsize=None)
def problem(family, M, N, K, groups=1, shared_a=True, seed=0):
    """Inputs of one problem and its raw products: A [GA, M, K] (GA = 1 for a shared A, else groups), W [groups * N, K],
    bias [groups * N], R [M, N], gamma / beta [N], add2 [M, N]; acc64 / acc32 [groups, M, N] = A_g W_g^T + b_g in float64 /
    float32.  Nothing here depends on a tile, a precision mode or the split point K1: the cases of every kernel share it."""
    assert K <= K_CAP and N % 64 == 0 and K % 32 == 0
    GA = 1 if shared_a else groups
    g = _gen(family, M, N, K, groups, shared_a, seed)
    if family in ("exact", "onehot"):
        W = _hash_quarters(groups * N, K, 1 + seed)
        bias = _hash_quarters(1, groups * N, 2 + seed)[0]
        R = _hash_quarters(M, N, 3 + seed)
        if family == "exact":
            A = torch.stack([_hash_quarters(M, K, 4 + seed + 10 * a) for a in range(GA)])
        else:
            A = torch.zeros((GA, M, K))
            rows = torch.arange(M)
            for a in range(GA):
                A[a, rows, (7 * rows + 3 + a) % K] = 1.0
    elif family in ("normal", "sentinel"):
        A = torch.randn((GA, M, K), generator=g)
        W = torch.randn((groups * N, K), generator=g) / K ** 0.5
        bias = torch.randn((groups * N,), generator=g)
        R = torch.randn((M, N), generator=g)
    else:
        raise ValueError(family)
    gamma = 1.0 + 0.5 * torch.randn((N,), generator=g)
    beta = torch.randn((N,), generator=g)
    add2 = torch.randn((M, N), generator=g)
    acc = {}
    for dt in (torch.float64, torch.float32):
        acc[dt] = torch.stack([A[i if GA > 1 else 0].to(dt) @ W[i * N:(i + 1) * N].to(dt).t() + bias[i * N:(i + 1) * N].to(dt)
                               for i in range(groups)])
    return dict(family=family, M=M, N=N, K=K, groups=groups, shared_a=shared_a, A=A, W=W, bias=bias, R=R, gamma=gamma, beta=beta,
                add2=add2, acc64=acc[torch.float64], acc32=acc[torch.float32])


def epilogue(x, p, act, residual, norm=0, add2=False):
    """The family's epilogue in x's dtype: a restatement of GemmArgs (csrc/lt_gemm.h) -- activation, then the residual, then the
    row normalisation (LayerNorm with eps inside the sqrt / L2 with floor 1e-12), then add2."""
    dt = x.dtype
    if act == 1:
        x = torch.relu(x)
    elif act == 2:
        x = 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    elif act == 3:
        x = (2.0 - 2.0 * x).clamp(min=0)
    if residual:
        x = x + p["R"].to(dt)
    if norm == 1:
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        x = (x - mean) / torch.sqrt(var + LN_EPS) * p["gamma"].to(dt) + p["beta"].to(dt)
    elif norm == 2:
        x = x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp(min=1e-12)
    if add2:
        x = x + p["add2"].to(dt)
    return x


def references(p, act=0, residual=False, norm=0, add2=False):
    """(ref64, ref32) [groups, M, N]"""
    return epilogue(p["acc64"], p, act, residual, norm, add2), epilogue(p["acc32"], p, act, residual, norm, add2)


def exact_is_exact(p, act, residual):
    """the premise of the zero tolerance: the float32 reference of an exact / onehot case IS the float64 one"""
    r64, r32 = references(p, act, residual)
    return bool((r32.double() == r64).all())


def bar(mode, ref64, ref32):
    """the largest |gpu - ref64| a case allows in this precision mode"""
    top = ref64.abs().max().item() if ref64.numel() else 0.0
    if mode in TWO_PLANE_TOL:
        return TWO_PLANE_TOL[mode] * top
    own = (ref32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    return FACTOR * max(own, 2.0 ** -23 * top)


def _pad(strided, n):
    return n + (36 if strided else 0)      # row stride of a strided view: a multiple of 4 that is no multiple of the 128-byte line


def launch(eng, p, tile, *, act=0, residual=False, K1=0, lda2_extra=8, strided=True, norm=0, add2=False, via_row_norm=False,
           bad_groups=()):
    """Runs the problem on `tile` (a name; -1: the dispatcher's choice).  Every operand sits in a buffer whose other elements -- the
    rows behind M, the columns behind the view of a row-strided operand, the operands of the groups in `bad_groups` -- hold +-1e4,
    and Y is a marked buffer; asserts that nothing outside the [M, N] views changed, and that a call that raises (a refusal) left
    the whole buffer untouched.  Returns (Y [groups, M, N] on the CPU, name of
    the kernel that ran).  norm != 0 keeps Y / R / add2 at row stride 256 (the family's contract)."""
    dev = eng.device
    M, N, K, G = p["M"], p["N"], p["K"], p["groups"]
    GA = p["A"].shape[0]
    g = _gen("pack", M, N, K, G)
    rows = M + SPARE_ROWS
    Ka = K1 if K1 else K
    lda, ldy = _pad(strided, Ka), _pad(strided and not norm, N)
    lda2 = _pad(strided, K - K1) + lda2_extra if K1 else 0
    gA = rows * max(lda, lda2)       # the kernels step A and A2 by the same group stride
    Aflat = sentinel_block((GA, gA), g)
    Abuf = Aflat[:, :rows * lda].view(GA, rows, lda)
    Abuf[:, :M, :Ka] = p["A"][:, :, :Ka]
    if K1:
        A2flat = sentinel_block((GA, gA), g)
        A2buf = A2flat[:, :rows * lda2].view(GA, rows, lda2)
        A2buf[:, :M, :K - K1] = p["A"][:, :, K1:]
    W, bias = p["W"].clone(), p["bias"].clone()
    for b in bad_groups:
        W[b * N:(b + 1) * N] = sentinel_block((N, K), g)
        bias[b * N:(b + 1) * N] = sentinel_block((N,), g)
        if GA > 1:
            Aflat[b] = sentinel_block((gA,), g)
            if K1:
                A2flat[b] = sentinel_block((gA,), g)
    Rbuf = None
    if residual:
        Rbuf = sentinel_block((rows, ldy), g)
        Rbuf[:M, :N] = p["R"]
        Rbuf = Rbuf.to(dev)
    Ybuf = torch.full((G, rows, ldy), MARKER, dtype=torch.float32, device=dev)
    Adev = Aflat.to(dev)
    kw = {}
    if K1:
        kw["A2"] = A2flat.to(dev)[0, :rows * lda2].view(rows, lda2)[:M, :K - K1]
    if norm:
        kw.update(norm=norm, gamma=p["gamma"], beta=p["beta"], eps=LN_EPS, via_row_norm=via_row_norm)
        if add2:
            kw["add2"] = p["add2"].to(dev)
    try:
        _, used = eng.debug_gemm_case(Adev[0, :rows * lda].view(rows, lda)[:M, :Ka], W, bias, Rbuf[:M, :N] if residual else None, act,
                                      groups=G, gA=gA if GA > 1 else 0, gY=Ybuf[0].numel(), tile=tile, out=Ybuf[0, :M, :N], **kw)
    except Exception:
        # a refused call launches nothing: the WHOLE output buffer, the [M, N] views included, still holds its marker
        torch.cuda.synchronize()
        assert bool((Ybuf == MARKER).all()), "a refused call wrote into Y"
        raise
    torch.cuda.synchronize()
    Y = Ybuf[:, :M, :N].cpu()
    Ybuf[:, :M, :N] = MARKER
    assert bool((Ybuf == MARKER).all()), f"{used}: something outside the [M, N] views of Y was written"
    return Y, used


def mismatches(Y, ref64, groups=None):
    """[(group, row, column, got, want)] (the first few) where Y differs from ref64 in any bit"""
    bad = (Y.double() != ref64)
    if groups is not None:
        keep = torch.zeros_like(bad)
        keep[list(groups)] = True
        bad &= keep
    idx = bad.nonzero()
    return int(bad.sum()), [(int(a), int(b), int(c), float(Y[a, b, c]), float(ref64[a, b, c])) for a, b, c in idx[:4]]
