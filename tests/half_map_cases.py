"""Cases of the half-precision map tests: tests/test_gpu_half_maps.py and tests/test_half_maps_cpu.py read them from here.

The question of every GPU test is the same: does a call that reads a float16 / bfloat16 map IN PLACE (LINETR_DENSE_F16 / LINETR_DENSE_BF16
in `dense_is_nhwc`, or linetr_superpoint_heads_typed) give what the same call gives on the map's exact float32 upcast?  A half element
widens to float32 without rounding and the arithmetic behind the load is the float32 kernel's, so the bar is 0 differing bits
(ragged_cases.DESC_BATCH_BAR, the bar between two batch compositions, is not drawn on).  Half OUTPUTS of the head producer are the float32
outputs rounded to nearest-even, which is what torch's .half() / .bfloat16() do: 0 differing bits again.

Half maps are made ONCE per (seed, shape, type) by rounding a seeded, unit-norm float32 map with torch; the comparison call is fed
`map16.float()`.

Sizes.  The head producer's descriptor kernel works on blocks of 32 cells, its score kernel on blocks of 64; the layout pass on tiles of
64 positions; the 8-byte vector paths need Hc * Wc to be a multiple of 4 (producer) or an 8-byte aligned row (layout pass)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ragged_cases as rc
import sample_cases as sc
from linetr_amd import _native as nat

D = 256
HALF = {"f16": (torch.float16, nat.DENSE_F16), "bf16": (torch.bfloat16, nat.DENSE_BF16)}
KINDS = tuple(HALF)

# ---- head producer: B = 2; HW = 1, 15 (odd: the scalar path), 33, 32, 35, 64, 65
HEAD_B = 2
HEAD_MAPS = ((1, 1), (3, 5), (3, 11), (4, 8), (5, 7), (8, 8), (5, 13))
DESC_BLOCK, SCORE_BLOCK = 32, 64

# ---- layout pass and samplers: 63, 64, 65 positions around the 64-position tile, and an odd product
SAMPLE_MAPS = ((7, 9), (8, 8), (5, 13), (3, 5))
LAYOUT_TILE = 64
SUBNORMAL_CELL = (0, 0)            # 256 channels k * 2^-24, k = 1 .. 256: fp16 subnormals (exact in bfloat16 too: k has at most 8 bits + 256 = 2^8)
MAX_CHANNEL = 7                    # channel of the last cell that holds the type's largest finite value

# ---- pooling kernels alone: T = 5, two images of 8 x 12 cells, three sub-lines of 5, 1 and 3 valid tokens
POOL_T, POOL_HW, POOL_IMAGES = 5, (8, 12), 2
POOL_KERNELS = {1: "cls_pool_online_kernel<1>", 3: "cls_pool_online_kernel<4>"}
#              (n_tok, n_sub, image)   key-line 0: sub-lines of 5 and 1 valid tokens (4 padding tokens); key-line 1: 3 valid, 2 padding
POOL_LINES = ((6, 2, 0), (3, 1, 1))

# ---- whole calls
WHOLE_HW = (64, 96)
SMALL_HW = (40, 24)


def _gen(*key):
    return torch.Generator().manual_seed(int(np.frombuffer(repr(key).encode(), np.uint8).astype(np.int64).sum()) * 7919 + len(repr(key)))


@functools.lru_cache(maxsize=None)
def map32(seed, n, Hc, Wc):
    """seeded unit-norm float32 NCHW map [n, 256, Hc, Wc]"""
    return F.normalize(torch.randn((n, D, Hc, Wc), generator=_gen("half map", seed, n, Hc, Wc)), p=2, dim=1)


@functools.lru_cache(maxsize=None)
def map16(kind, seed, n, Hc, Wc, special=False):
    """the map rounded to `kind` by torch, NCHW.  special: cell SUBNORMAL_CELL of image 0 holds k * 2^-24 in channel k - 1, channel
    MAX_CHANNEL of the last cell of image 0 the largest finite value of the type"""
    m = map32(seed, n, Hc, Wc).clone()
    dtype = HALF[kind][0]
    if special:
        m[0, :, SUBNORMAL_CELL[0], SUBNORMAL_CELL[1]] = special_subnormals()
        m[0, MAX_CHANNEL, Hc - 1, Wc - 1] = torch.finfo(dtype).max
    return m.to(dtype)


def special_subnormals():
    return torch.arange(1, D + 1, dtype=torch.float32) * 2.0 ** -24


def special_points(Hc, Wc):
    """the two pixel coordinates that sample cell (0, 0) and cell (Hc - 1, Wc - 1) at weight 1 under align_corners = 1: the grid
    arithmetic of sample_descriptors maps 3.5 to cell 0 and 8 cells - 1 to the last cell exactly"""
    return torch.tensor([[3.5, 3.5], [8.0 * Wc - 1.0, 8.0 * Hc - 1.0]], dtype=torch.float32)


def centre_points(Hc, Wc):
    """pixel coordinates whose grid coordinate under align_corners = 1 is the cell index wherever the division is exact; the first and
    the last are (special_points)"""
    xs = torch.tensor([3.5 + (8.0 * Wc - 4.5) * i / max(Wc - 1, 1) for i in range(Wc)], dtype=torch.float32)
    ys = torch.tensor([3.5 + (8.0 * Hc - 4.5) * i / max(Hc - 1, 1) for i in range(Hc)], dtype=torch.float32)
    return torch.stack([xs.repeat(Hc), ys.repeat_interleave(Wc)], dim=1)


@functools.lru_cache(maxsize=None)
def sample_points(Hc, Wc):
    """the point sets of tests/sample_cases.py for this map (its 169 border points: map corners, up to 6 px outside; 40 uniform ones)
    and the cell centres"""
    return torch.cat([special_points(Hc, Wc), sc.border_points(Hc, Wc), sc.uniform_points(sc.N_POINTS, Hc, Wc, _gen("points", Hc, Wc)),
                      centre_points(Hc, Wc)]).contiguous()


def straddles(sizes, block):
    """do the sizes hold block - 1 or less, exactly block, and block + 1 or more within one block of it?"""
    sizes = set(sizes)
    return block in sizes and block + 1 in sizes and any(s < block for s in sizes) and any(block < s <= 2 * block for s in sizes)


# ---- guards ----------------------------------------------------------------------------------------------------------------------

def guarded16(a, device, offset=0):
    """rc.guarded for a half tensor: (the allocation, the view of `a` in it) with NaN halves on either side; offset: elements the view is
    moved by off the 16-byte grid (1: a 2-byte-odd address)"""
    a = a.contiguous()
    whole = torch.full((a.numel() + 2 * rc.GUARD + offset,), float("nan"), dtype=a.dtype, device=device)
    view = whole[rc.GUARD + offset:rc.GUARD + offset + a.numel()]
    view.copy_(a.reshape(-1))
    return whole, view.view(a.shape)


def guarded32(a, device):
    """rc.guarded for a torch tensor"""
    return rc.guarded(a.contiguous().numpy(), device)


class Out:
    """one output buffer of `numel` elements of `dtype` between rc.GUARD-word guards of rc.PATTERN; offset_bytes moves the view"""

    def __init__(self, shape, dtype, device, offset_bytes=0):
        n = int(np.prod(shape))
        words = (n * torch.empty((), dtype=dtype).element_size() + 3) // 4
        self.whole = torch.full((words + 2 * rc.GUARD + 4,), rc.PATTERN, dtype=torch.int32, device=device)
        raw = self.whole.view(torch.uint8)[rc.GUARD * 4 + offset_bytes:]
        self.view = raw[:n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)
        self.lo, self.hi = rc.GUARD * 4 + offset_bytes, rc.GUARD * 4 + offset_bytes + n * torch.empty((), dtype=dtype).element_size()

    def guards_intact(self):
        raw, pat = self.whole.view(torch.uint8), torch.full_like(self.whole, rc.PATTERN).view(torch.uint8)
        return bool((raw[:self.lo] == pat[:self.lo]).all() and (raw[self.hi:] == pat[self.hi:]).all())

    def untouched(self):
        return bool((self.whole == rc.PATTERN).all())


def bits_equal(a, b):
    """same shape, same dtype, same bit patterns"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


# ---- the pooling case ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pool_case():
    """records, sub-line map, compact token coordinates and a4 rows of POOL_LINES"""
    T = POOL_T
    recs = np.zeros(len(POOL_LINES), dtype=nat.REC_DTYPE)
    sub2line, first_sub, first_tok = [], 0, 0
    for k, (n_tok, n_sub, image) in enumerate(POOL_LINES):
        assert (n_tok + T - 1) // T == n_sub
        recs[k]["n_tok"], recs[k]["n_sub"], recs[k]["image"] = n_tok, n_sub, image
        recs[k]["first_sub"], recs[k]["first_tok"], recs[k]["line_local"] = first_sub, first_tok, 0
        sub2line += [k] * n_sub
        first_sub += n_sub
        first_tok += n_tok
    g = _gen("pool")
    Hc, Wc = POOL_HW
    cpnt = torch.rand((first_tok + POOL_IMAGES, 2), generator=g) * torch.tensor([8.0 * Wc - 1, 8.0 * Hc - 1])
    cpnt[first_tok:] = 0.0            # the images' padding tokens sit at (0, 0)
    a4 = torch.randn((first_tok + POOL_IMAGES, D), generator=g)
    return dict(recs=recs, sub2line=np.asarray(sub2line, np.int32), N=first_sub, first_pad=first_tok, cpnt=cpnt, a4=a4, T=T)


def pool_valid_tokens():
    """valid tokens per sub-line of the pooling case"""
    c, out = pool_case(), []
    for n in range(c["N"]):
        r = c["recs"][c["sub2line"][n]]
        out.append(min(c["T"], int(r["n_tok"]) - (n - int(r["first_sub"])) * c["T"]))
    return out
