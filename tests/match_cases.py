"""Case generator, references and bars of the matcher's unit tests (tests/test_gpu_match_kernels.py; premises checked on the CPU by
tests/test_match_cases_cpu.py; reused by tools/match_unit_report.py, which writes profiles/match_unit_errors.txt).  Test
infrastructure only.

The restatement is NumPy float64: D = clip(2 - 2 a.b, 0) (models/line_process.py:198-201), the segmented mean with 1 / num_sublines
rows (models/line_transformer.py:277-282) and nn_matcher_distmat's rules (models/nn_matcher.py:3-31: first-index argmin on rows and
columns, strict <, optional mutual check -- oracle.linetr_oracle.mutual_nn).

Families
  exact_clip / exact_lattice   descriptor entries are integers in -2 .. 2 over 8 / over 16 and sub-line counts are 1, 2 or 4: every
            product, every partial sum in any order, 2 - 2 dot and both pooling stages are exact in float32 (checked on the CPU), so
            a kernel must return the float64 Dk BIT FOR BIT and match01 must be the rules applied to it.  Over 8, dot exceeds 1 on
            ~2 % of the entries (the clip, and zeros that tie across blocks); over 16 nothing clips and D sits on a 2^-7 lattice around
            2, where minima tie and a threshold taken from the lattice bites.
  normal    float32 unit descriptors, sub-line counts 1 .. 4.  Two bars, both properties of the references alone:
              reference bar   max |gpu - ref64| <= FACTOR max(max |ref32 - ref64|, 2^-23 max |Dk|) per pair, FACTOR = 8 as in
                              attn_cases.py; ref32 = a sequential float32 accumulation over the 256 channels and float32 pooling;
              forward bound   per entry 2 * 256 * 2^-24 (|a|.|b|) + 4 * 2^-24, carried through the pooling as the same weighted mean,
                              plus (s0 + s1 + 2) * 2^-24 * 4 (s: the sub-line counts of the entry's key-lines) -- never exceeded.
            match01 must be the rules applied to the kernel's own float32 Dk.  A single pair's seed is chosen so that no decision of
            the rules sits within 2 x the reference bar (near_ties): results inside the bar then agree on match01 by arithmetic.
  sentinel  'normal' in the compared pairs; the other pairs of the batch hold +-1e4 descriptors.  (A single pair is launched at a row
            offset behind sentinel rows instead.)
Every launch, whatever the family: SPARE_ROWS of +-1e4 sit behind the descriptor arrays, Dk and match01 are prefilled with a marker
and every pair's region is followed by GUARD marker elements that must survive."""
import functools
import zlib

import numpy as np
import torch

from oracle import linetr_oracle as O

FACTOR = 8.0
SENTINEL = 1.0e4
MARKER = -777.25
MARKER_I = -777
SPARE_ROWS = 8
LEAD_ROWS = 3             # sentinel rows in front of a single pair of the 'sentinel' family
GUARD = 5                 # marker elements behind every pair's Dk and match01 region
MAX_N, MAX_P = 1024, 9    # caps of every case
EXACT = {"exact_clip": 8.0, "exact_lattice": 16.0}
FAMILIES = ("exact_clip", "exact_lattice", "normal", "sentinel")
PATHS = ("three_launch", "fused", "fused_ident")
U24 = 2.0 ** -24

DIST_N = (1, 31, 32, 33, 63, 64, 65, 129)
DIST_OFF = ((1, 129), (33, 65), (63, 65), (31, 32))
POOL_K0 = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 143, 144, 145, 257)   # chunks 1 .. 6, 8, 9, 10, 17
POOL_K1 = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
FUSED_N1 = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1024)
FUSED_K0 = (1, 15, 16, 17, 33)
IDENT_N1 = (1, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1023, 1024)
IDENT_K0 = (1, 15, 16, 17, 33, 257)
POINTS_N = ((1, 33), (31, 65), (32, 32), (33, 1), (65, 31))
# image 0 of the one-launch cases: block 0's 16 key-lines own 45 sub-lines (block 1 starts at 45, no multiple of 16) and key-line 5
# (sub-lines 13 .. 16) straddles the first 16-row tile; with 33 key-lines block 1 owns 16 x 4 = 64 sub-lines: four row tiles
FUSED_HEAD = (1, 2, 4, 4, 2, 4, 1, 4, 4, 2, 4, 4, 1, 2, 4, 2)
FUSED_HEAD_N = (1, 2, 4, 3, 3, 4, 1, 4, 3, 2, 4, 4, 1, 3, 4, 2)      # the same for the normal family: count 3 included


def _rs(*key):
    """A generator seeded by the key's text (stable from process to process, unlike hash())."""
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def allowed_counts(family):
    return (1, 2, 4) if family in EXACT else (1, 2, 3, 4)


def counts_of(family, k, key):
    return tuple(int(c) for c in _rs("counts", family, k, key).choice(allowed_counts(family), k)) if k else ()


def counts_summing(family, n, key):
    """Sub-line counts that add up to exactly n (the last key-line takes what is left, split into allowed counts)."""
    rs, out, left = _rs("sum", family, n, key), [], n
    while left > 0:
        c = int(rs.choice([c for c in allowed_counts(family) if c <= left]))
        out.append(c)
        left -= c
    return tuple(out)


def fused_counts0(family, k0, key):
    head = FUSED_HEAD if family in EXACT else FUSED_HEAD_N
    if k0 <= 16:
        return head[:k0] if k0 > 1 else (4,)
    return head + (4,) * min(16, k0 - 16) + counts_of(family, max(0, k0 - 32), key)


# ---------------------------------------------------------------------------------------------------------------- pairs and references
def _base(family):
    return "normal" if family == "sentinel" else family


@functools.lru_cache(maxsize=None)
def pair(family, c0, c1, seed=0, sentinel=False):
    """One image pair: descriptor rows d0 [n0, 256] / d1 [n1, 256] float32, sub-line -> key-line maps s0 / s1, counts c0 / c1."""
    rs = _rs("pair", family, c0, c1, seed, sentinel)
    out = dict(family=family, c0=c0, c1=c1, k0=len(c0), k1=len(c1), n0=int(sum(c0)), n1=int(sum(c1)), sentinel=sentinel)
    for s, c in (("0", c0), ("1", c1)):
        n = int(sum(c))
        if sentinel:
            d = (SENTINEL * (rs.randint(0, 2, (n, 256)) * 2 - 1)).astype(np.float32)
        elif family in EXACT:
            d = (rs.randint(-2, 3, (n, 256)) / EXACT[family]).astype(np.float32)
        else:
            d = rs.standard_normal((n, 256))
            d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        out["d" + s] = d
        out["s" + s] = np.repeat(np.arange(len(c)), c).astype(np.int32)
    return out


def pool_matrix(c, dtype=np.float64, plus=0):
    """[k, n] rows of 1 / (num_sublines + plus)."""
    c = np.asarray(c, dtype=np.int64)
    A = np.zeros((len(c), int(c.sum())), dtype=dtype)
    A[np.repeat(np.arange(len(c)), c), np.arange(int(c.sum()))] = np.repeat((1.0 / (c + plus)).astype(dtype), c)
    return A


def dk64(p):
    D = (2.0 - 2.0 * (p["d0"].astype(np.float64) @ p["d1"].astype(np.float64).T)).clip(min=0)
    return pool_matrix(p["c0"]) @ D @ pool_matrix(p["c1"]).T


def _pool32(X, c, plus=0):
    """Rows of X pooled per key-line in float32, sub-lines ascending: sum_a w X[a] with w = float32(1) / float32(count + plus)."""
    c = np.asarray(c, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64)
    w = (np.float32(1.0) / (c + plus).astype(np.float32)).astype(np.float32)
    out = np.zeros((len(c), X.shape[1]), dtype=np.float32)
    for q in range(int(c.max()) if len(c) else 0):
        m = c > q
        out[m] = out[m] + w[m, None] * X[start[m] + q]
    return out


def dk32(p, order=1, drop_k=None, plus=0):
    """The float32 chain: a sequential accumulation over the 256 channels (order -1: descending), 2 - 2 dot clipped, then the two
    pooling stages t = sum_a w0 D, Dk = sum_b t w1.  Mutations: drop_k = first channel of a K step of 4 that is left out; plus = 1:
    the weight 1 / (count + 1)."""
    a, b = p["d0"], p["d1"]
    acc = np.zeros((p["n0"], p["n1"]), dtype=np.float32)
    for ch in range(256)[::order]:
        if drop_k is not None and drop_k <= ch < drop_k + 4:
            continue
        acc = acc + a[:, ch, None] * b[None, :, ch]
    D = np.maximum(np.float32(2.0) - np.float32(2.0) * acc, np.float32(0.0))
    t = _pool32(D, p["c0"], plus)
    return np.ascontiguousarray(_pool32(np.ascontiguousarray(t.T), p["c1"], plus).T)


def forward_bound(p):
    """Per entry of Dk, what no float32 evaluation of the formula can exceed (module docstring)."""
    absdot = np.abs(p["d0"]).astype(np.float64) @ np.abs(p["d1"]).astype(np.float64).T
    E = 2 * 256 * U24 * absdot + 4 * U24
    c0, c1 = np.asarray(p["c0"], dtype=np.float64), np.asarray(p["c1"], dtype=np.float64)
    return pool_matrix(p["c0"]) @ E @ pool_matrix(p["c1"]).T + (c0[:, None] + c1[None, :] + 2) * U24 * 4


@functools.lru_cache(maxsize=None)
def reference(family, c0, c1, seed=0):
    """The references of pair(family, c0, c1, seed): ref64, ref32, the reference bar and the forward bound.  Read-only."""
    p = pair(family, c0, c1, seed)
    r64, r32 = dk64(p), dk32(p)
    own = float(np.abs(r32.astype(np.float64) - r64).max()) if r64.size else 0.0
    bar = FACTOR * max(own, 2.0 ** -23 * (float(r64.max()) if r64.size else 0.0))
    out = dict(ref64=r64, ref32=r32, own=own, bar=bar, bound=forward_bound(p))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def nn_rules(dk, thr, mutual, last=False, le=False, merge=None):
    """nn_matcher_distmat's rules as a match01 vector (column or -1).  Mutations: last = last-index argmin; le = `<=` at the
    threshold; merge = 'reverse': the column argmin taken per chunk of 16 rows and merged in reverse chunk order."""
    k0, k1 = dk.shape
    if k0 == 0 or k1 == 0:
        return np.full(k0, -1, dtype=np.int32)
    dm = dk.clip(min=0)
    arg = (lambda m, ax: m.shape[ax] - 1 - np.argmin(np.flip(m, ax), axis=ax)) if last else (lambda m, ax: np.argmin(m, axis=ax))
    j = arg(dm, 1)
    best = dm[np.arange(k0), j]
    keep = best <= thr if le else best < thr
    if mutual:
        back = arg(dm, 0)
        if merge == "reverse":
            bv, back = np.full(k1, np.inf), np.zeros(k1, dtype=np.int64)
            for i0 in range(0, k0, 16)[::-1]:
                a = np.argmin(dm[i0:i0 + 16], axis=0)
                v = dm[i0:i0 + 16][a, np.arange(k1)]
                take = v < bv
                bv[take], back[take] = v[take], a[take] + i0
        keep = keep & (np.arange(k0) == back[j])
    return np.where(keep, j, -1).astype(np.int32)


def oracle_rules(dk, thr, mutual):
    """The same vector from oracle.linetr_oracle.mutual_nn's 0/1 matrix."""
    if dk.size == 0:
        return np.full(dk.shape[0], -1, dtype=np.int32)
    m = O.mutual_nn(dk[None], thr, mutual)[0]
    return np.where(m.any(axis=1), m.argmax(axis=1), -1).astype(np.int32)


def thresholds(family, r64):
    """[(thr, mutual)]: thresholds are float32 values.  Exact families: a value that occurs in Dk -- the median row minimum -- and
    nextafter of it, mutual and one-sided.  Normal: the middle of the widest gap between consecutive row minima of the middle half
    (a single row: a quarter above its minimum), mutual and one-sided, and one above every distance."""
    if r64.size == 0:
        return [(1.0, True), (1.0, False)]
    m = np.sort(r64.min(axis=1))
    if family in EXACT:
        v = np.float32(m[len(m) // 2])
        up = np.nextafter(v, np.float32(np.inf))
        return [(float(v), True), (float(up), True), (float(v), False), (float(up), False)]
    if len(m) == 1:
        v = np.float32(m[0] + 0.25)
    else:
        lo, hi = (len(m) - 1) // 4, max((len(m) - 1) // 4 + 1, 3 * (len(m) - 1) // 4 + 1)
        g = lo + int(np.argmax(np.diff(m[lo:hi + 1])))
        v = np.float32(0.5 * (m[g] + m[g + 1]))
    return [(float(v), True), (float(v), False), (4.5, True)]


def near_ties(ref, thr_list):
    """How many decisions of the rules sit within 2 x the reference bar on ref64: a row or column whose runner-up is that close to
    its minimum, a row minimum that close to a threshold.  Two float32 results that both pass the reference bar (each within `bar`
    of ref64 everywhere) take every decision alike when this is 0 -- that, not luck, is why the paths' match01 must agree."""
    d, tol = ref["ref64"], 2 * ref["bar"]
    if d.size == 0:
        return 0
    n = 0
    for ax in (0, 1):
        if d.shape[ax] > 1:
            two = np.partition(d, 1, axis=ax).take([0, 1], axis=ax)
            n += int((np.diff(two, axis=ax) <= tol).sum())
    rm = d.min(axis=1)
    return n + sum(int((np.abs(rm - t) <= tol).sum()) for t in {t for t, _ in thr_list})


@functools.lru_cache(maxsize=None)
def separated_seed(family, c0, c1, seed):
    """The first seed from 1000 seed on whose normal-family pair has no near tie (near_ties); the exact families keep their seed:
    their ties are the point, and exact.  So the normal family holds NO near tie and no threshold close to a minimum: ties, and
    thresholds on a value of Dk, are covered by the exact families alone."""
    if family in EXACT:
        return seed
    for s in range(1000 * seed, 1000 * seed + 200):
        ref = reference(family, c0, c1, s)
        if near_ties(ref, thresholds(family, ref["ref64"])) == 0:
            return s
    raise RuntimeError("no separated seed")


# ---------------------------------------------------------------------------------------------------------------- cases
def _case(grid, family, specs, check=None, refused=False, **kw):
    """specs: [(c0, c1, seed, sentinel)].  check: the compared pairs (default: all that are not sentinels).  refused: a case that is
    never launched (the refusal tests) may exceed the caps."""
    specs = tuple(specs)
    assert refused or (len(specs) <= MAX_P and all(sum(s[0]) <= MAX_N and sum(s[1]) <= MAX_N for s in specs))
    check = tuple(i for i, s in enumerate(specs) if not s[3]) if check is None else tuple(check)
    name = f"{grid}-{family}-" + "+".join(f"{sum(s[0])}/{len(s[0])}x{sum(s[1])}/{len(s[1])}" for s in specs[:3]) + ("+.." if len(specs) > 3 else "")
    return dict(grid=grid, family=family, base=_base(family), specs=specs, check=check, name=name, lead=0, **kw)


def _single(grid, family, c0, c1, seed=0, **kw):
    c0, c1 = tuple(c0), tuple(c1)
    if not kw.get("refused"):
        seed = separated_seed(_base(family), c0, c1, seed)
    c = _case(grid, family, [(c0, c1, seed, False)], **kw)
    c["lead"] = LEAD_ROWS if family == "sentinel" else 0
    return c


def dist_shapes():
    s = [(n, n) for n in DIST_N]
    for a, b in DIST_OFF:
        s += [(a, b), (b, a)]
    return s


@functools.lru_cache(maxsize=None)
def dist_cases(family):
    """pair_dist_kernel's tile edges: (n0, n1) around the 32 x 32 quarters and the 64 x 64 tile, mixed sub-line counts."""
    f = _base(family)
    return tuple(_single("dist", family, counts_summing(f, a, ("d0", a, b)), counts_summing(f, b, ("d1", a, b)), i) for i, (a, b) in enumerate(dist_shapes()))


def pool_shapes():
    return [(k0, POOL_K1[(i + o) % len(POOL_K1)]) for i, k0 in enumerate(POOL_K0) for o in (0, 5)]


@functools.lru_cache(maxsize=None)
def pool_cases(family):
    """pair_pool_kernel / pair_final_kernel: key-line counts around the 16-row chunk, the 256 x 4 element pass and the 4-chunk loop."""
    f = _base(family)
    return tuple(_single("pool", family, counts_of(f, k0, ("p0", k1)), counts_of(f, k1, ("p1", k0)), i) for i, (k0, k1) in enumerate(pool_shapes()))


def pool_forced_cases(family):
    """the reduced list every (seg1_global, cache_dk) combination runs on"""
    return pool_cases(family)[::7]


@functools.lru_cache(maxsize=None)
def cache_edge_cases(family):
    """k1 = 896 / 897: where the matcher stops keeping the pooled rows in LDS (nothing forced but the three launches)."""
    f = _base(family)
    return tuple(_single("cache_edge", family, counts_of(f, 17, ("c0", k1)), (1,) * (k1 - 40) + (2,) * 40, k1) for k1 in (896, 897))


@functools.lru_cache(maxsize=None)
def fused_cases(family):
    """pair_match_fused_kernel<false>: n1 exactly at the 16-column tile, the two-tile switch (n_ct 8 / 9), the second trip (16 / 17)."""
    f = _base(family)
    out = []
    for i, n1 in enumerate(FUSED_N1):
        for k0 in sorted({FUSED_K0[i % 5], FUSED_K0[(i + 2) % 5]} | ({33} if n1 in (129, 257) else set())):
            out.append(_single("fused", family, fused_counts0(f, k0, n1), counts_summing(f, n1, ("f1", k0)), i))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ident_cases(family):
    """pair_match_fused_kernel<true>: identity maps; gridDim.y splits the columns at 128 / 129."""
    out = []
    for i, n1 in enumerate(IDENT_N1):
        for k0 in sorted({IDENT_K0[i % 6], IDENT_K0[(i + 3) % 6]}):
            out.append(_single("ident", family, (1,) * k0, (1,) * n1, i))
    return tuple(out)


BATCH_DIMS = ((5, 7), (17, 3), (33, 18), (1, 1), (16, 65), (20, 9), (3, 40), (49, 16), (2, 5))   # (k0, k1) of a batch's pairs


@functools.lru_cache(maxsize=None)
def batch_case(family, P, variant=0, parity=0):
    """P heterogeneous pairs (row offsets are multiples of nothing).  Pairs without key-lines sit first, in the middle and last:
    variant 0: k1 = n1 = 0 | k0 = n0 = 0 | k1 = n1 = 0; variant 1 the other way round (P = 2: none).  'sentinel':
    the pairs of `parity` hold +-1e4 and are not compared."""
    f = _base(family)
    specs = []
    empties = {} if P < 3 else {0: variant, P // 2: 1 - variant, P - 1: variant}
    for i in range(P):
        k0, k1 = BATCH_DIMS[(i + 3 * variant) % len(BATCH_DIMS)]
        c0, c1 = counts_of(f, k0, ("b0", i, P)), counts_of(f, k1, ("b1", i, P))
        if i in empties:
            c0, c1 = (c0, ()) if empties[i] == 0 else ((), c1)
        specs.append((c0, c1, 100 + i, family == "sentinel" and i % 2 == parity))
    return _case("batch", family, specs, variant=variant, parity=parity)


def single_cases(family):
    """every P = 1 case of a family"""
    return dist_cases(family) + pool_cases(family) + cache_edge_cases(family) + fused_cases(family) + ident_cases(family)


def legal_paths(case):
    """the paths linetr_debug_match serves the case on"""
    if len(case["specs"]) != 1:
        return (0,)
    c0, c1 = case["specs"][0][:2]
    if not c0 or not c1 or sum(c1) > 1024:
        return (0,)
    return (0, 1, 2) if max(c0) == 1 and max(c1) == 1 else (0, 1)


def case_pairs(case):
    return [pair(case["base"], s[0], s[1], s[2], s[3]) for s in case["specs"]]


def case_reference(case, i):
    s = case["specs"][i]
    return reference(case["base"], s[0], s[1], s[2])


def case_thresholds(case):
    """The thresholds of a case come from its first compared pair that has key-lines on both sides."""
    for i in case["check"]:
        r = case_reference(case, i)["ref64"]
        if r.size:
            return thresholds(case["base"], r)
    return thresholds(case["base"], np.zeros((0, 0)))


# ---------------------------------------------------------------------------------------------------------------- launch and check
def layout(case):
    """Host arrays of a launch: descriptor rows / maps of all pairs one after the other (`lead` sentinel rows in front, SPARE_ROWS
    behind), dims, the four offset arrays and the sizes of the marker-filled outputs."""
    ps = case_pairs(case)
    g = _rs("layout", case["name"])
    sent = lambda n: (SENTINEL * (g.randint(0, 2, (n, 256)) * 2 - 1)).astype(np.float32)
    out = dict(dims=np.array([[p["n0"], p["k0"], p["n1"], p["k1"]] for p in ps], dtype=np.int32).reshape(-1, 4))
    for s in ("0", "1"):
        out["d" + s] = np.concatenate([sent(case["lead"])] + [p["d" + s] for p in ps] + [sent(SPARE_ROWS)])
        out["s" + s] = np.concatenate([np.zeros(case["lead"], np.int32)] + [p["s" + s] for p in ps] + [np.zeros(SPARE_ROWS, np.int32)])
        out["off_n" + s] = case["lead"] + np.concatenate([[0], np.cumsum([p["n" + s] for p in ps])[:-1]]).astype(np.int64)
    out["off_dk"] = np.concatenate([[0], np.cumsum([p["k0"] * p["k1"] + GUARD for p in ps])]).astype(np.int64)
    out["off_k0"] = np.concatenate([[0], np.cumsum([p["k0"] + GUARD for p in ps])]).astype(np.int64)
    return out


class Launcher:
    """A case's operands on the device (uploaded once); run() launches one path and returns the compared pairs' results after
    asserting that every guard kept its marker."""

    def __init__(self, eng, case):
        self.eng, self.case, self.L = eng, case, layout(case)
        dev = eng.device
        self.t = {k: torch.from_numpy(self.L[k]).to(dev) for k in ("d0", "d1", "s0", "s1")}
        self.dk = torch.empty(int(self.L["off_dk"][-1]) + GUARD, dtype=torch.float32, device=dev)
        self.m01 = torch.empty(int(self.L["off_k0"][-1]) + GUARD, dtype=torch.int32, device=dev)

    def run(self, path, thr, mutual, **force):
        L, t = self.L, self.t
        self.dk.fill_(MARKER)
        self.m01.fill_(MARKER_I)
        used = self.eng.debug_match(path, L["dims"], t["d0"], L["off_n0"], t["s0"], t["d1"], L["off_n1"], t["s1"], thr, mutual, self.dk,
                                    L["off_dk"][:-1], self.m01, L["off_k0"][:-1], **force)
        dk, m01 = self.dk.cpu().numpy(), self.m01.cpu().numpy()
        res = {}
        for i, d in enumerate(L["dims"]):
            k0, k1 = int(d[1]), int(d[3])
            a, b = int(L["off_dk"][i]), int(L["off_k0"][i])
            assert (dk[a + k0 * k1:a + k0 * k1 + GUARD] == MARKER).all(), f"{self.case['name']}: the guard behind pair {i}'s Dk was written"
            assert (m01[b + k0:b + k0 + GUARD] == MARKER_I).all(), f"{self.case['name']}: the guard behind pair {i}'s match01 was written"
            res[i] = (dk[a:a + k0 * k1].reshape(k0, k1).copy(), m01[b:b + k0].copy())
        assert (dk[-GUARD:] == MARKER).all() and (m01[-GUARD:] == MARKER_I).all()
        return res, used


def check_pair(family, ref, dk, m01, thr, mutual):
    """Failures (strings) of one pair's result against its references; family: the pair's base family."""
    r64 = ref["ref64"]
    out = []
    if family in EXACT:
        want = r64.astype(np.float32)
        if not np.array_equal(dk.view(np.uint32), want.view(np.uint32)):
            bad = np.argwhere(dk.view(np.uint32) != want.view(np.uint32))
            out.append(f"Dk differs from float64 in {len(bad)} entries, first at {tuple(bad[0])}: {dk[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")
        rules = oracle_rules(r64, thr, mutual)
    else:
        err = np.abs(dk.astype(np.float64) - r64)
        if err.size and not err.max() <= ref["bar"]:
            out.append(f"error {err.max():.3e} > reference bar {ref['bar']:.3e} (x{err.max() / ref['bar']:.1f})")
        if err.size and not (err <= ref["bound"]).all():
            out.append(f"forward bound exceeded in {int((err > ref['bound']).sum())} entries, worst x{(err / ref['bound']).max():.2f}")
        rules = oracle_rules(dk, thr, mutual)
    if not np.array_equal(m01, rules):
        bad = np.nonzero(m01 != rules)[0]
        out.append(f"match01 differs from the rules in {len(bad)} rows, first row {bad[0]}: {m01[bad[0]]} != {rules[bad[0]]} (thr {thr!r}, mutual {mutual})")
    return out


def measure(ref, dk):
    """(max error, reference bar, largest error / forward bound) of a normal-family result (tools/match_unit_report.py)."""
    err = np.abs(dk.astype(np.float64) - ref["ref64"])
    if not err.size:
        return 0.0, ref["bar"], 0.0
    return float(err.max()), ref["bar"], float((err / ref["bound"]).max())


def run_and_check(eng, case, path, **force):
    """Launches `path` at every threshold of the case; returns ({(thr, mutual): {pair: (Dk, match01)}}, failures)."""
    ln = Launcher(eng, case)
    results, fails = {}, []
    for thr, mutual in case_thresholds(case):
        res, used = ln.run(path, thr, mutual, **force)
        if used != path:
            fails.append(f"{case['name']}: path {used} launched instead of {path}")
        results[(thr, mutual)] = res
        for i in case["check"]:
            fails += [f"{case['name']} path {PATHS[path]} {force or ''} pair {i}: {f}"
                      for f in check_pair(case["base"], case_reference(case, i), *res[i], thr, mutual)]
    return results, fails
