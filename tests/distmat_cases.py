"""Case generator, references and bars of the distance-matrix entry points' unit tests (tests/test_gpu_distmat.py; premises checked on
the CPU by tests/test_distmat_cases_cpu.py; reused by tools/distmat_unit_report.py, which writes profiles/distmat_unit_errors.txt).
Test infrastructure only.

The entry points take a distance matrix that already exists: linetr_match_distmat / linetr_match_distmat_f64 (nn_matcher_distmat,
models/nn_matcher.py:3-31), linetr_pool_distmat / linetr_pool_distmat_dense (subline2keyline, models/line_transformer.py:277-282, by
maps and by the matrices the reference passes around).  None goes through match_run: each builds its own pair table, workspace
offsets and grids (linetr_amd/csrc/linetr_match.hip).  The restatements are NumPy float64; nn_rules, pool_matrix, FACTOR and the
markers are match_cases.py's.

Matcher (exact: no arithmetic beyond max(d, 0) and compares -- match01 must equal nn_rules on the float64 of the same matrix, entry
for entry, mutual and one-way, no tolerance)
  Matrices are drawn from a handful of values (VALS32 / VALS64), so ties are the norm, and hold PLANTS: rows and columns whose
  minimum occurs two or three times exactly where a reduction changes hands (tags below), a row of +inf and a row whose minimum is
  the threshold.  A planted row is redrawn from the values >= 0.25 and its plant columns are redrawn likewise, so the plant IS the
  row's / column's minimum; the first of the tied entries holds 0 or -0, a later one -1 (equal only after the clip).
    row tags   s64: columns j | j + 64 (| j + 128): one lane, consecutive strides       l63: columns 63 | 64 (lanes 63 | 0)
               c255: columns 255 | 256                                                   last: columns n1 - 65 | n1 - 1
               merge (f64): 0.25 + 1e-12 | 0.25 - 1e-12, equal in float32 -- the SECOND is the minimum
    col tags   r15 / r63 / r127 / r255: rows 15 | 16, 63 | 64, 127 | 128, 255 | 256 (pair_pool_kernel's chunks, pair_final_kernel's
               groups of four chunks and its remainder loop, the i += 256 loops and match_final_f64_kernel's second block),
               r3: rows 3 | 4 (argmin_rows_f64_kernel's four rows per block); the plants from r63 on sit in columns 256 and 255 when
               they exist (argmin_cols_f64_kernel's second block, the j += 256 loops), r3 / r15 leave those to the row tag c255
    thr / inf  the threshold row and the +inf row

Pooling by maps (linetr_pool_distmat)
  exact   sub-line counts 1, 2 or 4, D entries integers 0 .. 64 over 16: (A0 D) A1^T is exact in float32 in any order; Dk must equal
          the float64 product bit for bit.
  normal  counts 1 .. 5, D uniform in [0, 4]; reference float64 A0 D A1^T with A the float32 matrices pool_matrix builds.  An entry
          passes inside BOTH  FACTOR x the largest error of NumPy's own float32 A0 @ D @ A1.T on the case  and the forward bound
          (s0 + s1 + 2) 2^-24 max|D| over its s0 x s1 segment (s0 + s1 roundings in the order (sum_a w0 D) w1 summed over b; 2 spare).

Pooling by matrices (linetr_pool_distmat_dense)
  A tokeniser's matrix: verdict 0, Dk bit-identical to linetr_pool_distmat on the map, inside the bars above.  Any other matrix:
  the verdict word (include/linetr_hip.h; restated by verdict_rules) has exactly the expected bits and Dk is the product AS GIVEN:
  inside FACTOR x NumPy's float32 error and inside (n0 + n1 + 2) 2^-24 (|A0| |D| |A1|^T) entry-wise (n0 + n1 roundings at most on any
  summation order of the two products).  NaN is compared with equal_nan.

Every launch: outputs prefilled with a marker, GUARD marker elements behind them that must survive, inputs bit-identical after."""
import ctypes as C
import functools
import zlib

import numpy as np

from match_cases import FACTOR, GUARD, MARKER, MARKER_I, nn_rules, pool_matrix

U24 = 2.0 ** -24
WS_FILL = 0x5A                         # byte the workspaces are prefilled with
WS_WORD = 0x5A5A5A5A                   # ... read as an int32
THR32 = np.float32(0.8)
THR32_BELOW, THR32_ABOVE = np.nextafter(THR32, np.float32(0)), np.nextafter(THR32, np.float32(4))
INF = np.float32(np.inf)
VALS32 = np.array([-1.0, -0.0, 0.0, 0.25, THR32_BELOW, THR32, THR32_ABOVE, 1.0, 4.0, INF], dtype=np.float32)
POS32 = VALS32[3:]                     # what the rest of a planted row / column is drawn from
ABOVE32 = VALS32[6:]                   # ... and of the threshold row
THR64 = 0.8 + 1e-12                    # the f64 threshold; the float32 of it is float32(0.8) > THR64
VALS64 = np.array([-1.0, -0.0, 0.0, 0.25, 0.8, 1.0, 4.0, np.inf])
POS64 = VALS64[4:]                     # (0.25 is kept for the 'merge' plant)

MATCH32_N0 = (1, 15, 16, 17, 48, 49, 64, 65, 129, 257)
MATCH32_N1 = (1, 63, 64, 65, 255, 256, 257, 896, 897)
MATCH64_N0 = (1, 3, 4, 5, 255, 256, 257)
MATCH64_N1 = (1, 63, 64, 65, 128, 129, 255, 256, 257)
ROW_TAGS = ("s64", "l63", "c255", "last", "merge")
COL_TAGS = ("r3", "r15", "r63", "r127", "r255")
MUTATIONS32 = ("last", "le", "no_mutual", "no_clip")
MUTATIONS64 = MUTATIONS32 + ("as_f32",)


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------- matcher cases
def match_shapes(dtype):
    """[(n0, n1[, first])]: every n0 with two n1 and every n1 with at least two n0 (a sparse cross), plus float32's 3 x 12000 / 12001
    and shapes whose few rows go to the plant `first`"""
    if dtype == "f32":
        n0s, n1s = MATCH32_N0, MATCH32_N1
        extra = [(3, 12000, "last"), (3, 12001, "last"), (3, 12000, "c255"), (3, 12001, "s64"), (257, 257), (129, 897), (65, 896), (16, 257), (15, 257)]
    else:
        n0s, n1s = MATCH64_N0, MATCH64_N1
        extra = [(257, 257), (5, 257), (256, 129), (255, 65), (3, 257, "c255"), (4, 257, "c255"), (4, 65, "l63"), (5, 256), (257, 63)]
    s = [(n0, n1s[(2 * i + o) % len(n1s)]) for i, n0 in enumerate(n0s) for o in (0, 5)]
    return list(dict.fromkeys(s + extra))


def _row_plants(n1, dtype):
    """[(tag, columns)] that fit n1"""
    out = []
    if dtype == "f64" and n1 >= 3:
        out.append(("merge", (n1 // 3, 2 * n1 // 3)))
    if n1 >= 300:
        out.append(("last", (n1 - 65, n1 - 1)))
    if n1 >= 65:
        j = min(5, n1 - 65)
        out.append(("s64", (j, j + 64) + ((j + 128,) if n1 > j + 128 else ())))
        out.append(("l63", (63, 64)))
    if n1 >= 257:
        out.append(("c255", (255, 256)))
    return out


def _col_plants(n0, dtype):
    """[(tag, rows)] that fit n0"""
    edges = (("r3", 3),) if dtype == "f64" else ()
    edges += (("r15", 15), ("r63", 63), ("r127", 127), ("r255", 255))
    return [(t, (r, r + 1)) for t, r in edges if n0 >= r + 2]


@functools.lru_cache(maxsize=None)
def match_case(dtype, n0, n1, first=None, seed=0):
    """One matrix with its plants.  Returns dict(d, thr, plants = [(tag, kind, rows, cols)], name); d is read-only."""
    rs = _rs("match", dtype, n0, n1, first, seed)
    f64 = dtype == "f64"
    vals, pos, above = (VALS64, POS64, POS64[1:]) if f64 else (VALS32, POS32, ABOVE32)

    def draw(pool, shape):
        base = pool[rs.randint(0, len(pool), shape)]
        if not f64:
            return base
        j = rs.randint(-2, 3, shape) * 1e-12          # distinct distances that are equal in float32
        return np.where(j == 0, base, base + j)       # (-0 + 0 would lose its sign)

    d = draw(vals, (n0, n1))
    if f64:
        d[d < 0] = -1e-12                      # negatives clip to ties at 0
    thr = THR64 if f64 else float(THR32)
    free_rows = list(range(n0))[::-1]          # rows are handed out from the bottom (a first-index rule is tested far from index 0)
    used_cols = set()
    plants, todo = [], []
    for tag, rows in _col_plants(n0, dtype):   # fixed rows, any free column: the later edges take 256 and 255, r3 / r15 leave them to 'c255'
        prefer = (n1 // 2, 1, 2, 3, 4, 0, n1 - 1) if tag in ("r3", "r15") else (256, 255, n1 - 1, n1 // 2, 1, 2, 3, 4, 0)
        col = next((c for c in prefer if 0 <= c < n1 and c not in used_cols), None)
        if col is None or any(r not in free_rows for r in rows):
            continue
        used_cols.add(col)
        for r in rows:
            free_rows.remove(r)
        todo.append((tag, "col", rows, (col,)))
    rp = _row_plants(n1, dtype)
    rot = next((i for i, (t, _) in enumerate(rp) if t == first), (n0 + n1) % max(len(rp), 1))      # a shape with few rows: not always the same plant
    rp = rp[rot:] + rp[:rot]
    for i, (tag, cols) in enumerate(rp + [("inf", (0,))]):    # fixed columns, any free row; the threshold row right behind the first
        if not free_rows:
            break
        if tag == "inf":
            todo.append((tag, tag, (free_rows.pop(0),), cols))
        elif not any(c in used_cols for c in cols):
            used_cols.update(cols)
            todo.append((tag, "row", (free_rows.pop(0),), cols))
        if i == 0 and free_rows:
            todo.append(("thr", "thr", (free_rows.pop(0),), (n1 - 1,)))
    if not rp and not any(t[0] == "thr" for t in todo) and free_rows:
        todo.append(("thr", "thr", (free_rows.pop(0),), (n1 - 1,)))
    # every planted row and plant column is first redrawn from the values that cannot undercut a plant (a redraw may pass through
    # another plant's row or column: it only leaves such values there) ...
    for tag, kind, rows, cols in todo:
        if kind in ("row", "col"):
            for r in rows:
                d[r, :] = draw(pos, n1)
            for c in cols:
                d[:, c] = draw(pos, n0)
    # ... then the plants themselves
    for tag, kind, rows, cols in todo:
        if kind == "row" and tag == "merge":
            d[rows[0], cols[0]], d[rows[0], cols[1]] = 0.25 + 1e-12, 0.25 - 1e-12
        elif kind == "row":
            z = [-0.0, -1e-12 if f64 else -1.0, 0.0]
            for i, c in enumerate(cols):
                d[rows[0], c] = z[i]
        elif kind == "col":
            d[rows[0], cols[0]], d[rows[1], cols[0]] = 0.0, (-1e-12 if f64 else -1.0)
        elif kind == "thr":                         # everything above the threshold, the threshold itself twice
            d[rows[0], :] = draw(above, n1)
            d[rows[0], cols[0]] = d[rows[0], cols[0] // 2] = thr
        else:
            d[rows[0], :] = np.inf
        plants.append((tag, kind, rows, cols))
    d = np.ascontiguousarray(d, dtype=np.float64 if f64 else np.float32)
    return _frozen(dict(d=d, thr=thr, plants=tuple(plants), dtype=dtype, n0=n0, n1=n1, name=f"match-{dtype}-{n0}x{n1}" + (f"-{first}" if first else "")))


@functools.lru_cache(maxsize=None)
def match_cases(dtype):
    return tuple(match_case(dtype, *shape) for shape in match_shapes(dtype))


def match_want(case, mutual, mutation=None):
    """match01 by the rules on the float64 of the case's matrix; `mutation`: one deliberate mistake."""
    d, thr = case["d"].astype(np.float64), case["thr"]
    if mutation == "as_f32":
        d, thr = d.astype(np.float32).astype(np.float64), float(np.float32(thr))
    if mutation == "no_clip":
        return _rules_no_clip(d, thr, mutual)      # (nn_rules always clips)
    return nn_rules(d, thr, mutual and mutation != "no_mutual", last=mutation == "last", le=mutation == "le")


def _rules_no_clip(d, thr, mutual):
    n0, n1 = d.shape
    if n0 == 0 or n1 == 0:
        return np.full(n0, -1, dtype=np.int32)
    j = np.argmin(d, axis=1)
    keep = d[np.arange(n0), j] < thr
    if mutual:
        keep &= np.arange(n0) == np.argmin(d, axis=0)[j]
    return np.where(keep, j, -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- pooling cases
def _counts(family, k, key, last=None):
    allowed = (1, 2, 4) if family == "exact" else (1, 2, 3, 4, 5)
    c = [int(v) for v in _rs("counts", family, k, key).choice(allowed, k)]
    if last is not None and k:
        c[-1] = last
    return tuple(c)


def _summing(family, n, key, straddle=None):
    """Counts that add up to n; straddle = s: a key-line of 4 sub-lines covers s - 2 .. s + 1 (it straddles s - 1 | s)."""
    allowed = (1, 2, 4) if family == "exact" else (1, 2, 3, 4, 5)
    rs, out, at = _rs("sum", family, n, key), [], 0
    while at < n:
        if straddle is not None and at <= straddle - 2 and at + 5 > straddle - 2 and at != straddle - 2:
            c = straddle - 2 - at          # land exactly on the straddling key-line's first sub-line
            c = max(a for a in allowed if a <= c)
        elif straddle is not None and at == straddle - 2:
            c = 4
        else:
            c = int(rs.choice([a for a in allowed if a <= n - at]))
        out.append(c)
        at += c
    return tuple(out)


def pool_shapes(family):
    """[(c0, c1)]: k0 around the 16-row chunk; rows x k1 around the 4 x 256 element pass and its clamped tail; k1 around the LDS row
    cache (896) and the LDS segment table (12000); n0 / n1 around the segment-start scans' 256 stride; a key-line across sub-lines
    255 | 256; a last key-line of 1 and of the largest count."""
    big = 4 if family == "exact" else 5
    f = family
    kk = [(1, 1023), (1, 1024), (17, 1025), (33, 2047), (1, 2049), (16, 64), (15, 65), (16, 128), (17, 896), (15, 897), (33, 17), (16, 1), (1, 1)]
    out = [(_counts(f, k0, ("a", k1), last=(1, big)[i % 2]), _counts(f, k1, ("b", k0), last=(big, 1)[i % 2])) for i, (k0, k1) in enumerate(kk)]
    out.append(((1, 2), (1,) * 11999 + (2,)))               # k1 = 12000 | 12001 at n1 = 12001: the largest matrix is 3 x 12001
    out.append(((2, 1), (1,) * 12001))
    for n in (256, 257, 513):
        out.append((_summing(f, n, ("n0", n), straddle=256 if n > 257 else None), _counts(f, 9, ("nb", n))))
        out.append((_counts(f, 16 + n % 3, ("na", n)), _summing(f, n, ("n1", n), straddle=256 if n > 257 else None)))
    out.append((_summing(f, 300, "s0", straddle=256), _summing(f, 290, "s1", straddle=256)))
    return out


@functools.lru_cache(maxsize=None)
def pool_case(family, c0, c1):
    rs = _rs("pool", family, c0, c1)
    n0, n1 = int(sum(c0)), int(sum(c1))
    D = (rs.randint(0, 65, (n0, n1)) / 16.0).astype(np.float32) if family == "exact" else rs.uniform(0, 4, (n0, n1)).astype(np.float32)
    return _frozen(dict(family=family, c0=c0, c1=c1, k0=len(c0), k1=len(c1), n0=n0, n1=n1, D=D,
                        s0=np.repeat(np.arange(len(c0)), c0).astype(np.int32), s1=np.repeat(np.arange(len(c1)), c1).astype(np.int32),
                        name=f"pool-{family}-{n0}/{len(c0)}x{n1}/{len(c1)}"))


@functools.lru_cache(maxsize=None)
def pool_cases(family):
    return tuple(pool_case(family, c0, c1) for c0, c1 in pool_shapes(family))


def _segmax(D, c0, c1):
    """max |D| over every s0 x s1 segment: [k0, k1]"""
    st0, st1 = np.concatenate([[0], np.cumsum(c0)[:-1]]).astype(np.int64), np.concatenate([[0], np.cumsum(c1)[:-1]]).astype(np.int64)
    return np.maximum.reduceat(np.maximum.reduceat(np.abs(D).astype(np.float64), st0, axis=0), st1, axis=1)


@functools.lru_cache(maxsize=None)
def pool_reference(family, c0, c1):
    """ref64, NumPy's float32 product, its error (`own`), the reference bar and the per-entry forward bound.  Read-only."""
    p = pool_case(family, c0, c1)
    A0, A1 = pool_matrix(c0, np.float32), pool_matrix(c1, np.float32)
    r64 = A0.astype(np.float64) @ p["D"].astype(np.float64) @ A1.astype(np.float64).T
    r32 = A0 @ p["D"] @ A1.T
    own = float(np.abs(r32.astype(np.float64) - r64).max())
    s0, s1 = np.asarray(c0, np.float64), np.asarray(c1, np.float64)
    return _frozen(dict(ref64=r64, ref32=r32, own=own, bar=FACTOR * own, bound=(s0[:, None] + s1[None, :] + 2) * U24 * _segmax(p["D"], c0, c1)))


def check_pooled(family, ref, dk):
    """failures (strings) of a pooled Dk against the references of its case"""
    r64 = ref["ref64"]
    if family == "exact":
        want = r64.astype(np.float32)
        if np.array_equal(dk.view(np.uint32), want.view(np.uint32)):
            return []
        bad = np.argwhere(dk.view(np.uint32) != want.view(np.uint32))
        return [f"Dk differs from float64 in {len(bad)} entries, first at {tuple(bad[0])}: {dk[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"]
    err = np.abs(dk.astype(np.float64) - r64)
    out = []
    if not err.max() <= ref["bar"]:
        out.append(f"error {err.max():.3e} > reference bar {ref['bar']:.3e}")
    if not (err <= ref["bound"]).all():
        out.append(f"forward bound exceeded in {int((~(err <= ref['bound'])).sum())} entries, worst x{(err / np.maximum(ref['bound'], 1e-300)).max():.2f}")
    return out


# ---------------------------------------------------------------------------------------------------------------- dense: verdict and cases
def verdict_rules(A):
    """The verdict bits of ONE matrix as include/linetr_hip.h states them (an independent restatement, column by column)."""
    K, N = A.shape
    nz = ~(A == 0)                                             # NaN counts as non-zero, -0 as zero
    cnt = nz.sum(axis=0)
    m = np.where(cnt > 0, K - 1 - np.argmax(nz[::-1], axis=0), 0)      # the LAST non-zero row, 0 for an empty column
    val = np.where(cnt > 0, A[m, np.arange(N)], np.float32(0))
    bits = 1 if (cnt != 1).any() else 0
    if m[0] != 0 or m[-1] != K - 1 or not np.isin(np.diff(m), (0, 1)).all():
        bits |= 2
    starts = np.flatnonzero(np.r_[True, np.diff(m) != 0])
    lens = np.diff(np.r_[starts, N])
    w = np.repeat((1.0 / lens.astype(np.float64)).astype(np.float32), lens)
    if not (val == w).all():
        bits |= 4
    return bits


def expected_verdict(A0, A1):
    if A0.shape[0] > A0.shape[1] or A1.shape[0] > A1.shape[1]:
        return 1
    return verdict_rules(A0) | verdict_rules(A1)


def sanitised_map(k, n):
    return np.minimum(np.arange(n), k - 1)


def pooled_by_map(D, m0, k0, m1, k1):
    """float64 segmented mean of D by two maps (what the library would return had it pooled a matrix it should have multiplied out)"""
    P0, P1 = np.zeros((k0, len(m0))), np.zeros((k1, len(m1)))
    P0[m0, np.arange(len(m0))] = 1
    P1[m1, np.arange(len(m1))] = 1
    P0 /= np.maximum(P0.sum(axis=1, keepdims=True), 1)
    P1 /= np.maximum(P1.sum(axis=1, keepdims=True), 1)
    return P0 @ D.astype(np.float64) @ P1.T


MUT_N = 300                                                    # sub-lines of the mutated side; its columns 0, 255, 256, N - 1 are visited
MUT_STRADDLE = 256                                             # a key-line of 4 covers sub-lines 254 .. 257
OTHER_COUNTS = (2, 1, 5, 3, 4, 1, 2, 3, 5, 1, 4, 2, 3)         # the untouched side: 13 key-lines, 36 sub-lines


def mut_counts():
    return _summing("normal", MUT_N, "mut", straddle=MUT_STRADDLE)


def mutation_names():
    out = [f"{kind}@{c}" for kind in ("second", "emptycol") for c in (0, 255, 256, MUT_N - 1)]
    out += ["swap_rows", "empty_last_row", "empty_row0", "merge_last_row", "merge_row0"]
    out += [f"{kind}@{where}" for kind in ("ulp_up", "ulp_down", "negated", "nan") for where in ("mid", "straddle_last")]
    return out


def is_ulp(name):
    return name.startswith("ulp_")


def mutate(A, counts, name):
    """One mutation of a tokeniser's matrix (a copy): the smallest change that sets its bit."""
    A = A.copy()
    K, N = A.shape
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    row_of = np.repeat(np.arange(K), counts)
    kind, _, where = name.partition("@")
    if kind == "second":                                       # a second non-zero ABOVE the column's own (the map keeps its row), below in column 0
        c = int(where)
        A[row_of[c] - 1 if row_of[c] > 0 else 1, c] = np.float32(0.5)
    elif kind == "emptycol":
        A[:, int(where)] = 0
    elif kind == "swap_rows":
        r = K // 2
        A[[r, r + 1]] = A[[r + 1, r]]
    elif kind == "empty_last_row":
        A[K - 1] = 0
    elif kind == "empty_row0":
        A[0] = 0
    elif kind in ("merge_last_row", "merge_row0"):             # a key-line without sub-lines, every column still with one well-valued entry
        gone, to = (K - 1, K - 2) if kind == "merge_last_row" else (0, 1)
        A[gone] = 0
        lo, hi = min(start[gone], start[to]), max(start[gone + 1], start[to + 1])
        A[to, lo:hi] = np.float32(1.0 / float(hi - lo))
    else:
        ks = int(row_of[MUT_STRADDLE])                         # the straddling key-line
        if where == "straddle_last":
            r, c = ks, int(start[ks + 1] - 1)
        else:
            r = next(i for i in range(K // 3, K) if counts[i] >= 2 and i != ks)
            c = int(start[r])
        w = A[r, c]
        A[r, c] = {"ulp_up": np.nextafter(w, np.float32(2)), "ulp_down": np.nextafter(w, np.float32(0)), "negated": -w, "nan": np.float32(np.nan)}[kind]
    return A


@functools.lru_cache(maxsize=None)
def dense_mutation_case(side, name):
    """A0, A1, D of one mutation applied to `side` (0 / 1) alone, with the references of the AS-GIVEN product.  name None: the clean pair."""
    cm, co = mut_counts(), OTHER_COUNTS
    Am, Ao = pool_matrix(cm, np.float32), pool_matrix(co, np.float32)
    if name is not None:
        Am = mutate(Am, cm, name)
    A0, A1 = (Am, Ao) if side == 0 else (Ao, Am)
    c0, c1 = (cm, co) if side == 0 else (co, cm)
    D = _rs("mutD", side).uniform(0, 4, (A0.shape[1], A1.shape[1])).astype(np.float32)
    out = dict(A0=A0, A1=A1, D=D, c0=c0, c1=c1, name=f"dense-mut-A{side}-{name}", verdict=expected_verdict(A0, A1))
    out.update(product_reference(A0, D, A1))
    return _frozen(out)


def product_reference(A0, D, A1):
    """float64 A0 D A1^T, NumPy's float32 product, its error on the finite entries, the reference bar and the entry-wise bound"""
    with np.errstate(invalid="ignore"):
        r64 = A0.astype(np.float64) @ D.astype(np.float64) @ A1.astype(np.float64).T
        r32 = A0 @ D @ A1.T
        fin = np.isfinite(r64)
        own = float(np.abs(r32.astype(np.float64) - r64)[fin].max()) if fin.any() else 0.0
        mag = np.abs(A0).astype(np.float64) @ np.abs(D).astype(np.float64) @ np.abs(A1).astype(np.float64).T
    return dict(ref64=r64, ref32=r32, own=own, bar=FACTOR * own, bound=(A0.shape[1] + A1.shape[1] + 2) * U24 * mag)


def check_product(ref, dk):
    """failures of an as-given product against product_reference"""
    r64 = ref["ref64"]
    nan = np.isnan(r64)
    out = []
    if not np.array_equal(np.isnan(dk), nan):
        out.append(f"NaN in {int(np.isnan(dk).sum())} entries, expected in {int(nan.sum())}")
        return out
    err = np.abs(dk.astype(np.float64) - r64)[~nan]
    if err.size and not err.max() <= ref["bar"]:
        out.append(f"error {err.max():.3e} > reference bar {ref['bar']:.3e}")
    if err.size and not (err <= ref["bound"][~nan]).all():
        out.append(f"entry-wise bound exceeded, worst x{(err / np.maximum(ref['bound'][~nan], 1e-300)).max():.2f}")
    return out


AS_GIVEN_K1 = (1, 3, 4, 5)
AS_GIVEN_N1 = (1, 63, 64, 65, 255, 256, 257)
AS_GIVEN_K0, AS_GIVEN_N0 = 33, 40


@functools.lru_cache(maxsize=None)
def as_given_case(k0, n0, k1, n1):
    """dense random matrices (every entry non-zero): verdict 1 when K > N on a side, else whatever verdict_rules says of them"""
    rs = _rs("given", k0, n0, k1, n1)
    A0, A1 = rs.uniform(-1, 1, (k0, n0)).astype(np.float32), rs.uniform(-1, 1, (k1, n1)).astype(np.float32)
    D = rs.uniform(0, 4, (n0, n1)).astype(np.float32)
    out = dict(A0=A0, A1=A1, D=D, name=f"dense-given-{k0}x{n0}@{n0}x{n1}@{n1}x{k1}", verdict=expected_verdict(A0, A1))
    out.update(product_reference(A0, D, A1))
    return _frozen(out)


def as_given_cases():
    out = [as_given_case(AS_GIVEN_K0, AS_GIVEN_N0, k1, n1) for i, n1 in enumerate(AS_GIVEN_N1) for k1 in (AS_GIVEN_K1[i % 4], AS_GIVEN_K1[(i + 1) % 4])]
    out += [as_given_case(AS_GIVEN_K0, AS_GIVEN_N0, k1, 64) for k1 in AS_GIVEN_K1]
    out += [as_given_case(5, 3, 4, 65), as_given_case(5, 7, 5, 3), as_given_case(1, 1, 1, 1)]      # K > N on side 0, on side 1; 1 x 1
    return list({c["name"]: c for c in out}.values())


TOKENISER_N = (255, 256, 257, 513)


def tokeniser_shapes():
    """[(c0, c1)]: N at 255 | 256 | 257 and 513 on either side, a key-line across column 255 | 256 where N allows"""
    out = []
    for n in TOKENISER_N:
        big = _summing("normal", n, ("tok", n), straddle=256 if n >= 258 else None)
        out += [(big, OTHER_COUNTS), (OTHER_COUNTS, big)]
    out.append((mut_counts(), _summing("normal", 290, "tok1", straddle=256)))
    return out


# ---------------------------------------------------------------------------------------------------------------- launches (GPU)
class Raw:
    """The four entry points through the C ABI on marked buffers: outputs prefilled with MARKER / MARKER_I and followed by GUARD
    markers, workspaces prefilled with WS_FILL and sized exactly as the *_workspace_bytes query says; every run asserts that the
    guards survived and the inputs are bit-identical."""

    def __init__(self, eng):
        import torch
        self.t, self.eng, self.L, self.dev = torch, eng, eng._L, eng.device

    def up(self, a):
        return self.t.from_numpy(np.array(a, order="C", copy=True)).to(self.dev)      # (the cases are read-only arrays)

    def ws(self, nbytes, short=0):
        return self.t.full((max(int(nbytes) - short, 1),), WS_FILL, dtype=self.t.uint8, device=self.dev), int(nbytes) - short

    def stream(self):
        return C.c_void_p(self.t.cuda.current_stream(self.dev).cuda_stream)

    def _marked(self, n, dtype):
        return self.t.full((n + GUARD,), MARKER if dtype == self.t.float32 else MARKER_I, dtype=dtype, device=self.dev)

    def _same(self, t, a, what):
        got = t.cpu().numpy()
        assert got.tobytes() == np.ascontiguousarray(a).tobytes(), f"{what} was written"

    def match(self, d, thr, mutual, short=0, null=()):
        """linetr_match_distmat / _f64 by d's dtype -> (code, match01 [n0] or None, the whole marked buffer)"""
        f64 = d.dtype == np.float64
        n0, n1 = d.shape
        fn, wsq = (self.L.linetr_match_distmat_f64, self.L.linetr_match_distmat_f64_workspace_bytes) if f64 else \
                  (self.L.linetr_match_distmat, self.L.linetr_match_distmat_workspace_bytes)
        td = self.up(d) if d.size else self.t.zeros(1, dtype=self.t.float64 if f64 else self.t.float32, device=self.dev)
        m01 = self._marked(n0, self.t.int32)
        ws, wsb = self.ws(wsq(n0, n1), short)
        ptr = lambda name, t: None if name in null else t.data_ptr()
        code = fn(None, ptr("dist", td), n0, n1, float(thr), int(bool(mutual)), ptr("m01", m01), ptr("ws", ws), wsb, self.stream())
        self.t.cuda.synchronize(self.dev)
        got = m01.cpu().numpy()
        if d.size:
            self._same(td, d, "the distance matrix")
        if code != 0:
            return code, None, got
        assert (got[n0:] == MARKER_I).all(), "the guard behind match01 was written"
        return code, got[:n0].copy(), got

    def pool(self, D, s0, k0, s1, k1, short=0, null=()):
        """linetr_pool_distmat -> (code, Dk [k0, k1] or None, the whole marked buffer)"""
        n0, n1 = D.shape
        tD, t0, t1 = self.up(D), self.up(s0), self.up(s1)
        dk = self._marked(k0 * k1, self.t.float32)
        ws, wsb = self.ws(self.L.linetr_pool_distmat_workspace_bytes(k0, k1), short)
        ptr = lambda name, t: None if name in null else t.data_ptr()
        code = self.L.linetr_pool_distmat(None, ptr("dist", tD), n0, n1, ptr("s0", t0), k0, ptr("s1", t1), k1, ptr("dk", dk), ptr("ws", ws), wsb, self.stream())
        self.t.cuda.synchronize(self.dev)
        got = dk.cpu().numpy()
        self._same(tD, D, "the distance matrix")
        self._same(t0, s0, "map 0")
        self._same(t1, s1, "map 1")
        if code != 0:
            return code, None, got
        assert (got[k0 * k1:] == MARKER).all(), "the guard behind Dk was written"
        return code, got[:k0 * k1].reshape(k0, k1).copy(), got

    def dense(self, D, A0, A1, short=0, null=()):
        """linetr_pool_distmat_dense -> (code, Dk or None, the first int32 of the workspace after the call, the whole marked buffer)"""
        (k0, n0), (k1, n1) = A0.shape, A1.shape
        z = lambda a: self.up(a) if a.size else self.t.zeros(1, dtype=self.t.float32, device=self.dev)
        tD, t0, t1 = z(D), z(A0), z(A1)
        dk = self._marked(k0 * k1, self.t.float32)
        ws, wsb = self.ws(self.L.linetr_pool_distmat_dense_workspace_bytes(k0, n0, k1, n1), short)
        ptr = lambda name, t: None if name in null else t.data_ptr()
        code = self.L.linetr_pool_distmat_dense(None, ptr("dist", tD), n0, n1, ptr("A0", t0), k0, ptr("A1", t1), k1, ptr("dk", dk), ptr("ws", ws), wsb,
                                                self.stream())
        self.t.cuda.synchronize(self.dev)
        got = dk.cpu().numpy()
        word = int(ws[:4].view(self.t.int32).item()) if ws.numel() >= 4 else None
        for t, a, what in ((tD, D, "the distance matrix"), (t0, A0, "A0"), (t1, A1, "A1")):
            if a.size:
                self._same(t, a, what)
        if code != 0:
            return code, None, word, got
        assert (got[k0 * k1:] == MARKER).all(), "the guard behind Dk was written"
        return code, got[:k0 * k1].reshape(k0, k1).copy(), word, got
