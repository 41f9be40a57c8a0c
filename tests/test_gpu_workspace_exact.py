"""GPU: what the workspace size queries of the matcher and the tokeniser answer is sufficient and exact.  Every case runs twice through
the C ABI: on a generous workspace, then on one of exactly the queried bytes, 256-byte aligned, inside an allocation that carries 4096
marker bytes behind it.  Every output of the two runs must be equal bit for bit and the marker bytes untouched.  The shapes are the
smallest that reach each segment of each layout (linetr_match.hip: match_layout, points_layout, tail_layout, distmat_layout,
distmat_f64_layout; linetr_net.hip: tok_layout); the limits they sit at are read from lt_match.h.  The Python callers of
linetr_match_points (Engine.match_points, nn_matcher.nn_matcher) ask the query and must return what the generous C call returns."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from attn_cases import MARKER
from linetr_amd import _native as nat
from linetr_amd import nn_matcher as NM

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
D = 256
GUARD = 4096
MARKER_I = -777
LT_MATCH_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "linetr_amd", "csrc", "lt_match.h")).read()


def limit(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, LT_MATCH_H).group(1))


PF_MAX_N1, PF_MAX_K, PT_INLINE = limit("PF_MAX_N1"), limit("PF_MAX_K"), limit("PT_INLINE")
LINES = (40, 30, 50, 35)                                   # n0, k0, n1, k1: one pair of ordinary size (the one-launch matcher)
LINES_BEYOND = (40, 30, PF_MAX_N1 + 1, 600)                # image 1 beyond the one-launch matcher: the three launches
POINT_SHAPES = [(33, 31),                                  # the one-launch identity path: only the transposed rows are used
                (17, PF_MAX_N1 + 1)]                       # beyond it: the identity maps and the matcher's part are used too
THR = 1.25


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


def bits(t):
    return t.reshape(-1).view(torch.uint8)


def twice(need, run):
    """run(workspace address, workspace bytes) -> the call's output tensors (marker-filled before the call).  Returns the first run's."""
    need = int(need)
    assert need > 0
    big = torch.full((2 * need + (1 << 20),), 0x5A, dtype=torch.uint8, device="cuda")
    outs = run(big.data_ptr(), big.numel())
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    alloc = torch.full((need + 256 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    o = (-alloc.data_ptr()) % 256
    second = run(alloc.data_ptr() + o, need)
    torch.cuda.synchronize()
    assert len(first) == len(second)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(bits(a), bits(b)), f"output {i} differs between the generous and the exact workspace"
    assert bool((alloc[o + need:o + need + GUARD] == 0xA5).all()), "bytes behind the queried size were written"
    return first


def unit_rows(rs, n):
    d = rs.standard_normal((n, D))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def side(rs, n, k):
    """n sub-lines of k key-lines: (descriptors [n,256], sub-line -> key-line map [n], non-decreasing and onto)"""
    counts = np.ones(k, np.int64)
    np.add.at(counts, rs.randint(0, k, n - k), 1)
    return unit_rows(rs, n), np.repeat(np.arange(k), counts).astype(np.int32)


class MatchCase:
    """P pairs for linetr_match (each side's rows back to back) or linetr_match_gathered (both sides in ONE buffer behind a few rows
    of padding, the maps in another behind a different padding, so that off_s != off_n)"""

    def __init__(self, dims, seed, gathered=False):
        rs = np.random.RandomState(seed)
        self.gathered = gathered
        self.dims = np.ascontiguousarray(dims, dtype=np.int32)
        i64 = np.int64
        sides = [(side(rs, n0, k0), side(rs, n1, k1)) for n0, k0, n1, k1 in dims]
        if gathered:
            rows, maps, off_n, off_s = [unit_rows(rs, 3)], [np.full(5, MARKER_I, np.int32)], [[], []], [[], []]
            for pair in sides:
                for j, (d, s) in enumerate(pair):
                    off_n[j].append(sum(len(r) for r in rows)); off_s[j].append(sum(len(m) for m in maps))
                    rows.append(d); maps.append(s)
            desc, s2l = torch.from_numpy(np.concatenate(rows)).cuda(), torch.from_numpy(np.concatenate(maps)).cuda()
            self.desc, self.s2l = (desc, desc), (s2l, s2l)
            self.off_s = [np.array(o, i64) for o in off_s]
        else:
            self.desc = [torch.from_numpy(np.concatenate([p[j][0] for p in sides])).cuda() for j in (0, 1)]
            self.s2l = [torch.from_numpy(np.concatenate([p[j][1] for p in sides])).cuda() for j in (0, 1)]
            off_n = [np.cumsum([0] + [int(d[2 * j]) for d in dims])[:-1] for j in (0, 1)]
        self.off_n = [np.array(o, i64) for o in off_n]
        kk = [int(d[1]) * int(d[3]) for d in dims]
        self.off_dk, self.off_k0 = np.array(np.cumsum([0] + kk), i64), np.array(np.cumsum([0] + [int(d[1]) for d in dims]), i64)
        self.sums = (sum(int(d[0]) * int(d[2]) for d in dims), sum(int(d[1]) + int(d[3]) for d in dims))

    def need(self, L):
        return L.linetr_match_workspace_bytes(len(self.dims), self.sums[0], 0, self.sums[1])

    def run(self, L, st, ws, ws_bytes):
        dk = torch.full((int(self.off_dk[-1]) + 64,), MARKER, dtype=torch.float32, device="cuda")
        m01 = torch.full((int(self.off_k0[-1]) + 64,), MARKER_I, dtype=torch.int32, device="cuda")
        p = nat.np_ptr
        tail = (THR, 1, dk.data_ptr(), p(self.off_dk), m01.data_ptr(), p(self.off_k0), ws, ws_bytes, st)
        if self.gathered:
            code = L.linetr_match_gathered(None, len(self.dims), p(self.dims), self.desc[0].data_ptr(), p(self.off_n[0]), self.s2l[0].data_ptr(),
                                           p(self.off_s[0]), self.desc[1].data_ptr(), p(self.off_n[1]), self.s2l[1].data_ptr(), p(self.off_s[1]), *tail)
        else:
            code = L.linetr_match(None, len(self.dims), p(self.dims), self.desc[0].data_ptr(), p(self.off_n[0]), self.s2l[0].data_ptr(),
                                  self.desc[1].data_ptr(), p(self.off_n[1]), self.s2l[1].data_ptr(), *tail)
        nat.check(code, L)
        return [dk, m01]


@pytest.mark.parametrize("dims,gathered", [([LINES, (17, 17, 64, 64)], False),            # two pairs: the three launches, o_dist and o_scratch
                                           ([(5, 3, 6, 4)] * (PT_INLINE + 1), False),     # beyond the inline pair table: o_table
                                           ([LINES, (17, 17, 64, 64)], True)])
def test_match_on_exactly_the_queried_workspace(eng, dims, gathered):
    L, st = eng._L, eng._stream()
    case = MatchCase(dims, 31 + len(dims), gathered)
    dk, m01 = twice(case.need(L), lambda ws, nb: case.run(L, st, ws, nb))
    n_dk, n_k0 = int(case.off_dk[-1]), int(case.off_k0[-1])
    assert not bool((dk[:n_dk] == MARKER).any()) and not bool((m01[:n_k0] == MARKER_I).any())
    assert bool((dk[n_dk:] == MARKER).all()) and bool((m01[n_k0:] == MARKER_I).all())


def point_sets(n0, n1):
    """two [256,n] descriptor sets; the second holds noisy copies of some of the first's, so that there are matches"""
    rs = np.random.RandomState(1000 * n0 + n1)
    a, b = unit_rows(rs, n0), unit_rows(rs, n1)
    m = min(n0, n1) // 2
    b[:m] = a[:m] + 0.05 * b[:m]
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return np.ascontiguousarray(a.T), np.ascontiguousarray(b.T.astype(np.float32))


def points_run(L, st, p0, p1, ws, ws_bytes):
    n0, n1 = p0.shape[1], p1.shape[1]
    dist = torch.full((n0 * n1 + 64,), MARKER, dtype=torch.float32, device="cuda")
    m01 = torch.full((n0 + 64,), MARKER_I, dtype=torch.int32, device="cuda")
    nat.check(L.linetr_match_points(None, p0.data_ptr(), n0, p1.data_ptr(), n1, THR, 1, dist.data_ptr(), m01.data_ptr(), ws, ws_bytes, st), L)
    return [dist, m01]


@pytest.fixture(scope="module")
def points_results(eng):
    """computed once: {(n0, n1): (p0, p1 as NumPy, dist [n0,n1], match01 [n0] of the C call)}, the exactness of the query checked on the way"""
    L, st = eng._L, eng._stream()
    res = {}
    for n0, n1 in POINT_SHAPES:
        p0, p1 = point_sets(n0, n1)
        t0, t1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
        dist, m01 = twice(L.linetr_match_points_workspace_bytes(n0, n1), lambda ws, nb: points_run(L, st, t0, t1, ws, nb))
        assert not bool((dist[:n0 * n1] == MARKER).any()) and bool((dist[n0 * n1:] == MARKER).all())
        assert not bool((m01[:n0] == MARKER_I).any()) and bool((m01[n0:] == MARKER_I).all())
        res[n0, n1] = (p0, p1, dist[:n0 * n1].view(n0, n1).cpu().numpy(), m01[:n0].cpu().numpy())
    return res


@pytest.mark.parametrize("shape", POINT_SHAPES)
def test_match_points_on_exactly_the_queried_workspace(points_results, shape):
    _, _, dist, m01 = points_results[shape]
    assert (m01 >= 0).sum() >= min(shape) // 2 - 1          # the planted copies are found: the call did match


@pytest.mark.parametrize("shape", POINT_SHAPES)
def test_python_callers_of_match_points_ask_the_query(eng, points_results, shape):
    p0, p1, dist, m01 = points_results[shape]
    d_e, m_e = eng.match_points(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), THR, True)
    torch.cuda.synchronize()
    assert np.array_equal(d_e.cpu().numpy().view(np.uint32), dist.view(np.uint32)) and np.array_equal(m_e.cpu().numpy(), m01)
    mat, d_n = NM.nn_matcher(p0, p1, THR, True)
    assert d_n.dtype == np.float32 and np.array_equal(d_n[0].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(mat, NM.match01_to_matrix(m01, shape[1]))


@pytest.mark.parametrize("points,lines", [((33, 31), LINES), ((33, 31), LINES_BEYOND), ((33, 31), None), (None, LINES)])
def test_pair_tail_on_exactly_the_queried_workspace(eng, points, lines):
    L, st = eng._L, eng._stream()
    assert LINES_BEYOND[3] <= PF_MAX_K
    np0, np1 = points or (0, 0)
    n0, k0, n1, k1 = lines or (0, 0, 0, 0)
    rs = np.random.RandomState(77)
    keep = []
    ptr = lambda a: keep.append(torch.from_numpy(a).cuda()) or keep[-1].data_ptr()
    p0, p1 = (ptr(a) for a in point_sets(np0, np1)) if points else (None, None)
    (l0, s0), (l1, s1) = ((ptr(d), ptr(s)) for d, s in (side(rs, n0, k0), side(rs, n1, k1))) if lines else ((None, None), (None, None))
    offs = (ctypes.c_int64 * 4)()
    out_bytes = int(L.linetr_pair_tail_output_bytes(np0, np1, k0, k1, offs))

    def run(ws, ws_bytes):
        stage = torch.full((out_bytes + 256,), 0x3C, dtype=torch.uint8).pin_memory()
        nat.check(L.linetr_pair_tail(None, p0, np0, p1, np1, THR, l0, n0, s0, k0, l1, n1, s1, k1, THR, 1, stage.data_ptr(), out_bytes, ws, ws_bytes,
                                     st), L)
        return [stage]

    stage, = twice(L.linetr_pair_tail_workspace_bytes(np0, np1, n0, k0, n1, k1), run)
    host = stage.numpy()
    assert bool((host[out_bytes:] == 0x3C).all())
    for o, n, on in ((offs[0], np0 * np1, points), (offs[1], np0, points), (offs[2], k0 * k1, lines), (offs[3], k0, lines)):
        if on:                                               # (a float or an index of four 0x3C bytes is not a result of these inputs)
            assert not (host[o:o + 4 * n].view(np.uint32) == 0x3C3C3C3C).any()


def test_match_distmat_on_exactly_the_queried_workspace(eng):
    L, st = eng._L, eng._stream()
    rs = np.random.RandomState(5)
    for fn, query, n0, n1, dt in ((L.linetr_match_distmat, L.linetr_match_distmat_workspace_bytes, 17, 64, np.float32),
                                  (L.linetr_match_distmat_f64, L.linetr_match_distmat_f64_workspace_bytes, 5, 64, np.float64)):
        a = rs.uniform(0.1, 2.0, (n0, n1)).astype(dt)
        dist = torch.from_numpy(a).cuda()
        rows, r = np.arange(n0), a.argmin(1)
        want = np.where((a.argmin(0)[r] == rows) & (a[rows, r] < THR), r, -1)       # mutual nearest neighbours under the threshold

        def run(ws, ws_bytes):
            m01 = torch.full((n0 + 64,), MARKER_I, dtype=torch.int32, device="cuda")
            nat.check(fn(None, dist.data_ptr(), n0, n1, THR, 1, m01.data_ptr(), ws, ws_bytes, st), L)
            return [m01]

        m01, = twice(query(n0, n1), run)
        assert np.array_equal(m01[:n0].cpu().numpy(), want) and (want >= 0).any() and bool((m01[n0:] == MARKER_I).all())


def test_tokenize_on_exactly_the_queried_workspace(eng):
    """an NCHW-fed call with out.desc requested: the transposed map at o_nhwc and the global sub-line map at o_s2l are both used"""
    from test_gpu_heads_edges import token_setup, tokens_of
    L, st = eng._L, eng._stream()
    c = token_setup(eng)
    rs = np.random.RandomState(9)
    c["dd"].copy_(torch.from_numpy(rs.standard_normal(c["dd"].numel()).astype(np.float32)))
    c["ds"].copy_(torch.from_numpy(rs.uniform(0, 1, c["ds"].numel()).astype(np.float32)))
    N, T, bufs = c["N"], c["T"], c["bufs"]

    def run(ws, ws_bytes):
        for v in bufs.values():
            v.fill_(MARKER)
        c["s2l"].fill_(-7)
        nat.check(L.linetr_tokenize(None, c["d_recs"].data_ptr(), c["K"], N, 8.0, T, c["dd"].data_ptr(), c["ds"].data_ptr(), 2, c["H"], c["W"], 0, 0,
                                    0, 0, tokens_of(bufs, False), c["s2l"].data_ptr(), ws, ws_bytes, st), L)
        return [*bufs.values(), c["s2l"]]

    outs = dict(zip([*bufs, "s2l"], twice(L.linetr_tokenize_workspace_bytes(2, c["H"], c["W"], N), run)))
    assert N > 0 and not bool((outs["desc"][:N * T * D] == MARKER).any()) and bool((outs["desc"][N * T * D:] == MARKER).all())
    assert bool((outs["s2l"] >= 0).all())
