"""CPU: linetr_prefilter_ragged, the host pre-filter for a batch of differently sized images (every image with its own height, width,
min_length, token_distance and valid mask), against linetr_prefilter image by image and against linetr_prefilter_batch on equal
entries: records and prefix sums byte for byte.  The cases are tests/ragged_cases.py's."""
import numpy as np
import pytest

import ragged_cases as rc
from linetr_amd import _native as nat
from workloads import synth


@pytest.fixture(scope="module")
def L():
    return nat.lib()


@pytest.mark.parametrize("n_threads", [1, 4])
@pytest.mark.parametrize("max_keylines", [-1, 10])
def test_ragged_equals_prefilter_image_by_image(L, max_keylines, n_threads):
    lines, off, table, _masks = rc.batch()
    code, recs, cu_k, cu_n = rc.prefilter_ragged(L, lines, off, table, max_keylines, n_threads)
    nat.check(code, L)
    # the ties planted in images 3 and 7 are reported after this call as after linetr_prefilter_batch
    tied = np.full(9, -1, np.int32)
    assert L.linetr_prefilter_tied_images(nat.np_ptr(tied), 9) == 2 and tied[:2].tolist() == sorted(rc.TIED)
    assert cu_k[0] == 0 and cu_n[0] == 0
    tok = 0
    for i, rows in enumerate(lines):
        want, n = rc.prefilter_one(L, rows, table[i], max_keylines, i, int(cu_n[i]), tok)
        have = recs[cu_k[i]:cu_k[i + 1]]
        assert len(have) == len(want) and cu_n[i + 1] - cu_n[i] == n, i
        assert have.tobytes() == want.tobytes(), i
        tok += int(want["n_tok"].sum())
    # what the cases are there for: the empty image, the image whose single line [:-1] drops, three sub-lines in the smallest image,
    # the mask at work on its image only, and a cut that bites at max_keylines = 10
    k = np.diff(cu_k)
    assert k[4] == 0 and k[6] == (0 if max_keylines == -1 else 1)
    assert recs[cu_k[1]:cu_k[2]]["n_sub"].max() == 3
    assert (recs[cu_k[2]:cu_k[3]]["sp"][:, 0] >= 0).all() and k[2] < rc.IMAGES[2][5]
    assert k.max() == 10 if max_keylines == 10 else k.max() > 10


@pytest.mark.parametrize("n_threads", [1, 4])
def test_equal_entries_equal_prefilter_batch(L, n_threads):
    """a table of equal entries against the uniform entry point, with one valid mask, at a size where the worker pool is used"""
    H, W, td, ml = 480, 640, 8.0, 16.0
    lines = [synth.synth_lines(9200 + i, 40, H, W) for i in range(9)]
    lines[3][[2, 7], 4] = 33.0
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.int32)
    vm = np.ones((H, W))
    vm[:200] = 0
    table = np.zeros(9, dtype=nat.PREFILTER_IMAGE_DTYPE)
    table[:] = (H, W, ml, td, 0)
    table["valid_mask"][5] = vm.ctypes.data
    vms = (nat.C.c_void_p * 9)()
    vms[5] = vm.ctypes.data
    cat = np.ascontiguousarray(np.concatenate(lines))
    for max_keylines in (-1, 10):
        code, recs, cu_k, cu_n = rc.prefilter_ragged(L, lines, off, table, max_keylines, n_threads, max_tokens=21)
        nat.check(code, L)
        tied_r = np.full(9, -1, np.int32)
        n_tied_r = L.linetr_prefilter_tied_images(nat.np_ptr(tied_r), 9)
        want = np.zeros(len(cat), dtype=nat.REC_DTYPE)
        wk, wn = np.full(10, -7, np.int32), np.full(10, -7, np.int32)
        nat.check(L.linetr_prefilter_batch(nat.np_ptr(cat), nat.np_ptr(off), 9, H, W, rc.BORDER, ml, max_keylines, vms, td, 21, n_threads,
                                           nat.np_ptr(want), len(want), nat.np_ptr(wk), nat.np_ptr(wn)), L)
        tied_b = np.full(9, -1, np.int32)
        assert L.linetr_prefilter_tied_images(nat.np_ptr(tied_b), 9) == n_tied_r == 1 and tied_b[0] == tied_r[0] == 3
        assert np.array_equal(cu_k, wk) and np.array_equal(cu_n, wn)
        assert recs[:cu_k[-1]].tobytes() == want[:wk[-1]].tobytes()


def test_refusals(L):
    lines, off, table, _masks = rc.batch()
    ok = lambda **kw: rc.prefilter_ragged(L, lines, off, kw.pop("table", table), kw.pop("max_keylines", -1), kw.pop("n_threads", 1), **kw)[0]
    assert ok() == 0
    # linetr_prefilter_batch's own
    assert ok(n_threads=-1) == nat.E_ARG
    assert ok(border=-1) == nat.E_ARG
    assert ok(max_tokens=0) == nat.E_ARG
    assert ok(capacity=-1) == nat.E_ARG
    assert ok(capacity=3) not in (0, nat.E_ARG)                    # LINETR_E_CAPACITY
    bad_off = off.copy()
    bad_off[2] = bad_off[1] - 1
    assert rc.prefilter_ragged(L, lines, bad_off, table, -1, 1)[0] == nat.E_ARG
    cu = np.zeros(10, np.int32)
    recs = np.zeros(int(off[-1]), dtype=nat.REC_DTYPE)
    cat = np.ascontiguousarray(np.concatenate(lines))
    args = lambda o, k, n: (nat.np_ptr(cat), o, 9, nat.np_ptr(table), 8, -1, rc.T, 1, nat.np_ptr(recs), len(recs), k, n)
    assert L.linetr_prefilter_ragged(*args(None, nat.np_ptr(cu), nat.np_ptr(cu))) == nat.E_ARG
    assert L.linetr_prefilter_ragged(*args(nat.np_ptr(off), None, nat.np_ptr(cu))) == nat.E_ARG
    assert L.linetr_prefilter_ragged(*args(nat.np_ptr(off), nat.np_ptr(cu), None)) == nat.E_ARG
    # and the table's: no table, a negative size in one entry, a token distance that is not > 0 in the LAST entry -- all before a
    # line is read (the outputs keep their fill)
    assert ok(table=None) == nat.E_ARG
    for field, i, v in (("height", 4, -8), ("width", 0, -1), ("token_distance", 8, 0.0), ("token_distance", 8, float("nan"))):
        t = table.copy()
        t[field][i] = v
        code, r, cu_k, cu_n = rc.prefilter_ragged(L, lines, off, t, -1, 1)
        assert code == nat.E_ARG, (field, i, v)
        assert (cu_k == -7).all() and (cu_n == -7).all() and not r.view(np.uint8).any()
    # no image at all is fine
    code, r, cu_k, cu_n = rc.prefilter_ragged(L, [], np.zeros(1, np.int32), None, -1, 1)
    assert code == 0 and cu_k.tolist() == [0] and cu_n.tolist() == [0]

