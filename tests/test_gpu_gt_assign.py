"""GPU: the native ground-truth line assignment (linetr_gt_assign, csrc/lt_gtassign.h; Engine.line_ground_truth;
linetr_amd.gt_lines) against the fixture the real reference wrote (tests/golden/gt_assign.npz) and the NumPy restatement that
tests/test_gt_assign_fixture_cpu.py pins to it (tests/gt_assign_reference.py).  Every kernel call goes through the C ABI.

Identity is demanded everywhere.  An entry MAY differ from the reference only where its angle compare lies within R.BAND of flipping
(1e-3 degrees in float32, 1e-9 in float64: a few ulp of an arctan2 result in degrees, times about 30); the inputs are chosen so
that no entry does (asserted here and, on the CPU, in test_gt_assign_fixture_cpu.py::test_band_premise): 0 entries are excluded."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import load
import gt_assign_reference as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
E_ARG = -1
DTYPES = [(np.float32, "f32"), (np.float64, "f64")]
OUTPUTS = ("assign", "lmatches", "found", "match_dir", "overlap_dir", "proj0", "proj1")
SENTINEL, TAIL = 0xA5, 256


@pytest.fixture(scope="module")
def L():
    from linetr_amd import _native as nat
    return nat.lib()


@pytest.fixture(scope="module")
def fix():
    g = load("gt_assign")
    return {k: g[k] for k in g.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def h_pair(H):
    return np.stack([H, np.linalg.inv(H)], axis=1).reshape(len(H), 2, 9)


def run(L, lines0, lines1, H, counts=None, pad=1, M=8, want=OUTPUTS, thres=(3.0, 2.0, 0.3), expect=0, **override):
    """one linetr_gt_assign call with the outputs named in `want` (the others NULL); TAIL sentinel bytes sit behind every output
    and are checked.  Returns the outputs as NumPy arrays."""
    dtype = lines0.dtype
    B, n0, n1 = lines0.shape[0], lines0.shape[1], lines1.shape[1]
    shapes = {"assign": ((B, n0 + pad, n1 + pad), np.float32), "lmatches": ((B, M, 2), np.int32), "found": ((B,), np.int32),
              "match_dir": ((B, 2, n0, n1), np.uint8), "overlap_dir": ((B, 2, n0, n1), dtype), "proj0": ((B, n0, 2, 2), dtype),
              "proj1": ((B, n1, 2, 2), dtype)}
    bufs = {k: torch.full((int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
            for k in want}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None
    d0, d1, dH = dev(lines0), dev(lines1), dev(h_pair(H))
    c0, c1 = (dev(np.asarray(c, np.int32)) for c in counts) if counts is not None else (None, None)
    ws_bytes = L.linetr_gt_assign_workspace_bytes(B, n0, n1)
    ws = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device="cuda")
    a = dict(type=int(dtype == np.float64), l0=d0.data_ptr(), n0=n0, l1=d1.data_ptr(), n1=n1, H=dH.data_ptr(), B=B, pad=pad, M=M,
             ws=ws.data_ptr(), wsb=ws_bytes)
    a.update({k[4:]: v for k, v in override.items()})          # arg_<name>: what the call is told, whatever the buffers are
    code = L.linetr_gt_assign(None, a["type"], a["l0"], a["n0"], a["l1"], a["n1"], a["H"], a["B"], c0.data_ptr() if c0 is not None else None,
                              c1.data_ptr() if c1 is not None else None, thres[0], thres[1], thres[2], a["pad"], ptr("assign"),
                              ptr("lmatches"), a["M"], ptr("found"), ptr("match_dir"), ptr("overlap_dir"), ptr("proj0"), ptr("proj1"),
                              a["ws"], a["wsb"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == expect, code
    out = {}
    for k, buf in bufs.items():
        raw = buf.cpu().numpy()
        assert (raw[-TAIL:] == SENTINEL).all(), f"{k}: written behind the output"
        if expect != 0:
            assert (raw == SENTINEL).all(), f"{k}: written by a refused call"
        out[k] = raw[:-TAIL].view(shapes[k][1]).reshape(shapes[k][0]).copy()
    return out


def check(got, truth, pad, M, overlap_where=None):
    """every output present in `got` against the restatement's / fixture's `truth` (batch_truth layout), bit for bit"""
    for k in ("proj0", "proj1"):
        if k in got:
            assert np.array_equal(got[k], truth[k]), k
    if "match_dir" in got:
        assert np.array_equal(got["match_dir"][:, 0] > 0, truth["match0"]) and np.array_equal(got["match_dir"][:, 1] > 0, truth["match1"])
        assert got["match_dir"].max() <= 1
    if "overlap_dir" in got:
        for d in (0, 1):
            mine, want = got["overlap_dir"][:, d], truth[f"overlap{d}"]
            if overlap_where is not None:
                mine = np.where(overlap_where, mine, 0)
            assert np.array_equal(mine, want, equal_nan=True), f"overlap, direction {d}"
    if "assign" in got:
        a = got["assign"]
        want = truth["assign"].astype(np.float32)
        if pad:
            assert not a[:, -1, :].any() and not a[:, :, -1].any()                 # the zero dustbin
            a = a[:, :-1, :-1]
        assert np.array_equal(a, want)
    if "found" in got:
        assert np.array_equal(got["found"], [len(lm) for lm in truth["lmatches"]])   # never capped
    if "lmatches" in got:
        assert np.array_equal(got["lmatches"], R.padded_list(truth["lmatches"], M))


def fixture_truth(fix, tag):
    lm, found = fix[f"lmatches_{tag}"].astype(np.int32), fix[f"found_{tag}"]
    t = {k: fix[f"{k}_{tag}"] for k in ("proj0", "proj1", "assign")}
    t.update({k: fix[f"{k}_{tag}"] > 0 for k in ("match0", "match1")})
    t.update({k: fix[f"{k}_{tag}"].astype(fix[f"lines0_{tag}"].dtype) for k in ("overlap0", "overlap1")})
    t["lmatches"] = [lm[b, :found[b]] for b in range(len(lm))]
    return t


@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_fixture(L, fix, dtype, tag):
    lines0, lines1, H = fix[f"lines0_{tag}"], fix[f"lines1_{tag}"], fix["H"]
    assert R.batch_truth(lines0, lines1, H)["margin"] >= R.BAND[dtype]             # 0 entries excluded
    truth = fixture_truth(fix, tag)
    both = truth["match0"] & truth["match1"]                                       # (the builder fills its overlap matrices there only)
    M = fix[f"lmatches_{tag}"].shape[1]
    runs = [run(L, lines0, lines1, H, pad=pad, M=M) for pad in (0, 1, 1)]
    for pad, got in zip((0, 1, 1), runs):
        check(got, truth, pad, M, overlap_where=both)
        ex = fix["extra_pairs"]                                                    # calc_overlap where the builder never looks
        for d in (0, 1):
            assert np.array_equal(got["overlap_dir"][:, d][:, ex[:, 0], ex[:, 1]].astype(np.float64), fix[f"extra_overlap{d}_{tag}"])
    for k in OUTPUTS:                                                              # deterministic
        assert np.array_equal(runs[1][k], runs[2][k], equal_nan=True), k


@pytest.mark.parametrize("dtype,tag", DTYPES)
@pytest.mark.parametrize("shape", sorted(R.EDGE_CASES))
def test_edges(L, shape, dtype, tag):
    n0, n1 = shape
    lines0, lines1, H = R.case(R.EDGE_CASES[shape], R.EDGE_B, n0, n1, dtype)
    full = R.batch_truth(lines0, lines1, H)
    assert full["margin"] >= R.BAND[dtype]                                         # 0 entries excluded
    M = max(len(lm) for lm in full["lmatches"]) + 1
    check(run(L, lines0, lines1, H, M=M), full, 1, M)
    if shape == (129, 250):                                                        # the list crosses 64-column words and rows
        lm = full["lmatches"][0]
        assert len(set(lm[:, 0])) > 8 and len(set(lm[:, 1] // 64)) == 4
    counts = ([n0, 0, n0 - 1], [n1 - 1, n1, n1])
    truth = R.batch_truth(lines0, lines1, H, counts=counts)
    most = max(len(lm) for lm in truth["lmatches"])
    for M in (most - 1, most, most + 1):
        if M >= 0:
            check(run(L, lines0, lines1, H, counts=counts, pad=M & 1, M=M), truth, M & 1, M)
    for k in OUTPUTS:                                                              # every optional output NULL in turn
        check(run(L, lines0, lines1, H, counts=counts, M=most, want=[o for o in OUTPUTS if o != k]), truth, 1, most)
    check(run(L, lines0, lines1, H, counts=counts, M=most, want=["found"]), truth, 1, most)


def test_dropins_and_engine(fix):
    from linetr_amd import gt_lines
    from linetr_amd.engine import Engine
    for _, tag in DTYPES:
        lines0, lines1 = fix[f"lines0_{tag}"], fix[f"lines1_{tag}"]
        for b in range(2):
            p0, p1 = fix[f"proj0_{tag}"][b], fix[f"proj1_{tag}"][b]
            m0 = gt_lines.find_line_matches(lines0[b], p1, 3, 2)
            m1 = gt_lines.find_line_matches(lines1[b], p0, 3, 2)
            assert m0.dtype == np.float64 and np.array_equal(m0, fix[f"match0_{tag}"][b]) and np.array_equal(m1.T, fix[f"match1_{tag}"][b])
            lm0 = np.array(np.where((m0 > 0) & (m1.T > 0))).T
            mat0, ov0 = gt_lines.calculate_line_overlaps(lines0[b], p1, lm0)
            mat1, ov1 = gt_lines.calculate_line_overlaps(lines1[b], p0, lm0[:, ::-1])
            assert mat0.dtype == np.float64 and np.array_equal(mat0, fix[f"overlap0_{tag}"][b]) and np.array_equal(mat1.T, fix[f"overlap1_{tag}"][b])
            assert np.array_equal(ov0, mat0[lm0[:, 0], lm0[:, 1]]) and len(ov1) == len(lm0)
            ex = fix["extra_pairs"]
            assert np.array_equal(gt_lines.calculate_line_overlaps(lines0[b], p1, ex)[1], fix[f"extra_overlap0_{tag}"][b])
    eng = Engine.heads_only("cuda:0")
    lines0, lines1, H = fix["lines0_f32"], fix["lines1_f32"], fix["H"]
    res = eng.line_ground_truth(lines0, dev(lines1), H, directions=True, projected=True)
    M = int(48 * 1.5)
    assert res["lmatches"].shape == (3, M, 2) and np.array_equal(res["lmatches"].cpu().numpy(), fix["lmatches_f32"].astype(np.int32))
    assert np.array_equal(res["assign"].cpu().numpy()[:, :-1, :-1], fix["assign_f32"].astype(np.float32))
    assert np.array_equal(res["proj0"].cpu().numpy(), fix["proj0_f32"]) and res["overlap_dir"].dtype == torch.float32
    # a list that does not fit: once more with room for all; one pair as [n, 2, 2]; float64 selects the other instance
    small = eng.line_ground_truth(lines0, lines1, H, max_matches=1, dustbin=False)
    most = int(fix["found_f32"].max())
    assert small["lmatches"].shape == (3, most, 2) and np.array_equal(small["lmatches"].cpu().numpy(), fix["lmatches_f32"][:, :most].astype(np.int32))
    assert small["assign"].shape == (3, 48, 40) and np.array_equal(small["found"].cpu().numpy(), fix["found_f32"])
    one = gt_lines.line_ground_truth(fix["lines0_f64"][1], fix["lines1_f64"][1], H[1])
    assert np.array_equal(one["assign"].cpu().numpy()[0, :-1, :-1], fix["assign_f64"][1].astype(np.float32))
    # the assignment goes straight into the validation step: the same dict as the reference's matrix gives
    v = load("val_step")
    d0, d1 = dev(v["desc0"]), dev(v["desc1"])
    mine = eng.line_ground_truth(lines0[:, :40], lines1, H)["assign"]
    want = np.zeros((3, 41, 41), np.float32)
    want[:, :40, :40] = fix["assign_f32"][:, :40]
    a, b = eng.val_step(d0, d1, assign=mine, nn_thresh=0.7), eng.val_step(d0, d1, assign=dev(want), nn_thresh=0.7)
    for k in a:
        x, y = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a[k], b[k]))
        assert np.array_equal(x, y, equal_nan=True), k


def test_bad_arguments(L, fix):
    from linetr_amd import _native as nat
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "linetr_hip.h")).read()
    for name in ("linetr_gt_assign_workspace_bytes", "linetr_gt_assign"):
        assert name + "(" in hdr and name in nat.EXPORTS and hasattr(L, name)
    assert L.linetr_abi_version() == 6
    lines0, lines1, H = fix["lines0_f32"], fix["lines1_f32"], fix["H"]
    bad = [dict(arg_B=0), dict(arg_B=-1), dict(arg_n0=0), dict(arg_n1=-3), dict(arg_M=-1), dict(arg_pad=2), dict(arg_pad=-1),
           dict(arg_type=2), dict(arg_type=-1), dict(arg_l0=None), dict(arg_l1=None), dict(arg_H=None), dict(arg_ws=None)]
    for o in bad:
        run(L, lines0, lines1, H, expect=E_ARG, **o)                               # (run() checks that nothing was written)
    run(L, lines0, lines1, H, expect=E_ARG, arg_wsb=L.linetr_gt_assign_workspace_bytes(3, 48, 40) - 1)
    assert L.linetr_gt_assign_workspace_bytes(0, 48, 40) == 0 and L.linetr_gt_assign_workspace_bytes(3, 48, 0) == 0
    run(L, lines0, lines1, H)
