"""GPU: the native validation step (linetr_val_step / linetr_assign_from_matches, csrc/lt_valstep.h; Engine.val_step;
linetr_amd.evaluations) against the reference's fixture (tests/golden/val_step.npz) and the NumPy restatement that
tests/test_val_step_fixture_cpu.py pins to it (tests/val_step_reference.py).

The bar for values is the reference's own float32 error on the fixture's data, doubled: 2 * max(ref_err_f64, 2.4e-7).  Measured on
the MI355X: profiles/val_step_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load
import val_step_reference as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
E_ARG = -1


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def fix():
    g = load("val_step")
    return {k: g[k] for k in g.files}


def bar_of(fix):
    return 2 * max(float(fix["ref_err_f64"]), R.FP32_SPACING)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def step(eng, d0, d1, assign, thr, mutual):
    res = eng.val_step(dev(d0), dev(d1), assign=dev(assign), nn_thresh=thr, mutual=mutual)
    for k in ("row_pos", "row_neg", "match01"):
        res[k] = res[k].cpu().numpy()
    return res


def check_against_f64(res, d0, d1, assign, thr, mutual, bar, label=""):
    """selections identical to the float64 restatement, values within `bar`; returns the largest value errors"""
    ref = R.descriptor_loss(d0, d1, assign, np.float64)
    got_rows = np.nonzero(res["row_neg"].reshape(-1) > 0)[0]
    assert np.array_equal(got_rows, ref["rows"])
    assert res["count"] == len(ref["rows"])
    assert np.array_equal(res["row_pos"] > 0, ref["row_pos"] > 0)
    e_pos = np.abs(res["row_pos"] - ref["row_pos"]).max()
    e_neg = np.abs(res["row_neg"] - ref["row_neg"]).max()
    errs = {"row_pos": e_pos, "row_neg": e_neg}
    for k in ("loss", "hardest_positive", "hardest_negative"):
        if len(ref["rows"]):
            errs[k] = abs(res[k] - float(ref[k]))
        else:
            assert np.isnan(res[k])
    print(f"val_step errors {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bar {bar:.3e})")
    assert all(v <= bar for v in errs.values()), errs
    m01 = R.matcher(d0, d1, thr, mutual, np.float64)
    assert np.array_equal(res["match01"], m01)
    cnt = R.counts(m01, assign)
    assert np.array_equal(np.stack([res[k] for k in ("TP", "FP", "FN", "TN")], axis=1), cnt)
    assert np.abs(np.stack([res[k] for k in ("precision", "recall", "f1")], axis=1) - R.prf(cnt)).max() <= 1e-9
    return errs


@pytest.mark.parametrize("mutual", [True, False])
def test_fixture(eng, fix, mutual):
    tag = "mutual" if mutual else "oneway"
    d0, d1, assign, thr = fix["desc0"], fix["desc1"], fix["assign"], float(fix["nn_thresh"])
    res = step(eng, d0, d1, assign, thr, mutual)
    assert np.array_equal(np.nonzero(res["row_neg"].reshape(-1) > 0)[0], fix["anchor_rows"])
    assert np.array_equal(R.with_dustbins(res["match01"]), fix[f"mat_nn_{tag}"])
    assert np.array_equal(np.stack([res[k] for k in ("TP", "FP", "FN", "TN")], axis=1), fix[f"tfpn_{tag}"])
    bar = bar_of(fix)
    check_against_f64(res, d0, d1, assign, thr, mutual, bar, f"fixture B=3 n=40 {tag}")
    for k in ("loss", "hardest_positive", "hardest_negative"):
        assert abs(res[k] - float(fix[k])) <= bar, k
    assert np.abs(np.stack([res[k] for k in ("precision", "recall", "f1")], axis=1) - fix[f"prf_{tag}"]).max() <= 1e-9


def quarter_vectors():
    """8 + 8 descriptors with four entries of +-0.5: every dot product is a multiple of 0.25, exact in any summation order"""
    def v(*entries):
        x = np.zeros(256, np.float32)
        for p, s in entries:
            x[p] = 0.5 * s
        return x
    u = v((0, 1), (1, 1), (2, 1), (3, 1))
    t = v((0, 1), (1, 1), (2, 1), (3, -1))
    cols = [u, t, v((0, 1), (1, 1), (2, 1), (4, 1)), t, v((0, 1), (1, 1), (5, 1), (6, 1)), v((8, 1), (9, 1), (10, 1), (11, 1)),
            v((8, 1), (9, 1), (10, 1), (11, -1)), v((12, 1), (13, 1), (14, 1), (15, 1))]
    rows = [u, t, u, v((0, 1), (1, 1), (20, 1), (21, 1)), v((0, 1), (8, 1), (9, 1), (22, 1)), v((8, 1), (9, 1), (10, 1), (11, -1)),
            v((0, 1), (1, 1), (2, 1), (30, 1)), v((12, 1), (13, 1), (14, 1), (15, 1))]
    assign = np.zeros((1, 9, 9), np.float32)
    for a, c, w in ((0, 0, 1.0), (1, 1, 1.0), (3, 0, 1.0), (4, 5, 1.0), (5, 5, 0.3), (6, 0, 1.0), (7, 6, 1.0)):
        assign[0, a, c] = w
    return np.stack(rows).T[None].copy(), np.stack(cols).T[None].copy(), assign


@pytest.mark.parametrize("mutual", [True, False])
def test_strict_compares_on_exact_arithmetic(eng, mutual):
    d0, d1, assign = quarter_vectors()
    thr = 1.0
    # the case holds what it is meant to hold (float32 restatement: exact here)
    dist = (2 - 2 * R.dots(d0, d1, np.float32))[0]
    sc = R.scores(d0, d1, np.float32)[0]
    assert np.array_equal(dist, sc)
    g = assign[0, :-1, :-1]
    assert dist[3, 0] == 1 and g[3, 0] == 1 and (dist[3][g[3] <= 0] == 1).any()              # neg == pos
    assert dist[4, 5] == 1 and g[4, 5] == 1 and (dist[4][g[4] <= 0] == 1.5).any()            # neg == pos + 0.5
    assert sc[3].min() == thr                                                                # score == nn_thresh
    assert (sc[1] == sc[1].min()).sum() == 2 and sc[1].argmin() == 1                         # two equal row minima
    assert (sc[:, 0] == sc[:, 0].min()).sum() == 2 and sc[2].argmin() == 0                   # two equal column minima
    assert dist[0, 0] == 0 and g[0, 0] == 1                                                  # matched entry with D == 0
    assert g[5, 5] == np.float32(0.3)                                                        # an assign of exactly 0.3
    res = step(eng, d0, d1, assign, thr, mutual)
    ref = R.descriptor_loss(d0, d1, assign, np.float32)
    assert np.array_equal(res["row_pos"], ref["row_pos"]) and np.array_equal(res["row_neg"], ref["row_neg"])
    assert res["row_neg"][0, 3] == -1 and res["row_neg"][0, 4] == -1 and res["row_pos"][0, 0] == 0 and res["row_pos"][0, 5] == 0
    assert res["count"] == len(ref["rows"])
    for k in ("loss", "hardest_positive", "hardest_negative"):
        assert np.array_equal(np.float64(res[k]), np.float64(ref[k]), equal_nan=True)
    m01 = R.matcher(d0, d1, thr, mutual, np.float32)
    assert np.array_equal(res["match01"], m01)
    assert m01[0, 3] == -1 and m01[0, 1] == 1 and m01[0, 2] == (-1 if mutual else 0)
    cnt = R.counts(m01, assign)
    assert np.array_equal(np.stack([res[k] for k in ("TP", "FP", "FN", "TN")], axis=1), cnt)
    assert np.array_equal(np.stack([res[k] for k in ("precision", "recall", "f1")], axis=1), R.prf(cnt))


# seeds chosen on the CPU so that the float64 restatement has every margin >= 1e-5 (asserted below)
EDGE_SEEDS = {(1, 1): 0, (3, 1): 0, (1, 31): 0, (3, 31): 0, (1, 33): 0, (3, 33): 0, (1, 64): 0, (3, 64): 0, (1, 65): 0, (3, 65): 0,
              (1, 250): 1, (3, 250): 1,
              # beyond 256: val_final_kernel's `a += 256` loop runs a second time and val_select_kernel gets a fifth column block
              (1, 256): 0, (2, 256): 0, (1, 257): 0, (2, 257): 0, (1, 300): 0, (2, 300): 0}


@pytest.mark.parametrize("B,n", [(B, n) for n in (1, 31, 33, 64, 65, 250) for B in (1, 3)] + [(B, n) for n in (256, 257, 300) for B in (1, 2)])
def test_tile_edges(eng, fix, B, n):
    d0, d1, assign = R.clustered_case(EDGE_SEEDS[(B, n)], B, n)
    thr = 0.7
    assert R.margins(d0, d1, assign, thr) >= R.MIN_MARGIN
    for mutual in (True, False):
        check_against_f64(step(eng, d0, d1, assign, thr, mutual), d0, d1, assign, thr, mutual, bar_of(fix), f"B={B} n={n} mutual={mutual}")


def test_no_surviving_anchor(eng):
    B, n = 2, 5
    d = np.zeros((B, 256, n), np.float32)
    d[:, :4] = 0.5
    assign = np.zeros((B, n + 1, n + 1), np.float32)
    assign[:, np.arange(n), np.arange(n)] = 1
    res = step(eng, d, d, assign, 0.7, True)
    assert res["count"] == 0 and np.isnan(res["loss"]) and np.isnan(res["hardest_positive"]) and np.isnan(res["hardest_negative"])
    from linetr_amd.evaluations import descriptor_loss
    with pytest.raises(RuntimeError):
        descriptor_loss()({"line_desc0": dev(d), "line_desc1": dev(d)}, {"mat_assign_sublines": dev(assign)})


def test_assign_from_matches(eng, fix):
    B, n, M = 3, 40, 50
    rs = np.random.RandomState(5)
    lm = np.full((B, M, 2), -1, np.int64)
    for b in range(B):
        k = 20 + 5 * b
        lm[b, :k, 0], lm[b, :k, 1] = rs.permutation(n)[:k], rs.permutation(n)[:k]
        lm[b, k] = lm[b, 0]                                   # a duplicate pair
        lm[b, k + 1] = (n, 3)                                 # an unmatched marker in the dustbin row
    want = torch.zeros((B, n + 1, n + 1))
    for i, batch in enumerate(torch.from_numpy(lm)):          # the reference's loop, as written
        batch = batch[batch[:, 0] != -1]
        want[i, batch[:, 0], batch[:, 1]] = 1
    got = eng.assign_from_matches(dev(lm), n)
    assert np.array_equal(got.cpu().numpy(), want.numpy())
    d0, d1 = dev(fix["desc0"]), dev(fix["desc1"])
    a = eng.val_step(d0, d1, assign=got, nn_thresh=0.7)
    b = eng.val_step(d0, d1, lmatches=dev(lm.astype(np.float32)), nn_thresh=0.7)
    for k in a:
        x, y = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a[k], b[k]))
        assert np.array_equal(x, y, equal_nan=True), k


def test_deterministic_and_stream_independent(eng, fix):
    d0, d1, assign = dev(fix["desc0"]), dev(fix["desc1"]), dev(fix["assign"])
    runs = [eng.val_step(d0, d1, assign=assign, nn_thresh=0.7) for _ in range(5)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(eng.val_step(d0, d1, assign=assign, nn_thresh=0.7))
    side.synchronize()
    first = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in runs[0].items()}
    for r in runs[1:]:
        for k, v in r.items():
            assert np.array_equal(first[k], v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v), equal_nan=True), k


def test_surface(eng, fix):
    import types
    import evaluations.criteria
    import evaluations.metric
    import linetr_amd.evaluations as E
    assert evaluations.criteria.descriptor_loss is E.descriptor_loss and evaluations.metric.Result is E.Result
    d0, d1, assign, thr = dev(fix["desc0"]), dev(fix["desc1"]), dev(fix["assign"]), float(fix["nn_thresh"])
    bar = bar_of(fix)
    pred, target = {"line_desc0": d0, "line_desc1": d1}, {"mat_assign_sublines": assign}
    out = E.descriptor_loss()(pred, target)
    for t, k in zip(out, ("loss", "hardest_positive", "hardest_negative")):
        assert t.dim() == 0 and t.device == d0.device and not t.requires_grad and abs(float(t) - float(fix[k])) <= bar
    for mutual, tag in ((True, "mutual"), (False, "oneway")):
        mat = E.nn_matcher_batches(d0, d1, thr, is_mutual_NN=mutual)
        assert mat.dtype == np.float64 and mat.shape == (3, 41, 41) and np.array_equal(mat, fix[f"mat_nn_{tag}"])
        assert np.array_equal(E.nn_matcher_batches(fix["desc0"], fix["desc1"], thr, is_mutual_NN=mutual), mat)     # NumPy in, as metric.py passes
        args = types.SimpleNamespace(dataset_type="homography", nn_thresh=thr, mutual_nn=mutual)
        res = E.Result("val", args)
        assert res.evaluate(pred, target, 0.0, 0) is pred
        assert np.abs(np.array([res.precision, res.recall, res.f1_score]).T - fix[f"prf_{tag}"]).max() <= 1e-9
        meter = E.AverageMeter(args)
        meter.update(res, 0.5, 3)
        mean = meter.average()
        assert abs(mean.precision[0] - fix[f"prf_{tag}"][:, 0].mean()) <= 1e-9 and mean.gpu_time == 0.5 and mean.loss == 0.0
        p, r, f = E.Evaluate_PR(args).get_precision_recall(mat[:, :-1, :-1], fix["assign"][:, :-1, :-1])
        assert np.abs(np.array([p, r, f]).T - fix[f"prf_{tag}"]).max() <= 1e-9
    # the transposed view of [B*n,256] rows (what this build's forward returns) and the rows themselves
    rows0, rows1 = d0.transpose(1, 2).contiguous(), d1.transpose(1, 2).contiguous()
    a = eng.val_step(d0, d1, assign=assign, nn_thresh=thr)
    for x0, x1 in ((rows0.transpose(1, 2), rows1.transpose(1, 2)), (rows0.view(-1, 256), rows1.view(-1, 256))):
        assert not x0.is_contiguous() or x0.dim() == 2
        b = eng.val_step(x0, x1, assign=assign, nn_thresh=thr)
        for k in a:
            x, y = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a[k], b[k]))
            assert np.array_equal(x, y, equal_nan=True), k


def test_argument_errors(eng, fix):
    from linetr_amd import _native as nat
    L = nat.lib()
    B, n = 3, 40
    d0, d1, assign = dev(fix["desc0"]).transpose(1, 2).contiguous(), dev(fix["desc1"]).transpose(1, 2).contiguous(), dev(fix["assign"])
    with pytest.raises(nat.NativeError, match="error -1"):                     # n0 != n1 at the Python surface
        eng.val_step(dev(fix["desc0"]), dev(fix["desc1"][:, :, :39]), assign=assign)
    offs = (C.c_int64 * 4)()
    out_bytes = L.linetr_val_step_output_bytes(B, offs)
    ws_bytes = L.linetr_val_step_workspace_bytes(B, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    host = torch.zeros(out_bytes, dtype=torch.uint8).pin_memory()
    pos = torch.full((B, 2 * n), 7.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(d0p=d0.data_ptr(), n0=n, n1=n, Bc=B, hostp=host.data_ptr(), wsp=ws.data_ptr(), wsb=ws_bytes, asg=assign.data_ptr()):
        return L.linetr_val_step(None, d0p, n0, d1.data_ptr(), n1, asg, Bc, 0.7, 1, pos.data_ptr(), None, None, hostp, out_bytes, wsp, wsb, st)

    assert call(n1=n - 1) == E_ARG
    assert call(Bc=0) == E_ARG and call(Bc=-2) == E_ARG
    assert call(wsb=ws_bytes - 1) == E_ARG
    assert call(d0p=None) == E_ARG and call(asg=None) == E_ARG and call(hostp=None) == E_ARG and call(wsp=None) == E_ARG
    assert L.linetr_assign_from_matches(None, None, B, 4, n, None, st) == E_ARG
    assert L.linetr_assign_from_matches(None, d0.data_ptr(), 65535, 2 ** 31 - 1, 1, assign.data_ptr(), st) == E_ARG   # more pairs than a grid holds
    torch.cuda.synchronize()
    assert (pos == 7.0).all() and not host.numpy().any()                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not (pos == 7.0).all() and host.numpy().any()
