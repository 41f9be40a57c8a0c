"""GPU: fixed-size training samples in one native call (Engine.fixed_size_batch / linetr_fixed_size) against the real
conv_fixed_size (tests/golden/fixed_size.npz), against the per-image path (tokenize + tokenize + cat / slice), its refusals, the
drop-in util_lines.conv_fixed_size, and one training iteration fed by it."""
import numpy as np
import pytest
import torch

import fixed_size_reference as R
import keyline_reference as KR
from workloads import synth

pytestmark = pytest.mark.gpu

HW = (480, 640)
PRE = dict(remove_borders=8, min_length=16, max_keylines=-1, token_distance=R.TD, max_tokens=R.T)
GUARD, MARKER = 64, -777.25


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine.heads_only("cuda:0")


@pytest.fixture(scope="module")
def g():
    return R.fixture()


def maps_of(seeds):
    dd, ds = zip(*(synth.synth_dense_maps_np(int(s), *HW) for s in seeds))
    return torch.from_numpy(np.concatenate(dd)).cuda(), torch.from_numpy(np.concatenate(ds)).cuda()


def prefilter(eng, rows):
    """the native pre-filter with NumPy's own angles, as LineTransformer.preprocess packs its records (line_process.prefilter_tokenize:
    libm's cos / sin may differ from NumPy's in the last ulp, and the fixture holds NumPy's)"""
    from linetr_amd import line_process as lp
    recs, cu_k, cu_n = eng.prefilter(list(rows), *HW, **PRE)
    if len(recs):
        recs["angle"] = lp.get_angles(np.stack([recs["sp"], recs["ep"]], axis=1))
    return recs, cu_k, cu_n


def batch_call(eng, rows, maps, M, **kw):
    recs, cu_k, cu_n = prefilter(eng, rows)
    return eng.fixed_size_batch(recs, cu_k, cu_n, *maps, max_sublines=M, token_distance=R.TD, max_tokens=R.T, **kw), (recs, cu_k, cu_n)


def host(out, b=None):
    sel = slice(None) if b is None else slice(b, b + 1)
    return {k: out[k][sel].cpu().numpy() for k in R.ALL_KEYS + ("num_klns", "num_slns")}


def per_image(eng, rows, maps, b, M, pseudo):
    """the per-image path: Engine.tokenize of the real lines, Engine.tokenize of the pseudo lines with the swapped clip, cat / slice,
    and the key-line arrays / the matrix as conv_fixed_size assembles them"""
    dd, ds = maps[0][b:b + 1], maps[1][b:b + 1]
    recs, cu_k, cu_n = prefilter(eng, [rows])
    K, N = int(cu_k[1]), int(cu_n[1])

    def as_dict(tb):
        return {"klines": tb.klines[None], "length_klines": tb.length[None], "angles": tb.angles[None], "sublines": tb.sublines[None],
                "pnt_sublines": tb.pnt[None], "mask_sublines": tb.mask[None, :, :, None], "resp_sublines": tb.resp[None, :, None],
                "angle_sublines": tb.angle_sub[None], "desc_sublines": tb.desc[None], "score_sublines": tb.score[None, :, :, None],
                "mat_klines2sublines": tb.mat[None] if tb.mat is not None else None}
    if K:
        real = as_dict(eng.tokenize(recs, cu_k, cu_n, dd, ds, token_distance=R.TD, max_tokens=R.T, want_mat=True))
    else:
        shapes = eng.fixed_size_shapes(1, 0, R.T)
        real = {k: torch.zeros(sh, device="cuda") for k, sh in shapes.items()}
    tok = None
    if pseudo is not None:
        precs, n = eng.pack(pseudo["klines"], pseudo["length_klines"], pseudo["angles"], R.TD, R.T)
        tok = as_dict(eng.tokenize(precs, np.array([0, len(precs)], np.int32), np.array([0, n], np.int32), dd, ds, token_distance=R.TD,
                                   max_tokens=R.T, clip_shape=R.RESIZE))
    return R.conv_fixed_size_np({k: v.cpu().numpy() for k, v in real.items()},
                                {k: v.cpu().numpy() for k, v in tok.items() if v is not None} if tok is not None else None, M)


def same_bits(a, b, keys=R.ALL_KEYS + ("num_klns", "num_slns")):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.astype(x.dtype).tobytes(), k


def test_every_fixture_case_equals_the_reference(eng, g):
    for name in R.cases(g):
        M = int(g[f"{name}_M"])
        maps = maps_of([g[f"{name}_seed"]])
        out, _ = batch_call(eng, [g[f"{name}_lines"]], maps, M, pseudo_lines=[R.pseudo_of(g, name)])
        assert out["num_klns"].dtype == torch.int64 and out["num_slns"].dtype == torch.int64
        shapes = eng.fixed_size_shapes(1, M, R.T)
        assert all(tuple(out[k].shape) == sh and out[k].dtype == torch.float32 for k, sh in shapes.items())
        R.check_against_fixture(g, name, host(out))


RAGGED = ("exact", "cut_unsplit", "mostly_pseudo", "empty", "pad_stray", "cut_straddle", "klns_eq_max", "pad_more", "cut_more")


def ragged_rows(g):
    """B = 9 images at M = 16 that mix every branch: padded, exact, cut between and inside key-lines, num_klns == M, (almost) all
    pseudo, no line at all"""
    rows = {n: g[f"{n}_lines"] for n in ("exact", "cut_unsplit", "mostly_pseudo", "pad_stray")}
    rows["empty"] = np.zeros((0, 6))
    # one line of three sub-lines in front of lines of two: sub-lines 15 and 16 belong to the same key-line, the cut falls inside it
    rows["cut_straddle"] = np.concatenate([synth.synth_lines(701, 9, *HW, 200.0, 330.0), np.array([[100.0, 50.0, 500.0, 50.0, 400.0, 0.0]])])
    rows["klns_eq_max"] = synth.synth_lines(702, 17, *HW, 150.0, 330.0)        # 16 of them survive the pre-filter
    rows["pad_more"] = synth.synth_lines(703, 9, *HW, 17.0, 330.0)
    rows["cut_more"] = synth.synth_lines(704, 14, *HW, 100.0, 330.0)
    return [rows[n] for n in RAGGED]


def test_ragged_batch_of_nine_equals_the_per_image_path_bit_for_bit(eng, g):
    M, B = 16, len(RAGGED)
    rows = ragged_rows(g)
    maps = maps_of(range(800, 800 + B))
    # outputs carved between sentinel-filled guards
    shapes = eng.fixed_size_shapes(B, M, R.T)
    sizes = {k: int(np.prod(sh)) for k, sh in shapes.items()}
    pool = torch.full((sum(sizes.values()) + GUARD * (len(sizes) + 1),), MARKER, device="cuda")
    carved, at = {}, GUARD
    for k, sh in shapes.items():
        carved[k] = pool[at:at + sizes[k]].view(sh)
        at += sizes[k] + GUARD
    out, (recs, cu_k, cu_n) = batch_call(eng, rows, maps, M, seed=5, out=carved)
    nk, ns = np.diff(cu_k), np.diff(cu_n)
    print("ragged batch: key-lines", nk.tolist(), "sub-lines", ns.tolist())
    assert nk[3] == 0 and ns[3] == 0 and (ns < M).sum() >= 4 and (ns > M).sum() >= 3 and (ns == M).sum() >= 1 and (nk == M).sum() >= 2
    assert out["num_klns"].tolist() == nk.tolist() and out["num_slns"].tolist() == ns.tolist()
    at = 0
    for k in shapes:                                             # the guards are intact, and every byte between them was written
        assert bool((pool[at:at + GUARD] == MARKER).all()), k
        at += GUARD + sizes[k]
    assert bool((pool[at:at + GUARD] == MARKER).all())
    got = host(out)
    for k in R.ALL_KEYS:
        assert not (got[k] == MARKER).any(), k
    straddles = 0
    for b in range(B):
        want = per_image(eng, rows[b], maps, b, M, out["pseudo_lines"][b])
        same_bits({k: v[b:b + 1] for k, v in got.items()}, want)
        if ns[b] > M:
            mat = got["mat_klines2sublines"][b]
            owner = int(np.flatnonzero(mat[:nk[b], M - 1])[0])
            straddles += 0 < mat[owner].sum() < 1.0
    assert straddles >= 1
    again, _ = batch_call(eng, rows, maps, M, seed=5)
    same_bits(host(again), got)


def test_generator_seed_decides_the_batch(eng, g):
    M = 16
    rows = [g["mostly_pseudo_lines"], g["pad_stray_lines"]]
    maps = maps_of([810, 811])
    a, _ = batch_call(eng, rows, maps, M, seed=11)
    b, _ = batch_call(eng, rows, maps, M, seed=11)
    c, _ = batch_call(eng, rows, maps, M, seed=12)
    same_bits(host(a), host(b))
    assert not torch.equal(a["pnt_sublines"], c["pnt_sublines"])
    for p, q in zip(a["pseudo_lines"], b["pseudo_lines"]):
        assert all(p[k].dtype == np.float64 and p[k].tobytes() == q[k].tobytes() for k in R.KLINE_KEYS)
    fed, _ = batch_call(eng, rows, maps, M, pseudo_lines=a["pseudo_lines"])
    same_bits(host(fed), host(a))


def test_refusals_launch_nothing(eng, g):
    from linetr_amd import _native as nat
    M = 16
    rows = [g["pad_stray_lines"], g["exact_lines"]]
    maps = maps_of([820, 821])
    recs, cu_k, cu_n = prefilter(eng, rows)
    shapes = eng.fixed_size_shapes(2, M, R.T)
    out = {k: torch.full(sh, MARKER, device="cuda") for k, sh in shapes.items()}
    kw = dict(max_sublines=M, token_distance=R.TD, max_tokens=R.T, out=out)
    good = eng.fixed_size_batch(recs, cu_k, cu_n, *maps, **{**kw, "out": None}, seed=3)["pseudo_lines"]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == MARKER).all()) for t in out.values())
    out8 = {k: torch.full(sh, MARKER, device="cuda") for k, sh in eng.fixed_size_shapes(2, 8, R.T).items()}
    with pytest.raises(nat.NativeError, match="more than max_sublines"):      # num_klns > M
        eng.fixed_size_batch(recs, cu_k, cu_n, *maps, **{**kw, "max_sublines": 8, "out": out8})
    torch.cuda.synchronize()
    assert all(bool((t == MARKER).all()) for t in out8.values())
    with pytest.raises(nat.NativeError, match="exactly one"):                # a pseudo line of two sub-lines
        eng.fixed_size_batch(recs, cu_k, cu_n, *maps, **{**kw, "token_distance": 4}, pseudo_lines=[
            {"klines": np.array([[[20.0, 20.0], [120.0, 20.0]]] * int(M - (cu_n[1] - cu_n[0]))), "length_klines": np.full(int(M - (cu_n[1] - cu_n[0])), 100.0),
             "angles": np.zeros((int(M - (cu_n[1] - cu_n[0])), 2))}, None])
    assert untouched()
    short = {k: v[:-1] for k, v in good[0].items()}
    with pytest.raises(nat.NativeError, match="pseudo lines, got"):          # a wrong pseudo count
        eng.fixed_size_batch(recs, cu_k, cu_n, *maps, **kw, pseudo_lines=[short, None])
    assert untouched()
    with pytest.raises(nat.NativeError, match="pseudo lines, got"):          # pseudo lines where none is needed
        eng.fixed_size_batch(recs, cu_k, cu_n, *maps, **kw, pseudo_lines=[good[0], good[0]])
    assert untouched()
    # a misaligned desc and a workspace that is too small: the C entry point itself
    L = eng._L
    cu_k32, cu_n32 = np.ascontiguousarray(cu_k, np.int32), np.ascontiguousarray(cu_n, np.int32)
    cu_p = np.array([0, len(good[0]["klines"]), len(good[0]["klines"])], np.int32)
    precs = np.zeros(int(cu_p[-1]), dtype=nat.REC_DTYPE)
    n_out = nat.C.c_int32()
    nat.check(L.linetr_pack_lines(*(nat.np_ptr(np.ascontiguousarray(good[0][k])) for k in R.KLINE_KEYS), int(cu_p[1]), float(R.TD), R.T, 0, 0, 0,
                                  nat.np_ptr(precs), nat.C.byref(n_out)), L)
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).cuda()
    d_precs = torch.from_numpy(precs.view(np.uint8).reshape(-1)).cuda()
    need = int(L.linetr_fixed_size_workspace_bytes(2, *HW, 0))
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    odd = torch.full((out["desc_sublines"].numel() + 4,), MARKER, device="cuda")

    def call(desc_ptr, ws_ptr, ws_bytes):
        ct = nat.Tokens()
        for field, key in zip(eng._FIXED_SIZE_FIELDS, shapes):
            setattr(ct, field, out[key].data_ptr())
        ct.desc = desc_ptr
        return L.linetr_fixed_size(None, d_recs.data_ptr(), nat.np_ptr(cu_k32), nat.np_ptr(cu_n32), d_precs.data_ptr(), nat.np_ptr(precs),
                                   nat.np_ptr(cu_p), 2, M, R.T, float(R.TD), maps[0].data_ptr(), maps[1].data_ptr(), *HW, 0, 0, 640, 480, 0, 0, ct,
                                   counts[0].data_ptr(), counts[1].data_ptr(), ws_ptr, ws_bytes, None)
    assert call(odd.data_ptr() + 4, ws.data_ptr(), ws.numel()) == nat.E_ARG and b"16-byte" in L.linetr_last_error()
    assert call(out["desc_sublines"].data_ptr(), ws.data_ptr() + 4, ws.numel() - 4) == nat.E_ARG
    assert call(out["desc_sublines"].data_ptr(), ws.data_ptr(), need - 1) == nat.E_WORKSPACE
    assert untouched() and bool((odd == MARKER).all()) and bool((counts == -7).all())
    assert call(out["desc_sublines"].data_ptr(), ws.data_ptr(), need) == 0       # and the same call, unbroken, is served
    torch.cuda.synchronize()
    assert not any(bool((t == MARKER).any()) for t in out.values()) and counts.tolist() == [np.diff(cu_k).tolist(), np.diff(cu_n).tolist()]


def test_conv_fixed_size_on_one_image_equals_the_batch_row(eng, g):
    from linetr_amd import util_lines as U
    from linetr_amd import line_process as lp
    conf = {"data": {"resize": R.RESIZE}, "feature": {"linetr": {"token_distance": R.TD, "max_tokens": R.T, "max_sublines": 16, "min_length": 16}}}
    names = ("pad_stray", "cut_unsplit")
    rows = [g[f"{n}_lines"] for n in names]
    maps = maps_of([830, 831])
    out, _ = batch_call(eng, rows, maps, 16, seed=21)
    for b in range(2):
        pred = {"dense_descriptor": maps[0][b:b + 1], "dense_score": maps[1][b:b + 1]}
        obj = lp.preprocess(synth.array_to_keylines(rows[b]), HW, pred, mask=None,
                            conf={"min_length": 16, "max_sublines": -1, "token_distance": R.TD, "max_tokens": R.T, "remove_borders": 8})
        one = U.conv_fixed_size(obj, conf, func_token=None, pred_sp=pred, pseudo_lines=out["pseudo_lines"][b])
        same_bits(host(out, b), {k: one[k].cpu().numpy() for k in R.ALL_KEYS + ("num_klns", "num_slns")})
    with pytest.raises(NotImplementedError):
        U.conv_fixed_size({"keypoints": None}, conf)


def test_one_training_iteration_from_detector_lines_to_updated_weights(eng):
    """prefilter -> fixed_size_batch of both views -> line_ground_truth -> TrainableLineTransformer + descriptor_loss -> backward -> Adam,
    against the same iteration fed by the per-image path"""
    import linetr_amd.evaluations as E
    from linetr_amd.optim import Adam
    from linetr_amd.train_ops import TrainableLineTransformer
    B, M = 2, 16
    pairs = [synth.homography_pair(900 + b, 14, *HW, 17.0, 200.0, strength=0.3) for b in range(B)]
    views = [[p[0] for p in pairs], [p[1] for p in pairs]]
    H = np.stack([p[2] for p in pairs])
    maps = [maps_of([910, 911]), maps_of([912, 913])]
    native = [batch_call(eng, views[v], maps[v], M, seed=40 + v)[0] for v in range(2)]
    slow = []
    for v in range(2):
        per = [per_image(eng, views[v][b], maps[v], b, M, native[v]["pseudo_lines"][b]) for b in range(B)]
        slow.append({k: torch.from_numpy(np.concatenate([p[k] for p in per])).cuda() for k in R.ALL_KEYS})
    sd = KR.loss_case()[0]
    crit = E.descriptor_loss()

    def iteration(d0, d1):
        mod = TrainableLineTransformer({})
        mod.load_state_dict(KR.tensors(sd), strict=True)
        mod = mod.cuda().train()
        params = list(mod.parameters())
        opt = Adam(params, lr=1e-3)
        gt = eng.line_ground_truth(d0["sublines"], d1["sublines"], H)
        with torch.enable_grad():
            loss = crit({"line_desc0": mod(d0)["line_desc"], "line_desc1": mod(d1)["line_desc"]}, {"mat_assign_sublines": gt["assign"]})[0]
            loss.backward()
        grads = [p.grad.clone() if p.grad is not None else None for p in params]
        before = [p.detach().clone() for p in params]
        opt.step()
        moved = sum(not torch.equal(p.detach(), q) for p, q in zip(params, before))
        return float(loss.detach()), grads, moved, int(gt["found"].sum())
    loss, grads, moved, found = iteration(*native)
    print(f"end to end: loss {loss:.6f}, {found} ground-truth pairs, {moved} tensors moved by the step")
    assert np.isfinite(loss) and found > 0
    assert len(grads) == 153 and all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads)
    assert moved > 0
    loss2, grads2, _, found2 = iteration(*slow)
    assert loss2 == loss and found2 == found
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
