"""GPU: linetr_describe_ragged -- tokeniser, layout pass, descriptor sampler and CLS pooling for a batch of differently sized images
in one native call -- against linetr_describe (equal sizes: bit for bit; image by image: tokens bit for bit, descriptors to the
batch-composition bar), the oracle and the reference's mixed-size golden.  Cases, bars and the guard helpers: tests/ragged_cases.py.
Every map lies between NaN guards and every output between guards of one bit pattern, inside one allocation each: a read or a write
beyond an image's own extent shows up as a wrong value."""
import numpy as np
import pytest
import torch

import ragged_cases as rc
from helpers import TOK_KEYS, load, oracle_image
from linetr_amd import _native as nat
from workloads import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine(synth.calibrated_state_dict(), DEV)


def same(a, b):
    return torch.equal(a, b) if a.dtype == torch.int32 else torch.equal(a.view(torch.int32), b.view(torch.int32))


def compare(out, ref, rows, n_rows, k_rows, fields=rc.TOK_FIELDS):
    """the outputs of a ragged call (rows n_rows / k_rows of them) against one TokenBatch: differing elements per tokeniser tensor"""
    bad = {}
    for f in fields:
        have = out.views[f][k_rows if f in ("klines", "length", "angles") else n_rows]
        want = getattr(ref, f)
        assert have.shape == want.shape, (f, have.shape, want.shape)
        n = int((have.view(torch.int32) != want.view(torch.int32)).sum()) if have.numel() else 0
        if n:
            bad[f] = n
    return bad


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("nhwc", [False, True])
def test_equal_sizes_equal_linetr_describe_bit_for_bit(eng, nhwc, align):
    """three 64 x 96 images: every output of the ragged call, line_desc included, is linetr_describe's"""
    H, W, Tm = 64, 96, 21
    lines = [synth.synth_lines(9300 + i, 8, H, W, len_hi=40.0) for i in range(3)]
    maps = [synth.synth_dense_maps_np(9300 + i, H, W) for i in range(3)]
    dd = np.concatenate([m[0] for m in maps])
    recs, cu_k, cu_n = eng.prefilter(lines, H, W, remove_borders=8, min_length=16, max_keylines=-1, token_distance=8, max_tokens=Tm,
                                     tie_order="stable")
    recs = recs.copy()
    tb, ld = eng.describe(recs, cu_k, cu_n, torch.from_numpy(dd.transpose(0, 2, 3, 1).copy() if nhwc else dd).to(DEV),
                          torch.from_numpy(np.concatenate([m[1] for m in maps])).to(DEV), token_distance=8, max_tokens=Tm,
                          align_corners=bool(align), want_tokens=True, dense_layout="nhwc" if nhwc else "nchw", want_mat=True)
    sep = []
    for m in maps:
        d = m[0][0].transpose(1, 2, 0) if nhwc else m[0][0]
        kd, dv = rc.guarded(d, DEV)
        ks, sv = rc.guarded(m[1][0], DEV)
        sep.append((dv, sv, (kd, ks)))
    code, out, _ = rc.describe_ragged(eng, recs, cu_k, cu_n, rc.image_table(sep, [8.0] * 3), nhwc, align, True, Tm=Tm)
    nat.check(code, eng._L)
    assert out.guards_intact()
    assert compare(out, tb, None, slice(None), slice(None)) == {}
    assert same(out.views["mat"], tb.mat.reshape(-1))
    assert same(out.views["ld"], ld) and bool(torch.isfinite(ld).all())


def reference_per_image(eng, ids, nhwc, align, max_keylines, n_lines=None):
    """linetr_describe once per image (the parent's only route), on the same guarded maps: [(TokenBatch, line_desc)], the maps"""
    maps = [rc.image_maps(i, nhwc, DEV) for i in ids]
    refs = []
    for j, i in enumerate(ids):
        h, w, td, ml = rc.IMAGES[i][:4]
        vm = rc.valid_mask(i)
        recs, cu_k, cu_n = eng.prefilter([rc.image_lines(i, (n_lines or {}).get(i))], h, w, remove_borders=rc.BORDER, min_length=ml, max_keylines=max_keylines,
                                         token_distance=td, max_tokens=rc.T, valid_masks=[vm] if vm is not None else None, tie_order="stable")
        refs.append(eng.describe(recs.copy(), cu_k, cu_n, maps[j][0][None], maps[j][1][None], token_distance=td, max_tokens=rc.T,
                                 align_corners=bool(align), want_tokens=True, dense_layout="nhwc" if nhwc else "nchw", want_mat=True))
    return refs, maps


def ragged_vs_per_image(eng, ids, nhwc, align, max_keylines=-1, n_lines=None):
    refs, maps = reference_per_image(eng, ids, nhwc, align, max_keylines, n_lines)
    lines, off, table, masks = rc.batch(ids, n_lines)
    code, recs, cu_k, cu_n = rc.prefilter_ragged(eng._L, lines, off, table, max_keylines, 1)
    nat.check(code, eng._L)
    want_mat = len(ids) <= 8
    code, out, _ = rc.describe_ragged(eng, recs, cu_k, cu_n, rc.image_table(maps, [rc.IMAGES[i][2] for i in ids]), nhwc, align, want_mat)
    nat.check(code, eng._L)
    assert out.guards_intact()
    worst, mat_off = 0.0, 0
    for j, (tb, ld) in enumerate(refs):
        n_rows, k_rows = slice(int(cu_n[j]), int(cu_n[j + 1])), slice(int(cu_k[j]), int(cu_k[j + 1]))
        assert tb.N == n_rows.stop - n_rows.start and tb.K == k_rows.stop - k_rows.start, j
        bad = compare(out, tb, None, n_rows, k_rows)
        print(f"image {ids[j]} ({rc.IMAGES[ids[j]][0]} x {rc.IMAGES[ids[j]][1]}): K {tb.K} N {tb.N} differing token elements {bad or 0}", end="")
        assert bad == {}, (ids[j], bad)
        if want_mat and tb.K:
            assert same(out.views["mat"][mat_off:mat_off + tb.K * tb.N], tb.mat.reshape(-1)), j
            mat_off += tb.K * tb.N
        if tb.N:
            err = float((out.views["ld"][n_rows] - ld).abs().max())
            print(f", max |line_desc - per image| {err:.2e} / {rc.DESC_BATCH_BAR:.0e}")
            worst = max(worst, err)
        else:
            print()
    assert bool(torch.isfinite(out.views["ld"]).all())
    assert worst <= rc.DESC_BATCH_BAR, worst
    return out, recs, cu_k, cu_n


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("ids", [(3,), (1, 5), tuple(range(9))], ids=["B1", "B2", "B9"])
def test_ragged_equals_linetr_describe_image_by_image(eng, ids, nhwc):
    """B = 1 (odd Hc * Wc), B = 2 (three sub-lines in the smallest image + the other odd size), B = 9 (all sizes, an empty image in the
    middle, the image max_keylines = -1 empties): tokens bit for bit, mat_klines2sublines up to 8 images, line_desc within 5e-6"""
    out, recs, cu_k, cu_n = ragged_vs_per_image(eng, ids, nhwc, align=0)
    if len(ids) == 9:
        k = np.diff(cu_k)
        assert k[4] == 0 and k[6] == 0 and recs[cu_k[1]:cu_k[2]]["n_sub"].max() == 3


def test_many_sub_lines_take_the_one_wave_per_sub_line_kernel(eng):
    """above 2048 sub-lines the pooling runs one wave per sub-line, last sub-lines first (cls_pool_plan): three sizes, 600 lines in each
    of the two larger images"""
    out, recs, cu_k, cu_n = ragged_vs_per_image(eng, (2, 3, 5), nhwc=True, align=1, max_keylines=10000, n_lines=rc.MANY_LINES)
    assert cu_n[-1] > 2048, cu_n


@pytest.mark.parametrize("nhwc", [False, True])
def test_against_the_oracle_through_the_engine(eng, nhwc):
    """the nine-image batch through Engine.describe_lines_ragged (angles='native', ties ordered by NumPy) against the oracle image by image"""
    ids = list(range(9))
    lines, off, table, masks = rc.batch(ids)
    maps = [synth.synth_dense_maps_np(rc.IMAGES[i][4], *rc.IMAGES[i][:2]) for i in ids]
    dds = [torch.from_numpy(m[0][0].transpose(1, 2, 0).copy() if nhwc else m[0][0]).to(DEV) for m in maps]
    dss = [torch.from_numpy(m[1][0]).to(DEV) for m in maps]
    tb, ld = eng.describe_lines_ragged(np.concatenate(lines), off, dds, dss, remove_borders=rc.BORDER, min_length=[im[3] for im in rc.IMAGES],
                                       max_keylines=-1, token_distance=[im[2] for im in rc.IMAGES], max_tokens=rc.T, align_corners=False,
                                       want_tokens=True, dense_layout="nhwc" if nhwc else "nchw", angles="native", valid_masks=masks)
    sd_t = synth.to_torch_state_dict(synth.calibrated_state_dict())
    names = {"klines": "klines", "length_klines": "length", "angles": "angles", "sublines": "sublines", "pnt_sublines": "pnt",
             "mask_sublines": "mask", "resp_sublines": "resp", "angle_sublines": "angle_sub", "score_sublines": "score", "desc_sublines": "desc"}
    for j, i in enumerate(ids):
        h, w, td, ml = rc.IMAGES[i][:4]
        cfg = dict(min_length=ml, token_distance=td, max_tokens=rc.T, remove_borders=rc.BORDER, max_keylines=-1)
        if len(lines[j]) == 0:      # (no detector rows at all: the reference itself raises on them)
            assert tb.cu_k[j + 1] == tb.cu_k[j]
            continue
        o = oracle_image(sd_t, lines[j], torch.from_numpy(maps[j][0]), torch.from_numpy(maps[j][1]), (h, w), cfg, masks[j], False, (480, 640))
        n_rows, k_rows = slice(int(tb.cu_n[j]), int(tb.cu_n[j + 1])), slice(int(tb.cu_k[j]), int(tb.cu_k[j + 1]))
        if tb.cu_k[j + 1] == tb.cu_k[j]:
            assert len(o["klines"]) == 0, i
            continue
        for key, f in names.items():
            have = getattr(tb, f)[k_rows if f in ("klines", "length", "angles") else n_rows].cpu().numpy()
            want = o[key][0].numpy().reshape(have.shape)
            if f == "desc":       # sampled token descriptors: the oracle's grid_sample on the CPU, bit for bit on these maps
                assert np.abs(have - want).max() <= rc.SAMPLED_DESC_ORACLE_BAR, (i, key)
            else:
                assert np.abs(have - want).max() <= (rc.ANGLE_ORACLE_BAR if "angle" in key else 0), (i, key)
        err = np.abs(ld[n_rows].cpu().numpy().T - o["line_desc"][0].numpy()).max()
        print(f"image {i}: max |line_desc - oracle| {err:.2e} / {rc.DESC_ORACLE_BAR:.0e}")
        assert err <= rc.DESC_ORACLE_BAR, (i, err)


def matching(g, swap=False, n=1):
    from models.matching import Matching
    seeds, sets = [int(g["map_seed0"]), int(g["map_seed1"])], [g["lines0"], g["lines1"]]
    order = [(seeds, sets), (seeds[::-1], sets[::-1])][:n] if not swap else [(seeds[::-1], sets[::-1])]
    mt = Matching({"auto_min_length": True, "linetransformer": {"mode": "train", "max_keylines": -1, "min_length": 16, "token_distance": 8,
                                                                "nn_threshold": 0.8}},
                  superpoint=rc.FakeSuperPoint([s for sd, _ in order for s in sd]), lsd=rc.FakeLSD([l for _, ls in order for l in ls]))
    mt.linetransformer.load_state_dict(synth.to_torch_state_dict(synth.calibrated_state_dict()))
    return mt.eval().to("cuda")


def check_against_golden(pred, g, swapped):
    for s in "01":
        gs = "10"[int(s)] if swapped else s
        for k in TOK_KEYS:
            if k + s not in pred:       # forward_batch does not materialise the dense per-token tensors
                continue
            want, have = g[k + gs], pred[k + s].cpu().numpy()
            assert have.shape == want.shape, (k, s)
            assert np.array_equal(have, want), (k, s)       # angles too: both surfaces take NumPy's, like the reference
        assert np.abs(pred["line_desc" + s].cpu().numpy() - g["line_desc" + gs]).max() <= rc.DESC_ORACLE_BAR
    tr = (lambda a: a.transpose(0, 2, 1)) if swapped else (lambda a: a)
    assert np.array_equal(pred["matches_l"].numpy(), tr(g["matches_l"])) and g["matches_l"].sum() > 0
    assert np.abs(pred["matching_scores_l"].numpy() - tr(g["matching_scores_l"])).max() <= 1e-4


def test_forward_batch_of_mixed_sizes_against_the_real_reference():
    """Matching.forward_batch on the reference's 480 x 640 + 960 x 1280 golden as pair 0 and the same pair with its sides swapped as
    pair 1: one ragged native call for the four images, every image with the thresholds of its own shape"""
    g = load("mixed_size_pair")
    mt = matching(g, n=2)
    imgs = {s: torch.zeros(1, 1, *(int(v) for v in g["hw" + s]), device="cuda") for s in "01"}
    preds = mt.forward_batch([{"image0": imgs["0"], "image1": imgs["1"]}, {"image0": imgs["1"], "image1": imgs["0"]}])
    check_against_golden(preds[0], g, False)
    check_against_golden(preds[1], g, True)
    # the config is left on the LAST image's values: pair 1's image1 is the 480 x 640 one
    assert mt.linetransformer.config["min_length"] == 16 and mt.linetransformer.config["token_distance"] == 8
    assert tuple(mt.linetransformer.config["image_shape"]) == tuple(imgs["0"].shape)


def test_forward_of_a_mixed_size_pair_takes_the_fused_path(monkeypatch):
    """Matching.forward on the golden: ONE fused call (Matching._describe_fused returns the dicts, nothing falls back to the per-image
    path), results the reference's, config left on image1's values"""
    from linetr_amd.engine import Engine
    from models.matching import Matching
    g = load("mixed_size_pair")
    fused, ragged, staged = [], [], []
    orig, orig_r, orig_t = Matching._describe_fused, Engine.describe_ragged, Engine.tokenize
    monkeypatch.setattr(Matching, "_describe_fused", lambda self, *a: fused.append(orig(self, *a)) or fused[-1])
    monkeypatch.setattr(Engine, "describe_ragged", lambda self, *a, **kw: ragged.append(1) or orig_r(self, *a, **kw))
    monkeypatch.setattr(Engine, "tokenize", lambda self, *a, **kw: staged.append(1) or orig_t(self, *a, **kw))
    mt = matching(g)
    imgs = {s: torch.zeros(1, 1, *(int(v) for v in g["hw" + s]), device="cuda") for s in "01"}
    pred = mt({"image0": imgs["0"], "image1": imgs["1"]})
    assert len(fused) == 1 and fused[0] is not None and ragged == [1] and staged == []
    check_against_golden(pred, g, False)
    assert mt.linetransformer.config["min_length"] == float(g["final_min_length"])
    assert mt.linetransformer.config["token_distance"] == float(g["final_token_distance"])


def test_refusals_leave_everything_untouched(eng):
    ids = (1, 5)
    lines, off, table, masks = rc.batch(ids)
    code, recs, cu_k, cu_n = rc.prefilter_ragged(eng._L, lines, off, table, -1, 1)
    nat.check(code, eng._L)
    tds = [rc.IMAGES[i][2] for i in ids]
    for nhwc in (False, True):
        maps = [rc.image_maps(i, nhwc, DEV) for i in ids]
        good = rc.image_table(maps, tds)
        call = lambda t=good, **kw: rc.describe_ragged(eng, recs, cu_k, cu_n, t, nhwc, 0, kw.pop("want_mat", False), **kw)
        code, out, nbytes = call()
        assert code == 0 and not out.untouched() and nbytes > 0

        def edited(field, i, v):
            t = good.copy()
            t[field][i] = v
            return t
        cases = [edited("height", 0, 60), edited("width", 1, 0), edited("height", 1, -8), edited("d_dense_desc", 0, 0),
                 edited("d_dense_score", 1, 0), edited("token_distance", 1, 0.0), edited("token_distance", 0, float("nan"))]
        if nhwc:
            cases.append(edited("d_dense_desc", 1, int(good["d_dense_desc"][1]) + 4))       # a channel-last map off the 16-byte grid
        for t in cases:
            code, out, _ = call(t)
            assert code == nat.E_ARG and out.untouched(), t
        for kw in (dict(t=None), dict(n_images=0)):                                        # a NULL table, an empty one
            code, out, nb = call(**kw)
            assert code == nat.E_ARG and nb == -1 and out.untouched(), kw
        code, out, _ = call(ws_offset=4, ws_short=4)                                       # the workspace off the 16-byte grid
        assert code == nat.E_ARG and out.untouched()
        code, out, _ = call(ws_short=1)
        assert code == nat.E_WORKSPACE and out.untouched()
        bad = recs.copy()
        bad["image"][int(cu_k[1])] = 2                                                     # a record outside the table of two
        code, out, _ = rc.describe_ragged(eng, bad, cu_k, cu_n, good, nhwc, 0, False)
        assert code == nat.E_ARG and out.untouched()
    # mat_klines2sublines beyond eight images: refused cleanly
    ids = tuple(range(9))
    lines, off, table, masks = rc.batch(ids)
    code, recs, cu_k, cu_n = rc.prefilter_ragged(eng._L, lines, off, table, -1, 1)
    maps = [rc.image_maps(i, True, DEV) for i in ids]
    code, out, _ = rc.describe_ragged(eng, recs, cu_k, cu_n, rc.image_table(maps, [im[2] for im in rc.IMAGES]), True, 0, True)
    assert code == nat.E_ARG and out.untouched()
    # and the Python surface says what is wrong with a map
    with pytest.raises(ValueError):
        eng.describe_ragged(recs, cu_k, cu_n, [m[0] for m in maps], [m[1] for m in maps][::-1], token_distance=8, max_tokens=rc.T,
                            dense_layout="nhwc")


def test_two_calls_give_the_same_bytes(eng):
    ids = (0, 3, 5, 1)
    lines, off, table, masks = rc.batch(ids)
    code, recs, cu_k, cu_n = rc.prefilter_ragged(eng._L, lines, off, table, -1, 1)
    nat.check(code, eng._L)
    maps = [rc.image_maps(i, False, DEV) for i in ids]
    t = rc.image_table(maps, [rc.IMAGES[i][2] for i in ids])
    outs = []
    for _ in range(2):
        code, out, _ = rc.describe_ragged(eng, recs, cu_k, cu_n, t, False, 0, True)
        nat.check(code, eng._L)
        outs.append(out)
    assert torch.equal(outs[0].whole, outs[1].whole)
