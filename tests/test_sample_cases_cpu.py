"""CPU: the premises of tests/sample_cases.py -- the generator keeps its distance from the sampler's discontinuities, the exact
families are exact in both references, zero vectors do occur -- and that each bar catches a planted mistake in a CPU restatement of
the kernels (one tap from the neighbouring cell, zero padding replaced by clamping, image 0's map for every image, a block of 64 key
points written one column off), while the restatement itself passes.  Also: the argument checks refuse a pointer that is not 16-byte
aligned before anything is launched (they are host-side integer tests: no device is needed to be refused)."""
import torch

import sample_cases as S
from linetr_amd import _native as nat

torch.set_grad_enabled(False)


# ---- samplers ---------------------------------------------------------------------------------------------------------------------

def all_point_cases():
    return list(S.sampler_cases()) + list(S.keypoint_cases())


def test_points_keep_their_distance_from_the_discontinuities():
    worst = float("inf")
    for case in all_point_cases():
        m = float(S.margin(case["points"], case["Hc"], case["Wc"], case["align_corners"]).min())
        assert m >= S.MARGIN, (S.label(case), case["family"], m)
        worst = min(worst, m)
    print("smallest distance to a discontinuity:", worst, "cells")


def test_border_family_reaches_every_tap_pattern_and_the_zero_vector():
    for hw in S.MAPS:
        for ac in (False, True):
            case = S.sampler_case("border", hw, ac)
            assert case["points"].shape[0] == 169
            p = case["points"].double()
            cx, cy = S.grid_coord(p[:, 0], hw[1], ac), S.grid_coord(p[:, 1], hw[0], ac)
            inside = lambda c, n: ((torch.floor(c) >= 0) & (torch.floor(c) < n)).long() + ((torch.floor(c) + 1 >= 0) & (torch.floor(c) + 1 < n)).long()
            taps = inside(cx, hw[1]) * inside(cy, hw[0])                      # taps inside the map: 0, 1, 2 or 4
            assert torch.equal(case["zero"], taps == 0), (hw, ac)
            degenerate = ac and hw in ((1, 1), (1, 2), (2, 1))                 # align_corners pins an axis of one cell to coordinate 0
            assert bool(case["zero"].any()) != degenerate, (hw, ac)
            assert bool((taps == 4).any()) == (min(hw) > 1) and bool(((taps == 1) | (taps == 2)).any())
            # the references agree on which vectors are zero, and the others are unit vectors
            assert torch.equal((case["ref32"] == 0).all(dim=1), case["zero"])
            assert float((case["ref64"][~case["zero"]].norm(dim=1) - 1).abs().max()) < 1e-12


def test_sampler_references_are_close_and_the_restatement_passes():
    own = []
    for case in all_point_cases():
        own.append(float((case["ref32"].double() - case["ref64"]).abs().max()))
        assert own[-1] < 2e-6, (S.label(case), case["family"], own[-1])
        rows = S.sample_errors(S.restate(case), case)
        assert not S.failures(rows), S.failures(rows)
    print("max |ref32 - ref64| over the cases: from", min(own), "to", max(own))


def test_planted_maps_name_the_cell():
    case = S.sampler_case("planted", (7, 9), False)
    assert torch.equal(case["dense"][0].sum(dim=0), torch.ones(7, 9))
    assert int(case["dense"][0, (3 * 9 + 4) % 256, 3, 4]) == 1
    bad = S.restate(case, "neighbour")
    assert S.failures(S.sample_errors(bad, case)) and S.explain_planted(bad, case)


def test_bar_catches_a_tap_from_the_neighbouring_cell():
    for family in ("normal", "planted"):
        for hw in ((3, 5), (7, 9), (8, 8)):
            for ac in (False, True):
                case = S.sampler_case(family, hw, ac)
                assert S.failures(S.sample_errors(S.restate(case, "neighbour"), case)), (family, hw, ac)


def test_bar_catches_clamping_instead_of_zero_padding():
    for hw in S.MAPS:
        for ac in (False, True):
            if ac and hw in ((1, 1), (1, 2), (2, 1)):
                continue        # there every sample is one cell's vector up to its weight: clamping gives the same normalised vector
            case = S.sampler_case("border", hw, ac)
            bad = S.failures(S.sample_errors(S.restate(case, "clamp"), case))
            assert bad, (hw, ac)
            if hw[0] * hw[1] > 2:
                assert any("/zero" not in b for b in bad), (hw, ac)             # not only the zero vectors: partial taps too


def test_bar_catches_image_zero_for_every_image():
    for case in S.keypoint_cases():
        if sum(1 for c in case["counts"] if c) < 2 or case["counts"][0] == int(case["cu"][-1]):
            continue
        rows = S.kp_block_errors(S.kp_blocks(S.restate(case, "image0"), case["cu"]), case)
        bad = S.failures(rows)
        assert bad and all("image 0" not in b for b in bad), case["counts"]


def test_bar_catches_a_block_written_one_column_off():
    seen = 0
    for case in S.keypoint_cases():
        good = S.restate(case)
        assert not S.failures(S.kp_block_errors(S.kp_blocks(good, case["cu"]), case))
        for b, n in enumerate(case["counts"]):
            for chunk in range(-(-n // 64)):
                if n - 64 * chunk < 2:
                    continue                                                   # a chunk of one point in the last column: nothing lands
                bad = S.failures(S.kp_block_errors(S.kp_blocks(good, case["cu"], shifted=(b, chunk)), case))
                assert bad and all(f"image {b}" in x for x in bad), (case["counts"], b, chunk)
                seen += 1
    assert seen > 20


def test_keypoint_batches_cover_the_counts():
    counts = [c for batch in S.KP_BATCHES for c in batch]
    assert set(counts) == set(S.KP_COUNTS)
    assert {len(b) for b in S.KP_BATCHES} == {1, 3, 4}
    multi = [b for b in S.KP_BATCHES if len(b) > 1]
    assert any(b[0] == 0 for b in multi) and any(b[-1] == 0 for b in multi) and any(0 in b[1:-1] for b in multi)
    maps = S.dense_maps(3, (7, 9))
    assert not torch.equal(maps[0], maps[1]) and not torch.equal(maps[1], maps[2])


# ---- heads ------------------------------------------------------------------------------------------------------------------------

def test_head_shapes_cover_the_ragged_vector_blocks():
    hw = [h * w for h, w in S.HEAD_MAPS]
    assert hw == [1, 31, 32, 33, 36, 63, 64, 65, 68, 100]
    assert any(v % 4 == 0 and v % 32 for v in hw) and any(v % 4 == 0 and v % 64 for v in hw) and any(v % 4 for v in hw)


def test_onehot_premises():
    for family, hw, B in ((f, hw, B) for f in S.EXACT for hw in S.HEAD_MAPS for B in S.HEAD_B):
        case = S.head_case(family, hw, B)
        HW = hw[0] * hw[1]
        for d in (case["desc64"], case["desc32"]):
            flat = d.permute(0, 2, 3, 1).reshape(B * HW, 256)
            p = torch.arange(B * HW)
            assert bool((flat[p, (7 * p + 3) % 256].abs() == 1).all()) and int((flat != 0).sum()) == B * HW
            assert torch.equal(flat[p, (7 * p + 3) % 256].double(), torch.where((p // 17) % 2 == 0, 1.0, -1.0).double())
        assert torch.equal(case["desc32"].double(), case["desc64"])
        for s in (case["score64"], case["score32"]):
            patches = s.reshape(B, hw[0], 8, hw[1], 8).permute(0, 1, 3, 2, 4).reshape(B * HW, 64)
            for p in range(B * HW):
                c = int(S.hot_channel(family, p))
                hot = torch.zeros(64, dtype=torch.bool)
                if c < 64:
                    dy, dx = divmod(c, 8)
                    hot[8 * dy + dx] = True
                    assert patches[p, c].item() == 1.0
                assert bool((patches[p][~hot] < 1e-30).all()) and bool((patches[p] >= 0).all())
        assert torch.equal(case["score64"] == 1.0, case["score32"] == 1.0)
        # ref32 and ref64 agree inside the floor of the bar (a map whose only cell has the dustbin hot holds nothing above 1e-30)
        assert float((case["score32"].double() - case["score64"]).abs().max()) <= max(2.0 ** -23 * float(case["score64"].abs().max()), 1e-30)
    assert {int(S.hot_channel("onehot65", p)) for p in range(100)} == set(range(65)), "every channel, the dustbin too, must be hot somewhere"


def test_head_bars_catch_a_wrong_cell_and_a_wrong_channel():
    for hw in ((4, 8), (6, 6), (5, 13)):
        case = S.head_case("normal", hw, 3)
        good = {"score": case["score32"], "nchw": case["desc32"], "nhwc": case["desc32"].permute(0, 2, 3, 1)}
        assert not S.failures(S.head_errors(good, case))
        for name, t in good.items():
            bad = dict(good)
            bad[name] = torch.roll(t, 1, dims=-1)                              # one pixel / cell / channel off
            assert S.failures(S.head_errors(bad, case)), (hw, name)
        bad = dict(good, score=torch.roll(case["score32"], 1, dims=0))         # another image's map
        assert S.failures(S.head_errors(bad, case)), hw


# ---- alignment refusals need no device --------------------------------------------------------------------------------------------

def test_entry_points_refuse_misaligned_pointers_before_any_launch():
    """Addresses that are never dereferenced: every call returns LINETR_E_ARG from its argument checks."""
    L = nat.lib()
    A, M = 0x10000, 0x10004                  # an aligned and a misaligned address
    msg = lambda: L.linetr_last_error().decode()
    heads = lambda **kw: L.linetr_superpoint_heads(None, kw.get("sl", A), kw.get("dr", A), 1, kw.get("Hc", 4), kw.get("Wc", 8), kw.get("s", A), kw.get("a", A), kw.get("b", A), None)
    for kw in (dict(sl=M), dict(dr=M), dict(s=M), dict(a=M), dict(b=M), dict(Hc=3, Wc=3, s=M), dict(Hc=3, Wc=3, a=M), dict(Hc=3, Wc=3, b=M)):
        assert heads(**kw) == nat.E_ARG and "16-byte" in msg(), kw
    rows = lambda **kw: L.linetr_superpoint_heads_rows(None, M, 65, M, 256, 1, 4, 8, kw.get("s", A), kw.get("a", A), kw.get("b", A), None)
    for kw in (dict(s=M), dict(a=M), dict(b=M)):
        assert rows(**kw) == nat.E_ARG and "16-byte" in msg(), kw
    samp = lambda **kw: L.linetr_sample_descriptors(None, M, 4, kw.get("dd", A), 4, 8, 0, kw.get("nhwc", 1), kw.get("out", A), kw.get("ws", A), 1 << 20, None)
    for kw in (dict(dd=M), dict(out=M), dict(ws=M), dict(nhwc=0, out=M), dict(nhwc=0, ws=M)):
        assert samp(**kw) == nat.E_ARG and "16-byte" in msg(), kw
    pd = lambda **kw: L.linetr_point_descriptors(None, M, A, 1, 4, kw.get("dd", A), 4, 8, 0, kw.get("nhwc", 1), M, kw.get("ws", A), 1 << 20, None)
    for kw in (dict(dd=M), dict(ws=M), dict(nhwc=0, ws=M)):
        assert pd(**kw) == nat.E_ARG and "16-byte" in msg(), kw

    def tok(dd=A, desc=A, ws=A, nhwc=1):
        t = nat.Tokens()
        for k in ("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "score"):
            setattr(t, k, M)
        t.desc = desc
        return L.linetr_tokenize(None, A, 1, 1, 8.0, 3, dd, A, 1, 64, 96, 0, 0, 0, nhwc, t, A, ws, 1 << 24, None)
    for kw in (dict(dd=M), dict(desc=M), dict(ws=M), dict(nhwc=0, desc=M), dict(nhwc=0, ws=M)):
        assert tok(**kw) == nat.E_ARG and "16-byte" in msg(), kw
