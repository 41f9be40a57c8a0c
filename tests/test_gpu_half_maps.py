"""GPU: float16 / bfloat16 dense descriptor maps and raw head outputs read IN PLACE (LINETR_DENSE_F16 / LINETR_DENSE_BF16,
linetr_superpoint_heads_typed) against the same calls on the exact float32 upcast.  Cases, sizes and the guard helpers:
tests/half_map_cases.py (and tests/ragged_cases.py, whose NaN and bit-pattern guards every input and output sits between).

Bars: 0 differing bits everywhere -- a half element widens exactly and the arithmetic behind the load is the float32 kernel's -- except
where noted: `line_desc` of the whole calls follows the pooling kernels (bit for bit here as well) and is also held to
ragged_cases.DESC_ORACLE_BAR against the oracle fed the upcast map."""
import ctypes as C

import numpy as np
import pytest
import torch

import half_map_cases as hc
import ragged_cases as rc
from helpers import oracle_image
from linetr_amd import _native as nat
from workloads import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
KINDS = pytest.mark.parametrize("kind", hc.KINDS)


@pytest.fixture(scope="module")
def eng():
    from linetr_amd.engine import Engine
    return Engine(synth.calibrated_state_dict(), DEV)


def stream(eng):
    return C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


# =====================================================================================================================================
# 1. head producer
# =====================================================================================================================================

@pytest.fixture(scope="module")
def head_inputs():
    """{(Hc, Wc): (logits32, raw32)} seeded once"""
    out = {}
    for Hc, Wc in hc.HEAD_MAPS:
        g = hc._gen("heads", Hc, Wc)
        out[Hc, Wc] = (torch.randn((hc.HEAD_B, 65, Hc, Wc), generator=g) * 3.0, torch.randn((hc.HEAD_B, 256, Hc, Wc), generator=g))
    return out


def run_heads(eng, logits, raw, in_bits, out_bits, want=("score", "nhwc", "nchw"), typed=True, out_offset=0):
    """linetr_superpoint_heads(_typed) as it is: (status, {name: hc.Out}); inputs between NaN guards, outputs between pattern guards"""
    B, _, Hc, Wc = raw.shape
    odt = {0: torch.float32, nat.DENSE_F16: torch.float16, nat.DENSE_BF16: torch.bfloat16}.get(out_bits, torch.float32)
    keep = [(hc.guarded16 if t.dtype != torch.float32 else hc.guarded32)(t, DEV) for t in (logits, raw)]
    outs = {"score": hc.Out((B, Hc * 8, Wc * 8), torch.float32, DEV), "nhwc": hc.Out((B, Hc, Wc, 256), odt, DEV, out_offset),
            "nchw": hc.Out((B, 256, Hc, Wc), odt, DEV, out_offset)}
    p = lambda name: outs[name].view.data_ptr() if name in want else None
    with torch.cuda.device(eng.device):
        if typed:
            code = eng._L.linetr_superpoint_heads_typed(eng._h, keep[0][1].data_ptr(), keep[1][1].data_ptr(), in_bits, B, Hc, Wc, p("score"),
                                                        p("nhwc"), p("nchw"), out_bits, stream(eng))
        else:
            code = eng._L.linetr_superpoint_heads(eng._h, keep[0][1].data_ptr(), keep[1][1].data_ptr(), B, Hc, Wc, p("score"), p("nhwc"),
                                                  p("nchw"), stream(eng))
        torch.cuda.synchronize()
    return code, outs


@KINDS
@pytest.mark.parametrize("hw", hc.HEAD_MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_heads_half_inputs_equal_the_float32_call_on_the_upcast(eng, head_inputs, hw, kind):
    dtype, bits = hc.HALF[kind]
    l16, r16 = (t.to(dtype) for t in head_inputs[hw])
    code, ref = run_heads(eng, l16.float(), r16.float(), 0, 0, typed=False)
    nat.check(code, eng._L)
    code, got = run_heads(eng, l16, r16, bits, 0)
    nat.check(code, eng._L)
    for name in ("score", "nhwc", "nchw"):
        assert got[name].guards_intact() and ref[name].guards_intact(), name
        assert bool(torch.isfinite(got[name].view).all()), name
        assert hc.bits_equal(got[name].view, ref[name].view), (hw, kind, name, float((got[name].view - ref[name].view).abs().max()))
    # half outputs = the float32 outputs rounded by torch; from half inputs and from float32 inputs
    for in_bits, (li, ri) in ((bits, (l16, r16)), (0, (l16.float(), r16.float()))):
        code, half = run_heads(eng, li, ri, in_bits, bits)
        nat.check(code, eng._L)
        for name in ("nhwc", "nchw"):
            assert half[name].guards_intact(), name
            assert half[name].view.dtype == dtype and hc.bits_equal(half[name].view, ref[name].view.to(dtype)), (hw, kind, name, in_bits)
        assert hc.bits_equal(half["score"].view, ref["score"].view)


@KINDS
@pytest.mark.parametrize("only", ["nhwc", "nchw"])
def test_heads_one_descriptor_output_alone(eng, head_inputs, kind, only):
    dtype, bits = hc.HALF[kind]
    l16, r16 = (t.to(dtype) for t in head_inputs[5, 13])
    code, ref = run_heads(eng, l16.float(), r16.float(), 0, 0, typed=False)
    nat.check(code, eng._L)
    code, got = run_heads(eng, l16, r16, bits, bits, want=(only,))
    nat.check(code, eng._L)
    other = "nchw" if only == "nhwc" else "nhwc"
    assert got[other].untouched() and got["score"].untouched()
    assert got[only].guards_intact() and hc.bits_equal(got[only].view, ref[only].view.to(dtype))


@KINDS
def test_heads_refusals(eng, head_inputs, kind):
    dtype, bits = hc.HALF[kind]
    l16, r16 = (t.to(dtype) for t in head_inputs[4, 8])
    # half outputs off the 8-byte grid
    for off in (2, 4, 6):
        code, got = run_heads(eng, l16, r16, bits, bits, out_offset=off)
        assert code == nat.E_ARG and "aligned" in eng._L.linetr_last_error().decode(), off
        assert all(o.untouched() for o in got.values())
    # an unknown type code, either side: refused with nothing written
    for in_bits, out_bits in ((0x300, 0), (0x400, 0), (1, 0), (bits, 0x300), (bits, 3), (0, 0x800)):
        code, got = run_heads(eng, l16, r16, in_bits, out_bits)
        assert code == nat.E_ARG and "type code" in eng._L.linetr_last_error().decode(), (in_bits, out_bits)
        assert all(o.untouched() for o in got.values())


# =====================================================================================================================================
# 2. layout pass and samplers
# =====================================================================================================================================

def run_sample(eng, dmap, fmt, pts, Hc, Wc, align, ws_bytes=None):
    """linetr_sample_descriptors on image 0 of `dmap` (a device view in the layout `fmt` says): (status, hc.Out [n, 256])"""
    L = eng._L
    n = pts.shape[0]
    out = hc.Out((n, 256), torch.float32, DEV)
    need = L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, fmt)
    ws = torch.empty(max(need, 0) + 256, dtype=torch.uint8, device=DEV)
    keep_p, d_pts = hc.guarded32(pts, DEV)
    with torch.cuda.device(eng.device):
        code = L.linetr_sample_descriptors(eng._h, d_pts.data_ptr(), n, dmap.data_ptr(), Hc, Wc, align, fmt, out.view.data_ptr(), ws.data_ptr(),
                                           max(need, 0) if ws_bytes is None else ws_bytes, stream(eng))
        torch.cuda.synchronize()
    return code, out


def run_points(eng, dmap, fmt, pts, counts, Hc, Wc, align):
    """linetr_point_descriptors for len(counts) images: (status, hc.Out [256 * n_total])"""
    L = eng._L
    B, n_total = len(counts), int(sum(counts))
    cu = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)
    out = hc.Out((256 * n_total,), torch.float32, DEV)
    need = L.linetr_point_descriptors_workspace_bytes(B, Hc, Wc, fmt)
    ws = torch.empty(max(need, 0) + 256, dtype=torch.uint8, device=DEV)
    keep_p, d_pts = hc.guarded32(pts[:n_total], DEV)
    with torch.cuda.device(eng.device):
        code = L.linetr_point_descriptors(eng._h, d_pts.data_ptr(), cu.data_ptr(), B, n_total, dmap.data_ptr(), Hc, Wc, align, fmt,
                                          out.view.data_ptr(), ws.data_ptr(), max(need, 0), stream(eng))
        torch.cuda.synchronize()
    return code, out


def layouts(m16, offset_odd):
    """[(label, half device view, its float32 upcast as a device view, nhwc flag)] of an NCHW half map [n, 256, Hc, Wc]"""
    out = []
    for nhwc in (0, 1):
        t = m16.permute(0, 2, 3, 1).contiguous() if nhwc else m16
        out.append(("nhwc" if nhwc else "nchw", hc.guarded16(t, DEV), hc.guarded32(t.float(), DEV), nhwc))
    if offset_odd:
        out.append(("nchw at a 2-byte-odd address", hc.guarded16(m16, DEV, offset=1), hc.guarded32(m16.float(), DEV), 0))
    return out


@KINDS
@pytest.mark.parametrize("hw", hc.SAMPLE_MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_samplers_on_a_half_map_equal_the_upcast(eng, hw, kind):
    Hc, Wc = hw
    dtype, bits = hc.HALF[kind]
    m16 = hc.map16(kind, 11, 2, Hc, Wc, special=True)
    pts = hc.sample_points(Hc, Wc)
    n = pts.shape[0]
    counts = (n // 2, n - n // 2)
    for label, (k16, v16), (k32, v32), nhwc in layouts(m16, offset_odd=True):
        if "odd" in label:
            assert v16.data_ptr() % 4 == 2
        for align in (0, 1):
            code, ref = run_sample(eng, v32, nhwc, pts, Hc, Wc, align)
            nat.check(code, eng._L)
            code, got = run_sample(eng, v16, nhwc | bits, pts, Hc, Wc, align)
            nat.check(code, eng._L)
            assert got.guards_intact() and bool(torch.isfinite(got.view).all()), (label, align)
            assert hc.bits_equal(got.view, ref.view), (label, align, float((got.view - ref.view).abs().max()))
            if align == 1:      # the planted cells, sampled at weight 1: subnormals are not flushed, the largest value arrives
                sub = hc.special_subnormals().to(DEV)
                assert float(got.view[0].abs().min()) > 0 and bool((got.view[0][1:] > got.view[0][:-1]).all())      # k / ||k||, k = 1 .. 256
                assert bool((got.view[1] == ref.view[1]).all()) and bool(torch.isfinite(got.view[1]).all())
            code, ref = run_points(eng, v32, nhwc, pts, counts, Hc, Wc, align)
            nat.check(code, eng._L)
            code, got = run_points(eng, v16, nhwc | bits, pts, counts, Hc, Wc, align)
            nat.check(code, eng._L)
            assert got.guards_intact() and hc.bits_equal(got.view, ref.view), (label, align)


@KINDS
def test_sampler_refusals(eng, kind):
    Hc, Wc = 3, 5
    dtype, bits = hc.HALF[kind]
    m16 = hc.map16(kind, 11, 2, Hc, Wc)
    pts = hc.sample_points(Hc, Wc)[:8]
    nhwc16 = m16.permute(0, 2, 3, 1).contiguous()
    msg = lambda: eng._L.linetr_last_error().decode()
    for off in (1, 2, 3):       # a half NHWC map off the 8-byte grid
        keep, v = hc.guarded16(nhwc16, DEV, offset=off)
        code, out = run_sample(eng, v, 1 | bits, pts, Hc, Wc, 0)
        assert code == nat.E_ARG and "aligned" in msg() and out.untouched(), off
        code, out = run_points(eng, v, 1 | bits, pts, (4, 4), Hc, Wc, 0)
        assert code == nat.E_ARG and "aligned" in msg() and out.untouched(), off
    keep, v = hc.guarded16(nhwc16, DEV)
    for fmt in (1 | nat.DENSE_F16 | nat.DENSE_BF16, 1 | 0x400, bits | 0x1000, 0x10000):      # both type bits, a higher bit
        code, out = run_sample(eng, v, fmt, pts, Hc, Wc, 0, ws_bytes=1 << 20)
        assert code == nat.E_ARG and "dense_is_nhwc" in msg() and out.untouched(), hex(fmt)
        code, out = run_points(eng, v, fmt, pts, (4, 4), Hc, Wc, 0)
        assert code == nat.E_ARG and out.untouched(), hex(fmt)


# =====================================================================================================================================
# 3. pooling kernels alone
# =====================================================================================================================================

@KINDS
@pytest.mark.parametrize("kernel", sorted(hc.POOL_KERNELS))
def test_pooling_kernels_on_a_half_map_equal_the_upcast(eng, kernel, kind):
    """cls_pool_online_kernel<1> (kernel 1) and <4> (kernel 3), bit for bit: both instantiations keep the float32 kernel's
    contractions (ragged_cases.DESC_BATCH_BAR, the bar between two batch compositions, is not drawn on)"""
    c = hc.pool_case()
    assert hc.pool_valid_tokens() == [5, 1, 3]
    Hc, Wc = hc.POOL_HW
    m16 = hc.map16(kind, 23, hc.POOL_IMAGES, Hc, Wc).permute(0, 2, 3, 1).contiguous()
    recs = torch.from_numpy(c["recs"].view(np.uint8).copy()).to(DEV)
    s2l = torch.from_numpy(c["sub2line"]).to(DEV)
    kc, cpnt = hc.guarded32(c["cpnt"], DEV)
    ka, a4 = hc.guarded32(c["a4"], DEV)
    outs = []
    for keep, dmap in (hc.guarded32(m16.float(), DEV), hc.guarded16(m16, DEV)):
        out = hc.Out((c["N"], 4, 544), torch.float32, DEV)
        _, used = eng.debug_cls_pool(kernel, a4, out.view, c["N"], c["T"], recs=recs, sub2line=s2l, cpnt=cpnt, first_pad=c["first_pad"],
                                     n_images=hc.POOL_IMAGES, dense_map=dmap, nhwc=True, Hc=Hc, Wc=Wc)
        torch.cuda.synchronize()
        assert used == kernel and out.guards_intact() and bool(torch.isfinite(out.view).all())
        outs.append(out)
    err = float((outs[0].view - outs[1].view).abs().max())
    print(f"{hc.POOL_KERNELS[kernel]} {kind}: max |half - upcast| {err:.2e}")
    assert hc.bits_equal(outs[0].view, outs[1].view), err


# =====================================================================================================================================
# 4. whole calls
# =====================================================================================================================================

def whole_batch(eng, sizes, seeds, n_lines):
    """records of a batch of images of `sizes` with seeded lines, and their float32 maps: (recs, cu_k, cu_n, lines, [(dd [1,256,Hc,Wc], ds)])"""
    lines = [synth.synth_lines(s, n, h, w, len_lo=17.0, len_hi=40.0) if n else np.zeros((0, 6)) for s, n, (h, w) in zip(seeds, n_lines, sizes)]
    maps = [synth.synth_dense_maps_np(s, h, w) for s, (h, w) in zip(seeds, sizes)]
    return lines, maps


def describe_raw(eng, entry, recs, cu_k, cu_n, dd, ds, H, W, fmt, slot=None):
    """linetr_describe / linetr_describe_submit as they are on device maps dd / ds, want_tokens on: (status, rc.Outputs)"""
    L = eng._L
    B, K, N = len(cu_k) - 1, int(cu_k[-1]), int(cu_n[-1])
    out = rc.Outputs(K, N, rc.T, 0, DEV)
    recs = np.ascontiguousarray(recs[:K])
    n_real = int(recs["n_tok"].sum())
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(DEV)
    cu_n32 = np.ascontiguousarray(cu_n, np.int32)
    need = L.linetr_describe_workspace_bytes(eng._h, B, H, W, N, n_real)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    tok = out.tokens(False, None)
    args = (eng._h, d_recs.data_ptr(), K, N, n_real, nat.np_ptr(cu_n32), None, B, 8.0, rc.T, dd.data_ptr(), ds.data_ptr(), H, W, 0, fmt, tok,
            out.views["sub2line"].data_ptr(), out.views["ld"].data_ptr(), ws.data_ptr(), need)
    with torch.cuda.device(eng.device):
        if entry == "describe":
            code = L.linetr_describe(*args, stream(eng))
        else:
            code = L.linetr_describe_submit(*args, 0, 2, stream(eng))
            if code == 0:
                nat.check(L.linetr_describe_join(eng._h, 0, stream(eng)), L)
        torch.cuda.synchronize()
    return code, out


def assert_same_outputs(a, b, what):
    for f in rc.TOK_FIELDS + ("ld",):
        assert hc.bits_equal(a.views[f], b.views[f]), (what, f)


@KINDS
@pytest.mark.parametrize("nhwc", [0, 1])
def test_describe_on_a_half_map(eng, nhwc, kind):
    """linetr_describe on two 64 x 96 images: every token tensor (out.desc included) and line_desc bit for bit the upcast call's;
    line_desc within 1e-4 of the oracle on the upcast map; linetr_describe_submit gives linetr_describe's bits"""
    dtype, bits = hc.HALF[kind]
    H, W = hc.WHOLE_HW
    lines, maps = whole_batch(eng, [(H, W)] * 2, (9400, 9401), (8, 8))
    recs, cu_k, cu_n = eng.prefilter(lines, H, W, remove_borders=rc.BORDER, min_length=16, max_keylines=-1, token_distance=8,
                                     max_tokens=rc.T, tie_order="stable")
    recs = recs.copy()
    d16 = torch.from_numpy(np.concatenate([m[0] for m in maps])).to(dtype)          # NCHW, rounded once
    ds = torch.from_numpy(np.concatenate([m[1] for m in maps]))
    lay = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if nhwc else (lambda t: t)
    k16, v16 = hc.guarded16(lay(d16), DEV)
    k32, v32 = hc.guarded32(lay(d16.float()), DEV)
    ks, vs = hc.guarded32(ds, DEV)
    code, ref = describe_raw(eng, "describe", recs, cu_k, cu_n, v32, vs, H, W, nhwc)
    nat.check(code, eng._L)
    code, got = describe_raw(eng, "describe", recs, cu_k, cu_n, v16, vs, H, W, nhwc | bits)
    nat.check(code, eng._L)
    assert got.guards_intact() and bool(torch.isfinite(got.views["ld"]).all())
    assert_same_outputs(got, ref, "half against upcast")
    code, sub = describe_raw(eng, "submit", recs, cu_k, cu_n, v16, vs, H, W, nhwc | bits)
    nat.check(code, eng._L)
    assert sub.guards_intact()
    assert_same_outputs(sub, got, "submit against describe")
    sd_t = synth.to_torch_state_dict(synth.calibrated_state_dict())
    cfg = dict(min_length=16, token_distance=8, max_tokens=rc.T, remove_borders=rc.BORDER, max_keylines=-1)
    for j in range(2):
        o = oracle_image(sd_t, lines[j], d16[j:j + 1].float(), ds[j:j + 1], (H, W), cfg, None, False, (480, 640))
        rows = slice(int(cu_n[j]), int(cu_n[j + 1]))
        err = np.abs(got.views["ld"][rows].cpu().numpy().T - o["line_desc"][0].numpy()).max()
        print(f"image {j}: max |line_desc - oracle(upcast)| {err:.2e} / {rc.DESC_ORACLE_BAR:.0e}")
        assert err <= rc.DESC_ORACLE_BAR, (j, err)


@KINDS
@pytest.mark.parametrize("nhwc", [0, 1])
def test_describe_ragged_on_half_maps(eng, nhwc, kind):
    """linetr_describe_ragged on 64 x 96 + 40 x 24 + an image without lines"""
    dtype, bits = hc.HALF[kind]
    sizes = [hc.WHOLE_HW, hc.SMALL_HW, hc.WHOLE_HW]
    lines, maps = whole_batch(eng, sizes, (9410, 9411, 9412), (8, 3, 0))
    # lines that fit a 40 x 24 image inside its border (max_keylines = -1 is the reference's [:-1]: the shortest of them is dropped)
    fit = [(8.5, 8.5, 14.5, 30.5), (15.0, 9.0, 9.5, 31.0), (9.0, 12.0, 15.5, 29.0)]
    lines[1] = np.array([[sx, sy, ex, ey, float(np.float32(np.hypot(ex - sx, ey - sy))), 0.0] for sx, sy, ex, ey in fit])
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.int32)
    table = np.zeros(3, dtype=nat.PREFILTER_IMAGE_DTYPE)
    for j, (h, w) in enumerate(sizes):
        table[j] = (h, w, 16.0, 8.0, 0)
    code, recs, cu_k, cu_n = rc.prefilter_ragged(eng._L, lines, off, table, -1, 1)
    nat.check(code, eng._L)
    assert cu_k[3] == cu_k[2] and cu_k[2] > cu_k[1] > 0
    lay = (lambda t: t.permute(1, 2, 0).contiguous()) if nhwc else (lambda t: t)
    d16 = [torch.from_numpy(m[0][0]).to(dtype) for m in maps]
    half = [(hc.guarded16(lay(d), DEV)[1], hc.guarded32(torch.from_numpy(m[1][0]), DEV)[1], None) for d, m in zip(d16, maps)]
    full = [(hc.guarded32(lay(d.float()), DEV)[1], s, None) for d, (_, s, _) in zip(d16, half)]
    tds = [8.0] * 3
    code, ref, _ = rc.describe_ragged(eng, recs, cu_k, cu_n, rc.image_table(full, tds), nhwc, 0, True)
    nat.check(code, eng._L)
    code, got, nbytes = rc.describe_ragged(eng, recs, cu_k, cu_n, rc.image_table(half, tds), nhwc | bits, 0, True)
    nat.check(code, eng._L)
    assert got.guards_intact() and bool(torch.isfinite(got.views["ld"]).all())
    for f in rc.TOK_FIELDS + ("ld", "mat"):
        assert hc.bits_equal(got.views[f], ref.views[f]), f
    sd_t = synth.to_torch_state_dict(synth.calibrated_state_dict())
    for j in range(2):
        h, w = sizes[j]
        cfg = dict(min_length=16, token_distance=8, max_tokens=rc.T, remove_borders=rc.BORDER, max_keylines=-1)
        o = oracle_image(sd_t, lines[j], d16[j][None].float(), torch.from_numpy(maps[j][1]), (h, w), cfg, None, False, (480, 640))
        rows = slice(int(cu_n[j]), int(cu_n[j + 1]))
        err = np.abs(got.views["ld"][rows].cpu().numpy().T - o["line_desc"][0].numpy()).max()
        print(f"image {j}: max |line_desc - oracle(upcast)| {err:.2e} / {rc.DESC_ORACLE_BAR:.0e}")
        assert err <= rc.DESC_ORACLE_BAR, (j, err)


@KINDS
def test_fixed_size_batch_still_upcasts_a_half_map(eng, kind):
    """Engine.fixed_size_batch (linetr_fixed_size takes float32 maps only) on a half map: what it gives on map16.float(), as before"""
    dtype, bits = hc.HALF[kind]
    H, W = hc.WHOLE_HW
    rows = synth.synth_lines(9400, 8, H, W, len_lo=17.0, len_hi=40.0)
    _, maps = whole_batch(eng, [(H, W)] * 2, (9400, 9401), (0, 0))
    recs, cu_k, cu_n = eng.prefilter([rows, rows], H, W, remove_borders=rc.BORDER, min_length=16, max_keylines=-1, token_distance=8,
                                     max_tokens=rc.T, tie_order="stable")
    recs = recs.copy()
    M = int(cu_k[1])                      # as many sub-lines as key-lines: no pseudo line is needed, every image is cut to M
    assert 0 < M <= int(cu_n[1]) and int(cu_k[2]) == 2 * M
    d16 = torch.from_numpy(np.concatenate([m[0] for m in maps])).to(dtype).to(DEV)
    ds = torch.from_numpy(np.concatenate([m[1] for m in maps])).to(DEV)
    for layout in ("nchw", "nhwc"):
        dd = d16.permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else d16
        kw = dict(max_sublines=M, token_distance=8, max_tokens=rc.T, dense_layout=layout)
        a = eng.fixed_size_batch(recs, cu_k, cu_n, dd, ds, **kw)
        b = eng.fixed_size_batch(recs, cu_k, cu_n, dd.float(), ds, **kw)
        torch.cuda.synchronize()
        for k in eng.fixed_size_shapes(2, M, rc.T):
            assert hc.bits_equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()), (layout, k)
        assert torch.equal(a["num_slns"], b["num_slns"])


def test_ragged_size_query_with_format_bits(eng):
    """linetr_describe_ragged_workspace_bytes with a real handle: a half format needs no more than float32, a refused one answers -1"""
    L = eng._L
    table = np.zeros(2, dtype=nat.IMAGE_DTYPE)
    table[0] = (4096, 8192, 64, 96, 8.0)
    table[1] = (4096, 8192, 40, 24, 8.0)
    q = lambda fmt: L.linetr_describe_ragged_workspace_bytes(eng._h, nat.np_ptr(table), 2, fmt, 12, 40)
    for nhwc in (0, 1):
        f32 = q(nhwc)
        assert f32 > 0
        for bits in (nat.DENSE_F16, nat.DENSE_BF16):
            assert 0 < q(nhwc | bits) <= f32, (nhwc, bits)
        assert q(nhwc | nat.DENSE_F16) < f32 or nhwc          # the half channel-last copies of the NCHW maps are smaller
        for fmt in (nhwc | nat.DENSE_F16 | nat.DENSE_BF16, nhwc | 0x400, nhwc | nat.DENSE_BF16 | 0x1000):
            assert q(fmt) == -1, hex(fmt)
    table[0]["d_dense_desc"] = 4096 + 4          # a half NHWC map off the 8-byte grid; a half NCHW map may lie there
    assert q(1 | nat.DENSE_F16) == -1 and q(nat.DENSE_F16) > 0


def test_fixed_size_refuses_a_format_bit(eng):
    L = eng._L
    z = torch.zeros(1 << 16, device=DEV)
    tok = nat.Tokens()
    for k in ("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "desc", "score", "mat"):
        setattr(tok, k, z.data_ptr())
    cu = np.zeros(2, np.int32)
    for fmt in (nat.DENSE_F16, 1 | nat.DENSE_BF16, 0x400):
        assert L.linetr_fixed_size_workspace_bytes(1, 64, 96, fmt) == 0
        marker = z.clone()
        code = L.linetr_fixed_size(eng._h, None, nat.np_ptr(cu), nat.np_ptr(cu), None, None, nat.np_ptr(cu), 1, 4, rc.T, 8.0, z.data_ptr(),
                                   z.data_ptr(), 64, 96, 0, 0, 0, 0, 0, fmt, tok, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1 << 18, stream(eng))
        torch.cuda.synchronize()
        assert code == nat.E_ARG and "float32" in L.linetr_last_error().decode(), hex(fmt)
        assert torch.equal(z, marker)


# =====================================================================================================================================
# 5. Python surface
# =====================================================================================================================================

@KINDS
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_engine_describe_reads_a_half_map_in_place(eng, layout, kind):
    dtype, bits = hc.HALF[kind]
    H, W = hc.WHOLE_HW
    lines, maps = whole_batch(eng, [(H, W)] * 2, (9400, 9401), (8, 8))
    recs, cu_k, cu_n = eng.prefilter(lines, H, W, remove_borders=rc.BORDER, min_length=16, max_keylines=-1, token_distance=8,
                                     max_tokens=rc.T, tie_order="stable")
    recs = recs.copy()
    d16 = torch.from_numpy(np.concatenate([m[0] for m in maps])).to(dtype).to(DEV)
    if layout == "nhwc":
        d16 = d16.permute(0, 2, 3, 1).contiguous()
    ds = torch.from_numpy(np.concatenate([m[1] for m in maps])).to(DEV)
    passed, passed_bits = eng._dense_map(d16)
    assert passed_bits == bits and passed.data_ptr() == d16.data_ptr() and passed.dtype == dtype      # in place: no copy
    kw = dict(token_distance=8, max_tokens=rc.T, want_tokens=True, dense_layout=layout)
    tb16, ld16 = eng.describe(recs, cu_k, cu_n, d16, ds, **kw)
    tb32, ld32 = eng.describe(recs, cu_k, cu_n, d16.float(), ds, **kw)
    assert hc.bits_equal(ld16, ld32) and hc.bits_equal(tb16.desc, tb32.desc) and hc.bits_equal(tb16.pnt, tb32.pnt)
    # the ragged surface: one type in place, mixed types upcast together -- the same numbers either way
    per = [d16[i] for i in range(2)]
    _, ldr = eng.describe_ragged(recs, cu_k, cu_n, per, [ds[0], ds[1]], token_distance=8, max_tokens=rc.T, dense_layout=layout)
    _, ldm = eng.describe_ragged(recs, cu_k, cu_n, [per[0], per[1].float()], [ds[0], ds[1]], token_distance=8, max_tokens=rc.T, dense_layout=layout)
    assert hc.bits_equal(ldr, ld32) and hc.bits_equal(ldm, ld32)
    pts = hc.sample_points(H // 8, W // 8).to(DEV)
    assert hc.bits_equal(eng.sample_descriptors(pts, d16[0], dense_layout=layout), eng.sample_descriptors(pts, d16[0].float(), dense_layout=layout))


class TinySuperPoint(torch.nn.Module):
    """the reference SuperPoint's attributes and helper functions in miniature (seeded 3x3 / 1x1 convolutions of the same names)"""
    config = {"nms_radius": 4, "keypoint_threshold": 0.005, "remove_borders": 4, "max_keypoints": -1}

    def __init__(self):
        super().__init__()
        torch.manual_seed(77)
        nn = torch.nn
        self.relu, self.pool = nn.ReLU(inplace=True), nn.MaxPool2d(2, 2)
        c = [1, 8, 8, 8, 8, 16, 16, 16, 16]
        for name, i in zip(("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"), range(8)):
            setattr(self, name, nn.Conv2d(c[i], c[i + 1], 3, padding=1))
        self.convPa, self.convPb = nn.Conv2d(16, 32, 3, padding=1), nn.Conv2d(32, 65, 1)
        self.convDa, self.convDb = nn.Conv2d(16, 32, 3, padding=1), nn.Conv2d(32, 256, 1)


@KINDS
def test_fused_head_superpoint_in_half_precision(eng, kind):
    from linetr_amd.superpoint import FusedHeadSuperPoint
    dtype, bits = hc.HALF[kind]
    sp = TinySuperPoint().to(DEV).to(dtype).eval()
    img = torch.rand((2, 1, 40, 56), generator=hc._gen("image")).to(DEV).to(dtype)
    fused = FusedHeadSuperPoint(sp, engine=eng, native_keypoints=True, align_corners=True)
    out = fused({"image": img})
    logits, raw = fused.encode(img)
    assert logits.dtype == dtype and raw.dtype == dtype
    score, nhwc, nchw = eng.superpoint_heads(logits.float(), raw.float(), nhwc=True, nchw=True)
    assert out["dense_descriptor"].dtype == torch.float32 and out["dense_score"].dtype == torch.float32
    assert hc.bits_equal(out["dense_score"], score) and hc.bits_equal(out["dense_descriptor_nhwc"], nhwc)
    assert hc.bits_equal(out["dense_descriptor"], nchw)
    half = FusedHeadSuperPoint(sp, engine=eng, native_keypoints=True, align_corners=True, dense_dtype=dtype)({"image": img})
    assert half["dense_descriptor"].dtype == dtype and half["dense_descriptor_nhwc"].dtype == dtype
    assert all(d.dtype == dtype for d in half["descriptors"]) and half["dense_score"].dtype == torch.float32
    assert hc.bits_equal(half["dense_descriptor_nhwc"], nhwc.to(dtype)) and hc.bits_equal(half["dense_descriptor"], nchw.to(dtype))
    assert len(half["keypoints"]) == 2 and all(k.dtype == torch.float32 for k in half["keypoints"])


@pytest.mark.parametrize("native_keypoints", [False, True])
def test_matching_forward_with_half_dense_maps(monkeypatch, native_keypoints):
    """Matching.forward at the asset pair's size with its two line lists and config['dense_dtype'] = float16 (the golden holds no
    pixels: seeded images through a SuperPoint with the reference's layers and seeded weights): the key set of the float32 run, half
    descriptor maps, float32 finite line descriptors of the same shapes"""
    import sys
    import types
    from helpers import load
    from test_gpu_producer import _Helpers, _StandInSuperPoint

    class SuperPoint(_StandInSuperPoint):
        def __init__(self, config):
            super().__init__()
            self.config = {**self.config, "nn_threshold": 0.7, "max_keypoints": 256, **config}
            self.load_state_dict({k: torch.from_numpy(v) for k, v in synth.superpoint_state_dict(0).items()})

    mod = types.ModuleType("models.superpoint")
    mod.SuperPoint = SuperPoint
    for fn in ("simple_nms", "remove_borders", "top_k_keypoints", "sample_descriptors"):
        setattr(mod, fn, getattr(_Helpers, fn))
    SuperPoint.__module__ = "models.superpoint"
    monkeypatch.setitem(sys.modules, "models.superpoint", mod)
    from linetr_amd.superpoint import FusedHeadSuperPoint
    from models.matching import Matching
    g = load("asset_pair")
    H, W = (int(v) for v in g["hw"])
    rs = np.random.RandomState(3)
    imgs = [torch.from_numpy(rs.rand(1, 1, H, W).astype(np.float32)).to(DEV) for _ in range(2)]
    lt_cfg = {"mode": "train", "max_keylines": -1, "min_length": 16, "token_distance": 8, "nn_threshold": 0.8}
    preds = []
    for dense_dtype in (None, torch.float16):
        mt = Matching({"auto_min_length": True, "linetransformer": dict(lt_cfg), "native_keypoints": native_keypoints, "dense_dtype": dense_dtype},
                      lsd=rc.FakeLSD([g["lines0"], g["lines1"]]))
        assert isinstance(mt.superpoint, FusedHeadSuperPoint) and mt.superpoint.dense_dtype == dense_dtype
        mt.linetransformer.load_state_dict(synth.to_torch_state_dict(synth.calibrated_state_dict()))
        preds.append(mt.eval().to(DEV)({"image0": imgs[0], "image1": imgs[1]}))
    full, half = preds
    assert set(half) == set(full) and "line_desc0" in half and "matches_l" in half
    for s in "01":
        assert half["dense_descriptor" + s].dtype == torch.float16 and half["dense_descriptor_nhwc" + s].dtype == torch.float16
        assert half["dense_score" + s].dtype == torch.float32
        ld = half["line_desc" + s]
        assert ld.dtype == torch.float32 and ld.shape == full["line_desc" + s].shape and bool(torch.isfinite(ld).all())
        assert torch.equal(half["klines" + s].cpu(), full["klines" + s].cpu())
        print(f"image {s}: max |line_desc(fp16 maps) - line_desc(float32 maps)| {float((ld - full['line_desc' + s]).abs().max()):.2e}")
