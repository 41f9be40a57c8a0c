"""Case generator, references and error measure of the unit tests of the kernels that read and write the dense maps
(tests/test_gpu_sampler.py, tests/test_gpu_heads_edges.py, tests/test_sample_cases_cpu.py; reused by tools/sampler_unit_report.py,
which writes profiles/sampler_unit_errors.txt).  Test infrastructure only.

The samplers are sample_desc_kernel and sp_kp_desc_kernel (lt_token.h, both on sample_one); the heads are sp_desc_head_kernel and
sp_score_head_kernel (lt_producer.h), each fed NCHW or channel-last rows.  Every case has two CPU references of the same formula,
float64 (`ref64`) and plain float32 torch (`ref32`), both built from the same float32-representable inputs:

    samplers   oracle.linetr_oracle.sample_token_desc (models/line_process.py:86-98: grid_sample, zero padding, F.normalize)
    heads      softmax over the 65 logits + depth-to-space of the first 64 (models/superpoint.py:161-167); F.normalize over the
               256 channels (:190-193)

A kernel passes a case (an image of a batch, where a call has several) when

    max |gpu - ref64|  <=  FACTOR * max( max |ref32 - ref64| ,  2^-23 * max |ref64| )        (FACTOR = 8, as attn_cases.py)

The bar is a property of the CPU references alone, never of a kernel's output.  Where ref64 is an exactly zero vector (every tap
outside the map: F.normalize's eps branch) the kernel's vector must be exactly zero, and the exact families (`onehot`, `onehot65`) are compared
bit for bit; both are reported as an error against a bar of 0.

The normalised sample is discontinuous where the un-normalised grid coordinate crosses -1 or the cell count (the last tap leaves the
map: a unit vector becomes the zero vector), so every generated point keeps MARGIN cells from those values in float64
(tests/test_sample_cases_cpu.py asserts it)."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from attn_cases import FACTOR, MARKER, SENTINEL, SPARE_ROWS, _gen, cu_of
from linetr_amd import _native as nat
from oracle import linetr_oracle as O

D = 256
CELL = 8
MARGIN = 1e-3                      # cells between any point's grid coordinate and the discontinuities at -1 and the cell count


def _sentinel(shape, g):
    return SENTINEL * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def _max(t):
    return t.abs().max().item() if t.numel() else 0.0


def bar_of(r64, r32):
    return FACTOR * max(_max(r32.double() - r64), 2.0 ** -23 * _max(r64))


def failures(rows):
    """rows: (kernel, family, where, error, bar)"""
    return [f"{k} / {f} / {w}: error {e:.3e} > bar {b:.3e} (x{e / b if b else float('inf'):.1f})" for k, f, w, e, b in rows if not e <= b]


def worst(rows):
    """{(kernel, family, map): [units, worst error / bar, where]} -- what the GPU tests print and the report tool writes"""
    stat = {}
    for k, f, w, e, b in rows:
        s = stat.setdefault((k, f, w.split(",")[0]), [0, 0.0, ""])
        s[0] += 1
        ratio = e / b if b else (0.0 if e == 0 else float("inf"))
        if ratio >= s[1]:
            s[1], s[2] = ratio, f"{w}: err {e:.3e}, bar {b:.3e}"
    return stat


def worst_lines(rows):
    return [f"{k:<24s} {f:<18s} {m:<7s} units {s[0]:5d}  worst error / bar {s[1]:6.3f}   ({s[2]})" for (k, f, m), s in worst(rows).items()]


# =================================================================================================================================
# samplers
# =================================================================================================================================

MAPS = ((1, 1), (1, 2), (2, 1), (3, 5), (7, 9), (8, 8), (60, 80))          # Hc x Wc
SAMPLER_FAMILIES = ("normal", "border", "planted")
SAMPLE_N = (1, 3, 4, 5, 8, 9)                                              # sample_desc_kernel: four points per block
N_POINTS = 40                                                              # points of a `normal` / `planted` case
KP_COUNTS = (0, 1, 63, 64, 65, 128, 129)                                   # sp_kp_desc_kernel: 64 key points per block
KP_BATCHES = ((1,), (63,), (64,), (65,), (128,), (129,),                   # B = 1, 3, 4; the empty image first, in the middle, last
              (0, 64, 129), (65, 0, 1), (128, 63, 0), (0, 129, 0, 65), (1, 64, 63, 0), (129, 1, 128, 65))
KP_MAPS = ((3, 5), (7, 9))


def grid_coord(p, cells, align_corners):
    """the un-normalised grid coordinate (in cells) of pixel coordinate `p` along an axis of `cells` cells, in p's precision
    (line_process.py:88-92 and grid_sample's un-normalisation)"""
    g = (p - CELL / 2 + 0.5) / (cells * CELL - CELL / 2 - 0.5) * 2 - 1
    return (g + 1) * (cells - 1) / 2 if align_corners else (g + 1) * cells / 2 - 0.5


def margin(points, Hc, Wc, align_corners):
    """[n]: cells between every point's grid coordinates and the nearest discontinuity (-1 or the cell count, either axis), float64"""
    p = points.double()
    m = torch.full((p.shape[0],), float("inf"), dtype=torch.float64)
    for axis, cells in ((0, Wc), (1, Hc)):
        c = grid_coord(p[:, axis], cells, align_corners)
        m = torch.minimum(m, torch.minimum((c + 1).abs(), (c - cells).abs()))
    return m


def border_values(cells):
    """per-axis coordinates of the `border` family: zero to two taps of the axis outside the map"""
    size = float(CELL * cells)
    return (-6.0, -0.3, 0.0, 0.5, 3.4, 3.5, 3.6, size / 2, size - 4.4, size - 1, size - 0.6, size + 0.2, size + 6)


def border_points(Hc, Wc):
    """[169, 2]: the Cartesian product of the axes' border values"""
    return torch.tensor(list(itertools.product(border_values(Wc), border_values(Hc))), dtype=torch.float32)


def uniform_points(n, Hc, Wc, g):
    """n points uniform over the image, those closer than MARGIN to a discontinuity (under either align_corners value) drawn again"""
    out = torch.zeros((0, 2))
    while out.shape[0] < n:
        p = torch.rand((2 * n + 8, 2), generator=g) * torch.tensor([float(CELL * Wc), float(CELL * Hc)])
        ok = torch.minimum(margin(p, Hc, Wc, False), margin(p, Hc, Wc, True)) >= 2 * MARGIN
        out = torch.cat([out, p[ok]])
    return out[:n].contiguous()


@functools.lru_cache(maxsize=None)
def dense_maps(n_images, hw_cells, planted=False):
    """unit-norm NCHW maps [n_images, 256, Hc, Wc], a different one per image.  planted: cell (h, w) of every image is the one-hot unit
    vector of channel (h * Wc + w) % 256 (maps of at most 256 cells: a wrong tap names the cell it came from)"""
    Hc, Wc = hw_cells
    if planted:
        if Hc * Wc > D:
            raise ValueError("planted maps hold at most 256 cells")
        m = torch.zeros((D, Hc * Wc))
        m[torch.arange(Hc * Wc) % D, torch.arange(Hc * Wc)] = 1.0
        return m.view(1, D, Hc, Wc).expand(n_images, D, Hc, Wc).contiguous()
    return F.normalize(torch.randn((n_images, D, Hc, Wc), generator=_gen("sample map", n_images, hw_cells)), p=2, dim=1)


def sample_reference(points, image, dense, align_corners, dtype):
    """[n, 256] in `dtype`: sample_token_desc of every point in its image's map"""
    out = torch.zeros((points.shape[0], D), dtype=dtype)
    for i in range(dense.shape[0]):
        sel = (image == i).nonzero()[:, 0]
        if len(sel):
            d = O.sample_token_desc(points[sel].to(dtype).view(1, -1, 1, 2), dense[i:i + 1].to(dtype), CELL, bool(align_corners))
            out[sel] = d[0].t()
    return out


def build_case(kernel, family, points, image, dense, align_corners, **extra):
    """dict: points [n, 2] float32, image [n] (the map every point is sampled in), dense [B, 256, Hc, Wc], ref64 / ref32 [n, 256], zero
    [n] (ref64 is the zero vector: every tap outside)"""
    r64 = sample_reference(points, image, dense, align_corners, torch.float64)
    r32 = sample_reference(points, image, dense, align_corners, torch.float32)
    return dict(kernel=kernel, family=family, points=points.contiguous(), image=image, dense=dense, Hc=int(dense.shape[2]),
                Wc=int(dense.shape[3]), align_corners=bool(align_corners), ref64=r64, ref32=r32, zero=(r64 == 0).all(dim=1), **extra)


def label(case):
    return f"{case['Hc']}x{case['Wc']}, align_corners={int(case['align_corners'])}"


@functools.lru_cache(maxsize=None)
def sampler_case(family, hw_cells, align_corners):
    """One image and its points, for linetr_sample_descriptors (the GPU test also runs every prefix of SAMPLE_N points).  Families:
      normal    N_POINTS points uniform over the image
      border    the 169 points of border_points(), shuffled
      planted   `normal` points in the one-hot map"""
    if family not in SAMPLER_FAMILIES:
        raise ValueError(family)
    Hc, Wc = hw_cells
    g = _gen("sampler", family, hw_cells)
    if family == "border":
        pts = border_points(Hc, Wc)
        pts = pts[torch.randperm(pts.shape[0], generator=g)]
    else:
        pts = uniform_points(N_POINTS, Hc, Wc, g)
    dense = dense_maps(1, hw_cells, family == "planted")
    return build_case("sample_desc", family, pts, torch.zeros(pts.shape[0], dtype=torch.long), dense, align_corners)


def sampler_cases():
    for family in SAMPLER_FAMILIES:
        for hw in MAPS:
            if family == "planted" and hw[0] * hw[1] > D:
                continue
            for ac in (False, True):
                yield sampler_case(family, hw, ac)


@functools.lru_cache(maxsize=None)
def keypoint_case(counts, hw_cells, align_corners):
    """A batch of packed key points for linetr_point_descriptors: image b has counts[b] points, every second one from the `border`
    product, the others uniform; every image has its own map"""
    Hc, Wc = hw_cells
    g = _gen("keypoints", counts, hw_cells)
    n = int(sum(counts))
    pts = uniform_points(n, Hc, Wc, g)
    edge = border_points(Hc, Wc)
    pick = torch.randint(0, edge.shape[0], (n,), generator=g)
    pts[1::2] = edge[pick[1::2]]
    image = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    return build_case("sp_kp_desc", "counts", pts, image, dense_maps(len(counts), hw_cells), align_corners, counts=counts, cu=cu_of(counts))


def keypoint_cases():
    for i, counts in enumerate(KP_BATCHES):
        for j, hw in enumerate(KP_MAPS):
            yield keypoint_case(counts, hw, bool((i + j) % 2))


def sample_errors(got, case, rows=None, where=""):
    """[(kernel, family, where, error, bar)] of sampled rows `rows` (default: all): max |got - ref64| against the references' bar, and
    -- where ref64 holds exactly zero vectors -- the largest magnitude the kernel wrote there against a bar of 0"""
    rows = slice(None) if rows is None else rows
    r64, r32, zero = case["ref64"][rows], case["ref32"][rows], case["zero"][rows]
    if r64.shape[0] == 0:
        return []
    where = label(case) + (", " + where if where else "")
    out = [(case["kernel"], case["family"], where, _max(got.double() - r64), bar_of(r64, r32))]
    if bool(zero.any()):
        out.append((case["kernel"], case["family"] + "/zero", where, _max(got[zero]), 0.0))
    return out


def explain_planted(got, case, rows=None):
    """for a `planted` case: the cells whose channel is off by more than the bar, per point"""
    rows = slice(None) if rows is None else rows
    r64, r32 = case["ref64"][rows], case["ref32"][rows]
    bad = ((got.double() - r64).abs() > bar_of(r64, r32)).nonzero()
    return [f"point {int(i)} {case['points'][rows][int(i)].tolist()}: cell {divmod(int(c), case['Wc'])} has {got[int(i), int(c)].item():.6f}, "
            f"expected {r64[int(i), int(c)].item():.6f}" for i, c in bad[:8]]


# ---- a CPU restatement of the samplers in float32, with the mistakes the bars have to catch -------------------------------------

MISTAKES = ("neighbour", "clamp", "image0")


def restate(case, mistake=None):
    """[n, 256] float32: sample_one's arithmetic restated in torch (lt_token.h), every point in its image's map.  mistake:
      neighbour   the south-east tap is taken from the cell to its right (clamped into the map)
      clamp       taps outside the map read the nearest cell instead of zero
      image0      every point is sampled in image 0's map"""
    if mistake not in (None,) + MISTAKES:
        raise ValueError(mistake)
    Hc, Wc, ac = case["Hc"], case["Wc"], case["align_corners"]
    p = case["points"]
    nhwc = case["dense"].permute(0, 2, 3, 1)
    img = torch.zeros_like(case["image"]) if mistake == "image0" else case["image"]

    def coord(v, cells):
        g = ((v - CELL / 2) + 0.5) / torch.tensor(cells * CELL - CELL / 2 - 0.5, dtype=torch.float32) * 2.0 - 1.0
        return (g + 1.0) * ((cells - 1) / 2.0) if ac else (g + 1.0) * (cells / 2.0) - 0.5
    ix, iy = coord(p[:, 0], Wc), coord(p[:, 1], Hc)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    w, n = ix - x0, iy - y0
    e, s = 1.0 - w, 1.0 - n
    acc = torch.zeros((p.shape[0], D))
    for k, wt in enumerate((s * e, s * w, n * e, n * w)):
        yy, xx = y0.long() + (k >> 1), x0.long() + (k & 1)
        if mistake == "neighbour" and k == 3:
            xx = xx + 1
        inside = (xx >= 0) & (xx < Wc) & (yy >= 0) & (yy < Hc)
        if mistake == "neighbour" and k == 3:
            inside = (xx - 1 >= 0) & (xx - 1 < Wc) & (yy >= 0) & (yy < Hc)
        v = nhwc[img, yy.clamp(0, Hc - 1), xx.clamp(0, Wc - 1)]
        if mistake != "clamp":
            v = v * inside[:, None]
        acc = acc + v * wt[:, None]
    return acc / acc.norm(dim=1, keepdim=True).clamp_min(1e-12)


def kp_blocks(desc_rows, cu, shifted=None):
    """What sp_kp_desc_kernel writes: image b's [256][n_b] block at 256 cu[b], from rows [n_total, 256].  shifted = (image, chunk): that
    chunk of 64 key points is written one column off (its last column falls into the next chunk, or out of the block)"""
    out = torch.zeros((D * int(cu[-1]),))
    for b in range(len(cu) - 1):
        a, n = int(cu[b]), int(cu[b + 1] - cu[b])
        blk = desc_rows[a:a + n].t().clone()
        if shifted is not None and shifted[0] == b:
            j0 = 64 * shifted[1]
            nj = min(64, n - j0)
            src = desc_rows[a + j0:a + j0 + nj].t()
            blk[:, j0:j0 + nj] = 0.0
            blk[:, j0 + 1:min(j0 + 1 + nj, n)] = src[:, :min(nj, n - j0 - 1)]
        out[D * a:D * (a + n)] = blk.reshape(-1)
    return out


def kp_block_errors(flat, case, where=""):
    """sample_errors of every image's [256][n_b] block of the flat output"""
    rows = []
    cu = case["cu"]
    for b in range(len(cu) - 1):
        a, n = int(cu[b]), int(cu[b + 1] - cu[b])
        if n:
            rows += sample_errors(flat[D * a:D * (a + n)].view(D, n).t(), case, slice(a, a + n), f"counts {case['counts']} image {b}" + where)
    return rows


# ---- launches ---------------------------------------------------------------------------------------------------------------------

def _layout(nchw, layout):
    return nchw if layout == "nchw" else nchw.permute(0, 2, 3, 1).contiguous()


def guarded_map(case, layout, device, n_images=None):
    """the case's maps on the device in `layout` with one more image of +-1e4 behind them; returns the view of the real images"""
    dense = case["dense"] if n_images is None else case["dense"][:n_images]
    g = _gen("guard map", case["Hc"], case["Wc"])
    buf = torch.cat([_layout(dense, layout), _layout(_sentinel((1,) + tuple(dense.shape[1:]), g), layout)]).to(device)
    return buf[:dense.shape[0]]


def run_sample_descriptors(eng, case, n, layout):
    """the case's first n points through Engine.sample_descriptors; SPARE_ROWS points of +-1e4 and a map of +-1e4 lie behind the inputs"""
    pts = torch.cat([case["points"][:n], _sentinel((SPARE_ROWS, 2), _gen("guard points", n))]).to(eng.device)
    dd = guarded_map(case, layout, eng.device)
    out = eng.sample_descriptors(pts[:n], dd[0], align_corners=case["align_corners"], dense_layout=layout)
    torch.cuda.synchronize()
    return out.cpu()


def run_point_descriptors(eng, case, layout):
    """linetr_point_descriptors through the C ABI, twice; returns the flat output [256 n_total] on the CPU after asserting that the
    256 floats behind it still hold the marker and that both calls gave the same bits"""
    L, dev = eng._L, eng.device
    cu, B, n_total = case["cu"], len(case["counts"]), int(case["cu"][-1])
    kp = torch.cat([case["points"], _sentinel((SPARE_ROWS, 2), _gen("guard kp", case["counts"]))]).to(dev)
    d_cu = torch.from_numpy(np.ascontiguousarray(cu, dtype=np.int32)).to(dev)
    dd = guarded_map(case, layout, dev)
    need = L.linetr_point_descriptors_workspace_bytes(B, case["Hc"], case["Wc"], int(layout == "nhwc"))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((D * n_total + D,), MARKER, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nat.check(L.linetr_point_descriptors(eng._h, kp.data_ptr(), d_cu.data_ptr(), B, n_total, dd.data_ptr(), case["Hc"], case["Wc"],
                                                 int(case["align_corners"]), int(layout == "nhwc"), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 eng._stream()), L)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert bool((outs[0][D * n_total:] == MARKER).all()), f"counts {case['counts']}: the floats behind the output were written"
    assert torch.equal(outs[0], outs[1]), f"counts {case['counts']}: two calls gave different bits"
    return outs[0][:D * n_total]


def sweep_sample_descriptors(eng):
    """every sampler case through linetr_sample_descriptors at every prefix length of SAMPLE_N and in full, both layouts"""
    rows = []
    for case in sampler_cases():
        for n in SAMPLE_N + (case["points"].shape[0],):
            got = {layout: run_sample_descriptors(eng, case, n, layout) for layout in ("nhwc", "nchw")}
            r = sample_errors(got["nhwc"], case, slice(0, n), f"n {n}")
            if case["family"] == "planted" and failures(r):
                r[0] = r[0][:2] + (r[0][2] + " " + "; ".join(explain_planted(got["nhwc"], case, slice(0, n))),) + r[0][3:]
            rows += r
            rows.append((case["kernel"], case["family"] + "/layouts", label(case) + f", n {n}", _max(got["nhwc"] - got["nchw"]), 0.0))
    return rows


def sweep_point_descriptors(eng):
    """every key-point batch through linetr_point_descriptors: blocks against ref64 and, bit for bit, against linetr_sample_descriptors
    of the same image (transposed)"""
    rows = []
    for i, case in enumerate(keypoint_cases()):
        layout = ("nhwc", "nchw")[(i // 2) % 2]
        flat = run_point_descriptors(eng, case, layout)
        rows += kp_block_errors(flat, case, f" {layout}")
        cu = case["cu"]
        for b in range(len(cu) - 1):
            a, n = int(cu[b]), int(cu[b + 1] - cu[b])
            if n == 0:
                continue
            one = eng.sample_descriptors(case["points"][a:a + n].to(eng.device), guarded_map(case, "nhwc", eng.device)[b],
                                         align_corners=case["align_corners"], dense_layout="nhwc").cpu()
            rows.append((case["kernel"], "counts/same", label(case) + f", counts {case['counts']} image {b}",
                         _max(flat[D * a:D * (a + n)].view(D, n).t() - one), 0.0))
    return rows


TOK_HW = (64, 96)
TOK_T = (1, 3, 5)


@functools.lru_cache(maxsize=None)
def tokenize_maps():
    """three images' descriptor maps [3, 256, 8, 12] and score maps [3, 64, 96], every image its own"""
    return dense_maps(3, (TOK_HW[0] // CELL, TOK_HW[1] // CELL)), torch.rand((3,) + TOK_HW, generator=_gen("score maps"))


def sweep_tokenize(eng):
    """sample_desc_kernel with records and the tokeniser's score gather: detector lines on three 64 x 96 images with different maps
    through Engine.prefilter + Engine.tokenize.  desc against ref64 at the returned pnt, image by image; score bit-equal to the
    image's own map at the rounded coordinates (torch.round: half to even; clipped to the map)"""
    from test_gpu_tokenizer_fuzz import BORDER, MIN_LEN, fuzz_lines
    H, W = TOK_HW
    Hc, Wc = H // CELL, W // CELL
    dense, score = tokenize_maps()
    rows = []
    for T in TOK_T:
        lines = [fuzz_lines(4000 + 10 * T + i, 12, 8, T, hw=TOK_HW) for i in range(3)]
        recs, cu_k, cu_n = eng.prefilter(lines, H, W, remove_borders=BORDER, min_length=MIN_LEN, max_keylines=-1, token_distance=8, max_tokens=T)
        for ac in (False, True):
            for layout in ("nchw", "nhwc"):
                tb = eng.tokenize(recs, cu_k, cu_n, _layout(dense, layout).to(eng.device), score.to(eng.device), token_distance=8,
                                  max_tokens=T, align_corners=ac, dense_layout=layout)
                torch.cuda.synchronize()
                pnt, desc, sc = tb.pnt.cpu(), tb.desc.cpu(), tb.score.cpu()
                for i in range(3):
                    n0, n1 = int(tb.cu_n[i]), int(tb.cu_n[i + 1])
                    assert n1 > n0, "every image must keep lines"
                    pts = pnt[n0:n1].reshape(-1, 2)
                    assert float(margin(pts, Hc, Wc, ac).min()) >= MARGIN
                    case = build_case("sample_desc(records)", "tokens", pts, torch.zeros(pts.shape[0], dtype=torch.long), dense[i:i + 1], ac)
                    rows += sample_errors(desc[n0:n1].reshape(-1, D), case, None, f"T {T} image {i} {layout}")
                    ix = torch.round(pts[:, 0]).long().clamp(0, W - 1)
                    iy = torch.round(pts[:, 1]).long().clamp(0, H - 1)
                    rows.append(("tokenize(score gather)", "tokens", label(case) + f", T {T} image {i} {layout}",
                                 float((sc[n0:n1].reshape(-1) != score[i][iy, ix]).sum()), 0.0))
    return rows


# =================================================================================================================================
# SuperPoint heads
# =================================================================================================================================

HEAD_MAPS = ((1, 1), (1, 31), (4, 8), (3, 11), (6, 6), (7, 9), (8, 8), (5, 13), (4, 17), (10, 10))    # HW = 1 31 32 33 36 63 64 65 68 100
HEAD_B = (1, 3)
HEAD_FAMILIES = ("normal", "onehot", "onehot65", "sentinel")
EXACT = ("onehot", "onehot65")
HEAD_FORMS = (("nchw", 0), ("rows", 0), ("rows", 3))                        # (form, pad columns behind every row)
HEAD_WANTS = (("score",), ("nhwc",), ("nchw",), ("score", "nhwc", "nchw"))
GAP = 64                                                                    # marker floats behind every output


def score_reference(logits, dtype):
    """[B, 8 Hc, 8 Wc]: softmax over the 65 channels, dustbin dropped, channel 8 dy + dx to pixel (8 h + dy, 8 w + dx)"""
    p = torch.softmax(logits.to(dtype), dim=1)[:, :64]
    B, _, Hc, Wc = p.shape
    return p.permute(0, 2, 3, 1).reshape(B, Hc, Wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, Hc * 8, Wc * 8)


def desc_reference(raw, dtype):
    return F.normalize(raw.to(dtype), p=2, dim=1)


def hot_channel(family, p):
    return (5 * p + 1) % 65 if family == "onehot" else (3 * p + 64) % 65


@functools.lru_cache(maxsize=None)
def head_case(family, hw_cells, B):
    """dict: logits [B, 65, Hc, Wc], raw [B, 256, Hc, Wc] float32; score64 / score32 [B, 8 Hc, 8 Wc], desc64 / desc32 [B, 256, Hc, Wc].
      normal    logits 3 N(0, 1); descriptors N(0, 1) x a per-cell scale in [0.01, 30]
      onehot    cell p (counted through the batch) holds +-2^k, k = p % 17 - 8, at channel (7 p + 3) % 256: the output is exactly +-1
                there and 0 elsewhere; its logits are 90 at channel (5 p + 1) % 65 and 0 elsewhere: exactly 1.0 at sub-pixel divmod(c, 8)
                of the cell and below 1e-30 elsewhere, the whole patch below 1e-30 where the hot channel is the dustbin
      onehot65  `onehot` with the hot logit at channel (3 p + 64) % 65 ((5 p + 1) % 65 reaches 13 channels and never the dustbin; this
                one reaches all 65, cell 0 the dustbin)
      sentinel  `normal` values; the launches put +-1e4 behind the inputs and markers behind the outputs"""
    if family not in HEAD_FAMILIES:
        raise ValueError(family)
    Hc, Wc = hw_cells
    HW = Hc * Wc
    g = _gen("heads", family, hw_cells, B)
    if family in EXACT:
        p = torch.arange(B * HW)
        raw = torch.zeros((B * HW, D))
        raw[p, (7 * p + 3) % D] = torch.where((p // 17) % 2 == 0, 1.0, -1.0) * torch.pow(2.0, (p % 17 - 8).float())
        logits = torch.zeros((B * HW, 65))
        logits[p, hot_channel(family, p)] = 90.0
        raw = raw.view(B, Hc, Wc, D).permute(0, 3, 1, 2).contiguous()
        logits = logits.view(B, Hc, Wc, 65).permute(0, 3, 1, 2).contiguous()
    else:
        logits = 3.0 * torch.randn((B, 65, Hc, Wc), generator=g)
        raw = torch.randn((B, D, Hc, Wc), generator=g) * (0.01 + 29.99 * torch.rand((B, 1, Hc, Wc), generator=g))
    return dict(family=family, B=B, Hc=Hc, Wc=Wc, logits=logits, raw=raw,
                score64=score_reference(logits, torch.float64), score32=score_reference(logits, torch.float32),
                desc64=desc_reference(raw, torch.float64), desc32=desc_reference(raw, torch.float32))


def head_cases():
    for family in HEAD_FAMILIES:
        for hw in HEAD_MAPS:
            for B in HEAD_B:
                yield head_case(family, hw, B)


def head_label(case):
    return f"{case['Hc']}x{case['Wc']}, B {case['B']}"


def head_inputs(case, form, pad, device):
    """(score input, descriptor input) on the device as the views a caller hands over.  nchw: one more image of +-1e4 behind the batch;
    rows: [B HW, C] views of [B HW + SPARE_ROWS, C + pad] buffers whose spare rows and pad columns hold +-1e4"""
    B, HW = case["B"], case["Hc"] * case["Wc"]
    views = []
    for t in (case["logits"], case["raw"]):
        C_ = int(t.shape[1])
        g = _gen("guard heads", form, pad, C_)
        if form == "nchw":
            views.append(torch.cat([t, _sentinel((1,) + tuple(t.shape[1:]), g)]).to(device)[:B])
        else:
            buf = _sentinel((B * HW + SPARE_ROWS, C_ + pad), g)
            buf[:B * HW, :C_] = t.permute(0, 2, 3, 1).reshape(B * HW, C_)
            views.append(buf.to(device)[:B * HW, :C_])
    return views


def run_heads(eng, case, form, pad, want):
    """the case through Engine.superpoint_heads / Engine.superpoint_heads_rows; returns {output name: CPU tensor} of `want`"""
    sl, dr = head_inputs(case, form, pad, eng.device)
    sl = sl if "score" in want else None
    dr = dr if ("nhwc" in want or "nchw" in want) else None
    kw = dict(nhwc="nhwc" in want, nchw="nchw" in want)
    if form == "nchw":
        out = eng.superpoint_heads(sl, dr, **kw)
    else:
        out = eng.superpoint_heads_rows(sl, dr, (case["B"], case["Hc"], case["Wc"]), **kw)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in zip(("score", "nhwc", "nchw"), out) if v is not None}
    assert set(got) == set(want), (set(got), want)
    return got


def run_heads_guarded(eng, case, form, pad, want):
    """the case through the C ABI with every output in one marker-filled allocation, GAP floats behind each; returns ({name: CPU
    tensor}, floats outside the requested outputs that no longer hold the marker)"""
    L, dev = eng._L, eng.device
    B, Hc, Wc = case["B"], case["Hc"], case["Wc"]
    HW = Hc * Wc
    sizes = {"score": B * 64 * HW, "nhwc": B * D * HW, "nchw": B * D * HW}
    shapes = {"score": (B, Hc * 8, Wc * 8), "nhwc": (B, Hc, Wc, D), "nchw": (B, D, Hc, Wc)}
    offs, o = {}, 0
    for k in ("score", "nhwc", "nchw"):
        offs[k] = o
        o += sizes[k] + GAP
    arena = torch.full((o,), MARKER, dtype=torch.float32, device=dev)
    sl, dr = head_inputs(case, form, pad, dev)
    p = lambda k: arena[offs[k]:].data_ptr() if k in want else None
    p_sl = sl.data_ptr() if "score" in want else None
    p_dr = dr.data_ptr() if ("nhwc" in want or "nchw" in want) else None
    with torch.cuda.device(dev):
        if form == "nchw":
            nat.check(L.linetr_superpoint_heads(eng._h, p_sl, p_dr, B, Hc, Wc, p("score"), p("nhwc"), p("nchw"), eng._stream()), L)
        else:
            nat.check(L.linetr_superpoint_heads_rows(eng._h, p_sl, sl.stride(0), p_dr, dr.stride(0), B, Hc, Wc, p("score"), p("nhwc"), p("nchw"),
                                                     eng._stream()), L)
    torch.cuda.synchronize()
    a = arena.cpu()
    keep = torch.ones(o, dtype=torch.bool)
    got = {}
    for k in want:
        keep[offs[k]:offs[k] + sizes[k]] = False
        got[k] = a[offs[k]:offs[k] + sizes[k]].view(shapes[k])
    return got, int((a[keep] != MARKER).sum())


def head_errors(got, case, where=""):
    """[(kernel, family, where, error, bar)] of the outputs in `got`.  normal / sentinel: against the references' bar; onehot: bit for
    bit (the descriptor outputs equal desc64; the score is exactly 1.0 where score64 is and below 1e-30 elsewhere)"""
    fam = case["family"]
    where = head_label(case) + (", " + where if where else "")
    rows = []
    for name, t in got.items():
        kernel = "sp_score_head" if name == "score" else "sp_desc_head"
        r64 = case["score64"] if name == "score" else (case["desc64"] if name == "nchw" else case["desc64"].permute(0, 2, 3, 1))
        r32 = case["score32"] if name == "score" else (case["desc32"] if name == "nchw" else case["desc32"].permute(0, 2, 3, 1))
        if fam not in EXACT:
            rows.append((kernel, fam, where + f" {name}", _max(t.double() - r64), bar_of(r64, r32)))
        elif name == "score":
            hot = r64 == 1.0
            rows.append((kernel, fam, where + " score", float((t[hot] != 1.0).sum() + (t[~hot] >= 1e-30).sum() + (t[~hot] < 0).sum()), 0.0))
        else:
            rows.append((kernel, fam, where + f" {name}", float((t.double() != r64).sum()), 0.0))
    if "nhwc" in got and "nchw" in got:
        rows.append(("sp_desc_head", fam + "/layouts", where, _max(got["nhwc"] - got["nchw"].permute(0, 2, 3, 1)), 0.0))
    return rows


def sweep_heads(eng):
    """every head case in every form and every combination of requested outputs: against the bar, NHWC against NCHW, the row forms
    against the NCHW form bit for bit; the `sentinel` family through the C ABI with markers behind and between the outputs"""
    rows = []
    for case in head_cases():
        base = {}
        for form, pad in HEAD_FORMS:
            for want in HEAD_WANTS:
                where = f"{form}+{pad} {'+'.join(want)}"
                if case["family"] == "sentinel":
                    got, touched = run_heads_guarded(eng, case, form, pad, want)
                    rows.append(("sp_heads", "sentinel/markers", head_label(case) + ", " + where, float(touched), 0.0))
                else:
                    got = run_heads(eng, case, form, pad, want)
                rows += head_errors(got, case, where)
                for k, t in got.items():
                    if form == "nchw":
                        base[(want, k)] = t
                    else:
                        rows.append(("sp_score_head" if k == "score" else "sp_desc_head", case["family"] + "/forms",
                                     head_label(case) + ", " + where + f" {k}", _max(t - base[(want, k)]), 0.0))
    return rows
