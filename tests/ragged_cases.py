"""Cases and bars of the ragged (mixed image size) pre-filter and describe tests: tests/test_prefilter_ragged_cpu.py,
tests/test_gpu_describe_ragged.py and tools/ragged_describe_report.py read them from here.

The batch: nine images of five sizes in a non-monotone order (large, small, large), three token distances, min_length per image.
  0  1024 x 1024  td 12.8  the reference's auto_min_length values of this shape (max(16, 1024 / 40), max(8, 1024 / 80))
  1    64 x   96  td  8    holds one diagonal of 12 tokens: THREE sub-lines at max_tokens = 5, in the smallest image
  2   480 x  640  td  8    the only image with a valid mask (its left 150 columns are invalid)
  3    72 x   88  td  8    9 x 11 descriptor cells: Hc * Wc is odd; equal lengths planted
  4   480 x  640  td  8    no line at all: an empty image in the middle of the batch
  5   488 x  648  td 16    61 x 81 cells, odd again, with the third token distance
  6    64 x   96  td  8    ONE line: max_keylines = -1 ([:-1]) drops it
  7  1024 x 1024  td 12.8  equal lengths planted
  8    72 x   88  td 16
max_tokens is 5, not the model's 21: only then does a line that fits a 64 x 96 image have three sub-lines.

Bars.  Tokeniser tensors: 0 differing elements wherever two native paths, or a native path and the oracle, compute the same float64 /
float32 expressions (angles against the oracle: 1.2e-7, libm's last float64 ulp of cos / sin after the float32 cast, the bound
tests/test_gpu_dropin.py documents for angles="native").  line_desc between two batch compositions: 5e-6 (other GEMM tiles for other
row counts, the bar tests/test_gpu_dropin.py sets between the fused pair and the per-image path).  line_desc against the oracle and
the reference's golden: 1e-4, the bar of every oracle comparison of the suite."""
import ctypes as C

import numpy as np

from linetr_amd import _native as nat
from workloads import synth

T = 5
BORDER = 8
DESC_BATCH_BAR = 5e-6
DESC_ORACLE_BAR = 1e-4
ANGLE_ORACLE_BAR = 1.2e-7
SAMPLED_DESC_ORACLE_BAR = 1e-6     # sampled token descriptors against torch's CPU grid_sample: the bar of the asset-pair test
TOK_FIELDS = ("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "score", "desc", "sub2line")

#         (height, width, token_distance, min_length, seed, lines)
IMAGES = [(1024, 1024, 12.8, 25.6, 9100, 40),
          (64, 96, 8.0, 16.0, 9101, 6),
          (480, 640, 8.0, 16.0, 9102, 30),
          (72, 88, 8.0, 16.0, 9103, 6),
          (480, 640, 8.0, 16.0, 9104, 0),
          (488, 648, 16.0, 20.0, 9105, 30),
          (64, 96, 8.0, 16.0, 9106, 1),
          (1024, 1024, 12.8, 25.6, 9107, 30),
          (72, 88, 16.0, 16.0, 9108, 4)]
TIED = {3: ((0, 2, 4), 19.0), 7: ((1, 5, 9, 20), 30.0)}       # image -> (rows given one equal length, the length)
MASKED = 2


MANY_LINES = {2: 600, 5: 600}       # line counts that take a three-image batch (2, 3, 5) above 2048 sub-lines


def image_lines(i, n=None):
    """the detector rows [K,6] of image i (n: another number of seeded lines than the table's)"""
    h, w, td, ml, seed = IMAGES[i][:5]
    n = IMAGES[i][5] if n is None else n
    small = max(h, w) < 200
    rows = synth.synth_lines(seed, n, h, w, len_lo=17.0, len_hi=40.0 if small else 167.0) if n else np.zeros((0, 6))
    if i == 1:      # the diagonal of the 64 x 96 image inside its border: 12 tokens of 8 px, three sub-lines of 5
        sx, sy, ex, ey = 8.5, 8.5, 86.5, 54.5
        rows = np.concatenate([rows, [[sx, sy, ex, ey, float(np.float32(np.hypot(ex - sx, ey - sy))), 0.0]]])
    if i in TIED:
        rows[list(TIED[i][0]), 4] = TIED[i][1]
    return rows


def valid_mask(i):
    if i != MASKED:
        return None
    vm = np.ones(IMAGES[i][:2])
    vm[:, :150] = 0
    return vm


def batch(ids=None, n_lines=None):
    """(lines per image, row offsets, the LinetrPrefilterImage table, the masks kept alive) of the images `ids` (default: all nine);
    n_lines: {image: another line count}"""
    ids = list(range(len(IMAGES))) if ids is None else list(ids)
    lines = [image_lines(i, (n_lines or {}).get(i)) for i in ids]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.int32)
    table = np.zeros(len(ids), dtype=nat.PREFILTER_IMAGE_DTYPE)
    masks = [valid_mask(i) for i in ids]
    for j, i in enumerate(ids):
        h, w, td, ml = IMAGES[i][:4]
        table[j] = (h, w, ml, td, masks[j].ctypes.data if masks[j] is not None else 0)
    return lines, off, table, masks


def prefilter_ragged(L, lines, off, table, max_keylines, n_threads, capacity=None, max_tokens=T, border=BORDER):
    """linetr_prefilter_ragged as it is: (status, recs, cu_k, cu_n)"""
    cat = np.ascontiguousarray(np.concatenate(lines) if len(lines) else np.zeros((0, 6)), dtype=np.float64)
    B = len(off) - 1
    cap = int(off[-1]) if capacity is None else capacity
    recs = np.zeros(max(cap, 1), dtype=nat.REC_DTYPE)
    cu_k, cu_n = np.full(B + 1, -7, np.int32), np.full(B + 1, -7, np.int32)
    code = L.linetr_prefilter_ragged(nat.np_ptr(cat), nat.np_ptr(off), B, nat.np_ptr(table) if table is not None else None, border,
                                     max_keylines, max_tokens, n_threads, nat.np_ptr(recs), cap, nat.np_ptr(cu_k), nat.np_ptr(cu_n))
    return code, recs, cu_k, cu_n


def prefilter_one(L, rows, entry, max_keylines, image, sub_base, tok_base, max_tokens=T, border=BORDER):
    """linetr_prefilter of one image with the settings of its table entry"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    recs = np.zeros(max(len(rows), 1), dtype=nat.REC_DTYPE)
    k, n = C.c_int32(), C.c_int32()
    nat.check(L.linetr_prefilter(nat.np_ptr(rows), len(rows), int(entry["height"]), int(entry["width"]), border, float(entry["min_length"]),
                                 max_keylines, C.c_void_p(int(entry["valid_mask"]) or None), float(entry["token_distance"]), max_tokens,
                                 image, sub_base, tok_base, nat.np_ptr(recs), len(recs), C.byref(k), C.byref(n)), L)
    return recs[:k.value], n.value


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU side: maps between NaN guards, outputs between guards of one bit pattern, linetr_describe_ragged called as it is
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 64                      # floats on either side (a multiple of 4: the guarded views stay 16-byte aligned)
PATTERN = 0x5A5AC3C3            # what every output word holds before the call


def guarded(a, device):
    """(the whole allocation, the view of `a` inside it): NaN on either side, so a read beyond the map shows up in the results"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    whole = torch.full((a.size + 2 * GUARD,), float("nan"), device=device)
    view = whole[GUARD:GUARD + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    return whole, view.view(a.shape)


def image_maps(i, nhwc, device):
    """the seeded maps of image i, each in an allocation of its own between NaN guards: (descriptor map, score map, what keeps them alive)"""
    h, w = IMAGES[i][:2]
    dd, ds = synth.synth_dense_maps_np(IMAGES[i][4], h, w)
    dd = dd[0].transpose(1, 2, 0) if nhwc else dd[0]
    keep_d, dd_v = guarded(dd, device)
    keep_s, ds_v = guarded(ds[0], device)
    return dd_v, ds_v, (keep_d, keep_s)


class Outputs:
    """Every output of a describe call as views of ONE int32 allocation filled with PATTERN, GUARD words between neighbours."""

    def __init__(self, K, N, Tm, mat_floats, device):
        import torch
        shapes = [("ld", (N, 256)), ("klines", (K, 2, 2)), ("length", (K,)), ("angles", (K, 2)), ("sublines", (N, 2, 2)), ("pnt", (N, Tm, 2)),
                  ("mask", (N, Tm + 1)), ("resp", (N,)), ("angle_sub", (N, 2)), ("score", (N, Tm)), ("desc", (N, Tm, 256)), ("sub2line", (N,)),
                  ("mat", (mat_floats,))]
        sizes = [(int(np.prod(sh)) + 3) // 4 * 4 for _, sh in shapes]
        self.whole = torch.full((sum(sizes) + GUARD * (len(shapes) + 1),), PATTERN, dtype=torch.int32, device=device)
        self.views, self.spans, o = {}, [], GUARD
        for (name, sh), sz in zip(shapes, sizes):
            n = int(np.prod(sh))
            v = self.whole[o:o + n]
            self.views[name] = (v if name == "sub2line" else v.view(torch.float32)).view(sh)
            self.spans.append((o, o + n))
            o += sz + GUARD

    def guards_intact(self):
        import torch
        inside = torch.zeros(self.whole.numel(), dtype=torch.bool, device=self.whole.device)
        for a, b in self.spans:
            inside[a:b] = True
        return bool((self.whole[~inside] == PATTERN).all())

    def untouched(self):
        return bool((self.whole == PATTERN).all())

    def tokens(self, want_mat, cu_k32):
        t = nat.Tokens()
        for k in ("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "desc", "score"):
            setattr(t, k, self.views[k].data_ptr())
        if want_mat:
            t.mat = self.views["mat"].data_ptr()
            t.h_cu_klines = cu_k32.ctypes.data
        return t


def image_table(maps, tds):
    table = np.zeros(len(maps), dtype=nat.IMAGE_DTYPE)
    for j, ((dd, ds, _keep), td) in enumerate(zip(maps, tds)):
        table[j] = (dd.data_ptr(), ds.data_ptr(), ds.shape[0], ds.shape[1], td)
    return table


def describe_ragged(eng, recs, cu_k, cu_n, table, nhwc, align_corners, want_mat, Tm=T, ws_short=0, ws_offset=0, with_h_recs=True,
                    tokens_edit=None, n_images=None):
    """linetr_describe_ragged as it is, outputs between guards: (status, Outputs).  ws_short: bytes taken off the workspace size;
    ws_offset: bytes the workspace pointer is moved by; tokens_edit(tokens): a last change to the LinetrTokens struct; table None: a
    NULL table; n_images: another image count than the prefix sums'."""
    import torch
    L, dev = eng._L, eng.device
    B, K, N = len(cu_k) - 1, int(cu_k[-1]), int(cu_n[-1])
    cu_k32, cu_n32 = np.ascontiguousarray(cu_k, np.int32), np.ascontiguousarray(cu_n, np.int32)
    mat_floats = int((np.diff(cu_k32).astype(np.int64) * np.diff(cu_n32)).sum()) if want_mat else 0
    out = Outputs(K, N, Tm, mat_floats, dev)
    recs = np.ascontiguousarray(recs[:K])
    n_real = int(recs["n_tok"].sum())
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    p_table = nat.np_ptr(table) if table is not None else None
    n_img = B if n_images is None else n_images
    nbytes = L.linetr_describe_ragged_workspace_bytes(eng._h, p_table, n_img, int(nhwc), N, n_real)
    ws = torch.empty(max(nbytes, 0) + 256, dtype=torch.uint8, device=dev)
    tok = out.tokens(want_mat, cu_k32)
    if tokens_edit:
        tokens_edit(tok)
    with torch.cuda.device(dev):
        code = L.linetr_describe_ragged(eng._h, d_recs.data_ptr(), nat.np_ptr(recs) if with_h_recs else None, K, N, n_real,
                                        nat.np_ptr(cu_n32), None, p_table, n_img, Tm, int(align_corners), int(nhwc), tok,
                                        out.views["sub2line"].data_ptr(), out.views["ld"].data_ptr(), ws.data_ptr() + ws_offset,
                                        max(nbytes, 0) - ws_short, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
    return code, out, nbytes


class FakeSuperPoint:
    """seeded dense maps of the image's own size + a few unit point descriptors (what tests/test_gpu_dropin.py feeds Matching)"""
    config = {"nn_threshold": 0.7}

    def __init__(self, seeds):
        self.seeds = list(seeds)

    def __call__(self, data):
        import torch
        seed = self.seeds.pop(0)
        dd, ds = synth.synth_dense_maps(seed, *data["image"].shape[-2:])
        rs = np.random.RandomState(seed)
        n = 50 + seed % 7
        desc = torch.nn.functional.normalize(torch.from_numpy(rs.standard_normal((256, n)).astype(np.float32)), dim=0)
        kp = torch.from_numpy(rs.uniform(8, 400, (n, 2)).astype(np.float32))
        dev = data["image"].device
        return {"keypoints": [kp.to(dev)], "scores": [torch.rand(n).to(dev)], "descriptors": [desc.to(dev)],
                "dense_descriptor": dd.to(dev), "dense_score": ds.to(dev)}


class FakeLSD:
    def __init__(self, line_sets):
        self.sets = list(line_sets)

    def detect_torch(self, image):
        return synth.array_to_keylines(self.sets.pop(0))
