"""Host-side driver of the native library: owns the handle, device workspaces and the var-len batch
plumbing.  PyTorch is used for device memory, streams and H2D/D2H copies only; every arithmetic step
of the hot path is a HIP kernel behind the C ABI (include/linetr_hip.h).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as nat

D = 256

DEFAULT_MODEL = dict(descriptor_dim=256, keyline_encoder=[32, 64, 128, 256], n_heads=4,
                     n_line_descriptive_layers=1, d_inner=1024, n_sig_layers=7, image_shape=[480, 640], bn_batch_stats=False)


def _as_numpy_f32(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


@dataclass
class TokenBatch:
    """Device tensors produced by the tokeniser for a batch of images (images concatenated)."""
    n_images: int
    max_tokens: int
    cu_k: np.ndarray          # [B+1] host prefix sums of key-lines
    cu_n: np.ndarray          # [B+1] host prefix sums of sub-lines
    recs: np.ndarray          # host LineRec array [K]
    klines: torch.Tensor      # [K,2,2]
    length: torch.Tensor      # [K]
    angles: torch.Tensor      # [K,2]
    sublines: torch.Tensor    # [N,2,2]
    pnt: torch.Tensor         # [N,T,2]
    mask: torch.Tensor        # [N,T+1]
    resp: torch.Tensor        # [N]
    angle_sub: torch.Tensor   # [N,2]
    desc: torch.Tensor        # [N,T,256]
    score: torch.Tensor       # [N,T]
    sub2line: torch.Tensor    # [N] int32, key-line index inside the image
    mat: torch.Tensor = None  # mat_klines2sublines with want_mat=True: [K,N] for one image, the flat per-image blocks for a batch (mat_of)
    extra: dict = field(default_factory=dict)

    @property
    def K(self):
        return int(self.cu_k[-1])

    @property
    def N(self):
        return int(self.cu_n[-1])

    def mat_of(self, i: int) -> torch.Tensor:
        """mat_klines2sublines [K_i,N_i] of image i (describe(..., want_mat=True))."""
        k = np.diff(self.cu_k).astype(np.int64)
        n = np.diff(self.cu_n).astype(np.int64)
        off = int((k[:i] * n[:i]).sum())
        return self.mat.reshape(-1)[off:off + int(k[i] * n[i])].view(int(k[i]), int(n[i]))

    def c_tokens(self) -> nat.Tokens:
        t = nat.Tokens()
        for k in ("klines", "length", "angles", "sublines", "pnt", "mask", "resp", "angle_sub", "desc", "score"):
            setattr(t, k, getattr(self, k).data_ptr())
        t.mat = self.mat.data_ptr() if self.mat is not None else None
        return t


def repack_like_numpy(L, recs, cu_k, cu_n, i, rows, height, width, border, min_length, max_keylines, token_distance,
                      max_tokens, valid_mask=None):
    """Image i of a pre-filtered batch holds equal lengths: redo a1-a3 the way the per-image path does (NumPy's own argsort,
    models/line_process.py:6-21) and overwrite the image's records in place.  Equal lengths mean equal token counts, so the
    number of key-lines / sub-lines / tokens of the image -- and every later image's offsets -- stay as they are."""
    from . import line_process as lp
    vm = np.asarray(valid_mask, dtype=np.float64) if valid_mask is not None else None
    kl = lp.filter_by_length(lp.remove_borders(lp.lines_from_rows(rows.copy()), border, height, width, vm), min_length,
                             max_keylines)
    k0, k1 = int(cu_k[i]), int(cu_k[i + 1])
    if len(kl["klines"]) != k1 - k0:
        raise RuntimeError(f"pre-filter: NumPy keeps {len(kl['klines'])} lines of image {i}, the native pass {k1 - k0}")
    if k1 == k0:
        return
    n_out = C.c_int32()
    tok = int(recs["first_tok"][k0])
    n_tok = int(recs["n_tok"][k0:k1].sum())
    a, b, c = (np.ascontiguousarray(kl[k], dtype=np.float64) for k in ("klines", "length_klines", "angles"))
    nat.check(L.linetr_pack_lines(nat.np_ptr(a), nat.np_ptr(b), nat.np_ptr(c), k1 - k0, float(token_distance), int(max_tokens), i,
                                  int(cu_n[i]), tok, nat.np_ptr(recs[k0:k1]), C.byref(n_out)), L)
    if n_out.value != int(cu_n[i + 1] - cu_n[i]) or int(recs["n_tok"][k0:k1].sum()) != n_tok:
        raise RuntimeError(f"pre-filter: re-ordering image {i} changed its sub-line / token count")


class Engine:
    """One native model instance on one GPU."""

    def __init__(self, state_dict, device="cuda:0", lib_path=None, **model_cfg):
        """lib_path: another build of the library (nat.EXPERIMENTS_LIB_PATH for tools / experiment tests)."""
        cfg = {**DEFAULT_MODEL, **model_cfg}
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("linetr_amd.Engine needs a HIP device (torch device 'cuda:N'); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.cfg = cfg
        L = nat.lib(lib_path)
        mc = nat.ModelConfig()
        mc.d_model, mc.n_heads, mc.d_inner = cfg["descriptor_dim"], cfg["n_heads"], cfg["d_inner"]
        mc.n_sig_layers, mc.n_desc_layers = cfg["n_sig_layers"], cfg["n_line_descriptive_layers"]
        for i, c in enumerate(cfg["keyline_encoder"]):
            mc.enc_channels[i] = c
        shape = cfg["image_shape"]
        mc.norm_height, mc.norm_width = int(shape[-2]), int(shape[-1])
        mc.bn_batch_stats = int(bool(cfg["bn_batch_stats"]))     # a training-mode handle: forward_train_tensors only
        names, arrs = [], []
        for k, v in state_dict.items():
            if k.endswith("num_batches_tracked"):
                continue
            names.append(k.encode())
            arrs.append(_as_numpy_f32(v))
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        c_numel = (C.c_int64 * n)(*[a.size for a in arrs])
        h = C.c_void_p()
        nat.check(L.linetr_create(C.byref(mc), n, c_names, c_ptrs, c_numel, self.device.index, C.byref(h)))
        self._h = h
        self._L = L
        self._ws = {}

    @classmethod
    def heads_only(cls, device="cuda:0"):
        """An Engine without a LineTR model: only the weight-free entry points work (superpoint_heads, superpoint_keypoints,
        match_points, match_distmat).  Used by FusedHeadSuperPoint when no LineTransformer engine is at hand."""
        self = cls.__new__(cls)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("linetr_amd.Engine needs a HIP device (torch device 'cuda:N'); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.cfg = dict(DEFAULT_MODEL)
        self._L = nat.lib()
        self._h = None
        self._ws = {}
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._L.linetr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, tag: str, nbytes: int) -> torch.Tensor:
        ws = self._ws.get(tag)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=self.device)
            self._ws[tag] = ws
        return ws

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        return t

    # ------------------------------------------------------------------ host pre-filter
    def _pinned_slot(self, nbytes):
        """ring of pinned staging buffers; a slot is reused only after its last H2D copy has completed."""
        ring = self.__dict__.setdefault("_ring", {"i": 0, "slots": [None] * 12})
        ring["i"] = (ring["i"] + 1) % len(ring["slots"])
        slot = ring["slots"][ring["i"]]
        if slot is None or slot["buf"].numel() < nbytes:
            slot = {"buf": torch.empty(int(nbytes * 1.5) + 4096, dtype=torch.uint8, pin_memory=True), "event": None}
            ring["slots"][ring["i"]] = slot
        if slot["event"] is not None:
            slot["event"].synchronize()
            slot["event"] = None
        return slot

    def _record_blob(self, n_recs, B):
        """A pinned staging slot laid out  records | cu_k [B+1] | cu_n [B+1]  -- what _upload_recs() sends with ONE asynchronous copy.
        Returns the three NumPy views and remembers the slot as the origin of `recs`."""
        rec_bytes = max(n_recs, 1) * nat.REC_DTYPE.itemsize
        slot = self._pinned_slot(rec_bytes + 8 * (B + 1) + 64)
        host = slot["buf"].numpy()
        recs = host[:rec_bytes].view(nat.REC_DTYPE)
        cu_k = host[rec_bytes:rec_bytes + 4 * (B + 1)].view(np.int32)
        cu_n = host[rec_bytes + 4 * (B + 1):rec_bytes + 8 * (B + 1)].view(np.int32)
        self._last_host = {"slot": slot, "recs_ptr": recs.ctypes.data, "rec_bytes": rec_bytes, "B": B}
        return recs, cu_k, cu_n

    def prefilter(self, lines6, height, width, *, remove_borders, min_length, max_keylines, token_distance,
                  max_tokens, valid_masks=None, offsets=None, n_threads=0, tie_order="numpy"):
        """a1-a3 for a batch.  `lines6` is a list of [K_i,6] float64 arrays, or one concatenated [sum K,6] array
        with `offsets` [B+1].  Returns (recs, cu_k, cu_n); recs lives in pinned memory ready for an async H2D.

        tie_order: the length sort of models/line_process.py:15-16 is np.argsort, whose order among EQUAL lengths is NumPy's
        business (unstable, CPU-dispatched).  "numpy" (default): the images the native pre-filter reports as holding equal
        lengths (linetr_prefilter_tied_images; rare with a real detector) are re-ordered with NumPy itself and re-packed, so the
        batched path gives the reference's rows on this machine, like the per-image path does.  "stable": keep the native order
        (stable ascending argsort, reversed) -- machine-independent."""
        if tie_order not in ("numpy", "stable"):
            raise ValueError("tie_order must be 'numpy' or 'stable'")
        if offsets is None:
            lens = [len(l) for l in lines6]
            offsets = np.zeros(len(lens) + 1, dtype=np.int32)
            np.cumsum(lens, out=offsets[1:])
            cat = (np.concatenate([np.asarray(l, dtype=np.float64).reshape(-1, 6) for l in lines6])
                   if len(lens) else np.zeros((0, 6)))
        else:
            cat = lines6
            offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        cat = np.ascontiguousarray(cat, dtype=np.float64)
        B = len(offsets) - 1
        cap = int(offsets[-1])
        recs, cu_k, cu_n = self._record_blob(cap, B)
        vm_ptrs = None
        keep = []
        if valid_masks is not None:
            arr = (C.c_void_p * B)()
            for i, vm in enumerate(valid_masks):
                if vm is not None:
                    if np.ndim(vm) != 2 or np.shape(vm) != (int(height), int(width)):
                        # prefilter_core reads vm[y * width + x]: any other shape would be read out of bounds or mis-addressed
                        raise ValueError(f"valid mask {i} has shape {np.shape(vm)}, the native pre-filter needs ({int(height)}, "
                                         f"{int(width)}) (other shapes: the NumPy remove_borders of linetr_amd.line_process)")
                    vm = np.ascontiguousarray(vm, dtype=np.float64)
                    keep.append(vm)
                    arr[i] = vm.ctypes.data
            vm_ptrs = arr
        nat.check(self._L.linetr_prefilter_batch(nat.np_ptr(cat), nat.np_ptr(offsets), B, int(height), int(width),
                                                 int(remove_borders), float(min_length), int(max_keylines), vm_ptrs,
                                                 float(token_distance), int(max_tokens), int(n_threads),
                                                 nat.np_ptr(recs), cap, nat.np_ptr(cu_k), nat.np_ptr(cu_n)), self._L)
        if tie_order == "numpy":
            tied = np.empty(max(B, 1), dtype=np.int32)
            n_tied = self._L.linetr_prefilter_tied_images(nat.np_ptr(tied), B)
            for i in tied[:n_tied].tolist():
                repack_like_numpy(self._L, recs, cu_k, cu_n, i, cat[offsets[i]:offsets[i + 1]], int(height), int(width),
                                  remove_borders, min_length, max_keylines, token_distance, max_tokens,
                                  valid_masks[i] if valid_masks is not None else None)
        return recs[:int(cu_k[-1])], cu_k.copy(), cu_n.copy()

    def pack(self, klines, length, angles, token_distance, max_tokens, image=0, sub_base=0):
        """records for already-filtered lines (float64 arrays, reference layout).  They are written into a pinned staging
        slot together with the two prefix sums, so that tokenize() uploads them with ONE asynchronous copy."""
        K = len(klines)
        recs, cu_k, cu_n = self._record_blob(K, 1)
        n_out = C.c_int32()
        kl = np.ascontiguousarray(klines, dtype=np.float64)
        ln = np.ascontiguousarray(length, dtype=np.float64)
        an = np.ascontiguousarray(angles, dtype=np.float64)
        nat.check(self._L.linetr_pack_lines(nat.np_ptr(kl), nat.np_ptr(ln), nat.np_ptr(an), K, float(token_distance),
                                            int(max_tokens), int(image), int(sub_base), 0, nat.np_ptr(recs), C.byref(n_out)), self._L)
        cu_k[:] = (0, K)
        cu_n[:] = (0, n_out.value)
        return recs[:K], n_out.value

    def pack_many(self, lines, token_distance, max_tokens):
        """pack() for several images of one batch (each entry: {'klines', 'length_klines', 'angles'} float64, already filtered and
        ordered): one pinned blob  records | cu_k | cu_n, laid out like prefilter()'s, so describe() uploads it with one async copy."""
        B = len(lines)
        ks = [len(l["klines"]) for l in lines]
        K = int(sum(ks))
        recs, cu_k, cu_n = self._record_blob(K, B)
        cu_k[0] = cu_n[0] = 0
        tok = 0
        n_out = C.c_int32()
        for i, l in enumerate(lines):
            k0 = int(cu_k[i])
            kl = np.ascontiguousarray(l["klines"], dtype=np.float64)
            ln = np.ascontiguousarray(l["length_klines"], dtype=np.float64)
            an = np.ascontiguousarray(l["angles"], dtype=np.float64)
            nat.check(self._L.linetr_pack_lines(nat.np_ptr(kl), nat.np_ptr(ln), nat.np_ptr(an), ks[i], float(token_distance),
                                                int(max_tokens), i, int(cu_n[i]), tok, nat.np_ptr(recs[k0:k0 + max(ks[i], 1)]),
                                                C.byref(n_out)), self._L)
            cu_k[i + 1] = k0 + ks[i]
            cu_n[i + 1] = cu_n[i] + n_out.value
            tok += int(recs["n_tok"][k0:k0 + ks[i]].sum())
        return recs[:K], cu_k.copy(), cu_n.copy()

    # ------------------------------------------------------------------ device stages
    def _dense_maps(self, dense_desc, dense_score, B, dense_layout):
        """The dense maps of a B-image call as float32 device tensors with a batch axis, checked against each other: dense_score
        [B,H,W] and dense_desc [B,256,H/8,W/8] ('nchw') or [B,H/8,W/8,256] ('nhwc').  Returns (dense_desc, dense_score, H, W, nhwc)."""
        dense_desc = self._f32(dense_desc)
        dense_score = self._f32(dense_score)
        if dense_score.dim() == 2:
            dense_score = dense_score[None]
        if dense_desc.dim() == 3:
            dense_desc = dense_desc[None]
        if dense_desc.shape[0] != B or dense_score.shape[0] != B:
            raise ValueError("dense maps must have one entry per image")
        H, W = int(dense_score.shape[-2]), int(dense_score.shape[-1])
        nhwc = dense_layout == "nhwc"
        want = (B, H // 8, W // 8, D) if nhwc else (B, D, H // 8, W // 8)
        if tuple(dense_desc.shape) != want:
            raise ValueError(f"dense_descriptor shape {tuple(dense_desc.shape)} does not match {want} ({dense_layout})")
        return dense_desc, dense_score, H, W, nhwc

    def _pooled(self, shapes):
        """Named float32 device tensors as views of ONE allocation, each on a 16-byte boundary (a dozen torch.empty calls are ~40 us of
        host time on the latency path of a single pair); 'sub2line' is viewed as int32.  Returns (views, the allocation)."""
        sizes = [(math.prod(sh) + 3) // 4 * 4 for _, sh in shapes]
        pool = torch.empty((sum(sizes),), dtype=torch.float32, device=self.device)
        views, o = {}, 0
        for (name, sh), sz in zip(shapes, sizes):
            views[name] = pool[o:o + math.prod(sh)].view(sh)
            o += sz
        views["sub2line"] = views["sub2line"].view(torch.int32)
        return views, pool

    def tokenize(self, recs, cu_k, cu_n, dense_desc, dense_score, *, token_distance, max_tokens, align_corners=False,
                 sample_desc=True, dense_layout="nchw", want_mat=False, clip_shape=None) -> TokenBatch:
        """line_tokenizer on the device.  dense_desc [B,256,H/8,W/8] (dense_layout='nchw') or [B,H/8,W/8,256]
        ('nhwc', the producer's layout: no transposition pass), dense_score [B,H,W].  clip_shape: the (height, width) the
        reference's `image_shape` argument carries when it is not the maps' shape (it only sets the end-point clip)."""
        B = len(cu_k) - 1
        K, N, T = int(cu_k[-1]), int(cu_n[-1]), int(max_tokens)
        dense_desc, dense_score, H, W, nhwc = self._dense_maps(dense_desc, dense_score, B, dense_layout)
        f = dict(dtype=torch.float32, device=self.device)
        if want_mat and B != 1:
            raise ValueError("want_mat needs a single-image call (the reference's matrix is per image)")
        # the small token tensors are views of ONE allocation
        shapes = [("klines", (K, 2, 2)), ("length", (K,)), ("angles", (K, 2)), ("sublines", (N, 2, 2)), ("pnt", (N, T, 2)),
                  ("mask", (N, T + 1)), ("resp", (N,)), ("angle_sub", (N, 2)), ("score", (N, T)), ("sub2line", (N,))]
        if want_mat:
            shapes.append(("mat", (K, N)))                  # written by extra blocks of the tokeniser's own launch
        views, pool = self._pooled(shapes)
        tb = TokenBatch(n_images=B, max_tokens=T, cu_k=np.asarray(cu_k, np.int32), cu_n=np.asarray(cu_n, np.int32), recs=recs,
                        desc=torch.empty((N, T, D), **f) if sample_desc else torch.empty((0,), **f), **views)
        if K == 0 or N == 0:
            return tb
        d_recs, _ = self._upload_recs(recs, K, B, tb)
        nbytes = self._L.linetr_tokenize_workspace_bytes(B, H, W, N)
        ws = self._workspace("tok", nbytes)
        ct = tb.c_tokens()
        if not sample_desc:
            ct.desc = None
        with torch.cuda.device(self.device):     # a weight-less engine has no handle: the current device is used
            nat.check(self._L.linetr_tokenize(self._h, d_recs.data_ptr(), K, N, float(token_distance), T,
                                              dense_desc.data_ptr(), dense_score.data_ptr(), B, H, W,
                                              int(clip_shape[0]) if clip_shape is not None else 0,
                                              int(clip_shape[1]) if clip_shape is not None else 0, int(bool(align_corners)),
                                              int(nhwc), ct, tb.sub2line.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return tb

    def describe(self, recs, cu_k, cu_n, dense_desc, dense_score, *, token_distance, max_tokens, align_corners=False,
                 want_tokens=False, dense_layout="nchw", want_mat=False, pipeline_slot=None):
        """Fused tokenise + descriptor network for a batch (linetr_describe): real tokens only, descriptors sampled
        on the fly.  Returns (TokenBatch, line_desc [N,256]).  With want_tokens=False the dense [N,T,...] token
        tensors (pnt / mask / score / desc) are not materialised (zero-sized in the TokenBatch).

        pipeline_slot = (slot, n_slots): linetr_describe_submit -- the batch runs on the library's stage streams, overlapped with the
        batches submitted to the other slots, and is NOT joined: the returned tensors may be read only after describe_join(slot)
        (class DescribePipeline does the bookkeeping)."""
        B = len(cu_k) - 1
        K, N, T = int(cu_k[-1]), int(cu_n[-1]), int(max_tokens)
        dense_desc, dense_score, H, W, nhwc = self._dense_maps(dense_desc, dense_score, B, dense_layout)
        f = dict(dtype=torch.float32, device=self.device)
        # the small outputs and line_desc are views of ONE allocation
        shapes = [("ld", (N, D)), ("klines", (K, 2, 2)), ("length", (K,)), ("angles", (K, 2)), ("sublines", (N, 2, 2)),
                  ("resp", (N,)), ("angle_sub", (N, 2)), ("sub2line", (N,))]
        if want_tokens:
            shapes += [("pnt", (N, T, 2)), ("mask", (N, T + 1)), ("score", (N, T))]
        if want_mat:     # the per-image [K_i,N_i] blocks back to back, written by extra blocks of the tokeniser's launch (<= 8 images)
            shapes.append(("mat", (int((np.diff(np.asarray(cu_k, np.int64)) * np.diff(np.asarray(cu_n, np.int64))).sum()),)))
        views, pool = self._pooled(shapes)
        ld = views.pop("ld")
        z = pool[:0]
        for name in ("pnt", "mask", "score"):
            views.setdefault(name, z)
        tb = TokenBatch(n_images=B, max_tokens=T, cu_k=np.asarray(cu_k, np.int32), cu_n=np.asarray(cu_n, np.int32), recs=recs,
                        desc=torch.empty((N, T, D), **f) if want_tokens else z, **views)
        if K == 0 or N == 0:
            return tb, ld
        n_real = int(recs["n_tok"][:K].sum())
        d_recs, d_cu = self._upload_recs(recs, K, B, tb)
        ct = tb.c_tokens()
        if not want_tokens:
            ct.pnt = ct.mask = ct.desc = ct.score = None
        cu_k32 = np.ascontiguousarray(cu_k, dtype=np.int32)
        if want_mat:
            ct.h_cu_klines = cu_k32.ctypes.data
            if B == 1:
                tb.mat = tb.mat.view(K, N)
        nbytes = self._L.linetr_describe_workspace_bytes(self._h, B, H, W, N, n_real)
        cu = np.ascontiguousarray(cu_n, dtype=np.int32)
        args = (self._h, d_recs.data_ptr(), K, N, n_real, nat.np_ptr(cu), d_cu.data_ptr() if d_cu is not None else None, B,
                float(token_distance), T, dense_desc.data_ptr(), dense_score.data_ptr(), H, W, int(bool(align_corners)), int(nhwc), ct,
                tb.sub2line.data_ptr(), ld.data_ptr())
        if pipeline_slot is None:
            ws = self._workspace("desc", nbytes)
            nat.check(self._L.linetr_describe(*args, ws.data_ptr(), ws.numel(), self._stream()), self._L)
        else:
            slot, n_slots = (int(v) for v in pipeline_slot)
            tag = f"desc_pipe{slot}"
            old = self._ws.get(tag)
            if old is not None and old.numel() < nbytes:
                # the slot's workspace has to grow: its previous batch may still be running on the library's streams, which the caching
                # allocator knows nothing about -- let the device drain before the old block goes back to the pool (rare: sizes settle)
                torch.cuda.synchronize(self.device)
            ws = self._workspace(tag, nbytes)      # one workspace per slot: n_slots batches are in flight
            tb.extra["dense"] = (dense_desc, dense_score)          # read by the stage streams after this call returns
            nat.check(self._L.linetr_describe_submit(*args, ws.data_ptr(), ws.numel(), slot, n_slots, self._stream()), self._L)
        return tb, ld

    def describe_join(self, slot: int):
        """The current stream waits for the batch last submitted to `slot` (linetr_describe_join)."""
        nat.check(self._L.linetr_describe_join(self._h, int(slot), self._stream()), self._L)

    def describe_lines(self, lines6, offsets, dense_desc, dense_score, *, remove_borders, min_length, max_keylines,
                       token_distance, max_tokens, align_corners=False, want_tokens=False,
                       dense_layout="nchw", angles="native", pipeline_slot=None):
        """prefilter + describe for a batch given as one [sum K,6] array + row offsets [B+1].

        angles: "native" -- (cos 2theta, sin 2theta) from the host pre-filter's libm (the throughput path: nothing of the step runs in
        Python); "numpy" -- recomputed with NumPy from the filtered lines in one vectorised call, exactly what get_angles of the
        per-image surface computes (models/line_process.py:28-41): the two can differ in the last float64 ulp (<= 1.2e-7 after the
        float32 cast), and the batched drop-in surface (Matching.forward_batch) asks for NumPy's so that it returns forward()'s tensors.

        pipeline_slot = (slot, n_slots): see describe() / DescribePipeline.
        Returns (TokenBatch, line_desc [N,256]) for the whole batch."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        B = len(offsets) - 1
        H, W = int(dense_score.shape[-2]), int(dense_score.shape[-1])
        kw = dict(remove_borders=remove_borders, min_length=min_length, max_keylines=max_keylines,
                  token_distance=token_distance, max_tokens=max_tokens)
        if angles not in ("native", "numpy"):
            raise ValueError("angles must be 'native' or 'numpy'")
        recs, cu_k, cu_n = self.prefilter(lines6, H, W, offsets=offsets, **kw)
        if angles == "numpy" and len(recs):
            from .line_process import get_angles
            recs["angle"] = get_angles(np.stack([recs["sp"], recs["ep"]], axis=1))     # (records live in the pinned upload slot)
        return self.describe(recs, cu_k, cu_n, dense_desc, dense_score, token_distance=token_distance,
                             max_tokens=max_tokens, align_corners=align_corners, want_tokens=want_tokens,
                             dense_layout=dense_layout, pipeline_slot=pipeline_slot)

    def _upload_recs(self, recs, K, B, tb):
        """H2D of the line records (+ the sub-line prefix sums when they sit in the same pinned blob: ONE asynchronous copy, no host /
        device synchronisation).  The device copies are kept in tb.extra until the TokenBatch goes: the stream reads them later."""
        dev = self.device
        last = getattr(self, "_last_host", None)
        if last is not None and K > 0 and recs.ctypes.data == last["recs_ptr"] and last["B"] == B:
            nb = last["rec_bytes"] + 8 * (B + 1)
            d_blob = torch.empty(nb, dtype=torch.uint8, device=dev)
            d_blob.copy_(last["slot"]["buf"][:nb], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            last["slot"]["event"] = ev
            d_cu = d_blob[last["rec_bytes"] + 4 * (B + 1):].view(torch.int32)
            tb.extra["d_recs"], tb.extra["d_cu_n"] = d_blob, d_cu
            tb.extra["d_cu_k"] = d_blob[last["rec_bytes"]:last["rec_bytes"] + 4 * (B + 1)].view(torch.int32)
            return d_blob, d_cu
        d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
        tb.extra["d_recs"] = d_recs
        return d_recs, None

    def _dense_tokens(self, sublines, pnt, resp, angle_sub, desc, score, cu_n):
        """The reference's dense [N,T] token tensors as the native Tokens struct.  Returns (N, T, struct, cu_n as int32, the float32
        device tensors the struct points to -- to be kept alive over the call)."""
        N, T = int(pnt.shape[0]), int(pnt.shape[1])
        t = nat.Tokens()
        keep = [self._f32(x) for x in (sublines, pnt, resp, angle_sub, desc, score)]
        t.sublines, t.pnt, t.resp, t.angle_sub, t.desc, t.score = [x.data_ptr() for x in keep]
        cu = np.ascontiguousarray(cu_n, dtype=np.int32)
        if int(cu[-1]) != N:
            raise ValueError("cu_n does not match the number of sub-lines")
        return N, T, t, cu, keep

    def forward_tensors(self, sublines, pnt, resp, angle_sub, desc, score, cu_n, out=None, d_cu_n=None) -> torch.Tensor:
        """LineTransformer.forward on flat tensors; returns line_desc [N,256] (row-major)."""
        N, T, t, cu, _keep = self._dense_tokens(sublines, pnt, resp, angle_sub, desc, score, cu_n)
        if out is None:
            out = torch.empty((N, D), dtype=torch.float32, device=self.device)
        if N == 0:
            return out
        nbytes = self._L.linetr_forward_workspace_bytes(self._h, N, T)
        ws = self._workspace("fwd", nbytes)
        nat.check(self._L.linetr_forward(self._h, C.byref(t), nat.np_ptr(cu), d_cu_n.data_ptr() if d_cu_n is not None else None,
                                         len(cu) - 1, T, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return out

    def bn_stats_floats(self) -> int:
        return int(self._L.linetr_bn_stats_floats(self._h))

    def forward_train_tensors(self, sublines, pnt, resp, angle_sub, desc, score, cu_n, bn_running, momentum=0.1, want_batch_stats=False):
        """The training-time forward (train.py:127,163-164) on flat tensors, on an Engine made with bn_batch_stats=True: BatchNorm on
        the statistics of THIS batch; `bn_running` (float32 device tensor of bn_stats_floats() entries: per BatchNorm layer
        mean[C] | var[C]; word encoder's four layers, line encoder's four, then one per signature layer) is updated in place.  Returns line_desc [N,256], and with want_batch_stats the batch mean
        | biased variance packed the same way."""
        N, T, t, cu, _keep = self._dense_tokens(sublines, pnt, resp, angle_sub, desc, score, cu_n)
        n_stats = self.bn_stats_floats()
        if (bn_running.dtype != torch.float32 or bn_running.device != self.device or not bn_running.is_contiguous()
                or bn_running.numel() != n_stats):
            raise ValueError(f"bn_running must be a contiguous float32 tensor of {n_stats} entries on {self.device}")
        out = torch.empty((N, D), dtype=torch.float32, device=self.device)
        batch = torch.empty((n_stats,), dtype=torch.float32, device=self.device) if want_batch_stats else None
        if N == 0:
            return (out, batch) if want_batch_stats else out
        ws = self._workspace("fwd", self._L.linetr_forward_train_workspace_bytes(self._h, N, T))
        nat.check(self._L.linetr_forward_train(self._h, C.byref(t), nat.np_ptr(cu), None, len(cu) - 1, T, float(momentum),
                                               bn_running.data_ptr(), batch.data_ptr() if batch is not None else None,
                                               out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return (out, batch) if want_batch_stats else out

    def forward(self, tb: TokenBatch, out=None) -> torch.Tensor:
        return self.forward_tensors(tb.sublines, tb.pnt, tb.resp, tb.angle_sub, tb.desc, tb.score, tb.cu_n, out,
                                    tb.extra.get("d_cu_n"))

    def match(self, desc0, cu_n0, sub2line0, cu_k0, desc1, cu_n1, sub2line1, cu_k1, thr, mutual=True):
        """Match image i of side 0 with image i of side 1 for all i.  desc* are [N,256] row-major.
        Returns (Dk_flat float32 device, off_dk host int64 [P+1], match01 int32 device [K0_total])."""
        P = len(cu_n0) - 1
        assert len(cu_n1) - 1 == P
        i64 = np.int64
        if P == 1:                      # latency path of a single pair: no diffs, cumsums, reductions (~15 us of NumPy calls)
            n0, k0, n1, k1 = int(cu_n0[1] - cu_n0[0]), int(cu_k0[1] - cu_k0[0]), int(cu_n1[1] - cu_n1[0]), int(cu_k1[1] - cu_k1[0])
            dims = np.array([[n0, k0, n1, k1]], dtype=np.int32)
            off_n0, off_n1, off_k0 = (np.array([int(c[0])], dtype=i64) for c in (cu_n0, cu_n1, cu_k0))
            off_dk = np.array([0, k0 * k1], dtype=i64)
            sum_nn, sum_k = n0 * n1, k0 + k1
        else:
            dims = np.zeros((P, 4), dtype=np.int32)
            dims[:, 0] = np.diff(cu_n0); dims[:, 1] = np.diff(cu_k0)
            dims[:, 2] = np.diff(cu_n1); dims[:, 3] = np.diff(cu_k1)
            off_n0 = np.ascontiguousarray(cu_n0[:-1], dtype=i64)
            off_n1 = np.ascontiguousarray(cu_n1[:-1], dtype=i64)
            off_k0 = np.ascontiguousarray(cu_k0[:-1], dtype=i64)
            kk = dims[:, 1].astype(i64) * dims[:, 3].astype(i64)
            off_dk = np.zeros(P + 1, dtype=i64)
            np.cumsum(kk, out=off_dk[1:])
            sum_nn = int((dims[:, 0].astype(i64) * dims[:, 2].astype(i64)).sum())
            sum_k = int(dims[:, 1].sum() + dims[:, 3].sum())
        dk = torch.empty((max(int(off_dk[-1]), 1),), dtype=torch.float32, device=self.device)
        m01 = torch.empty((max(int(cu_k0[-1]), 1),), dtype=torch.int32, device=self.device)
        if P == 0:
            return dk[:0], off_dk, m01[:0]
        nbytes = self._L.linetr_match_workspace_bytes(P, sum_nn, 0, sum_k)
        ws = self._workspace("match", nbytes)
        d0, d1 = self._f32(desc0), self._f32(desc1)
        nat.check(self._L.linetr_match(self._h, P, nat.np_ptr(dims), d0.data_ptr(), nat.np_ptr(off_n0),
                                       sub2line0.data_ptr(), d1.data_ptr(), nat.np_ptr(off_n1), sub2line1.data_ptr(),
                                       float(thr), int(bool(mutual)), dk.data_ptr(), nat.np_ptr(off_dk[:-1].copy()),
                                       m01.data_ptr(), nat.np_ptr(off_k0), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return dk[:int(off_dk[-1])], off_dk, m01[:int(cu_k0[-1])]

    def match_offsets(self, desc_flat, s2l_flat, dims, off_n0, off_s0, off_n1, off_s1, thr, mutual=True):
        """linetr_match_gathered: P pairs whose descriptors (rows of desc_flat [R,256]) and key-line maps (elements of
        s2l_flat int32) sit at arbitrary offsets of the same two buffers -- the form global matching over the all-gathered
        set uses (parallel.global_match).  dims [P,4] = (n0,k0,n1,k1).
        Returns (Dk_flat, off_dk host [P+1], match01 int32 [sum k0], off_k0 host [P+1])."""
        P = len(dims)
        i64 = np.int64
        if P == 1:
            # latency path of a single pair: the seven small host tables of a given (dims, offsets) are built once and kept (a
            # NumPy array costs ~1 us to make; the call is ~45 us end to end)
            key1 = (int(dims[0][0]), int(dims[0][1]), int(dims[0][2]), int(dims[0][3]), int(off_n0[0]), int(off_s0[0]), int(off_n1[0]),
                    int(off_s1[0]))
            cache = self.__dict__.setdefault("_pair_tables", {})
            tabs = cache.get(key1)
            if tabs is None:
                if len(cache) > 256:
                    cache.clear()
                n0, k0, n1, k1 = key1[:4]
                tabs = cache[key1] = (np.array([key1[:4]], dtype=np.int32), np.array([0, k0 * k1], dtype=i64), np.array([0, k0], dtype=i64),
                                      np.array([key1[4]], dtype=i64), np.array([key1[6]], dtype=i64), np.array([key1[5]], dtype=i64),
                                      np.array([key1[7]], dtype=i64), self._L.linetr_match_workspace_bytes(1, n0 * n1, 0, k0 + k1))
            dims1, off_dk, off_k0, o0, o1, s0, s1, ws_bytes = tabs
            dk = torch.empty((max(int(off_dk[1]), 1),), dtype=torch.float32, device=self.device)
            m01 = torch.empty((max(int(off_k0[1]), 1),), dtype=torch.int32, device=self.device)
            ws = self._workspace("match", ws_bytes)
            d = desc_flat if (desc_flat.dtype == torch.float32 and desc_flat.is_contiguous() and desc_flat.device == self.device) \
                else self._f32(desc_flat)
            nat.check(self._L.linetr_match_gathered(self._h, 1, dims1.ctypes.data, d.data_ptr(), o0.ctypes.data, s2l_flat.data_ptr(),
                                                    s0.ctypes.data, d.data_ptr(), o1.ctypes.data, s2l_flat.data_ptr(),
                                                    s1.ctypes.data, float(thr), int(bool(mutual)), dk.data_ptr(),
                                                    off_dk.ctypes.data, m01.data_ptr(), off_k0.ctypes.data, ws.data_ptr(), ws.numel(),
                                                    self._stream()), self._L)
            return dk[:int(off_dk[1])], off_dk, m01[:int(off_k0[1])], off_k0
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(P, 4)
        off_dk = np.zeros(P + 1, dtype=i64)
        np.cumsum(dims[:, 1].astype(i64) * dims[:, 3].astype(i64), out=off_dk[1:])
        off_k0 = np.zeros(P + 1, dtype=i64)
        np.cumsum(dims[:, 1].astype(i64), out=off_k0[1:])
        sum_nn = int((dims[:, 0].astype(i64) * dims[:, 2].astype(i64)).sum()) if P else 0
        sum_k = int(dims[:, 1].sum() + dims[:, 3].sum()) if P else 0
        dk = torch.empty((max(int(off_dk[-1]), 1),), dtype=torch.float32, device=self.device)
        m01 = torch.empty((max(int(off_k0[-1]), 1),), dtype=torch.int32, device=self.device)
        if P == 0:
            return dk[:0], off_dk, m01[:0], off_k0
        key = (P, sum_nn, sum_k)
        if self.__dict__.get("_match_ws_key") != key:     # the workspace query is a ctypes call: cache it per shape
            self._match_ws_key = key
            self._match_ws_bytes = self._L.linetr_match_workspace_bytes(P, sum_nn, 0, sum_k)
        ws = self._workspace("match", self._match_ws_bytes)
        c64 = lambda a: np.ascontiguousarray(a, dtype=i64)
        o0, o1, s0, s1 = c64(off_n0), c64(off_n1), c64(off_s0), c64(off_s1)
        d = desc_flat if (desc_flat.dtype == torch.float32 and desc_flat.is_contiguous() and desc_flat.device == self.device) \
            else self._f32(desc_flat)
        nat.check(self._L.linetr_match_gathered(self._h, P, dims.ctypes.data, d.data_ptr(), o0.ctypes.data, s2l_flat.data_ptr(),
                                                s0.ctypes.data, d.data_ptr(), o1.ctypes.data, s2l_flat.data_ptr(),
                                                s1.ctypes.data, float(thr), int(bool(mutual)), dk.data_ptr(),
                                                off_dk.ctypes.data, m01.data_ptr(), off_k0.ctypes.data, ws.data_ptr(), ws.numel(),
                                                self._stream()), self._L)
        return dk[:int(off_dk[-1])], off_dk, m01[:int(off_k0[-1])], off_k0

    def pool_distmat(self, dist: torch.Tensor, sub2line0: torch.Tensor, k0: int, sub2line1: torch.Tensor, k1: int):
        """subline2keyline on the device: dist [n0,n1] + the two sub-line -> key-line maps -> Dk [k0,k1]."""
        d = self._f32(dist)
        n0, n1 = int(d.shape[0]), int(d.shape[1])
        dk = torch.empty((k0, k1), dtype=torch.float32, device=self.device)
        if k0 == 0 or k1 == 0:
            return dk
        ws = self._workspace("pool", self._L.linetr_pool_distmat_workspace_bytes(k0, k1))
        s0 = sub2line0.to(device=self.device, dtype=torch.int32)
        s1 = sub2line1.to(device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_pool_distmat(self._h, d.data_ptr(), n0, n1, s0.data_ptr(), k0, s1.data_ptr(), k1,
                                                  dk.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return dk

    def pool_distmat_dense(self, dist: torch.Tensor, mat0: torch.Tensor, mat1: torch.Tensor, return_verdict=False):
        """subline2keyline on the device from the two mat_klines2sublines MATRICES ([K,N] float32): a tokeniser's matrix is
        reduced to its map and pooled by the segmented-mean kernel, any other is multiplied out as given
        (linetr_pool_distmat_dense; decided on the device, asynchronous).  Returns Dk [k0,k1]; with return_verdict (tests and
        diagnosis: it waits for the device) (Dk, verdict): the word the decision was taken by (bits in include/linetr_hip.h; 0 =
        pooled by the maps), or None where the library writes none (an inner or outer dimension of 0)."""
        d, a0, a1 = self._f32(dist), self._f32(mat0), self._f32(mat1)
        n0, n1 = int(d.shape[0]), int(d.shape[1])
        k0, k1 = int(a0.shape[0]), int(a1.shape[0])
        if tuple(a0.shape) != (k0, n0) or tuple(a1.shape) != (k1, n1):
            raise ValueError(f"subline2keyline: shapes {tuple(a0.shape)} @ {tuple(d.shape)} @ {tuple(a1.shape)}^T do not chain")
        dk = torch.empty((k0, k1), dtype=torch.float32, device=self.device)
        if k0 == 0 or k1 == 0:
            return (dk, None) if return_verdict else dk
        ws = self._workspace("pool", self._L.linetr_pool_distmat_dense_workspace_bytes(k0, n0, k1, n1))
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_pool_distmat_dense(self._h, d.data_ptr(), n0, n1, a0.data_ptr(), k0, a1.data_ptr(), k1,
                                                        dk.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        if return_verdict:      # the first int32 of the workspace (stream-ordered read-back; not written for an empty inner dimension)
            return dk, (int(ws[:4].view(torch.int32).item()) if n0 > 0 and n1 > 0 else None)
        return dk

    def match_distmat(self, dist: torch.Tensor, thr, mutual=True):
        """nn_matcher_distmat on a device matrix [n0,n1]: match01 [n0] (device, int32; -1 = no match)."""
        d = self._f32(dist)
        n0, n1 = int(d.shape[0]), int(d.shape[1])
        m01 = torch.full((n0,), -1, dtype=torch.int32, device=self.device)
        if n0 == 0 or n1 == 0:
            return m01
        ws = self._workspace("match_dm", self._L.linetr_match_distmat_workspace_bytes(n0, n1))
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_match_distmat(self._h, d.data_ptr(), n0, n1, float(thr), int(bool(mutual)), m01.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return m01

    def sample_descriptors(self, points: torch.Tensor, dense_desc: torch.Tensor, *, align_corners=False, dense_layout="nchw"):
        """sample_descriptors (line_process.py:86-98) for n points [n,2] of one image; dense_desc [256,Hc,Wc] or
        [Hc,Wc,256]; returns [n,256]."""
        pts = self._f32(points.reshape(-1, 2))
        dd = self._f32(dense_desc)
        nhwc = dense_layout == "nhwc"
        Hc, Wc = (int(dd.shape[0]), int(dd.shape[1])) if nhwc else (int(dd.shape[1]), int(dd.shape[2]))
        n = int(pts.shape[0])
        out = torch.empty((n, D), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        ws = self._workspace("sample", self._L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, int(nhwc)) + 256)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_sample_descriptors(self._h, pts.data_ptr(), n, dd.data_ptr(), Hc, Wc, int(bool(align_corners)),
                                                        int(nhwc), out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return out

    def _host_stage(self, nbytes):
        """The next of a ring of four pinned device -> host staging buffers, at least nbytes long.  Returns (buffer, the ring's
        generation counters, slot, the slot's generation now): a ticket handed out on the slot before is stale from here on, which
        collect() / collect_tail() find by comparing the last two."""
        ring = self.__dict__.setdefault("_host_ring", {"i": 0, "bufs": [None] * 4, "gen": [0] * 4})
        i = ring["i"] = (ring["i"] + 1) % len(ring["bufs"])
        ring["gen"][i] += 1
        stage = ring["bufs"][i]
        if stage is None or stage.numel() < nbytes:
            stage = ring["bufs"][i] = torch.empty(nbytes * 2 + 4096, dtype=torch.uint8, pin_memory=True)
        return stage, ring["gen"], i, ring["gen"][i]

    def to_host_async(self, *tensors):
        """Queues the device -> host copies of `tensors` into a pinned staging buffer on the current stream and returns a ticket for
        collect().  Nothing is waited for: a result that is ready early (the point matcher's, queued before the line branch) travels
        while the device works on what was queued behind it."""
        sizes = [t.numel() * t.element_size() for t in tensors]
        offs = [0]
        for b in sizes:
            offs.append(offs[-1] + (b + 255) // 256 * 256)
        stage, *gen = self._host_stage(offs[-1])
        views = []
        for t, o, b in zip(tensors, offs[:-1], sizes):
            v = stage[o:o + b].view(t.dtype).view(t.shape)
            v.copy_(t.contiguous(), non_blocking=True)
            views.append(v)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return (views, ev, *gen)

    @staticmethod
    def collect(ticket):
        """Waits for a to_host_async ticket and returns its tensors as NumPy arrays (copies: the staging buffer is reused).
        At most three younger tickets may be taken before a ticket is collected (a ring of four staging buffers): a ticket whose
        buffer has been handed out again raises instead of returning another call's data."""
        views, ev, gens, i, gen = ticket
        ev.synchronize()
        if gens[i] != gen:
            raise RuntimeError("to_host_async ticket collected too late: its staging buffer has been reused (collect within three "
                               "younger tickets)")
        return [v.numpy().copy() for v in views]

    def to_host(self, *tensors):
        """Device tensors -> NumPy arrays with ONE synchronisation: every tensor is copied asynchronously into a pinned staging
        buffer, then the copies are waited for once (`.cpu()` per tensor would synchronise per tensor)."""
        return self.collect(self.to_host_async(*tensors))

    def pair_tail(self, pdesc0_cn, pdesc1_cn, thr_p, ldesc0, s2l0, k0, ldesc1, s2l1, k1, thr_l, mutual=True):
        """The matching tail of Matching.forward in ONE native call (linetr_pair_tail): point matcher on the two [256,n] SuperPoint
        descriptor sets, line matcher on the two [N,256] line-descriptor sets with their sub-line -> key-line maps, and the device ->
        host copies of the four results into one pinned block.  Asynchronous; returns a ticket for collect_tail().  A branch is
        skipped when its descriptors are None."""
        pts = pdesc0_cn is not None and pdesc1_cn is not None
        lns = ldesc0 is not None and ldesc1 is not None and k0 > 0 and k1 > 0
        p0, p1 = (self._f32(pdesc0_cn), self._f32(pdesc1_cn)) if pts else (None, None)
        np0, np1 = (int(p0.shape[1]), int(p1.shape[1])) if pts else (0, 0)
        l0, l1 = (self._f32(ldesc0), self._f32(ldesc1)) if lns else (None, None)
        n0, n1 = (int(l0.shape[0]), int(l1.shape[0])) if lns else (0, 0)
        if not lns:
            k0 = k1 = 0
        key = (np0, np1, n0, int(k0), n1, int(k1))
        cache = self.__dict__.setdefault("_tail_tables", {})
        tab = cache.get(key)
        if tab is None:
            if len(cache) > 256:
                cache.clear()
            offs = (C.c_int64 * 4)()
            out_bytes = int(self._L.linetr_pair_tail_output_bytes(np0, np1, int(k0), int(k1), offs))
            tab = cache[key] = (out_bytes, tuple(int(v) for v in offs), int(self._L.linetr_pair_tail_workspace_bytes(*key)))
        out_bytes, offs, ws_bytes = tab
        stage, *gen = self._host_stage(out_bytes)
        ws = self._workspace("tail", ws_bytes)
        s0 = s2l0 if (lns and s2l0.dtype == torch.int32 and s2l0.device == self.device and s2l0.is_contiguous()) else \
            (s2l0.to(device=self.device, dtype=torch.int32).contiguous() if lns else None)
        s1 = s2l1 if (lns and s2l1.dtype == torch.int32 and s2l1.device == self.device and s2l1.is_contiguous()) else \
            (s2l1.to(device=self.device, dtype=torch.int32).contiguous() if lns else None)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_pair_tail(self._h, p0.data_ptr() if pts else None, np0, p1.data_ptr() if pts else None, np1, float(thr_p),
                                               l0.data_ptr() if lns else None, n0, s0.data_ptr() if lns else None, int(k0),
                                               l1.data_ptr() if lns else None, n1, s1.data_ptr() if lns else None, int(k1), float(thr_l),
                                               int(bool(mutual)), stage.data_ptr(), stage.numel(), ws.data_ptr(), ws.numel(), self._stream()),
                      self._L)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        return (stage, offs, key, ev, *gen, (p0, p1, l0, l1, s0, s1))     # (inputs kept alive until collected)

    @staticmethod
    def collect_tail(ticket):
        """Waits for a pair_tail ticket: (point distances [np0,np1] f32, point match01 [np0] i32, Dk [k0,k1] f32, line match01 [k0] i32)
        as NumPy arrays (copies); the entries of a skipped branch are empty."""
        stage, offs, (np0, np1, _n0, k0, _n1, k1), ev, gens, i, gen, _keep = ticket
        ev.synchronize()
        if gens[i] != gen:
            raise RuntimeError("pair_tail ticket collected too late: its staging buffer has been reused")
        host = stage.numpy()
        f = lambda o, n, dt: host[o:o + 4 * n].view(dt).copy()
        return (f(offs[0], np0 * np1, np.float32).reshape(np0, np1), f(offs[1], np0, np.int32),
                f(offs[2], k0 * k1, np.float32).reshape(k0, k1), f(offs[3], k0, np.int32))

    def _desc_rows(self, desc: torch.Tensor):
        """Line descriptors as linetr_val_step reads them: ([B*n, 256] contiguous float32, B or None, n).  Accepts the reference's
        [B, 256, n] (contiguous, or the transposed view of [B*n, 256] rows that this build's forward returns: no copy then) or the
        rows themselves."""
        if desc.dim() == 3:
            if int(desc.shape[1]) != D:
                raise ValueError(f"line descriptors must be [B, {D}, n], got {tuple(desc.shape)}")
            B, n = int(desc.shape[0]), int(desc.shape[2])
            return self._f32(desc.transpose(1, 2)).view(B * n, D), B, n
        if desc.dim() != 2 or int(desc.shape[1]) != D:
            raise ValueError(f"line descriptors must be [B, {D}, n] or [B*n, {D}], got {tuple(desc.shape)}")
        return self._f32(desc), None, None

    def assign_from_matches(self, lmatches: torch.Tensor, n: int) -> torch.Tensor:
        """train.py:176-183 on the device (linetr_assign_from_matches): the loader's lmatches [B, M, 2] (rows whose first entry is -1
        are padding) -> mat_assign_sublines [B, n+1, n+1] float32."""
        lm = lmatches.to(device=self.device, dtype=torch.int32).contiguous()
        B, M = int(lm.shape[0]), int(lm.shape[1])
        assign = torch.empty((B, n + 1, n + 1), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_assign_from_matches(self._h, lm.data_ptr(), B, M, int(n), assign.data_ptr(), self._stream()), self._L)
        return assign

    def val_step(self, desc0, desc1, assign=None, lmatches=None, nn_thresh=0.7, mutual=True):
        """The reference's validation step after the forward, in one native call (linetr_val_step): descriptor_loss
        (evaluations/criteria.py), nn_matcher_batches (evaluations/matcher.py) and the precision / recall / F1 of
        evaluations/evaluate_pr.py.  desc0 / desc1: [B, 256, n] or [B*n, 256] (then `assign` / `lmatches` gives B); the ground truth is
        either `assign` [B, n+1, n+1] (mat_assign_sublines) or the loader's `lmatches` [B, M, 2].  One host wait.  Returns a dict:
        loss, hardest_positive, hardest_negative (float; NaN when count == 0), count, TP / FP / FN / TN (int32 [B]), precision /
        recall / f1 (float64 [B]) and the device tensors row_pos, row_neg [B, 2n] (row_neg -1: no anchor, or no semi-hard negative)
        and match01 [B, n]."""
        if (assign is None) == (lmatches is None):
            raise ValueError("val_step: give exactly one of assign / lmatches")
        d0, B0, n0 = self._desc_rows(desc0)
        d1, B1, n1 = self._desc_rows(desc1)
        B = int((assign if assign is not None else lmatches).shape[0])
        if B <= 0 or any(b is not None and b != B for b in (B0, B1)) or d0.shape[0] % B or d1.shape[0] % B:
            raise ValueError("val_step: the descriptors and the ground truth disagree about the batch size")
        n0, n1 = int(d0.shape[0]) // B, int(d1.shape[0]) // B
        n = n0
        if assign is None:
            assign = self.assign_from_matches(lmatches, n)
        else:
            assign = self._f32(assign)
            if n0 == n1 and tuple(assign.shape) != (B, n + 1, n + 1):
                raise ValueError(f"val_step: assign must be [{B}, {n + 1}, {n + 1}], got {tuple(assign.shape)}")
        offs = (C.c_int64 * 4)()
        out_bytes = int(self._L.linetr_val_step_output_bytes(B, offs))
        ws = self._workspace("val_step", max(int(self._L.linetr_val_step_workspace_bytes(B, n)), 256))
        stage, *_gen = self._host_stage(out_bytes)
        row_pos = torch.empty((B, 2 * n), dtype=torch.float32, device=self.device)
        row_neg = torch.empty((B, 2 * n), dtype=torch.float32, device=self.device)
        match01 = torch.empty((B, n), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_val_step(self._h, d0.data_ptr(), n0, d1.data_ptr(), n1, assign.data_ptr(), B, float(nn_thresh),
                                              int(bool(mutual)), row_pos.data_ptr(), row_neg.data_ptr(), match01.data_ptr(),
                                              stage.data_ptr(), stage.numel(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        ev.synchronize()
        host = stage.numpy()
        scalars = host[offs[0]:offs[0] + 24].view(np.float64)
        counts = host[offs[2]:offs[2] + 16 * B].view(np.int32).reshape(B, 4).copy()
        scores = host[offs[3]:offs[3] + 24 * B].view(np.float64).reshape(B, 3).copy()
        return {"loss": float(scalars[0]), "hardest_positive": float(scalars[1]), "hardest_negative": float(scalars[2]),
                "count": int(host[offs[1]:offs[1] + 8].view(np.int64)[0]),
                "TP": counts[:, 0], "FP": counts[:, 1], "FN": counts[:, 2], "TN": counts[:, 3],
                "precision": scores[:, 0], "recall": scores[:, 1], "f1": scores[:, 2],
                "row_pos": row_pos, "row_neg": row_neg, "match01": match01}

    def loss_step(self, desc0, desc1, assign=None, lmatches=None, upstream=None):
        """descriptor_loss AND its gradient with respect to both descriptor sets in one native call (linetr_desc_loss_grad): what
        `loss.backward()` leaves in line_desc0.grad / line_desc1.grad when the reference's criterion (evaluations/criteria.py) is
        differentiated by torch.  Inputs as val_step takes them; `upstream`: the gradient arriving at the loss, a one-element float32
        device tensor (read on the device: no host wait for it), default 1.  One host wait.  Returns a dict: loss, hardest_positive,
        hardest_negative (float; NaN when count == 0), count, and the device tensors grad0 / grad1 in the shape of desc0 / desc1
        ([B, 256, n] inputs: the transposed view of the [B*n, 256] rows the kernels write); count == 0: both all zero.
        Like val_step, every call uses the engine's one cached workspace whatever the stream: calls from two streams are safe only
        because each ends in its host wait before it returns."""
        if (assign is None) == (lmatches is None):
            raise ValueError("loss_step: give exactly one of assign / lmatches")
        d0, B0, n0 = self._desc_rows(desc0.detach())
        d1, B1, n1 = self._desc_rows(desc1.detach())
        B = int((assign if assign is not None else lmatches).shape[0])
        if B <= 0 or any(b is not None and b != B for b in (B0, B1)) or d0.shape[0] % B or d1.shape[0] % B:
            raise ValueError("loss_step: the descriptors and the ground truth disagree about the batch size")
        n0, n1 = int(d0.shape[0]) // B, int(d1.shape[0]) // B
        n = n0
        if assign is None:
            assign = self.assign_from_matches(lmatches, n)
        else:
            assign = self._f32(assign)
            if n0 == n1 and tuple(assign.shape) != (B, n + 1, n + 1):
                raise ValueError(f"loss_step: assign must be [{B}, {n + 1}, {n + 1}], got {tuple(assign.shape)}")
        if upstream is not None:
            upstream = self._f32(upstream.detach().reshape(-1))
            if upstream.numel() != 1:
                raise ValueError("loss_step: upstream must hold one element")
        ws = self._workspace("loss_step", max(int(self._L.linetr_desc_loss_grad_workspace_bytes(B, n)), 256))
        stage, *_gen = self._host_stage(32)
        grad0, grad1 = torch.empty_like(d0), torch.empty_like(d1)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_desc_loss_grad(self._h, d0.data_ptr(), n0, d1.data_ptr(), n1, assign.data_ptr(), B,
                                                    upstream.data_ptr() if upstream is not None else None, grad0.data_ptr(),
                                                    grad1.data_ptr(), stage.data_ptr(), stage.numel(), ws.data_ptr(), ws.numel(),
                                                    self._stream()), self._L)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        ev.synchronize()
        host = stage.numpy()
        scalars = host[:24].view(np.float64)
        grad0, grad1 = (g.view(B, n, D).transpose(1, 2) if d.dim() == 3 else g for g, d in ((grad0, desc0), (grad1, desc1)))
        return {"loss": float(scalars[0]), "hardest_positive": float(scalars[1]), "hardest_negative": float(scalars[2]),
                "count": int(host[24:32].view(np.int64)[0]), "grad0": grad0, "grad1": grad1}

    # ------------------------------------------------------------------ backward of the 1x1 layers and the descriptor head
    def _act_rows(self, t: torch.Tensor, width: int, what: str, strided=True):
        """Activations as the point-wise layers read them: a float32 [rows, width] tensor whose rows are `stride(0)` floats apart
        (a multiple of 4, 16-byte aligned; anything else is copied).  Accepts [B, width, n] (contiguous, or the transposed view of
        [B*n, width] rows: no copy then) or the rows themselves.  Returns (rows, B or None, n or None)."""
        t = t.detach()
        if t.dim() == 3:
            if int(t.shape[1]) != width:
                raise ValueError(f"{what} must be [B, {width}, n] or [rows, {width}], got {tuple(t.shape)}")
            B, n = int(t.shape[0]), int(t.shape[2])
            return self._f32(t.transpose(1, 2)).view(B * n, width), B, n
        if t.dim() != 2 or int(t.shape[1]) != width:
            raise ValueError(f"{what} must be [B, {width}, n] or [rows, {width}], got {tuple(t.shape)}")
        ok = (strided and t.device == self.device and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) >= width
              and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)
        return (t if ok else self._f32(t)), None, None

    @staticmethod
    def _like_input(rows: torch.Tensor, B, n):
        """[B*n, C] rows back in the shape of a [B, C, n] input (the transposed view), or the rows of a 2-D input"""
        return rows if B is None else rows.view(B, n, rows.shape[1]).transpose(1, 2)

    def _weight_2d(self, weight: torch.Tensor) -> torch.Tensor:
        """a Conv1d(k=1) [N, K, 1] or a Linear [N, K] weight as [N, K] float32 on the device"""
        w = weight.detach()
        if w.dim() == 3 and int(w.shape[2]) == 1:
            w = w[:, :, 0]
        if w.dim() != 2:
            raise ValueError(f"a point-wise weight must be [N, K] or [N, K, 1], got {tuple(weight.shape)}")
        return self._f32(w)

    def _stream_workspace(self, tag: str, nbytes: int) -> torch.Tensor:
        """the cached workspace of `tag` for the current stream (these calls return without a host wait: one per stream)"""
        return self._workspace(f"{tag}:{torch.cuda.current_stream(self.device).cuda_stream}", max(int(nbytes), 256))

    def linear_forward(self, x, weight, bias=None, relu=False) -> torch.Tensor:
        """A point-wise linear layer (Conv1d(k=1) / Linear) on the unfolded weight, by exact-fp32 MFMA (linetr_linear_forward):
        y = act(x W^T + b).  x: [B, K, n] or [rows, K]; weight [N, K] or [N, K, 1]; y in x's layout ([B, N, n] inputs: the transposed
        view of the [B*n, N] rows the kernel writes).  No host wait."""
        W = self._weight_2d(weight)
        N, K = int(W.shape[0]), int(W.shape[1])
        xr, B, n = self._act_rows(x, K, "x")
        b = self._f32(bias.detach().reshape(-1)) if bias is not None else None
        if b is not None and b.numel() != N:
            raise ValueError(f"bias must hold {N} elements")
        y = torch.empty((xr.shape[0], N), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_linear_forward(self._h, xr.data_ptr(), xr.stride(0), W.data_ptr(), b.data_ptr() if b is not None else None,
                                                    int(xr.shape[0]), N, K, int(bool(relu)), y.data_ptr(), N, self._stream()), self._L)
        return self._like_input(y, B, n)

    def linear_backward(self, x, weight, grad_out, mask=None, need=(True, True, True)):
        """The layer's backward (linetr_linear_backward): (dx, dW, db) for the gradient `grad_out` arriving at y = act(x W^T + b);
        `mask`: the layer's own post-ReLU output (the gradient passes where it is > 0), None for no activation.  dx in x's layout, dW in
        the weight's shape, db [N]; `need` = which of the three to compute (the others are None).  Deterministic; no host wait."""
        W = self._weight_2d(weight)
        N, K = int(W.shape[0]), int(W.shape[1])
        xr, B, n = self._act_rows(x, K, "x")
        g, _, _ = self._act_rows(grad_out, N, "grad_out", strided=mask is None)
        m = self._act_rows(mask, N, "mask", strided=False)[0] if mask is not None else None
        rows = int(xr.shape[0])
        if int(g.shape[0]) != rows or (m is not None and int(m.shape[0]) != rows):
            raise ValueError("linear_backward: x, grad_out and mask disagree about the number of rows")
        dx = torch.empty_strided((rows, K), (xr.stride(0), 1), dtype=torch.float32, device=self.device) if need[0] else None
        dW = torch.empty((N, K), dtype=torch.float32, device=self.device) if need[1] else None
        db = torch.empty((N,), dtype=torch.float32, device=self.device) if need[2] else None
        ws = self._stream_workspace("linear_bwd", self._L.linetr_linear_backward_workspace_bytes(rows, N, K))
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_linear_backward(self._h, xr.data_ptr(), xr.stride(0), W.data_ptr(), g.data_ptr(), g.stride(0), ptr(m), rows,
                                                     N, K, ptr(dx), ptr(dW), ptr(db), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return (self._like_input(dx, B, n) if dx is not None else None, dW.view(weight.shape) if dW is not None else None, db)

    def _head_args(self, x, weight, bias):
        W = self._weight_2d(weight)
        if tuple(W.shape) != (D, D) or bias is None or bias.numel() != D:
            raise ValueError(f"the descriptor head is final_proj: a [{D}, {D}] weight and a [{D}] bias")
        xr, B, n = self._act_rows(x, D, "x", strided=False)
        return xr, W, self._f32(bias.detach().reshape(-1)), B, n

    def head_forward(self, x, weight, bias) -> torch.Tensor:
        """The descriptor head (models/line_transformer.py:245-246; linetr_head_forward): line_desc = F.normalize(final_proj(x), dim=1),
        one kernel.  x: the pre-head features [B, 256, n] or [rows, 256]; line_desc in x's layout.  No host wait."""
        xr, W, b, B, n = self._head_args(x, weight, bias)
        desc = torch.empty_like(xr)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_head_forward(self._h, xr.data_ptr(), W.data_ptr(), b.data_ptr(), int(xr.shape[0]), desc.data_ptr(),
                                                  self._stream()), self._L)
        return self._like_input(desc, B, n)

    def head_backward(self, x, weight, bias, grad_desc, need=(True, True, True)):
        """The head's backward (linetr_head_backward): (dx, dW, db) for the gradient `grad_desc` arriving at line_desc, as torch autograd
        differentiates F.normalize(final_proj(x)).  Shapes and `need` as linear_backward.  Deterministic; no host wait."""
        xr, W, b, B, n = self._head_args(x, weight, bias)
        g = self._act_rows(grad_desc, D, "grad_desc", strided=False)[0]
        rows = int(xr.shape[0])
        if int(g.shape[0]) != rows:
            raise ValueError("head_backward: x and grad_desc disagree about the number of rows")
        dx = torch.empty_like(xr) if need[0] else None
        dW = torch.empty((D, D), dtype=torch.float32, device=self.device) if need[1] else None
        db = torch.empty((D,), dtype=torch.float32, device=self.device) if need[2] else None
        ws = self._stream_workspace("head_bwd", self._L.linetr_head_backward_workspace_bytes(rows))
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_head_backward(self._h, xr.data_ptr(), W.data_ptr(), b.data_ptr(), g.data_ptr(), rows, ptr(dx), ptr(dW),
                                                   ptr(db), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return (self._like_input(dx, B, n) if dx is not None else None, dW.view(weight.shape) if dW is not None else None, db)

    # ------------------------------------------------------------------ neighbour-line attention for training
    def _cu_sub_dev(self, cu_sub) -> torch.Tensor:
        """sub-line offsets [n_images + 1] as an int32 tensor on the device (a device tensor is taken as it is: no host wait)"""
        cu = cu_sub if isinstance(cu_sub, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(cu_sub, dtype=np.int32)))
        cu = cu.detach().reshape(-1)
        if cu.numel() < 2:
            raise ValueError("cu_sub must hold n_images + 1 >= 2 offsets")
        if cu.device != self.device or cu.dtype != torch.int32 or not cu.is_contiguous():
            cu = cu.to(device=self.device, dtype=torch.int32).contiguous()
        return cu

    def _attn_rows(self, named, N=None):
        """head-major [N, 256] rows as the attention kernels read them: strided row views pass as they are, anything else is copied"""
        rows = [self._act_rows(t, D, name)[0] for name, t in named]
        N = int(rows[0].shape[0]) if N is None else N
        for (name, _), r in zip(named, rows):
            if r.dim() != 2 or int(r.shape[0]) != N:
                raise ValueError(f"{name} must be [{N}, {D}] head-major rows, got {tuple(r.shape)}")
        return rows, N

    def sig_attention_forward(self, q, k, v, cu_sub):
        """The neighbour-line attention softmax(q^T k / 8) v of models/line_transformer.py:132-136 with its softmax statistics
        (linetr_sig_attention_forward; exact-fp32 MFMA).  q, k, v: head-major rows [N, 256] (column h*64 + d), q UNSCALED; each may be a
        strided row view, e.g. a column block of one [N, 768] buffer.  cu_sub [n_images + 1]: one image is one softmax domain (a device
        int32 tensor is read in place).  Returns (message [N, 256] head-major, lse [N, 4] = m + log l).  No host wait."""
        (qr, kr, vr), N = self._attn_rows((("q", q), ("k", k), ("v", v)))
        cu = self._cu_sub_dev(cu_sub)
        msg = torch.empty((N, D), dtype=torch.float32, device=self.device)
        lse = torch.empty((N, 4), dtype=torch.float32, device=self.device)
        if N == 0:                                   # (an empty tensor has no address to hand over)
            return msg, lse
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_sig_attention_forward(self._h, qr.data_ptr(), qr.stride(0), kr.data_ptr(), kr.stride(0), vr.data_ptr(),
                                                           vr.stride(0), cu.data_ptr(), cu.numel() - 1, N, msg.data_ptr(), D, lse.data_ptr(),
                                                           self._stream()), self._L)
        return msg, lse

    def sig_attention_backward(self, q, k, v, o, lse, grad_out, cu_sub, need=(True, True, True)):
        """The attention's backward (linetr_sig_attention_backward): (dq, dk, dv) [N, 256] head-major for the gradient `grad_out` arriving at
        the message `o`; q, k, v, o, lse as sig_attention_forward took and returned them.  P is recomputed from q, k and lse; nothing n x n
        is stored.  `need` = which of the three to compute (the others are None).  Deterministic; no host wait."""
        (qr, kr, vr, orow, g), N = self._attn_rows((("q", q), ("k", k), ("v", v), ("o", o), ("grad_out", grad_out)))
        ls = self._f32(lse.detach())
        if tuple(ls.shape) != (N, 4):
            raise ValueError(f"lse must be [{N}, 4], got {tuple(ls.shape)}")
        cu = self._cu_sub_dev(cu_sub)
        dq, dk, dv = (torch.empty((N, D), dtype=torch.float32, device=self.device) if n else None for n in need)
        if N == 0:
            return dq, dk, dv
        ws = self._stream_workspace("sig_attn_bwd", self._L.linetr_sig_attention_backward_workspace_bytes(N))
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_sig_attention_backward(self._h, qr.data_ptr(), qr.stride(0), kr.data_ptr(), kr.stride(0), vr.data_ptr(),
                                                            vr.stride(0), orow.data_ptr(), orow.stride(0), ls.data_ptr(), g.data_ptr(), g.stride(0),
                                                            cu.data_ptr(), cu.numel() - 1, N, ptr(dq), D, ptr(dk), D, ptr(dv), D, ws.data_ptr(),
                                                            ws.numel(), self._stream()), self._L)
        return dq, dk, dv

    def line_ground_truth(self, lines0, lines1, H, *, thres_reprojected=3, thres_angdiff=2, min_overlap_ratio=0.3, max_matches=None,
                          counts=None, dustbin=True, directions=False, projected=False):
        """The ground truth of homography pairs in one native call (linetr_gt_assign): what the reference's dataset builder computes
        per pair with find_line_matches / calculate_line_overlaps in both directions (dataloaders/build_homography_dataset.py:210-237,
        dataloaders/utils/util_lines.py:67-171).

        lines0 [B, n0, 2, 2] / lines1 [B, n1, 2, 2] (or [n, 2, 2] for one pair; then H is [3, 3]): the sub-lines' end points, torch or
        NumPy.  float32 on both sides computes as the reference does; float64 on either side selects the float64 instance.  H [B, 3, 3]
        takes image-0 pixels to image-1 pixels; its inverse is np.linalg.inv(H), as in the builder.  `counts` = (count0 [B], count1 [B]):
        the valid prefix of each item.  max_matches (M) defaults to the builder's int(max_sublines * 1.5) with max_sublines = n0; an item
        with more pairs than that makes the call run once more with room for all of them (0: no list, `found` only).  Returns a dict of device tensors:
        assign [B, n0 + 1, n1 + 1] float32 (`dustbin`; what val_step(assign=...) takes) or [B, n0, n1], lmatches [B, M, 2] int32 with -1
        behind each list, found [B] int32; with `directions` match_dir [B, 2, n0, n1] uint8 and overlap_dir [B, 2, n0, n1] (direction 1
        as [i][j]); with `projected` proj0 / proj1.  One host wait (the list sizes)."""
        def arr(x):
            return x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        l0, l1 = arr(lines0), arr(lines1)
        Hm = np.asarray(H.detach().cpu() if isinstance(H, torch.Tensor) else H, dtype=np.float64)
        if l0.dim() == 3 and l1.dim() == 3 and Hm.shape == (3, 3):
            l0, l1, Hm = l0[None], l1[None], Hm[None]
        if l0.dim() != 4 or l1.dim() != 4 or tuple(l0.shape[2:]) != (2, 2) or tuple(l1.shape[2:]) != (2, 2) or l0.shape[0] != l1.shape[0]:
            raise ValueError(f"line_ground_truth: lines must be [B, n, 2, 2], got {tuple(l0.shape)} and {tuple(l1.shape)}")
        B, n0, n1 = int(l0.shape[0]), int(l0.shape[1]), int(l1.shape[1])
        if Hm.shape != (B, 3, 3):
            raise ValueError(f"line_ground_truth: H must be [{B}, 3, 3], got {Hm.shape}")
        dt = torch.float64 if torch.float64 in (l0.dtype, l1.dtype) else torch.float32
        l0, l1 = (t.to(device=self.device, dtype=dt).contiguous() for t in (l0, l1))
        Hd = torch.from_numpy(np.stack([Hm, np.linalg.inv(Hm)], axis=1).reshape(B, 2, 9)).to(self.device)
        c0 = c1 = None
        if counts is not None:
            c0, c1 = (arr(c).to(device=self.device, dtype=torch.int32).contiguous() for c in counts)
            if tuple(c0.shape) != (B,) or tuple(c1.shape) != (B,):
                raise ValueError("line_ground_truth: counts must be two arrays of B entries")
        M = int(n0 * 1.5) if max_matches is None else int(max_matches)
        pad = int(bool(dustbin))
        ptr = lambda t: t.data_ptr() if t is not None else None
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):     # a heads-only engine has no handle: the current device is used
            assign = new((B, n0 + pad, n1 + pad), torch.float32)
            found = new((B,), torch.int32)
            mdir = new((B, 2, n0, n1), torch.uint8) if directions else None
            odir = new((B, 2, n0, n1), dt) if directions else None
            p0, p1 = (new((B, n0, 2, 2), dt), new((B, n1, 2, 2), dt)) if projected else (None, None)
            ws = self._workspace("gt_assign", int(self._L.linetr_gt_assign_workspace_bytes(B, n0, n1)))
            while True:
                lm = new((B, M, 2), torch.int32)
                nat.check(self._L.linetr_gt_assign(self._h, int(dt == torch.float64), l0.data_ptr(), n0, l1.data_ptr(), n1, Hd.data_ptr(), B,
                                                   ptr(c0), ptr(c1), float(thres_reprojected), float(thres_angdiff), float(min_overlap_ratio),
                                                   pad, assign.data_ptr(), lm.data_ptr(), M, found.data_ptr(), ptr(mdir), ptr(odir), ptr(p0),
                                                   ptr(p1), ws.data_ptr(), ws.numel(), self._stream()), self._L)
                most = int(found.max())
                if most <= M or M == 0:          # (max_matches = 0: no list is wanted, `found` alone)
                    break
                M = most                         # once more with room for every pair
        out = {"assign": assign, "lmatches": lm, "found": found}
        if directions:
            out["match_dir"], out["overlap_dir"] = mdir, odir
        if projected:
            out["proj0"], out["proj1"] = p0, p1
        return out

    def match_points(self, desc0_cn: torch.Tensor, desc1_cn: torch.Tensor, thr, mutual=True):
        """nn_matcher on [256,n] descriptors; returns (dist [n0,n1] device, match01 [n0] device)."""
        d0, d1 = self._f32(desc0_cn), self._f32(desc1_cn)
        n0, n1 = int(d0.shape[1]), int(d1.shape[1])
        dist = torch.empty((n0, n1), dtype=torch.float32, device=self.device)
        m01 = torch.full((n0,), -1, dtype=torch.int32, device=self.device)
        if n0 == 0 or n1 == 0:
            return dist, m01
        need = 4 * (n0 + n1) * (D + 1) + 2048 + self._L.linetr_match_workspace_bytes(1, n0 * n1, 0, n0 + n1)
        ws = self._workspace("match", need)
        nat.check(self._L.linetr_match_points(self._h, d0.data_ptr(), n0, d1.data_ptr(), n1, float(thr),
                                              int(bool(mutual)), dist.data_ptr(), m01.data_ptr(), ws.data_ptr(),
                                              ws.numel(), self._stream()), self._L)
        return dist, m01

    def superpoint_heads(self, score_logits: torch.Tensor = None, desc_raw: torch.Tensor = None, *, nhwc=True,
                         nchw=False):
        """Fused SuperPoint head post-processing (models/superpoint.py:161-167, 190-193).

        score_logits [B,65,Hc,Wc] (convPb output) -> dense_score [B,8Hc,8Wc];
        desc_raw [B,256,Hc,Wc] (convDb output) -> L2-normalised descriptors as [B,Hc,Wc,256] (`nhwc`, the layout
        `describe_lines(..., dense_layout='nhwc')` consumes without a transposition pass) and/or [B,256,Hc,Wc]
        (`nchw`, the reference's 'dense_descriptor').  Returns (dense_score, desc_nhwc, desc_nchw), None where not
        requested."""
        sl = self._f32(score_logits) if score_logits is not None else None
        dr = self._f32(desc_raw) if desc_raw is not None else None
        ref = sl if sl is not None else dr
        if ref is None:
            raise ValueError("superpoint_heads needs at least one head")
        B, _, Hc, Wc = (int(v) for v in ref.shape)
        if sl is not None and tuple(sl.shape) != (B, 65, Hc, Wc):
            raise ValueError(f"score_logits must be [B,65,Hc,Wc], got {tuple(sl.shape)}")
        if dr is not None and tuple(dr.shape) != (B, D, Hc, Wc):
            raise ValueError(f"desc_raw must be [B,{D},Hc,Wc], got {tuple(dr.shape)}")
        score = torch.empty((B, Hc * 8, Wc * 8), dtype=torch.float32, device=self.device) if sl is not None else None
        o_nhwc = torch.empty((B, Hc, Wc, D), dtype=torch.float32, device=self.device) if (dr is not None and nhwc) else None
        o_nchw = torch.empty((B, D, Hc, Wc), dtype=torch.float32, device=self.device) if (dr is not None and nchw) else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):     # a heads-only engine has no handle: the current device is used
            nat.check(self._L.linetr_superpoint_heads(self._h, ptr(sl), ptr(dr), B, Hc, Wc, ptr(score), ptr(o_nhwc),
                                                      ptr(o_nchw), self._stream()), self._L)
        return score, o_nhwc, o_nchw

    def superpoint_keypoints(self, dense_score: torch.Tensor, dense_desc: torch.Tensor = None, *, nms_radius=4,
                             keypoint_threshold=0.005, remove_borders=4, max_keypoints=-1, align_corners=False,
                             dense_layout="nhwc"):
        """SuperPoint's key-point branch for a batch (models/superpoint.py:168-187, 195-197) in native calls: simple_nms,
        threshold, remove_borders, top_k_keypoints, (row, col) -> (x, y) and sample_descriptors.

        dense_score [B,H,W]; dense_desc [B,Hc,Wc,256] ('nhwc', what superpoint_heads emits) or [B,256,Hc,Wc] ('nchw'), or None.
        Returns three per-image lists: keypoints [n_b,2] (x, y), scores [n_b], descriptors [256,n_b] -- views into three batch
        buffers -- or None in place of the descriptors when no map is given.  Key points and scores are the reference's bit for
        bit, in its order (row-major; with max_keypoints and more candidates than that: descending score, equal scores by ascending
        row-major index).  ONE host wait per call: the packed offsets come back before the descriptor buffer is sized.  (Maps with
        exactly equal neighbouring scores can hold more key points than the default capacity: then the detector runs a second
        time with the capacity it reported.)"""
        ds = self._f32(dense_score)
        if ds.dim() != 3:
            raise ValueError(f"dense_score must be [B,H,W], got {tuple(ds.shape)}")
        B, H, W = (int(v) for v in ds.shape)
        r, k, border = int(nms_radius), int(max_keypoints), int(remove_borders)
        thr = float(np.float32(keypoint_threshold))
        if not 0 <= r <= 8:
            raise ValueError(f"nms_radius must be 0..8, got {r}")
        if k < -1 or k == 0 or k > 4096:
            raise ValueError(f"max_keypoints must be -1 (all) or 1..4096, got {k}")
        if not thr >= 0 or border < 0:
            raise ValueError("keypoint_threshold and remove_borders must be >= 0")
        if dense_layout not in ("nhwc", "nchw"):
            raise ValueError("dense_layout must be 'nhwc' or 'nchw'")
        dd = None
        if dense_desc is not None:
            dd = self._f32(dense_desc)
            nhwc = dense_layout == "nhwc"
            if dd.dim() != 4 or int(dd.shape[0]) != B or int(dd.shape[3 if nhwc else 1]) != D:
                raise ValueError(f"dense_desc must be [B,Hc,Wc,{D}] (nhwc) or [B,{D},Hc,Wc] (nchw), got {tuple(dd.shape)}")
            Hc, Wc = (int(dd.shape[1]), int(dd.shape[2])) if nhwc else (int(dd.shape[2]), int(dd.shape[3]))
        if B == 0 or H == 0 or W == 0:
            e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
            return ([e(0, 2) for _ in range(B)], [e(0) for _ in range(B)],
                    [e(D, 0) for _ in range(B)] if dd is not None else None)
        # kept points of a tie-free map lie at Chebyshev distance >= r + 1 from each other
        cap = min(H * W, -(-H // (r + 1)) * -(-W // (r + 1)))
        with torch.cuda.device(self.device):     # a heads-only engine has no handle: the current device is used
            cu = torch.empty(B + 1, dtype=torch.int32, device=self.device)
            found = torch.empty(B, dtype=torch.int32, device=self.device)
            while True:
                kp = torch.empty((B * cap, 2), dtype=torch.float32, device=self.device)
                sc = torch.empty((B * cap,), dtype=torch.float32, device=self.device)
                ws = self._workspace("keypoints", self._L.linetr_superpoint_keypoints_workspace_bytes(B, H, W, cap))
                nat.check(self._L.linetr_superpoint_keypoints(self._h, ds.data_ptr(), B, H, W, r, thr, border, k, cap, kp.data_ptr(),
                                                              sc.data_ptr(), cu.data_ptr(), found.data_ptr(), ws.data_ptr(), ws.numel(),
                                                              self._stream()), self._L)
                h_cu, h_found = self.collect(self.to_host_async(cu, found))
                if int(h_found.max()) <= cap:
                    break
                cap = int(h_found.max())         # exact ties only: once more with room for every candidate
            n_total = int(h_cu[-1])
            desc = None
            if dd is not None:
                desc = torch.empty((D * n_total,), dtype=torch.float32, device=self.device)
                if n_total > 0:
                    wd = self._workspace("sample", self._L.linetr_point_descriptors_workspace_bytes(B, Hc, Wc, int(nhwc)) + 256)
                    nat.check(self._L.linetr_point_descriptors(self._h, kp.data_ptr(), cu.data_ptr(), B, n_total, dd.data_ptr(), Hc, Wc,
                                                               int(bool(align_corners)), int(nhwc), desc.data_ptr(), wd.data_ptr(),
                                                               wd.numel(), self._stream()), self._L)
        o = h_cu.tolist()
        kps = [kp[o[b]:o[b + 1]] for b in range(B)]
        scs = [sc[o[b]:o[b + 1]] for b in range(B)]
        descs = [desc[D * o[b]:D * o[b + 1]].view(D, o[b + 1] - o[b]) for b in range(B)] if desc is not None else None
        return kps, scs, descs

    PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16x6": 2, "f16x3": 3}

    def set_precision(self, mode: str):
        """arithmetic mode of the dense contractions: 'f32' | 'bf16x6' (fp32-faithful, default) | 'bf16x3'."""
        nat.check(self._L.linetr_set_precision(self._h, self.PRECISIONS[mode]), self._L)

    def get_precision(self) -> str:
        code = self._L.linetr_get_precision(self._h)
        return {v: k for k, v in self.PRECISIONS.items()}[code]

    def debug_posenc(self, which: str, in0, in1, in2=None):
        """Layers 1-3 of the word ('word': points [rows,2], scores [rows]) or line ('line': sub-lines [rows,2,2],
        resp [rows], angles [rows,2]) positional encoder alone -> [rows,128] (unit tests of the fused MLP kernel)."""
        a, b = self._f32(in0), self._f32(in1)
        c = self._f32(in2) if in2 is not None else None
        rows = int(b.shape[0])
        out = torch.empty((rows, 128), dtype=torch.float32, device=self.device)
        nat.check(self._L.linetr_debug_posenc(self._h, {"word": 0, "line": 1}[which], a.data_ptr(), b.data_ptr(),
                                                 c.data_ptr() if c is not None else None, rows, out.data_ptr(),
                                                 self._stream()), self._L)
        return out

    def debug_gemm(self, A, W, bias=None, residual=None, act=0, cache_weights=False, out=None):
        """Y = act(A @ W.T + bias) (+ residual) on the library's MFMA GEMM (diagnostics / unit tests).
        A / out / residual may be row-strided views (stride(0) multiple of 4, stride(1) == 1)."""
        W = self._f32(W)
        if A.dtype != torch.float32 or A.device != self.device or A.stride(1) != 1:
            A = self._f32(A)
        M, K = A.shape
        N = W.shape[0]
        Y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=self.device)
        b = self._f32(bias) if bias is not None else None
        r = residual
        if r is not None and (r.stride(0) != Y.stride(0) or r.stride(1) != 1):
            r = self._f32(r) if Y.stride(0) == N else None
            assert r is not None, "residual must share the output's row stride"
        nat.check(self._L.linetr_debug_gemm(self._h, A.data_ptr(), A.stride(0), W.data_ptr(),
                                            b.data_ptr() if b is not None else None,
                                            r.data_ptr() if r is not None else None, Y.data_ptr(), Y.stride(0), M, N, K,
                                            int(act), int(cache_weights), self._stream()), self._L)
        return Y

    # tile names of linetr_debug_gemm_case (csrc/lt_gemm_split.h: SplitTile, csrc/lt_gemm.h: F32Tile), by index
    GEMM_SPLIT_TILES = ("32x32k4", "112x256", "128x64", "256x128", "128x256", "64x256", "128x128", "128x128s", "256x256", "64x64",
                        "64x128")
    GEMM_F32_TILES = ("128x64", "128x128", "64x128")
    GEMM_WS = "ws64x256"          # LINETR_GEMM_TILE_WS
    _GEMM_TILE_WS = 100

    def _gemm_tile_code(self, tile):
        if tile is None or tile == -1:
            return -1
        if tile == self.GEMM_WS:
            return self._GEMM_TILE_WS
        names = self.GEMM_F32_TILES if self.get_precision() == "f32" else self.GEMM_SPLIT_TILES
        if tile not in names:
            raise ValueError(f"no GEMM tile {tile!r} in {self.get_precision()} mode")
        return names.index(tile)

    def _gemm_tile_name(self, code):
        if code == self._GEMM_TILE_WS:
            return self.GEMM_WS
        return (self.GEMM_F32_TILES if self.get_precision() == "f32" else self.GEMM_SPLIT_TILES)[code]

    def gemm_tile(self, M, N, K, *, groups=1, act=0, residual=False, concat=False, norm=0, lda=None, ldy=None, tile=-1) -> str:
        """Name of the GEMM kernel the forward pass takes for act([A | A2] W^T + b) (+ R) of this shape at the current precision
        (`tile`: of the kernel that launches when that tile is asked for); nothing is launched."""
        flag = C.c_void_p(16)      # never dereferenced: says that the operand is there
        c = nat.GemmCase(A=None, lda=int(lda or K), A2=flag if concat else None, lda2=int(K), K1=32 if concat else 0, W=None, bias=None,
                         R=flag if residual else None, Y=None, ldy=int(ldy or N), M=int(M), N=int(N), K=int(K), act=int(act),
                         groups=int(groups), gA=0, gY=0, norm=int(norm), gamma=None, beta=None, add2=None, eps=0.0, via_row_norm=0,
                         tile=self._gemm_tile_code(tile))
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_gemm_case(self._h, C.byref(c), C.byref(used), None), self._L)
        return self._gemm_tile_name(used.value)

    def debug_gemm_case(self, A, W, bias=None, residual=None, act=0, *, A2=None, groups=1, gA=0, gY=None, norm=0, gamma=None,
                        beta=None, add2=None, eps=0.0, via_row_norm=False, tile=-1, out=None):
        """ONE kernel of the GEMM family alone on a full problem description (linetr_debug_gemm_case; diagnostics / unit tests):
        Y_g = norm(act([A_g | A2_g] @ W_g.T + bias_g) (+ residual)) (+ add2).  A [M, K1], A2 [M, K - K1], residual and out [M, N]
        are group 0's views (row-strided: stride(0) a multiple of 4, stride(1) == 1); group g sits gA / gY floats behind them in the
        same storage.  W [groups * N, K].  tile: -1 (the forward pass's choice), a name of GEMM_SPLIT_TILES / GEMM_F32_TILES or
        GEMM_WS.  Returns (out -- or a new [M, N] / [groups, M, N] tensor --, name of the kernel that ran).  Every operand is
        checked against the storage behind it before anything is launched."""
        W = self._f32(W)
        M, K1 = (int(v) for v in A.shape)
        K = K1 + (int(A2.shape[1]) if A2 is not None else 0)
        N = int(W.shape[0]) // groups
        if W.shape != (groups * N, K) or not W.is_contiguous():
            raise ValueError(f"W must be a contiguous [{groups} * N, {K}] tensor")
        if out is None:
            full = torch.empty((groups, M, N), dtype=torch.float32, device=self.device)
            out, gY = full[0], M * N
        else:
            full = out
        gY = int(gY or 0)

        def extent(t, rows, cols, gstride, what):
            """t's first `rows` x `cols` block of every group must lie inside t's storage"""
            if t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what}: a float32 matrix on the engine's device with unit column stride expected")
            if t.shape[0] < rows or t.shape[1] < cols:
                raise ValueError(f"{what}: shape {tuple(t.shape)} is smaller than [{rows}, {cols}]")
            have = t.untyped_storage().nbytes() // 4 - t.storage_offset()
            need = (groups - 1) * gstride + (rows - 1) * t.stride(0) + cols if rows > 0 else 0
            if need > have:
                raise ValueError(f"{what}: {need} floats needed behind its first element, the storage holds {have}")
            return t

        extent(A, M, K1, int(gA), "A")
        if A2 is not None:
            extent(A2, M, K - K1, int(gA), "A2")
        extent(out, M, N, gY, "out")
        if groups > 1 and gY < (M - 1) * out.stride(0) + N:
            raise ValueError("gY: the groups' outputs overlap")
        if residual is not None and extent(residual, M, N, 0, "residual").stride(0) != out.stride(0):
            raise ValueError("residual must share the output's row stride")
        vec = lambda t, n, what: None if t is None else extent(self._f32(t).reshape(1, -1), 1, n, 0, what)
        b, ga, be = vec(bias, groups * N, "bias"), vec(gamma, N, "gamma"), vec(beta, N, "beta")
        if add2 is not None and (extent(add2, M, N, 0, "add2").stride(0) != D or N != D):
            raise ValueError("add2 must have row stride 256")
        ptr = lambda t: t.data_ptr() if t is not None else None
        c = nat.GemmCase(A=ptr(A), lda=A.stride(0), A2=ptr(A2), lda2=A2.stride(0) if A2 is not None else 0, K1=K1 if A2 is not None else 0,
                         W=ptr(W), bias=ptr(b), R=ptr(residual), Y=ptr(out), ldy=out.stride(0), M=M, N=N, K=K, act=int(act),
                         groups=int(groups), gA=int(gA), gY=gY, norm=int(norm), gamma=ptr(ga), beta=ptr(be), add2=ptr(add2),
                         eps=float(eps), via_row_norm=int(bool(via_row_norm)), tile=self._gemm_tile_code(tile))
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_gemm_case(self._h, C.byref(c), C.byref(used), self._stream()), self._L)
        return (full if groups > 1 or full is out else out), self._gemm_tile_name(used.value)

    SIG_KERNELS = ("sig_attn", "sig_attn_small", "sig_attn_split4", "sig_attn_split8", "sig_qkv_attn")

    def sig_attention_kernel(self, cu_sub) -> int:
        """Which signature-attention kernel (index into SIG_KERNELS) the forward pass takes for a batch with these sub-line
        offsets at the current precision; nothing is launched."""
        cu = np.ascontiguousarray(np.asarray(cu_sub, dtype=np.int32))
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_sig_attention(self._h, -1, 0, None, 0, cu.ctypes.data, len(cu) - 1, None,
                                                     C.byref(used), self._stream()), self._L)
        return used.value

    def debug_sig_attention(self, kernel, x, cu_sub, layer=0, out=None):
        """ONE signature-attention kernel alone (linetr_debug_sig_attention; diagnostics / unit tests).  kernel: -1 (the
        forward pass's choice) or an index into SIG_KERNELS.  x: q/k/v rows [N, 768] head-major, q pre-scaled by 1/8 (kernels
        0-3; may be the columns 256.. of [N, 1024] rows for kernel 1), or z rows [N, 256] for the fused kernel 4, which
        projects them with signature layer `layer`.  Returns (message [N, 256] head-major, kernel used)."""
        if x.dtype != torch.float32 or x.device != self.device or x.stride(1) != 1:
            x = self._f32(x)
        cu = np.ascontiguousarray(np.asarray(cu_sub, dtype=np.int32))
        N = int(cu[-1]) if len(cu) else 0
        if int(x.shape[0]) < N:
            raise ValueError(f"{N} rows expected, got {int(x.shape[0])}")
        msg = out if out is not None else torch.empty((N, D), dtype=torch.float32, device=self.device)
        if msg.dtype != torch.float32 or msg.device != self.device or not msg.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor on the engine's device")
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_sig_attention(self._h, int(kernel), int(layer), x.data_ptr(), x.stride(0), cu.ctypes.data,
                                                     len(cu) - 1, msg.data_ptr(), C.byref(used), self._stream()), self._L)
        return msg, used.value

    TOK_MLP_VARIANTS = ("tok_mlp_word", "tok_mlp_line", "tok_mlp_dual", "tok_mlp_seq", "mlp123_gemm_chain")

    def tok_mlp_variant(self, rows_word, rows_line) -> int:
        """Which launch (index into TOK_MLP_VARIANTS) the forward pass takes for the two positional encoders at these row counts
        and the current precision; nothing is launched."""
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_tok_mlp(self._h, -1, None, None, int(rows_word), None, None, None, int(rows_line), None, None, 0,
                                               C.byref(used), self._stream()), self._L)
        return used.value

    def debug_tok_mlp(self, variant, word=None, line=None, out_word=None, out_line=None, max_blocks=0):
        """ONE launch of the positional encoders' MLP up to its fourth ReLU alone (linetr_debug_tok_mlp; diagnostics / unit tests).
        variant: -1 (the forward pass's choice) or an index into TOK_MLP_VARIANTS.  word = (pnt [>= rows, 2], score [>= rows], rows),
        line = (sublines [>= rows, 2, 2], resp [>= rows], angle [>= rows, 2], rows): contiguous float32 tensors on the engine's
        device.  out_word / out_line: contiguous [>= rows, 256] (made here when None).  max_blocks > 0 caps the persistent grid.
        Returns (out_word, out_line, variant used)."""
        def f32(t, n, what):
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f"{what}: a contiguous float32 tensor of at least {n} elements on the engine's device expected")
            return t.data_ptr()
        pw = [None, None]; pl = [None, None, None]
        rw = rl = 0
        if word is not None:
            rw = int(word[2])
            pw = [f32(word[0], 2 * rw, "pnt"), f32(word[1], rw, "score")]
            if out_word is None:
                out_word = torch.empty((rw, D), dtype=torch.float32, device=self.device)
            f32(out_word, rw * D, "out_word")
        if line is not None:
            rl = int(line[3])
            pl = [f32(line[0], 4 * rl, "sublines"), f32(line[1], rl, "resp"), f32(line[2], 2 * rl, "angle")]
            if out_line is None:
                out_line = torch.empty((rl, D), dtype=torch.float32, device=self.device)
            f32(out_line, rl * D, "out_line")
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_tok_mlp(self._h, int(variant), pw[0], pw[1], rw, pl[0], pl[1], pl[2], rl,
                                               out_word.data_ptr() if out_word is not None else None,
                                               out_line.data_ptr() if out_line is not None else None, int(max_blocks), C.byref(used),
                                               self._stream()), self._L)
        return out_word, out_line, used.value

    def debug_bn_train(self, which, *, z=None, rows=0, channels=0, ld=0, gamma=None, beta=None, word=None, line=None, out=None,
                       momentum=0.1, running=None, batch=None, affine=None):
        """BatchNorm(batch statistics) + ReLU alone (linetr_debug_bn_train; diagnostics / unit tests), on an Engine made with
        bn_batch_stats=True.  which = -1: one free-standing layer on z (a float32 device tensor holding `rows` rows of `channels` channels
        at row stride `ld`, transformed in place; a view keeps its offset), gamma / beta [C], running [2 C] (in place), batch and
        affine [2 C] (optional outputs: mean | biased variance, alpha | beta').  which = 0 / 1: the word / line encoder's four
        layers on word = (pnt, score, rows) / line = (sublines, resp, angle, rows) as debug_tok_mlp takes them; out
        [>= rows, keyline_encoder[3]] (made here when None); running / batch hold the encoder's four layers packed.
        Returns (out or z, number of row chunks the statistics were summed in)."""
        def f32(t, n, what):
            if t is None:
                return None
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f"{what}: a contiguous float32 tensor of at least {n} elements on the engine's device expected")
            return t.data_ptr()
        which = int(which)
        e = list(self.cfg["keyline_encoder"])
        ins = [None, None, None]
        if which < 0:
            rows, C_, ld = int(rows), int(channels), int(ld)
            n_stats = 2 * C_
            pz = f32(z, (rows - 1) * ld + C_ if rows > 0 else 0, "z")
            res = z
        else:
            C_, ld, pz = 0, 0, None
            n_stats = 2 * sum(e)
            if which == 0:
                rows = int(word[2])
                ins = [f32(word[0], 2 * rows, "pnt"), f32(word[1], rows, "score"), None]
            else:
                rows = int(line[3])
                ins = [f32(line[0], 4 * rows, "sublines"), f32(line[1], rows, "resp"), f32(line[2], 2 * rows, "angle")]
            if out is None:
                out = torch.empty((rows, e[3]), dtype=torch.float32, device=self.device)
            res = out
        nbytes = self._L.linetr_debug_bn_train_workspace_bytes(self._h, which, rows)
        if nbytes < 0:
            raise ValueError("debug_bn_train: which must be -1, 0 or 1 and rows non-negative")
        ws = self._workspace("bn_debug", nbytes)
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_bn_train(self._h, which, pz, rows, C_, ld, f32(gamma, C_, "gamma"), f32(beta, C_, "beta"), *ins,
                                                f32(out, rows * e[3], "out") if which >= 0 else None, float(momentum),
                                                f32(running, n_stats, "running"), f32(batch, n_stats, "batch"), f32(affine, n_stats, "affine"),
                                                C.byref(used), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return res, used.value

    CLS_POOL_KERNELS = ("cls_pool", "cls_pool_online", "cls_pool_online_reverse", "cls_pool_online_split4")

    def cls_pool_kernel(self, N, dense=False) -> int:
        """Which pooling kernel (index into CLS_POOL_KERNELS) the forward pass takes for N sub-lines (dense: the [N, T] token
        tensors of linetr_forward instead of linetr_describe's compact token list); nothing is launched."""
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_cls_pool(self._h, -1, None, 0, None, int(N), 1, None, None, 0, 1, None, 1, 1, 1, 0,
                                                C.c_void_p(16) if dense else None, None, C.byref(used), self._stream()), self._L)
        return used.value

    def debug_cls_pool(self, kernel, a4, out, N, T, *, recs=None, sub2line=None, cpnt=None, first_pad=0, n_images=1, dense_map=None,
                       nhwc=True, Hc=0, Wc=0, align_corners=False, desc_dense=None):
        """ONE CLS-pooling kernel alone (linetr_debug_cls_pool; diagnostics / unit tests).  kernel: -1 (the forward pass's choice)
        or an index into CLS_POOL_KERNELS.  Kernel 0 reads desc_dense [N, T, 256] and a4 [N * T, 256]; the online kernels the
        records `recs` (a uint8 device tensor holding LineRec[K]), sub2line [N] int32, cpnt [first_pad + n_images, 2], a4
        [first_pad + n_images, 256] and n_images maps of Hc x Wc cells (`nhwc`: channel-last, else NCHW).  out: contiguous float32
        [>= N, 4, 544].  Returns (out, kernel used)."""
        for t in (a4, out, cpnt, dense_map, desc_dense):
            if t is not None and (t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous()):
                raise ValueError("contiguous float32 tensors on the engine's device expected")
        if out.numel() < N * 4 * 544:
            raise ValueError("out is smaller than [N, 4, 544]")
        if desc_dense is None:
            if recs.dtype != torch.uint8 or sub2line.dtype != torch.int32 or sub2line.numel() < N:
                raise ValueError("recs: uint8 bytes of LineRec[K]; sub2line: int32 [N]")
            if a4.numel() < (first_pad + n_images) * D or cpnt.numel() < (first_pad + n_images) * 2 or dense_map.numel() < n_images * Hc * Wc * D:
                raise ValueError("a4 / cpnt / dense_map are smaller than first_pad + n_images rows / n_images maps")
        elif a4.numel() < N * T * D or desc_dense.numel() < N * T * D:
            raise ValueError("a4 / desc_dense are smaller than [N * T, 256]")
        ptr = lambda t: t.data_ptr() if t is not None else None
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_cls_pool(self._h, int(kernel), ptr(recs), recs.numel() // nat.REC_DTYPE.itemsize if recs is not None else 0,
                                                ptr(sub2line), int(N), int(T), ptr(cpnt), ptr(a4), int(first_pad), int(n_images),
                                                ptr(dense_map), int(bool(nhwc)), int(Hc), int(Wc), int(bool(align_corners)),
                                                ptr(desc_dense), ptr(out), C.byref(used), self._stream()), self._L)
        return out, used.value

    MATCH_PATHS = ("pair_dist + pair_pool + pair_final", "pair_match_fused<false>", "pair_match_fused<true>")

    def match_path(self, dims) -> int:
        """Which path (index into MATCH_PATHS) linetr_match takes for pairs of these dims [P, 4] = (n0, k0, n1, k1); nothing is
        launched."""
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1, 4)
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_match(self._h, len(dims), dims.ctypes.data, None, None, None, None, None, None, 0.0, 0, None, None,
                                             None, None, None, 0, -1, -1, -1, -1, C.byref(used), self._stream()), self._L)
        return used.value

    def debug_match(self, path, dims, desc0, off_n0, s2l0, desc1, off_n1, s2l1, thr, mutual, dk, off_dk, m01, off_k0, *,
                    seg1_global=-1, cache_dk=-1, device_table=-1) -> int:
        """ONE path of the matcher alone (linetr_debug_match; diagnostics / unit tests).  path: -1 (the matcher's choice) or an index
        into MATCH_PATHS; seg1_global / cache_dk / device_table: -1 or 0 / 1, path 0 only.  Operands as linetr_match: dims [P, 4],
        float32 descriptor rows desc0 / desc1 [>= rows, 256], int32 maps, the four host offset arrays [P], and the caller's own
        outputs dk (float32) and m01 (int32), written at off_dk / off_k0.  Tensors go to the library as they are (a view keeps its
        offset).  Returns the path that launched."""
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1, 4)
        P = len(dims)
        offs = [np.ascontiguousarray(o, dtype=np.int64) for o in (off_n0, off_dk, off_n1, off_k0)]
        if any(len(o) != P for o in offs):
            raise ValueError("one offset per pair expected")
        for t, dt in ((desc0, torch.float32), (desc1, torch.float32), (dk, torch.float32), (s2l0, torch.int32), (s2l1, torch.int32), (m01, torch.int32)):
            if t is not None and (t.dtype != dt or t.device != self.device or not t.is_contiguous()):
                raise ValueError("contiguous float32 / int32 tensors on the engine's device expected")
        d64 = dims.astype(np.int64)
        ws = self._workspace("match", self._L.linetr_match_workspace_bytes(P, int((d64[:, 0] * d64[:, 2]).sum()), 0, int((d64[:, 1] + d64[:, 3]).sum())))
        ptr = lambda t: t.data_ptr() if t is not None else None
        used = C.c_int32(-1)
        nat.check(self._L.linetr_debug_match(self._h, P, dims.ctypes.data, ptr(desc0), offs[0].ctypes.data, ptr(s2l0), ptr(desc1),
                                             offs[2].ctypes.data, ptr(s2l1), float(thr), int(bool(mutual)), ptr(dk), offs[1].ctypes.data,
                                             ptr(m01), offs[3].ctypes.data, ws.data_ptr(), ws.numel(), int(path), int(seg1_global),
                                             int(cache_dk), int(device_table), C.byref(used), self._stream()), self._L)
        return used.value

    # ------------------------------------------------------------------ split-tile operands (csrc/lt_st_image.h; the GEMM on them: experiments/csrc/lt_gemm_st.h)
    def to_st(self, X):
        """fp32 [rows, K] -> ST image (uint8 tensor); K % 32 == 0."""
        X = self._f32(X)
        rows, K = X.shape
        out = torch.empty(int(self._L.linetr_st_bytes(rows, K)), dtype=torch.uint8, device=self.device)
        nat.check(self._L.linetr_debug_to_st(self._h, X.data_ptr(), X.stride(0), rows, K, out.data_ptr(), self._stream()), self._L)
        return out

    def from_st(self, st, rows, K):
        X = torch.empty((rows, K), dtype=torch.float32, device=self.device)
        nat.check(self._L.linetr_debug_from_st(self._h, st.data_ptr(), rows, K, X.data_ptr(), K, self._stream()), self._L)
        return X

    def gemm_st(self, A1, K1, W, M, N, A2=None, K2=0, bias=None, residual=None, act=0, out_st=None, out=None):
        """act([A1 | A2] W^T + bias) (+ residual) on ST images; returns the ST image `out_st` or the fp32 matrix `out`."""
        b = self._f32(bias) if bias is not None else None
        nat.check(self._L.linetr_debug_gemm_st(
            self._h, A1.data_ptr(), K1, A2.data_ptr() if A2 is not None else None, K2, W.data_ptr(),
            b.data_ptr() if b is not None else None, residual.data_ptr() if residual is not None else None,
            out_st.data_ptr() if out_st is not None else None, out.data_ptr() if out is not None else None,
            out.stride(0) if out is not None else 0, M, N, int(act), self._stream()), self._L)
        return out_st if out_st is not None else out

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, on: bool):
        nat.check(self._L.linetr_set_profiling(self._h, int(on)), self._L)

    def get_profile(self):
        arr = (nat.ProfileEntry * 64)()
        n = C.c_int32()
        nat.check(self._L.linetr_get_profile(self._h, arr, 64, C.byref(n)), self._L)
        return [dict(name=arr[i].name.decode(), calls=arr[i].calls, ms=arr[i].ms, flops=arr[i].flops,
                     bytes=arr[i].bytes) for i in range(min(n.value, 64))]


class DescribePipeline:
    """Software pipeline over CONSECUTIVE batches of Engine.describe_lines (linetr_describe_submit / linetr_describe_join, SURVEY.md
    section 7 step 5): a batch is cut into stages that run on their own streams, so batch i + 1's front (layout pass, tokeniser, token
    MLP, pooling -- half of it HBM-bound) runs on the GPU under batch i's line-signature network (MFMA-bound).  Each batch is described
    whole -- every GEMM sees the full batch -- and its results are those of describe_lines bit for bit; what is traded is depth - 1
    batches of latency:

        pipe = DescribePipeline(engine)            # depth 2: two batches in flight
        for batch in batches:
            done = pipe.submit(lines6, offsets, dense_desc, dense_score, ...)   # -> (TokenBatch, line_desc) of an EARLIER batch, or None
            if done: consume(*done)
        for done in pipe.drain(): consume(*done)

    The tensors a submit returns are ordered on the current stream like describe_lines' own."""

    def __init__(self, engine: "Engine", depth: int = 2):
        if not 2 <= depth <= engine._L.linetr_pipeline_max_slots():
            raise ValueError(f"depth must be 2 .. {engine._L.linetr_pipeline_max_slots()}")
        self.eng, self.depth = engine, int(depth)
        self.i = 0
        self.inflight = []            # [(slot, (tb, ld))] submitted and not joined yet, oldest first

    def _join(self, entry):
        slot, (tb, ld) = entry
        if tb.K > 0 and tb.N > 0:     # an empty batch queues nothing
            self.eng.describe_join(slot)
        return tb, ld

    def submit(self, *args, **kw):
        slot = self.i % self.depth
        self.i += 1
        self.inflight.append((slot, self.eng.describe_lines(*args, pipeline_slot=(slot, self.depth), **kw)))
        return self._join(self.inflight.pop(0)) if len(self.inflight) >= self.depth else None

    def drain(self):
        """joins and returns every batch still in flight, oldest first."""
        out = [self._join(e) for e in self.inflight]
        self.inflight = []
        return out

    def __del__(self):
        # a pipeline dropped with batches in flight: their output tensors go back to torch's caching allocator, which orders re-use on
        # the CURRENT stream only -- join them first, so that whoever gets those blocks next is queued behind the library's streams
        try:
            self.drain()
        except Exception:
            pass
