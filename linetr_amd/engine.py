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
from ._shapes import D, ptr
from .engine_debug import _DebugSurface
from .engine_train import _TrainSurface

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


def _hip_device(device) -> torch.device:
    """`device` as a torch device with an index; anything but a HIP device is refused"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("linetr_amd.Engine needs a HIP device (torch device 'cuda:N'); there is no CPU path")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


class Engine(_TrainSurface, _DebugSurface):
    """One native model instance on one GPU.  This file holds construction, the helpers every surface shares and the inference
    surface; training and evaluation are engine_train.py, the single-kernel entry points of the unit tests and tools engine_debug.py."""

    def __init__(self, state_dict, device="cuda:0", lib_path=None, **model_cfg):
        """lib_path: another build of the library (nat.EXPERIMENTS_LIB_PATH for tools / experiment tests)."""
        cfg = {**DEFAULT_MODEL, **model_cfg}
        self.device = _hip_device(device)
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
        self.device = _hip_device(device)
        self.cfg = dict(DEFAULT_MODEL)
        self._L = nat.lib()
        self._h = None
        self._ws = {}
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._L.linetr_destroy(self._h)
            self._h = None
        sp = self.__dict__.pop("_sp", None)
        if sp and sp["enc"] is not None:
            self._L.linetr_sp_encoder_destroy(sp["enc"])

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name: str, *args):
        """One native call `name`(handle, *args, current stream) with the engine's device current (a weight-less engine has no handle:
        the current device is what the library uses); a failure raises with the text of the library the call went through."""
        with torch.cuda.device(self.device):
            nat.check(getattr(self._L, name)(self._h, *args, self._stream()), self._L)

    def _event(self) -> torch.cuda.Event:
        """an event recorded on the current stream"""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return ev

    @staticmethod
    def _await_stage(what, ev, gens, i, gen):
        """Waits for the copies into a _host_stage() buffer that `ev` closes; raises where the buffer has been handed out again since."""
        ev.synchronize()
        if gens[i] != gen:
            raise RuntimeError(f"{what} ticket collected too late: its staging buffer has been reused (collect within three younger "
                               "tickets)")

    def _workspace(self, tag: str, nbytes: int) -> torch.Tensor:
        ws = self._ws.get(tag)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=self.device)
            self._ws[tag] = ws
        return ws

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.data_ptr() % 16:       # a contiguous view at an odd storage offset: the kernels load and store 16-byte vectors
            t = t.clone()
        return t

    def _dense_map(self, t: torch.Tensor):
        """A dense descriptor map (or a raw head output) as the kernels take it: (tensor, format bits).  A contiguous float16, bfloat16
        or float32 tensor on this device is passed as it is and read in place, the half types with their LINETR_DENSE_* bit; anything
        else -- another dtype, another device, a non-contiguous tensor -- becomes a float32 copy (_f32)."""
        bits = self._half_bits(t)
        if bits:
            return (t if t.data_ptr() % 16 == 0 else t.clone()), bits
        return self._f32(t), 0

    def _half_bits(self, t: torch.Tensor) -> int:
        """The LINETR_DENSE_* bit of a tensor the kernels would read in place as a half map (nothing is converted); 0 for every other"""
        bits = nat.dense_type_bits(t.dtype)
        return bits if bits and t.device == self.device and t.is_contiguous() else 0

    def _dense_maps_typed(self, tensors):
        """Tensors that one native call reads with ONE element type (the maps of a ragged batch, the two raw head outputs): (tensors,
        format bits).  All of one half type: each as _dense_map passes it; anything else: every one through _f32.  Each tensor is
        converted or cloned at most once."""
        kinds = {self._half_bits(t) for t in tensors}
        bits = kinds.pop() if len(kinds) == 1 else 0
        return [self._dense_map(t)[0] if bits else self._f32(t) for t in tensors], bits

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

    @staticmethod
    def _lines_blob(lines6, offsets, tie_order):
        """The lines of a batch as the pre-filter entry points take them: (one [sum K,6] float64 array, row offsets [B+1] int32, B,
        the number of rows)."""
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
        return cat, offsets, len(offsets) - 1, int(offsets[-1])

    def prefilter(self, lines6, height, width, *, remove_borders, min_length, max_keylines, token_distance,
                  max_tokens, valid_masks=None, offsets=None, n_threads=0, tie_order="numpy"):
        """a1-a3 for a batch.  `lines6` is a list of [K_i,6] float64 arrays, or one concatenated [sum K,6] array
        with `offsets` [B+1].  Returns (recs, cu_k, cu_n); recs lives in pinned memory ready for an async H2D.

        tie_order: the length sort of models/line_process.py:15-16 is np.argsort, whose order among EQUAL lengths is NumPy's
        business (unstable, CPU-dispatched).  "numpy" (default): the images the native pre-filter reports as holding equal
        lengths (linetr_prefilter_tied_images; rare with a real detector) are re-ordered with NumPy itself and re-packed, so the
        batched path gives the reference's rows on this machine, like the per-image path does.  "stable": keep the native order
        (stable ascending argsort, reversed) -- machine-independent."""
        cat, offsets, B, cap = self._lines_blob(lines6, offsets, tie_order)
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

    def prefilter_ragged(self, lines6, shapes, *, remove_borders, min_length, max_keylines, token_distance, max_tokens,
                         valid_masks=None, offsets=None, n_threads=0, tie_order="numpy"):
        """prefilter() for images of DIFFERENT sizes (linetr_prefilter_ragged).  `shapes` [B] holds every image's (height, width);
        `min_length` and `token_distance` are one value for the batch or one per image (the reference's auto_min_length gives every
        image max(16, max(shape) / 40) and max(8, max(shape) / 80) of its own shape); a valid mask has its own image's shape.  The rest,
        the returned (recs, cu_k, cu_n) and tie_order are prefilter()'s."""
        cat, offsets, B, cap = self._lines_blob(lines6, offsets, tie_order)
        if len(shapes) != B:
            raise ValueError(f"{len(shapes)} image shapes for {B} images")
        per_image = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (B,))
        table = np.zeros(B, dtype=nat.PREFILTER_IMAGE_DTYPE)
        table["height"], table["width"] = [int(s[0]) for s in shapes], [int(s[1]) for s in shapes]
        table["min_length"], table["token_distance"] = per_image(min_length), per_image(token_distance)
        keep = []
        for i, vm in enumerate(valid_masks if valid_masks is not None else []):
            if vm is not None:
                if np.ndim(vm) != 2 or np.shape(vm) != (int(table["height"][i]), int(table["width"][i])):
                    raise ValueError(f"valid mask {i} has shape {np.shape(vm)}, the native pre-filter needs its image's "
                                     f"({int(table['height'][i])}, {int(table['width'][i])})")
                keep.append(np.ascontiguousarray(vm, dtype=np.float64))
                table["valid_mask"][i] = keep[-1].ctypes.data
        recs, cu_k, cu_n = self._record_blob(cap, B)
        nat.check(self._L.linetr_prefilter_ragged(nat.np_ptr(cat), nat.np_ptr(offsets), B, nat.np_ptr(table), int(remove_borders),
                                                  int(max_keylines), int(max_tokens), int(n_threads), nat.np_ptr(recs), cap,
                                                  nat.np_ptr(cu_k), nat.np_ptr(cu_n)), self._L)
        if tie_order == "numpy":
            tied = np.empty(max(B, 1), dtype=np.int32)
            n_tied = self._L.linetr_prefilter_tied_images(nat.np_ptr(tied), B)
            for i in tied[:n_tied].tolist():     # every tied image with the settings of ITS table entry
                repack_like_numpy(self._L, recs, cu_k, cu_n, i, cat[offsets[i]:offsets[i + 1]], int(table["height"][i]),
                                  int(table["width"][i]), remove_borders, float(table["min_length"][i]), max_keylines,
                                  float(table["token_distance"][i]), max_tokens, valid_masks[i] if valid_masks is not None else None)
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
    def _dense_maps(self, dense_desc, dense_score, B, dense_layout, in_place=True):
        """The dense maps of a B-image call as device tensors with a batch axis, checked against each other: dense_score [B,H,W]
        (float32) and dense_desc [B,256,H/8,W/8] ('nchw') or [B,H/8,W/8,256] ('nhwc'), float32 or -- read in place, _dense_map -- float16 /
        bfloat16.  in_place=False: for an entry point that takes float32 maps only (linetr_fixed_size), every map goes through _f32.
        Returns (dense_desc, dense_score, H, W, the native `dense_is_nhwc`: layout flag | element-type bits)."""
        dense_desc, bits = self._dense_map(dense_desc) if in_place else (self._f32(dense_desc), 0)
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
        return dense_desc, dense_score, H, W, int(nhwc) | bits

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
        on the fly.  A contiguous float16 / bfloat16 dense_desc on this device is read in place (no float32 copy; the results are those
        of its exact upcast); dense_score and every output are float32.  Returns (TokenBatch, line_desc [N,256]).  With want_tokens=False the dense [N,T,...] token
        tensors (pnt / mask / score / desc) are not materialised (zero-sized in the TokenBatch).

        pipeline_slot = (slot, n_slots): linetr_describe_submit -- the batch runs on the library's stage streams, overlapped with the
        batches submitted to the other slots, and is NOT joined: the returned tensors may be read only after describe_join(slot)
        (class DescribePipeline does the bookkeeping)."""
        B = len(cu_k) - 1
        K, N, T = int(cu_k[-1]), int(cu_n[-1]), int(max_tokens)
        dense_desc, dense_score, H, W, nhwc = self._dense_maps(dense_desc, dense_score, B, dense_layout)
        tb, ld, ct = self._describe_outputs(recs, cu_k, cu_n, T, want_tokens, want_mat)
        if K == 0 or N == 0:
            return tb, ld
        n_real = int(recs["n_tok"][:K].sum())
        d_recs, d_cu = self._upload_recs(recs, K, B, tb)
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

    def _describe_outputs(self, recs, cu_k, cu_n, T, want_tokens, want_mat):
        """The outputs of a fused describe call (describe / describe_ragged): (TokenBatch, line_desc [N,256], the native Tokens struct
        that points into them)."""
        B = len(cu_k) - 1
        K, N = int(cu_k[-1]), int(cu_n[-1])
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
        ct = tb.c_tokens()
        if not want_tokens:
            ct.pnt = ct.mask = ct.desc = ct.score = None
        if want_mat and K and N:
            tb.extra["cu_k32"] = cu_k32 = np.ascontiguousarray(cu_k, dtype=np.int32)     # read by the native call: kept with the batch
            ct.h_cu_klines = cu_k32.ctypes.data
            if B == 1:
                tb.mat = tb.mat.view(K, N)
        return tb, ld, ct

    def describe_ragged(self, recs, cu_k, cu_n, dense_descs, dense_scores, *, token_distance, max_tokens, align_corners=False,
                        want_tokens=False, dense_layout="nchw", want_mat=False):
        """describe() for images of DIFFERENT sizes (linetr_describe_ragged).  `dense_descs` / `dense_scores` are lists with one map per
        image, each its own tensor of its own shape -- [256,H/8,W/8] ('nchw') or [H/8,W/8,256] ('nhwc'), and [H,W]; a leading batch axis
        of 1 is accepted -- and need not be packed.  A call has one element type: if every descriptor map is a contiguous float16 (or every
        one a bfloat16) device tensor they are read in place, a batch of mixed element types is upcast to float32 together.  `token_distance`: one value, or one per image (what the records were made with:
        prefilter_ragged).  Returns (TokenBatch, line_desc [N,256]) like describe(); want_mat serves up to 8 images."""
        B = len(cu_k) - 1
        K, N, T = int(cu_k[-1]), int(cu_n[-1]), int(max_tokens)
        if len(dense_descs) != B or len(dense_scores) != B:
            raise ValueError("dense maps must have one entry per image")
        nhwc = dense_layout == "nhwc"
        table = np.zeros(B, dtype=nat.IMAGE_DTYPE)
        table["token_distance"] = np.broadcast_to(np.asarray(token_distance, dtype=np.float64), (B,))
        maps = []
        typed, bits = self._dense_maps_typed(list(dense_descs))
        for i, (dd, ds) in enumerate(zip(typed, dense_scores)):
            ds = self._f32(ds)
            dd, ds = (dd[0] if dd.dim() == 4 else dd), (ds[0] if ds.dim() == 3 else ds)
            H, W = int(ds.shape[-2]), int(ds.shape[-1])
            want = (H // 8, W // 8, D) if nhwc else (D, H // 8, W // 8)
            if ds.dim() != 2 or tuple(dd.shape) != want:
                raise ValueError(f"image {i}: dense_descriptor shape {tuple(dd.shape)} does not match {want} ({dense_layout}) of its "
                                 f"{H} x {W} score map")
            maps.append((dd, ds))
            table[i] = (dd.data_ptr(), ds.data_ptr(), H, W, table["token_distance"][i])
        tb, ld, ct = self._describe_outputs(recs, cu_k, cu_n, T, want_tokens, want_mat)
        if K == 0 or N == 0:
            return tb, ld
        tb.extra["dense"] = maps          # the stream reads them after this call returns
        n_real = int(recs["n_tok"][:K].sum())
        d_recs, d_cu = self._upload_recs(recs, K, B, tb)
        nbytes = self._L.linetr_describe_ragged_workspace_bytes(self._h, nat.np_ptr(table), B, int(nhwc) | bits, N, n_real)
        if nbytes < 0:      # the table is refused: the call says why
            nbytes = 0
        ws = self._workspace("desc", nbytes)
        cu = np.ascontiguousarray(cu_n, dtype=np.int32)
        recs_c = np.ascontiguousarray(recs[:K])
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_describe_ragged(self._h, d_recs.data_ptr(), nat.np_ptr(recs_c), K, N, n_real, nat.np_ptr(cu),
                                                     d_cu.data_ptr() if d_cu is not None else None, nat.np_ptr(table), B, T,
                                                     int(bool(align_corners)), int(nhwc) | bits, ct, tb.sub2line.data_ptr(), ld.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return tb, ld

    def describe_lines_ragged(self, lines6, offsets, dense_descs, dense_scores, *, remove_borders, min_length, max_keylines,
                              token_distance, max_tokens, align_corners=False, want_tokens=False, dense_layout="nchw",
                              angles="native", want_mat=False, valid_masks=None):
        """describe_lines() for images of DIFFERENT sizes: prefilter_ragged + describe_ragged.  The image sizes are those of the score
        maps; `min_length` / `token_distance`: one value or one per image; `angles` as in describe_lines()."""
        if angles not in ("native", "numpy"):
            raise ValueError("angles must be 'native' or 'numpy'")
        shapes = [(int(ds.shape[-2]), int(ds.shape[-1])) for ds in dense_scores]
        recs, cu_k, cu_n = self.prefilter_ragged(lines6, shapes, offsets=offsets, remove_borders=remove_borders, min_length=min_length,
                                                 max_keylines=max_keylines, token_distance=token_distance, max_tokens=max_tokens,
                                                 valid_masks=valid_masks)
        if angles == "numpy" and len(recs):
            from .line_process import get_angles
            recs["angle"] = get_angles(np.stack([recs["sp"], recs["ep"]], axis=1))     # (records live in the pinned upload slot)
        return self.describe_ragged(recs, cu_k, cu_n, dense_descs, dense_scores, token_distance=token_distance, max_tokens=max_tokens,
                                    align_corners=align_corners, want_tokens=want_tokens, dense_layout=dense_layout, want_mat=want_mat)

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
            last["slot"]["event"] = self._event()
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
        [Hc,Wc,256], float32 or (read in place) float16 / bfloat16; returns [n,256] float32."""
        pts = self._f32(points.reshape(-1, 2))
        dd, bits = self._dense_map(dense_desc)
        Hc, Wc = (int(dd.shape[0]), int(dd.shape[1])) if dense_layout == "nhwc" else (int(dd.shape[1]), int(dd.shape[2]))
        nhwc = int(dense_layout == "nhwc") | bits          # the native `dense_is_nhwc`: layout flag | element-type bits
        n = int(pts.shape[0])
        out = torch.empty((n, D), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        ws = self._workspace("sample", self._L.linetr_sample_descriptors_workspace_bytes(Hc, Wc, int(nhwc)))
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
        return (views, self._event(), *gen)

    @staticmethod
    def collect(ticket):
        """Waits for a to_host_async ticket and returns its tensors as NumPy arrays (copies: the staging buffer is reused).
        At most three younger tickets may be taken before a ticket is collected (a ring of four staging buffers): a ticket whose
        buffer has been handed out again raises instead of returning another call's data."""
        views, *waited = ticket
        Engine._await_stage("to_host_async", *waited)
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
            ev = self._event()
        return (stage, offs, key, ev, *gen, (p0, p1, l0, l1, s0, s1))     # (inputs kept alive until collected)

    @staticmethod
    def collect_tail(ticket):
        """Waits for a pair_tail ticket: (point distances [np0,np1] f32, point match01 [np0] i32, Dk [k0,k1] f32, line match01 [k0] i32)
        as NumPy arrays (copies); the entries of a skipped branch are empty."""
        stage, offs, (np0, np1, _n0, k0, _n1, k1), *waited, _keep = ticket
        Engine._await_stage("pair_tail", *waited)
        host = stage.numpy()
        f = lambda o, n, dt: host[o:o + 4 * n].view(dt).copy()
        return (f(offs[0], np0 * np1, np.float32).reshape(np0, np1), f(offs[1], np0, np.int32),
                f(offs[2], k0 * k1, np.float32).reshape(k0, k1), f(offs[3], k0, np.int32))

    def match_points(self, desc0_cn: torch.Tensor, desc1_cn: torch.Tensor, thr, mutual=True):
        """nn_matcher on [256,n] descriptors; returns (dist [n0,n1] device, match01 [n0] device)."""
        d0, d1 = self._f32(desc0_cn), self._f32(desc1_cn)
        n0, n1 = int(d0.shape[1]), int(d1.shape[1])
        dist = torch.empty((n0, n1), dtype=torch.float32, device=self.device)
        m01 = torch.full((n0,), -1, dtype=torch.int32, device=self.device)
        if n0 == 0 or n1 == 0:
            return dist, m01
        ws = self._workspace("match", self._L.linetr_match_points_workspace_bytes(n0, n1))
        nat.check(self._L.linetr_match_points(self._h, d0.data_ptr(), n0, d1.data_ptr(), n1, float(thr),
                                              int(bool(mutual)), dist.data_ptr(), m01.data_ptr(), ws.data_ptr(),
                                              ws.numel(), self._stream()), self._L)
        return dist, m01

    def superpoint_heads(self, score_logits: torch.Tensor = None, desc_raw: torch.Tensor = None, *, nhwc=True,
                         nchw=False, dense_dtype=None):
        """Fused SuperPoint head post-processing (models/superpoint.py:161-167, 190-193).

        score_logits [B,65,Hc,Wc] (convPb output) -> dense_score [B,8Hc,8Wc];
        desc_raw [B,256,Hc,Wc] (convDb output) -> L2-normalised descriptors as [B,Hc,Wc,256] (`nhwc`, the layout
        `describe_lines(..., dense_layout='nhwc')` consumes without a transposition pass) and/or [B,256,Hc,Wc]
        (`nchw`, the reference's 'dense_descriptor').  Returns (dense_score, desc_nhwc, desc_nchw), None where not
        requested.

        The raw head outputs are read in the type the convolutions produced: contiguous float16 / bfloat16 device tensors (a SuperPoint
        under autocast) in place, both heads in one type (a mixed pair is upcast to float32 together).  dense_dtype: the element type
        of the two descriptor maps, None / torch.float32 (the default), torch.float16 or torch.bfloat16; dense_score is float32 always."""
        out_bits = nat.dense_type_bits(dense_dtype or torch.float32)
        if out_bits is None:
            raise ValueError(f"dense_dtype must be None, torch.float32, torch.float16 or torch.bfloat16, got {dense_dtype}")
        typed, in_bits = self._dense_maps_typed([t for t in (score_logits, desc_raw) if t is not None])
        sl = typed[0] if score_logits is not None else None
        dr = typed[-1] if desc_raw is not None else None
        ref = sl if sl is not None else dr
        if ref is None:
            raise ValueError("superpoint_heads needs at least one head")
        B, _, Hc, Wc = (int(v) for v in ref.shape)
        if sl is not None and tuple(sl.shape) != (B, 65, Hc, Wc):
            raise ValueError(f"score_logits must be [B,65,Hc,Wc], got {tuple(sl.shape)}")
        if dr is not None and tuple(dr.shape) != (B, D, Hc, Wc):
            raise ValueError(f"desc_raw must be [B,{D},Hc,Wc], got {tuple(dr.shape)}")
        score = torch.empty((B, Hc * 8, Wc * 8), dtype=torch.float32, device=self.device) if sl is not None else None
        odt = dense_dtype or torch.float32
        o_nhwc = torch.empty((B, Hc, Wc, D), dtype=odt, device=self.device) if (dr is not None and nhwc) else None
        o_nchw = torch.empty((B, D, Hc, Wc), dtype=odt, device=self.device) if (dr is not None and nchw) else None
        with torch.cuda.device(self.device):     # a heads-only engine has no handle: the current device is used
            if in_bits or out_bits:
                nat.check(self._L.linetr_superpoint_heads_typed(self._h, ptr(sl), ptr(dr), in_bits, B, Hc, Wc, ptr(score), ptr(o_nhwc),
                                                                ptr(o_nchw), out_bits, self._stream()), self._L)
            else:
                nat.check(self._L.linetr_superpoint_heads(self._h, ptr(sl), ptr(dr), B, Hc, Wc, ptr(score), ptr(o_nhwc),
                                                          ptr(o_nchw), self._stream()), self._L)
        return score, o_nhwc, o_nchw

    def superpoint_heads_rows(self, score_rows: torch.Tensor = None, desc_rows: torch.Tensor = None, shape=None, *, nhwc=True,
                              nchw=False):
        """superpoint_heads for channel-last raw head outputs (linetr_superpoint_heads_rows): score_rows [B*Hc*Wc, 65] and desc_rows
        [B*Hc*Wc, 256], float32 on the device with contiguous columns (a row stride is taken as it is), `shape` = (B, Hc, Wc) -- what
        superpoint_encode returns.  Same outputs as superpoint_heads, bit for bit given the same values."""
        if score_rows is None and desc_rows is None:
            raise ValueError("superpoint_heads_rows needs at least one head")
        B, Hc, Wc = (int(v) for v in shape)

        def rows(t, width, what):
            if t is None:
                return None
            if t.device != self.device or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
                t = t.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(t.shape) != (B * Hc * Wc, width):
                raise ValueError(f"{what} must be [{B * Hc * Wc},{width}], got {tuple(t.shape)}")
            return t
        sl, dr = rows(score_rows, 65, "score_rows"), rows(desc_rows, D, "desc_rows")
        score = torch.empty((B, Hc * 8, Wc * 8), dtype=torch.float32, device=self.device) if sl is not None else None
        o_nhwc = torch.empty((B, Hc, Wc, D), dtype=torch.float32, device=self.device) if (dr is not None and nhwc) else None
        o_nchw = torch.empty((B, D, Hc, Wc), dtype=torch.float32, device=self.device) if (dr is not None and nchw) else None
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_superpoint_heads_rows(self._h, ptr(sl), sl.stride(0) if sl is not None else 0, ptr(dr),
                                                           dr.stride(0) if dr is not None else 0, B, Hc, Wc, ptr(score), ptr(o_nhwc),
                                                           ptr(o_nchw), self._stream()), self._L)
        return score, o_nhwc, o_nchw

    # ------------------------------------------------------------------ homography views (csrc/lt_warp.h; linetr_amd/homography.py)
    WARP_MODES = {"bilinear": 0, "nearest": 1}

    def warp_tiles(self):
        """((TH, TW) of the warp kernel, (TH, TW) of the erosion kernel) in pixels"""
        v = [C.c_int32() for _ in range(4)]
        nat.check(self._L.linetr_warp_tile(*(C.byref(x) for x in v)), self._L)
        return (v[0].value, v[1].value), (v[2].value, v[3].value)

    def _on_device(self, t, what):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise RuntimeError(f"{what} must be a tensor on the HIP device {self.device}; there is no CPU path")
        return t

    def warp_images(self, images: torch.Tensor, mat_dst_to_src, mode="bilinear", return_valid=False, out=None, out_valid=None):
        """Every image of a float32 [B,C,H,W] batch seen through its own homography, in one native call (linetr_warp_images):
        out[b, c, y, x] = images[b, c] at M_b (x, y, 1), in pixel coordinates.  mat_dst_to_src: [B,3,3] or one [3,3] for the whole
        batch, read on the host in float64 (a device tensor is copied, which waits for it; nothing else waits).  mode 'bilinear'
        (zero padding, F.grid_sample's align_corners=True in pixel units) or 'nearest'.  return_valid: also the uint8 [B,H,W] mask of
        the pixels whose nearest source pixel lies inside the image.  `out` / `out_valid`: write there instead of into new tensors."""
        if mode not in self.WARP_MODES:
            raise ValueError(f"mode must be one of {sorted(self.WARP_MODES)}, got {mode!r}")
        img = self._on_device(images, "images")
        if img.dim() != 4 or img.dtype != torch.float32:
            raise ValueError(f"images must be float32 [B,C,H,W], got {img.dtype} {tuple(img.shape)}")
        img = img.contiguous()
        B, Cn, H, W = (int(v) for v in img.shape)
        m = mat_dst_to_src.detach().cpu().numpy() if isinstance(mat_dst_to_src, torch.Tensor) else np.asarray(mat_dst_to_src)
        m = m.astype(np.float64).reshape(-1, 3, 3)
        m = np.ascontiguousarray(np.broadcast_to(m, (B, 3, 3)) if len(m) == 1 else m)
        if m.shape != (B, 3, 3):
            raise ValueError(f"{m.shape[0]} matrices for {B} images")
        if out is None:
            out = torch.empty_like(img)
        valid = out_valid
        if valid is None and return_valid:
            valid = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        for t, shape, dtype, what in ((out, (B, Cn, H, W), torch.float32, "out"), (valid, (B, H, W), torch.uint8, "out_valid")):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"{what} must be a contiguous {dtype} {shape} tensor on {self.device}")
        self._call("linetr_warp_images", img.data_ptr(), B, Cn, H, W, nat.np_ptr(m), self.WARP_MODES[mode], out.data_ptr(), ptr(valid))
        return (out, valid) if return_valid else out

    def erode_mask(self, mask: torch.Tensor, radius: int, out=None):
        """Binary erosion of a uint8 [B,H,W] (or [H,W]) device mask by the (2 radius + 1)^2 square of ones, outside the image counting as
        set (linetr_mask_erode): radius 2 is the dataset builder's cv2.erode(mask, np.ones((5, 5))).  Returns a new 0 / 1 mask."""
        mk = self._on_device(mask, "mask")
        if mk.dtype != torch.uint8 or mk.dim() not in (2, 3):
            raise ValueError(f"mask must be uint8 [B,H,W] or [H,W], got {mk.dtype} {tuple(mk.shape)}")
        mk = mk.contiguous()
        B, H, W = (1, *mk.shape) if mk.dim() == 2 else mk.shape
        if out is None:
            out = torch.empty_like(mk)
        if tuple(out.shape) != tuple(mk.shape) or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 {tuple(mk.shape)} tensor on {self.device}")
        self._call("linetr_mask_erode", mk.data_ptr(), int(B), int(H), int(W), int(radius), out.data_ptr())
        return out

    # ------------------------------------------------------------------ photometric augmentation (csrc/lt_photometric.h; linetr_amd/photometric.py)
    def photometric_tile(self):
        """dict of the photometric kernels' tiles in pixels: 'point' (TH, TW, halo), 'row' (TH, TW), 'col' (TH, TW), 'max_radius'"""
        v = [C.c_int32() for _ in range(8)]
        nat.check(self._L.linetr_photometric_tile(*(C.byref(x) for x in v)), self._L)
        v = [x.value for x in v]
        return {"point": tuple(v[0:3]), "row": tuple(v[3:5]), "col": tuple(v[5:7]), "max_radius": v[7]}

    def photometric_params(self, config, B, H, W, seed, first=0):
        """The drawn values of the images first .. first + B - 1 of an H x W batch as a NumPy record array (nat.PHOTO_PARAMS_DTYPE), by the
        host sampler linetr_photometric_sample.  config: a nat.PhotoConfig, or the reference's `augmentation` dict (homography.yaml)."""
        if not isinstance(config, nat.PhotoConfig):
            from .photometric import photo_config
            config = photo_config(config)
        params = np.zeros(int(B), nat.PHOTO_PARAMS_DTYPE)
        nat.check(self._L.linetr_photometric_sample(C.byref(config), int(seed), int(first), int(B), int(H), int(W), nat.np_ptr(params)), self._L)
        return params

    def _plane_batch(self, images, channels=None):
        img = self._on_device(images, "images")
        if img.dim() != 4 or img.dtype != torch.float32 or (channels is not None and img.shape[1] != channels):
            raise ValueError(f"images must be float32 [B,{channels or 'C'},H,W], got {img.dtype} {tuple(img.shape)}")
        return img.contiguous()

    def _like(self, out, img):
        if out is None:
            return torch.empty_like(img)
        if tuple(out.shape) != tuple(img.shape) or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {tuple(img.shape)} tensor on {self.device}")
        return out

    def photometric(self, images: torch.Tensor, params, seed, quantise_out=False, out=None, first=0):
        """The photometric stages of params[b] applied to image b of a float32 [B,1,H,W] batch in [0,1], in one native call
        (linetr_photometric; csrc/lt_photometric.h states every stage).  params: the record array of photometric_params (or planted
        values of the same dtype), read on the host.  Image b draws its per-pixel randomness with the key (seed, first + b).
        quantise_out: the builder's (... * 255).astype('uint8') / 255 of the result."""
        img = self._plane_batch(images, 1)
        B, _, H, W = (int(v) for v in img.shape)
        params = np.ascontiguousarray(params, dtype=nat.PHOTO_PARAMS_DTYPE)
        if params.shape != (B,):
            raise ValueError(f"{params.shape} parameter records for {B} images")
        out = self._like(out, img)
        ws = self._workspace("photo", self._L.linetr_photometric_workspace_bytes(B, 1, H, W))
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_photometric(self._h, img.data_ptr(), B, H, W, nat.np_ptr(params), int(seed), int(first), int(bool(quantise_out)),
                                                 out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return out

    def gaussian_blur(self, images: torch.Tensor, ksize, sigma=0.0, quantise=False, out=None):
        """The separable Gaussian of stage 6 alone on a float32 [B,C,H,W] batch (linetr_gaussian_blur): odd ksize <= 351 and sigma (0 =
        OpenCV's 0.3 ((ksize - 1) / 2 - 1) + 0.8), each one value or one per image; border reflect-101.  quantise: round to levels 0..255."""
        img = self._plane_batch(images)
        B, Cn, H, W = (int(v) for v in img.shape)
        ks = np.ascontiguousarray(np.broadcast_to(np.asarray(ksize, dtype=np.int32), (B,)))
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,)))
        out = self._like(out, img)
        ws = self._workspace("photo", self._L.linetr_photometric_workspace_bytes(B, Cn, H, W))
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_gaussian_blur(self._h, img.data_ptr(), B, Cn, H, W, nat.np_ptr(ks), nat.np_ptr(sg), int(bool(quantise)),
                                                   out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return out

    # ------------------------------------------------------------------ line segment detector (csrc/lt_linedet.h; linetr_amd/frontends)
    DETECT_DEFAULTS = {"n_octave": 2, "scale": 2, "grad_threshold": 28160, "min_region_size": 16, "density": 0.6}

    def detect_tile(self):
        """(TH, TW): the tile of the detector's gradient and labelling kernels in cells"""
        th, tw = C.c_int32(), C.c_int32()
        nat.check(self._L.linetr_detect_tile(C.byref(th), C.byref(tw)), self._L)
        return th.value, tw.value

    @classmethod
    def detect_config(cls, **config) -> nat.DetectConfig:
        """LinetrDetectConfig from the keys of DETECT_DEFAULTS (the reference's 'n_octave' / 'scale' and the detector's own three)"""
        unknown = set(config) - set(cls.DETECT_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown detector settings {sorted(unknown)}")
        c = {**cls.DETECT_DEFAULTS, **config}
        return nat.DetectConfig(int(c["n_octave"]), int(c["scale"]), int(c["grad_threshold"]), int(c["min_region_size"]), float(c["density"]))

    def _detect_images(self, images):
        """a device image batch as the detector takes it: contiguous [B,H,W], uint8 or float32"""
        img = self._on_device(images, "images")
        if img.dim() == 2:
            img = img[None]
        elif img.dim() == 4 and img.shape[1] == 1:
            img = img[:, 0]
        if img.dim() != 3:
            raise ValueError(f"images must be [B,H,W], [B,1,H,W] or [H,W], got {tuple(img.shape)}")
        if img.dtype != torch.uint8:
            if not img.dtype.is_floating_point:
                raise ValueError(f"images must be uint8 or floating point in [0,1], got {img.dtype}")
            img = img.to(torch.float32)
        return img.contiguous()

    def detect_lines(self, images, *, capacity=None, debug=False, **config):
        """The line segments of a device image batch [B,H,W] / [B,1,H,W] / [H,W], uint8 or float in [0,1], in one native call
        (linetr_detect_lines): (rows [K,6] float64 ndarray, offsets [B+1] int32), image b's rows at offsets[b]:offsets[b+1], each
        (startX, startY, endX, endY, lineLength, octave) -- what Engine.prefilter takes as (lines6, offsets=).  The pixels stay on the
        device; the host waits once, reads the counts from pinned memory and copies exactly the rows.  `capacity`: rows per image the
        first call has room for (default: what the largest image needed so far, at least 512); where an image holds more the call runs
        once more with room for all.  config: the keys of DETECT_DEFAULTS.  debug=True: also the int64 [K,10] region rows
        (octave, partition, label, n, sw, swx, swy, swxx, swxy, swyy) and the counts [B, n_octave]."""
        img = self._detect_images(images)
        B, H, W = (int(v) for v in img.shape)
        cfg = self.detect_config(**config)
        n_oct = cfg.n_octaves
        nbytes = self._L.linetr_detect_lines_workspace_bytes(B, H, W, n_oct)
        ws = self._workspace("detect_lines", max(int(nbytes), 256))
        pinned = self.__dict__.get("_detect_counts")
        if pinned is None or pinned.numel() < B * max(n_oct, 1):
            pinned = self.__dict__["_detect_counts"] = torch.empty(max(B * max(n_oct, 1), 64), dtype=torch.int32, pin_memory=True)
        cap = int(capacity) if capacity is not None else max(512, self.__dict__.get("_detect_cap", 0))
        for attempt in range(2):
            rows = torch.empty((B, cap, 6), dtype=torch.float64, device=self.device)
            dbg = torch.empty((B, cap, 10), dtype=torch.int64, device=self.device) if debug else None
            self._call("linetr_detect_lines", img.data_ptr(), int(img.dtype != torch.uint8), B, H, W, C.byref(cfg), cap, rows.data_ptr(),
                       pinned.data_ptr(), ptr(dbg), ws.data_ptr(), ws.numel())
            torch.cuda.current_stream(self.device).synchronize()
            counts = pinned[:B * n_oct].numpy().reshape(B, n_oct).copy()
            per_image = counts.sum(axis=1)
            if int(per_image.max()) <= cap:
                break
            cap = int(per_image.max())
        if capacity is None:
            self.__dict__["_detect_cap"] = max(cap, self.__dict__.get("_detect_cap", 0))
        offsets = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(per_image, out=offsets[1:])

        def gather(t):
            return (t[0, :int(per_image[0])] if B == 1 else torch.cat([t[b, :int(per_image[b])] for b in range(B)])).cpu().numpy()
        out = gather(rows)
        return (out, offsets, gather(dbg), counts) if debug else (out, offsets)

    def detect_debug_labels(self, buckets: torch.Tensor, out=None) -> torch.Tensor:
        """the labelling kernels alone: int8 [B,H,W] bucket maps (-1 = unused) -> int32 [B,H,W] labels (into `out` if given)"""
        bk = self._on_device(buckets, "buckets")
        if bk.dtype != torch.int8 or bk.dim() != 3:
            raise ValueError(f"buckets must be int8 [B,H,W], got {bk.dtype} {tuple(bk.shape)}")
        bk = bk.contiguous()
        B, H, W = (int(v) for v in bk.shape)
        ws = self._workspace("detect_labels", max(int(self._L.linetr_detect_debug_labels_workspace_bytes(B, H, W)), 256))
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.int32, device=self.device)
        if tuple(out.shape) != (B, H, W) or out.dtype != torch.int32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int32 {(B, H, W)} tensor on {self.device}")
        self._call("linetr_detect_debug_labels", bk.data_ptr(), B, H, W, out.data_ptr(), ws.data_ptr(), ws.numel())
        return out

    def detect_debug_gradient(self, images, octave=0, **config):
        """quantisation, pyramid and gradient kernel alone: (m2 int32, bucket A int8, bucket B int8), each [B, Ho - 1, Wo - 1] of `octave`"""
        img = self._detect_images(images)
        B, H, W = (int(v) for v in img.shape)
        cfg = self.detect_config(**config)
        Ho, Wo = H, W
        for _ in range(int(octave)):
            Ho, Wo = (Ho + 1) // 2, (Wo + 1) // 2
        shape = (B, Ho - 1, Wo - 1) if Ho >= 2 and Wo >= 2 else (B, 0, 0)
        m2 = torch.empty(shape, dtype=torch.int32, device=self.device)
        bka, bkb = (torch.empty(shape, dtype=torch.int8, device=self.device) for _ in range(2))
        ws = self._workspace("detect_lines", max(int(self._L.linetr_detect_lines_workspace_bytes(B, H, W, cfg.n_octaves)), 256))
        # an empty tensor has no address: the library wants non-NULL pointers even where it writes nothing
        dummy = torch.empty(16, dtype=torch.int32, device=self.device)
        p = (lambda t: t.data_ptr() if t.numel() else dummy.data_ptr())
        self._call("linetr_detect_debug_gradient", img.data_ptr(), int(img.dtype != torch.uint8), B, H, W, C.byref(cfg), int(octave), p(m2), p(bka),
                   p(bkb), ws.data_ptr(), ws.numel())
        return m2, bka, bkb

    # ------------------------------------------------------------------ native SuperPoint encoder (off by default everywhere)
    SP_CONV_NAMES = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb")

    def sp_conv_tile(self):
        """(TH, TW): the spatial tile of the 3x3 kernel in pixels"""
        th, tw = C.c_int32(), C.c_int32()
        nat.check(self._L.linetr_sp_conv3x3_tile(C.byref(th), C.byref(tw)), self._L)
        return th.value, tw.value

    def sp_conv3x3_pack(self, weight: torch.Tensor) -> torch.Tensor:
        """a state_dict weight [Cout,Cin,3,3] in the K order linetr_sp_conv3x3 walks"""
        w = self._f32(weight)
        cout, cin = int(w.shape[0]), int(w.shape[1])
        nbytes = self._L.linetr_sp_conv3x3_pack_bytes(cin, cout)
        if tuple(w.shape[2:]) != (3, 3) or nbytes == 0:
            raise ValueError(f"no native 3x3 layer for a weight of shape {tuple(w.shape)}")
        packed = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._L.linetr_sp_conv3x3_pack(w.data_ptr(), cin, cout, packed.data_ptr(), self._stream()), self._L)
        return packed

    def sp_conv3x3(self, x: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, pool=False, out: torch.Tensor = None):
        """One encoder layer alone (linetr_sp_conv3x3): x [B,H,W,Cin] channel-last -> relu(conv3x3 + bias) [B,H,W,Cout], or its 2x2
        maximum [B,H//2,W//2,Cout] with `pool`.  `out`: write there instead of into a new tensor (the unit tests' guarded buffers)."""
        B, H, W, cin = (int(v) for v in x.shape)
        cout = int(bias.numel())
        if out is None:
            out = torch.empty((B, H // 2, W // 2, cout) if pool else (B, H, W, cout), dtype=torch.float32, device=self.device)
        self._call("linetr_sp_conv3x3", x.data_ptr(), B, H, W, cin, packed.data_ptr(), bias.data_ptr(), cout, int(pool), out.data_ptr())
        return out

    def sp_conv1a(self, image: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out: torch.Tensor = None):
        """The first layer alone (linetr_sp_conv1a): image [B,1,H,W] -> relu(conv1a) [B,H,W,64], weight [64,1,3,3]."""
        B, _, H, W = (int(v) for v in image.shape)
        if out is None:
            out = torch.empty((B, H, W, 64), dtype=torch.float32, device=self.device)
        self._call("linetr_sp_conv1a", image.data_ptr(), B, H, W, weight.data_ptr(), bias.data_ptr(), out.data_ptr())
        return out

    def _sp_encoder(self, weights):
        """The native encoder with `weights` packed: a mapping name -> tensor holding '<conv>.weight' / '<conv>.bias' of SP_CONV_NAMES
        (a SuperPoint state_dict, or dict(module.named_parameters())).  Packed again when any of the 24 tensors has another address
        or version than at the last call."""
        ts = [weights[n + s] for s in (".weight", ".bias") for n in self.SP_CONV_NAMES]
        key = tuple((t.data_ptr(), t._version, t.device, t.dtype) for t in ts)
        st = self.__dict__.setdefault("_sp", {"enc": None, "key": None})
        if st["enc"] is None:
            enc = C.c_void_p()
            nat.check(self._L.linetr_sp_encoder_create(self.device.index, C.byref(enc)), self._L)
            st["enc"] = enc
        if st["key"] != key:
            ts32 = [self._f32(t.detach()) for t in ts]
            arr = lambda part: (C.c_void_p * 12)(*[t.data_ptr() for t in part])
            with torch.cuda.device(self.device):
                nat.check(self._L.linetr_sp_encoder_set_weights(st["enc"], arr(ts32[:12]), arr(ts32[12:]), self._stream()), self._L)
            for t in ts32:       # a converted copy is read by the packing kernels queued above: keep it until they have run
                t.record_stream(torch.cuda.current_stream(self.device))
            st["key"] = key
        return st["enc"]

    def superpoint_encode(self, image: torch.Tensor, weights, *, max_workspace_bytes=2 << 30, return_feat=False):
        """SuperPoint's shared encoder and the two head convolutions natively (linetr_sp_encoder_forward; the torch counterpart is
        FusedHeadSuperPoint.encode): image [B,1,H,W] float32 -> (score_rows [B*Hc*Wc,65], desc_rows [B*Hc*Wc,256], (B, Hc, Wc)), the
        raw head outputs as channel-last rows for superpoint_heads_rows (score_rows is a view with a row stride of 68 floats).  `weights`: see _sp_encoder.  The batch is cut into chunks
        of as many images as keep the workspace under max_workspace_bytes (at least one); every image's result is independent of the
        chunking.  No host wait.  return_feat: conv4b's output [B,Hc,Wc,128] as a fourth element (tests)."""
        img = self._f32(image)
        if img.dim() != 4 or int(img.shape[1]) != 1:
            raise ValueError(f"image must be [B,1,H,W], got {tuple(img.shape)}")
        B, _, H, W = (int(v) for v in img.shape)
        if H < 8 or W < 8:
            raise ValueError(f"the encoder needs at least 8 x 8 pixels, got {H} x {W}")
        Hc, Wc = H // 8, W // 8
        cells = Hc * Wc
        score = torch.empty((B * cells, 68), dtype=torch.float32, device=self.device)[:, :65]     # LINETR_SP_SCORE_LD: 16-byte aligned rows
        desc = torch.empty((B * cells, D), dtype=torch.float32, device=self.device)
        feat = torch.empty((B, Hc, Wc, 128), dtype=torch.float32, device=self.device) if return_feat else None
        if B > 0:
            enc = self._sp_encoder(weights)
            per_image = self._L.linetr_sp_encoder_workspace_bytes(1, H, W)
            n = max(1, min(B, int(max_workspace_bytes) // max(per_image, 1)))
            ws = self._workspace("sp_encoder", self._L.linetr_sp_encoder_workspace_bytes(n, H, W))
            with torch.cuda.device(self.device):
                for b0 in range(0, B, n):
                    nb = min(n, B - b0)
                    src = img[b0:b0 + nb]
                    if src.data_ptr() % 16:          # an odd H * W: a later chunk's first image is not 16-byte aligned inside the batch
                        src = src.clone()
                    nat.check(self._L.linetr_sp_encoder_forward(enc, src.data_ptr(), nb, H, W, score[b0 * cells:].data_ptr(),
                                                                desc[b0 * cells:].data_ptr(), ptr(feat[b0:]) if return_feat else None,
                                                                ws.data_ptr(), ws.numel(), self._stream()), self._L)
        return (score, desc, (B, Hc, Wc), feat) if return_feat else (score, desc, (B, Hc, Wc))

    def superpoint_keypoints(self, dense_score: torch.Tensor, dense_desc: torch.Tensor = None, *, nms_radius=4,
                             keypoint_threshold=0.005, remove_borders=4, max_keypoints=-1, align_corners=False,
                             dense_layout="nhwc"):
        """SuperPoint's key-point branch for a batch (models/superpoint.py:168-187, 195-197) in native calls: simple_nms,
        threshold, remove_borders, top_k_keypoints, (row, col) -> (x, y) and sample_descriptors.

        dense_score [B,H,W]; dense_desc [B,Hc,Wc,256] ('nhwc', what superpoint_heads emits) or [B,256,Hc,Wc] ('nchw'), float32 or (read
        in place) float16 / bfloat16, or None.
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
            dd, bits = self._dense_map(dense_desc)
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
                    wd = self._workspace("sample", self._L.linetr_point_descriptors_workspace_bytes(B, Hc, Wc, int(nhwc) | bits))
                    nat.check(self._L.linetr_point_descriptors(self._h, kp.data_ptr(), cu.data_ptr(), B, n_total, dd.data_ptr(), Hc, Wc,
                                                               int(bool(align_corners)), int(nhwc) | bits, desc.data_ptr(), wd.data_ptr(),
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
