"""The single-kernel surface of Engine (a mixin: engine.py declares `class Engine(_TrainSurface, _DebugSurface)` and holds the helpers
used here -- _call, _f32, _workspace, get_precision): one kernel or one path of the library alone (the debug_* entry points), the queries
that tell which kernel the forward pass would take, and their name tables.  For the unit tests and tools/ only; nothing of the product
path calls in here."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._shapes import D, ptr


class _DebugSurface:
    def debug_posenc(self, which: str, in0, in1, in2=None):
        """Layers 1-3 of the word ('word': points [rows,2], scores [rows]) or line ('line': sub-lines [rows,2,2],
        resp [rows], angles [rows,2]) positional encoder alone -> [rows,128] (unit tests of the fused MLP kernel)."""
        a, b = self._f32(in0), self._f32(in1)
        c = self._f32(in2) if in2 is not None else None
        rows = int(b.shape[0])
        out = torch.empty((rows, 128), dtype=torch.float32, device=self.device)
        self._call("linetr_debug_posenc", {"word": 0, "line": 1}[which], a.data_ptr(), b.data_ptr(), ptr(c), rows, out.data_ptr())
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
        self._call("linetr_debug_gemm", A.data_ptr(), A.stride(0), W.data_ptr(), ptr(b), ptr(r), Y.data_ptr(), Y.stride(0), M, N, K, int(act),
                   int(cache_weights))
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
        c = nat.GemmCase(A=ptr(A), lda=A.stride(0), A2=ptr(A2), lda2=A2.stride(0) if A2 is not None else 0, K1=K1 if A2 is not None else 0,
                         W=ptr(W), bias=ptr(b), R=ptr(residual), Y=ptr(out), ldy=out.stride(0), M=M, N=N, K=K, act=int(act),
                         groups=int(groups), gA=int(gA), gY=gY, norm=int(norm), gamma=ptr(ga), beta=ptr(be), add2=ptr(add2),
                         eps=float(eps), via_row_norm=int(bool(via_row_norm)), tile=self._gemm_tile_code(tile))
        used = C.c_int32(-1)
        self._call("linetr_debug_gemm_case", C.byref(c), C.byref(used))
        return (full if groups > 1 or full is out else out), self._gemm_tile_name(used.value)

    SIG_KERNELS = ("sig_attn", "sig_attn_small", "sig_attn_split4", "sig_attn_split8", "sig_qkv_attn")
    SIG_EIGHT_WAVES = 32         # LINETR_SIG_EIGHT_WAVES: added to 4 (forced only), sig_qkv_attn with eight compute waves at any size

    def sig_attention_kernel(self, cu_sub) -> int:
        """Which signature-attention kernel (index into SIG_KERNELS) the forward pass takes for a batch with these sub-line
        offsets at the current precision; nothing is launched."""
        cu = np.ascontiguousarray(np.asarray(cu_sub, dtype=np.int32))
        used = C.c_int32(-1)
        self._call("linetr_debug_sig_attention", -1, 0, None, 0, cu.ctypes.data, len(cu) - 1, None, C.byref(used))
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
        self._call("linetr_debug_sig_attention", int(kernel), int(layer), x.data_ptr(), x.stride(0), cu.ctypes.data, len(cu) - 1, msg.data_ptr(),
                   C.byref(used))
        return msg, used.value

    TOK_MLP_VARIANTS = ("tok_mlp_word", "tok_mlp_line", "tok_mlp_dual", "tok_mlp_seq", "mlp123_gemm_chain")

    def tok_mlp_variant(self, rows_word, rows_line) -> int:
        """Which launch (index into TOK_MLP_VARIANTS) the forward pass takes for the two positional encoders at these row counts
        and the current precision; nothing is launched."""
        used = C.c_int32(-1)
        self._call("linetr_debug_tok_mlp", -1, None, None, int(rows_word), None, None, None, int(rows_line), None, None, 0, C.byref(used))
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
        self._call("linetr_debug_tok_mlp", int(variant), pw[0], pw[1], rw, pl[0], pl[1], pl[2], rl, ptr(out_word), ptr(out_line), int(max_blocks),
                   C.byref(used))
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
        self._call("linetr_debug_bn_train", which, pz, rows, C_, ld, f32(gamma, C_, "gamma"), f32(beta, C_, "beta"), *ins,
                   f32(out, rows * e[3], "out") if which >= 0 else None, float(momentum), f32(running, n_stats, "running"),
                   f32(batch, n_stats, "batch"), f32(affine, n_stats, "affine"), C.byref(used), ws.data_ptr(), ws.numel())
        return res, used.value

    CLS_POOL_KERNELS = ("cls_pool", "cls_pool_online", "cls_pool_online_reverse", "cls_pool_online_split4")

    def cls_pool_kernel(self, N, dense=False) -> int:
        """Which pooling kernel (index into CLS_POOL_KERNELS) the forward pass takes for N sub-lines (dense: the [N, T] token
        tensors of linetr_forward instead of linetr_describe's compact token list); nothing is launched."""
        used = C.c_int32(-1)
        self._call("linetr_debug_cls_pool", -1, None, 0, None, int(N), 1, None, None, 0, 1, None, 1, 1, 1, 0, C.c_void_p(16) if dense else None,
                   None, C.byref(used))
        return used.value

    def debug_cls_pool(self, kernel, a4, out, N, T, *, recs=None, sub2line=None, cpnt=None, first_pad=0, n_images=1, dense_map=None,
                       nhwc=True, Hc=0, Wc=0, align_corners=False, desc_dense=None):
        """ONE CLS-pooling kernel alone (linetr_debug_cls_pool; diagnostics / unit tests).  kernel: -1 (the forward pass's choice)
        or an index into CLS_POOL_KERNELS.  Kernel 0 reads desc_dense [N, T, 256] and a4 [N * T, 256]; the online kernels the
        records `recs` (a uint8 device tensor holding LineRec[K]), sub2line [N] int32, cpnt [first_pad + n_images, 2], a4
        [first_pad + n_images, 256] and n_images maps of Hc x Wc cells (`nhwc`: channel-last, else NCHW; float32, or float16 / bfloat16
        read in place).  out: contiguous float32 [>= N, 4, 544].  Returns (out, kernel used)."""
        for t in (a4, out, cpnt, dense_map, desc_dense):
            if t is not None and (t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous()) and \
                    not (t is dense_map and nat.dense_type_bits(t.dtype) and t.device == self.device and t.is_contiguous()):
                raise ValueError("contiguous float32 tensors (dense_map: or float16 / bfloat16) on the engine's device expected")
        bits = nat.dense_type_bits(dense_map.dtype) if dense_map is not None else 0
        if out.numel() < N * 4 * 544:
            raise ValueError("out is smaller than [N, 4, 544]")
        if desc_dense is None:
            if recs.dtype != torch.uint8 or sub2line.dtype != torch.int32 or sub2line.numel() < N:
                raise ValueError("recs: uint8 bytes of LineRec[K]; sub2line: int32 [N]")
            if a4.numel() < (first_pad + n_images) * D or cpnt.numel() < (first_pad + n_images) * 2 or dense_map.numel() < n_images * Hc * Wc * D:
                raise ValueError("a4 / cpnt / dense_map are smaller than first_pad + n_images rows / n_images maps")
        elif a4.numel() < N * T * D or desc_dense.numel() < N * T * D:
            raise ValueError("a4 / desc_dense are smaller than [N * T, 256]")
        used = C.c_int32(-1)
        self._call("linetr_debug_cls_pool", int(kernel), ptr(recs), recs.numel() // nat.REC_DTYPE.itemsize if recs is not None else 0,
                   ptr(sub2line), int(N), int(T), ptr(cpnt), ptr(a4), int(first_pad), int(n_images), ptr(dense_map), int(bool(nhwc)) | bits, int(Hc),
                   int(Wc), int(bool(align_corners)), ptr(desc_dense), ptr(out), C.byref(used))
        return out, used.value

    STAGES = ("tail", "sig")
    SIG_FOLD_NEXT = 8            # LINETR_STAGE_FOLD_NEXT: added to an index into SIG_KERNELS in debug_stage's `plan`

    def debug_stage(self, stage, in0, in1=None, cu_sub=None, plan=-1, outs=(None, None, None)):
        """ONE stage from the middle of the forward pass alone (linetr_debug_stage; diagnostics / unit tests), by the host functions
        the forward pass calls.  'tail': in0 = pooled [>= N, 4, 544], in1 = line_pos [>= N, 256], N = cu_sub (an int here);
        outs = (att, o, zA), each [>= N, 256] or None.  'sig': in0 = z0 [>= N, 256], cu_sub the images' prefix sums; outs =
        (line_desc [>= N, 256], taps [>= L - 1, N, 256] or None, None); plan: -1 (the forward pass's choice) or an index into
        SIG_KERNELS (+ SIG_FOLD_NEXT).  Tensors are contiguous float32 on the engine's device and go to the library as they are.
        Returns the plan that ran (-1 for the tail)."""
        sig = self.STAGES.index(stage) == 1
        cu = np.ascontiguousarray(np.asarray(cu_sub, dtype=np.int32)) if sig else None
        N = (int(cu[-1]) if len(cu) else 0) if sig else int(cu_sub)
        n_taps = max(int(self.cfg["n_sig_layers"]) - 1, 0)
        need = (N * D, 0, N * D, N * n_taps * D, 0) if sig else (N * 4 * 544, N * D, N * D, N * D, N * D)
        for t, n in zip((in0, in1, *outs), need):
            if t is not None and (t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"contiguous float32 tensors of at least {n} elements on the engine's device expected")
        n_images = len(cu) - 1 if sig else 1
        ws = self._workspace("stage", max(self._L.linetr_debug_stage_workspace_bytes(self._h, N, n_images), 0))
        used = C.c_int32(-1)
        self._call("linetr_debug_stage", int(sig), N, ptr(in0), ptr(in1), cu.ctypes.data if sig else None, n_images, int(plan),
                   ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), C.byref(used), ws.data_ptr(), ws.numel())
        return used.value

    MATCH_PATHS = ("pair_dist + pair_pool + pair_final", "pair_match_fused<false>", "pair_match_fused<true>")

    def match_path(self, dims) -> int:
        """Which path (index into MATCH_PATHS) linetr_match takes for pairs of these dims [P, 4] = (n0, k0, n1, k1); nothing is
        launched."""
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1, 4)
        used = C.c_int32(-1)
        self._call("linetr_debug_match", len(dims), dims.ctypes.data, None, None, None, None, None, None, 0.0, 0, None, None, None, None, None, 0,
                   -1, -1, -1, -1, C.byref(used))
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
        used = C.c_int32(-1)
        self._call("linetr_debug_match", P, dims.ctypes.data, ptr(desc0), offs[0].ctypes.data, ptr(s2l0), ptr(desc1), offs[2].ctypes.data,
                   ptr(s2l1), float(thr), int(bool(mutual)), ptr(dk), offs[1].ctypes.data, ptr(m01), offs[3].ctypes.data, ws.data_ptr(),
                   ws.numel(), int(path), int(seg1_global), int(cache_dk), int(device_table), C.byref(used))
        return used.value

    # ------------------------------------------------------------------ split-tile operands (csrc/lt_st_image.h; the GEMM on them: experiments/csrc/lt_gemm_st.h)
    def to_st(self, X):
        """fp32 [rows, K] -> ST image (uint8 tensor); K % 32 == 0."""
        X = self._f32(X)
        rows, K = X.shape
        out = torch.empty(int(self._L.linetr_st_bytes(rows, K)), dtype=torch.uint8, device=self.device)
        self._call("linetr_debug_to_st", X.data_ptr(), X.stride(0), rows, K, out.data_ptr())
        return out

    def from_st(self, st, rows, K):
        X = torch.empty((rows, K), dtype=torch.float32, device=self.device)
        self._call("linetr_debug_from_st", st.data_ptr(), rows, K, X.data_ptr(), K)
        return X

    def gemm_st(self, A1, K1, W, M, N, A2=None, K2=0, bias=None, residual=None, act=0, out_st=None, out=None):
        """act([A1 | A2] W^T + bias) (+ residual) on ST images; returns the ST image `out_st` or the fp32 matrix `out`."""
        b = self._f32(bias) if bias is not None else None
        self._call("linetr_debug_gemm_st", A1.data_ptr(), K1, ptr(A2), K2, W.data_ptr(), ptr(b), ptr(residual), ptr(out_st), ptr(out),
                   out.stride(0) if out is not None else 0, M, N, int(act))
        return out_st if out_st is not None else out
