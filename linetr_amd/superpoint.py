"""SuperPoint with the fused head producer.

`FusedHeadSuperPoint(sp)` wraps an existing SuperPoint module -- the reference's `models.superpoint.SuperPoint`,
unchanged, or anything with the same conv attributes -- and returns the same dict from `forward`
(models/superpoint.py:146-201), but computes the two dense maps with `linetr_superpoint_heads`:

    softmax / drop dustbin / depth-to-space  (superpoint.py:161-167)   -> 'dense_score'
    F.normalize over channels                (superpoint.py:190-193)   -> 'dense_descriptor' (NCHW, as the reference)
                                                                        + 'dense_descriptor_nhwc' [B,Hc,Wc,256]

The extra NHWC key is the layout the line tokeniser samples from, so `Engine.describe_lines(...,
dense_layout='nhwc')` skips its NCHW->NHWC pass.  The convolutions stay in PyTorch (MIOpen).  Key-point extraction
(`simple_nms`, `remove_borders`, `top_k_keypoints`, `sample_descriptors`) is delegated to the wrapped module's own
module-level functions, image by image, unless `native_keypoints=True`: then it is one `Engine.superpoint_keypoints`
call for the batch (`linetr_superpoint_keypoints` + `linetr_point_descriptors`), fed the channel-last map the heads call
has just produced -- same key points and scores bit for bit, one host wait per batch instead of one per image.

Half precision: the raw head outputs are read in the type the convolutions produced, so a wrapped module in `.half()` / `.bfloat16()`
(or run under `torch.autocast`) costs no float32 copy.  `dense_dtype=None` writes float32 maps from them; `dense_dtype=torch.float16`
or `torch.bfloat16` writes half 'dense_descriptor' / 'dense_descriptor_nhwc' (the float32 values rounded to nearest-even), which the
line tokeniser, `Engine.describe*` and the native key-point branch read in place, and 'descriptors' follows that type as the wrapped
module's would.  'dense_score', key points and scores are float32 always.
"""
from __future__ import annotations

import sys

import torch
from torch import nn


class FusedHeadSuperPoint(nn.Module):
    def __init__(self, superpoint: nn.Module, engine=None, helpers=None, want_nchw: bool = True,
                 native_keypoints: bool = False, align_corners=None, native_encoder: bool = False, dense_dtype=None):
        super().__init__()
        if dense_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"dense_dtype must be None, torch.float32, torch.float16 or torch.bfloat16, got {dense_dtype}")
        if native_encoder and dense_dtype in (torch.float16, torch.bfloat16):
            raise ValueError("native_encoder=True writes float32 maps only (its channel-last producer has no half output)")
        self.dense_dtype = None if dense_dtype == torch.float32 else dense_dtype
        self.sp = superpoint
        self.config = superpoint.config
        self.want_nchw = want_nchw
        self.native_keypoints = bool(native_keypoints)
        self.native_encoder = bool(native_encoder)
        # grid_sample flag of the native descriptor lookup; None = the reference's own version switch (superpoint.py:88)
        self.align_corners = align_corners
        self._engine = engine
        # simple_nms / remove_borders / top_k_keypoints / sample_descriptors of the wrapped implementation
        self._fn = helpers if helpers is not None else sys.modules[type(superpoint).__module__]

    def engine(self):
        if self._engine is None:
            from .engine import Engine
            dev = next(self.sp.parameters()).device
            self._engine = Engine.heads_only(dev)
        return self._engine

    def encode(self, image):
        """shared encoder + the two head convolutions (superpoint.py:148-160, 188-189): raw head outputs."""
        sp, relu = self.sp, self.sp.relu
        x = relu(sp.conv1a(image)); x = relu(sp.conv1b(x)); x = sp.pool(x)
        x = relu(sp.conv2a(x)); x = relu(sp.conv2b(x)); x = sp.pool(x)
        x = relu(sp.conv3a(x)); x = relu(sp.conv3b(x)); x = sp.pool(x)
        x = relu(sp.conv4a(x)); x = relu(sp.conv4b(x))
        return sp.convPb(relu(sp.convPa(x))), sp.convDb(relu(sp.convDa(x)))

    def _dense_maps_native(self, image):
        """The dense maps through the native encoder: no autograd graph, so a trainable encoder under enabled grad is refused."""
        params = dict(self.sp.named_parameters())
        eng = self.engine()
        if torch.is_grad_enabled() and any(params[n + s].requires_grad for n in eng.SP_CONV_NAMES for s in (".weight", ".bias")):
            raise RuntimeError("FusedHeadSuperPoint(native_encoder=True) is inference only: an encoder parameter requires grad. Call it "
                               "under torch.no_grad(), freeze the encoder, or use native_encoder=False.")
        with torch.no_grad():
            score_rows, desc_rows, shape = eng.superpoint_encode(image, params)
            return eng.superpoint_heads_rows(score_rows, desc_rows, shape, nhwc=True, nchw=self.want_nchw) + (shape[1], shape[2])

    def forward(self, data):
        if self.native_encoder:
            dense_score, d_nhwc, d_nchw, hc, wc = self._dense_maps_native(data["image"])
        else:
            score_logits, desc_raw = self.encode(data["image"])
            dense_score, d_nhwc, d_nchw = self.engine().superpoint_heads(score_logits, desc_raw, nhwc=True,
                                                                         nchw=self.want_nchw, dense_dtype=self.dense_dtype)
            hc, wc = int(score_logits.shape[2]), int(score_logits.shape[3])
        if d_nchw is None:                       # a view with the reference's shape (not contiguous)
            d_nchw = d_nhwc.permute(0, 3, 1, 2)
        if self.native_keypoints:
            keypoints, scores, descriptors = self._keypoints_native(dense_score, d_nhwc)
        else:
            # (the wrapped module's grid_sample cannot mix a half map with its float32 grid: it is handed a float32 tensor made by torch)
            keypoints, scores, descriptors = self._keypoints(dense_score, d_nchw if self.dense_dtype is None else d_nchw.float(),
                                                             hc * 8, wc * 8)
        if self.dense_dtype is not None:
            descriptors = [d.to(self.dense_dtype) for d in descriptors]
        return {"keypoints": keypoints, "scores": scores, "descriptors": descriptors, "dense_descriptor": d_nchw,
                "dense_score": dense_score, "dense_descriptor_nhwc": d_nhwc}

    def _keypoints(self, dense_score, dense_desc, height, width):
        """Key-point branch of the wrapped implementation (superpoint.py:168-187, 195-197), image by image, through its
        own helpers: NMS, threshold, border removal, optional top-k, (row, col) -> (x, y), descriptor sampling."""
        fn, cfg = self._fn, self.config
        nms = fn.simple_nms(dense_score, cfg["nms_radius"])
        kps, scs, descs = [], [], []
        for b in range(nms.shape[0]):
            rc = torch.nonzero(nms[b] > cfg["keypoint_threshold"])
            val = nms[b][rc[:, 0], rc[:, 1]]
            rc, val = fn.remove_borders(rc, val, cfg["remove_borders"], height, width)
            if cfg["max_keypoints"] >= 0:
                rc, val = fn.top_k_keypoints(rc, val, cfg["max_keypoints"])
            xy = rc.flip(1).float()
            kps.append(xy)
            scs.append(val)
            descs.append(fn.sample_descriptors(xy[None], dense_desc[b][None], 8)[0])
        return kps, tuple(scs), descs

    def _keypoints_native(self, dense_score, dense_desc_nhwc):
        """The same branch for the whole batch on the device (Engine.superpoint_keypoints); same containers as _keypoints."""
        cfg = self.config
        align = self.align_corners if self.align_corners is not None else int(torch.__version__[2]) > 2
        kps, scs, descs = self.engine().superpoint_keypoints(
            dense_score, dense_desc_nhwc, nms_radius=cfg["nms_radius"], keypoint_threshold=cfg["keypoint_threshold"],
            remove_borders=cfg["remove_borders"], max_keypoints=cfg["max_keypoints"], align_corners=align, dense_layout="nhwc")
        return kps, tuple(scs), descs
