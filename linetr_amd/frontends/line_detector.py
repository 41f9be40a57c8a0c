"""The surface of the reference's models/line_detector.py:11-28 (LSD(config).detect / detect_torch) on the native line segment detector
(Engine.detect_lines / linetr_detect_lines, csrc/lt_linedet.h).  It is NOT OpenCV's LSD: it is a detector of the same family whose every
step is independent of any processing order, so its lines differ from cv2's.  Images must live on a HIP device (a uint8
ndarray is uploaded); the pixels never come back to the host, only the rows do."""
from __future__ import annotations

import math

import numpy as np
import torch


class KeyLine:
    """The fields of cv2.line_descriptor.KeyLine that a detector fills.  linetr_amd.line_process reads startPointX/Y, endPointX/Y,
    lineLength and octave.  lineLength and the *InOctave points are in pixels of the line's octave, the rest in pixels of the image."""
    __slots__ = ("startPointX", "startPointY", "endPointX", "endPointY", "sPointInOctaveX", "sPointInOctaveY", "ePointInOctaveX",
                 "ePointInOctaveY", "lineLength", "octave", "numOfPixels", "angle", "response", "size", "pt", "class_id")

    def __init__(self, row, class_id, extent):
        sx, sy, ex, ey, length, octave = (float(v) for v in row)
        s = 2.0 ** octave
        self.startPointX, self.startPointY, self.endPointX, self.endPointY = sx, sy, ex, ey
        self.sPointInOctaveX, self.sPointInOctaveY, self.ePointInOctaveX, self.ePointInOctaveY = sx / s, sy / s, ex / s, ey / s
        self.lineLength, self.octave = length, int(octave)
        self.numOfPixels = int(math.floor(length)) + 1
        self.angle = math.atan2(ey - sy, ex - sx)
        self.response = length / extent           # cv2: the line's length over the larger extent of its octave image
        self.size = abs(ex - sx) * abs(ey - sy)
        self.pt = ((sx + ex) / 2.0, (sy + ey) / 2.0)
        self.class_id = int(class_id)

    def __repr__(self):
        return (f"KeyLine(({self.startPointX:.2f}, {self.startPointY:.2f}) -> ({self.endPointX:.2f}, {self.endPointY:.2f}), "
                f"octave {self.octave}, length {self.lineLength:.2f})")


class LSD:
    default_config = {
        'n_octave': 2,
        'scale': 2,
        'grad_threshold': 28160,      # on gx^2 + gy^2 of the 2 x 2 cell of the 16-fold smoothed image: LSD's rho at 22.5 degrees
        'min_region_size': 16,
        'density': 0.6,
    }

    def __init__(self, config=None, device=None):
        """device: where a host ndarray handed to detect() is uploaded (default: the current HIP device)"""
        self.config = {**self.default_config, **(config or {})}
        unknown = set(self.config) - set(self.default_config)
        if unknown:
            raise ValueError(f"unknown LSD settings {sorted(unknown)}")
        if self.config['scale'] != 2:
            raise ValueError("LSD: only scale 2 is supported")
        self.device = device

    def _engine(self, device):
        from ..homography import _engine
        return _engine(device)

    def _as_batch(self, image):
        """any of the reference's shapes ([H,W], [1,H,W], [1,1,H,W], [B,1,H,W]) as a device tensor [B,H,W]"""
        if isinstance(image, np.ndarray):
            dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            image = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
        if not isinstance(image, torch.Tensor) or image.device.type != "cuda":
            raise RuntimeError("LSD: the image must be an ndarray or a tensor on a HIP device (torch device 'cuda:N'); there is no CPU path")
        while image.dim() > 3 and image.shape[1] == 1:
            image = image.squeeze(1)
        if image.dim() == 2:
            image = image[None]
        if image.dim() != 3:
            raise ValueError(f"LSD: cannot read an image of shape {tuple(image.shape)} as gray images")
        return image

    def detect_batch(self, images):
        """(rows [K,6] float64 ndarray, offsets [B+1] int32) of a device batch [B,1,H,W] / [B,H,W], uint8 or float in [0,1]: the form
        Engine.prefilter takes (lines6=rows, offsets=offsets).  No Python object per line."""
        img = self._as_batch(images)
        return self._engine(img.device).detect_lines(img, **self.config)

    def _keylines(self, image, single):
        img = self._as_batch(image)
        if single and img.shape[0] != 1:
            raise ValueError(f"LSD: one image expected, got a batch of {img.shape[0]}")
        rows, _ = self._engine(img.device).detect_lines(img, **self.config)
        H, W = int(img.shape[-2]), int(img.shape[-1])
        extent = {}
        h, w = H, W
        for o in range(int(self.config['n_octave'])):
            extent[o] = float(max(h, w))
            h, w = (h + 1) // 2, (w + 1) // 2
        return [KeyLine(r, i, extent[int(r[5])]) for i, r in enumerate(rows)]

    def detect(self, image):
        """image: uint8 [H,W] ndarray or device tensor"""
        return self._keylines(image, True)

    def detect_torch(self, image):
        """image: float tensor in [0,1] on a HIP device, any of the reference's shapes; quantised on the device as the reference does on
        the host, uint8(image * 255)"""
        return self._keylines(image, True)
