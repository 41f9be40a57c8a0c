"""Photometric augmentation on the device: the distortions of the reference's dataset builder (dataloaders/build_homography_dataset.py:105-121,
154-158) under the reference's names (dataloaders/utils/photometric.py: ImgAugTransform, customizedTransform), taking the reference's
config dict.  One native call per batch (Engine.photometric / linetr_photometric; csrc/lt_photometric.h states every stage and the
deviations from imgaug / OpenCV).  Inputs must live on a HIP device: there is no CPU path.  Every call takes an explicit `seed`; image b
of a batch draws with the key (seed, first + b), so the same seed gives the same bits and a batch gives each image what it gets alone."""
from __future__ import annotations

import torch

from . import _native as nat
from .homography import _device_of, _engine, homography_views


def photo_config(augmentation) -> nat.PhotoConfig:
    """LinetrPhotoConfig from the reference's `augmentation` dict (homography.yaml: augmentation.photometric.enable / .params)"""
    ph = augmentation["photometric"]
    prm = ph["params"] if ph.get("enable", False) else {}
    c = nat.PhotoConfig()
    c.stages, c.max_kernel_size = 0, 3
    c.strength_range[:] = (1.0, 1.0)
    c.kernel_size_range[:] = (1, 2)
    S = nat.PHOTO_STAGES
    if prm.get("random_brightness"):
        c.stages |= S["brightness"]
        c.max_abs_change = int(prm["random_brightness"]["max_abs_change"])
    if prm.get("random_contrast"):
        c.stages |= S["contrast"]
        c.strength_range[:] = [float(v) for v in prm["random_contrast"]["strength_range"]]
    if prm.get("additive_gaussian_noise"):
        c.stages |= S["noise"]
        c.stddev_range[:] = [float(v) for v in prm["additive_gaussian_noise"]["stddev_range"]]
    if prm.get("additive_speckle_noise"):
        c.stages |= S["impulse"]
        c.prob_range[:] = [float(v) for v in prm["additive_speckle_noise"]["prob_range"]]
    if prm.get("motion_blur"):
        c.stages |= S["motion"]
        c.max_kernel_size = int(prm["motion_blur"]["max_kernel_size"])
    if prm.get("GaussianBlur"):
        c.stages |= S["blur"]
        c.blur_sigma = float(prm["GaussianBlur"]["sigma"])
    if prm.get("additive_shade"):
        sh = prm["additive_shade"]          # the defaults of customizedTransform.additive_shade
        c.stages |= S["shade"]
        c.nb_ellipses = int(sh.get("nb_ellipses", 20))
        c.transparency_range[:] = [float(v) for v in sh.get("transparency_range", (-0.5, 0.8))]
        c.kernel_size_range[:] = [int(v) for v in sh.get("kernel_size_range", (250, 350))]
    return c


def _as_batch(img):
    """a device image [H,W], [H,W,1] or [B,1,H,W], float in [0,1] or uint8, as float32 [B,1,H,W] in [0,1], and how to shape the result back"""
    _device_of(img, "img")
    shape = tuple(img.shape)
    if img.dim() == 3 and shape[2] == 1:
        img = img[:, :, 0]
    if img.dim() == 2:
        img = img[None, None]
    if img.dim() != 4 or img.shape[1] != 1:
        raise ValueError(f"img must be [H,W], [H,W,1] or [B,1,H,W], got {shape}")
    img = img.to(torch.float32) / 255.0 if img.dtype == torch.uint8 else img.to(torch.float32)
    return img.contiguous(), shape


def _run(img, config, stage_mask, seed, first, quantise_out=False):
    batch, shape = _as_batch(img)
    eng = _engine(batch.device)
    B, _, H, W = batch.shape
    cfg = photo_config(config)
    cfg.stages &= stage_mask
    params = eng.photometric_params(cfg, B, H, W, seed, first)
    return eng.photometric(batch, params, seed, quantise_out=quantise_out, first=first).view(shape)


_SHADE = nat.PHOTO_STAGES["shade"]


class ImgAugTransform:
    """photometric.py:9-76: brightness, contrast, Gaussian noise, impulse noise, motion blur and Gaussian blur as the config enables them,
    on levels 0..255; returns float32 in [0,1] shaped like the input.  The reference's motion_blur branch appends the PREVIOUS augmenter
    again for max_kernel_size > 3 (a bug); its evident intent is implemented: an odd K up to the maximum, applied with probability 0.5."""

    def __init__(self, **config):
        self.config = config

    def __call__(self, img, seed, first=0):
        return _run(img, self.config, ~_SHADE, seed, first)


class customizedTransform:
    """photometric.py:81-115: the additive shade when config['photometric']['params']['additive_shade'] is set, else the input (both
    pass through the 0..255 levels: an input k / 255 comes back as itself)."""

    def __init__(self):
        pass

    def __call__(self, img, seed, first=0, **config):
        return _run(img, config, _SHADE, seed, first)


def augment(images, config, seed, first=0, quantise_out=True):
    """ImgAugTransform followed by customizedTransform in ONE native call: float32 [B,1,H,W] (or what the classes accept) in, the same
    shape out.  quantise_out: the builder's (... * 255).astype('uint8') of line 157, returned as level / 255."""
    return _run(images, config, -1, seed, first, quantise_out)


def augmented_views(images, m_pix, config, seed, erosion_radius=2):
    """A training pair per image as the dataset builder makes it: the photometric augmentation of `images` (float32 [B,1,H,W] in [0,1]
    on the device), then homography_views of the AUGMENTED batch.  Like the builder, the second view is the warp of the augmented first
    view: build_homography_dataset.py:165 overwrites the separately augmented copy of line 158 with gray0, so only one augmentation
    reaches a pair.  Returns (image0, image1, valid_mask1)."""
    image0 = augment(images, config, seed)
    image1, valid = homography_views(image0, m_pix, erosion_radius)
    return image0, image1, valid
