"""Homography views on the device: the step of the reference's dataset builder between "an image" and "a training pair"
(dataloaders/build_homography_dataset.py:123-127, 164-167, 179-184) and the warping functions of dataloaders/utils/utils.py
(:317-370 inv_warp_image_batch / inv_warp_image, :677-704 compute_valid_mask) under the reference's names.  One native call warps a
batch and writes its valid mask (Engine.warp_images / linetr_warp_images), one erodes the mask (Engine.erode_mask /
linetr_mask_erode); no [B,H,W,2] grid exists and the mask never leaves the device.  Inputs must live on a HIP device: there is no
CPU path.  uint8 images are converted by the caller."""
from __future__ import annotations

import numpy as np
import torch

_engines = {}


def _engine(device):
    """one weight-less Engine per device for the module-level functions"""
    from .engine import Engine, _hip_device
    device = _hip_device(device)
    if device not in _engines:
        _engines[device] = Engine.heads_only(device)
    return _engines[device]


def _device_of(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what} must be a tensor on a HIP device (torch device 'cuda:N'); there is no CPU path")
    return t.device


def _host_f64(m):
    m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    return m.astype(np.float64)


def normalised_to_pixel(mat, height, width):
    """The reference's NORMALISED homographies (its linspace(-1, 1, W) / align_corners=True convention: pixel x <-> 2 x / (W - 1) - 1)
    as pixel homographies, float64: P^-1 mat P with P the pixel -> normalised map.  An extent of 1 sits at -1, as linspace puts it."""
    mat = _host_f64(mat).reshape(-1, 3, 3)
    sx, sy = (width - 1) / 2.0, (height - 1) / 2.0
    to_pix = np.array([[sx, 0.0, sx], [0.0, sy, sy], [0.0, 0.0, 1.0]])
    to_norm = np.array([[1.0 / sx if sx else 0.0, 0.0, -1.0], [0.0, 1.0 / sy if sy else 0.0, -1.0], [0.0, 0.0, 1.0]])
    return to_pix @ mat @ to_norm


def scale_homography(H, shape, shift=(-1, -1)):
    """build_homography_dataset.py:123-127: a homography sampled on the square [shift, shift + 2]^2 rescaled to the pixels of an image
    of `shape` = (height, width): inv(trans) @ H @ trans, float64."""
    height, width = shape[0], shape[1]
    trans = np.array([[2. / width, 0., shift[0]], [0., 2. / height, shift[1]], [0., 0., 1.]])
    return np.linalg.inv(trans) @ np.asarray(H, dtype=np.float64) @ trans


def inv_warp_image_batch(img, mat_homo_inv, device='cpu', mode='bilinear'):
    """utils.py:317-351 with its signature, shapes and dtype: img [B,C,H,W] (or [H,W] / [H,W,1], viewed as [1,1,H,W]) sampled through
    the NORMALISED matrices mat_homo_inv [B,3,3] (or one [3,3]) that take a destination point to its source point; bilinear or
    nearest, zero padding.  Returns float32 [B,C,H,W] on img's device.  `device` is accepted and ignored: img decides, and it must be
    a HIP device."""
    dev = _device_of(img, "img")
    if len(img.shape) == 2 or len(img.shape) == 3:
        img = img.view(1, 1, img.shape[0], img.shape[1])
    _, _, H, W = img.shape
    return _engine(dev).warp_images(img.float(), normalised_to_pixel(mat_homo_inv, H, W), mode=mode)


def inv_warp_image(img, mat_homo_inv, device='cpu', mode='bilinear'):
    """utils.py:353-370: inv_warp_image_batch of one image, squeezed to [H,W]"""
    return inv_warp_image_batch(img, mat_homo_inv, device, mode).squeeze()


def compute_valid_mask(image_shape, inv_homography, device='cpu', erosion_radius=0):
    """utils.py:677-704: the float32 [B,H,W] mask (1 = valid) of the pixels of a view of `image_shape` = (H, W) whose nearest source
    pixel under the NORMALISED inv_homography [B,3,3] (or [3,3]) lies inside the image, eroded by erosion_radius.  `device` must
    name a HIP device.

    Deviation from the reference: the erosion uses the (2 r + 1)^2 SQUARE of ones, the element of the dataset builder's own
    cv2.erode(mask, np.ones((5, 5))) at r = 2.  The reference's cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (2 r, 2 r)) needs
    OpenCV, which this package does not depend on and whose version the reference does not pin.  erosion_radius = 0 is the
    reference's result."""
    eng = _engine(device)
    H, W = int(image_shape[0]), int(image_shape[1])
    m = normalised_to_pixel(inv_homography, H, W)
    ones = torch.ones((len(m), 1, H, W), dtype=torch.float32, device=eng.device)
    _, valid = eng.warp_images(ones, m, mode="nearest", return_valid=True)
    if erosion_radius > 0:
        valid = eng.erode_mask(valid, int(erosion_radius))
    return valid.to(torch.float32)


def homography_views(images, m_pix, erosion_radius=2):
    """The second view of every image of a float32 [B,C,H,W] device batch and its valid mask, as the dataset builder makes them
    (build_homography_dataset.py:164-167, 179-184).  m_pix: B pixel homographies x1 ~ M x0 taking image-0 pixels to image-1 pixels
    (workloads.synth.pixel_homography's convention); like the builder's cv2.warpPerspective the view is sampled through the
    INVERSE, image1(x1) = image0(M^-1 x1), bilinear with zero padding.

    Returns (image1 [B,C,H,W] float32, valid_mask1 [B,H,W] uint8), both on the device.  The mask comes from GEOMETRY: a pixel is
    valid when its nearest source pixel lies inside image 0, eroded by the (2 erosion_radius + 1)^2 square (the builder's 5 x 5
    at the default).  The builder instead tests "all three channels of the warped image are 0", which also marks genuinely black
    pixels of the scene invalid; that is not reproduced."""
    dev = _device_of(images, "images")
    eng = _engine(dev)
    inv = np.linalg.inv(_host_f64(m_pix).reshape(-1, 3, 3))
    image1, valid = eng.warp_images(images, inv, mode="bilinear", return_valid=True)
    if erosion_radius > 0:
        valid = eng.erode_mask(valid, int(erosion_radius))
    return image1, valid


def prefilter_mask(valid_mask, image=0):
    """One image's valid mask as Engine.prefilter takes it (valid_masks=[...]): the float64 [H,W] host array of image `image` of a
    [B,H,W] (or of a [H,W]) device mask.  This copy waits for the mask."""
    m = valid_mask if valid_mask.dim() == 2 else valid_mask[int(image)]
    return m.to(torch.float64).cpu().numpy()
