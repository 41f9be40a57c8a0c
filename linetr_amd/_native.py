"""ctypes binding of liblinetr_hip.so (the C ABI of include/linetr_hip.h).

There is NO fallback: if the shared library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "liblinetr_hip.so")
# the product sources + experiments/csrc built with -DLINETR_EXPERIMENTS (`python -m linetr_amd.build --experiments`): tuning
# switches and the kernels that were measured and lost.  Lives OUTSIDE the package; only tools/ and `pytest -m experiments` load it.
EXPERIMENTS_LIB_PATH = os.path.join(os.path.dirname(_HERE), "experiments", "liblinetr_hip_experiments.so")

E_ARG, E_ASSERT, E_WORKSPACE = -1, -4, -5     # LinetrStatus codes that callers tell apart (include/linetr_hip.h)
# element type of a dense descriptor map, OR-ed into `dense_is_nhwc` (LINETR_DENSE_F16 / LINETR_DENSE_BF16); also the type codes of
# linetr_superpoint_heads_typed
DENSE_F16, DENSE_BF16 = 0x100, 0x200


def dense_type_bits(dtype) -> int:
    """The format bits of a torch dtype the kernels read in place (0: float32); None for every other dtype."""
    import torch
    return {torch.float32: 0, torch.float16: DENSE_F16, torch.bfloat16: DENSE_BF16}.get(dtype)


class ModelConfig(C.Structure):
    _fields_ = [("d_model", C.c_int32), ("n_heads", C.c_int32), ("d_inner", C.c_int32),
                ("n_sig_layers", C.c_int32), ("n_desc_layers", C.c_int32), ("enc_channels", C.c_int32 * 4),
                ("norm_height", C.c_int32), ("norm_width", C.c_int32), ("bn_batch_stats", C.c_int32)]


class LineRec(C.Structure):
    _fields_ = [("sp", C.c_double * 2), ("ep", C.c_double * 2), ("length", C.c_double),
                ("angle", C.c_double * 2), ("first_sub", C.c_int32), ("n_tok", C.c_int32),
                ("n_sub", C.c_int32), ("image", C.c_int32), ("line_local", C.c_int32), ("first_tok", C.c_int32)]


REC_DTYPE = np.dtype([("sp", "<f8", 2), ("ep", "<f8", 2), ("length", "<f8"), ("angle", "<f8", 2),
                      ("first_sub", "<i4"), ("n_tok", "<i4"), ("n_sub", "<i4"), ("image", "<i4"),
                      ("line_local", "<i4"), ("first_tok", "<i4")])
assert REC_DTYPE.itemsize == C.sizeof(LineRec) == 80


class Tokens(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("klines", "length", "angles", "sublines", "pnt", "mask", "resp",
                                          "angle_sub", "desc", "score", "mat", "h_cu_klines")]


# LinetrPrefilterImage / LinetrImage: one row of the HOST tables linetr_prefilter_ragged / linetr_describe_ragged take (pointers: 0 = NULL)
PREFILTER_IMAGE_DTYPE = np.dtype([("height", "<i4"), ("width", "<i4"), ("min_length", "<f8"), ("token_distance", "<f8"), ("valid_mask", "<u8")])
IMAGE_DTYPE = np.dtype([("d_dense_desc", "<u8"), ("d_dense_score", "<u8"), ("height", "<i4"), ("width", "<i4"), ("token_distance", "<f8")])
assert PREFILTER_IMAGE_DTYPE.itemsize == IMAGE_DTYPE.itemsize == 32


class GemmCase(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int32), ("A2", C.c_void_p), ("lda2", C.c_int32), ("K1", C.c_int32),
                ("W", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p), ("Y", C.c_void_p), ("ldy", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("act", C.c_int32), ("groups", C.c_int32),
                ("gA", C.c_int64), ("gY", C.c_int64), ("norm", C.c_int32), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("add2", C.c_void_p), ("eps", C.c_float), ("via_row_norm", C.c_int32), ("tile", C.c_int32)]


class Dropout(C.Structure):
    """LinetrDropout: what a dropout kernel draws its masks from.  `make` is the one place a probability becomes a threshold."""
    _fields_ = [("seed", C.c_uint64), ("call", C.c_uint32), ("threshold", C.c_uint32), ("scale", C.c_float)]

    @classmethod
    def make(cls, seed: int, call: int, p: float) -> "Dropout":
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout probability {p}: 0 <= p < 1")
        if not 0 <= int(seed) < 1 << 64 or not 0 <= int(call) < 1 << 32:
            raise ValueError(f"dropout seed {seed} / call {call}: a 64-bit seed and a 32-bit call index")
        return cls(int(seed), int(call), int(p * 4294967296.0), 1.0 / (1.0 - p))       # floor(p 2^32) in double; float32(1 / (1 - p))


# LinetrAdamTensor: one row of the HOST table linetr_adam_step / linetr_grad_norm take (p, g, m, v: device pointers; 0 = NULL)
ADAM_TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"), ("bc2_sqrt", "<f4")])
assert ADAM_TENSOR_DTYPE.itemsize == 48


def adam_bias_corrections(lr: float, beta1: float, beta2: float, step: float):
    """(step_size, bc2_sqrt) of one parameter as torch's _single_tensor_adam makes them, in double: lr / (1 - beta1^step) and
    sqrt(1 - beta2^step).  The one place a step count becomes what the kernel reads (each is then rounded to float32 once)."""
    step = float(step)
    return float(lr) / (1.0 - float(beta1) ** step), (1.0 - float(beta2) ** step) ** 0.5


class AdamHyper(C.Structure):
    """LinetrAdamHyper"""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double), ("lr", C.c_double),
                ("decoupled", C.c_int32)]


class DetectConfig(C.Structure):
    """LinetrDetectConfig"""
    _fields_ = [("n_octaves", C.c_int32), ("scale", C.c_int32), ("grad_threshold", C.c_int32), ("min_region_size", C.c_int32),
                ("density", C.c_double)]


class PhotoConfig(C.Structure):
    """LinetrPhotoConfig: the ranges of homography.yaml's augmentation.photometric.params"""
    _fields_ = [("stages", C.c_int32), ("max_abs_change", C.c_int32), ("strength_range", C.c_double * 2), ("stddev_range", C.c_double * 2),
                ("prob_range", C.c_double * 2), ("max_kernel_size", C.c_int32), ("nb_ellipses", C.c_int32), ("blur_sigma", C.c_double),
                ("transparency_range", C.c_double * 2), ("kernel_size_range", C.c_int32 * 2)]


class PhotoParams(C.Structure):
    """LinetrPhotoParams: one image's drawn values"""
    _fields_ = [("stages", C.c_int32), ("d", C.c_int32), ("alpha", C.c_double), ("sigma", C.c_double), ("thr", C.c_uint32), ("K", C.c_int32),
                ("weights", C.c_float * 49), ("blur_ksize", C.c_int32), ("blur_sigma", C.c_double), ("n_ellipses", C.c_int32),
                ("ellipse", (C.c_double * 6) * 20), ("t", C.c_double), ("shade_ksize", C.c_int32)]


# the same 1224 bytes as a NumPy record (arrays of images: np.zeros(B, PHOTO_PARAMS_DTYPE))
PHOTO_PARAMS_DTYPE = np.dtype({"names": ["stages", "d", "alpha", "sigma", "thr", "K", "weights", "blur_ksize", "blur_sigma", "n_ellipses",
                                         "ellipse", "t", "shade_ksize"],
                               "formats": ["<i4", "<i4", "<f8", "<f8", "<u4", "<i4", ("<f4", 49), "<i4", "<f8", "<i4", ("<f8", (20, 6)), "<f8", "<i4"],
                               "offsets": [0, 4, 8, 16, 24, 28, 32, 228, 232, 240, 248, 1208, 1216], "itemsize": 1224})
assert PHOTO_PARAMS_DTYPE.itemsize == C.sizeof(PhotoParams) == 1224 and C.sizeof(PhotoConfig) == 96
PHOTO_STAGES = {"brightness": 1, "contrast": 2, "noise": 4, "impulse": 8, "motion": 16, "blur": 32, "shade": 64}      # LINETR_PHOTO_*


# LinetrPreparedEntry: one row of the table linetr_debug_prepare fills
PREPARED_ENTRY_DTYPE = np.dtype([("name", "S24"), ("offset", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
assert PREPARED_ENTRY_DTYPE.itemsize == 48


class ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char_p), ("calls", C.c_int32), ("ms", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double)]


vp, i32, i64, f64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float
_P = C.POINTER

# The C ABI of include/linetr_hip.h, in the header's order: name -> (restype, argtypes).  lib() applies it; EXPORTS is its name set.
# (i32: a LinetrStatus unless the name says otherwise.)
ABI = {
    "linetr_abi_version": (i32, []),
    "linetr_last_error": (C.c_char_p, []),
    "linetr_create": (i32, [_P(ModelConfig), i32, _P(C.c_char_p), _P(vp), _P(i64), i32, _P(vp)]),
    "linetr_destroy": (None, [vp]),
    "linetr_prefilter": (i32, [vp, i32, i32, i32, i32, f64, i32, vp, f64, i32, i32, i32, i32, vp, i32, _P(i32), _P(i32)]),
    "linetr_prefilter_batch": (i32, [vp, vp, i32, i32, i32, i32, f64, i32, vp, f64, i32, i32, vp, i32, vp, vp]),
    "linetr_prefilter_ragged": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp, i32, vp, vp]),
    "linetr_prefilter_tied_images": (i32, [vp, i32]),
    "linetr_pack_lines": (i32, [vp, vp, vp, i32, f64, i32, i32, i32, i32, vp, _P(i32)]),
    "linetr_tokenize_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_tokenize": (i32, [vp, vp, i32, i32, f64, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, Tokens, vp, vp, i64, vp]),
    "linetr_sample_descriptors_workspace_bytes": (i64, [i32, i32, i32]),
    "linetr_sample_descriptors": (i32, [vp, vp, i64, vp, i32, i32, i32, i32, vp, vp, i64, vp]),
    "linetr_forward_workspace_bytes": (i64, [vp, i32, i32]),
    "linetr_forward": (i32, [vp, _P(Tokens), vp, vp, i32, i32, vp, vp, i64, vp]),
    "linetr_bn_stats_floats": (i64, [vp]),
    "linetr_forward_train_workspace_bytes": (i64, [vp, i32, i32]),
    "linetr_forward_train": (i32, [vp, _P(Tokens), vp, vp, i32, i32, f32, vp, vp, vp, vp, i64, vp]),
    "linetr_describe_workspace_bytes": (i64, [vp, i32, i32, i32, i32, i64]),
    "linetr_describe": (i32, [vp, vp, i32, i32, i64, vp, vp, i32, f64, i32, vp, vp, i32, i32, i32, i32, Tokens, vp, vp, vp, i64, vp]),
    "linetr_describe_ragged_workspace_bytes": (i64, [vp, vp, i32, i32, i32, i64]),
    "linetr_describe_ragged": (i32, [vp, vp, vp, i32, i32, i64, vp, vp, vp, i32, i32, i32, i32, Tokens, vp, vp, vp, i64, vp]),
    "linetr_describe_submit": (i32, [vp, vp, i32, i32, i64, vp, vp, i32, f64, i32, vp, vp, i32, i32, i32, i32, Tokens, vp, vp, vp, i64, i32,
                                     i32, vp]),
    "linetr_pipeline_max_slots": (i32, []),
    "linetr_describe_join": (i32, [vp, i32, vp]),
    "linetr_match_workspace_bytes": (i64, [i32, i64, i64, i64]),
    "linetr_match": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "linetr_match_gathered": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "linetr_match_distmat_workspace_bytes": (i64, [i32, i32]),
    "linetr_match_distmat": (i32, [vp, vp, i32, i32, f32, i32, vp, vp, i64, vp]),
    "linetr_match_distmat_f64_workspace_bytes": (i64, [i32, i32]),
    "linetr_match_distmat_f64": (i32, [vp, vp, i32, i32, f64, i32, vp, vp, i64, vp]),
    "linetr_pool_distmat_workspace_bytes": (i64, [i32, i32]),
    "linetr_pool_distmat": (i32, [vp, vp, i32, i32, vp, i32, vp, i32, vp, vp, i64, vp]),
    "linetr_pool_distmat_dense_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_pool_distmat_dense": (i32, [vp, vp, i32, i32, vp, i32, vp, i32, vp, vp, i64, vp]),
    "linetr_match_points_workspace_bytes": (i64, [i32, i32]),
    "linetr_match_points": (i32, [vp, vp, i32, vp, i32, f32, i32, vp, vp, vp, i64, vp]),
    "linetr_pair_tail_workspace_bytes": (i64, [i32, i32, i32, i32, i32, i32]),
    "linetr_pair_tail_output_bytes": (i64, [i32, i32, i32, i32, vp]),
    "linetr_pair_tail": (i32, [vp, vp, i32, vp, i32, f32, vp, i32, vp, i32, vp, i32, vp, i32, f32, i32, vp, i64, vp, i64, vp]),
    "linetr_val_step_workspace_bytes": (i64, [i32, i32]),
    "linetr_val_step_output_bytes": (i64, [i32, vp]),
    "linetr_val_step": (i32, [vp, vp, i32, vp, i32, vp, i32, f64, i32, vp, vp, vp, vp, i64, vp, i64, vp]),
    "linetr_assign_from_matches": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "linetr_desc_loss_grad_workspace_bytes": (i64, [i32, i32]),
    "linetr_desc_loss_grad": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, i64, vp, i64, vp]),
    "linetr_hardnet_loss_grad_workspace_bytes": (i64, [i32, i32]),
    "linetr_hardnet_loss_grad": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp]),
    "linetr_linear_backward_chunk_rows": (i32, []),
    "linetr_linear_backward_workspace_bytes": (i64, [i64, i32, i32]),
    "linetr_linear_forward": (i32, [vp, vp, i64, vp, vp, i64, i32, i32, i32, vp, i64, vp]),
    "linetr_linear_backward": (i32, [vp, vp, i64, vp, vp, i64, vp, i64, i32, i32, vp, vp, vp, vp, i64, vp]),
    "linetr_head_backward_workspace_bytes": (i64, [i64]),
    "linetr_head_forward": (i32, [vp, vp, vp, vp, i64, vp, vp]),
    "linetr_head_backward": (i32, [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]),
    "linetr_sig_attention_backward_workspace_bytes": (i64, [i64]),
    "linetr_sig_attention_forward": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, i32, i64, vp, i64, vp, vp]),
    "linetr_sig_attention_backward": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, i32, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                            vp]),
    "linetr_bn_forward_workspace_bytes": (i64, [i64, i32]),
    "linetr_bn_forward": (i32, [vp, vp, i64, i64, i32, vp, vp, f32, f32, vp, i32, i32, vp, i64, vp, vp, i64, vp]),
    "linetr_bn_backward_workspace_bytes": (i64, [i64, i32]),
    "linetr_bn_backward": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, i32, vp, i64, vp, vp, vp, i64, vp]),
    "linetr_cls_pool_train_forward": (i32, [vp, vp, i64, vp, i64, i64, i32, vp, vp, vp]),
    "linetr_cls_pool_train_backward": (i32, [vp, vp, i64, vp, i64, vp, vp, vp, i64, i32, vp, i64, vp, i64, vp]),
    "linetr_layer_norm_backward_workspace_bytes": (i64, [i64, i32]),
    "linetr_layer_norm_forward": (i32, [vp, vp, i64, vp, i64, vp, vp, f32, i64, i32, vp, i64, vp, vp]),
    "linetr_layer_norm_backward": (i32, [vp, vp, i64, vp, i64, vp, vp, vp, i64, i64, i32, vp, i64, vp, vp, vp, i64, vp]),
    "linetr_cls_pool_dropout_forward": (i32, [vp, vp, i64, vp, i64, i64, i32, _P(Dropout), vp, vp, vp, vp]),
    "linetr_cls_pool_dropout_backward": (i32, [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, i32, _P(Dropout), vp, i64, vp, i64, vp]),
    "linetr_layer_norm_dropout_forward": (i32, [vp, vp, i64, vp, i64, vp, vp, f32, i64, i32, _P(Dropout), i32, vp, i64, vp, vp]),
    "linetr_layer_norm_dropout_backward": (i32, [vp, vp, i64, vp, i64, vp, vp, vp, i64, i64, i32, _P(Dropout), i32, vp, i64, vp, i64, vp, vp, vp,
                                                 i64, vp]),
    "linetr_dropout_factors": (i32, [vp, _P(Dropout), i32, i64, i64, vp, vp]),
    "linetr_gelu_forward": (i32, [vp, vp, i64, i64, i32, vp, i64, vp]),
    "linetr_gelu_backward": (i32, [vp, vp, i64, vp, i64, i64, i32, vp, i64, vp]),
    "linetr_input_layer_chunk_rows": (i32, []),
    "linetr_input_layer_backward_workspace_bytes": (i64, [i64, i32, i32]),
    "linetr_input_layer_forward": (i32, [vp, vp, i64, vp, vp, i64, i32, i32, vp, i64, vp]),
    "linetr_input_layer_backward": (i32, [vp, vp, i64, vp, i64, i64, i32, i32, vp, vp, vp, i64, vp]),
    "linetr_token_assemble_backward_workspace_bytes": (i64, [i64]),
    "linetr_token_assemble_forward": (i32, [vp, vp, vp, vp, i64, i32, vp, vp]),
    "linetr_token_assemble_backward": (i32, [vp, vp, i64, i32, vp, vp, vp, i64, vp]),
    "linetr_gt_assign_workspace_bytes": (i64, [i32, i32, i32]),
    "linetr_gt_assign": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, f64, f64, f64, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
    "linetr_make_pseudo_lines": (i32, [C.c_uint64, i32, i32, f64, f64, f64, vp]),
    "linetr_find_line_attributes": (i32, [vp, i32, f64, i32, vp, vp, vp, _P(i32)]),
    "linetr_fixed_size_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_fixed_size": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f64, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, Tokens, vp, vp,
                                vp, i64, vp]),
    "linetr_adam_workspace_bytes": (i64, [i32, i64]),
    "linetr_adam_step": (i32, [vp, vp, i32, _P(AdamHyper), vp, vp, i64, vp]),
    "linetr_grad_norm_workspace_bytes": (i64, [i32, i64]),
    "linetr_grad_norm": (i32, [vp, vp, i32, f64, vp, vp, vp, i64, vp]),
    "linetr_superpoint_heads": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "linetr_superpoint_heads_typed": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp]),
    "linetr_superpoint_keypoints_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_superpoint_keypoints": (i32, [vp, vp, i32, i32, i32, i32, f32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "linetr_point_descriptors_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_point_descriptors": (i32, [vp, vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp, i64, vp]),
    "linetr_superpoint_heads_rows": (i32, [vp, vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, vp]),
    "linetr_warp_images": (i32, [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]),
    "linetr_warp_tile": (i32, [_P(i32), _P(i32), _P(i32), _P(i32)]),
    "linetr_mask_erode": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "linetr_photometric_sample": (i32, [_P(PhotoConfig), C.c_uint64, i32, i32, i32, i32, vp]),
    "linetr_photometric_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_photometric": (i32, [vp, vp, i32, i32, i32, vp, C.c_uint64, i32, i32, vp, vp, i64, vp]),
    "linetr_gaussian_blur": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp]),
    "linetr_photometric_tile": (i32, [_P(i32)] * 8),
    "linetr_detect_lines_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "linetr_detect_lines": (i32, [vp, vp, i32, i32, i32, i32, _P(DetectConfig), i32, vp, vp, vp, vp, i64, vp]),
    "linetr_detect_tile": (i32, [_P(i32), _P(i32)]),
    "linetr_detect_debug_labels_workspace_bytes": (i64, [i32, i32, i32]),
    "linetr_detect_debug_labels": (i32, [vp, vp, i32, i32, i32, vp, vp, i64, vp]),
    "linetr_detect_debug_gradient": (i32, [vp, vp, i32, i32, i32, i32, _P(DetectConfig), i32, vp, vp, vp, vp, i64, vp]),
    "linetr_sp_conv3x3_tile": (i32, [_P(i32), _P(i32)]),
    "linetr_sp_conv3x3_pack_bytes": (i64, [i32, i32]),
    "linetr_sp_conv3x3_pack": (i32, [vp, i32, i32, vp, vp]),
    "linetr_sp_conv3x3": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    "linetr_sp_conv1a": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "linetr_sp_encoder_create": (i32, [i32, _P(vp)]),
    "linetr_sp_encoder_destroy": (None, [vp]),
    "linetr_sp_encoder_set_weights": (i32, [vp, _P(vp), _P(vp), vp]),
    "linetr_sp_encoder_workspace_bytes": (i64, [i32, i32, i32]),
    "linetr_sp_encoder_forward": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
    "linetr_set_precision": (i32, [vp, i32]),
    "linetr_get_precision": (i32, [vp]),
    "linetr_debug_posenc": (i32, [vp, i32, vp, vp, vp, i64, vp, vp]),
    "linetr_debug_gemm": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "linetr_debug_gemm_case": (i32, [vp, _P(GemmCase), vp, vp]),
    "linetr_debug_sig_attention": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp]),
    "linetr_debug_tok_mlp": (i32, [vp, i32, vp, vp, i64, vp, vp, vp, i64, vp, vp, i32, vp, vp]),
    "linetr_debug_bn_train_workspace_bytes": (i64, [vp, i32, i64]),
    "linetr_debug_bn_train": (i32, [vp, i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, i64, vp]),
    "linetr_debug_cls_pool": (i32, [vp, i32, vp, i32, vp, i32, i32, vp, vp, i64, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "linetr_debug_match": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    "linetr_debug_stage_workspace_bytes": (i64, [vp, i32, i32]),
    "linetr_debug_stage": (i32, [vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "linetr_debug_prepare": (i32, [_P(ModelConfig), i32, _P(C.c_char_p), _P(vp), _P(i64), vp, i64, vp, i32, _P(i64), _P(i32)]),
    "linetr_allgather_desc": (i32, [vp, vp, vp, i64, vp]),
    "linetr_set_allgather_fn": (i32, [vp]),
    "linetr_pack_slab": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp]),
    "linetr_set_profiling": (i32, [vp, i32]),
    "linetr_get_profile": (i32, [vp, _P(ProfileEntry), i32, _P(i32)]),
}
# the experiments build only (include/linetr_hip.h, LINETR_EXPERIMENTS)
EXPERIMENT_ABI = {
    "linetr_st_bytes": (i64, [i64, i32]),
    "linetr_debug_to_st": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "linetr_debug_from_st": (i32, [vp, vp, i32, i32, vp, i32, vp]),
    "linetr_debug_gemm_st": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "linetr_debug_pairnet_stamps": (i32, [vp, vp]),
}
EXPORTS = list(ABI)
EXPERIMENT_EXPORTS = list(EXPERIMENT_ABI)

_libs = {}


def lib(path=None):
    """Load the in-tree shared library (built by ``python -m linetr_amd.build`` / __graft_entry__.build()).
    `path`: another build of the same sources (EXPERIMENTS_LIB_PATH, a tools/ variant); default = the product library,
    or $LINETR_LIB when set."""
    # torch ships its own libamdhip64; importing it first makes liblinetr_hip.so bind to the SAME HIP runtime
    # (one context, shared streams and device pointers) instead of a second copy from /opt/rocm.
    import torch  # noqa: F401
    path = os.path.abspath(path or os.environ.get("LINETR_LIB", LIB_PATH))
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built (run `python -m linetr_amd.build`). "
            "linetr_amd has no CPU fallback.")
    L = C.CDLL(path)
    table = {**ABI, **EXPERIMENT_ABI} if hasattr(L, "linetr_debug_gemm_st") else ABI
    for name, (restype, argtypes) in table.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.linetr_abi_version() != 6:
        raise RuntimeError("liblinetr_hip.so ABI version mismatch")
    _libs[path] = L
    return L


class NativeError(RuntimeError):
    pass


def check(code: int, L=None):
    """`L`: the library the failing call went through (every .so keeps its own thread-local error text); default = the
    product library."""
    if code == 0:
        return
    msg = (L if L is not None else lib()).linetr_last_error().decode("utf-8", "replace")
    if code == E_ASSERT:
        raise AssertionError(msg)     # same exception type the reference raises (line_process.py:44-45)
    raise NativeError(f"liblinetr_hip error {code}: {msg}")


def np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)
