"""ctypes binding of libdfdclip_hip.so (C ABI declared in include/dfdclip.h).

There is no CPU or PyTorch fallback: if the library is missing or a call fails, this module
raises.  Tensors are passed as raw device pointers; every call enqueues on
`torch.cuda.current_stream()` and returns without synchronising.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint, c_uint8, c_uint32, c_uint64, c_void_p

import torch

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libdfdclip_hip.so")

F32, BF16 = 0, 1
EPI_BIAS, EPI_BIAS_QUICKGELU, EPI_BIAS_RESIDUAL, EPI_PATCH_EMBED, EPI_QKV_EXPORT, EPI_RESIDUAL_POS, EPI_BIAS_GELU = range(7)
ABI_VERSION = 17

_DTYPE = {torch.float32: F32, torch.bfloat16: BF16}
FP8 = 2           # ABI code of OCP e4m3; stored in uint8 / torch.float8_e4m3fn tensors
FP8_MAX = 448.0   # largest finite e4m3 value
FP8_MIN_ROWS = 1024  # dfd_gemm_fp8 serves M >= 1024 (gemm_plan's rule; tests/test_abi_cpu.py holds this constant to it)


class DfdError(RuntimeError):
    pass


GEMM_STREAM_OUT = 1
GEMM_SPARE_IF_FREE = 2  # spare_cus is honoured only where it costs this shape no extra round of tiles
GEMM_C_BLOCKED = 4  # C written / A read in the fragment-blocked layout of the MLP intermediate (blocked.py)
GEMM_A_BLOCKED = 8


class GemmExtra(Structure):
    _fields_ = [("pos", c_void_p), ("cls", c_void_p), ("k_export", c_void_p), ("v_export", c_void_p),
                ("tokens", c_int32), ("frames_per_clip", c_int32), ("residual", c_void_p), ("qkv_first", c_int32),
                ("drop_rng", c_void_p), ("drop_site", c_uint32), ("drop_p", c_float), ("flags", c_uint32)]


OPTIM_SGD, OPTIM_ADAMW = 0, 1


class OptimExtra(Structure):
    """dfd_optim_extra: what `dfd_sgd_step` needs beyond SGD's arguments."""
    _fields_ = [("kind", c_int32), ("reserved", c_int32), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("step", c_int64), ("exp_avg_sq", c_void_p)]


class DropoutDesc(Structure):
    _fields_ = [("rng_state", c_void_p), ("site", c_uint32), ("p", c_float)]


class Dropout:
    """One dropout layer of one step: `rng` = device int64[2] {seed, step}, `site` = which layer, `p`."""
    __slots__ = ("rng", "site", "p")

    def __init__(self, rng, site, p):
        assert rng.is_cuda and rng.dtype == torch.int64 and rng.numel() == 2 and 0.0 <= p < 1.0
        self.rng, self.site, self.p = rng, int(site), float(p)

    def desc(self):
        return DropoutDesc(self.rng.data_ptr(), self.site, self.p)


def _drop(d):
    return ctypes.byref(d.desc()) if d is not None and d.p > 0 else None


# name -> (restype, argtypes); mirrors include/dfdclip.h one to one
SIGNATURES = {
    "dfd_last_error": (c_char_p, []),
    "dfd_abi_version": (c_int, []),
    "dfd_gemm_last_path": (c_int, []),
    "dfd_gemm_set_variant": (c_int, [c_int]),
    "dfd_dropout": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, POINTER(DropoutDesc), c_void_p]),
    "dfd_device_check": (c_int, []),
    "dfd_layernorm": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_float, c_float, c_void_p]),
    "dfd_layernorm2": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_float,
                               c_float, c_void_p]),
    "dfd_add_layernorm": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                  c_int, c_int64, c_int, c_float, c_float, c_void_p]),
    "dfd_patchify": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "dfd_preprocess_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float),
                                  c_void_p, c_int, c_int, c_int, c_void_p]),
    "dfd_preprocess_geometry": (c_int, [c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "dfd_gemm": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_int,
                         POINTER(GemmExtra), c_int64, c_int, c_int, c_void_p]),
    "dfd_gemm_fp8": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_float, c_int,
                             POINTER(GemmExtra), c_int64, c_int, c_int, c_void_p]),
    "dfd_gemm_at_b_workspace": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "dfd_gemm_at_b": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "dfd_adapter_norm_gelu": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                      c_void_p]),
    "dfd_attention_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "dfd_linear_rows": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "dfd_linear_rows_t_workspace": (c_size_t, [c_int, c_int, c_int]),
    "dfd_linear_rows_t": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p]),
    "dfd_decoder_attn_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfd_decoder_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "dfd_decoder_attn_modes_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                           c_int, c_int, c_void_p]),
    "dfd_decoder_attn_modes_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                           c_int, c_int, c_void_p]),
    "dfd_decoder_attn_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfd_decoder_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                     c_int, c_void_p]),
    "dfd_adapter_norm_gelu_bwd_workspace": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfd_adapter_norm_gelu_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "dfd_linear_rows_bwd_weight": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "dfd_transpose_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "dfd_sgd_blocks": (c_int64, [c_int64, c_int, c_int, c_int]),
    "dfd_sgd_step": (c_int, [c_void_p, c_int, c_int64, c_float, c_float, c_float, c_int, c_void_p, POINTER(OptimExtra)]),
    "dfd_layernorm_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_int, c_int, c_float, c_int, c_void_p]),
    "dfd_quickgelu": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(DropoutDesc), c_void_p]),
    "dfd_head_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                             c_void_p]),
    "dfd_head_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                             c_int, c_float, POINTER(DropoutDesc), c_void_p]),
    "dfd_adapter_bn_workspace": (c_size_t, [c_int64, c_int, c_int]),
    "dfd_adapter_bn_stats": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                     c_int, c_float, c_float, c_void_p]),
    "dfd_adapter_bn_apply": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     POINTER(DropoutDesc), c_int64, c_int, c_int, c_int, c_void_p]),
    "dfd_adapter_bn_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   POINTER(DropoutDesc), c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "dfd_gelu_erf": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, POINTER(DropoutDesc), c_void_p]),
    "dfd_gelu_erf_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int64, POINTER(DropoutDesc), c_void_p]),
    "dfd_compinv_loss_workspace": (c_size_t, [c_int, c_int]),
    "dfd_compinv_loss_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "dfd_compinv_loss_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
}

# entry points appended to the ABI after version 17 without a new number (include/dfdclip_ext.h)
EXT_SIGNATURES = {
    "dfd_layernorm_dual": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_float,
                                   c_float, c_void_p]),
    "dfd_layernorm2_dual": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                    c_int64, c_int, c_float, c_float, c_void_p]),
    "dfd_add_layernorm_dual": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                       c_void_p, c_int64, c_int64, c_int, c_float, c_float, c_void_p]),
}

# explanation entry points beside the ABI, in a header of their own (include/dfdclip_explain.h)
EXPLAIN_SIGNATURES = {
    "dfd_decoder_attn_map": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_int, c_int, c_int, c_void_p]),
}


class AugmentSet(Structure):
    """dfd_augment_set_t (include/dfdclip_augment.h): one draw of the training augmentation."""
    _fields_ = [("flags", c_uint32), ("hue", c_int32), ("sat", c_int32), ("val", c_int32), ("quality", c_int32),
                ("reserved", c_int32 * 3), ("rgb_lut", (c_uint8 * 256) * 3), ("tone_lut", c_uint8 * 256)]


AUG_RGB_LUT, AUG_HSV, AUG_TONE_LUT, AUG_FLIP = 1, 2, 4, 8
AUGMENT_SET_BYTES = ctypes.sizeof(AugmentSet)  # the header documents it as DFD_AUGMENT_SET_BYTES

# training augmentation beside the ABI, in a header of its own (include/dfdclip_augment.h)
AUGMENT_SIGNATURES = {
    "dfd_augment_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
}

class AlignFrame(Structure):
    """dfd_align_frame_t (include/dfdclip_align.h): one frame's inverse map, crop origin, window origin and border."""
    _fields_ = [("q", c_int64 * 6), ("x0", c_int32), ("y0", c_int32), ("win_x", c_int32), ("win_y", c_int32), ("border", c_int32),
                ("flags", c_uint32)]


ALIGN_HWC, ALIGN_CHW = 0, 1
ALIGN_SWAP_RB = 1
ALIGN_FRAME_INVALID = 1
ALIGN_FRAME_BYTES = ctypes.sizeof(AlignFrame)  # the header documents it as DFD_ALIGN_FRAME_BYTES

# face alignment beside the ABI, in a header of its own (include/dfdclip_align.h)
ALIGN_SIGNATURES = {
    "dfd_align_crop_u8": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_uint32,
                                  c_void_p]),
}


class YuvMatrix(Structure):
    """dfd_yuv_matrix_t (include/dfdclip_yuv.h): the Q16 conversion matrix of one call; host data."""
    _fields_ = [("y_off", c_int32), ("cy", c_int32), ("crv", c_int32), ("cgu", c_int32), ("cgv", c_int32), ("cbu", c_int32),
                ("reserved", c_int32 * 2)]


class Yuv420Source(Structure):
    """dfd_yuv420_t (include/dfdclip_yuv.h): three device planes and their byte strides; host data."""
    _fields_ = [("y", c_void_p), ("u", c_void_p), ("v", c_void_p), ("y_row_stride", c_int64), ("y_frame_stride", c_int64),
                ("c_row_stride", c_int64), ("c_frame_stride", c_int64), ("c_px_stride", c_int32), ("reserved", c_int32)]


YUV_MATRIX_BYTES = ctypes.sizeof(YuvMatrix)    # the header documents it as DFD_YUV_MATRIX_BYTES
YUV420_BYTES = ctypes.sizeof(Yuv420Source)     # ... as DFD_YUV420_BYTES
YUV_COEF_MAX = 1 << 21

# 4:2:0 sources beside the ABI, in a header of its own (include/dfdclip_yuv.h)
YUV_SIGNATURES = {
    "dfd_yuv420_to_rgb_u8": (c_int, [POINTER(Yuv420Source), c_int, c_int, c_void_p, c_int, POINTER(YuvMatrix), c_void_p]),
    "dfd_align_crop_yuv420": (c_int, [POINTER(Yuv420Source), c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, POINTER(YuvMatrix),
                                      c_void_p]),
}

ELASTIC_MAX_RADIUS, ELASTIC_TAP_ONE, ELASTIC_SITE = 128, 32768, 0xE1A57100

# elastic warp (the reference's `ssl_fake`) beside the ABI, in a header of its own (include/dfdclip_elastic.h)
ELASTIC_SIGNATURES = {
    "dfd_elastic_field": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_uint64, c_void_p, c_int, c_int32, c_void_p]),
    "dfd_elastic_remap_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
}

SWIGLU_VEC16, SWIGLU_ELEMENT = 1, 2  # dfd_swiglu_last_path: 16-byte accesses, or element by element

# the gate of a SwiGLU feed-forward (DINOv2 ViT-g/14) beside the ABI, in a header of its own (include/dfdclip_swiglu.h)
SWIGLU_SIGNATURES = {
    "dfd_swiglu_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int64, c_int, c_void_p]),
    "dfd_swiglu_last_path": (c_int, []),
}

KVGATHER_VEC16, KVGATHER_ELEMENT = 1, 2  # dfd_kv_gather_last_path: 16-byte accesses, or element by element

# the K/V row gather of patch-masked training beside the ABI, in a header of its own (include/dfdclip_kvgather.h)
KVGATHER_SIGNATURES = {
    "dfd_kv_gather_patches": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "dfd_kv_gather_last_path": (c_int, []),
}

KVFRAMES_VEC16, KVFRAMES_ELEMENT = 1, 2  # dfd_kv_move_last_path: 16-byte accesses, or element by element
KVFRAMES_SRC_ONCE = 1  # flags of dfd_kv_move_frames: the source is read once, its loads follow the STREAM_DECODER_KV policy bit

# the K/V frame mover of the streaming path beside the ABI, in a header of its own (include/dfdclip_kvframes.h)
KVFRAMES_SIGNATURES = {
    "dfd_kv_move_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                   c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "dfd_kv_move_last_path": (c_int, []),
}

# decoder attention over a frame store, read in place through a slot table, beside the ABI, in a header of its own
# (include/dfdclip_kvtable.h): the arguments of dfd_decoder_attn_fwd / dfd_decoder_attn_map, then frame_table and store_frames
KVTABLE_SIGNATURES = {
    "dfd_decoder_attn_fwd_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "dfd_decoder_attn_map_frames": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                            c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
}

# the EMA-teacher update beside the ABI, in a header of its own (include/dfdclip_ema.h)
EMA_SIGNATURES = {
    "dfd_ema_step": (c_int, [c_void_p, c_int, c_int64, c_float, c_float, c_void_p]),
}

# test / measurement hooks outside the ABI header (include/dfdclip_hooks.h)
class AttentionPlan(Structure):
    """dfd_attention_plan_t (include/dfdclip_hooks.h)."""
    _fields_ = [("path", c_int32), ("grid", c_uint32), ("block", c_uint32), ("chunk", c_int32), ("lds", c_uint64)]


class GemmPlan(Structure):
    """dfd_gemm_plan_t (include/dfdclip_hooks.h)."""
    _fields_ = [("kernel", c_int32), ("epilogue", c_int32), ("tile_rows", c_int32), ("tiles_m", c_int32), ("ntiles", c_int64),
                ("grid", c_uint32), ("grid_y", c_uint32), ("block", c_uint32), ("c_blocked", c_int32), ("a_blocked", c_int32),
                ("dynamic", c_int32)]


class AdapterPlan(Structure):
    """dfd_adapter_plan_t (include/dfdclip_hooks.h)."""
    _fields_ = [("path", c_int32), ("grid", c_uint32), ("block", c_uint32), ("slabs", c_int32), ("groups_per_slab", c_int32)]


HOOK_SIGNATURES = {
    "dfd_adapter_norm_gelu_last_path": (c_int, []),
    "dfd_adapter_norm_gelu_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(AdapterPlan)]),
    "dfd_gemm_last_kernel": (c_int, []),
    "dfd_gemm_plan": (c_int, [c_int, c_int, c_int, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_uint32, c_int, c_int, c_int, c_uint,
                              c_uint, c_int, POINTER(GemmPlan)]),
    "dfd_attention_set_variant": (c_int, [c_int]),
    "dfd_attention_last_path": (c_int, []),
    "dfd_attention_plan": (c_int, [c_int, c_int, c_int, c_int, c_int64, c_int64, c_int, POINTER(AttentionPlan)]),
    "dfd_gemm_pair_set_variant": (c_int, [c_int]),
    "dfd_gemm_pair_plan": (c_int, [c_int64, c_int, c_int]),
    "dfd_gemm_pair_launches": (c_int64, []),
    "dfd_gemm_at_b_last_path": (c_int, []),
    "dfd_stream_policy_set": (c_uint, [c_uint]),
    "dfd_stream_policy_get": (c_uint, []),
}

# kernels behind dfd_attention_fwd (DFD_ATTN_* of include/dfdclip_hooks.h, which holds the selection table)
(ATTN_ROWS, ATTN_ROWS_CHUNKED, ATTN_ITEM7, ATTN_ITEM9, ATTN_PERSIST7_SHORT, ATTN_PERSIST7, ATTN_XROW,
 ATTN_STREAM) = range(1, 9)

# kernels behind dfd_adapter_norm_gelu and the group pass of its backward (DFD_ADP_* of include/dfdclip_hooks.h)
ADP_ROW256, ADP_JOINT_REG, ADP_JOINT, ADP_ROW = range(1, 5)

# kernels behind dfd_gemm / dfd_gemm_fp8 (DFD_GEMM_* of include/dfdclip_hooks.h, which holds the selection table), and the
# pointer bits of dfd_gemm_plan
GEMM_GENERAL, GEMM_TILE, GEMM_PERSISTENT, GEMM_PINGPONG = range(1, 5)
(GEMM_PTR_A, GEMM_PTR_W, GEMM_PTR_C, GEMM_PTR_BIAS, GEMM_PTR_POS, GEMM_PTR_CLS, GEMM_PTR_RESIDUAL, GEMM_PTR_COL_SCALE,
 GEMM_PTR_EXPORT) = (1 << i for i in range(9))

# families of dfd_stream_policy_set (include/dfdclip_hooks.h)
STREAM_DECODER_KV, STREAM_DECODER_WEIGHTS, STREAM_OPTIMIZER, STREAM_ENCODER_ROWS, STREAM_ALL = 1, 2, 4, 8, 15
STREAM_DEFAULT = STREAM_DECODER_KV | STREAM_ENCODER_ROWS

_lib = None


def load_library(path=None):
    """dlopen the kernel library and bind every declared symbol.  Raises DfdError when the
    file is absent (run `python -c "import __graft_entry__ as g; g.build()"` or
    `python dfd-clip_amd/build.py`), a symbol is missing or the ABI version differs."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise DfdError(f"{path} not found: the HIP kernel library is not built and there is no fallback path")
    lib = ctypes.CDLL(path)
    for name, (res, args) in {**SIGNATURES, **EXT_SIGNATURES, **EXPLAIN_SIGNATURES, **AUGMENT_SIGNATURES, **ALIGN_SIGNATURES,
                               **ELASTIC_SIGNATURES, **YUV_SIGNATURES, **SWIGLU_SIGNATURES, **KVGATHER_SIGNATURES,
                               **KVFRAMES_SIGNATURES, **KVTABLE_SIGNATURES, **EMA_SIGNATURES, **HOOK_SIGNATURES}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise DfdError(f"{path} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    if lib.dfd_abi_version() != ABI_VERSION:
        raise DfdError(f"{path}: ABI version {lib.dfd_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise DfdError(f"{what} failed ({rc}): {load_library().dfd_last_error().decode()}")


def _stream():
    # torch's current stream on the current device, as a raw hipStream_t: ~0.3 us, where
    # torch.cuda.current_stream().cuda_stream costs ~8 us (700+ launches per train step)
    return c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _dev(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise DfdError("HIP kernels need device tensors; got a CPU tensor (there is no CPU path)")


def _out_dtype(t):
    """ABI dtype code of an output tensor: one-byte tensors (uint8 / float8_e4m3fn storage) are e4m3."""
    return FP8 if t.element_size() == 1 else _DTYPE[t.dtype]


def layernorm(x, gamma, beta, out, eps=1e-5, out_inv_scale=0.0):
    """out[rows, cols] = LayerNorm(x[rows, cols]); x f32; out f32 (may alias x), bf16, or e4m3 bytes of the result
    times `out_inv_scale`."""
    _dev(x, gamma, beta, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and out.shape == x.shape
    assert x.stride(1) == 1 and out.stride(1) == 1
    _check(load_library().dfd_layernorm(_ptr(x), x.stride(0), _ptr(gamma), _ptr(beta), _ptr(out), out.stride(0),
                                        _out_dtype(out), x.shape[0], x.shape[1], eps, float(out_inv_scale), _stream()), "dfd_layernorm")
    return out


def layernorm2(x, gamma_a, beta_a, gamma_b, beta_b, out, eps=1e-5, out_inv_scale=0.0):
    """x <- LayerNorm_a(x) in place (f32), out = LayerNorm_b(x): one pass over the rows."""
    _dev(x, gamma_a, beta_a, gamma_b, beta_b, out)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1 and out.shape == x.shape
    _check(load_library().dfd_layernorm2(_ptr(x), x.stride(0), _ptr(gamma_a), _ptr(beta_a), _ptr(gamma_b), _ptr(beta_b), _ptr(out),
                                         out.stride(0), _out_dtype(out), x.shape[0], x.shape[1], eps, float(out_inv_scale), _stream()),
           "dfd_layernorm2")
    return out


def add_layernorm(x, delta, gamma, beta, out, eps=1e-5, delta2=None, store_x=True, out_inv_scale=0.0):
    """v = (x + delta) [+ delta2] (x f32, deltas f32 / bf16); out = LayerNorm(v) in f32, bf16 or e4m3 (times
    `out_inv_scale`); x <- v when `store_x`."""
    _dev(x, delta, gamma, beta, out, delta2)
    assert x.dtype == torch.float32 and x.dim() == 2 and out.shape == x.shape and delta.shape == x.shape
    assert x.stride(1) == 1 and out.stride(1) == 1 and delta.stride(1) == 1
    assert delta2 is None or (delta2.dtype == delta.dtype and delta2.shape == x.shape and delta2.stride() == delta.stride())
    _check(load_library().dfd_add_layernorm(_ptr(x), x.stride(0), _ptr(delta), _ptr(delta2), delta.stride(0), _DTYPE[delta.dtype],
                                            int(bool(store_x)), _ptr(gamma), _ptr(beta), _ptr(out), out.stride(0), _out_dtype(out),
                                            x.shape[0], x.shape[1], eps, float(out_inv_scale), _stream()), "dfd_add_layernorm")
    return out


def _dual_outputs(x, out16, out8, out8_inv_scale):
    assert out16.dtype == torch.bfloat16 and out8.element_size() == 1 and out16.shape == x.shape and out8.shape == x.shape
    assert out16.stride(1) == 1 and out8.stride(1) == 1 and out8_inv_scale > 0


def layernorm_dual(x, gamma, beta, out16, out8, out8_inv_scale, eps=1e-5):
    """`layernorm` with two outputs from one pass: out16 (bf16) and out8 (e4m3 bytes of the result times `out8_inv_scale`),
    each bit-identical to the single-output call's."""
    _dev(x, gamma, beta, out16, out8)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    _dual_outputs(x, out16, out8, out8_inv_scale)
    _check(load_library().dfd_layernorm_dual(_ptr(x), x.stride(0), _ptr(gamma), _ptr(beta), _ptr(out16), out16.stride(0), _ptr(out8),
                                             out8.stride(0), x.shape[0], x.shape[1], eps, float(out8_inv_scale), _stream()),
           "dfd_layernorm_dual")
    return out16, out8


def layernorm2_dual(x, gamma_a, beta_a, gamma_b, beta_b, out16, out8, out8_inv_scale, eps=1e-5):
    """`layernorm2` with the bf16 and the e4m3 output of LayerNorm_b from one pass."""
    _dev(x, gamma_a, beta_a, gamma_b, beta_b, out16, out8)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    _dual_outputs(x, out16, out8, out8_inv_scale)
    _check(load_library().dfd_layernorm2_dual(_ptr(x), x.stride(0), _ptr(gamma_a), _ptr(beta_a), _ptr(gamma_b), _ptr(beta_b), _ptr(out16),
                                              out16.stride(0), _ptr(out8), out8.stride(0), x.shape[0], x.shape[1], eps,
                                              float(out8_inv_scale), _stream()), "dfd_layernorm2_dual")
    return out16, out8


def add_layernorm_dual(x, delta, gamma, beta, out16, out8, out8_inv_scale, eps=1e-5, delta2=None, store_x=True):
    """`add_layernorm` with the bf16 and the e4m3 output from one pass."""
    _dev(x, delta, gamma, beta, out16, out8, delta2)
    assert x.dtype == torch.float32 and x.dim() == 2 and delta.shape == x.shape and x.stride(1) == 1 and delta.stride(1) == 1
    assert delta2 is None or (delta2.dtype == delta.dtype and delta2.shape == x.shape and delta2.stride() == delta.stride())
    _dual_outputs(x, out16, out8, out8_inv_scale)
    _check(load_library().dfd_add_layernorm_dual(_ptr(x), x.stride(0), _ptr(delta), _ptr(delta2), delta.stride(0), _DTYPE[delta.dtype],
                                                 int(bool(store_x)), _ptr(gamma), _ptr(beta), _ptr(out16), out16.stride(0), _ptr(out8),
                                                 out8.stride(0), x.shape[0], x.shape[1], eps, float(out8_inv_scale), _stream()),
           "dfd_add_layernorm_dual")
    return out16, out8


def patchify(frames, out, res, patch):
    _dev(frames, out)
    assert frames.dtype == torch.float32 and frames.is_contiguous() and out.is_contiguous()
    n = frames.shape[0]
    _check(load_library().dfd_patchify(_ptr(frames), _ptr(out), _DTYPE[out.dtype], n, res, patch, out.shape[1], _stream()),
           "dfd_patchify")
    return out


def preprocess_geometry(in_h, in_w, res):
    """(resized_h, resized_w, crop_top, crop_left) of `preprocess_u8`."""
    v = [c_int() for _ in range(4)]
    _check(load_library().dfd_preprocess_geometry(in_h, in_w, res, *[ctypes.byref(i) for i in v]), "dfd_preprocess_geometry")
    return tuple(i.value for i in v)


def preprocess_u8(frames, out, res, patch, mean, std, antialias=True, patch_rows=True):
    """uint8 frames [n,3,H,W] -> normalised patch rows [n*P, kpad] (`patch_rows`) or frames
    [n,3,res,res]; the device-side `Detector._transform` (reference `src/models.py:756-768`)."""
    _dev(frames, out)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[1] == 3
    assert frames.is_contiguous() and out.is_contiguous()
    n, _, h, w = frames.shape
    m3 = (c_float * 3)(*[float(v) for v in mean])
    s3 = (c_float * 3)(*[float(v) for v in std])
    if patch_rows:
        assert out.dim() == 2 and out.shape[0] == n * (res // patch) ** 2
        kpad = out.shape[1]
    else:
        assert tuple(out.shape) == (n, 3, res, res)
        kpad = 0
    _check(load_library().dfd_preprocess_u8(_ptr(frames), n, h, w, res, patch, int(bool(antialias)), m3, s3, _ptr(out),
                                            _DTYPE[out.dtype], 1 if patch_rows else 0, kpad, _stream()), "dfd_preprocess_u8")
    return out


def augment_u8(frames, out, sets, set_of_frame):
    """out[f] = the augmentation `sets[set_of_frame[f]]` of frames[f] (include/dfdclip_augment.h); frames, out u8
    [n,3,H,W] (distinct), sets u8 [n_sets, AUGMENT_SET_BYTES] = dfd_augment_set_t records, set_of_frame i32 [n]; an index outside
    [0, n_sets) copies the frame.  The device-side colour / JPEG / flip presets of reference `src/datasets.py:288-399`."""
    _dev(frames, out, sets, set_of_frame)
    assert frames.dtype == torch.uint8 and out.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[1] == 3
    assert frames.is_contiguous() and out.is_contiguous() and out.shape == frames.shape
    assert sets.dtype == torch.uint8 and sets.is_contiguous() and sets.dim() == 2 and sets.shape[1] == AUGMENT_SET_BYTES
    n, _, h, w = frames.shape
    assert set_of_frame.dtype == torch.int32 and set_of_frame.is_contiguous() and set_of_frame.numel() == n
    _check(load_library().dfd_augment_u8(_ptr(frames), _ptr(out), n, h, w, _ptr(sets), sets.shape[0], _ptr(set_of_frame), _stream()),
           "dfd_augment_u8")
    return out


def align_crop_u8(src, out, records, layout, row_stride, frame_stride, win_h, win_w, swap_rb=False):
    """out [n,3,oh,ow] u8 = the face-aligned crops of the n source windows behind `src` (include/dfdclip_align.h): `src` any u8
    device tensor whose memory from its first element on holds the frames at the given byte strides (`layout` ALIGN_HWC:
    [win_h, win_w, 3] interleaved, ALIGN_CHW: [3, win_h, win_w] planar), `records` u8 [n, ALIGN_FRAME_BYTES] =
    dfd_align_frame_t.  The device-side `affine_transform` + `cut_patch` of reference `pipeline.py:114-182`."""
    _dev(src, out, records)
    assert src.dtype == torch.uint8 and out.dtype == torch.uint8 and out.dim() == 4 and out.shape[1] == 3 and out.is_contiguous()
    n, _, oh, ow = out.shape
    assert records.dtype == torch.uint8 and records.is_contiguous() and tuple(records.shape) == (n, ALIGN_FRAME_BYTES)
    if n > 0 and win_h > 0 and win_w > 0:  # the memory behind `src` must hold what the strides describe
        span = (n - 1) * frame_stride + (win_h * (1 if layout == ALIGN_HWC else 3) - 1) * row_stride + win_w * (3 if layout == ALIGN_HWC else 1)
        have = src.untyped_storage().nbytes() - src.storage_offset()
        assert span <= have, f"the strides describe {span} bytes, the tensor's memory holds {have} from its first element on"
    _check(load_library().dfd_align_crop_u8(_ptr(src), int(layout), int(row_stride), int(frame_stride), int(win_h), int(win_w), _ptr(out),
                                            n, oh, ow, _ptr(records), ALIGN_SWAP_RB if swap_rb else 0, _stream()), "dfd_align_crop_u8")
    return out


def yuv420_to_rgb_u8(source, out, matrix):
    """out [n,3,h,w] u8 = the n frames of `source` (a Yuv420Source whose planes are device memory) as RGB under `matrix` (a
    YuvMatrix); include/dfdclip_yuv.h.  The caller answers for the memory behind the three pointers (yuv.Yuv420 derives them
    from tensor views, which cannot describe more than they hold)."""
    _dev(out)
    assert out.dtype == torch.uint8 and out.dim() == 4 and out.shape[1] == 3 and out.is_contiguous()
    n, _, h, w = out.shape
    _check(load_library().dfd_yuv420_to_rgb_u8(ctypes.byref(source), h, w, _ptr(out), n, ctypes.byref(matrix), _stream()),
           "dfd_yuv420_to_rgb_u8")
    return out


def align_crop_yuv420(source, win_h, win_w, out, records, matrix):
    """out [n,3,oh,ow] u8 = the face-aligned crops of the n 4:2:0 windows of `source` (win_h x win_w pixels each), converted
    under `matrix` tap by tap; `records` u8 [n, ALIGN_FRAME_BYTES] = dfd_align_frame_t on the device (include/dfdclip_yuv.h)."""
    _dev(out, records)
    assert out.dtype == torch.uint8 and out.dim() == 4 and out.shape[1] == 3 and out.is_contiguous()
    n, _, oh, ow = out.shape
    assert records.dtype == torch.uint8 and records.is_contiguous() and tuple(records.shape) == (n, ALIGN_FRAME_BYTES)
    _check(load_library().dfd_align_crop_yuv420(ctypes.byref(source), int(win_h), int(win_w), _ptr(out), n, oh, ow, _ptr(records),
                                                ctypes.byref(matrix), _stream()), "dfd_align_crop_yuv420")
    return out


def elastic_field(field, field_ids, seed, taps, alpha_q):
    """field[f] = the displacement field with id field_ids[f] (include/dfdclip_elastic.h): field i16 [n,H,W,2] on the device
    ((dx5, dy5) in 1/32-pixel units), field_ids i64 [n] on the device, `seed` a 64-bit integer, `taps` a HOST int32 array of
    2 * radius + 1 Q15 weights summing to 32768, alpha_q = round(256 * alpha)."""
    _dev(field, field_ids)
    assert field.dtype == torch.int16 and field.dim() == 4 and field.shape[3] == 2 and field.is_contiguous()
    n, h, w, _ = field.shape
    assert field_ids.dtype == torch.int64 and field_ids.is_contiguous() and field_ids.numel() == n
    taps = [int(t) for t in taps]
    assert len(taps) % 2 == 1
    t = (c_int32 * len(taps))(*taps)
    _check(load_library().dfd_elastic_field(_ptr(field), n, h, w, _ptr(field_ids), int(seed) & 0xFFFFFFFFFFFFFFFF, t, len(taps) // 2,
                                            int(alpha_q), _stream()), "dfd_elastic_field")
    return field


def elastic_remap_u8(clips, out, field, field_of_clip):
    """out[b] = clips[b] warped by field[field_of_clip[b]], every frame and channel alike (include/dfdclip_elastic.h); clips,
    out u8 [B,T,3,H,W] (distinct), field i16 [n,H,W,2] as `elastic_field` wrote it, field_of_clip i32 [B] on the device; an
    index outside [0, n) copies the clip."""
    _dev(clips, out, field, field_of_clip)
    assert clips.dtype == torch.uint8 and out.dtype == torch.uint8 and clips.dim() == 5 and clips.shape[2] == 3
    assert clips.is_contiguous() and out.is_contiguous() and out.shape == clips.shape
    B, T, _, h, w = clips.shape
    assert field.dtype == torch.int16 and field.is_contiguous() and field.dim() == 4 and tuple(field.shape[1:]) == (h, w, 2)
    assert field_of_clip.dtype == torch.int32 and field_of_clip.is_contiguous() and field_of_clip.numel() == B
    _check(load_library().dfd_elastic_remap_u8(_ptr(clips), _ptr(out), B, T, h, w, _ptr(field) if field.shape[0] else c_void_p(0),
                                               field.shape[0], _ptr(field_of_clip), _stream()), "dfd_elastic_remap_u8")
    return out


_profile = {"epilogue": None, "events": [], "base": None}


def swiglu_fwd(x12, hidden):
    """hidden[r, j] = silu(x12[r, j]) * x12[r, H + j] (include/dfdclip_swiglu.h): x12 [rows, 2H], hidden [rows, H], both bf16 or both
    f32, unit column stride, any row stride (views of wider buffers are fine); x12 is read once, nothing between the rows of
    `hidden` is written."""
    _dev(x12, hidden)
    assert x12.dim() == 2 and hidden.dim() == 2 and x12.shape == (hidden.shape[0], 2 * hidden.shape[1]), (x12.shape, hidden.shape)
    assert x12.dtype == hidden.dtype and x12.dtype in _DTYPE, (x12.dtype, hidden.dtype)
    assert x12.stride(1) == 1 and hidden.stride(1) == 1
    rows, H = hidden.shape
    _check(load_library().dfd_swiglu_fwd(_ptr(x12), x12.stride(0) if rows > 1 else max(x12.stride(0), 2 * H), _ptr(hidden),
                                         hidden.stride(0) if rows > 1 else max(hidden.stride(0), H), _DTYPE[x12.dtype], rows, H, _stream()),
           "dfd_swiglu_fwd")
    return hidden


def swiglu_last_path():
    """SWIGLU_VEC16 / SWIGLU_ELEMENT: the form the last `swiglu_fwd` of this thread launched (0: none, or a no-op)."""
    return load_library().dfd_swiglu_last_path()


def kv_gather_patches(k, v, index, pos, k_out=None, v_out=None, T=1, P=None, index_host=None):
    """k_out[l, f*S + j] = k[l, f, index[l, j]] (+ pos[f % T]), the same for v (include/dfdclip_kvgather.h): the kept patch rows
    of patch-masked training, K and V of every tapped layer in one launch.

    k, v: two views of one layout, bf16 or f32 — 4-D [L, frames, P, D] with unit column stride and any other strides (the
    views `extract_kv(in_place=)` returns), or contiguous 3-D [L, frames*P, D] with `P=` given.  index: device int32 [L, S].
    pos: device f32 [T, D] or None.  k_out / v_out: contiguous [L, frames*S, D] of the sources' dtype, allocated when None.
    Raises before the launch when the table has an entry outside [0, P) (the kernel would clamp it): `index_host` is the
    host copy to look at — without it the device table is copied back, which synchronises.  Returns (k_out, v_out)."""
    _dev(k, v, index, pos, k_out, v_out)
    assert k.dtype == v.dtype and k.dtype in _DTYPE, (k.dtype, v.dtype)
    assert k.shape == v.shape and k.stride() == v.stride(), "k and v are two views of one layout"
    if k.dim() == 4:
        L, frames, P_, D = k.shape
        assert P is None or P == P_, (P, P_)
        assert k.stride(3) == 1 or D <= 1, "rows are dense: unit column stride"
        s_layer, s_frame, s_patch = k.stride(0), k.stride(1), k.stride(2)
    else:
        assert k.dim() == 3 and k.is_contiguous() and v.is_contiguous() and P is not None and P > 0 and k.shape[1] % P == 0, (k.shape, P)
        L, D, P_ = k.shape[0], k.shape[2], int(P)
        frames = k.shape[1] // P_
        s_layer, s_frame, s_patch = frames * P_ * D, P_ * D, D
    # (a dimension of size 1 may carry any stride in torch; the ABI wants stride_patch >= D whatever the sizes)
    s_patch = max(s_patch, D)
    assert index.dtype == torch.int32 and index.dim() == 2 and index.shape[0] == L and index.is_contiguous(), (index.shape, index.dtype, L)
    S = index.shape[1]
    host = index.cpu() if index_host is None else index_host
    assert tuple(host.shape) == (L, S), (host.shape, L, S)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= P_):
        raise DfdError(f"kv_gather_patches: the index table has an entry outside [0, {P_}) (min {int(host.min())}, max {int(host.max())})")
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and tuple(pos.shape) == (T, D), (pos.shape, pos.dtype, T, D)
    if k_out is None:
        k_out = torch.empty(L, frames * S, D, device=k.device, dtype=k.dtype)
    if v_out is None:
        v_out = torch.empty(L, frames * S, D, device=k.device, dtype=k.dtype)
    for o in (k_out, v_out):
        assert tuple(o.shape) == (L, frames * S, D) and o.dtype == k.dtype and o.is_contiguous(), (o.shape, o.dtype)
    if k_out.numel() == 0:
        return k_out, v_out  # (an empty tensor has no address to hand over; the ABI's no-op)
    _check(load_library().dfd_kv_gather_patches(_ptr(k), _ptr(v), _DTYPE[k.dtype], s_layer, s_frame, s_patch, _ptr(index), _ptr(pos),
                                                _ptr(k_out), _ptr(v_out), L, frames, int(T), P_, S, D, _stream()), "dfd_kv_gather_patches")
    return k_out, v_out


def kv_gather_last_path():
    """KVGATHER_VEC16 / KVGATHER_ELEMENT: the form the last `kv_gather_patches` of this thread launched (0: none, or a no-op)."""
    return load_library().dfd_kv_gather_last_path()


def _frame_table(name, table, host, frames):
    """Checks one side's frame table of `kv_move_frames`; returns (its length or None, the host copy or None)."""
    if table is None:
        return None, None
    assert table.dtype == torch.int32 and table.dim() == 1 and table.is_contiguous(), (name, table.shape, table.dtype)
    host = table.cpu() if host is None else torch.as_tensor(host)
    assert host.numel() == table.numel(), (name, host.shape, table.shape)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= frames):
        raise DfdError(f"kv_move_frames: {name} has an entry outside [0, {frames}) (min {int(host.min())}, max {int(host.max())})")
    return table.numel(), host


def kv_move_frames(k, v, k_out, v_out, src_frame=None, dst_frame=None, src_once=False, src_host=None, dst_host=None):
    """k_out[l, dst_frame[i], p] = k[l, src_frame[i], p], the same for v (include/dfdclip_kvframes.h): whole frames of K and V of
    every tapped layer in one launch, bits copied.

    k, v: two views of one layout [L, src_frames, P, D], bf16 or f32, unit column stride and any other strides (the views
    `extract_kv(in_place=)` returns, or a dense store).  k_out, v_out: the same for the destination, [L, dst_frames, P, D].
    src_frame / dst_frame: device int32 [n], or None for the identity (then n is the other table's length, or the frame
    count both sides share).  src_once: the source is read once (an ingest), so its loads follow the STREAM_DECODER_KV bit.
    Raises before the launch when a table has an entry outside its side, or dst_frame names a frame twice (the kernel
    would clamp the one and race on the other): `src_host` / `dst_host` are the host copies to look at — without them the
    device tables are copied back, which synchronises.  Returns (k_out, v_out)."""
    _dev(k, v, k_out, v_out, src_frame, dst_frame)
    assert k.dtype == v.dtype == k_out.dtype == v_out.dtype and k.dtype in _DTYPE, (k.dtype, v.dtype, k_out.dtype, v_out.dtype)
    assert k.dim() == 4 and k.shape == v.shape and k.stride() == v.stride(), "k and v are two views of one layout"
    assert k_out.dim() == 4 and k_out.shape == v_out.shape and k_out.stride() == v_out.stride(), "k_out and v_out are two views of one layout"
    L, src_frames, P, D = k.shape
    assert (k_out.shape[0], k_out.shape[2], k_out.shape[3]) == (L, P, D), (k.shape, k_out.shape)
    dst_frames = k_out.shape[1]
    assert (k.stride(3) == 1 and k_out.stride(3) == 1) or D <= 1, "rows are dense: unit column stride"
    n_src, _ = _frame_table("src_frame", src_frame, src_host, src_frames)
    n_dst, host = _frame_table("dst_frame", dst_frame, dst_host, dst_frames)
    if n_src is not None and n_dst is not None:
        assert n_src == n_dst, (n_src, n_dst)
    n = n_src if n_src is not None else n_dst
    if n is None:
        assert src_frames == dst_frames, "without a table both sides hold the same frames"
        n = src_frames
    if (src_frame is None and n > src_frames) or (dst_frame is None and n > dst_frames):
        raise DfdError(f"kv_move_frames: {n} frames under an identity table exceed that side (src {src_frames}, dst {dst_frames})")
    if host is not None and len(set(host.tolist())) != host.numel():
        raise DfdError("kv_move_frames: dst_frame names a frame twice: two moves into one frame would race")
    if L == 0 or n == 0 or P == 0 or D == 0:
        return k_out, v_out  # (an empty tensor has no address to hand over; the ABI's no-op)
    # (a dimension of size 1 may carry any stride in torch; the ABI wants stride_patch >= D whatever the sizes)
    _check(load_library().dfd_kv_move_frames(_ptr(k), _ptr(v), _ptr(k_out), _ptr(v_out), _DTYPE[k.dtype], k.stride(0), k.stride(1),
                                             max(k.stride(2), D), k_out.stride(0), k_out.stride(1), max(k_out.stride(2), D),
                                             _ptr(src_frame), _ptr(dst_frame), L, n, src_frames, dst_frames, P, D,
                                             KVFRAMES_SRC_ONCE if src_once else 0, _stream()), "dfd_kv_move_frames")
    return k_out, v_out


def kv_move_last_path():
    """KVFRAMES_VEC16 / KVFRAMES_ELEMENT: the form the last `kv_move_frames` of this thread launched (0: none, or a no-op)."""
    return load_library().dfd_kv_move_last_path()


def profile_gemm(epilogue=None):
    """Time every `gemm` launch with this epilogue from now on: a HIP event pair is recorded on
    the launch stream around the kernel (bench.py's roofline leg).  None switches it off."""
    _profile["epilogue"] = epilogue
    _profile["events"] = []
    _profile["base"] = None
    if epilogue is not None:
        _profile["base"] = torch.cuda.Event(enable_timing=True)
        _profile["base"].record()


def profile_gemm_collect():
    """(start_ms, end_ms, FLOPs) of each timed launch since `profile_gemm`, on one time base (launches
    may sit on different streams and overlap); call after a device sync."""
    base = _profile["base"]
    spans = [(base.elapsed_time(a), base.elapsed_time(b), flops) for a, b, flops in _profile["events"]]
    profile_gemm(None)
    return spans


def gemm(a, w, c, bias=None, epilogue=EPI_BIAS, m=None, pos=None, cls=None, k_export=None, v_export=None, tokens=0,
         frames_per_clip=0, residual=None, qkv_first=0, drop=None, stream_out=False, spare_cus=0, tile_blocks=0, spare_if_free=False,
         c_blocked=False, a_blocked=False):
    """c = epilogue(a[M,K] @ w[N,K]^T).  `m` limits the rows used (buffers may be over-allocated).
    `c_blocked` / `a_blocked`: the halves of a c_fc -> c_proj pair whose intermediate is kept fragment-blocked
    (blocked.py; `w`, `bias` of the c_fc half are then the permuted copies, `blocked.fc_channel_perm`)."""
    _dev(a, w, c, bias, pos, cls, k_export, v_export, residual)
    assert a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1 and c.stride(1) == 1
    M = a.shape[0] if m is None else m
    N, K = w.shape
    assert a.shape[1] == K
    assert residual is None or (residual.dtype == c.dtype and residual.stride(0) == c.stride(0))
    assert drop is None or epilogue == EPI_RESIDUAL_POS
    assert 0 <= epilogue <= EPI_BIAS_GELU, f"unknown epilogue {epilogue}"
    if c_blocked or a_blocked:  # whole row groups of 16 behind the pointer
        blk = c if c_blocked else a
        assert blk.shape[0] >= (M + 15) // 16 * 16, "a blocked matrix needs its rows rounded up to 16"
    extra = GemmExtra(_ptr(pos).value, _ptr(cls).value, _ptr(k_export).value, _ptr(v_export).value, tokens, frames_per_clip,
                      _ptr(residual).value, qkv_first, drop.rng.data_ptr() if drop is not None and drop.p > 0 else None,
                      drop.site if drop is not None else 0, drop.p if drop is not None else 0.0, (GEMM_STREAM_OUT if stream_out else 0) | (GEMM_SPARE_IF_FREE if spare_if_free else 0) | ((int(spare_cus) & 0xff) << 8) | ((int(tile_blocks) & 0xf) << 16)
                      | (GEMM_C_BLOCKED if c_blocked else 0) | (GEMM_A_BLOCKED if a_blocked else 0))
    timed = _profile["epilogue"] == epilogue
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _check(load_library().dfd_gemm(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _DTYPE[a.dtype], _ptr(c), c.stride(0),
                                   _DTYPE[c.dtype], _ptr(bias), epilogue, ctypes.byref(extra), M, N, K, _stream()), "dfd_gemm")
    if timed:
        e1.record()
        _profile["events"].append((e0, e1, 2.0 * M * N * K))
    return c


def gemm_fp8(a, w, c, col_scale, bias=None, epilogue=EPI_BIAS, m=None, out_inv_scale=0.0, pos=None, k_export=None, v_export=None,
             tokens=0, frames_per_clip=0, qkv_first=0, stream_out=False, spare_cus=0, spare_if_free=False):
    """c = epilogue((a[M,K] @ w[N,K]^T) * col_scale + bias) on e4m3 operands (uint8 / float8_e4m3fn storage);
    c bf16, or e4m3 bytes of result * out_inv_scale."""
    _dev(a, w, c, col_scale, bias, pos, k_export, v_export)
    assert a.element_size() == 1 and w.element_size() == 1 and a.stride(1) == 1 and w.stride(1) == 1 and c.stride(1) == 1
    assert col_scale.dtype == torch.float32 and col_scale.is_contiguous()
    M = a.shape[0] if m is None else m
    N, K = w.shape
    assert a.shape[1] == K and col_scale.numel() == N
    c_dtype = FP8 if c.element_size() == 1 else _DTYPE[c.dtype]
    extra = GemmExtra(_ptr(pos).value, None, _ptr(k_export).value, _ptr(v_export).value, tokens, frames_per_clip, None, qkv_first,
                      None, 0, 0.0, (GEMM_STREAM_OUT if stream_out else 0) | (GEMM_SPARE_IF_FREE if spare_if_free else 0) | ((int(spare_cus) & 0xff) << 8))
    timed = _profile["epilogue"] == epilogue
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _check(load_library().dfd_gemm_fp8(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(c), c.stride(0), c_dtype, _ptr(col_scale),
                                       _ptr(bias), float(out_inv_scale), epilogue, ctypes.byref(extra), M, N, K, _stream()),
           "dfd_gemm_fp8")
    if timed:
        e1.record()
        _profile["events"].append((e0, e1, 2.0 * M * N * K))
    return c


def gemm_set_variant(variant):
    """0 = every GEMM kernel eligible, tiles dealt statically (default); 1 = skip the ping-pong kernel (tests / A-B runs);
    3 = the ping-pong kernel hands its tiles out dynamically (per-XCD counters).  Per thread.  Returns the previous value."""
    return load_library().dfd_gemm_set_variant(int(variant))


def gemm_pair_set_variant(variant):
    """The c_fc -> c_proj pair: 0 = fragment-blocked intermediate where `gemm_pair_plan` says so (default); 1 = row-major
    everywhere (the A/B switch; a flagged call keeps its kernel and runs row-major); 2 = the plan also answers 1 below
    1024 rows (tests).  Per thread.  Returns the previous value."""
    return load_library().dfd_gemm_pair_set_variant(int(variant))


def gemm_pair_plan(M, D, H):
    """True where an MLP pair [M, D] -> [M, H] -> [M, D] on dense bf16 operands keeps its intermediate fragment-blocked."""
    return bool(load_library().dfd_gemm_pair_plan(int(M), int(D), int(H)))


def gemm_pair_launches():
    """This thread's `gemm` launches so far that wrote or read a fragment-blocked matrix."""
    return load_library().dfd_gemm_pair_launches()


def stream_policy_set(mask):
    """Which kernel families issue their read-once loads / write-once stores non-temporally (STREAM_* bits; results are
    bit-identical either way).  Process-wide, read at launch: a captured graph keeps what was set at capture.  Returns the
    previous mask."""
    return load_library().dfd_stream_policy_set(int(mask))


def stream_policy_get():
    return load_library().dfd_stream_policy_get()


def gemm_last_path():
    """257 / 256 when this thread's last gemm ran on the ping-pong / another tuned 256x256 bf16 kernel, 128 for the general kernel."""
    return load_library().dfd_gemm_last_path()


def gemm_last_kernel():
    """GEMM_* of this thread's last `gemm` or `gemm_fp8` that launched a kernel; 0 = none yet."""
    return load_library().dfd_gemm_last_kernel()


def gemm_plan(ab_dtype, c_dtype, epilogue, M, N, K, lda=None, ldw=None, ldc=None, flags=0, tokens=0, frames_per_clip=0, qkv_first=0,
              has=0, misaligned=0, n_cu=256):
    """What `gemm` (ab_dtype F32 / BF16) or `gemm_fp8` (FP8) would do with this call under the thread's variants: a GemmPlan,
    or DfdError for what the entry point refuses.  Dtypes are ABI codes; dense rows unless a leading dimension is given;
    `flags` as GemmExtra.flags; `has` / `misaligned`: GEMM_PTR_* bits.  No pointer and, with `n_cu` > 0, no device."""
    out = GemmPlan()
    rc = load_library().dfd_gemm_plan(ab_dtype, c_dtype, epilogue, M, N, K, K if lda is None else lda, K if ldw is None else ldw,
                                      N if ldc is None else ldc, flags, tokens, frames_per_clip, qkv_first, has, misaligned, n_cu,
                                      ctypes.byref(out))
    if rc < 0:
        raise DfdError(f"dfd_gemm_plan failed ({rc}): {load_library().dfd_last_error().decode()}")
    return out


def gemm_at_b_workspace_bytes(R, Ma, Nb, dtype):
    return load_library().dfd_gemm_at_b_workspace(R, Ma, Nb, _DTYPE[dtype])


def gemm_at_b_last_path():
    """128 / 256 when this thread's last gemm_at_b ran on the gemm_tn kernel of that tile width, 1 for the transpose +
    general-kernel fallback, 0 before any call."""
    return load_library().dfd_gemm_at_b_last_path()


def gemm_at_b(a, b, c, workspace):
    """c[Ma, Nb] (f32) = a[R, Ma]^T @ b[R, Nb]."""
    _dev(a, b, c, workspace)
    assert a.dtype == b.dtype and a.stride(1) == 1 and b.stride(1) == 1 and c.is_contiguous() and c.dtype == torch.float32
    R, Ma = a.shape
    Nb = b.shape[1]
    assert b.shape[0] == R and tuple(c.shape) == (Ma, Nb)
    assert workspace.numel() * workspace.element_size() >= gemm_at_b_workspace_bytes(R, Ma, Nb, a.dtype)
    _check(load_library().dfd_gemm_at_b(_ptr(a), a.stride(0), _ptr(b), b.stride(0), _DTYPE[a.dtype], _ptr(c), R, Ma, Nb,
                                        _ptr(workspace), _stream()), "dfd_gemm_at_b")
    return c


def adapter_norm_gelu(a, y, weight, bias, frames, patches, x, joint, eps=1e-5):
    """y = GELU(LayerNorm(a)) on [frames, patches, x]; mode `joint`: 0 per row, 1 statistics over (patches, x),
    2 = LayerNorm(GELU(a)) per row.  a may be f32 with a bf16 y."""
    _dev(a, y, weight, bias)
    assert (a.dtype == y.dtype or a.dtype == torch.float32) and a.is_contiguous() and y.is_contiguous()
    assert weight.is_contiguous() and bias.is_contiguous()
    _check(load_library().dfd_adapter_norm_gelu(_ptr(a), _DTYPE[a.dtype], _ptr(y), _DTYPE[y.dtype], _ptr(weight), _ptr(bias), frames,
                                                patches, x, int(joint), eps, _stream()), "dfd_adapter_norm_gelu")
    return y


def adapter_norm_gelu_bwd_workspace_bytes(frames, patches, x, joint):
    return load_library().dfd_adapter_norm_gelu_bwd_workspace(frames, patches, x, int(joint))


def adapter_norm_gelu_bwd(a, dy, da, weight, bias, dweight, dbias, workspace, frames, patches, x, joint, eps=1e-5):
    _dev(a, dy, da, weight, bias, dweight, dbias, workspace)
    assert dy.dtype == da.dtype and (a.dtype == dy.dtype or a.dtype == torch.float32)
    assert a.is_contiguous() and dy.is_contiguous() and da.is_contiguous()
    _check(load_library().dfd_adapter_norm_gelu_bwd(_ptr(a), _DTYPE[a.dtype], _ptr(dy), _ptr(da), _DTYPE[dy.dtype], _ptr(weight), _ptr(bias),
                                                    _ptr(dweight), _ptr(dbias), _ptr(workspace), frames, patches, x, int(joint),
                                                    eps, _stream()), "dfd_adapter_norm_gelu_bwd")
    return da


def attention_set_variant(variant):
    """0 = default; 1 = the rows kernel stages K and V in 16-key chunks at every token count (bit-identical to the whole-head
    form); 2 = skip the streaming bf16 MFMA kernel, so the rows kernel serves what it served before.  Per thread.  Returns
    the previous value."""
    return load_library().dfd_attention_set_variant(int(variant))


def attention_last_path():
    """ATTN_* of the kernel that served this thread's last successful attention_fwd, 0 before any."""
    return load_library().dfd_attention_last_path()


def attention_plan(dtype, n_frames, tokens, heads, ld_qkv=None, ld_out=None, n_cu=256):
    """What attention_fwd would launch for this shape under the thread's variant: an AttentionPlan (path, grid, block,
    chunk, lds).  Dense rows unless ld_qkv / ld_out (elements) are given; n_cu <= 0 asks the current device.  Raises
    DfdError for a shape attention_fwd refuses.  Touches no device with n_cu > 0."""
    D = heads * 64
    plan = AttentionPlan()
    rc = load_library().dfd_attention_plan(_DTYPE[dtype], n_frames, tokens, heads, 3 * D if ld_qkv is None else ld_qkv,
                                           D if ld_out is None else ld_out, n_cu, ctypes.byref(plan))
    if rc < 0:
        raise DfdError(f"dfd_attention_plan failed ({rc}): {load_library().dfd_last_error().decode()}")
    return plan


def attention_fwd(qkv, out, n_frames, tokens, heads, head_dim=64):
    _dev(qkv, out)
    assert qkv.dtype == out.dtype and qkv.stride(1) == 1 and out.stride(1) == 1
    _check(load_library().dfd_attention_fwd(_ptr(qkv), qkv.stride(0), _ptr(out), out.stride(0), _DTYPE[qkv.dtype], n_frames,
                                            tokens, heads, head_dim, head_dim ** -0.5, _stream()), "dfd_attention_fwd")
    return out


def linear_rows(x, w, bias, y, epilogue=EPI_BIAS):
    _dev(x, w, bias, y)
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and y.dtype == torch.float32
    assert x.stride(1) == 1 and y.stride(1) == 1 and w.is_contiguous()
    B, K = x.shape
    N = w.shape[0]
    _check(load_library().dfd_linear_rows(_ptr(x), x.stride(0), _ptr(w), _ptr(bias), _ptr(y), y.stride(0), epilogue, B, N, K,
                                          _stream()), "dfd_linear_rows")
    return y


def linear_rows_t_workspace_bytes(B, N, K):
    return load_library().dfd_linear_rows_t_workspace(B, N, K)


def linear_rows_t(x, wt, bias, y, workspace, epilogue=EPI_BIAS, residual=None):
    """y[B,N] = epilogue(x[B,K] @ wt[K,N] + bias): forward with wt = weight^T, data gradient with wt = weight.
    EPI_BIAS_RESIDUAL adds `residual` [B,N] (None: y itself, in place)."""
    _dev(x, wt, bias, y, workspace, residual)
    assert residual is None or (residual.dtype == torch.float32 and residual.stride(1) == 1 and residual.shape == y.shape)
    assert x.dtype == torch.float32 and wt.dtype == torch.float32 and y.dtype == torch.float32
    assert x.stride(1) == 1 and y.stride(1) == 1 and wt.is_contiguous()
    B, K = x.shape
    N = wt.shape[1]
    assert wt.shape[0] == K and workspace.numel() * workspace.element_size() >= linear_rows_t_workspace_bytes(B, N, K)
    _check(load_library().dfd_linear_rows_t(_ptr(x), x.stride(0), _ptr(wt), _ptr(bias), _ptr(residual),
                                            residual.stride(0) if residual is not None else 0, _ptr(y), y.stride(0), epilogue, B, N, K,
                                            _ptr(workspace), _stream()), "dfd_linear_rows_t")
    return y


def decoder_attn_workspace_bytes(B, heads, d, splits):
    return load_library().dfd_decoder_attn_workspace(B, heads, d, splits)


class KvLayoutDesc(ctypes.Structure):
    """dfd_kv_layout_t"""
    _fields_ = [("row_stride", c_int64), ("frame_stride", c_int64), ("pos", c_void_p)]


def _kv_layout(x, other, pos, B, T, patches, D):
    """Keys / values as the dense export [B*T*patches, D] (contiguous, any leading shape) or as a strided view
    [B*T, patches, D] of a larger activation (e.g. qkv[:, 1:, D:2*D] of the encoder's [frames, tokens, 3*D]);
    `pos` [T, D] f32: temporal positional embedding added on the fly.  Returns (layout or None, keep-alive)."""
    if other is not None:
        assert other.dtype == x.dtype and other.shape == x.shape and other.stride() == x.stride()
    if x.is_contiguous() and pos is None:
        assert x.numel() == B * T * patches * D
        return None, None
    if x.is_contiguous():
        rs, fs = D, patches * D
    else:
        assert x.dim() == 3 and x.shape == (B * T, patches, D) and x.stride(2) == 1, "strided K/V must be [B*T, patches, D] views"
        fs, rs = x.stride(0), x.stride(1)
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape == (T, D) and pos.device == x.device
    lay = KvLayoutDesc(rs, fs, pos.data_ptr() if pos is not None else None)
    return ctypes.byref(lay), lay


def decoder_attn_fwd(q, k, v, frame_mask, mix, stats, workspace, splits, B, T, patches, heads, d=64, mix_softmax=None,
                     ext_weights=None, pos=None):
    _dev(q, k, v, frame_mask, mix, stats, workspace, mix_softmax, ext_weights)
    assert q.dtype == torch.float32 and q.is_contiguous()
    assert frame_mask.dtype == torch.uint8 and frame_mask.is_contiguous()
    assert ext_weights is None or (ext_weights.is_contiguous() and ext_weights.numel() == B * heads * T * patches)
    lay, _keep = _kv_layout(k, v, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _DTYPE[k.dtype], lay, _ptr(frame_mask), _ptr(ext_weights),
                                               _ptr(mix), _ptr(mix_softmax), _ptr(stats), _ptr(workspace), splits, B, T, patches,
                                               heads, d, _stream()),
           "dfd_decoder_attn_fwd")
    return mix


ATTN_MODE_BITS = {"frame": 1, "temporal": 2}


def decoder_attn_modes_fwd(q, k, frame_mask, modes, scores, weights, B, T, patches, heads, d=64, pos=None):
    """attn_mode softmax branch: scores [B,heads,S] and grouped-softmax weights [B,heads,S]."""
    _dev(q, k, frame_mask, scores, weights)
    assert q.is_contiguous() and scores.is_contiguous() and weights.is_contiguous()
    assert scores.numel() == B * heads * T * patches == weights.numel()
    lay, _keep = _kv_layout(k, None, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_modes_fwd(_ptr(q), _ptr(k), _DTYPE[k.dtype], lay, _ptr(frame_mask), modes, _ptr(scores),
                                                     _ptr(weights), B, T, patches, heads, d, _stream()),
           "dfd_decoder_attn_modes_fwd")
    return weights


def decoder_attn_map(q, k, frame_mask, stats, aff, B, T, patches, heads, d=64, ext_weights=None, branches=None, pos=None):
    """aff [B,heads,S] f32 = the per-key weight ½(softmax + CoDA) that `decoder_attn_fwd` applied to v, from the `stats` it
    wrote (or `ext_weights` under attn_mode; `stats` may then be None); `branches` [2,B,heads,S]: the two weights without
    the ½.  K as for the forward: dense, or a strided view with `pos` added on the fly."""
    _dev(q, k, frame_mask, stats, aff, ext_weights, branches)
    assert q.dtype == torch.float32 and q.is_contiguous()
    assert frame_mask.dtype == torch.uint8 and frame_mask.is_contiguous()
    n = B * heads * T * patches
    assert aff.dtype == torch.float32 and aff.is_contiguous() and aff.numel() == n
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == B * heads * 2)
    assert ext_weights is None or (ext_weights.dtype == torch.float32 and ext_weights.is_contiguous() and ext_weights.numel() == n)
    assert branches is None or (branches.dtype == torch.float32 and branches.is_contiguous() and branches.numel() == 2 * n)
    lay, _keep = _kv_layout(k, None, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_map(_ptr(q), _ptr(k), _DTYPE[k.dtype], lay, _ptr(frame_mask), _ptr(stats), _ptr(ext_weights),
                                               _ptr(aff), _ptr(branches), B, T, patches, heads, d, _stream()),
           "dfd_decoder_attn_map")
    return aff


def _store_layout(who, k, v, table, table_host, pos, B, T, patches, D):
    """One layer of a frame store [C, patches, D] (contiguous, or a strided view with unit column stride) and the slot
    table of `decoder_attn_fwd_frames` / `decoder_attn_map_frames`, checked: -> (layout, keep-alive, store_frames).  Raises
    before any launch when the table has an entry outside [0, C) (the kernel would clamp it): `table_host` is the host copy to
    look at — without it the device table is copied back, which synchronises."""
    assert k.dim() == 3 and k.shape[1:] == (patches, D) and (k.stride(2) == 1 or D <= 1), f"{who}: a store layer is [C, {patches}, {D}] with unit column stride"
    if v is not None:
        assert v.dtype == k.dtype and v.shape == k.shape and v.stride() == k.stride(), f"{who}: k and v are two views of one layout"
    C = k.shape[0]
    assert table.dtype == torch.int32 and table.dim() == 1 and table.is_contiguous() and table.numel() == B * T, (who, table.shape, table.dtype)
    host = table.cpu() if table_host is None else torch.as_tensor(table_host)
    assert host.numel() == table.numel(), (who, host.shape, table.shape)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= C):
        raise DfdError(f"{who}: the frame table has an entry outside [0, {C}) (min {int(host.min())}, max {int(host.max())})")
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape == (T, D) and pos.device == k.device
    # (a dimension of size 1 may carry any stride in torch; the ABI wants row_stride >= D and frame_stride > 0 whatever the sizes)
    lay = KvLayoutDesc(max(k.stride(1), D), max(k.stride(0), 1), pos.data_ptr() if pos is not None else None)
    return ctypes.byref(lay), lay, C


def decoder_attn_fwd_frames(q, k, v, table, frame_mask, mix, stats, workspace, splits, B, T, patches, heads, d=64, mix_softmax=None,
                            ext_weights=None, pos=None, table_host=None):
    """`decoder_attn_fwd` with the keys and values of clip b's frame tf read at frame `table[b*T + tf]` of the store layer
    k, v [C, patches, D] (include/dfdclip_kvtable.h): no dense copy of the windows' frames.  `table`: device int32 [B*T];
    `frame_mask` [B, T] and `pos` [T, D] stay indexed by the clip's own frame."""
    _dev(q, k, v, table, frame_mask, mix, stats, workspace, mix_softmax, ext_weights)
    assert q.dtype == torch.float32 and q.is_contiguous()
    assert frame_mask.dtype == torch.uint8 and frame_mask.is_contiguous()
    assert ext_weights is None or (ext_weights.is_contiguous() and ext_weights.numel() == B * heads * T * patches)
    lay, _keep, C = _store_layout("decoder_attn_fwd_frames", k, v, table, table_host, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_fwd_frames(_ptr(q), _ptr(k), _ptr(v), _DTYPE[k.dtype], lay, _ptr(frame_mask), _ptr(ext_weights),
                                                      _ptr(mix), _ptr(mix_softmax), _ptr(stats), _ptr(workspace), splits, B, T, patches,
                                                      heads, d, _ptr(table), C, _stream()),
           "dfd_decoder_attn_fwd_frames")
    return mix


def decoder_attn_map_frames(q, k, table, frame_mask, stats, aff, B, T, patches, heads, d=64, ext_weights=None, branches=None, pos=None,
                            table_host=None):
    """`decoder_attn_map` over the store layer k [C, patches, D] and the slot table that `decoder_attn_fwd_frames` read."""
    _dev(q, k, table, frame_mask, stats, aff, ext_weights, branches)
    assert q.dtype == torch.float32 and q.is_contiguous()
    assert frame_mask.dtype == torch.uint8 and frame_mask.is_contiguous()
    n = B * heads * T * patches
    assert aff.dtype == torch.float32 and aff.is_contiguous() and aff.numel() == n
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == B * heads * 2)
    assert ext_weights is None or (ext_weights.dtype == torch.float32 and ext_weights.is_contiguous() and ext_weights.numel() == n)
    assert branches is None or (branches.dtype == torch.float32 and branches.is_contiguous() and branches.numel() == 2 * n)
    lay, _keep, C = _store_layout("decoder_attn_map_frames", k, None, table, table_host, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_map_frames(_ptr(q), _ptr(k), _DTYPE[k.dtype], lay, _ptr(frame_mask), _ptr(stats), _ptr(ext_weights),
                                                      _ptr(aff), _ptr(branches), B, T, patches, heads, d, _ptr(table), C, _stream()),
           "dfd_decoder_attn_map_frames")
    return aff


def decoder_attn_modes_bwd(scores, v, dmix, modes, dwv_ws, dscores, B, T, patches, heads, d=64, pos=None):
    _dev(scores, v, dmix, dwv_ws, dscores)
    assert scores.is_contiguous() and dmix.is_contiguous()
    assert dwv_ws.numel() >= B * heads * T * patches and dscores.numel() == B * heads * T * patches
    lay, _keep = _kv_layout(v, None, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_modes_bwd(_ptr(scores), _ptr(v), _DTYPE[v.dtype], lay, _ptr(dmix), modes, _ptr(dwv_ws),
                                                     _ptr(dscores), B, T, patches, heads, d, _stream()),
           "dfd_decoder_attn_modes_bwd")
    return dscores


def head_fwd(x, gamma, beta, proj, feat, raw, logits, eps=1e-5, drop=None):
    _dev(x, gamma, beta, proj, feat, raw, logits)
    B, D = x.shape
    assert proj.is_contiguous() and proj.shape[0] == D and feat.is_contiguous()
    _check(load_library().dfd_head_fwd(_ptr(x), x.stride(0), _ptr(gamma), _ptr(beta), _ptr(proj), _ptr(feat), _ptr(raw),
                                       _ptr(logits), B, D, proj.shape[1], eps, _drop(drop), _stream()), "dfd_head_fwd")
    return logits


# ---- adapter structs without a LayerNorm: 768-bn, 768-xxx-768, linear (csrc/adapter_structs.hip) -----------------

BN_EVAL, BN_TRAIN, BN_TRAIN_UPDATE = 0, 1, 2


def adapter_norm_gelu_last_path():
    """ADP_* of this thread's last adapter_norm_gelu or adapter_norm_gelu_bwd that launched a kernel; 0 = none yet."""
    return load_library().dfd_adapter_norm_gelu_last_path()


def adapter_norm_gelu_plan(frames, patches, x, joint, a_dtype, dtype, misaligned=False, backward=False):
    """What adapter_norm_gelu (or, with `backward`, adapter_norm_gelu_bwd) would do with this shape: an AdapterPlan (path ADP_*,
    grid, block, slabs, groups_per_slab).  DfdError for what the entry point refuses.  Touches no device."""
    p = AdapterPlan()
    rc = load_library().dfd_adapter_norm_gelu_plan(frames, patches, x, int(joint), _DTYPE[a_dtype], _DTYPE[dtype], int(bool(misaligned)),
                                                   int(bool(backward)), ctypes.byref(p))
    if rc < 0:
        raise DfdError(f"dfd_adapter_norm_gelu_plan failed ({rc}): {load_library().dfd_last_error().decode()}")
    return p


def adapter_bn_workspace_bytes(frames, patches, width):
    return load_library().dfd_adapter_bn_workspace(frames, patches, width)


def _bn_shape(t, frames, patches, width):
    assert t.is_contiguous() and t.numel() == frames * patches * width, (tuple(t.shape), frames, patches, width)


def adapter_bn_stats(y, stats, workspace, frames, patches, T, mode, running_mean=None, running_var=None,
                     num_batches_tracked=None, momentum=0.1, eps=1e-5):
    """stats [2, T] f32 = (mean, invstd) per frame channel t = frame % T of y [frames*patches, width]; mode BN_EVAL reads
    the running statistics, BN_TRAIN_UPDATE also advances them (and num_batches_tracked) on the device."""
    _dev(y, stats, workspace, running_mean, running_var, num_batches_tracked)
    width = y.shape[-1]
    _bn_shape(y, frames, patches, width)
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2 * T
    for b in (running_mean, running_var):
        assert b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.numel() == T)
    assert num_batches_tracked is None or num_batches_tracked.dtype == torch.int64
    assert workspace.numel() * workspace.element_size() >= adapter_bn_workspace_bytes(frames, patches, width)
    _check(load_library().dfd_adapter_bn_stats(_ptr(y), _DTYPE[y.dtype], _ptr(stats), _ptr(running_mean), _ptr(running_var),
                                               _ptr(num_batches_tracked), _ptr(workspace), frames, patches, width, T, int(mode),
                                               momentum, eps, _stream()), "dfd_adapter_bn_stats")
    return stats


def adapter_bn_apply(y, out, frames, patches, T, stats=None, gamma=None, beta=None, residual=None, pos=None, drop=None):
    """out = residual + drop(γ_t·(y - μ_t)·invstd_t + β_t) + pos[t]; stats None: out = residual + drop(y) + pos."""
    _dev(y, out, stats, gamma, beta, residual, pos)
    width = y.shape[-1]
    _bn_shape(y, frames, patches, width)
    _bn_shape(out, frames, patches, width)
    assert residual is None or (residual.dtype == out.dtype and residual.is_contiguous() and residual.numel() == out.numel())
    assert pos is None or (pos.dtype == torch.float32 and pos.is_contiguous() and pos.numel() == T * width)
    _check(load_library().dfd_adapter_bn_apply(_ptr(y), _DTYPE[y.dtype], _ptr(residual), _ptr(out), _DTYPE[out.dtype], _ptr(stats),
                                               _ptr(gamma), _ptr(beta), _ptr(pos), _drop(drop), frames, patches, width, T,
                                               _stream()), "dfd_adapter_bn_apply")
    return out


def adapter_bn_bwd(y, dout, dy, stats, gamma, dgamma, dbeta, workspace, frames, patches, T, train, drop=None):
    """dy (dtype of y) and dγ / dβ [T] of out = drop(BN(y)); dout in y's dtype or f32."""
    _dev(y, dout, dy, stats, gamma, dgamma, dbeta, workspace)
    width = y.shape[-1]
    for t in (y, dout, dy):
        _bn_shape(t, frames, patches, width)
    assert dy.dtype == y.dtype and dout.dtype in (y.dtype, torch.float32)
    assert workspace.numel() * workspace.element_size() >= adapter_bn_workspace_bytes(frames, patches, width)
    _check(load_library().dfd_adapter_bn_bwd(_ptr(y), _ptr(dout), _DTYPE[dout.dtype], _ptr(dy), _DTYPE[y.dtype], _ptr(stats),
                                             _ptr(gamma), _ptr(dgamma), _ptr(dbeta), _drop(drop), _ptr(workspace), frames,
                                             patches, width, T, int(bool(train)), _stream()), "dfd_adapter_bn_bwd")
    return dy


def gelu_erf(a, out, drop=None):
    """out = drop(GELU(a)), nn.GELU()'s erf form."""
    _dev(a, out)
    assert a.is_contiguous() and out.is_contiguous() and a.numel() == out.numel()
    _check(load_library().dfd_gelu_erf(_ptr(a), _DTYPE[a.dtype], _ptr(out), _DTYPE[out.dtype], a.numel(), _drop(drop), _stream()),
           "dfd_gelu_erf")
    return out


def gelu_erf_bwd(a, dh, da, drop=None):
    """da = GELU'(a)·drop(dh)."""
    _dev(a, dh, da)
    assert a.is_contiguous() and dh.is_contiguous() and da.is_contiguous() and a.numel() == dh.numel() == da.numel()
    assert dh.dtype == da.dtype
    _check(load_library().dfd_gelu_erf_bwd(_ptr(a), _DTYPE[a.dtype], _ptr(dh), _DTYPE[dh.dtype], _ptr(da), _DTYPE[da.dtype], a.numel(),
                                           _drop(drop), _stream()), "dfd_gelu_erf_bwd")
    return da


def dropout(x, out, drop):
    """out = dropout(x) elementwise (element index = flat position); also its own backward.  In place allowed."""
    _dev(x, out)
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel() and drop is not None
    _check(load_library().dfd_dropout(_ptr(x), _DTYPE[x.dtype], _ptr(out), _DTYPE[out.dtype], x.numel(),
                                      ctypes.byref(drop.desc()), _stream()), "dfd_dropout")
    return out


# ---- decoder backward ------------------------------------------------------------------------

def decoder_attn_bwd_workspace_bytes(B, T, heads, d=64):
    return load_library().dfd_decoder_attn_bwd_workspace(B, T, heads, d)


def decoder_attn_bwd(q, k, v, frame_mask, dmix, mix_softmax, stats, dq, dpos, workspace, B, T, patches, heads, d=64, dk=None,
                     dv=None, ext_weights=None, ext_dscores=None, pos=None):
    _dev(q, k, v, frame_mask, dmix, mix_softmax, stats, dq, dpos, workspace, dk, dv, ext_weights, ext_dscores)
    assert q.is_contiguous() and dmix.is_contiguous()
    assert mix_softmax is None or mix_softmax.is_contiguous()
    lay, _keep = _kv_layout(k, v, pos, B, T, patches, heads * d)
    _check(load_library().dfd_decoder_attn_bwd(_ptr(q), _ptr(k), _ptr(v), _DTYPE[k.dtype], lay, _ptr(frame_mask), _ptr(dmix),
                                               _ptr(mix_softmax), _ptr(stats), _ptr(ext_weights), _ptr(ext_dscores), _ptr(dq),
                                               _ptr(dpos), _ptr(dk), _ptr(dv),
                                               _DTYPE[dk.dtype] if dk is not None else F32, _ptr(workspace), B, T, patches,
                                               heads, d, _stream()), "dfd_decoder_attn_bwd")
    return dq


def linear_rows_bwd_weight(dy, x, dw, db=None):
    _dev(dy, x, dw, db)
    assert dy.stride(1) == 1 and x.stride(1) == 1 and dw.is_contiguous()
    B, N = dy.shape
    K = x.shape[1]
    assert tuple(dw.shape) == (N, K)
    _check(load_library().dfd_linear_rows_bwd_weight(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dw), _ptr(db), B, N, K,
                                                     _stream()), "dfd_linear_rows_bwd_weight")
    return dw


def transpose(src, dst):
    _dev(src, dst)
    assert src.is_contiguous() and dst.is_contiguous() and src.dtype == torch.float32
    R, C = src.shape
    _check(load_library().dfd_transpose_f32(_ptr(src), _ptr(dst), R, C, _stream()), "dfd_transpose_f32")
    return dst


def sgd_blocks(numel, rows=0, cols=0, mirrored=False):
    return int(load_library().dfd_sgd_blocks(int(numel), int(rows), int(cols), 1 if mirrored else 0))


def adamw_extra(beta1, beta2, eps, step, exp_avg_sq):
    """The `extra` of an AdamW `sgd_step`: `exp_avg_sq` = device int64 tensor [n] of the second moments' addresses, parallel
    to the table; `step` = the count after this step (1 on the first)."""
    _dev(exp_avg_sq)
    assert exp_avg_sq.dtype == torch.int64 and exp_avg_sq.is_contiguous() and exp_avg_sq.dim() == 1
    return OptimExtra(OPTIM_ADAMW, 0, float(beta1), float(beta2), float(eps), int(step), exp_avg_sq.data_ptr())


def sgd_step(table, n, total_blocks, lr, momentum, weight_decay, first_step, extra=None):
    """`table`: device int64 tensor [n, 7] laid out as dfd_sgd_param (p, g, buf, mirror, numel, rows | cols << 32, first_block).
    `extra`: None = SGD; an `OptimExtra` (`adamw_extra`) = AdamW, `buf` then being exp_avg."""
    _dev(table)
    assert table.dtype == torch.int64 and table.is_contiguous() and table.shape == (n, 7)
    _check(load_library().dfd_sgd_step(_ptr(table), int(n), int(total_blocks), float(lr), float(momentum), float(weight_decay),
                                       1 if first_step else 0, _stream(), None if extra is None else ctypes.byref(extra)), "dfd_sgd_step")


def ema_factors(ratio):
    """(keep, take) of `ema_step`: the Python doubles 1 - r and r, which torch casts to f32 inside `(1 - r) * t + r * s`."""
    r = float(ratio)
    return 1.0 - r, r


def ema_step(table, n, total_blocks, ratio, table_host=None):
    """t <- (1 - ratio) t + ratio s over every entry of `table`, in one launch (include/dfdclip_ema.h).  `table`: device int64
    tensor [n, 7] laid out as dfd_sgd_param (`sgd_step`): p = the teacher's parameter, g = the student's, buf = 0, mirror =
    the teacher's transposed copy or 0.  Raises before the launch when an entry's p and g are one address, has a `buf` or
    a null pointer: `table_host` is the host copy to look at — without it the device table is copied back, which synchronises."""
    _dev(table)
    if table.dtype != torch.int64 or not table.is_contiguous() or table.dim() != 2 or tuple(table.shape) != (int(n), 7) or n <= 0:
        raise DfdError(f"ema_step: empty table, or not a contiguous int64 [n, 7] tensor (n={n}, table {tuple(table.shape)} {table.dtype})")
    host = table.cpu() if table_host is None else table_host
    if tuple(host.shape) != (int(n), 7):
        raise DfdError(f"ema_step: table_host is {tuple(host.shape)}, the table [{n}, 7]")
    if bool((host[:, 0] == host[:, 1]).any()):
        raise DfdError("ema_step: an entry blends a tensor with itself (p == g): (1 - r) x + r x is not x in f32; skip the pair")
    if bool((host[:, 0] == 0).any() or (host[:, 1] == 0).any() or (host[:, 2] != 0).any()):
        raise DfdError("ema_step: every entry needs p and g, and buf must be NULL")
    keep, take = ema_factors(ratio)
    _check(load_library().dfd_ema_step(_ptr(table), int(n), int(total_blocks), keep, take, _stream()), "dfd_ema_step")


def ema_reference(t, s, ratio):
    """What `ema_step` leaves in `t`'s place, restated op for op on NumPy arrays or torch tensors (any device): both
    products rounded to f32, then the sum — fadd(fmul(f32(1 - r), t), fmul(f32(r), s)).  Returns a new f32 array / tensor."""
    keep, take = ema_factors(ratio)
    if torch.is_tensor(t):
        k = torch.tensor(keep, dtype=torch.float32, device=t.device)
        r = torch.tensor(take, dtype=torch.float32, device=t.device)
        a = torch.mul(t.to(torch.float32), k)
        b = torch.mul(s.to(torch.float32), r)
        return torch.add(a, b)
    import numpy as np
    with np.errstate(all="ignore"):
        a = np.multiply(np.asarray(t, dtype=np.float32), np.float32(keep), dtype=np.float32)
        b = np.multiply(np.asarray(s, dtype=np.float32), np.float32(take), dtype=np.float32)
        return np.add(a, b, dtype=np.float32)


def layernorm_bwd(x, gamma, dy, dx, dgamma, dbeta, xhat_ws, accumulate_dx=False, eps=1e-5):
    _dev(x, gamma, dy, dx, dgamma, dbeta, xhat_ws)
    rows, cols = x.shape
    _check(load_library().dfd_layernorm_bwd(_ptr(x), x.stride(0), _ptr(gamma), _ptr(dy), dy.stride(0), _ptr(dx), dx.stride(0),
                                            _ptr(dgamma), _ptr(dbeta), _ptr(xhat_ws), rows, cols, eps, int(accumulate_dx),
                                            _stream()), "dfd_layernorm_bwd")
    return dx


def quickgelu(u, out, du=None, drop=None):
    _dev(u, out, du)
    assert u.is_contiguous() and out.is_contiguous() and (du is None or du.is_contiguous())
    _check(load_library().dfd_quickgelu(_ptr(u), _ptr(du), _ptr(out), u.numel(), _drop(drop), _stream()), "dfd_quickgelu")
    return out


def head_bwd(raw, dlogits, proj, feat, dfeat_ext, dz, dfeat, dproj):
    _dev(raw, dlogits, proj, feat, dfeat_ext, dz, dfeat, dproj)
    B, od = raw.shape
    D = proj.shape[0]
    assert dlogits.is_contiguous() and proj.is_contiguous() and feat.is_contiguous()
    _check(load_library().dfd_head_bwd(_ptr(raw), _ptr(dlogits), _ptr(proj), _ptr(feat), _ptr(dfeat_ext), _ptr(dz), _ptr(dfeat),
                                       _ptr(dproj), B, D, od, _stream()), "dfd_head_bwd")
    return dfeat


# ---- CompInvEncoder pair loss ------------------------------------------------------------------

def compinv_loss_workspace_bytes(P, D):
    return int(load_library().dfd_compinv_loss_workspace(int(P), int(D)))


def _compinv_check(k, v, B, T, P, L):
    assert k.dtype == v.dtype and k.shape == v.shape and k.is_contiguous() and v.is_contiguous()
    assert k.dim() == 3 and k.shape[0] == L and k.shape[1] == B * T * P, (tuple(k.shape), B, T, P, L)


def compinv_loss_fwd(k, v, B, T, P, workspace, match, norm, recon=None):
    """k, v [L, B*T*P, D] (the adapted K/V) -> workspace[:P*D] = M, match = ||M|| / P, norm = ||M||, recon = 0
    (device f32 scalars; nothing is read back)."""
    _dev(k, v, workspace, match, norm, recon)
    L, _, D = k.shape
    _compinv_check(k, v, B, T, P, L)
    assert workspace.dtype == torch.float32 and workspace.numel() * 4 >= compinv_loss_workspace_bytes(P, D)
    assert match.dtype == norm.dtype == torch.float32 and (recon is None or recon.dtype == torch.float32)
    _check(load_library().dfd_compinv_loss_fwd(_ptr(k), _ptr(v), _DTYPE[k.dtype], B, T, P, D, L, _ptr(workspace), _ptr(match),
                                               _ptr(norm), _ptr(recon), _stream()), "dfd_compinv_loss_fwd")
    return match


def compinv_loss_bwd(k, v, B, T, P, workspace, norm, grad, dk, dv):
    """dk, dv (dtype and layout of k, v) = d match / d (k, v) scaled by the device scalar `grad`."""
    _dev(k, v, workspace, norm, grad, dk, dv)
    L, _, D = k.shape
    _compinv_check(k, v, B, T, P, L)
    assert dk.dtype == dv.dtype == k.dtype and dk.shape == dv.shape == k.shape and dk.is_contiguous() and dv.is_contiguous()
    assert grad.dtype == norm.dtype == torch.float32 and grad.numel() == 1 and norm.numel() == 1
    _check(load_library().dfd_compinv_loss_bwd(_ptr(k), _ptr(v), _DTYPE[k.dtype], B, T, P, D, L, _ptr(workspace), _ptr(norm),
                                               _ptr(grad), _ptr(dk), _ptr(dv), _stream()), "dfd_compinv_loss_bwd")
    return dk, dv
