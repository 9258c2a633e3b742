"""ctypes binding of lib/libprobpose_hip.so (C ABI: include/probpose_hip.h)."""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libprobpose_hip.so")

PP_F32, PP_BF16, PP_FP8 = 0, 1, 2
PP_MAX_RADIUS = 9
PP_MAX_TAPS = 2 * PP_MAX_RADIUS + 1
EPI_BIAS, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_OUT_F32, EPI_ROWBIAS, EPI_HEATMAP = 1, 2, 4, 8, 16, 32, 64
DECODE_NO_WAVE, DECODE_SCREEN, DECODE_ALL_PIXEL, DECODE_WAVE = 1, 2, 4, 16
EPI_HEADMAJOR = 4096
EPI_OUT_FP8, EPI_NOCLAMP, EPI_FUSE_FINAL = 512, 1024, 2048      # 128 / 256: retired (LayerNorm fusion, round 1)

_lock = threading.Lock()
_lib = None


class HipExtensionError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p),
        ("bias", C.c_void_p), ("residual", C.c_void_p), ("rowbias", C.c_void_p),
        ("rowoff", C.c_void_p), ("out_rowmap", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("Kd", C.c_int),
        ("lda", C.c_int), ("ldw", C.c_int), ("ldc", C.c_int),
        ("seg_len", C.c_int), ("rowbias_period", C.c_int), ("batch", C.c_int),
        ("strideA", C.c_longlong), ("strideW", C.c_longlong), ("strideC", C.c_longlong),
        ("strideBias", C.c_longlong), ("strideRowoff", C.c_longlong), ("strideRowmap", C.c_longlong),
        ("dtype", C.c_int), ("epilogue", C.c_int),
        ("hm_K", C.c_int), ("hm_HW", C.c_int), ("hm_temperature", C.c_float),
        ("C2", C.c_void_p), ("ldc2", C.c_int), ("stats_out", C.c_void_p), ("stats_in", C.c_void_p),
        ("stats_parts", C.c_int), ("colsum", C.c_void_p), ("ln_eps", C.c_float), ("tile", C.c_int),
        ("out_scale", C.c_float),
        ("splitk", C.c_int),
        ("strideA_k", C.c_longlong), ("strideW_k", C.c_longlong), ("strideC_k", C.c_longlong),
        ("strideRowoff_k", C.c_longlong),
        ("final_w", C.c_void_p), ("final_b", C.c_void_p),
    ]


class WgradArgs(C.Structure):
    _fields_ = [
        ("dY", C.c_void_p), ("dy_rowmap", C.c_void_p), ("ldd", C.c_longlong),
        ("A", C.c_void_p), ("rowoff", C.c_void_p), ("seg_len", C.c_int), ("lda", C.c_int),
        ("dW", C.c_void_p), ("lddw", C.c_longlong),
        ("dB", C.c_void_p),
        ("parts", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("Kd", C.c_int), ("batch", C.c_int),
        ("strideDY", C.c_longlong), ("strideA", C.c_longlong), ("strideRowoff", C.c_longlong),
        ("strideRowmap", C.c_longlong), ("strideDW", C.c_longlong), ("strideDB", C.c_longlong),
        ("dtype", C.c_int),
    ]


_vp, _i, _f, _d = C.c_void_p, C.c_int, C.c_float, C.c_double
_SIGNATURES = {
    "pp_version": (C.c_int, []),
    "pp_last_error": (C.c_char_p, []),
    "pp_device_ok": (C.c_int, []),
    "pp_decode_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "pp_decode_f32": (C.c_int, [_vp] * 5 + [_i] * 4 + [_vp, _vp] + [_d] * 4 + [_vp] * 8 + [_i, _vp]),
    "pp_gemm": (C.c_int, [C.POINTER(GemmArgs), _vp]),
    "pp_layernorm": (C.c_int, [_vp, _vp, _vp, _f, _i, _i, _vp, _i, _vp]),
    "pp_layernorm_fp8": (C.c_int, [_vp, _vp, _vp, _f, _i, _i, _vp, _f, _vp]),
    "pp_attention": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "pp_attention_headmajor": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pp_attention_fp8out": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "pp_qkv_attention_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pp_patchify": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "pp_maxpool_relu": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pp_maxpool_relu_sum": (C.c_int, [_vp, _i, C.c_longlong, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pp_final_heatmap": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "pp_final_logits": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "pp_sparsemax_rows": (C.c_int, [_vp, C.c_longlong, _i, _f, _vp]),
    "pp_dark_decode_lds_bytes": (C.c_size_t, [_i, _i, _i]),
    "pp_dark_decode_f32": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _d, _d, _vp, _vp, _vp, _vp]),
    "pp_aux_tail": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pp_tokens_to_nchw": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pp_nchw_to_tokens": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pp_encode_probmaps": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pp_heatmap_argmax": (C.c_int, [_vp, C.c_longlong, _i, _i, _vp, _vp, _vp]),
    "pp_pck_counts": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _d, _i, _i, _vp, _vp, _vp]),
    "pp_frontend_plan_bytes": (C.c_longlong, [_i, _vp, _i, _i]),
    "pp_frontend_plan_build": (C.c_int, [_i, _vp, _i, _i, _vp, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "pp_frontend_crop_resize": (C.c_int, [_vp, _i, _i, C.c_longlong, _vp, _i, _i, C.c_longlong, _i, _i, _vp, _vp]),
    "pp_frontend_multi_plan_bytes": (C.c_longlong, [_i, _vp, _i, _i]),
    "pp_frontend_multi_plan_build": (C.c_int, [_i, _vp, _vp, C.c_longlong, _i, _i, _vp, C.POINTER(C.c_int),
                                               C.POINTER(C.c_longlong)]),
    "pp_frontend_crop_resize_multi": (C.c_int, [_vp, _vp, _i, _i, C.c_longlong, _i, _i, _vp, _vp]),
    "pp_dataset_ground_truth": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _f, _f] + [_vp] * 7),
    "pp_augment_check": (C.c_int, [_i, _vp, C.c_longlong, _vp, _vp, _i, _vp]),
    "pp_augment_warp": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pp_dataset_ground_truth_affine": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f] + [_vp] * 7),
    "pp_augment_post_check": (C.c_int, [_i, _vp, _i, _i, _i]),
    "pp_augment_post": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pp_hflip_pair": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pp_flip_merge": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pp_oks_heatmap_loss": (C.c_int, [_vp, _vp, _vp, _i, _vp, C.c_longlong, C.c_longlong, _i, _i] + [_f] * 4
                            + [_i] * 4 + [_vp] * 5),
    "pp_probpose_loss_terms": (C.c_int, [_vp] * 10 + [_d, _i, _i, _i] + [_vp] * 6),
    "pp_oks_heatmap_loss_backward": (C.c_int, [_vp, _vp, _vp, _i, _vp, C.c_longlong, C.c_longlong, _i, _i]
                                     + [_f] * 4 + [_i, _vp] + [C.c_longlong] * 4 + [_i] * 4 + [_vp, _vp]),
    "pp_probpose_loss_grads": (C.c_int, [_vp] * 13 + [_i, _i] + [_vp] * 5),
    "pp_wgrad_workspace_floats": (C.c_longlong, [_i, _i, _i, _i]),
    "pp_wgrad_gemm": (C.c_int, [C.POINTER(WgradArgs), _vp]),
    "pp_bn_workspace_bytes": (C.c_longlong, [_i, _i]),
    "pp_bn_train_stats": (C.c_int, [_vp, C.c_longlong, _i, _i, _vp, _vp, _f, _f] + [_vp] * 8),
    "pp_bn_apply_relu": (C.c_int, [_vp, C.c_longlong, _i, _i, _vp, _vp, _vp, C.c_longlong, _i, _i, _vp]),
    "pp_bn_pool_relu": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "pp_bn_train_backward": (C.c_int, [_vp, C.c_longlong, _vp, C.c_longlong, _i, _i] + [_vp] * 5
                             + [_i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.c_longlong, _i, _vp, _vp]),
    "pp_aux_tail_backward": (C.c_int, [_vp] * 4 + [_i, _i, _i] + [_vp] * 3 + [_i, _vp]),
    "pp_heat_clamp": (C.c_int, [_vp, _vp, C.c_longlong, _f, _vp]),
    "pp_heat_tail_backward": (C.c_int, [_vp, _vp, _i, _i, _i, _f, _i, _f, _vp, _i, _i, _vp]),
    "pp_layernorm_backward_workspace_bytes": (C.c_longlong, [_i, _i]),
    "pp_layernorm_backward": (C.c_int, [_vp, _vp, _f, _i, _i, _vp, C.c_longlong, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "pp_gelu_forward": (C.c_int, [_vp, C.c_longlong, _vp, _i, _vp]),
    "pp_gelu_backward": (C.c_int, [_vp, _vp, C.c_longlong, _vp, _i, _vp]),
    "pp_attention_backward_workspace_bytes": (C.c_longlong, [_i, _i, _i]),
    "pp_attention_backward": (C.c_int, [_vp] * 4 + [_i] * 5 + [_vp, _vp]),
    "pp_rows_period_sum": (C.c_int, [_vp, _i, _i, _i, _vp, _vp]),
    "pp_crop_rows_gather": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _vp]),
    "pp_droppath_add": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "pp_crop_rows_scatter_add": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "pp_optim_table_bytes": (C.c_longlong, [_i, _vp, _i]),
    "pp_optim_table_build": (C.c_int, [_i] + [_vp] * 7 + [_i] + [_vp] * 3 + [_i, C.POINTER(C.c_int),
                                                                             C.POINTER(C.c_longlong)]),
    "pp_grad_sqnorm_partials": (C.c_int, [_vp, _i, _vp, _vp]),
    "pp_grad_norm_finish": (C.c_int, [_vp, _i, _i, _d, _i, _vp, _vp]),
    "pp_adamw_step": (C.c_int, [_vp, _i, _vp, _i, _vp]),
    "pp_ema_table_bytes": (C.c_longlong, [_i, _vp]),
    "pp_ema_table_build": (C.c_int, [_i] + [_vp] * 5 + [C.POINTER(C.c_int)]),
    "pp_ema_update": (C.c_int, [_vp, _i, _d, _vp]),
    "pp_cocoeval_oks": (C.c_int, [_i, _i] + [C.c_longlong] * 3 + [_vp] * 10),
    "pp_cocoeval_exoks": (C.c_int, [_i, _i] + [C.c_longlong] * 3 + [_vp] * 10 + [_d, _vp, _vp]),
    "pp_cocoeval_match": (C.c_int, [_i, _i, _i] + [C.c_longlong] * 3 + [_vp] * 13),
    "pp_cocoeval_accumulate": (C.c_int, [C.c_longlong, _i, _i, _i] + [_vp] * 10),
    "pp_posenms_rescore": (C.c_int, [C.c_longlong, _i, _vp, _vp, _d, _vp, _vp]),
    "pp_posenms": (C.c_int, [_i, _i, C.c_longlong] + [_vp] * 7 + [_i, _d, _d, _i] + [_vp] * 4),
    "pp_track_state_bytes": (C.c_longlong, [_i, _i]),
    "pp_track_oks": (C.c_int, [_i, _i, _i, C.c_longlong] + [_vp] * 7 + [_d, _vp, _vp]),
    "pp_track_assign": (C.c_int, [_i, _i, _i, C.c_longlong] + [_vp] * 5 + [_d, _i, _d, _d] + [_vp] * 6),
    "pp_track_assign_optimal": (C.c_int, [_i, _i, _i, C.c_longlong] + [_vp] * 5 + [_d, _i, _d, _d] + [_vp] * 7),
    "pp_track_oks_predicted": (C.c_int, [_i, _i, _i, C.c_longlong] + [_vp] * 7 + [_d, _d, _d, _vp, _vp]),
    "pp_track_assign_staged": (C.c_int, [_i, _i, _i, C.c_longlong] + [_vp] * 6 + [_d, _d, _d, _i, _d, _i, _i, _d, _d]
                               + [_vp] * 7),
    "pp_track_filter": (C.c_int, [_i, _i, C.c_longlong] + [_vp] * 4 + [_d] + [_vp] * 3 + [_i, _d, _d, _d, _vp, _vp]),
    "pp_track_boxes": (C.c_int, [_i, _i, _i, _vp, _d, _i, _d, _i, _i, _d, _i, _i, _d, _d, _d] + [_vp] * 4 + [_d]
                       + [_vp] * 5),
    "pp_trackeval_clear": (C.c_int, [_i] * 3 + [C.c_longlong] * 4 + [_vp] * 16),
    "pp_trackeval_overlap": (C.c_int, [_i] * 3 + [C.c_longlong] * 4 + [_vp] * 11),
    "pp_trackeval_identity": (C.c_int, [_i, _i, C.c_longlong] + [_vp] * 5),
    "pp_trackeval_hota_align": (C.c_int, [_i, _i] + [C.c_longlong] * 4 + [_vp] * 9),
    "pp_trackeval_hota_weights": (C.c_int, [_i, _i] + [C.c_longlong] * 6 + [_vp] * 12),
    "pp_trackeval_hota_match": (C.c_int, [_i] * 3 + [C.c_longlong] * 4 + [_vp] * 15),
    "pp_trackeval_hota_assoc": (C.c_int, [_i] * 3 + [C.c_longlong] * 3 + [_vp] * 10),
    "pp_viz_render": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _vp, _i, _i, _i] + [_vp] * 5 + [_i, _i, _vp, _i, _d, _i, _i,
                                                                                          _vp]),
    "pp_viz_colorize": (C.c_int, [_vp, _vp, C.c_longlong, _i, _i, _vp, _i, _vp]),
    "pp_valmeter_state_words": (C.c_longlong, [_i, _i]),
    "pp_valmeter_update": (C.c_int, [_vp] * 10 + [_i] + [_vp] * 3 + [_i, _i, _vp, _vp]),
    "pp_valmeter_report": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pp_calib_fit": (C.c_int, [_vp, _i, _i, C.c_longlong, _vp, _vp, _vp, _vp]),
    "pp_calib_apply": (C.c_int, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "pp_calib_score": (C.c_int, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
}
PP_VALMETER_BINS, PP_VALMETER_MAX_THRESHOLDS = 1024, 64
PP_VIZ_MAX_SIDE = 8192
PP_AUGMENT_POST_TILE_W, PP_AUGMENT_POST_TILE_H, PP_AUGMENT_POST_WORDS = 64, 16, 24
PP_EMA_LERP_F32, PP_EMA_COPY_WORDS = 0, 1
PP_COCO_GT_CROWD, PP_COCO_GT_NO_VISIBLE = 1, 2
PP_POSENMS_HARD, PP_POSENMS_SOFT_GAUSSIAN, PP_POSENMS_SOFT_LINEAR = 0, 1, 2
PP_POSENMS_MAX_DETS = 4096
PP_TRACK_MAX_TRACKS, PP_TRACK_MAX_DETS = 4096, 4096
PP_TRACK_OPT_MAX = 256
(PP_TRACK_BOX_FREE, PP_TRACK_BOX_PROPOSED, PP_TRACK_BOX_OLD, PP_TRACK_BOX_FEW, PP_TRACK_BOX_OUTSIDE,
 PP_TRACK_BOX_SUPPRESSED) = range(6)
PP_TRACKEVAL_MAX_FRAME, PP_TRACKEVAL_MAX_IDS = 256, 1024
PP_TRACKEVAL_HOTA_MAX_ALPHAS, PP_TRACKEVAL_HOTA_MAX_FRAMES = 32, 1 << 20
EXPORTS = tuple(_SIGNATURES)


def lib():
    """Load the extension once; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise HipExtensionError(
                    f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
            h = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(h, name)  # AttributeError => header/library mismatch
                fn.restype, fn.argtypes = res, args
            _lib = h
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().pp_last_error().decode("utf-8", "replace")
        raise HipExtensionError(f"{what or 'libprobpose_hip'} failed ({rc}): {msg}")


# the int-returning entries whose value is an answer, not a status
_INT_VALUES = ("pp_version", "pp_device_ok")


def call(name: str, *args):
    """``name(*args)`` in the library: tensors and numpy arrays go as their addresses, None as a null pointer, the rest
    as given (ctypes checks it against ``_SIGNATURES``).  Raises for a non-zero status and for a negative size;
    otherwise returns the value."""
    r = getattr(lib(), name)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else
                               C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in args])
    if name.endswith(("_bytes", "_floats")):
        if r < 0:
            check(r, name)
    elif _SIGNATURES[name][0] is C.c_int and name not in _INT_VALUES:
        check(r, name)
    return r


def launch(name: str, *args):
    """``call`` for the entries that enqueue work: torch's current stream is the last argument."""
    return call(name, *args, stream_ptr())


def require_device(t=None) -> None:
    """The product path is HIP-only: refuse CPU tensors / missing GPU."""
    if not torch.cuda.is_available():
        raise HipExtensionError("no HIP device visible: the ProbPose hot path has no CPU fallback")
    if t is not None and not t.is_cuda:
        raise HipExtensionError("expected a tensor on the GPU (cuda/HIP device)")


def ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
