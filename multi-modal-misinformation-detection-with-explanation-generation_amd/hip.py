"""ctypes binding of libmmf_hip.so (include/mmf_hip.h).

The product path has no CPU fallback: if the library is missing or fails to load, `load()`
raises.  Build it with `make -C <pkg>/csrc` (or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libmmf_hip.so")

# exported symbols and their C signatures (kept in sync with include/mmf_hip.h)
_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_D = ctypes.c_double
SIGNATURES = {
    "mmf_create": (_I, [_I, ctypes.POINTER(_P)]),
    "mmf_destroy": (None, [_P]),
    "mmf_last_error": (ctypes.c_char_p, []),
    "mmf_version": (ctypes.c_char_p, []),
    "mmf_load_tensor": (_I, [_P, ctypes.c_char_p, _I, _I, ctypes.POINTER(ctypes.c_int64), _P]),
    "mmf_finalize": (_I, [_P, _I]),
    "mmf_ready": (_I, [_P]),
    "mmf_reserve": (_I, [_P, _I, _I, _I]),
    "mmf_text_forward": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "mmf_text_pooled": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "mmf_head_train_ws_bytes": (ctypes.c_int64, [_I]),
    "mmf_head_train_epoch": (_I, [_P, _P, _I, _P, _P, _F, _I, _P, _D, _D, _D, _D, _D, _I, _P, _P, _P, _P, _P, _P, _P,
                                  _P, ctypes.c_int64, _P]),
    "mmf_head_eval": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "mmf_effnet_forward": (_I, [_P, _P, _I, _P, _P, _P]),
    "mmf_effnet_forward_f32": (_I, [_P, _P, _I, _P, _P, _P]),
    "mmf_effnet_pooled": (_I, [_P, _P, _I, _P, _P]),
    "mmf_hflip_u8": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "mmf_color_jitter_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "mmf_gaussian_blur_u8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "mmf_jpeg_roundtrip_ws_bytes": (ctypes.c_int64, [_I, _I]),
    "mmf_jpeg_roundtrip_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "mmf_effcls_train_epoch": (_I, [_P, _P, _I, _P, _I, _P, _F, _I, _D, _D, _D, _D, _D, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mmf_effcls_eval": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "mmf_effnet_trunk": (_I, [_P, _P, _I, _P, _P]),
    "mmf_effhead_ws_bytes": (ctypes.c_int64, [_I]),
    "mmf_effhead_train_epoch": (_I, [_P, _P, _I, _P, _I, _P, _F, _I, _P, _P, _D, _D, _D, _D, _D, _D, _I, _P, _P, _P, _P,
                                     _P, _P, _P, ctypes.c_int64, _P]),
    "mmf_effhead_eval": (_I, [_P, _P, _I, _I, _P, _P, _P, _D, _P, _P, _P, ctypes.c_int64, _P]),
    "mmf_clip_image": (_I, [_P, _P, _I, _P, _P]),
    "mmf_clip_text": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "mmf_clip_consistency": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "mmf_clip_pooled": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "mmf_set_clip_projections": (_I, [_P, _P, _P, _P]),
    "mmf_clip_train_ws_bytes": (ctypes.c_int64, [_I]),
    "mmf_clip_train_epoch": (_I, [_P, _P, _I, _P, _I, _D, _D, _D, _D, _D, _D, _I, _P, _P, _P, _P, _P, _P, _P,
                                  ctypes.c_int64, _P]),
    "mmf_clip_contrastive_eval": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "mmf_clip_train_trials_ws_bytes": (ctypes.c_int64, [_I, _I]),
    "mmf_clip_train_epoch_trials": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _P, _P, _P, _P, _P, _I,
                                         _P, ctypes.c_int64, _P]),
    "mmf_clip_contrastive_eval_trials": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, ctypes.c_int64, _P]),
    "mmf_resize_pil": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "mmf_resize_supported": (_I, [_I, _I]),
    "mmf_jpeg_header": (_I, [_P, ctypes.c_int64, _P]),
    "mmf_jpeg_entropy": (_I, [_P, ctypes.c_int64, _P, _P]),
    "mmf_jpeg_packed_bound": (ctypes.c_int64, [ctypes.c_int32]),
    "mmf_jpeg_entropy_packed": (_I, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P]),
    "mmf_jpeg_stage_packed": (_I, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P]),
    "mmf_jpeg_header_batch": (_I, [_P, _P, _I, _P, _P, _I]),
    "mmf_jpeg_stage_packed_batch": (_I, [_P, _P, _I, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _I, _P]),
    "mmf_jpeg_reconstruct": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "mmf_set_vault": (_I, [_P, _P, _I, _I]),
    "mmf_set_vault_normalized": (_I, [_P, _P, _I, _I]),
    "mmf_set_vault_titles": (_I, [_P, _P, _P, _I, _I, _P]),
    "mmf_vault_topk": (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P]),
    "mmf_vault_search_ws_bytes": (ctypes.c_int64, [_I, _I, _I]),
    "mmf_vault_search_rows": (_I, [_P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _I, _P, _P, _P, _P, ctypes.c_int64, _I, _P]),
    "mmf_fusion": (_I, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "mmf_fusion_train_epoch": (_I, [_P, _P, _I, _P, _P, _F, _I, _D, _D, _D, _D, _D, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mmf_analyze_batch": (_I, [_P, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mmf_mixed_plan": (_I, [_P, _I, _P, _P]),
    "mmf_analyze_mixed": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                               _P]),
    "mmf_profile_begin": (_I, [_P]),
    "mmf_profile_end": (_I, [_P, _I, _P, _P, _P, _P]),
    "mmf_profile_kind_name": (ctypes.c_char_p, [_I]),
    "mmf_set_option": (_I, [_P, ctypes.c_char_p, _I]),
    "mmf_get_option": (_I, [_P, ctypes.c_char_p, ctypes.POINTER(_I)]),
    "mmf_option_name": (ctypes.c_char_p, [_I]),
    "mmf_device_bytes": (ctypes.c_int64, [_P]),
    "mmf_gemm_f16": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "mmf_gemm_f16_ex": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "mmf_gemm_f16_split": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mmf_attention_f16": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "mmf_dwconv_nchunks": (_I, [_I, _I, _I, _I]),
    "mmf_dwconv_f16": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mmf_expand_dw_f16": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mmf_se_f32": (_I, [_P, _I, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mmf_effnet_stem_f16": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "mmf_effnet_stem_dw_f16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mmf_gap_classifier_f16": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    # fp32 EfficientNet tower kernels on raw operands (csrc/effnet_host.cpp)
    "mmf_pw32_variant": (_I, [_I, _I, _I, _I, _P]),
    "mmf_pw32_f32": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "mmf_dw32_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mmf_sum32_f32": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "mmf_gap32_f32": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "mmf_effnet_stem32_f32": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    # transformer-tower kernels on raw operands (csrc/test_host.cpp)
    "mmf_layernorm_f32": (_I, [_P, _I, _P, _I, _P, _P, _F, _P, _I, _P, _I, _I, _I, _P]),
    "mmf_add_ln_f32": (_I, [_P, _I, _P, _I, _P, _P, _F, _P, _P, _P, _I, _I, _I, _P]),
    "mmf_add_ln_f16": (_I, [_P, _I, _P, _I, _P, _P, _F, _P, _P, _I, _I, _I, _P]),
    "mmf_add_ln_hilo_f16": (_I, [_P, _P, _I, _P, _I, _P, _P, _F, _I, _I, _P, _I, _P]),
    "mmf_hilo_rows_f32": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "mmf_layernorm_split3_f32": (_I, [_P, _P, _P, _P, _F, _P, _I, _I, _I, _P]),
    "mmf_roberta_embed_f32": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mmf_clip_text_embed_f32": (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _P]),
    "mmf_clip_vision_assemble_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _P]),
    "mmf_clip_im2col_f16": (_I, [_P, _P, _I, _P]),
    "mmf_eos_index_i32": (_I, [_P, _P, _I, _I, _I, _P]),
    "mmf_gather_ln_f32": (_I, [_P, _P, _I, _P, _P, _F, _P, _P, _I, _I, _P]),
    "mmf_gather_rows2": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _I, _P]),
    "mmf_l2norm_f32": (_I, [_P, _I, _I, _P]),
    "mmf_split3_f32": (_I, [_P, _I, _P, _I, _I, _I, _P]),
    "mmf_attention32_f32": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "mmf_attention_q1_f16": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mmf_gemm_splitk_factor": (_I, [_I, _I, _I, _I]),
    "mmf_gemm_f16_splitk": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, ctypes.c_int64, _P]),
    "mmf_gemm_ln_tn": (_I, [_I, _I, _I]),
    "mmf_gemm_f16_raw": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, ctypes.POINTER(_I), _P]),
    "mmf_gemm_f16_ln_producer": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "mmf_gemm_f16_ln_consumer": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _P, _F, _P, _I, _I, _I, _I, _I, _P]),
    "mmf_gemm_f16_attn": (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mmf_gemm_f16_ln_attn": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _P, _F, _P, _I, _I, _P, _I, _I, _I, _I, _P]),
    # the closing fp32 kernels and the vault's stages on raw operands (csrc/test_host.cpp)
    "mmf_text_heads_f32": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P]),
    "mmf_text_cls_rows_f32": (_I, [_P, _I, _P, _P, _I, _P]),
    "mmf_fusion_raw_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mmf_rowdot_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "mmf_mixed_finish_raw": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P,
                                  _P, _P, _P, _P, _P, _P, _P, _P]),
    "mmf_vault_sims_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "mmf_vault_topk_f32": (_I, [_P, _I, _I, _I, _F, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P]),
    "mmf_vault_sort_cand_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "mmf_jpeg_block_roundtrip_raw": (_I, [_P, _P, _I, _P, _P, _P, _P]),
    # mmf_resize_pil's plan and coefficient kernel for one image (csrc/resize_host.cpp)
    "mmf_resize_plan": (_I, [_I, _I, _I, _P]),
    "mmf_resize_coef_raw": (_I, [_I, _I, _I, _P, _P, _P]),
}

JITTER_CHUNKS = 256  # MMF_JITTER_CHUNKS: mmf_color_jitter_u8's ws is uint64 [B][JITTER_CHUNKS]

_lib = None


class MMFError(RuntimeError):
    pass


def load(path: str | None = None):
    """Load libmmf_hip.so and declare the ABI.  Raises MMFError (never falls back)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MMF_HIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise MMFError(f"libmmf_hip.so not found at {p}; build it with `make -C {PKG_DIR}/csrc`")
    # torch before the library, for every caller: its wheel preloads its own bundled HIP runtime by path; loaded
    # after libmmf_hip.so has pulled in the system one, the process holds two runtimes and the second to initialise
    # finds no device (mmf_create fails).  A process without torch has no second runtime to meet.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:
        raise MMFError(f"failed to load {p}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mmf_last_error().decode(errors="replace")
        raise MMFError(f"{what or 'mmf call'} failed ({rc}): {msg}")


def set_process_option(name: str, value: int) -> None:
    """Process-wide default of a library option (mmf_set_option with a NULL handle): used by the
    handle-less ops and by handles created afterwards."""
    check(load().mmf_set_option(None, name.encode(), int(value)), f"mmf_set_option({name})")


def get_process_option(name: str) -> int:
    v = ctypes.c_int()
    check(load().mmf_get_option(None, name.encode(), ctypes.byref(v)), f"mmf_get_option({name})")
    return v.value


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None passes NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream
