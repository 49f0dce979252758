"""ctypes binding of libmcd_hip.so (include/mcd_hip.h).  No fallback: a missing library is an error."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCD_LIB_PATH") or os.path.join(_HERE, "csrc", "libmcd_hip.so")   # MCD_LIB_PATH: dev builds of the same ABI

_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float
_p = ctypes.c_void_p
_sz = ctypes.c_size_t

# name -> (restype, argtypes): exactly the symbols include/mcd_hip.h declares
SIGNATURES = {
    "mcd_last_error": (ctypes.c_char_p, []),
    "mcd_abi_version": (_int, []),
    "mcd_normalize_rows": (_int, [_p, _i64, _i64, _i64, _p, _i64, _p]),
    "mcd_center_cube_normalize_rows": (_int, [_p, _i64, _i64, _i64, _f, _p, _i64, _p]),
    "mcd_prepare_rows_gathered": (_int, [_p, _i64, _i64, _int, ctypes.POINTER(_i64), _i64, _i64, _i64, _int, _f, _p, _i64,
                                         _p]),
    "mcd_embed_gemm_workspace": (_sz, [_i64, _i64, _i64, _int]),
    "mcd_embed_gemm": (_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _int, _p, _i64, _p, _sz, _p]),
    "mcd_embed_gemm_exp_workspace": (_sz, [_i64, _i64, _i64]),
    "mcd_embed_gemm_exp": (_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _f, _int, _p, _i64, _p, _p, _sz, _p]),
    "mcd_embed_gemm_exp_time_kernel": (_int, [_int]),
    "mcd_embed_gemm_exp_kernel_ms": (_f, []),
    "mcd_wpmi_score_bf16_workspace": (_sz, [_i64, _int]),
    "mcd_wpmi_score_bf16": (_int, [_p, _i64, _i64, _i64, _p, _p, _i64, _i64, _int, _p, _f, _int, _p, _i64, _p, _sz, _p]),
    "mcd_row_softmax": (_int, [_p, _i64, _i64, _i64, _f, _p, _i64, _p]),
    "mcd_col_topk_workspace": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "mcd_col_topk": (_int, [_p, _i64, _i64, _i64, _i64, _int, _p, _p, _i64, _p, _sz, _p]),
    "mcd_transpose": (_int, [_p, _i64, _i64, _i64, _p, _i64, _p]),
    "mcd_wpmi_score": (_int, [_p, _i64, _i64, _i64, _p, _i64, _i64, _int, _p, _f, _int, _int, _p, _i64, _p]),
    "mcd_logsumexp_sub_workspace": (_sz, [_i64, _i64, _int]),
    "mcd_logsumexp_sub": (_int, [_p, _i64, _i64, ctypes.POINTER(_i64), _int, _f, _int, _p, _i64, _p, _sz, _p]),
    "mcd_row_topk": (_int, [_p, _i64, _i64, _i64, _int, _p, _p, _p]),
    "mcd_hook_pool": (_int, [_p, _i64, _i64, _i64, _int, _p, _i64, _i64, _i64, _i64, _p]),
    "mcd_rank_reorder": (_int, [_p, _i64, _i64, _i64, _p, _p, _i64, _i64, _int, _p, _int, _f, _f, _p, _p, _i64, _p]),
    "mcd_vit_attention": (_int, [_p, _i64, _i64, _i64, _p, _p]),
    "mcd_vit_attention_long": (_int, [_p, _i64, _i64, _i64, _p, _p]),
    "mcd_vit_attention_cls": (_int, [_p, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    "mcd_layer_norm": (_int, [_p, _i64, _i64, _p, _p, _f, _p, _p]),
    "mcd_patchify": (_int, [_p, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    "mcd_conv_stem_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _i64, _p, _p]),
    "mcd_dwconv_bn_silu": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _int, _int, _int, _p, _p, _i64, _p]),
    "mcd_se_gate": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _i64, _p, _p, _p, _p]),
    "mcd_channel_scale": (_int, [_p, _i64, _i64, _i64, _p, _p]),
    "mcd_hook_pool_nhwc": (_int, [_p, _i64, _i64, _i64, _int, _p, _i64, _i64, _i64, _i64, _p]),
    "mcd_conv7x7s2_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _i64, _p, _p]),
    "mcd_bn_relu_maxpool_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    "mcd_conv_igemm_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _i64, _int, _int, _int, _int, _p, _p]),
    "mcd_conv_igemm_res_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _p, _i64, _int, _int, _int, _int, _p, _p]),
    "mcd_conv3x3s2_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _i64, _int, _p, _p]),
    "mcd_avgpool2_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p]),
    "mcd_attnpool_tokens": (_int, [_p, _i64, _i64, _i64, _p, _p, _p]),
    "mcd_image_preprocess": (_int, [_p, _i64, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _i64,
                                    _p]),
    "mcd_image_minmax_workspace": (_sz, [_i64, _i64, _i64, _i64]),
    "mcd_image_minmax_normalize": (_int, [_p, _i64, _i64, _i64, _i64, _int, _f, _f, _p, _i64, _p, _sz, _p]),
}
# the text-tower entries of the same library, declared in include/mcd_text.h (additive to ABI version 9)
TEXT_SIGNATURES = {
    "mcd_vit_attention_keylen": (_int, [_p, _i64, _i64, _i64, _p, _p, _p]),
    "mcd_text_embed_ln": (_int, [_p, _p, _p, _p, _p, _p, _p, _f, _i64, _i64, _i64, _i64, _i64, _p, _p]),
}
# the OpenAI-CLIP entries of the same library, declared in include/mcd_clip.h (additive to ABI version 9)
CLIP_SIGNATURES = {
    "mcd_vit_attention_causal": (_int, [_p, _i64, _i64, _i64, _p, _p]),
    "mcd_quick_gelu": (_int, [_p, _i64, _p, _p]),
}
# the token-reduction entry of the same library, declared in include/mcd_tokens.h (additive to ABI version 9)
TOKEN_SIGNATURES = {
    "mcd_token_mean": (_int, [_p, _int, _int, _int, _i64, _i64, _int, _p, _i64, _p]),
}
# the sentence-encoder entries of the same library, declared in include/mcd_sentence.h (additive to ABI version 9)
SENTENCE_SIGNATURES = {
    "mcd_vit_attention_relbias": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p]),
    "mcd_masked_mean_l2": (_int, [_p, _int, _int, _int, _p, _int, _p, _p]),
}
# the masked-autoencoder entries of the same library, declared in include/mcd_mask.h (additive to ABI version 9)
MASK_SIGNATURES = {
    "mcd_patchify_kept": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    "mcd_token_restore": (_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _p]),
}
# the activation-cache streaming entries of the same library, declared in include/mcd_cache.h (additive to ABI version 9)
_pp = ctypes.POINTER(_p)
CACHE_SIGNATURES = {
    "mcd_hook_pool_rows": (_int, [_p, _i64, _i64, _i64, _int, _p, _i64, _i64, _i64, _i64, _p, _i64, _p]),
    "mcd_cache_stream_open": (_int, [_int, _pp, ctypes.POINTER(_i64), _p, _int, _sz, _pp]),
    "mcd_cache_stream_reserve": (_int, [_p, _int, _p]),
    "mcd_cache_stream_push": (_int, [_p, _int, _p, _i64, _i64, _p]),
    "mcd_cache_stream_close": (_int, [_p]),
    "mcd_cache_stream_abort": (_int, [_p]),
}
# the class-token fold entries of the same library, declared in include/mcd_clsfold.h (additive to ABI version 9)
CLSFOLD_SIGNATURES = {
    "mcd_cls_token_mix": (_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p]),
    "mcd_cls_token_mix_max_t": (_i64, [_i64, _i64]),
}
# the Swin entries of the same library, declared in include/mcd_swin.h (additive to ABI version 9)
SWIN_SIGNATURES = {
    "mcd_window_attention": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p]),
    "mcd_patch_merge_ln": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _f, _p, _p]),
}
# the 7x7 / 2 stem with its epilogue, of the same library, declared in include/mcd_stem.h (additive to ABI version 9)
STEM_SIGNATURES = {
    "mcd_conv7x7s2_bias_relu_nhwc": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _i64, _int, _p, _p]),
}

MCD_E_ARG = -1
MCD_E_RANGE = -2
MCD_E_WORKSPACE = -3
MCD_E_UNSUPPORTED = -5

_lib = None


class McdError(RuntimeError):
    """An MCD_E_* status from libmcd_hip.so, with mcd_last_error() as the message."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def load():
    """Load libmcd_hip.so once.  Raises ImportError (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "mammo-clip-dissect_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C mammo-clip-dissect_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(TEXT_SIGNATURES.items()) + list(CLIP_SIGNATURES.items())
                                  + list(TOKEN_SIGNATURES.items()) + list(SENTENCE_SIGNATURES.items())
                                  + list(MASK_SIGNATURES.items()) + list(CACHE_SIGNATURES.items())
                                  + list(CLSFOLD_SIGNATURES.items()) + list(SWIN_SIGNATURES.items())
                                  + list(STEM_SIGNATURES.items())):
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        msg = load().mcd_last_error().decode("utf-8", "replace")
        raise McdError(rc, msg)


# ---- libmcd_blaslt.so: the optional hipBLASLt companion (include/mcd_blaslt.h) ------------------------------
BLASLT_PATH = os.path.join(os.path.dirname(LIB_PATH), "libmcd_blaslt.so")
BLASLT_SIGNATURES = {
    "mcd_blaslt_last_error": (ctypes.c_char_p, []),
    "mcd_linear_residual_workspace": (_sz, []),
    "mcd_linear_residual": (_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _sz, _p]),
    "mcd_linear_residual_relu": (_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _sz, _p]),
    "mcd_linear_residual_plan_info": (_int, [_i64, _i64, _i64, ctypes.POINTER(_f), ctypes.POINTER(_int)]),
    "mcd_linear_residual_get_picks": (_int, [ctypes.POINTER(_i64), _int]),
    "mcd_linear_residual_set_pick": (_int, [_i64, _i64, _i64, _int, _int]),
}
_blaslt = None


def load_blaslt():
    """libmcd_blaslt.so, or None when it has not been built / hipBLASLt cannot be loaded.  It only serves an encoder-side
    fusion (core.linear_residual); callers keep PyTorch's own linear + add without it."""
    global _blaslt
    if _blaslt is None:
        try:
            L = ctypes.CDLL(BLASLT_PATH)
            for name, (res, args) in BLASLT_SIGNATURES.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _blaslt = L
        except (OSError, AttributeError):
            _blaslt = False
    return _blaslt or None


# ---- libmcd_host.so: the container half of include/mcd_cache.h (plain C, no GPU) ---------------------------------
HOST_PATH = os.path.join(_HERE, "csrc", "libmcd_host.so")
CACHE_HOST_SIGNATURES = {
    "mcd_zip_crc32": (ctypes.c_uint32, [ctypes.c_uint32, _p, _sz]),
    "mcd_cachefile_open": (_int, [ctypes.c_char_p, ctypes.c_char_p, _i64, _i64, _i64, _i64, _i64, _pp]),
    "mcd_cachefile_append": (_int, [_p, _p, _i64, _i64]),
    "mcd_cachefile_close": (_int, [_p]),
    "mcd_cachefile_abort": (None, [_p]),
    "mcd_cachefile_last_error": (ctypes.c_char_p, []),
}
_cache_host = None


class CacheIO(ctypes.Structure):
    """mcd_cache_io_t: the container's entry points as mcd_cache_stream_open takes them."""
    _fields_ = [("append", _p), ("close", _p), ("abort", _p), ("last_error", _p)]


def load_cache_host():
    """libmcd_host.so with the container entries, or None when it has not been built (the cache files are then written by the
    Python writer thread, concept_vit/utils.py)."""
    global _cache_host
    if _cache_host is None:
        try:
            L = ctypes.CDLL(HOST_PATH)
            for name, (res, args) in CACHE_HOST_SIGNATURES.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _cache_host = L
        except (OSError, AttributeError):
            _cache_host = False
    return _cache_host or None


def cache_io(H):
    """The mcd_cache_io_t of the container in libmcd_host.so (H = load_cache_host())."""
    return CacheIO(*[ctypes.cast(getattr(H, "mcd_cachefile_" + n), _p) for n in ("append", "close", "abort", "last_error")])
