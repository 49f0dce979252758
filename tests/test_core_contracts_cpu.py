"""The host side of the encoder-side wrappers of core.py (K9 .. K32, the token ops), pinned without a GPU: which
inputs are refused, with which exception and text, and what an accepted call hands the library -- the entry, every
scalar, every stride, and which operand's address (as an offset from its base) sits in which position.  Plus the
argument checks of the K9 family's four C entries, status and mcd_last_error() text.

The operands are host tensors that say they are on the GPU (util.FakeCuda) and the wrappers are called below
_on_device (`__wrapped__`), which would refuse a host device before the wrapper's own checks run."""
import pytest
import torch

import util

STREAM = 0x5EED            # what core._stream() is replaced by
EPS = 1e-5


def f32(*shape, dtype=torch.float32, device=None):
    return torch.zeros(*shape, dtype=dtype, device=device).as_subclass(util.FakeCuda)


def i32(*shape, device=None):
    return f32(*shape, dtype=torch.int32, device=device)


def i64(*shape):
    return f32(*shape, dtype=torch.int64)


def gapped(*shape, dtype=torch.float32):
    """A tensor of `shape` whose inner stride is 2: neither contiguous nor unit-stride."""
    return f32(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]


def host(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


# ---- refusals -------------------------------------------------------------------------------------------------------------
NEED_GPU = "mammo-clip-dissect_amd runs on the GPU only: expected a CUDA/HIP tensor, got cpu"
QKV = "qkv must be a contiguous float32 [B, T, 3*heads*64] tensor"
QKV_WIDTH = "qkv last dimension 192 is not 3 * 2 heads * 64"
OUT_BTW = "out must be a contiguous float32 [B, T, heads*64] tensor"
LENS_QKV = "lens must be a contiguous int32 [B] tensor on qkv's device (or None)"
LENS_X = "lens must be a contiguous int32 [B] tensor on x's device (or None)"
REL = "rel must be a contiguous float32 [heads, 2T-1] tensor on qkv's device (or None)"
CLS_KV = "vit_attention_cls: float32 k and v of one shape [B, T, heads, 64]"
CLS_ADJ = "vit_attention_cls: the heads*64 floats of a token must be adjacent in q, k and v"
MIX_ADJ = "cls_token_mix: the D floats of a row, and the heads of an image in u, must be adjacent"
MIX_OUT = "out must be a float32 [B, heads, D] tensor with an image's heads*D floats adjacent"
WIN_QKV = "qkv must be a contiguous float32 [B, H*W, 3*heads*32] tensor"
WIN_TABLE = "table must be a contiguous float32 [(2*window-1)^2, heads] tensor"
WIN_PAD = "pad_qkv must be a contiguous float32 tensor of 3*heads*32 elements (or None)"
PM_WB = "patch_merge_ln: contiguous float32 [4C] weight / bias"
LN = "layer_norm: contiguous float32 x and [D] weight / bias"
TE_IDS = "text_embed_ln: ids (and type_ids) must be int64 [B, T]"
TE_TABLES = "text_embed_ln: contiguous float32 [rows, D] tables"
TE_WIDTH = "text_embed_ln: the tables, weight and bias must share the width D=8"
SRC = "src must be a contiguous float32 [B, 1 + Lk, D] or [1 + Lk, D] tensor"


def te(ids=None, type_ids=None, word=None, pos=None, table=None, weight=None, bias=None, **kw):
    """text_embed_ln's arguments: B = 2, T = 3, D = 8, a vocabulary of 7, 4 positions, 2 types; one of them replaced."""
    pick = lambda t, default: default() if t is None else t
    return (pick(ids, lambda: i64(2, 3)), type_ids, pick(word, lambda: f32(7, 8)), pick(pos, lambda: f32(4, 8)),
            pick(table, lambda: f32(2, 8)), pick(weight, lambda: f32(8)), pick(bias, lambda: f32(8)), EPS), kw


def tr(src=None, restore=None, fill=None, add=None, out=None):
    """token_restore's arguments: B = 2, Lk = 2, L = 4, D = 8; one of them replaced."""
    return (f32(2, 3, 8) if src is None else src, i32(2, 4) if restore is None else restore), dict(fill=fill, add=add, out=out)


# (id, wrapper, () -> (args, kwargs), exception, text): every input has ONE fault
REFUSALS = [
    # K9, K9L, K9A: _attention
    ("k9-host", "vit_attention", lambda: ((host(1, 2, 192), 1), {}), TypeError, NEED_GPU),
    ("k9-dtype", "vit_attention", lambda: ((f32(1, 2, 192, dtype=torch.float64), 1), {}), TypeError, QKV),
    ("k9-rank", "vit_attention", lambda: ((f32(2, 192), 1), {}), TypeError, QKV),
    ("k9-gapped", "vit_attention", lambda: ((gapped(1, 2, 192), 1), {}), TypeError, QKV),
    ("k9-width", "vit_attention", lambda: ((f32(1, 2, 192), 2), {}), ValueError, QKV_WIDTH),
    ("k9-out-shape", "vit_attention", lambda: ((f32(1, 2, 192), 1), dict(out=f32(1, 3, 64))), TypeError, OUT_BTW),
    ("k9-out-dtype", "vit_attention", lambda: ((f32(1, 2, 192), 1), dict(out=f32(1, 2, 64, dtype=torch.float16))),
     TypeError, OUT_BTW),
    ("k9-out-gapped", "vit_attention", lambda: ((f32(1, 2, 192), 1), dict(out=gapped(1, 2, 64))), TypeError, OUT_BTW),
    ("k9l-dtype", "vit_attention_long", lambda: ((f32(1, 2, 192, dtype=torch.float64), 1), {}), TypeError, QKV),
    ("k9l-width", "vit_attention_long", lambda: ((f32(1, 2, 192), 2), {}), ValueError, QKV_WIDTH),
    ("k9l-out", "vit_attention_long", lambda: ((f32(1, 2, 192), 1), dict(out=f32(1, 2, 128))), TypeError, OUT_BTW),
    ("k9a-gapped", "vit_attention_causal", lambda: ((gapped(1, 2, 192), 1), {}), TypeError, QKV),
    ("k9a-width", "vit_attention_causal", lambda: ((f32(1, 2, 192), 2), {}), ValueError, QKV_WIDTH),
    ("k9a-out", "vit_attention_causal", lambda: ((f32(1, 2, 192), 1), dict(out=f32(2, 64))), TypeError, OUT_BTW),
    # K9M
    ("k9m-host", "vit_attention_keylen", lambda: ((host(2, 2, 192), 1, None), {}), TypeError, NEED_GPU),
    ("k9m-lens-host", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 1, host(2, dtype=torch.int32)), {}), TypeError,
     NEED_GPU),
    ("k9m-dtype", "vit_attention_keylen", lambda: ((f32(2, 2, 192, dtype=torch.float64), 1, None), {}), TypeError, QKV),
    ("k9m-rank", "vit_attention_keylen", lambda: ((f32(2, 2, 1, 192), 1, None), {}), TypeError, QKV),
    ("k9m-gapped", "vit_attention_keylen", lambda: ((gapped(2, 2, 192), 1, None), {}), TypeError, QKV),
    ("k9m-width", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 2, None), {}), ValueError, QKV_WIDTH),
    ("k9m-lens-dtype", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 1, i64(2)), {}), TypeError, LENS_QKV),
    ("k9m-lens-shape", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 1, i32(3)), {}), TypeError, LENS_QKV),
    ("k9m-lens-gapped", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 1, gapped(2, dtype=torch.int32)), {}), TypeError,
     LENS_QKV),
    ("k9m-lens-device", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 1, i32(2, device="meta")), {}), TypeError,
     LENS_QKV),
    ("k9m-out", "vit_attention_keylen", lambda: ((f32(2, 2, 192), 1, None), dict(out=f32(2, 2, 65))), TypeError, OUT_BTW),
    # K9B
    ("k9b-rel-host", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, None, host(1, 3)), {}), TypeError, NEED_GPU),
    ("k9b-dtype", "vit_attention_relbias", lambda: ((f32(2, 2, 192, dtype=torch.bfloat16), 1, None, None), {}), TypeError,
     QKV),
    ("k9b-gapped", "vit_attention_relbias", lambda: ((gapped(2, 2, 192), 1, None, None), {}), TypeError, QKV),
    ("k9b-width", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 2, None, None), {}), ValueError, QKV_WIDTH),
    ("k9b-lens-dtype", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, i64(2), None), {}), TypeError, LENS_QKV),
    ("k9b-lens-shape", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, i32(2, 1), None), {}), TypeError, LENS_QKV),
    ("k9b-rel-dtype", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, None, f32(1, 3, dtype=torch.float64)), {}),
     TypeError, REL),
    ("k9b-rel-shape", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, None, f32(1, 4)), {}), TypeError, REL),
    ("k9b-rel-gapped", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, None, gapped(1, 3)), {}), TypeError, REL),
    ("k9b-rel-device", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, None, f32(1, 3, device="meta")), {}),
     TypeError, REL),
    ("k9b-out", "vit_attention_relbias", lambda: ((f32(2, 2, 192), 1, None, None), dict(out=gapped(2, 2, 64))), TypeError,
     OUT_BTW),
    # K27
    ("k27-host", "masked_mean_l2", lambda: ((host(2, 3, 8), None), {}), TypeError, NEED_GPU),
    ("k27-out-host", "masked_mean_l2", lambda: ((f32(2, 3, 8), None), dict(out=host(2, 8))), TypeError, NEED_GPU),
    ("k27-dtype", "masked_mean_l2", lambda: ((f32(2, 3, 8, dtype=torch.float64), None), {}), TypeError,
     "x must be a contiguous float32 [B, T, D] tensor"),
    ("k27-rank", "masked_mean_l2", lambda: ((f32(6, 8), None), {}), TypeError,
     "x must be a contiguous float32 [B, T, D] tensor"),
    ("k27-gapped", "masked_mean_l2", lambda: ((gapped(2, 3, 8), None), {}), TypeError,
     "x must be a contiguous float32 [B, T, D] tensor"),
    ("k27-lens-dtype", "masked_mean_l2", lambda: ((f32(2, 3, 8), i64(2)), {}), TypeError, LENS_X),
    ("k27-lens-shape", "masked_mean_l2", lambda: ((f32(2, 3, 8), i32(1)), {}), TypeError, LENS_X),
    ("k27-lens-device", "masked_mean_l2", lambda: ((f32(2, 3, 8), i32(2, device="meta")), {}), TypeError, LENS_X),
    ("k27-out", "masked_mean_l2", lambda: ((f32(2, 3, 8), None), dict(out=f32(2, 3, 8))), TypeError,
     "out must be a contiguous float32 [B, D] tensor"),
    # K25
    ("k25-host", "quick_gelu", lambda: ((host(2, 3),), {}), TypeError, NEED_GPU),
    ("k25-dtype", "quick_gelu", lambda: ((f32(2, 3, dtype=torch.float16),), {}), TypeError,
     "x must be a contiguous float32 tensor"),
    ("k25-gapped", "quick_gelu", lambda: ((gapped(2, 3),), {}), TypeError, "x must be a contiguous float32 tensor"),
    ("k25-out-shape", "quick_gelu", lambda: ((f32(2, 3),), dict(out=f32(3, 2))), TypeError,
     "out must be a contiguous float32 tensor of x's shape"),
    ("k25-out-gapped", "quick_gelu", lambda: ((f32(2, 3),), dict(out=gapped(2, 3))), TypeError,
     "out must be a contiguous float32 tensor of x's shape"),
    # K26
    ("k26-host", "token_mean", lambda: ((host(2, 3, 8),), {}), TypeError, NEED_GPU),
    ("k26-dtype", "token_mean", lambda: ((f32(2, 3, 8, dtype=torch.float64),), {}), TypeError,
     "x must be a float32 [B, T, D] tensor with a unit inner stride"),
    ("k26-rank", "token_mean", lambda: ((f32(1, 2, 3, 8),), {}), TypeError,
     "x must be a float32 [B, T, D] tensor with a unit inner stride"),
    ("k26-gapped", "token_mean", lambda: ((gapped(2, 3, 8),), {}), TypeError,
     "x must be a float32 [B, T, D] tensor with a unit inner stride"),
    ("k26-out-shape", "token_mean", lambda: ((f32(2, 3, 8),), dict(out=f32(2, 4))), TypeError,
     "out must be a float32 [B, D] tensor with a unit inner stride"),
    ("k26-out-gapped", "token_mean", lambda: ((f32(2, 3, 8),), dict(out=gapped(2, 8))), TypeError,
     "out must be a float32 [B, D] tensor with a unit inner stride"),
    # K9C
    ("k9c-host", "vit_attention_cls", lambda: ((f32(2, 64), f32(2, 3, 1, 64), host(2, 3, 1, 64)), {}), TypeError, NEED_GPU),
    ("k9c-dtype", "vit_attention_cls", lambda: ((f32(2, 64, dtype=torch.float64), f32(2, 3, 1, 64), f32(2, 3, 1, 64)), {}),
     TypeError, CLS_KV),
    ("k9c-k-rank", "vit_attention_cls", lambda: ((f32(2, 64), f32(2, 3, 64), f32(2, 3, 64)), {}), TypeError, CLS_KV),
    ("k9c-head-width", "vit_attention_cls", lambda: ((f32(2, 32), f32(2, 3, 1, 32), f32(2, 3, 1, 32)), {}), TypeError, CLS_KV),
    ("k9c-v-shape", "vit_attention_cls", lambda: ((f32(2, 64), f32(2, 3, 1, 64), f32(2, 4, 1, 64)), {}), TypeError, CLS_KV),
    ("k9c-q3-shape", "vit_attention_cls", lambda: ((f32(2, 1, 64), f32(2, 3, 2, 64), f32(2, 3, 2, 64)), {}), ValueError,
     "vit_attention_cls: q must be [B, heads, 64] with a row's heads adjacent"),
    ("k9c-q3-heads-apart", "vit_attention_cls",
     lambda: ((f32(2, 2, 128)[:, :, :64], f32(2, 3, 2, 64), f32(2, 3, 2, 64)), {}), ValueError,
     "vit_attention_cls: q must be [B, heads, 64] with a row's heads adjacent"),
    ("k9c-q2-shape", "vit_attention_cls", lambda: ((f32(2, 64), f32(2, 3, 2, 64), f32(2, 3, 2, 64)), {}), ValueError,
     "vit_attention_cls: q has shape (2, 64), k (2, 3, 2, 64)"),
    ("k9c-q-gapped", "vit_attention_cls", lambda: ((gapped(2, 64), f32(2, 3, 1, 64), f32(2, 3, 1, 64)), {}), ValueError,
     CLS_ADJ),
    ("k9c-k-gapped", "vit_attention_cls", lambda: ((f32(2, 64), gapped(2, 3, 1, 64), f32(2, 3, 1, 64)), {}), ValueError,
     CLS_ADJ),
    ("k9c-v-heads-apart", "vit_attention_cls",
     lambda: ((f32(2, 128), f32(2, 3, 2, 64), f32(2, 3, 2, 128)[..., :64]), {}), ValueError, CLS_ADJ),
    ("k9c-out", "vit_attention_cls", lambda: ((f32(2, 64), f32(2, 3, 1, 64), f32(2, 3, 1, 64)), dict(out=f32(2, 1, 64))),
     TypeError, "out must be a contiguous float32 [B, heads*64] tensor"),
    # K30
    ("k30-host", "cls_token_mix", lambda: ((f32(2, 1, 8), host(2, 3, 8)), {}), TypeError, NEED_GPU),
    ("k30-dtype", "cls_token_mix", lambda: ((f32(2, 1, 8), f32(2, 3, 8, dtype=torch.float64)), {}), TypeError,
     "cls_token_mix: float32 u [B, heads, D] and n [B, T, D]"),
    ("k30-rank", "cls_token_mix", lambda: ((f32(2, 8), f32(2, 3, 8)), {}), TypeError,
     "cls_token_mix: float32 u [B, heads, D] and n [B, T, D]"),
    ("k30-batch", "cls_token_mix", lambda: ((f32(2, 1, 8), f32(1, 3, 8)), {}), ValueError,
     "cls_token_mix: u has shape (2, 1, 8), n (1, 3, 8)"),
    ("k30-width", "cls_token_mix", lambda: ((f32(2, 1, 8), f32(2, 3, 4)), {}), ValueError,
     "cls_token_mix: u has shape (2, 1, 8), n (2, 3, 4)"),
    ("k30-n-gapped", "cls_token_mix", lambda: ((f32(2, 1, 8), gapped(2, 3, 8)), {}), ValueError, MIX_ADJ),
    ("k30-u-heads-apart", "cls_token_mix", lambda: ((f32(2, 2, 16)[..., :8], f32(2, 3, 8)), {}), ValueError, MIX_ADJ),
    ("k30-out-shape", "cls_token_mix", lambda: ((f32(2, 1, 8), f32(2, 3, 8)), dict(out=f32(2, 8))), TypeError, MIX_OUT),
    ("k30-out-heads-apart", "cls_token_mix", lambda: ((f32(2, 2, 8), f32(2, 3, 8)), dict(out=f32(2, 2, 16)[..., :8])),
     TypeError, MIX_OUT),
    # K31
    ("k31-host", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, host(9, 1)), {}), TypeError, NEED_GPU),
    ("k31-qkv-dtype", "window_attention", lambda: ((f32(1, 6, 96, dtype=torch.float64), (2, 3), 2, 0, f32(9, 1)), {}),
     TypeError, WIN_QKV),
    ("k31-qkv-gapped", "window_attention", lambda: ((gapped(1, 6, 96), (2, 3), 2, 0, f32(9, 1)), {}), TypeError, WIN_QKV),
    ("k31-table-rank", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, f32(9)), {}), TypeError, WIN_TABLE),
    ("k31-table-gapped", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, gapped(9, 1)), {}), TypeError, WIN_TABLE),
    ("k31-tokens", "window_attention", lambda: ((f32(1, 5, 96), (2, 3), 2, 0, f32(9, 1)), {}), ValueError,
     "window_attention: qkv (1, 5, 96) is not [B, 2*3, 3 * 1 heads * 32]"),
    ("k31-width", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, f32(9, 2)), {}), ValueError,
     "window_attention: qkv (1, 6, 96) is not [B, 2*3, 3 * 2 heads * 32]"),
    ("k31-table-rows", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, f32(8, 1)), {}), ValueError,
     "window_attention: the table has 8 rows, window 2 needs 9"),
    ("k31-pad-size", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, f32(9, 1)), dict(pad_qkv=f32(32))),
     TypeError, WIN_PAD),
    ("k31-pad-dtype", "window_attention",
     lambda: ((f32(1, 6, 96), (2, 3), 2, 0, f32(9, 1)), dict(pad_qkv=f32(96, dtype=torch.float64))), TypeError, WIN_PAD),
    ("k31-out", "window_attention", lambda: ((f32(1, 6, 96), (2, 3), 2, 0, f32(9, 1)), dict(out=f32(1, 6, 96))), TypeError,
     "out must be a contiguous float32 [B, H*W, heads*32] tensor"),
    # K32
    ("k32-host", "patch_merge_ln", lambda: ((f32(1, 6, 8), (2, 3), f32(32), host(32), EPS), {}), TypeError, NEED_GPU),
    ("k32-dtype", "patch_merge_ln", lambda: ((f32(1, 6, 8, dtype=torch.float64), (2, 3), f32(32), f32(32), EPS), {}),
     TypeError, "x must be a contiguous float32 [B, H*W, C] tensor"),
    ("k32-rank", "patch_merge_ln", lambda: ((f32(1, 2, 3, 8), (2, 3), f32(32), f32(32), EPS), {}), TypeError,
     "x must be a contiguous float32 [B, H*W, C] tensor"),
    ("k32-tokens", "patch_merge_ln", lambda: ((f32(1, 6, 8), (2, 2), f32(32), f32(32), EPS), {}), ValueError,
     "patch_merge_ln: x has 6 tokens, the grid is 2x2"),
    ("k32-weight-shape", "patch_merge_ln", lambda: ((f32(1, 6, 8), (2, 3), f32(8), f32(32), EPS), {}), TypeError, PM_WB),
    ("k32-bias-dtype", "patch_merge_ln", lambda: ((f32(1, 6, 8), (2, 3), f32(32), f32(32, dtype=torch.float64), EPS), {}),
     TypeError, PM_WB),
    ("k32-bias-gapped", "patch_merge_ln", lambda: ((f32(1, 6, 8), (2, 3), f32(32), gapped(32), EPS), {}), TypeError, PM_WB),
    ("k32-out", "patch_merge_ln", lambda: ((f32(1, 6, 8), (2, 3), f32(32), f32(32), EPS), dict(out=f32(1, 6, 32))),
     TypeError, "out must be a contiguous float32 [B, ceil(H/2)*ceil(W/2), 4C] tensor"),
    # K10
    ("k10-host", "layer_norm", lambda: ((f32(2, 8), host(8), f32(8), EPS), {}), TypeError, NEED_GPU),
    ("k10-dtype", "layer_norm", lambda: ((f32(2, 8, dtype=torch.float64), f32(8), f32(8), EPS), {}), TypeError, LN),
    ("k10-gapped", "layer_norm", lambda: ((gapped(2, 8), f32(8), f32(8), EPS), {}), TypeError, LN),
    ("k10-weight", "layer_norm", lambda: ((f32(2, 8), f32(4), f32(8), EPS), {}), TypeError, LN),
    ("k10-bias", "layer_norm", lambda: ((f32(2, 8), f32(8), f32(1, 8), EPS), {}), TypeError, LN),
    # K24
    ("k24-host", "text_embed_ln", lambda: te(word=host(7, 8)), TypeError, NEED_GPU),
    ("k24-out-host", "text_embed_ln", lambda: te(out=host(2, 3, 8)), TypeError, NEED_GPU),
    ("k24-ids-rank", "text_embed_ln", lambda: te(ids=i64(6)), TypeError, TE_IDS),
    ("k24-ids-dtype", "text_embed_ln", lambda: te(ids=i32(2, 3)), TypeError, TE_IDS),
    ("k24-types-dtype", "text_embed_ln", lambda: te(type_ids=i32(2, 3)), TypeError, TE_IDS),
    ("k24-types-shape", "text_embed_ln", lambda: te(type_ids=i64(2, 2)), TypeError, TE_IDS),
    ("k24-word-dtype", "text_embed_ln", lambda: te(word=f32(7, 8, dtype=torch.float64)), TypeError, TE_TABLES),
    ("k24-pos-rank", "text_embed_ln", lambda: te(pos=f32(1, 4, 8)), TypeError, TE_TABLES),
    ("k24-table-gapped", "text_embed_ln", lambda: te(table=gapped(2, 8)), TypeError, TE_TABLES),
    ("k24-pos-width", "text_embed_ln", lambda: te(pos=f32(4, 4)), ValueError, TE_WIDTH),
    ("k24-table-width", "text_embed_ln", lambda: te(table=f32(2, 16)), ValueError, TE_WIDTH),
    ("k24-weight", "text_embed_ln", lambda: te(weight=f32(4)), ValueError, TE_WIDTH),
    ("k24-bias", "text_embed_ln", lambda: te(bias=f32(8, 1)), ValueError, TE_WIDTH),
    ("k24-no-token", "text_embed_ln", lambda: te(ids=i64(2, 0)), ValueError,
     "text_embed_ln: T=0 tokens, the position table has 4 rows"),
    ("k24-long", "text_embed_ln", lambda: te(ids=i64(2, 5)), ValueError,
     "text_embed_ln: T=5 tokens, the position table has 4 rows"),
    ("k24-id-high", "text_embed_ln", lambda: te(ids=torch.full((2, 3), 7)), ValueError, "text_embed_ln: ids outside [0, 7)"),
    ("k24-id-negative", "text_embed_ln", lambda: te(ids=torch.full((2, 3), -1)), ValueError,
     "text_embed_ln: ids outside [0, 7)"),
    ("k24-type-high", "text_embed_ln", lambda: te(type_ids=torch.full((2, 3), 2)), ValueError,
     "text_embed_ln: type_ids outside [0, 2)"),
    ("k24-out", "text_embed_ln", lambda: te(out=f32(2, 3, 4)), TypeError, "out must be a contiguous float32 [B, T, D] tensor"),
    # K11
    ("k11-host", "patchify", lambda: ((host(1, 3, 4, 4), 2), {}), TypeError, NEED_GPU),
    ("k11-dtype", "patchify", lambda: ((f32(1, 3, 4, 4, dtype=torch.float64), 2), {}), TypeError,
     "patchify: contiguous float32 [B, Cin, H, W]"),
    ("k11-rank", "patchify", lambda: ((f32(3, 4, 4), 2), {}), TypeError, "patchify: contiguous float32 [B, Cin, H, W]"),
    ("k11-gapped", "patchify", lambda: ((gapped(1, 3, 4, 4), 2), {}), TypeError, "patchify: contiguous float32 [B, Cin, H, W]"),
    ("k11-height", "patchify", lambda: ((f32(1, 3, 5, 4), 2), {}), ValueError,
     "patchify: 5x4 is not a multiple of the 2-pixel patch"),
    ("k11-width", "patchify", lambda: ((f32(1, 3, 4, 6), 4), {}), ValueError,
     "patchify: 4x6 is not a multiple of the 4-pixel patch"),
    # K28
    ("k28-host", "patchify_kept", lambda: ((host(1, 3, 4, 4), 2, i32(1, 2)), {}), TypeError, NEED_GPU),
    ("k28-keep-host", "patchify_kept", lambda: ((f32(1, 3, 4, 4), 2, host(1, 2, dtype=torch.int32)), {}), TypeError, NEED_GPU),
    ("k28-gapped", "patchify_kept", lambda: ((gapped(1, 3, 4, 4), 2, i32(1, 2)), {}), TypeError,
     "patchify_kept: contiguous float32 [B, Cin, H, W]"),
    ("k28-size", "patchify_kept", lambda: ((f32(1, 3, 4, 6), 4, i32(1, 2)), {}), ValueError,
     "patchify_kept: 4x6 is not a multiple of the 4-pixel patch"),
    ("k28-keep-dtype", "patchify_kept", lambda: ((f32(1, 3, 4, 4), 2, i64(1, 2)), {}), TypeError,
     "keep must be a contiguous int32 [B, n] tensor"),
    ("k28-keep-rank", "patchify_kept", lambda: ((f32(1, 3, 4, 4), 2, i32(2)), {}), TypeError,
     "keep must be a contiguous int32 [B, n] tensor"),
    ("k28-keep-batch", "patchify_kept", lambda: ((f32(1, 3, 4, 4), 2, i32(2, 2)), {}), TypeError,
     "keep must be a contiguous int32 [B, n] tensor"),
    ("k28-keep-gapped", "patchify_kept", lambda: ((f32(1, 3, 4, 4), 2, gapped(1, 2, dtype=torch.int32)), {}), TypeError,
     "keep must be a contiguous int32 [B, n] tensor"),
    # K29
    ("k29-host", "token_restore", lambda: tr(src=host(2, 3, 8)), TypeError, NEED_GPU),
    ("k29-fill-host", "token_restore", lambda: tr(fill=host(8)), TypeError, NEED_GPU),
    ("k29-src-dtype", "token_restore", lambda: tr(src=f32(2, 3, 8, dtype=torch.float64)), TypeError, SRC),
    ("k29-src-rank", "token_restore", lambda: tr(src=f32(2, 1, 3, 8)), TypeError, SRC),
    ("k29-src-gapped", "token_restore", lambda: tr(src=gapped(2, 3, 8)), TypeError, SRC),
    ("k29-images", "token_restore", lambda: tr(src=f32(3, 3, 8)), ValueError,
     "token_restore: src has 3 images, restore (2, 4)"),
    ("k29-restore-dtype", "token_restore", lambda: tr(restore=i64(2, 4)), TypeError,
     "restore must be a contiguous int32 [B, n] tensor"),
    ("k29-restore-rank", "token_restore", lambda: tr(src=f32(3, 8), restore=i32(8)), TypeError,
     "restore must be a contiguous int32 [B, n] tensor"),
    ("k29-restore-gapped", "token_restore", lambda: tr(restore=gapped(2, 4, dtype=torch.int32)), TypeError,
     "restore must be a contiguous int32 [B, n] tensor"),
    ("k29-no-row", "token_restore", lambda: tr(src=f32(0, 8)), ValueError, "token_restore: src has no row 0"),
    ("k29-fill-shape", "token_restore", lambda: tr(fill=f32(4)), TypeError,
     "fill must be a contiguous float32 tensor of shape (8,)"),
    ("k29-fill-dtype", "token_restore", lambda: tr(fill=f32(8, dtype=torch.float64)), TypeError,
     "fill must be a contiguous float32 tensor of shape (8,)"),
    ("k29-add-shape", "token_restore", lambda: tr(add=f32(4, 8)), TypeError,
     "add must be a contiguous float32 tensor of shape (5, 8)"),
    ("k29-add-gapped", "token_restore", lambda: tr(add=gapped(5, 8)), TypeError,
     "add must be a contiguous float32 tensor of shape (5, 8)"),
    ("k29-out", "token_restore", lambda: tr(out=f32(2, 4, 8)), TypeError,
     "out must be a contiguous float32 [B, 1 + L, D] tensor"),
]


class Recorder:
    """Stands in for the loaded library: every entry records its name and arguments and reports MCD_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture
def recorded(core, monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(core._lib, "load", lambda: rec)
    monkeypatch.setattr(core, "_stream", lambda: STREAM)
    return rec


@pytest.mark.parametrize("wrapper,make,exc,text", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_an_input_with_one_fault_is_refused_before_the_library(core, recorded, wrapper, make, exc, text):
    args, kwargs = make()
    with pytest.raises(exc) as e:
        getattr(core, wrapper).__wrapped__(*args, **kwargs)
    assert str(e.value) == text
    assert recorded.calls == []


def test_the_refusal_table_names_every_wrapper_in_scope():
    assert {r[1] for r in REFUSALS} == {
        "vit_attention", "vit_attention_long", "vit_attention_keylen", "vit_attention_relbias", "vit_attention_causal",
        "masked_mean_l2", "quick_gelu", "token_mean", "vit_attention_cls", "cls_token_mix", "window_attention",
        "patch_merge_ln", "layer_norm", "text_embed_ln", "patchify", "patchify_kept", "token_restore"}
    assert len({r[0] for r in REFUSALS}) == len(REFUSALS)


# ---- accepted calls -------------------------------------------------------------------------------------------------------
def symbolic(args, operands):
    """The recorded arguments with every address inside an operand's storage written as (operand, byte offset)."""
    out = []
    for a in args:
        if isinstance(a, int) and not isinstance(a, bool):
            for name, t in operands.items():
                base = t.untyped_storage().data_ptr()
                if base <= a < base + t.untyped_storage().nbytes():
                    a = (name, a - base)
                    break
        out.append(a)
    return tuple(out)


def A(fn, operands, *args, **kwargs):
    """One accepted call: the wrapper's name, the named operands (base tensors; the arguments may be views of them), the
    arguments."""
    return fn, operands, args, kwargs


def accepted_calls():
    """(id, call, entry, arguments, shape of the result).  ("out", 0) in the arguments is the returned tensor; an `out`
    operand is the caller's and must be the one returned."""
    S = STREAM
    cases = []

    def add(ident, call, entry, args, shape):
        cases.append(pytest.param(call, entry, args, shape, id=ident))

    # K9, K9L, K9A
    o = dict(qkv=f32(2, 5, 384))
    add("k9", A("vit_attention", o, o["qkv"], 2), "mcd_vit_attention", (("qkv", 0), 2, 5, 2, ("out", 0), S), (2, 5, 128))
    o = dict(qkv=f32(1, 3, 192), out=f32(1, 3, 64))
    add("k9-out", A("vit_attention", o, o["qkv"], 1, out=o["out"]), "mcd_vit_attention",
        (("qkv", 0), 1, 3, 1, ("out", 0), S), (1, 3, 64))
    o = dict(qkv=f32(1, 3, 192))
    add("k9l", A("vit_attention_long", o, o["qkv"], 1), "mcd_vit_attention_long", (("qkv", 0), 1, 3, 1, ("out", 0), S),
        (1, 3, 64))
    o = dict(qkv=f32(2, 5, 384), out=f32(2, 5, 128))
    add("k9l-out", A("vit_attention_long", o, o["qkv"], 2, o["out"]), "mcd_vit_attention_long",
        (("qkv", 0), 2, 5, 2, ("out", 0), S), (2, 5, 128))
    o = dict(qkv=f32(2, 5, 192))
    add("k9a", A("vit_attention_causal", o, o["qkv"], 1), "mcd_vit_attention_causal", (("qkv", 0), 2, 5, 1, ("out", 0), S),
        (2, 5, 64))
    # K9M
    o = dict(qkv=f32(2, 5, 192))
    add("k9m-none", A("vit_attention_keylen", o, o["qkv"], 1, None), "mcd_vit_attention_keylen",
        (("qkv", 0), 2, 5, 1, None, ("out", 0), S), (2, 5, 64))
    o = dict(qkv=f32(2, 5, 384), lens=i32(2), out=f32(2, 5, 128))
    add("k9m-lens-out", A("vit_attention_keylen", o, o["qkv"], 2, o["lens"], out=o["out"]), "mcd_vit_attention_keylen",
        (("qkv", 0), 2, 5, 2, ("lens", 0), ("out", 0), S), (2, 5, 128))
    # K9B
    o = dict(qkv=f32(2, 5, 192))
    add("k9b-none", A("vit_attention_relbias", o, o["qkv"], 1, None, None), "mcd_vit_attention_relbias",
        (("qkv", 0), 2, 5, 1, None, None, ("out", 0), S), (2, 5, 64))
    o = dict(qkv=f32(2, 5, 384), lens=i32(2), rel=f32(2, 9))
    add("k9b-lens-rel", A("vit_attention_relbias", o, o["qkv"], 2, o["lens"], o["rel"]), "mcd_vit_attention_relbias",
        (("qkv", 0), 2, 5, 2, ("lens", 0), ("rel", 0), ("out", 0), S), (2, 5, 128))
    o = dict(qkv=f32(1, 2, 192), rel=f32(1, 3), out=f32(1, 2, 64))
    add("k9b-rel-out", A("vit_attention_relbias", o, o["qkv"], 1, None, o["rel"], o["out"]), "mcd_vit_attention_relbias",
        (("qkv", 0), 1, 2, 1, None, ("rel", 0), ("out", 0), S), (1, 2, 64))
    # K27
    o = dict(x=f32(2, 4, 8))
    add("k27-none", A("masked_mean_l2", o, o["x"], None), "mcd_masked_mean_l2", (("x", 0), 2, 4, 8, None, 1, ("out", 0), S),
        (2, 8))
    o = dict(x=f32(2, 4, 8), lens=i32(2), out=f32(2, 8))
    add("k27-lens-raw-out", A("masked_mean_l2", o, o["x"], o["lens"], normalize=False, out=o["out"]), "mcd_masked_mean_l2",
        (("x", 0), 2, 4, 8, ("lens", 0), 0, ("out", 0), S), (2, 8))
    # K25
    o = dict(x=f32(2, 3, 4))
    add("k25", A("quick_gelu", o, o["x"]), "mcd_quick_gelu", (("x", 0), 24, ("out", 0), S), (2, 3, 4))
    add("k25-in-place", A("quick_gelu", o, o["x"], out=o["x"]), "mcd_quick_gelu", (("x", 0), 24, ("x", 0), S), (2, 3, 4))
    # K26
    o = dict(x=f32(2, 5, 8))
    add("k26", A("token_mean", o, o["x"]), "mcd_token_mean", (("x", 0), 2, 5, 8, 40, 8, 1, ("out", 0), 8, S), (2, 8))
    o = dict(base=f32(2, 6, 16), out=f32(2, 12))
    add("k26-views", A("token_mean", o, o["base"][:, 1:, 4:12], t0=2, out=o["out"][:, :8]), "mcd_token_mean",
        (("base", 80), 2, 5, 8, 96, 16, 2, ("out", 0), 12, S), (2, 8))
    # K9C
    o = dict(qkv=f32(2, 5, 3, 2, 64))
    add("k9c-views", A("vit_attention_cls", o, o["qkv"][:, 0, 0], o["qkv"][:, :, 1], o["qkv"][:, :, 2]),
        "mcd_vit_attention_cls", (("qkv", 0), 1920, ("qkv", 512), 384, 1920, ("qkv", 1024), 384, 1920, 2, 5, 2, ("out", 0), S),
        (2, 128))
    o = dict(q=f32(1, 64), k=f32(1, 1, 1, 64), v=f32(1, 1, 1, 64), out=f32(1, 64))
    add("k9c-one", A("vit_attention_cls", o, o["q"], o["k"], o["v"], out=o["out"]), "mcd_vit_attention_cls",
        (("q", 0), 64, ("k", 0), 64, 64, ("v", 0), 64, 64, 1, 1, 1, ("out", 0), S), (1, 64))
    o = dict(q=f32(2, 128), k=f32(2, 3, 2, 64), v=f32(2, 3, 2, 64))
    add("k9c-flat-q", A("vit_attention_cls", o, o["q"], o["k"], o["v"]), "mcd_vit_attention_cls",
        (("q", 0), 128, ("k", 0), 128, 384, ("v", 0), 128, 384, 2, 3, 2, ("out", 0), S), (2, 128))
    # K30
    o = dict(u=f32(2, 2, 8), base=f32(2, 6, 16))
    add("k30-view", A("cls_token_mix", o, o["u"], o["base"][:, 1:, :8]), "mcd_cls_token_mix",
        (("u", 0), 16, ("base", 64), 16, 96, 2, 5, 2, 8, ("out", 0), 16, S), (2, 2, 8))
    o = dict(u=f32(1, 1, 8), n=f32(1, 1, 8))
    add("k30-one", A("cls_token_mix", o, o["u"], o["n"]), "mcd_cls_token_mix",
        (("u", 0), 8, ("n", 0), 8, 8, 1, 1, 1, 8, ("out", 0), 8, S), (1, 1, 8))
    o = dict(ubase=f32(2, 3, 8), n=f32(2, 5, 8), out=f32(2, 4, 8))
    add("k30-strided-u-out", A("cls_token_mix", o, o["ubase"][:, 1:], o["n"], out=o["out"][:, :2]), "mcd_cls_token_mix",
        (("ubase", 32), 24, ("n", 0), 8, 40, 2, 5, 2, 8, ("out", 0), 32, S), (2, 2, 8))
    # K31: a 2 x 3 grid
    o = dict(qkv=f32(1, 6, 96), table=f32(9, 1), pad=f32(96))
    add("k31-pad", A("window_attention", o, o["qkv"], (2, 3), 2, 1, o["table"], pad_qkv=o["pad"]), "mcd_window_attention",
        (("qkv", 0), ("pad", 0), 1, 2, 3, 1, 2, 1, ("table", 0), ("out", 0), S), (1, 6, 32))
    o = dict(qkv=f32(2, 6, 192), table=f32(1, 2), out=f32(2, 6, 64))
    add("k31-no-pad-out", A("window_attention", o, o["qkv"], (2, 3), 1, 0, o["table"], out=o["out"]), "mcd_window_attention",
        (("qkv", 0), None, 2, 2, 3, 2, 1, 0, ("table", 0), ("out", 0), S), (2, 6, 64))
    # K32: C = 8
    o = dict(x=f32(1, 6, 8), w=f32(32), b=f32(32))
    add("k32", A("patch_merge_ln", o, o["x"], (2, 3), o["w"], o["b"], EPS), "mcd_patch_merge_ln",
        (("x", 0), 1, 2, 3, 8, ("w", 0), ("b", 0), EPS, ("out", 0), S), (1, 2, 32))
    o = dict(x=f32(2, 4, 8), w=f32(32), b=f32(32), out=f32(2, 1, 32))
    add("k32-out", A("patch_merge_ln", o, o["x"], (2, 2), o["w"], o["b"], EPS, out=o["out"]), "mcd_patch_merge_ln",
        (("x", 0), 2, 2, 2, 8, ("w", 0), ("b", 0), EPS, ("out", 0), S), (2, 1, 32))
    # K10
    o = dict(x=f32(2, 3, 8), w=f32(8), b=f32(8))
    add("k10", A("layer_norm", o, o["x"], o["w"], o["b"], EPS), "mcd_layer_norm",
        (("x", 0), 6, 8, ("w", 0), ("b", 0), EPS, ("out", 0), S), (2, 3, 8))
    o = dict(x=f32(8), w=f32(8), b=f32(8))
    add("k10-one-row", A("layer_norm", o, o["x"], o["w"], o["b"], 1), "mcd_layer_norm",
        (("x", 0), 1, 8, ("w", 0), ("b", 0), 1.0, ("out", 0), S), (8,))
    # K24: host ids (range-checked) and ids that say they are on the device
    o = dict(ids=torch.tensor([[0, 6, 3], [1, 2, 5]]), word=f32(7, 8), pos=f32(4, 8), table=f32(2, 8), w=f32(8), b=f32(8))
    add("k24-no-types", A("text_embed_ln", o, o["ids"], None, o["word"], o["pos"], o["table"], o["w"], o["b"], EPS),
        "mcd_text_embed_ln", (("ids", 0), None, ("word", 0), ("pos", 0), ("table", 0), ("w", 0), ("b", 0), EPS, 6, 3, 8, 7, 2,
                              ("out", 0), S), (2, 3, 8))
    o = dict(ids=i64(2, 3), types=torch.tensor([[0, 1, 1], [1, 0, 0]]), word=f32(7, 8), pos=f32(3, 8), table=f32(2, 8),
             w=f32(8), b=f32(8), out=f32(2, 3, 8))
    add("k24-types-out", A("text_embed_ln", o, o["ids"], o["types"], o["word"], o["pos"], o["table"], o["w"], o["b"], EPS,
                           out=o["out"]),
        "mcd_text_embed_ln", (("ids", 0), ("types", 0), ("word", 0), ("pos", 0), ("table", 0), ("w", 0), ("b", 0), EPS, 6, 3, 8, 7,
                              2, ("out", 0), S), (2, 3, 8))
    # K11, K28
    o = dict(x=f32(1, 3, 4, 4))
    add("k11", A("patchify", o, o["x"], 2), "mcd_patchify", (("x", 0), 1, 3, 4, 4, 2, ("out", 0), S), (1, 5, 12))
    o = dict(x=f32(2, 1, 4, 8), keep=i32(2, 3))
    add("k28", A("patchify_kept", o, o["x"], 4, o["keep"]), "mcd_patchify_kept",
        (("x", 0), ("keep", 0), 2, 1, 4, 8, 4, 3, ("out", 0), S), (2, 4, 16))
    # K29
    o = dict(src=f32(2, 3, 8), restore=i32(2, 4), fill=f32(8), add=f32(5, 8))
    add("k29-fill-add", A("token_restore", o, o["src"], o["restore"], fill=o["fill"], add=o["add"]), "mcd_token_restore",
        (("src", 0), 24, ("restore", 0), ("fill", 0), ("add", 0), 2, 4, 2, 8, ("out", 0), S), (2, 5, 8))
    o = dict(src=f32(3, 8), restore=i32(2, 4), out=f32(2, 5, 8))
    add("k29-shared-table-out", A("token_restore", o, o["src"], o["restore"], out=o["out"]), "mcd_token_restore",
        (("src", 0), 0, ("restore", 0), None, None, 2, 4, 2, 8, ("out", 0), S), (2, 5, 8))
    o = dict(src=f32(1, 1, 8), restore=i32(1, 2), add=f32(3, 8))
    add("k29-add-only", A("token_restore", o, o["src"], o["restore"], add=o["add"]), "mcd_token_restore",
        (("src", 0), 8, ("restore", 0), None, ("add", 0), 1, 2, 0, 8, ("out", 0), S), (1, 3, 8))
    return cases


@pytest.mark.parametrize("call,entry,args,shape", accepted_calls())
def test_an_accepted_call_hands_the_library_these_arguments(core, recorded, call, entry, args, shape):
    wrapper, operands, a, kw = call
    got = getattr(core, wrapper).__wrapped__(*a, **kw)
    assert tuple(got.shape) == shape and got.dtype == torch.float32 and got.device == torch.device("cpu")
    new = "out" not in operands and ("out", 0) in args
    assert new != any(got is t for t in list(a) + list(kw.values()))       # the caller's own `out` comes back, not a copy
    if new:
        assert not any(got.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for t in operands.values())
        assert got.is_contiguous()
    (name, raw), = recorded.calls
    assert name == entry
    assert symbolic(raw, dict(operands, **({} if "out" in operands else {"out": got}))) == args
    for x, y in zip(symbolic(raw, {}), args):           # EPS and the flags compare equal across int / float: pin the type
        if not isinstance(y, tuple):
            assert type(x) is type(y), (x, y)


# ---- the K9 family's C entries: K9, K9M, K9B, K9A -----------------------------------------------------------------------
P, Q, R, LENS = 4096, 8192, 16384, 32768     # aligned non-NULL addresses: the checks return before anything is touched
K9_ENTRIES = {              # entry -> its alignment sentence
    "mcd_vit_attention": "qkv and out must be 16-byte aligned",
    "mcd_vit_attention_keylen": "qkv and out must be 16-byte aligned, lens 4-byte aligned",
    "mcd_vit_attention_relbias": "qkv, out and rel must be 16-byte aligned, lens 4-byte aligned",
    "mcd_vit_attention_causal": "qkv and out must be 16-byte aligned",
}
E_ARG, E_UNSUPPORTED = -1, -5


def k9(mcd, name, qkv=P, B=1, T=4, H=1, lens=None, rel=None, out=Q):
    """(status, mcd_last_error()) of one of the four entries; lens and rel go to the entries that take them."""
    extra = {"mcd_vit_attention_keylen": (lens,), "mcd_vit_attention_relbias": (lens, rel)}.get(name, ())
    rc = util.entry_rc(mcd, name, qkv, B, T, H, *extra, out, None)
    return rc, mcd._lib.load().mcd_last_error().decode()


@pytest.mark.parametrize("name", sorted(K9_ENTRIES))
def test_the_k9_entries_refuse_bad_arguments_before_any_device_call(mcd, name):
    limit = (E_UNSUPPORTED, name + ": B and H must be <= 65535")
    aligned = (E_ARG, "%s: %s" % (name, K9_ENTRIES[name]))
    assert k9(mcd, name, qkv=None) == (E_ARG, name + ": NULL pointer")
    assert k9(mcd, name, out=None) == (E_ARG, name + ": NULL pointer")
    assert k9(mcd, name, T=0) == (E_ARG, name + ": bad shape B=1 T=0 H=1")
    assert k9(mcd, name, T=257) == (E_UNSUPPORTED, name + ": T=257 tokens, at most 256 (one wave per 32 queries, 8 waves)")
    assert k9(mcd, name, B=65536) == limit
    assert k9(mcd, name, H=65536) == limit
    assert k9(mcd, name, qkv=P + 4) == aligned
    assert k9(mcd, name, out=Q + 4) == aligned
    if name in ("mcd_vit_attention_keylen", "mcd_vit_attention_relbias"):
        assert k9(mcd, name, lens=LENS + 2) == aligned
        assert k9(mcd, name, lens=LENS, T=0)[0] == E_ARG
    if name == "mcd_vit_attention_relbias":
        assert k9(mcd, name, rel=R + 4) == aligned
        assert k9(mcd, name, lens=LENS, rel=R + 4) == aligned
    # the order of the checks: a NULL pointer before the shape, the shape before the limits, the limits before the alignment
    assert k9(mcd, name, qkv=None, T=0)[1] == name + ": NULL pointer"
    assert k9(mcd, name, T=0, B=65536)[1] == name + ": bad shape B=65536 T=0 H=1"
    assert k9(mcd, name, T=257, H=65536)[0:1] == (E_UNSUPPORTED,) and "T=257" in k9(mcd, name, T=257, H=65536)[1]
    assert k9(mcd, name, B=65536, out=Q + 4) == limit
    # no image: MCD_OK and nothing is launched (there is no device here to launch on)
    assert k9(mcd, name, B=0)[0] == 0
    assert k9(mcd, name, B=0, lens=LENS, rel=R)[0] == 0
    assert k9(mcd, name, B=0, out=Q + 4) == aligned          # ... but only after every check
    assert k9(mcd, name, B=-1)[0] == E_ARG
