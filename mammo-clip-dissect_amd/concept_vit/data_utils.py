"""Offline target-model and probe-data factory: mirror of the reference's concept_vit/data_utils.py.

Same entry points -- get_target_model(target_name, device, ...) -> (model.eval(), preprocess) and
get_data(dataset_name, preprocess) -- (reference data_utils.py:38-93, :102-311), but every reference
loader fetches weights or datasets from the network, which this build never does.
Here the architectures are built locally with the hook-point names the reference's launch scripts use
(run_clipdissect.sh, run_og_clip.sh) and get random-init weights under a fixed seed, or weights from a
LOCAL checkpoint path.  These modules are host-side PyTorch plumbing (the encoder forwards); the
dissection core they feed is the HIP library.

    target_name            hook points (target_layers)                 neurons
    breastclip             image_encoder._blocks[0..38]                EfficientNet-B5: 6992 (with a checkpoint: the tower
                                                                       its keys name -- EfficientNet b0 .. b7, B2 = the
                                                                       second released Mammo-CLIP, 23 blocks; or Swin)
    breastclip_vit         image_encoder.encoder.layer[0..11]          ViT-B/16: 12 x 768
    breastclip_swin        image_encoder.image_encoder.encoder.layers[0..3] (and .blocks[j])   Swin-T: 192/384/768/768
                                                                       (sized from a checkpoint's shapes when one is given)
    breastclip_classifier  image_encoder._blocks[0..38]                + linear head (n_class); the tower follows the
                                                                       checkpoint as for breastclip
    clip                   vision_model.encoder.layers[0..11]          CLIP ViT-B/16: 12 x 768 (with a checkpoint, ckpt= or
                                                                       registered: HFClip = CLIPForImageClassification)
    resnet50 / 101 / 152   conv1, layer1..layer4                       64/256/512/1024/2048
    resnet18 / 34          conv1, layer1..layer4                       64/64/128/256/512
    resnet18_places        as resnet18, 365 classes (reference :70-79)
    clip_rn50 / clip_rn101 visual.layer1..layer4, visual.attnpool      CLIP RN50 / RN101: 256/512/1024/2048, 1024 | 512
    openai_clip            visual.transformer.resblocks[i], transformer.resblocks[i]   OpenAI CLIP under its own keys (ckpt=)
    vit / -cub / -bloodmnist   vit.encoder.layer[0..11]                HF ViT-B/16 classifier: 12 x 768
    dino / -cub / -bloodmnist  dinov2.encoder.layer[0..11]             HF DINOv2-base classifier (patch 14): 12 x 768
    mae                    vit.encoder.layer[0..11]                    HF ViT-MAE-base (with a checkpoint, ckpt= or registered:
                                                                       HFMae = ViTMAEForPreTraining): 12 x 768
"""
import collections
import math
import os
import unicodedata
import zlib

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.modules import module as _nn_module

from .. import core
from . import checkpoint_io

PROJ_DIM = 512
# The image tower's mask-free fp32 attention runs on the HIP kernels K9 (T <= 256) and K9L (longer sequences, the
# high-resolution towers); MCD_NO_HIP_ATTENTION=1 (or setting this to False) keeps PyTorch's SDPA, e.g. to time one
# against the other.  Masked (text tower), autograd or non-fp32 calls always take SDPA (attention_route).
HIP_ATTENTION = os.environ.get("MCD_NO_HIP_ATTENTION", "0") != "1"
# bench.py sets this to a list to time K9 inside the forwards: every 8th call appends (start, end, B, T, heads) with
# two HIP events recorded on the launch stream around the kernel.
ATTENTION_EVENTS = None
_attention_calls = 0
# The two residual updates of a block, x + proj(.) and x + fc2(.), as one hipBLASLt GEMM each (bias epilogue + beta*C,
# core.linear_residual) instead of nn.Linear + an elementwise add over the residual stream.  Inference-time fp32 only;
# MCD_NO_FUSED_RESIDUAL=1 (or False here, or a missing libmcd_blaslt.so) keeps PyTorch's two kernels.
FUSED_RESIDUAL = os.environ.get("MCD_NO_FUSED_RESIDUAL", "0") != "1"
# encode_image reads token 0 of the tower's output, and so does every activation hook of the package (core.hook_pool
# on a 3-D output): of the LAST encoder block only the class-token row is ever used.  With this on, that block computes
# K and V for all tokens and everything else (q, attention on K9C, proj, the MLP, the final LayerNorm) for the class
# token alone and returns [B, 1, D] (cls_tail_route).  MCD_NO_CLS_ONLY_TAIL=1 (or False here) keeps the full block.
CLS_ONLY_TAIL = os.environ.get("MCD_NO_CLS_ONLY_TAIL", "0") != "1"
# The class-token tail without its K|V projection (cls_fold_route, _attend_cls_folded): the one query row needs
# q_h . k_t = (W_k,h^T q_h) . n_t and sum_t p_t v_t = W_v,h (sum_t p_t n_t) + b_v,h, so W_k and W_v are applied to one
# row per image and K30 (core.cls_token_mix) does the rest on LN1(x).  MCD_NO_CLS_FOLD=1 (or False here) keeps the K|V
# GEMM + K9C.  The fold trades one GEMM of B*T rows for 2 * heads + 1 launches that do not shrink with the batch, so it is
# taken from CLS_FOLD_MIN_ROWS token rows (B*T) up.  Measured on the ViT-B/16 tail block (scripts/cls_fold_timing.py,
# profiles/cls_fold_timing.txt): the folded tail takes 0.73 ms at any small batch (its launches), the K|V GEMM + K9C
# 0.59 ms at 25 216 rows and 1.10 ms at 50 432; the two cross near 32 000 rows.  At 492 500 rows: 1.74 against 9.31 ms.
CLS_FOLD = os.environ.get("MCD_NO_CLS_FOLD", "0") != "1"
CLS_FOLD_MIN_ROWS = 32768


# nn.LayerNorm of the towers on the HIP kernel K10 (csrc/k_ln.hip); MCD_NO_HIP_LAYER_NORM=1 keeps ATen's.
HIP_LAYER_NORM = os.environ.get("MCD_NO_HIP_LAYER_NORM", "0") != "1"
# The EfficientNet-B5 tower's inference route (mbconv_route): channels-last activations, batch norm folded into the
# weights, every 1x1 convolution one hipBLASLt GEMM (core.linear_residual) and K12-K15 / K0n (csrc/k_mbconv.hip) for the
# rest.  MCD_NO_HIP_MBCONV=1 (or setting this to False) keeps the ATen route: MIOpen convolutions, ATen batch norm,
# SiLU, mean, sigmoid-multiply and add -- the tests' reference and the other side of the timing A/B.
HIP_MBCONV = os.environ.get("MCD_NO_HIP_MBCONV", "0") != "1"
# The ResNet targets' inference route on channels-last activations with folded batch norm (core.conv7x7s2_nhwc,
# bn_relu_maxpool_nhwc, conv_igemm_nhwc: K16-K18).  Bottleneck networks (50 / 101 / 152): the 1x1 convolutions are
# hipBLASLt GEMMs with the skip add and the ReLU in their epilogue.  BasicBlock networks (18 / 34 / resnet18_places):
# every convolution is K18, the skip add and the ReLU in its epilogue -- no library GEMM in front of a hooked output.
# MCD_NO_HIP_RESNET=1 restores the ATen NCHW route everywhere.
HIP_RESNET = os.environ.get("MCD_NO_HIP_RESNET", "0") != "1"
# The OpenAI-CLIP RN50 / RN101 dissectors' inference route (clip_rn_route): the anti-aliased stem on K19 + K18 + K20, the
# blocks on GEMMs + K18 + K20 (the 2x2 average pooling that stands in for every stride), the attention pool on K21, two
# GEMMs, K9C and c_proj.  MCD_NO_HIP_CLIP_RN=1 (or setting this to False) keeps the ATen route of the same modules.
HIP_CLIP_RN = os.environ.get("MCD_NO_HIP_CLIP_RN", "0") != "1"
# The BERT text tower's inference route (text_route): the embedding rows on K24, per layer the fused qkv GEMM, K9M (the
# attention with a key count per sequence: the padded batch's mask), the two residual GEMMs and K10 behind each.
# MCD_NO_HIP_TEXT=1 (or setting this to False) keeps the ATen route of the same modules, SDPA under the mask included.
HIP_TEXT = os.environ.get("MCD_NO_HIP_TEXT", "0") != "1"
# OpenAIClip's inference route (clip_tower_route), both towers: per block K10, the fused qkv GEMM, K9A (the text side's causal
# attention) or K9 / K9L (the image side), the two residual GEMMs and K25 (QuickGELU) behind c_fc.  MCD_NO_HIP_CLIP_TEXT=1 (or
# setting this to False) keeps the ATen route of the same modules: SDPA with is_causal and x * sigmoid(1.702 x).
HIP_CLIP_TEXT = os.environ.get("MCD_NO_HIP_CLIP_TEXT", "0") != "1"
MAX_BATCH = 65535     # the images of one call that the K12-K18 entries accept


# ---- the gate: when a forward may leave ATen for the HIP kernels ---------------------------------------------------------
def _hip_eligible(on_gpu, dtype, grad):
    """The base of every route: a call may leave ATen when it is fp32 on the GPU and autograd does not record it."""
    return bool(on_gpu) and dtype == torch.float32 and not grad


def _eligible(x):
    """_hip_eligible for the tensor a module was called with, under the current grad mode."""
    return isinstance(x, torch.Tensor) and _hip_eligible(x.is_cuda, x.dtype, torch.is_grad_enabled())


def _tower_gate(flag, module, x):
    """What mbconv_route and resnet_route ask before they look at shapes: the route's flag, an eligible 4-D tensor, eval
    mode, at most MAX_BATCH images, and libmcd_blaslt.so loaded (the 1x1 convolutions are its GEMMs)."""
    return bool(flag and _eligible(x) and x.dim() == 4 and not module.training and x.shape[0] <= MAX_BATCH
                and core.linear_residual_available())


def _under_2g(*elements):
    """Every one of these fp32 element counts (one image's tensors) is under 2^31 bytes: the kernels index an image
    with 32-bit byte offsets."""
    return all(n * 4 < 2 ** 31 for n in elements)


class _LayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameters / state_dict keys); inference-time fp32 CUDA inputs take K10."""

    def forward(self, x):
        D = x.shape[-1]
        if (HIP_LAYER_NORM and _eligible(x) and x.is_contiguous() and len(self.normalized_shape) == 1 and D % 4 == 0
                and D <= 2048 and self.weight is not None and self.bias is not None):
            return core.layer_norm(x, self.weight, self.bias, self.eps)
        return super().forward(x)


def _linear(mod, x):
    """mod(x) for an nn.Linear; on the fused path through libmcd_blaslt.so as well (res = None: same hipBLASLt GEMM with
    the bias epilogue as PyTorch's, but with this process's own best-of-32 pick instead of the library default)."""
    if _fused_residual_ok(x) and x.is_contiguous() and mod.bias is not None:
        return core.linear_residual(None, x, mod.weight, mod.bias)
    return mod(x)


def _fused_residual_ok(x):
    return bool(FUSED_RESIDUAL and _eligible(x) and core.linear_residual_available())


# ------------------------------------------------------------------------------------------------------
# ViT-B/16 tower (module names follow HF ViTModel: embeddings / encoder.layer[i] / layernorm)
# ------------------------------------------------------------------------------------------------------
def attention_route(T, D, heads, masked, on_gpu, dtype, needs_grad):
    """Which attention a _Block takes for T tokens of width D = 64 * heads: 'k9' (T <= 256), 'long' (K9L,
    up to core.VIT_ATTENTION_LONG_MAX_T tokens and one image's qkv under 2^31 bytes) or 'sdpa' (masked, autograd,
    non-fp32 or off-GPU calls, HIP_ATTENTION off, other head widths, and anything past K9L's limits)."""
    if not (HIP_ATTENTION and not masked and _hip_eligible(on_gpu, dtype, needs_grad) and D == 64 * heads):
        return "sdpa"
    if T <= core.VIT_ATTENTION_MAX_T:
        return "k9"
    if T <= core.VIT_ATTENTION_LONG_MAX_T and _under_2g(T * 3 * D):
        return "long"
    return "sdpa"


def cls_tail_route(flag, fused_ok, masked, training, T, D, heads, depth, hooks_clear, last_hooks_token0):
    """Whether a tower forward asked for its class token only may prune its last block to that row: CLS_ONLY_TAIL
    (`flag`) and HIP_ATTENTION on, the fused-residual path available for the call (fp32 on the GPU, no autograd:
    `fused_ok`), no mask, eval mode, D = 64 * heads, T within K9C's limit, at least one block, no hook that would see a
    skipped call or a pruned tensor (`hooks_clear`: no global hooks, none inside the last block, none on the encoder or
    the final LayerNorm, no pre-hook on the last block) and every forward hook on the last block or on the tower
    declaring token0_only (`last_hooks_token0`)."""
    return bool(flag and HIP_ATTENTION and fused_ok and not masked and not training and D == 64 * heads
                and 1 <= T <= core.VIT_ATTENTION_CLS_MAX_T and depth >= 1 and hooks_clear and last_hooks_token0)


def cls_fold_route(flag, B, T, D, heads, min_rows):
    """Whether a class-token tail that cls_tail_route has opened also folds its K|V projection away: CLS_FOLD (`flag`),
    at least `min_rows` token rows in the call (CLS_FOLD_MIN_ROWS) and K30's limits -- D = 64 * heads <= 2 048, T within
    its LDS budget, B within its grid."""
    return bool(flag and B * T >= min_rows and D == 64 * heads and D <= 2048 and 1 <= B <= core.CLS_TOKEN_MIX_MAX_B
                and 1 <= T <= core.cls_token_mix_max_t(heads, D))


def embed_gate(P, H, W, table_rows):
    """Whether ViTTower.embed may write the patch embedding as K11 + one GEMM: an even patch size (K11 reads 16-byte
    pieces of a patch row at P % 4 == 0, 8-byte pieces at any other even P, and nothing narrower), an image of whole
    patches, and a position table with one row per token."""
    return bool(P >= 2 and P % 2 == 0 and H % P == 0 and W % P == 0 and 1 + (H // P) * (W // P) == table_rows)


def _token0_hooks(m):
    """Every forward hook on m declares (attribute token0_only) that of a [B, T, D] output it reads token 0 only."""
    return all(getattr(h, "token0_only", False) for h in m._forward_hooks.values())


def _cls_tail_ok(x, blocks, container, clear=(), token0=()):
    """cls_tail_route for the embedded tokens x [B, T, D] in front of `blocks`, the ModuleList inside `container`, and the
    hooks the tower carries right now.  clear: further modules that must carry no hook, nor hold one inside (the ViT's
    final LayerNorm); token0: the modules beside the last block whose forward hooks must declare token0_only (the ViT
    tower, whose output is the pruned tensor; none for CLIP, whose forward slices the class-token row itself)."""
    if not (CLS_ONLY_TAIL and isinstance(x, torch.Tensor) and x.dim() == 3) or len(blocks) == 0:
        return False
    last = blocks[-1]
    hooks_clear = not (_nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks or last._forward_pre_hooks
                       or any(_hooked(c) for c in last.children()) or any(_hooked(m) for m in clear)
                       or container._forward_hooks or container._forward_pre_hooks)
    return cls_tail_route(CLS_ONLY_TAIL, _fused_residual_ok(x), False, container.training or last.training, x.shape[1],
                          x.shape[2], last.attn.heads, len(blocks), hooks_clear, all(_token0_hooks(m) for m in (last,) + token0))


def _class_pos_residual(pos, cls, bias, B):
    """[B, T, D]: the residual operand of the patch embedding written as K11 + one GEMM -- the position table pos [T, D]
    for every image, with cls [D] + its row 0 - bias in row 0 (the class-token slot, a zero row of K11's; the GEMM adds the
    bias back).  bias None: a convolution without one."""
    r = pos.detach().expand(B, -1, -1).contiguous()
    r[:, 0] = cls.detach() + pos.detach()[0] if bias is None else cls.detach() + pos.detach()[0] - bias.detach()
    return r


def _attend(qkv, heads, choice, arg=None):
    """The concatenated head outputs [B, T, D] of the fused projection's output qkv [B, T, 3 D] -- attention before the
    output projection -- on the kernel `choice` names: 'k9' (K9), 'long' (K9L: one workgroup per 256 queries of a head, no
    T x T buffer), 'causal' (K9A), 'keylen' (K9M, arg: the int32 [B] key counts or None), 'relbias' (K9B, arg: the key
    counts and the [heads, 2T-1] bias table), 'window' / 'window-aten' (Swin's shifted windows on K31 / on ATen, arg: the
    grid, window, shift, bias table and a padded token's qkv) or 'sdpa' (PyTorch's, arg: the mask or None).  The HIP kernels
    (csrc/k_attn.hip) read the projection's layout and write the proj input's."""
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    if choice == "k9":
        global _attention_calls
        _attention_calls += 1
        timed = ATTENTION_EVENTS is not None and _attention_calls % 8 == 0
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        o = core.vit_attention(qkv, heads)
        if timed:
            e1.record()
            ATTENTION_EVENTS.append((e0, e1, B, T, heads))
        return o
    if choice == "long":
        return core.vit_attention_long(qkv, heads)
    if choice == "causal":
        return core.vit_attention_causal(qkv, heads)
    if choice == "keylen":
        return core.vit_attention_keylen(qkv, heads, arg)
    if choice == "relbias":
        return core.vit_attention_relbias(qkv, heads, *arg)
    if choice == "window":                                   # K31, arg: (grid, window, shift, table, pad_qkv)
        return core.window_attention(qkv, *arg)
    if choice == "window-aten":                              # the same operands through ATen (windows K31 does not take)
        return _window_attend_aten(qkv, heads, *arg)
    q, k, v = qkv.view(B, T, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=arg)
    return o.transpose(1, 2).reshape(B, T, D)


def _attend_cls(q, kv):
    """K9C: one query row per image, q [B, D], against the keys and values of kv [B, T, 2, heads, 64] -> [B, D]."""
    return core.vit_attention_cls(q, kv[:, :, 0], kv[:, :, 1])


_LOG2E = 1.4426950408889634


def _attend_cls_folded(owner, qkv, heads, q, n):
    """_attend_cls without K and V (CLS_FOLD): q [B, D] the class token's query, n [B, T, D] = LN1(x) -> [B, D].
    u[:, h] = q_h W_k,h * log2(e)/8 and o_h = W_v,h m_h + b_v,h are `heads` GEMMs of B rows each (K = 64, then N = 64),
    K30 between them turns u and n into m.  W_k is read through a transposed copy [heads, D, 64] with the scale folded in,
    built once per weight (_folded on `owner`, the module that holds the qkv parameters)."""
    w, b = qkv
    B, T, D = n.shape
    wkt = _folded(owner, (), lambda m: (w.detach()[D:2 * D].view(heads, 64, D).transpose(1, 2) * (_LOG2E / 8.0)).contiguous(),
                  own=True)
    u = torch.empty((B, heads, D), dtype=n.dtype, device=n.device)
    for h in range(heads):
        core.linear_residual(None, q[:, 64 * h:64 * h + 64], wkt[h], None, out=u[:, h])
    m = core.cls_token_mix(u, n)
    o = torch.empty((B, D), dtype=n.dtype, device=n.device)
    for h in range(heads):
        r = slice(2 * D + 64 * h, 2 * D + 64 * h + 64)
        core.linear_residual(None, m[:, h], w[r], None if b is None else b[r], out=o[:, 64 * h:64 * h + 64])
    return o


# The operands of one transformer block on the HIP route (_block_hip): ln1 / ln2 as (weight, bias, eps), qkv / proj / fc1 /
# fc2 as (weight, bias), the head count; owner: the module whose parameters the qkv pair is (the cache of the folded tail's
# derived weight hangs on it; None: no fold).  Each block class builds it from its own parameters (its _ops()).
_BlockOps = collections.namedtuple("_BlockOps", "ln1 ln2 qkv proj fc1 fc2 heads owner", defaults=(None,))


def _ln_ops(ln):
    return ln.weight, ln.bias, ln.eps


def _lin_ops(lin):
    return lin.weight, lin.bias


def _norm(x, ln, k10=True):
    return core.layer_norm(x, *ln) if k10 else F.layer_norm(x, x.shape[-1:], *ln)                # K10, or ATen's


def _gelu(h):
    return F.gelu(h)                                                                              # erf GELU, ATen's


def _quick_gelu_(h):
    return core.quick_gelu(h, out=h)                                                              # K25, in place


def _block_hip(p, x, attn, attn_arg=None, post=False, act=_gelu, cls_only=False, k10=True):
    """One transformer block [B, T, D] -> [B, T, D] on the HIP route, from the operands p (a _BlockOps): the fused qkv
    GEMM, the attention `attn` (_attend's choice, with attn_arg), the two residual GEMMs, `act` behind fc1.
    Pre-norm (ViT, CLIP):    x1 = x + proj(attention(ln1(x))),    out = x1 + fc2(act(fc1(ln2(x1)))).
    post=True (BERT):        x1 = ln1(x + proj(attention(x))),    out = ln2(x1 + fc2(act(fc1(x1)))).
    x1 is a new tensor (the block's input is left alone); a pre-norm block's second update is in place on x1.  k10=False
    keeps ATen's LayerNorm (_Block under HIP_LAYER_NORM).
    cls_only (pre-norm; the caller has checked cls_tail_route): the class-token row of the same block, as [B, 1, D].  K and
    V need every token -- ln1 and the K|V two thirds of the qkv projection run on all rows -- everything after them is
    computed for row 0 of each image only.  The weight slices are contiguous views, x[:, 0] and ln1(x)[:, 0] go into the
    GEMMs as row-strided operands: no copies.  Where cls_fold_route agrees, the K|V projection is folded out as well
    (_attend_cls_folded): ln1 on all rows, K30 on its output, and every GEMM of the block has B rows."""
    B, T, D = x.shape
    x = x.contiguous()
    n = x if post else _norm(x, p.ln1, k10)
    w, b = p.qkv
    if cls_only and p.owner is not None and cls_fold_route(CLS_FOLD, B, T, D, p.heads, CLS_FOLD_MIN_ROWS):
        o = _attend_cls_folded(p.owner, p.qkv, p.heads, core.linear_residual(None, n[:, 0], w[:D], None if b is None else b[:D]), n)
        x = x[:, 0]
    elif cls_only:
        kv = core.linear_residual(None, n, w[D:], None if b is None else b[D:]).view(B, T, 2, p.heads, D // p.heads)
        o = _attend_cls(core.linear_residual(None, n[:, 0], w[:D], None if b is None else b[:D]), kv)
        x = x[:, 0]
    else:
        o = _attend(core.linear_residual(None, n, w, b), p.heads, attn, attn_arg).contiguous()
    x1 = core.linear_residual(x, o, *p.proj)
    if post:
        x1 = _norm(x1, p.ln1, k10)
    h = act(core.linear_residual(None, x1 if post else _norm(x1, p.ln2, k10), *p.fc1))
    if post:
        return _norm(core.linear_residual(x1, h, *p.fc2), p.ln2, k10)
    out = core.linear_residual(x1, h, *p.fc2, out=x1)
    return out.unsqueeze(1) if cls_only else out


class _Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, mask=None):
        return self.proj(self.heads_out(x, mask))

    def heads_out(self, x, mask=None):
        """The concatenated head outputs [B, T, D], i.e. attention before the output projection."""
        qkv = self.qkv(x)
        route = attention_route(x.shape[1], x.shape[2], self.heads, mask is not None, qkv.is_cuda, qkv.dtype,
                                torch.is_grad_enabled() and qkv.requires_grad)
        return _attend(qkv, self.heads, route, mask)


class _LayerScale(nn.Module):
    """DINOv2's per-channel scale of a branch in front of its residual add (Dinov2LayerScale: the parameter lambda1)."""

    def __init__(self, dim, init):
        super().__init__()
        self.lambda1 = nn.Parameter(init * torch.ones(dim))

    def forward(self, x):
        return x * self.lambda1


_BLOCK_SKIPPED = ("norm1", "attn", "norm2", "fc1", "fc2", "layer_scale1", "layer_scale2")


class _Block(nn.Module):
    """Pre-norm transformer block.  eps: the LayerNorms' (HF ViT 1e-12, DINOv2 1e-6).  layer_scale: None, or the initial
    value of the two LayerScales a DINOv2 block has, x + layer_scale1(proj(.)) and x + layer_scale2(fc2(.)); None builds
    no such module (the state dict and the arithmetic of a plain block)."""

    def __init__(self, dim, heads, mlp, eps=1e-12, layer_scale=None):
        super().__init__()
        self.norm1 = _LayerNorm(dim, eps=eps)
        self.attn = _Attention(dim, heads)
        self.norm2 = _LayerNorm(dim, eps=eps)
        self.fc1 = nn.Linear(dim, mlp)
        self.fc2 = nn.Linear(mlp, dim)
        self.scaled = layer_scale is not None
        if self.scaled:
            self.layer_scale1 = _LayerScale(dim, layer_scale)
            self.layer_scale2 = _LayerScale(dim, layer_scale)

    def forward(self, x, mask=None, cls_only=False):
        cls_only = cls_only and mask is None      # a masked call keeps the full block whatever the caller asked for
        if cls_only or (_fused_residual_ok(x) and not _hooks_on(self, _BLOCK_SKIPPED)):
            B, T, D = x.shape
            route = attention_route(T, D, self.attn.heads, mask is not None, x.is_cuda, x.dtype, False)
            return _block_hip(self._ops(), x, route, mask, cls_only=cls_only, k10=HIP_LAYER_NORM and D % 4 == 0 and D <= 2048)
        # ATen, also for a block with a hook inside (or under a global one): every submodule through __call__, so that
        # the hook fires, once, with the module's own output
        if self.scaled:
            x = x + self.layer_scale1(self.attn(self.norm1(x), mask))
            return x + self.layer_scale2(self.fc2(F.gelu(self.fc1(self.norm2(x)))))
        x = x + self.attn(self.norm1(x), mask)
        return x + self.fc2(F.gelu(self.fc1(self.norm2(x))))

    def _ops(self):
        wp, bp, w2, b2 = self._residual_weights()
        return _BlockOps(_ln_ops(self.norm1), _ln_ops(self.norm2), _lin_ops(self.attn.qkv), (wp, bp), _lin_ops(self.fc1),
                         (w2, b2), self.attn.heads, self.attn)

    def _residual_weights(self):
        """(proj weight, proj bias, fc2 weight, fc2 bias) of the two fused residual GEMMs.  With LayerScale,
        lambda * (W h + b) = (lambda (.) W) h + lambda (.) b: the scale is folded into the rows of the weight and into the
        bias once (_folded: nothing is registered, the cache follows the parameters), so the GEMM's epilogue still does
        the residual add and no pass over the activations is added."""
        a = self.attn
        if not self.scaled:
            return a.proj.weight, a.proj.bias, self.fc2.weight, self.fc2.bias

        def build(m):
            l1, l2 = m.layer_scale1.lambda1.detach(), m.layer_scale2.lambda1.detach()
            return ((l1[:, None] * m.attn.proj.weight.detach()).contiguous(), (l1 * m.attn.proj.bias.detach()).contiguous(),
                    (l2[:, None] * m.fc2.weight.detach()).contiguous(), (l2 * m.fc2.bias.detach()).contiguous())
        return _folded(self, ("layer_scale1", "layer_scale2", "attn", "fc2"), build)


class _Encoder(nn.Module):
    def __init__(self, depth, dim, heads, mlp, list_name, eps=1e-12, layer_scale=None):
        super().__init__()
        setattr(self, list_name, nn.ModuleList([_Block(dim, heads, mlp, eps, layer_scale) for _ in range(depth)]))
        self._list_name = list_name

    def forward(self, x, mask=None, cls_only=False):
        """cls_only (ViTTower.forward has checked cls_tail_route): the last block is called, through __call__ so that its
        hooks fire, for its class-token row alone and the result is [B, 1, D]."""
        blocks = getattr(self, self._list_name)
        for i, blk in enumerate(blocks):
            x = blk(x, mask, cls_only=True) if cls_only and i == len(blocks) - 1 else blk(x, mask)
        return x


def image_hw(image_size):
    """(H, W) of an image_size that is an int (square) or an (H, W) pair."""
    if isinstance(image_size, (tuple, list)):
        h, w = image_size
        return int(h), int(w)
    return int(image_size), int(image_size)


def _parse_hw(text):
    """'<S>' -> S (square, as before), '<H>x<W>' -> (H, W); None if `text` is neither."""
    if text.isdigit():
        return int(text)
    h, sep, w = text.partition("x")
    if sep and h.isdigit() and w.isdigit():
        return int(h), int(w)
    return None


class ViTTower(nn.Module):
    """[B,3,H,W] -> token sequence [B, 1+(H/16)*(W/16), 768]; hook points encoder.<list_name>[i].  image_size is an int
    (square) or (H, W): (H/16)*(W/16) + 1 position embeddings, e.g. 5 416 for Mammo-CLIP's 1520 x 912.  eps and
    layer_scale: the blocks' (_Block) and the final LayerNorm's."""

    def __init__(self, image_size=224, patch=16, dim=768, depth=12, heads=12, mlp=3072, list_name="layer", eps=1e-12,
                 layer_scale=None):
        super().__init__()
        self.out_dim = dim
        h, w = image_hw(image_size)
        self._build_embedding(dim, patch, (h // patch) * (w // patch))
        self.encoder = _Encoder(depth, dim, heads, mlp, list_name, eps, layer_scale)
        self.layernorm = _LayerNorm(dim, eps=eps)

    def _build_embedding(self, dim, patch, n):
        """The embedding parameters, as this tower's own patch_embed / cls_token / pos_embed (HFTower keeps them in an
        `embeddings` submodule under transformers' names)."""
        self.patch_embed = nn.Conv2d(3, dim, patch, patch)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n + 1, dim))

    def pos_table(self, H, W):
        """The [1, T, dim] position table for an H x W image: pos_embed as it is (HFTower: interpolated to the image's
        patch grid when `interpolate` is set)."""
        return self.pos_embed

    def forward(self, x, cls_only=False):
        """cls_only=True: the caller reads [:, 0] of the result and nothing else.  Where cls_tail_route allows, the last
        block and the final LayerNorm then run on the class-token row alone and the result is [B, 1, D]; otherwise (and
        for every plain tower(x)) the full [B, T, D], computed exactly as before."""
        x = self.embed(x)
        if cls_only and self._cls_tail_ok(x):
            return self.layernorm(self.encoder(x, cls_only=True))
        return self.layernorm(self.encoder(x))

    def _cls_tail_ok(self, x):
        """cls_tail_route for the embedded tokens x [B, T, D] and the hooks this tower carries right now."""
        enc = self.encoder
        return _cls_tail_ok(x, getattr(enc, enc._list_name), enc, clear=(self.layernorm,), token0=(self,))

    def embed(self, x):
        """Patch embedding + class token + position embedding -> [B, 1 + n, dim]."""
        P = self.patch_embed.kernel_size[0]
        if (_fused_residual_ok(x) and x.is_contiguous() and x.dim() == 4 and self.patch_embed.bias is not None
                and embed_gate(P, x.shape[2], x.shape[3], self.pos_table(x.shape[2], x.shape[3]).shape[1])):
            # the convolution as ONE GEMM that writes the token sequence directly (K11 + libmcd_blaslt.so): rows of
            # patch pixels (a zero row in every image's class-token slot) times the conv weight, plus the bias, plus a
            # residual operand that holds the position embedding (and cls + pos[0] - bias in the class-token rows).
            # No MIOpen call (its choice of algorithm varied between 0.5 and 1.2 ms from box to box), no cat, no add.
            return core.linear_residual(self._embed_residual(x.shape[0], x.shape[2], x.shape[3]), core.patchify(x, P),
                                        self.patch_embed.weight.view(self.patch_embed.out_channels, -1), self.patch_embed.bias)
        H, W = x.shape[2:]
        x = self.patch_embed(x).flatten(2).transpose(1, 2)
        return torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1) + self.pos_table(H, W)

    def _embed_residual(self, B, H, W):
        """[B, 1 + n, dim]: the position table of an H x W image (pos_table), with cls_token + its row 0 - bias in row 0
        (the GEMM adds the bias back)."""
        return _folded(self, ("pos_embed", "cls_token", "patch_embed"), lambda m: _class_pos_residual(
            m.pos_table(H, W)[0], m.cls_token[0, 0], m.patch_embed.bias, B), extra=(B, H, W))


# ------------------------------------------------------------------------------------------------------
# EfficientNet-B5 tower (parameter names follow the public EfficientNet-PyTorch layout so a local
# Mammo-CLIP checkpoint's image_encoder.* keys line up: _conv_stem, _bn0, _blocks[i]._expand_conv ...)
# ------------------------------------------------------------------------------------------------------
class _SameConv(nn.Conv2d):
    """TensorFlow 'SAME' padding (asymmetric for stride 2), as the b5 'tf_' weights expect."""

    def forward(self, x):
        (_, pt, pb), (_, pl, pr) = (core.same_pad(n, k, s) for n, k, s in zip(x.shape[-2:], self.kernel_size, self.stride))
        if pt or pb or pl or pr:
            x = F.pad(x, [pl, pr, pt, pb])
        return F.conv2d(x, self.weight, self.bias, self.stride, 0, self.dilation, self.groups)


def _bn_affine64(bn):
    """(scale, shift) in float64 of an eval-mode batch norm as y = x * scale + shift: g / sqrt(var + eps) and
    beta - mean * scale."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def bn_scale_shift(bn):
    """(scale, shift) of an eval-mode batch norm as y = x * scale + shift, computed in float64, returned in its dtype."""
    scale, shift = _bn_affine64(bn)
    return scale.to(bn.weight.dtype).contiguous(), shift.to(bn.weight.dtype).contiguous()


def fold_bn(weight, bn):
    """(W', b'): the eval-mode batch norm `bn` folded into the bias-free convolution weight [Cout, ...] in front of it,
    W' = W * scale per output channel, b' = shift (_bn_affine64).  Computed in float64, returned in the weight's dtype."""
    scale, shift = _bn_affine64(bn)
    w = weight.detach().double() * scale.view(-1, *([1] * (weight.dim() - 1)))
    return w.to(weight.dtype), shift.to(weight.dtype)


def igemm_weight(w):
    """K18's weight layout: [Cout, Cin, kh, kw] -> [Cout, kh*kw*Cin], tap-major then channel."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


_FOLD_LAYOUTS = {"gemm": lambda w: w.flatten(1),                     # [Cout, Cin] of a 1x1: a GEMM's weight
                 "igemm": igemm_weight,                              # K18
                 "tap": lambda w: w.permute(1, 2, 3, 0)}             # [Cin, kh, kw, Cout]: the image stems (K12, K19)


def _fold_conv(conv, bn, layout):
    """(w, b) of the bias-free convolution `conv` with the batch norm `bn` behind it folded in (fold_bn), the weight in
    the layout its kernel reads ("gemm", "igemm" or "tap"), both contiguous."""
    w, b = fold_bn(conv.weight, bn)
    return _FOLD_LAYOUTS[layout](w).contiguous(), b.contiguous()


def _folded(module, names, build, own=False, extra=()):
    """build(module) -> the tensors derived from the module's weights (folded, relaid), computed once and cached in the
    module's __dict__ (no parameter or buffer is registered: state_dict() and the module tree stay as they are).  The
    cache is keyed on the version counter and the storage of every source tensor -- the named parameters, and all tensors
    of the named submodules, nested ones included (own=True: of the module itself) -- on the device and dtype, and on
    `extra` (whatever else build depends on)."""
    srcs = []
    for m in [module] if own else [getattr(module, n, None) for n in names]:
        if isinstance(m, torch.Tensor):
            srcs.append(m)
        elif m is not None:
            srcs += list(m.parameters()) + list(m.buffers())
    key = tuple((t._version, t.data_ptr()) for t in srcs) + (srcs[0].device, srcs[0].dtype) + tuple(extra)
    cache = module.__dict__.setdefault("_fold_cache", {})
    if cache.get("key") != key:
        with torch.no_grad():
            cache["val"] = build(module)
        cache["key"] = key
    return cache["val"]


_MBCONV_SKIPPED = ("_expand_conv", "_bn0", "_depthwise_conv", "_bn1", "_se_reduce", "_se_expand", "_project_conv", "_bn2")
_TOWER_SKIPPED = ("_conv_stem", "_bn0", "_conv_head", "_bn1")


def _hooked(m):
    """A forward (pre-)hook on the module m or on any module inside it."""
    return bool(m._forward_hooks or m._forward_pre_hooks
                or (m._modules and any(_hooked(c) for c in m._modules.values() if c is not None)))


def _hooks_on(module, names):
    """A global module hook, or a forward (pre-)hook on one of the named submodules or on a module inside one (a
    ResNet downsample's convolution, say): the HIP route calls none of them."""
    if _nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks:
        return True
    return any(m is not None and _hooked(m) for m in map(module._modules.get, names))


def mbconv_route(module, x):
    """'hip' when the B5 tower (an EfficientNetB5Tower with its NCHW-contiguous input image) or one of its blocks (an
    _MBConv with a channels_last-contiguous input) can take the HIP route: HIP_MBCONV on, a CUDA fp32 tensor, inference
    (no autograd, eval mode), libmcd_blaslt.so loaded, channel counts that are multiples of 4 (the SE width may be
    anything), one image's tensors under 2^31 bytes, and no hook on a submodule the route does not call (--target_layers
    may name any module path: a hook on _blocks[5]._depthwise_conv must fire, so that block takes ATen).  'aten'
    otherwise."""
    if not _tower_gate(HIP_MBCONV, module, x):
        return "aten"
    B, C, H, W = x.shape
    if isinstance(module, _MBConv):
        ok = (C == module.cin and not (module.cin % 4 or module.mid % 4 or module.cout % 4) and module.k in (3, 5)
              and module.s in (1, 2) and core.channels_last(x) and not x.data_ptr() % 16
              and _under_2g(module.mid * H * W, module.cin * H * W))
        names = _MBCONV_SKIPPED
    elif isinstance(module, EfficientNetB5Tower):
        stem, head = module._conv_stem, module._conv_head
        sizes = [(H, W)]
        for _ in range(5):                           # the five stride-2 stages (the output size does not depend on k)
            sizes.append(tuple(core.same_pad(n, 3, 2)[0] for n in sizes[-1]))
        (hs, ws), (hh, wh) = sizes[1], sizes[5]      # the stem's output and the head's input
        ok = (C == stem.in_channels and C <= 4 and not stem.out_channels % 4 and stem.kernel_size == (3, 3)
              and stem.stride == (2, 2) and not (head.in_channels % 4 or head.out_channels % 4) and x.is_contiguous()
              and _under_2g(stem.out_channels * hs * ws, head.out_channels * hh * wh))
        names = _TOWER_SKIPPED
    else:
        return "aten"
    return "hip" if ok and not _hooks_on(module, names) else "aten"


class _MBConv(nn.Module):
    def __init__(self, cin, cout, k, s, expand, se_ratio=0.25):
        super().__init__()
        mid = cin * expand
        self.cin, self.mid, self.cout, self.k, self.s = cin, mid, cout, k, s
        self.expand = expand != 1
        if self.expand:
            self._expand_conv = _SameConv(cin, mid, 1, bias=False)
            self._bn0 = nn.BatchNorm2d(mid, momentum=0.01, eps=1e-3)
        self._depthwise_conv = _SameConv(mid, mid, k, s, groups=mid, bias=False)
        self._bn1 = nn.BatchNorm2d(mid, momentum=0.01, eps=1e-3)
        sq = max(1, int(cin * se_ratio))
        self._se_reduce = _SameConv(mid, sq, 1)
        self._se_expand = _SameConv(sq, mid, 1)
        self._project_conv = _SameConv(mid, cout, 1, bias=False)
        self._bn2 = nn.BatchNorm2d(cout, momentum=0.01, eps=1e-3)
        self.skip = s == 1 and cin == cout

    def forward(self, x):
        if mbconv_route(self, x) == "hip":
            return self._forward_hip(x)
        y = x
        if self.expand:
            y = F.silu(self._bn0(self._expand_conv(y)))
        y = F.silu(self._bn1(self._depthwise_conv(y)))
        se = self._se_expand(F.silu(self._se_reduce(y.mean(dim=[2, 3], keepdim=True))))
        y = self._bn2(self._project_conv(torch.sigmoid(se) * y))
        return x + y if self.skip else y

    def _forward_hip(self, x):
        """The block on channels-last activations: expand GEMM (raw, folded BN0 as its bias), K13 (SiLU of the expand
        output on the way in, depthwise + folded BN1 + SiLU, SE partial sums), K14 (SE gate), K15 (scale, in place),
        project GEMM (folded BN2 as its bias, the skip as its residual operand: a new tensor, x is left alone).
        Returns [B, C, H, W] in channels_last memory, the reference's logical shape."""
        f = _folded(self, _MBCONV_SKIPPED, _MBConv._fold)
        xn = x.permute(0, 2, 3, 1)                                   # [B, H, W, cin], contiguous
        h = core.linear_residual(None, xn, f["w0"], f["b0"]) if self.expand else xn
        d, psum = core.dwconv_bn_silu(h, f["wd"], f["bd"], self.k, self.s, self.expand)
        gate = core.se_gate(psum, d.shape[1] * d.shape[2], f["wr"], f["br"], f["we"], f["be"])
        core.channel_scale_(d, gate)
        y = core.linear_residual(xn if self.skip else None, d, f["wp"], f["bp"])
        return y.permute(0, 3, 1, 2)

    def _fold(self):
        f = {}
        if self.expand:
            f["w0"], f["b0"] = _fold_conv(self._expand_conv, self._bn0, "gemm")
        wd, f["bd"] = fold_bn(self._depthwise_conv.weight, self._bn1)
        f["wd"] = wd.view(self.mid, self.k * self.k).t().contiguous()          # tap-major [k*k, mid]
        sq = self._se_reduce.out_channels
        f["wr"] = self._se_reduce.weight.detach().reshape(sq, self.mid).contiguous()
        f["br"] = self._se_reduce.bias.detach().contiguous()
        f["we"] = self._se_expand.weight.detach().reshape(self.mid, sq).t().contiguous()       # transposed: [sq, mid]
        f["be"] = self._se_expand.bias.detach().contiguous()
        f["wp"], f["bp"] = _fold_conv(self._project_conv, self._bn2, "gemm")
        return f


def _round_filters(f, width, divisor=8):
    f *= width
    nf = max(divisor, int(f + divisor / 2) // divisor * divisor)
    if nf < 0.9 * f:
        nf += divisor
    return int(nf)


class EfficientNetB5Tower(nn.Module):
    """EfficientNet-B5 (width 1.6, depth 2.2): 39 MBConv blocks, output [B, 2048] pooled features."""
    # B0 stage table: repeats, kernel, stride, expand, out channels
    STAGES = [(1, 3, 1, 1, 16), (2, 3, 2, 6, 24), (2, 5, 2, 6, 40), (3, 3, 2, 6, 80), (3, 5, 1, 6, 112),
              (4, 5, 2, 6, 192), (1, 3, 1, 6, 320)]

    def __init__(self, width=1.6, depth=2.2, num_classes=1):
        super().__init__()
        stem = _round_filters(32, width)
        self._conv_stem = _SameConv(3, stem, 3, 2, bias=False)
        self._bn0 = nn.BatchNorm2d(stem, momentum=0.01, eps=1e-3)
        blocks, cin = [], stem
        for r, k, s, e, o in self.STAGES:
            cout = _round_filters(o, width)
            for i in range(int(math.ceil(depth * r))):
                blocks.append(_MBConv(cin, cout, k, s if i == 0 else 1, e))
                cin = cout
        self._blocks = nn.ModuleList(blocks)
        self.out_dim = _round_filters(1280, width)
        self._conv_head = _SameConv(cin, self.out_dim, 1, bias=False)
        self._bn1 = nn.BatchNorm2d(self.out_dim, momentum=0.01, eps=1e-3)
        self._fc = nn.Linear(self.out_dim, num_classes)

    def forward(self, x):
        if mbconv_route(self, x) == "hip":
            return self._forward_hip(x)
        x = F.silu(self._bn0(self._conv_stem(x)))
        for b in self._blocks:
            x = b(x)
        x = F.silu(self._bn1(self._conv_head(x)))
        return x.mean(dim=[2, 3])

    def _forward_hip(self, x):
        """Stem by K12 (NCHW image -> channels-last), the blocks called as modules (hooks on _blocks[i] fire; each block
        picks its own route), the head as one GEMM (folded BN1 as its bias) and K0n's mean of SiLU."""
        f = _folded(self, _TOWER_SKIPPED, EfficientNetB5Tower._fold)
        x = core.conv_stem_nhwc(x, f["ws"], f["bs"]).permute(0, 3, 1, 2)
        for b in self._blocks:
            # a block that took ATen (a hook inside it, say) may hand on NCHW memory: back to channels-last for the next
            x = b(x).contiguous(memory_format=torch.channels_last)
        xn = x.permute(0, 2, 3, 1)
        return core.silu_avg_pool_nhwc(core.linear_residual(None, xn, f["wh"], f["bh"]))

    def _fold(self):
        f = {}
        f["ws"], f["bs"] = _fold_conv(self._conv_stem, self._bn0, "tap")
        f["wh"], f["bh"] = _fold_conv(self._conv_head, self._bn1, "gemm")
        return f


EfficientNetTower = EfficientNetB5Tower       # the class at any compound scaling (width, depth): B5 is its default only


# ------------------------------------------------------------------------------------------------------
# text tower (BERT-base shaped) + offline tokenizer
# ------------------------------------------------------------------------------------------------------
class HashTokenizer:
    """Deterministic offline stand-in for BertTokenizerFast('emilyalsentzer/Bio_ClinicalBERT') (whose vocab
    is not in the container): lower-cased whitespace/punctuation split, ids = 1000 + crc32(word) % 27000,
    [CLS]=101 ... [SEP]=102, padding 0.  Returns the same dict the reference's tokenize() returns."""
    vocab_size = 28996

    def __call__(self, texts, max_length=256, padding=True, truncation=True, return_tensors="pt"):
        rows = []
        for t in texts:
            words = "".join(ch if ch.isalnum() else " " for ch in t.lower()).split()
            ids = [101] + [1000 + zlib.crc32(w.encode()) % 27000 for w in words]
            ids = ids[:max_length - 1] + [102]
            rows.append(ids)
        L = max(len(r) for r in rows)
        input_ids = torch.zeros(len(rows), L, dtype=torch.long)
        mask = torch.zeros(len(rows), L, dtype=torch.long)
        for i, r in enumerate(rows):
            input_ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return {"input_ids": input_ids, "attention_mask": mask, "token_type_ids": torch.zeros_like(input_ids)}


class TextTower(nn.Module):
    def __init__(self, vocab=28996, dim=768, depth=12, heads=12, mlp=3072, max_pos=512):
        super().__init__()
        self.out_dim = dim
        self.word = nn.Embedding(vocab, dim)
        self.pos = nn.Embedding(max_pos, dim)
        self.norm = nn.LayerNorm(dim, eps=1e-12)
        self.encoder = _Encoder(depth, dim, heads, mlp, "layer")

    def forward(self, tokens):
        ids, mask = tokens["input_ids"], tokens["attention_mask"]
        x = self.norm(self.word(ids) + self.pos(torch.arange(ids.shape[1], device=ids.device))[None])
        attn = mask[:, None, None, :].bool()
        return self.encoder(x, attn)


# ------------------------------------------------------------------------------------------------------
# the reference's own text tower: transformers.BertModel (Bio_ClinicalBERT) restated, and its WordPiece tokenizer
#   model/modules/text_encoder.py:37,48 (BertModel(config), output["last_hidden_state"]); model/clip.py:17, :60-79
# Module tree and state-dict keys are those of transformers 4.41.1, the reference's pin: a Mammo-CLIP checkpoint's
# text_encoder.text_encoder.* keys load unchanged.  Post-norm blocks, erf GELU, eps from the configuration (1e-12).
# ------------------------------------------------------------------------------------------------------
def prefix_mask_lengths(mask):
    """The key count of every row of a PREFIX attention mask [B, T] -- ones (non-zeros), then zeros, at least one 1 per
    row: what padding to the longest sequence produces -- as an int32 [B] tensor on the mask's device, or None for any
    other mask (a hole, a leading zero, an all-zero row): only a prefix mask is a key count, which is what K9M takes.
    One device-to-host sync for a mask on the GPU."""
    if mask.dim() != 2 or mask.shape[1] < 1:
        return None
    m = mask != 0
    lens = m.sum(dim=1)
    prefix = torch.arange(mask.shape[1], device=mask.device)[None, :] < lens[:, None]
    if not bool(((m == prefix).all() & (lens >= 1).all()).item()):
        return None
    return lens.to(torch.int32)


def text_route(tower, ids):
    """'hip' when a BertTextTower call on the token ids `ids` may leave ATen: HIP_TEXT on, the weights fp32 on the GPU
    with the ids beside them, no autograd (_hip_eligible), eval mode, hidden = 64 * heads (K9M's head width), at most
    core.VIT_ATTENTION_MAX_T tokens and no more than the position table has rows, a width K10 / K24 take, and the
    fused-residual library loaded (every projection is its GEMM).  Otherwise 'aten'.  The mask and the hooks are looked
    at by the caller: a mask that is not a prefix mask takes SDPA, a layer with a hook inside takes its ATen modules."""
    w = tower.embeddings.word_embeddings.weight
    B, T = ids.shape
    D = w.shape[1]
    ok = (HIP_TEXT and _hip_eligible(w.is_cuda and ids.is_cuda, w.dtype, torch.is_grad_enabled()) and not tower.training
          and D == 64 * tower.heads and 1 <= T <= min(core.VIT_ATTENTION_MAX_T, tower.embeddings.position_embeddings.num_embeddings)
          and D % 4 == 0 and D <= 2048 and 1 <= B <= MAX_BATCH and FUSED_RESIDUAL and core.linear_residual_available())
    return "hip" if ok else "aten"


_BERT_EMB_SKIPPED = ("word_embeddings", "position_embeddings", "token_type_embeddings", "LayerNorm")
_BERT_LAYER_SKIPPED = ("attention", "intermediate", "output")


class _BertEmbeddings(nn.Module):
    def __init__(self, vocab, hidden, max_pos, n_type, eps):
        super().__init__()
        self.word_embeddings = nn.Embedding(vocab, hidden)
        self.position_embeddings = nn.Embedding(max_pos, hidden)
        self.token_type_embeddings = nn.Embedding(n_type, hidden)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)

    def forward(self, ids, type_ids=None, hip=False):
        if hip and not _hooks_on(self, _BERT_EMB_SKIPPED):       # K24: the three gathers, both adds and the LayerNorm
            n = self.LayerNorm
            return core.text_embed_ln(ids, type_ids, self.word_embeddings.weight, self.position_embeddings.weight,
                                      self.token_type_embeddings.weight, n.weight, n.bias, n.eps)
        if type_ids is None:
            type_ids = torch.zeros_like(ids)
        pos = self.position_embeddings(torch.arange(ids.shape[1], device=ids.device))
        return self.LayerNorm((self.word_embeddings(ids) + self.token_type_embeddings(type_ids)) + pos[None])   # HF's order


class _BertSelfAttention(nn.Module):
    def __init__(self, hidden, heads):
        super().__init__()
        self.heads = heads
        self.query = nn.Linear(hidden, hidden)
        self.key = nn.Linear(hidden, hidden)
        self.value = nn.Linear(hidden, hidden)

    def forward(self, x, mask=None):
        B, T, D = x.shape
        q, k, v = (m(x).view(B, T, self.heads, D // self.heads).transpose(1, 2) for m in (self.query, self.key, self.value))
        return F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, T, D)

    def fused_qkv(self):
        """(weight [3 D, D], bias [3 D]) of query | key | value as ONE projection -- the [B, T, 3, heads, 64] operand K9M
        reads -- concatenated once (_folded: nothing is registered, the cache follows the three modules' parameters)."""
        return _folded(self, ("query", "key", "value"),
                       lambda m: (torch.cat([m.query.weight, m.key.weight, m.value.weight]).contiguous(),
                                  torch.cat([m.query.bias, m.key.bias, m.value.bias]).contiguous()))


class _BertAddNorm(nn.Module):
    """BertSelfOutput / BertOutput: LayerNorm(dense(h) + residual) (dropout is the identity at inference)."""

    def __init__(self, in_dim, hidden, eps):
        super().__init__()
        self.dense = nn.Linear(in_dim, hidden)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)

    def forward(self, h, residual):
        return self.LayerNorm(self.dense(h) + residual)


class _BertAttention(nn.Module):
    def __init__(self, hidden, heads, eps):
        super().__init__()
        setattr(self, "self", _BertSelfAttention(hidden, heads))
        self.output = _BertAddNorm(hidden, hidden, eps)

    def forward(self, x, mask=None):
        return self.output(getattr(self, "self")(x, mask), x)


class _BertIntermediate(nn.Module):
    def __init__(self, hidden, mlp):
        super().__init__()
        self.dense = nn.Linear(hidden, mlp)

    def forward(self, x):
        return F.gelu(self.dense(x))


class _BertLayer(nn.Module):
    """BertLayer, post-norm: x1 = LN(x + proj(attention(x))), out = LN(x1 + fc2(gelu(fc1(x1))))."""

    def __init__(self, hidden, heads, mlp, eps):
        super().__init__()
        self.attention = _BertAttention(hidden, heads, eps)
        self.intermediate = _BertIntermediate(hidden, mlp)
        self.output = _BertAddNorm(mlp, hidden, eps)

    def forward(self, x, mask=None, lens=None, hip=False):
        """mask: None or the bool [B, 1, 1, T] key mask for SDPA; hip (the tower has checked text_route and the mask):
        the HIP route with lens (int32 [B] key counts, None = all T) -- unless a hook sits inside this layer."""
        if hip and not _hooks_on(self, _BERT_LAYER_SKIPPED):
            return _block_hip(self._ops(), x, "keylen", lens, post=True)                                   # K9M
        x1 = self.attention(x, mask)
        return self.output(self.intermediate(x1), x1)

    def _ops(self):
        s, so, o = getattr(self.attention, "self"), self.attention.output, self.output
        return _BlockOps(_ln_ops(so.LayerNorm), _ln_ops(o.LayerNorm), s.fused_qkv(), _lin_ops(so.dense),
                         _lin_ops(self.intermediate.dense), _lin_ops(o.dense), s.heads)


class _BertEncoder(nn.Module):
    def __init__(self, depth, hidden, heads, mlp, eps):
        super().__init__()
        self.layer = nn.ModuleList([_BertLayer(hidden, heads, mlp, eps) for _ in range(depth)])

    def forward(self, x, mask=None, lens=None, hip=False):
        for layer in self.layer:
            x = layer(x, mask, lens, hip)
        return x


class BertTextTower(nn.Module):
    """transformers.BertModel without its pooler (nothing reads pooler_output): forward(tokens) -> last_hidden_state
    [B, T, hidden] for the tokenizer's dict (input_ids, attention_mask, token_type_ids; the last two optional).
    heads = hidden / 64 (BERT's head width at every size the reference uses, and K9M's)."""

    def __init__(self, vocab=28996, hidden=768, depth=12, mlp=3072, max_pos=512, n_type=2, eps=1e-12, heads=None):
        super().__init__()
        self.out_dim = hidden
        self.heads = hidden // 64 if heads is None else heads
        if hidden % self.heads:
            raise ValueError("BertTextTower: hidden %d is not a multiple of %d heads" % (hidden, self.heads))
        self.embeddings = _BertEmbeddings(vocab, hidden, max_pos, n_type, eps)
        self.encoder = _BertEncoder(depth, hidden, self.heads, mlp, eps)

    def forward(self, tokens):
        ids, mask, type_ids = tokens["input_ids"], tokens.get("attention_mask"), tokens.get("token_type_ids")
        hip = text_route(self, ids) == "hip"
        lens = None
        if hip and mask is not None:
            lens = prefix_mask_lengths(mask)          # the one sync of the text path
            layers_hip = lens is not None             # any other mask: SDPA
        else:
            layers_hip = hip
        x = self.embeddings(ids, type_ids, hip)
        attn = None if mask is None else mask[:, None, None, :].bool()
        return self.encoder(x, attn, lens, layers_hip)


def bert_config_from_state_dict(sd, prefix="text_encoder.text_encoder."):
    """BertTextTower's constructor arguments read from the shapes of a checkpoint's tensors under `prefix`."""
    def shape(name):
        key = prefix + name
        if key not in sd:
            raise RuntimeError("the checkpoint has text keys under %r but lacks %r" % (prefix, key))
        return tuple(sd[key].shape)
    vocab, hidden = shape("embeddings.word_embeddings.weight")
    layer = prefix + "encoder.layer."
    depth = 1 + max([int(k[len(layer):].split(".")[0]) for k in sd if k.startswith(layer)], default=-1)
    if depth < 1:
        raise RuntimeError("the checkpoint has no %s* keys" % layer)
    return dict(vocab=vocab, hidden=hidden, depth=depth, mlp=shape("encoder.layer.0.intermediate.dense.weight")[0],
                max_pos=shape("embeddings.position_embeddings.weight")[0],
                n_type=shape("embeddings.token_type_embeddings.weight")[0])


class HFTextEncoder(nn.Module):
    """The reference's HuggingfaceTextEncoder (model/modules/text_encoder.py:5-49): holds the tower as .text_encoder, so
    that inside BreastClip its keys are text_encoder.text_encoder.*, and returns last_hidden_state."""

    def __init__(self, **config):
        super().__init__()
        self.text_encoder = BertTextTower(**config)
        self.out_dim = self.text_encoder.out_dim

    def forward(self, tokens):
        return self.text_encoder(tokens)


def _is_cjk(cp):
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


def _is_punct(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:     # all of ASCII's, `$` and `^` included
        return True
    return unicodedata.category(ch).startswith("P")


BERT_SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")       # padding, unknown, first, last
MPNET_SPECIALS = ("<pad>", "<unk>", "<s>", "</s>")


class WordPieceTokenizer:
    """BertTokenizerFast restated in pure Python (no transformers import): what the reference's tokenize() runs
    (model/clip.py:81-101 on AutoTokenizer('emilyalsentzer/Bio_ClinicalBERT')), from a local vocab.txt.

      1. clean the text: drop NUL, U+FFFD and control characters, every whitespace character becomes a space;
      2. spaces around CJK characters;
      3. with do_lower_case: NFD, drop the combining marks (Mn), lower-case;
      4. split on whitespace, then every punctuation character is a word of its own;
      5. greedy longest-match WordPiece, continuation pieces prefixed ##; a word with a piece the vocabulary lacks, or
         longer than 100 characters, is [UNK];
      6. [CLS] ids [SEP], truncated to max_length so that [SEP] survives, padded with [PAD] to the longest sequence.
    Returns {input_ids, token_type_ids, attention_mask}, int64 [B, L]: the dict the reference's tokenize() returns.

    do_lower_case=True is BertTokenizerFast's own default, and by our reading of its hub repository -- which ships no
    tokenizer configuration -- it is what the reference gets for Bio_ClinicalBERT, a cased vocabulary notwithstanding.
    That reading cannot be checked offline.  Not restated: special-token strings such as '[SEP]' inside the text (the
    fast tokenizer maps them to the special ids; here they are split like any other text).

    specials names the padding, unknown, first and last token in that order: BERT's by default, MPNET_SPECIALS for the
    lower-cased WordPiece vocabulary of MPNet (MPNetTokenizer: <s> ids </s>, padded with <pad>), the same steps otherwise."""

    def __init__(self, vocab_file, do_lower_case=True, max_chars_per_word=100, specials=BERT_SPECIALS):
        with open(vocab_file, encoding="utf-8") as f:
            tokens = [line.rstrip("\n") for line in f]
        while tokens and tokens[-1] == "":
            tokens.pop()
        self.vocab = {}
        for i, t in enumerate(tokens):
            self.vocab[t] = i                     # (a repeated token keeps its last id, as a dict built in file order does)
        self.vocab_size = len(tokens)
        self.do_lower_case = do_lower_case
        self.max_chars = max_chars_per_word
        missing = [t for t in specials if t not in self.vocab]
        if missing:
            raise ValueError("%s lacks the special tokens %s" % (vocab_file, missing))
        self.pad_id, self.unk_id, self.cls_id, self.sep_id = (self.vocab[t] for t in specials)

    def words(self, text):
        out = []
        for ch in text:
            cp, cat = ord(ch), unicodedata.category(ch)
            if ch in " \t\n\r":
                out.append(" ")
            elif cp == 0 or cp == 0xFFFD or cat.startswith("C"):
                continue
            elif cat == "Zs" or ch.isspace():
                out.append(" ")
            elif _is_cjk(cp):
                out += [" ", ch, " "]
            else:
                out.append(ch)
        text = "".join(out)
        if self.do_lower_case:
            text = "".join(c for c in unicodedata.normalize("NFD", text) if unicodedata.category(c) != "Mn").lower()
        words = []
        for w in text.split():
            cur = ""
            for ch in w:
                if _is_punct(ch):
                    if cur:
                        words.append(cur)
                    words.append(ch)
                    cur = ""
                else:
                    cur += ch
            if cur:
                words.append(cur)
        return words

    def wordpiece(self, word):
        if len(word) > self.max_chars:
            return [self.unk_id]
        ids, start = [], 0
        while start < len(word):
            end = len(word)
            while end > start:
                piece = ("##" if start else "") + word[start:end]
                if piece in self.vocab:
                    break
                end -= 1
            if end == start:
                return [self.unk_id]
            ids.append(self.vocab[piece])
            start = end
        return ids

    def encode(self, text, max_length=None, truncation=True):
        ids = [i for w in self.words(text) for i in self.wordpiece(w)]
        if truncation and max_length is not None:
            ids = ids[:max(max_length - 2, 0)]
        return [self.cls_id] + ids + [self.sep_id]

    def __call__(self, texts, max_length=256, padding=True, truncation=True, return_tensors="pt"):
        if isinstance(texts, str):
            texts = [texts]
        rows = [self.encode(t, max_length, truncation) for t in texts]
        L = max(len(r) for r in rows) if padding else None
        if L is None and len(set(len(r) for r in rows)) > 1:
            raise ValueError("WordPieceTokenizer: sequences of different lengths need padding=True")
        L = len(rows[0]) if L is None else L
        input_ids = torch.full((len(rows), L), self.pad_id, dtype=torch.long)
        mask = torch.zeros(len(rows), L, dtype=torch.long)
        for i, r in enumerate(rows):
            input_ids[i, :len(r)] = torch.tensor(r, dtype=torch.long)
            mask[i, :len(r)] = 1
        return {"input_ids": input_ids, "token_type_ids": torch.zeros_like(input_ids), "attention_mask": mask}


TOKENIZER_VOCABS = {}


def register_tokenizer(name, vocab_path, do_lower_case=True):
    """Where a text tower's vocabulary lives (like register_dataset for probe sets): name 'bert' or 'mpnet' (the sentence
    encoder's lower-cased WordPiece vocabulary, MCD_MPNET_VOCAB), a LOCAL vocab.txt, or
    name 'clip', a LOCAL BPE merges file in bpe_simple_vocab_16e6.txt format, plain or gzipped (do_lower_case does not
    apply: CLIP's tokenizer always lower-cases).  The environment variables MCD_BERT_VOCAB=/path/vocab.txt and
    MCD_CLIP_BPE=/path/bpe_simple_vocab_16e6.txt.gz do the same for a process that registers nothing.  A 'clip' file is
    read here, once: one that is no merges file is refused at registration."""
    if name not in ("bert", "clip", "mpnet"):
        raise ValueError("register_tokenizer: %r is not a tokenizer of this package ('bert', 'clip', 'mpnet')" % (name,))
    if name == "clip":
        try:
            ClipBPETokenizer(vocab_path)
        except ValueError as e:
            raise ValueError("register_tokenizer('clip', ...): %s (a WordPiece vocab.txt is registered as 'bert')" % (e,)) from e
    TOKENIZER_VOCABS[name] = (vocab_path, bool(do_lower_case))


def bert_tokenizer():
    """The WordPieceTokenizer of the registered vocabulary; without one an error -- never the hashing stand-in, whose ids
    would address arbitrary rows of a real embedding table."""
    entry = TOKENIZER_VOCABS.get("bert")
    if entry is None and os.environ.get("MCD_BERT_VOCAB"):
        entry = (os.environ["MCD_BERT_VOCAB"], True)
    if entry is None:
        raise RuntimeError("the BERT text tower needs its WordPiece vocabulary: call data_utils.register_tokenizer('bert', "
                           "'/path/vocab.txt') or set MCD_BERT_VOCAB=/path/vocab.txt (the vocab.txt of the checkpoint's "
                           "text model, e.g. Bio_ClinicalBERT's); there is no fallback to the hashing tokenizer")
    return WordPieceTokenizer(entry[0], do_lower_case=entry[1])


class LinearProjectionHead(nn.Module):
    def __init__(self, in_dim, proj_dim):
        super().__init__()
        self.projection = nn.Linear(in_dim, proj_dim, bias=False)

    def forward(self, x):
        return self.projection(x)


# ------------------------------------------------------------------------------------------------------
# Mammo-CLIP ("BreastClip") shaped model: same public surface as reference model/clip.py:12-137
# ------------------------------------------------------------------------------------------------------
class BreastClip(nn.Module):
    """encode_image / encode_text / tokenize / image_projection / text_projection / projection, as the
    reference's utils.py:315-414 uses them.  image tower: 'cnn' = EfficientNet-B5 (the shipped Mammo-CLIP),
    'vit' = ViT-B/16 (reference model/modules/image_encoder.py:14-52, CLS token model/clip.py:49-52).
    text tower: 'stand-in' (the default) = TextTower + HashTokenizer; 'bert' = the reference's own, HFTextEncoder around
    BertTextTower (bert_config: its constructor arguments) with the WordPiece tokenizer of the registered vocabulary.
    text_pooling: 'eos' (the default), 'bos' or 'mean' (model/clip.py:66-77).
    'swin' = HFImageEncoder around a SwinTower (swin_config: its constructor arguments, swin-tiny's by default), token 0 of
    its last_hidden_state as the image feature (model/clip.py:49-52).  width / depth: the EfficientNet's compound-scaling
    coefficients ('cnn' only; B5's by default, 1.1 / 1.2 give B2, out_dim 1408).
    'resnet' = ResNetImageEncoder, the wrapped torchvision ResNet without its fc (layers: the block counts, resnet50's by
    default), out_dim 2048; its flattened average pool is the image feature as it is (the reference's model_type 'cnn'
    branch, model/clip.py:47-48)."""

    def __init__(self, image_tower="cnn", image_size=224, text_depth=12, text_tower="stand-in", bert_config=None,
                 text_pooling="eos", swin_config=None, width=1.6, depth=2.2, layers=None):
        super().__init__()
        self.model_type = image_tower
        if image_tower == "cnn":
            self.image_encoder = EfficientNetTower(width, depth)
        elif image_tower == "swin":
            self.image_encoder = HFImageEncoder(SwinTower(**(swin_config or SWIN_TINY)))
        elif image_tower == "resnet":
            self.image_encoder = ResNetImageEncoder(layers or (3, 4, 6, 3))
        else:
            self.image_encoder = ViTTower(image_size=image_size)
        if text_tower not in ("stand-in", "bert"):
            raise ValueError("text_tower must be 'stand-in' or 'bert', got %r" % (text_tower,))
        self.text_tower = text_tower
        self.text_encoder = TextTower(depth=text_depth) if text_tower == "stand-in" else HFTextEncoder(**(bert_config or {}))
        self.text_pooling = text_pooling
        self.projection = True
        self.image_projection = LinearProjectionHead(self.image_encoder.out_dim, PROJ_DIM)
        self.text_projection = LinearProjectionHead(self.text_encoder.out_dim, PROJ_DIM)
        self.tokenizer = HashTokenizer() if text_tower == "stand-in" else None    # 'bert': resolved at tokenize()

    def encode_image(self, image):
        if self.model_type in ("cnn", "resnet"):
            return self.image_encoder(image)
        if self.model_type == "swin":
            return self.image_encoder(image)[:, 0]
        return self.image_encoder(image, cls_only=True)[:, 0]

    def encode_text(self, text_tokens):
        if not isinstance(text_tokens, dict):
            raise ValueError("Text tokens must be a dictionary")
        f = self.text_encoder(text_tokens)
        if self.text_pooling == "eos":
            eos = text_tokens["attention_mask"].sum(dim=-1) - 1  # 'eos' pooling, model/clip.py:66-69
            return f[torch.arange(f.shape[0], device=f.device), eos]
        if self.text_pooling == "bos":                           # model/clip.py:70-71
            return f[:, 0]
        if self.text_pooling == "mean":                          # model/clip.py:72-75
            m = text_tokens["attention_mask"].unsqueeze(-1).expand(f.size()).float()
            return torch.sum(f * m, dim=1) / torch.clamp(m.sum(dim=1), min=1e-9)
        raise NotImplementedError("Not supported pooling method : %s" % (self.text_pooling,))

    def tokenize(self, texts, max_length=256, padding=True, truncation=True):
        if isinstance(texts, str):
            texts = [texts]
        if self.tokenizer is None:      # the BERT tower: its own vocabulary or an error, never the hashing stand-in
            self.tokenizer = bert_tokenizer()
        tok = self.tokenizer(texts, max_length=max_length, padding=padding, truncation=truncation)
        if self.text_tower == "bert":   # the ids are still on the host: refuse what the embedding table does not have
            rows = self.text_encoder.text_encoder.embeddings.word_embeddings.num_embeddings
            if tok["input_ids"].numel() and int(tok["input_ids"].max()) >= rows:
                raise ValueError("the vocabulary gives token id %d, the checkpoint's embedding table has %d rows: this is "
                                 "not the vocab.txt of the checkpoint's text model" % (int(tok["input_ids"].max()), rows))
        return tok


class BreastClipClassifier(nn.Module):
    """Fine-tuned classifier target (reference Classifiers/models/breast_clip_classifier.py:6-81):
    EfficientNet-B5 image encoder + linear head; forward(images) -> logits [B, n_class].
    width / depth: the EfficientNet's compound-scaling coefficients (1.1 / 1.2: B2, out_dim 1408).  image_tower='swin': the
    reference's other branch, HFImageEncoder around a SwinTower (swin_config) and token 0 of its output; the images are
    [B, 3, H, W] like everywhere in this package (the reference's forward permutes its dataset's channels-last batch).
    image_tower='resnet': ResNetImageEncoder (layers: the block counts of layer1..4), out_dim 2048."""

    def __init__(self, n_class=1, image_tower="cnn", swin_config=None, width=1.6, depth=2.2, layers=None):
        super().__init__()
        self.model_type = image_tower
        if image_tower == "swin":
            self.image_encoder = HFImageEncoder(SwinTower(**(swin_config or SWIN_TINY)))
        elif image_tower == "resnet":
            self.image_encoder = ResNetImageEncoder(layers or (3, 4, 6, 3))
        else:
            self.image_encoder = EfficientNetTower(width, depth)
        self.classifier = nn.Linear(self.image_encoder.out_dim, n_class)

    def encode_image(self, image):
        if self.model_type == "swin":
            return self.image_encoder(image)[:, 0]
        return self.image_encoder(image)

    def forward(self, images):
        return self.classifier(self.encode_image(images))


class ClipViT(nn.Module):
    """OpenAI-CLIP ViT-B/16 shaped dissector/target: hook points vision_model.encoder.layers[i]."""

    def __init__(self, image_size=224, text_depth=12):
        super().__init__()
        self.vision_model = ViTTower(image_size=image_size, list_name="layers")
        self.visual_projection = nn.Linear(768, PROJ_DIM, bias=False)
        self.text_model = TextTower(vocab=49408, dim=512, heads=8, mlp=2048, depth=text_depth, max_pos=77)
        self.text_projection = nn.Linear(512, PROJ_DIM, bias=False)

    def encode_image(self, image):
        return self.visual_projection(self.vision_model(image, cls_only=True)[:, 0])

    def encode_text(self, tokens):
        f = self.text_model(tokens)
        eos = tokens["attention_mask"].sum(dim=-1) - 1
        return self.text_projection(f[torch.arange(f.shape[0], device=f.device), eos])

    def forward(self, image):
        return self.encode_image(image)


# ------------------------------------------------------------------------------------------------------
# HF ViT / DINOv2 image classifiers (the `vit` / `dino` rows of the reference's MODELS table, data_utils.py:21-36:
# ViTForImageClassification / Dinov2ForImageClassification behind AutoModelForImageClassification)
# ------------------------------------------------------------------------------------------------------
class _PatchEmbeddings(nn.Module):
    def __init__(self, dim, patch):
        super().__init__()
        self.projection = nn.Conv2d(3, dim, patch, patch)


class _HFEmbeddings(nn.Module):
    """The embedding parameters under transformers' names: cls_token, position_embeddings,
    patch_embeddings.projection."""

    def __init__(self, dim, patch, n):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.position_embeddings = nn.Parameter(torch.zeros(1, n + 1, dim))
        self.patch_embeddings = _PatchEmbeddings(dim, patch)


def interpolate_pos_table(pos, patch, H, W):
    """transformers' interpolate_pos_encoding (Dinov2Embeddings, the `size=` form of the current releases): the class
    row as it is, the square grid of patch rows resampled to (H / patch) x (W / patch), bicubic, align_corners=False,
    computed in fp32 whatever the table's dtype.  The table is returned untouched when the grid is already the image's
    and H == W."""
    n = pos.shape[1] - 1
    gh, gw = H // patch, W // patch
    if gh * gw == n and H == W:
        return pos
    side = int(n ** 0.5)
    grid = pos[:, 1:].reshape(1, side, side, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid.float(), size=(gh, gw), mode="bicubic", align_corners=False).to(pos.dtype)
    return torch.cat([pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)], dim=1)


class HFTower(ViTTower):
    """ViTTower with its embedding parameters in an `embeddings` submodule (the module tree of transformers' ViTModel /
    Dinov2Model: embeddings, encoder.layer[i], layernorm).  interpolate=True (DINOv2): the position table is resampled to
    the image's patch grid (interpolate_pos_table), once per (H, W)."""

    def __init__(self, interpolate=False, **kw):
        super().__init__(**kw)
        self.interpolate = interpolate

    def _build_embedding(self, dim, patch, n):
        self.embeddings = _HFEmbeddings(dim, patch, n)

    patch_embed = property(lambda self: self.embeddings.patch_embeddings.projection)
    cls_token = property(lambda self: self.embeddings.cls_token)
    pos_embed = property(lambda self: self.embeddings.position_embeddings)

    def pos_table(self, H, W):
        pos, P = self.pos_embed, self.patch_embed.kernel_size[0]
        if not self.interpolate or ((H // P) * (W // P) == pos.shape[1] - 1 and H == W):
            return pos
        if torch.is_grad_enabled() and pos.requires_grad:      # training: the interpolation is part of the graph
            return interpolate_pos_table(pos, P, H, W)
        # cached on the embeddings module: the tower's own cache slot holds the fused path's residual operand
        return _folded(self.embeddings, ("position_embeddings",), lambda m: interpolate_pos_table(
            m.position_embeddings.detach(), P, H, W), extra=(H, W))


def _hf_layer_map(prefix, i, dino, stem="encoder.layer"):
    """transformers-4.41.1 module names of layer i of the list prefix.stem -> this mirror's (q / k / v are handled apart)."""
    base = "%s.%s.%d." % (prefix, stem, i)
    names = {"attention.output.dense": "attn.proj"}
    if dino:                                         # norm1 / norm2 / layer_scale1 / layer_scale2 keep their names
        names.update({"mlp.fc1": "fc1", "mlp.fc2": "fc2"})
    else:
        names.update({"layernorm_before": "norm1", "layernorm_after": "norm2", "intermediate.dense": "fc1",
                      "output.dense": "fc2"})
    return {base + a + "." + leaf: base + b + "." + leaf for a, b in names.items() for leaf in ("weight", "bias")}


def hf_state_dict(sd, prefix, depth, stem="encoder.layer"):
    """A ViTForImageClassification / Dinov2ForImageClassification state dict with transformers-4.41.1 key names (the
    reference's pin) -> the mirror's: the query / key / value projections of a layer concatenated into attn.qkv, the
    other modules renamed, DINOv2's mask_token dropped (it only enters masked-image pre-training).  Keys that are the
    mirror's already pass through, so a dict saved from the mirror loads as well.  stem: the layer list under `prefix`
    (ViTMAEForPreTraining's decoder keeps the same layers in decoder.decoder_layers)."""
    dino = prefix == "dinov2"
    sd = dict(sd)
    sd.pop(prefix + ".embeddings.mask_token", None)
    out = {}
    for i in range(depth):
        base = "%s.%s.%d." % (prefix, stem, i)
        for leaf in ("weight", "bias"):
            parts = [sd.pop(base + "attention.attention.%s.%s" % (n, leaf), None) for n in ("query", "key", "value")]
            if all(t is not None for t in parts):
                out[base + "attn.qkv." + leaf] = torch.cat(parts, dim=0)
            elif any(t is not None for t in parts):
                raise KeyError("%sattention.attention: query, key and value %s must come together" % (base, leaf))
        for old, new in _hf_layer_map(prefix, i, dino, stem).items():
            if old in sd:
                out[new] = sd.pop(old)
    out.update(sd)
    return out


class _HFClassifier(nn.Module):
    """What HFViT and HFDinov2 share: the tower under `prefix`, the linear classifier, the checkpoint mapping."""
    prefix = None

    @property
    def tower(self):
        return getattr(self, self.prefix)

    def convert_state_dict(self, sd):
        enc = self.tower.encoder
        return hf_state_dict(sd, self.prefix, len(getattr(enc, enc._list_name)))

    def encode_image(self, image):
        return self(image)


class HFViT(_HFClassifier):
    """google/vit-base-patch16-224-in21k shaped target (ViTForImageClassification): hook points vit.encoder.layer[i];
    LayerNorm eps 1e-12, exact GELU, the classifier on the class token of vit.layernorm's output.  Only the class token
    is read, so the tower is asked for cls_only (cls_tail_route prunes the last block when the hooks allow)."""
    prefix = "vit"

    def __init__(self, num_labels=2, image_size=224, **kw):
        super().__init__()
        self.vit = HFTower(image_size=image_size, **kw)
        self.classifier = nn.Linear(self.vit.out_dim, num_labels)

    def forward(self, image):
        return _linear(self.classifier, self.vit(image, cls_only=True)[:, 0].contiguous())


class HFDinov2(_HFClassifier):
    """facebook/dinov2-base shaped target (Dinov2ForImageClassification): hook points dinov2.encoder.layer[i]; patch 14,
    LayerNorm eps 1e-6, LayerScale behind the attention projection and behind fc2, the classifier on cat(class token,
    mean of the patch tokens) of dinov2.layernorm's output.  The mean reads every token: the tower always runs whole.
    image_size sizes the position table (Dinov2Config's default 224: 16 x 16 + 1 rows); any other patch grid, or
    H != W, gets the table interpolated."""
    prefix = "dinov2"

    def __init__(self, num_labels=2, image_size=224, patch=14, layer_scale=1.0, eps=1e-6, **kw):
        super().__init__()
        self.dinov2 = HFTower(interpolate=True, image_size=image_size, patch=patch, eps=eps, layer_scale=layer_scale, **kw)
        self.classifier = nn.Linear(2 * self.dinov2.out_dim, num_labels)

    def forward(self, image):
        t = self.dinov2(image)
        return _linear(self.classifier, torch.cat([t[:, 0], t[:, 1:].mean(dim=1)], dim=1))


# name -> (class, classifier width; None: n_class, or transformers' default of 2): reference data_utils.py:21-36.  The
# -cub / -bloodmnist names are the same architectures fine-tuned on CUB-200 and BloodMNIST (8 classes).
HF_TARGETS = {"vit": (HFViT, None), "vit-cub": (HFViT, 200), "vit-bloodmnist": (HFViT, 8),
              "dino": (HFDinov2, None), "dino-cub": (HFDinov2, 200), "dino-bloodmnist": (HFDinov2, 8)}


# ------------------------------------------------------------------------------------------------------
# ResNet-18 / 34 / 50 / 101 / 152 (torchvision layout: conv1, bn1, layer1..4, fc)
# ------------------------------------------------------------------------------------------------------
_BOTTLENECK_SKIPPED = ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "downsample")
_BASICBLOCK_SKIPPED = ("conv1", "bn1", "conv2", "bn2", "downsample")
_RESNET_SKIPPED = ("bn1",)


def _bottleneck_ok(module, x, out_hw):
    """What resnet_route and clip_rn_route both ask of a Bottleneck (conv1 1x1, conv2 3x3, conv3 1x1, .stride) and its
    input: the block's input channels, every width a multiple of 32, stride 1 or 2, channels_last memory at a 16-byte
    address, and one image's widest input, its output (out_hw(stride) pixels) and conv2's weight under 2^31 bytes."""
    B, C, H, W = x.shape
    cin, width, cout, s = module.conv1.in_channels, module.conv2.in_channels, module.conv3.out_channels, module.stride
    return (C == cin and not (cin % 32 or width % 32 or cout % 32) and s in (1, 2) and core.channels_last(x)
            and not x.data_ptr() % 16 and _under_2g(max(cin, width) * H * W, cout * out_hw(s), 9 * width * width))


def resnet_route(module, x):
    """'hip' when a ResNet target (a ResNet or its stem convolution, with the NCHW-contiguous input image) or one of its
    blocks (a _Bottleneck or a _BasicBlock with a channels_last-contiguous input) can take the HIP route: HIP_RESNET on,
    a CUDA fp32 tensor, inference (no autograd, eval mode), libmcd_blaslt.so loaded, widths K16-K18 take (stem: Cin <= 4,
    Cout a multiple of 4, 7x7 / 2 / pad 3; block: every width a multiple of 32, stride 1 or 2), one image's tensors under
    2^31 bytes, at most 65535 images, and no hook on a submodule the route does not call (a hook on layer2[0].conv2 must
    fire, so that block takes ATen; the hook points of the tower itself -- conv1 and layer1..4 -- are called as modules
    on either route).  'aten' otherwise.
    A _BasicBlock calls no library GEMM, but it asks for libmcd_blaslt.so like everything else (_tower_gate): one gate
    for the whole family, so a tower never runs half of its stages on each route for want of a library.  Its stride-1
    block with cin != width (a 1x1 / 1 downsample, which K18 does not do and torchvision does not build) takes ATen."""
    if not _tower_gate(HIP_RESNET, module, x):
        return "aten"
    B, C, H, W = x.shape
    if H < 1 or W < 1:
        return "aten"
    if isinstance(module, _Bottleneck):
        ok = _bottleneck_ok(module, x, lambda s: core.conv_out(H, 3, s, 1) * core.conv_out(W, 3, s, 1))
        names = _BOTTLENECK_SKIPPED                     # "downsample" covers the convolution and the batch norm in it
    elif isinstance(module, _BasicBlock):
        cin, width, s = module.conv1.in_channels, module.conv2.out_channels, module.stride
        ok = (C == cin and not (cin % 32 or width % 32) and s in (1, 2) and (s == 2 or cin == width)
              and core.channels_last(x) and not x.data_ptr() % 16
              and _under_2g(cin * H * W, width * core.conv_out(H, 3, s, 1) * core.conv_out(W, 3, s, 1),
                            9 * max(cin, width) * width))
        names = _BASICBLOCK_SKIPPED
    elif isinstance(module, (ResNet, _StemConv)):
        stem = module.conv1 if isinstance(module, ResNet) else module
        ho, wo = core.conv_out(H, 7, 2, 3), core.conv_out(W, 7, 2, 3)
        ok = (C == stem.in_channels and C <= 4 and not stem.out_channels % 4 and stem.kernel_size == (7, 7)
              and stem.stride == (2, 2) and stem.padding == (3, 3) and stem.dilation == (1, 1) and stem.groups == 1
              and stem.bias is None and x.is_contiguous() and not x.data_ptr() % 16
              and _under_2g(C * H * W, stem.out_channels * ho * wo))
        if isinstance(module, _StemConv):
            return "hip" if ok else "aten"              # nothing inside it is skipped; its own hooks fire
        ok = ok and ho >= 1 and wo >= 1 and isinstance(stem, _StemConv)
        names = _RESNET_SKIPPED
    else:
        return "aten"
    return "hip" if ok and not _hooks_on(module, names) else "aten"


class _StemConv(nn.Conv2d):
    """A ResNet's conv1.  On the HIP route K16 computes it and the result comes back as a [B, Cout, Ho, Wo] view of
    channels-last memory; it is still called as a module, so a hook on conv1 sees the raw convolution output."""

    def forward(self, x):
        if resnet_route(self, x) == "hip":
            w = _folded(self, (), lambda m: m.weight.detach().permute(1, 2, 3, 0).contiguous(), own=True)   # tap-major
            return core.conv7x7s2_nhwc(x, w).permute(0, 3, 1, 2)
        return super().forward(x)


def _bottleneck_hip(x, f, stride):
    """A bottleneck block on channels-last activations, from its folded operands f (w1, b1: "gemm"; w2, b2: "igemm"; w3,
    b3: "gemm"; wd, bd: "igemm", absent without a projection on the skip): conv1 as a GEMM (raw, folded bn1 as its bias;
    its ReLU is K18's relu_in), conv2 by K18 (3x3 / stride, folded bn2, ReLU on the way in and out), the projection as a
    GEMM (stride 1) or K18 1x1 / 2 (stride 2) with folded BN, conv3 as one GEMM with folded bn3 as its bias, the skip as its
    residual operand and the ReLU as its epilogue.  Returns [B, C, H, W] in channels_last memory.  The one launch
    sequence of torchvision's Bottleneck (_Bottleneck) and transformers' ResNetBottleNeckLayer (_HFResNetBottleNeckLayer)."""
    xn = x.permute(0, 2, 3, 1)                                   # [B, H, W, cin], contiguous
    h = core.linear_residual(None, xn, f["w1"], f["b1"])
    h = core.conv_igemm_nhwc(h, f["w2"], f["b2"], 3, stride, relu_in=True, relu_out=True)
    if "wd" not in f:
        res = xn
    elif stride == 1:
        res = core.linear_residual(None, xn, f["wd"], f["bd"])
    else:
        res = core.conv_igemm_nhwc(xn, f["wd"], f["bd"], 1, 2)
    return core.linear_residual(res, h, f["w3"], f["b3"], relu=True).permute(0, 3, 1, 2)


def _basic_block_hip(x, f, stride):
    """A basic block on channels-last activations, from its folded operands f (w1, b1, w2, b2, and wd, bd with a
    projection on the skip; all "igemm"): two K18 launches (three with a projection) and nothing else: conv1 (3x3 /
    stride, folded bn1, ReLU on the way out), the skip (x itself, or K18 1x1 / 2 with the folded batch norm), conv2
    (3x3 / 1, folded bn2) with the skip as K18's residual operand and the ReLU behind the add.  x is left alone.  Returns
    [B, C, H, W] in channels_last memory.  Shared by _BasicBlock and _HFResNetBasicLayer."""
    xn = x.permute(0, 2, 3, 1)                                   # [B, H, W, cin], contiguous
    h = core.conv_igemm_nhwc(xn, f["w1"], f["b1"], 3, stride, relu_out=True)
    res = xn if "wd" not in f else core.conv_igemm_nhwc(xn, f["wd"], f["bd"], 1, 2)
    return core.conv_igemm_nhwc(h, f["w2"], f["b2"], 3, 1, relu_out=True, res=res).permute(0, 3, 1, 2)


class _Bottleneck(nn.Module):
    expansion = 4                                    # output channels / width

    def __init__(self, cin, width, stride):
        super().__init__()
        cout = width * 4
        self.stride = stride
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        if resnet_route(self, x) == "hip":
            return self._forward_hip(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))

    def _forward_hip(self, x):
        return _bottleneck_hip(x, _folded(self, _BOTTLENECK_SKIPPED, _Bottleneck._fold), self.stride)

    def _fold(self):
        f = {}
        f["w1"], f["b1"] = _fold_conv(self.conv1, self.bn1, "gemm")
        f["w2"], f["b2"] = _fold_conv(self.conv2, self.bn2, "igemm")
        f["w3"], f["b3"] = _fold_conv(self.conv3, self.bn3, "gemm")
        if self.downsample is not None:
            f["wd"], f["bd"] = _fold_conv(self.downsample[0], self.downsample[1], "igemm")   # 1x1: [Cout, Cin] either way
        return f


class _BasicBlock(nn.Module):
    """torchvision's BasicBlock (ResNet-18 / -34): conv3x3 -> bn -> relu -> conv3x3 -> bn -> (+ skip) -> relu; the output
    has `width` channels."""
    expansion = 1                                    # output channels / width

    def __init__(self, cin, width, stride):
        super().__init__()
        self.stride = stride
        self.conv1 = nn.Conv2d(cin, width, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.downsample = None
        if stride != 1 or cin != width:
            self.downsample = nn.Sequential(nn.Conv2d(cin, width, 1, stride, bias=False), nn.BatchNorm2d(width))

    def forward(self, x):
        if resnet_route(self, x) == "hip":
            return self._forward_hip(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))

    def _forward_hip(self, x):
        return _basic_block_hip(x, _folded(self, _BASICBLOCK_SKIPPED, _BasicBlock._fold), self.stride)

    def _fold(self):
        f = {}
        f["w1"], f["b1"] = _fold_conv(self.conv1, self.bn1, "igemm")
        f["w2"], f["b2"] = _fold_conv(self.conv2, self.bn2, "igemm")
        if self.downsample is not None:
            f["wd"], f["bd"] = _fold_conv(self.downsample[0], self.downsample[1], "igemm")
        return f


class _Stage(nn.Sequential):
    """layer1..4: a Sequential that keeps handing on channels-last memory when it was given channels-last memory (a
    block that took ATen, for a hook inside it, say, may hand back NCHW memory, which the next block's HIP route
    refuses).  On NCHW input it is a plain Sequential."""

    def forward(self, x):
        keep = core.channels_last(x, only=True)
        for b in self:
            x = b(x)
            if keep:
                x = x.contiguous(memory_format=torch.channels_last)
        return x


class ResNet(nn.Module):
    """The torchvision ResNet of `block` (_BasicBlock or _Bottleneck) with layers[i] blocks of width 64 << i in
    layer<i+1>; the stem, the stages, the pooling and fc are the same for every depth.  num_classes=None builds it
    without fc (no fc.* key): forward then returns the flattened average pool [B, 512 * expansion], which is what
    Mammo-CLIP's ResNet image encoder keeps of torchvision's model (ResNetImageEncoder)."""

    def __init__(self, block, layers, num_classes=1000):
        super().__init__()
        self.conv1 = _StemConv(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for i, (w, n, s) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 2)), 1):
            blocks = []
            for j in range(n):
                blocks.append(block(cin, w, s if j == 0 else 1))
                cin = w * block.expansion
            setattr(self, "layer%d" % i, _Stage(*blocks))
        self.out_dim = cin
        if num_classes is not None:
            self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        if resnet_route(self, x) == "hip":
            return self._forward_hip(x)
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = x.mean(dim=[2, 3])
        return self.fc(x) if hasattr(self, "fc") else x

    def _forward_hip(self, x):
        """conv1 called as a module (K16 inside; a hook on it fires on the raw output), bn1 + ReLU + max pooling by K17,
        layer1..4 called as modules (hooks on them fire; each block picks its own route), the mean over the pixels by
        K0n, fc."""
        scale, shift = _folded(self, _RESNET_SKIPPED, lambda m: bn_scale_shift(m.bn1))
        x = self.conv1(x).contiguous(memory_format=torch.channels_last)     # a no-op copy on the HIP route
        x = core.bn_relu_maxpool_nhwc(x.permute(0, 2, 3, 1), scale, shift).permute(0, 3, 1, 2)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))         # _Stage keeps the memory channels-last
        pooled = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        core.hook_pool(x, "avg", pooled, 0, 0, False)                      # K0n: the mean over the pixels, batch-invariant
        return self.fc(pooled) if hasattr(self, "fc") else pooled

    encode_image = forward  # describe_og_neurons.py calls encode_image on every target


class ResNet50(ResNet):
    def __init__(self, num_classes=1000):
        super().__init__(_Bottleneck, [3, 4, 6, 3], num_classes)


# name -> (block, layers, classes): the reference's torchvision targets and its Places365 ResNet-18 (data_utils.py:70-89)
RESNETS = {"resnet18": (_BasicBlock, [2, 2, 2, 2], 1000), "resnet34": (_BasicBlock, [3, 4, 6, 3], 1000),
           "resnet101": (_Bottleneck, [3, 4, 23, 3], 1000), "resnet152": (_Bottleneck, [3, 8, 36, 3], 1000),
           "resnet18_places": (_BasicBlock, [2, 2, 2, 2], 365)}
PLACES_CKPT = "data/resnet18_places365.pth.tar"      # where the reference keeps it, relative to the working directory


class ResNetImageEncoder(nn.Module):
    """Mammo-CLIP's ResNet image encoder (reference model/modules/image_encoder.py:123-156): torchvision's resnet50 /
    resnet101 / resnet152 held as `.resnet`, its fc deleted, forward = the flattened average pool [B, 2048].  The wrapped
    module is a ResNet of _Bottlenecks, so the HIP route is resnet_route's as it stands; hook points are
    image_encoder.resnet.conv1 and .layer1..4."""

    def __init__(self, layers=(3, 4, 6, 3)):
        super().__init__()
        self.resnet = ResNet(_Bottleneck, list(layers), num_classes=None)
        self.out_dim = self.resnet.out_dim

    def forward(self, image):
        return self.resnet(image)


RESNET_TOWER_KEY = "image_encoder.resnet.conv1.weight"      # what tells a Mammo-CLIP checkpoint with a ResNet image tower
RESNET_TOWER_LAYERS = ([3, 4, 6, 3], [3, 4, 23, 3], [3, 8, 36, 3])     # resnet50 / 101 / 152, what the reference builds


def resnet_tower_layers(sd, prefix="image_encoder.resnet."):
    """The block counts of layer1..4 under `prefix`, read from the keys of a state dict."""
    counts = []
    for i in range(1, 5):
        stem = "%slayer%d." % (prefix, i)
        counts.append(1 + max([int(k[len(stem):].split(".")[0]) for k in sd if k.startswith(stem)], default=-1))
    return counts


# ------------------------------------------------------------------------------------------------------
# transformers' ResNetForImageClassification under its own module names (the reference's `resnet`, `resnet-cub` and
# `resnet-bloodmnist` targets, data_utils.py:21-36 and :63-69: microsoft/resnet-50 and its fine-tunes)
# ------------------------------------------------------------------------------------------------------
HF_RESNET_KEY = "resnet.embedder.embedder.convolution.weight"     # what tells a ResNetForImageClassification state dict
_HF_LAYER_SKIPPED = ("shortcut", "layer", "activation")
_HF_CONVLAYER_SKIPPED = ("convolution", "normalization", "activation")
_HF_EMBEDDINGS_SKIPPED = ("pooler",)
_HF_MODEL_SKIPPED = ("pooler",)


def hf_resnet_route(module, x):
    """'hip' when a module of an HFResNet can take the HIP route for the tensor it is called with: resnet_route's gate and
    rules, under the same flag -- HIP_RESNET on (MCD_NO_HIP_RESNET=1 turns it off), a CUDA fp32 tensor, inference (no
    autograd, eval mode), libmcd_blaslt.so loaded, at most 65535 images, one image's tensors under 2^31 bytes -- and no
    hook on a submodule that the route would skip (the module then takes ATen, for itself alone).  'aten' otherwise.
      the stem _HFResNetConvLayer (resnet.embedder.embedder) with the NCHW-contiguous image: a 7x7 / 2 / pad 3 convolution without
        bias, Cin <= 4, Cout a multiple of 4, a ReLU behind it; skipped: convolution, normalization, activation.  A hook on
        the unit itself fires on either route and sees the tensor behind the ReLU.  Any other _HFResNetConvLayer called on its
        own takes ATen (inside a layer, the layer's route decides).
      _HFResNetEmbeddings (resnet.embedder): the stem's shapes as above (a stem that takes ATen for a hook inside it still hands
        its output to K17), an output of at least one pixel; skipped: pooler.
      _HFResNetBottleNeckLayer with a channels_last-contiguous input: _bottleneck_ok's rules (every width a multiple of 32,
        stride 1 or 2, 16-byte address) with the stride on the 3x3.  downsample_in_bottleneck=True moves the stride to the
        first 1x1, which is no GEMM any more: such a layer with stride 2 takes ATen, its stride-1 layers are the same
        module either way and take HIP.  Skipped: shortcut, layer, activation (a hook on layer[1].convolution must fire,
        so that layer takes ATen and its neighbours do not).
      _HFResNetBasicLayer with a channels_last-contiguous input: the rules of a _BasicBlock (widths multiples of 32, stride 2 or
        cin == width: K18 has no 1x1 / 1).  Skipped: shortcut, layer, activation.
      _HFResNetModel (resnet) with the last stage's output: any 4-D tensor K0n pools; skipped: pooler (a hooked pooler is
        called as a module)."""
    if not _tower_gate(HIP_RESNET, module, x):
        return "aten"
    B, C, H, W = x.shape
    if H < 1 or W < 1:
        return "aten"
    if isinstance(module, _HFResNetBottleNeckLayer):
        ok = (not (module.downsample_in_bottleneck and module.stride != 1)
              and _bottleneck_ok(module, x, lambda s: core.conv_out(H, 3, s, 1) * core.conv_out(W, 3, s, 1)))
        names = _HF_LAYER_SKIPPED
    elif isinstance(module, _HFResNetBasicLayer):
        cin, width, s = module.conv1.in_channels, module.conv2.out_channels, module.stride
        ok = (C == cin and not (cin % 32 or width % 32) and s in (1, 2) and (s == 2 or cin == width)
              and core.channels_last(x) and not x.data_ptr() % 16
              and _under_2g(cin * H * W, width * core.conv_out(H, 3, s, 1) * core.conv_out(W, 3, s, 1),
                            9 * max(cin, width) * width))
        names = _HF_LAYER_SKIPPED
    elif isinstance(module, (_HFResNetConvLayer, _HFResNetEmbeddings)):
        unit = module.embedder if isinstance(module, _HFResNetEmbeddings) else module
        stem = unit.convolution
        ho, wo = core.conv_out(H, 7, 2, 3), core.conv_out(W, 7, 2, 3)
        ok = (C == stem.in_channels and C <= 4 and not stem.out_channels % 4 and stem.kernel_size == (7, 7)
              and stem.stride == (2, 2) and stem.padding == (3, 3) and stem.dilation == (1, 1) and stem.groups == 1
              and stem.bias is None and isinstance(unit.activation, nn.ReLU) and x.is_contiguous()
              and not x.data_ptr() % 16 and ho >= 1 and wo >= 1 and _under_2g(C * H * W, stem.out_channels * ho * wo))
        names = _HF_EMBEDDINGS_SKIPPED if isinstance(module, _HFResNetEmbeddings) else _HF_CONVLAYER_SKIPPED
    elif isinstance(module, _HFResNetModel):
        ok, names = _under_2g(C * H * W), _HF_MODEL_SKIPPED
    else:
        return "aten"
    return "hip" if ok and not _hooks_on(module, names) else "aten"


class _HFResNetConvLayer(nn.Module):
    """transformers' ResNetConvLayer: convolution (no bias, pad k // 2), normalization, activation (ReLU, or Identity)."""

    def __init__(self, cin, cout, k=3, stride=1, act=True):
        super().__init__()
        self.convolution = nn.Conv2d(cin, cout, k, stride, k // 2, bias=False)
        self.normalization = nn.BatchNorm2d(cout)
        self.activation = nn.ReLU() if act else nn.Identity()

    def forward(self, x):
        if hf_resnet_route(self, x) == "hip":
            # the stem: one launch, the folded batch norm as bias and the ReLU in the epilogue; a [B, Cout, Ho, Wo] view
            # of channels-last memory comes back
            w, b = _folded(self, _HF_CONVLAYER_SKIPPED, lambda m: _fold_conv(m.convolution, m.normalization, "tap"))
            return core.conv7x7s2_bias_relu_nhwc(x, w, b, relu=True).permute(0, 3, 1, 2)
        return self.activation(self.normalization(self.convolution(x)))


class _HFResNetEmbeddings(nn.Module):
    """transformers' ResNetEmbeddings: embedder (the 7x7 / 2 unit) and pooler (max pooling 3 / 2 / 1)."""

    def __init__(self, num_channels, embedding_size):
        super().__init__()
        self.embedder = _HFResNetConvLayer(num_channels, embedding_size, 7, 2)
        self.pooler = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.num_channels = num_channels

    def forward(self, x):
        if x.shape[1] != self.num_channels:
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the "
                             "configuration.")
        if hf_resnet_route(self, x) != "hip":
            return self.pooler(self.embedder(x))
        # K17 with unit scale and zero shift: relu(fma(x, 1, 0)) is x on a ReLU's output, so this is the max pooling
        y = self.embedder(x).contiguous(memory_format=torch.channels_last)     # a no-op copy on the HIP route
        one, zero = _folded(self, ("embedder",), lambda m: (torch.ones_like(m.embedder.normalization.weight),
                                                            torch.zeros_like(m.embedder.normalization.weight)))
        return core.bn_relu_maxpool_nhwc(y.permute(0, 2, 3, 1), one, zero).permute(0, 3, 1, 2)


class _HFResNetShortCut(nn.Module):
    """transformers' ResNetShortCut: convolution 1x1 / stride (no bias), normalization."""

    def __init__(self, cin, cout, stride=2):
        super().__init__()
        self.convolution = nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False)
        self.normalization = nn.BatchNorm2d(cout)

    def forward(self, x):
        return self.normalization(self.convolution(x))


class _HFResNetLayer(nn.Module):
    """What both of transformers' residual layers share: shortcut (a _HFResNetShortCut, or Identity when neither the channel
    count nor the stride changes), layer (a Sequential of _HFResNetConvLayers, the last without activation), activation."""

    def _build(self, cin, cout, stride, units):
        self.stride = stride
        self.shortcut = _HFResNetShortCut(cin, cout, stride) if cin != cout or stride != 1 else nn.Identity()
        self.layer = nn.Sequential(*units)
        self.activation = nn.ReLU()

    def forward(self, x):
        if hf_resnet_route(self, x) == "hip":
            return self._hip(x, _folded(self, _HF_LAYER_SKIPPED, type(self)._fold), self.stride)
        return self.activation(self.layer(x) + self.shortcut(x))

    def _fold_units(self, layouts):
        f = {}
        for i, (unit, layout) in enumerate(zip(self.layer, layouts), 1):
            f["w%d" % i], f["b%d" % i] = _fold_conv(unit.convolution, unit.normalization, layout)
        if isinstance(self.shortcut, _HFResNetShortCut):
            f["wd"], f["bd"] = _fold_conv(self.shortcut.convolution, self.shortcut.normalization, "igemm")
        return f


class _HFResNetBottleNeckLayer(_HFResNetLayer):
    """transformers' ResNetBottleNeckLayer: 1x1, 3x3 / stride, 1x1 (reduction 4); downsample_in_bottleneck moves the
    stride to the first 1x1.  On the HIP route it is _bottleneck_hip, the launches of a torchvision Bottleneck."""

    def __init__(self, cin, cout, stride=1, reduction=4, downsample_in_bottleneck=False):
        super().__init__()
        mid = cout // reduction
        self.downsample_in_bottleneck = downsample_in_bottleneck
        self._build(cin, cout, stride, [_HFResNetConvLayer(cin, mid, 1, stride if downsample_in_bottleneck else 1),
                                       _HFResNetConvLayer(mid, mid, 3, 1 if downsample_in_bottleneck else stride),
                                       _HFResNetConvLayer(mid, cout, 1, act=False)])

    conv1 = property(lambda self: self.layer[0].convolution)       # what _bottleneck_ok reads
    conv2 = property(lambda self: self.layer[1].convolution)
    conv3 = property(lambda self: self.layer[2].convolution)
    _hip = staticmethod(_bottleneck_hip)

    def _fold(self):
        return self._fold_units(("gemm", "igemm", "gemm"))


class _HFResNetBasicLayer(_HFResNetLayer):
    """transformers' ResNetBasicLayer: 3x3 / stride, 3x3.  On the HIP route it is _basic_block_hip."""

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self._build(cin, cout, stride, [_HFResNetConvLayer(cin, cout, 3, stride), _HFResNetConvLayer(cout, cout, 3, act=False)])

    conv1 = property(lambda self: self.layer[0].convolution)
    conv2 = property(lambda self: self.layer[1].convolution)
    _hip = staticmethod(_basic_block_hip)

    def _fold(self):
        return self._fold_units(("igemm", "igemm"))


class _HFResNetStage(nn.Module):
    """transformers' ResNetStage: layers, a Sequential (a _Stage: it keeps channels-last memory between the layers)."""

    def __init__(self, layer_type, cin, cout, stride, depth, downsample_in_bottleneck):
        super().__init__()
        if layer_type == "bottleneck":
            first = _HFResNetBottleNeckLayer(cin, cout, stride, downsample_in_bottleneck=downsample_in_bottleneck)
            rest = [_HFResNetBottleNeckLayer(cout, cout) for _ in range(depth - 1)]
        else:
            first = _HFResNetBasicLayer(cin, cout, stride)
            rest = [_HFResNetBasicLayer(cout, cout) for _ in range(depth - 1)]
        self.layers = _Stage(first, *rest)

    def forward(self, x):
        return self.layers(x)


class _HFResNetEncoder(nn.Module):
    def __init__(self, layer_type, embedding_size, hidden_sizes, depths, downsample_in_first_stage,
                 downsample_in_bottleneck):
        super().__init__()
        self.stages = nn.ModuleList()
        cin = embedding_size
        for i, (cout, depth) in enumerate(zip(hidden_sizes, depths)):
            stride = 2 if i or downsample_in_first_stage else 1
            self.stages.append(_HFResNetStage(layer_type, cin, cout, stride, depth, downsample_in_bottleneck))
            cin = cout

    def forward(self, x):
        for stage in self.stages:
            x = stage(x)
        return x


class _HFResNetModel(nn.Module):
    """transformers' ResNetModel: embedder, encoder, pooler; forward returns the pooler's output [B, C, 1, 1]."""

    def __init__(self, num_channels, embedding_size, hidden_sizes, depths, layer_type, downsample_in_first_stage,
                 downsample_in_bottleneck):
        super().__init__()
        self.embedder = _HFResNetEmbeddings(num_channels, embedding_size)
        self.encoder = _HFResNetEncoder(layer_type, embedding_size, hidden_sizes, depths, downsample_in_first_stage,
                                  downsample_in_bottleneck)
        self.pooler = nn.AdaptiveAvgPool2d((1, 1))

    def forward(self, x):
        x = self.encoder(self.embedder(x))
        if hf_resnet_route(self, x) != "hip":
            return self.pooler(x)
        pooled = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        core.hook_pool(x, "avg", pooled, 0, 0, False)                      # K0n: the mean over the pixels, batch-invariant
        return pooled[:, :, None, None]


def hf_resnet_config(sd, downsample_in_first_stage=False, downsample_in_bottleneck=False):
    """HFResNet's constructor arguments read from the shapes of a ResNetForImageClassification state dict: num_channels
    and embedding_size from the stem's weight, depths by counting the layers of every stage, hidden_sizes from each
    stage's last convolution, layer_type 'bottleneck' exactly when a layer.2 exists, num_labels from classifier.1.weight
    when the file has one (else the key is absent: the caller decides).  The state dict does not carry the two
    downsample_* flags: False, microsoft/resnet-*'s value, unless the caller says otherwise."""
    def shape(key):
        if key not in sd:
            raise RuntimeError("not a ResNetForImageClassification state dict: it lacks %r" % (key,))
        return tuple(sd[key].shape)
    embedding_size, num_channels = shape(HF_RESNET_KEY)[:2]
    stem = "resnet.encoder.stages."
    found = {}
    for k in sd:
        if k.startswith(stem) and k.endswith(".convolution.weight"):
            parts = k[len(stem):].split(".")
            if len(parts) >= 3 and parts[1] == "layers" and parts[0].isdigit() and parts[2].isdigit():
                found.setdefault(int(parts[0]), set()).add(int(parts[2]))
    shape(stem + "0.layers.0.layer.0.convolution.weight")
    depths = [1 + max(found[s]) for s in sorted(found)]
    bottleneck = stem + "0.layers.0.layer.2.convolution.weight" in sd
    last = 2 if bottleneck else 1
    hidden_sizes = [shape("%s%d.layers.0.layer.%d.convolution.weight" % (stem, s, last))[0] for s in range(len(depths))]
    cfg = dict(num_channels=num_channels, embedding_size=embedding_size, hidden_sizes=hidden_sizes, depths=depths,
               layer_type="bottleneck" if bottleneck else "basic", downsample_in_first_stage=downsample_in_first_stage,
               downsample_in_bottleneck=downsample_in_bottleneck)
    if "classifier.1.weight" in sd:
        cfg["num_labels"] = shape("classifier.1.weight")[0]
    return cfg


class HFResNet(nn.Module):
    """transformers' ResNetForImageClassification under transformers' own module and parameter names, so that a real state
    dict loads strictly and the reference's --target_layers resolve: resnet.embedder.embedder.{convolution, normalization,
    activation}, resnet.embedder.pooler, resnet.encoder.stages[s].layers[l].{shortcut.{convolution, normalization},
    layer[k].{convolution, normalization, activation}}, resnet.pooler, classifier = Sequential(Flatten, Linear).  The
    defaults are microsoft/resnet-50's.

    forward(pixel_values) -> the logits tensor [B, num_labels] (encode_image is the same call).
    Hook points: every module of the tree; a dissection uses resnet.embedder (behind the pooling),
    resnet.embedder.embedder (behind the ReLU), resnet.encoder.stages[i] and .layers[j], resnet.pooler, classifier.

    The HIP route (HIP_RESNET, hf_resnet_route; every module picks its own): the stem unit in one launch (K16's kernel with
    the folded batch norm as bias and the ReLU in its epilogue, include/mcd_stem.h), K17 as the max pooling, per layer
    the launches of the torchvision blocks (_bottleneck_hip, _basic_block_hip) on channels-last memory, K0n for the
    mean, the classifier's Linear."""

    def __init__(self, num_labels=1000, num_channels=3, embedding_size=64, hidden_sizes=(256, 512, 1024, 2048),
                 depths=(3, 4, 6, 3), layer_type="bottleneck", downsample_in_first_stage=False,
                 downsample_in_bottleneck=False):
        super().__init__()
        if layer_type not in ("basic", "bottleneck"):
            raise ValueError("layer_type must be 'basic' or 'bottleneck', got %r" % (layer_type,))
        if len(hidden_sizes) != len(depths) or not depths or min(depths) < 1:
            raise ValueError("hidden_sizes %r and depths %r must be equally long, every depth at least 1"
                             % (tuple(hidden_sizes), tuple(depths)))
        self.resnet = _HFResNetModel(num_channels, embedding_size, list(hidden_sizes), list(depths), layer_type,
                                     downsample_in_first_stage, downsample_in_bottleneck)
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(hidden_sizes[-1], num_labels))

    @classmethod
    def from_state_dict(cls, sd, n_class=None, **flags):
        """The model of a ResNetForImageClassification state dict: sized by hf_resnet_config (flags: its two downsample_*
        keywords), fp16 tensors upcast, loaded STRICTLY -- a missing or an unexpected key is an error, never a model of
        random weights.  A file without classifier.* keeps the freshly initialised head with n_class outputs (2 when
        None, transformers' default), as HFClip.from_state_dict does."""
        sd = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}
        cfg = hf_resnet_config(sd, **flags)
        cfg.setdefault("num_labels", 2 if n_class is None else n_class)
        model = cls(**cfg)
        want = set(model.state_dict())
        if not any(k.startswith("classifier.") for k in sd):
            want -= {"classifier.1.weight", "classifier.1.bias"}
        missing, unexpected = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or unexpected:
            raise RuntimeError("the checkpoint does not match ResNetForImageClassification: %d missing key(s) %s, %d "
                               "unexpected key(s) %s" % (len(missing), missing[:4], len(unexpected), unexpected[:4]))
        model.load_state_dict(sd, strict=False)          # (the key sets were compared above; shapes are checked here)
        return model

    def forward(self, pixel_values):
        return self.classifier(self.resnet(pixel_values.to(self.classifier[1].weight.dtype)))

    def encode_image(self, image):
        return self(image)


HF_RESNET_TARGETS = ("resnet", "resnet-cub", "resnet-bloodmnist")
HF_CLIP_TARGETS = ("clip", "clip-cub", "clip-bloodmnist")


# ------------------------------------------------------------------------------------------------------
# OpenAI-CLIP RN50 / RN101 (the anti-aliased "ModifiedResNet" with an attention-pooling head; parameter names under
# `visual.` follow OpenAI's layout so that a local CLIP state dict's visual.* keys load strictly)
# ------------------------------------------------------------------------------------------------------
_CLIP_BOTTLENECK_SKIPPED = ("conv1", "bn1", "conv2", "bn2", "avgpool", "conv3", "bn3", "downsample")
_CLIP_STEM_SKIPPED = ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "avgpool")
_ATTNPOOL_SKIPPED = ("q_proj", "k_proj", "v_proj", "c_proj")


def _plain_conv(conv, k, s, p):
    """conv is the bias-free, ungrouped k x k / s convolution with pad p."""
    return (conv.kernel_size == (k, k) and conv.stride == (s, s) and conv.padding == (p, p) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None)


def clip_rn_route(module, x):
    """'hip' when a piece of the CLIP ResNet can take the HIP route: HIP_CLIP_RN on, a CUDA fp32 4-D tensor, inference (no
    autograd, eval mode), libmcd_blaslt.so loaded, at most 65535 images, one image's tensors under 2^31 bytes, and no hook
    on a submodule the route does not call (a hook on visual.layer2[0].conv2 must fire, so that block takes ATen; the hook
    points visual.layer1..4 and visual.attnpool are called as modules on either route).  'aten' otherwise.
      ModifiedResNet   its stem, on the NCHW-contiguous image: Cin <= 4, width a multiple of 64 (K18 takes multiples of
                       32 and the stem's first two convolutions have width / 2 channels: the RN50x4 / x16 / x64 widths
                       80, 96, 128 are out of scope and take ATen, 128 included, for one rule), at least 2 x 2 pixels
                       in front of the pooling;
      _ClipBottleneck  a channels_last-contiguous input, every width a multiple of 32, stride 1 or 2 (2: at least 2 x 2
                       pixels);
      AttentionPool2d  a channels_last-contiguous input of embed_dim = 64 * heads channels whose pixels + 1 are the rows
                       of positional_embedding, within K9C's token limit, all four projections with a bias."""
    if not _tower_gate(HIP_CLIP_RN, module, x):
        return "aten"
    B, C, H, W = x.shape
    if H < 1 or W < 1:
        return "aten"
    if isinstance(module, _ClipBottleneck):
        ok = _bottleneck_ok(module, x, lambda s: (H // s) * (W // s)) and (module.stride == 1 or (H >= 2 and W >= 2))
        names = _CLIP_BOTTLENECK_SKIPPED               # "downsample" covers the pooling, the convolution and the batch norm
    elif isinstance(module, AttentionPool2d):
        E, T = module.embed_dim, H * W + 1
        ok = (C == E and E == 64 * module.num_heads and T == module.positional_embedding.shape[0]
              and T <= core.VIT_ATTENTION_CLS_MAX_T and core.channels_last(x) and not x.data_ptr() % 16
              and all(getattr(module, n).bias is not None for n in _ATTNPOOL_SKIPPED) and _under_2g(T * 2 * E))
        names = _ATTNPOOL_SKIPPED
    elif isinstance(module, ModifiedResNet):
        c1, c3 = module.conv1.out_channels, module.conv3.out_channels
        ho, wo = core.conv_out(H, 3, 2, 1), core.conv_out(W, 3, 2, 1)
        ok = (C == module.conv1.in_channels and C <= 4 and c3 % 64 == 0 and 2 * c1 == c3
              and module.conv2.in_channels == c1 and module.conv2.out_channels == c1 and module.conv3.in_channels == c1
              and _plain_conv(module.conv1, 3, 2, 1) and _plain_conv(module.conv2, 3, 1, 1)
              and _plain_conv(module.conv3, 3, 1, 1) and ho >= 2 and wo >= 2 and x.is_contiguous()
              and not x.data_ptr() % 16 and _under_2g(C * H * W, c3 * ho * wo))
        names = _CLIP_STEM_SKIPPED
    else:
        return "aten"
    return "hip" if ok and not _hooks_on(module, names) else "aten"


class _ClipBottleneck(nn.Module):
    """CLIP's anti-aliased Bottleneck: every convolution has stride 1; a block of stride s > 1 average-pools s x s behind
    conv2 and, on the skip, in front of the 1x1 downsample convolution (downsample."-1")."""
    expansion = 4

    def __init__(self, cin, width, stride=1):
        super().__init__()
        cout = width * self.expansion
        self.stride = stride
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.avgpool = nn.Identity() if stride == 1 else nn.AvgPool2d(stride, stride)     # no parameters: no keys
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride > 1 or cin != cout:
            self.downsample = nn.Sequential()
            self.downsample.add_module("-1", nn.AvgPool2d(stride))
            self.downsample.add_module("0", nn.Conv2d(cin, cout, 1, bias=False))
            self.downsample.add_module("1", nn.BatchNorm2d(cout))

    def forward(self, x):
        if clip_rn_route(self, x) == "hip":
            return self._forward_hip(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.avgpool(F.relu(self.bn2(self.conv2(y))))
        y = self.bn3(self.conv3(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))

    def _forward_hip(self, x):
        """The block on channels-last activations: conv1 as a GEMM (raw, folded bn1 as its bias; its ReLU is K18's
        relu_in), conv2 by K18 (3x3 / 1, folded bn2, ReLU on the way in and out); at stride 2, K20 on conv2's output and
        on the block's input for the skip; the downsample as a GEMM on the (pooled) input with folded BN; conv3 as one
        GEMM with folded bn3 as its bias, the skip as its residual operand and the ReLU as its epilogue.  x is left alone.
        Returns [B, C, H, W] in channels_last memory."""
        f = _folded(self, _CLIP_BOTTLENECK_SKIPPED, _ClipBottleneck._fold)
        xn = x.permute(0, 2, 3, 1)                                   # [B, H, W, cin], contiguous
        h = core.linear_residual(None, xn, f["w1"], f["b1"])
        h = core.conv_igemm_nhwc(h, f["w2"], f["b2"], 3, 1, relu_in=True, relu_out=True)
        if self.stride == 2:
            h, xn = core.avgpool2_nhwc(h), core.avgpool2_nhwc(xn)
        res = xn if self.downsample is None else core.linear_residual(None, xn, f["wd"], f["bd"])
        return core.linear_residual(res, h, f["w3"], f["b3"], relu=True).permute(0, 3, 1, 2)

    def _fold(self):
        f = {}
        f["w1"], f["b1"] = _fold_conv(self.conv1, self.bn1, "gemm")
        f["w2"], f["b2"] = _fold_conv(self.conv2, self.bn2, "igemm")
        f["w3"], f["b3"] = _fold_conv(self.conv3, self.bn3, "gemm")
        if self.downsample is not None:
            f["wd"], f["bd"] = _fold_conv(self.downsample[1], self.downsample[2], "gemm")    # children: "-1", "0", "1"
        return f


class AttentionPool2d(nn.Module):
    """CLIP's pooling head: the pixels of [B, C, H, W] become H*W tokens, their mean is put in front as the query token,
    a position embedding is added, and one multi-head attention (separate q / k / v projections, output projection
    c_proj) is read at the query token: [B, output_dim]."""

    def __init__(self, side, embed_dim, num_heads, output_dim=None):
        """side: pixels along one edge of the pooled map (side * side + 1 position rows).  The parameters are registered
        in the order of OpenAI's state dict: positional_embedding, k_proj, q_proj, v_proj, c_proj."""
        super().__init__()
        tokens = side * side + 1
        self.positional_embedding = nn.Parameter(torch.empty(tokens, embed_dim).normal_(std=embed_dim ** -0.5))
        for name in ("k_proj", "q_proj", "v_proj"):
            setattr(self, name, nn.Linear(embed_dim, embed_dim))
        self.c_proj = nn.Linear(embed_dim, embed_dim if output_dim is None else output_dim)
        self.embed_dim, self.num_heads = embed_dim, num_heads

    def forward(self, x):
        if clip_rn_route(self, x) == "hip":
            return self._forward_hip(x)
        B, C = x.shape[:2]
        t = x.flatten(2).transpose(1, 2)                             # [B, HW, C]
        t = torch.cat([t.mean(dim=1, keepdim=True), t], dim=1) + self.positional_embedding.to(t.dtype)
        T, hd = t.shape[1], C // self.num_heads
        # only the query token's output is read: its row of the attention is all that is computed
        q = self.q_proj(t[:, :1]).view(B, 1, self.num_heads, hd).transpose(1, 2)
        k = self.k_proj(t).view(B, T, self.num_heads, hd).transpose(1, 2)
        v = self.v_proj(t).view(B, T, self.num_heads, hd).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v)                  # softmax(q k^T / sqrt(hd)) v
        return self.c_proj(o.transpose(1, 2).reshape(B, C))

    def _forward_hip(self, x):
        """K21 builds the tokens from the channels-last pixels; one GEMM of all B*T tokens against cat(k_proj, v_proj)
        gives [B, T, 2, heads, 64]; q_proj runs on the query rows alone (a row-strided GEMM operand); K9C (its / 8 is the
        q scaling at head width 64); c_proj."""
        wkv, bkv = _folded(self, _ATTNPOOL_SKIPPED, AttentionPool2d._fold)
        B = x.shape[0]
        tok = core.attnpool_tokens(x.permute(0, 2, 3, 1), self.positional_embedding.detach())      # [B, T, C]
        kv = core.linear_residual(None, tok, wkv, bkv).view(B, tok.shape[1], 2, self.num_heads, 64)
        q = core.linear_residual(None, tok[:, 0], self.q_proj.weight, self.q_proj.bias)
        return core.linear_residual(None, _attend_cls(q, kv), self.c_proj.weight, self.c_proj.bias)      # K9C, c_proj

    def _fold(self):
        return (torch.cat([self.k_proj.weight.detach(), self.v_proj.weight.detach()]).contiguous(),
                torch.cat([self.k_proj.bias.detach(), self.v_proj.bias.detach()]).contiguous())


class ModifiedResNet(nn.Module):
    """CLIP's ResNet: a stem of three 3x3 convolutions (the first of stride 2) and a 2x2 average pooling instead of
    7x7 / 2 + max pooling, anti-aliased stride-2 blocks (_ClipBottleneck), and an attention pool instead of the mean.
    Hook points: layer1..4 (4-D) and attnpool ([B, output_dim])."""

    def __init__(self, layers, output_dim, heads, input_resolution=224, width=64):
        super().__init__()
        self.output_dim, self.input_resolution = output_dim, input_resolution
        self.conv1 = nn.Conv2d(3, width // 2, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.conv2 = nn.Conv2d(width // 2, width // 2, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.conv3 = nn.Conv2d(width // 2, width, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.avgpool = nn.AvgPool2d(2)
        cin = width
        for i, (n, s) in enumerate(zip(layers, (1, 2, 2, 2)), 1):
            blocks = []
            for j in range(n):
                blocks.append(_ClipBottleneck(cin, width << (i - 1), s if j == 0 else 1))
                cin = (width << (i - 1)) * _ClipBottleneck.expansion
            setattr(self, "layer%d" % i, _Stage(*blocks))
        self.attnpool = AttentionPool2d(input_resolution // 32, cin, heads, output_dim)

    def forward(self, x):
        x = x.to(self.conv1.weight.dtype)
        if clip_rn_route(self, x) == "hip":
            x = self._stem_hip(x)
        else:
            x = self.stem(x)
            if _tower_gate(HIP_CLIP_RN, self, x):                    # a hooked stem took ATen: the blocks need not
                x = x.contiguous(memory_format=torch.channels_last)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))     # _Stage keeps the memory channels-last
        return self.attnpool(x)

    def stem(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        return self.avgpool(F.relu(self.bn3(self.conv3(x))))

    def _stem_hip(self, x):
        """K19 (conv1 + folded bn1 + ReLU, NCHW image -> channels-last), K18 twice (conv2, conv3: 3x3 / 1, folded BN,
        ReLU on the way out), K20.  Returns [B, width, H/4, W/4] in channels_last memory."""
        f = _folded(self, _CLIP_STEM_SKIPPED, ModifiedResNet._fold_stem)
        h = core.conv3x3s2_nhwc(x, f["w1"], f["b1"], relu=True)
        h = core.conv_igemm_nhwc(h, f["w2"], f["b2"], 3, 1, relu_out=True)
        h = core.conv_igemm_nhwc(h, f["w3"], f["b3"], 3, 1, relu_out=True)
        return core.avgpool2_nhwc(h).permute(0, 3, 1, 2)

    def _fold_stem(self):
        f = {}
        f["w1"], f["b1"] = _fold_conv(self.conv1, self.bn1, "tap")
        f["w2"], f["b2"] = _fold_conv(self.conv2, self.bn2, "igemm")
        f["w3"], f["b3"] = _fold_conv(self.conv3, self.bn3, "igemm")
        return f


class ClipResNet(nn.Module):
    """OpenAI-CLIP RN50 / RN101 shaped dissector/target: hook points visual.layer1..4 and visual.attnpool; the text side
    as ClipViT's (width 512, 8 heads), projected to the image tower's embed_dim."""

    def __init__(self, layers, embed_dim, image_size=224, width=64, text_depth=12):
        super().__init__()
        self.embed_dim = embed_dim
        self.visual = ModifiedResNet(layers, embed_dim, width * 32 // 64, image_size, width)
        self.text_model = TextTower(vocab=49408, dim=512, heads=8, mlp=2048, depth=text_depth, max_pos=77)
        self.text_projection = nn.Linear(512, embed_dim, bias=False)

    def encode_image(self, image):
        return self.visual(image)

    def encode_text(self, tokens):
        f = self.text_model(tokens)
        eos = tokens["attention_mask"].sum(dim=-1) - 1
        return self.text_projection(f[torch.arange(f.shape[0], device=f.device), eos])

    def forward(self, image):
        return self.encode_image(image)


# name -> (layers, embed_dim): reference concept_vit/clip/model.py:258-266 with OpenAI's RN50 / RN101 configurations
CLIP_RESNETS = {"clip_rn50": ((3, 4, 6, 3), 1024), "clip_rn101": ((3, 4, 23, 3), 512)}


# ------------------------------------------------------------------------------------------------------
# OpenAI CLIP itself: the reference's concept_vit/clip/model.py CLIP (:239-383) restated under OpenAI's own parameter
# names, so that a real state dict loads strictly, and its byte-pair tokenizer (simple_tokenizer.py, clip.py:196-232)
# ------------------------------------------------------------------------------------------------------
_CLIP_BLOCK_SKIPPED = ("ln_1", "attn", "mlp", "ln_2")
_CLIP_IGNORED = ("input_resolution", "context_length", "vocab_size")       # scalars of OpenAI's archives; build_model deletes them


def clip_tower_route(flag, on_gpu, dtype, grad, training, B, T, D, heads, fused_ok):
    """'hip' when a tower of OpenAIClip may leave ATen for a call of B sequences of T tokens of width D: HIP_CLIP_TEXT
    (`flag`) on, fp32 on the GPU without autograd (_hip_eligible), eval mode, D = 64 * heads (the head width of K9, K9A
    and K9L), a width K10 takes, a token count one of the attention kernels takes, at most MAX_BATCH sequences, and
    the fused-residual GEMMs available for the call (`fused_ok`: every projection is one).  Otherwise 'aten'.  Hooks are
    looked at per block: one with a hook inside runs its ATen modules."""
    ok = (flag and _hip_eligible(on_gpu, dtype, grad) and not training and D == 64 * heads and D % 4 == 0 and D <= 2048
          and 1 <= T <= core.VIT_ATTENTION_LONG_MAX_T and _under_2g(T * 3 * D) and 1 <= B <= MAX_BATCH and fused_ok)
    return "hip" if ok else "aten"


def quick_gelu(x):
    """x * sigmoid(1.702 x) on ATen (model.py:162-164): three launches on the GPU; the HIP route calls K25 instead."""
    return x * torch.sigmoid(1.702 * x)


class _QuickGELU(nn.Module):
    def forward(self, x):
        return quick_gelu(x)


class _ClipMHA(nn.Module):
    """The parameters of nn.MultiheadAttention under its names (in_proj_weight, in_proj_bias, out_proj.*), batch first,
    self-attention only; forward is the ATen route: one projection, SDPA (is_causal for the text side), out_proj."""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = nn.Linear(dim, dim)

    def forward(self, x, causal=False):
        B, T, D = x.shape
        q, k, v = F.linear(x, self.in_proj_weight, self.in_proj_bias).view(B, T, 3, self.heads, D // self.heads).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=causal)
        return self.out_proj(o.transpose(1, 2).reshape(B, T, D))


class _ClipResBlock(nn.Module):
    """ResidualAttentionBlock (model.py:167-188), pre-norm: x1 = x + attn(ln_1(x)), out = x1 + c_proj(QuickGELU(c_fc(ln_2(x1)))).
    causal: the text transformer's mask (model.py:324-330), query t sees keys 0 .. t."""

    def __init__(self, dim, heads, causal=False):
        super().__init__()
        self.causal = causal
        self.attn = _ClipMHA(dim, heads)
        self.ln_1 = nn.LayerNorm(dim)
        self.mlp = nn.Sequential()
        self.mlp.add_module("c_fc", nn.Linear(dim, 4 * dim))
        self.mlp.add_module("gelu", _QuickGELU())
        self.mlp.add_module("c_proj", nn.Linear(4 * dim, dim))
        self.ln_2 = nn.LayerNorm(dim)

    def forward(self, x, hip=False, cls_only=False):
        """hip: the tower has checked clip_tower_route; the block takes the HIP route unless a hook sits inside it.
        cls_only (the tower has checked cls_tail_route as well): the class-token row alone, as [B, 1, D]."""
        if hip and not _hooks_on(self, _CLIP_BLOCK_SKIPPED):
            attn = "causal" if self.causal else "k9" if x.shape[1] <= core.VIT_ATTENTION_MAX_T else "long"   # K9A, K9, K9L
            return _block_hip(self._ops(), x, attn, act=_quick_gelu_, cls_only=cls_only)
        x = x + self.attn(self.ln_1(x), self.causal)
        return x + self.mlp(self.ln_2(x))

    def _ops(self):
        a, m = self.attn, self.mlp
        return _BlockOps(_ln_ops(self.ln_1), _ln_ops(self.ln_2), (a.in_proj_weight, a.in_proj_bias), _lin_ops(a.out_proj),
                         _lin_ops(m.c_fc), _lin_ops(m.c_proj), a.heads, a)


class _ClipTransformer(nn.Module):
    def __init__(self, width, layers, heads, causal=False):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.ModuleList([_ClipResBlock(width, heads, causal) for _ in range(layers)])

    def forward(self, x, hip=False, cls_only=False):
        """Each block through __call__, so that its hooks fire; cls_only prunes the last one to its class-token row."""
        for i, blk in enumerate(self.resblocks):
            x = blk(x, hip, cls_only and i == len(self.resblocks) - 1)
        return x


class _ClipVisionTransformer(nn.Module):
    """VisionTransformer (model.py:202-236): a patch convolution WITHOUT bias, class_embedding, positional_embedding,
    ln_pre, the blocks, ln_post on the class-token row, @ proj.  Returns [B, output_dim]."""

    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.output_dim = input_resolution, output_dim
        self.conv1 = nn.Conv2d(3, width, patch_size, patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = _ClipTransformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def route(self, x):
        P = self.conv1.kernel_size[0]
        n = self.positional_embedding.shape[0]
        heads = self.transformer.resblocks[0].attn.heads if len(self.transformer.resblocks) else 0
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_contiguous()
                and embed_gate(P, x.shape[2], x.shape[3], n)):
            return "aten"
        return clip_tower_route(HIP_CLIP_TEXT, x.is_cuda, x.dtype, torch.is_grad_enabled(), self.training, x.shape[0], n,
                                self.conv1.out_channels, heads, _fused_residual_ok(x))

    def forward(self, x):
        x = x.to(self.conv1.weight.dtype)
        if self.route(x) == "hip":
            return self._forward_hip(x)
        x = self.conv1(x).flatten(2).transpose(1, 2)
        x = torch.cat([self.class_embedding.expand(x.shape[0], 1, -1), x], dim=1) + self.positional_embedding
        x = self.transformer(self.ln_pre(x))
        return self.ln_post(x[:, 0]) @ self.proj

    def _forward_hip(self, x):
        B = x.shape[0]
        P = self.conv1.kernel_size[0]
        # K11 + one GEMM without a bias term: the rows of patch pixels (a zero row in the class-token slot) times the conv
        # weight, plus a residual operand that holds the position table with class_embedding + its row 0 in row 0
        t = core.linear_residual(self._embed_residual(B), core.patchify(x, P), self.conv1.weight.view(self.conv1.out_channels, -1))
        if _hooked(self.ln_pre) or _nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks:
            t = self.ln_pre(t)
        else:
            t = core.layer_norm(t, self.ln_pre.weight, self.ln_pre.bias, self.ln_pre.eps)               # K10
        # nothing reads any row of the last block but the class token's: this forward slices it, the package's hooks declare it
        t = self.transformer(t, True, _cls_tail_ok(t, self.transformer.resblocks, self.transformer))
        row = t[:, 0].contiguous()
        if _hooked(self.ln_post):
            return self.ln_post(row) @ self.proj
        return core.layer_norm(row, self.ln_post.weight, self.ln_post.bias, self.ln_post.eps) @ self.proj

    def _embed_residual(self, B):
        return _folded(self, ("positional_embedding", "class_embedding"), lambda m: _class_pos_residual(
            m.positional_embedding, m.class_embedding, None, B), extra=(B,))


def openai_clip_config(sd):
    """OpenAIClip's constructor arguments read from the shapes of an OpenAI CLIP state dict, as the reference's build_model
    does (model.py:410-433): a ViT when the state dict has visual.proj, else a ModifiedResNet; heads = width // 64."""
    def shape(key):
        if key not in sd:
            raise RuntimeError("not an OpenAI CLIP state dict: it lacks %r" % (key,))
        return tuple(sd[key].shape)
    if "visual.proj" in sd:
        width, _, patch, _ = shape("visual.conv1.weight")
        layers = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
        grid = round((shape("visual.positional_embedding")[0] - 1) ** 0.5)
        resolution = patch * grid
    else:
        layers = tuple(len(set(k.split(".")[2] for k in sd if k.startswith("visual.layer%d." % b))) for b in (1, 2, 3, 4))
        width = shape("visual.layer1.0.conv1.weight")[0]
        side = round((shape("visual.attnpool.positional_embedding")[0] - 1) ** 0.5)
        if side * side + 1 != shape("visual.attnpool.positional_embedding")[0]:
            raise RuntimeError("visual.attnpool.positional_embedding has %d rows: not a square grid plus one"
                               % shape("visual.attnpool.positional_embedding")[0])
        patch, resolution = None, side * 32
    t_width = shape("ln_final.weight")[0]
    return dict(embed_dim=shape("text_projection")[1], image_resolution=resolution, vision_layers=layers, vision_width=width,
                vision_patch_size=patch, context_length=shape("positional_embedding")[0],
                vocab_size=shape("token_embedding.weight")[0], transformer_width=t_width, transformer_heads=t_width // 64,
                transformer_layers=len(set(k.split(".")[2] for k in sd if k.startswith("transformer.resblocks."))))


VIT_B16 = dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=16,
               context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12)


class OpenAIClip(nn.Module):
    """OpenAI CLIP as the reference's clip.load builds it (model.py:239-383), under OpenAI's parameter names: visual.*
    (a _ClipVisionTransformer, or the ModifiedResNet of the RN dissectors when vision_layers is a tuple), transformer.*,
    token_embedding, positional_embedding, ln_final, text_projection, logit_scale.  The default arguments are ViT-B/16's.

    encode_image(image) -> [B, embed_dim]; encode_text(tokens) -> [B, embed_dim] for a plain int64 [B, context_length]
    tensor of token ids (ClipBPETokenizer's output: the end-of-text id is the largest of a row, so argmax finds it);
    forward(image) = encode_image, as ClipViT's.  Hook points: visual.transformer.resblocks[i] and
    transformer.resblocks[i].  Block outputs are [B, T, D], batch first as everywhere in this project -- the reference's
    blocks see [T, B, D].  Computes in fp32 (fp16 checkpoints are upcast on load: clip.load(device="cpu") does the same).

    The HIP route (HIP_CLIP_TEXT, clip_tower_route): per block K10, the fused qkv GEMM, K9A (text: causal) or K9 / K9L
    (image), the two residual GEMMs and K25 behind c_fc; the image side embeds through K11 + one GEMM and prunes its last
    block to the class-token row (cls_tail_route, K9C)."""

    def __init__(self, embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=16,
                 context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12,
                 vision_heads=None):
        super().__init__()
        self.context_length, self.vocab_size, self.embed_dim = context_length, vocab_size, embed_dim
        if isinstance(vision_layers, (tuple, list)):
            self.visual = ModifiedResNet(tuple(vision_layers), embed_dim, vision_width * 32 // 64, image_resolution, vision_width)
        else:
            self.visual = _ClipVisionTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                                 vision_heads or vision_width // 64, embed_dim)
        self.transformer = _ClipTransformer(transformer_width, transformer_layers, transformer_heads, causal=True)
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.tokenizer = None                       # resolved at tokenize(): the registered merges file or an error
        self._init_parameters()

    def _init_parameters(self):
        """Seeded stand-in weights at the scales CLIP trains from (model.py:295-322), for a model built without a checkpoint."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        towers = [self.transformer] + ([self.visual.transformer] if isinstance(self.visual, _ClipVisionTransformer) else [])
        for tr in towers:
            for blk in tr.resblocks:
                nn.init.normal_(blk.attn.in_proj_weight, std=tr.width ** -0.5)
                nn.init.normal_(blk.attn.out_proj.weight, std=tr.width ** -0.5 * (2 * tr.layers) ** -0.5)
                nn.init.normal_(blk.mlp.c_fc.weight, std=(2 * tr.width) ** -0.5)
                nn.init.normal_(blk.mlp.c_proj.weight, std=tr.width ** -0.5 * (2 * tr.layers) ** -0.5)
        nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    @classmethod
    def from_state_dict(cls, sd, **heads):
        """The model of an OpenAI CLIP state dict: the configuration from its shapes (openai_clip_config), the three
        scalar keys input_resolution / context_length / vocab_size ignored by name, floating tensors upcast to fp32, and
        a STRICT load: a missing or an unexpected key is an error, never a tower of random weights.  heads:
        vision_heads= / transformer_heads= of a ViT CLIP whose head counts are known (a snapshot's config.json) in place
        of width // 64."""
        sd = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()
              if k not in _CLIP_IGNORED}
        model = cls(**dict(openai_clip_config(sd), **heads))
        model.load_state_dict(sd, strict=True)
        return model

    def text_route(self, tokens):
        """clip_tower_route for the text side on the ids `tokens` [B, T]; K9A takes up to core.VIT_ATTENTION_MAX_T tokens."""
        w = self.token_embedding.weight
        B, T = tokens.shape
        if T > core.VIT_ATTENTION_MAX_T or not self.transformer.layers:
            return "aten"
        return clip_tower_route(HIP_CLIP_TEXT, w.is_cuda and tokens.is_cuda, w.dtype, torch.is_grad_enabled(), self.training,
                                B, T, w.shape[1], self.transformer.resblocks[0].attn.heads,
                                FUSED_RESIDUAL and core.linear_residual_available())

    def encode_image(self, image):
        return self.visual(image)

    def encode_text(self, tokens):
        if isinstance(tokens, dict) or tokens.dim() != 2 or tokens.dtype != torch.int64:
            raise ValueError("OpenAIClip.encode_text takes an int64 [B, context_length] tensor of token ids")
        if tokens.shape[1] > self.context_length:
            raise ValueError("%d tokens, the position table has %d rows" % (tokens.shape[1], self.context_length))
        x = self.token_embedding(tokens) + self.positional_embedding[:tokens.shape[1]]
        x = self.transformer(x, self.text_route(tokens) == "hip")
        # the end-of-text row (the largest id of a sequence), THEN ln_final on those B rows: LayerNorm is per row
        x = x[torch.arange(x.shape[0], device=x.device), tokens.argmax(dim=-1)]
        return self.ln_final(x) @ self.text_projection

    def forward(self, image):
        return self.encode_image(image)

    def tokenize(self, texts, truncate=False):
        """clip.tokenize at this model's context length, with the registered merges file (register_tokenizer('clip', path)
        or MCD_CLIP_BPE); without one an error -- never the hashing stand-in."""
        if self.tokenizer is None:
            self.tokenizer = clip_tokenizer()
        tok = self.tokenizer(texts, context_length=self.context_length, truncate=truncate)
        if tok.numel() and int(tok.max()) >= self.vocab_size:
            raise ValueError("the merges file gives token id %d, the checkpoint's embedding table has %d rows: this is not "
                             "the merges file of the checkpoint's tokenizer" % (int(tok.max()), self.vocab_size))
        return tok


# the White_Space property: what \s of the reference's pattern (the `regex` package, a str pattern) matches
_UNICODE_SPACE = frozenset("\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a"
                           "\u2028\u2029\u202f\u205f\u3000")
_CLIP_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")  # in the pattern's order
_CLIP_SOT, _CLIP_EOT = "<|startoftext|>", "<|endoftext|>"


def _clip_byte_table():
    """byte -> the printable character that stands for it in the merges file (GPT-2's table): the printable Latin-1 bytes
    are themselves, the other 68 take the code points from 256 up, in byte order."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table = {b: chr(b) for b in keep}
    spare = 256
    for b in range(256):
        if b not in table:
            table[b] = chr(spare)
            spare += 1
    return keep + [b for b in range(256) if b not in set(keep)], table


class ClipBPETokenizer:
    """OpenAI CLIP's tokenizer restated in pure Python (standard library + torch; neither `regex` nor `ftfy`): the
    reference's SimpleTokenizer (concept_vit/clip/simple_tokenizer.py) and clip.tokenize (clip.py:196-232), from a local
    merges file in bpe_simple_vocab_16e6.txt format, plain or gzipped.

      1. clean: html.unescape twice, strip, every run of white space becomes one space, strip, lower-case;
      2. split: at each position the first that applies of -- one of the two special strings; one of the contractions
         's 't 're 've 'm 'll 'd; a run of letters (category L*); ONE number character (N*); a run of anything that is
         neither white space, letter nor number -- a scanner over unicodedata categories for the reference's pattern;
      3. each piece: its UTF-8 bytes through the byte table, the last character marked </w>, then the lowest-ranked
         adjacent pair is merged, all its occurrences at once, until no pair of the word has a rank;
      4. start id + ids + end id, zero padding to context_length; longer: RuntimeError, or with truncate=True cut to
         context_length with the end id last.
    Vocabulary: the 256 byte characters, the same with </w>, one entry per merge -- lines [1 : 49152 - 256 - 2 + 1] of the
    file, the reference's slice -- then the two specials, whose ids are read from the vocabulary that results: a shorter
    merges file gives a consistent smaller vocabulary, and the end-of-text id is always the largest.
    Not restated: ftfy.fix_text in front of step 1 (mojibake repair) -- text is taken as given."""

    MAX_MERGES = 49152 - 256 - 2

    def __init__(self, bpe_path):
        with open(bpe_path, "rb") as f:
            raw = f.read()
        if raw[:2] == b"\x1f\x8b":
            import gzip
            raw = gzip.decompress(raw)
        lines = raw.decode("utf-8").split("\n")[1:self.MAX_MERGES + 1]
        merges = [tuple(line.split()) for line in lines]        # (an empty line is the entry '' here as in the reference)
        bad = [i + 2 for i, m in enumerate(merges) if len(m) not in (0, 2)]
        if bad or not any(merges):
            raise ValueError("%r is not a BPE merges file: line %s is not a pair of symbols" % (bpe_path, bad[0] if bad else 2))
        order, self.byte_table = _clip_byte_table()
        vocab = [self.byte_table[b] for b in order]
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + [_CLIP_SOT, _CLIP_EOT]
        self.encoder = {}
        for i, v in enumerate(vocab):
            self.encoder[v] = i                    # a repeated entry keeps its last id, as the reference's dict(zip()) does
        self.vocab_size = len(vocab)
        self.ranks = {}
        for i, m in enumerate(merges):
            self.ranks[m] = i
        self.sot_id, self.eot_id = self.encoder[_CLIP_SOT], self.encoder[_CLIP_EOT]
        self._cache = {}

    @staticmethod
    def clean(text):
        import html
        text = html.unescape(html.unescape(text)).strip()
        out, gap = [], False
        for ch in text:
            if ch in _UNICODE_SPACE:
                gap = True
                continue
            if gap and out:
                out.append(" ")
            gap = False
            out.append(ch)
        return "".join(out).lower()

    @staticmethod
    def split(text):
        pieces, i, n = [], 0, len(text)
        while i < n:
            ch = text[i]
            special = next((s for s in (_CLIP_SOT, _CLIP_EOT) + _CLIP_CONTRACTIONS if text.startswith(s, i)), None)
            if special is not None:
                pieces.append(special)
                i += len(special)
                continue
            kind = unicodedata.category(ch)[0]
            if kind == "N":
                pieces.append(ch)
                i += 1
                continue
            if ch in _UNICODE_SPACE:
                i += 1
                continue
            j = i + 1
            if kind == "L":
                while j < n and unicodedata.category(text[j])[0] == "L":
                    j += 1
            else:
                while j < n and text[j] not in _UNICODE_SPACE and unicodedata.category(text[j])[0] not in "LN":
                    j += 1
            pieces.append(text[i:j])
            i = j
        return pieces

    def bpe(self, piece):
        """The ids of one piece of the split."""
        if piece in self._cache:
            return self._cache[piece]
        if piece in (_CLIP_SOT, _CLIP_EOT):
            ids = [self.encoder[piece]]
        else:
            word = [self.byte_table[b] for b in piece.encode("utf-8")]
            word[-1] += "</w>"
            while len(word) > 1:
                best = min(zip(word, word[1:]), key=lambda p: self.ranks.get(p, float("inf")))
                if best not in self.ranks:
                    break
                merged, k = [], 0
                while k < len(word):
                    if k + 1 < len(word) and (word[k], word[k + 1]) == best:
                        merged.append(word[k] + word[k + 1])
                        k += 2
                    else:
                        merged.append(word[k])
                        k += 1
                word = merged
            ids = [self.encoder[w] for w in word]
        self._cache[piece] = ids
        return ids

    def encode(self, text):
        return [i for piece in self.split(self.clean(text)) for i in self.bpe(piece)]

    def __call__(self, texts, context_length=77, truncate=False):
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.long)
        for r, text in enumerate(texts):
            ids = [self.sot_id] + self.encode(text) + [self.eot_id]
            if len(ids) > context_length:
                if not truncate:
                    raise RuntimeError("Input %s is too long for context length %d" % (text, context_length))
                ids = ids[:context_length]
                ids[-1] = self.eot_id
            out[r, :len(ids)] = torch.tensor(ids, dtype=torch.long)
        return out


def clip_tokenizer():
    """The ClipBPETokenizer of the registered merges file; without one an error -- never the hashing stand-in, whose ids
    would address arbitrary rows of a real embedding table."""
    entry = TOKENIZER_VOCABS.get("clip")
    path = entry[0] if entry is not None else os.environ.get("MCD_CLIP_BPE")
    if not path:
        raise RuntimeError("OpenAI CLIP's text tower needs its BPE merges file: call data_utils.register_tokenizer('clip', "
                           "'/path/bpe_simple_vocab_16e6.txt.gz') or set MCD_CLIP_BPE=/path/bpe_simple_vocab_16e6.txt.gz; "
                           "there is no fallback to the hashing tokenizer")
    return ClipBPETokenizer(path)


# --clip_model name (or any name) -> a LOCAL OpenAI CLIP checkpoint, like register_dataset for probe sets
CLIP_CHECKPOINTS = {}


def register_clip_checkpoint(name, path):
    """Where the OpenAI CLIP checkpoint of --clip_model `name` lives (a state dict file or OpenAI's TorchScript archive).
    The environment variable MCD_CLIP_CKPTS='ViT-B/16=/path/a.pt,RN50=/path/b.pt' does the same for a process that
    registers nothing."""
    CLIP_CHECKPOINTS[name] = path


def clip_checkpoint(name):
    """The registered checkpoint path of `name`, or None."""
    if name in CLIP_CHECKPOINTS:
        return CLIP_CHECKPOINTS[name]
    for item in os.environ.get("MCD_CLIP_CKPTS", "").split(","):
        key, sep, path = item.partition("=")
        if sep and key.strip() == name:
            return path.strip()
    return None


def _is_torchscript_archive(path):
    """A zip with TorchScript's code/ folder and constants.pkl beside data.pkl: what torch.jit.save writes and OpenAI
    distributes; torch.save writes neither."""
    import zipfile
    if not zipfile.is_zipfile(path):
        return False
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
    return any(n.endswith("/constants.pkl") for n in names) and any("/code/" in n for n in names)


def openai_clip_state_dict(ckpt):
    """ckpt: a state dict, or a LOCAL path to one (read with weights_only=True), to a .safetensors file or a snapshot
    directory (checkpoint_io.resolve_checkpoint), or to a TorchScript archive, whose state_dict() is taken as clip.load
    does (clip.py:126-138; loading such an archive unpickles its code).  A transformers CLIPModel state dict comes back
    as it is: get_target_model('openai_clip') renames it (hf_clip_to_openai)."""
    if isinstance(ckpt, str):
        if os.path.isfile(ckpt) and _is_torchscript_archive(ckpt):
            return dict(torch.jit.load(ckpt, map_location="cpu").state_dict())
        ckpt = checkpoint_io.resolve_checkpoint(ckpt).state_dict()
    return ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt and "text_projection" not in ckpt else ckpt


# ------------------------------------------------------------------------------------------------------
# The HF `clip` target: transformers' CLIPForImageClassification (the reference's MODELS["clip"] =
# "openai/clip-vit-base-patch16" behind AutoModelForImageClassification, data_utils.py:21-36, :63-69) under its own names
# ------------------------------------------------------------------------------------------------------
# HFClip's inference route (clip_tower_route): K11 + one GEMM for the embedding, K10 for pre_layrnorm, per layer K10, the
# fused qkv GEMM, K9 / K9L, the two residual GEMMs and K25 behind fc1, K26 for the mean of the patch tokens, one GEMM for the
# classifier.  MCD_NO_HIP_HF_CLIP=1 (or setting this to False) keeps the ATen route of the same modules.
HIP_HF_CLIP = os.environ.get("MCD_NO_HIP_HF_CLIP", "0") != "1"
HF_CLIP_KEY = "vision_model.embeddings.class_embedding"      # what tells a CLIPForImageClassification state dict
_HF_CLIP_LAYER_SKIPPED = ("self_attn", "layer_norm1", "mlp", "layer_norm2")
# what a hub CLIPModel file carries beside the vision tower and from_pretrained drops for this class; older files store the
# position_ids buffer
_HF_CLIP_IGNORED = ("vision_model.embeddings.position_ids", "text_model.", "visual_projection.", "text_projection.",
                    "logit_scale")


class _HFClipEmbeddings(nn.Module):
    """CLIPVisionEmbeddings: class_embedding [D], patch_embedding (a convolution WITHOUT bias), position_embedding (an
    nn.Embedding of 1 + grid^2 rows).  No interpolation: an image of another patch grid is a ValueError."""

    def __init__(self, dim, image_size, patch):
        super().__init__()
        self.image_size, self.patch_size = image_size, patch
        self.class_embedding = nn.Parameter(torch.randn(dim))
        self.patch_embedding = nn.Conv2d(3, dim, patch, patch, bias=False)
        self.position_embedding = nn.Embedding((image_size // patch) ** 2 + 1, dim)

    def check(self, x):
        if x.dim() != 4 or tuple(x.shape[2:]) != (self.image_size, self.image_size):
            raise ValueError("Input image size (%s) doesn't match model (%d*%d)."
                             % ("*".join(str(s) for s in x.shape[2:]), self.image_size, self.image_size))

    def forward(self, x):
        self.check(x)
        t = self.patch_embedding(x.to(self.patch_embedding.weight.dtype)).flatten(2).transpose(1, 2)
        return torch.cat([self.class_embedding.expand(t.shape[0], 1, -1), t], dim=1) + self.position_embedding.weight


class _HFClipAttention(nn.Module):
    """CLIPAttention: k_proj, v_proj, q_proj, out_proj as four nn.Linear (each a hook point); forward is the ATen route."""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.k_proj = nn.Linear(dim, dim)
        self.v_proj = nn.Linear(dim, dim)
        self.q_proj = nn.Linear(dim, dim)
        self.out_proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, T, D = x.shape
        q, k, v = (p(x).view(B, T, self.heads, D // self.heads).transpose(1, 2) for p in (self.q_proj, self.k_proj, self.v_proj))
        return self.out_proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, D))

    def fused_qkv(self):
        """([3D, D], [3D]): the three projections as the one GEMM the attention kernels read, cached until a parameter of
        one of them is replaced or written."""
        return _folded(self, ("q_proj", "k_proj", "v_proj"), lambda m: (
            torch.cat([m.q_proj.weight, m.k_proj.weight, m.v_proj.weight]).contiguous(),
            torch.cat([m.q_proj.bias, m.k_proj.bias, m.v_proj.bias]).contiguous()))


class _HFClipMLP(nn.Module):
    def __init__(self, dim, mlp, hidden_act):
        super().__init__()
        self.activation_fn = _QuickGELU() if hidden_act == "quick_gelu" else nn.GELU()
        self.fc1 = nn.Linear(dim, mlp)
        self.fc2 = nn.Linear(mlp, dim)

    def forward(self, x):
        return self.fc2(self.activation_fn(self.fc1(x)))


class _HFClipLayer(nn.Module):
    """CLIPEncoderLayer, pre-norm: x1 = x + self_attn(layer_norm1(x)), out = x1 + mlp(layer_norm2(x1)).  Returns the
    hidden-state tensor."""

    def __init__(self, dim, heads, mlp, hidden_act, eps=1e-5):
        super().__init__()
        self.self_attn = _HFClipAttention(dim, heads)
        self.layer_norm1 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _HFClipMLP(dim, mlp, hidden_act)
        self.layer_norm2 = nn.LayerNorm(dim, eps=eps)

    def forward(self, x, hip=False):
        """hip: the model has checked clip_tower_route; the layer takes the HIP route unless a hook sits inside it."""
        if hip and not _hooks_on(self, _HF_CLIP_LAYER_SKIPPED):
            attn = "k9" if x.shape[1] <= core.VIT_ATTENTION_MAX_T else "long"                     # K9, K9L
            act = _quick_gelu_ if isinstance(self.mlp.activation_fn, _QuickGELU) else _gelu         # K25, or ATen's erf GELU
            return _block_hip(self._ops(), x, attn, act=act)
        x = x + self.self_attn(self.layer_norm1(x))
        return x + self.mlp(self.layer_norm2(x))

    def _ops(self):
        a, m = self.self_attn, self.mlp
        return _BlockOps(_ln_ops(self.layer_norm1), _ln_ops(self.layer_norm2), a.fused_qkv(), _lin_ops(a.out_proj),
                         _lin_ops(m.fc1), _lin_ops(m.fc2), a.heads)


class _HFClipEncoder(nn.Module):
    def __init__(self, depth, dim, heads, mlp, hidden_act, eps=1e-5):
        super().__init__()
        self.layers = nn.ModuleList([_HFClipLayer(dim, heads, mlp, hidden_act, eps) for _ in range(depth)])

    def forward(self, x, hip=False):
        for layer in self.layers:                    # through __call__: the hooks on layers[i] fire
            x = layer(x, hip)
        return x


class _HFClipVisionTransformer(nn.Module):
    """CLIPVisionTransformer: embeddings, pre_layrnorm (transformers' spelling), encoder, post_layernorm.  forward returns
    last_hidden_state [B, T, D], which has NOT gone through post_layernorm.  transformers applies that module to the class
    token for pooler_output, and CLIPForImageClassification discards the result; here it holds its parameters and is not
    computed at all, so a hook on vision_model.post_layernorm fires in transformers and never here."""

    def __init__(self, dim, image_size, patch, depth, heads, mlp, hidden_act, eps=1e-5):
        super().__init__()
        self.embeddings = _HFClipEmbeddings(dim, image_size, patch)
        self.pre_layrnorm = nn.LayerNorm(dim, eps=eps)
        self.encoder = _HFClipEncoder(depth, dim, heads, mlp, hidden_act, eps)
        self.post_layernorm = nn.LayerNorm(dim, eps=eps)

    def forward(self, x, hip=False):
        if not hip:
            return self.encoder(self.pre_layrnorm(self.embeddings(x)))
        emb, ln = self.embeddings, self.pre_layrnorm
        unhooked = not (_nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks)
        if unhooked and not _hooked(emb):
            # K11 + one GEMM without a bias term, the position table with class_embedding + its row 0 as the residual operand
            w = emb.patch_embedding.weight
            t = core.linear_residual(self._embed_residual(x.shape[0]), core.patchify(x, emb.patch_size), w.view(w.shape[0], -1))
        else:
            t = emb(x)
        t = core.layer_norm(t, ln.weight, ln.bias, ln.eps) if unhooked and not _hooked(ln) else ln(t)       # K10
        return self.encoder(t, True)

    def _embed_residual(self, B):
        # (a copy of the table goes in: for B = 1 _class_pos_residual's expand(1, ..).contiguous() is a view of its operand,
        # and row 0 is then written in place)
        return _folded(self.embeddings, ("position_embedding", "class_embedding"), lambda m: _class_pos_residual(
            m.position_embedding.weight.detach().clone(), m.class_embedding, None, B), extra=(B,))


def hf_clip_config(sd, heads=None):
    """HFClip's constructor arguments read from the shapes of a CLIPForImageClassification state dict: the width from
    class_embedding, the patch from patch_embedding.weight, the grid (and with it the resolution) from the position rows,
    the depth by counting layers, the MLP width from fc1, num_labels from classifier.weight when the file has one (else the
    key is absent: the caller decides).  The state dict does not carry the head count: every OpenAI vision tower has
    64-wide heads, so heads = width // 64 unless `heads` says otherwise."""
    def shape(key):
        if key not in sd:
            raise RuntimeError("not a CLIPForImageClassification state dict: it lacks %r" % (key,))
        return tuple(sd[key].shape)
    hidden = shape(HF_CLIP_KEY)[0]
    patch = shape("vision_model.embeddings.patch_embedding.weight")[2]
    rows = shape("vision_model.embeddings.position_embedding.weight")[0]
    grid = round((rows - 1) ** 0.5)
    if grid * grid + 1 != rows:
        raise RuntimeError("vision_model.embeddings.position_embedding.weight has %d rows: not a square grid plus one" % rows)
    layers = len([k for k in sd if k.startswith("vision_model.encoder.layers.") and k.endswith(".self_attn.q_proj.weight")])
    cfg = dict(image_size=grid * patch, patch=patch, hidden=hidden, layers=layers, heads=heads or hidden // 64,
               mlp=shape("vision_model.encoder.layers.0.mlp.fc1.weight")[0] if layers else 4 * hidden)
    if "classifier.weight" in sd:
        cfg["num_labels"] = shape("classifier.weight")[0]
    return cfg


class HFClip(nn.Module):
    """transformers' CLIPForImageClassification under transformers' own module and parameter names, so that a real state
    dict loads strictly: vision_model.embeddings.{class_embedding, patch_embedding (no bias), position_embedding},
    vision_model.pre_layrnorm, vision_model.encoder.layers[i].{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2,
    mlp.{fc1, fc2}}, vision_model.post_layernorm, classifier.  The defaults are openai/clip-vit-base-patch16's.

    forward(images) -> the logits tensor [B, num_labels] (encode_image is the same call): the patch convolution, the class
    embedding in front, + the position table, pre_layrnorm, the pre-norm layers (QuickGELU for hidden_act 'quick_gelu', erf
    GELU for 'gelu'; LayerNorm eps `eps`, CLIPVisionConfig's layer_norm_eps, 1e-5 by default), then the mean of
    last_hidden_state[:, 1:] -- last_hidden_state does not pass post_layernorm, whose parameters are loaded and whose result nothing reads (transformers computes it for pooler_output
    and this class discards it; here it is not computed) -- and the classifier.
    Hook points: vision_model.encoder.layers[i] and every module under it.  A layer returns its hidden-state tensor
    [B, T, D]: so does transformers 5.x; transformers 4.41.1, the reference's pin, returns a 1-tuple, which the reference's
    'avg' hook unwraps (utils.get_activation does the same), so both read the same rows.

    The HIP route (HIP_HF_CLIP, clip_tower_route): K11 + one GEMM, K10, per layer _block_hip on the concatenated q / k / v
    projection with K9 / K9L and K25, K26 for the mean, one GEMM for the classifier.  The head reads every token, so the
    last layer always runs whole.  A layer with a hook on a module inside it runs its ATen modules for that call."""

    def __init__(self, num_labels=2, image_size=224, patch=16, hidden=768, layers=12, heads=12, mlp=3072,
                 hidden_act="quick_gelu", eps=1e-5):
        super().__init__()
        if hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError("hidden_act must be 'quick_gelu' or 'gelu', got %r" % (hidden_act,))
        if not isinstance(image_size, int):
            raise ValueError("HFClip: image_size must be an int (the position table is a square grid), got %r" % (image_size,))
        self.heads = heads
        self.vision_model = _HFClipVisionTransformer(hidden, image_size, patch, layers, heads, mlp, hidden_act, eps)
        self.classifier = nn.Linear(hidden, num_labels)

    @classmethod
    def from_state_dict(cls, sd, n_class=None, heads=None, hidden_act="quick_gelu", eps=1e-5):
        """The model of a CLIPForImageClassification (or hub CLIPModel) state dict: sized by hf_clip_config, fp16 tensors
        upcast, everything under vision_model. and classifier. loaded STRICTLY -- a missing or an unexpected key is an
        error, never a tower of random weights.  The names of _HF_CLIP_IGNORED are dropped, as from_pretrained drops them
        for this class.  A file without classifier.* keeps the freshly initialised head with n_class outputs (2 when
        None, transformers' default): what from_pretrained of the base checkpoint gives."""
        sd = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()
              if not k.startswith(_HF_CLIP_IGNORED)}
        cfg = hf_clip_config(sd, heads)
        cfg.setdefault("num_labels", 2 if n_class is None else n_class)
        model = cls(hidden_act=hidden_act, eps=eps, **cfg)
        want = set(model.state_dict())
        if not any(k.startswith("classifier.") for k in sd):
            want -= {"classifier.weight", "classifier.bias"}
        missing, unexpected = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or unexpected:
            raise RuntimeError("the checkpoint does not match CLIPForImageClassification: %d missing key(s) %s, %d unexpected "
                               "key(s) %s" % (len(missing), missing[:4], len(unexpected), unexpected[:4]))
        model.load_state_dict(sd, strict=False)          # (the key sets were compared above; shapes are checked here)
        return model

    def route(self, x):
        emb = self.vision_model.embeddings
        n = emb.position_embedding.weight.shape[0]
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_contiguous()
                and embed_gate(emb.patch_size, x.shape[2], x.shape[3], n)):
            return "aten"
        return clip_tower_route(HIP_HF_CLIP, x.is_cuda, x.dtype, torch.is_grad_enabled(), self.training, x.shape[0], n,
                                emb.patch_embedding.out_channels, self.heads, _fused_residual_ok(x))

    def forward(self, images):
        self.vision_model.embeddings.check(images)
        x = images.to(self.classifier.weight.dtype)
        hip = self.route(x) == "hip"
        t = self.vision_model(x, hip)
        if not hip:
            return self.classifier(torch.mean(t[:, 1:, :], dim=1))
        pooled = core.token_mean(t, 1)                                                               # K26
        if _hooked(self.classifier) or _nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks:
            return self.classifier(pooled)
        return _linear(self.classifier, pooled)

    def encode_image(self, image):
        return self(image)


# ------------------------------------------------------------------------------------------------------
# ViT-MAE (the `mae` row of the reference's MODELS table, data_utils.py:21-36 and :65-66: facebook/vit-mae-base behind
# AutoModelForPreTraining = transformers' ViTMAEForPreTraining)
# ------------------------------------------------------------------------------------------------------
# HFMae's inference route (HFMae.route): K28 (the kept patches' pixel rows) + one GEMM whose residual operand K29 gathers from
# the position table, _block_hip for every encoder layer, K10, the decoder_embed GEMM, K29 (mask-token fill, un-shuffle,
# position add), _block_hip for the decoder layers (SDPA inside at 32-wide heads), K10, the decoder_pred GEMM; the loss on
# ATen.  MCD_NO_HIP_MAE=1 (or setting this to False) keeps the modules' own forward: the convolution over all patches,
# gather, cat, repeat and the unfused blocks (whose LayerNorm and attention stay under HIP_LAYER_NORM / HIP_ATTENTION, as in
# HFViT).
HIP_MAE = os.environ.get("MCD_NO_HIP_MAE", "0") != "1"
MAE_KEYS = ("vit.embeddings.cls_token", "decoder.mask_token")      # what tells a ViTMAEForPreTraining state dict
MaeOutput = collections.namedtuple("MaeOutput", "loss logits mask ids_restore")


def _plain_call(mod, x):
    """mod(x) for an nn.Linear on the HIP route: through __call__ when a hook (the module's or a global one) must fire."""
    if _hooked(mod) or _nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks:
        return mod(x)
    return _linear(mod, x)


class _MaeLayer(_Block):
    """ViTMAELayer: _Block (pre-norm, LayerNorm eps 1e-12, exact GELU) whose caller decides the route.  hip=True: _Block's
    own choice (_block_hip unless a hook sits inside); hip=False: the submodules one by one."""

    def forward(self, x, hip=True):
        if hip:
            return super().forward(x)
        x = x + self.attn(self.norm1(x))
        return x + self.fc2(F.gelu(self.fc1(self.norm2(x))))


class _MaeEncoder(nn.Module):
    def __init__(self, depth, dim, heads, mlp, eps=1e-12):
        super().__init__()
        self.layer = nn.ModuleList([_MaeLayer(dim, heads, mlp, eps=eps) for _ in range(depth)])

    def forward(self, x, hip=False):
        for layer in self.layer:                     # through __call__: the hooks on layer[i] fire
            x = layer(x, hip)
        return x


class _MaeViT(nn.Module):
    """ViTMAEModel: embeddings (cls_token, position_embeddings, patch_embeddings.projection), encoder.layer[i], layernorm.
    forward(x, ids_keep) embeds the patches ids_keep [B, Lk] names, puts the class token in front and returns
    layernorm(encoder(.)) as [B, 1 + Lk, D]."""

    def __init__(self, dim, image_size, patch, depth, heads, mlp, eps=1e-12):
        super().__init__()
        self.image_size, self.patch = image_size, patch
        self.embeddings = _HFEmbeddings(dim, patch, (image_size // patch) ** 2)
        self.encoder = _MaeEncoder(depth, dim, heads, mlp, eps)
        self.layernorm = _LayerNorm(dim, eps=eps)

    def embed(self, x, ids_keep, hip=False):
        emb = self.embeddings
        conv, pos = emb.patch_embeddings.projection, emb.position_embeddings
        if hip and not _hooks_on(self, ("embeddings",)):
            # K28: the pixel rows of the kept patches alone (a zero row in the class-token slot); K29: their position rows
            # (and cls_token + position 0 - bias in row 0) out of one table; one GEMM with the bias and that residual operand
            keep = ids_keep.to(torch.int32).contiguous()
            res = core.token_restore(self._class_pos_table(), keep)
            return core.linear_residual(res, core.patchify_kept(x, self.patch, keep), conv.weight.view(conv.out_channels, -1),
                                        conv.bias, out=res)
        t = conv(x).flatten(2).transpose(1, 2) + pos[:, 1:]
        t = torch.gather(t, 1, ids_keep.unsqueeze(-1).expand(-1, -1, t.shape[2]))
        return torch.cat([(emb.cls_token + pos[:, :1]).expand(t.shape[0], -1, -1), t], dim=1)

    def _class_pos_table(self):
        """[1 + L, D]: a COPY of the position table with cls_token + its row 0 - bias in row 0 (the GEMM adds the bias
        back): the class/position trick of _class_pos_residual on one table for all images, which K29 then gathers."""
        def build(m):
            table = m.position_embeddings.detach()[0].clone()
            table[0] += m.cls_token.detach()[0, 0] - m.patch_embeddings.projection.bias.detach()
            return table
        return _folded(self.embeddings, ("position_embeddings", "cls_token", "patch_embeddings"), build)

    def forward(self, x, ids_keep, hip=False):
        return self.layernorm(self.encoder(self.embed(x, ids_keep, hip), hip))


class _MaeDecoder(nn.Module):
    """ViTMAEDecoder: decoder_embed, mask_token, decoder_pos_embed, decoder_layers[i], decoder_norm, decoder_pred.
    forward(latent [B, 1 + Lk, D], ids_restore [B, L]) -> the pixel predictions [B, L, patch^2 * 3] (the class row dropped)."""

    def __init__(self, dim, num_patches, width, depth, heads, mlp, out_dim, eps=1e-12):
        super().__init__()
        self.mask_token = nn.Parameter(torch.zeros(1, 1, width))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, width), requires_grad=False)
        self.decoder_embed = nn.Linear(dim, width)
        self.decoder_layers = nn.ModuleList([_MaeLayer(width, heads, mlp, eps=eps) for _ in range(depth)])
        self.decoder_norm = _LayerNorm(width, eps=eps)
        self.decoder_pred = nn.Linear(width, out_dim)

    def forward(self, latent, ids_restore, hip=False):
        if hip:
            # K29: mask tokens behind the kept rows, the un-shuffle, the class row in front and + decoder_pos_embed, one launch
            h = core.token_restore(_plain_call(self.decoder_embed, latent), ids_restore.to(torch.int32).contiguous(),
                                   self.mask_token.detach().view(-1), self.decoder_pos_embed.detach()[0])
        else:
            h = self.decoder_embed(latent)
            B, L = ids_restore.shape
            tokens = torch.cat([h[:, 1:], self.mask_token.repeat(B, L + 1 - h.shape[1], 1)], dim=1)
            tokens = torch.gather(tokens, 1, ids_restore.unsqueeze(-1).repeat(1, 1, h.shape[2]))
            h = torch.cat([h[:, :1], tokens], dim=1) + self.decoder_pos_embed
        for layer in self.decoder_layers:
            h = layer(h, hip)
        h = self.decoder_norm(h)
        return (_plain_call(self.decoder_pred, h) if hip else self.decoder_pred(h))[:, 1:]


def mae_config(sd, heads=None, decoder_heads=None):
    """HFMae's constructor arguments read from the shapes of a ViTMAEForPreTraining state dict (transformers-4.41.1 key
    names, or the mirror's own): the width from cls_token, the patch from the projection, the grid (and with it the
    resolution) from the position rows, the depths by counting layers, the MLP widths from the first layer, the decoder's
    width from mask_token.  The state dict does not carry the head counts: width // 64 for the encoder (every ViT-MAE
    encoder has 64-wide heads) and width // 32 for the decoder (facebook/vit-mae-base, -large and -huge: 16 heads on 512)
    unless `heads` / `decoder_heads` say otherwise."""
    def shape(*keys):
        for key in keys:
            if key in sd:
                return tuple(sd[key].shape)
        raise RuntimeError("not a ViTMAEForPreTraining state dict: it lacks %r" % (keys[0],))

    def depth(stem):
        return len([k for k in sd if k.startswith(stem) and k.endswith((".layernorm_before.weight", ".norm1.weight"))])
    hidden = shape(MAE_KEYS[0])[2]
    patch = shape("vit.embeddings.patch_embeddings.projection.weight")[2]
    rows = shape("vit.embeddings.position_embeddings")[1]
    grid = round((rows - 1) ** 0.5)
    if grid * grid + 1 != rows:
        raise RuntimeError("vit.embeddings.position_embeddings has %d rows: not a square grid plus one" % rows)
    if shape("decoder.decoder_pos_embed")[1] != rows:
        raise RuntimeError("decoder.decoder_pos_embed has %d rows, vit.embeddings.position_embeddings %d"
                           % (shape("decoder.decoder_pos_embed")[1], rows))
    width = shape(MAE_KEYS[1])[2]
    layers, dlayers = depth("vit.encoder.layer."), depth("decoder.decoder_layers.")
    return dict(image_size=grid * patch, patch=patch, hidden=hidden, layers=layers, heads=heads or max(1, hidden // 64),
                mlp=shape("vit.encoder.layer.0.intermediate.dense.weight", "vit.encoder.layer.0.fc1.weight")[0] if layers
                else 4 * hidden,
                decoder_hidden=width, decoder_layers=dlayers, decoder_heads=decoder_heads or max(1, width // 32),
                decoder_mlp=shape("decoder.decoder_layers.0.intermediate.dense.weight", "decoder.decoder_layers.0.fc1.weight")[0]
                if dlayers else 4 * width)


class HFMae(nn.Module):
    """transformers' ViTMAEForPreTraining (the reference's `mae` target, facebook/vit-mae-base; the defaults are its
    configuration).  Module tree: vit.embeddings.{cls_token, position_embeddings, patch_embeddings.projection},
    vit.encoder.layer[i], vit.layernorm, decoder.{mask_token, decoder_pos_embed, decoder_embed, decoder_layers[i],
    decoder_norm, decoder_pred}.  A layer is a _Block (attn.qkv, attn.proj, norm1, norm2, fc1, fc2); convert_state_dict maps
    the transformers-4.41.1 names of a real checkpoint (attention.attention.{query,key,value}, attention.output.dense,
    layernorm_before / after, intermediate.dense, output.dense) onto them and from_state_dict loads STRICTLY.  The two
    position tables are the fixed sin-cos tables the checkpoint stores; they are loaded, never regenerated.

    forward(pixel_values, noise=None) -> MaeOutput(loss, logits, mask, ids_restore), transformers' steps: the patch embedding
    + position_embeddings[:, 1:]; len_keep = int(L * (1 - mask_ratio)); ids_shuffle = argsort(noise), ids_restore =
    argsort(ids_shuffle); the first len_keep patches of the shuffle are kept; mask [B, L] is 0 on kept patches and 1 on
    removed ones, in patch order; cls_token + position_embeddings[:, :1] in front; the encoder layers; vit.layernorm;
    decoder_embed; L - len_keep mask tokens appended behind the kept rows and gathered by ids_restore; the class row back in
    front; + decoder_pos_embed; the decoder layers; decoder_norm; decoder_pred; the class row dropped; loss = the mean
    squared error per patch against patchify(pixel_values) ((dy, dx, c) order; per-patch normalised under norm_pix_loss),
    averaged over the removed patches.  noise=None draws torch.rand(B, L, device=...) from torch's global generator, as
    transformers does: the mask of a dissection run is random unless the caller seeds torch.
    Hook points: vit.encoder.layer[i]; an output is [B, 1 + len_keep, D] and a dissection hook reads token 0.  vit.layernorm
    and the decoder read every row: the last block always runs whole.  encode_image is forward."""

    def __init__(self, image_size=224, patch=16, hidden=768, layers=12, heads=12, mlp=3072, decoder_hidden=512,
                 decoder_layers=8, decoder_heads=16, decoder_mlp=2048, mask_ratio=0.75, norm_pix_loss=False, eps=1e-12):
        super().__init__()
        if not isinstance(image_size, int):
            raise ValueError("HFMae: image_size must be an int (the position table is a square grid), got %r" % (image_size,))
        self.mask_ratio, self.norm_pix_loss = float(mask_ratio), bool(norm_pix_loss)
        self.num_patches = (image_size // patch) ** 2
        self.vit = _MaeViT(hidden, image_size, patch, layers, heads, mlp, eps)
        self.decoder = _MaeDecoder(hidden, self.num_patches, decoder_hidden, decoder_layers, decoder_heads, decoder_mlp,
                                   patch * patch * 3, eps)

    def convert_state_dict(self, sd):
        sd = hf_state_dict(sd, "vit", len(self.vit.encoder.layer))
        return hf_state_dict(sd, "decoder", len(self.decoder.decoder_layers), stem="decoder_layers")

    @classmethod
    def from_state_dict(cls, sd, heads=None, decoder_heads=None, mask_ratio=0.75, norm_pix_loss=False, eps=1e-12):
        """The model of a ViTMAEForPreTraining state dict: sized by mae_config, fp16 tensors upcast, loaded STRICTLY -- a
        missing or an unexpected key is an error, never a tower of random weights."""
        sd = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}
        model = cls(mask_ratio=mask_ratio, norm_pix_loss=norm_pix_loss, eps=eps, **mae_config(sd, heads, decoder_heads))
        sd = model.convert_state_dict(sd)
        want = set(model.state_dict())
        missing, unexpected = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or unexpected:
            raise RuntimeError("the checkpoint does not match ViTMAEForPreTraining: %d missing key(s) %s, %d unexpected "
                               "key(s) %s" % (len(missing), missing[:4], len(unexpected), unexpected[:4]))
        model.load_state_dict(sd, strict=True)
        return model

    def patchify(self, x):
        """[B, 3, H, W] -> [B, L, patch^2 * 3], a patch's pixels in transformers' (dy, dx, c) order."""
        B, C, P = x.shape[0], x.shape[1], self.vit.patch
        g = x.shape[2] // P
        return x.reshape(B, C, g, P, g, P).permute(0, 2, 4, 3, 5, 1).reshape(B, g * g, P * P * C)

    def route(self, x):
        v, d = self.vit, self.decoder
        conv = v.embeddings.patch_embeddings.projection
        ok = (_tower_gate(HIP_MAE, self, x) and x.shape[0] >= 1 and x.is_contiguous() and x.shape[1] == conv.in_channels
              and conv.bias is not None
              and embed_gate(v.patch, x.shape[2], x.shape[3], v.embeddings.position_embeddings.shape[1])
              and conv.out_channels % 4 == 0 and d.decoder_embed.out_features % 4 == 0
              and _under_2g(x.shape[1] * x.shape[2] * x.shape[3],
                            (1 + self.num_patches) * max(conv.out_channels, d.decoder_embed.out_features,
                                                         conv.weight[0].numel())))
        return "hip" if ok else "aten"

    def forward(self, pixel_values, noise=None):
        size = self.vit.image_size
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[2:]) != (size, size):
            raise ValueError("Input image size (%s) doesn't match model (%d*%d)."
                             % ("*".join(str(s) for s in pixel_values.shape[2:]), size, size))
        x = pixel_values.to(self.vit.embeddings.cls_token.dtype)
        B, L = x.shape[0], self.num_patches
        len_keep = int(L * (1 - self.mask_ratio))
        if noise is None:
            noise = torch.rand(B, L, device=x.device)
        ids_shuffle = torch.argsort(noise, dim=1).to(x.device)
        ids_restore = torch.argsort(ids_shuffle, dim=1)
        mask = (ids_restore >= len_keep).to(torch.get_default_dtype())      # the 0 / 1 row of the shuffle, gathered by ids_restore
        hip = self.route(x) == "hip"
        latent = self.vit(x, ids_shuffle[:, :len_keep], hip)
        logits = self.decoder(latent, ids_restore, hip)
        target = self.patchify(x)
        if self.norm_pix_loss:
            target = (target - target.mean(dim=-1, keepdim=True)) / (target.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5
        loss = ((logits - target) ** 2).mean(dim=-1)
        return MaeOutput((loss * mask).sum() / mask.sum(), logits, mask, ids_restore)

    def encode_image(self, image, noise=None):
        return self(image, noise)


# ------------------------------------------------------------------------------------------------------
# The Swin image tower (reference model/modules/image_encoder.py:27-28, :50-52: `source: huggingface, model_type: swin`,
# transformers.SwinModel, last_hidden_state) under transformers-4.41.1's names, pooler excluded (nothing reads it)
# ------------------------------------------------------------------------------------------------------
# SwinTower's inference route (swin_route): per block K10, the fused q|k|v GEMM, K31 (the attention inside shifted windows:
# padding, roll, partition, bias, mask, softmax, P.V, reverse in one launch), the two residual GEMMs and ATen's erf GELU
# (_block_hip with the 'window' attention); per stage end K32 (the 2x2 gather under LayerNorm) and the reduction GEMM.  A
# block whose window holds more than 64 tokens or whose heads are not 32 wide keeps ATen for its attention alone; a merge
# wider than K32 takes (4C > 2048: Swin-L's last) is ATen's.  The 4x4 patch convolution stays ATen's.  MCD_NO_HIP_SWIN=1
# (or setting this to False) keeps the ATen route of the same modules: pad, roll, view / permute, bmm, softmax, bmm.
HIP_SWIN = os.environ.get("MCD_NO_HIP_SWIN", "0") != "1"
SWIN_KEY = "embeddings.patch_embeddings.projection.weight"     # what tells a SwinModel state dict (under its prefix)
SWIN_MASK = -100.0                                             # transformers' shift-mask value: not -inf
SWIN_TINY = dict(patch=4, width=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), window=7, mlp_ratio=4.0)   # microsoft/swin-tiny-patch4-window7-224
_SWIN_LAYER_SKIPPED = ("layernorm_before", "attention", "layernorm_after", "intermediate", "output")
_SWIN_MERGE_SKIPPED = ("norm", "reduction")
_SWIN_IGNORED = "attention.self.relative_position_index"       # a buffer of index arithmetic: recomputed, never loaded


def swin_route(flag, on_gpu, dtype, grad, training, fused_ok, B):
    """'hip' when a SwinTower forward may leave ATen: HIP_SWIN (`flag`), the base gate (fp32 on the GPU, no autograd), eval
    mode, the fused-residual path available for the call (`fused_ok`) and a batch K31's grid takes; 'aten' otherwise."""
    ok = flag and _hip_eligible(on_gpu, dtype, grad) and not training and fused_ok and 1 <= B <= MAX_BATCH
    return "hip" if ok else "aten"


def swin_attention_route(window, dim, heads, tokens):
    """Which attention a block on the HIP route takes: 'window' (K31) for a window of at most 64 tokens, heads 32 wide and
    one image's qkv under 2^31 bytes; 'window-aten' (the same operands through ATen) otherwise."""
    ok = (1 <= window <= core.WINDOW_ATTENTION_MAX_W and dim == core.WINDOW_ATTENTION_HEAD * heads and heads <= MAX_BATCH
          and _under_2g(tokens * 3 * dim))
    return "window" if ok else "window-aten"


def swin_merge_route(dim, tokens):
    """'k32' when a stage's patch merging fits K32 (C a multiple of 4, 4C within K10's 2 048, an image under 2^31 bytes);
    'aten' otherwise (Swin-L's last merge)."""
    return "k32" if dim % 4 == 0 and dim <= core.PATCH_MERGE_MAX_C and _under_2g(tokens * dim) else "aten"


def swin_window_shift(H, W, window, shift):
    """(window, shift) of a block on an H x W grid: transformers' set_shift_and_window_size -- a grid whose smaller side is
    no larger than the window takes that side as its window and no shift.  The bias table has (2 * window - 1)^2 rows for
    the checkpoint's window, so a grid under it cannot be served: ValueError."""
    if min(H, W) < window:
        raise ValueError("SwinTower: a %dx%d token grid is smaller than the window %d its relative-position table was "
                         "built for" % (H, W, window))
    return (window, 0) if min(H, W) == window else (window, shift)


def swin_bias_index(window, device=None):
    """[w^2, w^2] int64: the row of relative_position_bias_table for query (i, j) and key (i', j'),
    (i - i' + w - 1)(2w - 1) + (j - j' + w - 1) -- transformers' relative_position_index."""
    c = torch.arange(window, device=device)
    i, j = (t.reshape(-1) for t in torch.meshgrid(c, c, indexing="ij"))
    return (i[:, None] - i[None, :] + window - 1) * (2 * window - 1) + (j[:, None] - j[None, :] + window - 1)


def swin_shift_mask(Hp, Wp, window, shift, dtype, device=None):
    """None without a shift, else [nW, w^2, w^2]: SWIN_MASK where two tokens of a window lie in different regions of the
    rolled Hp x Wp grid -- rows (and columns) fall in region 0, 1 or 2 below Hp - w, below Hp - s, or past it -- else 0."""
    if shift <= 0:
        return None
    r, c = torch.arange(Hp, device=device), torch.arange(Wp, device=device)
    region = (3 * ((r >= Hp - window).long() + (r >= Hp - shift).long())[:, None]
              + ((c >= Wp - window).long() + (c >= Wp - shift).long())[None, :])
    region = _window_partition(region[None, :, :, None], window).view(-1, window * window)
    return (region[:, None, :] != region[:, :, None]).to(dtype) * SWIN_MASK


def _window_partition(x, w):
    """[B, Hp, Wp, C] -> [B * nW, w * w, C], windows in row-major order, tokens of a window in row-major order."""
    B, Hp, Wp, C = x.shape
    return x.view(B, Hp // w, w, Wp // w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w, C)


def _window_reverse(x, w, Hp, Wp):
    """_window_partition's inverse: [B * nW, w * w, C] -> [B, Hp, Wp, C]."""
    C = x.shape[-1]
    return x.view(-1, Hp // w, Wp // w, w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, Hp, Wp, C)


def _window_softmax_pv(q, k, v, heads, table, window, mask):
    """softmax(q k^T / sqrt(head width) + bias + mask) v for windows q, k, v [B * nW, w^2, C] -> [B * nW, w^2, C]: the
    bias gathered from table [(2w-1)^2, heads], mask None or swin_shift_mask's [nW, w^2, w^2] (windows of one image
    adjacent)."""
    N, T, C = q.shape
    q, k, v = (t.reshape(N, T, heads, C // heads).transpose(1, 2) for t in (q, k, v))
    scores = q @ k.transpose(-1, -2) / math.sqrt(C // heads)
    scores = scores + table[swin_bias_index(window, table.device).view(-1)].view(T, T, heads).permute(2, 0, 1)[None]
    if mask is not None:
        nW = mask.shape[0]
        scores = (scores.view(N // nW, nW, heads, T, T) + mask[None, :, None]).view(N, heads, T, T)
    return (torch.softmax(scores, dim=-1) @ v).transpose(1, 2).reshape(N, T, C)


def _window_attend_aten(qkv, heads, grid, window, shift, table, pad_qkv):
    """core.window_attention's operands through ATen: qkv [B, H*W, 3C] in token order -> [B, H*W, C].  The padded tokens
    take pad_qkv, as in K31."""
    B, T, C3 = qkv.shape
    H, W = grid
    Hp, Wp = -(-H // window) * window, -(-W // window) * window
    x = qkv.view(B, H, W, C3)
    if (Hp, Wp) != (H, W):
        full = pad_qkv.detach().expand(B, Hp, Wp, C3).clone()
        full[:, :H, :W] = x
        x = full
    if shift > 0:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    q, k, v = _window_partition(x, window).chunk(3, dim=-1)
    o = _window_softmax_pv(q, k, v, heads, table, window, swin_shift_mask(Hp, Wp, window, shift, qkv.dtype, qkv.device))
    o = _window_reverse(o, window, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o[:, :H, :W].reshape(B, T, C3 // 3)


class _SwinSelfAttention(nn.Module):
    """SwinSelfAttention: query, key, value and relative_position_bias_table [(2w-1)^2, heads]."""

    def __init__(self, dim, heads, window):
        super().__init__()
        if dim % heads:
            raise ValueError("SwinTower: width %d is not a multiple of %d heads" % (dim, heads))
        self.heads, self.window = heads, window
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))
        self.query = nn.Linear(dim, dim)
        self.key = nn.Linear(dim, dim)
        self.value = nn.Linear(dim, dim)

    def forward(self, x, mask=None):
        """x [B * nW, w^2, C], the windows; mask None or [nW, w^2, w^2]."""
        return _window_softmax_pv(self.query(x), self.key(x), self.value(x), self.heads, self.relative_position_bias_table,
                                  self.window, mask)

    def fused_qkv(self):
        """(weight [3 C, C], bias [3 C]) of query | key | value as ONE projection -- the [B, T, 3, heads, 32] operand K31
        reads, and its bias the q | k | v of a padded (zero) token -- concatenated once (_folded)."""
        return _folded(self, ("query", "key", "value"),
                       lambda m: (torch.cat([m.query.weight, m.key.weight, m.value.weight]).contiguous(),
                                  torch.cat([m.query.bias, m.key.bias, m.value.bias]).contiguous()))


class _SwinDense(nn.Module):
    """SwinSelfOutput / SwinOutput: one Linear named dense (dropout is the identity at inference)."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.dense = nn.Linear(in_dim, out_dim)

    def forward(self, x):
        return self.dense(x)


class _SwinAttention(nn.Module):
    def __init__(self, dim, heads, window):
        super().__init__()
        setattr(self, "self", _SwinSelfAttention(dim, heads, window))
        self.output = _SwinDense(dim, dim)

    def forward(self, x, mask=None):
        return self.output(getattr(self, "self")(x, mask))


class _SwinLayer(nn.Module):
    """SwinLayer, pre-norm: x1 = x + proj(window attention(layernorm_before(x))), out = x1 + fc2(gelu(fc1(layernorm_after(x1)))).
    forward(x [B, H*W, C], grid (H, W), hip) -> [B, H*W, C], a plain tensor (transformers returns a tuple around it)."""

    def __init__(self, dim, heads, window, shift, mlp, eps):
        super().__init__()
        self.window, self.shift = window, shift
        self.layernorm_before = _LayerNorm(dim, eps=eps)
        self.attention = _SwinAttention(dim, heads, window)
        self.layernorm_after = _LayerNorm(dim, eps=eps)
        self.intermediate = _BertIntermediate(dim, mlp)
        self.output = _SwinDense(mlp, dim)

    def forward(self, x, grid, hip=False):
        B, T, C = x.shape
        H, W = grid
        w, s = swin_window_shift(H, W, self.window, self.shift)
        att = getattr(self.attention, "self")
        if hip and not _hooks_on(self, _SWIN_LAYER_SKIPPED):
            wqkv, bqkv = att.fused_qkv()
            ops = _BlockOps(_ln_ops(self.layernorm_before), _ln_ops(self.layernorm_after), (wqkv, bqkv),
                            _lin_ops(self.attention.output.dense), _lin_ops(self.intermediate.dense),
                            _lin_ops(self.output.dense), att.heads)
            arg = ((H, W), w, s, att.relative_position_bias_table.detach(), bqkv)
            return _block_hip(ops, x, swin_attention_route(w, C, att.heads, T), arg,
                              k10=HIP_LAYER_NORM and C % 4 == 0 and C <= 2048)
        # ATen, transformers' own steps; every submodule through __call__, so that a hook inside fires
        h = self.layernorm_before(x).view(B, H, W, C)
        Hp, Wp = -(-H // w) * w, -(-W // w) * w
        h = F.pad(h, (0, 0, 0, Wp - W, 0, Hp - H))         # zeros AFTER the norm: a padded token's q, k, v are the biases
        if s > 0:
            h = torch.roll(h, (-s, -s), (1, 2))
        a = self.attention(_window_partition(h, w), swin_shift_mask(Hp, Wp, w, s, x.dtype, x.device))
        a = _window_reverse(a, w, Hp, Wp)
        if s > 0:
            a = torch.roll(a, (s, s), (1, 2))
        x = x + a[:, :H, :W].reshape(B, T, C)
        return x + self.output(self.intermediate(self.layernorm_after(x)))


class _SwinPatchMerging(nn.Module):
    """SwinPatchMerging: the 2x2 neighbours of the (zero-padded to even sizes) grid side by side -- (0,0), (1,0), (0,1),
    (1,1) in (row, column) offsets --, norm = LayerNorm(4C), reduction = Linear(4C, 2C) without a bias."""

    def __init__(self, dim, eps):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = _LayerNorm(4 * dim, eps=eps)

    def forward(self, x, grid, hip=False):
        B, T, C = x.shape
        H, W = grid
        if hip and swin_merge_route(C, T) == "k32" and not _hooks_on(self, _SWIN_MERGE_SKIPPED):
            n = core.patch_merge_ln(x.contiguous(), (H, W), self.norm.weight, self.norm.bias, self.norm.eps)       # K32
            return core.linear_residual(None, n, self.reduction.weight, None)
        x = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)
        return self.reduction(self.norm(x.view(B, -1, 4 * C)))


class _SwinStage(nn.Module):
    """SwinStage: blocks[j] (shift 0 on even j, window // 2 on odd j) and downsample (None on the last stage).
    forward -> the stage's output AFTER downsampling, [B, ceil(H/2)*ceil(W/2), 2C], a plain tensor."""

    def __init__(self, dim, depth, heads, window, mlp, eps, downsample):
        super().__init__()
        self.blocks = nn.ModuleList([_SwinLayer(dim, heads, window, 0 if j % 2 == 0 else window // 2, mlp, eps)
                                     for j in range(depth)])
        self.downsample = _SwinPatchMerging(dim, eps) if downsample else None

    def forward(self, x, grid, hip=False):
        for blk in self.blocks:                      # through __call__: the hooks on blocks[j] fire
            x = blk(x, grid, hip)
        return x if self.downsample is None else self.downsample(x, grid, hip)


class _SwinEncoder(nn.Module):
    def __init__(self, width, depths, heads, windows, mlp_ratio, eps):
        super().__init__()
        self.layers = nn.ModuleList([_SwinStage(width << i, depths[i], heads[i], windows[i], int(mlp_ratio * (width << i)), eps,
                                                i < len(depths) - 1) for i in range(len(depths))])

    def forward(self, x, grid, hip=False):
        for stage in self.layers:
            x = stage(x, grid, hip)
            if stage.downsample is not None:
                grid = ((grid[0] + 1) // 2, (grid[1] + 1) // 2)
        return x


class _SwinEmbeddings(nn.Module):
    """SwinEmbeddings without absolute position embeddings and mask token: patch_embeddings.projection (a P x P
    convolution of stride P on the image zero-padded to whole patches) and norm."""

    def __init__(self, dim, patch, eps):
        super().__init__()
        self.patch = patch
        self.patch_embeddings = _PatchEmbeddings(dim, patch)
        self.norm = _LayerNorm(dim, eps=eps)

    def forward(self, x):
        P = self.patch
        x = self.patch_embeddings.projection(F.pad(x, (0, -x.shape[3] % P, 0, -x.shape[2] % P)))
        return self.norm(x.flatten(2).transpose(1, 2).contiguous()), (x.shape[2], x.shape[3])


class SwinTower(nn.Module):
    """transformers.SwinModel without its pooler: embeddings.{patch_embeddings.projection, norm},
    encoder.layers[i].blocks[j].{layernorm_before, attention.self.{query, key, value, relative_position_bias_table},
    attention.output.dense, layernorm_after, intermediate.dense, output.dense}, encoder.layers[i].downsample.{norm,
    reduction}, layernorm -- the state-dict keys of transformers 4.41.1, the reference's pin.  forward(image [B, 3, H, W]) ->
    last_hidden_state [B, T, out_dim] at any image size (the grid is padded per block, as transformers pads it).  The
    defaults are microsoft/swin-tiny-patch4-window7-224.  window: one int, or one per stage.  Hook points:
    encoder.layers[i] and encoder.layers[i].blocks[j]; every output is a plain [B, T, C] tensor and a dissection hook reads
    token 0 of it, as the reference does for a 3-D output."""

    def __init__(self, patch=4, width=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), window=7, mlp_ratio=4.0, eps=1e-5):
        super().__init__()
        depths, heads = tuple(depths), tuple(heads)
        windows = (window,) * len(depths) if isinstance(window, int) else tuple(window)
        if not (len(depths) == len(heads) == len(windows) >= 1):
            raise ValueError("SwinTower: depths %s, heads %s and window %s must name the same stages" % (depths, heads, windows))
        self.config = dict(patch=patch, width=width, depths=depths, heads=heads, window=windows, mlp_ratio=mlp_ratio)
        self.out_dim = width << (len(depths) - 1)
        self.embeddings = _SwinEmbeddings(width, patch, eps)
        self.encoder = _SwinEncoder(width, depths, heads, windows, mlp_ratio, eps)
        self.layernorm = _LayerNorm(self.out_dim, eps=eps)

    def route(self, x):
        return swin_route(HIP_SWIN, x.is_cuda, x.dtype, torch.is_grad_enabled(), self.training, _fused_residual_ok(x),
                          x.shape[0])

    def forward(self, x):
        hip = x.dim() == 4 and self.route(x) == "hip"
        t, grid = self.embeddings(x)
        return self.layernorm(self.encoder(t, grid, hip))

    @staticmethod
    def config_from_state_dict(sd, prefix=""):
        """SwinTower's constructor arguments read from the shapes of a SwinModel state dict under `prefix`: patch and width
        from the projection, the depths by counting keys, per stage the heads from the bias table's columns and the window
        from its rows ((2w-1)^2), the MLP ratio from intermediate.dense."""
        def shape(name):
            if prefix + name not in sd:
                raise RuntimeError("not a SwinModel state dict: it lacks %r" % (prefix + name,))
            return tuple(sd[prefix + name].shape)
        for name in ("embeddings.position_embeddings", "embeddings.mask_token"):
            if prefix + name in sd:
                raise ValueError("SwinTower: the checkpoint has %r (absolute position embeddings / masked image modelling), "
                                 "which this tower does not build" % (prefix + name,))
        width, _, patch, _ = shape(SWIN_KEY)
        stem = prefix + "encoder.layers."
        blocks = {}
        for k in sd:
            if k.startswith(stem) and k.endswith(".layernorm_before.weight"):
                i, _, j = k[len(stem):].split(".")[:3]
                blocks[int(i)] = max(blocks.get(int(i), 0), int(j) + 1)
        if not blocks or sorted(blocks) != list(range(len(blocks))):
            raise RuntimeError("not a SwinModel state dict: stages %s under %r" % (sorted(blocks), stem))
        depths = tuple(blocks[i] for i in range(len(blocks)))
        heads, windows = [], []
        for i in range(len(depths)):
            rows, h = shape("encoder.layers.%d.blocks.0.attention.self.relative_position_bias_table" % i)
            w = (math.isqrt(rows) + 1) // 2
            if (2 * w - 1) ** 2 != rows:
                raise RuntimeError("stage %d: a relative-position table of %d rows is no (2w-1)^2" % (i, rows))
            heads.append(h)
            windows.append(w)
        return dict(patch=patch, width=width, depths=depths, heads=tuple(heads), window=tuple(windows),
                    mlp_ratio=shape("encoder.layers.0.blocks.0.intermediate.dense.weight")[0] / width)

    @classmethod
    def from_state_dict(cls, sd, prefix=""):
        """The tower of a SwinModel state dict (the keys under `prefix`): sized by config_from_state_dict, fp16 tensors
        upcast, loaded STRICTLY -- relative_position_index buffers and a pooler are ignored by name, any other missing or
        unexpected key is an error, never a tower of random weights."""
        cfg = cls.config_from_state_dict(sd, prefix)
        model = cls(**cfg)
        own = {k[len(prefix):]: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()
               if k.startswith(prefix) and not k.endswith(_SWIN_IGNORED) and not k[len(prefix):].startswith("pooler.")}
        model.load_state_dict(own, strict=True)
        return model


class HFImageEncoder(nn.Module):
    """The reference's HuggingfaceImageEncoder (model/modules/image_encoder.py:14-52) around a Swin tower: holds it as
    .image_encoder, so a Mammo-CLIP checkpoint's image_encoder.image_encoder.* keys load as they are; out_dim and
    model_type are the reference's names.  forward(image) -> last_hidden_state [B, T, out_dim]."""

    def __init__(self, tower):
        super().__init__()
        self.model_type = "swin"
        self.image_encoder = tower
        self.out_dim = tower.out_dim

    def forward(self, image):
        return self.image_encoder(image)


SWIN_PREFIX = "image_encoder.image_encoder."
# EfficientNet's compound scaling (Tan & Le 2019, table of the b0 .. b7 family): name -> (width, depth) coefficients
EFFICIENTNET_SCALING = {"b0": (1.0, 1.0), "b1": (1.0, 1.1), "b2": (1.1, 1.2), "b3": (1.2, 1.4), "b4": (1.4, 1.8),
                        "b5": (1.6, 2.2), "b6": (1.8, 2.6), "b7": (2.0, 3.1)}


def efficientnet_scaling(stem, head, blocks):
    """(name, width, depth) of the EfficientNet whose stem channels, head channels and block count these are; None when
    no member of the family matches."""
    for name, (width, depth) in EFFICIENTNET_SCALING.items():
        n = sum(int(math.ceil(depth * r)) for r, _, _, _, _ in EfficientNetB5Tower.STAGES)
        if (_round_filters(32, width), _round_filters(1280, width), n) == (stem, head, blocks):
            return name, width, depth
    return None


def image_tower_of(sd):
    """What image tower a BreastClip / BreastClipClassifier state dict carries: ('swin', SwinTower's configuration),
    ('cnn', dict(width=, depth=)), ('resnet', dict(layers=)) for the wrapped torchvision resnet50 / 101 / 152 (block counts
    read from the keys; any other counts are an error naming them), or None when it has no image_encoder.* key at all (a
    text-only or a head-only file).  Keys under image_encoder. that are none of these are an error naming what was found."""
    if SWIN_PREFIX + SWIN_KEY in sd:
        return "swin", SwinTower.config_from_state_dict(sd, SWIN_PREFIX)
    if "image_encoder._conv_stem.weight" in sd:
        stem = sd["image_encoder._conv_stem.weight"].shape[0]
        head = sd["image_encoder._conv_head.weight"].shape[0] if "image_encoder._conv_head.weight" in sd else -1
        stemk = "image_encoder._blocks."
        blocks = 1 + max([int(k[len(stemk):].split(".")[0]) for k in sd if k.startswith(stemk)], default=-1)
        found = efficientnet_scaling(stem, head, blocks)
        if found is None:
            raise ValueError("the checkpoint's image encoder is no EfficientNet b0 .. b7: stem %d, head %d channels, %d blocks"
                             % (stem, head, blocks))
        return "cnn", dict(width=found[1], depth=found[2])
    if RESNET_TOWER_KEY in sd:
        layers = resnet_tower_layers(sd)
        if layers not in RESNET_TOWER_LAYERS:
            raise ValueError("the checkpoint's image encoder is a ResNet with %s blocks in layer1..4: neither resnet50 "
                             "[3, 4, 6, 3], resnet101 [3, 4, 23, 3] nor resnet152 [3, 8, 36, 3]" % (layers,))
        return "resnet", dict(layers=layers)
    keys = sorted(k for k in sd if k.startswith("image_encoder."))
    if keys:
        raise ValueError("the checkpoint's image encoder is neither a Swin tower (%s*) nor an EfficientNet "
                         "(image_encoder._conv_stem.weight); its first keys: %s" % (SWIN_PREFIX + "embeddings.patch_embeddings.", keys[:4]))
    return None


# ------------------------------------------------------------------------------------------------------
# The sentence encoder of get_cos_similarity (reference concept_vit/utils.py:618-646: SentenceTransformer
# 'all-mpnet-base-v2'.encode): transformers.MPNetModel under its own names + sentence-transformers' Pooling(mean) + Normalize
# ------------------------------------------------------------------------------------------------------
# MPNetSentenceEncoder's inference route (sentence_route): the embedding rows on K24, per layer the fused qkv GEMM, K9B (K9M
# with the relative-position bias), the two residual GEMMs and K10 behind each (_block_hip, post-norm), then K27 (masked mean
# + L2 norm).  MCD_NO_HIP_SENTENCE=1 (or setting this to False) keeps the ATen route: SDPA under bias + key mask.
HIP_SENTENCE = os.environ.get("MCD_NO_HIP_SENTENCE", "0") != "1"
MPNET_MAX_TOKENS = 256            # encode() truncates here (K9B's limit; all-mpnet-base-v2's own max_seq_length is 384)
MPNET_PAD_ID = 1                  # MPNetEmbeddings.padding_idx: <pad>, and the base of the position ids
_MPNET_IGNORED = ("pooler.", "embeddings.position_ids")
_MPNET_EMB_SKIPPED = ("word_embeddings", "position_embeddings", "LayerNorm")
_MPNET_LAYER_SKIPPED = ("attention", "intermediate", "output")


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """MPNetEncoder.relative_position_bucket (bidirectional T5 buckets) on an int64 tensor of key-minus-query distances,
    with transformers' own torch operations: half the buckets per sign, the first half of each exact, the rest
    logarithmic up to max_distance."""
    n = -relative_position
    num_buckets //= 2
    ret = (n < 0).to(torch.long) * num_buckets
    n = torch.abs(n)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_if_large = max_exact + (
        torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, num_buckets - 1))
    return ret + torch.where(is_small, n, val_if_large)


def mpnet_position_ids(ids, padding_idx=MPNET_PAD_ID):
    """transformers' create_position_ids_from_input_ids: the k-th non-padding token of a row gets padding_idx + k (k from
    1), a padding token padding_idx.  Valid token t of a right-padded row: t + 2."""
    mask = ids.ne(padding_idx).int()
    return (torch.cumsum(mask, dim=1).type_as(mask) * mask).long() + padding_idx


def sentence_route(flag, on_gpu, dtype, grad, training, B, T, D, heads, pos_rows, fused_ok, prefix_mask):
    """'hip' when an MPNetSentenceEncoder call may leave ATen: HIP_SENTENCE (`flag`), fp32 weights and ids on the GPU without
    autograd (_hip_eligible), eval mode, D = 64 * heads (K9B's head width), 1 <= T <= core.VIT_ATTENTION_MAX_T with the
    T + 2 position rows K24 reads in the table, a width K10 / K24 / K27 take, the fused-residual library loaded
    (`fused_ok`), and `prefix_mask`: a right-padded attention mask (prefix_mask_lengths gave key counts), or no mask and
    no <pad> among the ids.  Only a prefix mask is a key count; and MPNet takes its position ids from ids != <pad>, not
    from the mask, so only in these two cases is the position row of every token a key attends to t + 2, which is what
    K24 is given.  Otherwise 'aten'.  A pure function."""
    ok = (flag and _hip_eligible(on_gpu, dtype, grad) and not training and D == 64 * heads
          and 1 <= T <= core.VIT_ATTENTION_MAX_T and T + MPNET_PAD_ID + 1 <= pos_rows and D % 4 == 0 and D <= 2048
          and 1 <= B <= MAX_BATCH and fused_ok and prefix_mask)
    return "hip" if ok else "aten"


class _MPNetEmbeddings(nn.Module):
    def __init__(self, vocab, hidden, max_pos, eps):
        super().__init__()
        self.word_embeddings = nn.Embedding(vocab, hidden, padding_idx=MPNET_PAD_ID)
        self.position_embeddings = nn.Embedding(max_pos, hidden, padding_idx=MPNET_PAD_ID)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)

    def forward(self, ids, hip=False):
        if hip and not _hooks_on(self, _MPNET_EMB_SKIPPED):
            # K24 with the position table entered two rows down and one zero type row: LayerNorm((word + 0) + pos[t + 2]).
            # A padded position gets row t + 2 where MPNetEmbeddings takes row 1 -- such rows are masked as keys and left
            # out of the mean, nothing reads them.
            n = self.LayerNorm
            zero = _folded(self, ("LayerNorm",), lambda m: torch.zeros_like(m.LayerNorm.weight)[None])
            return core.text_embed_ln(ids, None, self.word_embeddings.weight, self.position_embeddings.weight[MPNET_PAD_ID + 1:],
                                      zero, n.weight, n.bias, n.eps)
        return self.LayerNorm(self.word_embeddings(ids) + self.position_embeddings(mpnet_position_ids(ids)))


class _MPNetSelfAttention(nn.Module):
    """MPNetSelfAttention: q, k, v and the output projection o; the scores take an additive bias."""

    def __init__(self, hidden, heads):
        super().__init__()
        self.heads = heads
        self.q = nn.Linear(hidden, hidden)
        self.k = nn.Linear(hidden, hidden)
        self.v = nn.Linear(hidden, hidden)
        self.o = nn.Linear(hidden, hidden)

    def forward(self, x, bias=None):
        B, T, D = x.shape
        q, k, v = (m(x).view(B, T, self.heads, D // self.heads).transpose(1, 2) for m in (self.q, self.k, self.v))
        return self.o(F.scaled_dot_product_attention(q, k, v, attn_mask=bias).transpose(1, 2).reshape(B, T, D))

    def fused_qkv(self):
        """(weight [3 D, D], bias [3 D]) of q | k | v as ONE projection, the [B, T, 3, heads, 64] operand K9B reads."""
        return _folded(self, ("q", "k", "v"),
                       lambda m: (torch.cat([m.q.weight, m.k.weight, m.v.weight]).contiguous(),
                                  torch.cat([m.q.bias, m.k.bias, m.v.bias]).contiguous()))


class _MPNetAttention(nn.Module):
    def __init__(self, hidden, heads, eps):
        super().__init__()
        self.attn = _MPNetSelfAttention(hidden, heads)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)

    def forward(self, x, bias=None):
        return self.LayerNorm(self.attn(x, bias) + x)


class _MPNetLayer(nn.Module):
    """MPNetLayer, post-norm like BertLayer: x1 = LN(x + o(attention(x))), out = LN(x1 + fc2(gelu(fc1(x1))))."""

    def __init__(self, hidden, heads, mlp, eps):
        super().__init__()
        self.attention = _MPNetAttention(hidden, heads, eps)
        self.intermediate = _BertIntermediate(hidden, mlp)
        self.output = _BertAddNorm(mlp, hidden, eps)

    def forward(self, x, bias=None, lens=None, rel=None, hip=False):
        """bias: a callable that gives the additive [B or 1, heads, T, T] SDPA mask (position bias + key mask), built
        only if some layer takes ATen; hip (the encoder has checked sentence_route): K9B with lens (int32 [B] key counts,
        None = all T) and rel ([heads, 2T-1]) -- unless a hook sits inside this layer."""
        if hip and not _hooks_on(self, _MPNET_LAYER_SKIPPED):
            return _block_hip(self._ops(), x, "relbias", (lens, rel), post=True)                             # K9B
        x1 = self.attention(x, bias())
        return self.output(self.intermediate(x1), x1)

    def _ops(self):
        a, o = self.attention, self.output
        return _BlockOps(_ln_ops(a.LayerNorm), _ln_ops(o.LayerNorm), a.attn.fused_qkv(), _lin_ops(a.attn.o),
                         _lin_ops(self.intermediate.dense), _lin_ops(o.dense), a.attn.heads)


class _MPNetEncoder(nn.Module):
    def __init__(self, depth, hidden, heads, mlp, eps, buckets=32):
        super().__init__()
        self.layer = nn.ModuleList([_MPNetLayer(hidden, heads, mlp, eps) for _ in range(depth)])
        self.relative_attention_bias = nn.Embedding(buckets, heads)

    def rel_table(self, T):
        """[heads, 2T-1] on the weights' device: rel[h, d + T - 1] = relative_attention_bias[bucket(d), h] for the
        key-minus-query distances d = -(T-1) .. T-1 -- every diagonal of compute_position_bias's [heads, T, T] matrix,
        once.  Built once per T and kept on the module (again when the embedding's storage or version changes)."""
        w = self.relative_attention_bias.weight
        key = (w._version, w.data_ptr(), w.device, w.dtype)
        cache = self.__dict__.setdefault("_rel_cache", {})
        if cache.get("key") != key:
            cache.clear()
            cache["key"] = key
        if T not in cache:
            with torch.no_grad():
                d = torch.arange(-(T - 1), T, dtype=torch.long)
                bucket = relative_position_bucket(d, num_buckets=w.shape[0]).to(w.device)
                cache[T] = w.detach()[bucket].t().contiguous()
        return cache[T]

    def position_bias(self, T):
        """compute_position_bias as MPNetEncoder writes it: the buckets of the [T, T] distances on the host, the
        embedding lookup, [1, heads, T, T].  Entry (t, j) is rel_table(T)[:, (j - t) + T - 1]."""
        t = torch.arange(T, dtype=torch.long)
        bucket = relative_position_bucket(t[None, :] - t[:, None], num_buckets=self.relative_attention_bias.num_embeddings)
        return self.relative_attention_bias(bucket.to(self.relative_attention_bias.weight.device)).permute(2, 0, 1)[None]

    def forward(self, x, mask=None, lens=None, hip=False):
        T = x.shape[1]
        rel = self.rel_table(T) if hip else None
        made = []

        def bias():
            if not made:
                b = self.position_bias(T).to(x.dtype)
                if mask is not None:
                    b = b.masked_fill(~mask.to(b.device)[:, None, None, :].bool(), float("-inf"))
                made.append(b)
            return made[0]
        for layer in self.layer:
            x = layer(x, bias, lens, rel, hip)
        return x


class MPNetSentenceEncoder(nn.Module):
    """transformers.MPNetModel without its pooler, under MPNetModel's module tree and key names, with
    sentence-transformers' Pooling(mean) + Normalize behind it: what SentenceTransformer('all-mpnet-base-v2') runs.
    forward(tokens) -> last_hidden_state [B, T, hidden] for {input_ids, attention_mask (optional)};
    embed(tokens) -> the unit sentence vectors [B, hidden]; encode(sentences) -> the same as a float32 numpy array, from
    strings.  heads need not be hidden / 64, but only that width takes the HIP route.  fp32 only on the HIP route.
    layer_norm_eps is not in a state dict: eps defaults to all-mpnet-base-v2's 1e-5."""

    def __init__(self, vocab=30527, hidden=768, depth=12, heads=12, mlp=3072, max_pos=514, eps=1e-5, buckets=32):
        super().__init__()
        if hidden % heads:
            raise ValueError("MPNetSentenceEncoder: hidden %d is not a multiple of %d heads" % (hidden, heads))
        self.out_dim = hidden
        self.heads = heads
        self.embeddings = _MPNetEmbeddings(vocab, hidden, max_pos, eps)
        self.encoder = _MPNetEncoder(depth, hidden, heads, mlp, eps, buckets)
        self.tokenizer = None

    @classmethod
    def from_state_dict(cls, sd, eps=1e-5):
        """The model of an MPNetModel state dict: sized from its shapes (heads = the columns of relative_attention_bias,
        depth from the keys, vocabulary and position rows from the tables), pooler.* and embeddings.position_ids ignored
        by name, floating tensors upcast to fp32, and a STRICT load: a missing or an unexpected key is an error."""
        sd = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()
              if not k.startswith(_MPNET_IGNORED)}

        def shape(key):
            if key not in sd:
                raise RuntimeError("not an MPNetModel state dict: it lacks %r (its first keys: %s)" % (key, sorted(sd)[:4]))
            return tuple(sd[key].shape)
        vocab, hidden = shape("embeddings.word_embeddings.weight")
        buckets, heads = shape("encoder.relative_attention_bias.weight")
        layer = "encoder.layer."
        depth = 1 + max([int(k[len(layer):].split(".")[0]) for k in sd if k.startswith(layer)], default=-1)
        if depth < 1:
            raise RuntimeError("the state dict has no %s* keys" % layer)
        model = cls(vocab=vocab, hidden=hidden, depth=depth, heads=heads, mlp=shape("encoder.layer.0.intermediate.dense.weight")[0],
                    max_pos=shape("embeddings.position_embeddings.weight")[0], eps=eps, buckets=buckets)
        model.load_state_dict(sd, strict=True)
        return model

    def route(self, ids, mask=None):
        """(sentence_route's answer, the int32 [B] key counts on the weights' device or None) for the ids [B, T] and the
        attention mask.  The mask is looked at where it lies: a host mask (the tokenizer's) costs no device sync.  Without
        a mask every token is a key, <pad> tokens included, and those take position row 1, not t + 2: such ids go to ATen
        (looking for them is one sync when the ids are on the GPU)."""
        w = self.embeddings.word_embeddings.weight
        B, T = ids.shape
        lens = None if mask is None else prefix_mask_lengths(mask)
        prefix = lens is not None if mask is not None else not bool((ids == MPNET_PAD_ID).any())
        route = sentence_route(HIP_SENTENCE, w.is_cuda and ids.is_cuda, w.dtype, torch.is_grad_enabled(), self.training, B, T,
                               w.shape[1], self.heads, self.embeddings.position_embeddings.num_embeddings,
                               FUSED_RESIDUAL and core.linear_residual_available(), prefix)
        return route, (None if lens is None or route != "hip" else lens.to(w.device))

    def _hidden(self, tokens):
        ids, mask = tokens["input_ids"], tokens.get("attention_mask")
        route, lens = self.route(ids, mask)
        hip = route == "hip"
        x = self.embeddings(ids, hip)
        if mask is not None and not hip:
            mask = mask.to(x.device)
        return self.encoder(x, mask, lens, hip), mask, lens, hip

    def forward(self, tokens):
        return self._hidden(tokens)[0]

    def embed(self, tokens):
        """Pooling(mean) + Normalize on forward(tokens): m = sum(x * mask) / clamp(sum(mask), 1e-9), m / max(||m||, 1e-12)."""
        x, mask, lens, hip = self._hidden(tokens)
        if hip:
            return core.masked_mean_l2(x.contiguous(), lens)                                               # K27
        m = torch.ones(x.shape[:2], device=x.device) if mask is None else mask
        m = m.unsqueeze(-1).expand(x.size()).to(x.dtype)
        return F.normalize(torch.sum(x * m, 1) / torch.clamp(m.sum(1), min=1e-9), p=2, dim=1)

    def encode(self, sentences, batch_size=32):
        """SentenceTransformer.encode's default: the unit sentence vectors of `sentences` as a float32 numpy array [n, hidden]
        in input order.  Batches are taken in input order, each padded to its own longest sequence (no length-sorted
        batching: a row's result does not depend on its batch); sequences over MPNET_MAX_TOKENS tokens are truncated
        there, with a warning.  The tokenizer is self.tokenizer, or the registered 'mpnet' vocabulary (mpnet_tokenizer)."""
        if isinstance(sentences, str):
            sentences = [sentences]
        if self.tokenizer is None:
            self.tokenizer = mpnet_tokenizer()
        tok = self.tokenizer
        device = self.embeddings.word_embeddings.weight.device
        rows = [tok.encode(s, None) for s in sentences]
        long = sum(len(r) > MPNET_MAX_TOKENS for r in rows)
        if long:
            import warnings
            warnings.warn("MPNetSentenceEncoder.encode: %d of %d sentences are over %d tokens and were truncated"
                          % (long, len(rows), MPNET_MAX_TOKENS))
            rows = [r if len(r) <= MPNET_MAX_TOKENS else r[:MPNET_MAX_TOKENS - 1] + [tok.sep_id] for r in rows]
        out = torch.empty(len(rows), self.out_dim, dtype=torch.float32)
        with torch.no_grad():
            for i in range(0, len(rows), batch_size):
                batch = rows[i:i + batch_size]
                T = max(len(r) for r in batch)
                ids = torch.full((len(batch), T), tok.pad_id, dtype=torch.long)
                mask = torch.zeros(len(batch), T, dtype=torch.long)
                for j, r in enumerate(batch):
                    ids[j, :len(r)] = torch.tensor(r, dtype=torch.long)
                    mask[j, :len(r)] = 1
                out[i:i + len(batch)] = self.embed({"input_ids": ids.to(device), "attention_mask": mask}).float().cpu()
        return out.numpy()


def mpnet_tokenizer():
    """The WordPieceTokenizer of the registered MPNet vocabulary (register_tokenizer('mpnet', path) or MCD_MPNET_VOCAB) with
    MPNet's special tokens; without one an error -- never the hashing stand-in."""
    entry = TOKENIZER_VOCABS.get("mpnet")
    if entry is None and os.environ.get("MCD_MPNET_VOCAB"):
        entry = (os.environ["MCD_MPNET_VOCAB"], True)
    if entry is None:
        raise RuntimeError("the MPNet sentence encoder needs its WordPiece vocabulary: call data_utils.register_tokenizer("
                           "'mpnet', '/path/vocab.txt') or set MCD_MPNET_VOCAB=/path/vocab.txt (all-mpnet-base-v2's "
                           "vocab.txt); there is no fallback to the hashing tokenizer")
    try:      # MPNetTokenizer's unknown token is '[UNK]' (its default, and all-mpnet-base-v2's configuration), which that
        #       vocabulary holds beside '<unk>'; a vocabulary without it takes '<unk>'
        return WordPieceTokenizer(entry[0], do_lower_case=entry[1], specials=MPNET_SPECIALS[:1] + ("[UNK]",) + MPNET_SPECIALS[2:])
    except ValueError:
        return WordPieceTokenizer(entry[0], do_lower_case=entry[1], specials=MPNET_SPECIALS)


SENTENCE_CHECKPOINT = {}


def register_sentence_checkpoint(path):
    """Where the sentence encoder's checkpoint lives: a LOCAL file holding an MPNetModel state dict (all-mpnet-base-v2's
    pytorch_model.bin or model.safetensors) or the snapshot directory itself, which must exist now; a directory's
    vocab.txt becomes the `mpnet` vocabulary when none is registered.  The environment variable MCD_MPNET_CKPT does the same for a process that
    registers nothing."""
    if not isinstance(path, str) or not (os.path.isfile(path) or os.path.isdir(path)):
        raise FileNotFoundError("register_sentence_checkpoint: %r is not an existing local file or snapshot directory" % (path,))
    SENTENCE_CHECKPOINT["path"] = path
    vocab = os.path.join(path, "vocab.txt")
    if os.path.isdir(path) and os.path.isfile(vocab) and "mpnet" not in TOKENIZER_VOCABS:
        register_tokenizer("mpnet", vocab)


def sentence_encoder(device, ckpt=None):
    """The MPNetSentenceEncoder of get_cos_similarity's mpnet_model argument, in eval mode on `device`: from ckpt (a state
    dict, a LOCAL file or a snapshot directory), else from the registered checkpoint (register_sentence_checkpoint / MCD_MPNET_CKPT).  Files are
    read with weights_only=True; the load is strict.  Nothing is downloaded: without a checkpoint this is an error."""
    ckpt = ckpt if ckpt is not None else SENTENCE_CHECKPOINT.get("path") or os.environ.get("MCD_MPNET_CKPT")
    if ckpt is None:
        raise RuntimeError("the sentence encoder needs a local MPNetModel checkpoint: pass ckpt=, call "
                           "data_utils.register_sentence_checkpoint('/path/pytorch_model.bin') or set MCD_MPNET_CKPT")
    sd = _state_dict_of(ckpt)
    return MPNetSentenceEncoder.from_state_dict(sd, **snapshot_kwargs("mpnet", _config_of(ckpt), sd)).to(device).eval()


# ------------------------------------------------------------------------------------------------------
# config.json of a Hugging Face snapshot -> the mirrors' constructor arguments
# ------------------------------------------------------------------------------------------------------
def hf_vit_config(sd, prefix, heads=None):
    """HFViT's / HFDinov2's constructor arguments read from the shapes of a ViTForImageClassification /
    Dinov2ForImageClassification state dict (transformers' key names or the mirror's; prefix 'vit' / 'dinov2'): the width
    from cls_token, the patch from the projection, the grid (and with it the resolution the position table was built for)
    from the position rows, the depth by counting layers, the MLP width from the first layer, num_labels from
    classifier.weight when the file has one (else the key is absent: the caller decides).  The state dict does not carry
    the head count: width // 64 (every released ViT and DINOv2 has 64-wide heads) unless `heads` says otherwise."""
    def shape(*keys):
        for key in keys:
            if key in sd:
                return tuple(sd[key].shape)
        raise RuntimeError("not a %s classifier's state dict: it lacks %r" % (prefix, keys[0]))
    dim = shape(prefix + ".embeddings.cls_token")[2]
    patch = shape(prefix + ".embeddings.patch_embeddings.projection.weight")[2]
    rows = shape(prefix + ".embeddings.position_embeddings")[1]
    grid = round((rows - 1) ** 0.5)
    if grid * grid + 1 != rows:
        raise RuntimeError("%s.embeddings.position_embeddings has %d rows: not a square grid plus one" % (prefix, rows))
    stem = prefix + ".encoder.layer."
    depth = len([k for k in sd if k.startswith(stem) and k.endswith((".layernorm_before.weight", ".norm1.weight"))])
    first = stem + "0."
    cfg = dict(image_size=grid * patch, patch=patch, dim=dim, depth=depth, heads=heads or max(1, dim // 64),
               mlp=shape(first + "intermediate.dense.weight", first + "mlp.fc1.weight", first + "fc1.weight")[0] if depth
               else 4 * dim)
    if "classifier.weight" in sd:
        cfg["num_labels"] = shape("classifier.weight")[0]
    return cfg


# family -> (the model_type values its config.json may carry, transformers' class defaults of the fields that are not in
# a state dict: a config.json written as a difference to the defaults leaves such a field out)
_SNAPSHOT_FAMILIES = {
    "vit": (("vit",), dict(num_attention_heads=12, layer_norm_eps=1e-12, hidden_act="gelu", qkv_bias=True)),
    "dino": (("dinov2",), dict(num_attention_heads=12, layer_norm_eps=1e-6, hidden_act="gelu", qkv_bias=True,
                               layerscale_value=1.0, use_swiglu_ffn=False)),
    "clip": (("clip", "clip_vision_model"), dict(num_attention_heads=12, layer_norm_eps=1e-5, hidden_act="quick_gelu")),
    "openai_clip": (("clip",), dict(layer_norm_eps=1e-5, hidden_act="quick_gelu")),
    "resnet": (("resnet",), dict(downsample_in_first_stage=False, downsample_in_bottleneck=False, layer_type="bottleneck",
                                 hidden_act="relu")),
    "mae": (("vit_mae",), dict(num_attention_heads=12, decoder_num_attention_heads=16, mask_ratio=0.75, norm_pix_loss=False,
                               layer_norm_eps=1e-12, hidden_act="gelu", qkv_bias=True)),
    "mpnet": (("mpnet",), dict(layer_norm_eps=1e-12, relative_attention_num_buckets=32, hidden_act="gelu")),
}


def _config_labels(config):
    """num_labels of a config.json: the field itself, else the length of id2label (what transformers stores)."""
    if "num_labels" in config:
        return int(config["num_labels"])
    return len(config["id2label"]) if isinstance(config.get("id2label"), dict) else None


def snapshot_kwargs(family, config, sd=None):
    """The keyword arguments a snapshot's config.json adds to a mirror's constructor / from_state_dict: what a state dict
    does not carry (head counts, LayerNorm eps, the activation, MAE's mask_ratio / norm_pix_loss, the HF ResNet's
    downsample_* flags, ...).  family: 'vit' (HFViT), 'dino' (HFDinov2), 'clip' (HFClip; a CLIPModel config's
    vision_config, or a clip_vision_model one), 'resnet' (HFResNet), 'mae' (HFMae), 'mpnet' (MPNetSentenceEncoder),
    'openai_clip' (OpenAIClip from a CLIPModel snapshot: hf_clip_to_openai).  config None: {} -- the shape-based guesses
    stay as they are.
    A model_type that is not the family's is a ValueError; a configuration the mirror cannot compute (use_swiglu_ffn,
    another activation, qkv_bias false, ...) a NotImplementedError naming the field; with `sd`, a field that the state
    dict's shapes give as well (widths, depths, patch, grid, classifier width) and give differently a RuntimeError naming
    the field and both values."""
    if config is None:
        return {}
    types, defaults = _SNAPSHOT_FAMILIES[family]
    kind = config.get("model_type")
    if kind not in types:
        raise ValueError("config.json describes a %r model, which is not the %r target's family (model_type %s)"
                         % (kind, family, " or ".join(repr(t) for t in types)))
    top = config

    def tower(name):
        sub = top.get(name) if kind == "clip" else top
        if not isinstance(sub, dict):
            raise ValueError("config.json of model_type 'clip' has no %s object" % name)
        return sub

    def get(cfg, field):
        return cfg[field] if field in cfg and cfg[field] is not None else defaults[field]

    def refuse(field, value, takes):
        raise NotImplementedError("config.json: %s = %r is not something %s computes (it takes %s)"
                                  % (field, value, family, takes))

    def act(cfg, allowed, field="hidden_act"):
        value = get(cfg, field)
        if value not in allowed:
            refuse(field, value, " or ".join(repr(a) for a in allowed))
        return value

    def agree(cfg, pairs, shapes, where=""):
        for field, key in pairs:
            if field in cfg and cfg[field] is not None and key in shapes:
                a, b = cfg[field], shapes[key]
                if isinstance(b, (list, tuple)):
                    a, b = list(a) if isinstance(a, (list, tuple)) else a, list(b)
                if a != b:
                    raise RuntimeError("config.json says %s%s = %r, the state dict's shapes say %r" % (where, field, a, b))

    if family in ("vit", "dino", "mae"):
        if not get(config, "qkv_bias"):
            refuse("qkv_bias", config["qkv_bias"], "projections with a bias")
        act(config, ("gelu",))
    if family in ("vit", "dino"):
        out = dict(heads=int(get(config, "num_attention_heads")), eps=float(get(config, "layer_norm_eps")))
        if family == "dino":
            if get(config, "use_swiglu_ffn"):
                refuse("use_swiglu_ffn", True, "the fc1 / GELU / fc2 MLP")
            out["layer_scale"] = float(get(config, "layerscale_value"))
        if sd is not None:
            shapes = hf_vit_config(sd, "vit" if family == "vit" else "dinov2")
            if family == "dino" and config.get("mlp_ratio") is not None and config.get("hidden_size") is not None:
                shapes["mlp_ratio_width"] = shapes["mlp"]
                config = dict(config, mlp_ratio_width=int(config["hidden_size"] * config["mlp_ratio"]))
            labels = _config_labels(config)
            agree(dict(config, num_labels=labels),
                  (("hidden_size", "dim"), ("num_hidden_layers", "depth"), ("intermediate_size", "mlp"), ("patch_size", "patch"),
                   ("image_size", "image_size"), ("num_labels", "num_labels"), ("mlp_ratio_width", "mlp_ratio_width")), shapes)
        return out
    if family == "clip":
        vision = tower("vision_config")
        out = dict(heads=int(get(vision, "num_attention_heads")), hidden_act=act(vision, ("quick_gelu", "gelu")),
                   eps=float(get(vision, "layer_norm_eps")))
        if sd is not None and HF_CLIP_KEY in sd:
            agree(dict(vision, num_labels=_config_labels(top) if any(k.startswith("classifier.") for k in sd) else None),
                  (("hidden_size", "hidden"), ("num_hidden_layers", "layers"), ("intermediate_size", "mlp"),
                   ("patch_size", "patch"), ("image_size", "image_size"), ("num_labels", "num_labels")),
                  hf_clip_config(sd), "vision_config." if kind == "clip" else "")
        return out
    if family == "openai_clip":
        vision, text = tower("vision_config"), tower("text_config")
        for name, cfg in (("vision_config", vision), ("text_config", text)):
            act(cfg, ("quick_gelu",))
            if float(get(cfg, "layer_norm_eps")) != 1e-5:
                refuse(name + ".layer_norm_eps", cfg["layer_norm_eps"], "1e-05")
        out = {}
        if vision.get("num_attention_heads") is not None:
            out["vision_heads"] = int(vision["num_attention_heads"])
        if text.get("num_attention_heads") is not None:
            out["transformer_heads"] = int(text["num_attention_heads"])
        if sd is not None:
            shapes = openai_clip_config(sd)
            agree(vision, (("hidden_size", "vision_width"), ("num_hidden_layers", "vision_layers"),
                           ("patch_size", "vision_patch_size"), ("image_size", "image_resolution")), shapes, "vision_config.")
            agree(text, (("hidden_size", "transformer_width"), ("num_hidden_layers", "transformer_layers"),
                         ("vocab_size", "vocab_size"), ("max_position_embeddings", "context_length")), shapes, "text_config.")
            agree(top, (("projection_dim", "embed_dim"),), shapes)
        return out
    if family == "resnet":
        act(config, ("relu",))
        out = dict(downsample_in_first_stage=bool(get(config, "downsample_in_first_stage")),
                   downsample_in_bottleneck=bool(get(config, "downsample_in_bottleneck")))
        if get(config, "layer_type") not in ("basic", "bottleneck"):
            refuse("layer_type", config["layer_type"], "'basic' or 'bottleneck'")
        if sd is not None:
            agree(dict(config, num_labels=_config_labels(config) if "classifier.1.weight" in sd else None),
                  (("num_channels", "num_channels"), ("embedding_size", "embedding_size"), ("hidden_sizes", "hidden_sizes"),
                   ("depths", "depths"), ("layer_type", "layer_type"), ("num_labels", "num_labels")), hf_resnet_config(sd))
        return out
    if family == "mae":
        out = dict(heads=int(get(config, "num_attention_heads")), decoder_heads=int(get(config, "decoder_num_attention_heads")),
                   mask_ratio=float(get(config, "mask_ratio")), norm_pix_loss=bool(get(config, "norm_pix_loss")),
                   eps=float(get(config, "layer_norm_eps")))
        if sd is not None:
            agree(config, (("hidden_size", "hidden"), ("num_hidden_layers", "layers"), ("intermediate_size", "mlp"),
                           ("patch_size", "patch"), ("image_size", "image_size"), ("decoder_hidden_size", "decoder_hidden"),
                           ("decoder_num_hidden_layers", "decoder_layers"), ("decoder_intermediate_size", "decoder_mlp")),
                  mae_config(sd))
        return out
    act(config, ("gelu",))                                                                         # mpnet
    out = dict(eps=float(get(config, "layer_norm_eps")))
    if sd is not None:
        shapes = {}
        for key, axis, name in (("embeddings.word_embeddings.weight", 0, "vocab_size"),
                                ("embeddings.word_embeddings.weight", 1, "hidden_size"),
                                ("embeddings.position_embeddings.weight", 0, "max_position_embeddings"),
                                ("encoder.relative_attention_bias.weight", 0, "relative_attention_num_buckets"),
                                ("encoder.relative_attention_bias.weight", 1, "num_attention_heads"),
                                ("encoder.layer.0.intermediate.dense.weight", 0, "intermediate_size")):
            if key in sd:
                shapes[name] = tuple(sd[key].shape)[axis]
        shapes["num_hidden_layers"] = len([k for k in sd if k.startswith("encoder.layer.") and k.endswith(".attention.attn.q.weight")])
        agree(dict(config, relative_attention_num_buckets=get(config, "relative_attention_num_buckets")),
              tuple((name, name) for name in shapes), shapes)
    return out


def hf_clip_to_openai(sd, config=None):
    """A transformers CLIPModel state dict (openai/clip-vit-*'s model.safetensors) under OpenAI's names, so that
    OpenAIClip.from_state_dict loads it strictly.  The two layouts dictate the rules: q_proj | k_proj | v_proj concatenated
    into attn.in_proj_weight / in_proj_bias; visual_projection.weight and text_projection.weight transposed into
    visual.proj and text_projection; pre_layrnorm -> ln_pre, post_layernorm -> ln_post, final_layer_norm -> ln_final;
    layer_norm1 / 2 -> ln_1 / 2; mlp.fc1 / fc2 -> mlp.c_fc / c_proj; the patch convolution, the class and position tables
    under visual.conv1 / class_embedding / positional_embedding; position_ids buffers dropped.  config (the snapshot's
    config.json) is checked by snapshot_kwargs('openai_clip', ...); only the ViT CLIPs exist in this format."""
    if config is not None:
        snapshot_kwargs("openai_clip", config)
    fixed = {"vision_model.embeddings.class_embedding": "visual.class_embedding",
             "vision_model.embeddings.patch_embedding.weight": "visual.conv1.weight",
             "vision_model.embeddings.position_embedding.weight": "visual.positional_embedding",
             "text_model.embeddings.token_embedding.weight": "token_embedding.weight",
             "text_model.embeddings.position_embedding.weight": "positional_embedding",
             "logit_scale": "logit_scale"}
    norms = {"vision_model.pre_layrnorm.": "visual.ln_pre.", "vision_model.post_layernorm.": "visual.ln_post.",
             "text_model.final_layer_norm.": "ln_final."}
    towers = {"vision_model.encoder.layers.": "visual.transformer.resblocks.", "text_model.encoder.layers.": "transformer.resblocks."}
    inner = {"self_attn.out_proj.": "attn.out_proj.", "layer_norm1.": "ln_1.", "layer_norm2.": "ln_2.", "mlp.fc1.": "mlp.c_fc.",
             "mlp.fc2.": "mlp.c_proj."}
    out, qkv = {}, {}
    for key, value in sd.items():
        if key.endswith(".position_ids"):
            continue
        if key in fixed:
            out[fixed[key]] = value
        elif key == "visual_projection.weight":
            out["visual.proj"] = value.t().contiguous()
        elif key == "text_projection.weight":
            out["text_projection"] = value.t().contiguous()
        elif key.startswith(tuple(norms)):
            old = next(n for n in norms if key.startswith(n))
            out[norms[old] + key[len(old):]] = value
        elif key.startswith(tuple(towers)):
            old = next(t for t in towers if key.startswith(t))
            index, _, rest = key[len(old):].partition(".")
            base = towers[old] + index + "."
            part = next((p for p in ("q_proj", "k_proj", "v_proj") if rest.startswith("self_attn.%s." % p)), None)
            if part is not None:
                qkv.setdefault((base, rest.rsplit(".", 1)[1]), {})[part] = value
                continue
            name = next((n for n in inner if rest.startswith(n)), None)
            if name is None:
                raise RuntimeError("not a CLIPModel state dict: %r has no OpenAI name" % (key,))
            out[base + inner[name] + rest[len(name):]] = value
        else:
            raise RuntimeError("not a CLIPModel state dict: %r has no OpenAI name" % (key,))
    for (base, leaf), parts in qkv.items():
        if sorted(parts) != ["k_proj", "q_proj", "v_proj"]:
            raise RuntimeError("%sself_attn: q_proj, k_proj and v_proj %s must come together" % (base, leaf))
        out["%sattn.in_proj_%s" % (base, leaf)] = torch.cat([parts["q_proj"], parts["k_proj"], parts["v_proj"]], dim=0)
    return out


HF_CLIP_MODEL_KEY = "text_model.embeddings.token_embedding.weight"       # what tells a CLIPModel state dict (with HF_CLIP_KEY)


# target name -> a LOCAL checkpoint of that target, like register_clip_checkpoint for the dissector
TARGET_CHECKPOINTS = {}
_TARGET_TABLE = {}       # the parsed MCD_TARGET_CKPTS file and its (path, mtime, size)


class RegisteredCheckpoint(str):
    """The path of a checkpoint that was registered for a target: a model built for that target must take at least one of
    the file's keys (_load_local), or the registration names a wrong file."""


def register_target_checkpoint(name, path):
    """Where the checkpoint of --target_model `name` lives (a state dict file or {'model': state dict}, a .safetensors
    file, or a Hugging Face snapshot directory, whose config.json then sizes the model: snapshot_kwargs; local paths
    only, and the path must exist now).  The drivers then build that target from it: for `clip` an HFClip sized from the
    file; for every other target that is not a breastclip* one, the file in place of the Mammo-CLIP checkpoint.  The
    environment variable MCD_TARGET_CKPTS names a JSON file {name: path} that does the same for a process that registers
    nothing."""
    if not isinstance(path, str) or not (os.path.isfile(path) or os.path.isdir(path)):
        raise FileNotFoundError("register_target_checkpoint(%r): %r is not an existing local file or snapshot directory"
                                % (name, path))
    TARGET_CHECKPOINTS[name] = path


def target_checkpoint(name):
    """The registered checkpoint path of target `name` (a RegisteredCheckpoint), or None."""
    path = TARGET_CHECKPOINTS.get(name)
    table = os.environ.get("MCD_TARGET_CKPTS", "")
    if path is None and table:
        stamp = (table, os.path.getmtime(table), os.path.getsize(table))
        if _TARGET_TABLE.get("stamp") != stamp:          # parsed once per file, again when the file changes
            import json
            with open(table, "r", encoding="utf-8") as f:
                entries = json.load(f)
            if not isinstance(entries, dict):
                raise ValueError("MCD_TARGET_CKPTS=%r: the file must hold one JSON object {target name: path}" % (table,))
            _TARGET_TABLE.update(stamp=stamp, entries=entries)
        path = _TARGET_TABLE["entries"].get(name)
        if path is not None and not (isinstance(path, str) and (os.path.isfile(path) or os.path.isdir(path))):
            raise FileNotFoundError("MCD_TARGET_CKPTS=%r: %r -> %r is not an existing local file or snapshot directory"
                                    % (table, name, path))
    return None if path is None else RegisteredCheckpoint(path)


def target_ckpt_or(target_name, ckpt):
    """What the drivers pass to get_target_model as `ckpt`: the checkpoint registered for the target when there is one and
    the target is not a breastclip* model (those take the Mammo-CLIP checkpoint), else `ckpt`, as before."""
    if target_name.startswith("breastclip"):
        return ckpt
    return target_checkpoint(target_name) or ckpt


# ------------------------------------------------------------------------------------------------------
# factories
# ------------------------------------------------------------------------------------------------------
BERT_PREFIX = "text_encoder.text_encoder."
_BERT_IGNORED = (BERT_PREFIX + "pooler.", BERT_PREFIX + "embeddings.position_ids")


def _state_dict_of(ckpt):
    """The state dict in ckpt: a state dict, {'model': state dict} (reference utils.py:451-455), or a LOCAL path to
    either (loaded with weights_only=True: nothing from the file is executed), to a .safetensors file or to a Hugging
    Face snapshot directory (checkpoint_io.resolve_checkpoint)."""
    if isinstance(ckpt, str):
        ckpt = checkpoint_io.resolve_checkpoint(ckpt).state_dict()
    return ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt


def _config_of(ckpt):
    """The parsed config.json that comes with ckpt: a snapshot directory's, or the one beside a .safetensors file; None
    for a state dict and for a torch file (those never carried one: the shapes size the model, as before)."""
    if isinstance(ckpt, str) and checkpoint_io.is_snapshot_path(ckpt):
        return checkpoint_io.resolve_checkpoint(ckpt).config
    return None


def _load_local(model, ckpt, text_strict=False, sd=None):
    """ckpt: None, a state dict, {'model': state dict} (reference utils.py:451-455), or a LOCAL path
    (_state_dict_of: nothing from the file is executed); sd: ckpt's state dict when the caller has read it already.
    text_strict (a BreastClip with the BERT tower): the text side loads strictly -- pooler.* and
    embeddings.position_ids are ignored by name (BertTextTower has no pooler; 4.41.1 no longer stores the buffer, older
    checkpoints do), any other missing or unexpected key under text_encoder. is an error instead of a tower of random
    weights.  A BreastClip / BreastClipClassifier with the ResNet image tower loads the image side strictly in the same
    way whenever the state dict has a key under image_encoder. at all."""
    if ckpt is None:
        return model
    sd = _state_dict_of(ckpt) if sd is None else sd
    if isinstance(model, (_HFClassifier, HFMae)):    # transformers' key names -> the mirror's
        sd = model.convert_state_dict(sd)
    if text_strict:
        sd = {k: v for k, v in sd.items() if not k.startswith(_BERT_IGNORED)}
    result = model.load_state_dict(sd, strict=False)
    if isinstance(ckpt, RegisteredCheckpoint) and len(result.unexpected_keys) == len(sd):
        raise RuntimeError("the checkpoint registered for this target, %r, has no key that %s takes (its first keys: %s): a "
                           "wrong file, or a wrong target name" % (str(ckpt), type(model).__name__, sorted(sd)[:4]))
    if getattr(model, "model_type", None) == "resnet" and any(k.startswith("image_encoder.") for k in sd):
        missing = [k for k in result.missing_keys if k.startswith("image_encoder.")]
        unexpected = [k for k in result.unexpected_keys if k.startswith("image_encoder.")]
        if missing or unexpected:
            raise RuntimeError("the checkpoint's image encoder does not match the ResNet tower: %d missing key(s) %s, %d "
                               "unexpected key(s) %s" % (len(missing), missing[:4], len(unexpected), unexpected[:4]))
    if text_strict:
        missing = [k for k in result.missing_keys if k.startswith("text_encoder.")]
        unexpected = [k for k in result.unexpected_keys if k.startswith("text_encoder.")]
        if missing or unexpected:
            raise RuntimeError("the checkpoint's text tower does not match BertTextTower: %d missing key(s) %s, %d unexpected "
                               "key(s) %s" % (len(missing), missing[:4], len(unexpected), unexpected[:4]))
    return model


def _load_places(model, ckpt):
    """resnet18_places (reference data_utils.py:70-79): ckpt is None (the reference's relative PLACES_CKPT if that file
    exists, else the seeded weights stay), a state dict, the reference's {'state_dict': {...}} container, or a LOCAL
    path to either.  A leading 'module.' (DataParallel) is stripped from the keys and the load is strict, as the
    reference's is.  Files are read with weights_only=True; one that cannot be read that way is an error, not a random
    model."""
    if ckpt is None:
        if not os.path.isfile(PLACES_CKPT):
            return model
        ckpt = PLACES_CKPT
    if isinstance(ckpt, str):
        try:
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
        except Exception as e:
            raise RuntimeError("resnet18_places: %r cannot be loaded with weights_only=True (%s: %s); re-save it as a "
                               "plain {'state_dict': tensors} file" % (ckpt, type(e).__name__, e)) from e
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    model.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()})
    return model


def get_target_model(target_name, device, args=None, ckpt=None, n_class=None, finetuned_ckpt=None, seed=0, image_size=224,
                     text_tower=None, use_registered=True):
    """Returns (target model in eval mode, preprocess) -- reference data_utils.py:38-93.  Weights are
    random-init under `seed` unless a local checkpoint is given; nothing is downloaded.
    ckpt / finetuned_ckpt: a state dict, {'model': state dict}, or a LOCAL path -- a torch file, a .safetensors file or a
    Hugging Face snapshot directory (checkpoint_io.resolve_checkpoint).  A directory's (or a .safetensors file's)
    config.json gives what the shapes do not -- head counts, LayerNorm eps, activation, MAE's mask_ratio, the HF ResNet's
    downsample_* flags (snapshot_kwargs) -- and must agree with the shapes; `vit` / `dino` are sized from such a
    checkpoint's shapes (hf_vit_config).  `openai_clip` also takes a transformers CLIPModel snapshot (hf_clip_to_openai).
    image_size: input resolution of the ViT towers, an int (square) or (H, W) (position embeddings are sized for it;
    the reference's HF ViT is built for its checkpoint's resolution the same way); also accepted as a suffix,
    'breastclip_vit_1024' or 'breastclip_vit_1520x912' (H x W, Mammo-CLIP's own input).  The attention is HIP at
    every resolution: K9 up to 256 tokens, K9L beyond (attention_route).
    text_tower (breastclip, breastclip_vit): 'stand-in', 'bert', or None = 'bert' exactly when the checkpoint's state dict
    has keys starting text_encoder.text_encoder. (a Mammo-CLIP checkpoint), else the stand-in.  The BERT tower's hidden
    size, depth, intermediate size, vocabulary and position rows are read from the checkpoint's shapes.
    use_registered (clip): False keeps the checkpoint registered for the `clip` TARGET out of this call -- the drivers build
    their stand-in DISSECTOR under the same name (og_utils._clip_dissector).
    `mae` exists only with a checkpoint (ckpt= holding MAE_KEYS, or one registered for `mae`): HFMae sized from it.
    `resnet`, `resnet-cub`, `resnet-bloodmnist` likewise (ckpt= holding HF_RESNET_KEY, or one registered for the name): an
    HFResNet sized from it, the classifier's width included; `clip-cub`, `clip-bloodmnist`: an HFClip, as `clip` with a
    checkpoint.  breastclip / breastclip_classifier follow the checkpoint's image keys: Swin, EfficientNet or the wrapped
    torchvision ResNet (image_tower_of)."""
    if text_tower not in (None, "stand-in", "bert"):
        raise ValueError("text_tower must be None, 'stand-in' or 'bert', got %r" % (text_tower,))
    if target_name == "openai_clip":
        # OpenAI CLIP itself: ckpt a state dict, or a LOCAL path to one or to OpenAI's TorchScript archive -- the model is
        # sized from its shapes and loaded strictly; without ckpt, ViT-B/16's configuration with seeded weights
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            if ckpt is None:
                model = OpenAIClip(**VIT_B16)
            else:
                sd, heads = openai_clip_state_dict(ckpt), {}
                config = _config_of(ckpt)
                if HF_CLIP_KEY in sd and HF_CLIP_MODEL_KEY in sd:
                    # a transformers CLIPModel (the hub's openai/clip-vit-*): OpenAI's names, the head counts of config.json
                    sd = hf_clip_to_openai(sd, config)
                    heads = snapshot_kwargs("openai_clip", config, sd)
                model = OpenAIClip.from_state_dict(sd, **heads)
        return model.to(device).eval(), None
    if target_name in HF_CLIP_TARGETS:
        # transformers' CLIPForImageClassification when a checkpoint of it is at hand: `ckpt` itself when it carries the
        # vision tower's keys, else the one registered for the name (`clip`, or the fine-tunes `clip-cub` /
        # `clip-bloodmnist`, which exist only with such a checkpoint: without one they fall to the ValueError below).  Sized from the shapes (a fine-tuned clip-cub /
        # clip-bloodmnist file is this target with that file) and loaded strictly.  Without either, the stand-in below.
        sd = config = None
        if ckpt is not None:
            loaded = _state_dict_of(ckpt)
            if HF_CLIP_KEY in loaded or isinstance(ckpt, RegisteredCheckpoint):
                sd, config = loaded, _config_of(ckpt)
            else:
                ckpt = loaded                    # read once: the stand-in below loads from the state dict
        if sd is None and use_registered:
            registered = target_checkpoint(target_name)
            sd, config = (None, None) if registered is None else (_state_dict_of(registered), _config_of(registered))
        if sd is not None:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                model = HFClip.from_state_dict(sd, n_class=n_class, **snapshot_kwargs("clip", config, sd))
            _load_local(model, finetuned_ckpt)
            return model.to(device).eval(), None
    if target_name in HF_RESNET_TARGETS:
        # transformers' ResNetForImageClassification (microsoft/resnet-50 and its fine-tunes), and only from a checkpoint of
        # it: `ckpt` itself when it carries HF_RESNET_KEY (or is the registered file), else the one registered for the name.
        # Sized from the shapes, the classifier's width included, and loaded strictly.  Without either the name stays
        # unknown (the ValueError below).
        sd = config = None
        if ckpt is not None:
            loaded = _state_dict_of(ckpt)
            if isinstance(ckpt, RegisteredCheckpoint) or (isinstance(loaded, dict) and HF_RESNET_KEY in loaded):
                sd, config = loaded, _config_of(ckpt)
        if sd is None and use_registered:
            registered = target_checkpoint(target_name)
            sd, config = (None, None) if registered is None else (_state_dict_of(registered), _config_of(registered))
        if sd is not None:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                model = HFResNet.from_state_dict(sd, n_class=n_class, **snapshot_kwargs("resnet", config, sd))
            _load_local(model, finetuned_ckpt)
            return model.to(device).eval(), None
    if target_name == "mae":
        # transformers' ViTMAEForPreTraining, and only from a checkpoint of it: `ckpt` itself when it carries MAE_KEYS (or is
        # the registered file), else the one registered for `mae`.  Sized from the shapes and loaded strictly; n_class is
        # ignored (the model has no classifier).  Without either the name stays unknown (the ValueError below): a seeded
        # stand-in of a pre-training model would dissect nothing anybody trained.
        sd = config = None
        if ckpt is not None:
            loaded = _state_dict_of(ckpt)
            if isinstance(ckpt, RegisteredCheckpoint) or (isinstance(loaded, dict) and all(k in loaded for k in MAE_KEYS)):
                sd, config = loaded, _config_of(ckpt)
        if sd is None and use_registered:
            registered = target_checkpoint("mae")
            sd, config = (None, None) if registered is None else (_state_dict_of(registered), _config_of(registered))
        if sd is not None:
            model = HFMae.from_state_dict(sd, **snapshot_kwargs("mae", config, sd))
            _load_local(model, finetuned_ckpt)
            return model.to(device).eval(), None
    hf_kw, hf_sd = {}, None
    if target_name in HF_TARGETS and ckpt is not None:
        # a ViTForImageClassification / Dinov2ForImageClassification checkpoint sizes the tower: the widths, the patch, the
        # position table's resolution and the classifier's width from its shapes (hf_vit_config), the head count, the
        # LayerNorm eps and DINOv2's LayerScale value from a snapshot's config.json (snapshot_kwargs).  A state dict
        # without the tower's embedding keys (a partial one) leaves the base configuration, as before.
        hf_sd, prefix = _state_dict_of(ckpt), HF_TARGETS[target_name][0].prefix
        config = _config_of(ckpt)
        if isinstance(hf_sd, dict) and prefix + ".embeddings.cls_token" in hf_sd:
            hf_kw = hf_vit_config(hf_sd, prefix)
            hf_kw.update(snapshot_kwargs("vit" if prefix == "vit" else "dino", config, hf_sd))
        elif config is not None:
            snapshot_kwargs("vit" if prefix == "vit" else "dino", config)      # a wrong family is an error all the same
    text_kw = {}
    if target_name.startswith("breastclip") and target_name != "breastclip_classifier" and (ckpt is not None or text_tower):
        if ckpt is not None:
            ckpt = _state_dict_of(ckpt)
        has_bert = ckpt is not None and any(k.startswith(BERT_PREFIX) for k in ckpt)
        if text_tower is None:
            text_tower = "bert" if has_bert else "stand-in"
        if text_tower == "bert":
            text_kw = dict(text_tower="bert", bert_config=bert_config_from_state_dict(ckpt) if has_bert else None)
    if target_name.startswith("breastclip_vit_"):
        hw = _parse_hw(target_name[len("breastclip_vit_"):])
        if hw is not None:
            image_size = hw
            target_name = "breastclip_vit"
    # the image tower follows the checkpoint (reference model/modules/__init__.py:load_image_encoder builds it from the
    # checkpoint's config): Swin keys -> the Swin tower sized from them, an EfficientNet's -> its compound scaling (B2, B5,
    # ...); `ckpt` first, `finetuned_ckpt` when only that carries an image encoder.  No checkpoint: B5 / swin-tiny, seeded.
    tower, tower_kw = ("swin" if target_name == "breastclip_swin" else "cnn"), {}
    if target_name in ("breastclip", "breastclip_classifier", "breastclip_swin"):
        if ckpt is not None:
            ckpt = _state_dict_of(ckpt)
        if finetuned_ckpt is not None:
            finetuned_ckpt = _state_dict_of(finetuned_ckpt)
        found = next((f for f in (image_tower_of(sd) for sd in (ckpt, finetuned_ckpt) if sd is not None) if f), None)
        if found is not None:
            if target_name == "breastclip_swin" and found[0] != "swin":
                raise ValueError("breastclip_swin: the checkpoint's image encoder is %s, not a Swin tower"
                                 % ("a ResNet" if found[0] == "resnet" else "an EfficientNet"))
            tower = found[0]
            tower_kw = dict(swin_config=found[1]) if tower == "swin" else found[1]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        if target_name in ("breastclip", "breastclip_swin"):
            model = BreastClip(tower, **tower_kw, **text_kw)
        elif target_name == "breastclip_vit":
            model = BreastClip("vit", image_size=image_size, **text_kw)
        elif target_name == "breastclip_classifier":
            if n_class is None:
                raise ValueError("Arguments `args`, `ckpt`, and `n_class` must be provided for BreastClipClassifier.")
            model = BreastClipClassifier(n_class=n_class, image_tower=tower, **tower_kw)
        elif target_name == "clip":
            model = ClipViT(image_size=image_size)
        elif target_name == "resnet50":
            model = ResNet50()
        elif target_name in RESNETS:
            block, layers, classes = RESNETS[target_name]
            model = ResNet(block, layers, classes)
        elif target_name in CLIP_RESNETS:
            if not isinstance(image_size, int):
                raise ValueError("%s: image_size must be an int (the attention pool is square), got %r"
                                 % (target_name, image_size))
            layers, embed = CLIP_RESNETS[target_name]
            model = ClipResNet(layers, embed, image_size=image_size)
        elif target_name in HF_TARGETS:
            cls, width = HF_TARGETS[target_name]
            labels = hf_kw.pop("num_labels", width if width is not None else (2 if n_class is None else n_class))
            model = cls(num_labels=labels, **dict({"image_size": image_size}, **hf_kw))
        else:
            raise ValueError("unknown target model %r (offline build: breastclip, breastclip_vit, breastclip_swin, "
                             "breastclip_classifier, clip, openai_clip, clip_rn50, clip_rn101, resnet18, resnet18_places, resnet34, "
                             "resnet50, resnet101, resnet152, vit, vit-cub, vit-bloodmnist, dino, dino-cub, "
                             "dino-bloodmnist).  mae is built from a ViTMAEForPreTraining checkpoint only: pass ckpt= or "
                             "register one (register_target_checkpoint('mae', path)).  resnet, resnet-cub and resnet-bloodmnist are built "
                             "from a ResNetForImageClassification checkpoint only, clip-cub and clip-bloodmnist from a "
                             "CLIPForImageClassification checkpoint only, in the same two ways" % (target_name,))
    if target_name == "resnet18_places":
        _load_places(model, ckpt)
    else:
        _load_local(model, ckpt, text_strict=bool(text_kw), sd=hf_sd)
    _load_local(model, finetuned_ckpt)
    return model.to(device).eval(), None


class SyntheticImages(torch.utils.data.Dataset):
    """D_probe stand-in: image i is randn(3,H,W) from (seed, i) -- the same image on every rank/shard.
    Items follow the reference datasets: ((image, label)) tuples (reference data_utils.py:102-311)."""

    def __init__(self, n, size=224, seed=1234):
        self.n, self.size, self.seed = n, size, seed   # size: an int (square) or (H, W)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        return torch.randn(3, *image_hw(self.size), generator=g), 0

    def on_device(self, device, lo=0, hi=None):
        """The same kind of probe set generated ON the device and kept resident in HBM (images lo..hi-1)."""
        return DeviceSyntheticImages(self.n, self.size, self.seed, device, lo, self.n if hi is None else hi)


class DeviceSyntheticImages(torch.utils.data.Dataset):
    """Synthetic probe images generated on the GPU and resident in HBM: image i is randn(3,H,W) of a device generator
    seeded with (seed, i), so it is the same image whatever the batch size, the shard or the rank (not the same VALUES
    as the CPU SyntheticImages: the two generators are different algorithms).  The extraction loop slices batches
    straight out of the resident tensor (no DataLoader, no host round trip) -- 6 GB for 10 000 images of 224 x 224, of
    the 288 GB of an MI355X.  Holds images lo..hi-1 of the n (this rank's shard)."""

    def __init__(self, n, size, seed, device, lo=0, hi=None):
        self.n_total, self.seed = int(n), int(seed)
        self.size = image_hw(size) if isinstance(size, (tuple, list)) else int(size)   # an int (square) or (H, W)
        self.lo, self.hi = int(lo), int(self.n_total if hi is None else hi)
        self.device = torch.device(device)
        self._images = None

    def __len__(self):
        return self.hi - self.lo

    def images(self):
        if self._images is None:
            g = torch.Generator(device=self.device)
            x = torch.empty((len(self), 3) + image_hw(self.size), dtype=torch.float32, device=self.device)
            for j in range(len(self)):
                g.manual_seed(self.seed * 1000003 + self.lo + j)
                x[j].normal_(generator=g)
            self._images = x
        return self._images

    def __getitem__(self, i):
        return self.images()[i], 0

    def device_batches(self, batch_size):
        x = self.images()
        for i in range(0, x.shape[0], batch_size):
            yield x[i:i + batch_size]


# ------------------------------------------------------------------------------------------------------
# file probe sets: the reference's image datasets (data_utils.py:102-311, data/Imagenet_custom_dataloader.py)
# ------------------------------------------------------------------------------------------------------
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")     # torchvision's


def list_txt(txt_file):
    """CustomImageDatasetFromTxt (Imagenet_custom_dataloader.py:17-22): one `path label` per line, in file order."""
    samples = []
    with open(txt_file, "r") as f:
        for line in f:
            img_path, label = line.strip().split(" ")
            samples.append((img_path, int(label)))
    return samples


def list_folder(root):
    """torchvision's ImageFolder: classes = the sorted sub-directory names, label = the class's index; inside a class
    the directories in sorted order (os.walk, links followed), the files of each sorted by name, IMG_EXTENSIONS only
    (case-insensitive)."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError("no class folders in %s" % root)
    samples = []
    for label, cls in enumerate(classes):
        for d, _, names in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            for name in sorted(names):
                if name.lower().endswith(IMG_EXTENSIONS):
                    samples.append((os.path.join(d, name), label))
    return samples


# EMBED_Dataset / EMBED_marker_Dataset (Imagenet_custom_dataloader.py:55, :88): label column -> its mapping
CSV_LABELS = {"Implant_type": {"non-implant": 0, "implant": 1}, "Marker": {"No": 0, "Yes": 1}}


def list_csv(root, csv_file, label_column="Implant_type"):
    """EMBED_Dataset (label_column 'Implant_type') / EMBED_marker_Dataset ('Marker'): the CSV's rows in file order,
    path = root / filename, label mapped as the reference maps it (a value outside the mapping is NaN, pandas' map)."""
    import pandas as pd
    data = pd.read_csv(csv_file)
    if "filename" not in data.columns or label_column not in data.columns:
        raise ValueError("CSV file must contain 'filename' and '%s' columns." % label_column)
    labels = data[label_column].map(CSV_LABELS[label_column])
    return [(os.path.join(root, name), label) for name, label in zip(data["filename"], labels)]


def decode_rgb(path):
    """Image.open(path).convert("RGB") as a uint8 [H, W, 3] array: what every dataset of the reference starts from."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as img:
        return np.asarray(img.convert("RGB"), dtype=np.uint8)


# the mammogram sets: reference concept_vit/data_utils.py:114-158 (vindr, vindr_alt) and :254-298 (csaw, csaw_all_splits)
VINDR_IMG_DIR = "VinDR_MammoCLIP/images_png"
VINDR_CSV = "VinDR-data/vindr_detection_v1_folds.csv"
VINDR_DTYPES = {"patient_id": str, "image_id": str, "laterality": str, "view": str, "text1": str, "text_aug": str,
                "fold": int}                                                       # data/datamodule.py:31-39


def list_vindr(data_dir, img_dir=VINDR_IMG_DIR, csv=VINDR_CSV):
    """DataModule.valid_dataloader() of the vindr set (data/datamodule.py:53-98): the CSV data_dir / csv read with the
    reference's dtype table (patient_id stays a string: '007' is not 7), NaN -> 0, the rows with split == 'test' in file
    order.  path = data_dir / img_dir / patient_id / image_id, '.png' appended when the name does not end in it
    (image_classification_zs.py:51-63); the label is the row's Mass (the drivers ignore labels)."""
    import pandas as pd
    df = pd.read_csv(os.path.join(data_dir, csv), dtype=VINDR_DTYPES).fillna(0)
    df = df[df["split"] == "test"]
    samples = []
    for patient_id, image_id, mass in zip(df["patient_id"], df["image_id"], df["Mass"]):
        path = os.path.join(data_dir, img_dir, str(patient_id), image_id)
        samples.append((path if path.endswith(".png") else path + ".png", int(mass)))
    return samples


def list_csaw(root, csv, images, split="test"):
    """CSAWDataset (split 'test' for csaw) / CSAWDataset_all_splits (split None: every row), CSAW_dataset.py:32-48: the
    CSV root / csv in file order, path = images / anon_filename without its last four characters ('.dcm') + '.png',
    label = Cancer_visible.  The reference's loader shuffles without a seed; this one keeps the CSV's order."""
    import pandas as pd
    df = pd.read_csv(os.path.join(root, csv))
    if split is not None:
        df = df.loc[df["split"] == split]
    return [(os.path.join(images, name[:-4] + ".png"), label) for name, label in zip(df["anon_filename"], df["Cancer_visible"])]


def decode_vindr(path):
    """Image.open(path).convert('RGB') (image_classification_zs.py:72-73) with the replication left out: a mode-L file
    stays uint8 [H, W] -- .convert('RGB') of it is the same byte three times, and one byte per pixel is uploaded --
    anything else is converted to uint8 [H, W, 3]."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as img:
        if img.mode == "L":
            return np.asarray(img, dtype=np.uint8)
        return np.asarray(img.convert("RGB"), dtype=np.uint8)


def decode_csaw(path):
    """np.array(Image.open(path)) of a grey file (CSAW_dataset.py:49-52).  Mode L: uint8 [H, W], converted on the device.
    Any other 2-D mode (I;16, I, F): float32 [H, W] as the reference's np.array(image, dtype=np.float32) gives it (there
    is no 16-bit kernel).  A file that decodes to three dimensions is a ValueError (the reference's repeat fails on it)."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as img:
        arr = np.asarray(img, dtype=np.uint8) if img.mode == "L" else np.array(img, dtype=np.float32)
    if arr.ndim != 2:
        raise ValueError("csaw: %s decodes to shape %s; the set takes grey images [H, W]" % (path, arr.shape))
    return arr


def host_minmax(arr, mean, std):
    """The host route of the vindr transform and the yardstick of K23: image_classification_zs.py:81-85 in numpy on one
    uint8 [H, W, 3] (or [H, W], replicated as .convert('RGB') does) array -- float32, in-place minus min, in-place
    divided by max, then (img - mean) / std with the Python floats -- and utils.py:176's permute -> fp32 [3, H, W]."""
    import numpy as np
    img = np.asarray(arr)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    img = img.astype("float32")
    with np.errstate(invalid="ignore", divide="ignore"):      # a constant image is 0 / 0: NaN, as in the reference
        img -= img.min()
        img /= img.max()
        t = torch.tensor((img - mean) / std, dtype=torch.float32)
    return t.permute(2, 0, 1).contiguous()


def host_raw(arr):
    """The host route of the csaw transform: CSAW_dataset.py:50-52 (float32, repeated to three channels) and ToTensor,
    which on a float array is the permute alone -> fp32 [3, H, W]."""
    import numpy as np
    image = np.array(arr, dtype=np.float32)
    image = np.repeat(image[:, :, np.newaxis], 3, axis=2)
    return torch.from_numpy(image).permute(2, 0, 1).contiguous()


def host_preprocess(arr, pre):
    """The host route, and the yardstick of K22: `pre` on one uint8 [H, W, 3] array with PIL itself (Image.resize,
    Image.crop) and the three torch operations of ToTensor / Normalize -> fp32 [3, OH, OW] on the CPU.  The per-pixel
    specs go to their own host routes (host_minmax, host_raw)."""
    import numpy as np
    from PIL import Image
    if isinstance(pre, core.MinMaxNormalize):
        return host_minmax(arr, pre.mean, pre.std)
    if isinstance(pre, core.RawGray):
        return host_raw(arr)
    plan = pre.plan(arr.shape[0], arr.shape[1])
    img = Image.fromarray(np.ascontiguousarray(arr), "RGB")
    if (plan.RH, plan.RW) != (plan.H, plan.W):
        img = img.resize((plan.RW, plan.RH), {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[pre.filter])
    if (plan.OH, plan.OW) != (plan.RH, plan.RW):
        img = img.crop((plan.left, plan.top, plan.left + plan.OW, plan.top + plan.OH))
    t = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if pre.mean is not None:
        t = t.sub(torch.as_tensor(pre.mean, dtype=torch.float32)[:, None, None]).div(
            torch.as_tensor(pre.std, dtype=torch.float32)[:, None, None])
    return t


class ImageFileProbe(torch.utils.data.Dataset):
    """A probe set of image files.  samples: [(path, label)] in the reference's order (list_txt / list_folder /
    list_csv); the row order is the `images` column of the drivers' CSV.  preprocess: the target's transform (a preset
    name or a core.Preprocess); clip_preprocess: the dissector's when it differs -- every item / batch is then the pair
    (target view, dissector view) made from ONE decoded image.  decode: path -> uint8 [H, W, 3] (default decode_rgb).
    lo / hi: this rank's shard of the sample list.
    A per-pixel spec (core.MinMaxNormalize: vindr, core.RawGray: csaw) is the only view of its set; its decode
    (decode_vindr, decode_csaw) may give uint8 [H, W] as well, and its device route is K23 (core.image_minmax_normalize).

    Host route (device None): dataset[i] -> (tensor, label), PIL + torch (host_preprocess).
    Device route (a CUDA device): device_batches(batch_size) decodes on a thread pool one batch ahead, uploads the
    uint8 pixels through pinned memory and runs K22 (core.image_preprocess) once per run of consecutive same-size
    images, straight into the batch tensor(s)."""

    def __init__(self, samples, preprocess, clip_preprocess=None, decode=None, lo=0, hi=None, device=None):
        samples = list(samples)
        self.n_total = len(samples)
        self.lo, self.hi = int(lo), int(self.n_total if hi is None else hi)
        self.samples = samples[self.lo:self.hi]
        self.preprocess = core.get_preprocess(preprocess)
        clip = None if clip_preprocess is None else core.get_preprocess(clip_preprocess)
        self.clip_preprocess = None if clip == self.preprocess else clip
        pixel = [isinstance(p, (core.MinMaxNormalize, core.RawGray)) for p in self.views]
        if any(pixel) and len(pixel) > 1:
            raise ValueError("ImageFileProbe: %r is the transform of its set for both views, not one of a pair"
                             % (self.views[pixel.index(True)],))
        if decode is None:
            decode = {core.MinMaxNormalize: decode_vindr, core.RawGray: decode_csaw}.get(type(self.preprocess), decode_rgb)
        self.decode = decode
        self.device = None if device is None or torch.device(device).type != "cuda" else torch.device(device)

    @property
    def views(self):
        return [self.preprocess] + ([] if self.clip_preprocess is None else [self.clip_preprocess])

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        path, label = self.samples[i]
        arr = self.decode(path)
        out = [host_preprocess(arr, p) for p in self.views]
        return (out[0] if len(out) == 1 else tuple(out)), label

    def sample(self):
        """The first image's target view as a [1, 3, OH, OW] batch on the device (the layer-width probe)."""
        batches = self._batches(1, 1)
        try:
            return next(batches)[0]
        finally:
            batches.close()

    def device_batches(self, batch_size):
        """Batches [B, 3, OH, OW] on the device, in sample order; with two views, pairs (target, dissector) of them."""
        if self.device is None:
            raise RuntimeError("ImageFileProbe.device_batches: the probe set was built without a CUDA device")
        for out in self._batches(batch_size, len(self)):
            yield out[0] if len(out) == 1 else tuple(out)

    def _batches(self, batch_size, n):
        from concurrent.futures import ThreadPoolExecutor
        spans = [(i, min(i + batch_size, n)) for i in range(0, n, batch_size)]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            def submit(span):
                return [pool.submit(self.decode, self.samples[i][0]) for i in range(*span)]
            ahead = submit(spans[0]) if spans else None
            for k in range(len(spans)):
                arrays = [f.result() for f in ahead]
                ahead = submit(spans[k + 1]) if k + 1 < len(spans) else None     # decoded while the GPU works on batch k
                yield self._to_device(arrays)

    def _pixels_to_device(self, arrays, spec):
        """One batch of a per-pixel spec (MinMaxNormalize, RawGray): a run of consecutive images of one shape, channel
        count and dtype -> one pinned upload -> one K23 call into the batch slice.  float32 arrays (a 16-bit csaw file)
        and images past K23's limits are made on the host and uploaded."""
        sizes = {tuple(a.shape[:2]) for a in arrays}
        if len(sizes) != 1:
            raise ValueError("ImageFileProbe: %r gives images of different sizes in one batch: %s" % (spec, sorted(sizes)))
        H, W = sizes.pop()
        out = torch.empty((len(arrays), 3, H, W), dtype=torch.float32, device=self.device)
        i = 0
        while i < len(arrays):
            a = arrays[i]
            j = i + 1
            while j < len(arrays) and arrays[j].shape == a.shape and arrays[j].dtype == a.dtype:
                j += 1
            if a.dtype.name == "uint8" and a.size < 2 ** 31 and 12 * H * W < 2 ** 31:
                pinned = torch.empty((j - i,) + tuple(a.shape), dtype=torch.uint8, pin_memory=True)
                staged = pinned.numpy()
                for r in range(i, j):
                    staged[r - i] = arrays[r]
                src = pinned.to(self.device, non_blocking=True)
                core.image_minmax_normalize(src, spec.mean, spec.std, spec.mode, out=out[i:j])
            else:
                out[i:j].copy_(torch.stack([host_preprocess(b, spec) for b in arrays[i:j]]))
            i = j
        return [out]

    def _to_device(self, arrays):
        """One batch: uint8 [H, W, 3] arrays -> a [B, 3, OH, OW] device tensor per view."""
        if isinstance(self.preprocess, (core.MinMaxNormalize, core.RawGray)):
            return self._pixels_to_device(arrays, self.preprocess)
        plans = [[p.plan(a.shape[0], a.shape[1]) for a in arrays] for p in self.views]
        outs = []
        for p, pl in zip(self.views, plans):
            sizes = {(q.OH, q.OW) for q in pl}
            if len(sizes) != 1:
                raise ValueError("ImageFileProbe: %r gives images of different sizes in one batch: %s" % (p, sorted(sizes)))
            outs.append(torch.empty((len(arrays), 3) + sizes.pop(), dtype=torch.float32, device=self.device))
        i = 0
        while i < len(arrays):
            j = i + 1
            while j < len(arrays) and arrays[j].shape == arrays[i].shape:
                j += 1
            if all(pl[i].device_ok for pl in plans):
                H, W = arrays[i].shape[:2]
                pinned = torch.empty((j - i, H, W, 3), dtype=torch.uint8, pin_memory=True)
                staged = pinned.numpy()
                for r in range(i, j):
                    staged[r - i] = arrays[r]
                src = pinned.to(self.device, non_blocking=True)            # ONE upload feeds every view
                for p, out in zip(self.views, outs):
                    core.image_preprocess(src, p, out=out[i:j])
            else:      # past K22's limits (core.ImagePlan.device_ok): this run is made on the host and uploaded
                for p, out in zip(self.views, outs):
                    out[i:j].copy_(torch.stack([host_preprocess(a, p) for a in arrays[i:j]]))
            i = j
        return outs


# name -> how the reference's get_data builds the set (data_utils.py:106-113, :169-251, :304-309) and the transform it
# gets when the caller passes none.  Paths are not part of the package: register_dataset, or a JSON file named by
# MCD_DATASETS ({name: {"path": ..} | {"root": .., "csv": ..}}).
DATASET_KINDS = {"imagenet_subsets": ("txt", "tensor"), "imagenet_val": ("folder", "imagenet"),
                 "broden": ("folder", "imagenet"), "imagenet_broden": ("concat", "imagenet"),
                 "embed_png": ("csv:Implant_type", "embed"), "embed_marker_84": ("csv:Marker", "embed"),
                 "embed_implant": ("csv:Implant_type", "embed"), "embed_marker_only": ("csv:Marker", "embed"),
                 "embed_non_implant": ("csv:Implant_type", "embed"), "embed_non_implant_100": ("csv:Implant_type", "embed"),
                 "vindr": ("vindr", "vindr"), "vindr_alt": ("vindr", "vindr"),
                 "csaw": ("csaw:test", "csaw"), "csaw_all_splits": ("csaw:", "csaw")}
# the mammogram sets always use their own transform, for the target and for the dissector: the reference's get_data
# ignores `preprocess` for them and one loader feeds both models (utils.py:523-551)
FIXED_TRANSFORM = ("vindr", "vindr_alt", "csaw", "csaw_all_splits")
# a set that is registered under another name: the reference's two differ in returning a loader or its dataset
# (vindr_alt) or in the split filter (csaw_all_splits)
REGISTERED_AS = {"vindr_alt": "vindr", "csaw_all_splits": "csaw"}
CONCAT_PARTS = {"imagenet_broden": ("imagenet_val", "broden")}
DATASET_ROOTS = {}


def register_dataset(name, path=None, root=None, csv=None, kind=None, default_preprocess=None):
    """Where a probe set lives: `path` (the text file of a 'txt' set, the class-folder tree of a 'folder' set) or
    `root` + `csv` (a 'csv:<label column>' set).  kind / default_preprocess: for a name the reference does not have.
    vindr: root = the reference's data_dir; path (the image folder) and csv are relative to it and default to the
    reference's VINDR_IMG_DIR and VINDR_CSV.  csaw: root, csv (relative to root) and path (the image folder, taken as it
    is: the reference's imagefolder_path)."""
    if name not in DATASET_KINDS:
        if kind is None:
            raise ValueError("register_dataset: %r is not one of the reference's probe sets; give its kind "
                             "('txt', 'folder', 'csv:Implant_type' or 'csv:Marker')" % (name,))
        DATASET_KINDS[name] = (kind, default_preprocess or "imagenet")
    DATASET_ROOTS[name] = {"path": path, "root": root, "csv": csv}


def _registered(name):
    entry = DATASET_ROOTS.get(name)
    table = os.environ.get("MCD_DATASETS")
    if entry is None and table:
        import json
        with open(table) as f:
            entry = json.load(f).get(name)
    return entry


def _list_samples(name):
    kind = DATASET_KINDS[name][0]
    if kind == "concat":
        return [s for part in CONCAT_PARTS[name] for s in _list_samples(part)]
    entry = _registered(name)
    if entry is None and name in REGISTERED_AS:
        entry = _registered(REGISTERED_AS[name])
    if entry is None:
        raise ValueError("dataset %r has no path: register_dataset(%r, ...) or name a JSON table in MCD_DATASETS"
                         % (name, name))
    if kind == "vindr" or kind.startswith("csaw:"):
        return _list_mammo(name, kind, entry)
    paths = [entry.get("root"), entry.get("csv")] if kind.startswith("csv:") else [entry.get("path")]
    for p in paths:
        if p is None or not os.path.exists(p):
            raise FileNotFoundError("dataset %r: %s does not exist" % (name, p))
    if kind == "txt":
        return list_txt(paths[0])
    if kind == "folder":
        return list_folder(paths[0])
    return list_csv(paths[0], paths[1], kind[len("csv:"):])


def _list_mammo(name, kind, entry):
    root = entry.get("root")
    if kind == "vindr":
        img_dir, csv = entry.get("path") or VINDR_IMG_DIR, entry.get("csv") or VINDR_CSV
    else:
        img_dir, csv = entry.get("path"), entry.get("csv")
    under = [csv, img_dir] if kind == "vindr" else [csv]          # csaw's image folder is a path of its own, as in the reference
    needed = [root] + [None if p is None or root is None else os.path.join(root, p) for p in under]
    for p in needed if kind == "vindr" else needed + [img_dir]:
        if p is None or not os.path.exists(p):
            raise FileNotFoundError("dataset %r: %s does not exist" % (name, p))
    if kind == "vindr":
        return list_vindr(root, img_dir, csv)
    return list_csaw(root, csv, img_dir, kind[len("csaw:"):] or None)


def target_preset(target_name):
    """The transform the reference's get_target_model hands back with a target (data_utils.py:38-93): none for the
    Mammo-CLIP models, the ImageNet one for everything else."""
    return None if target_name.startswith("breastclip") else "imagenet"


def get_data(dataset_name, preprocess=None, device=None, lo=0, hi=None, clip_preprocess=None):
    """'synthetic_<N>', 'synthetic_<N>_<size>' (e.g. synthetic_10000_224) or 'synthetic_<N>_<H>x<W>' (H rows, W columns,
    e.g. synthetic_64_1520x912): with a CUDA `device` the probe set is generated on the device and stays resident there
    (DeviceSyntheticImages); lo/hi select a rank's shard of it.
    The reference's file sets (DATASET_KINDS: imagenet_subsets, imagenet_val, broden, imagenet_broden, embed_*, and the
    mammogram sets vindr, vindr_alt, csaw, csaw_all_splits, which keep their own transform: K23, FIXED_TRANSFORM) once
    their paths are registered: an ImageFileProbe over images lo..hi-1.  preprocess / clip_preprocess: a preset name, a
    core.Preprocess or None (preprocess: the set's own default, 'tensor', 'imagenet' or 'embed' as in the reference;
    clip_preprocess: no second view; 'default' there names the set's own default).  With a CUDA `device` the set
    preprocesses on the GPU (K22)."""
    if dataset_name.startswith("synthetic"):
        parts = dataset_name.split("_")
        n = int(parts[1]) if len(parts) > 1 else 256
        size = _parse_hw(parts[2]) if len(parts) > 2 else 224
        if size is None:
            raise ValueError("dataset %r: the size is <S> or <H>x<W>" % (dataset_name,))
        ds = SyntheticImages(n, size)
        if device is not None and torch.device(device).type == "cuda":
            return ds.on_device(device, lo, hi)
        if lo != 0 or (hi is not None and hi != n):
            return torch.utils.data.Subset(ds, range(lo, n if hi is None else hi))
        return ds
    if dataset_name in DATASET_KINDS:
        default = DATASET_KINDS[dataset_name][1]
        if dataset_name in FIXED_TRANSFORM:
            for given in (preprocess, clip_preprocess):
                if not (given is None or (isinstance(given, str) and given == "default")
                        or core.get_preprocess(given) == core.PRESETS[default]):
                    raise ValueError("dataset %r always uses its own transform %r for the target and for the dissector "
                                     "(the reference ignores `preprocess` for it); got %r"
                                     % (dataset_name, core.PRESETS[default], given))
            return ImageFileProbe(_list_samples(dataset_name), default, None, lo=lo, hi=hi, device=device)
        if isinstance(clip_preprocess, str) and clip_preprocess == "default":
            clip_preprocess = default
        return ImageFileProbe(_list_samples(dataset_name), default if preprocess is None else preprocess,
                              clip_preprocess, lo=lo, hi=hi, device=device)
    if dataset_name == "combined":
        raise ValueError("dataset 'combined' is not available offline: it mixes imagenet_subsets (224 x 224) and vindr_alt "
                         "(1520 x 912) in one loader, and a batch here holds images of one size; dissect the two sets apart")
    raise ValueError("dataset %r is not available offline; use synthetic_<N>[_<size> | _<H>x<W>] or one of %s"
                     % (dataset_name, ", ".join(sorted(DATASET_KINDS))))
