"""Tensor-level wrappers over the C ABI (include/mcd_hip.h).

Every function takes torch tensors that already live in HBM, passes their device pointers and
strides to libmcd_hip.so on torch's current stream, and returns torch tensors.  torch is used for
memory and streams only; all arithmetic happens in the HIP kernels.  Nothing here runs on the CPU:
a CPU tensor is a TypeError, a missing library an ImportError.
"""
import ctypes
import functools

import torch

from . import _lib
from ._lib import McdError, check  # noqa: F401

POOL_MODES = {"avg": 0, "max": 1, "cls": 2, "none": 3}
POOL_SILU_AVG = 4      # mcd_hook_pool_nhwc only
GEMM_MODES = {"f32": 0, "bf16x3": 1, "bf16": 2}


def _stream():
    """torch's current stream of the CURRENT device; every wrapper runs under _on_device, which makes the tensors'
    device current first."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_device(fn):
    """Run `fn` with the device of its tensor arguments current: the library launches on torch's current stream and
    keeps its one-time kernel attributes per HIP device, so a call on tensors of cuda:1 from a process whose current
    device is cuda:0 must switch first.  Tensors on different devices are an error (no silent peer access)."""
    @functools.wraps(fn)
    def wrapper(*args, **kw):
        dev = None
        for a in list(args) + list(kw.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise ValueError("%s: tensors on different devices (%s and %s)" % (fn.__name__, dev, a.device))
        if dev is None:
            return fn(*args, **kw)          # CPU or no tensors: the wrapper's own checks raise
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return wrapper


def _need_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError("mammo-clip-dissect_amd runs on the GPU only: expected a CUDA/HIP tensor, got %s"
                            % (t.device if isinstance(t, torch.Tensor) else type(t)))


def _f32_rows(t, name):
    """2-D fp32 tensor with unit inner stride (a row-major matrix with leading dimension stride(0))."""
    _need_gpu(t)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if t.dim() != 2:
        raise ValueError("%s must be 2-D, got shape %s" % (name, tuple(t.shape)))
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _f32_out(t, name):
    """An OUTPUT matrix: the kernel must write into the caller's memory, so a layout the ABI cannot address is an
    error, never a silent copy."""
    _need_gpu(t)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError("%s must be a 2-D float32 tensor" % name)
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("%s must have unit inner stride and a leading dimension >= its width (strides %s)"
                         % (name, tuple(t.stride())))
    return t


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _dense(t, message, dim=None, shape=None, device=None):
    """t must be a contiguous float32 tensor -- of `dim` dimensions, of exactly `shape`, on `device`, where given;
    TypeError(message) otherwise.  Returns t's shape.  That t is a GPU tensor at all is _need_gpu's to say."""
    got = t.shape
    if (t.dtype != torch.float32 or (dim is not None and len(got) != dim) or (shape is not None and got != shape)
            or not t.is_contiguous() or (device is not None and t.device != device)):
        raise TypeError(message)
    return got


def _key_counts(lens, B, device, name):
    """The optional key counts of K9M, K9B and K27: None, or a contiguous int32 [B] tensor on `device`, the device of the
    operand the message calls `name`."""
    if lens is not None and (lens.dtype != torch.int32 or lens.shape != (B,) or not lens.is_contiguous()
                             or lens.device != device):
        raise TypeError("lens must be a contiguous int32 [B] tensor on %s's device (or None)" % name)


def _out(out, shape, device, message, dense=True):
    """The caller's `out` -- float32, of `shape`, contiguous (dense=False: a unit inner stride is enough), or
    TypeError(message) -- or, for None, a new contiguous tensor on `device`."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or out.shape != shape or not (out.is_contiguous() if dense else out.stride(-1) == 1):
        raise TypeError(message)
    return out


def _ptr(t):
    """The address of an optional operand: NULL for None."""
    return None if t is None else t.data_ptr()


def _nchw_image(x, message):
    """x must be a contiguous fp32 NCHW image batch on the GPU; TypeError(message) otherwise."""
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise TypeError(message)
    return x


def _aligned16(message, *tensors):
    """The kernels read these with 16-byte vector loads; ValueError(message) if one of them cannot be."""
    if any(t.data_ptr() % 16 for t in tensors):
        raise ValueError(message)


def channels_last(x, only=False):
    """x is a 4-D tensor whose memory is channels-last contiguous.  only=True: and not NCHW-contiguous as well (one
    channel, or one pixel, is both), i.e. the layout has to be handled as channels-last."""
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not (only and x.is_contiguous())


def sum_split(C):
    """ATen torch.sum(dim=0) CPU rule: columns below use the cascade order, the rest row_sum."""
    return (C // 32) * 32 if C >= 8 else (C // 4) * 4


def pad_cols(C, mult=64):
    return (C + mult - 1) // mult * mult


# ---- K1a / K1 ----------------------------------------------------------------------------------
@_on_device
def normalize_rows(x, out=None):
    """y = x / ||x||_2 per row (utils.py:577-578).  out may be x itself (in place)."""
    x = _f32_rows(x, "x")
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    out = _f32_out(out, "out")
    L = _lib.load()
    check(L.mcd_normalize_rows(x.data_ptr(), _ld(x), x.shape[0], x.shape[1], out.data_ptr(), _ld(out), _stream()))
    return out


@_on_device
def center_cube_normalize_rows(x, min_norm=1e-3, out=None):
    """Rows centred, cubed and scaled to unit norm (norm clipped at min_norm): similarity.py:15-22 with the
    image axis contiguous."""
    x = _f32_rows(x, "x")
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    out = _f32_out(out, "out")
    L = _lib.load()
    check(L.mcd_center_cube_normalize_rows(x.data_ptr(), _ld(x), x.shape[0], x.shape[1], float(min_norm), out.data_ptr(),
                                           _ld(out), _stream()))
    return out


PREP_MODES = {"normalize": 0, "center_cube": 1}


@_on_device
def prepare_rows_gathered(src, counts, rows, mode, min_norm=1e-3, out=None):
    """normalize_rows (mode "normalize") or center_cube_normalize_rows (mode "center_cube") of logical rows that arrive in
    pieces.  src: [G, R, ld] (the rank-major message of an all-gather: block g = rank g's [R, ld] rows, their first
    counts[g] columns valid) or a 2-D [R, >= counts[0]] matrix for G = 1.  rows = (row0, row1).  Logical row u is the
    concatenation of src[g, u, :counts[g]] over g; returns the prepared rows row0..row1-1 as [row1 - row0, sum(counts)],
    bit-equal to the one-piece kernels on the concatenated rows."""
    _need_gpu(src)
    if src.dtype != torch.float32 or src.dim() not in (2, 3) or (src.shape[-1] > 1 and src.stride(-1) != 1):
        raise TypeError("src must be a float32 [R, ld] or [G, R, ld] tensor with unit inner stride")
    if src.dim() == 2:
        src = src.unsqueeze(0)
    G, R, _ = src.shape
    counts = [int(c) for c in counts]
    if len(counts) != G or any(c < 0 or c > src.shape[2] for c in counts):
        raise ValueError("counts %s do not fit %d blocks of %d columns" % (counts, G, src.shape[2]))
    row0, row1 = int(rows[0]), int(rows[1])
    if not 0 <= row0 <= row1 <= R:
        raise ValueError("rows [%d, %d) outside the %d rows of src" % (row0, row1, R))
    n = sum(counts)
    ld_src = src.stride(1) if R > 1 else src.shape[2]
    ld_block = src.stride(0) if G > 1 else R * ld_src
    if out is None:
        out = torch.empty((row1 - row0, n), dtype=torch.float32, device=src.device)
    out = _f32_out(out, "out")
    arr = (ctypes.c_int64 * G)(*counts)
    L = _lib.load()
    check(L.mcd_prepare_rows_gathered(src.data_ptr(), ld_src, ld_block, G, arr, n, row0, row1, PREP_MODES[mode],
                                      float(min_norm), out.data_ptr(), _ld(out), _stream()))
    return out


@_on_device
def embed_gemm(I, T, mode="f32", out=None, use_workspace=True):
    """P = I @ T.T for I [N,D], T [C,D] (utils.py:594).  mode: "f32" (the parity mode: exact fp32 fma chains
    over the K-blocks MKL's sgemm uses, so P equals torch's CPU matmul to the bit),
    "bf16x3" (split bf16, fp32-class accuracy) or "bf16" (single pass, stress configuration only)."""
    I = _f32_rows(I, "I")
    T = _f32_rows(T, "T")
    if I.shape[1] != T.shape[1]:
        raise RuntimeError("mat1 and mat2 shapes cannot be multiplied (%dx%d and %dx%d)"
                           % (I.shape[0], I.shape[1], T.shape[1], T.shape[0]))
    N, D = I.shape
    C = T.shape[0]
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=I.device)
    out = _f32_out(out, "out")
    L = _lib.load()
    nws = L.mcd_embed_gemm_workspace(N, C, D, GEMM_MODES[mode]) if use_workspace else 0
    ws = torch.empty((nws,), dtype=torch.uint8, device=I.device) if nws else None
    check(L.mcd_embed_gemm(I.data_ptr(), _ld(I), T.data_ptr(), _ld(T), N, C, D, GEMM_MODES[mode], out.data_ptr(),
                           _ld(out), ws.data_ptr() if ws is not None else None, nws, _stream()))
    return out


# ---- K1s / K4s: the stress chain (bf16, no parity claim) ----------------------------------------------------
@_on_device
def embed_gemm_exp(I, T, a, normalize=False):
    """K1 + K2 of the stress configuration in one kernel that never writes fp32 P (utils.py:594 + similarity.py:54):
    returns (E, rinv) with E = bf16(exp(a (I @ T.T - 1))) as a [N, C] view of a buffer whose rows are padded with zeros
    to a multiple of 128 concepts, and rinv[n] = 1 / rowsum, so that softmax(a P) = E * rinv[:, None].  I and T must
    be row-normalised, or raw embeddings with normalize=True (utils.py:577-578 folded into the bf16 conversion)."""
    I = _f32_rows(I, "I")
    T = _f32_rows(T, "T")
    if I.shape[1] != T.shape[1]:
        raise RuntimeError("mat1 and mat2 shapes cannot be multiplied (%dx%d and %dx%d)"
                           % (I.shape[0], I.shape[1], T.shape[1], T.shape[0]))
    N, D = I.shape
    C = T.shape[0]
    ldE = pad_cols(C, 128)
    E = torch.empty((N, ldE), dtype=torch.bfloat16, device=I.device)
    rinv = torch.empty((N,), dtype=torch.float32, device=I.device)
    L = _lib.load()
    nws = L.mcd_embed_gemm_exp_workspace(N, C, D)
    ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=I.device)
    check(L.mcd_embed_gemm_exp(I.data_ptr(), _ld(I), T.data_ptr(), _ld(T), N, C, D, float(a), 1 if normalize else 0, E.data_ptr(), ldE,
                               rinv.data_ptr(), ws.data_ptr(), nws, _stream()))
    return E[:, :C], rinv


@_on_device
def wpmi_score_bf16(E, rinv, idx, p, min_prob, soft, out=None):
    """K4 on the stress chain's representation: pdge[u,c] = sum_j log(term(E[idx[u,j], c] * rinv[idx[u,j]])).
    E: the [N, C] bf16 view embed_gemm_exp returns (rows padded to a multiple of 128); idx [U,K] int32."""
    _need_gpu(E, rinv, idx)
    if E.dtype != torch.bfloat16 or E.dim() != 2 or (E.shape[1] > 1 and E.stride(1) != 1) or E.stride(0) % 128 != 0:
        raise TypeError("E must be a bfloat16 [N, C] view with unit inner stride and rows padded to a multiple of 128")
    if rinv.dtype != torch.float32 or rinv.numel() != E.shape[0] or not rinv.is_contiguous():
        raise TypeError("rinv must be N contiguous float32 values")
    if idx.dtype != torch.int32 or idx.dim() != 2 or (idx.shape[1] > 1 and idx.stride(1) != 1):
        raise TypeError("idx must be a [U,K] int32 tensor with unit inner stride")
    N, C = E.shape
    U, K = idx.shape
    if out is None:
        out = torch.empty((U, C), dtype=torch.float32, device=E.device)
    out = _f32_out(out, "out")
    if soft:
        _need_gpu(p)
        if p.dtype != torch.float32 or p.numel() != K:
            raise TypeError("p must be K float32 values")
        p = p.contiguous()
    L = _lib.load()
    nws = int(L.mcd_wpmi_score_bf16_workspace(U, K))
    ws = torch.empty(max(nws, 8) // 8, dtype=torch.int64, device=E.device)
    check(L.mcd_wpmi_score_bf16(E.data_ptr(), E.stride(0), N, C, rinv.data_ptr(), idx.data_ptr(),
                                idx.stride(0) if U > 1 else K, U, K, p.data_ptr() if soft else None, float(min_prob),
                                1 if soft else 0, out.data_ptr(), _ld(out), ws.data_ptr(), nws, _stream()))
    return out


# ---- K2 ------------------------------------------------------------------------------------------
@_on_device
def row_softmax(P, a, pad_to=192):
    """S = softmax(a*P, dim=1) (similarity.py:54) into a buffer whose leading dimension is padded to a
    multiple of `pad_to` floats (padding columns are 0).  Returns the [N, C] view of that buffer.
    192 = lcm(64, 96): whole 96-concept slices for K4's XCD-sliced kernel at any C (763 -> 768, 10 000 -> 10 176)."""
    P = _f32_rows(P, "clip_feats")
    N, C = P.shape
    ldS = pad_cols(C, pad_to) if pad_to else C
    S = torch.empty((N, ldS), dtype=torch.float32, device=P.device)
    L = _lib.load()
    check(L.mcd_row_softmax(P.data_ptr(), _ld(P), N, C, float(a), S.data_ptr(), ldS, _stream()))
    return S[:, :C]


# ---- K3 ------------------------------------------------------------------------------------------
@_on_device
def col_topk(A, K, neuron_major=False, want_vals=True):
    """Per neuron, the K most activating images, sorted descending (similarity.py:55).

    A is image-major [N,U] (what the reference passes) or, with neuron_major=True, [U,N].
    Returns (vals [U,K] float32 or None, idx [U,K] int32) -- neuron-major, i.e. torch.topk(A, K, dim=0)
    transposed.  K > N raises RuntimeError like torch.topk.
    """
    A = _f32_rows(A, "target_feats")
    if neuron_major:
        U, N = A.shape
        sn, su = 1, _ld(A)
    else:
        N, U = A.shape
        sn, su = _ld(A), 1
    L = _lib.load()
    K = int(K)
    idx = torch.empty((U, K), dtype=torch.int32, device=A.device)
    vals = torch.empty((U, K), dtype=torch.float32, device=A.device) if want_vals else None
    ws_bytes = L.mcd_col_topk_workspace(N, U, sn, su, K) if (N > 0 and K >= 1) else 0
    ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.float32, device=A.device)
    rc = L.mcd_col_topk(A.data_ptr(), N, U, sn, su, K, vals.data_ptr() if want_vals else None, idx.data_ptr(),
                        K, ws.data_ptr(), ws_bytes, _stream())
    if rc == _lib.MCD_E_RANGE:
        raise RuntimeError("selected index k out of range")
    check(rc)
    return vals, idx


@_on_device
def transpose(A, out=None):
    """image-major [N,U] -> neuron-major [U,N]."""
    A = _f32_rows(A, "A")
    N, U = A.shape
    if out is None:
        out = torch.empty((U, N), dtype=torch.float32, device=A.device)
    out = _f32_out(out, "out")
    L = _lib.load()
    check(L.mcd_transpose(A.data_ptr(), _ld(A), N, U, out.data_ptr(), _ld(out), _stream()))
    return out


# ---- K4 / K5 -------------------------------------------------------------------------------------
@_on_device
def wpmi_score(S, idx, p, min_prob, soft, split=-1, out=None, fast_log=False, s_is_prob=False):
    """pdge[u,c] = sum_j log(term(S[idx[u,j], c])) (similarity.py:59-65, 84-88); idx is [U,K] int32.
    fast_log=True trades the accurate (near correctly rounded) log for the v_log_f32 based one (<= ~1.5 ulp).
    s_is_prob=True promises S in [0,1] (it came from row_softmax) and p in [0,1]: the log-table range check is skipped."""
    S = _f32_rows(S, "S")
    _need_gpu(idx)
    if idx.dtype != torch.int32 or idx.dim() != 2 or (idx.shape[1] > 1 and idx.stride(1) != 1):
        raise TypeError("idx must be a [U,K] int32 tensor with unit inner stride")
    N, C = S.shape
    U, K = idx.shape
    if out is None:
        out = torch.empty((U, C), dtype=torch.float32, device=S.device)
    out = _f32_out(out, "out")
    if soft:
        _need_gpu(p)
        if p.dtype != torch.float32 or p.numel() != K:
            raise TypeError("p must be K float32 values")
        p = p.contiguous()
    L = _lib.load()
    check(L.mcd_wpmi_score(S.data_ptr(), _ld(S), N, C, idx.data_ptr(), idx.stride(0) if U > 1 else K, U, K,
                           p.data_ptr() if soft else None, float(min_prob), (1 if soft else 0) | (2 if fast_log else 0) | (4 if s_is_prob else 0), int(split),
                           out.data_ptr(), _ld(out), _stream()))
    return out


@_on_device
def logsumexp_sub(pdge, lam, seg_offsets=None, split=-1, out=None):
    """out = pdge - lam*(logsumexp(pdge, 0) - log U), per row segment (one segment per layer)."""
    pdge = _f32_rows(pdge, "pdge")
    U, C = pdge.shape
    if seg_offsets is None:
        seg_offsets = [0, U]
    if out is None:
        out = torch.empty((U, C), dtype=torch.float32, device=pdge.device)
    out = _f32_out(out, "out")
    L = _lib.load()
    for s0 in range(0, len(seg_offsets) - 1, 64):  # the ABI takes at most 64 segments per call
        seg = list(seg_offsets[s0:s0 + 65])
        arr = (ctypes.c_int64 * len(seg))(*seg)
        ws_bytes = L.mcd_logsumexp_sub_workspace(seg[-1] - seg[0], C, len(seg) - 1)
        ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.float32, device=pdge.device)
        check(L.mcd_logsumexp_sub(pdge.data_ptr(), _ld(pdge), C, arr, len(seg) - 1, float(lam), int(split),
                                  out.data_ptr(), _ld(out), ws.data_ptr(), ws_bytes, _stream()))
    return out


# ---- K6 ------------------------------------------------------------------------------------------
@_on_device
def row_topk(sim, k):
    """torch.topk(sim, k, dim=1) (k=1: torch.max(sim, dim=1)); returns (vals [U,k], idx [U,k] int32)."""
    sim = _f32_rows(sim, "similarities")
    U, C = sim.shape
    k = int(k)
    vals = torch.empty((U, k), dtype=torch.float32, device=sim.device)
    idx = torch.empty((U, k), dtype=torch.int32, device=sim.device)
    L = _lib.load()
    rc = L.mcd_row_topk(sim.data_ptr(), _ld(sim), U, C, k, vals.data_ptr(), idx.data_ptr(), _stream())
    if rc == _lib.MCD_E_RANGE:
        raise RuntimeError("selected index k out of range")
    check(rc)
    return vals, idx


# ---- K8 ------------------------------------------------------------------------------------------
@_on_device
def rank_reorder(P, tvals, tidx, perms, p=3, scale_p=0.5, out=None):
    """rank_reorder scores of one layer (similarity.py:107-132).  tvals/tidx: [U, top_n] from col_topk (descending
    activations, image indices); perms: int32 [U, n_perm, top_n] baseline permutations.  Returns [U, C]."""
    P = _f32_rows(P, "P")
    N, C = P.shape
    if _ld(P) % 4 != 0 or P.data_ptr() % 16 != 0:     # 16-byte gathers need rows padded to whole quads
        Pp = torch.zeros((N, pad_cols(C, 4)), dtype=torch.float32, device=P.device)
        Pp[:, :C] = P
        P = Pp[:, :C]
    tvals = _f32_rows(tvals, "tvals")
    _need_gpu(tidx, perms)
    U, top_n = tvals.shape
    if tidx.dtype != torch.int32 or tuple(tidx.shape) != (U, top_n) or perms.dtype != torch.int32 or perms.dim() != 3 \
            or perms.shape[0] != U or perms.shape[2] != top_n:
        raise ValueError("tidx must be int32 [U, top_n] and perms int32 [U, n_perm, top_n]")
    tidx = tidx.contiguous()
    tvals = tvals.contiguous()
    perms = perms.contiguous()
    if out is None:
        out = torch.empty((U, C), dtype=torch.float32, device=P.device)
    out = _f32_out(out, "out")
    ws = torch.empty((max(U, 1),), dtype=torch.float32, device=P.device)
    L = _lib.load()
    check(L.mcd_rank_reorder(P.data_ptr(), _ld(P), N, C, tvals.data_ptr(), tidx.data_ptr(), top_n, U, top_n,
                             perms.data_ptr(), perms.shape[1], float(p), float(scale_p), ws.data_ptr(), out.data_ptr(),
                             _ld(out), _stream()))
    return out


# ---- K9 ------------------------------------------------------------------------------------------
VIT_ATTENTION_MAX_T = 256


def _attention(entry, qkv, heads, out, *masks):
    """The argument checks and the output of the K9 family, then the library entry `entry`.  masks: the optional operands
    an entry takes between H and out -- (lens,) for K9M, (lens, rel) for K9B -- each a tensor or None."""
    _need_gpu(qkv, *masks)
    B, T, W = _dense(qkv, "qkv must be a contiguous float32 [B, T, 3*heads*64] tensor", 3)
    if W != 3 * heads * 64:
        raise ValueError("qkv last dimension %d is not 3 * %d heads * 64" % (W, heads))
    device = qkv.device
    if masks:
        _key_counts(masks[0], B, device, "qkv")
        if len(masks) == 2 and masks[1] is not None:
            _dense(masks[1], "rel must be a contiguous float32 [heads, 2T-1] tensor on qkv's device (or None)",
                   shape=(heads, 2 * T - 1), device=device)
    out = _out(out, (B, T, heads * 64), device, "out must be a contiguous float32 [B, T, heads*64] tensor")
    check(getattr(_lib.load(), entry)(qkv.data_ptr(), B, T, heads, *map(_ptr, masks), out.data_ptr(), _stream()))
    return out


@_on_device
def vit_attention(qkv, heads, out=None):
    """softmax(q k^T / 8) v per head for the ViT tower: qkv [B, T, 3*heads*64] (the fused projection's output,
    q | k | v along the last axis, heads inside each) -> [B, T, heads*64].  fp32, head dimension 64, T <= 256."""
    return _attention("mcd_vit_attention", qkv, heads, out)


VIT_ATTENTION_LONG_MAX_T = 32768


@_on_device
def vit_attention_long(qkv, heads, out=None):
    """vit_attention for any T from 1 to VIT_ATTENTION_LONG_MAX_T (K9L): the same layout and arithmetic, one workgroup
    per 256 queries of a head; for T <= 256 the same bits as vit_attention.  Allocates only the [B, T, heads*64] output
    (no T x T scores)."""
    return _attention("mcd_vit_attention_long", qkv, heads, out)


# ---- K9M -----------------------------------------------------------------------------------------
@_on_device
def vit_attention_keylen(qkv, heads, lens, out=None):
    """vit_attention with a key count per sequence (K9M, include/mcd_text.h): qkv [B, T, 3*heads*64], T <= 256; lens a
    contiguous int32 [B] tensor on qkv's device, or None (every length is T: vit_attention's bits).  Sequence b attends to
    keys 0 .. L-1, L = clamp(lens[b], 1, T) -- the kernel clamps, the values are not read back.  Every query row is
    computed, padded ones included; no K or V row >= L is read."""
    return _attention("mcd_vit_attention_keylen", qkv, heads, out, lens)


# ---- K9B -----------------------------------------------------------------------------------------
@_on_device
def vit_attention_relbias(qkv, heads, lens, rel, out=None):
    """vit_attention_keylen with a bias per head and key-minus-query distance added to the scores (K9B,
    include/mcd_sentence.h): rel a contiguous float32 [heads, 2T-1] tensor, rel[h, (j - t) + T - 1] the bias of key j for
    query t, or None (vit_attention_keylen's bits).  Valid rows t < L attend to the L valid keys; the padded query rows are
    written but carry a clamped bias -- nothing may read them.  Of rel only the distances |d| < L of a sequence are read."""
    return _attention("mcd_vit_attention_relbias", qkv, heads, out, lens, rel)


# ---- K27 -----------------------------------------------------------------------------------------
@_on_device
def masked_mean_l2(x, lens, normalize=True, out=None):
    """The mean of the first L = clamp(lens[b], 1, T) token rows of every sequence, L2-normalised unless normalize is
    False, in one launch (K27, include/mcd_sentence.h): x a contiguous float32 [B, T, D] tensor, lens a contiguous int32
    [B] tensor on x's device or None (L = T) -> [B, D].  sentence-transformers' Pooling(mean) + Normalize."""
    _need_gpu(x, lens, out)
    B, T, D = _dense(x, "x must be a contiguous float32 [B, T, D] tensor", 3)
    device = x.device
    _key_counts(lens, B, device, "x")
    out = _out(out, (B, D), device, "out must be a contiguous float32 [B, D] tensor")
    check(_lib.load().mcd_masked_mean_l2(x.data_ptr(), B, T, D, _ptr(lens), 1 if normalize else 0, out.data_ptr(), _stream()))
    return out


# ---- K9A -----------------------------------------------------------------------------------------
@_on_device
def vit_attention_causal(qkv, heads, out=None):
    """vit_attention under a causal mask (K9A, include/mcd_clip.h): query t attends to keys 0 .. t.  The same layout and
    limits (T <= 256); row t carries the bits of vit_attention on the sequence truncated to t + 1 tokens."""
    return _attention("mcd_vit_attention_causal", qkv, heads, out)


# ---- K25 -----------------------------------------------------------------------------------------
@_on_device
def quick_gelu(x, out=None):
    """x * sigmoid(1.702 x) in one launch (K25, include/mcd_clip.h): x a contiguous float32 tensor of any shape; out None
    (a new tensor), x itself (in place) or another contiguous float32 tensor of x's shape."""
    _need_gpu(x, out)
    shape = _dense(x, "x must be a contiguous float32 tensor")
    out = _out(out, shape, x.device, "out must be a contiguous float32 tensor of x's shape")
    check(_lib.load().mcd_quick_gelu(x.data_ptr(), x.numel(), out.data_ptr(), _stream()))
    return out


# ---- K26 -----------------------------------------------------------------------------------------
@_on_device
def token_mean(x, t0=1, out=None):
    """The mean of the tokens t0 .. T-1 of every image in one launch (K26, include/mcd_tokens.h): x a float32 [B, T, D]
    tensor with a unit inner stride -- contiguous, or a view whose tokens and images lie further apart -- -> [B, D];
    out None (a new tensor) or a float32 [B, D] tensor with a unit inner stride (a row-strided view too).  t0 = 1 is
    x[:, 1:].mean(dim=1), the mean of a ViT's patch tokens.  The entry checks widths, strides, alignment and overlap."""
    _need_gpu(x, out)
    strides = x.stride()
    if x.dtype != torch.float32 or len(strides) != 3 or strides[2] != 1:
        raise TypeError("x must be a float32 [B, T, D] tensor with a unit inner stride")
    B, T, D = x.shape
    out = _out(out, (B, D), x.device, "out must be a float32 [B, D] tensor with a unit inner stride", False)
    check(_lib.load().mcd_token_mean(x.data_ptr(), B, T, D, strides[0], strides[1], t0, out.data_ptr(), out.stride(0),
                                     _stream()))
    return out


# ---- K9C -----------------------------------------------------------------------------------------
VIT_ATTENTION_CLS_MAX_T = 32768


@_on_device
def vit_attention_cls(q, k, v, out=None):
    """softmax(q k^T / 8) v per head for ONE query row per image (K9C): q [B, heads, 64] or [B, heads*64], k and v
    [B, T, heads, 64] -> [B, heads*64].  The operands are read where they lie: q rows any distance apart, k and v with
    any token (dim 1) and image (dim 0) strides, as long as a token's heads*64 floats are adjacent -- views of a
    [B, T, 2, heads, 64] K|V projection or of a [B, T, 3, heads, 64] qkv.  fp32, 1 <= T <= VIT_ATTENTION_CLS_MAX_T."""
    _need_gpu(q, k, v, out)
    if any(t.dtype != torch.float32 for t in (q, k, v)) or k.dim() != 4 or k.shape[3] != 64 or v.shape != k.shape:
        raise TypeError("vit_attention_cls: float32 k and v of one shape [B, T, heads, 64]")
    B, T, H, _ = k.shape
    qs, kvs = q.stride(), (k.stride(), v.stride())
    if q.dim() == 3:
        if tuple(q.shape) != (B, H, 64) or (H > 1 and qs[1] != 64):
            raise ValueError("vit_attention_cls: q must be [B, heads, 64] with a row's heads adjacent")
    elif tuple(q.shape) != (B, H * 64):
        raise ValueError("vit_attention_cls: q has shape %s, k %s" % (tuple(q.shape), tuple(k.shape)))
    if qs[-1] != 1 or any(s[3] != 1 or (H > 1 and s[2] != 64) for s in kvs):
        raise ValueError("vit_attention_cls: the heads*64 floats of a token must be adjacent in q, k and v")
    W = H * 64
    out = _out(out, (B, W), k.device, "out must be a contiguous float32 [B, heads*64] tensor")
    q_img = qs[0] if B > 1 else W
    row = [s[1] if T > 1 else W for s in kvs]
    img = [s[0] if B > 1 else max(T * r, W) for s, r in zip(kvs, row)]
    check(_lib.load().mcd_vit_attention_cls(q.data_ptr(), q_img, k.data_ptr(), row[0], img[0], v.data_ptr(), row[1], img[1],
                                            B, T, H, out.data_ptr(), _stream()))
    return out


# ---- K30 -----------------------------------------------------------------------------------------
CLS_TOKEN_MIX_MAX_B = 65535


def cls_token_mix_max_t(heads, D):
    """The most tokens cls_token_mix takes for `heads` score vectors of width D (its scores stay in LDS); 0 when heads and
    D themselves are refused (D a multiple of 64 * heads, at most 2 048)."""
    return int(_lib.load().mcd_cls_token_mix_max_t(int(heads), int(D)))


@_on_device
def cls_token_mix(u, n, out=None):
    """m[b, h] = sum_t softmax_t(u[b, h] . n[b, t]) n[b, t] in one launch (K30, include/mcd_clsfold.h): u [B, heads, D], the
    score vectors already scaled by log2(e)/8, n [B, T, D] -> [B, heads, D].  fp32; the operands are read where they lie:
    u and out with any image stride (an image's heads*D floats adjacent), n with any token and image strides (a view of
    a larger tensor).  D a multiple of 64 * heads and at most 2 048, 1 <= T <= cls_token_mix_max_t(heads, D),
    B <= CLS_TOKEN_MIX_MAX_B."""
    _need_gpu(u, n, out)
    if u.dtype != torch.float32 or n.dtype != torch.float32 or u.dim() != 3 or n.dim() != 3:
        raise TypeError("cls_token_mix: float32 u [B, heads, D] and n [B, T, D]")
    B, H, D = u.shape
    T = n.shape[1]
    if n.shape[0] != B or n.shape[2] != D:
        raise ValueError("cls_token_mix: u has shape %s, n %s" % (tuple(u.shape), tuple(n.shape)))
    if u.stride(2) != 1 or n.stride(2) != 1 or (H > 1 and u.stride(1) != D):
        raise ValueError("cls_token_mix: the D floats of a row, and the heads of an image in u, must be adjacent")
    message = "out must be a float32 [B, heads, D] tensor with an image's heads*D floats adjacent"
    out = _out(out, (B, H, D), n.device, message, False)
    if H > 1 and out.stride(1) != D:
        raise TypeError(message)
    u_img, m_img = (t.stride(0) if B > 1 else H * D for t in (u, out))
    n_row = n.stride(1) if T > 1 else D
    n_img = n.stride(0) if B > 1 else max(T * n_row, D)
    check(_lib.load().mcd_cls_token_mix(u.data_ptr(), u_img, n.data_ptr(), n_row, n_img, B, T, H, D, out.data_ptr(), m_img,
                                        _stream()))
    return out


# ---- K31 -----------------------------------------------------------------------------------------
WINDOW_ATTENTION_MAX_W = 8      # a window of at most 64 tokens: one per lane of a wave
WINDOW_ATTENTION_HEAD = 32      # Swin's head width at every released size


@_on_device
def window_attention(qkv, grid, window, shift, table, pad_qkv=None, out=None):
    """Swin's attention inside shifted windows in one launch (K31, include/mcd_swin.h): qkv a contiguous float32
    [B, H*W, 3*heads*32] tensor (the fused projection's output: q | k | v along the last axis, heads of 32 inside each, the
    tokens of the H x W grid in row-major order), grid = (H, W), window 1 .. WINDOW_ATTENTION_MAX_W, 0 <= shift < window,
    table the contiguous float32 [(2*window-1)^2, heads] relative_position_bias_table as the checkpoint stores it ->
    [B, H*W, heads*32] in token order.  pad_qkv: the contiguous float32 [3*heads*32] q | k | v of a padded token (the fused
    bias), needed when H or W is no multiple of window.  Padding, roll, partition, bias gather, the -100 shift mask,
    softmax, P.V, reverse and un-roll all happen inside the kernel."""
    _need_gpu(qkv, table, pad_qkv, out)
    B, T, W3 = _dense(qkv, "qkv must be a contiguous float32 [B, H*W, 3*heads*32] tensor", 3)
    _dense(table, "table must be a contiguous float32 [(2*window-1)^2, heads] tensor", 2)
    H, W = (int(n) for n in grid)
    window, shift, heads = int(window), int(shift), table.shape[1]
    if T != H * W or W3 != 3 * heads * WINDOW_ATTENTION_HEAD:
        raise ValueError("window_attention: qkv %s is not [B, %d*%d, 3 * %d heads * 32]" % (tuple(qkv.shape), H, W, heads))
    if table.shape[0] != (2 * window - 1) ** 2:
        raise ValueError("window_attention: the table has %d rows, window %d needs %d"
                         % (table.shape[0], window, (2 * window - 1) ** 2))
    if pad_qkv is not None and (pad_qkv.dtype != torch.float32 or pad_qkv.numel() != W3 or not pad_qkv.is_contiguous()):
        raise TypeError("pad_qkv must be a contiguous float32 tensor of 3*heads*32 elements (or None)")
    out = _out(out, (B, T, heads * WINDOW_ATTENTION_HEAD), qkv.device, "out must be a contiguous float32 [B, H*W, heads*32] tensor")
    check(_lib.load().mcd_window_attention(qkv.data_ptr(), _ptr(pad_qkv), B, H, W, heads, window, shift, table.data_ptr(),
                                           out.data_ptr(), _stream()))
    return out


# ---- K32 -----------------------------------------------------------------------------------------
PATCH_MERGE_MAX_C = 512         # 4C <= 2048, K10's limit


@_on_device
def patch_merge_ln(x, grid, weight, bias, eps, out=None):
    """Swin's patch merging up to its LayerNorm in one launch (K32, include/mcd_swin.h): x a contiguous float32
    [B, H*W, C] tensor, grid = (H, W), weight / bias [4C] -> [B, ceil(H/2)*ceil(W/2), 4C]: every output row is
    x[2i, 2j] | x[2i+1, 2j] | x[2i, 2j+1] | x[2i+1, 2j+1] (zeros past an odd edge) under LayerNorm -- the bits of layer_norm
    on the gathered rows.  C a multiple of 4, at most PATCH_MERGE_MAX_C."""
    _need_gpu(x, weight, bias, out)
    B, T, C = _dense(x, "x must be a contiguous float32 [B, H*W, C] tensor", 3)
    H, W = (int(n) for n in grid)
    if T != H * W:
        raise ValueError("patch_merge_ln: x has %d tokens, the grid is %dx%d" % (T, H, W))
    for t in (weight, bias):
        _dense(t, "patch_merge_ln: contiguous float32 [4C] weight / bias", shape=(4 * C,))
    out = _out(out, (B, ((H + 1) // 2) * ((W + 1) // 2), 4 * C), x.device,
               "out must be a contiguous float32 [B, ceil(H/2)*ceil(W/2), 4C] tensor")
    check(_lib.load().mcd_patch_merge_ln(x.data_ptr(), B, H, W, C, weight.data_ptr(), bias.data_ptr(), float(eps),
                                         out.data_ptr(), _stream()))
    return out


# ---- K10 -----------------------------------------------------------------------------------------
@_on_device
def layer_norm(x, weight, bias, eps):
    """LayerNorm over the last dimension of a contiguous fp32 tensor (torch.nn.functional.layer_norm semantics)."""
    _need_gpu(x, weight, bias)
    D = x.shape[-1]
    if x.dtype != torch.float32 or not x.is_contiguous() or weight.shape != (D,) or bias.shape != (D,):
        raise TypeError("layer_norm: contiguous float32 x and [D] weight / bias")
    y = torch.empty_like(x)
    L = _lib.load()
    check(L.mcd_layer_norm(x.data_ptr(), x.numel() // D, D, weight.data_ptr(), bias.data_ptr(), float(eps), y.data_ptr(),
                           _stream()))
    return y


# ---- K24 -----------------------------------------------------------------------------------------
@_on_device
def text_embed_ln(ids, type_ids, word, pos, type_table, weight, bias, eps, out=None):
    """BERT's embedding rows in one launch (K24, include/mcd_text.h): ids [B, T] int64 (type_ids the same shape, or None =
    row 0 of type_table), word [vocab, D], pos [>= T, D], type_table [n_type, D], weight / bias [D] ->
    LayerNorm((word[ids] + type_table[type_ids]) + pos[:T]) as [B, T, D]: the bits of layer_norm on ATen's sum.
    The ids are range-checked HERE when they are still host tensors (the tokenizer's output: no sync); device ids are
    passed on as they are and the kernel clamps them into the tables."""
    _need_gpu(word, pos, type_table, weight, bias, out)
    if ids.dim() != 2 or ids.dtype != torch.int64 or (type_ids is not None and (type_ids.dtype != torch.int64
                                                                               or type_ids.shape != ids.shape)):
        raise TypeError("text_embed_ln: ids (and type_ids) must be int64 [B, T]")
    B, T = ids.shape
    for t in (word, pos, type_table):
        _dense(t, "text_embed_ln: contiguous float32 [rows, D] tables", 2)
    D = word.shape[1]
    if pos.shape[1] != D or type_table.shape[1] != D or weight.shape != (D,) or bias.shape != (D,):
        raise ValueError("text_embed_ln: the tables, weight and bias must share the width D=%d" % D)
    if T < 1 or T > pos.shape[0]:
        raise ValueError("text_embed_ln: T=%d tokens, the position table has %d rows" % (T, pos.shape[0]))
    for name, t, n in (("ids", ids, word.shape[0]), ("type_ids", type_ids, type_table.shape[0])):
        if t is not None and not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError("text_embed_ln: %s outside [0, %d)" % (name, n))
    ids = ids.to(word.device).contiguous()
    type_ids = None if type_ids is None else type_ids.to(word.device).contiguous()
    out = _out(out, (B, T, D), word.device, "out must be a contiguous float32 [B, T, D] tensor")
    check(_lib.load().mcd_text_embed_ln(ids.data_ptr(), _ptr(type_ids), word.data_ptr(), pos.data_ptr(), type_table.data_ptr(),
                                        weight.data_ptr(), bias.data_ptr(), float(eps), B * T, T, D, word.shape[0],
                                        type_table.shape[0], out.data_ptr(), _stream()))
    return out


# ---- K11 -----------------------------------------------------------------------------------------
@_on_device
def patchify(x, patch):
    """[B, Cin, H, W] -> [B, 1 + (H/patch)(W/patch), Cin*patch*patch]: row 0 of every image zero (class-token slot),
    then the patches in (c, dy, dx) order -- the operand of the patch embedding written as a GEMM."""
    B, Cin, H, W = _nchw_image(x, "patchify: contiguous float32 [B, Cin, H, W]").shape
    if H % patch or W % patch:
        raise ValueError("patchify: %dx%d is not a multiple of the %d-pixel patch" % (H, W, patch))
    out = torch.empty((B, 1 + (H // patch) * (W // patch), Cin * patch * patch), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_patchify(x.data_ptr(), B, Cin, H, W, patch, out.data_ptr(), _stream()))
    return out


# ---- K28 -----------------------------------------------------------------------------------------
def _index_rows(t, B, name):
    """A contiguous int32 [B, n] index list on the GPU (K28's keep, K29's restore)."""
    _need_gpu(t)
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != B or not t.is_contiguous():
        raise TypeError("%s must be a contiguous int32 [B, n] tensor" % name)
    return t


@_on_device
def patchify_kept(x, patch, keep):
    """patchify for the patches keep [B, Lk] names (int32 patch numbers, row-major over the patch grid) and no others, in
    one launch (K28, include/mcd_mask.h): [B, Cin, H, W] -> [B, 1 + Lk, Cin*patch*patch], row 0 of every image zero, row
    1 + j patch keep[b, j] in (c, dy, dx) order.  The kernel clamps an index into the grid."""
    B, Cin, H, W = _nchw_image(x, "patchify_kept: contiguous float32 [B, Cin, H, W]").shape
    if H % patch or W % patch:
        raise ValueError("patchify_kept: %dx%d is not a multiple of the %d-pixel patch" % (H, W, patch))
    Lk = _index_rows(keep, B, "keep").shape[1]
    out = torch.empty((B, 1 + Lk, Cin * patch * patch), dtype=torch.float32, device=x.device)
    check(_lib.load().mcd_patchify_kept(x.data_ptr(), keep.data_ptr(), B, Cin, H, W, patch, Lk, out.data_ptr(), _stream()))
    return out


# ---- K29 -----------------------------------------------------------------------------------------
@_on_device
def token_restore(src, restore, fill=None, add=None, out=None):
    """Rows gathered through an index list, a fill row past the source, a table added, in one launch (K29,
    include/mcd_mask.h).  src: contiguous float32 [B, 1 + Lk, D], or [1 + Lk, D] -- one table shared by all images;
    restore: contiguous int32 [B, L]; fill: [D] or None; add: [1 + L, D] or None -> [B, 1 + L, D] with
    out[b, 0] = src[b, 0] + add[0] and out[b, t] = (r < Lk ? src[b, 1 + r] : fill) + add[t], r = restore[b, t - 1].
    fill None: r is clamped to Lk - 1 and no row is filled.  The decoder of a masked autoencoder (fill = the mask token,
    add = its position table), and, with a shared table, fill = add = None, the position rows of the kept patches."""
    _need_gpu(src, restore, fill, add, out)
    if src.dtype != torch.float32 or src.dim() not in (2, 3) or not src.is_contiguous():
        raise TypeError("src must be a contiguous float32 [B, 1 + Lk, D] or [1 + Lk, D] tensor")
    B = restore.shape[0] if restore.dim() == 2 else -1
    if src.dim() == 3 and src.shape[0] != B:
        raise ValueError("token_restore: src has %d images, restore %s" % (src.shape[0], tuple(restore.shape)))
    L = _index_rows(restore, B, "restore").shape[1]
    rows, D = src.shape[-2], src.shape[-1]
    if rows < 1:
        raise ValueError("token_restore: src has no row 0")
    for name, t, shape in (("fill", fill, (D,)), ("add", add, (1 + L, D))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise TypeError("%s must be a contiguous float32 tensor of shape %s" % (name, shape))
    out = _out(out, (B, 1 + L, D), src.device, "out must be a contiguous float32 [B, 1 + L, D] tensor")
    check(_lib.load().mcd_token_restore(src.data_ptr(), rows * D if src.dim() == 3 else 0, restore.data_ptr(), _ptr(fill),
                                        _ptr(add), B, L, rows - 1, D, out.data_ptr(), _stream()))
    return out


# ---- K12 - K15: the EfficientNet-B5 tower on channels-last activations (csrc/k_mbconv.hip) ----------------------
DWCONV_TILE = 8      # K13's SE partial sums: one per 8 x 8 tile of output pixels


def _nhwc(t, name):
    _need_gpu(t)
    if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
        raise TypeError("%s must be a contiguous float32 [B, H, W, C] tensor" % name)
    return t


def _vec(t, n, name):
    _need_gpu(t)
    if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
        raise TypeError("%s must be %d contiguous float32 values" % (name, n))
    return t


def same_pad(n, k, s):
    """TF-SAME padding of one axis (data_utils._SameConv): (output size, pad in front, pad behind)."""
    o = -(-n // s)
    p = max((o - 1) * s + k - n, 0)
    return o, p // 2, p - p // 2


def dwconv_tiles(Ho, Wo):
    """T, the number of K13's SE partial-sum tiles of an Ho x Wo output."""
    return -(-Ho // DWCONV_TILE) * -(-Wo // DWCONV_TILE)


def _stem_args(name, x, w_tap, k, bias=None, strict=True):
    """The arguments of an image stem (K12, K16, K19): x NCHW [B, Cin, H, W], w_tap [Cin, k, k, Cout] tap-major, bias
    [Cout] or None.  Returns (B, Cin, H, W, Cout).  strict: refuse here, with a ValueError, a weight of another shape,
    Cin > 4, Cout % 4, an empty image and a pointer that is not 16-byte aligned; K12 leaves those to its entry."""
    B, Cin, H, W = _nchw_image(x, "%s: x must be a contiguous float32 [B, Cin, H, W] tensor" % name).shape
    if strict:
        if w_tap.dim() != 4 or tuple(w_tap.shape[:3]) != (Cin, k, k) or Cin > 4 or w_tap.shape[3] % 4:
            raise ValueError("%s: w_tap must be [Cin, %d, %d, Cout] with Cin = %d <= 4 and Cout %% 4 == 0, got %s"
                             % (name, k, k, Cin, tuple(w_tap.shape)))
        if H < 1 or W < 1:
            raise ValueError("%s: empty image" % name)
    Cout = w_tap.shape[-1]
    _vec(w_tap, Cin * k * k * Cout, "w_tap")
    if bias is not None:
        _vec(bias, Cout, "bias")
    if strict:
        _aligned16("%s: w_tap and bias must be 16-byte aligned" % name, *(t for t in (w_tap, bias) if t is not None))
    return B, Cin, H, W, Cout


@_on_device
def conv_stem_nhwc(x, w_tap, bias):
    """K12: SiLU(conv3x3/2(x) + bias) with TF-SAME padding: x NCHW [B, Cin, H, W] (Cin <= 4), w_tap [Cin, 3, 3, Cout]
    (the folded weight, tap-major) -> NHWC [B, ceil(H/2), ceil(W/2), Cout]."""
    B, Cin, H, W, Cout = _stem_args("conv_stem_nhwc", x, w_tap, 3, bias, strict=False)
    y = torch.empty((B, same_pad(H, 3, 2)[0], same_pad(W, 3, 2)[0], Cout), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_conv_stem_nhwc(x.data_ptr(), B, Cin, H, W, w_tap.data_ptr(), bias.data_ptr(), Cout, y.data_ptr(), _stream()))
    return y


@_on_device
def dwconv_bn_silu(x, w_tap, bias, k, stride, silu_in):
    """K13: depthwise k x k / stride on NHWC x [B, H, W, C] with the folded weight w_tap [k*k, C] and bias [C]:
    y = SiLU(conv(a(x)) + bias), a = SiLU if silu_in else the identity.  Returns (y [B, Ho, Wo, C], psum [B, T, C]) with
    psum the per-tile sums of y (dwconv_tiles(Ho, Wo) tiles)."""
    x = _nhwc(x, "x")
    B, H, W, C = x.shape
    _vec(w_tap, k * k * C, "w_tap")
    _vec(bias, C, "bias")
    Ho, Wo = same_pad(H, k, stride)[0], same_pad(W, k, stride)[0]
    T = dwconv_tiles(Ho, Wo)
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    psum = torch.empty((B, T, C), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_dwconv_bn_silu(x.data_ptr(), B, H, W, C, w_tap.data_ptr(), bias.data_ptr(), int(k), int(stride),
                               1 if silu_in else 0, y.data_ptr(), psum.data_ptr(), T, _stream()))
    return y, psum


@_on_device
def se_gate(psum, hw, w_r, b_r, w_et, b_e):
    """K14: s [B, C] = sigmoid(b_e + w_et^T . SiLU(b_r + w_r . mean)), mean = psum summed over its tiles / hw;
    w_r [sq, C] (the reduce convolution's weight), w_et [sq, C] (the expand convolution's weight, transposed)."""
    _need_gpu(psum)
    B, T, C = _dense(psum, "psum must be a contiguous float32 [B, T, C] tensor", 3)
    sq = b_r.numel()
    _vec(w_r, sq * C, "w_r")
    _vec(b_r, sq, "b_r")
    _vec(w_et, C * sq, "w_et")
    _vec(b_e, C, "b_e")
    s = torch.empty((B, C), dtype=torch.float32, device=psum.device)
    L = _lib.load()
    check(L.mcd_se_gate(psum.data_ptr(), B, T, C, int(hw), w_r.data_ptr(), b_r.data_ptr(), sq, w_et.data_ptr(),
                        b_e.data_ptr(), s.data_ptr(), _stream()))
    return s


@_on_device
def channel_scale_(y, s):
    """K15: y [B, H, W, C] *= s[:, None, None, :] in place; returns y."""
    y = _nhwc(y, "y")
    B, H, W, C = y.shape
    _need_gpu(s)
    _dense(s, "s must be a contiguous float32 [B, C] tensor", shape=(B, C))
    L = _lib.load()
    check(L.mcd_channel_scale(y.data_ptr(), B, H * W, C, s.data_ptr(), _stream()))
    return y


@_on_device
def silu_avg_pool_nhwc(x):
    """K0n's MCD_POOL_SILU_AVG: x NHWC [B, H, W, C] -> [B, C] = mean over H, W of SiLU(x) (the tower's head)."""
    x = _nhwc(x, "x")
    B, H, W, C = x.shape
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_hook_pool_nhwc(x.data_ptr(), B, C, H * W, POOL_SILU_AVG, out.data_ptr(), 0, 0, C, 1, _stream()))
    return out


# ---- K16 - K18: the ResNet targets on channels-last activations (csrc/k_resnet.hip) ---------------------------
def conv_out(n, k, s, p):
    """Output size of one axis under ResNet's symmetric padding: (n + 2p - k) // s + 1."""
    return (n + 2 * p - k) // s + 1


@_on_device
def conv7x7s2_nhwc(x, w_tap):
    """K16: the raw stem convolution conv7x7/2, pad 3 (no bias, no batch norm, no ReLU): x NCHW [B, Cin, H, W]
    (Cin <= 4), w_tap [Cin, 7, 7, Cout] (tap-major, Cout % 4 == 0) -> NHWC [B, Ho, Wo, Cout]."""
    B, Cin, H, W, Cout = _stem_args("conv7x7s2_nhwc", x, w_tap, 7)
    y = torch.empty((B, conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3), Cout), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_conv7x7s2_nhwc(x.data_ptr(), B, Cin, H, W, w_tap.data_ptr(), Cout, y.data_ptr(), _stream()))
    return y


@_on_device
def conv7x7s2_bias_relu_nhwc(x, w_tap, bias, relu=False):
    """K16's kernel with K19's epilogue (include/mcd_stem.h): the stem of transformers' ResNet, conv7x7/2, pad 3, + bias
    (+ ReLU): x NCHW [B, Cin, H, W] (Cin <= 4), w_tap [Cin, 7, 7, Cout] (the folded weight, tap-major, Cout % 4 == 0),
    bias [Cout] -> NHWC [B, Ho, Wo, Cout]."""
    B, Cin, H, W, Cout = _stem_args("conv7x7s2_bias_relu_nhwc", x, w_tap, 7, bias)
    y = torch.empty((B, conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3), Cout), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_conv7x7s2_bias_relu_nhwc(x.data_ptr(), B, Cin, H, W, w_tap.data_ptr(), bias.data_ptr(), Cout,
                                         1 if relu else 0, y.data_ptr(), _stream()))
    return y


@_on_device
def bn_relu_maxpool_nhwc(x, scale, shift):
    """K17: max over the 3x3 / stride 2 / pad 1 window of relu(x * scale[c] + shift[c]): NHWC [B, H, W, C] (C % 4 == 0)
    -> [B, Ho, Wo, C]."""
    x = _nhwc(x, "x")
    B, H, W, C = x.shape
    if C % 4 or H < 1 or W < 1:
        raise ValueError("bn_relu_maxpool_nhwc: C = %d must be a multiple of 4 and the image non-empty" % C)
    _vec(scale, C, "scale")
    _vec(shift, C, "shift")
    _aligned16("bn_relu_maxpool_nhwc: tensors must be 16-byte aligned", x, scale, shift)
    y = torch.empty((B, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), C), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_bn_relu_maxpool_nhwc(x.data_ptr(), B, H, W, C, scale.data_ptr(), shift.data_ptr(), y.data_ptr(), _stream()))
    return y


@_on_device
def conv_igemm_nhwc(x, w_tap, bias, k, stride, relu_in=False, relu_out=False, res=None, out=None):
    """K18: implicit-GEMM convolution on the exact-fp32 MFMA: x NHWC [B, H, W, Cin], w_tap [Cout, k*k*Cin] (tap-major,
    then channel), bias [Cout] -> NHWC [B, Ho, Wo, Cout] = act_out(bias + conv(act_in(x)) + res), act = ReLU where the
    flag is set.  k = 3 with stride 1 or 2 (pad 1), or k = 1 with stride 2 (pad 0); Cin and Cout multiples of 32.
    res: None, or a residual NHWC [B, Ho, Wo, Cout] added after the bias and before the ReLU (mcd_conv_igemm_res_nhwc;
    None calls mcd_conv_igemm_nhwc, the same bits as before the keyword existed).  out: None (a new tensor), or the
    tensor to write, of the output's shape; it must not share memory with res."""
    x = _nhwc(x, "x")
    B, H, W, Cin = x.shape
    if (k, stride) not in ((3, 1), (3, 2), (1, 2)):
        raise ValueError("conv_igemm_nhwc: k = %r, stride = %r (3x3 / 1, 3x3 / 2 or 1x1 / 2)" % (k, stride))
    if w_tap.dim() != 2 or w_tap.shape[1] != k * k * Cin:
        raise ValueError("conv_igemm_nhwc: w_tap must be [Cout, %d], got %s" % (k * k * Cin, tuple(w_tap.shape)))
    Cout = w_tap.shape[0]
    if Cin % 32 or Cout % 32 or H < 1 or W < 1:
        raise ValueError("conv_igemm_nhwc: Cin = %d and Cout = %d must be multiples of 32 and the image non-empty"
                         % (Cin, Cout))
    _vec(w_tap, Cout * k * k * Cin, "w_tap")
    _vec(bias, Cout, "bias")
    _aligned16("conv_igemm_nhwc: tensors must be 16-byte aligned", x, w_tap, bias)
    pad = 1 if k == 3 else 0
    shape = (B, conv_out(H, k, stride, pad), conv_out(W, k, stride, pad), Cout)
    for t, name in ((res, "res"), (out, "out")):
        if t is None:
            continue
        _nhwc(t, name)
        if tuple(t.shape) != shape:
            raise ValueError("conv_igemm_nhwc: %s must be %s, got %s" % (name, shape, tuple(t.shape)))
        _aligned16("conv_igemm_nhwc: tensors must be 16-byte aligned", t)
    y = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    L = _lib.load()
    if res is None:
        check(L.mcd_conv_igemm_nhwc(x.data_ptr(), B, H, W, Cin, w_tap.data_ptr(), bias.data_ptr(), Cout, int(k),
                                    int(stride), 1 if relu_in else 0, 1 if relu_out else 0, y.data_ptr(), _stream()))
        return y
    nbytes = y.numel() * 4
    if res.data_ptr() < y.data_ptr() + nbytes and y.data_ptr() < res.data_ptr() + nbytes:
        raise ValueError("conv_igemm_nhwc: res must not share memory with the output")
    check(L.mcd_conv_igemm_res_nhwc(x.data_ptr(), B, H, W, Cin, w_tap.data_ptr(), bias.data_ptr(), res.data_ptr(), Cout,
                                    int(k), int(stride), 1 if relu_in else 0, 1 if relu_out else 0, y.data_ptr(),
                                    _stream()))
    return y


# ---- K19 - K21: OpenAI-CLIP's anti-aliased ResNet (K19: csrc/k_resnet.hip; K20, K21: csrc/k_clip_rn.hip) --------
@_on_device
def conv3x3s2_nhwc(x, w_tap, bias, relu=False):
    """K19: the anti-aliased stem's first convolution, conv3x3/2, pad 1, + bias (+ ReLU): x NCHW [B, Cin, H, W]
    (Cin <= 4), w_tap [Cin, 3, 3, Cout] (the folded weight, tap-major, Cout % 4 == 0), bias [Cout] -> NHWC
    [B, Ho, Wo, Cout]."""
    B, Cin, H, W, Cout = _stem_args("conv3x3s2_nhwc", x, w_tap, 3, bias)
    y = torch.empty((B, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), Cout), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_conv3x3s2_nhwc(x.data_ptr(), B, Cin, H, W, w_tap.data_ptr(), bias.data_ptr(), Cout, 1 if relu else 0,
                               y.data_ptr(), _stream()))
    return y


@_on_device
def avgpool2_nhwc(x):
    """K20: nn.AvgPool2d(2) on NHWC [B, H, W, C] (C % 4 == 0) -> [B, H // 2, W // 2, C], the bits of F.avg_pool2d(x, 2).
    An odd trailing row or column is dropped; H == 1 or W == 1 gives the empty output torch gives."""
    x = _nhwc(x, "x")
    B, H, W, C = x.shape
    if C % 4 or H < 1 or W < 1:
        raise ValueError("avgpool2_nhwc: C = %d must be a multiple of 4 and the image non-empty" % C)
    _aligned16("avgpool2_nhwc: x must be 16-byte aligned", x)
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    if y.numel() == 0:          # nothing to write (and an empty tensor has no address to hand to the entry)
        return y
    L = _lib.load()
    check(L.mcd_avgpool2_nhwc(x.data_ptr(), B, H, W, C, y.data_ptr(), _stream()))
    return y


@_on_device
def attnpool_tokens(x, pos):
    """K21: the attention pool's tokens: x NHWC [B, H, W, C] or [B, HW, C], pos [HW + 1, C] -> [B, HW + 1, C] with
    row 0 = the mean over the pixels + pos[0] and row 1 + p = x[:, p] + pos[1 + p].  C % 4 == 0."""
    _need_gpu(x, pos)
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or not x.is_contiguous():
        raise TypeError("attnpool_tokens: x must be a contiguous float32 [B, H, W, C] or [B, HW, C] tensor")
    B, C = x.shape[0], x.shape[-1]
    HW = x.shape[1] if x.dim() == 3 else x.shape[1] * x.shape[2]
    if C % 4 or HW < 1:
        raise ValueError("attnpool_tokens: C = %d must be a multiple of 4 and the image non-empty" % C)
    if pos.dtype != torch.float32 or tuple(pos.shape) != (HW + 1, C) or not pos.is_contiguous():
        raise TypeError("attnpool_tokens: pos must be a contiguous float32 [%d, %d] tensor" % (HW + 1, C))
    _aligned16("attnpool_tokens: x and pos must be 16-byte aligned", x, pos)
    tok = torch.empty((B, HW + 1, C), dtype=torch.float32, device=x.device)
    L = _lib.load()
    check(L.mcd_attnpool_tokens(x.data_ptr(), B, HW, C, pos.data_ptr(), tok.data_ptr(), _stream()))
    return tok


# ---- encoder-side linear + bias + residual on hipBLASLt (libmcd_blaslt.so) ------------------------
_blaslt_ws = {}
# bench.py sets this to a list to time the library GEMMs inside the forwards: every call then appends
# (start, end, M, N, K) with two HIP events recorded on the launch stream around the hipBLASLt call.
LINEAR_EVENTS = None


def linear_residual_available():
    return _lib.load_blaslt() is not None


def encoder_gemm_picks():
    """[(M, N, K, has_res, pick)]: the hipBLASLt algorithm (index into the heuristic's list) this process keeps for every
    encoder GEMM shape it has run through linear_residual.  has_res: bit 0 = a residual operand, bit 1 = relu=True."""
    L = _lib.load_blaslt()
    if L is None:
        return []
    n = L.mcd_linear_residual_get_picks(None, 0)
    buf = (ctypes.c_int64 * (5 * max(n, 1)))()
    n = min(n, L.mcd_linear_residual_get_picks(buf, n))
    return [tuple(int(buf[5 * i + j]) for j in range(5)) for i in range(n)]


def set_encoder_gemm_picks(picks):
    """Force the algorithm for the given shapes (what another process reported with encoder_gemm_picks()): same
    algorithm => same summation order => the same image encodes to the same bits on every rank."""
    L = _lib.load_blaslt()
    if L is None:
        return
    for M, N, K, has_res, pick in picks:
        L.mcd_linear_residual_set_pick(int(M), int(N), int(K), int(has_res), int(pick))


def _row_strided(t):
    """A 2-D matrix whose rows are contiguous and at least their width apart (rows picked out of a larger tensor)."""
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]


@_on_device
def linear_residual(res, h, weight, bias=None, out=None, relu=False):
    """out = res + h @ weight.T + bias in ONE hipBLASLt GEMM (bias epilogue + beta*C), instead of nn.Linear followed
    by an elementwise add over the whole residual stream.  res, h: [..., N] / [..., K] contiguous fp32 with the same
    leading shape; weight [N, K]; out defaults to a new tensor (pass out=res for in place).  res may be None.
    A 2-D h, res or out may also be row-strided (unit inner stride, rows at least their width apart, e.g. x[:, 0] of a
    [B, T, K] tensor, or a column block o[:, 64:128] to write): the GEMM reads and writes the rows where they lie, with
    the true leading dimension.
    relu=True: out = relu(res + h @ weight.T + bias), the library's ReLU epilogue (mcd_linear_residual_relu; its plans
    and picks are kept apart from the plain entry's)."""
    L = _lib.load_blaslt()
    if L is None:
        raise ImportError("libmcd_blaslt.so is not available (make -C mammo-clip-dissect_amd/csrc)")
    _need_gpu(h, weight, bias, res, out)
    K = h.shape[-1]
    N = weight.shape[0]
    if weight.shape[1] != K or (res is not None and (res.shape[-1] != N or res.shape[:-1] != h.shape[:-1])):
        raise ValueError("linear_residual: shapes h %s, weight %s, res %s do not match"
                         % (tuple(h.shape), tuple(weight.shape), None if res is None else tuple(res.shape)))
    for t in (h, weight, bias, res, out):
        if t is not None and (t.dtype != torch.float32
                              or not (t.is_contiguous() or (t is h or t is res or t is out) and _row_strided(t))):
            raise TypeError("linear_residual: contiguous float32 tensors only (h, res and out: or 2-D row-strided)")
    M = h.numel() // K
    ldh = K if h.is_contiguous() else h.stride(0)
    ldr = N if res is None or res.is_contiguous() else res.stride(0)
    ldo = N if out is None or out.is_contiguous() else out.stride(0)
    if out is None:
        out = torch.empty(h.shape[:-1] + (N,), dtype=torch.float32, device=h.device)
    elif tuple(out.shape) != tuple(h.shape[:-1]) + (N,):
        raise ValueError("linear_residual: out has shape %s" % (tuple(out.shape),))
    ws = _blaslt_ws.get(h.device)
    if ws is None:
        ws = _blaslt_ws[h.device] = torch.empty((L.mcd_linear_residual_workspace(),), dtype=torch.uint8, device=h.device)
    ev = LINEAR_EVENTS
    if ev is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    fn = L.mcd_linear_residual_relu if relu else L.mcd_linear_residual
    rc = fn(h.data_ptr(), ldh, weight.data_ptr(), K, bias.data_ptr() if bias is not None else None,
            res.data_ptr() if res is not None else None, ldr, out.data_ptr(), ldo, M, N, K, ws.data_ptr(), ws.numel(), _stream())
    if ev is not None:
        e1.record()
        ev.append((e0, e1, M, N, K))
    if rc != 0:
        raise _lib.McdError(rc, L.mcd_blaslt_last_error().decode("utf-8", "replace"))
    return out


# ---- K0 ------------------------------------------------------------------------------------------
@_on_device
def hook_pool(x, mode, dst, row0, col0, neuron_major, rows=None):
    """Pool a hooked tensor (utils.py:27-52) and write it into the activation matrix `dst`.

    mode: "avg"/"max" for 4-D [B,Cout,H,W]; 3-D [B,T,F] takes token 0; 2-D [B,F] is copied.
    dst: [U_total, N] when neuron_major else [N, U_total]; rows row0.. / columns col0.. are written.
    rows: optional contiguous float32 [>= B, Cout] staging block that receives the same block image-major, the layout of the
    layer's activation-cache file (mcd_hook_pool_rows, include/mcd_cache.h: one kernel, two stores).
    Returns the number of neurons written.
    """
    _need_gpu(x, dst)
    if rows is not None:
        _need_gpu(rows)
    if x.dtype != torch.float32:
        x = x.float()
    # a channels-last 4-D output (the B5 tower's HIP route) is pooled where it lies by K0n: the same bits as K0 on the
    # NCHW-contiguous copy, without the copy
    nhwc = mode in ("avg", "max") and channels_last(x, only=True)
    if not nhwc:
        x = x.contiguous()
    if x.dim() == 4:
        B, Cout, HW = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
        m = POOL_MODES[mode]
    elif x.dim() == 3:
        B, HW, Cout = x.shape
        m = POOL_MODES["cls"]
    elif x.dim() == 2:
        B, Cout = x.shape
        HW = 1
        m = POOL_MODES["none"]
    else:
        raise ValueError("unsupported hook output shape %s" % (tuple(x.shape),))
    if dst.dtype != torch.float32 or dst.dim() != 2 or dst.stride(1) != 1:
        raise TypeError("dst must be a 2-D float32 matrix with unit inner stride")
    need = (col0 + Cout, row0 + B) if neuron_major else (row0 + B, col0 + Cout)
    if row0 < 0 or col0 < 0 or dst.shape[0] < need[0] or dst.shape[1] < need[1]:
        raise IndexError("hook_pool: block [%d:%d, %d:%d] outside the activation matrix %s"
                         % (row0, row0 + B, col0, col0 + Cout, tuple(dst.shape)))
    if neuron_major:
        sn, su = 1, dst.stride(0)
    else:
        sn, su = dst.stride(0), 1
    if rows is not None and (rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous()
                             or rows.shape[0] < B or rows.shape[1] != Cout):
        raise TypeError("rows must be a contiguous float32 [>= %d, %d] block" % (B, Cout))
    L = _lib.load()
    if nhwc:
        check(L.mcd_hook_pool_nhwc(x.data_ptr(), B, Cout, HW, m, dst.data_ptr(), int(row0), int(col0), sn, su, _stream()))
        if rows is not None:      # K0n has no second store: the block just written, transposed by the HIP transpose kernel
            if not neuron_major:
                raise TypeError("hook_pool: rows with a channels-last input needs a neuron-major dst")
            if B > 0:
                transpose(dst[col0:col0 + Cout, row0:row0 + B], out=rows[:B])
        return Cout
    if rows is not None:
        check(L.mcd_hook_pool_rows(x.data_ptr(), B, Cout, HW, m, dst.data_ptr(), int(row0), int(col0), sn, su, rows.data_ptr(),
                                   Cout, _stream()))
        return Cout
    check(L.mcd_hook_pool(x.data_ptr(), B, Cout, HW, m, dst.data_ptr(), int(row0), int(col0), sn, su, _stream()))
    return Cout


# ---- K22: probe-image preprocessing (csrc/k_image.hip) ----------------------------------------------
IMAGE_MAX_TAPS = 128       # coefficients per table row mcd_image_preprocess takes (kMaxTaps)
_PRECISION_BITS = 22       # PIL Resample.c, 8 bits per channel
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


@functools.lru_cache(maxsize=None)
def resample_table(in_size, out_size, filter):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for one axis, in doubles: an int32 CPU tensor
    [out_size, 2 + k], row o = {first, count, coef[0 .. k)} zero padded, k = the widest row.  The horizontal and the
    vertical pass of Image.resize read the same kind of table.  Cached: treat the tensor as read-only."""
    fn, support = FILTERS[filter]
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_table: sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ss = 1.0 / filterscale
    rows = []
    for o in range(out_size):
        center = (o + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        last = min(int(center + support + 0.5), in_size)
        w = [fn((j + first - center + 0.5) * ss) for j in range(last - first)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        half = 0.5
        rows.append((first, [int(v * (1 << _PRECISION_BITS) - half) if v < 0 else int(v * (1 << _PRECISION_BITS) + half)
                             for v in w]))
    k = max(len(c) for _, c in rows)
    t = torch.zeros((out_size, 2 + k), dtype=torch.int32)
    for o, (first, c) in enumerate(rows):
        t[o, 0], t[o, 1] = first, len(c)
        if c:
            t[o, 2:2 + len(c)] = torch.tensor(c, dtype=torch.int32)
    return t


class ImagePlan:
    """What Preprocess.plan(H, W) gives: the resized size RH x RW, the crop window (top, left, OH, OW) inside it and
    the two pass tables (None where the axis keeps its size: PIL skips that pass)."""

    def __init__(self, H, W, RH, RW, top, left, OH, OW, filter):
        self.H, self.W, self.RH, self.RW, self.top, self.left, self.OH, self.OW = H, W, RH, RW, top, left, OH, OW
        self.xtab = resample_table(W, RW, filter) if RW != W else None
        self.ytab = resample_table(H, RH, filter) if RH != H else None

    @property
    def taps(self):
        """(kx, ky): coefficients per row of the two tables (0 for a skipped pass)."""
        return tuple(0 if t is None else t.shape[1] - 2 for t in (self.xtab, self.ytab))

    @property
    def device_ok(self):
        """K22 takes this plan (IMAGE_MAX_TAPS, one image under 2^31 bytes); otherwise the caller keeps the host route."""
        return max(self.taps) <= IMAGE_MAX_TAPS and self.H * self.W * 3 < 2 ** 31 and 12 * self.OH * self.OW < 2 ** 31


class Preprocess:
    """Resize -> CenterCrop -> ToTensor -> Normalize on an RGB PIL image, as a spec.  filter: 'bilinear' | 'bicubic';
    resize: None, an int (shorter side, torchvision's Resize(int)) or (h, w); crop: None, an int or (h, w) (CenterCrop);
    mean / std: per channel, or None for ToTensor alone."""

    def __init__(self, filter="bilinear", resize=None, crop=None, mean=None, std=None):
        if filter not in FILTERS:
            raise ValueError("Preprocess: filter must be one of %s, got %r" % (sorted(FILTERS), filter))
        if (mean is None) != (std is None):
            raise ValueError("Preprocess: mean and std come together")
        self.filter = filter
        self.resize = None if resize is None else (int(resize) if isinstance(resize, int) else tuple(int(v) for v in resize))
        self.crop = None if crop is None else ((int(crop), int(crop)) if isinstance(crop, int) else tuple(int(v) for v in crop))
        self.mean = None if mean is None else tuple(float(v) for v in mean)
        self.std = None if std is None else tuple(float(v) for v in std)
        self._lut = None

    def _key(self):
        return (self.filter, self.resize, self.crop, self.mean, self.std)

    def __eq__(self, other):
        return isinstance(other, Preprocess) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Preprocess(filter=%r, resize=%r, crop=%r, mean=%r, std=%r)" % self._key()

    def plan(self, H, W):
        """ImagePlan for an H x W source: torchvision's sizes -- Resize(int s): the shorter side -> s, the longer ->
        int(s * long / short); CenterCrop: top = int(round((RH - ch) / 2.0)), Python's round (4.5 -> 4, 5.5 -> 6).  A crop
        larger than the resized image is a ValueError (torchvision would pad)."""
        H, W = int(H), int(W)
        if self.resize is None:
            RH, RW = H, W
        elif isinstance(self.resize, int):
            short, long = (W, H) if W <= H else (H, W)
            new_short, new_long = self.resize, int(self.resize * long / short)
            RW, RH = (new_short, new_long) if W <= H else (new_long, new_short)
        else:
            RH, RW = self.resize
        if self.crop is None:
            top, left, OH, OW = 0, 0, RH, RW
        else:
            OH, OW = self.crop
            if OH > RH or OW > RW:
                raise ValueError("Preprocess: a %d x %d crop of a %d x %d image (resized from %d x %d)"
                                 % (OH, OW, RH, RW, H, W))
            top, left = int(round((RH - OH) / 2.0)), int(round((RW - OW) / 2.0))
        return ImagePlan(H, W, RH, RW, top, left, OH, OW, self.filter)

    def lut(self):
        """[3, 256] fp32 on the CPU: channel c's value for byte v, computed with the torch operations ToTensor and
        Normalize run: v.to(float32).div(255), then .sub(mean32).div(std32)."""
        if self._lut is None:
            t = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).repeat(3, 1)
            if self.mean is not None:
                mean = torch.as_tensor(self.mean, dtype=torch.float32)
                std = torch.as_tensor(self.std, dtype=torch.float32)
                t = t.sub(mean[:, None]).div(std[:, None])
            self._lut = t.contiguous()
        return self._lut


# the transforms the reference builds (file:line of the reference)
PRESETS = {
    "imagenet": Preprocess("bilinear", 256, 224, IMAGENET_MEAN, IMAGENET_STD),      # concept_vit/data_utils.py:95-100
    "clip": Preprocess("bicubic", 224, 224, CLIP_MEAN, CLIP_STD),                   # concept_vit/clip/clip.py:79-86
    "embed": Preprocess("bilinear", (1520, 912)),                                   # concept_vit/data_utils.py:176-179
    "tensor": Preprocess("bilinear", None, None, IMAGENET_MEAN, IMAGENET_STD),      # concept_vit/data_utils.py:111
}


class _PixelSpec:
    """A transform that keeps the source size and maps every byte on its own (K23): no plan, no resample table."""
    _fields = ()

    def _key(self):
        return tuple(getattr(self, f) for f in self._fields)

    def __eq__(self, other):
        return type(other) is type(self) and self._key() == other._key()

    def __hash__(self):
        return hash((type(self).__name__,) + self._key())

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (f, getattr(self, f)) for f in self._fields))


class MinMaxNormalize(_PixelSpec):
    """The vindr transform (image_classification_zs.py:81-84): per-image min-max over all channels to [0, 1], then
    (x - mean) / std with one scalar mean and std.  Output size = source size."""
    _fields = ("mean", "std")
    mode = "minmax"

    def __init__(self, mean, std):
        self.mean, self.std = float(mean), float(std)


class RawGray(_PixelSpec):
    """The csaw transform (CSAW_dataset.py:49-55): the grey values as fp32, repeated to three channels.  Output size =
    source size."""
    mode = "raw"
    mean, std = 0.0, 1.0


def get_preprocess(p):
    """A preset name or a spec (Preprocess, MinMaxNormalize, RawGray) -> the spec."""
    if isinstance(p, (Preprocess, _PixelSpec)):
        return p
    if p not in PRESETS:
        raise ValueError("unknown preprocess %r (presets: %s)" % (p, ", ".join(sorted(PRESETS))))
    return PRESETS[p]


_image_consts = {}


def _device_const(key, device, make):
    """A small CPU tensor (a pass table, a look-up table) uploaded once per device."""
    k = (key, str(device))
    if k not in _image_consts:
        _image_consts[k] = make().to(device)
    return _image_consts[k]


@_on_device
def image_preprocess(src_u8, preprocess, out=None):
    """K22: packed RGB uint8 images [n, H, W, 3] of one source size on the GPU -> fp32 [n, 3, OH, OW], the bits of
    `preprocess` (a preset name or a Preprocess) run with PIL + torch on every image.  out: where to write, e.g. a
    slice of a batch tensor: fp32 [n, 3, OH, OW] with each image contiguous (stride(0) >= 3*OH*OW).  A plan past the
    kernel's limits (ImagePlan.device_ok) raises McdError(MCD_E_UNSUPPORTED)."""
    _need_gpu(src_u8, out)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise TypeError("image_preprocess: src must be a contiguous uint8 [n, H, W, 3] tensor")
    pre = get_preprocess(preprocess)
    n, H, W = src_u8.shape[:3]
    plan = pre.plan(H, W)
    shape = (n, 3, plan.OH, plan.OW)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src_u8.device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or (n > 0 and not out[0].is_contiguous()) \
            or (n > 1 and out.stride(0) < 3 * plan.OH * plan.OW):
        raise ValueError("image_preprocess: out must be float32 %s with contiguous images" % (shape,))
    if n == 0:
        return out
    dev = src_u8.device
    xtab = None if plan.xtab is None else _device_const(("tab", W, plan.RW, pre.filter), dev, lambda: plan.xtab)
    ytab = None if plan.ytab is None else _device_const(("tab", H, plan.RH, pre.filter), dev, lambda: plan.ytab)
    lut = _device_const(("lut", pre.mean, pre.std), dev, pre.lut)
    kx, ky = plan.taps
    L = _lib.load()
    check(L.mcd_image_preprocess(src_u8.data_ptr(), n, H, W, None if xtab is None else xtab.data_ptr(), kx, plan.RW,
                                 None if ytab is None else ytab.data_ptr(), ky, plan.RH, plan.top, plan.left, plan.OH,
                                 plan.OW, lut.data_ptr(), out.data_ptr(), out.stride(0) if n > 1 else 3 * plan.OH * plan.OW,
                                 _stream()))
    return out


# ---- K23: per-image min-max normalisation (csrc/k_image.hip) -----------------------------------------
IMAGE_MINMAX_CHUNK = 16384                 # MCD_IMAGE_MINMAX_CHUNK: the bytes one workgroup of the reduction covers
IMAGE_MODES = {"minmax": 0, "raw": 1}      # MCD_IMG_MINMAX, MCD_IMG_RAW
PRESETS["vindr"] = MinMaxNormalize(0.3089279, 0.25053555408335154)                  # concept_vit/data_utils.py:121-122
PRESETS["csaw"] = RawGray()                                                         # concept_vit/data_utils.py:254-257


@_on_device
def image_minmax_normalize(src_u8, mean, std, mode="minmax", out=None):
    """K23: uint8 images of one size on the GPU, contiguous [n, H, W, 3] or [n, H, W] (grey) -> fp32 [n, 3, H, W].
    mode 'minmax': ((v - min) / (max - min) - mean) / std with the image's own min and max over all channels, the fp32
    bits of the reference's numpy operations (a constant image is NaN); 'raw': f32(v), mean and std ignored.  out: where
    to write, e.g. a slice of a batch tensor: fp32 [n, 3, H, W] with each image contiguous (image_preprocess's rules)."""
    _need_gpu(src_u8, out)
    if src_u8.dtype != torch.uint8 or not src_u8.is_contiguous() or not (
            src_u8.dim() == 3 or (src_u8.dim() == 4 and src_u8.shape[3] == 3)):
        raise TypeError("image_minmax_normalize: src must be a contiguous uint8 [n, H, W, 3] or [n, H, W] tensor")
    if mode not in IMAGE_MODES:
        raise ValueError("image_minmax_normalize: mode must be one of %s, got %r" % (sorted(IMAGE_MODES), mode))
    n, H, W = src_u8.shape[:3]
    channels = 3 if src_u8.dim() == 4 else 1
    shape = (n, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src_u8.device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or (n > 0 and not out[0].is_contiguous()) \
            or (n > 1 and out.stride(0) < 3 * H * W):
        raise ValueError("image_minmax_normalize: out must be float32 %s with contiguous images" % (shape,))
    if n == 0:
        return out
    L = _lib.load()
    ws, ws_bytes = None, 0
    if mode == "minmax":
        ws_bytes = int(L.mcd_image_minmax_workspace(n, H, W, channels))
        ws = torch.empty((max(ws_bytes, 8) // 4,), dtype=torch.int32, device=src_u8.device)
    check(L.mcd_image_minmax_normalize(src_u8.data_ptr(), n, H, W, channels, IMAGE_MODES[mode], float(mean), float(std),
                                       out.data_ptr(), out.stride(0) if n > 1 else 3 * H * W,
                                       None if ws is None else ws.data_ptr(), ws_bytes, _stream()))
    return out
