"""A CPU stand-in for mammo_clip_dissect_amd.core built on the ORACLE, for tests only.

The product's Dissector takes its compute backend as a parameter (`ops`); the default -- and the only one
the package ships -- is the HIP library.  The multi-rank host logic (sharding, index offsets, the three
all-gathers, the candidate merge, the neuron split) has no arithmetic of its own, so the tests run it on CPU
under gloo with this oracle-backed backend and require bit-identical results for 1 and 2 ranks."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle as O  # noqa: E402


def _np(t):
    return t.detach().cpu().numpy()


def normalize_rows(x, out=None):
    y = torch.from_numpy(O.normalize_rows(_np(x)))
    if out is not None:
        out.copy_(y)
        return out
    return y


def embed_gemm(I, T, mode="f32", out=None):
    P = np.empty((I.shape[0], T.shape[0]), np.float32)
    O.lib().mcd_o_gemm_nt(O._f(np.ascontiguousarray(_np(I))), O._f(np.ascontiguousarray(_np(T))),
                          O._i64(I.shape[0]), O._i64(T.shape[0]), O._i64(I.shape[1]), O._f(P))   # k-ordered: deterministic
    return torch.from_numpy(P)


def row_softmax(P, a, pad_to=192):
    S = O.row_softmax(_np(P), float(a))
    C = S.shape[1]
    ld = (C + pad_to - 1) // pad_to * pad_to
    buf = torch.zeros(S.shape[0], ld)
    buf[:, :C] = torch.from_numpy(S)
    return buf[:, :C]


def col_topk(A, K, neuron_major=False, want_vals=True):
    a = _np(A).T if neuron_major else _np(A)
    v, i = O.col_topk(np.ascontiguousarray(a), int(K))
    return (torch.from_numpy(v.T.copy()) if want_vals else None), torch.from_numpy(i.T.astype(np.int32).copy())


def wpmi_score(S, idx, p, min_prob, soft, split=-1, out=None, fast_log=False, s_is_prob=False):
    r = O.wpmi_score(np.ascontiguousarray(_np(S)), _np(idx).T.astype(np.int64).copy(), _np(p) if soft else None,
                     np.float32(min_prob), 1 if soft else 0, split)
    r = torch.from_numpy(r)
    if out is not None:
        out.copy_(r)
        return out
    return r


def logsumexp_sub(pdge, lam, seg_offsets=None, split=-1, out=None):
    x = np.ascontiguousarray(_np(pdge))
    segs = seg_offsets or [0, x.shape[0]]
    r = np.concatenate([O.logsumexp_sub(x[a:b], float(lam), split) for a, b in zip(segs[:-1], segs[1:])])
    return torch.from_numpy(r)


def row_topk(sim, k):
    v, i = O.row_topk(np.ascontiguousarray(_np(sim)), int(k))
    return torch.from_numpy(v), torch.from_numpy(i.astype(np.int32))


def hook_pool(x, mode, dst, row0, col0, neuron_major):
    r = torch.from_numpy(O.hook_pool(_np(x), mode))
    B, W = r.shape
    if neuron_major:
        dst[col0:col0 + W, row0:row0 + B] = r.t()
    else:
        dst[row0:row0 + B, col0:col0 + W] = r
    return W


# ---- what tests/scoring_fuzz.py needs beyond the Dissector's backend: K7, the gathered row preparation, K8 on given lists ---
def center_cube_normalize_rows(x, min_norm=1e-3, out=None):
    """K7 in oracle.cos_similarity_cubed's fp32 steps (centre, cube, norm clipped at min_norm), one row at a time, so that a
    row's bits depend on nothing but the row."""
    f32 = np.float32
    a = np.ascontiguousarray(_np(x), dtype=f32)
    y = np.empty_like(a)
    with np.errstate(invalid="ignore"):
        for r in range(a.shape[0]):
            c = a[r] - a[r].mean(dtype=f32)
            c = c * c * c
            y[r] = c / np.clip(np.sqrt((c * c).sum(dtype=f32)), f32(min_norm), None)
    y = torch.from_numpy(y)
    if out is not None:
        out.copy_(y)
        return out
    return y


def prepare_rows_gathered(pieces, rows, mode, min_norm=1e-3):
    """mcd_prepare_rows_gathered on the pieces [R, counts[g]] of the logical rows: the one-piece preparation of the
    concatenated rows row0 .. row1 - 1 (mode "normalize": the oracle's bits)."""
    whole = torch.cat([p for p in pieces], dim=1)[int(rows[0]):int(rows[1])].contiguous()
    return normalize_rows(whole) if mode == "normalize" else center_cube_normalize_rows(whole, min_norm)


def rank_reorder(P, tvals, tidx, perms, p=3, scale_p=0.5, out=None, order=None, colsum=None):
    """core.rank_reorder's signature on the oracle's primitives: oracle.rank_reorder's loop body (similarity.py:107-132) on
    GIVEN top lists -- tvals / tidx [U, top_n] descending activations and their images, perms [U, n_perm, top_n].  `order`
    (the ascending argsort of the gathered columns) and `colsum` (torch.sum(dim=0)'s order) are what a test may swap out."""
    f32 = np.float32
    order = order or (lambda G: np.argsort(G, axis=0, kind="stable"))
    colsum = colsum or O.sum0
    Pn, tv, ti, pm = _np(P).astype(f32), _np(tvals).astype(f32), _np(tidx).astype(np.int64), _np(perms).astype(np.int64)
    U, top_n = tv.shape
    res = np.empty((U, Pn.shape[1]), f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for u in range(U):
            G = np.ascontiguousarray(Pn[ti[u]])
            avg = (colsum(G) / f32(top_n)).astype(f32)
            rank = np.argsort(order(G), axis=0, kind="stable")
            t = tv[u][:, None]
            st = t[::-1]
            base = st - np.concatenate([st[pm[u, k]] for k in range(pm.shape[1])], axis=1)
            ab = np.abs(base).astype(f32)
            base = (O._pow(ab, p).sum(dtype=f32) / f32(ab.size)).astype(f32)
            d = np.abs(t - st[:, 0][rank]).astype(f32)
            err = (O.sum0(O._pow(d, p)) / f32(top_n)).astype(f32) / base
            res[u] = -(err / O._pow(avg, scale_p)).astype(f32)
    res = torch.from_numpy(res)
    if out is not None:
        out.copy_(res)
        return out
    return res
