"""CPU: pipeline.Dissector's fused route for rank_reorder, cos_similarity and cos_similarity_cubed -- the host logic
(shards, the gathers of P and of the activation rows, the neuron split, the host permutation draw, the images column)
under gloo with an oracle-backed stand-in for the kernels: G ranks give the one-rank bits, the permutation stream and
the generator state are the per-layer loop's, the argument checks raise what the drop-in raises."""
import os
import sys

import numpy as np
import pytest
import torch

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_FNS = ("rank_reorder", "cos_similarity", "cos_similarity_cubed")
f32 = np.float32


class RowOps:
    """tests/cpu_ops.py plus the kernels the three functions use, as deterministic CPU restatements: K1a through the oracle,
    K7 and K8 in numpy in the oracle's formulation (similarity.py:15-22, oracle.rank_reorder)."""

    def __init__(self):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import cpu_ops
        self.c = cpu_ops
        self.O = cpu_ops.O
        self.normalize_rows = cpu_ops.normalize_rows
        self.col_topk = cpu_ops.col_topk
        self.row_topk = cpu_ops.row_topk

    @staticmethod
    def _store(r, out):
        if out is not None:
            out.copy_(r)
            return out
        return r

    def embed_gemm(self, I, T, mode="f32", out=None):
        return self._store(self.c.embed_gemm(I.contiguous(), T.contiguous()), out)

    @staticmethod
    def transpose(A, out=None):
        return RowOps._store(A.t().contiguous(), out)

    @staticmethod
    def _ccn(x, min_norm):
        x = np.asarray(x, f32)
        d = x - (x.sum(1, keepdims=True, dtype=f32) / f32(x.shape[1])).astype(f32)
        c = (d * d) * d
        nrm = np.maximum(np.sqrt((c * c).sum(1, keepdims=True, dtype=f32)), f32(min_norm))
        return torch.from_numpy((c / nrm).astype(f32))

    def center_cube_normalize_rows(self, x, min_norm=1e-3, out=None):
        return self._store(self._ccn(x.numpy(), min_norm), out)

    def prepare_rows_gathered(self, src, counts, rows, mode, min_norm=1e-3, out=None):
        if src.dim() == 2:
            src = src.unsqueeze(0)
        r0, r1 = rows
        x = torch.cat([src[g, r0:r1, :counts[g]] for g in range(src.shape[0])], dim=1).contiguous()
        y = self.normalize_rows(x) if mode == "normalize" else self._ccn(x.numpy(), min_norm)
        return self._store(y, out)

    def rank_reorder(self, P, tvals, tidx, perms, p=3, scale_p=0.5, out=None):
        O = self.O
        P, vals, idx, perms = P.numpy(), tvals.numpy(), tidx.numpy().astype(np.int64), perms.numpy().astype(np.int64)
        U, top_n = vals.shape
        res = np.empty((U, P.shape[1]), f32)
        for u in range(U):                                      # oracle.rank_reorder's loop on the given top-n / permutations
            G = P[idx[u]]
            avg = (O.sum0(G) / f32(top_n)).astype(f32)
            rank = np.argsort(np.argsort(G, axis=0, kind="stable"), axis=0, kind="stable")
            t = vals[u][:, None]
            st = t[::-1]
            base = st - np.concatenate([st[perms[u, k]] for k in range(perms.shape[1])], axis=1)
            ab = np.abs(base).astype(f32)
            base = (O._pow(ab, p).sum(dtype=f32) / f32(ab.size)).astype(f32)
            reorg = st[:, 0][rank]
            d = np.abs(t - reorg).astype(f32)
            with np.errstate(invalid="ignore", divide="ignore"):     # a zero baseline or a negative mean: NaN, as the reference
                err = (O.sum0(O._pow(d, p)) / f32(top_n)).astype(f32) / base
                res[u] = -(err / O._pow(avg, scale_p)).astype(f32)
        return self._store(torch.from_numpy(res), out)


def _problem(N, widths, C, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sum(widths), N, generator=g), torch.randn(N, D, generator=g), torch.randn(C, D, generator=g)


def _dissector(world, rank, N, widths, C, D, seed, group=None):
    sys.path.insert(0, ROOT)
    from mammo_clip_dissect_amd.pipeline import Dissector, shard_bounds
    At, E_img, E_txt = _problem(N, widths, C, D, seed)
    lo, hi = shard_bounds(N, world, rank)
    dis = Dissector(hi - lo, ["l%d" % i for i in range(len(widths))], widths, C, D, "cpu", ops=RowOps(), group=group)
    dis.At[:, :hi - lo] = At[:, lo:hi]
    dis.E_img[:] = E_img[lo:hi]
    dis.cursor = hi - lo
    return dis, E_txt


def _run_all(world, rank, N, widths, C, D, seed, top_fraction, group=None):
    """The three functions on one Dissector, rank_reorder under torch.manual_seed(seed)."""
    dis, E_txt = _dissector(world, rank, N, widths, C, D, seed, group)
    out = {}
    for fn in ROW_FNS:
        if fn == "rank_reorder":
            dis.set_scoring(fn, top_fraction=top_fraction)
            torch.manual_seed(seed)
        else:
            dis.set_scoring(fn)
        r = dis.finish(E_txt, k_desc=min(10, C), k_img=min(5, N))
        out[fn] = [t.numpy().copy() for t in (r.sim, r.vals, r.ids, r.top_ids, r.top_vals)]
    out["rng"] = torch.get_rng_state().numpy()
    return out


@pytest.mark.parametrize("world,case", [(2, (240, [7, 12], 37, 16, 5, 0.05)),
                                        (3, (130, [9, 4], 37, 16, 7, 0.5)),       # 44 + 43 + 43 images, top_n = 65: every shard < top_n
                                        (4, (201, [13, 8, 3], 40, 16, 9, 0.1)),   # 51 + 50 + 50 + 50
                                        (3, (2, [3], 11, 8, 8, 0.5)),             # N < ranks: rank 2 holds no image; top_n = 1 < k_img
                                        (8, (810, [13, 8], 37, 16, 11, 0.05))])   # 21 neurons over 8 ranks (rank 7: none)
def test_row_fns_ranks_bit_identical_to_one(mcd, world, case):
    """Every output of the three functions at G ranks equals the one-rank output bit for bit, and every rank's CPU generator
    ends where the one-rank run's does (each rank draws the whole permutation stream)."""
    single = _run_all(1, 0, *case)
    got = util.run_ranks(world, _run_all, case, timeout=300)
    for r in range(world):
        for fn in ROW_FNS:
            for a, b in zip(single[fn], got[r][fn]):
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (r, fn)
        assert np.array_equal(single["rng"], got[r]["rng"]), r


def test_fused_rank_reorder_is_the_per_layer_loop(mcd, oracle):
    """rank_reorder through the fused route == oracle.rank_reorder layer by layer on the same P under the same seed
    (the oracle draws its permutations from the global generator in the reference's order), and the generator state
    afterwards is the per-layer loop's."""
    N, widths, C, D, seed = 300, [6, 11, 4], 29, 16, 3
    dis, E_txt = _dissector(1, 0, N, widths, C, D, seed)
    dis.set_scoring("rank_reorder")
    torch.manual_seed(1234)
    res = dis.finish(E_txt)
    state_fused = torch.get_rng_state()
    ops = RowOps()
    P = ops.embed_gemm(ops.normalize_rows(dis.E_img), ops.normalize_rows(E_txt)).numpy()
    torch.manual_seed(1234)
    o = 0
    for w in widths:
        ref = oracle.rank_reorder(P, dis.At[o:o + w, :N].t().contiguous().numpy())
        assert np.array_equal(res.sim[o:o + w].numpy(), ref, equal_nan=True)
        o += w
    assert torch.equal(torch.get_rng_state(), state_fused)
    # the images column: torch.topk(target_feats, 5, dim=0) of every layer
    _, t5 = oracle.col_topk(dis.At[:, :N].t().contiguous().numpy(), 5)
    assert np.array_equal(res.top_ids.numpy(), t5.T)


def test_fused_cos_functions_against_the_oracle(mcd, oracle):
    """The stand-in route computes the reference's cos_similarity / cos_similarity_cubed (numpy column formulation in the
    oracle; another summation order, hence a tolerance)."""
    N, widths, C, D, seed = 257, [10, 7], 31, 16, 4
    dis, E_txt = _dissector(1, 0, N, widths, C, D, seed)
    ops = RowOps()
    P = ops.embed_gemm(ops.normalize_rows(dis.E_img), ops.normalize_rows(E_txt)).numpy()
    A = dis.At[:, :N].t().contiguous().numpy()
    for fn in ("cos_similarity", "cos_similarity_cubed"):
        dis.set_scoring(fn)
        got = dis.finish(E_txt).sim.numpy()
        ref = getattr(oracle, fn)(P, A)
        assert np.abs(got - ref).max() <= 1e-6, fn


@pytest.mark.parametrize("fn", ROW_FNS)
def test_set_scoring_rejects_the_bf16_chain(mcd, fn):
    """gemm_mode='bf16' never writes fp32 P: the three functions refuse it, at construction and in set_scoring."""
    from mammo_clip_dissect_amd.pipeline import Dissector
    with pytest.raises(NotImplementedError, match="bf16"):
        Dissector(10, ["l"], [3], 5, 8, "cpu", similarity_fn=fn, gemm_mode="bf16", ops=RowOps())
    dis = Dissector(10, ["l"], [3], 5, 8, "cpu", gemm_mode="bf16", ops=RowOps())
    with pytest.raises(NotImplementedError, match="bf16"):
        dis.set_scoring(fn)
    assert dis.similarity_fn == "soft_wpmi"


@pytest.mark.parametrize("fn", ROW_FNS)
def test_set_scoring_refuses_top_k_like_the_reference(mcd, fn):
    """The reference's rank_reorder / cos_similarity* take no top_k: passing one is a TypeError (utils.py:602)."""
    from mammo_clip_dissect_amd.pipeline import Dissector
    dis = Dissector(10, ["l"], [3], 5, 8, "cpu", ops=RowOps())
    with pytest.raises(TypeError, match="top_k"):
        dis.set_scoring(fn, 100)


def test_rank_reorder_top_n_below_one_raises_the_drop_in_error(mcd):
    """int(N * top_fraction) < 1: the drop-in's RuntimeError (the reference divides by zero there), before any collective."""
    dis, E_txt = _dissector(1, 0, 19, [4], 7, 8, 1)
    dis.set_scoring("rank_reorder")                 # 19 * 0.05 -> 0 images
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match=r"rank_reorder: top_fraction\*N = 0 images"):
        dis.finish(E_txt)
    assert torch.equal(torch.get_rng_state(), state)


def test_rank_reorder_top_n_past_the_kernels_is_unsupported(mcd):
    """K3 and K8 stop at 4 096 images per neuron: beyond, the library's MCD_E_UNSUPPORTED error."""
    from mammo_clip_dissect_amd import core
    dis, E_txt = _dissector(1, 0, 5000, [2], 7, 8, 1)
    dis.set_scoring("rank_reorder", top_fraction=0.9)
    with pytest.raises(core.McdError, match="4096") as e:
        dis.finish(E_txt)
    assert e.value.code == -5
