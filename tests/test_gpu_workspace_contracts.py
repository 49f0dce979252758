"""GPU: the workspace contract of the C ABI (include/mcd_hip.h, include/mcd_blaslt.h): "the caller owns every buffer".

core.py hands every entry a torch.empty of exactly the size its *_workspace() function returns: a store past the end lands
in the caching allocator's slack, and what the block held before is whatever tensor lived there last.  Here every workspace
entry is called through mcd._lib.load() / load_blaslt() with its workspace inside util.framed_ws() -- 4096 guard bytes on
both sides, all of it, the interior included, one fill byte -- and its outputs in util.FramedOut frames:

  a. exact size: ws_bytes is exactly what the size function returns; both guards keep their fill;
  b. poison: one run per fill in util.WS_FILLS (0x00; 0xFF = int32 -1, K3's mark, and a NaN as fp32 and as bf16; 0x7F = a large
     finite fp32 and a bf16 NaN) and one on a workspace left dirty by the same entry at a larger shape (framed at the larger
     size, called with the smaller ws_bytes): all runs bit-identical, the first anchored to the plain reference of the
     entry's existing test at that test's tolerance (named at each anchor);
  c. a workspace 16 bytes short, and one 4 bytes off where the entry states an alignment: the status the header states,
     outputs and workspace untouched (mcd_embed_gemm: its documented fall-back to the small kernel, the same anchor).

The shapes are the smallest that reach each path; the comments at the case lists name the path.  The builders return
Case objects that tests/test_gpu_stream_contracts.py runs again on a side stream and under hipGraph capture; the case lists
and WS_TABLE are plain data (importing this module needs no GPU): tests/test_exec_contract_cpu.py checks WS_TABLE against the
headers."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from util import (OUT_FILL, WS_FILLS, WS_GUARD, FramedIn, FramedOut, assert_same_bits, check_ws_guards, check_ws_untouched,
                  framed_ws)

pytestmark = pytest.mark.gpu

IDX_FILL = -77777                       # the OUT_FILL of int32 outputs
E_ARG, E_RANGE, E_WS = -1, -2, -3       # MCD_E_ARG, MCD_E_RANGE, MCD_E_WORKSPACE
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    return O


@pytest.fixture(scope="module")
def L(mcd, dev):
    return mcd._lib.load()


def ceil_to(x, m):
    return (x + m - 1) // m * m


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def unit_rows(n, d, seed):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=1, keepdim=True)


class Case:
    """One entry at one shape.  call(ws_ptr, ws_bytes, output pointers, stream) -> status; outs: one (rows, width, pitch, dtype,
    fill, zero_pad) per output; need: what the entry's size function returns; ins: the device tensors the call reads and
    gen(seed) -> fresh valid contents for them (the stream tests refill them in place); host: the ctypes arrays the call
    takes; anchor(dense outputs): the plain reference, raises; align / misaligned_rc: the alignment the entry states for ws
    and the status of a pointer 4 bytes off; short_rc: the status of a workspace 16 bytes short ("fallback": the call
    succeeds without touching it and fallback(dense outputs) checks the result); then: a Case of the same size run on the
    same workspace right after; bigger(): the same entry at a larger shape."""

    def __init__(self, what, call, outs, need, ins=(), gen=None, host=(), anchor=None, align=0, misaligned_rc=None, short_rc=E_WS,
                 fallback=None, then=None, bigger=None, tol=None, inout=None):
        self.what, self.call, self.outs, self.need, self.ins, self.gen, self.host = what, call, outs, int(need), list(ins), gen, host
        self.anchor, self.align, self.misaligned_rc, self.short_rc, self.fallback = anchor, align, misaligned_rc, short_rc, fallback
        self.then, self.bigger, self.tol, self.inout = then, bigger, tol, inout or {}

    def frames(self, dev, fills=None):
        return [FramedOut(r, w, p, 0, dt, dev, tail=p - w if zp else 0, fill=(fills[j] if fills else f))
                for j, (r, w, p, dt, f, zp) in enumerate(self.outs)]

    def run(self, dev, ws_ptr, ws_bytes, fills=None, stream=None):
        outs = self.frames(dev, fills)
        return self.call(ws_ptr, ws_bytes, [o.ptr for o in outs], stream), outs

    def check(self, outs, expected, what):
        for o, e, spec in zip(outs, expected, self.outs):
            o.check(e, zero_pad=spec[5], what=what)

    def check_untouched(self, outs, what):
        for o, (r, w, p, dt, f, zp) in zip(outs, self.outs):
            assert bool((o.flat == torch.full((1,), f, dtype=dt, device=o.flat.device)).all()), (what, "a refused call wrote an output")


def dense(outs):
    return [o.view.contiguous() for o in outs]


def err(L):
    return L.mcd_last_error().decode()


def check_sizes_and_poison(L, dev, c):
    """a. and b. of the module docstring; returns the first run's dense outputs."""
    first = first_then = None
    for fill in WS_FILLS:
        what = (c.what, "ws fill 0x%02X" % fill)
        flat, ptr, n = framed_ws(c.need, WS_GUARD, fill, dev)
        rc, outs = c.run(dev, ptr, n)
        assert rc == 0, (what, err(L))
        check_ws_guards(flat, n, fill, what)
        if first is None:
            first = dense(outs)
            c.anchor(first)
        c.check(outs, first, what)
        if c.then is not None:                      # the same workspace, as the call above left it
            assert c.then.need == c.need
            rc, outs = c.then.run(dev, ptr, n)
            assert rc == 0, (what, "then", err(L))
            check_ws_guards(flat, n, fill, what + ("then",))
            if first_then is None:
                first_then = dense(outs)
                c.then.anchor(first_then)
            c.then.check(outs, first_then, what + ("then",))
    big = c.bigger()
    what = (c.what, "dirty from", big.what)
    assert big.need >= c.need, what
    flat, ptr, n = framed_ws(big.need, WS_GUARD, 0x00, dev)
    rc, _ = big.run(dev, ptr, n)
    assert rc == 0, (what, err(L))
    rc, outs = c.run(dev, ptr, c.need)
    assert rc == 0, (what, err(L))
    check_ws_guards(flat, n, 0x00, what)
    c.check(outs, first, what)
    return first


def check_refusals(L, dev, c, first):
    """c. of the module docstring."""
    for kind in ("short", "misaligned"):
        if kind == "short" and (c.need == 0 or c.short_rc is None) or kind == "misaligned" and not c.align:
            continue
        what = (c.what, kind)
        flat, ptr, n = framed_ws(c.need + 256, WS_GUARD, 0xFF, dev)
        want = c.short_rc if kind == "short" else c.misaligned_rc
        rc, outs = c.run(dev, ptr + (4 if kind == "misaligned" else 0), max(c.need - 16, 0) if kind == "short" else c.need)
        check_ws_untouched(flat, 0xFF, what)
        if want == "fallback":
            assert rc == 0, (what, err(L))
            c.fallback(dense(outs), first)
            c.check(outs, dense(outs), what)            # (the frame: nothing outside the logical region)
        else:
            assert rc == want, (what, rc, err(L))
            c.check_untouched(outs, what)


# ---- K3 -----------------------------------------------------------------------------------------------------------------
def topk_columns(N, U, seed, mixed):
    """[N, U]; mixed: column u is normal (u % 3 == 0), ~88 % ties at its bound (1: the fast kernel leaves it to the streaming
    kernel) or dead (2), as test_col_topk_edges builds them, so that both values of K3's per-neuron mark occur in one call."""
    A = np.random.default_rng(seed).standard_normal((N, U)).astype(np.float32)
    if mixed:
        for u in range(U):
            if u % 3 == 1:
                A[:, u] = np.maximum(A[:, u], 1.2)
            elif u % 3 == 2:
                A[:, u] = 0.0
    return A


def lexsort_topk(A, K):
    """value descending, index ascending (test_col_topk_edges' reference): neuron-major (vals [U, K], idx [U, K])."""
    order = np.lexsort((np.broadcast_to(np.arange(A.shape[0])[:, None], A.shape), -A), axis=0)[:K]
    return np.ascontiguousarray(np.take_along_axis(A, order, 0).T), np.ascontiguousarray(order.T.astype(np.int32))


# (N, U, K): N = 37: one wave's worth, the 256 x 1 class; 1025: 256 x 2 (K <= 128), 1024 x 1 (K = 200); 10001: 256 x 10 with
# the quad across a row's end, 1024 x 3 (K = 200), streaming only (K = 1030: the mark is unused).  K = 100 > N = 37 is
# MCD_E_RANGE (test_col_topk_k_out_of_range below).
TOPK_SHAPES = [(37, 5, 5), (1025, 3, 5), (1025, 3, 100), (1025, 3, 200), (10001, 4, 5), (10001, 4, 100), (10001, 4, 200),
               (10001, 4, 1030)]
TOPK_CASES = [(nm,) + s for nm in (False, True) for s in TOPK_SHAPES]     # image-major: transposed through ws


def col_topk_case(L, dev, neuron_major, N, U, K, mixed=True, seed=3, top=True):
    A = topk_columns(N, U, seed + N + K, mixed)
    if neuron_major:
        a = FramedIn(T(A.T, dev), ceil_to(N, 4), 0, NAN)        # the binding's pitch: the 16-byte loads; the pad columns hold NaN
        sn, su = 1, a.ld
    else:
        a = FramedIn(T(A, dev), U, 0, NAN)
        sn, su = U, 1
    need = L.mcd_col_topk_workspace(N, U, sn, su, K)
    want_v, want_i = lexsort_topk(A, K)

    def call(ws, nb, o, st):
        return L.mcd_col_topk(a.ptr, N, U, sn, su, K, o[0], o[1], K, ws, nb, st)

    def anchor(got):     # test_col_topk_edges: numpy lexsort, exact
        assert np.array_equal(got[1].cpu().numpy(), want_i) and np.array_equal(got[0].cpu().numpy(), want_v)

    def gen(s):
        x = topk_columns(N, U, s, mixed)
        return [torch.from_numpy(np.ascontiguousarray(x.T if neuron_major else x))]
    c = Case(("K3", "neuron-major" if neuron_major else "image-major", N, U, K, "mixed" if mixed else "normal"), call,
             [(U, K, K, torch.float32, OUT_FILL, False), (U, K, K, torch.int32, IDX_FILL, False)], need, ins=[a.view], gen=gen,
             anchor=anchor, align=16, misaligned_rc=E_ARG)
    c.keep = a
    if top:
        c.then = col_topk_case(L, dev, neuron_major, N, U, K, mixed=False, seed=seed + 1, top=False)
        c.bigger = lambda: col_topk_case(L, dev, neuron_major, N + 64, U + 3, K, seed=seed + 2, top=False)
    return c


@pytest.mark.parametrize("params", TOPK_CASES, ids=str)
def test_col_topk_workspace(L, dev, params):
    c = col_topk_case(L, dev, *params)
    check_refusals(L, dev, c, check_sizes_and_poison(L, dev, c))


@pytest.mark.parametrize("neuron_major", [False, True])
def test_col_topk_k_out_of_range(L, dev, neuron_major):
    """K = 100 on N = 37: MCD_E_RANGE (the header), outputs and workspace untouched."""
    c = col_topk_case(L, dev, neuron_major, 37, 5, 100, top=False)
    flat, ptr, n = framed_ws(c.need, WS_GUARD, 0xFF, dev)
    rc, outs = c.run(dev, ptr, n)
    assert rc == E_RANGE, (rc, err(L))
    c.check_untouched(outs, c.what)
    check_ws_untouched(flat, 0xFF, c.what)


# ---- K6 -----------------------------------------------------------------------------------------------------------------
# C >= 4096: K3's workgroup-per-row kernel, whose "left to the streaming kernel" mark lives in the row's first output index, and
# the streaming kernel behind it; 4099: rows off the 16-byte grid (element loads), 4100: the 16-byte loads
ROW_TOPK_CASES = [(C, k) for C in (4099, 4100) for k in (1, 10)]


def row_topk_case(L, dev, C, k, seed=5, top=True):
    U = 6       # rows 0, 3: normal; 1, 4: ~88 % ties at the top; 2, 5: dead
    sim = np.ascontiguousarray(topk_columns(C, U, seed + C + k, True).T)
    simd = T(sim, dev)
    v, i = lexsort_topk(np.ascontiguousarray(sim.T), k)

    def call(ws, nb, o, st):
        return L.mcd_row_topk(simd.data_ptr(), C, U, C, k, o[0], o[1], st)

    def anchor(got):     # test_row_topk_long_rows_pitches: the oracle's order = numpy lexsort, exact
        assert np.array_equal(got[1].cpu().numpy(), i) and np.array_equal(got[0].cpu().numpy(), v)
    return Case(("K6", C, k), call, [(U, k, k, torch.float32, OUT_FILL, False), (U, k, k, torch.int32, IDX_FILL, False)], 0,
                ins=[simd], gen=lambda s: [torch.from_numpy(np.ascontiguousarray(topk_columns(C, U, s, True).T))], anchor=anchor)


@pytest.mark.parametrize("params", ROW_TOPK_CASES, ids=str)
def test_row_topk_stale_outputs(L, dev, params):
    """No workspace: on long rows the mark lives in idx, so stale output content of -1 (the mark's own value) or 0 is an input
    of the second launch.  idx pre-filled with -1, 0 and IDX_FILL, vals with NaN and OUT_FILL: the same bits, the frames kept."""
    c = row_topk_case(L, dev, *params)
    runs = []
    for vfill, ifill in ((OUT_FILL, IDX_FILL), (NAN, -1), (NAN, 0)):
        rc, outs = c.run(dev, None, 0, fills=(vfill, ifill))
        assert rc == 0, err(L)
        got = dense(outs)
        if not runs:
            c.anchor(got)
        c.check(outs, got, (c.what, vfill, ifill))
        runs.append(((vfill, ifill), got))
    assert_same_bits(runs, c.what)


# ---- K1 -----------------------------------------------------------------------------------------------------------------
# (8193, 3845, 70): 33 x 16 tiles of 256 x 256 = 528 >= 512, the smallest "big" dispatch; both tile edges ragged (8193 = 32 * 256
# + 1, 3845 = 15 * 256 + 5), K zero-padded from 70 to 128 in the bf16 image.  mode 1: the split kernel (hi / lo arrays), 2: the
# persistent single-pass kernel.
GEMM_CASES = [(1, 8193, 3845, 70), (2, 8193, 3845, 70)]


def gemm_case(L, dev, mode, N, C, D, seed=11, top=True):
    I, Tt = unit_rows(N, D, seed).to(dev), unit_rows(C, D, seed + 1).to(dev)
    need = L.mcd_embed_gemm_workspace(N, C, D, mode)

    def call(ws, nb, o, st, m=mode):
        return L.mcd_embed_gemm(I.data_ptr(), D, Tt.data_ptr(), D, N, C, D, m, o[0], C, ws, nb, st)

    def plain(m):
        out = torch.empty(N, C, device=dev)
        assert call(None, 0, [out.data_ptr()], None, m) == 0, err(L)
        return out

    def anchor(got, small=None):
        # test_gemm_bf16_large_kernel: the 256 x 256-tile kernel against the 128 x 128 kernel of the same mode <= 2e-6, split bf16
        # against the fp32 mode <= 6e-6; test_gemm_bf16_modes: single-pass bf16 against the fp32 mode <= 8e-3
        small = plain(mode) if small is None else small
        ref = plain(0)
        assert float((got[0] - small).abs().max()) <= 2e-6
        assert float((small - ref).abs().max()) <= (6e-6 if mode == 1 else 8e-3)
        assert float((got[0] - ref).abs().max()) <= (6e-6 if mode == 1 else 8e-3)

    def fallback(got, first):       # the header: "without it (NULL / too small) they run the 128x128 kernel"
        small = plain(mode)
        assert torch.equal(got[0], small)
        anchor(first, small)
    c = Case(("K1", mode, N, C, D), call, [(N, C, C, torch.float32, OUT_FILL, False)], need, ins=[I, Tt],
             gen=lambda s: [unit_rows(N, D, s), unit_rows(C, D, s + 1)], anchor=anchor, align=16, misaligned_rc="fallback",
             short_rc="fallback", fallback=fallback)
    if top:
        c.bigger = lambda: gemm_case(L, dev, mode, N, C, D + 130, seed + 2, top=False)     # K padded to 256: twice the bf16 image, no larger output
    return c


@pytest.mark.parametrize("params", GEMM_CASES, ids=str)
def test_embed_gemm_workspace(L, dev, params):
    c = gemm_case(L, dev, *params)
    assert c.need == (2 if params[0] == 1 else 1) * (8193 + 3845) * 128 * 2
    check_refusals(L, dev, c, check_sizes_and_poison(L, dev, c))


# ---- K1s ----------------------------------------------------------------------------------------------------------------
# (N, C, D): (17, 33, 70): a second 16-row image block with one live row, a second pair of concept blocks with one live row, K
# padded 70 -> 128; (37, 40, 128): K whole, the binding's smallest test shape; (257, 513, 130): a second 256-image tile with one
# row, a third 256-concept tile with one column, K padded 130 -> 256.  flags: 0 | MCD_GEMM_EXP_NORMALIZE (the other conversion
# kernel).  wide: ldE = 256 * ceil(C / 256) + 16 (the zero-pad launch) instead of ceil16(C).
GEXP_CASES = [(N, C, D, flags, wide) for (N, C, D) in ((17, 33, 70), (37, 40, 128), (257, 513, 130)) for flags in (0, 1)
              for wide in (False, True)]
GEXP_A = 10.0


def gexp_inputs(N, C, D, flags, seed):
    g = torch.Generator().manual_seed(seed)
    I, Tt = torch.randn(N, D, generator=g), torch.randn(C, D, generator=g)
    if flags:
        return [I * 3.0, Tt * 0.2]                # raw embeddings (test_embed_gemm_exp's)
    return [I / I.norm(dim=1, keepdim=True), Tt / Tt.norm(dim=1, keepdim=True)]


def gexp_case(L, dev, N, C, D, flags, wide, seed=21, top=True):
    I, Tt = [t.to(dev) for t in gexp_inputs(N, C, D, flags, seed + N)]
    ldE = ceil_to(C, 256) + 16 if wide else ceil_to(C, 16)
    need = L.mcd_embed_gemm_exp_workspace(N, C, D)

    def call(ws, nb, o, st):
        return L.mcd_embed_gemm_exp(I.data_ptr(), D, Tt.data_ptr(), D, N, C, D, GEXP_A, flags, o[0], ldE, o[1], ws, nb, st)

    def anchor(got):     # test_embed_gemm_exp: float64 exp(a (P - 1)) and 1 / sum, its two bounds
        In, Tn = I.double(), Tt.double()
        In, Tn = In / In.norm(dim=1, keepdim=True), Tn / Tn.norm(dim=1, keepdim=True)
        ref = torch.exp(GEXP_A * (In @ Tn.t() - 1.0))
        assert float((got[0].double() / ref - 1.0).abs().max()) <= GEXP_A * 8e-3 + 2.0 ** -7
        assert float((got[1][0].double() * ref.sum(dim=1) - 1.0).abs().max()) <= GEXP_A * 4e-3 + 1e-3
    c = Case(("K1s", N, C, D, flags, ldE), call, [(N, C, ldE, torch.bfloat16, OUT_FILL, True), (1, N, N, torch.float32, OUT_FILL, False)],
             need, ins=[I, Tt], gen=lambda s: gexp_inputs(N, C, D, flags, s), anchor=anchor, align=16, misaligned_rc=E_WS)
    if top:
        c.bigger = lambda: gexp_case(L, dev, N + 300, C + 300, D + 128, flags, wide, seed + 1, top=False)
    return c


@pytest.mark.parametrize("params", GEXP_CASES, ids=str)
def test_embed_gemm_exp_workspace(L, dev, params):
    assert L.mcd_embed_gemm_exp_time_kernel(0) == 0        # the measurement hook off: its default
    c = gexp_case(L, dev, *params)
    check_refusals(L, dev, c, check_sizes_and_poison(L, dev, c))


# ---- K4s ----------------------------------------------------------------------------------------------------------------
# N = 37, C = 40 (ldE 128: one slice); U = 1, 5: one group of 16 neurons with 1 / 5 live; K = 1, 5, 17: less than one group of
# four arguments, one group + 1, a second batch of 16 rows with one row
WPMI_BF16_CASES = [(U, K, soft) for U in (1, 5) for K in (1, 5, 17) for soft in (1, 0)]


def wpmi_bf16_inputs(N, C, ldE, U, K, seed):
    g = torch.Generator().manual_seed(seed)
    E = torch.zeros(N, ldE, dtype=torch.bfloat16)
    E[:, :C] = (torch.rand(N, C, generator=g) * 0.9 + 0.05).to(torch.bfloat16)      # test_wpmi_score_bf16_batch_edges' operands
    rinv = torch.rand(N, generator=g) * 0.01 + 0.001
    idx = torch.randint(0, N, (U, K), generator=g, dtype=torch.int32)
    return [E, rinv, idx]


def wpmi_bf16_case(L, dev, U, K, soft, N=37, C=40, seed=31, top=True):
    ldE = 128
    E, rinv, idx = [t.to(dev) for t in wpmi_bf16_inputs(N, C, ldE, U, K, seed + U + K)]
    p = torch.linspace(0.998, 0.97, K).float().to(dev)
    need = L.mcd_wpmi_score_bf16_workspace(U, K)

    def call(ws, nb, o, st):
        return L.mcd_wpmi_score_bf16(E.data_ptr(), ldE, N, C, rinv.data_ptr(), idx.data_ptr(), K, U, K, p.data_ptr() if soft else None,
                                     1e-7, soft, o[0], C, ws, nb, st)

    def anchor(got):     # test_wpmi_score_bf16: the same expression in float64 on the same E and rinv, <= 2e-3 absolute
        S = E[:, :C].double() * rinv.double()[:, None]
        gsel = S[idx.long()]
        w = 1.0 + p.double()[None, :, None] * (gsel - 1.0) + 1e-7 if soft else gsel + 1e-7
        assert float((got[0].double() - torch.log(w).sum(dim=1)).abs().max()) <= 2e-3
    c = Case(("K4s", U, K, soft), call, [(U, C, C, torch.float32, OUT_FILL, False)], need, ins=[E, rinv, idx],
             gen=lambda s: wpmi_bf16_inputs(N, C, ldE, U, K, s), anchor=anchor, align=8, misaligned_rc=E_WS)
    if top:
        c.bigger = lambda: wpmi_bf16_case(L, dev, U + 3, K + 4, soft, seed=seed + 1, top=False)
    return c


@pytest.mark.parametrize("params", WPMI_BF16_CASES, ids=str)
def test_wpmi_score_bf16_workspace(L, dev, params):
    c = wpmi_bf16_case(L, dev, *params)
    assert c.need == 8 * params[0] * params[1]
    check_refusals(L, dev, c, check_sizes_and_poison(L, dev, c))


# ---- K5 -----------------------------------------------------------------------------------------------------------------
# [0, 7, 7, 40]: the panel kernel (the middle segment has no rows); [0, 3905, 3905, 3950]: a segment of more than 3840 rows, the
# only way into the three-pass path in the product build -- 61 super-chunks of 64 rows + 1 row, micro-sums of 3905 / 16 rows
# read back from ws.  C = 5: one partial panel of 64 columns; 70: a second panel of 6.
LSE_CASES = [(offs, C) for offs in ((0, 7, 7, 40), (0, 3905, 3905, 3950)) for C in (5, 70)]
LSE_LAM = float(np.float32(0.6))


def lse_case(L, dev, offs, C, seed=41, top=True):
    Ut, n_seg = offs[-1], len(offs) - 1
    make = lambda s: torch.randn(Ut, C, generator=torch.Generator().manual_seed(s)) * 3 - 400
    x = make(seed + C).to(dev)
    seg = (ctypes.c_int64 * (n_seg + 1))(*offs)
    need = L.mcd_logsumexp_sub_workspace(Ut, C, n_seg)

    def call(ws, nb, o, st):
        return L.mcd_logsumexp_sub(x.data_ptr(), C, C, seg, n_seg, LSE_LAM, -1, o[0], C, ws, nb, st)

    def anchor(got):     # oracle.logsumexp_sub per segment at lam = 0.6, as test_logsumexp_sub_given_reference_inputs calls it: exact
        O, xs, g = _oracle(), x.cpu().numpy(), got[0].cpu().numpy()
        for a, b in zip(offs[:-1], offs[1:]):
            if b > a:
                ref = O.logsumexp_sub(xs[a:b], LSE_LAM)
                print("K5", offs, C, "rows %d..%d max |diff| %.3g" % (a, b, float(np.abs(g[a:b] - ref).max())))
                assert np.array_equal(g[a:b], ref)
    c = Case(("K5", offs, C), call, [(Ut, C, C, torch.float32, OUT_FILL, False)], need, ins=[x], gen=lambda s: [make(s)], host=[seg],
             anchor=anchor)
    if top:
        c.bigger = lambda: lse_case(L, dev, (0, offs[1] + 100, offs[2] + 100, offs[3] + 200), C + 64, seed + 1, top=False)
    return c


@pytest.mark.parametrize("params", LSE_CASES, ids=str)
def test_logsumexp_sub_workspace(L, dev, params):
    c = lse_case(L, dev, *params)
    check_refusals(L, dev, c, check_sizes_and_poison(L, dev, c))


# ---- K8 -----------------------------------------------------------------------------------------------------------------
RANK_CASES = [(300, 40, 7, 15)]          # baseline_ws of exactly U = 7 floats (28 bytes); top_n = 15 = int(0.05 N), the oracle's


def rank_inputs(N, C, U, top_n, seed):
    g = torch.Generator().manual_seed(seed)
    P = torch.softmax(4 * torch.randn(N, C, generator=g), dim=1)         # test_rank_reorder_against_oracle's operands
    A = torch.randn(N, U, generator=g)
    v, i = lexsort_topk(A.numpy(), top_n)
    perms = torch.stack([torch.randperm(top_n, generator=g) for _ in range(5 * U)]).view(U, 5, top_n).to(torch.int32)
    return P, A, [P, torch.from_numpy(v), torch.from_numpy(i), perms]


def rank_case(L, dev, N, C, U, top_n, seed=51, top=True):
    P, A, host = rank_inputs(N, C, U, top_n, seed)
    Pd, tv, ti, perms = [t.to(dev) for t in host]

    def call(ws, nb, o, st):
        return L.mcd_rank_reorder(Pd.data_ptr(), C, N, C, tv.data_ptr(), ti.data_ptr(), top_n, U, top_n, perms.data_ptr(), 5, 3.0, 0.5,
                                  ws, o[0], C, st)

    def anchor(got):     # test_rank_reorder_against_oracle: the oracle on the same permutations, NaN pattern equal, 5e-6 relative
        ref = _oracle().rank_reorder(P.numpy(), A.numpy(), p=3, scale_p=0.5, perms=host[3].numpy().astype(np.int64))
        g = got[0].cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(ref))
        m = ~np.isnan(ref)
        assert (np.abs(g[m] - ref[m]) / np.abs(ref[m])).max() <= 5e-6
    c = Case(("K8", N, C, U, top_n), call, [(U, C, C, torch.float32, OUT_FILL, False)], 4 * U, ins=[Pd, tv, ti, perms],
             gen=lambda s: rank_inputs(N, C, U, top_n, s)[2], anchor=anchor, short_rc=None)
    if top:
        c.bigger = lambda: rank_case(L, dev, N + 100, C, U + 5, top_n + 5, seed + 1, top=False)
    return c


@pytest.mark.parametrize("params", RANK_CASES, ids=str)
def test_rank_reorder_baseline_workspace(L, dev, params):
    c = rank_case(L, dev, *params)
    check_sizes_and_poison(L, dev, c)


# ---- mcd_linear_residual / mcd_linear_residual_relu ---------------------------------------------------------------------
LINEAR_CASES = [(relu, 37, 40, 100) for relu in (False, True)]       # test_linear_residual_frames' shape; ws: 32 MiB framed | NULL
LINEAR_TOL = 2e-5                                                     # test_linear_residual_matches_torch: 2e-5 * max|ref|


def linear_inputs(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05, torch.randn(N, generator=g),
            torch.randn(M, N, generator=g)]


def linear_case(B, dev, relu, M, N, K, seed=61, top=True):
    """MCD_BLASLT_PICK=heuristic must be set: no (shape, pitch) key then times candidates, allocates or synchronises."""
    h, W, bias, res = [t.to(dev) for t in linear_inputs(M, N, K, seed)]
    entry = B.mcd_linear_residual_relu if relu else B.mcd_linear_residual

    def call(ws, nb, o, st):
        return entry(h.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), res.data_ptr(), N, o[0], N, M, N, K, ws, nb, st)

    def anchor(got):
        ref = h.double() @ W.double().t() + bias.double() + res.double()
        ref = torch.relu(ref) if relu else ref
        assert float((got[0].double() - ref).abs().max()) <= LINEAR_TOL * float(ref.abs().max())
    c = Case(("linear", relu, M, N, K), call, [(M, N, N, torch.float32, OUT_FILL, False)], B.mcd_linear_residual_workspace(),
             ins=[h, W, bias, res], gen=lambda s: linear_inputs(M, N, K, s), anchor=anchor, tol=LINEAR_TOL)
    if top:
        c.bigger = lambda: linear_case(B, dev, relu, M + 27, N + 8, K + 28, seed + 1, top=False)
    return c


@pytest.mark.parametrize("params", LINEAR_CASES, ids=str)
def test_linear_residual_workspace(mcd, dev, monkeypatch, params):
    """The 32 MiB the size function asks for, framed: the guards keep their fill under every poison, the runs are bit-identical
    (one plan per key: the same algorithm) and within 2e-5 * max|ref| of float64.  The header: a smaller workspace, or none
    (ws = NULL, ws_bytes = 0), only narrows the choice of algorithms -- both calls succeed, to the same bound."""
    B = mcd._lib.load_blaslt()
    assert B is not None, "libmcd_blaslt.so not built"
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    c = linear_case(B, dev, *params)
    assert c.need == 32 << 20
    first = None
    for fill in WS_FILLS:
        flat, ptr, n = framed_ws(c.need, WS_GUARD, fill, dev)
        rc, outs = c.run(dev, ptr, n)
        assert rc == 0, B.mcd_blaslt_last_error().decode()
        check_ws_guards(flat, n, fill, (c.what, fill))
        if first is None:
            first = dense(outs)
            c.anchor(first)
        c.check(outs, first, (c.what, fill))
        del flat
    big = c.bigger()
    flat, ptr, n = framed_ws(c.need, WS_GUARD, 0x00, dev)
    assert big.run(dev, ptr, n)[0] == 0, B.mcd_blaslt_last_error().decode()
    rc, outs = c.run(dev, ptr, n)
    assert rc == 0
    check_ws_guards(flat, n, 0x00, (c.what, "dirty"))
    c.check(outs, first, (c.what, "dirty"))
    for ws_ptr, nb in ((None, 0), (ptr, n - 16)):
        rc, outs = c.run(dev, ws_ptr, nb)
        assert rc == 0, B.mcd_blaslt_last_error().decode()
        c.anchor(dense(outs))
        c.check(outs, dense(outs), (c.what, "ws", nb))
    check_ws_guards(flat, n, 0x00, (c.what, "short"))


# ---- K23 ----------------------------------------------------------------------------------------------------------------
MINMAX_CASES = [(2, 8, 12, 3)]      # (n, H, W, channels); frames and fills: tests/test_gpu_mammo_probe.py -- here the dirty run only


def minmax_case(L, dev, n, H, W, channels, seed=71, top=True):
    make = lambda s: torch.randint(3, 250, (n, H, W, channels) if channels == 3 else (n, H, W), dtype=torch.uint8,
                                   generator=torch.Generator().manual_seed(s))
    src = make(seed).to(dev)
    need = L.mcd_image_minmax_workspace(n, H, W, channels)

    def call(ws, nb, o, st):
        return L.mcd_image_minmax_normalize(src.data_ptr(), n, H, W, channels, 0, 0.3, 0.25, o[0], 3 * H * W, ws, nb, st)

    def anchor(got):     # test_k23_argument_contract: mammo_recipe.numpy_apply, bit for bit
        import mammo_recipe as R
        ref = R.numpy_apply(src.cpu().numpy(), dict(mode="minmax", mean=0.3, std=0.25))
        assert np.array_equal(got[0].cpu().numpy().reshape(ref.shape).view(np.uint32), ref.view(np.uint32))
    c = Case(("K23", n, H, W, channels), call, [(n, 3 * H * W, 3 * H * W, torch.float32, OUT_FILL, False)], need, ins=[src],
             gen=lambda s: [make(s)], anchor=anchor)
    if top:
        c.bigger = lambda: minmax_case(L, dev, n + 1, 160, 240, channels, seed + 1, top=False)     # 7 chunks per image
    return c


@pytest.mark.parametrize("params", MINMAX_CASES, ids=str)
def test_image_minmax_on_a_dirty_workspace(L, dev, params):
    c = minmax_case(L, dev, *params)
    flat, ptr, n = framed_ws(c.need, WS_GUARD, 0x00, dev)
    rc, outs = c.run(dev, ptr, n)
    assert rc == 0, err(L)
    first = dense(outs)
    c.anchor(first)
    big = c.bigger()
    flat, ptr, n = framed_ws(big.need, WS_GUARD, 0x7F, dev)
    assert big.need > c.need and big.run(dev, ptr, n)[0] == 0, err(L)
    rc, outs = c.run(dev, ptr, c.need)
    assert rc == 0, err(L)
    check_ws_guards(flat, n, 0x7F, c.what)
    c.check(outs, first, c.what)


# ---- the table tests/test_exec_contract_cpu.py checks against the headers -------------------------------------------------
# size function -> (the entries it serves, their case list)
WS_TABLE = {
    "mcd_embed_gemm_workspace": (("mcd_embed_gemm",), GEMM_CASES),
    "mcd_col_topk_workspace": (("mcd_col_topk",), TOPK_CASES),
    "mcd_embed_gemm_exp_workspace": (("mcd_embed_gemm_exp",), GEXP_CASES),
    "mcd_wpmi_score_bf16_workspace": (("mcd_wpmi_score_bf16",), WPMI_BF16_CASES),
    "mcd_logsumexp_sub_workspace": (("mcd_logsumexp_sub",), LSE_CASES),
    "mcd_image_minmax_workspace": (("mcd_image_minmax_normalize",), MINMAX_CASES),
    "mcd_linear_residual_workspace": (("mcd_linear_residual", "mcd_linear_residual_relu"), LINEAR_CASES),
}
# scratch without a size function: baseline_ws of U floats; the mark in the output
WS_TABLE_NO_SIZE_FN = {"mcd_rank_reorder": RANK_CASES, "mcd_row_topk": ROW_TOPK_CASES}
