"""GPU: the pitch, padding and aliasing contracts of the C ABI (include/mcd_hip.h), entry by entry, on framed buffers.

The binding (core.py) picks one pitch per entry, but the pitch and the base alignment select the kernel variant (16-byte or
element path, register or LDS kernel, sliced or generic, buffer-descriptor or plain stores).  Every case here calls the raw
entry through mcd._lib.load() on torch's current stream with operands inside util.framed() allocations:

  * outputs start as util.OUT_FILL; util.check_frame() then wants the logical region bit-equal to the expected values and
    every other element of the allocation -- pad columns, base offset, guards -- still OUT_FILL (promised zeros: exactly +0);
  * the gaps of the inputs hold NaN in one run and 1e30 in the next (util.GAP_FILLS); both runs are checked against the same
    expected bits, so nothing outside an input's logical region may influence a result;
  * inputs are bit-identical after the call (in-place cases excepted).

Expected values: the CPU oracle where the suite already asserts bit equality with it (K1a, K1 fp32, K2, K3, K6, and K4's hard
terms on power-of-two data, test_wpmi_score_summation_order_is_atens); elsewhere the same entry on dense copies at the
binding's own pitch, which the existing tests pin against float64 / the goldens.  Every comparison is bit equality.

Pitch classes of a row of width w: w, w + 1 (odd: no 16-byte path), ceil4(w) + 4, the binding's pitch and that plus one more
alignment unit; base offsets 0 and, where the header asks for no alignment, 1 element.  One operand varies at a time, plus
one combination with every pitch odd and every base offset 1."""
import ctypes

import numpy as np
import pytest
import torch

from util import FRAME_GUARD as GUARD   # elements: 256 bytes of fp32 / int32, 128 of bf16 -- base offset 0 is 16-byte aligned
from util import GAP_FILLS, OUT_FILL, check_frame, int_bits
from util import FramedIn as In, FramedOut as Out

pytestmark = pytest.mark.gpu

IDX_FILL = -77777   # the OUT_FILL of int32 outputs


@pytest.fixture(scope="module")
def L(mcd, dev):
    return mcd._lib.load()


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ceil_to(x, m):
    return (x + m - 1) // m * m


def uniq(xs):
    return list(dict.fromkeys(xs))


def pitches(w, binding=None, unit=4):
    """w, w + 1, an odd pitch (w + 1 may be a multiple of 4), ceil4(w) + 4, the binding's and that plus one alignment unit."""
    binding = w if binding is None else binding
    return uniq([w, w + 1, w + 1 + w % 2, ceil_to(w, 4) + 4, binding, binding + unit])


def one_at_a_time(*classes, offs):
    """classes[i]: the pitch classes of operand i, its first entry the default.  Yields (pitches, base offsets): every operand
    varied alone at base offset 0, each operand that allows it at base offset 1 alone, and one all-odd combination (the first
    odd pitch of every class, or its entry 1 where the header allows none; base offset 1 wherever allowed)."""
    base = [c[0] for c in classes]
    zero = [0] * len(classes)
    out = [(tuple(base), tuple(zero))]
    for i, c in enumerate(classes):
        for p in c[1:]:
            out.append((tuple(base[:i] + [p] + base[i + 1:]), tuple(zero)))
        if offs[i]:
            out.append((tuple(base), tuple(zero[:i] + [1] + zero[i + 1:])))
    out.append((tuple(next((p for p in c if p % 2), c[1]) for c in classes), tuple(1 if o else 0 for o in offs)))
    return uniq(out)


def dense(view):
    return view.contiguous()


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _idx_gap(gap, N):
    """What the gaps of an index matrix hold in the run whose float gaps hold `gap`: a valid row either way (0 | N - 1)."""
    return 0 if gap != gap else N - 1


def ok(rc, L):
    assert rc == 0, L.mcd_last_error().decode()


# ---- K1a ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 128, 129, 512, 513, 1024, 1030])     # the four per_lane instantiations and their edges
def test_normalize_rows_pitches_and_in_place(L, dev, oracle, d):
    n = 37
    x = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    want, xd = oracle.normalize_rows(x), T(x, dev)
    for (px, py), (ox, oy) in one_at_a_time(pitches(d), pitches(d), offs=(1, 1)):
        for gap in GAP_FILLS:
            a, y = In(xd, px, ox, gap), Out(n, d, py, oy, torch.float32, dev)
            ok(L.mcd_normalize_rows(a.ptr, px, n, d, y.ptr, py, st()), L)
            y.check(want, what=("K1a", d, px, py, ox, oy, gap))
            a.same()
            ok(L.mcd_normalize_rows(a.ptr, px, n, d, a.ptr, px, st()), L)     # y == x: the gaps are the frame's fill
            check_frame(a.flat, a.spec, want, what=("K1a in place", d, px, ox, gap))


# ---- K7 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 300, 1025])
def test_center_cube_normalize_rows_pitches_and_in_place(L, dev, n):
    rows = 9
    xd = torch.randn(rows, n, generator=torch.Generator().manual_seed(n)).to(dev)
    want = torch.empty_like(xd)
    ok(L.mcd_center_cube_normalize_rows(xd.data_ptr(), n, rows, n, 1e-3, want.data_ptr(), n, st()), L)
    for (px, py), (ox, oy) in one_at_a_time(pitches(n), pitches(n), offs=(1, 1)):
        for gap in GAP_FILLS:
            a, y = In(xd, px, ox, gap), Out(rows, n, py, oy, torch.float32, dev)
            ok(L.mcd_center_cube_normalize_rows(a.ptr, px, rows, n, 1e-3, y.ptr, py, st()), L)
            y.check(want, what=("K7", n, px, py, ox, oy, gap))
            a.same()
            ok(L.mcd_center_cube_normalize_rows(a.ptr, px, rows, n, 1e-3, a.ptr, px, st()), L)
            check_frame(a.flat, a.spec, want, what=("K7 in place", n, px, ox, gap))


# ---- K1a / K7 on gathered pieces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_prepare_rows_gathered_pitches(L, dev, mode):
    """G = 3 pieces of 40, 0 and 23 columns: bit-equal to K1a / K7 on the concatenated rows, at every pitch of dst; what the
    blocks hold past their counts (and between the blocks) changes nothing."""
    counts, R, row0, row1, ld_src = [40, 0, 23], 11, 2, 9, 44
    n, rows, ld_block = sum(counts), row1 - row0, R * ld_src + 5
    pieces = [torch.randn(R, c, generator=torch.Generator().manual_seed(7 + g)).to(dev) for g, c in enumerate(counts)]
    logical = torch.cat(pieces, dim=1)[row0:row1].contiguous()
    want = torch.empty_like(logical)
    if mode == 0:
        ok(L.mcd_normalize_rows(logical.data_ptr(), n, rows, n, want.data_ptr(), n, st()), L)
    else:
        ok(L.mcd_center_cube_normalize_rows(logical.data_ptr(), n, rows, n, 1e-3, want.data_ptr(), n, st()), L)
    arr = (ctypes.c_int64 * 3)(*counts)
    for ldd in pitches(n):
        for off in (0, 1):
            for gap in GAP_FILLS:
                src = torch.full((GUARD + off + 3 * ld_block + GUARD,), gap, device=dev)
                for g, p in enumerate(pieces):
                    if counts[g]:
                        torch.as_strided(src, (R, counts[g]), (ld_src, 1), GUARD + off + g * ld_block).copy_(p)
                snap = src.clone()
                y = Out(rows, n, ldd, off, torch.float32, dev)
                ok(L.mcd_prepare_rows_gathered(src.data_ptr() + 4 * (GUARD + off), ld_src, ld_block, 3, arr, n, row0, row1, mode,
                                               1e-3, y.ptr, ldd, st()), L)
                y.check(want, what=("gathered", mode, ldd, off, gap))
                assert torch.equal(int_bits(src), int_bits(snap))


# ---- K1 -----------------------------------------------------------------------------------------------------------------
def _gemm_inputs(oracle, N, C, D):
    rng = np.random.default_rng(N + C + D)
    a = oracle.normalize_rows(rng.standard_normal((N, D)).astype(np.float32))
    b = oracle.normalize_rows(rng.standard_normal((C, D)).astype(np.float32))
    return a, b


def _oracle_gemm(oracle, a, b):
    ref = np.empty((a.shape[0], b.shape[0]), np.float32)
    oracle.lib().mcd_o_gemm_nt(oracle._f(a), oracle._f(b), oracle._i64(a.shape[0]), oracle._i64(b.shape[0]),
                               oracle._i64(a.shape[1]), oracle._f(ref))
    return ref


@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(130, 257, 512), (37, 50, 70)])
def test_embed_gemm_pitches(L, dev, oracle, shape, mode, use_ws):
    """All three arithmetic modes, with and without the workspace the entry asks for (at these sizes it asks for none and the
    scratch handed in is ignored): the same bits at every pitch and base offset of I, T and P; the fp32 mode the oracle's
    k-ordered chain (test_gemm_follows_mkl_k_blocks claims it for every D)."""
    N, C, D = shape
    a, b = _gemm_inputs(oracle, N, C, D)
    ad, bd = T(a, dev), T(b, dev)
    nws = int(L.mcd_embed_gemm_workspace(N, C, D, mode)) if use_ws else 0
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev) if use_ws else None
    wsp, wsn = (ws.data_ptr(), ws.numel()) if use_ws else (None, 0)
    if mode == 0:
        want = _oracle_gemm(oracle, a, b)
    else:
        want = torch.empty(N, C, device=dev)
        ok(L.mcd_embed_gemm(ad.data_ptr(), D, bd.data_ptr(), D, N, C, D, mode, want.data_ptr(), C, wsp, wsn, st()), L)
    for (pi, pt, pp), (oi, ot, op) in one_at_a_time(pitches(D), pitches(D), pitches(C), offs=(1, 1, 1)):
        for gap in GAP_FILLS:
            i_, t_, p_ = In(ad, pi, oi, gap), In(bd, pt, ot, gap), Out(N, C, pp, op, torch.float32, dev)
            ok(L.mcd_embed_gemm(i_.ptr, pi, t_.ptr, pt, N, C, D, mode, p_.ptr, pp, wsp, wsn, st()), L)
            p_.check(want, what=("K1", shape, mode, pi, pt, pp, oi, ot, op, gap))
            i_.same(), t_.same()


def test_embed_gemm_wide_pitch_keeps_the_gap(L, dev, oracle):
    """N = 2 rows 9 000 000 floats apart: the fp32 epilogue's buffer-descriptor form makes 32-bit offsets for all 128 rows of
    its tile, which at this pitch wrap modulo 2^32 back inside the descriptor -- the entry has to take the plain stores.  Both
    rows equal the tight-pitch result and the gap between them, the base offset and the guards keep their fill (compared on
    the device)."""
    N, C, D, ldp = 2, 50, 64, 9_000_000
    a, b = _gemm_inputs(oracle, N, C, D)
    want = _oracle_gemm(oracle, a, b)
    ad, bd = T(a, dev), T(b, dev)
    tight = torch.empty(N, C, device=dev)
    ok(L.mcd_embed_gemm(ad.data_ptr(), D, bd.data_ptr(), D, N, C, D, 0, tight.data_ptr(), C, None, 0, st()), L)
    assert np.array_equal(tight.cpu().numpy(), want)
    for off in (0, 1):
        p_ = Out(N, C, ldp, off, torch.float32, dev)
        ok(L.mcd_embed_gemm(ad.data_ptr(), D, bd.data_ptr(), D, N, C, D, 0, p_.ptr, ldp, None, 0, st()), L)
        p_.check(want, what=("K1 wide pitch", off))
        del p_


# ---- K2 -----------------------------------------------------------------------------------------------------------------
def _softmax_case(L, dev, oracle, N, C):
    P = (torch.randn(N, C, generator=torch.Generator().manual_seed(C)) * 0.3).numpy()
    want, Pd = oracle.row_softmax(P, 10.0), T(P, dev)
    b = ceil_to(C, 192)
    lds = uniq([b, C, C + 1, ceil_to(C, 4) + 4, b + 192] + ([256, 260] if C <= 256 else []))   # 256 | 260: the register / LDS kernel
    for (pp, ps), (op, os_) in one_at_a_time(pitches(C), lds, offs=(1, 1)):
        for gap in GAP_FILLS:
            p_, s_ = In(Pd, pp, op, gap), Out(N, C, ps, os_, torch.float32, dev, tail=ps - C)
            ok(L.mcd_row_softmax(p_.ptr, pp, N, C, 10.0, s_.ptr, ps, st()), L)
            s_.check(want, zero_pad=True, what=("K2", N, C, pp, ps, op, os_, gap))
            p_.same()


@pytest.mark.parametrize("C", [5, 193, 250, 257, 763, 1030])
def test_row_softmax_pitches_and_zero_padding(L, dev, oracle, C):
    _softmax_case(L, dev, oracle, 37, C)


def test_row_softmax_streaming_kernel_pitches(L, dev, oracle):
    _softmax_case(L, dev, oracle, 3, 16390)


# ---- K3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 100])
@pytest.mark.parametrize("neuron_major", [False, True])
def test_col_topk_pitches_and_null_outputs(L, dev, oracle, neuron_major, K):
    N, U = 300, 41
    A = np.random.default_rng(K).standard_normal((N, U)).astype(np.float32)
    A[[3, 77, 200], 5] = 2.5                                    # ties: the lower image index first
    v, i = oracle.col_topk(A, K)
    want_v, want_i = np.ascontiguousarray(v.T), np.ascontiguousarray(i.T.astype(np.int32))
    Ad = T(A.T if neuron_major else A, dev)
    w = Ad.shape[1]
    for (ld, ldo), (off, _) in one_at_a_time([ceil_to(w, 4), w + 1 - w % 2, ceil_to(w, 4) + 4], [K, K + 3], offs=(1, 0)):
        for gap in GAP_FILLS:
            for need_v, need_i in ((1, 1), (0, 1), (1, 0)):
                a = In(Ad, ld, off, gap)
                sn, su = (1, ld) if neuron_major else (ld, 1)
                nws = int(L.mcd_col_topk_workspace(N, U, sn, su, K))
                ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
                vals, idx = Out(U, K, ldo, 0, torch.float32, dev), Out(U, K, ldo, 0, torch.int32, dev, fill=IDX_FILL)
                ok(L.mcd_col_topk(a.ptr, N, U, sn, su, K, vals.ptr if need_v else None, idx.ptr if need_i else None, ldo,
                                  ws.data_ptr(), nws, st()), L)
                what = ("K3", neuron_major, K, ld, ldo, off, gap, need_v, need_i)
                vals.check(want_v if need_v else torch.full((U, K), OUT_FILL), what=what)
                idx.check(want_i if need_i else torch.full((U, K), IDX_FILL, dtype=torch.int32), what=what)
                a.same()


def test_transpose_pitches(L, dev):
    N, U = 300, 41
    Ad = torch.randn(N, U, generator=torch.Generator().manual_seed(4)).to(dev)
    want = Ad.t().contiguous()
    for (ps, pd), (os_, od) in one_at_a_time(pitches(U), pitches(N), offs=(1, 1)):
        for gap in GAP_FILLS:
            a, y = In(Ad, ps, os_, gap), Out(U, N, pd, od, torch.float32, dev)
            ok(L.mcd_transpose(a.ptr, ps, N, U, y.ptr, pd, st()), L)
            y.check(want, what=("transpose", ps, pd, os_, od, gap))
            a.same()


# ---- K4 -----------------------------------------------------------------------------------------------------------------
MP = float(2.0 ** -30)


def _pow2_S(N, C, seed):
    """S = 2^-k - 2^-30: with min_prob = 2^-30 every hard-WPMI log argument is an exact power of two, which the kernel's log and
    the oracle's round alike (test_wpmi_score_summation_order_is_atens) -- the oracle then pins the bits of the hard terms."""
    k = np.random.default_rng(seed).integers(6, 26, (N, C))
    return (np.ldexp(1.0, -k) - 2.0 ** -30).astype(np.float32)


@pytest.mark.parametrize("soft", [1, 0])
@pytest.mark.parametrize("K", [20, 10])                                     # K % 4 == 0 (the sliced kernel may run) and not
@pytest.mark.parametrize("shape", [(300, 763, 41), (64, 10000, 17)])        # the second: split = 9 984 = 104 slices, then the tail kernel
def test_wpmi_score_pitches(L, dev, oracle, shape, K, soft):
    """ldS selects the sliced kernel (ldS % 96 == 0, aligned, K % 4 == 0), wpmi_main_kernel<2> or <1>; every variant gives the
    bits of the call on a dense, zero-padded S at the binding's pitch -- and, for the hard terms, the oracle's."""
    N, C, U = shape
    S = _pow2_S(N, C, N + K)
    idx = np.ascontiguousarray(np.random.default_rng(K).integers(0, N, (U, K)).astype(np.int32))
    p = oracle.p_in_examples(K)
    Sd, idxd, pd = T(S, dev), T(idx, dev), T(p, dev)
    b = ceil_to(C, 192)
    Sb = torch.zeros(N, b, device=dev)
    Sb[:, :C] = Sd
    want = torch.empty(U, C, device=dev)
    ok(L.mcd_wpmi_score(Sb.data_ptr(), b, N, C, idxd.data_ptr(), K, U, K, pd.data_ptr() if soft else None, MP, soft, -1,
                        want.data_ptr(), C, st()), L)
    if not soft:
        ref = oracle.wpmi_score(S, idx.T.astype(np.int64).copy(), None, np.float32(MP), 0)
        assert np.array_equal(want.cpu().numpy(), ref)
    for (pS, pidx, po), (oS, _, oo) in one_at_a_time([b, C, C + 1, b + 96], [K, K + 3], [C, C + 5], offs=(1, 0, 1)):
        for gap in GAP_FILLS:
            s_, i_ = In(Sd, pS, oS, gap), In(idxd, pidx, 0, _idx_gap(gap, N))
            out = Out(U, C, po, oo, torch.float32, dev)
            ok(L.mcd_wpmi_score(s_.ptr, pS, N, C, i_.ptr, pidx, U, K, pd.data_ptr() if soft else None, MP, soft, -1, out.ptr, po,
                                st()), L)
            out.check(want, what=("K4", shape, K, soft, pS, pidx, po, oS, oo, gap))
            s_.same(), i_.same()


# ---- K1s / K4s ----------------------------------------------------------------------------------------------------------
def _gexp(L, dev, Id, Td, N, C, D, flags, ldE):
    nws = int(L.mcd_embed_gemm_exp_workspace(N, C, D))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
    E = Out(N, C, ldE, 0, torch.bfloat16, dev, tail=ldE - C)
    rinv = Out(1, N, N, 0, torch.float32, dev)
    ok(L.mcd_embed_gemm_exp(Id.data_ptr(), D, Td.data_ptr(), D, N, C, D, 10.0, flags, E.ptr, ldE, rinv.ptr, ws.data_ptr(), nws,
                            st()), L)
    return E, rinv


def _gexp_inputs(oracle, dev, N, C, D, flags):
    rng = np.random.default_rng(N + C)
    a, b = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((C, D)).astype(np.float32)
    if not flags:
        a, b = oracle.normalize_rows(a), oracle.normalize_rows(b)
    return T(a, dev), T(b, dev)


@pytest.mark.parametrize("shape", [(37, 40, 128, 0), (300, 763, 512, 0), (130, 257, 70, 1)])   # the last: MCD_GEMM_EXP_NORMALIZE
def test_embed_gemm_exp_pitches(L, dev, oracle, shape):
    """Columns C..ldE-1 of every row are bf16 +0 at every pitch -- also past the kernel's last 256-concept tile, where a
    pass of its own clears them -- and E[:, :C] and rinv do not depend on the pitch."""
    N, C, D, flags = shape
    Id, Td = _gexp_inputs(oracle, dev, N, C, D, flags)
    span = ceil_to(C, 256)
    E0, r0 = _gexp(L, dev, Id, Td, N, C, D, flags, ceil_to(C, 128))
    want_E, want_r = dense(E0.view), dense(r0.view)
    assert bool(torch.isfinite(want_r).all()) and bool((want_E.float() > 0).any())
    for ldE in uniq([ceil_to(C, 128), ceil_to(C, 16), span + 16, span + 256]):
        E, rinv = _gexp(L, dev, Id, Td, N, C, D, flags, ldE)
        E.check(want_E, zero_pad=True, what=("K1s E", shape, ldE))
        rinv.check(want_r, what=("K1s rinv", shape, ldE))
    odd = Out(N, C, ceil_to(C, 16) + 8, 0, torch.bfloat16, dev)
    assert L.mcd_embed_gemm_exp(Id.data_ptr(), D, Td.data_ptr(), D, N, C, D, 10.0, flags, odd.ptr, odd.ld, r0.ptr, None, 0,
                                st()) == -5       # MCD_E_UNSUPPORTED: a pitch that is no multiple of 16 is refused, untouched
    odd.check(torch.full((N, C), OUT_FILL, dtype=torch.bfloat16))


@pytest.mark.parametrize("soft", [1, 0])
@pytest.mark.parametrize("shape", [(37, 40, 128), (300, 763, 512)])
def test_wpmi_score_bf16_pitches(L, dev, oracle, shape, soft):
    N, C, D = shape
    U, K = 13, 20
    Id, Td = _gexp_inputs(oracle, dev, N, C, D, 0)
    b = ceil_to(C, 128)
    E0, r0 = _gexp(L, dev, Id, Td, N, C, D, 0, b)
    Ed, rinv = dense(E0.view), dense(r0.view)
    idxd = T(np.random.default_rng(C).integers(0, N, (U, K)).astype(np.int32), dev)
    pd = T(oracle.p_in_examples(K), dev)
    nws = int(L.mcd_wpmi_score_bf16_workspace(U, K))
    ws = torch.empty(max(nws, 8) // 8, dtype=torch.int64, device=dev)

    def call(E_ptr, ldE, idx_ptr, ldidx, out_ptr, ldo):
        ok(L.mcd_wpmi_score_bf16(E_ptr, ldE, N, C, rinv.data_ptr(), idx_ptr, ldidx, U, K, pd.data_ptr() if soft else None, 1e-7, soft,
                                 out_ptr, ldo, ws.data_ptr(), nws, st()), L)
    Eb = torch.zeros(N, b, dtype=torch.bfloat16, device=dev)
    Eb[:, :C] = Ed
    want = torch.empty(U, C, device=dev)
    call(Eb.data_ptr(), b, idxd.data_ptr(), K, want.data_ptr(), C)
    assert bool(torch.isfinite(want).all())
    for (pE, pidx, po), (_, _, oo) in one_at_a_time([b, b + 128, b + 1024], [K, K + 3], [C, C + 5], offs=(0, 0, 1)):
        for gap in GAP_FILLS:
            e_, i_ = In(Ed, pE, 0, gap), In(idxd, pidx, 0, _idx_gap(gap, N))
            out = Out(U, C, po, oo, torch.float32, dev)
            call(e_.ptr, pE, i_.ptr, pidx, out.ptr, po)
            out.check(want, what=("K4s", shape, soft, pE, pidx, po, oo, gap))
            e_.same(), i_.same()


# ---- K5 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 70, 763])
def test_logsumexp_sub_pitches_and_in_place(L, dev, C):
    """Segments [0, 7, 7, 40] (the middle one has no rows and is skipped: the result is that of [0, 7, 40], which the
    existing tests pin): both pitches on and off the 16-byte path, and out == pdge in place at a padded pitch."""
    offs, lam = [0, 7, 7, 40], 0.6
    Ut = offs[-1]
    xd = (torch.randn(Ut, C, generator=torch.Generator().manual_seed(C)) * 3 - 400).to(dev)
    seg = (ctypes.c_int64 * 4)(*offs)
    nws = int(L.mcd_logsumexp_sub_workspace(Ut, C, 3))
    ws = torch.empty(max(nws, 4) // 4, device=dev)
    want, want2 = torch.empty_like(xd), torch.empty_like(xd)
    ok(L.mcd_logsumexp_sub(xd.data_ptr(), C, C, seg, 3, lam, -1, want.data_ptr(), C, ws.data_ptr(), nws, st()), L)
    ok(L.mcd_logsumexp_sub(xd.data_ptr(), C, C, (ctypes.c_int64 * 3)(0, 7, 40), 2, lam, -1, want2.data_ptr(), C, ws.data_ptr(), nws,
                           st()), L)
    assert torch.equal(want, want2) and bool(torch.isfinite(want).all())
    for (px, po), (ox, oo) in one_at_a_time(pitches(C), pitches(C), offs=(1, 1)):
        for gap in GAP_FILLS:
            a, y = In(xd, px, ox, gap), Out(Ut, C, po, oo, torch.float32, dev)
            ok(L.mcd_logsumexp_sub(a.ptr, px, C, seg, 3, lam, -1, y.ptr, po, ws.data_ptr(), nws, st()), L)
            y.check(want, what=("K5", C, px, po, ox, oo, gap))
            a.same()
            ok(L.mcd_logsumexp_sub(a.ptr, px, C, seg, 3, lam, -1, a.ptr, px, ws.data_ptr(), nws, st()), L)     # out == pdge
            check_frame(a.flat, a.spec, want, what=("K5 in place", C, px, ox, gap))


# ---- K6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("C", [1030, 4100])        # the wave-per-row kernel of long rows, and K3's workgroup-per-row kernel
def test_row_topk_long_rows_pitches(L, dev, oracle, C, k):
    U = 9
    sim = np.random.default_rng(C + k).standard_normal((U, C)).astype(np.float32)
    sim[2, [17, 900]] = sim[2].max() + 1                         # a tie for the top: the lower concept index first
    v, i = oracle.row_topk(sim, k)
    simd = T(sim, dev)
    for ld in pitches(C):
        for off in (0, 1):
            for gap in GAP_FILLS:
                a = In(simd, ld, off, gap)
                vals, idx = Out(U, k, k, off, torch.float32, dev), Out(U, k, k, off, torch.int32, dev, fill=IDX_FILL)
                ok(L.mcd_row_topk(a.ptr, ld, U, C, k, vals.ptr, idx.ptr, st()), L)
                vals.check(v, what=("K6 vals", C, k, ld, off, gap))
                idx.check(i.astype(np.int32), what=("K6 idx", C, k, ld, off, gap))
                a.same()


# ---- K8 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [763, 40])
def test_rank_reorder_pitches_without_the_repack(L, dev, oracle, C):
    """The entry itself (the binding repacks P to a pitch of whole quads): the 16-byte gather reads P's padding up to the
    4-column tile, which must not reach the result; every pitch gives the bits of the call on the zero-padded dense P."""
    N, U, top_n, n_perm = 300, 13, 20, 5
    rng = np.random.default_rng(C)
    P = (rng.random((N, C)) * 0.5 + 0.05).astype(np.float32)
    v, i = oracle.col_topk(rng.standard_normal((N, U)).astype(np.float32), top_n)
    tv, ti = T(v.T, dev), T(i.T.astype(np.int32), dev)
    perms = T(np.stack([[rng.permutation(top_n) for _ in range(n_perm)] for _ in range(U)]).astype(np.int32), dev)
    Pd = T(P, dev)
    b = ceil_to(C, 4)
    Pb = torch.zeros(N, b, device=dev)
    Pb[:, :C] = Pd
    base = torch.empty(U, device=dev)
    want = torch.empty(U, C, device=dev)

    def call(P_ptr, ldP, tv_ptr, ti_ptr, ldt, out_ptr, ldo):
        ok(L.mcd_rank_reorder(P_ptr, ldP, N, C, tv_ptr, ti_ptr, ldt, U, top_n, perms.data_ptr(), n_perm, 3.0, 0.5, base.data_ptr(),
                              out_ptr, ldo, st()), L)
    call(Pb.data_ptr(), b, tv.data_ptr(), ti.data_ptr(), top_n, want.data_ptr(), C)
    assert bool(torch.isfinite(want).all())
    for (pP, pt, po), (oP, _, oo) in one_at_a_time(uniq([b, C, C + 1, b + 4]), [top_n, top_n + 3], [C, C + 5], offs=(1, 0, 1)):
        for gap in GAP_FILLS:
            p_, v_, i_ = In(Pd, pP, oP, gap), In(tv, pt, 0, gap), In(ti, pt, 0, _idx_gap(gap, N))
            out = Out(U, C, po, oo, torch.float32, dev)
            call(p_.ptr, pP, v_.ptr, i_.ptr, pt, out.ptr, po)
            out.check(want, what=("K8", C, pP, pt, po, oP, oo, gap))
            p_.same(), v_.same(), i_.same()


# ---- K0 / K0n -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 4), (3, 5)])            # HW % 4 == 0: the float4 loads; otherwise the scalar walk
@pytest.mark.parametrize("neuron_major", [False, True])
def test_hook_pool_writes_only_its_block(L, dev, hw, neuron_major):
    """K0 and K0n at row0 = 20, col0 = 7 of an activation matrix wider and taller than the block: the block holds the bits of
    the same entry on a dense [B, Cout] destination (K0n: of K0 on the NCHW copy), everything else keeps its fill."""
    B, Cout, row0, col0, n_total, u_total = 5, 70, 20, 7, 30, 90
    H, W = hw
    x = torch.randn(B, Cout, H, W, generator=torch.Generator().manual_seed(H)).to(dev)
    x_nhwc = x.contiguous(memory_format=torch.channels_last)
    for mode in (0, 1):
        block = torch.empty(B, Cout, device=dev)
        ok(L.mcd_hook_pool(x.data_ptr(), B, Cout, H * W, mode, block.data_ptr(), 0, 0, Cout, 1, st()), L)
        assert bool(torch.isfinite(block).all())
        rows, width = (u_total, n_total) if neuron_major else (n_total, u_total)
        want = torch.full((rows, width), OUT_FILL, device=dev)
        if neuron_major:
            want[col0:col0 + Cout, row0:row0 + B] = block.t()
        else:
            want[row0:row0 + B, col0:col0 + Cout] = block
        for pitch in pitches(width):
            for off in (0, 1):
                for entry, src in ((L.mcd_hook_pool, x), (L.mcd_hook_pool_nhwc, x_nhwc)):
                    dst = Out(rows, width, pitch, off, torch.float32, dev)
                    sn, su = (1, pitch) if neuron_major else (pitch, 1)
                    snap = src.clone()
                    ok(entry(src.data_ptr(), B, Cout, H * W, mode, dst.ptr, row0, col0, sn, su, st()), L)
                    dst.check(want, what=("K0", hw, neuron_major, mode, pitch, off, entry is L.mcd_hook_pool_nhwc))
                    assert torch.equal(src, snap)
