"""GPU: the encoder-side entries of the C ABI (K9, K9L, K9C, K10 - K21 of include/mcd_hip.h and the two mcd_linear_residual*
entries of include/mcd_blaslt.h) on framed buffers, and where a single NaN may go.

1. Frames.  The bindings allocate every operand with torch.empty at its exact size, and torch's caching allocator rounds the
   block up and packs tensors side by side: a store a few elements past an output lands in slack or in a neighbour, a load
   past an input reads a finite value.  Here every case calls the raw entry through mcd._lib.load() / load_blaslt() on
   torch's current stream with its operands inside util.framed() / util.framed_dense() allocations (test_gpu_abi_contracts.py
   does the same for the scoring-side entries; a contiguous N-d operand is a frame of one row):
     * every output starts as util.OUT_FILL inside a guard of 64 elements on both sides; util.check_frame() then wants the
       logical region bit-equal to the expected bits and every other element of the allocation still the fill;
     * every input's guards -- and, where the entry takes strides (K9C, the linear entries), its gaps -- hold NaN in one run
       and 1e30 in the next (util.GAP_FILLS); both runs are checked against the same expected bits, and the input
       allocations are bit-identical after the call (K15's in-place y excepted);
     * expected bits: the same entry on plain dense tensors at the binding's layout, which the existing tests pin against
       float64 (and K9L against K9 where both run).  The linear entries may pick another hipBLASLt algorithm per leading
       dimension, so their logical region is held to test_linear_residual_matches_torch's 2e-5 * max|ref| against float64 and
       only the guards and the pad columns are compared on the bits.
   The shapes are the smallest that reach each tile tail; the comments at the cases name the tail.

2. NaN locality.  The header claims that images, heads, pixels and channel slices do not see each other.  One NaN in an input
   is the cheapest probe: the isnan mask of the output must equal that of the float64 reference the entry's existing test
   uses (computed on the CPU with the same NaN), and the finite elements stay within that test's tolerance.  (Inf inputs are
   outside the contract: mcd_hip.h, K9.)"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import GAP_FILLS, OUT_FILL, check_frame, framed, framed_dense, int_bits, nerr

pytestmark = pytest.mark.gpu

GUARD = 64          # elements: 256 bytes of fp32, so base offset 0 is 16-byte aligned
NAN = float("nan")


@pytest.fixture(scope="module")
def L(mcd, dev):
    return mcd._lib.load()


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, L):
    assert rc == 0, L.mcd_last_error().decode()


def rnd(shape, seed, dev, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(dev)


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class In:
    """A contiguous N-d input inside a framed allocation whose guards hold `gap`; .same(): the call left all of it untouched."""

    def __init__(self, data, gap, off=0):
        self.flat, self.view, self.spec = framed_dense(tuple(data.shape), off, GUARD, gap, data.dtype, data.device)
        self.view.copy_(data)
        self.snap = self.flat.clone()
        self.ptr = self.flat.data_ptr() + (GUARD + off) * self.flat.element_size()

    def same(self):
        assert torch.equal(int_bits(self.flat), int_bits(self.snap)), "the call changed an input"


class Out:
    """A contiguous N-d output (an empty one too) inside a framed allocation of OUT_FILL."""

    def __init__(self, shape, dev):
        self.flat, self.view, self.spec = framed_dense(tuple(shape), 0, GUARD, OUT_FILL, torch.float32, dev)
        self.ptr = self.flat.data_ptr() + GUARD * 4      # (an empty tensor has no data_ptr of its own)

    def check(self, expected, what=""):
        check_frame(self.flat, self.spec, expected, what=str(what))


class Strided:
    """An input read through strides -- [B, T, W] with image / row strides (img, row, 1) -- inside ONE allocation of `gap`: the
    guards, the floats between two rows and those between two images all hold the fill."""

    def __init__(self, data, row, img, gap):
        B, T, W = data.shape
        assert row >= W and (B == 1 or img >= (T - 1) * row + W)
        self.flat = torch.full((2 * GUARD + (B - 1) * img + (T - 1) * row + W,), gap, device=data.device)
        torch.as_strided(self.flat, (B, T, W), (img, row, 1), GUARD).copy_(data)
        self.snap = self.flat.clone()
        self.ptr = self.flat.data_ptr() + GUARD * 4

    same = In.same


def run_framed(L, call, ins, out_shapes, what, expect=None, offs=None):
    """call(input pointers, output pointers) -> status.  Expected bits (returned): `expect`, or the call on the dense `ins`
    and plain dense outputs.  Then one run per gap fill on framed operands (input i at base offset offs[i])."""
    dev = ins[0].device
    if expect is None:
        dense = [torch.empty(max(numel(s), 1), device=dev) for s in out_shapes]
        ok(call([None if t is None else t.data_ptr() for t in ins], [d.data_ptr() for d in dense]), L)
        expect = [d[:numel(s)] for d, s in zip(dense, out_shapes)]
    for gap in GAP_FILLS:
        fi = [None if t is None else In(t, gap, offs[i] if offs else 0) for i, t in enumerate(ins)]
        fo = [Out(s, dev) for s in out_shapes]
        ok(call([None if a is None else a.ptr for a in fi], [o.ptr for o in fo]), L)
        for j, (o, e) in enumerate(zip(fo, expect)):
            o.check(e, what=what + ("output %d" % j, "gap %r" % gap, offs))
        for a in fi:
            if a is not None:
                a.same()
    return expect


# =========================================================================================================================
# 1. frames
# =========================================================================================================================
# ---- K9 / K9L -----------------------------------------------------------------------------------------------------------
# (B, T, H): one key and one query; a last tile of 1 key and a second wave with 1 live query; 4 waves, a last tile of 4 keys;
# the 8-wave maximum
K9_SHAPES = [(2, 1, 1), (2, 33, 2), (1, 100, 3), (1, 256, 1)]


def _attn_call(entry, B, T, H):
    return lambda i, o: entry(i[0], B, T, H, o[0], st())


@pytest.mark.parametrize("shape", K9_SHAPES)
def test_k9_frame(L, dev, shape):
    B, T, H = shape
    qkv = rnd((B, T, 3 * H * 64), T + H, dev)
    run_framed(L, _attn_call(L.mcd_vit_attention, B, T, H), [qkv], [(B, T, H * 64)], ("K9", shape))


# (3, 257, 1): 6 (image, head, block) pairs on the 8-XCD grid -- two surplus workgroups return early -- and a last block with
# 1 live query; (1, 300, 2): a second block of two live waves, a last key tile of 12
@pytest.mark.parametrize("shape", K9_SHAPES + [(3, 257, 1), (1, 300, 2)])
def test_k9l_frame_and_k9_bits(L, dev, shape):
    B, T, H = shape
    qkv = rnd((B, T, 3 * H * 64), T + H, dev)
    expect = None
    if T <= 256:                                    # the header: for T <= 256 the result is K9's, bit for bit
        k9 = torch.empty(B, T, H * 64, device=dev)
        ok(L.mcd_vit_attention(qkv.data_ptr(), B, T, H, k9.data_ptr(), st()), L)
        expect = [k9]
    run_framed(L, _attn_call(L.mcd_vit_attention_long, B, T, H), [qkv], [(B, T, H * 64)], ("K9L", shape), expect=expect)


# ---- K9C ----------------------------------------------------------------------------------------------------------------
def _k9c(L, q_ptr, q_img, k_ptr, k_row, k_img, v_ptr, v_row, v_img, B, T, H, out_ptr):
    return L.mcd_vit_attention_cls(q_ptr, q_img, k_ptr, k_row, k_img, v_ptr, v_row, v_img, B, T, H, out_ptr, st())


# T = 1, 3: streams that never see a key; 5, 17: one pass with dead rows, a second pass; 513, 530: the four-wave split (a
# slice with one key; a partial last pass).  (3, 1): a workgroup of four pairs with a dead wave / a grid of three split pairs.
@pytest.mark.parametrize("BH", [(2, 2), (3, 1)])
@pytest.mark.parametrize("T", [1, 3, 5, 17, 513, 530])
def test_k9c_frame_and_strides(L, dev, T, BH):
    """Every stride of the entry varied alone over its pitch classes W, W + 4, 2 W, 3 W (the image strides: the tight value
    (T - 1) * row + W and that + 4), the gaps holding the fill: the bits of the call on dense [B, W] / [B, T, W] operands."""
    B, H = BH
    W = H * 64
    q, k, v = rnd((B, 1, W), T, dev), rnd((B, T, W), T + 1, dev), rnd((B, T, W), T + 2, dev)
    want = torch.empty(B, W, device=dev)
    ok(_k9c(L, q.data_ptr(), W, k.data_ptr(), W, T * W, v.data_ptr(), W, T * W, B, T, H, want.data_ptr()), L)
    assert bool(torch.isfinite(want).all())
    tight = lambda row: (T - 1) * row + W
    combos = [(W, W, None, W, None)]
    combos += [(p, W, None, W, None) for p in (W + 4, 2 * W, 3 * W)]
    combos += [(W, p, None, W, None) for p in (W + 4, 2 * W, 3 * W)]
    combos += [(W, W, None, p, None) for p in (W + 4, 2 * W, 3 * W)]
    combos += [(W, W, 4, W, None), (W, W, None, W, 4), (W + 4, 2 * W, 4, 3 * W, 4)]
    for q_img, k_row, dk, v_row, dv in combos:
        k_img, v_img = tight(k_row) + (dk or 0), tight(v_row) + (dv or 0)
        for gap in GAP_FILLS:
            q_, k_, v_ = Strided(q, W, q_img, gap), Strided(k, k_row, k_img, gap), Strided(v, v_row, v_img, gap)
            out = Out((B, W), dev)
            ok(_k9c(L, q_.ptr, q_img, k_.ptr, k_row, k_img, v_.ptr, v_row, v_img, B, T, H, out.ptr), L)
            out.check(want, what=("K9C", T, BH, q_img, k_row, k_img, v_row, v_img, gap))
            q_.same(), k_.same(), v_.same()


# ---- K10 ----------------------------------------------------------------------------------------------------------------
# (rows, D): NV = 1 with one live lane; NV = 2 (one lane in the second register row), a last workgroup of 1 live wave; D / 4 =
# 257 quads -> 5 register rows on the NV = 6 instantiation (a dead row), 3 live waves; 385 quads -> 7 rows on NV = 8; 2048: NV
# = 8, every lane of every row live, 2 live waves
@pytest.mark.parametrize("shape", [(1, 4), (5, 260), (7, 1028), (3, 1540), (2, 2048)])
def test_k10_frame(L, dev, shape):
    rows, D = shape
    x, g, b = rnd(shape, D, dev, 2.0, 1.0), rnd((D,), D + 1, dev), rnd((D,), D + 2, dev)
    run_framed(L, lambda i, o: L.mcd_layer_norm(i[0], rows, D, i[1], i[2], 1e-5, o[0], st()), [x, g, b], [shape], ("K10", shape))


# ---- K11 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 8, 8, 4), (1, 3, 16, 32, 8), (3, 2, 4, 12, 4)])
def test_k11_frame(L, dev, shape):
    B, Cin, H, W, P = shape
    x = rnd((B, Cin, H, W), H + W, dev)
    run_framed(L, lambda i, o: L.mcd_patchify(i[0], B, Cin, H, W, P, o[0], st()), [x],
               [(B, 1 + (H // P) * (W // P), Cin * P * P)], ("K11", shape))


# ---- K12 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 1, 1, 4), (1, 3, 7, 9, 48), (2, 4, 5, 4, 8)])
def test_k12_frame(L, dev, shape):
    B, Cin, H, W, Cout = shape
    x, w, b = rnd((B, Cin, H, W), H, dev), rnd((Cin, 3, 3, Cout), Cout, dev, 0.3), rnd((Cout,), 5, dev, 0.1)
    run_framed(L, lambda i, o: L.mcd_conv_stem_nhwc(i[0], B, Cin, H, W, i[1], i[2], Cout, o[0], st()), [x, w, b],
               [(B, (H + 1) // 2, (W + 1) // 2, Cout)], ("K12", shape))


# ---- K13 ----------------------------------------------------------------------------------------------------------------
# (C, H, W): one pixel, one quad; 5 quads in one slice, a tile with tails on both axes; 17 quads: slices of 9 + 8 (k = 3),
# 6 + 6 + 5 (k = 5, stride 2), output tiles with tails in both axes; 8 quads: two slices of 4 at k = 5, stride 2
@pytest.mark.parametrize("silu_in", [0, 1])
@pytest.mark.parametrize("ks", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("shape", [(4, 1, 1), (20, 5, 6), (68, 9, 17), (32, 8, 8)])
def test_k13_frame(L, core, dev, shape, ks, silu_in):
    C, H, W = shape
    (k, s), B = ks, 2
    x, w, b = rnd((B, H, W, C), C + H, dev), rnd((k * k, C), k, dev, 1.0 / k), rnd((C,), 3, dev, 0.1)
    Ho, Wo = -(-H // s), -(-W // s)
    T = core.dwconv_tiles(Ho, Wo)
    run_framed(L, lambda i, o: L.mcd_dwconv_bn_silu(i[0], B, H, W, C, i[1], i[2], k, s, silu_in, o[0], o[1], T, st()), [x, w, b],
               [(B, Ho, Wo, C), (B, T, C)], ("K13", shape, ks, silu_in))


# ---- K14 ----------------------------------------------------------------------------------------------------------------
# (B, T, C, sq): one tile, one SE unit; the 16-way unrolled tile loop plus a tail of 1, SE units on a second pass of the four
# waves; exactly one unrolled pass, channels on a second pass of the 256 threads
@pytest.mark.parametrize("shape", [(2, 1, 4, 1), (3, 17, 24, 5), (2, 16, 260, 3)])
def test_k14_frame(L, dev, shape):
    B, T, C, sq = shape
    hw = 7 * T
    ins = [rnd((B, T, C), C, dev, 3.0), rnd((sq, C), 1, dev, C ** -0.5), rnd((sq,), 2, dev, 0.1), rnd((sq, C), 3, dev, sq ** -0.5),
           rnd((C,), 4, dev, 0.1)]
    run_framed(L, lambda i, o: L.mcd_se_gate(i[0], B, T, C, hw, i[1], i[2], sq, i[3], i[4], o[0], st()), ins, [(B, C)],
               ("K14", shape))


# ---- K15 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 4), (3, 35, 20), (2, 64, 260)])
def test_k15_frame_in_place(L, dev, shape):
    """y is scaled in place: its frame's guards hold the gap fill and must keep it; s is an input like any other."""
    B, HW, C = shape
    y, s = rnd(shape, C, dev), rnd((B, C), HW, dev)
    want = y.clone()
    ok(L.mcd_channel_scale(want.data_ptr(), B, HW, C, s.data_ptr(), st()), L)
    for gap in GAP_FILLS:
        y_, s_ = In(y, gap), In(s, gap)
        ok(L.mcd_channel_scale(y_.ptr, B, HW, C, s_.ptr, st()), L)
        check_frame(y_.flat, y_.spec, want, what=("K15", shape, gap))
        s_.same()


# ---- K16 / K19 ----------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout): one pixel, the 4-channel pass; two tiles across, both partial; the 4-channel pass (Cout % 32) with
# four channels in, 2 x 2 tiles, partial; one whole tile, two 32-channel passes
STEM_SHAPES = [(2, 1, 1, 1, 4), (1, 3, 17, 33, 32), (2, 4, 31, 35, 36), (1, 2, 32, 32, 64)]


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_k16_frame(L, dev, shape):
    B, Cin, H, W, Cout = shape
    x, w = rnd((B, Cin, H, W), H, dev), rnd((Cin, 7, 7, Cout), Cout, dev, 0.1)
    run_framed(L, lambda i, o: L.mcd_conv7x7s2_nhwc(i[0], B, Cin, H, W, i[1], Cout, o[0], st()), [x, w],
               [(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout)], ("K16", shape))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_k19_frame(L, dev, shape, relu):
    """x needs 4-byte alignment only (the header): base offset 1 gives the same bits."""
    B, Cin, H, W, Cout = shape
    x, w, b = rnd((B, Cin, H, W), H, dev), rnd((Cin, 3, 3, Cout), Cout, dev, 0.2), rnd((Cout,), 6, dev)
    call = lambda i, o: L.mcd_conv3x3s2_nhwc(i[0], B, Cin, H, W, i[1], i[2], Cout, relu, o[0], st())
    shapes = [(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout)]
    want = run_framed(L, call, [x, w, b], shapes, ("K19", shape, relu))
    run_framed(L, call, [x, w, b], shapes, ("K19", shape, relu), expect=want, offs=(1, 0, 0))


# ---- K17 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 1, 4), (1, 2, 2, 8), (2, 7, 9, 20), (1, 33, 24, 64)])
def test_k17_frame(L, dev, shape):
    B, H, W, C = shape
    x, sc, sh = rnd(shape, H + C, dev), rnd((C,), 1, dev), rnd((C,), 2, dev, 0.3)
    run_framed(L, lambda i, o: L.mcd_bn_relu_maxpool_nhwc(i[0], B, H, W, C, i[1], i[2], o[0], st()), [x, sc, sh],
               [(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)], ("K17", shape))


# ---- K18 ----------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, k, stride): one pixel, half a channel tile; 105 pixels: one pixel tile spanning three images, channel
# tiles of 64 + 32; 150 pixels: two pixel tiles, the second of 22; stride 2, two k-steps per tap, a partial chunk at the end;
# 1 x 1 / 2, 72 pixels, channel tiles of 64 + 64 + 32
K18_SHAPES = [(1, 1, 1, 32, 32, 3, 1), (3, 5, 7, 32, 96, 3, 1), (5, 6, 5, 32, 64, 3, 1), (2, 9, 9, 64, 32, 3, 2),
              (2, 12, 11, 32, 160, 1, 2)]


def _k18_out(shape):
    B, H, W, Cin, Cout, k, s = shape
    pad = 1 if k == 3 else 0
    return B, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1, Cout


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", K18_SHAPES)
def test_k18_frame(L, dev, shape, relu, with_res):
    """relu_in / relu_out as 00 and 11; res is framed like an input.  res == NULL through the residual entry: the plain
    entry's bits (the header), on frames too."""
    B, H, W, Cin, Cout, k, s = shape
    oshape = _k18_out(shape)
    x, w, b = rnd((B, H, W, Cin), H + Cin, dev), rnd((Cout, k * k * Cin), Cout, dev, (k * k * Cin) ** -0.5), rnd((Cout,), 7, dev)
    res = rnd(oshape, 8, dev, 1.5) if with_res else None
    call = lambda i, o: L.mcd_conv_igemm_res_nhwc(i[0], B, H, W, Cin, i[1], i[2], i[3], Cout, k, s, relu, relu, o[0], st())
    if with_res:
        run_framed(L, call, [x, w, b, res], [oshape], ("K18 res", shape, relu))
        return
    plain = lambda i, o: L.mcd_conv_igemm_nhwc(i[0], B, H, W, Cin, i[1], i[2], Cout, k, s, relu, relu, o[0], st())
    want = run_framed(L, plain, [x, w, b], [oshape], ("K18", shape, relu))
    run_framed(L, call, [x, w, b, None], [oshape], ("K18 res = NULL", shape, relu), expect=want)


# ---- K20 ----------------------------------------------------------------------------------------------------------------
# (2, 1, 5, 8): one row pools to an empty output -- MCD_OK, and the whole output frame is still fill
@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 9, 11, 32), (1, 3, 2, 8), (2, 1, 5, 8)])
def test_k20_frame(L, dev, shape):
    B, H, W, C = shape
    x = rnd(shape, H * W, dev, 3.0)
    run_framed(L, lambda i, o: L.mcd_avgpool2_nhwc(i[0], B, H, W, C, o[0], st()), [x], [(B, H // 2, W // 2, C)], ("K20", shape))


# ---- K21 ----------------------------------------------------------------------------------------------------------------
# (B, HW, C): one pixel, one quad; 49 pixels (one pass past the four-fold unroll); 65 quads: a second workgroup of 1 live lane
@pytest.mark.parametrize("shape", [(2, 1, 4), (3, 49, 64), (2, 4, 260)])
def test_k21_frame(L, dev, shape):
    B, HW, C = shape
    x, pos = rnd(shape, HW + C, dev, 1.0, 0.5), rnd((HW + 1, C), C, dev, C ** -0.5)
    run_framed(L, lambda i, o: L.mcd_attnpool_tokens(i[0], B, HW, C, i[1], o[0], st()), [x, pos], [(B, HW + 1, C)], ("K21", shape))


# ---- mcd_linear_residual / mcd_linear_residual_relu ---------------------------------------------------------------------
class Mat:
    """A [rows, width] matrix of pitch ld in a util.framed() allocation of `fill` (the last row's padding included)."""

    def __init__(self, data, ld, fill):
        rows, width = data.shape
        self.spec = (rows, width, ld, 0, GUARD, fill)
        self.flat, self.view = framed(rows, width, ld, 0, GUARD, fill, torch.float32, data.device, tail=ld - width)
        self.view.copy_(data)
        self.snap = self.flat.clone()
        self.ptr = self.view.data_ptr()

    same = In.same

    def logical_and_rest(self):
        """(a copy of the logical region, whether everything else still has the bits it had at construction)."""
        got = self.view.clone()
        now, then = self.flat.clone(), self.snap.clone()
        for f in (now, then):
            torch.as_strided(f, self.spec[:2], (self.spec[2], 1), GUARD).zero_()
        return got, torch.equal(int_bits(now), int_bits(then))


def _ld_cases(widths):
    """One leading dimension at a time over w, w + 4, w + 1, plus all of them odd."""
    base = list(widths)
    out = [tuple(base)]
    for i, w in enumerate(base):
        for p in (w + 4, w + 1):
            out.append(tuple(base[:i] + [p] + base[i + 1:]))
    out.append(tuple(w + 1 + w % 2 for w in base))
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(5, 8, 4), (37, 40, 100)])
def test_linear_residual_frames(mcd, dev, monkeypatch, shape, relu):
    """res = NULL, res apart and res == out (in place, at a pitch: the pad columns must survive), with and without a bias, every
    leading dimension varied alone.  The logical region against float64 at 2e-5 * max|ref|; the guards and the pad columns of
    out, and all of h, W, bias and a separate res, on the bits.  A leading dimension the library refuses comes back as a
    non-zero status with the output frame untouched; it is recorded (and printed), not skipped -- the packed layout the
    binding uses must never be refused."""
    B = mcd._lib.load_blaslt()
    if B is None:
        pytest.skip("libmcd_blaslt.so not built")
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")      # no new (shape, pitch) key times 32 candidates
    M, N, K = shape
    entry = B.mcd_linear_residual_relu if relu else B.mcd_linear_residual
    ws = torch.empty(B.mcd_linear_residual_workspace(), dtype=torch.uint8, device=dev)
    h, W, bias, res = rnd((M, K), M, dev), rnd((N, K), N, dev, 0.05), rnd((1, N), K, dev), rnd((M, N), M + N, dev)
    prod = h.double() @ W.double().T
    refused, ran = [], 0
    for mode in ("none", "apart", "in_place"):
        for with_bias in (False, True):
            ref = prod + (res.double() if mode != "none" else 0) + (bias.double() if with_bias else 0)
            ref = F.relu(ref) if relu else ref
            tol = 2e-5 * float(ref.abs().max())
            lds = _ld_cases([K, K, N, N]) if mode == "apart" else [c[:2] + (c[2], c[2]) for c in _ld_cases([K, K, N])]
            for ldh, ldw, ldr, ldo in lds:
                for gap in GAP_FILLS:
                    what = (shape, relu, mode, with_bias, ldh, ldw, ldr, ldo, gap)
                    h_, w_, b_ = Mat(h, ldh, gap), Mat(W, ldw, gap), Mat(bias, N, gap)
                    out = Mat(res if mode == "in_place" else torch.full((M, N), OUT_FILL, device=dev), ldo, OUT_FILL)
                    r_ = Mat(res, ldr, gap) if mode == "apart" else None
                    rptr = {"none": None, "apart": r_ and r_.ptr, "in_place": out.ptr}[mode]
                    rc = entry(h_.ptr, ldh, w_.ptr, ldw, b_.ptr if with_bias else None, rptr, ldr, out.ptr, ldo, M, N, K,
                               ws.data_ptr(), ws.numel(), st())
                    got, rest_kept = out.logical_and_rest()
                    assert rest_kept, ("a guard or a pad column of out changed", what)
                    for a in (h_, w_, b_, r_):
                        if a is not None:
                            a.same()
                    if rc != 0:
                        out.same()                  # refused: nothing was written
                        assert (ldh, ldw, ldr, ldo) != (K, K, N, N), ("the packed layout was refused", what, rc)
                        refused.append(what + (rc, B.mcd_blaslt_last_error().decode()))
                        continue
                    ran += 1
                    err = float((got.double() - ref).abs().max())
                    assert err <= tol, (what, err, tol)      # (a NaN from a gap makes err NaN: not <= tol)
    print("mcd_linear_residual%s %s: %d calls ran, %d refused" % ("_relu" if relu else "", shape, ran, len(refused)))
    for r in refused:
        print("  refused:", r)
    assert ran > 0


# =========================================================================================================================
# 2. NaN locality and dominance
# =========================================================================================================================
def _attn64(q, k, v):
    """softmax(q k^T / 8) v per head without a BLAS call (a library GEMM may treat a NaN operand its own way): q [B, Tq, H, 64],
    k, v [B, T, H, 64] -> [B, Tq, H, 64], in the operands' precision."""
    s = (q[:, :, None] * k[:, None]).sum(-1) / 8.0                   # [B, Tq, T, H]
    p = torch.softmax(s, dim=2)
    return (p[..., None] * v[:, None]).sum(2)


def _attn_bound(ref, ref32):
    """test_vit_attention_matches_sdpa's (and test_k9c_matches_float64's) bound, on the finite elements."""
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(ref32))
    return fin, 3e-6 * max(1.0, float(ref[fin].abs().max())) + 3 * float((ref32.double() - ref)[fin].abs().max())


def _check_mask_and_values(got, ref, fin, bound, what):
    got = got.double().cpu()
    assert torch.equal(torch.isnan(got), ~fin), (what, "NaN mask", int(torch.isnan(got).sum()), int((~fin).sum()))
    err = float((got - ref)[fin].abs().max())
    print(what, "err %.3e bound %.3e" % (err, bound))
    assert err <= bound, (what, err, bound)


# where the NaN goes: (operand 0 = q | 1 = k | 2 = v, image, token, head, d); key 35 is in the last, partial key tile
ATTN_NANS = [(0, 1, 37, 1, 5), (1, 0, 35, 1, 60), (2, 1, 35, 0, 17)]


@pytest.mark.parametrize("entry", ["mcd_vit_attention", "mcd_vit_attention_long"])
def test_k9_nan_locality(L, dev, entry):
    """A NaN in q[b, t, h] -> exactly that output row of that head; in k[b, j, h] -> every query of (b, h) and nothing else; in
    v[b, j, h, d] -> column d of every query of (b, h) and nothing else."""
    B, T, H = 2, 40, 2
    for which, b, t, h, d in ATTN_NANS:
        qkv = rnd((B, T, 3, H, 64), 11, "cpu")
        qkv[b, t, which, h, d] = NAN
        ref = _attn64(*qkv.double().unbind(2))
        fin, bound = _attn_bound(ref, _attn64(*qkv.unbind(2)))
        want = torch.zeros(B, T, H, 64, dtype=torch.bool)
        if which == 0:
            want[b, t, h] = True
        elif which == 1:
            want[b, :, h] = True
        else:
            want[b, :, h, d] = True
        assert torch.equal(~fin, want)                                  # the reference itself states the claim
        g, out = qkv.to(dev), torch.empty(B, T, H * 64, device=dev)
        ok(getattr(L, entry)(g.data_ptr(), B, T, H, out.data_ptr(), st()), L)
        _check_mask_and_values(out.view(B, T, H, 64), ref, fin, bound, (entry, which, b, t, h, d))


@pytest.mark.parametrize("shape", [(2, 40, 2), (1, 530, 2)])
def test_k9c_nan_locality(L, dev, shape):
    B, T, H = shape
    W = H * 64
    for which, b, t, h, d in ATTN_NANS:
        b, t = min(b, B - 1), (0 if which == 0 else T - 5)               # (K9C's one query is token 0's)
        qkv = rnd((B, T, 3, H, 64), 12, "cpu")
        qkv[b, t, which, h, d] = NAN
        q, k, v = qkv.unbind(2)
        ref = _attn64(q[:, :1].double(), k.double(), v.double())[:, 0]
        fin, bound = _attn_bound(ref, _attn64(q[:, :1], k, v)[:, 0])
        want = torch.zeros(B, H, 64, dtype=torch.bool)
        if which == 2:
            want[b, h, d] = True
        else:
            want[b, h] = True
        assert torch.equal(~fin, want)
        g = qkv.to(dev)
        out = torch.empty(B, W, device=dev)
        ok(_k9c(L, g.data_ptr(), T * 3 * W, g.data_ptr() + 4 * W, 3 * W, T * 3 * W, g.data_ptr() + 8 * W, 3 * W, T * 3 * W, B, T, H,
                out.data_ptr()), L)
        _check_mask_and_values(out.view(B, H, 64), ref, fin, bound, ("K9C", shape, which, b, t, h, d))


def test_attention_dominant_key_in_the_last_partial_tile(L, dev):
    """(1, 40, 1) with every q = 50 k_j, j = 37 inside the last tile of 8 keys: score j leads the others by |k_j|^2 50 / 8 ~ 400
    against a spread of ~ 50, so every probability but p_j underflows and the output row is v_j -- to 3e-6 * max|v|, the
    bound of the existing K9 test.  A tile tail that drops, repeats or misplaces key j cannot pass."""
    B, T, H, j = 1, 40, 1, 37
    qkv = rnd((B, T, 3, H, 64), 13, "cpu")
    qkv[:, :, 0] = 50.0 * qkv[:, j:j + 1, 1]
    v_j, tol = qkv[0, j, 2, 0].double(), 3e-6 * float(qkv[:, :, 2].abs().max())
    g = qkv.to(dev)
    for entry in (L.mcd_vit_attention, L.mcd_vit_attention_long):
        out = torch.empty(B, T, 64, device=dev)
        ok(entry(g.data_ptr(), B, T, H, out.data_ptr(), st()), L)
        err = float((out[0].double().cpu() - v_j).abs().max())
        print("dominance", entry.__name__, "err %.3e tol %.3e" % (err, tol))
        assert err <= tol, (entry.__name__, err, tol)
    out = torch.empty(B, 64, device=dev)
    ok(_k9c(L, g.data_ptr(), T * 192, g.data_ptr() + 256, 192, T * 192, g.data_ptr() + 512, 192, T * 192, B, T, H, out.data_ptr()), L)
    err = float((out[0].double().cpu() - v_j).abs().max())
    print("dominance K9C err %.3e tol %.3e" % (err, tol))
    assert err <= tol, ("K9C", err, tol)


def test_k10_nan_locality(L, dev):
    """Row 5 of 8 shares its workgroup with rows 4, 6 and 7: a NaN in it makes that row NaN and no other."""
    rows, D = 8, 260
    x, g, b = rnd((rows, D), 1, "cpu", 2.0), rnd((D,), 2, "cpu"), rnd((D,), 3, "cpu")
    x[5, 100] = NAN
    ref = F.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-12)
    fin = torch.isfinite(ref)
    want = torch.zeros(rows, D, dtype=torch.bool)
    want[5] = True
    assert torch.equal(~fin, want)
    y, t = torch.empty(rows, D, device=dev), [a.to(dev) for a in (x, g, b)]
    ok(L.mcd_layer_norm(t[0].data_ptr(), rows, D, t[1].data_ptr(), t[2].data_ptr(), 1e-12, y.data_ptr(), st()), L)
    _check_mask_and_values(y, ref, fin, 3e-6 * max(1.0, float(ref[fin].abs().max())), "K10")     # test_layer_norm_matches_torch's


def _dw_ref(core, x64, w_tap, bias, k, s, silu_in):
    """test_gpu_mbconv.py's float64 reference of K13: depthwise conv on NHWC x64 with TF-SAME padding -> [B, Ho, Wo, C]."""
    B, H, W, C = x64.shape
    a = x64.permute(0, 3, 1, 2)
    if silu_in:
        a = F.silu(a)
    _, pt, pb = core.same_pad(H, k, s)
    _, pl, pr = core.same_pad(W, k, s)
    w = w_tap.double().t().reshape(C, 1, k, k)
    return F.silu(F.conv2d(F.pad(a, [pl, pr, pt, pb]), w, bias.double(), s, 0, 1, C)).permute(0, 2, 3, 1)


@pytest.mark.parametrize("silu_in", [0, 1])
def test_k13_nan_locality(L, core, dev, silu_in):
    """(68, 9, 17), k = 5, stride 2 (channel slices of 6 + 6 + 5 quads, output 5 x 9 = two tiles): a NaN at one pixel and channel
    -> the output pixels whose window holds it, that channel only, and the psum entries of the tiles those pixels lie in, that
    channel and image only.  y to test_k13_against_float64's 2e-6; psum as there, through the means it gives (on the (image,
    channel) pairs whose tiles are all finite)."""
    C, H, W, k, s, B = 68, 9, 17, 5, 2, 2
    x, w, b = rnd((B, H, W, C), 21, "cpu"), rnd((k * k, C), 22, "cpu", 1.0 / k), rnd((C,), 23, "cpu", 0.1)
    x[1, 4, 14, 37] = NAN                                             # its window's output pixels (columns 6 - 8) lie in both tiles
    ref = _dw_ref(core, x.double(), w, b, k, s, silu_in)
    Ho, Wo = ref.shape[1:3]
    T = core.dwconv_tiles(Ho, Wo)
    assert (Ho, Wo, T) == (5, 9, 2)
    fin = torch.isfinite(ref)
    bad = (~fin).nonzero()
    assert 0 < bad.shape[0] <= 9 and bool((bad[:, 0] == 1).all()) and bool((bad[:, 3] == 37).all())
    y, psum = torch.empty(B, Ho, Wo, C, device=dev), torch.empty(B, T, C, device=dev)
    t = [a.to(dev) for a in (x, w, b)]
    ok(L.mcd_dwconv_bn_silu(t[0].data_ptr(), B, H, W, C, t[1].data_ptr(), t[2].data_ptr(), k, s, silu_in, y.data_ptr(),
                            psum.data_ptr(), T, st()), L)
    y, psum = y.double().cpu(), psum.double().cpu()
    assert torch.equal(torch.isnan(y), ~fin)
    scale = float(ref[fin].abs().max())
    assert float((y - ref)[fin].abs().max()) / scale < 2e-6
    tiles = torch.stack([ref[:, :, 8 * t:8 * t + 8].sum(dim=(1, 2)) for t in range(T)], dim=1)        # [B, T, C] (one tile row)
    assert bool(torch.isnan(tiles[1, :, 37]).all()) and int(torch.isnan(tiles).sum()) == 2
    assert torch.equal(torch.isnan(psum), torch.isnan(tiles))
    mean, rmean = psum.sum(1) / (Ho * Wo), ref.mean(dim=(1, 2))
    mfin = torch.isfinite(rmean)
    assert torch.equal(torch.isfinite(mean), mfin)
    assert float((mean - rmean)[mfin].abs().max()) / float(rmean[mfin].abs().max()) < 2e-6


def test_k14_nan_locality(L, dev):
    """A NaN in one image's psum -> that image's gate (all of it: every SE unit reads every channel) and no other image's."""
    B, T, C, sq, hw = 3, 17, 24, 5, 119
    psum, wr, br = rnd((B, T, C), 31, "cpu", (hw / T) ** 0.5), rnd((sq, C), 32, "cpu", C ** -0.5), rnd((sq,), 33, "cpu", 0.1)
    we, be = rnd((C, sq), 34, "cpu", sq ** -0.5), rnd((C,), 35, "cpu", 0.1)
    psum[1, 9, 7] = NAN
    mean = psum.double().sum(1) / hw
    hid = F.silu((mean[:, None, :] * wr.double()[None]).sum(-1) + br.double())                  # (no BLAS call on a NaN)
    ref = torch.sigmoid((hid[:, None, :] * we.double()[None]).sum(-1) + be.double())
    fin = torch.isfinite(ref)
    want = torch.zeros(B, C, dtype=torch.bool)
    want[1] = True
    assert torch.equal(~fin, want)
    s = torch.empty(B, C, device=dev)
    t = [a.to(dev) for a in (psum, wr, br, we.t().contiguous(), be)]
    ok(L.mcd_se_gate(t[0].data_ptr(), B, T, C, hw, t[1].data_ptr(), t[2].data_ptr(), sq, t[3].data_ptr(), t[4].data_ptr(),
                     s.data_ptr(), st()), L)
    _check_mask_and_values(s, ref, fin, 2e-6 * float(ref[fin].abs().max()), "K14")              # test_k14_against_float64's


@pytest.mark.parametrize("relu", [0, 1])
def test_k18_nan_locality(L, dev, relu):
    """(3, 5, 7, 32, 96, 3, 1): the 105 output pixels of the three images share ONE pixel tile.  A NaN in x[b, y, x, c] -> the up
    to nine output pixels around it, all 96 channels, and no tile-mate of another image (the corner case: image 1's first
    pixel follows image 0's last in the tile); a NaN in res -> that one element.  Finite elements to the existing K18 bound,
    2 * (ATen's error on the NaN-free input) + 1e-6, of the output's maximum."""
    B, H, W, Cin, Cout, k, s = 3, 5, 7, 32, 96, 3, 1
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(B, H, W, Cout, generator=g) * 1.5
    w_tap = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    act = (lambda t: F.relu(t)) if relu else (lambda t: t)

    def ref_of(xx, ww, bb, rr):
        y = F.conv2d(act(xx.permute(0, 3, 1, 2)), ww, bb, s, 1) + rr.permute(0, 3, 1, 2)
        return act(y).permute(0, 2, 3, 1)
    clean = ref_of(x.double(), w.double(), bias.double(), res.double())
    aten = ref_of(x.to(dev), w.to(dev), bias.to(dev), res.to(dev))
    bound = 2 * nerr(aten, clean) + 1e-6
    scale = float(clean.abs().max())
    for where in ("x", "x corner", "res"):
        xn, rn = x.clone(), res.clone()
        want = torch.zeros(B, H, W, Cout, dtype=torch.bool)
        if where == "x":
            xn[1, 2, 3, 9] = NAN
            want[1, 1:4, 2:5] = True
        elif where == "x corner":
            xn[1, 0, 0, 30] = NAN
            want[1, 0:2, 0:2] = True
        else:
            rn[1, 2, 3, 50] = NAN
            want[1, 2, 3, 50] = True
        ref = ref_of(xn.double(), w.double(), bias.double(), rn.double())
        fin = torch.isfinite(ref)
        assert torch.equal(~fin, want), where
        t = [a.to(dev) for a in (xn, w_tap, bias, rn)]
        y = torch.empty(B, H, W, Cout, device=dev)
        ok(L.mcd_conv_igemm_res_nhwc(t[0].data_ptr(), B, H, W, Cin, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), Cout, k, s,
                                     relu, relu, y.data_ptr(), st()), L)
        _check_mask_and_values(y, ref, fin, bound * scale, ("K18", relu, where))


def test_k21_nan_locality(L, dev):
    """A NaN at x[b, p, c] -> tok[b, 0, c] (the mean) and tok[b, 1 + p, c], nothing else.  Rows 1.. are torch's bits; row 0 to
    test_k21_tokens' bound, 2 * (ATen's error on the NaN-free input) + 1e-6."""
    B, HW, C = 3, 49, 64
    x, pos = rnd((B, HW, C), 51, "cpu", 1.0, 0.5), rnd((HW + 1, C), 52, "cpu", C ** -0.5)
    r0 = x.double().mean(dim=1) + pos[0].double()
    bound = (2 * nerr(x.to(dev).mean(dim=1) + pos[0].to(dev), r0) + 1e-6) * float(r0.abs().max())
    x[1, 20, 13] = NAN
    ref = torch.cat([(x.double().mean(dim=1) + pos[0].double())[:, None], x.double() + pos[1:].double()], dim=1)
    fin = torch.isfinite(ref)
    want = torch.zeros(B, HW + 1, C, dtype=torch.bool)
    want[1, 0, 13] = want[1, 21, 13] = True
    assert torch.equal(~fin, want)
    tok, xg, pg = torch.empty(B, HW + 1, C, device=dev), x.to(dev), pos.to(dev)
    ok(L.mcd_attnpool_tokens(xg.data_ptr(), B, HW, C, pg.data_ptr(), tok.data_ptr(), st()), L)
    tok = tok.cpu()
    assert torch.equal(torch.isnan(tok), ~fin)
    rows = (x + pos[1:])
    assert torch.equal(tok[:, 1:][fin[:, 1:]], rows[fin[:, 1:]])
    _check_mask_and_values(tok[:, 0], ref[:, 0], fin[:, 0], bound, "K21 row 0")
