"""GPU: the ResNet-50 target's HIP route -- K16 (7x7 / 2 stem), K17 (bn + relu + max pooling) and K18 (implicit-GEMM
convolution on the exact-fp32 MFMA) against float64 and against ATen's own fp32 error, batch invariance bit for bit,
the ReLU epilogue of core.linear_residual, every distinct block and the whole tower against a float64 CPU forward,
routing, and the driver: two extractions give the same bytes, at one rank and at two.

The bound used throughout, as in test_gpu_mbconv.py: normalised error max|got - ref| / max|ref| at most twice that of
ATen's fp32 result on the same inputs (measured in the same test) plus 1e-6; the factor 2 is the project's allowance for
a different summation order."""
import ctypes
import ctypes.util
import glob
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import util
from util import mild_bn as _mild_bn, nerr as _nerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
LAYERS = ["conv1", "layer1", "layer2", "layer3", "layer4"]


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _bound(e_hip, e_aten, what):
    print("%s: hip %.3e aten %.3e" % (what, e_hip, e_aten))
    assert e_hip <= 2 * e_aten + 1e-6, (what, e_hip, e_aten)


# ---- 1. K18 -----------------------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, k, stride): the seven 3x3 and three 1x1 / 2 shapes of ResNet-50 at 224 x 224 (B = 3: layer4's 147
# pixels span images inside one tile and do not fill two), then edge shapes
RESNET_SHAPES = [(3, 64, 64, 56, 56, 3, 1), (3, 128, 128, 56, 56, 3, 2), (3, 128, 128, 28, 28, 3, 1),
                 (3, 256, 256, 28, 28, 3, 2), (3, 256, 256, 14, 14, 3, 1), (3, 512, 512, 14, 14, 3, 2),
                 (3, 512, 512, 7, 7, 3, 1), (3, 256, 512, 56, 56, 1, 2), (3, 512, 1024, 28, 28, 1, 2),
                 (3, 1024, 2048, 14, 14, 1, 2)]
EDGE_SHAPES = [(2, 64, 64, 65, 47, 3, 1), (2, 64, 128, 65, 47, 3, 2), (2, 64, 128, 65, 47, 1, 2), (5, 32, 96, 7, 7, 3, 1),
               (5, 32, 96, 7, 7, 3, 2), (5, 96, 32, 7, 7, 1, 2), (1, 32, 32, 1, 1, 3, 1), (7, 128, 256, 3, 5, 3, 2)]


def _igemm_case(core, dev, shape, relu_in, relu_out, seed=0):
    B, Cin, Cout, H, W, k, s = shape
    g = torch.Generator().manual_seed(seed + Cin + H)
    x = torch.randn(B, H, W, Cin, generator=g)                       # negative values: relu_in matters
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g)
    w_tap = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    pad = 1 if k == 3 else 0

    def ref(xx, ww, bb):
        a = xx.permute(0, 3, 1, 2)
        a = F.relu(a) if relu_in else a
        y = F.conv2d(a, ww, bb, s, pad)
        return (F.relu(y) if relu_out else y).permute(0, 2, 3, 1)
    r64 = ref(x.double(), w.double(), bias.double())
    aten = ref(x.to(dev), w.to(dev), bias.to(dev))
    got = core.conv_igemm_nhwc(x.to(dev), w_tap.to(dev), bias.to(dev), k, s, relu_in=relu_in, relu_out=relu_out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(r64.shape) and got.is_contiguous()
    return _nerr(got, r64), _nerr(aten, r64)


@pytest.mark.parametrize("shape", RESNET_SHAPES)
def test_k18_resnet_shapes_against_float64(core, dev, shape):
    flags = (True, True) if shape[5] == 3 else (False, False)         # how the block calls it
    e_hip, e_aten = _igemm_case(core, dev, shape, *flags)
    _bound(e_hip, e_aten, "K18 %s relu %s" % (shape, flags))
    e_hip, e_aten = _igemm_case(core, dev, shape, not flags[0], not flags[1], seed=1)
    _bound(e_hip, e_aten, "K18 %s relu %s" % (shape, (not flags[0], not flags[1])))


@pytest.mark.parametrize("shape", EDGE_SHAPES)
@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("relu_out", [False, True])
def test_k18_edge_shapes_against_float64(core, dev, shape, relu_in, relu_out):
    e_hip, e_aten = _igemm_case(core, dev, shape, relu_in, relu_out)
    _bound(e_hip, e_aten, "K18 %s relu %s" % (shape, (relu_in, relu_out)))


def test_k18_exact_on_exact_data(core, dev):
    """Exact data (small dyadic rationals: every product and every partial sum is exactly representable in float32, in
    any order): the result equals the float64 convolution bit for bit, so any difference is an indexing error -- a wrong
    tap, channel, lane or register map -- and not rounding."""
    g = torch.Generator().manual_seed(3)
    B, H, W, Cin, Cout = 2, 5, 4, 32, 32
    x = torch.randint(-8, 9, (B, H, W, Cin), generator=g).float() / 4
    w = torch.randint(-8, 9, (Cout, Cin, 3, 3), generator=g).float() / 8
    bias = torch.randint(-8, 9, (Cout,), generator=g).float() / 2
    w_tap = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    got = core.conv_igemm_nhwc(x.to(dev), w_tap.to(dev), bias.to(dev), 3, 1).cpu()
    ref = (F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), 1, 1)).permute(0, 2, 3, 1)
    assert torch.equal(got.double(), ref)
    got = core.conv_igemm_nhwc(x.to(dev), w_tap.to(dev), bias.to(dev), 3, 2, relu_in=True).cpu()
    ref = (F.conv2d(F.relu(x.double().permute(0, 3, 1, 2)), w.double(), bias.double(), 2, 1)).permute(0, 2, 3, 1)
    assert torch.equal(got.double(), ref)


def test_k18_wrapper_rejects_bad_arguments(core, dev):
    x = torch.randn(2, 8, 8, 64, device=dev)
    w = torch.randn(64, 576, device=dev)
    b = torch.zeros(64, device=dev)
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w, b, 5, 1)
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w, b, 1, 1)
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w[:, :64].contiguous(), b, 3, 1)                     # K does not match
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x[..., :48].contiguous(), torch.randn(64, 432, device=dev), b, 3, 1)   # Cin % 32
    with pytest.raises(TypeError):
        core.conv_igemm_nhwc(x.double(), w, b, 3, 1)
    with pytest.raises(TypeError):
        core.conv_igemm_nhwc(x.permute(0, 2, 1, 3), w, b, 3, 1)                      # not contiguous
    with pytest.raises(TypeError):
        core.conv_igemm_nhwc(x, w, b[:32], 3, 1)
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w, torch.zeros(65, device=dev)[1:], 3, 1)            # a 4-byte aligned bias
    with pytest.raises(ValueError):
        core.conv7x7s2_nhwc(torch.randn(1, 3, 8, 8, device=dev), torch.randn(3, 7, 7, 62, device=dev))
    with pytest.raises(ValueError):
        core.conv7x7s2_nhwc(torch.randn(1, 3, 8, 8, device=dev), torch.randn(3, 3, 3, 64, device=dev))
    with pytest.raises(ValueError):
        core.bn_relu_maxpool_nhwc(torch.randn(1, 8, 8, 6, device=dev), torch.ones(6, device=dev), torch.zeros(6, device=dev))
    with pytest.raises(TypeError):
        core.bn_relu_maxpool_nhwc(torch.randn(1, 8, 8, 8, device=dev), torch.ones(4, device=dev), torch.zeros(8, device=dev))


# ---- 2. K16, K17 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 3, 64, 224, 224), (2, 3, 64, 160, 96), (3, 3, 64, 65, 47), (2, 1, 8, 7, 7),
                                            (2, 4, 36, 33, 18), (1, 3, 64, 1, 2)])
def test_k16_against_float64(core, dev, B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 7, 7, generator=g) / (49 * Cin) ** 0.5
    r64 = F.conv2d(x.double(), w.double(), None, 2, 3).permute(0, 2, 3, 1)
    aten = F.conv2d(x.to(dev), w.to(dev), None, 2, 3).permute(0, 2, 3, 1)
    got = core.conv7x7s2_nhwc(x.to(dev), w.permute(1, 2, 3, 0).contiguous().to(dev))
    assert tuple(got.shape) == tuple(r64.shape) and got.is_contiguous()
    _bound(_nerr(got, r64), _nerr(aten, r64), "K16 %s" % ((B, Cin, Cout, H, W),))


# (B, Cin, H, W, Cout): a tile edge crossed both ways, CO = 32; an image smaller than the window, CO = 4; one pixel and a
# width that is no multiple of 32; Cin = 4 and three tiles across
@pytest.mark.parametrize("shape", [(2, 3, 65, 47, 64), (2, 1, 7, 7, 8), (1, 3, 1, 1, 36), (1, 4, 33, 70, 32)])
def test_k16_exact_on_integer_data(core, dev, shape):
    """Small integers in x and w: every product and partial sum is exact in fp32 in any order (at most 4 * 49 * 64), so
    the result equals the float64 one bit for bit, and any difference is an indexing or padding error."""
    B, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(7 + H)
    x = torch.randint(-8, 9, (B, Cin, H, W), generator=g).float()
    w = torch.randint(-8, 9, (Cout, Cin, 7, 7), generator=g).float()
    ref = F.conv2d(x.double(), w.double(), None, 2, 3).permute(0, 2, 3, 1)
    got = core.conv7x7s2_nhwc(x.to(dev), w.permute(1, 2, 3, 0).contiguous().to(dev)).cpu()
    assert torch.equal(got.double(), ref)


def _stem_in_documented_order(x, w, bias, relu):
    """The stem convolution (k x k / 2, pad k // 2) of x [B, Cin, H, W] with w [Cout, Cin, k, k] on the host, in the order
    the stem kernel documents: per output element one libm fmaf chain from 0.0 in ascending (channel, row, column), a
    padded tap entering as fmaf(w, 0, acc); then + bias, then the ReLU, where the kernel has them.  NHWC fp32."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    fmaf = libm.fmaf
    fmaf.restype, fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    (B, Cin, H, W), Cout, k = x.shape, w.shape[0], w.shape[2]
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    xp, wl = F.pad(x, (pad,) * 4).tolist(), w.tolist()
    out = torch.empty(B, Ho, Wo, Cout)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for co in range(Cout):
                    acc = 0.0
                    for ci in range(Cin):
                        for dy in range(k):
                            row, wrow = xp[b][ci][2 * oy + dy], wl[co][ci][dy]
                            for dx in range(k):
                                acc = fmaf(wrow[dx], row[2 * ox + dx], acc)
                    out[b, oy, ox, co] = acc
    if bias is not None:
        out = out + bias                                             # one fp32 addition per element
    return F.relu(out) if relu else out


# tiny shapes, (B, Cin, H, W, Cout): the 4-channel pass and the 32-channel pass
@pytest.mark.parametrize("shape", [(2, 3, 9, 11, 8), (1, 2, 5, 7, 32)])
@pytest.mark.parametrize("kernel", ["K16", "K19"])
def test_stem_kernels_keep_their_summation_order(core, dev, kernel, shape):
    """Random float data: the bits depend on the order of the sum, and they must be those of the documented order."""
    B, Cin, H, W, Cout = shape
    k = 7 if kernel == "K16" else 3
    g = torch.Generator().manual_seed(k + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g)
    w_tap = w.permute(1, 2, 3, 0).contiguous().to(dev)
    if kernel == "K16":
        assert torch.equal(core.conv7x7s2_nhwc(x.to(dev), w_tap).cpu(), _stem_in_documented_order(x, w, None, False))
        return
    bias = torch.randn(Cout, generator=g)
    for relu in (False, True):
        got = core.conv3x3s2_nhwc(x.to(dev), w_tap, bias.to(dev), relu=relu).cpu()
        assert torch.equal(got, _stem_in_documented_order(x, w, bias, relu)), relu


def test_k16_refuses_overlap(mcd, core, dev):
    """y aliased onto x: MCD_E_ARG, and nothing is launched (x keeps its bits).  The output, 8 * 8 * 4 floats, is
    smaller than x: the call stays inside the tensor whatever the entry does."""
    x = torch.randn(1, 3, 16, 16, device=dev)
    w = torch.randn(3, 7, 7, 4, device=dev)
    before = x.clone()
    L = mcd._lib.load()
    with pytest.raises(mcd._lib.McdError, match="overlaps") as e:
        mcd._lib.check(L.mcd_conv7x7s2_nhwc(x.data_ptr(), 1, 3, 16, 16, w.data_ptr(), 4, x.data_ptr(), core._stream()))
    assert e.value.code == mcd._lib.MCD_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(x, before)


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 112, 112), (2, 64, 80, 48), (3, 64, 33, 24), (2, 8, 7, 7), (2, 4, 1, 1),
                                     (2, 12, 2, 5)])
def test_k17_against_float64_and_bit_equal_to_torch(core, dev, B, C, H, W):
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B, H, W, C, generator=g)
    scale = torch.randn(C, generator=g)
    shift = torch.randn(C, generator=g)

    def ref(xx, sc, sh):
        return F.max_pool2d(F.relu(xx.permute(0, 3, 1, 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), 3, 2, 1) \
            .permute(0, 2, 3, 1)
    r64 = ref(x.double(), scale.double(), shift.double())
    aten = ref(x.to(dev), scale.to(dev), shift.to(dev))
    got = core.bn_relu_maxpool_nhwc(x.to(dev), scale.to(dev), shift.to(dev))
    assert tuple(got.shape) == tuple(r64.shape) and got.is_contiguous()
    _bound(_nerr(got, r64), _nerr(aten, r64), "K17 %s" % ((B, C, H, W),))
    # scale 1, shift 0: the same bits as max_pool2d(relu(x))
    xg = x.to(dev)
    one = core.bn_relu_maxpool_nhwc(xg, torch.ones(C, device=dev), torch.zeros(C, device=dev))
    want = F.max_pool2d(F.relu(xg.permute(0, 3, 1, 2)), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(one, want)


# ---- 3. batch invariance ----------------------------------------------------------------------------------------------
def _alone_vs_batch(run, make, dev):
    """run(batch tensor) -> output with the batch in dim 0; the image alone and at positions 0, 3, 6 of a batch of 7."""
    g = torch.Generator().manual_seed(17)
    img = make(1, g)
    alone = run(img.to(dev))
    for pos in (0, 3, 6):
        batch = make(7, g)
        batch[pos] = img[0]
        out = run(batch.to(dev))
        assert torch.equal(out[pos], alone[0]), pos


def test_batch_invariance_bit_exact(core, dev):
    g = torch.Generator().manual_seed(1)
    w7 = (torch.randn(3, 7, 7, 64, generator=g) / 12).to(dev)
    _alone_vs_batch(lambda x: core.conv7x7s2_nhwc(x, w7), lambda b, gg: torch.randn(b, 3, 96, 80, generator=gg), dev)
    sc, sh = torch.randn(64, generator=g).to(dev), torch.randn(64, generator=g).to(dev)
    _alone_vs_batch(lambda x: core.bn_relu_maxpool_nhwc(x, sc, sh), lambda b, gg: torch.randn(b, 47, 33, 64, generator=gg), dev)
    # every K18 instantiation (3x3 / 1, 3x3 / 2, 1x1 / 2; the 64- and the 128-channel tile), layer4's size included: 49
    # pixels per image, so the 128-pixel tiles span images and the image sits at a different place in its tile each time
    for Cin, Cout, H, W, k, s in [(64, 64, 14, 14, 3, 1), (128, 128, 14, 14, 3, 2), (128, 256, 14, 14, 1, 2),
                                  (64, 64, 9, 9, 1, 2), (512, 512, 7, 7, 3, 1), (512, 512, 14, 14, 3, 2),
                                  (1024, 2048, 14, 14, 1, 2), (64, 96, 7, 7, 3, 1)]:
        w = (torch.randn(Cout, k * k * Cin, generator=g) / (k * k * Cin) ** 0.5).to(dev)
        b = torch.randn(Cout, generator=g).to(dev)
        _alone_vs_batch(lambda x: core.conv_igemm_nhwc(x, w, b, k, s, relu_in=True, relu_out=True),
                        lambda n, gg: torch.randn(n, H, W, Cin, generator=gg), dev)


# ---- 4. the ReLU epilogue of linear_residual --------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(2 * 49, 2048, 512), (3 * 196, 1024, 256), (37, 256, 64)])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_linear_residual_relu_against_float64(core, dev, M, N, K, with_res, with_bias):
    g = torch.Generator().manual_seed(M + N + int(with_res) * 2 + int(with_bias))
    h = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g) if with_bias else None
    res = (torch.randn(M, N, generator=g) * 2 - 1) if with_res else None         # makes many sums negative
    ref = h.double() @ w.double().t()
    if with_bias:
        ref = ref + bias.double()
    if with_res:
        ref = ref + res.double()
    assert (ref < 0).float().mean() > 0.2                                           # the ReLU has work to do
    plain64 = ref
    ref = F.relu(ref)
    dv = lambda t: None if t is None else t.to(dev)                                # noqa: E731
    got = core.linear_residual(dv(res), dv(h), dv(w), dv(bias), relu=True)
    aten = F.linear(dv(h), dv(w), dv(bias))
    aten = F.relu(aten + dv(res) if with_res else aten)
    assert (got >= 0).all()
    _bound(_nerr(got, ref), _nerr(aten, ref), "linear_residual relu %s" % ((M, N, K, with_res, with_bias),))
    # the ReLU is applied to the whole sum (residual included): exactly zero wherever float64 is clearly negative
    assert (got.cpu()[plain64 < -1e-4] == 0).all()
    # relu=False is untouched: its own plan, and the ReLU of it is the ReLU entry's result up to the algorithm's order
    plain = core.linear_residual(dv(res), dv(h), dv(w), dv(bias))
    assert (plain < 0).any()
    again = core.linear_residual(dv(res), dv(h), dv(w), dv(bias))
    assert torch.equal(plain, again)
    assert _nerr(plain, plain64) <= 2 * _nerr(F.linear(dv(h), dv(w), dv(bias)) + (dv(res) if with_res else 0), plain64) + 1e-6
    picks = {p[:4]: p[4] for p in core.encoder_gemm_picks()}
    flag = 1 if with_res else 0
    assert (M, N, K, flag) in picks and (M, N, K, flag | 2) in picks               # kept apart


def test_linear_residual_plain_bits_do_not_depend_on_the_relu_entry(core, dev, monkeypatch):
    """relu=False with a given pick gives the bits it gave before the ReLU entry existed in the process: forcing the
    same pick for both entries, the plain result is the same before and after the ReLU entry has planned the shape."""
    g = torch.Generator().manual_seed(9)
    M, N, K = 91, 512, 128
    h, w = torch.randn(M, K, generator=g).to(dev), torch.randn(N, K, generator=g).to(dev)
    b, r = torch.randn(N, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    core.set_encoder_gemm_picks([(M, N, K, 1, 0), (M, N, K, 3, 0)])
    try:
        before = core.linear_residual(r, h, w, b)
        relu = core.linear_residual(r, h, w, b, relu=True)
        after = core.linear_residual(r, h, w, b)
        assert torch.equal(before, after)
        assert _nerr(relu, F.relu(before)) < 1e-5       # (the heuristic's list may differ between the two epilogues)
        picks = {p[:4]: p[4] for p in core.encoder_gemm_picks()}
        assert picks[(M, N, K, 1)] == 0 and picks[(M, N, K, 3)] == 0
    finally:
        core.set_encoder_gemm_picks([(M, N, K, 1, -1), (M, N, K, 3, -1)])


# ---- 5. blocks and the tower ------------------------------------------------------------------------------------------
NEW_WRAPPERS = ("conv7x7s2_nhwc", "bn_relu_maxpool_nhwc", "conv_igemm_nhwc")


@pytest.mark.parametrize("size", [(224, 224), (160, 96)])
def test_blocks_against_float64(du, core, dev, monkeypatch, size):
    torch.manual_seed(0)
    net = du.ResNet50()
    _mild_bn(net, 1)
    net.eval()
    blocks = [(li, bi, getattr(net, "layer%d" % li)[bi]) for li in (1, 2, 3, 4) for bi in (0, 1)]
    sizes = {}
    hs = [b.register_forward_pre_hook(lambda m, i, k=(li, bi): sizes.__setitem__(k, tuple(i[0].shape[1:])))
          for li, bi, b in blocks]
    with torch.no_grad():
        net(torch.zeros(1, 3, *size))
    for h in hs:
        h.remove()
    cnt = util.CallCounter(core, monkeypatch, NEW_WRAPPERS)
    for li, bi, blk in blocks:
        C, H, W = sizes[(li, bi)]
        g = torch.Generator().manual_seed(10 * li + bi)
        x = torch.randn(2, C, H, W, generator=g)
        with torch.no_grad():
            ref = blk.double().cpu()(x.double())
            blk.float().to(dev)
            xg = x.to(dev).contiguous(memory_format=torch.channels_last)
            x0 = xg.clone()
            before = cnt.n.get("conv_igemm_nhwc", 0), cnt.relu_gemms
            got = blk(xg)
            want = 2 if (blk.downsample is not None and blk.stride == 2) else 1
            assert (cnt.n["conv_igemm_nhwc"], cnt.relu_gemms) == (before[0] + want, before[1] + 1), (li, bi)
            assert torch.equal(xg, x0)                                # the block's input is left alone
            monkeypatch.setattr(du, "HIP_RESNET", False)
            aten = blk(x.to(dev))
            monkeypatch.setattr(du, "HIP_RESNET", True)
        assert tuple(got.shape) == tuple(ref.shape) and got.is_contiguous(memory_format=torch.channels_last)
        assert (got >= 0).all()
        _bound(_nerr(got, ref), _nerr(aten, ref), "block layer%d[%d] at %s" % (li, bi, size))


def _hooked(model, xin):
    outs = {}
    hs = [getattr(model, n).register_forward_hook(lambda m, i, o, n=n: outs.__setitem__(n, o.detach().double().cpu()))
          for n in LAYERS]
    with torch.no_grad():
        y = model(xin)
    for h in hs:
        h.remove()
    return y, outs


@pytest.mark.parametrize("size", [(224, 224), (160, 96)])
def test_tower_against_float64_and_routing(du, core, dev, monkeypatch, size):
    torch.manual_seed(0)
    net = du.ResNet50()
    _mild_bn(net, 2)
    net.eval()
    keys = list(net.state_dict().keys())
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, *size, generator=g)
    ref, ref_outs = _hooked(net.double(), x.double())
    net.float().to(dev)
    cnt = util.CallCounter(core, monkeypatch, NEW_WRAPPERS)
    monkeypatch.setattr(du, "HIP_RESNET", False)
    aten, aten_outs = _hooked(net, x.to(dev))
    assert cnt.n == {} and cnt.relu_gemms == 0                        # the flag off: no new kernel is called
    monkeypatch.setattr(du, "HIP_RESNET", True)
    xg = x.to(dev)
    got, got_outs = _hooked(net, xg)
    # all 16 blocks and the stem: one K16, one K17, 16 3x3 + 3 strided 1x1 on K18, 16 GEMMs with the ReLU epilogue
    assert cnt.n == {"conv7x7s2_nhwc": 1, "bn_relu_maxpool_nhwc": 1, "conv_igemm_nhwc": 19} and cnt.relu_gemms == 16
    assert torch.equal(xg, x.to(dev))
    assert list(net.state_dict().keys()) == keys
    for n in LAYERS:
        assert got_outs[n].shape == ref_outs[n].shape and got_outs[n].dim() == 4
        assert float(ref_outs[n].abs().max()) > 1e-3                  # neither vanished nor exploded
        _bound(_nerr(got_outs[n], ref_outs[n]), _nerr(aten_outs[n], ref_outs[n]), "tower %s at %s" % (n, size))
    _bound(_nerr(got, ref), _nerr(aten, ref), "tower logits at %s" % (size,))
    # a hook on layer3[2].conv2: that one block takes ATen, the hook fires, the outputs still agree within the bound
    seen = []
    h = net.layer3[2].conv2.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    cnt.n.clear()
    cnt.relu_gemms = 0
    y2, outs2 = _hooked(net, xg)
    h.remove()
    assert len(seen) == 1
    assert cnt.n == {"conv7x7s2_nhwc": 1, "bn_relu_maxpool_nhwc": 1, "conv_igemm_nhwc": 18} and cnt.relu_gemms == 15
    for n in LAYERS:
        _bound(_nerr(outs2[n], ref_outs[n]), _nerr(aten_outs[n], ref_outs[n]), "tower %s, one block on ATen" % n)
        assert _nerr(outs2[n], got_outs[n]) < 1e-4
    _bound(_nerr(y2, ref), _nerr(aten, ref), "tower logits, one block on ATen")
    # the same forward twice: the same bits
    y3, outs3 = _hooked(net, xg)
    assert torch.equal(y3, got) and all(torch.equal(outs3[n], got_outs[n]) for n in LAYERS)


# ---- 7. reproducibility of the extraction ---------------------------------------------------------------------------
def _run_driver(dev, tmp, tag, layers=LAYERS, n=256, batch=64):
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons as drv
    act, res = os.path.join(tmp, "acts_" + tag), os.path.join(tmp, "results_" + tag)
    out = drv.main(["--target_model", "resnet50", "--target_layers", ",".join(layers), "--d_probe",
                    "synthetic_%d_224" % n, "--concept_set", CONCEPTS, "--batch_size", str(batch), "--device", str(dev),
                    "--activation_dir", act, "--result_dir", res])
    return act, open(glob.glob(os.path.join(out, "*.csv"))[0], "rb").read()


def _layer_files(act):
    files = sorted(glob.glob(os.path.join(act, "**", "*.pt"), recursive=True))
    return {os.path.basename(f): f for f in files if "resnet50" in os.path.basename(f)}


def test_two_extractions_give_the_same_bytes(du, core, dev, tmp_path, monkeypatch):
    """describe_clip_neurons on conv1 + layer1..4 of the ResNet-50 target, twice, into two activation directories: the
    cached activation tensors and the CSV are byte-identical (on the ATen route they need not be: MIOpen's deepest
    convolutions).  The hipBLASLt pick is the heuristic's, so that the GEMM algorithm is not a timed choice.
    Then the same probe set at batch 32: conv1's pooled activations (K16 + K0n only) are bit-identical to batch 64's.
    For the deeper layers batch-size independence holds only where hipBLASLt's pick is the same for both GEMM heights,
    which this test does not assert."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    cnt = util.CallCounter(core, monkeypatch, NEW_WRAPPERS)
    act1, csv1 = _run_driver(dev, str(tmp_path), "one")
    assert cnt.n.get("conv_igemm_nhwc", 0) >= 19 * 4 and cnt.n.get("conv7x7s2_nhwc", 0) >= 4
    act2, csv2 = _run_driver(dev, str(tmp_path), "two")
    f1, f2 = _layer_files(act1), _layer_files(act2)
    assert sorted(f1) == sorted(f2) and len(f1) == 5
    for name in f1:
        a, b = torch.load(f1[name], weights_only=True), torch.load(f2[name], weights_only=True)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert csv1 == csv2 and len(csv1) > 10000
    act3, _ = _run_driver(dev, str(tmp_path), "b32", layers=["conv1"], batch=32)
    f3 = _layer_files(act3)
    (name,) = [k for k in f3 if "conv1" in k]
    assert torch.equal(torch.load(f3[name], weights_only=True), torch.load(f1[name], weights_only=True))


# ---- 8. one rank against two ------------------------------------------------------------------------------------------
def _rank_driver(world, rank, tmp, n_images, batch):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd import pipeline
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons
    if world > 1:   # one GPU holds every rank: the RCCL transport cannot, the host-staged rehearsal of it can
        staged = util.host_staged_gather()
        pipeline.rccl_all_gather_rows = lambda t, group=None: staged(t)
    out = describe_clip_neurons.main(
        ["--target_model", "resnet50", "--target_layers", ",".join(LAYERS), "--d_probe", "synthetic_%d_224" % n_images,
         "--concept_set", CONCEPTS, "--batch_size", str(batch), "--device", "cuda:0", "--activation_dir",
         os.path.join(tmp, "acts%d_%d" % (world, rank)), "--result_dir", os.path.join(tmp, "res%d" % world)])
    torch.cuda.synchronize()
    return out


def test_driver_csv_bytes_one_vs_two_ranks(mcd, dev, tmp_path, monkeypatch):
    """The whole ResNet-50 job through the HIP route at 1 rank and at 2 ranks (spawned processes on one GPU, gloo, equal
    batch shapes, the heuristic hipBLASLt pick): rank 0's CSV is the same bytes -- an image's activations do not depend
    on which rank or batch encodes it."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    monkeypatch.setenv("MCD_SHARD_ALIGN", "40")
    tmp = str(tmp_path)
    csv = {}
    for world in (1, 2):        # fresh processes: this one may keep timed GEMM picks for these shapes from other tests
        got = util.run_ranks(world, _rank_driver, (tmp, 160, 40), timeout=900, env=util.TORCHRUN_ENV)
        csv[world] = open(glob.glob(os.path.join(got[0], "*.csv"))[0], "rb").read()
    assert csv[1] == csv[2] and len(csv[1]) > 10000
