"""GPU: the ResNet-18 / -34 / -101 / -152 targets and K18's residual epilogue (mcd_conv_igemm_res_nhwc) -- the kernel
against float64 and ATen's own fp32 error, exact data, res=None against the plain entry bit for bit, batch invariance bit
for bit, every distinct _BasicBlock and the towers against a float64 CPU forward, routing and call counts, and the
drivers: a BasicBlock network's cached activations are the same bytes at batch 64 and batch 32 and at one rank and two,
because no library GEMM sits between the image and a hooked output.

The bound is the project's (test_gpu_resnet.py): normalised error max|got - ref| / max|ref| at most twice that of ATen's
fp32 result on the same inputs (measured in the same test) plus 1e-6."""
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
NEW_WRAPPERS = ("conv7x7s2_nhwc", "bn_relu_maxpool_nhwc", "conv_igemm_nhwc")


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _bound(e_hip, e_aten, what):
    print("%s: hip %.3e aten %.3e ratio to the bound %.3f" % (what, e_hip, e_aten, e_hip / (2 * e_aten + 1e-6)))
    assert e_hip <= 2 * e_aten + 1e-6, (what, e_hip, e_aten)


# ---- 1. K18 with a residual ---------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, k, stride, res): the distinct convolutions of the BasicBlock networks at 224 x 224, called the way
# the block calls them (conv2 with the skip and the ReLU, conv1 / 2 with the ReLU, the downsample bare)
NETWORK_SHAPES = [(3, 64, 64, 56, 56, 3, 1, True), (3, 128, 128, 28, 28, 3, 1, True), (3, 256, 256, 14, 14, 3, 1, True),
                  (3, 512, 512, 7, 7, 3, 1, True), (3, 64, 128, 56, 56, 3, 2, False), (3, 128, 256, 28, 28, 3, 2, False),
                  (3, 256, 512, 14, 14, 3, 2, False), (3, 64, 128, 56, 56, 1, 2, False), (3, 128, 256, 28, 28, 1, 2, False),
                  (3, 256, 512, 14, 14, 1, 2, False)]
# a partial pixel tile, a partial 64-channel tile (Cout = 96), tiles that span images, a single pixel
EDGE_SHAPES = [(2, 64, 64, 65, 47, 3, 1), (5, 32, 96, 7, 7, 3, 1), (5, 32, 96, 7, 7, 3, 2), (5, 96, 32, 7, 7, 1, 2),
               (1, 32, 32, 1, 1, 3, 1), (7, 128, 256, 3, 5, 3, 2)]


def _inputs(shape, seed=0):
    B, Cin, Cout, H, W, k, s = shape
    g = torch.Generator().manual_seed(seed + Cin + H)
    x = torch.randn(B, H, W, Cin, generator=g)                       # negative values: relu_in matters
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g)
    pad = 1 if k == 3 else 0
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    # conv + bias is about N(0, 2) around 0: a residual of the same kind keeps about half of the sums negative
    res = torch.randn(B, Ho, Wo, Cout, generator=g) * 1.5
    return x, w, bias, res, w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()


def _res_case(core, dev, shape, relu_in, relu_out, with_res, seed=0):
    k, s = shape[5], shape[6]
    x, w, bias, res, w_tap = _inputs(shape, seed)
    pad = 1 if k == 3 else 0

    def ref(xx, ww, bb, rr, act=True):
        a = xx.permute(0, 3, 1, 2)
        a = F.relu(a) if relu_in else a
        y = F.conv2d(a, ww, bb, s, pad)
        if with_res:
            y = y + rr.permute(0, 3, 1, 2)
        return (F.relu(y) if relu_out and act else y).permute(0, 2, 3, 1)
    plain64 = ref(x.double(), w.double(), bias.double(), res.double(), act=False)
    r64 = F.relu(plain64) if relu_out else plain64
    if with_res:
        neg = float((plain64 < 0).double().mean())
        assert 0.3 < neg < 0.7, neg                                   # the ReLU behind the add has work to do
    aten = ref(x.to(dev), w.to(dev), bias.to(dev), res.to(dev))
    rg = res.to(dev) if with_res else None
    r0 = None if rg is None else rg.clone()
    got = core.conv_igemm_nhwc(x.to(dev), w_tap.to(dev), bias.to(dev), k, s, relu_in=relu_in, relu_out=relu_out, res=rg)
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(r64.shape) and got.is_contiguous()
    assert rg is None or torch.equal(rg, r0)                          # the residual is read only
    if relu_out:
        assert (got >= 0).all()
        assert (got.cpu()[plain64 < -1e-4] == 0).all()               # the ReLU acts on the whole sum
    return _nerr(got, r64), _nerr(aten, r64)


@pytest.mark.parametrize("shape", NETWORK_SHAPES)
def test_k18_res_network_shapes_against_float64(core, dev, shape):
    *conv, with_res = shape
    relu_out = conv[5] == 3
    e_hip, e_aten = _res_case(core, dev, tuple(conv), False, relu_out, with_res)
    _bound(e_hip, e_aten, "K18+res %s relu_out %s" % (shape, relu_out))


@pytest.mark.parametrize("shape", EDGE_SHAPES)
@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("relu_out", [False, True])
def test_k18_res_edge_shapes_against_float64(core, dev, shape, relu_in, relu_out):
    e_hip, e_aten = _res_case(core, dev, shape, relu_in, relu_out, True)
    _bound(e_hip, e_aten, "K18+res edge %s relu %s" % (shape, (relu_in, relu_out)))


# ---- 2. exact data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_k18_res_exact_on_exact_data(core, dev, stride):
    """Small dyadic rationals in x, w, bias and res: every product and every partial sum is exactly representable in
    float32 in any order, so the result equals the float64 one bit for bit and any difference is an indexing error in
    the residual's lane / register map, not rounding."""
    g = torch.Generator().manual_seed(3 + stride)
    B, H, W, Cin, Cout = 2, 5, 4, 32, 32
    x = torch.randint(-8, 9, (B, H, W, Cin), generator=g).float() / 4
    w = torch.randint(-8, 9, (Cout, Cin, 3, 3), generator=g).float() / 8
    bias = torch.randint(-8, 9, (Cout,), generator=g).float() / 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randint(-64, 65, (B, Ho, Wo, Cout), generator=g).float() / 2      # every element its own value
    w_tap = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    got = core.conv_igemm_nhwc(x.to(dev), w_tap.to(dev), bias.to(dev), 3, stride, relu_out=True, res=res.to(dev)).cpu()
    ref = F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride, 1).permute(0, 2, 3, 1)
                 + res.double())
    assert (ref == 0).any() and (ref > 0).any()
    assert torch.equal(got.double(), ref)


# ---- 3. res=None is the plain kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_res_none_is_the_plain_entry_bit_for_bit(mcd, core, dev, shape):
    B, Cin, Cout, H, W, k, s = shape
    x, _, bias, res, w_tap = _inputs(shape, 5)
    x, bias, w_tap = x.to(dev), bias.to(dev), w_tap.to(dev)
    L = mcd._lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for relu_in, relu_out in ((False, False), (True, True)):
        got = core.conv_igemm_nhwc(x, w_tap, bias, k, s, relu_in=relu_in, relu_out=relu_out, res=None)
        plain, null = torch.full_like(got, float("nan")), torch.full_like(got, float("nan"))
        assert L.mcd_conv_igemm_nhwc(x.data_ptr(), B, H, W, Cin, w_tap.data_ptr(), bias.data_ptr(), Cout, k, s,
                                     int(relu_in), int(relu_out), plain.data_ptr(), stream) == 0
        assert L.mcd_conv_igemm_res_nhwc(x.data_ptr(), B, H, W, Cin, w_tap.data_ptr(), bias.data_ptr(), None, Cout, k, s,
                                         int(relu_in), int(relu_out), null.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(plain).any()
        assert torch.equal(got, plain) and torch.equal(null, plain)
        # a residual of zeros adds +0 to every element: the same values
        zero = core.conv_igemm_nhwc(x, w_tap, bias, k, s, relu_in=relu_in, relu_out=relu_out, res=torch.zeros_like(got))
        assert bool((zero == plain).all())


# ---- 4. batch invariance ------------------------------------------------------------------------------------------------
def _alone_vs_batch(run, make, dev):
    """run(batch tensors) -> output with the batch in dim 0; the image alone and at positions 0, 3, 6 of a batch of 7."""
    g = torch.Generator().manual_seed(17)
    img = make(1, g)
    alone = run(*[t.to(dev) for t in img])
    for pos in (0, 3, 6):
        batch = make(7, g)
        for t, one in zip(batch, img):
            t[pos] = one[0]
        out = run(*[t.to(dev) for t in batch])
        assert torch.equal(out[pos], alone[0]), pos


def test_batch_invariance_bit_exact(du, core, dev):
    g = torch.Generator().manual_seed(1)
    # the 64- and the 128-channel tile and a partial one; 49 pixels per image at 7 x 7: the 128-pixel tiles span images
    for Cin, Cout, H, W, k, s in [(64, 64, 14, 14, 3, 1), (512, 512, 7, 7, 3, 1), (64, 96, 7, 7, 3, 1)]:
        w = (torch.randn(Cout, k * k * Cin, generator=g) / (k * k * Cin) ** 0.5).to(dev)
        b = torch.randn(Cout, generator=g).to(dev)
        _alone_vs_batch(lambda x, r: core.conv_igemm_nhwc(x, w, b, k, s, relu_out=True, res=r),
                        lambda n, gg: (torch.randn(n, H, W, Cin, generator=gg), torch.randn(n, H, W, Cout, generator=gg)),
                        dev)
    for cin, width, stride in ((64, 64, 1), (64, 128, 2)):
        torch.manual_seed(cin + stride)
        blk = du._BasicBlock(cin, width, stride)
        _mild_bn(blk, 4)
        blk.eval().to(dev)

        def run(x):
            with torch.no_grad():
                assert du.resnet_route(blk, x.contiguous(memory_format=torch.channels_last)) == "hip"
                return blk(x.contiguous(memory_format=torch.channels_last))
        _alone_vs_batch(run, lambda n, gg: (torch.randn(n, cin, 14, 10, generator=gg),), dev)


# ---- 5. the wrapper's checks of res -------------------------------------------------------------------------------------
def test_wrapper_rejects_a_bad_res(core, dev):
    x = torch.randn(2, 8, 8, 64, device=dev)
    w = torch.randn(64, 576, device=dev)
    b = torch.zeros(64, device=dev)
    good = torch.randn(2, 8, 8, 64, device=dev)
    assert core.conv_igemm_nhwc(x, w, b, 3, 1, res=good).shape == good.shape
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=good[:1].contiguous())                # the shape
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w, b, 3, 2, res=good)                                 # the input's, not the output's
    with pytest.raises(TypeError):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=good.double())
    with pytest.raises(TypeError):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=good.permute(0, 2, 1, 3))             # not contiguous
    with pytest.raises(TypeError):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=good.flatten())                       # not 4-D
    with pytest.raises(ValueError):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=torch.zeros(good.numel() + 1, device=dev)[1:].view_as(good))   # 4-byte aligned
    with pytest.raises(TypeError, match="GPU only"):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=good.cpu())
    with pytest.raises(ValueError, match="share memory"):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=good, out=good)                       # aliasing the output
    big = torch.zeros(3, 8, 8, 64, device=dev)
    with pytest.raises(ValueError, match="share memory"):
        core.conv_igemm_nhwc(x, w, b, 3, 1, res=big[:2], out=big[1:])                 # overlapping it
    out = torch.empty_like(good)
    assert core.conv_igemm_nhwc(x, w, b, 3, 1, res=good, out=out) is out
    assert torch.equal(out, core.conv_igemm_nhwc(x, w, b, 3, 1, res=good))


# ---- 6. blocks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(224, 224), (160, 96)])
def test_basic_blocks_against_float64(du, core, dev, monkeypatch, size):
    torch.manual_seed(0)
    net = du.ResNet(du._BasicBlock, [2, 2, 2, 2])
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
            want = 3 if blk.stride == 2 else 2
            assert (blk.downsample is not None) == (blk.stride == 2)
            assert (cnt.n["conv_igemm_nhwc"], cnt.relu_gemms) == (before[0] + want, before[1]), (li, bi)
            assert torch.equal(xg, x0)                                # the block's input is left alone
            monkeypatch.setattr(du, "HIP_RESNET", False)
            aten = blk(x.to(dev))
            monkeypatch.setattr(du, "HIP_RESNET", True)
        assert tuple(got.shape) == tuple(ref.shape) and got.is_contiguous(memory_format=torch.channels_last)
        assert (got >= 0).all() and (got == 0).any()
        _bound(_nerr(got, ref), _nerr(aten, ref), "basic block layer%d[%d] at %s" % (li, bi, size))
    assert cnt.n == {"conv_igemm_nhwc": 5 * 2 + 3 * 3} and cnt.relu_gemms == 0


# ---- 7. towers ----------------------------------------------------------------------------------------------------------
def _hooked(model, xin):
    outs = {}
    hs = [getattr(model, n).register_forward_hook(lambda m, i, o, n=n: outs.__setitem__(n, o.detach().double().cpu()))
          for n in LAYERS]
    with torch.no_grad():
        y = model(xin)
    for h in hs:
        h.remove()
    return y, outs


# network -> (K18 calls, GEMMs with the ReLU epilogue) of one forward on the HIP route
COUNTS = {"resnet18": (19, 0), "resnet34": (35, 0), "resnet101": (36, 33), "resnet152": (53, 50)}


def _counts(k18, relu_gemms):
    return {"conv7x7s2_nhwc": 1, "bn_relu_maxpool_nhwc": 1, "conv_igemm_nhwc": k18}, relu_gemms


@pytest.mark.parametrize("name,size", [("resnet18", (224, 224)), ("resnet18", (160, 96)), ("resnet34", (224, 224)),
                                       ("resnet34", (160, 96)), ("resnet101", (160, 96))])
def test_towers_against_float64_and_routing(du, core, dev, monkeypatch, name, size):
    net, _ = du.get_target_model(name, "cpu")
    _mild_bn(net, 2)
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
    assert (cnt.n, cnt.relu_gemms) == _counts(*COUNTS[name])
    assert torch.equal(xg, x.to(dev))
    assert list(net.state_dict().keys()) == keys
    for n in LAYERS:
        assert got_outs[n].shape == ref_outs[n].shape and got_outs[n].dim() == 4
        assert float(ref_outs[n].abs().max()) > 1e-3                  # neither vanished nor exploded
        _bound(_nerr(got_outs[n], ref_outs[n]), _nerr(aten_outs[n], ref_outs[n]), "%s %s at %s" % (name, n, size))
    _bound(_nerr(got, ref), _nerr(aten, ref), "%s logits at %s" % (name, size))
    # the same forward twice: the same bits
    y3, outs3 = _hooked(net, xg)
    assert torch.equal(y3, got) and all(torch.equal(outs3[n], got_outs[n]) for n in LAYERS)
    if name != "resnet18":
        return
    # a hook on layer3[1].conv2: that one block takes ATen (two K18 calls fewer), the hook fires once, the outputs agree
    seen = []
    h = net.layer3[1].conv2.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    cnt.n.clear()
    y2, outs2 = _hooked(net, xg)
    h.remove()
    assert len(seen) == 1
    assert (cnt.n, cnt.relu_gemms) == _counts(17, 0)
    for n in LAYERS:
        _bound(_nerr(outs2[n], ref_outs[n]), _nerr(aten_outs[n], ref_outs[n]), "%s %s, one block on ATen" % (name, n))
        assert _nerr(outs2[n], got_outs[n]) < 1e-4
    _bound(_nerr(y2, ref), _nerr(aten, ref), "%s logits, one block on ATen" % name)


def test_resnet152_call_counts(du, core, dev, monkeypatch):
    net, _ = du.get_target_model("resnet152", dev)
    _mild_bn(net, 2)
    cnt = util.CallCounter(core, monkeypatch, NEW_WRAPPERS)
    with torch.no_grad():
        y = net(torch.randn(2, 3, 160, 96, generator=torch.Generator().manual_seed(5)).to(dev))
    assert tuple(y.shape) == (2, 1000) and bool(torch.isfinite(y).all())
    assert (cnt.n, cnt.relu_gemms) == _counts(*COUNTS["resnet152"])


# ---- 8. reproducible extraction -----------------------------------------------------------------------------------------
def _run_driver(dev, tmp, tag, batch=64):
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons as drv
    act, res = os.path.join(tmp, "acts_" + tag), os.path.join(tmp, "results_" + tag)
    out = drv.main(["--target_model", "resnet18", "--target_layers", ",".join(LAYERS), "--d_probe", "synthetic_256_224",
                    "--concept_set", CONCEPTS, "--batch_size", str(batch), "--device", str(dev),
                    "--activation_dir", act, "--result_dir", res])
    return act, open(glob.glob(os.path.join(out, "*.csv"))[0], "rb").read()


def _layer_files(act):
    files = sorted(glob.glob(os.path.join(act, "**", "*.pt"), recursive=True))
    return {os.path.basename(f): f for f in files if "resnet18" in os.path.basename(f)}


def test_extraction_bytes_do_not_depend_on_the_batch_size(du, core, dev, tmp_path, monkeypatch):
    """describe_clip_neurons on conv1 + layer1..4 of the ResNet-18 target.  Twice at batch 64: the cached activation
    tensors and the CSV are byte-identical.  Once at batch 32: the cached activation tensors of ALL FIVE layers are the
    bits of batch 64's -- every kernel between the image and a hooked output (K16, K17, K18, K0n) has one fixed
    reduction order per output element, and no library GEMM is among them.  (The CSV may differ between batch sizes:
    the ViT dissector's GEMMs do depend on the batch.)"""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    cnt = util.CallCounter(core, monkeypatch, NEW_WRAPPERS)
    act1, csv1 = _run_driver(dev, str(tmp_path), "one")
    assert cnt.n.get("conv_igemm_nhwc", 0) >= 19 * 4 and cnt.n.get("conv7x7s2_nhwc", 0) >= 4 and cnt.relu_gemms == 0
    act2, csv2 = _run_driver(dev, str(tmp_path), "two")
    f1, f2 = _layer_files(act1), _layer_files(act2)
    assert sorted(f1) == sorted(f2) and len(f1) == 5
    for name in f1:
        a, b = torch.load(f1[name], weights_only=True), torch.load(f2[name], weights_only=True)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert csv1 == csv2 and len(csv1) > 10000
    act3, _ = _run_driver(dev, str(tmp_path), "b32", batch=32)
    f3 = _layer_files(act3)
    assert sorted(f3) == sorted(f1)
    for name in f1:
        a, b = torch.load(f1[name], weights_only=True), torch.load(f3[name], weights_only=True)
        assert a.shape == b.shape and a.shape[0] == 256 and torch.equal(a, b), name


# ---- 9. ranks -----------------------------------------------------------------------------------------------------------
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
        ["--target_model", "resnet18", "--target_layers", ",".join(LAYERS), "--d_probe", "synthetic_%d_224" % n_images,
         "--concept_set", CONCEPTS, "--batch_size", str(batch), "--device", "cuda:0", "--activation_dir",
         os.path.join(tmp, "acts%d_%d" % (world, rank)), "--result_dir", os.path.join(tmp, "res%d" % world)])
    torch.cuda.synchronize()
    return out


def test_driver_csv_bytes_one_vs_two_ranks(mcd, dev, tmp_path, monkeypatch):
    """The whole ResNet-18 job at 1 rank and at 2 ranks (spawned processes on one GPU, gloo, equal batch shapes, the
    heuristic hipBLASLt pick for the dissector): rank 0's CSV is the same bytes."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    monkeypatch.setenv("MCD_SHARD_ALIGN", "40")
    tmp = str(tmp_path)
    csv = {}
    for world in (1, 2):        # fresh processes: this one may keep timed GEMM picks for these shapes from other tests
        got = util.run_ranks(world, _rank_driver, (tmp, 160, 40), timeout=900, env=util.TORCHRUN_ENV)
        csv[world] = open(glob.glob(os.path.join(got[0], "*.csv"))[0], "rb").read()
    assert csv[1] == csv[2] and len(csv[1]) > 10000


def test_describe_og_neurons_resnet34(core, dev, tmp_path, monkeypatch):
    """The factory is all the drivers need: describe_og_neurons on the ResNet-34 target writes one row per neuron of
    conv1 + layer1..4 (64 + 64 + 128 + 256 + 512), through K18.  cos_similarity, because 64 images are fewer than the
    top_k = 100 that soft_wpmi selects (torch.topk raises there, in the reference as here)."""
    import pandas as pd
    from mammo_clip_dissect_amd.concept_vit import describe_og_neurons as drv
    cnt = util.CallCounter(core, monkeypatch, NEW_WRAPPERS)
    out = drv.main(["--target_model", "resnet34", "--target_layers", ",".join(LAYERS), "--d_probe", "synthetic_64_224",
                    "--concept_set", CONCEPTS, "--batch_size", "32", "--device", str(dev),
                    "--similarity_fn", "cos_similarity", "--activation_dir", str(tmp_path / "acts"),
                    "--result_dir", str(tmp_path / "results")])
    df = pd.read_csv(os.path.join(out, "descriptions.csv"))
    assert len(df) == 1024 and [int((df.layer == n).sum()) for n in LAYERS] == [64, 64, 128, 256, 512]
    assert cnt.n.get("conv_igemm_nhwc", 0) >= 35 * 2 and cnt.relu_gemms == 0
