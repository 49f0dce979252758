"""CPU: the host side of the ResNet-50 target's HIP route (K16-K18, mcd_linear_residual_relu): the new symbols are in
the headers, the ctypes tables and both libraries; resnet_route's refusals; the folded and relaid weights reproduce
bn(conv(x)) in float64 with randomised batch-norm state; the output-size arithmetic; the argument checks of the C
entries and the wrappers; the module tree and state_dict() of ResNet50.  No kernel runs here."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from util import FakeCuda as _FakeCuda, entry_rc as _rc, nhwc_input as _nhwc_input, randomise_bn as _randomise_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = None
P = 4096            # a non-NULL, 16-byte aligned pointer value that no rejected call may dereference
E_ARG, E_UNS = -1, -5


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _core():
    from mammo_clip_dissect_amd import core
    return core


# ---- symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_everywhere(mcd):
    h = open(os.path.join(ROOT, "include", "mcd_hip.h")).read()
    L = mcd._lib.load()
    for name in ("mcd_conv7x7s2_nhwc", "mcd_bn_relu_maxpool_nhwc", "mcd_conv_igemm_nhwc"):
        assert "int %s(" % name in h
        assert name in mcd._lib.SIGNATURES and hasattr(L, name)
    assert "v_mfma_f32_32x32x2_f32" in h and "data_utils.py:85-93" in h
    hb = open(os.path.join(ROOT, "include", "mcd_blaslt.h")).read()
    assert "int mcd_linear_residual_relu(" in hb
    assert "mcd_linear_residual_relu" in mcd._lib.BLASLT_SIGNATURES
    assert mcd._lib.BLASLT_SIGNATURES["mcd_linear_residual_relu"] == mcd._lib.BLASLT_SIGNATURES["mcd_linear_residual"]
    B = mcd._lib.load_blaslt()
    assert B is not None and hasattr(B, "mcd_linear_residual_relu")
    assert L.mcd_abi_version() == 9
    mk = open(os.path.join(ROOT, "mammo-clip-dissect_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bk_resnet\.hip\b", mk, flags=re.M)
    core = _core()
    for name in ("conv7x7s2_nhwc", "bn_relu_maxpool_nhwc", "conv_igemm_nhwc"):
        assert callable(getattr(core, name))
    import inspect
    assert inspect.signature(core.linear_residual).parameters["relu"].default is False


# ---- routing ------------------------------------------------------------------------------------------------------
def test_route_fallbacks(du, monkeypatch):
    core = _core()
    monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    monkeypatch.setattr(du, "HIP_RESNET", True)
    net = du.ResNet50().eval()
    blk = net.layer2[0]
    x = _nhwc_input(256)
    img = torch.randn(2, 3, 40, 36).as_subclass(_FakeCuda)
    with torch.no_grad():
        assert du.resnet_route(net, img) == "hip"
        assert du.resnet_route(net.conv1, img) == "hip"
        assert du.resnet_route(blk, x) == "hip"
        assert du.resnet_route(net.layer1[0], _nhwc_input(64)) == "hip"
        assert du.resnet_route(net.layer4[2], _nhwc_input(2048, 3, 2)) == "hip"
        # a CPU tensor
        for m, t in ((net, img), (net.conv1, img), (blk, x)):
            assert du.resnet_route(m, t.as_subclass(torch.Tensor)) == "aten"
        # fp64, wrong layout, wrong width, a module the route does not know
        assert du.resnet_route(blk, x.double()) == "aten" and du.resnet_route(net, img.double()) == "aten"
        assert du.resnet_route(blk, x.contiguous()) == "aten"
        assert du.resnet_route(net, img.contiguous(memory_format=torch.channels_last)) == "aten"
        assert du.resnet_route(blk, _nhwc_input(128)) == "aten"
        assert du.resnet_route(du._Bottleneck(48, 24, 1).eval(), _nhwc_input(48)) == "aten"      # widths % 32
        assert du.resnet_route(net.bn1, img) == "aten"
        assert du.resnet_route(net, torch.randn(2, 5, 40, 36).as_subclass(_FakeCuda)) == "aten"
        # training mode
        net.train()
        assert du.resnet_route(net, img) == "aten" and du.resnet_route(blk, x) == "aten"
        assert du.resnet_route(net.conv1, img) == "aten"
        net.eval()
        # HIP_RESNET off
        monkeypatch.setattr(du, "HIP_RESNET", False)
        assert du.resnet_route(net, img) == "aten" and du.resnet_route(blk, x) == "aten"
        assert du.resnet_route(net.conv1, img) == "aten"
        monkeypatch.setattr(du, "HIP_RESNET", True)
        # no hipBLASLt companion
        monkeypatch.setattr(core, "linear_residual_available", lambda: False)
        assert du.resnet_route(net, img) == "aten" and du.resnet_route(blk, x) == "aten"
        monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    with torch.enable_grad():
        assert du.resnet_route(net, img) == "aten" and du.resnet_route(blk, x) == "aten"
        assert du.resnet_route(net.conv1, img) == "aten"
    with torch.no_grad():
        # a hook on layer2[0].conv2: that block only
        h = net.layer2[0].conv2.register_forward_hook(lambda m, i, o: None)
        assert du.resnet_route(blk, x) == "aten"
        assert du.resnet_route(net.layer2[1], _nhwc_input(512)) == "hip"
        assert du.resnet_route(net, img) == "hip" and du.resnet_route(net.conv1, img) == "hip"
        h.remove()
        assert du.resnet_route(blk, x) == "hip"
        # every inner module of a block, the downsample's members included; pre-hooks too
        for name in ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "downsample"):
            h = getattr(blk, name).register_forward_hook(lambda m, i, o: None)
            assert du.resnet_route(blk, x) == "aten", name
            h.remove()
        for sub in blk.downsample:
            h = sub.register_forward_pre_hook(lambda m, i: None)
            assert du.resnet_route(blk, x) == "aten"
            h.remove()
        # hooks on the hook points of the tower (conv1, layer1..4, a block itself) leave the route alone
        hs = [m.register_forward_hook(lambda m, i, o: None) for m in (net.conv1, net.layer1, net.layer4, blk)]
        assert du.resnet_route(net, img) == "hip" and du.resnet_route(blk, x) == "hip"
        assert du.resnet_route(net.conv1, img) == "hip"
        for h in hs:
            h.remove()
        # bn1 of the tower is fused into K17: a hook on it sends the tower to ATen
        h = net.bn1.register_forward_hook(lambda m, i, o: None)
        assert du.resnet_route(net, img) == "aten"
        h.remove()
        h = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
        try:
            assert du.resnet_route(blk, x) == "aten" and du.resnet_route(net, img) == "aten"
        finally:
            h.remove()
        assert du.resnet_route(blk, x) == "hip"


def test_cpu_forward_is_the_aten_route(du):
    """On a CPU tensor every module takes ATen: the forward equals the plain torchvision-layout computation."""
    g = torch.Generator().manual_seed(3)
    net = du.ResNet50().eval()
    with torch.no_grad():
        _randomise_bn(net, g)
        x = torch.randn(1, 3, 64, 48, generator=g)
        y = F.max_pool2d(F.relu(net.bn1(F.conv2d(x, net.conv1.weight, None, 2, 3))), 3, 2, 1)
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for b in layer:
                z = F.relu(b.bn1(b.conv1(y)))
                z = F.relu(b.bn2(b.conv2(z)))
                z = b.bn3(b.conv3(z))
                y = F.relu(z + (y if b.downsample is None else b.downsample(y)))
        ref = net.fc(y.mean(dim=[2, 3]))
        assert torch.equal(net(x), ref)


# ---- folding ------------------------------------------------------------------------------------------------------
def _igemm_conv64(x, w_tap, bias, k, s):
    """What K18 computes, in float64 on the host: x NCHW, w_tap [Cout, k*k*Cin] tap-major then channel."""
    cout, cin = w_tap.shape[0], x.shape[1]
    w = w_tap.view(cout, k, k, cin).permute(0, 3, 1, 2)
    return F.conv2d(x, w, bias, s, 1 if k == 3 else 0)


@pytest.mark.parametrize("cin,width,stride", [(256, 128, 2), (64, 64, 1), (512, 128, 1)])
def test_bottleneck_folding_float64(du, cin, width, stride):
    g = torch.Generator().manual_seed(cin + stride)
    blk = du._Bottleneck(cin, width, stride).double().eval()
    with torch.no_grad():
        _randomise_bn(blk, g)
        f = blk._fold()
        H, W = 13, 10
        x = torch.randn(2, cin, H, W, generator=g, dtype=torch.float64)
        ref = blk.bn1(blk.conv1(x))
        got = torch.einsum("bchw,mc->bmhw", x, f["w1"]) + f["b1"].view(1, -1, 1, 1)
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        h = torch.randn(2, width, H, W, generator=g, dtype=torch.float64)
        ref = blk.bn2(blk.conv2(h))                                  # the 3x3 (stride 2 in the first case)
        assert f["w2"].shape == (width, 9 * width) and f["w2"].is_contiguous()
        got = _igemm_conv64(h, f["w2"], f["b2"], 3, stride)
        assert got.shape == ref.shape and (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        # tap-major then channel: element [o, (dy*3 + dx)*Cin + c] is weight[o, c, dy, dx] * scale[o]
        scale = blk.bn2.weight / torch.sqrt(blk.bn2.running_var + blk.bn2.eps)
        assert torch.allclose(f["w2"][5, (1 * 3 + 2) * width + 7], blk.conv2.weight[5, 7, 1, 2] * scale[5], rtol=1e-14)
        y = torch.randn(2, width, 5, 4, generator=g, dtype=torch.float64)
        ref = blk.bn3(blk.conv3(y))
        got = torch.einsum("bchw,mc->bmhw", y, f["w3"]) + f["b3"].view(1, -1, 1, 1)
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        if blk.downsample is not None:
            ref = blk.downsample(x)                                  # the 1x1 / 2 in the first case
            got = _igemm_conv64(x, f["wd"], f["bd"], 1, stride)
            assert got.shape == ref.shape and (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        else:
            assert "wd" not in f


def test_stem_folding_float64(du):
    g = torch.Generator().manual_seed(11)
    net = du.ResNet50().double().eval()
    with torch.no_grad():
        _randomise_bn(net, g)
        x = torch.randn(2, 3, 37, 30, generator=g, dtype=torch.float64)
        w_tap = net.conv1.weight.permute(1, 2, 3, 0).contiguous()    # what _StemConv hands K16
        raw = F.conv2d(x, w_tap.permute(3, 0, 1, 2), None, 2, 3)
        assert torch.equal(raw, net.conv1(x))
        scale, shift = du.bn_scale_shift(net.bn1)
        got = raw * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        ref = net.bn1(net.conv1(x))
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        # K17 in float64: the maximum of relu over the real pixels of the window
        pooled = F.max_pool2d(F.relu(got), 3, 2, 1)
        assert (pooled - F.max_pool2d(F.relu(ref), 3, 2, 1)).abs().max() <= 1e-12 * ref.abs().max()


def test_fold_conv_layouts(du):
    """_fold_conv's three layouts against the expressions the _fold methods spelled out before it, bit for bit."""
    g = torch.Generator().manual_seed(5)
    conv, bn = torch.nn.Conv2d(4, 8, 3, bias=False), torch.nn.BatchNorm2d(8).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(8, 4, 3, 3, generator=g))
        _randomise_bn(bn, g)
        w, b = du.fold_bn(conv.weight, bn)
        assert not torch.equal(w, conv.weight) and b.abs().min() > 0      # a batch norm that does something
        for layout, want in (("gemm", w.flatten(1).contiguous()), ("igemm", du.igemm_weight(w)),
                             ("tap", w.permute(1, 2, 3, 0).contiguous())):
            got_w, got_b = du._fold_conv(conv, bn, layout)
            assert got_w.shape == want.shape and got_w.dtype == want.dtype and torch.equal(got_w, want), layout
            assert got_w.is_contiguous() and got_b.is_contiguous() and torch.equal(got_b, b), layout
        assert tuple(du._fold_conv(conv, bn, "gemm")[0].shape) == (8, 36)
        assert tuple(du._fold_conv(conv, bn, "igemm")[0].shape) == (8, 36)
        assert tuple(du._fold_conv(conv, bn, "tap")[0].shape) == (4, 3, 3, 8)
    with pytest.raises(KeyError):
        du._fold_conv(conv, bn, "nchw")


def test_fold_cache_follows_the_parameters(du):
    blk = du._Bottleneck(256, 128, 2).eval()
    f1 = du._folded(blk, du._BOTTLENECK_SKIPPED, du._Bottleneck._fold)
    assert du._folded(blk, du._BOTTLENECK_SKIPPED, du._Bottleneck._fold) is f1
    with torch.no_grad():
        blk.downsample[1].running_mean.add_(1.0)                     # nested in the Sequential
    f2 = du._folded(blk, du._BOTTLENECK_SKIPPED, du._Bottleneck._fold)
    assert f2 is not f1 and not torch.equal(f1["bd"], f2["bd"]) and torch.equal(f1["w2"], f2["w2"])
    with torch.no_grad():
        blk.conv2.weight.mul_(2.0)
    f3 = du._folded(blk, du._BOTTLENECK_SKIPPED, du._Bottleneck._fold)
    assert torch.equal(f3["w2"], f2["w2"] * 2)


# ---- sizes ----------------------------------------------------------------------------------------------------------
def test_output_size_arithmetic():
    core = _core()
    g = torch.Generator().manual_seed(0)
    for n in list(range(1, 40)) + [47, 56, 65, 112, 223, 224, 225]:
        for k, s, p in ((7, 2, 3), (3, 2, 1), (3, 1, 1), (1, 2, 0)):
            m = 23                                                    # non-square: the other axis differs
            ref = F.conv2d(torch.zeros(1, 1, n, m), torch.zeros(1, 1, k, k), None, s, p).shape
            assert (core.conv_out(n, k, s, p), core.conv_out(m, k, s, p)) == tuple(ref[2:]), (n, k, s, p)
        assert core.conv_out(n, 3, 2, 1) == F.max_pool2d(torch.zeros(1, 1, n, 5), 3, 2, 1).shape[2]
    assert core.conv_out(224, 7, 2, 3) == 112 and core.conv_out(112, 3, 2, 1) == 56
    assert core.conv_out(65, 3, 2, 1) == 33 and core.conv_out(47, 1, 2, 0) == 24 and core.conv_out(7, 3, 2, 1) == 4


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments(mcd):
    s = None
    # K16 mcd_conv7x7s2_nhwc(x, B, Cin, H, W, w, Cout, y, stream)
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", NULL, 2, 3, 8, 8, P, 64, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 2, 3, 8, 8, P, 62, P, s) == E_ARG               # Cout % 4
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 2, 5, 8, 8, P, 64, P, s) == E_ARG               # Cin > 4
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, -1, 3, 8, 8, P, 64, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 2, 3, 8, 8, P + 4, 64, P, s) == E_ARG           # alignment
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 2, 3, 40000, 40000, P, 64, P, s) == E_UNS       # one image >= 2^31 B
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 65536, 3, 8, 8, P, 64, P, s) == E_UNS
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 2, 3, 8, 8, P + 65536, 64, P + 16, s) == E_ARG  # y starts inside x
    assert b"overlap" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 2, 3, 8, 8, P + 65536 + 1024, 64, P + 65536, s) == E_ARG   # w inside y
    assert _rc(mcd, "mcd_conv7x7s2_nhwc", P, 0, 3, 8, 8, P, 64, P, s) == 0                   # B = 0: nothing to do
    # K17 mcd_bn_relu_maxpool_nhwc(x, B, H, W, C, scale, shift, y, stream)
    assert _rc(mcd, "mcd_bn_relu_maxpool_nhwc", P, 2, 8, 8, 64, NULL, P, P, s) == E_ARG
    assert _rc(mcd, "mcd_bn_relu_maxpool_nhwc", P, 2, 8, 8, 62, P, P, P, s) == E_ARG         # C % 4
    assert _rc(mcd, "mcd_bn_relu_maxpool_nhwc", P, 2, 0, 8, 64, P, P, P, s) == E_ARG
    assert _rc(mcd, "mcd_bn_relu_maxpool_nhwc", P + 8, 2, 8, 8, 64, P, P, P, s) == E_ARG
    assert _rc(mcd, "mcd_bn_relu_maxpool_nhwc", P, 2, 4096, 4096, 64, P, P, P, s) == E_UNS
    assert _rc(mcd, "mcd_bn_relu_maxpool_nhwc", P, 0, 8, 8, 64, P, P, P, s) == 0
    # K18 mcd_conv_igemm_nhwc(x, B, H, W, Cin, w, bias, Cout, k, stride, relu_in, relu_out, y, stream)
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 8, 8, 64, P, NULL, 64, 3, 1, 1, 1, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 0, 8, 64, P, P, 64, 3, 1, 1, 1, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 8, 8, 64, P, P + 4, 64, 3, 1, 1, 1, P, s) == E_ARG
    for k, st in ((5, 1), (3, 3), (1, 1), (7, 2)):                                              # instantiations
        assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 8, 8, 64, P, P, 64, k, st, 0, 0, P, s) == E_UNS, (k, st)
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 8, 8, 48, P, P, 64, 3, 1, 0, 0, P, s) == E_UNS   # Cin % 32
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 8, 8, 64, P, P, 80, 3, 1, 0, 0, P, s) == E_UNS   # Cout % 32
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 4096, 4096, 64, P, P, 64, 3, 1, 0, 0, P, s) == E_UNS
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 65536, 8, 8, 64, P, P, 64, 3, 1, 0, 0, P, s) == E_UNS
    assert b"65535" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 0, 8, 8, 64, P, P, 64, 1, 2, 0, 0, P, s) == 0


def test_wrappers_refuse_host_tensors():
    """The wrappers check before they load or call the library: a CPU tensor never reaches it."""
    core = _core()
    with pytest.raises(TypeError, match="GPU only"):
        core.conv7x7s2_nhwc(torch.randn(1, 3, 8, 8), torch.randn(3, 7, 7, 64))
    with pytest.raises(TypeError, match="GPU only"):
        core.bn_relu_maxpool_nhwc(torch.randn(1, 8, 8, 64), torch.ones(64), torch.zeros(64))
    with pytest.raises(TypeError, match="GPU only"):
        core.conv_igemm_nhwc(torch.randn(1, 8, 8, 64), torch.randn(64, 576), torch.zeros(64), 3, 1)
    with pytest.raises(TypeError, match="GPU only"):
        core.linear_residual(None, torch.randn(4, 8), torch.randn(8, 8), relu=True)


# ---- module tree ----------------------------------------------------------------------------------------------------
def test_module_tree_and_state_dict_unchanged(du):
    """The torchvision layout: the same names, shapes and order of state_dict() as before the route existed."""
    net = du.ResNet50()
    sd = net.state_dict()
    assert len(sd) == 320
    assert list(sd)[:7] == ["conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var",
                            "bn1.num_batches_tracked", "layer1.0.conv1.weight"]
    assert list(sd)[-2:] == ["fc.weight", "fc.bias"]
    assert sd["conv1.weight"].shape == (64, 3, 7, 7) and sd["layer4.0.downsample.0.weight"].shape == (2048, 1024, 1, 1)
    assert [n for n, _ in net.named_children()] == ["conv1", "bn1", "layer1", "layer2", "layer3", "layer4", "fc"]
    assert [len(getattr(net, "layer%d" % i)) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert [n for n, _ in net.layer2[0].named_children()] == ["conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "downsample"]
    assert isinstance(net.conv1, torch.nn.Conv2d) and isinstance(net.layer1, torch.nn.Sequential)
    # the same random initialisation as a plain Conv2d / Sequential tree under the same seed
    torch.manual_seed(0)
    a = du.ResNet50().state_dict()
    torch.manual_seed(0)
    ref_conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    assert torch.equal(a["conv1.weight"], ref_conv.weight)
    # folding registers nothing
    blk = net.layer2[0].eval()
    du._folded(blk, du._BOTTLENECK_SKIPPED, du._Bottleneck._fold)
    assert list(net.state_dict()) == list(sd)
