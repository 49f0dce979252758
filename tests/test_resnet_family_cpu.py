"""CPU: the host side of the ResNet-18 / -34 / -101 / -152 / resnet18_places targets and of K18's residual entry
(mcd_conv_igemm_res_nhwc): the symbol in the header, the ctypes table and the library; the entry's argument checks by
return code; the module trees and state_dict() of the new towers; the _BasicBlock fold in float64; the CPU forward
against the hand-written torchvision computation; resnet_route's table for a _BasicBlock; the factory and the
Places365 checkpoint container.  No kernel runs here."""
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

from util import FakeCuda as _FakeCuda, entry_rc as _rc, nhwc_input as _nhwc_input, randomise_bn as _randomise_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = None
P, Q = 4096, 1 << 20     # non-NULL, 16-byte aligned pointer values, 1 MiB apart, that no rejected call may dereference
E_ARG, E_UNS = -1, -5
RES = "mcd_conv_igemm_res_nhwc"


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _core():
    from mammo_clip_dissect_amd import core
    return core


# ---- the symbol ---------------------------------------------------------------------------------------------------------
def test_res_symbol_everywhere(mcd):
    h = open(os.path.join(ROOT, "include", "mcd_hip.h")).read()
    L = mcd._lib.load()
    assert "int %s(" % RES in h and "data_utils.py:70-89" in h
    assert RES in mcd._lib.SIGNATURES and hasattr(L, RES)
    old, new = mcd._lib.SIGNATURES["mcd_conv_igemm_nhwc"], mcd._lib.SIGNATURES[RES]
    assert old[0] == new[0] and len(new[1]) == len(old[1]) + 1            # one more pointer; the old entry as it was
    assert new[1][:7] == old[1][:7] and new[1][8:] == old[1][7:]
    assert L.mcd_abi_version() == 9
    assert inspect.signature(_core().conv_igemm_nhwc).parameters["res"].default is None


# ---- the entry's argument checks ----------------------------------------------------------------------------------------
def test_res_entry_rejects_bad_arguments(mcd):
    # mcd_conv_igemm_res_nhwc(x, B, H, W, Cin, w, bias, res, Cout, k, stride, relu_in, relu_out, y, stream)
    s = None
    ok = [P, 2, 8, 8, 64, P, P, Q, 64, 3, 1, 1, 1, P, s]
    for i in (0, 5, 6, 13):                                                # x, w, bias, y
        a = list(ok)
        a[i] = NULL
        assert _rc(mcd, RES, *a) == E_ARG, i
    assert _rc(mcd, RES, P, 2, 0, 8, 64, P, P, Q, 64, 3, 1, 1, 1, P, s) == E_ARG
    assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P + 4, Q, 64, 3, 1, 1, 1, P, s) == E_ARG
    assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P, Q + 4, 64, 3, 1, 1, 1, P, s) == E_ARG          # a 4-byte aligned res
    assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P, Q, 64, 3, 1, 1, 1, Q, s) == E_ARG              # res == y
    assert b"overlap" in mcd._lib.load().mcd_last_error()
    # y is 2 * 8 * 8 * 64 * 4 = 32 768 bytes: a res that starts or ends inside it overlaps, one right behind it does not
    # (that call would launch, so it is made with B = 0, where the kernel is not started)
    assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P, Q + 32768 - 16, 64, 3, 1, 1, 1, Q, s) == E_ARG
    assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P, Q - 32768 + 16, 64, 3, 1, 1, 1, Q, s) == E_ARG
    for res in (NULL, Q):
        for k, st in ((5, 1), (3, 3), (1, 1), (7, 2)):                                          # instantiations
            assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P, res, 64, k, st, 0, 0, P, s) == E_UNS, (k, st)
        assert _rc(mcd, RES, P, 2, 8, 8, 48, P, P, res, 64, 3, 1, 0, 0, P, s) == E_UNS        # Cin % 32
        assert _rc(mcd, RES, P, 2, 8, 8, 64, P, P, res, 80, 3, 1, 0, 0, P, s) == E_UNS        # Cout % 32
        assert _rc(mcd, RES, P, 2, 4096, 4096, 64, P, P, res, 64, 3, 1, 0, 0, P, s) == E_UNS
        assert _rc(mcd, RES, P, 65536, 8, 8, 64, P, P, res, 64, 3, 1, 0, 0, P, s) == E_UNS
        assert b"65535" in mcd._lib.load().mcd_last_error()
        for k, st in ((3, 1), (3, 2), (1, 2)):
            assert _rc(mcd, RES, P, 0, 8, 8, 64, P, P, res, 64, k, st, 0, 0, P, s) == 0       # B = 0: nothing to do
    # the old entry is as it was
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 2, 8, 8, 64, P, NULL, 64, 3, 1, 1, 1, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv_igemm_nhwc", P, 0, 8, 8, 64, P, P, 64, 1, 2, 0, 0, P, s) == 0


def test_wrapper_refuses_a_host_res():
    core = _core()
    with pytest.raises(TypeError, match="GPU only"):
        core.conv_igemm_nhwc(torch.randn(1, 8, 8, 64), torch.randn(64, 576), torch.zeros(64), 3, 1,
                             res=torch.zeros(1, 8, 8, 64))


# ---- module trees -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_keys,depths,feat", [("resnet18", 122, [2, 2, 2, 2], 512), ("resnet34", 218, [3, 4, 6, 3], 512),
                                                     ("resnet101", 626, [3, 4, 23, 3], 2048),
                                                     ("resnet152", 932, [3, 8, 36, 3], 2048)])
def test_state_dict_of_the_new_towers(du, name, n_keys, depths, feat):
    net, pre = du.get_target_model(name, "cpu")
    assert pre is None and not net.training and isinstance(net, du.ResNet)
    sd = net.state_dict()
    assert len(sd) == n_keys
    assert list(sd)[0] == "conv1.weight" and list(sd)[-2:] == ["fc.weight", "fc.bias"]
    assert [n for n, _ in net.named_children()] == ["conv1", "bn1", "layer1", "layer2", "layer3", "layer4", "fc"]
    assert [len(getattr(net, "layer%d" % i)) for i in (1, 2, 3, 4)] == depths
    assert tuple(sd["fc.weight"].shape) == (1000, feat)
    assert net.encode_image.__func__ is net.forward.__func__


def test_basic_block_tree(du):
    net = du.get_target_model("resnet18", "cpu")[0]
    sd = net.state_dict()
    assert sd["layer2.0.downsample.0.weight"].shape == (128, 64, 1, 1)
    assert sd["layer1.0.conv1.weight"].shape == (64, 64, 3, 3) and "layer1.0.downsample.0.weight" not in sd
    blk = net.layer2[0]
    assert isinstance(blk, du._BasicBlock) and isinstance(net.layer2, torch.nn.Sequential)
    assert [n for n, _ in blk.named_children()] == ["conv1", "bn1", "conv2", "bn2", "downsample"]
    assert [n for n, _ in net.layer2[1].named_children()] == ["conv1", "bn1", "conv2", "bn2"]
    assert net.layer2[1].downsample is None and blk.conv1.stride == (2, 2) and blk.conv2.stride == (1, 1)
    assert isinstance(blk.downsample[0], torch.nn.Conv2d) and isinstance(blk.downsample[1], torch.nn.BatchNorm2d)
    assert du.get_target_model("resnet18_places", "cpu")[0].state_dict()["fc.weight"].shape[0] == 365
    # folding registers nothing
    keys = list(sd)
    du._folded(blk, du._BASICBLOCK_SKIPPED, du._BasicBlock._fold)
    assert list(net.state_dict()) == keys and not list(blk.buffers(recurse=False))
    # the seed decides the weights, and ResNet50 is the generic tower of bottlenecks under the same seed
    a = du.get_target_model("resnet18", "cpu", seed=3)[0].state_dict()
    b = du.get_target_model("resnet18", "cpu", seed=3)[0].state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    torch.manual_seed(0)
    r50 = du.ResNet50().state_dict()
    torch.manual_seed(0)
    gen = du.ResNet(du._Bottleneck, [3, 4, 6, 3]).state_dict()
    assert list(r50) == list(gen) and all(torch.equal(r50[k], gen[k]) for k in r50)


# ---- folding ------------------------------------------------------------------------------------------------------------
def _igemm_conv64(x, w_tap, bias, k, s):
    """What K18 computes, in float64 on the host: x NCHW, w_tap [Cout, k*k*Cin] tap-major then channel."""
    cout, cin = w_tap.shape[0], x.shape[1]
    w = w_tap.view(cout, k, k, cin).permute(0, 3, 1, 2)
    return F.conv2d(x, w, bias, s, 1 if k == 3 else 0)


@pytest.mark.parametrize("cin,width,stride", [(64, 64, 1), (64, 128, 2), (256, 512, 2)])
def test_basic_block_folding_float64(du, cin, width, stride):
    g = torch.Generator().manual_seed(cin + stride)
    blk = du._BasicBlock(cin, width, stride).double().eval()
    with torch.no_grad():
        _randomise_bn(blk, g)
        f = blk._fold()
        x = torch.randn(2, cin, 9, 6, generator=g, dtype=torch.float64)
        ref1 = blk.bn1(blk.conv1(x))
        assert f["w1"].shape == (width, 9 * cin) and f["w1"].is_contiguous()
        got1 = _igemm_conv64(x, f["w1"], f["b1"], 3, stride)
        assert got1.shape == ref1.shape and (got1 - ref1).abs().max() <= 1e-12 * ref1.abs().max()
        h = torch.randn(2, width, 5, 3, generator=g, dtype=torch.float64)
        ref2 = blk.bn2(blk.conv2(h))
        assert f["w2"].shape == (width, 9 * width)
        got2 = _igemm_conv64(h, f["w2"], f["b2"], 3, 1)
        assert got2.shape == ref2.shape and (got2 - ref2).abs().max() <= 1e-12 * ref2.abs().max()
        if blk.downsample is not None:
            refd = blk.downsample(x)
            skip = _igemm_conv64(x, f["wd"], f["bd"], 1, stride)
            assert skip.shape == refd.shape and (skip - refd).abs().max() <= 1e-12 * refd.abs().max()
        else:
            assert "wd" not in f and stride == 1
            skip = x
        # the whole block from the folded pieces, the skip added before the ReLU
        whole = F.relu(_igemm_conv64(F.relu(got1), f["w2"], f["b2"], 3, 1) + skip)
        ref = blk(x)
        assert whole.shape == ref.shape and (whole - ref).abs().max() <= 1e-12 * ref.abs().max()
        assert (ref == 0).any() and (ref > 0).any()


# ---- the CPU forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet18", "resnet34"])
def test_cpu_forward_is_the_torchvision_computation(du, name):
    g = torch.Generator().manual_seed(3)
    net = du.get_target_model(name, "cpu")[0]
    with torch.no_grad():
        _randomise_bn(net, g)
        x = torch.randn(1, 3, 64, 48, generator=g)
        y = F.max_pool2d(F.relu(net.bn1(F.conv2d(x, net.conv1.weight, None, 2, 3))), 3, 2, 1)
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for b in layer:
                z = F.relu(b.bn1(F.conv2d(y, b.conv1.weight, None, b.stride, 1)))
                z = b.bn2(F.conv2d(z, b.conv2.weight, None, 1, 1))
                if b.downsample is not None:
                    y = b.downsample[1](F.conv2d(y, b.downsample[0].weight, None, b.stride, 0))
                y = F.relu(z + y)
        ref = net.fc(y.mean(dim=[2, 3]))
        assert torch.equal(net(x), ref) and torch.equal(net.encode_image(x), ref)


# ---- routing ------------------------------------------------------------------------------------------------------------
def test_route_table_for_basic_blocks(du, monkeypatch):
    core = _core()
    monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    monkeypatch.setattr(du, "HIP_RESNET", True)
    net = du.get_target_model("resnet18", "cpu")[0]
    plain, down = net.layer1[0], net.layer2[0]
    x64 = _nhwc_input(64)
    img = torch.randn(2, 3, 40, 36).as_subclass(_FakeCuda)
    with torch.no_grad():
        assert du.resnet_route(net, img) == "hip" and du.resnet_route(net.conv1, img) == "hip"
        assert du.resnet_route(plain, x64) == "hip" and du.resnet_route(down, x64) == "hip"
        assert du.resnet_route(net.layer4[1], _nhwc_input(512, 3, 2)) == "hip"
        assert du.resnet_route(du._BasicBlock(96, 32, 2).eval(), _nhwc_input(96)) == "hip"
        # flag off
        monkeypatch.setattr(du, "HIP_RESNET", False)
        assert du.resnet_route(plain, x64) == "aten" and du.resnet_route(down, x64) == "aten"
        monkeypatch.setattr(du, "HIP_RESNET", True)
        # training mode
        net.train()
        assert du.resnet_route(plain, x64) == "aten" and du.resnet_route(down, x64) == "aten"
        net.eval()
        # a host tensor, NCHW memory, fp64, the wrong channel count
        assert du.resnet_route(plain, x64.as_subclass(torch.Tensor)) == "aten"
        assert du.resnet_route(plain, x64.contiguous()) == "aten" and du.resnet_route(down, x64.contiguous()) == "aten"
        assert du.resnet_route(plain, x64.double()) == "aten" and du.resnet_route(down, x64.double()) == "aten"
        assert du.resnet_route(plain, _nhwc_input(128)) == "aten"
        # width 48
        assert du.resnet_route(du._BasicBlock(48, 48, 1).eval(), _nhwc_input(48)) == "aten"
        assert du.resnet_route(du._BasicBlock(64, 48, 2).eval(), x64) == "aten"
        assert du.resnet_route(du._BasicBlock(48, 64, 2).eval(), _nhwc_input(48)) == "aten"
        # a stride-1 block with cin != width: a 1x1 / 1 downsample, which K18 does not do
        odd = du._BasicBlock(64, 128, 1).eval()
        assert odd.downsample is not None and du.resnet_route(odd, x64) == "aten"
        # the common gate: libmcd_blaslt.so is asked for although a _BasicBlock calls no library GEMM
        monkeypatch.setattr(core, "linear_residual_available", lambda: False)
        assert du.resnet_route(plain, x64) == "aten" and du.resnet_route(net, img) == "aten"
        monkeypatch.setattr(core, "linear_residual_available", lambda: True)
        # hooks on what the route does not call: that block only
        h = down.conv2.register_forward_hook(lambda m, i, o: None)
        assert du.resnet_route(down, x64) == "aten" and du.resnet_route(plain, x64) == "hip"
        assert du.resnet_route(net, img) == "hip"
        h.remove()
        h = down.downsample[1].register_forward_hook(lambda m, i, o: None)
        assert du.resnet_route(down, x64) == "aten"
        h.remove()
        for name in ("conv1", "bn1", "conv2", "bn2", "downsample"):
            h = getattr(down, name).register_forward_pre_hook(lambda m, i: None)
            assert du.resnet_route(down, x64) == "aten", name
            h.remove()
        assert du.resnet_route(down, x64) == "hip"
        # hooks on the hook points (a stage, a block itself) leave the route alone
        hs = [m.register_forward_hook(lambda m, i, o: None) for m in (net.layer2, down, plain)]
        assert du.resnet_route(down, x64) == "hip" and du.resnet_route(plain, x64) == "hip"
        for h in hs:
            h.remove()
    with torch.enable_grad():
        assert du.resnet_route(plain, x64) == "aten" and du.resnet_route(down, x64) == "aten"


# ---- the factory --------------------------------------------------------------------------------------------------------
def test_factory_names_and_places_checkpoint(du, tmp_path, monkeypatch):
    for name in ("resnet18", "resnet34", "resnet101", "resnet152", "resnet18_places"):
        net, _ = du.get_target_model(name, "cpu")
        assert isinstance(net, du.ResNet) and not net.training
    with pytest.raises(ValueError, match="unknown target model.*resnet18_places.*resnet152"):
        du.get_target_model("resnet19", "cpu")
    with pytest.raises(ValueError):
        du.get_target_model("resnet", "cpu")
    # the reference's container: {'state_dict': {'module.' + key: tensor}}
    src = du.get_target_model("resnet18_places", "cpu", seed=11)[0]
    with torch.no_grad():
        _randomise_bn(src, torch.Generator().manual_seed(1))
    path = str(tmp_path / "resnet18_places365.pth.tar")
    torch.save({"state_dict": {"module." + k: v for k, v in src.state_dict().items()}}, path)
    net, _ = du.get_target_model("resnet18_places", "cpu", ckpt=path)
    want, got = src.state_dict(), net.state_dict()
    assert list(want) == list(got) and all(torch.equal(want[k], got[k]) for k in want)
    assert not torch.equal(du.get_target_model("resnet18_places", "cpu")[0].fc.weight, src.fc.weight)
    # without a path: the reference's relative data/resnet18_places365.pth.tar
    os.makedirs(str(tmp_path / "data"))
    os.replace(path, str(tmp_path / "data" / "resnet18_places365.pth.tar"))
    monkeypatch.chdir(tmp_path)
    net, _ = du.get_target_model("resnet18_places", "cpu")
    assert torch.equal(net.fc.weight, src.fc.weight) and torch.equal(net.layer3[0].downsample[1].running_var,
                                                                      src.layer3[0].downsample[1].running_var)
    # a file weights_only=True cannot load is an error, not a random model
    bad = str(tmp_path / "bad.pth.tar")
    torch.save({"state_dict": {"fc.bias": torch.zeros(365)}, "extra": _NotATensor()}, bad)
    with pytest.raises(RuntimeError, match="weights_only"):
        du.get_target_model("resnet18_places", "cpu", ckpt=bad)
    # and so is one whose keys do not fit (the load is strict, as the reference's)
    torch.save({"state_dict": {"module.fc.bias": torch.zeros(365)}}, bad)
    with pytest.raises(RuntimeError):
        du.get_target_model("resnet18_places", "cpu", ckpt=bad)


class _NotATensor:
    """An object the weights-only unpickler refuses."""
