"""CPU: the EfficientNet-B5 tower's HIP route without a GPU -- batch-norm folding in float64, the TF-SAME pads and output
sizes the route computes, which route mbconv_route picks (and every reason it falls back to ATen), and the argument
checks the new C entries make before any device call."""

import pytest
import torch
import torch.nn.functional as F

from util import FakeCuda as _FakeCuda, entry_rc as _rc, nhwc_input as _nhwc_input, randomise_bn as _randomise_bn

NULL = None
P = 4096            # a non-NULL pointer value that no rejected call may dereference


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.mark.parametrize("cin,cout,k,s,expand", [(48, 24, 3, 1, 1), (24, 40, 5, 2, 6), (64, 64, 3, 1, 6)])
def test_folding_float64(du, cin, cout, k, s, expand):
    g = torch.Generator().manual_seed(cin + k)
    blk = du._MBConv(cin, cout, k, s, expand).double().eval()
    with torch.no_grad():
        _randomise_bn(blk, g)
        f = blk._fold()
        H = 13
        x = torch.randn(2, cin, H, H, generator=g, dtype=torch.float64)
        if blk.expand:
            ref = blk._bn0(blk._expand_conv(x))
            got = torch.einsum("bchw,mc->bmhw", x, f["w0"]) + f["b0"].view(1, -1, 1, 1)
            assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
            x = torch.randn(2, blk.mid, H, H, generator=g, dtype=torch.float64)
        ref = blk._bn1(blk._depthwise_conv(x))
        o, pt, pb = _core().same_pad(H, k, s)
        wd = f["wd"].t().reshape(blk.mid, 1, k, k)                      # back from tap-major [k*k, mid]
        got = F.conv2d(F.pad(x, [pt, pb, pt, pb]), wd, f["bd"], s, 0, 1, blk.mid)
        assert got.shape == ref.shape and (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        y = torch.randn(2, blk.mid, o, o, generator=g, dtype=torch.float64)
        ref = blk._bn2(blk._project_conv(y))
        got = torch.einsum("bchw,mc->bmhw", y, f["wp"]) + f["bp"].view(1, -1, 1, 1)
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


def test_tower_folding_float64(du):
    g = torch.Generator().manual_seed(5)
    t = du.EfficientNetB5Tower().double().eval()
    with torch.no_grad():
        _randomise_bn(t, g)
        f = t._fold()
        x = torch.randn(2, 3, 31, 20, generator=g, dtype=torch.float64)
        ref = t._bn0(t._conv_stem(x))
        (ho, pt, pb), (wo, pl, pr) = _core().same_pad(31, 3, 2), _core().same_pad(20, 3, 2)
        got = F.conv2d(F.pad(x, [pl, pr, pt, pb]), f["ws"].permute(3, 0, 1, 2), f["bs"], 2)
        assert got.shape == ref.shape == (2, 48, ho, wo)
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        h = torch.randn(2, 512, 3, 2, generator=g, dtype=torch.float64)
        ref = t._bn1(t._conv_head(h))
        got = torch.einsum("bchw,mc->bmhw", h, f["wh"]) + f["bh"].view(1, -1, 1, 1)
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


def test_fold_cache_follows_the_parameters(du):
    """The folded tensors are cached in the module's __dict__ (no parameter or buffer: state_dict keys unchanged) and
    rebuilt when a source tensor changes in place."""
    blk = du._MBConv(24, 24, 3, 1, 6).eval()
    keys = list(blk.state_dict().keys())
    a = du._folded(blk, du._MBCONV_SKIPPED, du._MBConv._fold)
    assert du._folded(blk, du._MBCONV_SKIPPED, du._MBConv._fold) is a
    with torch.no_grad():
        blk._bn1.running_var.mul_(4.0)
    b = du._folded(blk, du._MBCONV_SKIPPED, du._MBConv._fold)
    assert b is not a and not torch.equal(a["wd"], b["wd"]) and torch.equal(a["wp"], b["wp"])
    assert list(blk.state_dict().keys()) == keys and "_fold_cache" not in dict(blk.named_buffers())


def _core():
    from mammo_clip_dissect_amd import core
    return core


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
def test_same_padding_matches_sameconv(du, k, s):
    """For every size 5..225 the route's (output size, pad in front, pad behind) reproduce _SameConv: its output size,
    and the same values from an explicit (front, back) pad (a k x 1 kernel: only the row axis is padded)."""
    core = _core()
    g = torch.Generator().manual_seed(k * 10 + s)
    sq = du._SameConv(1, 1, k, s, bias=False).double()
    r = du._SameConv(1, 1, (k, 1), (s, 1), bias=False).double()
    with torch.no_grad():
        r.weight.copy_(torch.randn(r.weight.shape, generator=g, dtype=torch.float64))
        for n in range(5, 226):
            o, front, back = core.same_pad(n, k, s)
            assert sq(torch.zeros(1, 1, n, n, dtype=torch.float64)).shape[2:] == (o, o), (n, k, s)
            x = torch.randn(1, 1, n, 3, generator=g, dtype=torch.float64)
            ref = r(x)
            got = F.conv2d(F.pad(x, [0, 0, front, back]), r.weight, None, (s, 1))
            assert ref.shape[2] == o and torch.equal(ref, got), (n, k, s)
            assert core.dwconv_tiles(o, o) == (-(-o // 8)) ** 2
    assert core.same_pad(112, 3, 2) == (56, 0, 1)               # stride 2 is asymmetric: 0 on top, 1 at the bottom
    assert core.same_pad(224, 3, 2) == (112, 0, 1) and core.same_pad(57, 5, 2) == (29, 2, 2)


def test_route_fallbacks(du, monkeypatch):
    core = _core()
    monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    monkeypatch.setattr(du, "HIP_MBCONV", True)
    blk = du._MBConv(24, 24, 3, 1, 6).eval()
    tower = du.EfficientNetB5Tower().eval()
    x = _nhwc_input(24)
    img = torch.randn(2, 3, 40, 36).as_subclass(_FakeCuda)
    with torch.no_grad():
        assert du.mbconv_route(blk, x) == "hip"
        assert du.mbconv_route(tower, img) == "hip"
        # a CPU tensor
        assert du.mbconv_route(blk, x.as_subclass(torch.Tensor)) == "aten"
        assert du.mbconv_route(tower, img.as_subclass(torch.Tensor)) == "aten"
        # not channels_last for a block / not NCHW-contiguous for the tower, not fp32, wrong width
        assert du.mbconv_route(blk, x.contiguous()) == "aten"
        assert du.mbconv_route(tower, img.contiguous(memory_format=torch.channels_last)) == "aten"
        assert du.mbconv_route(blk, x.double()) == "aten"
        assert du.mbconv_route(blk, _nhwc_input(20)) == "aten"
        # training mode
        blk.train()
        assert du.mbconv_route(blk, x) == "aten"
        blk.eval()
        tower.train()
        assert du.mbconv_route(tower, img) == "aten"
        tower.eval()
        # HIP_MBCONV off
        monkeypatch.setattr(du, "HIP_MBCONV", False)
        assert du.mbconv_route(blk, x) == "aten" and du.mbconv_route(tower, img) == "aten"
        monkeypatch.setattr(du, "HIP_MBCONV", True)
        # no hipBLASLt companion
        monkeypatch.setattr(core, "linear_residual_available", lambda: False)
        assert du.mbconv_route(blk, x) == "aten"
        monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    # grad enabled
    with torch.enable_grad():
        assert du.mbconv_route(blk, x) == "aten" and du.mbconv_route(tower, img) == "aten"
    with torch.no_grad():
        # a hook on any submodule the route skips (forward or pre-hook); hooks on the block itself are fine
        for name in du._MBCONV_SKIPPED:
            h = getattr(blk, name).register_forward_hook(lambda m, i, o: None)
            assert du.mbconv_route(blk, x) == "aten", name
            h.remove()
        h = blk._depthwise_conv.register_forward_pre_hook(lambda m, i: None)
        assert du.mbconv_route(blk, x) == "aten"
        h.remove()
        for name in du._TOWER_SKIPPED:
            h = getattr(tower, name).register_forward_hook(lambda m, i, o: None)
            assert du.mbconv_route(tower, img) == "aten", name
            h.remove()
        h = blk.register_forward_hook(lambda m, i, o: None)
        assert du.mbconv_route(blk, x) == "hip"
        h.remove()
        # a global module hook
        h = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
        try:
            assert du.mbconv_route(blk, x) == "aten"
        finally:
            h.remove()
        assert du.mbconv_route(blk, x) == "hip"
        # a block without expansion (stage 1) and the stage-1 widths
        assert du.mbconv_route(du._MBConv(48, 24, 3, 1, 1).eval(), _nhwc_input(48)) == "hip"


def test_block_modules_and_state_dict_unchanged(du):
    """The route adds plain attributes only: the module tree and state_dict keys are the reference's."""
    blk = du._MBConv(24, 40, 5, 2, 6)
    assert [n for n, _ in blk.named_children()] == ["_expand_conv", "_bn0", "_depthwise_conv", "_bn1", "_se_reduce",
                                                     "_se_expand", "_project_conv", "_bn2"]
    assert (blk.cin, blk.mid, blk.cout, blk.k, blk.s) == (24, 144, 40, 5, 2)
    t = du.EfficientNetB5Tower()
    assert all(not k.startswith("_mbconv") for k in t.state_dict())


# ---- argument checks of the C entries (no device call happens on a rejected call) ------------------------------
E_ARG, E_UNS = -1, -5


def test_entries_reject_bad_arguments(mcd):
    s = None
    # K12 mcd_conv_stem_nhwc(x, B, Cin, H, W, w, bias, Cout, y, stream)
    assert _rc(mcd, "mcd_conv_stem_nhwc", NULL, 2, 3, 8, 8, P, P, 48, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv_stem_nhwc", P, 2, 3, 8, 8, P, P, 46, P, s) == E_ARG              # Cout % 4
    assert _rc(mcd, "mcd_conv_stem_nhwc", P, 2, 5, 8, 8, P, P, 48, P, s) == E_ARG              # Cin > 4
    assert _rc(mcd, "mcd_conv_stem_nhwc", P, -1, 3, 8, 8, P, P, 48, P, s) == E_ARG
    assert _rc(mcd, "mcd_conv_stem_nhwc", P, 2, 3, 8, 8, P + 4, P, 48, P, s) == E_ARG          # alignment
    assert _rc(mcd, "mcd_conv_stem_nhwc", P, 2, 3, 40000, 40000, P, P, 48, P, s) == E_UNS      # one image >= 2^31 B
    # K13 mcd_dwconv_bn_silu(x, B, H, W, C, w, bias, k, stride, silu_in, y, psum, T, stream)
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 16, 16, 24, P, P, 3, 1, 1, NULL, P, 4, s) == E_ARG
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 16, 16, 26, P, P, 3, 1, 1, P, P, 4, s) == E_ARG      # C % 4
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 0, 16, 24, P, P, 3, 1, 1, P, P, 4, s) == E_ARG       # H = 0
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 16, 16, 24, P, P, 3, 1, 1, P, P, 5, s) == E_ARG      # T != 2 x 2
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 16, 16, 24, P, P, 7, 1, 1, P, P, 4, s) == E_UNS      # k
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 16, 16, 24, P, P, 3, 3, 1, P, P, 4, s) == E_UNS      # stride
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 16, 16, 24, P + 8, P, 3, 1, 1, P, P, 4, s) == E_ARG  # alignment
    assert _rc(mcd, "mcd_dwconv_bn_silu", P, 2, 8192, 8192, 8, P, P, 3, 1, 1, P, P, 1024 * 1024, s) == E_UNS
    # K14 mcd_se_gate(psum, B, T, C, HW, w_r, b_r, sq, w_e, b_e, s, stream)
    assert _rc(mcd, "mcd_se_gate", P, 2, 4, 24, 256, P, P, 6, P, P, NULL, s) == E_ARG
    assert _rc(mcd, "mcd_se_gate", P, 2, 4, 22, 256, P, P, 6, P, P, P, s) == E_ARG                   # C % 4
    assert _rc(mcd, "mcd_se_gate", P, 2, 4, 24, 256, P, P, 0, P, P, P, s) == E_ARG                   # sq = 0
    assert _rc(mcd, "mcd_se_gate", P, 2, 0, 24, 256, P, P, 6, P, P, P, s) == E_ARG                   # T = 0
    assert _rc(mcd, "mcd_se_gate", P, 2, 4, 16384, 256, P, P, 6, P, P, P, s) == E_UNS                # C + sq
    # K15 mcd_channel_scale(y, B, HW, C, s, stream)
    assert _rc(mcd, "mcd_channel_scale", NULL, 2, 49, 24, P, s) == E_ARG
    assert _rc(mcd, "mcd_channel_scale", P, 2, 49, 26, P, s) == E_ARG                               # C % 4
    assert _rc(mcd, "mcd_channel_scale", P, 2, 0, 24, P, s) == E_ARG
    assert _rc(mcd, "mcd_channel_scale", P + 4, 2, 49, 24, P, s) == E_ARG                           # alignment
    assert _rc(mcd, "mcd_channel_scale", P, 2, 1 << 28, 8, P, s) == E_UNS
    # K0n mcd_hook_pool_nhwc(x, B, C, HW, mode, dst, row0, col0, stride_n, stride_u, stream)
    assert _rc(mcd, "mcd_hook_pool_nhwc", NULL, 2, 24, 49, 0, P, 0, 0, 24, 1, s) == E_ARG
    assert _rc(mcd, "mcd_hook_pool_nhwc", P, 2, 0, 49, 0, P, 0, 0, 24, 1, s) == E_ARG
    assert _rc(mcd, "mcd_hook_pool_nhwc", P, 2, 24, 49, 2, P, 0, 0, 24, 1, s) == E_ARG              # CLS: not a pooling
    assert _rc(mcd, "mcd_hook_pool_nhwc", P, 2, 24, 49, 5, P, 0, 0, 24, 1, s) == E_ARG
    assert _rc(mcd, "mcd_hook_pool_nhwc", P, 2, 1 << 20, 1 << 10, 0, P, 0, 0, 24, 1, s) == E_UNS
    # MCD_POOL_SILU_AVG is K0n's only: mcd_hook_pool keeps rejecting it
    assert _rc(mcd, "mcd_hook_pool", P, 2, 24, 49, 4, P, 0, 0, 24, 1, s) == E_ARG
    assert b"bad mode" in mcd._lib.load().mcd_last_error()


def test_header_declares_the_new_entries():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "mcd_hip.h")).read()
    for name in ("mcd_conv_stem_nhwc", "mcd_dwconv_bn_silu", "mcd_se_gate", "mcd_channel_scale", "mcd_hook_pool_nhwc"):
        assert "int %s(" % name in h
    assert "MCD_POOL_SILU_AVG = 4" in h and "efficientnet_custom.py:109-115" in h
