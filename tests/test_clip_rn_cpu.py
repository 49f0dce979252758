"""CPU: the host side of the OpenAI-CLIP RN50 / RN101 dissectors and of K19-K21 (mcd_conv3x3s2_nhwc, mcd_avgpool2_nhwc,
mcd_attnpool_tokens): the symbols in the header, the ctypes table and the library; the entries' argument checks by return
code; the module tree against the state-dict key list the reference's ModifiedResNet has (tests/golden/clip_rn_meta.json);
the mirror's CPU forward against the reference's float64 output on the recipe weights (tests/clip_rn_recipe.py), held to
the project's bound with the reference's own fp32 output as the ATen side; the HIP route's data flow restated in float64
(folded weights, tap-major stem weight, pooled skip, cat(k, v) projection, row-0 query) against the modules' float64
forward; clip_rn_route's table; the factory and _clip_dissector.  No kernel runs here."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_rn_recipe as recipe
import util
from util import FakeCuda as _FakeCuda, entry_rc as _rc, nhwc_input as _nhwc_input, randomise_bn as _randomise_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = None
P, Q = 4096, 1 << 20     # non-NULL, 16-byte aligned pointer values, 1 MiB apart, that no rejected call may dereference
E_ARG, E_UNS = -1, -5
K19, K20, K21 = "mcd_conv3x3s2_nhwc", "mcd_avgpool2_nhwc", "mcd_attnpool_tokens"


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(util.GOLDEN, "clip_rn.npz"))
    meta = json.load(open(os.path.join(util.GOLDEN, "clip_rn_meta.json")))
    return z, meta


def _core():
    from mammo_clip_dissect_amd import core
    return core


def _bound(e_got, e_aten, what):
    print("%s: got %.3e aten %.3e ratio to the bound %.3f" % (what, e_got, e_aten, e_got / (2 * e_aten + 1e-6)))
    assert e_got <= 2 * e_aten + 1e-6, (what, e_got, e_aten)


# ---- the symbols --------------------------------------------------------------------------------------------------------
def test_new_symbols_everywhere(mcd):
    h = open(os.path.join(ROOT, "include", "mcd_hip.h")).read()
    L = mcd._lib.load()
    for name in (K19, K20, K21):
        assert "int %s(" % name in h and name in mcd._lib.SIGNATURES and hasattr(L, name), name
    assert L.mcd_abi_version() == 9
    core = _core()
    assert all(callable(getattr(core, n)) for n in ("conv3x3s2_nhwc", "avgpool2_nhwc", "attnpool_tokens"))


# ---- the entries' argument checks ---------------------------------------------------------------------------------------
def test_k19_entry_rejects_bad_arguments(mcd):
    # mcd_conv3x3s2_nhwc(x, B, Cin, H, W, w, bias, Cout, relu, y, stream)
    s = None
    ok = [P, 2, 3, 8, 8, P, P, 32, 1, Q, s]
    for i in (0, 5, 6, 9):                                                 # x, w, bias, y
        a = list(ok)
        a[i] = NULL
        assert _rc(mcd, K19, *a) == E_ARG, i
    for i, bad in ((0, P + 2), (5, P + 4), (6, P + 8), (9, Q + 4)):        # misaligned
        a = list(ok)
        a[i] = bad
        assert _rc(mcd, K19, *a) == E_ARG, i
    assert _rc(mcd, K19, P, 2, 5, 8, 8, P, P, 32, 1, Q, s) == E_ARG        # Cin > 4
    assert _rc(mcd, K19, P, 2, 0, 8, 8, P, P, 32, 1, Q, s) == E_ARG
    assert _rc(mcd, K19, P, 2, 3, 8, 8, P, P, 30, 1, Q, s) == E_ARG        # Cout % 4
    assert _rc(mcd, K19, P, 2, 3, 0, 8, P, P, 32, 1, Q, s) == E_ARG
    assert _rc(mcd, K19, P, 2, 3, 16384, 16384, P, P, 32, 1, Q, s) == E_UNS    # the image: 3 * 2^28 * 4 bytes
    assert _rc(mcd, K19, P, 2, 1, 8192, 8192, P, P, 64, 1, Q, s) == E_UNS      # the output: 2^24 * 64 * 4 bytes
    assert _rc(mcd, K19, P, 65536, 3, 8, 8, P, P, 32, 1, Q, s) == E_UNS
    assert b"65535" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, K19, P, 2, 3, 8, 8, Q, Q, 32, 1, P + 16, s) == E_ARG   # y starts inside x (1 536 bytes)
    assert b"overlap" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, K19, P, 2, 3, 8, 8, Q + 1024, P, 32, 1, Q, s) == E_ARG    # w inside y (2 * 4 * 4 * 32 * 4 = 4 096 bytes)
    assert _rc(mcd, K19, P, 2, 3, 8, 8, P, Q + 4080, 32, 1, Q, s) == E_ARG    # bias starts in y's last 16 bytes
    assert _rc(mcd, K19, P, 0, 3, 8, 8, P, P, 32, 0, Q, s) == 0            # B = 0: nothing to do
    assert _rc(mcd, K19, P, 0, 1, 1, 1, P, P, 4, 0, Q, s) == 0


def test_k20_entry_rejects_bad_arguments(mcd):
    # mcd_avgpool2_nhwc(x, B, H, W, C, y, stream)
    s = None
    assert _rc(mcd, K20, NULL, 2, 8, 8, 32, Q, s) == E_ARG
    assert _rc(mcd, K20, P, 2, 8, 8, 32, NULL, s) == E_ARG
    assert _rc(mcd, K20, P + 4, 2, 8, 8, 32, Q, s) == E_ARG
    assert _rc(mcd, K20, P, 2, 8, 8, 32, Q + 8, s) == E_ARG
    assert _rc(mcd, K20, P, 2, 8, 8, 30, Q, s) == E_ARG                    # C % 4
    assert _rc(mcd, K20, P, 2, 8, 8, 0, Q, s) == E_ARG
    assert _rc(mcd, K20, P, 2, 0, 8, 32, Q, s) == E_ARG
    assert _rc(mcd, K20, P, 2, 8192, 8192, 32, Q, s) == E_UNS              # 2^26 * 32 * 4 bytes
    assert _rc(mcd, K20, P, 65536, 8, 8, 32, Q, s) == E_UNS
    assert b"65535" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, K20, P, 2, 8, 8, 32, P + 4096, s) == E_ARG             # y inside x (16 384 bytes)
    assert b"overlap" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, K20, P, 0, 8, 8, 32, Q, s) == 0                        # B = 0
    assert _rc(mcd, K20, P, 1, 1, 5, 8, Q, s) == 0                         # an empty output: accepted, nothing launched
    assert _rc(mcd, K20, P, 3, 7, 1, 8, Q, s) == 0


def test_k21_entry_rejects_bad_arguments(mcd):
    # mcd_attnpool_tokens(x, B, HW, C, pos, tok, stream)
    s = None
    ok = [P, 2, 49, 64, Q, 2 * Q, s]
    for i in (0, 4, 5):
        a = list(ok)
        a[i] = NULL
        assert _rc(mcd, K21, *a) == E_ARG, i
        a[i] = ok[i] + 4
        assert _rc(mcd, K21, *a) == E_ARG, i
    assert _rc(mcd, K21, P, 2, 49, 62, Q, 2 * Q, s) == E_ARG               # C % 4
    assert _rc(mcd, K21, P, 2, 0, 64, Q, 2 * Q, s) == E_ARG
    assert _rc(mcd, K21, P, 2, 1 << 20, 2048, Q, 2 * Q, s) == E_UNS        # 2^20 * 2^11 * 4 bytes of tokens
    assert _rc(mcd, K21, P, 65536, 49, 64, Q, 2 * Q, s) == E_UNS
    assert b"65535" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, K21, P, 2, 49, 64, Q, P + 256, s) == E_ARG             # tok inside x
    assert _rc(mcd, K21, P, 2, 49, 64, Q, Q + 16, s) == E_ARG              # tok inside pos
    assert b"overlap" in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, K21, P, 0, 49, 64, Q, 2 * Q, s) == 0


def test_wrappers_refuse_host_tensors():
    core = _core()
    with pytest.raises(TypeError, match="GPU only"):
        core.conv3x3s2_nhwc(torch.randn(1, 3, 8, 8), torch.randn(3, 3, 3, 32), torch.zeros(32))
    with pytest.raises(TypeError, match="GPU only"):
        core.avgpool2_nhwc(torch.randn(1, 8, 8, 32))
    with pytest.raises(TypeError, match="GPU only"):
        core.attnpool_tokens(torch.randn(1, 4, 64), torch.randn(5, 64))


# ---- the module tree and the factory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,embed,depths", [("clip_rn50", 1024, [3, 4, 6, 3]), ("clip_rn101", 512, [3, 4, 23, 3])])
def test_factory_names_and_module_tree(du, fixture, name, embed, depths):
    net, pre = du.get_target_model(name, "cpu")
    assert pre is None and not net.training and isinstance(net, du.ClipResNet) and net.embed_dim == embed
    v = net.visual
    assert isinstance(v, du.ModifiedResNet) and v.output_dim == embed
    assert [len(getattr(v, "layer%d" % i)) for i in (1, 2, 3, 4)] == depths
    assert all(isinstance(getattr(v, "layer%d" % i), du._Stage) for i in (1, 2, 3, 4))
    assert v.attnpool.num_heads == 32 and tuple(v.attnpool.positional_embedding.shape) == (50, 2048)
    assert tuple(v.attnpool.c_proj.weight.shape) == (embed, 2048)
    assert tuple(net.text_projection.weight.shape) == (embed, 512)
    assert net.text_model.encoder.layer[0].attn.heads == 8 and net.text_model.out_dim == 512
    assert [n for n, _ in net.named_children()] == ["visual", "text_model", "text_projection"]
    sd = [[k, list(t.shape)] for k, t in v.state_dict().items()]
    if name == "clip_rn50":
        assert sd == fixture[1]["rn50_state_dict"]                         # the reference's keys, shapes and order
        # a local OpenAI state dict's visual.* keys load strictly
        v.load_state_dict({k: torch.zeros(s) for k, s in fixture[1]["rn50_state_dict"]}, strict=True)
    else:       # RN101: the same tree but for layer3's depth and the output width
        want = [e for e in fixture[1]["rn50_state_dict"] if "layer3" not in e[0] and "c_proj" not in e[0]]
        assert [e for e in sd if "layer3" not in e[0] and "c_proj" not in e[0]] == want
        assert len(sd) == len(fixture[1]["rn50_state_dict"]) + 17 * 18       # 17 more blocks: 3 convolutions + 3 batch norms of 5 tensors
    blk = v.layer2[0]
    assert [n for n, _ in blk.named_children()] == ["conv1", "bn1", "conv2", "bn2", "avgpool", "conv3", "bn3", "downsample"]
    assert [n for n, _ in blk.downsample.named_children()] == ["-1", "0", "1"]
    assert blk.conv2.stride == (1, 1) and blk.stride == 2 and v.layer2[1].downsample is None
    # folding registers nothing
    keys = list(v.state_dict())
    du._folded(blk, du._CLIP_BOTTLENECK_SKIPPED, du._ClipBottleneck._fold)
    du._folded(v, du._CLIP_STEM_SKIPPED, du.ModifiedResNet._fold_stem)
    du._folded(v.attnpool, du._ATTNPOOL_SKIPPED, du.AttentionPool2d._fold)
    assert list(v.state_dict()) == keys and not list(blk.buffers(recurse=False))


def test_factory_error_text_and_seed(du):
    with pytest.raises(ValueError, match="unknown target model.*clip_rn50.*clip_rn101"):
        du.get_target_model("clip_rn51", "cpu")
    with pytest.raises(ValueError, match="image_size"):
        du.get_target_model("clip_rn50", "cpu", image_size=(224, 160))
    assert "clip_rn50 / clip_rn101" in du.__doc__
    a = du.get_target_model("clip_rn50", "cpu", seed=3)[0].visual.state_dict()
    b = du.get_target_model("clip_rn50", "cpu", seed=3)[0].visual.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    small = du.get_target_model("clip_rn50", "cpu", image_size=96)[0].visual
    assert tuple(small.attnpool.positional_embedding.shape) == (10, 2048)
    assert isinstance(du.get_target_model("clip", "cpu")[0], du.ClipViT)


def test_clip_dissector_follows_the_clip_name(du):
    from mammo_clip_dissect_amd.concept_vit import CLIP_og_utils, og_utils
    m50, tok = og_utils._clip_dissector("cpu", "RN50")
    assert isinstance(m50, du.ClipResNet) and m50.embed_dim == 1024
    assert tok(["a mass"])["input_ids"].shape[0] == 1
    m101 = og_utils._clip_dissector("cpu", "RN101")[0]
    assert isinstance(m101, du.ClipResNet) and m101.embed_dim == 512 and len(m101.visual.layer3) == 23
    assert isinstance(og_utils._clip_dissector("cpu")[0], du.ClipViT)      # the default is what it was
    for other in ("ViT-B/16", "ViT-B/32", "ViT-L/14", "RN50x4", "RN50x16", "RN50x64"):
        assert og_utils.CLIP_DISSECTORS.get(other, "clip") == "clip"
    assert CLIP_og_utils._clip_dissector is og_utils._clip_dissector
    with torch.no_grad():
        t = m50.encode_text(tok(["a mass", "calcification in the upper outer quadrant"]))
    assert tuple(t.shape) == (2, 1024)


# ---- the mirror's CPU forward against the reference's output ------------------------------------------------------------
def test_cpu_forward_against_the_reference_fixture(du, fixture):
    z, meta = fixture
    assert meta["small_config"] == {k: list(v) if isinstance(v, tuple) else v for k, v in recipe.SMALL.items()}
    net = du.ModifiedResNet(**recipe.SMALL).eval()
    assert [[k, list(t.shape)] for k, t in net.state_dict().items()] == meta["small_state_dict"]
    assert recipe.fill(net) == meta["weights_sha256"]
    x = recipe.make_input()
    assert recipe.sha256(x) == meta["input_sha256"] and np.array_equal(x.numpy(), z["x"])
    assert float(net.layer1[0].bn3.weight.detach().abs().min()) > 0.1
    means = {}
    hs = [getattr(net, n).register_forward_hook(lambda m, i, o, n=n: means.__setitem__(n, o.mean(dim=[2, 3])))
          for n in recipe.LAYERS]
    with torch.no_grad():
        y = net(x)
    for h in hs:
        h.remove()
    assert tuple(y.shape) == (2, 64) and float(np.abs(z["y_f64"]).max()) > 1e-2
    _bound(util.nerr(y, torch.from_numpy(z["y_f64"])), util.nerr(torch.from_numpy(z["y_f32"]), torch.from_numpy(z["y_f64"])),
           "small tower, embedding")
    for n in recipe.LAYERS:
        r64, r32 = torch.from_numpy(z[n + "_mean_f64"]), torch.from_numpy(z[n + "_mean_f32"])
        assert means[n].shape == r64.shape
        _bound(util.nerr(means[n], r64), util.nerr(r32, r64), "small tower, %s mean" % n)


# ---- the HIP route's data flow in float64 -------------------------------------------------------------------------------
def _igemm_conv64(x, w_tap, bias, k, s):
    """What K18 computes, in float64 on the host: x NCHW, w_tap [Cout, k*k*Cin] tap-major then channel."""
    cout, cin = w_tap.shape[0], x.shape[1]
    w = w_tap.view(cout, k, k, cin).permute(0, 3, 1, 2)
    return F.conv2d(x, w, bias, s, 1 if k == 3 else 0)


def _gemm64(x, w, b):
    """A 1x1 convolution as the GEMM over channels-last rows."""
    return F.linear(x.permute(0, 2, 3, 1), w, b).permute(0, 3, 1, 2)


def _close(got, ref, what):
    assert got.shape == ref.shape, what
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), what


@pytest.mark.parametrize("cin,width,stride,hw", [(64, 64, 1, (6, 5)), (256, 64, 1, (6, 5)), (256, 128, 2, (6, 8)),
                                                 (256, 128, 2, (7, 9))])
def test_bottleneck_data_flow_float64(du, cin, width, stride, hw):
    g = torch.Generator().manual_seed(cin + stride)
    blk = du._ClipBottleneck(cin, width, stride).double().eval()
    with torch.no_grad():
        _randomise_bn(blk, g)
        f = blk._fold()
        x = torch.randn(2, cin, *hw, generator=g, dtype=torch.float64)
        h = _gemm64(x, f["w1"], f["b1"])
        _close(h, blk.bn1(blk.conv1(x)), "conv1")
        h = F.relu(_igemm_conv64(F.relu(h), f["w2"], f["b2"], 3, 1))
        xs = x
        if stride == 2:
            h, xs = F.avg_pool2d(h, 2), F.avg_pool2d(x, 2)                 # K20 on conv2's output and on the input
        assert (blk.downsample is None) == (stride == 1 and cin == width * 4)
        res = xs if blk.downsample is None else _gemm64(xs, f["wd"], f["bd"])
        if blk.downsample is not None:
            _close(res, blk.downsample(x), "downsample")
        whole = F.relu(_gemm64(h, f["w3"], f["b3"]) + res)
        ref = blk(x)
        _close(whole, ref, "block")
        assert tuple(ref.shape) == (2, width * 4, hw[0] // stride, hw[1] // stride)
        assert (ref == 0).any() and (ref > 0).any()


def test_stem_data_flow_float64(du):
    g = torch.Generator().manual_seed(9)
    net = du.ModifiedResNet((1, 1, 1, 1), 64, 32, 64, 64).double().eval()
    with torch.no_grad():
        _randomise_bn(net, g)
        f = net._fold_stem()
        x = torch.randn(2, 3, 35, 37, generator=g, dtype=torch.float64)
        assert tuple(f["w1"].shape) == (3, 3, 3, 32) and f["w1"].is_contiguous()      # tap-major [Cin, 3, 3, Cout]
        h = F.relu(F.conv2d(x, f["w1"].permute(3, 0, 1, 2), f["b1"], 2, 1))
        _close(h, F.relu(net.bn1(net.conv1(x))), "conv1")
        h = F.relu(_igemm_conv64(h, f["w2"], f["b2"], 3, 1))
        h = F.relu(_igemm_conv64(h, f["w3"], f["b3"], 3, 1))
        _close(F.avg_pool2d(h, 2), net.stem(x), "stem")


@pytest.mark.parametrize("embed,heads,side,out", [(128, 2, 3, 40), (256, 4, 2, None)])
def test_attention_pool_data_flow_float64(du, embed, heads, side, out):
    g = torch.Generator().manual_seed(embed)
    pool = du.AttentionPool2d(side, embed, heads, out).double().eval()
    with torch.no_grad():
        for p in pool.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / p.shape[-1] ** 0.5)
        x = torch.randn(3, embed, side, side, generator=g, dtype=torch.float64)
        B, T = 3, side * side + 1
        wkv, bkv = pool._fold()
        assert tuple(wkv.shape) == (2 * embed, embed) and tuple(bkv.shape) == (2 * embed,)
        xn = x.permute(0, 2, 3, 1).reshape(B, T - 1, embed)               # the channels-last memory K21 reads
        pos = pool.positional_embedding
        tok = torch.cat([xn.mean(dim=1, keepdim=True) + pos[0], xn + pos[1:]], dim=1)
        kv = F.linear(tok, wkv, bkv).view(B, T, 2, heads, 64)
        q = F.linear(tok[:, 0], pool.q_proj.weight, pool.q_proj.bias).view(B, heads, 64)
        k, v = kv[:, :, 0], kv[:, :, 1]                                    # [B, T, heads, 64]
        p = torch.softmax(torch.einsum("bhd,bthd->bht", q, k) / 8, dim=-1)
        o = torch.einsum("bht,bthd->bhd", p, v).reshape(B, embed)
        got = F.linear(o, pool.c_proj.weight, pool.c_proj.bias)
        ref = pool(x)
        _close(got, ref, "attention pool")
        # and the module is the reference's computation: F.multi_head_attention_forward on (HW+1) N C, read at token 0
        t = x.flatten(2).permute(2, 0, 1)
        t = torch.cat([t.mean(dim=0, keepdim=True), t], dim=0) + pos[:, None, :]
        mha, _ = F.multi_head_attention_forward(
            t, t, t, embed, heads, None, torch.cat([pool.q_proj.bias, pool.k_proj.bias, pool.v_proj.bias]), None, None,
            False, 0.0, pool.c_proj.weight, pool.c_proj.bias, training=False, need_weights=False,
            use_separate_proj_weight=True, q_proj_weight=pool.q_proj.weight, k_proj_weight=pool.k_proj.weight,
            v_proj_weight=pool.v_proj.weight)
        _close(ref, mha[0], "the module against multi_head_attention_forward")
        assert tuple(ref.shape) == (B, out or embed)


# ---- routing ------------------------------------------------------------------------------------------------------------
def test_route_table(du, monkeypatch):
    core = _core()
    monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    monkeypatch.setattr(du, "HIP_CLIP_RN", True)
    net = du.ModifiedResNet((2, 1, 1, 1), 64, 32, 64, 64).eval()
    plain, down, pool = net.layer1[1], net.layer2[0], net.attnpool
    x256 = _nhwc_input(256)
    xpool = _nhwc_input(2048, 2, 2)
    img = torch.randn(2, 3, 64, 64).as_subclass(_FakeCuda)
    with torch.no_grad():
        assert du.clip_rn_route(net, img) == "hip"
        assert du.clip_rn_route(plain, x256) == "hip" and du.clip_rn_route(down, x256) == "hip"
        assert du.clip_rn_route(net.layer1[0], _nhwc_input(64)) == "hip"
        assert du.clip_rn_route(pool, xpool) == "hip"
        assert du.clip_rn_route(torch.nn.Conv2d(3, 8, 3), img) == "aten"  # not a piece of this network
        # flag off
        monkeypatch.setattr(du, "HIP_CLIP_RN", False)
        assert [du.clip_rn_route(m, t) for m, t in ((net, img), (plain, x256), (down, x256), (pool, xpool))] == ["aten"] * 4
        monkeypatch.setattr(du, "HIP_CLIP_RN", True)
        # the other towers' flags do not matter
        monkeypatch.setattr(du, "HIP_RESNET", False)
        assert du.clip_rn_route(plain, x256) == "hip"
        monkeypatch.setattr(du, "HIP_RESNET", True)
        # training mode
        net.train()
        assert [du.clip_rn_route(m, t) for m, t in ((net, img), (plain, x256), (down, x256), (pool, xpool))] == ["aten"] * 4
        net.eval()
        # a host tensor, fp64, NCHW memory to a block or the pool, channels-last memory to the stem, wrong channel counts
        assert du.clip_rn_route(plain, x256.as_subclass(torch.Tensor)) == "aten"
        assert du.clip_rn_route(net, img.as_subclass(torch.Tensor)) == "aten"
        assert du.clip_rn_route(plain, x256.double()) == "aten" and du.clip_rn_route(net, img.double()) == "aten"
        assert du.clip_rn_route(plain, x256.contiguous()) == "aten" and du.clip_rn_route(down, x256.contiguous()) == "aten"
        assert du.clip_rn_route(pool, xpool.contiguous()) == "aten"
        assert du.clip_rn_route(net, img.contiguous(memory_format=torch.channels_last)) == "aten"
        assert du.clip_rn_route(plain, _nhwc_input(128)) == "aten"
        assert du.clip_rn_route(pool, _nhwc_input(1024, 2, 2)) == "aten"
        assert du.clip_rn_route(pool, _nhwc_input(2048, 3, 3)) == "aten"  # 10 tokens, 5 position rows
        assert du.clip_rn_route(net, torch.randn(2, 4, 64, 64).as_subclass(_FakeCuda)) == "aten"
        # a stride-2 block needs 2 x 2 pixels, the stem 2 x 2 in front of its pooling
        assert du.clip_rn_route(down, _nhwc_input(256, 1, 5)) == "aten" and du.clip_rn_route(plain, _nhwc_input(256, 1, 5)) == "hip"
        assert du.clip_rn_route(net, torch.randn(2, 3, 2, 64).as_subclass(_FakeCuda)) == "aten"
        assert du.clip_rn_route(net, torch.randn(2, 3, 3, 5).as_subclass(_FakeCuda)) == "hip"
        # width 80 (RN50x4): out of scope, the stem and the blocks take ATen
        wide = du.ModifiedResNet((1, 1, 1, 1), 640, 40, 64, 80).eval()
        assert du.clip_rn_route(wide, img) == "aten"
        assert du.clip_rn_route(wide.layer1[0], _nhwc_input(80)) == "aten"
        assert du.clip_rn_route(du._ClipBottleneck(64, 48, 1).eval(), _nhwc_input(64)) == "aten"
        # heads that are not 64 wide
        assert du.clip_rn_route(du.AttentionPool2d(2, 2048, 16, 64).eval(), xpool) == "aten"
        # the common gate
        monkeypatch.setattr(core, "linear_residual_available", lambda: False)
        assert [du.clip_rn_route(m, t) for m, t in ((net, img), (plain, x256), (pool, xpool))] == ["aten"] * 3
        monkeypatch.setattr(core, "linear_residual_available", lambda: True)
        # hooks on what the route does not call: that piece only
        h = down.conv2.register_forward_hook(lambda m, i, o: None)
        assert du.clip_rn_route(down, x256) == "aten" and du.clip_rn_route(plain, x256) == "hip"
        assert du.clip_rn_route(net, img) == "hip" and du.clip_rn_route(pool, xpool) == "hip"
        h.remove()
        for name in ("conv1", "bn1", "conv2", "bn2", "avgpool", "conv3", "bn3", "downsample"):
            h = getattr(down, name).register_forward_pre_hook(lambda m, i: None)
            assert du.clip_rn_route(down, x256) == "aten", name
            h.remove()
        h = down.downsample[0].register_forward_hook(lambda m, i, o: None)       # the pooling "-1" inside the downsample
        assert du.clip_rn_route(down, x256) == "aten"
        h.remove()
        for name in ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "avgpool"):
            h = getattr(net, name).register_forward_hook(lambda m, i, o: None)
            assert du.clip_rn_route(net, img) == "aten" and du.clip_rn_route(plain, x256) == "hip", name
            h.remove()
        for name in ("q_proj", "k_proj", "v_proj", "c_proj"):
            h = getattr(pool, name).register_forward_hook(lambda m, i, o: None)
            assert du.clip_rn_route(pool, xpool) == "aten" and du.clip_rn_route(net, img) == "hip", name
            h.remove()
        assert du.clip_rn_route(down, x256) == "hip" and du.clip_rn_route(net, img) == "hip"
        # hooks on the hook points (a stage, a block, the pool) leave the routes alone
        hs = [m.register_forward_hook(lambda m, i, o: None) for m in (net.layer2, down, plain, pool)]
        assert du.clip_rn_route(down, x256) == "hip" and du.clip_rn_route(plain, x256) == "hip"
        assert du.clip_rn_route(pool, xpool) == "hip" and du.clip_rn_route(net, img) == "hip"
        for h in hs:
            h.remove()
    with torch.enable_grad():
        assert du.clip_rn_route(plain, x256) == "aten" and du.clip_rn_route(net, img) == "aten"
        assert du.clip_rn_route(pool, xpool) == "aten"


def test_flag_is_read_from_the_environment():
    """MCD_NO_HIP_CLIP_RN=1 at import switches the route off and nothing else; without it the route is on.  A fresh
    interpreter each: the flag is read once, when data_utils is imported."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import mammo_clip_dissect_amd\n"
            "from mammo_clip_dissect_amd.concept_vit import data_utils as du\n"
            "print(du.HIP_CLIP_RN, du.HIP_RESNET, du.HIP_MBCONV)" % ROOT)
    for value, want in ((None, "True True True"), ("1", "False True True"), ("0", "True True True")):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MCD_NO_HIP_")}
        if value is not None:
            env["MCD_NO_HIP_CLIP_RN"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want, (value, out.stdout)
