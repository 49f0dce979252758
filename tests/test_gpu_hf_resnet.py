"""GPU: the 7x7 / 2 stem with its epilogue (mcd_conv7x7s2_bias_relu_nhwc, include/mcd_stem.h) and the HIP route of
data_utils.HFResNet and of Mammo-CLIP's ResNet image tower.

The entry through the C ABI on framed, pre-filled operands against float64 conv2d + bias (+ ReLU) with ATen's fp32 result on
the same input as the measure; its equality with K16 under a zero bias; its independence of batch neighbours; the stream and
capture contracts with test_gpu_stream_contracts' machinery; K17 as a plain max pooling.  Then both models of the fixture
(tests/golden/hf_resnet.npz, what the installed transformers computed) on both routes against the float64 forward of the same
module, the launches by counted calls, the wrapped torchvision tower, and one describe_og_neurons run on a registered
checkpoint.  The bound is the project's for a HIP kernel on its ATen route: error against float64 at most twice ATen's on
the same input, plus 1e-6 (test_gpu_text_tower._bound); both errors are printed."""
import copy
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hf_resnet_recipe as recipe
import openai_clip_recipe as openai_recipe
import test_gpu_encoder_frames as EF
import test_gpu_stream_contracts as S
import test_gpu_text_tower as TT
import util
from test_gpu_text_tower import spin_cycles  # noqa: F401  (the fixture)
from util import int_bits, nerr

pytestmark = pytest.mark.gpu

_bound = TT._bound                      # e <= 2 * (ATen's error against float64) + 1e-6
FILL_BITS = int(int_bits(torch.full((1,), util.OUT_FILL))[0])
ENTRY = "mcd_conv7x7s2_bias_relu_nhwc"


@pytest.fixture(scope="module")
def L(mcd, dev):
    return mcd._lib.load()


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return (np.load(os.path.join(util.GOLDEN, "hf_resnet.npz")),
            json.load(open(os.path.join(util.GOLDEN, "hf_resnet_meta.json"))))


def out_hw(n):
    return (n + 6 - 7) // 2 + 1


# ---- the entry ----------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 9), (16, 16), (17, 33), (37, 29)]       # one pixel; one tile; tile tails both ways; odd sizes


def stem_inputs(dev, B, Cin, Cout, H, W):
    seed = 9000 + 1000 * Cin + 10 * Cout + H
    x = EF.rnd((B, Cin, H, W), seed, dev)
    w = EF.rnd((Cin, 7, 7, Cout), seed + 1, dev, (2.0 / (49 * Cin)) ** 0.5)          # tap-major
    bias = EF.rnd((Cout,), seed + 2, dev, 0.5)
    return x, w, bias


def stem(L, x, w, bias, relu):
    """The entry on framed operands, one run per gap fill; every output element written; returns [B, Ho, Wo, Cout]."""
    B, Cin, H, W = x.shape
    Cout = w.shape[-1]
    shape = (B, out_hw(H), out_hw(W), Cout)
    dense = torch.full(shape, util.OUT_FILL, device=x.device)
    EF.ok(L.mcd_conv7x7s2_bias_relu_nhwc(x.data_ptr(), B, Cin, H, W, w.data_ptr(), bias.data_ptr(), Cout, relu,
                                         dense.data_ptr(), EF.st()), L)
    torch.cuda.synchronize()
    assert not bool((int_bits(dense) == FILL_BITS).any()), "an output element was not written"
    EF.run_framed(L, lambda i, o: L.mcd_conv7x7s2_bias_relu_nhwc(i[0], B, Cin, H, W, i[1], i[2], Cout, relu, o[0], EF.st()),
                  [x, w, bias], [shape], (ENTRY, tuple(x.shape), Cout, relu), expect=[dense.view(-1)])
    return dense


def conv64(x, w, bias, relu):
    y = F.conv2d(x.double().cpu(), w.double().cpu().permute(3, 0, 1, 2), bias.double().cpu(), 2, 3)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


def conv_aten(x, w, bias, relu):
    y = F.conv2d(x, w.permute(3, 0, 1, 2).contiguous(), bias, 2, 3)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("Cout", [4, 32, 36, 64])
@pytest.mark.parametrize("Cin", [1, 3])
def test_entry_against_float64(L, core, dev, Cin, Cout, size):
    H, W = size
    x3, w, bias = stem_inputs(dev, 3, Cin, Cout, H, W)
    for B in (1, 3):
        x = x3[:B].contiguous()
        for relu in (0, 1):
            got = stem(L, x, w, bias, relu)
            ref = conv64(x, w, bias, relu)
            assert tuple(got.shape) == tuple(ref.shape)
            _bound(nerr(got, ref), nerr(conv_aten(x, w, bias, relu), ref), (ENTRY, Cin, Cout, size, B, relu))
            if relu:
                assert float(got.min()) >= 0.0
            assert torch.equal(int_bits(core.conv7x7s2_bias_relu_nhwc(x, w, bias, relu=bool(relu))), int_bits(got))
    # an image's bits depend neither on its batch nor on its place in it
    whole = stem(L, x3, w, bias, 1)
    for b in range(3):
        alone = stem(L, x3[b:b + 1].contiguous(), w, bias, 1)
        assert torch.equal(int_bits(alone[0]), int_bits(whole[b])), b
    # bias = 0, relu = 0: K16's values (a -0 may come back as +0: the epilogue adds +0)
    raw = stem(L, x3, w, torch.zeros_like(bias), 0)
    assert torch.equal(raw, core.conv7x7s2_nhwc(x3, w))


def b_stem(L, dev):
    B, Cin, H, W, Cout = 2, 3, 17, 33, 36
    return S.simple(L, dev, "stem7", [S._gen((B, Cin, H, W)), S._gen((Cin, 7, 7, Cout), 0.1), S._gen((Cout,), 0.5)],
                    [(B, out_hw(H), out_hw(W), Cout)],
                    lambda i, o, st: L.mcd_conv7x7s2_bias_relu_nhwc(i[0], B, Cin, H, W, i[1], i[2], Cout, 1, o[0], st))


def test_stream_rows_cover_the_header(mcd):
    assert sorted(mcd._lib.STEM_SIGNATURES) == [ENTRY]


def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles):  # noqa: F811
    r = S.Run(ENTRY, b_stem(L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, ENTRY)


def test_capture_and_replay(L, dev):
    """The entry alone in a captured graph (one kernel node: no parallel branches), replayed on fresh data to the eager bits."""
    r = S.Run(ENTRY, b_stem(L, dev), dev)
    data = [r.stage(3003), r.stage(4004)]
    want = [r.eager(d) for d in data]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert r.call(st.cuda_stream) == 0               # the warm-up on the stream
    st.synchronize()
    r.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=st):
            rc = r.call(torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert r.untouched(), "the call ran during the capture"
        for d, w in zip(data, want):
            r.poison()
            r.refill(d)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            r.same(r.outs, w, ENTRY)
    finally:
        g.reset()


@pytest.mark.parametrize("size", [(16, 20), (17, 13)], ids=lambda s: "%dx%d" % s)
def test_k17_with_unit_affine_is_the_max_pooling(core, dev, size):
    H, W = size
    x = F.relu(EF.rnd((3, H, W, 32), 9500 + H, dev))
    got = core.bn_relu_maxpool_nhwc(x, torch.ones(32, device=dev), torch.zeros(32, device=dev))
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(want.shape) and torch.equal(got, want)


# ---- the models ---------------------------------------------------------------------------------------------------------
_MODELS = {}


def models_of(du, dev, name):
    """(the mirror on the GPU, its float64 copy on the host) on the recipe's weights; built once, left unchanged."""
    if name not in _MODELS:
        sd, _ = recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])
        cpu = du.HFResNet.from_state_dict(sd).eval()
        _MODELS[name] = (copy.deepcopy(cpu).to(dev), cpu.double())
    return _MODELS[name]


def hooked_run(model, names, image):
    got, hooks = {}, []
    for name in names:
        hooks.append(model.get_submodule(name).register_forward_hook(
            lambda m, a, o, name=name: got.__setitem__(name, o.detach().clone())))
    try:
        with torch.no_grad():
            got["logits"] = model(image).detach().clone()
    finally:
        for h in hooks:
            h.remove()
    return got


def hook_points(cfg):
    """What a dissection hooks: the fixture's modules, the first layer of every stage, the pooler and the classifier."""
    return (recipe.hook_names(cfg) + ["resnet.encoder.stages.%d.layers.0" % i for i in range(len(cfg["depths"]))]
            + ["resnet.pooler", "classifier"])


# launches of one forward on the HIP route: (the stem entry, K17, K18, library GEMMs, of them with the ReLU epilogue)
#   bottleneck, depths [2, 1]: a 3x3 per layer and the 1x1 / 2 shortcut of stage 1; conv1 and conv3 per layer and the
#   stride-1 shortcut of stage 0 as GEMMs.  basic: two 3x3 per layer and the 1x1 / 2 shortcut of stage 1, no GEMM.
LAUNCHES = {"bottleneck": (1, 1, 4, 7, 3), "basic": (1, 1, 7, 0, 0)}
WRAPPERS = ("conv7x7s2_bias_relu_nhwc", "conv7x7s2_nhwc", "bn_relu_maxpool_nhwc", "conv_igemm_nhwc", "linear_residual")


def count_convs(monkeypatch):
    n, real = [0], F.conv2d

    def conv2d(*a, **kw):
        n[0] += 1
        return real(*a, **kw)
    monkeypatch.setattr(F, "conv2d", conv2d)
    return n


def counts_of(cnt):
    return tuple(cnt.n.get(k, 0) for k in ("conv7x7s2_bias_relu_nhwc", "bn_relu_maxpool_nhwc", "conv_igemm_nhwc",
                                           "linear_residual")) + (cnt.relu_gemms,)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", [(32, 40), (37, 29)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_models_on_both_routes_against_float64(du, core, dev, monkeypatch, name, size, B):
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    cfg = recipe.CONFIGS[name]
    gpu, f64 = models_of(du, dev, name)
    names = hook_points(cfg)
    image = recipe.make_image(name, B, *size)
    ref = hooked_run(f64, names, image.double())
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    convs = count_convs(monkeypatch)
    hip = hooked_run(gpu, names, image.to(dev))
    assert counts_of(cnt) == LAUNCHES[name] and convs[0] == 0 and "conv7x7s2_nhwc" not in cnt.n
    again = hooked_run(gpu, names, image.to(dev))
    monkeypatch.setattr(du, "HIP_RESNET", False)
    aten = hooked_run(gpu, names, image.to(dev))
    assert counts_of(cnt) == tuple(2 * v for v in LAUNCHES[name]) and convs[0] > 0          # ATen called none of them
    for k in names + ["logits"]:
        assert tuple(hip[k].shape) == tuple(ref[k].shape) == tuple(aten[k].shape), k
        _bound(nerr(hip[k], ref[k]), nerr(aten[k], ref[k]), (name, size, B, k))
        assert torch.equal(int_bits(hip[k].contiguous()), int_bits(again[k].contiguous())), k
    assert tuple(hip["logits"].shape) == (B, cfg["num_labels"])
    assert tuple(hip["resnet.pooler"].shape) == (B, cfg["hidden_sizes"][-1], 1, 1)


@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_models_meet_the_transformers_fixture(du, fixture, dev, monkeypatch, name):
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    z, meta = fixture
    cfg = recipe.CONFIGS[name]
    gpu, _ = models_of(du, dev, name)
    image = recipe.make_image(name)
    assert recipe.sha256(image) == meta[name + "_image_sha256"]
    with torch.no_grad():
        assert du.hf_resnet_route(gpu.resnet.embedder, image.to(dev)) == "hip"
    got = hooked_run(gpu, recipe.hook_names(cfg), image.to(dev))
    for k in recipe.hook_names(cfg) + ["logits"]:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        assert tuple(got[k].shape) == tuple(f64.shape), k
        _bound(nerr(got[k], f64), nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64), (name, "transformers", k))


@pytest.mark.parametrize("name,inner,fell", [("bottleneck", "resnet.encoder.stages.0.layers.0.layer.1.convolution", 4),
                                            ("basic", "resnet.encoder.stages.1.layers.0.layer.0.convolution", 3)])
def test_a_hook_inside_a_layer_sends_that_layer_alone_to_aten(du, core, dev, monkeypatch, name, inner, fell):
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    cfg = recipe.CONFIGS[name]
    gpu, f64 = models_of(du, dev, name)
    names = hook_points(cfg) + [inner]
    image = recipe.make_image(name, 3, 37, 29)
    ref = hooked_run(f64, names, image.double())
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    convs = count_convs(monkeypatch)
    hip = hooked_run(gpu, names, image.to(dev))
    stem, k17, k18, gemms, relu = LAUNCHES[name]
    # bottleneck stage 0 layer 0: its 3x3, conv1, conv3 and the stride-1 shortcut; basic stage 1 layer 0: two 3x3, the 1x1 / 2
    want = (stem, k17, k18 - 1, gemms - 3, relu - 1) if name == "bottleneck" else (stem, k17, k18 - 3, 0, 0)
    assert counts_of(cnt) == want and convs[0] == fell
    monkeypatch.setattr(du, "HIP_RESNET", False)
    aten = hooked_run(gpu, names, image.to(dev))
    for k in names + ["logits"]:
        _bound(nerr(hip[k], ref[k]), nerr(aten[k], ref[k]), (name, "hooked", k))


# ---- the wrapped torchvision tower ----------------------------------------------------------------------------------------
def test_breastclip_classifier_with_a_resnet_tower(du, core, dev, monkeypatch):
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    torch.manual_seed(21)
    clf = du.BreastClipClassifier(n_class=3, image_tower="resnet", layers=[1, 1, 1, 1]).eval()
    util.mild_bn(clf, 4)
    assert clf.image_encoder.out_dim == 2048 and not hasattr(clf.image_encoder.resnet, "fc")
    plain = du.ResNet(du._Bottleneck, [1, 1, 1, 1], num_classes=None).eval()
    plain.load_state_dict(clf.image_encoder.resnet.state_dict())
    image = torch.randn(2, 3, 64, 48, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        ref = copy.deepcopy(clf).double()(image.double())
    clf, plain = clf.to(dev), plain.to(dev)
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    with torch.no_grad():
        hip = clf(image.to(dev))
        assert cnt.n.get("conv7x7s2_nhwc") == 1 and cnt.n.get("bn_relu_maxpool_nhwc") == 1 and cnt.relu_gemms == 4
        feat = clf.encode_image(image.to(dev))
        assert tuple(feat.shape) == (2, 2048) and torch.equal(int_bits(feat), int_bits(plain(image.to(dev))))
        monkeypatch.setattr(du, "HIP_RESNET", False)
        aten = clf(image.to(dev))
    assert tuple(hip.shape) == (2, 3)
    _bound(nerr(hip, ref), nerr(aten, ref), "BreastClipClassifier(resnet)")


# ---- one driver run -------------------------------------------------------------------------------------------------------
LAYERS = ["resnet.embedder", "resnet.encoder.stages[0]", "resnet.encoder.stages[1]"]
PROBE = "synthetic_24_64"
CONCEPTS = list(openai_recipe.STRINGS[:12])


@pytest.fixture
def registries(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    for name in ("MCD_TARGET_CKPTS", "MCD_CLIP_CKPTS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")


def drive(drv, tmp, tag, dev, concepts):
    act, res = str(tmp / (tag + "_acts")), str(tmp / (tag + "_results"))
    out = drv.main(["--clip_model", "ViT-B/16", "--target_model", "resnet", "--target_layers", ",".join(LAYERS), "--d_probe", PROBE,
                    "--concept_set", str(concepts), "--batch_size", "16", "--device", str(dev), "--activation_dir", act,
                    "--result_dir", res, "--similarity_fn", "cos_similarity"])
    torch.cuda.synchronize()
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    return open(csvs[0], "rb").read()


def test_driver_with_a_registered_resnet_checkpoint(du, core, dev, tmp_path, monkeypatch, registries):
    """describe_og_neurons on the bottleneck fixture's weights as the registered `resnet` checkpoint; the dissector is a small
    OpenAI CLIP from a registered checkpoint (64 x 64 images, as the probe's)."""
    import io
    import pandas as pd
    from mammo_clip_dissect_amd.concept_vit import describe_og_neurons as drv
    sd, _ = recipe.weights(recipe.BOTTLENECK, recipe.SEED["bottleneck"])
    torch.save(sd, str(tmp_path / "hf_resnet.pt"))
    du.register_target_checkpoint("resnet", str(tmp_path / "hf_resnet.pt"))
    dissector = du.OpenAIClip(**openai_recipe.SMALL)
    openai_recipe.fill(dissector, seed=77)
    torch.save(dissector.state_dict(), str(tmp_path / "openai_small.pt"))
    du.register_clip_checkpoint("ViT-B/16", str(tmp_path / "openai_small.pt"))
    du.register_tokenizer("clip", openai_recipe.BPE_SMALL)
    concepts = tmp_path / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    first = drive(drv, tmp_path, "first", dev, concepts)
    assert cnt.n.get("conv7x7s2_bias_relu_nhwc", 0) >= 2 and cnt.n.get("conv7x7s2_nhwc", 0) == 0
    second = drive(drv, tmp_path, "second", dev, concepts)
    assert first == second
    df = pd.read_csv(io.BytesIO(first))
    assert [int((df.layer == layer).sum()) for layer in LAYERS] == [32, 128, 256] and len(df) == 416
