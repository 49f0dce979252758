"""CPU: the host side of the HF ResNet targets (data_utils.HFResNet: resnet, resnet-cub, resnet-bloodmnist), the clip-cub /
clip-bloodmnist names, Mammo-CLIP's ResNet image tower and the stem entry of include/mcd_stem.h: the module tree and the
state dict are transformers' own; the configuration is read from a key set; loading is strict; the CPU forward meets the
fixture (tests/golden/hf_resnet.npz, what transformers computes on the recipe's weights); hf_resnet_route's answers; the
factory; image_tower_of and the wrapped tower; the entry's header, ctypes row, export and argument refusals.  No kernel
runs here."""
import json
import os
import re

import numpy as np
import pytest
import torch

import hf_resnet_recipe as recipe
import util
from util import FakeCuda as _FakeCuda, entry_rc as _rc, nerr, nhwc_input as _nhwc_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = None
P = 4096            # a non-NULL, 16-byte aligned pointer value that no rejected call may dereference
E_ARG, E_UNS = -1, -5
ENTRY = "mcd_conv7x7s2_bias_relu_nhwc"


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return (np.load(os.path.join(util.GOLDEN, "hf_resnet.npz")),
            json.load(open(os.path.join(util.GOLDEN, "hf_resnet_meta.json"))))


@pytest.fixture
def no_registry(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_TARGET_CKPTS", raising=False)


def _bound(e_got, e_aten, what):       # test_vit_family_cpu's
    print("%s: got %.3e aten %.3e ratio to the bound %.3f" % (what, e_got, e_aten, e_got / (2 * e_aten + 1e-6)))
    assert e_got <= 2 * e_aten + 1e-6, (what, e_got, e_aten)


_MODELS = {}


def mirror(du, name, meta=None):
    """The mirror of a configuration on the recipe's weights, through the loader; built once, left unchanged."""
    if name not in _MODELS:
        sd, sha = recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])
        if meta is not None:
            assert sha == meta[name + "_weights_sha256"]
        _MODELS[name] = du.HFResNet.from_state_dict(sd).eval()
    return _MODELS[name]


def _weights(name):
    return recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])[0]


# ---- the tree, the keys, the configuration ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_state_dict_is_transformers(du, fixture, name):
    _, meta = fixture
    model = mirror(du, name, meta)
    mine = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert mine == meta[name + "_state_dict"] == [[k, list(s)] for k, s in recipe.keys(recipe.CONFIGS[name])]
    import transformers                                  # its absence is a failure: the fixture comes from it
    live = transformers.ResNetForImageClassification(transformers.ResNetConfig(hidden_act="relu", **recipe.CONFIGS[name]))
    assert mine == [[k, list(v.shape)] for k, v in live.state_dict().items()]
    assert [n for n, _ in model.named_modules()] == [n for n, _ in live.named_modules()]


def test_resnet50_defaults_are_microsofts(du, fixture):
    _, meta = fixture
    model = du.HFResNet()
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == meta["resnet-50_state_dict"]
    assert "resnet.encoder.stages.2.layers.0.layer.1.convolution.weight" in model.state_dict()
    assert model.get_submodule("resnet.encoder.stages")[3] is model.resnet.encoder.stages[3]
    assert model.resnet.encoder.stages[0].layers[0].layer[1].convolution.stride == (1, 1)
    assert model.resnet.encoder.stages[1].layers[0].layer[1].convolution.stride == (2, 2)      # the stride on the 3x3
    assert model.resnet.encoder.stages[1].layers[0].shortcut.convolution.stride == (2, 2)
    assert isinstance(model.resnet.encoder.stages[1].layers[1].shortcut, torch.nn.Identity)
    moved = du.HFResNet(depths=(1, 1), hidden_sizes=(128, 256), downsample_in_bottleneck=True,
                        downsample_in_first_stage=True)
    first = moved.resnet.encoder.stages[0].layers[0]
    assert first.layer[0].convolution.stride == (2, 2) and first.layer[1].convolution.stride == (1, 1)
    assert first.shortcut.convolution.stride == (2, 2)


@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_config_from_the_key_set(du, name):
    sd = _weights(name)
    assert du.hf_resnet_config(sd) == recipe.CONFIGS[name]
    assert du.hf_resnet_config(sd, downsample_in_bottleneck=True)["downsample_in_bottleneck"] is True
    shapes = {k: torch.empty(v.shape, device="meta") for k, v in sd.items()}          # shapes alone decide
    assert du.hf_resnet_config(shapes) == recipe.CONFIGS[name]
    for key in (du.HF_RESNET_KEY, "resnet.encoder.stages.0.layers.0.layer.0.convolution.weight",
                "resnet.encoder.stages.1.layers.0.layer.%d.convolution.weight" % (2 if name == "bottleneck" else 1)):
        with pytest.raises(RuntimeError, match=re.escape(repr(key))):
            du.hf_resnet_config({k: v for k, v in sd.items() if k != key})
    headless = {k: v for k, v in sd.items() if not k.startswith("classifier.")}
    assert "num_labels" not in du.hf_resnet_config(headless)


def test_strict_loading(du):
    sd = _weights("bottleneck")
    gone = "resnet.encoder.stages.1.layers.0.shortcut.normalization.running_var"
    with pytest.raises(RuntimeError, match="1 missing key.*" + re.escape(gone)):
        du.HFResNet.from_state_dict({k: v for k, v in sd.items() if k != gone})
    with pytest.raises(RuntimeError, match="1 unexpected key.*resnet.pooler.weight"):
        du.HFResNet.from_state_dict(dict(sd, **{"resnet.pooler.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        du.HFResNet.from_state_dict(dict(sd, **{"classifier.1.bias": torch.zeros(9)}))
    half = du.HFResNet.from_state_dict({k: (v.half() if v.is_floating_point() else v) for k, v in sd.items()})
    w = half.resnet.embedder.embedder.convolution.weight
    assert w.dtype == torch.float32 and torch.equal(w, sd[du.HF_RESNET_KEY].half().float())
    assert half.resnet.embedder.embedder.normalization.num_batches_tracked.dtype == torch.int64
    # a file without a head keeps a fresh one: n_class outputs, 2 when nobody says (HFClip's rule)
    headless = {k: v for k, v in sd.items() if not k.startswith("classifier.")}
    assert du.HFResNet.from_state_dict(headless).classifier[1].out_features == 2
    assert du.HFResNet.from_state_dict(headless, n_class=11).classifier[1].out_features == 11
    assert du.HFResNet.from_state_dict(sd, n_class=11).classifier[1].out_features == 7          # the file decides


# ---- the CPU forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bottleneck", "basic"])
def test_cpu_forward_meets_the_fixture(du, fixture, name):
    z, meta = fixture
    model, cfg = mirror(du, name, meta), recipe.CONFIGS[name]
    image = recipe.make_image(name)
    assert recipe.sha256(image) == meta[name + "_image_sha256"]
    got, hooks = {}, []
    for hook in recipe.hook_names(cfg):
        hooks.append(model.get_submodule(hook).register_forward_hook(
            lambda m, a, o, hook=hook: got.__setitem__(hook, o.detach().clone())))
    with torch.no_grad():
        got["logits"] = model(image)
        assert torch.equal(model.encode_image(image), got["logits"])
    for h in hooks:
        h.remove()
    assert tuple(got["logits"].shape) == (recipe.BATCH, cfg["num_labels"])
    for k in recipe.hook_names(cfg) + ["logits"]:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        assert tuple(got[k].shape) == tuple(f64.shape), k
        _bound(nerr(got[k], f64), nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64), "%s %s" % (name, k))
    assert float(got["resnet.embedder.embedder"].min()) == 0.0          # behind the ReLU


# ---- the route ------------------------------------------------------------------------------------------------------
def test_route_answers(du, monkeypatch):
    from mammo_clip_dissect_amd import core
    monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    monkeypatch.setattr(du, "HIP_RESNET", True)
    route = du.hf_resnet_route
    net = mirror(du, "bottleneck")
    basic = mirror(du, "basic")
    emb, unit = net.resnet.embedder, net.resnet.embedder.embedder
    l00, l01, l10 = (net.resnet.encoder.stages[0].layers[0], net.resnet.encoder.stages[0].layers[1],
                     net.resnet.encoder.stages[1].layers[0])
    b00, b10 = basic.resnet.encoder.stages[0].layers[0], basic.resnet.encoder.stages[1].layers[0]
    img = torch.randn(2, 3, 40, 36).as_subclass(_FakeCuda)
    x32, x128 = _nhwc_input(32), _nhwc_input(128)
    cases = [(emb, img), (unit, img), (l00, x32), (l01, x128), (l10, x128), (b00, x32), (b10, x32),
             (net.resnet, _nhwc_input(256, 3, 2))]
    with torch.no_grad():
        for m, t in cases:
            assert route(m, t) == "hip", type(m).__name__
        for m, t in cases:                               # a CPU tensor, fp16
            assert route(m, t.as_subclass(torch.Tensor)) == "aten"
            assert route(m, t.half()) == "aten"
        # layouts, widths, modules the route does not know or does not take on their own
        assert route(l00, x32.contiguous()) == "aten" and route(b00, x32.contiguous()) == "aten"
        assert route(unit, img.contiguous(memory_format=torch.channels_last)) == "aten"
        assert route(l01, x32) == "aten"                                                   # not its input width
        assert route(l00.layer[1], x32) == "aten" and route(l00.shortcut, x32) == "aten"
        assert route(net.resnet.encoder, x32) == "aten" and route(net.classifier, x32) == "aten"
        assert route(emb, torch.randn(2, 5, 40, 36).as_subclass(_FakeCuda)) == "aten"
        wide = du.HFResNet(embedding_size=48, hidden_sizes=(192,), depths=(1,)).eval()       # a width of 48
        assert route(wide.resnet.encoder.stages[0].layers[0], _nhwc_input(48)) == "aten"
        assert route(wide.resnet.embedder, img) == "hip"                                   # the stem takes Cout % 4
        thin = du.HFResNet(embedding_size=32, hidden_sizes=(48,), depths=(1,), layer_type="basic").eval()
        assert route(thin.resnet.encoder.stages[0].layers[0], x32) == "aten"
        flat = du.HFResNet(embedding_size=32, hidden_sizes=(64,), depths=(1,), layer_type="basic").eval()
        assert route(flat.resnet.encoder.stages[0].layers[0], x32) == "aten"               # 1x1 / 1 shortcut: not K18's
        # training mode, the flag, the companion library
        for m, t in cases:
            m.train()
            assert route(m, t) == "aten"
            m.eval()
        monkeypatch.setattr(du, "HIP_RESNET", False)
        assert all(route(m, t) == "aten" for m, t in cases)
        monkeypatch.setattr(du, "HIP_RESNET", True)
        monkeypatch.setattr(core, "linear_residual_available", lambda: False)
        assert all(route(m, t) == "aten" for m, t in cases)
        monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    with torch.enable_grad():                            # autograd
        assert all(route(m, t) == "aten" for m, t in cases)
    with torch.no_grad():
        # a hook on layer[1].convolution: that layer takes ATen, its neighbours do not
        h = l00.layer[1].convolution.register_forward_hook(lambda m, i, o: None)
        assert route(l00, x32) == "aten" and route(l01, x128) == "hip" and route(l10, x128) == "hip"
        assert route(emb, img) == "hip" and route(unit, img) == "hip"
        h.remove()
        assert route(l00, x32) == "hip"
        for sub in (l00.shortcut, l00.shortcut.normalization, l00.layer, l00.layer[2].normalization, l00.activation):
            h = sub.register_forward_pre_hook(lambda m, i: None)
            assert route(l00, x32) == "aten"
            h.remove()
        h = b10.layer[0].activation.register_forward_hook(lambda m, i, o: None)
        assert route(b10, x32) == "aten" and route(b00, x32) == "hip"
        h.remove()
        # the hook points of a dissection leave every route alone
        hs = [m.register_forward_hook(lambda m, i, o: None)
              for m in (emb, unit, net.resnet.encoder.stages[0], l00, net.resnet.encoder.stages[1].layers, net.classifier)]
        assert all(route(m, t) == "hip" for m, t in cases if m in (emb, unit, l00, l01, l10, net.resnet))
        for h in hs:
            h.remove()
        # inside the stem unit: the unit takes ATen, the pooling behind it stays; a hooked pooler takes its module
        h = unit.convolution.register_forward_hook(lambda m, i, o: None)
        assert route(unit, img) == "aten" and route(emb, img) == "hip"
        h.remove()
        h = emb.pooler.register_forward_hook(lambda m, i, o: None)
        assert route(emb, img) == "aten" and route(unit, img) == "hip"
        h.remove()
        h = net.resnet.pooler.register_forward_hook(lambda m, i, o: None)
        assert route(net.resnet, _nhwc_input(256, 3, 2)) == "aten"
        h.remove()
        h = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
        try:
            assert all(route(m, t) == "aten" for m, t in cases)
        finally:
            h.remove()
        assert all(route(m, t) == "hip" for m, t in cases)
        # downsample_in_bottleneck: the stride-2 layer is ATen's (its first 1x1 is no GEMM), the others are unchanged
        moved = du.HFResNet(embedding_size=32, hidden_sizes=(128, 256), depths=(2, 2), downsample_in_bottleneck=True).eval()
        s0, s1 = moved.resnet.encoder.stages[0].layers, moved.resnet.encoder.stages[1].layers
        assert route(s0[0], x32) == "hip" and route(s0[1], x128) == "hip"
        assert route(s1[0], x128) == "aten" and route(s1[1], _nhwc_input(256)) == "hip"
    # resnet_route's answers for the classes it knows are what they were; it does not know the new ones
    with torch.no_grad():
        assert du.resnet_route(l00, x32) == "aten" and du.resnet_route(unit, img) == "aten"
        blk = du._Bottleneck(32, 32, 1).eval()
        assert du.resnet_route(blk, x32) == "hip" and route(blk, x32) == "aten"


def test_mammogram_batch_passes_the_route(du, monkeypatch):
    """Mammo-CLIP's 1520 x 912 input: every tensor of one image is far under 2^31 bytes, at the stem and in layer1."""
    from mammo_clip_dissect_amd import core
    monkeypatch.setattr(core, "linear_residual_available", lambda: True)
    monkeypatch.setattr(du, "HIP_RESNET", True)
    tower = du.ResNetImageEncoder([1, 1, 1, 1]).eval()
    img = torch.empty(1, 3, 1520, 912).as_subclass(_FakeCuda)
    with torch.no_grad():
        assert du.resnet_route(tower.resnet, img) == "hip" and du.resnet_route(tower.resnet.conv1, img) == "hip"
        x = torch.empty(1, 64, 380, 228).contiguous(memory_format=torch.channels_last).as_subclass(_FakeCuda)
        assert du.resnet_route(tower.resnet.layer1[0], x) == "hip"
    assert 256 * 380 * 228 * 4 < 2 ** 31                 # layer1's output, the largest tensor of one image


# ---- the factory --------------------------------------------------------------------------------------------------------
RESNET_NAMES = ("resnet", "resnet-cub", "resnet-bloodmnist")
CLIP_NAMES = ("clip-cub", "clip-bloodmnist")


def _clip_sd(du, labels=6):
    torch.manual_seed(5)
    return du.HFClip(num_labels=labels, image_size=32, patch=16, hidden=64, layers=1, heads=1, mlp=128).state_dict()


def test_factory_with_ckpt(du, no_registry):
    sd = _weights("basic")
    for name in RESNET_NAMES:
        model, pre = du.get_target_model(name, "cpu", ckpt=sd, n_class=3)
        assert isinstance(model, du.HFResNet) and pre is None and not model.training
        assert model.classifier[1].out_features == 5                                        # read from the file
        assert torch.equal(model.resnet.embedder.embedder.convolution.weight, sd[du.HF_RESNET_KEY])
    csd = _clip_sd(du)
    for name in CLIP_NAMES:
        model, _ = du.get_target_model(name, "cpu", ckpt=csd)
        assert isinstance(model, du.HFClip) and model.classifier.out_features == 6
        assert torch.equal(model.classifier.weight, csd["classifier.weight"])
    assert du.target_preset("resnet-cub") == du.target_preset("resnet") == du.target_preset("resnet50")


def test_factory_with_registered_files(du, no_registry, tmp_path, monkeypatch):
    sd, csd = _weights("bottleneck"), _clip_sd(du)
    torch.save(sd, str(tmp_path / "resnet.pt"))
    torch.save({"model": csd}, str(tmp_path / "clip.pt"))
    table = {n: str(tmp_path / "resnet.pt") for n in RESNET_NAMES}
    table.update({n: str(tmp_path / "clip.pt") for n in CLIP_NAMES})
    (tmp_path / "table.json").write_text(json.dumps(table))
    monkeypatch.setenv("MCD_TARGET_CKPTS", str(tmp_path / "table.json"))
    for name in RESNET_NAMES:
        model, _ = du.get_target_model(name, "cpu", ckpt=du.target_ckpt_or(name, None))
        assert isinstance(model, du.HFResNet) and model.classifier[1].out_features == 7
        model, _ = du.get_target_model(name, "cpu")                                         # found by the factory itself
        assert torch.equal(model.classifier[1].weight, sd["classifier.1.weight"])
    for name in CLIP_NAMES:
        model, _ = du.get_target_model(name, "cpu")
        assert isinstance(model, du.HFClip) and torch.equal(model.classifier.bias, csd["classifier.bias"])
    # a registered file of the wrong kind: an error, never a random model
    table = {"resnet": str(tmp_path / "clip.pt"), "clip-cub": str(tmp_path / "resnet.pt")}
    (tmp_path / "wrong.json").write_text(json.dumps(table))
    monkeypatch.setenv("MCD_TARGET_CKPTS", str(tmp_path / "wrong.json"))
    with pytest.raises(RuntimeError, match="not a ResNetForImageClassification state dict"):
        du.get_target_model("resnet", "cpu")
    with pytest.raises(RuntimeError, match="not a ResNetForImageClassification state dict"):
        du.get_target_model("resnet", "cpu", ckpt=du.target_ckpt_or("resnet", None))
    with pytest.raises(RuntimeError, match="not a CLIPForImageClassification state dict"):
        du.get_target_model("clip-cub", "cpu")


def test_factory_without_a_checkpoint(du, no_registry):
    for name in RESNET_NAMES + CLIP_NAMES:
        with pytest.raises(ValueError, match="unknown target model.*resnet152, vit, vit-cub, vit-bloodmnist, dino, "
                                             "dino-cub, dino-bloodmnist"):
            du.get_target_model(name, "cpu")
    # a checkpoint of something else does not make the name known
    with pytest.raises(ValueError, match="unknown target model"):
        du.get_target_model("resnet", "cpu", ckpt={"fc.weight": torch.zeros(2, 2)})
    with pytest.raises(ValueError, match="unknown target model"):
        du.get_target_model("clip-cub", "cpu", ckpt={"fc.weight": torch.zeros(2, 2)})


# ---- Mammo-CLIP's ResNet image tower ------------------------------------------------------------------------------------
def _tower_keys(du, layers):
    """The image keys of a Mammo-CLIP checkpoint with the wrapped torchvision ResNet, as shapes (no memory)."""
    with torch.device("meta"):
        net = du.ResNet(du._Bottleneck, layers, num_classes=None)
    return {"image_encoder.resnet." + k: v for k, v in net.state_dict().items()}


def test_image_tower_of(du):
    for layers in ([3, 4, 6, 3], [3, 4, 23, 3], [3, 8, 36, 3]):
        sd = _tower_keys(du, layers)
        assert not any(".fc." in k for k in sd) and "image_encoder.resnet.layer4.2.bn3.weight" in sd
        assert du.image_tower_of(sd) == ("resnet", dict(layers=layers))
    with pytest.raises(ValueError, match=re.escape("[2, 2, 2, 2]")):
        du.image_tower_of(_tower_keys(du, [2, 2, 2, 2]))
    with pytest.raises(ValueError, match="^the checkpoint's image encoder is neither a Swin tower"):
        du.image_tower_of({"image_encoder.features.0.weight": torch.zeros(1)})
    assert du.image_tower_of({"classifier.weight": torch.zeros(1)}) is None
    # without a classifier the plain ResNet is unchanged otherwise; with one it is what it was
    assert list(du.ResNet50().state_dict())[-2:] == ["fc.weight", "fc.bias"]
    assert [n for n, _ in du.ResNet(du._Bottleneck, [1, 1, 1, 1], None).named_children()] == [
        "conv1", "bn1", "layer1", "layer2", "layer3", "layer4"]


def test_breastclip_with_a_resnet_tower(du, no_registry):
    torch.manual_seed(11)
    plain = du.ResNet(du._Bottleneck, [3, 4, 6, 3], num_classes=None).eval()
    util.mild_bn(plain, 7)
    sd = {"image_encoder.resnet." + k: v.clone() for k, v in plain.state_dict().items()}
    sd["classifier.weight"], sd["classifier.bias"] = torch.randn(2, 2048), torch.randn(2)
    clf, _ = du.get_target_model("breastclip_classifier", "cpu", ckpt=sd, n_class=2)
    assert clf.model_type == "resnet" and isinstance(clf.image_encoder, du.ResNetImageEncoder)
    assert clf.image_encoder.out_dim == 2048 and not hasattr(clf.image_encoder.resnet, "fc")
    assert not any(".fc." in k for k in clf.state_dict())
    assert clf.get_submodule("image_encoder.resnet.conv1") is clf.image_encoder.resnet.conv1
    x = torch.randn(1, 3, 64, 48)
    with torch.no_grad():
        feat = plain(x)
        assert tuple(feat.shape) == (1, 2048) and torch.equal(clf.encode_image(x), feat)
        assert torch.equal(clf(x), torch.nn.functional.linear(feat, sd["classifier.weight"], sd["classifier.bias"]))
    # from the fine-tuned file when only that carries an image encoder, as for Swin
    clf2, _ = du.get_target_model("breastclip_classifier", "cpu", ckpt={"classifier.bias": torch.zeros(2)},
                                  finetuned_ckpt=sd, n_class=2)
    assert clf2.model_type == "resnet" and torch.equal(clf2.image_encoder.resnet.conv1.weight, plain.conv1.weight)
    clip, _ = du.get_target_model("breastclip", "cpu", ckpt=sd)
    assert clip.model_type == "resnet" and clip.image_encoder.out_dim == 2048
    with torch.no_grad():
        assert torch.equal(clip.encode_image(x), feat)                    # the pooled features as they are
    # the image keys load strictly
    gone = "image_encoder.resnet.layer3.4.bn2.running_mean"
    with pytest.raises(RuntimeError, match="1 missing key.*" + re.escape(gone)):
        du.get_target_model("breastclip_classifier", "cpu", ckpt={k: v for k, v in sd.items() if k != gone}, n_class=2)
    with pytest.raises(RuntimeError, match="1 unexpected key.*image_encoder.resnet.fc.weight"):
        du.get_target_model("breastclip_classifier", "cpu", n_class=2,
                            ckpt=dict(sd, **{"image_encoder.resnet.fc.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="is a ResNet, not a Swin tower"):
        du.get_target_model("breastclip_swin", "cpu", ckpt=sd)


# ---- the entry of include/mcd_stem.h ------------------------------------------------------------------------------------
def test_stem_entry_header_table_and_export(mcd):
    lib = mcd._lib
    text = open(os.path.join(ROOT, "include", "mcd_stem.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text))) == sorted(lib.STEM_SIGNATURES) == [ENTRY]
    assert lib.STEM_SIGNATURES[ENTRY] == lib.SIGNATURES["mcd_conv3x3s2_nhwc"]              # K19's argument list
    L = lib.load()
    assert hasattr(L, ENTRY) and L.mcd_abi_version() == 9
    assert getattr(L, ENTRY).argtypes == lib.STEM_SIGNATURES[ENTRY][1]
    for other in ("mcd_hip.h", "mcd_blaslt.h"):          # additive: the two old headers do not know it
        assert ENTRY not in open(os.path.join(ROOT, "include", other)).read()
    tables = [lib.SIGNATURES, lib.TEXT_SIGNATURES, lib.CLIP_SIGNATURES, lib.TOKEN_SIGNATURES, lib.SENTENCE_SIGNATURES,
              lib.MASK_SIGNATURES, lib.CACHE_SIGNATURES, lib.CLSFOLD_SIGNATURES, lib.SWIN_SIGNATURES]
    assert not any(ENTRY in t for t in tables)
    from mammo_clip_dissect_amd import core
    assert callable(core.conv7x7s2_bias_relu_nhwc)
    with pytest.raises(TypeError, match="GPU only"):
        core.conv7x7s2_bias_relu_nhwc(torch.randn(1, 3, 8, 8), torch.randn(3, 7, 7, 64), torch.zeros(64))


def test_stem_entry_refusals_are_k19s(mcd):
    """Every refusal of K19, at K19's status code, and no refused call dereferences a pointer (P is no memory at all)."""
    s = None
    calls = [  # (x, B, Cin, H, W, w, bias, Cout, relu, y)
        ((NULL, 2, 3, 8, 8, P, P, 64, 1, P), E_ARG),
        ((P, 2, 3, 8, 8, NULL, P, 64, 1, P), E_ARG),
        ((P, 2, 3, 8, 8, P, NULL, 64, 1, P), E_ARG),                 # the epilogue needs its bias
        ((P, 2, 3, 8, 8, P, P, 64, 1, NULL), E_ARG),
        ((P, 2, 5, 8, 8, P, P, 64, 1, P), E_ARG),                    # Cin = 5
        ((P, 2, 0, 8, 8, P, P, 64, 1, P), E_ARG),
        ((P, 2, 3, 8, 8, P, P, 62, 1, P), E_ARG),                    # Cout % 4
        ((P, 2, 3, 8, 8, P, P, 0, 1, P), E_ARG),
        ((P, -1, 3, 8, 8, P, P, 64, 1, P), E_ARG),
        ((P, 2, 3, 0, 8, P, P, 64, 1, P), E_ARG),
        ((P, 2, 3, 8, 8, P + 4, P, 64, 1, P), E_ARG),                # misaligned w
        ((P, 2, 3, 8, 8, P, P + 8, 64, 1, P), E_ARG),                # misaligned bias
        ((P, 2, 3, 8, 8, P, P, 64, 1, P + 4), E_ARG),                # misaligned y
        ((P + 2, 2, 3, 8, 8, P, P, 64, 1, P), E_ARG),                # x: 4 bytes
        ((P, 2, 3, 8, 8, P + 65536, P + 32768, 64, 1, P + 16), E_ARG),                       # y starts inside x
        ((P, 2, 3, 8, 8, P + 65536 + 1024, P + 32768, 64, 1, P + 65536), E_ARG),             # w inside y
        ((P, 2, 3, 8, 8, P + 131072, P + 65536 + 64, 64, 1, P + 65536), E_ARG),              # bias inside y
        ((P, 2, 3, 40000, 40000, P, P, 64, 1, P), E_UNS),            # one image of x of 2^31 bytes or more
        ((P, 2, 1, 23170, 23171, P, P, 64, 1, P), E_UNS),            # x just over 2^31 bytes
        ((P, 2, 1, 8192, 8192, P, P, 128, 1, P), E_UNS),             # x small, one image of y = 2^31 bytes
        ((P, 65536, 3, 8, 8, P, P, 64, 1, P), E_UNS),
    ]
    for args, want in calls:
        for name in (ENTRY, "mcd_conv3x3s2_nhwc"):
            assert _rc(mcd, name, *args, s) == want, (name, args)
    assert _rc(mcd, ENTRY, P, 2, 3, 8, 8, P + 65536, P + 32768, 64, 1, P + 16, s) == E_ARG
    assert b"overlap" in mcd._lib.load().mcd_last_error() and ENTRY.encode() in mcd._lib.load().mcd_last_error()
    assert _rc(mcd, ENTRY, P, 0, 3, 8, 8, P, P, 64, 1, P, s) == 0                             # B = 0: nothing to do
