"""CPU: the Swin image tower's mirror (data_utils.SwinTower) against transformers' own SwinModel (tests/golden/swin.npz,
written by tests/golden/make_golden_swin.py from the weights of tests/swin_recipe.py), its checkpoint loader, the factory
names that reach it, the EfficientNet towers sized from a checkpoint (B2) and the route gates as pure functions.

Numerics, the project's rule for a mirror: its distance to the float64 fixture is at most twice the fp32 fixture's own
distance to it, plus 1e-6 (util.nerr: max |difference| / max |reference|)."""
import json
import os

import numpy as np
import pytest
import torch

import swin_recipe as recipe
import util
from util import nerr


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "swin.npz")), json.load(open(os.path.join(util.GOLDEN, "swin_meta.json")))


def tower_of(du, name, meta=None):
    sd, sha = recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])
    if meta is not None:
        assert sha == meta[name + "_weights_sha256"]
    return du.SwinTower.from_state_dict(sd).eval()


def rows_of(tower, image):
    """Token 0 of every block's and stage's output and layernorm's output, as the fixture names them."""
    rows, hooks = {}, []
    for i, stage in enumerate(tower.encoder.layers):
        hooks.append(stage.register_forward_hook(lambda m, a, o, i=i: rows.__setitem__("stage%d" % i, o[:, 0].detach().clone())))
        for j, blk in enumerate(stage.blocks):
            hooks.append(blk.register_forward_hook(
                lambda m, a, o, i=i, j=j: rows.__setitem__("stage%d_block%d" % (i, j), o[:, 0].detach().clone())))
    with torch.no_grad():
        rows["norm"] = tower(image)
    for h in hooks:
        h.remove()
    return rows


def accept(got, z, name, what):
    """Every fixture row of configuration `name`: distance to float64 <= 2 * (the fp32 fixture's) + 1e-6.  Returns them."""
    keys = sorted(k[len(name) + 1:-4] for k in z.files if k.startswith(name + "_") and k.endswith("_f64"))
    assert sorted(got) == keys, (sorted(got), keys)
    dist = {}
    for k in keys:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        e_ref = nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64)
        dist[k] = nerr(got[k], f64)
        print("%s %s %s: %.3e, fixture's fp32 %.3e, ratio to the bound %.3f" % (what, name, k, dist[k], e_ref,
                                                                                 dist[k] / (2 * e_ref + 1e-6)))
        assert tuple(got[k].shape) == tuple(f64.shape), (name, k)
        assert dist[k] <= 2 * e_ref + 1e-6, (what, name, k, dist[k], e_ref)
    return dist


# ---- numerics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "padded"])
def test_mirror_against_the_fixture(du, fixture, name):
    z, meta = fixture
    image = recipe.make_image(name)
    assert recipe.sha256(image) == meta[name + "_image_sha256"]
    tower = tower_of(du, name, meta)
    accept(rows_of(tower, image), z, name, "mirror fp32")
    d64 = accept(rows_of(tower.double(), image.double()), z, name, "mirror fp64")
    assert max(d64.values()) < 1e-12            # the rules themselves: float64 against float64


def test_patch_merging_against_the_fixture(du, fixture):
    z, meta = fixture
    sd, sha = recipe.merge_weights()
    assert sha == meta["merge_weights_sha256"]
    merge = du._SwinPatchMerging(recipe.MERGE["dim"], recipe.EPS).eval()
    merge.load_state_dict(sd, strict=True)
    x = recipe.make_merge_input()
    with torch.no_grad():
        got32, got64 = merge(x, recipe.MERGE["grid"]), merge.double()(x.double(), recipe.MERGE["grid"])
    f64 = torch.from_numpy(z["merge_f64"])
    assert tuple(got32.shape) == tuple(f64.shape) == (recipe.BATCH, 3 * 4, 2 * recipe.MERGE["dim"])
    assert nerr(got32, f64) <= 2 * nerr(torch.from_numpy(z["merge_f32"]), f64) + 1e-6
    assert nerr(got64, f64) < 1e-13


def test_the_fused_operands_through_aten_are_the_modules_attention(du):
    """_window_attend_aten (what a block on the HIP route falls back to for a window K31 does not take) on the fused
    projection's output equals the module path, padding, shift and mask included, in float64."""
    tower = tower_of(du, "padded").double()
    blk = tower.encoder.layers[0].blocks[1]                        # 10 x 10 under window 3, shift 1: padded to 12 x 12
    att = getattr(blk.attention, "self")
    x = torch.randn(2, 100, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        n = blk.layernorm_before(x)
        w, b = att.fused_qkv()
        o = du._window_attend_aten(n @ w.T + b, att.heads, (10, 10), 3, 1, att.relative_position_bias_table, b)
        x1 = x + blk.attention.output(o)
        want = blk(x, (10, 10))
        got = x1 + blk.output(blk.intermediate(blk.layernorm_after(x1)))
    assert nerr(got, want) < 1e-13


def test_the_mask_is_minus_100_on_region_pairs(du):
    m = du.swin_shift_mask(14, 14, 7, 3, torch.float64)
    assert tuple(m.shape) == (4, 49, 49) and set(m.unique().tolist()) == {-100.0, 0.0}
    assert not m[0].any() and m[1].any() and m[2].any() and m[3].any()       # only the interior window is unmasked
    assert du.swin_shift_mask(14, 14, 7, 0, torch.float64) is None
    idx = du.swin_bias_index(7)
    assert idx[0, 0] == 6 * 13 + 6 and idx[0, 48] == 0 and idx[48, 0] == 168 and tuple(idx.shape) == (49, 49)


# ---- loading ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "padded"])
def test_from_state_dict_recovers_the_configuration(du, fixture, name):
    _, meta = fixture
    cfg = recipe.CONFIGS[name]
    tower = tower_of(du, name)
    want = dict(recipe.tower_kwargs(cfg), window=(cfg["window"],) * len(cfg["depths"]))
    assert tower.config == want
    assert sorted([k, list(v.shape)] for k, v in tower.state_dict().items()) == sorted(list(e) for e in meta[name + "_state_dict"])
    assert tower.out_dim == cfg["width"] << (len(cfg["depths"]) - 1)


def test_the_default_is_swin_tiny(du, fixture):
    _, meta = fixture
    tower = du.SwinTower()
    assert tower.out_dim == 768
    assert sorted([k, list(v.shape)] for k, v in tower.state_dict().items()) == sorted(list(e) for e in meta["swin-tiny_state_dict"])
    assert tower.config == dict(recipe.tower_kwargs(recipe.TINY), window=(7,) * 4)
    assert du.SwinTower.config_from_state_dict(tower.state_dict()) == tower.config


def test_a_strict_load_ignores_the_index_buffer_and_nothing_else(du):
    cfg = recipe.CONFIGS["small"]
    sd, _ = recipe.weights(cfg, recipe.SEED["small"])
    plain = du.SwinTower.from_state_dict(sd)
    with_index = dict(sd, **recipe.index_buffers(cfg))
    assert len(with_index) == len(sd) + sum(cfg["depths"])
    tower = du.SwinTower.from_state_dict(with_index)
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), tower.state_dict().values()))
    assert not any("relative_position_index" in k for k in tower.state_dict())
    # transformers' own index is the mirror's index arithmetic
    assert torch.equal(next(iter(recipe.index_buffers(cfg).values())), du.swin_bias_index(cfg["window"]))
    with pytest.raises(RuntimeError):
        du.SwinTower.from_state_dict(dict(sd, stray=torch.zeros(1)))
    missing = dict(sd)
    del missing["encoder.layers.1.blocks.0.output.dense.bias"]
    with pytest.raises(RuntimeError):
        du.SwinTower.from_state_dict(missing)
    half = {k: v.half() for k, v in sd.items()}
    assert du.SwinTower.from_state_dict(half).layernorm.weight.dtype == torch.float32


@pytest.mark.parametrize("key,shape", [("embeddings.position_embeddings", (1, 196, 32)), ("embeddings.mask_token", (1, 1, 32))])
def test_absolute_embeddings_and_mask_tokens_are_refused(du, key, shape):
    sd, _ = recipe.weights(recipe.CONFIGS["small"], recipe.SEED["small"])
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        du.SwinTower.from_state_dict(dict(sd, **{key: torch.zeros(shape)}))


def test_a_grid_under_the_window_is_refused_and_an_equal_one_is_unshifted(du):
    tower = tower_of(du, "small")
    with pytest.raises(ValueError, match="smaller than the window 7"):
        tower(torch.zeros(1, 3, 24, 24))                            # a 6 x 6 grid
    assert du.swin_window_shift(7, 9, 7, 3) == (7, 0) and du.swin_window_shift(8, 9, 7, 3) == (7, 3)
    with torch.no_grad():
        assert tuple(tower(torch.zeros(1, 3, 55, 57)).shape) == (1, 7 * 8, 64)       # pixels padded to whole patches: 14 x 15


# ---- the factory ------------------------------------------------------------------------------------------------------------
def clip_state_dict(du, name):
    """A BreastClip state dict whose image encoder is the recipe's Swin tower under the reference's prefix."""
    cfg = recipe.CONFIGS[name]
    sd, _ = recipe.weights(cfg, recipe.SEED[name])
    out = {du.SWIN_PREFIX + k: v for k, v in dict(sd, **recipe.index_buffers(cfg)).items()}
    out["image_projection.projection.weight"] = torch.full((du.PROJ_DIM, cfg["width"] << (len(cfg["depths"]) - 1)), 0.25)
    return out, sd


def test_breastclip_swin_with_and_without_a_checkpoint(du):
    m, pre = du.get_target_model("breastclip_swin", "cpu")
    assert pre is None and not m.training and isinstance(m, du.BreastClip) and m.model_type == "swin"
    enc = m.image_encoder
    assert isinstance(enc, du.HFImageEncoder) and enc.model_type == "swin" and enc.out_dim == 768
    assert isinstance(enc.image_encoder, du.SwinTower) and enc.image_encoder.config["depths"] == (2, 2, 6, 2)
    assert m.image_projection.projection.in_features == 768
    m2, _ = du.get_target_model("breastclip_swin", "cpu")
    m3, _ = du.get_target_model("breastclip_swin", "cpu", seed=1)
    k = du.SWIN_PREFIX + "encoder.layers.0.blocks.0.attention.self.query.weight"
    assert torch.equal(m.state_dict()[k], m2.state_dict()[k]) and not torch.equal(m.state_dict()[k], m3.state_dict()[k])
    ckpt, sd = clip_state_dict(du, "small")
    for target in ("breastclip_swin", "breastclip"):                # the tower follows the checkpoint's keys
        c, _ = du.get_target_model(target, "cpu", ckpt={"model": ckpt})
        t = c.image_encoder.image_encoder
        assert c.model_type == "swin" and t.config["heads"] == (1, 2) and c.image_encoder.out_dim == 64
        assert all(torch.equal(t.state_dict()[k], v) for k, v in sd.items())
        assert float(c.image_projection.projection.weight.detach()[0, 0]) == 0.25
        image = recipe.make_image("small")
        with torch.no_grad():
            assert torch.equal(c.encode_image(image), t(image)[:, 0])
    clf, _ = du.get_target_model("breastclip_classifier", "cpu", ckpt=ckpt, n_class=3)
    assert clf.model_type == "swin" and clf.classifier.in_features == 64
    with torch.no_grad():
        assert tuple(clf(recipe.make_image("small")).shape) == (recipe.BATCH, 3)
    with pytest.raises(ValueError, match="neither a Swin tower"):
        du.get_target_model("breastclip", "cpu", ckpt={"image_encoder.encoder.layer.0.norm1.weight": torch.zeros(4)})


def b2_state_dict(du):
    torch.manual_seed(11)
    tower = du.EfficientNetTower(width=1.1, depth=1.2)
    assert len(tower._blocks) == 23 and tower._conv_stem.out_channels == 32 and tower.out_dim == 1408
    return {"image_encoder." + k: v.clone() for k, v in tower.state_dict().items()}


def test_a_b2_checkpoint_builds_b2(du):
    sd = b2_state_dict(du)
    assert du.efficientnet_scaling(32, 1408, 23) == ("b2", 1.1, 1.2) and du.efficientnet_scaling(48, 2048, 39)[0] == "b5"
    assert du.efficientnet_scaling(32, 1408, 24) is None
    m, _ = du.get_target_model("breastclip", "cpu", ckpt={"model": sd})
    assert m.image_encoder.out_dim == 1408 and len(m.image_encoder._blocks) == 23
    assert m.image_projection.projection.in_features == 1408
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    c, _ = du.get_target_model("breastclip_classifier", "cpu", ckpt=sd, n_class=4)
    assert c.image_encoder.out_dim == 1408 and c.classifier.in_features == 1408 and c.classifier.out_features == 4
    assert all(torch.equal(c.state_dict()[k], v) for k, v in sd.items())
    # only the fine-tuned file carries the image encoder
    c2, _ = du.get_target_model("breastclip_classifier", "cpu", ckpt={"classifier.bias": torch.zeros(4)}, n_class=4,
                                finetuned_ckpt=sd)
    assert c2.image_encoder.out_dim == 1408 and all(torch.equal(c2.state_dict()[k], v) for k, v in sd.items())
    with torch.no_grad():
        assert tuple(c(torch.zeros(1, 3, 64, 64)).shape) == (1, 4)
    with pytest.raises(ValueError, match="no EfficientNet b0 .. b7"):
        du.get_target_model("breastclip", "cpu", ckpt={"image_encoder._conv_stem.weight": torch.zeros(36, 3, 3, 3)})
    with pytest.raises(ValueError, match="not a Swin tower"):
        du.get_target_model("breastclip_swin", "cpu", ckpt=sd)


# sha256 of image_encoder._conv_stem.weight of the seeded (seed 0) no-checkpoint models, as the parent commit builds them
B5_STEM_SHA = "4b404dd6e6d5f36383614405d6d967c422b43ac5328cf16fa8ab3312c316d3cd"


def test_the_models_without_a_checkpoint_are_b5_as_before(du):
    assert du.EfficientNetTower is du.EfficientNetB5Tower
    torch.manual_seed(0)
    want = du.EfficientNetB5Tower()
    keys = ["image_encoder." + k for k in want.state_dict()]
    for m in (du.get_target_model("breastclip", "cpu")[0], du.get_target_model("breastclip_classifier", "cpu", n_class=2)[0]):
        assert type(m.image_encoder) is du.EfficientNetB5Tower and m.image_encoder.out_dim == 2048
        assert len(m.image_encoder._blocks) == 39
        assert [k for k in m.state_dict() if k.startswith("image_encoder.")] == keys
        assert torch.equal(m.image_encoder._conv_stem.weight, want._conv_stem.weight)
        assert recipe.sha256(m.image_encoder._conv_stem.weight) == B5_STEM_SHA
    assert isinstance(du.get_target_model("breastclip", "cpu")[0].text_encoder, du.TextTower)


def test_unknown_names_stay_unknown(du):
    for name in ("swin", "breastclip_swin_tiny", "breastclip_b2", "mae", "resnet", "vit_b_16"):
        with pytest.raises(ValueError, match="unknown target model.*breastclip_swin.*resnet18, resnet18_places.*resnet152, vit, "
                                             "vit-cub, vit-bloodmnist, dino, dino-cub, dino-bloodmnist"):
            du.get_target_model(name, "cpu")


# ---- the route gates ----------------------------------------------------------------------------------------------------------
def test_swin_route_gates(du):
    f32 = torch.float32
    assert du.swin_route(True, True, f32, False, False, True, 8) == "hip"
    for args in ((False, True, f32, False, False, True, 8),          # MCD_NO_HIP_SWIN=1
                 (True, False, f32, False, False, True, 8),          # a CPU tensor
                 (True, True, torch.float64, False, False, True, 8),
                 (True, True, torch.float16, False, False, True, 8),
                 (True, True, f32, True, False, True, 8),            # autograd records
                 (True, True, f32, False, True, True, 8),            # training mode
                 (True, True, f32, False, False, False, 8),          # no fused-residual path
                 (True, True, f32, False, False, True, 0),
                 (True, True, f32, False, False, True, 65536)):
        assert du.swin_route(*args) == "aten", args
    assert du.swin_attention_route(7, 96, 3, 3136) == "window" and du.swin_attention_route(8, 64, 2, 64) == "window"
    assert du.swin_attention_route(12, 128, 4, 9216) == "window-aten"            # 144 tokens a window
    assert du.swin_attention_route(7, 192, 3, 3136) == "window-aten"             # heads 64 wide
    assert du.swin_attention_route(7, 96, 3, -(-2 ** 31 // (4 * 288))) == "window-aten"      # one image's qkv of 2^31 bytes
    assert du.swin_attention_route(7, 96, 3, -(-2 ** 31 // (4 * 288)) - 1) == "window"
    assert du.swin_merge_route(96, 3136) == "k32" and du.swin_merge_route(512, 49) == "k32"
    assert du.swin_merge_route(768, 144) == "aten" and du.swin_merge_route(6, 4) == "aten"        # Swin-L's last merge; C % 4
    tower = du.SwinTower(width=32, depths=(1,), heads=(1,))
    assert tower.eval().route(torch.zeros(1, 3, 28, 28)) == "aten"               # a CPU tensor never leaves ATen
