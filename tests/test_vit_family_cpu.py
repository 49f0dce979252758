"""CPU: the HF ViT / DINOv2 targets (`vit`, `dino` and their -cub / -bloodmnist names) -- the factory, the hook points by
the reference's eval, the classifier widths, the checkpoint loader on the transformers-4.41.1 key lists of the fixture
(tests/golden/vit_family_meta.json), the small mirrors' CPU forward against transformers' own output (vit_family.npz) held
to the project's bound with transformers' fp32 output as the ATen side, the fused route's algebra restated in float64 (the
LayerScale fold, the embed residual with the interpolated table), the route table and K11's argument checks.  No kernel
runs here."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
import vit_family_recipe as recipe
from util import entry_rc as _rc, nerr as _nerr

P, Q = 4096, 1 << 20     # non-NULL, 16-byte aligned pointer values that no rejected call may dereference
E_ARG, E_UNS = -1, -5
NAMES = {"vit": ("vit", 2), "vit-cub": ("vit", 200), "vit-bloodmnist": ("vit", 8),
         "dino": ("dinov2", 2), "dino-cub": ("dinov2", 200), "dino-bloodmnist": ("dinov2", 8)}


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(util.GOLDEN, "vit_family.npz"))
    meta = json.load(open(os.path.join(util.GOLDEN, "vit_family_meta.json")))
    return z, meta


def _bound(e_got, e_aten, what):
    print("%s: got %.3e aten %.3e ratio to the bound %.3f" % (what, e_got, e_aten, e_got / (2 * e_aten + 1e-6)))
    assert e_got <= 2 * e_aten + 1e-6, (what, e_got, e_aten)


def small_mirror(du, name):
    """The mirror of a small configuration, filled with the recipe's 4.41.1-keyed weights through the loader."""
    kind, cfg = recipe.CONFIGS[name]
    net = (du.HFViT if kind == "vit" else du.HFDinov2)(**recipe.mirror_kwargs(cfg)).eval()
    sd, sha = recipe.weights(kind, cfg)
    assert du._load_local(net, sd) is net
    return net, sha


def cls_rows(net, x):
    """(logits, [layers, B, D] class-token rows of every encoder layer's output) of one forward."""
    rows = []
    hs = [b.register_forward_hook(lambda m, i, o: rows.append(o.detach()[:, 0].clone())) for b in net.tower.encoder.layer]
    with torch.no_grad():
        y = net(x)
    for h in hs:
        h.remove()
    return y, torch.stack(rows)


# ---- the factory --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NAMES))
def test_factory_names_hook_points_and_widths(du, name):
    prefix, width = NAMES[name]
    target_model, preprocess = du.get_target_model(name, "cpu")
    assert preprocess is None and not target_model.training
    for i in (0, 11):
        layer = "%s.encoder.layer[%d]" % (prefix, i)
        m = eval("target_model." + layer)                                  # the reference's way (utils.py:135-136)
        assert isinstance(m, du._Block) and m is getattr(target_model, prefix).encoder.layer[i]
    assert len(getattr(target_model, prefix).encoder.layer) == 12
    emb = getattr(target_model, prefix).embeddings
    assert sorted(k for k, _ in emb.named_parameters()) == ["cls_token", "patch_embeddings.projection.bias",
                                                            "patch_embeddings.projection.weight", "position_embeddings"]
    c = target_model.classifier
    assert (c.out_features, c.in_features) == (width, 768 if prefix == "vit" else 1536)
    P_ = 16 if prefix == "vit" else 14
    assert emb.patch_embeddings.projection.kernel_size == (P_, P_)
    assert emb.position_embeddings.shape == (1, 1 + (224 // P_) ** 2, 768)
    eps = 1e-12 if prefix == "vit" else 1e-6
    blk = getattr(target_model, prefix).encoder.layer[3]
    assert blk.norm1.eps == blk.norm2.eps == getattr(target_model, prefix).layernorm.eps == eps
    assert blk.scaled == (prefix == "dinov2") and hasattr(blk, "layer_scale2") == blk.scaled


def test_factory_n_class_seed_and_unknown_names(du):
    assert du.get_target_model("vit", "cpu", n_class=5)[0].classifier.out_features == 5
    assert du.get_target_model("dino", "cpu", n_class=7)[0].classifier.out_features == 7
    assert du.get_target_model("dino-cub", "cpu", n_class=7)[0].classifier.out_features == 200
    a, b = (du.get_target_model("dino", "cpu", seed=s)[0].dinov2.encoder.layer[0].fc1.weight.detach() for s in (3, 3))
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    for name in ("mae", "resnet", "resnet-cub", "clip-cub", "clip-bloodmnist", "resnet-bloodmnist", "vit_b_16"):
        with pytest.raises(ValueError, match="unknown target model.*resnet152, vit, vit-cub, vit-bloodmnist, dino, "
                                             "dino-cub, dino-bloodmnist"):
            du.get_target_model(name, "cpu")


def test_default_block_and_tower_are_unchanged(du):
    """The new constructor arguments' defaults: the parameters and state-dict keys the plain block and tower had, and
    the fused path's weights are the parameters themselves (nothing folded, nothing cached)."""
    blk = du._Block(128, 2, 512)
    assert list(blk.state_dict()) == [m + "." + l for m in ("norm1", "attn.qkv", "attn.proj", "norm2", "fc1", "fc2")
                                      for l in ("weight", "bias")]
    assert blk.norm1.eps == 1e-12 and not blk.scaled
    wp, bp, w2, b2 = blk._residual_weights()
    assert wp is blk.attn.proj.weight and bp is blk.attn.proj.bias and w2 is blk.fc2.weight and b2 is blk.fc2.bias
    assert "_fold_cache" not in blk.__dict__
    t = du.ViTTower(image_size=32, dim=128, depth=1, heads=2, mlp=256)
    assert list(t.state_dict())[:4] == ["cls_token", "pos_embed", "patch_embed.weight", "patch_embed.bias"]
    assert list(t.state_dict())[-2:] == ["layernorm.weight", "layernorm.bias"] and t.layernorm.eps == 1e-12
    assert t.pos_table(32, 32) is t.pos_embed and t.pos_table(64, 16) is t.pos_embed


# ---- the checkpoint loader ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,target", [("vit_base", "vit"), ("dino_base", "dino")])
def test_base_state_dict_is_the_mapped_reference_key_list(du, fixture, name, target):
    """The 4.41.1 key / shape list of the base configuration, through the loader's mapping, is the factory model's state
    dict (q / k / v concatenated, mask_token dropped); a zero-filled dict of those keys loads into every tensor."""
    _, meta = fixture
    entry = meta["configs"][name]
    assert [[k, list(s)] for k, s in recipe.keys(*recipe.CONFIGS[name])] == entry["state_dict"]
    model, _ = du.get_target_model(target, "cpu")
    zeros = {k: torch.zeros(s) for k, s in entry["state_dict"]}
    mapped = model.convert_state_dict(zeros)
    assert {k: tuple(v.shape) for k, v in mapped.items()} == {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert not any("mask_token" in k or "query" in k for k in mapped)
    assert all(float(v.abs().max()) > 0 for k, v in model.state_dict().items() if k.endswith("projection.weight"))
    model2, _ = du.get_target_model(target, "cpu", ckpt={"model": zeros})
    assert all(float(v.abs().max()) == 0 for v in model2.state_dict().values())
    # a dict saved from the mirror passes through the mapping as it is
    own = model.state_dict()
    again = model.convert_state_dict(own)
    assert list(again) != [] and all(again[k] is own[k] for k in own) and len(again) == len(own)


def test_loader_concatenates_qkv_in_order(du):
    kind, cfg = recipe.CONFIGS["dino_small"]
    sd, _ = recipe.weights(kind, cfg)
    net, _ = small_mirror(du, "dino_small")
    b = "dinov2.encoder.layer.1."
    w = net.state_dict()[b + "attn.qkv.weight"]
    for i, n in enumerate(("query", "key", "value")):
        assert torch.equal(w[128 * i:128 * (i + 1)], sd[b + "attention.attention.%s.weight" % n])
    assert torch.equal(net.state_dict()[b + "layer_scale2.lambda1"], sd[b + "layer_scale2.lambda1"])
    assert torch.equal(net.state_dict()[b + "fc2.bias"], sd[b + "mlp.fc2.bias"])
    half = {k: v for k, v in sd.items() if not k.endswith("attention.attention.key.weight")}
    with pytest.raises(KeyError, match="query, key and value"):
        net.convert_state_dict(half)


# ---- the mirrors against transformers' output -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(recipe.CASES))
def test_small_mirror_cpu_forward_matches_the_fixture(du, fixture, case):
    z, meta = fixture
    name, H, W = recipe.CASES[case]
    net, sha = small_mirror(du, name)
    assert sha == meta["configs"][name]["weights_sha256"]
    x = recipe.make_input(case)
    assert tuple(x.shape) == (recipe.BATCH, 3, H, W) and recipe.sha256(x) == meta["cases"][case]["input_sha256"]
    assert torch.equal(x, recipe.dequantize(z["q_" + case]))
    y64, c64 = torch.from_numpy(z["logits_f64_" + case]), torch.from_numpy(z["cls_f64_" + case])
    y32, c32 = torch.from_numpy(z["logits_f32_" + case]), torch.from_numpy(z["cls_f32_" + case])
    assert float(y64.abs().max()) > 0.1 and c64.shape == (2, recipe.BATCH, 128)
    y, c = cls_rows(net, x)
    _bound(_nerr(y, y64), _nerr(y32, y64), "%s logits" % case)
    for i in range(c64.shape[0]):
        _bound(_nerr(c[i], c64[i]), _nerr(c32[i], c64[i]), "%s layer %d class-token row" % (case, i))
    yd, cd = cls_rows(net.double(), x.double())
    assert _nerr(yd, y64) <= 1e-12 and _nerr(cd, c64) <= 1e-12


# ---- the fused route's algebra in float64 ---------------------------------------------------------------------------------
def test_layer_scale_fold_in_float64(du):
    """x + lambda * (W h + b) as one GEMM on (lambda (.) W, lambda (.) b): the two residual updates of a DINOv2-style
    block restated with the folded weights equal the module's explicit multiplication; the fold registers nothing, is
    cached, and follows an in-place change of lambda."""
    g = torch.Generator().manual_seed(5)
    blk = du._Block(128, 2, 512, eps=1e-6, layer_scale=1.0).double().eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / max(1, p.shape[-1]) ** 0.5)
        blk.layer_scale1.lambda1.copy_(1 + 0.3 * torch.randn(128, generator=g, dtype=torch.float64))
        blk.layer_scale2.lambda1.copy_(1 + 0.3 * torch.randn(128, generator=g, dtype=torch.float64))
    keys = list(blk.state_dict())
    assert "layer_scale1.lambda1" in keys and "layer_scale2.lambda1" in keys and len(keys) == 14
    x = torch.randn(2, 9, 128, generator=g, dtype=torch.float64)

    def folded_forward():
        wp, bp, w2, b2 = blk._residual_weights()
        x1 = x + F.linear(blk.attn.heads_out(blk.norm1(x)), wp, bp)
        return x1 + F.linear(F.gelu(blk.fc1(blk.norm2(x1))), w2, b2), wp
    with torch.no_grad():
        ref = blk(x)
        plain = x + blk.attn(blk.norm1(x))
        plain = plain + blk.fc2(F.gelu(blk.fc1(blk.norm2(plain))))
        got, wp = folded_forward()
        assert _nerr(got, ref) <= 1e-14 and _nerr(plain, ref) > 1e-2       # lambda matters
        assert blk._residual_weights()[0] is wp                              # cached
        assert list(blk.state_dict()) == keys and len(list(blk.parameters())) == 14
        blk.layer_scale1.lambda1.mul_(2.0)
        got2, wp2 = folded_forward()
        assert wp2 is not wp and _nerr(got2, blk(x)) <= 1e-14 and _nerr(got2, ref) > 1e-2


@pytest.mark.parametrize("hw", [(70, 70), (56, 84), (28, 28)])
def test_embed_residual_with_the_interpolated_table_in_float64(du, hw):
    """ViTTower.embed's GEMM form restated in float64 for a patch-14 tower with a 5 x 5 table: K11's rows (a zero row,
    then the patches in (c, dy, dx) order) times the convolution weight, plus the bias, plus the residual operand built
    from the interpolated table, equals convolution + cat + add with that table.  The table is transformers' at 70 x 70
    (untouched) and interpolated otherwise; it is computed once per (H, W)."""
    H, W = hw
    g = torch.Generator().manual_seed(H + W)
    net, _ = small_mirror(du, "dino_small")
    tower = net.dinov2.double()
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    nH, nW = H // 14, W // 14
    with torch.no_grad():
        ref = tower.embed(x)                                                # the ATen path: x is not on the GPU
        pos = tower.pos_table(H, W)
        assert pos.shape == (1, 1 + nH * nW, 128) and tower.pos_table(H, W) is pos
        assert (pos is tower.pos_embed) == (hw == (70, 70))
        assert du.embed_gate(14, H, W, pos.shape[1])
        rows = x.view(2, 3, nH, 14, nW, 14).permute(0, 2, 4, 1, 3, 5).reshape(2, nH * nW, 3 * 14 * 14)
        rows = torch.cat([torch.zeros(2, 1, rows.shape[2], dtype=torch.float64), rows], dim=1)
        res = tower._embed_residual(2, H, W)
        got = res + rows @ tower.patch_embed.weight.view(128, -1).T + tower.patch_embed.bias
        assert tuple(res.shape) == tuple(ref.shape) == (2, 1 + nH * nW, 128)
        assert _nerr(got, ref) <= 1e-14
        assert tower._embed_residual(2, H, W) is res and tower._embed_residual(3, H, W).shape[0] == 3
        if hw != (70, 70):
            # the interpolation itself: bicubic, align_corners=False, the `size=` form, in fp32
            grid = tower.pos_embed[:, 1:].reshape(1, 5, 5, 128).permute(0, 3, 1, 2).float()
            want = F.interpolate(grid, size=(nH, nW), mode="bicubic", align_corners=False).double()
            assert torch.equal(pos[:, 1:], want.permute(0, 2, 3, 1).reshape(1, nH * nW, 128))
            assert torch.equal(pos[:, :1], tower.pos_embed[:, :1])
    assert list(net.state_dict()) == list(small_mirror(du, "dino_small")[0].state_dict())     # nothing registered


# ---- the routes ---------------------------------------------------------------------------------------------------------
def test_route_table(du, monkeypatch):
    f32 = torch.float32
    assert du.attention_route(1 + (224 // 14) ** 2, 768, 12, False, True, f32, False) == "long"      # dino at 224: 257
    assert du.attention_route(1 + (70 // 14) ** 2, 128, 2, False, True, f32, False) == "k9"          # dino at 70: 26
    assert du.attention_route(197, 768, 12, False, True, f32, False) == "k9"                         # vit at 224
    assert du.attention_route(257, 768, 12, False, False, f32, False) == "sdpa"
    # the embed gate: any even patch size
    assert du.embed_gate(14, 224, 224, 257) and du.embed_gate(2, 4, 6, 7) and du.embed_gate(16, 224, 224, 197)
    assert not du.embed_gate(7, 224, 224, 1025) and not du.embed_gate(1, 4, 4, 17) and not du.embed_gate(0, 4, 4, 1)
    assert not du.embed_gate(14, 224, 224, 256) and not du.embed_gate(14, 225, 224, 257)
    assert not du.embed_gate(14, 224, 230, 257)
    # vit asks its tower for the class token only, dino never does
    asked = []
    real = du.ViTTower.forward

    def spy(self, x, cls_only=False):
        asked.append(cls_only)
        return real(self, x, cls_only=cls_only)
    monkeypatch.setattr(du.ViTTower, "forward", spy)
    vit, _ = small_mirror(du, "vit_small")
    dino, _ = small_mirror(du, "dino_small")
    with torch.no_grad():
        vit(recipe.make_input("vit"))
        dino(recipe.make_input("dino70"))
    assert asked == [True, False]
    # ... and what the tower then decides for vit's 197 tokens with the dissection's hooks (token 0 readers) in place
    assert du.cls_tail_route(True, True, False, False, 197, 768, 12, 12, True, True)
    assert not du.cls_tail_route(True, True, False, False, 197, 768, 12, 12, True, False)


def test_k11_entry_argument_checks(mcd):
    # mcd_patchify(x, B, Cin, H, W, P, out, stream): everything below returns before any launch
    for p in (7, 1, 3, 15, 0, -2):
        assert _rc(mcd, "mcd_patchify", P, 1, 3, 210, 210, p, Q, None) == E_UNS, p
    assert "bad shape" in mcd._lib.load().mcd_last_error().decode()
    assert _rc(mcd, "mcd_patchify", P, 1, 3, 224, 230, 14, Q, None) == E_UNS          # W is not a multiple of P
    assert _rc(mcd, "mcd_patchify", P, 1, 3, 230, 224, 14, Q, None) == E_UNS
    assert _rc(mcd, "mcd_patchify", P + 8, 1, 3, 28, 28, 14, Q, None) == E_ARG        # 8-byte aligned x: 16 are asked
    assert _rc(mcd, "mcd_patchify", P, 1, 3, 28, 28, 14, Q + 8, None) == E_ARG
    assert _rc(mcd, "mcd_patchify", None, 1, 3, 28, 28, 14, Q, None) == E_ARG
    assert _rc(mcd, "mcd_patchify", P, 0, 3, 28, 28, 14, Q, None) == 0                # no image: nothing to do
    assert mcd._lib.load().mcd_abi_version() == 9
