"""CPU: data_utils.HFClip (transformers' CLIPForImageClassification under its own names) against the fixture of
tests/golden/hf_clip.npz -- what the installed transformers computed on the recipe's weights (make_golden_hf_clip.py) --
its loader, its selection by a checkpoint in get_target_model, the target-checkpoint registry, the argument checks of K26
(mcd_token_mean) and the ABI surface of include/mcd_tokens.h."""
import json
import os
import re

import numpy as np
import pytest
import torch

import hf_clip_recipe as recipe
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "hf_clip.npz")), json.load(open(os.path.join(util.GOLDEN, "hf_clip_meta.json")))


_MODELS = {}


def mirror(du, name, meta=None):
    """The mirror of a configuration on the recipe's weights, built once and left unchanged."""
    if name not in _MODELS:
        m = du.HFClip(**recipe.CONFIGS[name]).eval()
        sha = recipe.fill(m, recipe.SEED[name])
        if meta is not None:
            assert sha == meta[name + "_weights_sha256"]
        _MODELS[name] = m
    return _MODELS[name]


def state_dict(du, name):
    return {k: v.clone() for k, v in mirror(du, name).state_dict().items()}


def rows_of(model, image):
    """{layer<i>: class-token rows, mean: the classifier's input, logits} of one forward, by hooks on the documented
    hook points."""
    got, hooks = {}, []
    for i, layer in enumerate(model.vision_model.encoder.layers):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: got.__setitem__("layer%d" % i, o[:, 0].detach().clone())))
    hooks.append(model.classifier.register_forward_hook(lambda m, a, o: got.__setitem__("mean", a[0].detach().clone())))
    with torch.no_grad():
        got["logits"] = model(image)
    for h in hooks:
        h.remove()
    return got


# ---- the module tree ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "long", "vit_b16"])
def test_state_dict_keys_and_shapes_are_transformers(du, fixture, name):
    _, meta = fixture
    m = du.HFClip(**recipe.CONFIGS[name])
    assert sorted([k, list(v.shape)] for k, v in m.state_dict().items()) == meta[name + "_state_dict"]


@pytest.mark.parametrize("name", ["small", "long", "vit_b16"])
def test_config_from_state_dict(du, name):
    cfg = recipe.CONFIGS[name]
    sd = du.HFClip(**cfg).state_dict()
    assert du.hf_clip_config(sd) == cfg
    assert du.hf_clip_config(sd, heads=4)["heads"] == 4
    headless = {k: v for k, v in sd.items() if not k.startswith("classifier.")}
    assert du.hf_clip_config(headless) == {k: v for k, v in cfg.items() if k != "num_labels"}
    with pytest.raises(RuntimeError, match="class_embedding"):
        du.hf_clip_config({"classifier.weight": torch.zeros(2, 4)})
    bad = dict(sd)
    bad["vision_model.embeddings.position_embedding.weight"] = torch.zeros(19, cfg["hidden"])
    with pytest.raises(RuntimeError, match="square"):
        du.hf_clip_config(bad)


def test_module_tree_and_hook_points(du):
    m = mirror(du, "small")
    layer = m.vision_model.encoder.layers[1]
    for p in (layer.self_attn.q_proj, layer.self_attn.k_proj, layer.self_attn.v_proj, layer.self_attn.out_proj, layer.mlp.fc1,
              layer.mlp.fc2, m.classifier):
        assert isinstance(p, torch.nn.Linear)
    assert m.vision_model.embeddings.patch_embedding.bias is None
    assert all(ln.eps == 1e-5 for ln in (m.vision_model.pre_layrnorm, m.vision_model.post_layernorm, layer.layer_norm1))
    seen = []
    h = layer.self_attn.q_proj.register_forward_hook(lambda mod, a, o: seen.append(tuple(o.shape)))
    with torch.no_grad():
        out = m(recipe.make_image("small"))
        assert torch.equal(m.encode_image(recipe.make_image("small")), out)
    h.remove()
    assert seen == [(3, 17, 128)] * 2 and tuple(out.shape) == (3, 5)
    with pytest.raises(ValueError, match="doesn't match model"):
        m(torch.zeros(1, 3, 80, 80))
    with pytest.raises(ValueError):
        du.HFClip(hidden_act="relu")


def test_post_layernorm_is_never_applied(du):
    m = du.HFClip(**recipe.SMALL).eval()
    recipe.fill(m, 5)
    image = recipe.make_image("small")
    with torch.no_grad():
        want = m(image)
        m.vision_model.post_layernorm.weight.fill_(float("nan"))
        assert torch.equal(m(image), want)


def test_gelu_variant(du):
    m = du.HFClip(hidden_act="gelu", **recipe.SMALL).eval()
    recipe.fill(m, 5)
    q = du.HFClip(**recipe.SMALL).eval()
    q.load_state_dict(m.state_dict())
    x = torch.randn(2, 17, 128)
    with torch.no_grad():
        assert torch.equal(m.vision_model.encoder.layers[0].mlp.activation_fn(x), torch.nn.functional.gelu(x))
        assert not torch.equal(m(recipe.make_image("small")), q(recipe.make_image("small")))


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "long"])
def test_mirror_against_the_goldens(du, fixture, name):
    z, meta = fixture
    m = mirror(du, name, meta)
    image = recipe.make_image(name)
    assert recipe.sha256(image) == meta[name + "_image_sha256"]
    got32 = rows_of(m, image)
    m64 = du.HFClip(**recipe.CONFIGS[name]).double().eval()
    m64.load_state_dict(m.state_dict())
    got64 = rows_of(m64, image.double())
    keys = ["layer%d" % i for i in range(recipe.CONFIGS[name]["layers"])] + ["mean", "logits"]
    assert sorted(got32) == sorted(keys)
    for k in keys:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        e64 = util.nerr(got64[k], f64)
        e_ref = util.nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64)
        e_mirror = util.nerr(got32[k], f64)
        print("%s %s: float64 %.3e, fp32 mirror %.3e, fixture's fp32 %.3e" % (name, k, e64, e_mirror, e_ref))
        assert got64[k].dtype == torch.float64 and e64 <= 1e-10, (name, k, e64)
        assert e_mirror <= 2 * e_ref + 1e-6, (name, k, e_mirror, e_ref)


# ---- the loader --------------------------------------------------------------------------------------------------------------
def test_loader_is_strict(du):
    sd = state_dict(du, "small")
    m = du.HFClip.from_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    missing = {k: v for k, v in sd.items() if k != "vision_model.encoder.layers.1.mlp.fc2.bias"}
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\) \['vision_model.encoder.layers.1.mlp.fc2.bias'\]"):
        du.HFClip.from_state_dict(missing)
    with pytest.raises(RuntimeError, match=r"1 unexpected key\(s\) \['vision_model.extra'\]"):
        du.HFClip.from_state_dict(dict(sd, **{"vision_model.extra": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="unexpected"):
        du.HFClip.from_state_dict(dict(sd, **{"something.else": torch.zeros(1)}))
    many = {k: v for k, v in sd.items() if ".layer_norm1." not in k}
    with pytest.raises(RuntimeError) as e:
        du.HFClip.from_state_dict(many)
    assert "4 missing key(s)" in str(e.value) and str(e.value).count("layer_norm1") == 4
    with pytest.raises(RuntimeError, match="classifier.bias"):                     # half a head is a missing key
        du.HFClip.from_state_dict({k: v for k, v in sd.items() if k != "classifier.bias"})


def test_loader_ignores_what_from_pretrained_drops(du):
    sd = state_dict(du, "small")
    hub = dict(sd, **{"vision_model.embeddings.position_ids": torch.arange(17)[None], "logit_scale": torch.tensor(4.6),
                      "text_model.embeddings.token_embedding.weight": torch.zeros(10, 8),
                      "text_model.final_layer_norm.bias": torch.zeros(8), "visual_projection.weight": torch.zeros(8, 128),
                      "text_projection.weight": torch.zeros(8, 8)})
    m = du.HFClip.from_state_dict(hub)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_loader_upcasts_fp16(du):
    sd = {k: v.half() for k, v in state_dict(du, "small").items()}
    m = du.HFClip.from_state_dict(sd)
    assert all(v.dtype == torch.float32 for v in m.state_dict().values())
    assert all(torch.equal(v, sd[k].float()) for k, v in m.state_dict().items())


def test_a_file_without_a_classifier_gets_the_seeded_head(du):
    sd = {k: v for k, v in state_dict(du, "small").items() if not k.startswith("classifier.")}
    assert du.HFClip.from_state_dict(sd).classifier.out_features == 2
    assert du.HFClip.from_state_dict(sd, n_class=7).classifier.out_features == 7
    a, _ = du.get_target_model("clip", "cpu", ckpt=sd, n_class=7, seed=3)
    b, _ = du.get_target_model("clip", "cpu", ckpt=sd, n_class=7, seed=3)
    c, _ = du.get_target_model("clip", "cpu", ckpt=sd, n_class=7, seed=4)
    assert a.classifier.out_features == 7 and torch.equal(a.classifier.weight, b.classifier.weight)
    assert not torch.equal(a.classifier.weight, c.classifier.weight)
    assert torch.equal(a.vision_model.pre_layrnorm.weight, sd["vision_model.pre_layrnorm.weight"])
    full = state_dict(du, "small")                                   # the file's own head wins over n_class
    assert du.get_target_model("clip", "cpu", ckpt=full, n_class=7)[0].classifier.out_features == 5


def test_container_and_path_load(du, tmp_path):
    sd = state_dict(du, "small")
    a, _ = du.get_target_model("clip", "cpu", ckpt={"model": sd})
    path = str(tmp_path / "hf_clip_small.pt")
    torch.save({"model": sd}, path)
    b, _ = du.get_target_model("clip", "cpu", ckpt=path)
    for m in (a, b):
        assert isinstance(m, du.HFClip) and not m.training
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


# ---- selection ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_registry(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_TARGET_CKPTS", raising=False)


def test_without_a_checkpoint_clip_is_the_stand_in(du, no_registry):
    m, pre = du.get_target_model("clip", "cpu")
    assert isinstance(m, du.ClipViT) and pre is None
    with pytest.raises(ValueError, match="unknown target model"):
        du.get_target_model("clip-cub", "cpu")


def test_a_clip_state_dict_selects_hf_clip_with_the_goldens_rows(du, fixture, no_registry):
    """Fails on the parent commit: there the state dict is dropped without a word and the model is a ClipViT."""
    z, _ = fixture
    m, _ = du.get_target_model("clip", "cpu", ckpt=state_dict(du, "small"))
    assert isinstance(m, du.HFClip) and not m.training
    from mammo_clip_dissect_amd.concept_vit import utils
    rows, hooks = {}, []
    for i in range(2):
        layer = utils.resolve_layer(m, "vision_model.encoder.layers[%d]" % i)
        hooks.append(layer.register_forward_hook(lambda mod, a, o, i=i: rows.__setitem__(i, o[:, 0].clone())))
    with torch.no_grad():
        logits = m(recipe.make_image("small"))
    for h in hooks:
        h.remove()
    for i in range(2):
        f64 = torch.from_numpy(z["small_layer%d_f64" % i])
        assert util.nerr(rows[i], f64) <= 2 * util.nerr(torch.from_numpy(z["small_layer%d_f32" % i]), f64) + 1e-6
    f64 = torch.from_numpy(z["small_logits_f64"])
    assert util.nerr(logits, f64) <= 2 * util.nerr(torch.from_numpy(z["small_logits_f32"]), f64) + 1e-6


def test_a_registered_checkpoint_selects_hf_clip(du, tmp_path, no_registry):
    path = str(tmp_path / "hf_clip_small.pt")
    sd = state_dict(du, "small")
    torch.save(sd, path)
    du.register_target_checkpoint("clip", path)
    m, _ = du.get_target_model("clip", "cpu")
    assert isinstance(m, du.HFClip) and torch.equal(m.classifier.weight, sd["classifier.weight"])
    # a Mammo-CLIP-shaped ckpt (what utils.build_mammo_models passes) beside the registration: still the registered model
    mammo = {"image_encoder._conv_stem.weight": torch.zeros(48, 3, 3, 3), "text_encoder.text_encoder.pooler.dense.bias": torch.zeros(4)}
    m, _ = du.get_target_model("clip", "cpu", ckpt=mammo)
    assert isinstance(m, du.HFClip) and torch.equal(m.classifier.weight, sd["classifier.weight"])
    # an explicit CLIP state dict wins over the registration
    other = du.HFClip(**recipe.SMALL)
    recipe.fill(other, 99)
    m, _ = du.get_target_model("clip", "cpu", ckpt=other.state_dict())
    assert torch.equal(m.classifier.weight, other.classifier.weight)
    # other targets are untouched by a registration for clip
    assert isinstance(du.get_target_model("vit", "cpu")[0], du.HFViT)


def test_the_registered_target_never_becomes_the_dissector(du, tmp_path, monkeypatch, no_registry):
    """Only the TARGET is registered (INTEGRATION.md's snippet): the drivers' stand-in dissector, built under the same name
    `clip`, stays a ClipViT with a text side; so does the RN50 one; the target is the HFClip."""
    from mammo_clip_dissect_amd.concept_vit import og_utils
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_CLIP_CKPTS", raising=False)
    path = str(tmp_path / "hf_clip_small.pt")
    torch.save(state_dict(du, "small"), path)
    du.register_target_checkpoint("clip", path)
    dissector, tokenize = og_utils._clip_dissector("cpu", "ViT-B/16")
    assert isinstance(dissector, du.ClipViT) and hasattr(dissector, "encode_text") and callable(tokenize)
    assert isinstance(og_utils._clip_dissector("cpu", "RN50")[0], du.ClipResNet)
    assert isinstance(du.get_target_model("clip", "cpu", use_registered=False)[0], du.ClipViT)
    assert isinstance(du.get_target_model("clip", "cpu", ckpt=du.target_ckpt_or("clip", None))[0], du.HFClip)
    # an explicit CLIP state dict is the caller's own choice, whatever the flag
    assert isinstance(du.get_target_model("clip", "cpu", ckpt=state_dict(du, "small"), use_registered=False)[0], du.HFClip)


def test_a_checkpoint_file_is_read_once(du, tmp_path, monkeypatch, no_registry):
    reads, load = [], torch.load
    monkeypatch.setattr(du.torch, "load", lambda f, *a, **kw: (reads.append(f), load(f, *a, **kw))[1])
    mammo = str(tmp_path / "mammo.pt")                               # a path without the CLIP keys: the stand-in loads from it
    torch.save({"model": {"visual_projection.weight": torch.ones(512, 768)}}, mammo)
    m, _ = du.get_target_model("clip", "cpu", ckpt=mammo)
    assert isinstance(m, du.ClipViT) and reads == [mammo] and bool((m.visual_projection.weight == 1).all())
    wrong = str(tmp_path / "resnet.pt")                              # a registered file that is no CLIP classifier: one read, an error
    torch.save({"fc.bias": torch.zeros(3)}, wrong)
    du.register_target_checkpoint("clip", wrong)
    del reads[:]
    with pytest.raises(RuntimeError, match="not a CLIPForImageClassification state dict"):
        du.get_target_model("clip", "cpu", ckpt=du.target_ckpt_or("clip", None))
    assert reads == [wrong]
    table = tmp_path / "targets.json"                                # the JSON table is parsed once per file
    table.write_text(json.dumps({"clip": wrong}))
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.setenv("MCD_TARGET_CKPTS", str(table))
    opened, real_open = [], open
    monkeypatch.setattr("builtins.open", lambda f, *a, **kw: (opened.append(str(f)), real_open(f, *a, **kw))[1])
    assert du.target_checkpoint("clip") == wrong and du.target_checkpoint("clip") == wrong and du.target_checkpoint("vit") is None
    assert opened.count(str(table)) <= 1


def test_a_registered_file_that_is_no_clip_classifier_is_an_error(du, tmp_path, no_registry):
    path = str(tmp_path / "resnet.pt")
    torch.save(du.get_target_model("resnet18", "cpu")[0].state_dict(), path)
    du.register_target_checkpoint("clip", path)
    with pytest.raises(RuntimeError, match="not a CLIPForImageClassification state dict"):
        du.get_target_model("clip", "cpu")


# ---- the registry ------------------------------------------------------------------------------------------------------------
def test_registry(du, tmp_path, monkeypatch, no_registry):
    assert du.target_checkpoint("clip") is None and du.target_ckpt_or("clip", None) is None
    with pytest.raises(FileNotFoundError):
        du.register_target_checkpoint("clip", str(tmp_path / "nowhere.pt"))
    assert du.target_checkpoint("clip") is None
    path = str(tmp_path / "hf_clip_small.pt")
    torch.save(state_dict(du, "small"), path)
    table = tmp_path / "targets.json"
    table.write_text(json.dumps({"clip": path, "resnet18": str(tmp_path / "nowhere.pt")}))
    monkeypatch.setenv("MCD_TARGET_CKPTS", str(table))
    got = du.target_checkpoint("clip")
    assert got == path and isinstance(got, du.RegisteredCheckpoint)
    assert du.target_checkpoint("resnet50") is None
    with pytest.raises(FileNotFoundError):
        du.target_checkpoint("resnet18")
    assert isinstance(du.get_target_model("clip", "cpu")[0], du.HFClip)
    # a registration made in the process wins over the table; breastclip* targets keep the Mammo-CLIP checkpoint
    other = str(tmp_path / "other.pt")
    torch.save(state_dict(du, "small"), other)
    du.register_target_checkpoint("clip", other)
    assert du.target_checkpoint("clip") == other
    du.register_target_checkpoint("breastclip_vit", other)
    assert du.target_ckpt_or("breastclip_vit", "mammo.tar") == "mammo.tar"
    assert du.target_ckpt_or("clip", "mammo.tar") == other and du.target_ckpt_or("resnet50", "mammo.tar") == "mammo.tar"


def test_a_registered_file_must_give_the_model_a_key(du, tmp_path, no_registry):
    path = str(tmp_path / "hf_clip_small.pt")
    sd = state_dict(du, "small")
    torch.save(sd, path)
    # unregistered: the silent non-strict load of an explicit ckpt=, as before
    before = du.get_target_model("resnet18", "cpu", ckpt=path)[0]
    plain = du.get_target_model("resnet18", "cpu")[0]
    assert all(torch.equal(v, plain.state_dict()[k]) for k, v in before.state_dict().items())
    du.register_target_checkpoint("resnet18", path)
    with pytest.raises(RuntimeError, match="has no key that ResNet takes"):
        du.get_target_model("resnet18", "cpu", ckpt=du.target_ckpt_or("resnet18", None))
    # a registration changes nothing for a name it does not carry, nor for a call that does not ask for it
    assert du.target_ckpt_or("resnet34", None) is None
    again = du.get_target_model("resnet18", "cpu")[0]
    assert all(torch.equal(v, plain.state_dict()[k]) for k, v in again.state_dict().items())
    # a registered file of the right target loads
    good = str(tmp_path / "resnet18.pt")
    want = du.get_target_model("resnet18", "cpu", seed=5)[0].state_dict()
    torch.save(want, good)
    du.register_target_checkpoint("resnet18", good)
    got = du.get_target_model("resnet18", "cpu", ckpt=du.target_ckpt_or("resnet18", "mammo.tar"))[0]
    assert all(torch.equal(v, want[k]) for k, v in got.state_dict().items())


# ---- the route's gate, on the CPU --------------------------------------------------------------------------------------------
def test_route_gate(du, monkeypatch):
    m = mirror(du, "small")
    x = recipe.make_image("small")
    assert m.route(x) == "aten"                                                     # not on the GPU
    monkeypatch.setattr(du.core, "linear_residual_available", lambda: True)
    fake = x.as_subclass(util.FakeCuda)
    with torch.no_grad():
        assert m.route(fake) == "hip"
        assert m.route(fake.double()) == "aten"
        monkeypatch.setattr(du, "HIP_HF_CLIP", False)
        assert m.route(fake) == "aten"
        monkeypatch.setattr(du, "HIP_HF_CLIP", True)
        m.train()
        try:
            assert m.route(fake) == "aten"
        finally:
            m.eval()
    assert m.route(fake) == "aten"                                                  # autograd is recording
    wide = du.HFClip(num_labels=2, image_size=32, patch=16, hidden=128, layers=1, heads=4, mlp=128).eval()
    with torch.no_grad():
        assert wide.route(torch.zeros(1, 3, 32, 32).as_subclass(util.FakeCuda)) == "aten"     # 32-wide heads


@pytest.mark.parametrize("B", [1, 3])
def test_embed_residual_leaves_the_position_table_alone(du, B):
    """The residual operand of the K11 + GEMM embedding: the position table per image with class_embedding + its row 0 in
    row 0 -- a tensor of its own.  (For one image expand(1, ..).contiguous() is a view of its operand: the table must go in
    as a copy, or the width probe of the drivers, a forward of one image, rewrites the parameter.)"""
    m = du.HFClip(**recipe.SMALL).eval()
    recipe.fill(m, 5)
    emb = m.vision_model.embeddings
    pos, cls = emb.position_embedding.weight.detach().clone(), emb.class_embedding.detach().clone()
    r = m.vision_model._embed_residual(B)
    assert torch.equal(emb.position_embedding.weight, pos) and torch.equal(emb.class_embedding, cls)
    assert tuple(r.shape) == (B, 17, 128) and r.data_ptr() != emb.position_embedding.weight.data_ptr()
    assert torch.equal(r[:, 1:], pos[1:].expand(B, -1, -1)) and torch.equal(r[:, 0], (cls + pos[0]).expand(B, -1))
    assert m.vision_model._embed_residual(B) is r


def test_the_environment_switch_is_read_at_import(du):
    """MCD_NO_HIP_HF_CLIP=1 is looked at once, when the module is imported: a fresh interpreter is the only honest way to ask."""
    import subprocess
    import sys
    assert du.HIP_HF_CLIP is (os.environ.get("MCD_NO_HIP_HF_CLIP", "0") != "1")
    code = ("import sys; sys.path.insert(0, %r); from mammo_clip_dissect_amd.concept_vit import data_utils as d; "
            "print(d.HIP_HF_CLIP)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MCD_NO_HIP_HF_CLIP="1"), capture_output=True,
                         text=True, check=True).stdout
    assert out.strip() == "False"


def test_fused_qkv_is_the_three_projections_and_follows_them(du):
    m = du.HFClip(**recipe.SMALL).eval()
    recipe.fill(m, 5)
    a = m.vision_model.encoder.layers[0].self_attn
    w, b = a.fused_qkv()
    assert torch.equal(w, torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]))
    assert torch.equal(b, torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]))
    assert a.fused_qkv()[0] is w                                                    # cached
    with torch.no_grad():
        a.k_proj.weight.mul_(2)                                                     # written in place
    w2, _ = a.fused_qkv()
    assert w2 is not w and torch.equal(w2[128:256], a.k_proj.weight)
    a.v_proj.bias = torch.nn.Parameter(torch.ones(128))                             # replaced
    assert torch.equal(a.fused_qkv()[1][256:], torch.ones(128))
    assert sorted(m.state_dict()) == sorted(du.HFClip(**recipe.SMALL).state_dict())  # the cache is no parameter or buffer


# ---- K26's argument checks -----------------------------------------------------------------------------------------------------
def test_token_mean_refuses_bad_arguments(mcd):
    P, Q = 1 << 20, 1 << 30       # non-NULL, 16-byte aligned pointer values that no rejected call may dereference
    ARG, UNSUPPORTED = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_UNSUPPORTED

    def rc(x=P, B=2, T=17, D=128, x_img=17 * 128, x_tok=128, t0=1, out=Q, out_img=128):
        return util.entry_rc(mcd, "mcd_token_mean", x, B, T, D, x_img, x_tok, t0, out, out_img, None)
    assert rc(x=None) == ARG and rc(out=None) == ARG
    assert rc(D=130, x_tok=132, x_img=17 * 132, out_img=132) == ARG                 # D % 4
    assert rc(D=0) == ARG and rc(D=2, x_tok=4, x_img=68, out_img=4) == ARG          # D < 4
    assert rc(T=0) == ARG and rc(t0=-1) == ARG and rc(t0=17) == ARG and rc(t0=18) == ARG
    assert rc(x_tok=124) == ARG and rc(out_img=124) == ARG
    assert rc(x_img=17 * 128 - 4) == ARG                                            # x_img < (T-1)*x_tok + D
    assert rc(x_tok=132, x_img=16 * 132 + 124) == ARG
    assert rc(x_tok=130, x_img=17 * 130 + 2) == ARG and rc(x_img=17 * 128 + 2) == ARG and rc(out_img=130) == ARG   # strides % 4
    assert rc(x=P + 4) == ARG and rc(out=Q + 8) == ARG                              # alignment
    assert rc(B=-1) == ARG
    # out inside x, x inside out's span, out on the last float4 of x's last token
    assert rc(out=P + 16) == ARG and rc(x=Q + 128 * 4, out=Q) == ARG
    assert rc(B=1, out=P + 4 * 17 * 128 - 16) == ARG
    assert rc(B=0, out=P + 16) == 0                                                 # B == 0 looks at nothing else
    assert rc(B=0, x=None, out=None, D=3, T=0) == 0
    assert rc(B=65536) == UNSUPPORTED
    assert rc(B=1, T=2, D=4, x_tok=1 << 29, x_img=(1 << 29) + 4) == UNSUPPORTED     # one image of 2^31 bytes
    assert rc(B=1, T=1 << 22, D=128, x_img=(1 << 22) * 128) == UNSUPPORTED
    assert b"mcd_token_mean" in mcd._lib.load().mcd_last_error()


def test_token_mean_has_no_host_fallback(mcd):
    from mammo_clip_dissect_amd import core
    with pytest.raises(TypeError):
        core.token_mean(torch.zeros(2, 5, 8))


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_abi_surface(mcd):
    lib = mcd._lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_tokens.h")).read(), flags=re.S)
    assert re.search(r"int mcd_token_mean\(const float\* x, int B, int T, int D, int64_t x_img, int64_t x_tok, int t0,\s*"
                     r"float\* out, int64_t out_img, mcd_stream_t stream\);", text)
    assert sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text))) == sorted(lib.TOKEN_SIGNATURES) == ["mcd_token_mean"]
    assert len(lib.TOKEN_SIGNATURES["mcd_token_mean"][1]) == 10
    L = lib.load()
    assert all(hasattr(L, n) for n in lib.TOKEN_SIGNATURES) and L.mcd_abi_version() == 9
    tables = [lib.SIGNATURES, lib.TEXT_SIGNATURES, lib.CLIP_SIGNATURES, lib.TOKEN_SIGNATURES]
    assert len(set().union(*tables)) == sum(len(t) for t in tables)                 # disjoint
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header != "mcd_tokens.h":
            assert not re.search(r"mcd_token_mean\s*\(", open(os.path.join(ROOT, "include", header)).read()), header
