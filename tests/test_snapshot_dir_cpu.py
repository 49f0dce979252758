"""CPU: Hugging Face snapshot directories as checkpoints.  One tiny model per family from the installed transformers, filled
with seeded weights and written by save_pretrained (config.json + model.safetensors); every configuration is one the
shape-based guesses get wrong (128 wide with 4 heads, a 64-wide MAE decoder with 4 heads, layer_norm_eps 1e-3, hidden_act
'gelu' for the CLIP classifier, downsample_in_bottleneck for the ResNet, mask_ratio 0.5).

Per family: (a) the directory load is torch.equal to the existing from_state_dict / constructor called with the true
hyperparameters by hand; (b) it agrees with transformers' own forward within the bound the family's golden tests use
(test_vit_family_cpu._bound: error against transformers' float64 result at most twice that of transformers' own fp32 result,
plus 1e-6); (c) the same weights without config.json miss that bound; then contradictions, refusals, fp16 snapshots,
registrations and the environment variables.

transformers is test-side only; its absence is a failure, not a skip."""
import json
import os
import shutil

import pytest
import torch

from util import nerr

SEED = 20


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture
def registries(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.setattr(du, "SENTENCE_CHECKPOINT", {})
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    for name in ("MCD_TARGET_CKPTS", "MCD_CLIP_CKPTS", "MCD_MPNET_CKPT", "MCD_MPNET_VOCAB"):
        monkeypatch.delenv(name, raising=False)


def _bound(e_got, e_ref, what):       # test_vit_family_cpu's
    print("%s: got %.3e transformers fp32 %.3e ratio to the bound %.3f" % (what, e_got, e_ref, e_got / (2 * e_ref + 1e-6)))
    assert e_got <= 2 * e_ref + 1e-6, (what, e_got, e_ref)


def _fill(model, seed):
    """Seeded weights at a scale where head counts, eps and the activation all matter (transformers' 0.02 init makes every
    attention row uniform).  LayerNorm inputs stay small against eps = 1e-3: the embeddings are scaled down."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() <= 1 and ("norm" in name.lower() or "lambda" in name):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g)) if name.endswith(("weight", "lambda1")) else \
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "embed" in name or "token" in name:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / max(1, p[0].numel()) ** 0.5 if p.dim() > 1 else 0.1))
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return model.eval()


VIT = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256, image_size=32, patch_size=16,
           layer_norm_eps=1e-3)
TEXT = dict(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256,
            max_position_embeddings=16, eos_token_id=99, bos_token_id=98, pad_token_id=0)


def _image(size, seed=1):
    return torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(seed))


class Family:
    """name: the target; make(): the transformers model; x: its input; hf(model, x) / ours(model, x): the compared tensors;
    explicit(du, sd): the mirror built by hand with the true hyperparameters."""


def _families():
    import transformers as T                             # its absence is a failure: the snapshots are its own
    fams = {}

    f = Family()
    f.target, f.x = "vit", _image(32)
    f.make = lambda: T.ViTForImageClassification(T.ViTConfig(num_labels=3, **VIT))
    f.hf = lambda m, x: [m(x).logits]
    f.ours = lambda m, x: [m(x)]

    def explicit(du, sd):
        net = du.HFViT(num_labels=3, image_size=32, patch=16, dim=128, depth=2, heads=4, mlp=256, eps=1e-3).eval()
        return du._load_local(net, sd)
    f.explicit = explicit
    fams["vit"] = f

    f = Family()
    f.target, f.x = "dino", _image(28)
    f.make = lambda: T.Dinov2ForImageClassification(T.Dinov2Config(
        hidden_size=128, num_hidden_layers=2, num_attention_heads=4, mlp_ratio=2, image_size=28, patch_size=14,
        layer_norm_eps=1e-3, num_labels=3))
    f.hf = lambda m, x: [m(x).logits]
    f.ours = lambda m, x: [m(x)]

    def explicit(du, sd):
        net = du.HFDinov2(num_labels=3, image_size=28, patch=14, dim=128, depth=2, heads=4, mlp=256, eps=1e-3).eval()
        return du._load_local(net, sd)
    f.explicit = explicit
    fams["dino"] = f

    f = Family()
    f.target, f.x = "clip", _image(32)
    f.make = lambda: T.CLIPForImageClassification(T.CLIPConfig(
        vision_config=dict(VIT, hidden_act="gelu"), text_config=dict(TEXT), projection_dim=64, num_labels=3))
    f.hf = lambda m, x: [m(x).logits]
    f.ours = lambda m, x: [m(x)]
    f.explicit = lambda du, sd: du.HFClip.from_state_dict(sd, heads=4, hidden_act="gelu", eps=1e-3).eval()
    fams["clip"] = f

    f = Family()
    f.target, f.x = "resnet", _image(64)
    f.make = lambda: T.ResNetForImageClassification(T.ResNetConfig(
        embedding_size=16, hidden_sizes=[32, 64], depths=[1, 2], layer_type="bottleneck", hidden_act="relu",
        downsample_in_bottleneck=True, num_labels=3))
    f.hf = lambda m, x: [m(x).logits]
    f.ours = lambda m, x: [m(x)]
    f.explicit = lambda du, sd: du.HFResNet.from_state_dict(sd, downsample_in_bottleneck=True).eval()
    fams["resnet"] = f

    f = Family()
    f.target = "mae"
    f.x = (_image(64), torch.rand(2, 16, generator=torch.Generator().manual_seed(2)))
    f.make = lambda: T.ViTMAEForPreTraining(T.ViTMAEConfig(
        **dict(VIT, image_size=64), decoder_hidden_size=64, decoder_num_hidden_layers=1, decoder_num_attention_heads=4,
        decoder_intermediate_size=128, mask_ratio=0.5, norm_pix_loss=True))

    def hf(m, x):
        out = m(pixel_values=x[0], noise=x[1].to(x[0].dtype))
        return [out.logits, out.loss.reshape(1), out.mask]
    f.hf = hf

    def ours(m, x):
        out = m(x[0], noise=x[1])
        return [out.logits, out.loss.reshape(1), out.mask]
    f.ours = ours
    f.explicit = lambda du, sd: du.HFMae.from_state_dict(sd, heads=4, decoder_heads=4, mask_ratio=0.5, norm_pix_loss=True,
                                                         eps=1e-3).eval()
    fams["mae"] = f

    f = Family()
    f.target = "mpnet"
    ids = torch.randint(4, 100, (3, 12), generator=torch.Generator().manual_seed(4))
    mask = torch.ones(3, 12, dtype=torch.long)
    mask[1, 9:], mask[2, 5:] = 0, 0
    ids[mask == 0] = 1                                   # <pad>
    f.x = (ids, mask)
    f.make = lambda: T.MPNetModel(T.MPNetConfig(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=4,
                                                intermediate_size=256, max_position_embeddings=40, layer_norm_eps=1e-3,
                                                relative_attention_num_buckets=32))   # (transformers' encoder buckets by 32 whatever this says)
    f.hf = lambda m, x: [m(input_ids=x[0], attention_mask=x[1]).last_hidden_state[x[1].bool()]]
    f.ours = lambda m, x: [m({"input_ids": x[0], "attention_mask": x[1]})[x[1].bool()]]
    f.explicit = lambda du, sd: du.MPNetSentenceEncoder.from_state_dict(sd, eps=1e-3).eval()
    fams["mpnet"] = f

    f = Family()
    f.target = "openai_clip"
    tokens = torch.randint(1, 98, (3, 16), generator=torch.Generator().manual_seed(6))
    tokens[:, 0] = 98
    for row, end in enumerate((15, 9, 4)):
        tokens[row, end] = 99                            # <|endoftext|>: the largest id of its row
        tokens[row, end + 1:] = 0
    f.x = (_image(32), tokens)
    # (OpenAI's towers: the MLP is four widths wide, LayerNorm eps 1e-5, QuickGELU -- what OpenAIClip computes)
    f.make = lambda: T.CLIPModel(T.CLIPConfig(
        vision_config=dict(VIT, layer_norm_eps=1e-5, hidden_act="quick_gelu", intermediate_size=512),
        text_config=dict(TEXT, hidden_act="quick_gelu", intermediate_size=512), projection_dim=64))

    def features(out):
        return out if torch.is_tensor(out) else out.pooler_output

    def hf(m, x):
        pad = (x[1] != 0).long()
        pad[:, 0] = 1
        return [features(m.get_image_features(pixel_values=x[0])), features(m.get_text_features(input_ids=x[1], attention_mask=pad))]
    f.hf = hf
    f.ours = lambda m, x: [m.encode_image(x[0]), m.encode_text(x[1])]
    f.explicit = lambda du, sd: du.OpenAIClip.from_state_dict(du.hf_clip_to_openai(sd), vision_heads=4, transformer_heads=4).eval()
    fams["openai_clip"] = f
    return fams


@pytest.fixture(scope="module")
def snapshots(tmp_path_factory):
    """family -> (Family, directory, transformers' float64 and fp32 outputs on the family's input)."""
    root = tmp_path_factory.mktemp("hub")
    out = {}
    for i, (name, fam) in enumerate(_families().items()):
        torch.manual_seed(SEED + i)
        model = _fill(fam.make(), SEED + i)
        d = str(root / name)
        model.save_pretrained(d)
        assert sorted(os.listdir(d)) == ["config.json", "model.safetensors"], os.listdir(d)
        with torch.no_grad():
            f32 = [t.clone() for t in fam.hf(model, fam.x)]
            x64 = tuple(t.double() if t.is_floating_point() else t for t in fam.x) if isinstance(fam.x, tuple) else fam.x.double()
            f64 = [t.clone() for t in fam.hf(model.double(), x64)]
        out[name] = (fam, d, f64, f32)
    return out


def _build(du, fam, path):
    if fam.target == "mpnet":
        return du.sentence_encoder("cpu", ckpt=path)
    return du.get_target_model(fam.target, "cpu", ckpt=path)[0]


def _without_config(d, tmp_path):
    bare = str(tmp_path / "bare")
    os.mkdir(bare)
    shutil.copy(os.path.join(d, "model.safetensors"), bare)
    return bare


FAMILIES = ["vit", "dino", "clip", "resnet", "mae", "mpnet", "openai_clip"]


@pytest.mark.parametrize("name", FAMILIES)
def test_directory_load(du, snapshots, registries, tmp_path, name):
    from safetensors.torch import load_file
    fam, d, f64, f32 = snapshots[name]
    model = _build(du, fam, d)
    assert not model.training
    with torch.no_grad():
        got = fam.ours(model, fam.x)
        # (a) bit-exact with the mirror built by hand from the same tensors and the true hyperparameters
        want = fam.ours(fam.explicit(du, load_file(os.path.join(d, "model.safetensors"))), fam.x)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == len(want)
        # ... and the single file beside config.json is the same model
        again = fam.ours(_build(du, fam, os.path.join(d, "model.safetensors")), fam.x)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        # (b) transformers' own forward, at the golden tests' bound
        for i, (g, r64, r32) in enumerate(zip(got, f64, f32)):
            assert tuple(g.shape) == tuple(r64.shape)
            _bound(nerr(g, r64), nerr(r32, r64), "%s output %d" % (name, i))
        # (c) the same weights without config.json: the shape-based guess computes something else
        bare = fam.ours(_build(du, fam, _without_config(d, tmp_path)), fam.x)
        e = nerr(bare[0], f64[0])
        print("%s without config.json: %.3e against the bound %.3e" % (name, e, 2 * nerr(f32[0], f64[0]) + 1e-6))
        assert e > 100 * (2 * nerr(f32[0], f64[0]) + 1e-6), (name, e)


def _copy_with(d, tmp_path, tag, **fields):
    """A copy of snapshot d whose config.json has `fields` set (a dotted key reaches into a sub-config)."""
    out = str(tmp_path / tag)
    shutil.copytree(d, out)
    path = os.path.join(out, "config.json")
    config = json.load(open(path))
    for key, value in fields.items():
        where = config
        *parents, leaf = key.split("__")
        for p in parents:
            where = where[p]
        where[leaf] = value
    json.dump(config, open(path, "w"))
    return out


CONTRADICTIONS = {"vit": "hidden_size", "dino": "hidden_size", "clip": "vision_config__hidden_size", "resnet": "embedding_size",
                  "mae": "decoder_hidden_size", "mpnet": "hidden_size", "openai_clip": "text_config__hidden_size"}


@pytest.mark.parametrize("name", FAMILIES)
def test_a_config_that_contradicts_the_shapes_is_an_error(du, snapshots, registries, tmp_path, name):
    fam, d, _, _ = snapshots[name]
    field = CONTRADICTIONS[name]
    with pytest.raises(RuntimeError, match=r"%s = 96\b.*\b(128|64|16)\b" % field.split("__")[-1]):
        _build(du, fam, _copy_with(d, tmp_path, "edited", **{field: 96}))


def test_more_contradictions_name_their_field(du, snapshots, registries, tmp_path):
    for name, field, value in (("vit", "patch_size", 8), ("vit", "num_hidden_layers", 3), ("vit", "image_size", 64),
                               ("vit", "id2label", {"0": "a"}), ("dino", "mlp_ratio", 4), ("resnet", "depths", [1, 1]),
                               ("resnet", "layer_type", "basic"), ("mae", "intermediate_size", 512),
                               ("mpnet", "relative_attention_num_buckets", 16), ("mpnet", "num_attention_heads", 2),
                               ("openai_clip", "projection_dim", 32)):
        fam, d, _, _ = snapshots[name]
        what = {"id2label": "num_labels", "mlp_ratio": "mlp_ratio"}.get(field, field)
        with pytest.raises(RuntimeError, match=what):
            _build(du, fam, _copy_with(d, tmp_path, "%s_%s" % (name, field), **{field: value}))


def test_a_snapshot_of_another_family_is_refused(du, snapshots, registries):
    with pytest.raises(ValueError, match="dinov2.*vit"):
        du.get_target_model("vit", "cpu", ckpt=snapshots["dino"][1])
    with pytest.raises(ValueError, match="model_type"):
        du.get_target_model("mae", "cpu", ckpt=du.register_target_checkpoint("mae", snapshots["vit"][1]) or du.target_checkpoint("mae"))
    with pytest.raises(ValueError, match="model_type"):
        du.sentence_encoder("cpu", ckpt=snapshots["vit"][1])


def test_what_a_mirror_cannot_compute_is_refused(du, snapshots, registries, tmp_path):
    for name, field, value in (("dino", "use_swiglu_ffn", True), ("vit", "hidden_act", "gelu_new"), ("vit", "qkv_bias", False),
                               ("mae", "qkv_bias", False), ("clip", "vision_config__hidden_act", "relu"),
                               ("resnet", "hidden_act", "gelu"), ("mpnet", "hidden_act", "relu"),
                               ("openai_clip", "text_config__hidden_act", "gelu"),
                               ("openai_clip", "vision_config__layer_norm_eps", 1e-6)):
        fam, d, _, _ = snapshots[name]
        with pytest.raises(NotImplementedError, match=field.split("__")[-1]):
            _build(du, fam, _copy_with(d, tmp_path, "%s_%s" % (name, field), **{field: value}))


@pytest.mark.parametrize("name", ["vit", "clip", "mae", "mpnet", "openai_clip"])
def test_an_fp16_snapshot_is_upcast(du, io, snapshots, registries, tmp_path, name):
    """The fp16 snapshot's model holds exactly the fp32 weights rounded to fp16, as fp32 tensors, and computes with them."""
    from safetensors.torch import load_file
    fam, d, f64, f32 = snapshots[name]
    half = str(tmp_path / "half")
    os.mkdir(half)
    shutil.copy(os.path.join(d, "config.json"), half)
    sd = load_file(os.path.join(d, "model.safetensors"))
    io.write_safetensors(os.path.join(half, "model.safetensors"),
                         {k: (v.half() if v.is_floating_point() else v) for k, v in sd.items()})
    full, model = _build(du, fam, d), _build(du, fam, half)
    for (k, a), (_, b) in zip(full.state_dict().items(), model.state_dict().items()):
        assert b.dtype == a.dtype and torch.equal(b, a.half().to(a.dtype) if a.is_floating_point() else a), k
    with torch.no_grad():
        got = fam.ours(model, fam.x)
    assert got[0].dtype == torch.float32 and nerr(got[0], f64[0]) < 2e-2


@pytest.fixture(scope="module")
def io(mcd):
    from mammo_clip_dissect_amd.concept_vit import checkpoint_io
    return checkpoint_io


# ---- registration and the drivers' entry points ---------------------------------------------------------------------------
def _reference(du, snapshots, name):
    from safetensors.torch import load_file
    fam, d, _, _ = snapshots[name]
    with torch.no_grad():
        return fam, d, fam.ours(fam.explicit(du, load_file(os.path.join(d, "model.safetensors"))), fam.x)


@pytest.mark.parametrize("name", ["vit", "dino", "clip", "resnet", "mae"])
def test_registered_directories_build_the_same_model(du, snapshots, registries, tmp_path, monkeypatch, name):
    fam, d, want = _reference(du, snapshots, name)
    with pytest.raises(FileNotFoundError, match="not an existing local file"):
        du.register_target_checkpoint(name, str(tmp_path / "nowhere"))
    du.register_target_checkpoint(name, d)
    path = du.target_ckpt_or(name, None)
    assert isinstance(path, du.RegisteredCheckpoint) and path == d
    with torch.no_grad():
        got = fam.ours(du.get_target_model(name, "cpu", ckpt=path)[0], fam.x)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # the JSON table of MCD_TARGET_CKPTS names the directory
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    table = tmp_path / "targets.json"
    table.write_text(json.dumps({name: d, "other": str(tmp_path / "nowhere")}))
    monkeypatch.setenv("MCD_TARGET_CKPTS", str(table))
    with torch.no_grad():
        got = fam.ours(du.get_target_model(name, "cpu", ckpt=du.target_ckpt_or(name, None))[0], fam.x)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(FileNotFoundError, match="not an existing local file"):
        du.target_checkpoint("other")


def test_the_clip_dissector_from_a_registered_snapshot(du, snapshots, registries, monkeypatch):
    from mammo_clip_dissect_amd.concept_vit import og_utils
    fam, d, want = _reference(du, snapshots, "openai_clip")
    du.register_clip_checkpoint("ViT-B/16", d)
    model, tokenize = og_utils._clip_dissector("cpu", "ViT-B/16")
    assert isinstance(model, du.OpenAIClip) and model.visual.transformer.resblocks[0].attn.heads == 4
    assert model.transformer.resblocks[0].attn.heads == 4
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(fam.ours(model, fam.x), want))
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.setenv("MCD_CLIP_CKPTS", "RN50=/nowhere/rn50.pt, ViT-B/16=%s" % d)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(fam.ours(og_utils._clip_dissector("cpu", "ViT-B/16")[0], fam.x), want))
        # the directory itself as --clip_model, the way clip.load takes a path
        assert all(torch.equal(a, b) for a, b in zip(fam.ours(og_utils._clip_dissector("cpu", d)[0], fam.x), want))
    # the rename: OpenAI's key set, the projections transposed
    from safetensors.torch import load_file
    sd = load_file(os.path.join(d, "model.safetensors"))
    renamed = du.hf_clip_to_openai(sd, json.load(open(os.path.join(d, "config.json"))))
    assert set(renamed) == set(model.state_dict())
    assert torch.equal(renamed["visual.proj"], sd["visual_projection.weight"].t())
    assert torch.equal(renamed["text_projection"], sd["text_projection.weight"].t())
    blk = "vision_model.encoder.layers.1.self_attn."
    assert torch.equal(renamed["visual.transformer.resblocks.1.attn.in_proj_weight"],
                       torch.cat([sd[blk + "q_proj.weight"], sd[blk + "k_proj.weight"], sd[blk + "v_proj.weight"]]))
    with pytest.raises(RuntimeError, match="no OpenAI name"):
        du.hf_clip_to_openai(dict(sd, **{"vision_model.extra.weight": torch.zeros(1)}))


def test_register_sentence_checkpoint_picks_up_the_vocabulary(du, snapshots, registries, tmp_path, monkeypatch):
    fam, d, want = _reference(du, snapshots, "mpnet")
    full = str(tmp_path / "all-mpnet-tiny")
    shutil.copytree(d, full)
    words = ["<s>", "<pad>", "</s>", "<unk>"] + ["w%d" % i for i in range(95)] + ["<mask>"]
    with open(os.path.join(full, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(words) + "\n")
    with pytest.raises(FileNotFoundError, match="not an existing local file"):
        du.register_sentence_checkpoint(str(tmp_path / "nowhere"))
    du.register_sentence_checkpoint(full)
    assert du.TOKENIZER_VOCABS["mpnet"][0] == os.path.join(full, "vocab.txt")
    model = du.sentence_encoder("cpu")
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(fam.ours(model, fam.x), want))
    vectors = model.encode(["w1 w2 w3", "w7"])
    assert vectors.shape == (2, 128)
    # a vocabulary registered before stays
    du.register_tokenizer("mpnet", os.path.join(d, "config.json"))
    du.register_sentence_checkpoint(full)
    assert du.TOKENIZER_VOCABS["mpnet"][0] == os.path.join(d, "config.json")
    # the environment variable names the directory
    monkeypatch.setattr(du, "SENTENCE_CHECKPOINT", {})
    monkeypatch.setenv("MCD_MPNET_CKPT", full)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(fam.ours(du.sentence_encoder("cpu"), fam.x), want))


def test_what_loaded_before_loads_as_before(du, snapshots, registries, tmp_path):
    """A state dict, a {'model': ...} dict and a torch file: no config.json is looked for, the guesses stay."""
    from safetensors.torch import load_file
    fam, d, _, _ = snapshots["mae"]
    sd = load_file(os.path.join(d, "model.safetensors"))
    guess = du.HFMae.from_state_dict(sd).eval()
    assert guess.vit.encoder.layer[0].attn.heads == 2 and guess.mask_ratio == 0.75
    path = os.path.join(d, "weights.pt")                 # a torch file beside a config.json: still the guess
    torch.save({"model": sd}, path)
    try:
        with torch.no_grad():
            want = fam.ours(guess, fam.x)
            for ckpt in (sd, {"model": sd}, path):
                got = fam.ours(du.get_target_model("mae", "cpu", ckpt=ckpt)[0], fam.x)
                assert all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        os.remove(path)
    assert du.snapshot_kwargs("mae", None) == {} and du.snapshot_kwargs("vit", None, sd) == {}
    for name in ("mae", "resnet", "clip-cub"):           # the message existing tests match on
        with pytest.raises(ValueError, match="unknown target model %r \\(offline build: breastclip, " % name):
            du.get_target_model(name, "cpu")
    with pytest.raises(FileNotFoundError):
        du.get_target_model("vit", "cpu", ckpt=str(tmp_path / "nowhere.pt"))
    with pytest.raises(FileNotFoundError):
        du.get_target_model("vit", "cpu", ckpt=str(tmp_path))            # a directory without a checkpoint
