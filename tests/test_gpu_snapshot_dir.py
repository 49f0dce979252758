"""GPU: models built from Hugging Face snapshot directories run the HIP routes.  The snapshots are written here by
checkpoint_io.write_safetensors plus a hand-written config.json, under transformers' key names (no transformers on this
side): the device read of a .safetensors file, a ViT and a ViT-MAE snapshot on the HIP tower route against the ATen route of
the same model (test_gpu_vit_family's / test_gpu_mae's bound: the error against the float64 host forward at most twice the
ATen route's, plus 1e-6), and describe_clip_neurons with MCD_TARGET_CKPTS naming the directory against the same weights as a
torch file."""
import glob
import json
import os

import pytest
import torch

import openai_clip_recipe as openai_recipe
import util
from test_gpu_clip_rn import _bound
from util import nerr

pytestmark = pytest.mark.gpu
WRAPPERS = ("patchify", "patchify_kept", "token_restore", "layer_norm", "vit_attention", "vit_attention_long", "vit_attention_cls")
ATEN_FLAGS = ("HIP_ATTENTION", "FUSED_RESIDUAL", "HIP_LAYER_NORM", "HIP_MAE")
# width 128 = 2 heads x 64, 2 layers, 32 x 32 images at patch 16: 4 patches + the class token
ENCODER = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, image_size=32, patch_size=16,
               hidden_act="gelu", qkv_bias=True)
BATCH = 3                                                # a partial tile in every kernel of the route


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    assert data_utils.core.linear_residual_available(), "libmcd_blaslt.so did not load"
    return data_utils


@pytest.fixture(scope="module")
def io(mcd):
    from mammo_clip_dissect_amd.concept_vit import checkpoint_io
    return checkpoint_io


@pytest.fixture
def registries(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    for name in ("MCD_TARGET_CKPTS", "MCD_CLIP_CKPTS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")


def _fill(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / max(1, p.shape[-1]) ** 0.5)
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return model


def _hf_names(du, sd, stems):
    """The mirror's state dict under transformers' key names: qkv split into query / key / value, the modules renamed back
    (the inverse of data_utils.hf_state_dict).  stems: [(prefix, list name, depth)]."""
    out = dict(sd)
    for prefix, stem, depth in stems:
        for i in range(depth):
            base = "%s.%s.%d." % (prefix, stem, i)
            for leaf in ("weight", "bias"):
                q, k, v = out.pop(base + "attn.qkv." + leaf).chunk(3, dim=0)
                for name, t in (("query", q), ("key", k), ("value", v)):
                    out[base + "attention.attention.%s.%s" % (name, leaf)] = t.clone()
            for old, new in du._hf_layer_map(prefix, i, False, stem).items():
                out[old] = out.pop(new)
    return out


def _write_snapshot(io, path, sd, config):
    os.makedirs(path)
    io.write_safetensors(os.path.join(path, "model.safetensors"), sd)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(config, f)
    return path


def _vit_snapshot(du, io, path, eps):
    net = _fill(du.HFViT(num_labels=3, image_size=32, patch=16, dim=128, depth=2, heads=2, mlp=512, eps=eps), 41)
    sd = _hf_names(du, net.state_dict(), [("vit", "encoder.layer", 2)])
    assert "vit.encoder.layer.1.attention.attention.query.weight" in sd and "vit.encoder.layer.0.layernorm_before.bias" in sd
    config = dict(ENCODER, model_type="vit", layer_norm_eps=eps, id2label={"0": "a", "1": "b", "2": "c"})
    return _write_snapshot(io, path, sd, config), sd


# ---- the device read ------------------------------------------------------------------------------------------------------
def test_device_read_is_the_cpu_read(io, dev, tmp_path):
    g = torch.Generator().manual_seed(9)
    base = torch.randn(37, 129, generator=g)
    t = {"f32": base, "f16": base.half(), "bf16": base.bfloat16(), "scalar": torch.tensor(1.5), "empty": torch.empty(0, 3),
         "ids": torch.arange(7)}
    path = str(tmp_path / "t.safetensors")
    io.write_safetensors(path, t)
    host, device = io.read_safetensors(path), io.read_safetensors(path, device=str(dev))
    assert sorted(host) == sorted(device) == sorted(t)
    for k, v in t.items():
        assert device[k].is_cuda and device[k].dtype == v.dtype and tuple(device[k].shape) == tuple(v.shape), k
        assert torch.equal(host[k], v) and torch.equal(device[k].cpu(), host[k]), k
    assert torch.equal(device["bf16"].view(torch.int16).cpu(), t["bf16"].view(torch.int16))      # bits, not values


# ---- the HIP route on snapshot-built models -----------------------------------------------------------------------------------
def test_vit_snapshot_on_the_hip_route(du, io, dev, tmp_path, monkeypatch, registries):
    d, _ = _vit_snapshot(du, io, str(tmp_path / "vit"), 1e-6)
    model, _ = du.get_target_model("vit", dev, ckpt=d)
    host, _ = du.get_target_model("vit", "cpu", ckpt=d)
    assert isinstance(model, du.HFViT) and not model.training
    assert model.vit.layernorm.eps == 1e-6 and model.vit.encoder.layer[0].norm1.eps == 1e-6
    assert model.vit.encoder.layer[0].attn.heads == 2 and model.classifier.out_features == 3
    assert tuple(model.vit.pos_embed.shape) == (1, 5, 128)
    x = torch.randn(BATCH, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    xg = x.to(dev)
    with torch.no_grad():
        ref = host.double()(x.double())
        cnt = util.CallCounter(du.core, monkeypatch, WRAPPERS)
        got = model(xg)
        torch.cuda.synchronize()
        # K9 in the first block, K9C for the class-token tail of the last one
        assert cnt.n.get("vit_attention", 0) + cnt.n.get("vit_attention_cls", 0) == 2 and cnt.n.get("vit_attention", 0) >= 1, cnt.n
        assert cnt.n.get("patchify") == 1 and cnt.n.get("layer_norm", 0) >= 1, cnt.n
        cnt.n.clear()
        for f in ATEN_FLAGS:
            monkeypatch.setattr(du, f, False)
        aten = model(xg)
        torch.cuda.synchronize()
        assert cnt.n == {}, cnt.n
    assert tuple(got.shape) == (BATCH, 3) and torch.equal(xg.cpu(), x)
    _bound(nerr(got, ref), nerr(aten, ref), "vit snapshot, logits")


def test_mae_snapshot_on_the_hip_route(du, io, dev, tmp_path, monkeypatch, registries):
    net = _fill(du.HFMae(image_size=32, patch=16, hidden=128, layers=2, heads=2, mlp=512, decoder_hidden=64, decoder_layers=1,
                         decoder_heads=2, decoder_mlp=128, eps=1e-6), 43)
    sd = _hf_names(du, net.state_dict(), [("vit", "encoder.layer", 2), ("decoder", "decoder_layers", 1)])
    config = dict(ENCODER, model_type="vit_mae", layer_norm_eps=1e-6, decoder_hidden_size=64, decoder_num_hidden_layers=1,
                  decoder_num_attention_heads=2, decoder_intermediate_size=128, mask_ratio=0.5, norm_pix_loss=True)
    d = _write_snapshot(io, str(tmp_path / "mae"), sd, config)
    model, _ = du.get_target_model("mae", dev, ckpt=d)
    host, _ = du.get_target_model("mae", "cpu", ckpt=d)
    assert isinstance(model, du.HFMae) and model.mask_ratio == 0.5 and model.norm_pix_loss is True
    assert model.vit.layernorm.eps == 1e-6 and model.decoder.decoder_norm.eps == 1e-6
    assert model.vit.encoder.layer[0].attn.heads == 2 and model.decoder.decoder_layers[0].attn.heads == 2
    g = torch.Generator().manual_seed(4)
    x, noise = torch.randn(BATCH, 3, 32, 32, generator=g), torch.rand(BATCH, 4, generator=g)
    xg, ng = x.to(dev), noise.to(dev)
    with torch.no_grad():
        ref = host.double()(x.double(), noise.double())
        assert model.route(xg) == "hip"
        cnt = util.CallCounter(du.core, monkeypatch, WRAPPERS)
        got = model(xg, ng)
        torch.cuda.synchronize()
        assert cnt.n.get("vit_attention") == 2 and cnt.n.get("patchify_kept") == 1 and cnt.n.get("token_restore") == 2, cnt.n
        cnt.n.clear()
        for f in ATEN_FLAGS:
            monkeypatch.setattr(du, f, False)
        assert model.route(xg) == "aten"
        aten = model(xg, ng)
        torch.cuda.synchronize()
        assert cnt.n == {}, cnt.n
    assert tuple(got.logits.shape) == (BATCH, 4, 16 * 16 * 3)
    assert torch.equal(got.mask.cpu(), ref.mask.float()) and torch.equal(got.ids_restore.cpu(), ref.ids_restore)
    _bound(nerr(got.logits, ref.logits), nerr(aten.logits, ref.logits), "mae snapshot, logits")
    _bound(nerr(got.loss.reshape(1), ref.loss.reshape(1)), nerr(aten.loss.reshape(1), ref.loss.reshape(1)), "mae snapshot, loss")


# ---- drop-in, end to end ----------------------------------------------------------------------------------------------------
CONCEPTS = list(openai_recipe.STRINGS[:12])
LAYERS = ["vit.encoder.layer[0]", "vit.encoder.layer[1]"]
PROBE = "synthetic_128_32"


def _drive(drv, tmp, tag, dev, concepts):
    act, res = str(tmp / (tag + "_acts")), str(tmp / (tag + "_results"))
    out = drv.main(["--clip_model", "ViT-B/16", "--target_model", "vit", "--target_layers", ",".join(LAYERS), "--d_probe", PROBE,
                    "--concept_set", str(concepts), "--batch_size", "64", "--device", str(dev), "--activation_dir", act,
                    "--result_dir", res, "--similarity_fn", "wpmi"])
    torch.cuda.synchronize()
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    return open(csvs[0], "rb").read()


def test_driver_with_a_snapshot_directory_is_the_torch_file_run(du, io, dev, tmp_path, monkeypatch, registries):
    """--target_model vit with MCD_TARGET_CKPTS naming the snapshot directory, then naming the same weights as a torch file.
    The configuration is one the shapes give as well (2 heads on 128, eps 1e-12): the two CSVs are the same bytes.  The
    dissector is a small OpenAI CLIP for 32 x 32 images from a registered checkpoint."""
    import importlib
    import io as _io
    import pandas as pd
    drv = importlib.import_module("mammo_clip_dissect_amd.concept_vit.describe_clip_neurons")
    d, sd = _vit_snapshot(du, io, str(tmp_path / "vit"), 1e-12)
    torch.save(sd, str(tmp_path / "vit.pt"))
    dissector = du.OpenAIClip(**dict(openai_recipe.SMALL, image_resolution=32))
    openai_recipe.fill(dissector, seed=78)
    torch.save(dissector.state_dict(), str(tmp_path / "openai_32.pt"))
    du.register_clip_checkpoint("ViT-B/16", str(tmp_path / "openai_32.pt"))
    du.register_tokenizer("clip", openai_recipe.BPE_SMALL)
    concepts = tmp_path / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    table = tmp_path / "targets.json"
    runs = {}
    for tag, path in (("dir", d), ("file", str(tmp_path / "vit.pt"))):
        table.write_text(json.dumps({"vit": path}))
        os.utime(str(table), ns=(len(runs), len(runs)))           # the table is re-read when its stamp changes
        monkeypatch.setenv("MCD_TARGET_CKPTS", str(table))
        assert du.target_checkpoint("vit") == path
        cnt = util.CallCounter(du.core, monkeypatch, WRAPPERS)
        runs[tag] = _drive(drv, tmp_path, tag, dev, concepts)
        assert cnt.n.get("vit_attention", 0) >= 3, cnt.n          # the width probe and two batches of 64, on K9
    assert runs["dir"] == runs["file"]
    df = pd.read_csv(_io.BytesIO(runs["dir"]))
    assert [int((df.layer == layer).sum()) for layer in LAYERS] == [128, 128] and len(df) == 256
