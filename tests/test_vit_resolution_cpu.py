"""CPU: the high-resolution ViT targets without a GPU -- probe-set and target names with an H x W suffix (the old forms
unchanged), position-embedding counts of non-square towers, which attention a call takes (K9, K9L or SDPA), and the
long attention's entry in the header and the ctypes table."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def test_probe_names(du):
    ds = du.get_data("synthetic_64_1520x912")
    assert len(ds) == 64 and ds.size == (1520, 912)
    img, label = ds[3]
    assert img.shape == (3, 1520, 912) and label == 0
    ds = du.get_data("synthetic_5_32x48", lo=1, hi=4)
    assert len(ds) == 3 and ds[0][0].shape == (3, 32, 48)
    # the old forms parse to what they parsed to before
    for name, n, size in (("synthetic_10000_224", 10000, 224), ("synthetic_104_1024", 104, 1024), ("synthetic_7", 7, 224),
                          ("synthetic", 256, 224)):
        ds = du.get_data(name)
        assert (ds.n, ds.size) == (n, size) and isinstance(ds.size, int), name
    assert du.get_data("synthetic_3_40")[0][0].shape == (3, 40, 40)
    # a square H x W suffix is the same probe set as the int one
    assert torch.equal(du.get_data("synthetic_3_40x40")[1][0], du.get_data("synthetic_3_40")[1][0])
    for bad in ("synthetic_3_40x", "synthetic_3_x40", "synthetic_3_abc", "synthetic_3_40x40x2"):
        with pytest.raises(ValueError):
            du.get_data(bad)


def test_device_probe_set_shape(du):
    """DeviceSyntheticImages (here on the host device: only the shapes are checked) generates [3, H, W] images."""
    ds = du.SyntheticImages(4, (24, 40)).on_device("cpu", 1, 3)
    x = ds.images()
    assert x.shape == (2, 3, 24, 40) and ds.size == (24, 40)
    assert [b.shape[0] for b in ds.device_batches(1)] == [1, 1]
    assert du.SyntheticImages(4, 24).on_device("cpu").images().shape == (4, 3, 24, 24)


@pytest.mark.parametrize("size,tokens", [(224, 197), (1024, 4097), ((1520, 912), 5416), ((912, 1520), 5416),
                                         ((224, 224), 197), ((64, 32), 9)])
def test_tower_position_embeddings(du, size, tokens):
    t = du.ViTTower(image_size=size, depth=1)
    assert tuple(t.pos_embed.shape) == (1, tokens, 768)
    x = torch.randn(1, 3, *du.image_hw(size)) if tokens < 300 else None
    if x is not None:                       # the conv path on the host: one token per patch + the class token
        with torch.no_grad():
            assert t(x).shape == (1, tokens, 768)


def test_target_names(du):
    m, _ = du.get_target_model("breastclip_vit_1520x912", "cpu")
    assert tuple(m.image_encoder.pos_embed.shape) == (1, 5416, 768)
    m, _ = du.get_target_model("breastclip_vit_1024", "cpu")
    assert tuple(m.image_encoder.pos_embed.shape) == (1, 4097, 768)
    m, _ = du.get_target_model("breastclip_vit", "cpu")
    assert tuple(m.image_encoder.pos_embed.shape) == (1, 197, 768)
    m, _ = du.get_target_model("breastclip_vit", "cpu", image_size=(448, 224))
    assert tuple(m.image_encoder.pos_embed.shape) == (1, 393, 768)
    c = du.ClipViT(image_size=(1520, 912), text_depth=1)
    assert tuple(c.vision_model.pos_embed.shape) == (1, 5416, 768)
    b = du.BreastClip("vit", image_size=(1520, 912), text_depth=1)
    assert tuple(b.image_encoder.pos_embed.shape) == (1, 5416, 768)
    for bad in ("breastclip_vit_1520x", "breastclip_vit_x912", "breastclip_vit_big"):
        with pytest.raises(ValueError):
            du.get_target_model(bad, "cpu")


def test_dissector_follows_the_target_resolution(du, monkeypatch):
    """utils.build_mammo_models builds the ViT dissector at the target's resolution (the name goes through)."""
    from mammo_clip_dissect_amd.concept_vit import utils
    seen = []
    real = du.get_target_model

    def spy(name, device, **kw):
        seen.append(name)
        return real(name, device, **kw)

    monkeypatch.setattr(du, "get_target_model", spy)
    clip_model, target = utils.build_mammo_models("breastclip_vit_1520x912", "cpu")
    assert seen == ["breastclip_vit_1520x912"] and target is clip_model
    assert tuple(clip_model.image_encoder.pos_embed.shape) == (1, 5416, 768)


def test_attention_route(du, monkeypatch):
    f32 = torch.float32
    r = du.attention_route
    assert du.HIP_ATTENTION
    for T in (1, 197, 256):
        assert r(T, 768, 12, False, True, f32, False) == "k9"
    for T in (257, 785, 4097, 5417, 16385, 32768):
        assert r(T, 768, 12, False, True, f32, False) == "long"
    assert r(32769, 768, 12, False, True, f32, False) == "sdpa"           # past K9L's limit
    assert r(32768, 64 * 100, 100, False, True, f32, False) == "sdpa"     # one image's qkv past 2^31 bytes
    for T in (197, 4097):
        assert r(T, 768, 12, True, True, f32, False) == "sdpa"            # masked (the text tower)
        assert r(T, 768, 12, False, False, f32, False) == "sdpa"          # off the GPU
        assert r(T, 768, 12, False, True, torch.float16, False) == "sdpa"
        assert r(T, 768, 12, False, True, f32, True) == "sdpa"            # autograd
        assert r(T, 512, 12, False, True, f32, False) == "sdpa"           # head width not 64
    monkeypatch.setattr(du, "HIP_ATTENTION", False)
    assert r(197, 768, 12, False, True, f32, False) == "sdpa"
    assert r(4097, 768, 12, False, True, f32, False) == "sdpa"


def test_long_attention_entry_declared(mcd):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_hip.h")).read(), flags=re.S)
    assert re.search(r"int mcd_vit_attention_long\(const float\* qkv, int64_t B, int64_t T, int64_t H, float\* out, "
                     r"mcd_stream_t stream\);", text)
    assert "mcd_vit_attention_long" in mcd._lib.SIGNATURES
    assert hasattr(mcd._lib.load(), "mcd_vit_attention_long")
    from mammo_clip_dissect_amd import core
    assert core.VIT_ATTENTION_LONG_MAX_T >= 16385
    with pytest.raises(TypeError):                     # the product path has no host fallback
        core.vit_attention_long(torch.zeros(1, 300, 192), 1)
