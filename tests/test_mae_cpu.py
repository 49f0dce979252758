"""CPU: data_utils.HFMae (transformers' ViTMAEForPreTraining) against the fixture of tests/golden/mae.npz -- what the
installed transformers computed on the recipe's weights (make_golden_mae.py) --, its checkpoint mapping and strict loader,
its selection by a checkpoint in get_target_model, the seeded default noise, the argument checks of K28 / K29
(mcd_patchify_kept, mcd_token_restore) and the ABI surface of include/mcd_mask.h.  No kernel runs here."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mae_recipe as recipe
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNKNOWN = "unknown target model.*resnet152, vit, vit-cub, vit-bloodmnist, dino, dino-cub, dino-bloodmnist"


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "mae.npz")), json.load(open(os.path.join(util.GOLDEN, "mae_meta.json")))


@pytest.fixture
def no_registry(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_TARGET_CKPTS", raising=False)


_MODELS = {}


def mirror(du, name, meta=None):
    """The mirror of a configuration on the recipe's 4.41.1-keyed weights, through the loader; built once, left unchanged."""
    if name not in _MODELS:
        sd, sha = recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])
        if meta is not None:
            assert sha == meta[name + "_weights_sha256"]
        _MODELS[name] = du.HFMae.from_state_dict(sd, norm_pix_loss=recipe.NORM_PIX_LOSS[name]).eval()
    return _MODELS[name]


def rows_of(model, image, noise):
    """{layer<i>: class-token rows, norm: vit.layernorm's output, logits, loss}, mask, ids_restore of one forward, by hooks
    on the documented hook points."""
    got, hooks = {}, []
    for i, layer in enumerate(model.vit.encoder.layer):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: got.__setitem__("layer%d" % i, o[:, 0].detach().clone())))
    hooks.append(model.vit.layernorm.register_forward_hook(lambda m, a, o: got.__setitem__("norm", o.detach().clone())))
    with torch.no_grad():
        out = model(image, noise)
    for h in hooks:
        h.remove()
    got.update(logits=out.logits, loss=out.loss.reshape(1))
    return got, out.mask, out.ids_restore


def accept(got32, z, name, what=""):
    """The acceptance rule of tests/test_hf_clip_cpu.py: the distance to the float64 fixture is bounded by twice the fp32
    fixture's own distance plus 1e-6."""
    for k in ["layer%d" % i for i in range(recipe.CONFIGS[name]["layers"])] + ["norm", "logits", "loss"]:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        e_ref = util.nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64)
        e_got = util.nerr(got32[k], f64)
        print("%s %s %s: %.3e, fixture's fp32 %.3e" % (what, name, k, e_got, e_ref))
        assert tuple(got32[k].shape) == tuple(f64.shape), (name, k)
        assert e_got <= 2 * e_ref + 1e-6, (what, name, k, e_got, e_ref)


# ---- the module tree and the checkpoint mapping ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "vit-mae-base"])
def test_state_dict_is_the_mapped_reference_key_list(du, fixture, name):
    _, meta = fixture
    listed = meta[name + "_state_dict"]
    assert [[k, list(s)] for k, s in recipe.keys(recipe.CONFIGS[name])] == listed
    model = du.HFMae(**recipe.CONFIGS[name])
    zeros = {k: torch.zeros(s) for k, s in listed}
    mapped = model.convert_state_dict(zeros)
    assert {k: tuple(v.shape) for k, v in mapped.items()} == {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert not any("query" in k or "intermediate" in k for k in mapped)
    own = model.state_dict()                              # a dict saved from the mirror passes through as it is
    again = model.convert_state_dict(own)
    assert len(again) == len(own) and all(again[k] is own[k] for k in own)
    tree = [n for n, _ in model.named_children()] + [n for n, _ in model.vit.named_children()] \
        + [n for n, _ in model.decoder.named_children()]
    assert tree == ["vit", "decoder", "embeddings", "encoder", "layernorm", "decoder_embed", "decoder_layers", "decoder_norm",
                    "decoder_pred"]
    assert model.vit.layernorm.eps == model.decoder.decoder_norm.eps == model.vit.encoder.layer[0].norm1.eps == 1e-12
    assert model.mask_ratio == 0.75 and model.norm_pix_loss is False


@pytest.mark.parametrize("name", ["small", "odd", "vit-mae-base"])
def test_mae_config_recovers_the_configuration(du, name):
    cfg = recipe.CONFIGS[name]
    zeros = {k: torch.zeros(s) for k, s in recipe.keys(cfg)}
    assert du.mae_config(zeros) == cfg                                             # transformers' names
    assert du.mae_config(du.HFMae(**cfg).state_dict()) == cfg                      # the mirror's
    got = du.mae_config(zeros, heads=4, decoder_heads=8)
    assert (got["heads"], got["decoder_heads"]) == (4, 8)
    with pytest.raises(RuntimeError, match="cls_token"):
        du.mae_config({"classifier.weight": torch.zeros(2, 4)})
    with pytest.raises(RuntimeError, match="square"):
        du.mae_config(dict(zeros, **{"vit.embeddings.position_embeddings": torch.zeros(1, 19, cfg["hidden"])}))


def test_loader_is_strict_and_keeps_the_stored_tables(du):
    sd, _ = recipe.weights(recipe.SMALL, recipe.SEED["small"])
    m = du.HFMae.from_state_dict(sd)
    assert torch.equal(m.vit.embeddings.position_embeddings, sd["vit.embeddings.position_embeddings"])
    assert torch.equal(m.decoder.decoder_pos_embed, sd["decoder.decoder_pos_embed"])
    w = m.state_dict()["decoder.decoder_layers.0.attn.qkv.weight"]
    for i, n in enumerate(("query", "key", "value")):
        assert torch.equal(w[64 * i:64 * (i + 1)], sd["decoder.decoder_layers.0.attention.attention.%s.weight" % n])
    assert torch.equal(m.state_dict()["vit.encoder.layer.1.fc2.bias"], sd["vit.encoder.layer.1.output.dense.bias"])
    missing = {k: v for k, v in sd.items() if k != "decoder.decoder_pred.bias"}
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\) \['decoder.decoder_pred.bias'\]"):
        du.HFMae.from_state_dict(missing)
    with pytest.raises(RuntimeError, match=r"1 unexpected key\(s\) \['vit.extra'\]"):
        du.HFMae.from_state_dict(dict(sd, **{"vit.extra": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"missing key\(s\) \['vit.encoder.layer.0.norm2.bias'"):
        du.HFMae.from_state_dict({k: v for k, v in sd.items() if "layer.0.layernorm_after" not in k})
    half = {k: v for k, v in sd.items() if not k.endswith("decoder_layers.0.attention.attention.key.weight")}
    with pytest.raises(KeyError, match="query, key and value"):
        du.HFMae.from_state_dict(half)
    fp16 = du.HFMae.from_state_dict({k: v.half() for k, v in sd.items()})
    assert all(v.dtype == torch.float32 for v in fp16.state_dict().values())


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "odd"])
def test_mirror_against_the_goldens(du, fixture, name):
    z, meta = fixture
    m = mirror(du, name, meta)
    image, noise = recipe.make_image(name), recipe.make_noise(name)
    assert recipe.sha256(image) == meta[name + "_image_sha256"] and recipe.sha256(noise) == meta[name + "_noise_sha256"]
    got32, mask, ids = rows_of(m, image, noise)
    L, keep = (recipe.CONFIGS[name]["image_size"] // recipe.CONFIGS[name]["patch"]) ** 2, recipe.len_keep(recipe.CONFIGS[name])
    assert keep == {"small": 4, "odd": 6}[name] and tuple(got32["norm"].shape) == (recipe.BATCH, 1 + keep, 128)
    assert mask.dtype == torch.float32 and ids.dtype == torch.int64 and tuple(mask.shape) == tuple(ids.shape) == (recipe.BATCH, L)
    assert torch.equal(mask, torch.from_numpy(z[name + "_mask"])) and torch.equal(ids, torch.from_numpy(z[name + "_ids_restore"]))
    accept(got32, z, name, "fp32 mirror")
    m64 = du.HFMae(norm_pix_loss=recipe.NORM_PIX_LOSS[name], **recipe.CONFIGS[name]).double().eval()
    m64.load_state_dict(m.state_dict())
    got64, mask64, ids64 = rows_of(m64, image.double(), noise.double())
    assert torch.equal(mask64, mask) and torch.equal(ids64, ids)
    for k, v in got64.items():
        e64 = util.nerr(v, torch.from_numpy(z["%s_%s_f64" % (name, k)]))
        assert v.dtype == torch.float64 and e64 <= 1e-10, (name, k, e64)


def test_norm_pix_loss_and_mask_ratio_are_constructor_arguments(du, fixture):
    z, _ = fixture
    m = mirror(du, "odd")
    plain = du.HFMae(**recipe.ODD).eval()
    plain.load_state_dict(m.state_dict())
    image, noise = recipe.make_image("odd"), recipe.make_noise("odd")
    with torch.no_grad():
        a, b = m(image, noise), plain(image, noise)
        assert torch.equal(a.logits, b.logits) and abs(float(a.loss) - float(b.loss)) > 1e-3
        half = du.HFMae(mask_ratio=0.5, **recipe.ODD).eval()
        half.load_state_dict(m.state_dict())
        assert int(half(image, noise).mask.sum()) == recipe.BATCH * (25 - 12)
    with pytest.raises(ValueError, match="doesn't match model"):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        du.HFMae(image_size=(32, 32))


def test_default_noise_is_torchs_global_generator(du):
    m = mirror(du, "small")
    image = recipe.make_image("small")
    with torch.no_grad():
        torch.manual_seed(7)
        a = m(image)
        torch.manual_seed(7)
        want = torch.rand(recipe.BATCH, 16)
        torch.manual_seed(7)
        b = m.encode_image(image)
        c = m(image)
        given = m(image, want)
    assert torch.equal(a.ids_restore, b.ids_restore) and torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss)
    assert torch.equal(a.ids_restore, given.ids_restore) and torch.equal(a.logits, given.logits)
    assert not torch.equal(a.ids_restore, c.ids_restore)                           # the generator moved on


# ---- selection ---------------------------------------------------------------------------------------------------------------
def test_without_a_checkpoint_mae_stays_unknown(du, no_registry):
    with pytest.raises(ValueError, match=UNKNOWN):
        du.get_target_model("mae", "cpu")
    with pytest.raises(ValueError, match=UNKNOWN + r"\)\.  mae is built from a ViTMAEForPreTraining checkpoint"):
        du.get_target_model("mae", "cpu")
    with pytest.raises(ValueError, match=UNKNOWN):                                 # a dict without the two keys selects nothing
        du.get_target_model("mae", "cpu", ckpt={"image_encoder._conv_stem.weight": torch.zeros(48, 3, 3, 3)})


def test_a_checkpoint_selects_hf_mae(du, fixture, tmp_path, no_registry):
    z, _ = fixture
    sd, _ = recipe.weights(recipe.SMALL, recipe.SEED["small"])
    m, pre = du.get_target_model("mae", "cpu", ckpt=sd, n_class=7)
    assert isinstance(m, du.HFMae) and not m.training and pre is None
    path = str(tmp_path / "mae_small.pt")
    torch.save({"model": sd}, path)
    m2, _ = du.get_target_model("mae", "cpu", ckpt=path)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m2.state_dict().items())
    from mammo_clip_dissect_amd.concept_vit import utils
    rows, hooks = {}, []
    for i in range(2):
        layer = utils.resolve_layer(m, "vit.encoder.layer[%d]" % i)
        hooks.append(layer.register_forward_hook(lambda mod, a, o, i=i: rows.__setitem__(i, o[:, 0].clone())))
    with torch.no_grad():
        m.encode_image(recipe.make_image("small"), recipe.make_noise("small"))
    for h in hooks:
        h.remove()
    for i in range(2):
        f64 = torch.from_numpy(z["small_layer%d_f64" % i])
        assert util.nerr(rows[i], f64) <= 2 * util.nerr(torch.from_numpy(z["small_layer%d_f32" % i]), f64) + 1e-6


def test_a_registered_checkpoint_is_honoured_and_a_foreign_file_is_an_error(du, tmp_path, no_registry):
    sd, _ = recipe.weights(recipe.SMALL, recipe.SEED["small"])
    path = str(tmp_path / "mae_small.pt")
    torch.save(sd, path)
    du.register_target_checkpoint("mae", path)
    m, _ = du.get_target_model("mae", "cpu")
    assert isinstance(m, du.HFMae) and torch.equal(m.decoder.mask_token, sd["decoder.mask_token"])
    # what the drivers pass: the registered file in place of the Mammo-CLIP checkpoint
    m, _ = du.get_target_model("mae", "cpu", ckpt=du.target_ckpt_or("mae", "mammo.tar"))
    assert isinstance(m, du.HFMae)
    # an explicit MAE state dict wins over the registration
    other, _ = recipe.weights(recipe.ODD, recipe.SEED["odd"])
    assert du.get_target_model("mae", "cpu", ckpt=other)[0].vit.image_size == 30
    assert isinstance(du.get_target_model("vit", "cpu")[0], du.HFViT)             # other targets are untouched
    foreign = str(tmp_path / "resnet.pt")
    torch.save(du.get_target_model("resnet18", "cpu")[0].state_dict(), foreign)
    du.register_target_checkpoint("mae", foreign)
    with pytest.raises(RuntimeError, match="not a ViTMAEForPreTraining state dict"):
        du.get_target_model("mae", "cpu")
    with pytest.raises(RuntimeError, match="not a ViTMAEForPreTraining state dict"):
        du.get_target_model("mae", "cpu", ckpt=du.target_ckpt_or("mae", None))


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
        monkeypatch.setattr(du, "HIP_MAE", False)
        assert m.route(fake) == "aten"
        monkeypatch.setattr(du, "HIP_MAE", True)
        m.train()
        try:
            assert m.route(fake) == "aten"
        finally:
            m.eval()
    assert m.route(fake) == "aten"                                                  # autograd is recording


def test_class_pos_table_is_a_copy(du):
    """The table K29 gathers the embedding GEMM's residual operand from: the position table with cls_token + its row 0 -
    bias in row 0, a tensor of its own (the parameter is never written)."""
    m = mirror(du, "small")
    emb = m.vit.embeddings
    pos = emb.position_embeddings.detach().clone()
    t = m.vit._class_pos_table()
    assert torch.equal(emb.position_embeddings, pos) and t.data_ptr() != emb.position_embeddings.data_ptr()
    assert tuple(t.shape) == (17, 128) and torch.equal(t[1:], pos[0, 1:])
    assert torch.equal(t[0], pos[0, 0] + (emb.cls_token[0, 0] - emb.patch_embeddings.projection.bias))
    assert m.vit._class_pos_table() is t
    assert sorted(m.state_dict()) == sorted(du.HFMae(**recipe.SMALL).state_dict())   # the cache is no parameter or buffer


def test_the_environment_switch_is_read_at_import(du):
    import subprocess
    import sys
    assert du.HIP_MAE is (os.environ.get("MCD_NO_HIP_MAE", "0") != "1")
    code = ("import sys; sys.path.insert(0, %r); from mammo_clip_dissect_amd.concept_vit import data_utils as d; "
            "print(d.HIP_MAE)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MCD_NO_HIP_MAE="1"), capture_output=True,
                         text=True, check=True).stdout
    assert out.strip() == "False"


# ---- the argument checks of K28 and K29 ----------------------------------------------------------------------------------------
P, Q, R = 1 << 20, 1 << 30, 1 << 24     # non-NULL, 16-byte aligned pointer values that no rejected call may dereference


def test_patchify_kept_refuses_bad_arguments(mcd):
    ARG, UNSUPPORTED = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_UNSUPPORTED

    def rc(x=P, keep=R, B=2, Cin=3, H=32, W=32, p=8, Lk=4, out=Q):
        return util.entry_rc(mcd, "mcd_patchify_kept", x, keep, B, Cin, H, W, p, Lk, out, None)
    for p in (7, 1, 3, 15, 0, -2):                                                  # odd or too small a patch
        assert rc(H=210, W=210, p=p) == UNSUPPORTED, p
    assert rc(W=36) == UNSUPPORTED and rc(H=36) == UNSUPPORTED and rc(Cin=0) == UNSUPPORTED
    assert rc(x=None) == ARG and rc(out=None) == ARG and rc(keep=None) == ARG
    assert rc(x=P + 8) == ARG and rc(out=Q + 8) == ARG and rc(keep=R + 2) == ARG
    assert rc(B=-1) == ARG and rc(Lk=-1) == ARG
    assert rc(B=0) == 0 and rc(B=0, x=None, keep=None, out=None, p=7) == 0          # no image: nothing to do
    assert rc(B=1 << 30) == UNSUPPORTED and rc(Lk=1 << 30) == UNSUPPORTED
    assert rc(Cin=1 << 14, H=1 << 14, W=1 << 14, p=2) == UNSUPPORTED                # one image of 2^31 bytes or more
    assert b"mcd_patchify_kept" in mcd._lib.load().mcd_last_error()


def test_token_restore_refuses_bad_arguments(mcd):
    ARG, UNSUPPORTED = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_UNSUPPORTED
    F, A = 1 << 26, 1 << 27

    def rc(src=P, src_img=5 * 64, restore=R, fill=F, add=A, B=2, L=16, Lk=4, D=64, dst=Q):
        return util.entry_rc(mcd, "mcd_token_restore", src, src_img, restore, fill, add, B, L, Lk, D, dst, None)
    assert rc(D=66, src_img=5 * 66) == ARG and rc(D=0) == ARG and rc(D=2, src_img=12) == ARG and rc(D=-4) == ARG
    assert rc(B=-1) == ARG and rc(L=-1) == ARG and rc(Lk=-1) == ARG
    assert rc(src=None) == ARG and rc(dst=None) == ARG and rc(restore=None) == ARG
    assert rc(fill=None, Lk=0, src_img=64) == ARG                                   # nothing to gather and nothing to fill with
    assert rc(src_img=5 * 64 - 4) == ARG and rc(src_img=5 * 64 + 2) == ARG and rc(src_img=-320) == ARG
    assert rc(src=P + 4) == ARG and rc(dst=Q + 8) == ARG and rc(fill=F + 4) == ARG and rc(add=A + 8) == ARG
    assert rc(restore=R + 2) == ARG
    assert rc(dst=P + 16) == ARG and rc(src=Q + 64, dst=Q) == ARG                   # dst inside src, src inside dst
    assert rc(src_img=0, dst=P + 4 * 5 * 64 - 16) == ARG                            # a shared table spans one image's rows
    assert rc(B=0) == 0 and rc(B=0, src=None, restore=None, dst=None) == 0
    assert rc(B=0, D=66) == ARG                                                     # D is looked at first
    assert rc(B=1 << 30) == UNSUPPORTED and rc(L=1 << 23, D=64) == UNSUPPORTED
    assert rc(Lk=1 << 23, D=64, src_img=((1 << 23) + 1) * 64) == UNSUPPORTED
    assert b"mcd_token_restore" in mcd._lib.load().mcd_last_error()


def test_the_kernels_have_no_host_fallback(mcd):
    from mammo_clip_dissect_amd import core
    with pytest.raises(TypeError):
        core.patchify_kept(torch.zeros(1, 3, 8, 8), 4, torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        core.token_restore(torch.zeros(1, 3, 8), torch.zeros(1, 4, dtype=torch.int32))


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_abi_surface(mcd):
    lib = mcd._lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_mask.h")).read(), flags=re.S)
    assert re.search(r"int mcd_patchify_kept\(const float\* x, const int32_t\* keep, int64_t B, int64_t Cin, int64_t H, "
                     r"int64_t W, int64_t P,\s*int64_t Lk, float\* out, mcd_stream_t stream\);", text)
    assert re.search(r"int mcd_token_restore\(const float\* src, int64_t src_img, const int32_t\* restore, const float\* fill, "
                     r"const float\* add,\s*int64_t B, int64_t L, int64_t Lk, int64_t D, float\* dst, mcd_stream_t stream\);", text)
    names = ["mcd_patchify_kept", "mcd_token_restore"]
    assert sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text))) == sorted(lib.MASK_SIGNATURES) == names
    assert len(lib.MASK_SIGNATURES["mcd_patchify_kept"][1]) == 10 and len(lib.MASK_SIGNATURES["mcd_token_restore"][1]) == 11
    L = lib.load()
    assert all(hasattr(L, n) for n in names) and L.mcd_abi_version() == 9
    tables = [lib.SIGNATURES, lib.TEXT_SIGNATURES, lib.CLIP_SIGNATURES, lib.TOKEN_SIGNATURES, lib.SENTENCE_SIGNATURES,
              lib.MASK_SIGNATURES, lib.CACHE_SIGNATURES]
    assert len(set().union(*tables)) == sum(len(t) for t in tables)                 # disjoint
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header != "mcd_mask.h":
            body = open(os.path.join(ROOT, "include", header)).read()
            assert not re.search(r"mcd_(patchify_kept|token_restore)\s*\(", body), header
