"""CPU: OpenAI CLIP's own dissector -- ClipBPETokenizer against the reference tokenizer's ids (tests/golden/openai_clip.npz, on
the small merges file clip_bpe_small.txt.gz), OpenAIClip's state dict against the reference CLIP's keys and shapes in three
configurations, its strict fp16-upcasting load, its ATen route on the CPU against the reference's float64 and fp32 outputs
on the recipe's weights (tests/openai_clip_recipe.py), the routes and gates as pure functions, the selection by checkpoint
in og_utils._clip_dissector, and the ABI surface of include/mcd_clip.h.  No kernel runs here."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import openai_clip_recipe as recipe
import util
from util import nerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "openai_clip.npz")), json.load(open(os.path.join(util.GOLDEN, "openai_clip_meta.json")))


@pytest.fixture(scope="module")
def tok(du):
    return du.ClipBPETokenizer(recipe.BPE_SMALL)


@pytest.fixture()
def unregistered(du, monkeypatch):
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_CLIP_BPE", raising=False)
    monkeypatch.delenv("MCD_CLIP_CKPTS", raising=False)


def _bound(e_got, e_ref, what):       # the project's convention (test_text_tower_cpu, test_vit_family_cpu)
    print("%s: got %.3e reference fp32 %.3e ratio to the bound %.3f" % (what, e_got, e_ref, e_got / (2 * e_ref + 1e-6)))
    assert e_got <= 2 * e_ref + 1e-6, (what, e_got, e_ref)


def small_model(du, dtype=torch.float32):
    m = du.OpenAIClip(**recipe.SMALL).eval()
    if dtype == torch.float64:
        m = m.double()
    return m, recipe.fill(m)


# ---- the tokenizer ---------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_recipe_says(fixture):
    z, meta = fixture
    assert meta["strings"] == len(recipe.STRINGS) == z["ids"].shape[0] and int(z["long_row"]) == recipe.LONG_ROW
    assert meta["small_config"] == recipe.SMALL and meta["n_merges"] == recipe.N_MERGES
    assert meta["image_sha256"] == recipe.sha256(recipe.make_image())
    lines = set(open(CONCEPTS).read().split("\n"))
    assert sum(s in lines for s in recipe.STRINGS) >= 12
    assert "keyhole sign (teardrop, noose)" in recipe.STRINGS and "postoperative seroma/hematoma" in recipe.STRINGS
    for name in ("openai_clip.npz", "openai_clip_meta.json", "clip_bpe_small.txt.gz"):
        assert os.path.getsize(os.path.join(util.GOLDEN, name)) < 1000000


def test_ids_equal_the_reference_tokenizers(tok, fixture):
    z, _ = fixture
    want = z["ids"].astype(np.int64)
    assert tok.vocab_size == recipe.SMALL["vocab_size"]
    assert (tok.sot_id, tok.eot_id) == (tok.vocab_size - 2, tok.vocab_size - 1)         # read from the vocabulary
    for i, s in enumerate(recipe.STRINGS):
        if i == recipe.LONG_ROW:
            continue
        got = tok([s], context_length=77)[0].numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want[i]), (s, got[:20], want[i][:20])
        e = int(got.argmax())                                                              # the end id is the largest
        assert got[e] == tok.eot_id and got[0] == tok.sot_id and not got[e + 1:].any() and (got[1:e] < tok.sot_id).all()
    batch = tok([s for i, s in enumerate(recipe.STRINGS) if i != recipe.LONG_ROW])
    assert np.array_equal(batch.numpy(), np.delete(want, recipe.LONG_ROW, axis=0))
    assert np.array_equal(tok("axe").numpy(), want[1:2])                                # a plain string is a batch of one


def test_too_long_raises_and_truncates(tok, fixture):
    z, _ = fixture
    long = recipe.STRINGS[recipe.LONG_ROW]
    with pytest.raises(RuntimeError, match="too long for context length 77"):
        tok([long], context_length=77)
    got = tok([long], context_length=77, truncate=True)[0]
    assert np.array_equal(got.numpy(), z["ids"][recipe.LONG_ROW].astype(np.int64)) and int(got[-1]) == tok.eot_id
    assert tok([long], context_length=200).shape == (1, 200)


def test_the_scanner_splits_like_the_pattern(du):
    sp = du.ClipBPETokenizer.split
    assert sp("don't!'s it's") == ["don", "'t", "!'", "s", "it", "'s"]
    assert sp("a12 b") == ["a", "1", "2", "b"]
    assert sp("x<|endoftext|>y .<|endoftext|>") == ["x", "<|endoftext|>", "y", ".<|", "endoftext", "|>"]
    assert sp("cm\u00b2 \u00e9\u00df") == ["cm", "\u00b2", "\u00e9\u00df"]
    assert du.ClipBPETokenizer.clean("  A &amp;amp;  B\t\nC\u00a0") == "a & b c"


def test_a_truncated_merges_file_gives_a_consistent_vocabulary(du, tmp_path):
    import gzip
    lines = gzip.open(recipe.BPE_SMALL).read().decode("utf-8").split("\n")
    p = tmp_path / "tiny.txt"
    p.write_text("\n".join(lines[:101]), encoding="utf-8")                   # plain text, 100 merges
    t = du.ClipBPETokenizer(str(p))
    assert t.vocab_size == 512 + 100 + 2 and t.eot_id == t.vocab_size - 1 and t.sot_id == t.vocab_size - 2
    row = t(["the axe"])[0]
    assert int(row.max()) == t.eot_id and int(row[0]) == t.sot_id and not bool(row[int(row.argmax()) + 1:].any())


def test_tokenize_without_a_merges_file_raises(du, unregistered):
    m = du.OpenAIClip(**recipe.SMALL)
    with pytest.raises(RuntimeError, match="register_tokenizer.*MCD_CLIP_BPE.*no fallback"):
        m.tokenize(["mass"])
    assert m.tokenizer is None
    with pytest.raises(ValueError, match="not a BPE merges file"):
        du.register_tokenizer("clip", os.path.join(util.GOLDEN, "text_vocab.txt"))
    du.register_tokenizer("clip", recipe.BPE_SMALL)
    assert m.tokenize(["mass"]).shape == (1, 77) and isinstance(m.tokenizer, du.ClipBPETokenizer)
    # a merges file larger than the embedding table is refused while the ids are on the host
    m2 = du.OpenAIClip(**dict(recipe.SMALL, vocab_size=1000))
    with pytest.raises(ValueError, match="embedding table has 1000 rows"):
        m2.tokenize(["mass"])


def test_the_environment_variable_registers_too(du, unregistered, monkeypatch):
    monkeypatch.setenv("MCD_CLIP_BPE", recipe.BPE_SMALL)
    assert du.OpenAIClip(**recipe.SMALL).tokenize("axe").shape == (1, 77)


def test_the_tokenizer_needs_neither_regex_nor_ftfy():
    code = ("import sys, importlib.abc\n"
            "class Block(importlib.abc.MetaPathFinder):\n"
            "    def find_spec(self, name, path, target=None):\n"
            "        if name.split('.')[0] in ('regex', 'ftfy'):\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            "sys.path.insert(0, %r)\n"
            "import mammo_clip_dissect_amd\n"
            "from mammo_clip_dissect_amd.concept_vit import data_utils as du\n"
            "t = du.ClipBPETokenizer(%r)\n"
            "print(t(['keyhole sign (teardrop, noose)']).shape[1], 'regex' in sys.modules, 'ftfy' in sys.modules)\n"
            % (ROOT, recipe.BPE_SMALL))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["77", "False", "False"]


@pytest.mark.skipif(not os.environ.get("MCD_CLIP_BPE"), reason="MCD_CLIP_BPE does not point at a merges file")
def test_all_concepts_with_the_full_merges_file(du):
    t = du.ClipBPETokenizer(os.environ["MCD_CLIP_BPE"])
    if t.vocab_size != 49408:
        pytest.skip("MCD_CLIP_BPE is not the full merges file")
    words = [w for w in open(CONCEPTS).read().split("\n") if w]
    assert len(words) in (762, 763)
    ids = t(words, context_length=77)
    assert bool((ids[:, 0] == 49406).all())
    assert bool((ids[torch.arange(len(words)), ids.argmax(-1)] == 49407).all())
    print("%d concepts, longest %d tokens" % (len(words), int((ids != 0).sum(1).max())))


# ---- the state dict --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "vit_b16", "rn50"])
def test_state_dict_is_the_references(du, fixture, name):
    _, meta = fixture
    cfg = dict(meta[name + "_config"])
    if isinstance(cfg["vision_layers"], list):
        cfg["vision_layers"] = tuple(cfg["vision_layers"])
    with torch.device("meta"):
        m = du.OpenAIClip(**cfg)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta[name + "_state_dict"]
    sd = {k: torch.empty(s, device="meta") for k, s in meta[name + "_state_dict"]}
    got = du.openai_clip_config(sd)
    assert got == cfg, (got, cfg)
    assert isinstance(m.visual, du.ModifiedResNet) == (name == "rn50")


def test_the_default_is_vit_b16(du, fixture):
    _, meta = fixture
    assert du.VIT_B16 == meta["vit_b16_config"]


def openai_checkpoint(du, cfg):
    """What OpenAI distributes, in the small: fp16 tensors and the three scalar keys."""
    m = du.OpenAIClip(**cfg)
    recipe.fill(m)
    sd = {k: (v.half() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    sd.update(input_resolution=torch.tensor(cfg["image_resolution"]), context_length=torch.tensor(cfg["context_length"]),
              vocab_size=torch.tensor(cfg["vocab_size"]))
    return sd


def test_strict_load_upcasts_and_ignores_the_scalars(du):
    sd = openai_checkpoint(du, recipe.SMALL)
    m = du.OpenAIClip.from_state_dict(sd)
    assert all(v.dtype == torch.float32 for v in m.state_dict().values() if v.is_floating_point())
    assert all(torch.equal(m.state_dict()[k], v.float()) for k, v in sd.items() if k not in du._CLIP_IGNORED)
    assert (m.context_length, m.vocab_size, m.embed_dim) == (77, recipe.SMALL["vocab_size"], 64)
    model, _ = du.get_target_model("openai_clip", "cpu", ckpt=sd)
    assert isinstance(model, du.OpenAIClip) and not model.training
    missing = {k: v for k, v in sd.items() if k != "transformer.resblocks.1.mlp.c_proj.bias"}
    with pytest.raises(RuntimeError, match="Missing key.*c_proj.bias"):
        du.OpenAIClip.from_state_dict(missing)
    with pytest.raises(RuntimeError, match="Unexpected key.*surplus"):
        du.OpenAIClip.from_state_dict(dict(sd, **{"visual.surplus": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="lacks 'ln_final.weight'"):
        du.OpenAIClip.from_state_dict({k: v for k, v in sd.items() if not k.startswith("ln_final")})


def test_checkpoint_files_state_dict_and_torchscript(du, tmp_path):
    sd = openai_checkpoint(du, recipe.SMALL)
    plain = tmp_path / "small.pt"
    torch.save(sd, str(plain))
    assert not du._is_torchscript_archive(str(plain))
    a, _ = du.get_target_model("openai_clip", "cpu", ckpt=str(plain))
    # a scripted container of tensors under the same names stands in for OpenAI's archive
    root = torch.nn.Module()
    for key, v in sd.items():
        mod = root
        *path, leaf = key.split(".")
        for p in path:
            if not hasattr(mod, p):
                mod.add_module(p, torch.nn.Module())
            mod = getattr(mod, p)
        mod.register_buffer(leaf, v.clone())
    archive = tmp_path / "small_jit.pt"
    torch.jit.save(torch.jit.script(root), str(archive))
    assert du._is_torchscript_archive(str(archive))
    b, _ = du.get_target_model("openai_clip", "cpu", ckpt=str(archive))
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())


def test_without_a_checkpoint_the_target_is_seeded_vit_b16(du):
    a, _ = du.get_target_model("openai_clip", "cpu", seed=3)
    assert isinstance(a.visual, du._ClipVisionTransformer) and a.visual.conv1.bias is None
    assert a.visual.positional_embedding.shape == (197, 768) and a.text_projection.shape == (512, 512)
    b = du.OpenAIClip(**du.VIT_B16)
    assert not torch.equal(a.text_projection, b.text_projection)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        c = du.OpenAIClip(**du.VIT_B16)
    assert torch.equal(a.text_projection, c.text_projection) and torch.equal(a.visual.proj, c.visual.proj)
    assert not getattr(a, "projection", False)          # extract_and_save must not project the text features a second time


# ---- the mirror against the reference, ATen route on the CPU -----------------------------------------------------------------
def run_mirror(m, image, tokens):
    rows = {}
    eot = tokens.argmax(dim=-1)
    hooks = []
    for i, blk in enumerate(m.visual.transformer.resblocks):
        hooks.append(blk.register_forward_hook(lambda mod, a, o, i=i: rows.__setitem__("img_block%d" % i, o[:, 0].detach().clone())))
    for i, blk in enumerate(m.transformer.resblocks):
        hooks.append(blk.register_forward_hook(
            lambda mod, a, o, i=i: rows.__setitem__("txt_block%d" % i, o[torch.arange(o.shape[0]), eot].detach().clone())))
    with torch.no_grad():
        rows["image"] = m.encode_image(image)
        rows["text"] = m.encode_text(tokens)
        assert torch.equal(m(image), rows["image"])                     # forward(image) is encode_image
    for h in hooks:
        h.remove()
    return rows


def test_mirror_in_float64(du, fixture):
    z, meta = fixture
    m, sha = small_model(du, torch.float64)
    assert sha == meta["weights_sha256"]
    rows = run_mirror(m, recipe.make_image().double(), torch.from_numpy(z["ids"].astype(np.int64)))
    assert sorted(rows) == sorted(k[:-4] for k in z.files if k.endswith("_f64"))
    for k, v in rows.items():
        e = nerr(v, torch.from_numpy(z[k + "_f64"]))
        print("%s: float64 nerr %.3e" % (k, e))
        assert v.dtype == torch.float64 and e <= 1e-10, (k, e)


def test_mirror_in_fp32(du, fixture):
    z, meta = fixture
    m, sha = small_model(du)
    assert sha == meta["weights_sha256"]
    rows = run_mirror(m, recipe.make_image(), torch.from_numpy(z["ids"].astype(np.int64)))
    for k, v in rows.items():
        f64 = torch.from_numpy(z[k + "_f64"])
        assert v.dtype == torch.float32
        _bound(nerr(v, f64), nerr(torch.from_numpy(z[k + "_f32"]), f64), k)


def test_text_rows_depend_on_nothing_after_the_end_token(du, fixture):
    """The causal mask: the padding behind the end-of-text id (and what a position past it holds) does not reach its row."""
    z, _ = fixture
    m, _ = small_model(du)
    ids = torch.from_numpy(z["ids"].astype(np.int64))[:6]
    other = ids.clone()
    for r in range(6):
        other[r, int(ids[r].argmax()) + 1:] = 5
    with torch.no_grad():
        assert nerr(m.encode_text(other), m.encode_text(ids)) <= 1e-6
    with pytest.raises(ValueError, match="int64"):
        m.encode_text({"input_ids": ids})


# ---- routes and gates ------------------------------------------------------------------------------------------------------
def test_clip_tower_route_is_a_pure_gate(du, monkeypatch):
    from mammo_clip_dissect_amd import core
    ok = dict(flag=True, on_gpu=True, dtype=torch.float32, grad=False, training=False, B=4, T=77, D=512, heads=8, fused_ok=True)
    assert du.clip_tower_route(**ok) == "hip"
    for change in (dict(flag=False), dict(on_gpu=False), dict(dtype=torch.float16), dict(dtype=torch.float64), dict(grad=True),
                   dict(training=True), dict(B=0), dict(B=du.MAX_BATCH + 1), dict(T=0), dict(T=core.VIT_ATTENTION_LONG_MAX_T + 1),
                   dict(heads=4), dict(D=2112, heads=33), dict(fused_ok=False)):
        assert du.clip_tower_route(**dict(ok, **change)) == "aten", change
    assert du.clip_tower_route(**dict(ok, T=577, D=1024, heads=16)) == "hip"           # ViT-L/14@336: K9L's tokens
    assert du.HIP_CLIP_TEXT is True                                                     # MCD_NO_HIP_CLIP_TEXT is not set here


def test_towers_on_the_cpu_take_aten(du, monkeypatch):
    m, _ = small_model(du)
    ids = torch.zeros(2, 77, dtype=torch.long)
    assert m.text_route(ids) == "aten" and m.visual.route(recipe.make_image()) == "aten"
    # every other condition holds for tensors that say they are on the GPU: the switch then decides
    monkeypatch.setattr(du.core, "linear_residual_available", lambda: True)
    fake = torch.zeros(2, 77, dtype=torch.long).as_subclass(util.FakeCuda)
    w = m.token_embedding.weight
    monkeypatch.setattr(m.token_embedding, "weight", torch.nn.Parameter(w.detach().as_subclass(util.FakeCuda), requires_grad=False))
    with torch.no_grad():
        assert m.text_route(fake) == "hip"
        assert m.text_route(torch.zeros(2, 257, dtype=torch.long).as_subclass(util.FakeCuda)) == "aten"      # past K9A's 256
        monkeypatch.setattr(du, "HIP_CLIP_TEXT", False)
        assert m.text_route(fake) == "aten"
        monkeypatch.setattr(du, "HIP_CLIP_TEXT", True)
    assert m.text_route(fake) == "aten"                                                                      # autograd on
    m.train()
    with torch.no_grad():
        assert m.text_route(fake) == "aten"


def test_clip_dissector_selection(du, unregistered, tmp_path):
    from mammo_clip_dissect_amd.concept_vit import og_utils
    model, tokenize = og_utils._clip_dissector("cpu", "RN50")
    assert isinstance(model, du.ClipResNet) and isinstance(tokenize(["a mass"]), dict)            # today's objects
    model, tokenize = og_utils._clip_dissector("cpu", "ViT-B/16")
    assert isinstance(model, du.ClipViT) and tokenize(["a mass"])["input_ids"].shape[1] <= 77
    # a registered name, a path, the environment variable: OpenAI CLIP itself with its own tokenizer
    ckpt = tmp_path / "vit_small.pt"
    torch.save(openai_checkpoint(du, recipe.SMALL), str(ckpt))
    du.register_tokenizer("clip", recipe.BPE_SMALL)
    for name in (str(ckpt), "ViT-B/16"):
        if name == "ViT-B/16":
            du.register_clip_checkpoint("ViT-B/16", str(ckpt))
        model, tokenize = og_utils._clip_dissector("cpu", name)
        assert isinstance(model, du.OpenAIClip) and not model.training
        ids = tokenize(["a mass", "dots"])
        assert ids.dtype == torch.int64 and ids.shape == (2, model.context_length)
        with torch.no_grad():
            assert model.encode_text(ids).shape == (2, 64)
    assert isinstance(og_utils._clip_dissector("cpu", "RN50")[0], du.ClipResNet)                  # other names: unchanged
    assert du.clip_checkpoint("RN50") is None


def test_a_resnet_checkpoint_gets_the_real_text_side(du, unregistered, monkeypatch, tmp_path):
    from mammo_clip_dissect_amd.concept_vit import og_utils
    cfg = dict(recipe.SMALL, vision_layers=(1, 1, 1, 1), vision_width=16, vision_patch_size=None, image_resolution=64)
    ckpt = tmp_path / "rn_small.pt"
    torch.save(openai_checkpoint(du, cfg), str(ckpt))
    monkeypatch.setenv("MCD_CLIP_CKPTS", "ViT-B/16=/nowhere.pt, RN50=%s" % ckpt)
    monkeypatch.setenv("MCD_CLIP_BPE", recipe.BPE_SMALL)
    model, tokenize = og_utils._clip_dissector("cpu", "RN50")
    assert isinstance(model, du.OpenAIClip) and isinstance(model.visual, du.ModifiedResNet)
    assert model.transformer.resblocks[0].causal and hasattr(model, "ln_final")
    with torch.no_grad():
        assert model.encode_text(tokenize(["dots"])).shape == (1, 64)
        assert model.encode_image(torch.randn(1, 3, 64, 64)).shape == (1, 64)


# ---- the ABI surface -------------------------------------------------------------------------------------------------------
def test_abi_surface_lists_both_entries(mcd):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_clip.h")).read(), flags=re.S)
    assert re.search(r"int mcd_vit_attention_causal\(const float\* qkv, int64_t B, int64_t T, int64_t H, float\* out, "
                     r"mcd_stream_t stream\);", text)
    assert re.search(r"int mcd_quick_gelu\(const float\* x, int64_t n, float\* out, mcd_stream_t stream\);", text)
    assert sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text))) == sorted(mcd._lib.CLIP_SIGNATURES)
    L = mcd._lib.load()
    assert len(mcd._lib.CLIP_SIGNATURES["mcd_vit_attention_causal"][1]) == 6
    assert len(mcd._lib.CLIP_SIGNATURES["mcd_quick_gelu"][1]) == 4
    assert all(hasattr(L, n) for n in mcd._lib.CLIP_SIGNATURES) and L.mcd_abi_version() == 9
    assert not set(mcd._lib.CLIP_SIGNATURES) & (set(mcd._lib.SIGNATURES) | set(mcd._lib.TEXT_SIGNATURES))
    for header in ("mcd_hip.h", "mcd_text.h"):                       # the new entries live in their own header only
        other = open(os.path.join(ROOT, "include", header)).read()
        assert not re.search(r"int\s+(mcd_vit_attention_causal|mcd_quick_gelu)\s*\(", other)
    from mammo_clip_dissect_amd import core
    with pytest.raises(TypeError):                     # the product path has no host fallback
        core.vit_attention_causal(torch.zeros(1, 3, 192), 1)
    with pytest.raises(TypeError):
        core.quick_gelu(torch.zeros(8))


def test_entries_refuse_bad_arguments(mcd):
    P, Q = 4096, 1 << 20          # non-NULL, 16-byte aligned pointer values that no rejected call may dereference
    rc = util.entry_rc
    assert rc(mcd, "mcd_vit_attention_causal", P, 1, 0, 1, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_causal", P, 1, 257, 1, Q, None) == -5
    assert rc(mcd, "mcd_vit_attention_causal", P, 1, 8, 0, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_causal", P + 4, 1, 8, 1, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_causal", P, 1, 8, 1, Q + 8, None) == -1
    assert rc(mcd, "mcd_vit_attention_causal", None, 1, 8, 1, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_causal", P, 1, 8, 65536, Q, None) == -5
    assert rc(mcd, "mcd_vit_attention_causal", P, 0, 8, 1, Q, None) == 0               # an empty batch launches nothing
    assert rc(mcd, "mcd_quick_gelu", P, 0, Q, None) == 0                                # n = 0: a no-op
    assert rc(mcd, "mcd_quick_gelu", None, 0, None, None) == 0
    assert rc(mcd, "mcd_quick_gelu", P, -1, Q, None) == -1
    assert rc(mcd, "mcd_quick_gelu", None, 4, Q, None) == -1
    assert rc(mcd, "mcd_quick_gelu", P + 4, 4, Q, None) == -1
    assert rc(mcd, "mcd_quick_gelu", P, 4, Q + 8, None) == -1
