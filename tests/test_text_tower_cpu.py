"""CPU: Mammo-CLIP's real text side -- WordPieceTokenizer against the fixture's BertTokenizerFast ids (and a live
BertTokenizerFast where transformers imports), BertTextTower's CPU forward and the three poolings against the fixture's
BertModel outputs (tests/golden/text_tower.npz) held to the project's bound with transformers' fp32 output as the ATen
side, the checkpoint loader on the fixture's 4.41.1 key list (strict on the text side, bert selected by the checkpoint's
keys), the prefix-mask gate, the vocabulary requirement and the ABI surface.  No kernel runs here."""
import json
import os
import re

import numpy as np
import pytest
import torch

import text_recipe as recipe
import util
from util import nerr as _nerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(util.GOLDEN, "text_vocab.txt")
KEYS = ("input_ids", "token_type_ids", "attention_mask")


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "text_tower.npz")), json.load(open(os.path.join(util.GOLDEN, "text_tower_meta.json")))


@pytest.fixture()
def vocab(du, monkeypatch):
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    monkeypatch.delenv("MCD_BERT_VOCAB", raising=False)
    du.register_tokenizer("bert", VOCAB)


def _bound(e_got, e_aten, what):       # test_vit_family_cpu's
    print("%s: got %.3e aten %.3e ratio to the bound %.3f" % (what, e_got, e_aten, e_got / (2 * e_aten + 1e-6)))
    assert e_got <= 2 * e_aten + 1e-6, (what, e_got, e_aten)


def checkpoint(extra=None):
    sd, sha = recipe.weights()
    sd = dict(sd)
    sd.update(extra or {})
    return sd, sha


@pytest.fixture(scope="module")
def bert_clip(du):
    """BreastClip built by the factory from a {'model': state dict} container whose text keys select the BERT tower."""
    sd, _ = checkpoint()
    model, _ = du.get_target_model("breastclip", "cpu", ckpt={"model": sd})
    return model


def tower_batch(z):
    rows, T = z["tower_rows"].astype(np.int64), int(z["tower_T"])
    return {k: torch.from_numpy(z[k + "_256"].astype(np.int64)[rows][:, :T].copy()) for k in KEYS}


# ---- the tokenizer ---------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_recipe_says(fixture):
    z, meta = fixture
    assert open(VOCAB, encoding="utf-8").read().split("\n")[:-1] == recipe.vocabulary()
    assert meta["vocab_size"] == len(recipe.vocabulary()) and 150 <= meta["vocab_size"] <= 250
    assert meta["config"] == recipe.CONFIG and meta["strings"] == len(recipe.STRINGS)
    assert os.path.getsize(os.path.join(util.GOLDEN, "text_tower.npz")) < 1000000
    lines = set(open(os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")).read().split("\n"))
    assert len(recipe.CONCEPTS) == 12 and all(c in lines for c in recipe.CONCEPTS)
    assert any(len(w) == 101 for s in recipe.STRINGS for w in s.split()) and "" in recipe.STRINGS
    # the edge cases do what they are there for: an [UNK], a truncation at 8 that cuts real tokens, a ragged batch
    unk = recipe.vocabulary().index("[UNK]")
    assert (z["input_ids_256"] == unk).any() and z["attention_mask_8"].sum(1).max() == 8 < z["attention_mask_256"].sum(1).max()
    assert len(set(z["attention_mask_256"].sum(1).tolist())) > 4


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("max_length", recipe.MAX_LENGTHS)
def test_tokenizer_matches_the_fixture(du, fixture, lower, max_length):
    z, _ = fixture
    tok = du.WordPieceTokenizer(VOCAB, do_lower_case=lower)
    assert tok.vocab_size == len(recipe.vocabulary())
    got = tok(recipe.STRINGS, max_length=max_length, padding=True, truncation=True)
    assert list(got) == list(KEYS)
    for k in KEYS:
        ref = z["%s_%s%d" % (k, "" if lower else "cased_", max_length)]
        assert got[k].dtype == torch.int64 and tuple(got[k].shape) == ref.shape, k
        bad = np.nonzero((got[k].numpy() != ref).any(axis=1))[0]
        assert bad.size == 0, "%s differs for %r" % (k, [recipe.STRINGS[i][:40] for i in bad])
    sep = tok.sep_id                                     # [SEP] survives the truncation: the last valid token of every row
    last = got["attention_mask"].sum(1) - 1
    assert bool((got["input_ids"][torch.arange(len(recipe.STRINGS)), last] == sep).all())
    one = tok("tiles", max_length=max_length)            # a single string is a batch of one
    assert one["input_ids"].tolist() == [[tok.cls_id, tok.vocab["tile"], tok.vocab["##s"], sep]]


@pytest.mark.parametrize("lower", [True, False])
def test_tokenizer_matches_a_live_bert_tokenizer_fast(du, lower):
    pytest.importorskip("transformers")
    hf = recipe.hf_tokenizer(VOCAB, lower)
    tok = du.WordPieceTokenizer(VOCAB, do_lower_case=lower)
    extra = ["Mass, with  (architectural) distortion;no 'lymph' node!?", "ABC abc aBc ab", "naïve NAÏVE", "im-plant/implanted"]
    for L in recipe.MAX_LENGTHS + (5,):
        ref = hf(recipe.STRINGS + extra, max_length=L, padding=True, truncation=True, return_tensors="pt")
        got = tok(recipe.STRINGS + extra, max_length=L, padding=True, truncation=True)
        for k in KEYS:
            assert torch.equal(got[k], ref[k]), (k, L)


def test_tokenizer_needs_its_special_tokens(du, tmp_path):
    p = tmp_path / "vocab.txt"
    p.write_text("[PAD]\n[UNK]\n[CLS]\nthe\n")
    with pytest.raises(ValueError, match=r"lacks the special tokens \['\[SEP\]'\]"):
        du.WordPieceTokenizer(str(p))


# ---- the tower ---------------------------------------------------------------------------------------------------------------
def test_factory_selects_the_bert_tower_from_the_checkpoint_keys(du, bert_clip, fixture):
    _, meta = fixture
    m = bert_clip
    assert m.text_tower == "bert" and isinstance(m.text_encoder, du.HFTextEncoder) and not m.training
    t = m.text_encoder.text_encoder
    assert isinstance(t, du.BertTextTower) and m.text_encoder.out_dim == 128 == m.text_projection.projection.in_features
    cfg = recipe.CONFIG
    assert (t.heads, len(t.encoder.layer)) == (cfg["hidden"] // 64, cfg["layers"]) == (2, 2)
    emb = t.embeddings
    assert emb.word_embeddings.num_embeddings == meta["vocab_size"] and emb.position_embeddings.num_embeddings == 64
    assert t.encoder.layer[1].intermediate.dense.out_features == 512 and emb.LayerNorm.eps == 1e-12
    # the mirror's keys are the fixture's 4.41.1 list, minus the pooler it ignores by name
    mine = [k for k in m.state_dict() if k.startswith("text_encoder.")]
    want = [k for k, _ in meta["state_dict"] if ".pooler." not in k]
    assert mine == want and len(want) == len(meta["state_dict"]) - 2
    assert [list(m.state_dict()[k].shape) for k in mine] == [s for k, s in meta["state_dict"] if ".pooler." not in k]
    sd, sha = checkpoint()
    assert sha == meta["weights_sha256"]
    for k in want + ["text_projection.projection.weight"]:
        assert torch.equal(m.state_dict()[k], sd[k]), k


def test_cpu_forward_matches_transformers(bert_clip, fixture):
    z, _ = fixture
    tok = tower_batch(z)
    with torch.no_grad():
        h = bert_clip.text_encoder(tok)
    f64 = torch.from_numpy(z["hidden_f64"])
    assert tuple(h.shape) == tuple(f64.shape) and h.dtype == torch.float32
    _bound(_nerr(h, f64), _nerr(torch.from_numpy(z["hidden_f32"]), f64), "last_hidden_state")


@pytest.mark.parametrize("pooling", ["eos", "bos", "mean"])
def test_poolings_match_transformers(bert_clip, fixture, monkeypatch, pooling):
    z, _ = fixture
    tok = tower_batch(z)
    assert bert_clip.text_pooling == "eos"
    monkeypatch.setattr(bert_clip, "text_pooling", pooling)
    with torch.no_grad():
        f = bert_clip.text_projection(bert_clip.encode_text(tok))
    f64 = torch.from_numpy(z["feat_%s_f64" % pooling])
    _bound(_nerr(f, f64), _nerr(torch.from_numpy(z["feat_%s_f32" % pooling]), f64), pooling)
    others = [p for p in ("eos", "bos", "mean") if p != pooling]
    assert all(_nerr(f, torch.from_numpy(z["feat_%s_f64" % p])) > 1e-2 for p in others)      # the three differ
    monkeypatch.setattr(bert_clip, "text_pooling", "cls")
    with pytest.raises(NotImplementedError):
        bert_clip.encode_text(tok)
    with pytest.raises(ValueError, match="must be a dictionary"):
        bert_clip.encode_text(tok["input_ids"])


def test_encode_text_from_strings_matches_the_fixture(bert_clip, fixture, vocab):
    """The whole text path as the drivers run it: tokenize -> encode_text -> text_projection.  With the text keys dropped
    (strict=False on a tower with other names) these are the stand-in's features and nothing matches."""
    z, _ = fixture
    strings = [recipe.STRINGS[i] for i in z["tower_rows"]]
    tok = bert_clip.tokenize(strings)
    for k in KEYS:
        assert torch.equal(tok[k], tower_batch(z)[k]), k
    with torch.no_grad():
        f = bert_clip.text_projection(bert_clip.encode_text(tok))
    f64 = torch.from_numpy(z["feat_eos_f64"])
    _bound(_nerr(f, f64), _nerr(torch.from_numpy(z["feat_eos_f32"]), f64), "encode_text + projection")


# ---- the loader --------------------------------------------------------------------------------------------------------------
def test_loader_ignores_pooler_and_position_ids_and_nothing_else(du):
    sd, _ = checkpoint({recipe.PREFIX + "embeddings.position_ids": torch.arange(64)[None]})
    assert recipe.PREFIX + "pooler.dense.weight" in sd
    m, _ = du.get_target_model("breastclip", "cpu", ckpt=sd)            # a bare state dict as well
    assert m.text_tower == "bert"

    missing = {k: v for k, v in sd.items() if k != recipe.PREFIX + "encoder.layer.1.output.dense.bias"}
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\) \['text_encoder.text_encoder.encoder.layer.1.output.dense.bias'\]"):
        du.get_target_model("breastclip", "cpu", ckpt=missing)
    renamed = dict(missing)
    renamed[recipe.PREFIX + "encoder.layer.1.output.dense.beta"] = sd[recipe.PREFIX + "encoder.layer.1.output.dense.bias"]
    with pytest.raises(RuntimeError, match=r"1 missing key\(s\).*1 unexpected key\(s\) \['text_encoder.text_encoder.encoder.layer.1.output.dense.beta'\]"):
        du.get_target_model("breastclip", "cpu", ckpt=renamed)
    stray = dict(sd)
    stray["text_encoder.norm.weight"] = torch.ones(128)                 # a stand-in tower's key
    with pytest.raises(RuntimeError, match="unexpected"):
        du.get_target_model("breastclip", "cpu", ckpt=stray)
    with pytest.raises(RuntimeError, match="missing"):                  # asked for by name, absent from the checkpoint
        du.get_target_model("breastclip", "cpu", ckpt={"image_projection.projection.weight": torch.zeros(512, 2048)},
                            text_tower="bert")
    with pytest.raises(ValueError, match="text_tower"):
        du.get_target_model("breastclip", "cpu", text_tower="clip")


def test_the_stand_in_stays_the_default(du, mcd):
    from mammo_clip_dissect_amd.concept_vit import utils
    m, _ = du.get_target_model("breastclip_vit", "cpu")
    assert m.text_tower == "stand-in" and isinstance(m.text_encoder, du.TextTower) and isinstance(m.tokenizer, du.HashTokenizer)
    assert m.text_pooling == "eos"
    assert [k for k in m.state_dict() if k.startswith("text_encoder.")][:3] == ["text_encoder.word.weight", "text_encoder.pos.weight",
                                                                               "text_encoder.norm.weight"]
    # a checkpoint without text_encoder.text_encoder.* keys keeps it, and so does asking for it by name
    sd = {"text_projection.projection.weight": torch.zeros(512, 768)}
    assert du.get_target_model("breastclip_vit", "cpu", ckpt=sd)[0].text_tower == "stand-in"
    full, _ = checkpoint()
    m2, _ = du.get_target_model("breastclip_vit", "cpu", ckpt={k: v for k, v in full.items() if k.startswith(recipe.PREFIX)},
                                text_tower="stand-in")
    assert m2.text_tower == "stand-in" and isinstance(m2.text_encoder, du.TextTower)
    # the CLIP dissectors keep the stand-in
    assert isinstance(du.get_target_model("clip", "cpu")[0].text_model, du.TextTower)
    # build_mammo_models passes the choice through
    clip_model, target = utils.build_mammo_models("breastclip_vit", "cpu", breast_clip_ckh=full)
    assert clip_model is target and clip_model.text_tower == "bert"
    text_only = {k: v for k, v in full.items() if k.startswith(recipe.PREFIX)}
    assert utils.build_mammo_models("breastclip_vit", "cpu", breast_clip_ckh=text_only, text_tower="stand-in")[0].text_tower == "stand-in"


def test_config_is_read_from_the_checkpoint_shapes(du):
    cfg = dict(recipe.CONFIG, hidden=192, layers=3, mlp=256, max_pos=40)
    sd, _ = recipe.weights(cfg, vocab=77)
    got = du.bert_config_from_state_dict(sd)
    assert got == dict(vocab=77, hidden=192, depth=3, mlp=256, max_pos=40, n_type=2)
    m, _ = du.get_target_model("breastclip", "cpu", ckpt=sd)
    assert m.text_encoder.text_encoder.heads == 3 and len(m.text_encoder.text_encoder.encoder.layer) == 3


# ---- the gate ----------------------------------------------------------------------------------------------------------------
def test_prefix_mask_gate(du):
    ok = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [1, 0, 0, 0]])
    lens = du.prefix_mask_lengths(ok)
    assert lens.dtype == torch.int32 and lens.tolist() == [4, 2, 1]
    assert du.prefix_mask_lengths(ok.bool()).tolist() == [4, 2, 1] and du.prefix_mask_lengths(ok[:1]).tolist() == [4]
    for bad in ([[1, 0, 1, 1]], [[0, 1, 1, 1]], [[1, 1, 1, 1], [0, 0, 0, 0]], [[1, 1, 0, 1], [1, 1, 1, 1]]):
        assert du.prefix_mask_lengths(torch.tensor(bad)) is None, bad
    assert du.prefix_mask_lengths(torch.ones(2, 3, 4)) is None


def test_text_route_conditions(du, bert_clip, monkeypatch):
    t = bert_clip.text_encoder.text_encoder
    ids = torch.zeros(2, 5, dtype=torch.long)
    assert du.text_route(t, ids) == "aten"                                   # a host tower
    monkeypatch.setattr(du.core, "linear_residual_available", lambda: True)
    fake = ids.as_subclass(util.FakeCuda)
    w = t.embeddings.word_embeddings.weight
    monkeypatch.setattr(t.embeddings.word_embeddings, "weight", torch.nn.Parameter(w.detach().as_subclass(util.FakeCuda)))
    with torch.no_grad():
        assert du.text_route(t, fake) == "hip"
        assert du.text_route(t, ids) == "aten"                               # the ids beside the weights
        assert du.text_route(t, torch.zeros(2, 65, dtype=torch.long).as_subclass(util.FakeCuda)) == "aten"   # 64 position rows
        monkeypatch.setattr(t, "heads", 1)
        assert du.text_route(t, fake) == "aten"                              # head width 128
        monkeypatch.setattr(t, "heads", 2)
        monkeypatch.setattr(du, "HIP_TEXT", False)
        assert du.text_route(t, fake) == "aten"
        monkeypatch.setattr(du, "HIP_TEXT", True)
        monkeypatch.setattr(du.core, "linear_residual_available", lambda: False)
        assert du.text_route(t, fake) == "aten"
        monkeypatch.setattr(du.core, "linear_residual_available", lambda: True)
        t.train()
        assert du.text_route(t, fake) == "aten"
        t.eval()
    assert du.text_route(t, fake) == "aten"                                  # autograd on
    t256 = du.BertTextTower(vocab=8, hidden=64, depth=1, mlp=64, max_pos=512).eval()
    monkeypatch.setattr(t256.embeddings.word_embeddings, "weight",
                        torch.nn.Parameter(t256.embeddings.word_embeddings.weight.detach().as_subclass(util.FakeCuda)))
    with torch.no_grad():
        assert du.text_route(t256, torch.zeros(1, 256, dtype=torch.long).as_subclass(util.FakeCuda)) == "hip"
        assert du.text_route(t256, torch.zeros(1, 257, dtype=torch.long).as_subclass(util.FakeCuda)) == "aten"


# ---- the vocabulary ------------------------------------------------------------------------------------------------------------
def test_a_bert_tower_without_a_vocabulary_raises(du, monkeypatch, tmp_path):
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    monkeypatch.delenv("MCD_BERT_VOCAB", raising=False)
    m = du.BreastClip("vit", text_tower="bert", bert_config=recipe.bert_kwargs())
    assert m.tokenizer is None
    with pytest.raises(RuntimeError, match="register_tokenizer.*MCD_BERT_VOCAB.*no fallback"):
        m.tokenize(["mass"])
    assert m.tokenizer is None
    monkeypatch.setenv("MCD_BERT_VOCAB", VOCAB)                              # the environment variable serves too
    assert m.tokenize("tiles")["input_ids"].shape == (1, 4) and isinstance(m.tokenizer, du.WordPieceTokenizer)
    with pytest.raises(ValueError, match="'bert'"):
        du.register_tokenizer("clip", VOCAB)
    # a vocabulary larger than the embedding table is refused while the ids are on the host
    big = tmp_path / "vocab.txt"
    big.write_text("\n".join(recipe.vocabulary() + ["zebra"]) + "\n", encoding="utf-8")
    du.register_tokenizer("bert", str(big), do_lower_case=True)
    m2 = du.BreastClip("vit", text_tower="bert", bert_config=recipe.bert_kwargs())
    assert m2.tokenize("tiles")["input_ids"].shape == (1, 4)
    with pytest.raises(ValueError, match="embedding table has %d rows" % len(recipe.vocabulary())):
        m2.tokenize("zebra")


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_abi_surface_lists_both_entries(mcd):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_text.h")).read(), flags=re.S)
    assert re.search(r"int mcd_vit_attention_keylen\(const float\* qkv, int64_t B, int64_t T, int64_t H,\s+const int32_t\* lens, "
                     r"float\* out,\s+mcd_stream_t stream\);", text)
    assert re.search(r"int mcd_text_embed_ln\(const int64_t\* ids, const int64_t\* type_ids\s*, const float\* word,\s+const float\* pos, "
                     r"const float\* type, const float\* gamma, const float\* beta, float eps, int64_t rows,\s+int64_t T, int64_t D, "
                     r"int64_t vocab, int64_t n_type, float\* out, mcd_stream_t stream\);", text)
    assert sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text))) == sorted(mcd._lib.TEXT_SIGNATURES)
    L = mcd._lib.load()
    assert len(mcd._lib.TEXT_SIGNATURES["mcd_vit_attention_keylen"][1]) == 7
    assert len(mcd._lib.TEXT_SIGNATURES["mcd_text_embed_ln"][1]) == 15
    assert all(hasattr(L, n) for n in mcd._lib.TEXT_SIGNATURES) and L.mcd_abi_version() == 9
    assert not set(mcd._lib.TEXT_SIGNATURES) & set(mcd._lib.SIGNATURES)
    from mammo_clip_dissect_amd import core
    with pytest.raises(TypeError):                     # the product path has no host fallback
        core.vit_attention_keylen(torch.zeros(1, 3, 192), 1, None)
    with pytest.raises(TypeError):
        core.text_embed_ln(torch.zeros(1, 3, dtype=torch.long), None, *[torch.zeros(4, 4)] * 3, torch.zeros(4), torch.zeros(4), 1e-12)


def test_entries_refuse_bad_arguments(mcd):
    P, Q = 4096, 1 << 20          # non-NULL, 16-byte aligned pointer values that no rejected call may dereference
    rc = util.entry_rc
    assert rc(mcd, "mcd_vit_attention_keylen", P, 1, 257, 1, None, Q, None) == -5
    assert rc(mcd, "mcd_vit_attention_keylen", P, 1, 0, 1, None, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_keylen", P + 4, 1, 8, 1, None, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_keylen", P, 1, 8, 1, P + 2, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_keylen", None, 1, 8, 1, None, Q, None) == -1
    assert rc(mcd, "mcd_vit_attention_keylen", P, 0, 8, 1, None, Q, None) == 0            # an empty batch launches nothing
    ok = (P, None, P, P, P, P, P, 1e-12)
    assert rc(mcd, "mcd_text_embed_ln", *ok, 0, 4, 8, 10, 2, Q, None) == 0
    assert rc(mcd, "mcd_text_embed_ln", *ok, 4, 4, 6, 10, 2, Q, None) == -5               # D % 4
    assert rc(mcd, "mcd_text_embed_ln", *ok, 4, 4, 2052, 10, 2, Q, None) == -5
    assert rc(mcd, "mcd_text_embed_ln", *ok, 4, 0, 8, 10, 2, Q, None) == -1
    assert rc(mcd, "mcd_text_embed_ln", *ok, 4, 4, 8, 0, 2, Q, None) == -1
    assert rc(mcd, "mcd_text_embed_ln", None, None, P, P, P, P, P, 1e-12, 4, 4, 8, 10, 2, Q, None) == -1
    assert rc(mcd, "mcd_text_embed_ln", P + 4, None, P, P, P, P, P, 1e-12, 4, 4, 8, 10, 2, Q, None) == -1
    assert rc(mcd, "mcd_text_embed_ln", P, None, P, P + 4, P, P, P, 1e-12, 4, 4, 8, 10, 2, Q, None) == -1
