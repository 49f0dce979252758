"""CPU: the sentence side of get_cos_similarity -- WordPieceTokenizer under MPNet's specials against the fixture's
MPNetTokenizer ids, the bucket and position-id restatements against transformers' own, MPNetSentenceEncoder's strict load and
its ATen forward / encode() against the fixture's MPNetModel outputs (tests/golden/mpnet.npz, make_golden_mpnet.py) held to
test_text_tower_cpu's bound, the route gate as a pure function, the registries, get_cos_similarity itself and the ABI
surface of include/mcd_sentence.h.  No kernel runs here."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import openai_clip_recipe as clip_recipe
import text_recipe
import util
from util import nerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(util.GOLDEN, "mpnet_vocab.txt")
# A dot product of two fp32 unit rows of n numbers: each row's norm is 1 to within a few ulps (the sum of n squares, a square
# root, a division: (n / 2 + 2) * 2^-24 relative at worst, far less on average), the n products and adds of the dot another
# n * 2^-24.  For n = 128 (the fixture) and n = 64 (the tiny CLIP's embed_dim) that is under 2.4e-5 in the worst case; what was
# measured on the fixture strings on the CPU is a mean of exactly 1.0 on both sides (single rows are off by up to 1.2e-7).
UNIT_DOT_TOL = (128 / 2 + 2 + 128) * 2.0 ** -24 * 2


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "mpnet.npz")), json.load(open(os.path.join(util.GOLDEN, "mpnet_meta.json")))


def state_dict(z):
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}


@pytest.fixture(scope="module")
def model(du, fixture):
    return du.MPNetSentenceEncoder.from_state_dict(state_dict(fixture[0])).eval()


@pytest.fixture()
def registries(du, monkeypatch):
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    monkeypatch.setattr(du, "SENTENCE_CHECKPOINT", {})
    for name in ("MCD_MPNET_VOCAB", "MCD_MPNET_CKPT", "MCD_CLIP_BPE", "MCD_BERT_VOCAB"):
        monkeypatch.delenv(name, raising=False)


def _bound(e_got, e_aten, what):       # test_text_tower_cpu's
    print("%s: got %.3e aten %.3e ratio to the bound %.3f" % (what, e_got, e_aten, e_got / (2 * e_aten + 1e-6)))
    assert e_got <= 2 * e_aten + 1e-6, (what, e_got, e_aten)


def batch(z):
    return {"input_ids": torch.from_numpy(z["input_ids"].astype(np.int64)),
            "attention_mask": torch.from_numpy(z["attention_mask"].astype(np.int64))}


# ---- the loader ----------------------------------------------------------------------------------------------------------------
def test_strict_load_takes_every_key_and_ignores_the_pooler(du, fixture):
    z, meta = fixture
    sd = state_dict(z)
    assert sorted(sd) == sorted(k for k, _ in meta["state_dict"]) and any(k.startswith("pooler.") for k in sd)
    m = du.MPNetSentenceEncoder.from_state_dict(sd)
    own = m.state_dict()
    assert sorted(own) == sorted(k for k in sd if not k.startswith("pooler."))          # every other key is taken, none is added
    for k, v in own.items():
        assert torch.equal(v, sd[k]), k
    cfg = meta["config"]
    assert (m.heads, len(m.encoder.layer), m.out_dim) == (cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["hidden_size"])
    assert m.embeddings.word_embeddings.num_embeddings == cfg["vocab_size"]
    assert m.embeddings.position_embeddings.num_embeddings == cfg["max_position_embeddings"]
    assert m.encoder.layer[1].intermediate.dense.out_features == cfg["intermediate_size"]
    assert m.embeddings.LayerNorm.eps == 1e-5 == m.encoder.layer[0].output.LayerNorm.eps               # the default
    assert du.MPNetSentenceEncoder.from_state_dict(sd, eps=1e-12).encoder.layer[1].attention.LayerNorm.eps == 1e-12
    # embeddings.position_ids (older checkpoints store the buffer) is ignored by name as well
    du.MPNetSentenceEncoder.from_state_dict(dict(sd, **{"embeddings.position_ids": torch.arange(48)[None]}))
    with pytest.raises(RuntimeError, match="extra.weight"):
        du.MPNetSentenceEncoder.from_state_dict(dict(sd, **{"encoder.extra.weight": torch.zeros(2)}))
    with pytest.raises(RuntimeError, match="attention.attn.o.bias"):
        du.MPNetSentenceEncoder.from_state_dict({k: v for k, v in sd.items() if k != "encoder.layer.1.attention.attn.o.bias"})
    with pytest.raises(RuntimeError, match="not an MPNetModel state dict"):
        du.MPNetSentenceEncoder.from_state_dict({k: v for k, v in sd.items() if "relative_attention_bias" not in k})
    half = du.MPNetSentenceEncoder.from_state_dict({k: v.half() if v.is_floating_point() else v for k, v in sd.items()})
    assert half.embeddings.word_embeddings.weight.dtype == torch.float32                               # fp32 only


def test_module_tree_is_transformers(du, fixture):
    import transformers                              # the fixture's generator needs it too: its absence is a failure, not a skip
    z, meta = fixture
    hf = transformers.MPNetModel(transformers.MPNetConfig(**meta["config"]))
    mine = du.MPNetSentenceEncoder.from_state_dict(state_dict(z))
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items() if not k.startswith("pooler.") and not k.endswith("position_ids")}
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == want


# ---- the tokenizer -------------------------------------------------------------------------------------------------------------
def test_tokenizer_ids_are_the_fixtures(du, fixture, registries):
    z, meta = fixture
    with pytest.raises(RuntimeError, match=r"register_tokenizer\(\s*'mpnet'"):
        du.mpnet_tokenizer()
    du.register_tokenizer("mpnet", VOCAB)
    tok = du.mpnet_tokenizer()
    assert (tok.cls_id, tok.pad_id, tok.sep_id) == (0, 1, 2) and tok.unk_id == tok.vocab["[UNK]"] == 4 == tok.vocab["<unk>"] + 1
    enc = tok(meta["strings"])
    assert np.array_equal(enc["input_ids"].numpy(), z["input_ids"].astype(np.int64))
    assert np.array_equal(enc["attention_mask"].numpy(), z["attention_mask"].astype(np.int64))
    assert (z["input_ids"] == tok.unk_id).sum() >= 2 and int(z["attention_mask"][0].sum()) == 3        # [UNK] occurs; one word
    assert np.array_equal(z["input_ids"][1], z["input_ids"][2])                                        # the padded twin
    plain = du.WordPieceTokenizer(VOCAB, specials=du.MPNET_SPECIALS)                                   # the four names as given
    assert plain.unk_id == 3 and plain.encode("mass zebra") == [0, plain.vocab["mass"], 3, 2]
    with pytest.raises(ValueError, match="lacks the special tokens"):
        du.WordPieceTokenizer(VOCAB)                                                                   # BERT's are not in it


def test_the_environment_variable_registers_too(du, registries, monkeypatch):
    monkeypatch.setenv("MCD_MPNET_VOCAB", VOCAB)
    assert du.mpnet_tokenizer().encode("dense") == [0, du.mpnet_tokenizer().vocab["dense"], 2]


def test_bert_tokenizer_is_unchanged(du):
    """The default specials are BERT's: on the text fixture's strings the ids are still BertTokenizerFast's."""
    z = np.load(os.path.join(util.GOLDEN, "text_tower.npz"))
    bert_vocab = os.path.join(util.GOLDEN, "text_vocab.txt")
    tok = du.WordPieceTokenizer(bert_vocab)
    assert du.BERT_SPECIALS == ("[PAD]", "[UNK]", "[CLS]", "[SEP]")
    enc = tok(text_recipe.STRINGS, max_length=256)
    for k in ("input_ids", "token_type_ids", "attention_mask"):
        assert np.array_equal(enc[k].numpy(), z[k + "_256"].astype(np.int64)), k
    with pytest.raises(ValueError, match="lacks the special tokens"):
        du.WordPieceTokenizer(bert_vocab, specials=du.MPNET_SPECIALS)


# ---- the restated arithmetic -----------------------------------------------------------------------------------------------------
def test_buckets_equal_transformers_for_all_511_distances(du, fixture, model):
    z, _ = fixture
    d = torch.arange(-255, 256, dtype=torch.long)
    got = du.relative_position_bucket(d)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), z["buckets"].astype(np.int64))
    assert sorted(set(z["buckets"].tolist())) == [b for b in range(32) if b != 16]     # (16 would be distance +0)
    # the per-distance table IS every diagonal of the [heads, T, T] bias
    for T in (1, 7, 27):
        rel = model.encoder.rel_table(T)
        assert tuple(rel.shape) == (2, 2 * T - 1) and model.encoder.rel_table(T) is rel                # built once per T
        full = model.encoder.position_bias(T)[0]
        t = torch.arange(T)
        assert torch.equal(full, rel[:, (t[None, :] - t[:, None]) + T - 1])
        w = model.encoder.relative_attention_bias.weight
        assert torch.equal(rel, w.detach()[torch.from_numpy(z["buckets"].astype(np.int64))[255 - (T - 1):255 + T]].t())


def test_position_ids_of_a_padded_batch(du, fixture):
    z, _ = fixture
    ids = torch.from_numpy(z["input_ids"].astype(np.int64))
    got = du.mpnet_position_ids(ids)
    assert np.array_equal(got.numpy(), z["position_ids"].astype(np.int64))
    mask = torch.from_numpy(z["attention_mask"]).bool()
    assert torch.equal(got[mask], (torch.arange(ids.shape[1])[None, :] + 2).expand_as(ids)[mask]) and bool((got[~mask] == 1).all())


# ---- the ATen route against transformers ---------------------------------------------------------------------------------------------
def test_hidden_states_and_embeddings_match_transformers(model, fixture):
    z, _ = fixture
    tok = batch(z)
    with torch.no_grad():
        h = model(tok)
        e = model.embed(tok)
    mask = tok["attention_mask"].bool()
    f64 = torch.from_numpy(z["hidden_f64"])
    assert h.dtype == torch.float32 and tuple(h.shape) == tuple(mask.shape) + (128,)
    _bound(nerr(h[mask], f64), nerr(torch.from_numpy(z["hidden_f32"]), f64), "last_hidden_state, valid rows")
    e64 = torch.from_numpy(z["embed_f64"])
    _bound(nerr(e, e64), nerr(torch.from_numpy(z["embed_f32"]), e64), "sentence vectors")
    assert float((e.norm(dim=1) - 1).abs().max()) < 1e-6
    # the bias matters to the fixture: without it nothing matches
    w = model.encoder.relative_attention_bias.weight
    keep = w.detach().clone()
    try:
        with torch.no_grad():
            w.zero_()
            assert nerr(model(tok)[mask], f64) > 1e-2
    finally:
        with torch.no_grad():
            w.copy_(keep)


def test_encode_from_strings(du, model, fixture, registries, monkeypatch):
    z, meta = fixture
    strings = meta["strings"]
    monkeypatch.setattr(model, "tokenizer", None)
    with pytest.raises(RuntimeError, match="MCD_MPNET_VOCAB"):
        model.encode(strings)
    du.register_tokenizer("mpnet", VOCAB)
    a = model.encode(strings)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (len(strings), 128)
    e64 = torch.from_numpy(z["embed_f64"])
    _bound(nerr(torch.from_numpy(a), e64), nerr(torch.from_numpy(z["embed_f32"]), e64), "encode()")
    # input order, and batches padded to their own longest sequence: the rows do not depend on the batch they were in, up to the
    # summation order of ATen's matrix products at another T (a few fp32 ulps of unit rows; measured 6e-8)
    for bs in (1, 5):
        b = model.encode(strings, batch_size=bs)
        assert float(np.abs(a - b).max()) <= 1e-6, bs
    order = [7, 0, 11, 3, 3, 1]
    c = model.encode([strings[i] for i in order], batch_size=4)
    assert float(np.abs(c - a[order]).max()) <= 1e-6
    assert np.array_equal(a[1], a[2])                                                      # the padded twin, same batch
    assert model.encode(strings[4]).shape == (1, 128)                                      # one string


def test_encode_truncates_at_256_tokens_with_a_warning(du, fixture, registries, monkeypatch):
    z, _ = fixture
    sd = state_dict(z)
    sd["embeddings.position_embeddings.weight"] = torch.randn(300, 128, generator=torch.Generator().manual_seed(3)) * 0.02
    m = du.MPNetSentenceEncoder.from_state_dict(sd).eval()
    du.register_tokenizer("mpnet", VOCAB)
    seen = []
    fwd = m.embed
    monkeypatch.setattr(m, "embed", lambda tok: (seen.append(tuple(tok["input_ids"].shape)), fwd(tok))[1])
    with pytest.warns(UserWarning, match="1 of 2 sentences are over 256 tokens"):
        out = m.encode(["dense breast " * 200, "mass"])
    assert seen == [(2, 256)] and out.shape == (2, 128) and bool(np.isfinite(out).all())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.encode(["dense breast " * 100])                                                   # 202 tokens: no warning


# ---- the gate ------------------------------------------------------------------------------------------------------------------
def test_sentence_route_is_a_pure_function(du, model, fixture, monkeypatch):
    ok = dict(flag=True, on_gpu=True, dtype=torch.float32, grad=False, training=False, B=12, T=27, D=768, heads=12, pos_rows=514,
              fused_ok=True, prefix_mask=True)
    assert du.sentence_route(**ok) == "hip"
    for change in (dict(prefix_mask=False), dict(T=257), dict(dtype=torch.float16), dict(grad=True), dict(flag=False),
                   dict(on_gpu=False), dict(training=True), dict(heads=8), dict(T=256, pos_rows=257),
                   dict(fused_ok=False), dict(D=2112, heads=33), dict(B=0), dict(T=0)):
        assert du.sentence_route(**dict(ok, **change)) == "aten", change
    assert du.sentence_route(**dict(ok, T=256)) == "hip" and du.sentence_route(**dict(ok, T=256, pos_rows=258)) == "hip"
    # what the model feeds it: a left-padded mask is no key count
    z, _ = fixture
    tok = batch(z)
    assert du.prefix_mask_lengths(tok["attention_mask"]).tolist() == z["attention_mask"].sum(1).tolist()
    assert du.prefix_mask_lengths(tok["attention_mask"].flip(1)) is None
    assert model.route(tok["input_ids"], tok["attention_mask"]) == ("aten", None)          # on the CPU
    seen = {}
    monkeypatch.setattr(du, "sentence_route", lambda *a: seen.setdefault("args", a) and "aten")
    model.route(tok["input_ids"], tok["attention_mask"].flip(1))
    assert seen["args"][-1] is False and seen["args"][5:10] == (12, 27, 128, 2, 48)
    # no mask: every token is a key, and a <pad> among them takes position row 1, not t + 2 -- such ids are no prefix either
    for ids, want in ((tok["input_ids"], False), (tok["input_ids"][-1:], True), (tok["input_ids"][:1, :3], True)):
        seen.clear()
        model.route(ids, None)
        assert seen["args"][-1] is want, tuple(ids.shape)
    assert du.HIP_SENTENCE is True


# ---- the registries and the factory ----------------------------------------------------------------------------------------------
def test_sentence_encoder_factory(du, fixture, registries, tmp_path, monkeypatch):
    z, _ = fixture
    sd = state_dict(z)
    with pytest.raises(RuntimeError, match="register_sentence_checkpoint"):
        du.sentence_encoder("cpu")
    with pytest.raises(FileNotFoundError):
        du.register_sentence_checkpoint(str(tmp_path / "absent.bin"))
    path = str(tmp_path / "pytorch_model.bin")
    torch.save(sd, path)
    du.register_sentence_checkpoint(path)
    m = du.sentence_encoder("cpu")
    assert isinstance(m, du.MPNetSentenceEncoder) and not m.training
    assert torch.equal(m.encoder.relative_attention_bias.weight, sd["encoder.relative_attention_bias.weight"])
    monkeypatch.setattr(du, "SENTENCE_CHECKPOINT", {})
    monkeypatch.setenv("MCD_MPNET_CKPT", path)
    assert torch.equal(du.sentence_encoder("cpu").embeddings.LayerNorm.bias, sd["embeddings.LayerNorm.bias"])
    assert len(du.sentence_encoder("cpu", ckpt={"model": sd}).encoder.layer) == 2
    # a pickle that is not plain tensors is refused by weights_only=True
    evil = str(tmp_path / "evil.bin")
    torch.save({"embeddings.word_embeddings.weight": object()}, evil)
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|Unpickl"):
        du.sentence_encoder("cpu", ckpt=evil)
    with pytest.raises(ValueError, match="'mpnet'"):
        du.register_tokenizer("t5", VOCAB)


# ---- get_cos_similarity --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_clip(du):
    m = du.OpenAIClip(**clip_recipe.SMALL).eval()
    clip_recipe.fill(m)
    return m


def test_get_cos_similarity(mcd, du, model, tiny_clip, fixture, registries):
    from mammo_clip_dissect_amd.concept_vit import CLIP_og_utils, og_utils, utils
    assert utils.get_cos_similarity is og_utils.get_cos_similarity is CLIP_og_utils.get_cos_similarity
    strings = fixture[1]["strings"]
    preds, gt = strings, strings[3:] + strings[:3]
    du.register_tokenizer("mpnet", VOCAB)
    with pytest.raises(RuntimeError, match=r"register_tokenizer\('clip'"):             # no merges file: no hashing fallback
        utils.get_cos_similarity(preds, gt, tiny_clip, model, device="cpu")
    du.register_tokenizer("clip", clip_recipe.BPE_SMALL)
    got = utils.get_cos_similarity(preds, gt, tiny_clip, model, device="cpu", batch_size=5)
    assert isinstance(got, tuple) and len(got) == 2 and all(type(v) is float for v in got)
    # recomputed from encode_text / encode
    tok = du.clip_tokenizer()
    with torch.no_grad():
        p = tiny_clip.encode_text(tok(preds, context_length=tiny_clip.context_length))
        g = tiny_clip.encode_text(tok(gt, context_length=tiny_clip.context_length))
    p, g = p / p.norm(dim=-1, keepdim=True), g / g.norm(dim=-1, keepdim=True)
    want_clip = float((p * g).sum(1).mean())
    want_mpnet = float(np.mean(np.sum(model.encode(preds) * model.encode(gt), axis=1)))
    assert abs(got[0] - want_clip) <= 1e-6 and abs(got[1] - want_mpnet) <= 1e-6, (got, want_clip, want_mpnet)
    assert -1 <= got[0] < 1 - 1e-3 and -1 <= got[1] < 1 - 1e-3                            # different strings: not 1
    one = utils.get_cos_similarity(preds, preds, tiny_clip, model, device="cpu")
    print("preds == gt:", one[0] - 1, one[1] - 1)
    assert abs(one[0] - 1) <= UNIT_DOT_TOL and abs(one[1] - 1) <= UNIT_DOT_TOL, one
    # batch_size does not change the pairing
    whole = utils.get_cos_similarity(preds, gt, tiny_clip, model, device="cpu", batch_size=200)
    assert abs(whole[0] - got[0]) <= 1e-6 and abs(whole[1] - got[1]) <= 1e-6
    # a string over the context length is an error, as in clip.tokenize
    with pytest.raises(RuntimeError, match="too long for context length"):
        utils.get_cos_similarity([clip_recipe.LONG], [clip_recipe.LONG], tiny_clip, model, device="cpu")


# ---- the bindings and the ABI surface ----------------------------------------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors(mcd):
    from mammo_clip_dissect_amd import core
    with pytest.raises(TypeError):
        core.vit_attention_relbias(torch.zeros(1, 4, 192), 1, None, torch.zeros(1, 7))
    with pytest.raises(TypeError):
        core.masked_mean_l2(torch.zeros(2, 5, 8), None)


def test_abi_surface(mcd):
    lib = mcd._lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcd_sentence.h")).read(), flags=re.S)
    assert re.search(r"int mcd_vit_attention_relbias\(const float\* qkv, int64_t B, int64_t T, int64_t H, const int32_t\* lens,\s*"
                     r"const float\* rel\s*, float\* out, mcd_stream_t stream\);", text)
    assert re.search(r"int mcd_masked_mean_l2\(const float\* x, int B, int T, int D, const int32_t\* lens\s*, int normalize,\s*"
                     r"float\* out, mcd_stream_t stream\);", text)
    names = ["mcd_masked_mean_l2", "mcd_vit_attention_relbias"]
    assert sorted(set(re.findall(r"\b(mcd_[a-z0-9_]+)\s*\(", text))) == sorted(lib.SENTENCE_SIGNATURES) == names
    assert len(lib.SENTENCE_SIGNATURES["mcd_vit_attention_relbias"][1]) == len(lib.TEXT_SIGNATURES["mcd_vit_attention_keylen"][1]) + 1
    assert len(lib.SENTENCE_SIGNATURES["mcd_masked_mean_l2"][1]) == 8
    L = lib.load()
    assert all(hasattr(L, n) for n in names) and L.mcd_abi_version() == 9
    tables = [lib.SIGNATURES, lib.TEXT_SIGNATURES, lib.CLIP_SIGNATURES, lib.TOKEN_SIGNATURES, lib.SENTENCE_SIGNATURES,
              lib.CACHE_SIGNATURES]
    assert len(set().union(*tables)) == sum(len(t) for t in tables)                 # disjoint
    for header in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if header != "mcd_sentence.h":
            other = open(os.path.join(ROOT, "include", header)).read()
            assert not re.search(r"mcd_(vit_attention_relbias|masked_mean_l2)\s*\(", other), header


def test_entries_refuse_bad_arguments_before_any_device_call(mcd):
    rc = lambda name, *a: util.entry_rc(mcd, name, *a)
    P, Q, R = 4096, 8192, 16384                 # aligned non-NULL addresses: the checks return before anything is touched
    assert rc("mcd_vit_attention_relbias", None, 1, 4, 1, None, R, Q, None) == -1
    assert rc("mcd_vit_attention_relbias", P, 1, 0, 1, None, R, Q, None) == -1
    assert rc("mcd_vit_attention_relbias", P, 1, 257, 1, None, R, Q, None) == -5
    assert rc("mcd_vit_attention_relbias", P, 1, 4, 1, None, R + 4, Q, None) == -1
    assert rc("mcd_vit_attention_relbias", P, 1, 4, 1, 2, R, Q, None) == -1
    assert rc("mcd_vit_attention_relbias", P, 0, 4, 1, None, R, Q, None) == 0
    assert rc("mcd_masked_mean_l2", None, 1, 4, 8, None, 1, Q, None) == -1
    assert rc("mcd_masked_mean_l2", P, 1, 4, 6, None, 1, Q, None) == -1
    assert rc("mcd_masked_mean_l2", P, 1, 0, 8, None, 1, Q, None) == -1
    assert rc("mcd_masked_mean_l2", P, 1, 4, 8, None, 2, Q, None) == -1
    assert rc("mcd_masked_mean_l2", P, 1, 4, 2052, None, 1, Q, None) == -5
    assert rc("mcd_masked_mean_l2", P, 1, 4, 8, None, 1, P + 64, None) == -1              # out inside x
    assert rc("mcd_masked_mean_l2", P + 4, 1, 4, 8, None, 1, Q, None) == -1
    assert rc("mcd_masked_mean_l2", P, -1, 4, 8, None, 1, Q, None) == -1
    assert rc("mcd_masked_mean_l2", None, 0, 4, 8, None, 1, None, None) == 0
