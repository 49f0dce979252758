"""The vocabulary, the strings, the configuration and the weights of the text-tower fixture (tests/golden/text_vocab.txt,
text_tower.npz, text_tower_meta.json), written once: the generator (tests/golden/make_golden_text.py) feeds them to
transformers' BertTokenizerFast and BertModel, the tests feed them to the mirrors in concept_vit/data_utils.py
(WordPieceTokenizer, BertTextTower inside BreastClip) through the checkpoint loader.  Weights are not stored, only the
sha256 of what this produces.

The vocabulary is our own (about 200 entries): the specials, a few [unusedN], every letter as a word and as a ## piece
(so that greedy longest-match has something to be greedy about), punctuation, whole words and pieces that cover the
concept lines below, one accented entry (reachable only without lower-casing: lower-casing strips the accent first) and
one CJK entry.  Digits are absent: a word with a digit is [UNK].

Weights are keyed by the module names of transformers 4.41.1 (the reference's pin) as a Mammo-CLIP checkpoint carries
them, text_encoder.text_encoder.*, the pooler included (BertModel has one; the mirror ignores it by name).  One seeded
torch.Generator, the keys walked in order: an embedding table 0.5 * randn; a linear weight randn / sqrt(fan_in); a
LayerNorm weight 1 + 0.2 * randn; every bias 0.1 * randn.
"""
import hashlib

import torch

SEED = 4242
PREFIX = "text_encoder.text_encoder."
PROJ_DIM = 512
CONFIG = dict(hidden=128, heads=2, layers=2, mlp=512, max_pos=64, n_type=2, eps=1e-12)
MAX_LENGTHS = (256, 8)

SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
LETTERS = "abcdefghijklmnopqrstuvwxyz"
PUNCT = list("-,.()/:;'\"!?")
WORDS = ["the", "from", "of", "and", "with", "in", "new", "no", "right", "left", "upper", "lower", "inner", "outer",
         "breast", "nipple", "distance", "foreign", "body", "including", "implant", "global", "spiral", "beige", "cement",
         "australian", "terrier", "tile", "mass", "density", "calc", "retro", "pop", "as", "popcorn", "calcification",
         "view", "skin", "focal", "benign", "naive", "naïve", "cafe", "乳", "architectural", "distortion", "cal",
         "lymph", "node", "axilla", "ab", "abc", "ret", "im"]
PIECES = ["##ification", "##de", "##ter", "##min", "##ant", "##ym", "##metry", "##corn", "##pec", "##toral", "##ing",
          "##ed", "##ly", "##al", "##ion", "##fication", "##ci", "##ro", "##plant", "##bc", "##fe", "##ve", "##ï"]


def vocabulary():
    """The lines of text_vocab.txt, in id order."""
    v = SPECIALS + ["[unused%d]" % i for i in range(1, 9)] + list(LETTERS) + ["##" + c for c in LETTERS] + PUNCT + WORDS + PIECES
    assert len(v) == len(set(v))
    return v


# a dozen lines of the package's Concepts/Specific_concepts_sorted.txt (every 64th line)
CONCEPTS = ["Australian terrier", "beige", "cement", "distance from the nipple", "foreign body including implants",
            "indeterminant calcification", "lower inner right breast", "new global asymmetry", "popcorn calcification",
            "retropectoral", "spiral", "tiles"]
EDGE = ["qu4rk density",                                        # an unknown word (no digit in the vocabulary)
        "x" + "a" * 100 + " mass",                              # a 101-character word: [UNK] whatever its pieces
        "a" * 100,                                              # 100 characters: still tokenised (100 pieces)
        "PopCorn CALCIFICATION Of The LEFT Breast",             # mixed case
        "Naïve café dénsity",                    # accents (stripped with lower-casing)
        "a-b,c",
        "",                                                     # the empty string: [CLS] [SEP]
        "distance from the nipple lower inner right breast new global asymmetry",   # truncates at max_length = 8
        "乳腺 mass\tin the  upper\nouter breast",    # CJK (one known, one unknown), odd whitespace
        "benign-appearing (focal) skin calc.\x00�\x07"]    # punctuation runs, characters that cleaning drops
STRINGS = CONCEPTS + EDGE
# the batch the tower runs on: every string but the 100-piece one, which would make T = 102 > max_pos = 64
TOWER_ROWS = [i for i, s in enumerate(STRINGS) if s != "a" * 100]


def keys(cfg=CONFIG, vocab=None):
    """[(4.41.1 key under PREFIX, shape)] of BertModel's state dict in that release's order (position_ids is a
    non-persistent buffer there: not in the dict)."""
    V = len(vocabulary()) if vocab is None else vocab
    D, M = cfg["hidden"], cfg["mlp"]

    def lin(name, o, i):
        return [(name + ".weight", (o, i)), (name + ".bias", (o,))]

    def norm(name):
        return [(name + ".weight", (D,)), (name + ".bias", (D,))]
    out = [("embeddings.word_embeddings.weight", (V, D)), ("embeddings.position_embeddings.weight", (cfg["max_pos"], D)),
           ("embeddings.token_type_embeddings.weight", (cfg["n_type"], D))] + norm("embeddings.LayerNorm")
    for i in range(cfg["layers"]):
        b = "encoder.layer.%d." % i
        out += (lin(b + "attention.self.query", D, D) + lin(b + "attention.self.key", D, D)
                + lin(b + "attention.self.value", D, D) + lin(b + "attention.output.dense", D, D)
                + norm(b + "attention.output.LayerNorm") + lin(b + "intermediate.dense", M, D)
                + lin(b + "output.dense", D, M) + norm(b + "output.LayerNorm"))
    out += lin("pooler.dense", D, D)
    return [(PREFIX + k, s) for k, s in out]


def weights(cfg=CONFIG, seed=SEED, vocab=None):
    """({key: tensor} -- the text tower's keys, then text_projection.projection.weight --, sha256 over all in order)."""
    g = torch.Generator().manual_seed(seed)
    sd, h = {}, hashlib.sha256()
    for key, shape in keys(cfg, vocab) + [("text_projection.projection.weight", (PROJ_DIM, cfg["hidden"]))]:
        leaf = key.rpartition(".")[2]
        r = torch.randn(shape, generator=g)
        if "_embeddings." in key:
            v = 0.5 * r
        elif leaf == "bias":
            v = 0.1 * r
        elif len(shape) == 1:
            v = 1 + 0.2 * r
        else:
            v = r / shape[1] ** 0.5
        sd[key] = v
        h.update(v.contiguous().numpy().tobytes())
    return sd, h.hexdigest()


def image_projection(in_dim, seed=SEED + 1):
    """image_projection.projection.weight for a checkpoint that carries both projections (not part of the fixture)."""
    r = torch.randn((PROJ_DIM, in_dim), generator=torch.Generator().manual_seed(seed))
    return {"image_projection.projection.weight": r / in_dim ** 0.5}


def bert_kwargs(cfg=CONFIG, vocab=None):
    """The constructor arguments of data_utils.BertTextTower for cfg."""
    return dict(vocab=len(vocabulary()) if vocab is None else vocab, hidden=cfg["hidden"], depth=cfg["layers"],
                mlp=cfg["mlp"], max_pos=cfg["max_pos"], n_type=cfg["n_type"], eps=cfg["eps"], heads=cfg["heads"])


def hf_tokenizer(vocab_file, do_lower_case=True):
    """transformers' BertTokenizerFast on a local vocab.txt (the generator and the live comparison).  4.x takes the file
    as vocab_file=; 5.x takes the token -> id dict as vocab= and silently ignores vocab_file (every word becomes [UNK])."""
    import inspect

    from transformers import BertTokenizerFast
    if "vocab" in inspect.signature(BertTokenizerFast.__init__).parameters:
        with open(vocab_file, encoding="utf-8") as f:
            vocab = {line.rstrip("\n"): i for i, line in enumerate(f)}
        tok = BertTokenizerFast(vocab=vocab, do_lower_case=do_lower_case)
    else:
        tok = BertTokenizerFast(vocab_file=vocab_file, do_lower_case=do_lower_case)
    assert tok.do_lower_case == do_lower_case and len(tok.get_vocab()) == len(vocabulary())
    return tok
