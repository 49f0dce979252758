"""Generator of tests/golden/mpnet_vocab.txt, mpnet.npz and mpnet_meta.json: what transformers' own MPNetTokenizer and
MPNetModel, and sentence-transformers' Pooling(mean) + Normalize written out below, say about the mirrors in
concept_vit/data_utils.py (WordPieceTokenizer with MPNet's specials, MPNetSentenceEncoder).

Run once on the CPU where transformers is installed:
    python tests/golden/make_golden_mpnet.py
Nothing is downloaded.  The model is MPNetModel(MPNetConfig(hidden 128, 2 heads, 2 layers, intermediate 256, 48 positions,
the vocabulary below, layer_norm_eps 1e-5 as in all-mpnet-base-v2's configuration)) under torch.manual_seed(SEED).  Three
things are done to the seeded state dict, stated because they bound what the fixture proves:
  * transformers initialises every bias and LayerNorm offset to zero, every LayerNorm gain to one and the relative
    attention bias to N(0, 0.02), under which a wrong bias or a dropped offset would hide: the relative attention bias is
    redrawn from N(0, 1), the biases and LayerNorm offsets from N(0, 0.1), the gains from 1 + N(0, 0.1);
  * the padding rows (index 1) of the two embedding tables are redrawn as well (transformers zeroes them; a trained
    checkpoint holds whatever training left there), so a position id that is off by one shows;
  * every tensor is rounded to the nearest bfloat16 and stored as float32: the low 16 bits are zero and the compressed
    state dict (301 568 numbers) fits the repository's file limit.  transformers computes with exactly these fp32 values.
The token ids come from the installed MPNetTokenizer built from the vocabulary file (it is a tokenizers-backed class in
the installed release and builds offline from `vocab=path`).  Its unknown token is '[UNK]', not '<unk>' -- the
constructor's default, and what all-mpnet-base-v2's tokenizer configuration says -- so the vocabulary holds both, as
all-mpnet-base-v2's does, and data_utils.mpnet_tokenizer() takes '[UNK]' where the vocabulary has it.
The float64 pass keeps everything in float64 (MPNetSelfAttention's softmax takes its input's dtype).
Outputs are data only:
  * mpnet_vocab.txt: the vocabulary, one token per line;
  * mpnet.npz: the state dict (sd/<key>), input_ids and attention_mask of the strings padded to the longest, the position
    ids transformers derives, the bucket of every distance -255 .. 255, and in fp32 and float64 the VALID rows of
    last_hidden_state (hidden_*: [sum of the lengths, hidden], sequence after sequence -- the padded rows are left out,
    nothing reads them and they are half of the bytes) and the unit sentence vectors (embed_*);
  * mpnet_meta.json: the strings, the configuration, the state dict's keys and shapes, the versions.
"""
import json
import os

import numpy as np
import torch
import transformers
from transformers import MPNetConfig, MPNetModel, MPNetTokenizer
from transformers.models.mpnet.modeling_mpnet import MPNetEncoder, create_position_ids_from_input_ids

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2718
CONFIG = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, max_position_embeddings=48,
              layer_norm_eps=1e-5)       # all-mpnet-base-v2's eps (MPNetConfig's own default is 1e-12); a state dict does not hold it

WORDS = """the a an of in on with and or is are no there left right upper lower outer inner breast mass masses dense density
calc ##ification ##ifications ##s ##es ##ed ##ing ##ly round oval irregular margin margins spic ##ulated circum ##scribed
obscured micro ##lob asymmetry focal global architectural distortion skin thick ##ening nipple retraction lymph node
nodes axillary benign malignant suspicious cluster linear branch segment ##al fine pleo ##morphic amorphous coarse
heterogeneous fat tissue fibro ##glandular scattered extremely implant marker view cc mlo bird dog cat red blue
striped texture 1 2 3 cm mm""".split()
PUNCT = list(".,-:/()")
VOCAB = ["<s>", "<pad>", "</s>", "<unk>", "[UNK]"] + WORDS + PUNCT + ["<mask>"]

STRINGS = [
    "mass",                                                       # one word
    "dense breast tissue",
    "dense breast tissue   ",                                     # differs from the one above in padding only
    "An irregular mass with spiculated margins in the upper outer left breast.",
    "fine pleomorphic calcifications, clustered",
    "there is no suspicious mass, calcification or architectural distortion",
    "skin thickening and nipple retraction",
    "Benign axillary lymph nodes (right).",
    "scattered fibroglandular densities",
    "a red striped bird",
    "zebra crossing: unknownword in the CC/MLO views",            # [UNK] twice
    "heterogeneously dense breasts with a 2 cm oval circumscribed mass and coarse linear branching calcifications in a "
    "segmental cluster",
]


def pooled(h, mask):
    """sentence-transformers Pooling(pooling_mode_mean_tokens) then Normalize, written out."""
    m = mask.unsqueeze(-1).expand(h.size()).to(h.dtype)
    e = torch.sum(h * m, 1) / torch.clamp(m.sum(1), min=1e-9)
    return torch.nn.functional.normalize(e, p=2, dim=1)


def main():
    assert len(set(VOCAB)) == len(VOCAB)
    vocab_file = os.path.join(HERE, "mpnet_vocab.txt")
    with open(vocab_file, "w", encoding="utf-8") as f:
        f.write("\n".join(VOCAB) + "\n")
    tok = MPNetTokenizer(vocab=vocab_file)
    assert tok.unk_token == "[UNK]" and tok.pad_token_id == 1
    enc = tok(STRINGS, padding=True, truncation=True, max_length=256, return_tensors="pt")
    ids, mask = enc["input_ids"], enc["attention_mask"]
    assert int(ids.max()) < len(VOCAB) and ids.shape[1] + 2 <= CONFIG["max_position_embeddings"]

    torch.manual_seed(SEED)
    model = MPNetModel(MPNetConfig(vocab_size=len(VOCAB), **CONFIG)).eval()
    assert model.config.layer_norm_eps == 1e-5 and model.config.hidden_act == "gelu"
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k == "encoder.relative_attention_bias.weight":
                p.copy_(torch.randn(p.shape, generator=g))
            elif k.endswith("LayerNorm.weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif k.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
        for emb in (model.embeddings.word_embeddings, model.embeddings.position_embeddings):
            emb.weight[1].copy_(0.02 * torch.randn(emb.weight.shape[1], generator=g))
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    out = {"sd/" + k: v.numpy() for k, v in sd.items()}
    out["input_ids"] = ids.numpy().astype(np.int16)
    out["attention_mask"] = mask.numpy().astype(np.int8)
    out["position_ids"] = create_position_ids_from_input_ids(ids, 1).numpy().astype(np.int16)
    d = torch.arange(-255, 256, dtype=torch.long)
    out["buckets"] = MPNetEncoder.relative_position_bucket(d, num_buckets=32).numpy().astype(np.int8)
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        m = model.to(dt)
        with torch.no_grad():
            h = m(input_ids=ids, attention_mask=mask).last_hidden_state
        out["hidden_" + name] = h[mask.bool()].numpy()
        out["embed_" + name] = pooled(h, mask).numpy()
    model.float()
    print("hidden", out["hidden_f64"].shape, float(np.abs(out["hidden_f32"] - out["hidden_f64"]).max()),
          "lens", mask.sum(1).tolist())
    np.savez_compressed(os.path.join(HERE, "mpnet.npz"), **out)
    meta = {"seed": SEED, "config": dict(CONFIG, vocab_size=len(VOCAB)), "strings": STRINGS,
            "state_dict": [[k, list(v.shape)] for k, v in sd.items()], "transformers": transformers.__version__,
            "tokenizers": __import__("tokenizers").__version__, "torch": torch.__version__, "unk_token": tok.unk_token}
    with open(os.path.join(HERE, "mpnet_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("bytes", os.path.getsize(os.path.join(HERE, "mpnet.npz")))


if __name__ == "__main__":
    main()
