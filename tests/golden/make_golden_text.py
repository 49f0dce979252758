"""Generator of tests/golden/text_vocab.txt, text_tower.npz and text_tower_meta.json: what transformers' BertTokenizerFast
and BertModel -- the classes behind the reference's tokenizer and text encoder (model/clip.py:81-101,
model/modules/text_encoder.py:37,48) -- say about the mirrors WordPieceTokenizer and BertTextTower in
concept_vit/data_utils.py.

    python tests/golden/make_golden_text.py

Both are built locally from the recipe (tests/text_recipe.py): BertTokenizerFast on the recipe's vocabulary
(recipe.hf_tokenizer; do_lower_case True is its default), BertModel(config) filled with the recipe's weights, which are keyed by
the module names of transformers 4.41.1, the reference's pin (installed_name: the explicit table for a release that
renamed a module; BERT's names have not moved so far).  Nothing is downloaded.  Outputs are data only:
  * text_vocab.txt: the vocabulary, one token per line;
  * text_tower.npz: input_ids / token_type_ids / attention_mask of the recipe's strings at max_length 256 and 8 (and, for
    the cased path, the ids at do_lower_case=False), last_hidden_state of the tower batch in fp32 and in float64, and
    the pooled ('eos', 'bos', 'mean': model/clip.py:66-77) and projected features in both;
  * text_tower_meta.json: the versions, the configuration, the sha256 of the weights, the 4.41.1 key / shape list read
    back from the transformers model and checked against the recipe's.
"""
import json
import os
import re
import sys

import numpy as np
import torch
import transformers
from transformers import BertConfig, BertModel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import text_recipe as recipe  # noqa: E402

RENAMED = []      # (pattern on the 4.41.1 key, replacement) for an installed release that renamed a BERT module: none so far


def installed_name(key, have):
    if key in have:
        return key
    for pat, new in RENAMED:
        k2, n = re.subn(pat, new, key)
        if n and k2 in have:
            return k2
    raise KeyError("no name in transformers %s for %s" % (transformers.__version__, key))


def pool(f, mask, how):
    if how == "eos":
        return f[torch.arange(f.shape[0]), mask.sum(dim=-1) - 1]
    if how == "bos":
        return f[:, 0]
    m = mask.unsqueeze(-1).expand(f.size()).to(f.dtype)
    return torch.sum(f * m, dim=1) / torch.clamp(m.sum(dim=1), min=1e-9)


def main():
    vocab_file = os.path.join(HERE, "text_vocab.txt")
    with open(vocab_file, "w", encoding="utf-8") as f:
        f.write("\n".join(recipe.vocabulary()) + "\n")
    out = {}
    for lower in (True, False):
        tok = recipe.hf_tokenizer(vocab_file, lower)
        for L in recipe.MAX_LENGTHS:
            enc = tok(recipe.STRINGS, max_length=L, padding=True, truncation=True, return_tensors="pt")
            tag = "%s%d" % ("" if lower else "cased_", L)
            for k in ("input_ids", "token_type_ids", "attention_mask"):
                assert enc[k].dtype == torch.int64
                out["%s_%s" % (k, tag)] = enc[k].numpy().astype(np.int16 if k == "input_ids" else np.int8)
            print(tag, tuple(enc["input_ids"].shape))

    cfg = recipe.CONFIG
    V = len(recipe.vocabulary())
    torch.manual_seed(0)
    model = BertModel(BertConfig(vocab_size=V, hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"],
                                 num_attention_heads=cfg["heads"], intermediate_size=cfg["mlp"],
                                 max_position_embeddings=cfg["max_pos"], type_vocab_size=cfg["n_type"],
                                 layer_norm_eps=cfg["eps"], hidden_act="gelu")).eval()
    sd, sha = recipe.weights()
    have = model.state_dict()
    bert = {k[len(recipe.PREFIX):]: v for k, v in sd.items() if k.startswith(recipe.PREFIX)}
    persistent = [k for k in have if not k.endswith("position_ids")]
    key_list = [[recipe.PREFIX + k, list(have[installed_name(k, have)].shape)] for k in bert]
    assert len(key_list) == len(persistent) and key_list == [[k, list(s)] for k, s in recipe.keys()]
    model.load_state_dict({installed_name(k, have): v for k, v in bert.items()}, strict=False)
    proj = sd["text_projection.projection.weight"]

    rows = recipe.TOWER_ROWS
    ids = torch.from_numpy(out["input_ids_256"].astype(np.int64))[rows]
    mask = torch.from_numpy(out["attention_mask_256"].astype(np.int64))[rows]
    keep = int(mask.sum(dim=1).max())                       # padded to the longest of THIS batch
    ids, mask = ids[:, :keep].contiguous(), mask[:, :keep].contiguous()
    out["tower_rows"] = np.asarray(rows, np.int16)
    out["tower_T"] = np.asarray(keep, np.int16)
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        m = model.to(dt)
        with torch.no_grad():
            h = m(input_ids=ids, attention_mask=mask, token_type_ids=torch.zeros_like(ids)).last_hidden_state
            out["hidden_" + name] = h.numpy()
            for how in ("eos", "bos", "mean"):
                out["feat_%s_%s" % (how, name)] = (pool(h, mask, how) @ proj.to(dt).t()).numpy()
    model.float()
    print("tower", tuple(out["hidden_f64"].shape), float(np.abs(out["hidden_f64"]).max()),
          float(np.abs(out["hidden_f32"] - out["hidden_f64"]).max()))
    np.savez_compressed(os.path.join(HERE, "text_tower.npz"), **out)
    meta = {"seed": recipe.SEED, "config": cfg, "vocab_size": V, "weights_sha256": sha, "state_dict": key_list,
            "strings": len(recipe.STRINGS), "transformers": transformers.__version__, "tokenizers": __import__("tokenizers").__version__,
            "torch": torch.__version__, "key_names": "transformers 4.41.1", "do_lower_case": True}
    with open(os.path.join(HERE, "text_tower_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
