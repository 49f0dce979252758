"""Generator of tests/golden/clip_bpe_small.txt.gz, openai_clip.npz and openai_clip_meta.json: what the REFERENCE's CLIP
(concept_vit/clip/model.py:239-383) and its tokenizer (clip/simple_tokenizer.py, clip.tokenize at clip/clip.py:196-232) say
about the mirror in concept_vit/data_utils.py (OpenAIClip, ClipBPETokenizer).

Run where the reference is checked out (MCD_REFERENCE; default: a directory `reference` beside the repository):
    python tests/golden/make_golden_openai_clip.py
The reference's clip/model.py and clip/simple_tokenizer.py are imported at generation time, by file path; no line of them
is copied.  Two things are put in their way, both stated here because they bound what the fixture proves:
  * the tokenizer imports ftfy, which this build does not have: a stub module whose fix_text is the identity stands in.  The
    recipe's strings are ones that ftfy leaves alone (NFC, no curly quotes, no ligatures, no control characters but a tab and
    a newline), so the stub is sound for them and for nothing else;
  * the reference's LayerNorm casts its input to fp32 (it exists for fp16 runs), which a float64 model cannot run: for the
    float64 pass alone its forward is nn.LayerNorm's own.  clip.tokenize is a module-level function bound to the full merges
    file; its framing (start id, ids, end id, zero padding, the error, the truncation) is done here with the reference
    tokenizer's encoder and encode(), which is what that function calls.
Outputs are data only:
  * clip_bpe_small.txt.gz: the header line and the first 4 000 merge lines of the reference's merges file, read by the
    reference's SimpleTokenizer(bpe_path=...) as it is;
  * openai_clip_meta.json: the state-dict keys and shapes of the reference's CLIP in ViT-B/16's, RN50's and the small
    configuration, and the sha256 of the recipe's weights and image input;
  * openai_clip.npz: the reference tokenizer's ids on the small file for the recipe's strings (the one that is too long:
    its truncate=True row, and the fact that it raises); for the small configuration on the recipe's weights the
    reference's encode_image, encode_text and the class-token / end-of-text rows of every block's output, fp32 and float64.
Weights are not stored: the recipe regenerates them.
"""
import gzip
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import openai_clip_recipe as recipe  # noqa: E402

REF = os.environ.get("MCD_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
CLIP_DIR = os.path.join(REF, "concept_vit", "clip")


def reference_module(name):
    spec = importlib.util.spec_from_file_location("ref_clip_" + name, os.path.join(CLIP_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_small_merges():
    with gzip.open(os.path.join(CLIP_DIR, "bpe_simple_vocab_16e6.txt.gz")) as f:
        lines = f.read().decode("utf-8").split("\n")[:1 + recipe.N_MERGES]
    with open(recipe.BPE_SMALL, "wb") as f:                       # mtime=0: the same bytes on every run
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
            z.write("\n".join(lines).encode("utf-8"))             # no trailing newline: no empty merge line


def tokenize(tok, texts, context, truncate=False):
    sot, eot = tok.encoder["<|startoftext|>"], tok.encoder["<|endoftext|>"]
    out = np.zeros((len(texts), context), dtype=np.int64)
    for i, text in enumerate(texts):
        ids = [sot] + tok.encode(text) + [eot]
        if len(ids) > context:
            if not truncate:
                raise RuntimeError("too long: %r" % (text,))
            ids = ids[:context]
            ids[-1] = eot
        out[i, :len(ids)] = ids
    return out


def shapes(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items()]


def run(model, image, tokens):
    """encode_image, encode_text and, per block, the class-token row (image) and the end-of-text row (text) of its output
    -- the reference's blocks see [T, B, D]."""
    rows = {}
    eot = tokens.argmax(dim=-1)
    hooks = []
    for i, blk in enumerate(model.visual.transformer.resblocks):
        hooks.append(blk.register_forward_hook(lambda m, a, o, i=i: rows.__setitem__("img_block%d" % i, o[0].detach().clone())))
    for i, blk in enumerate(model.transformer.resblocks):
        hooks.append(blk.register_forward_hook(
            lambda m, a, o, i=i: rows.__setitem__("txt_block%d" % i, o[eot, torch.arange(o.shape[1])].detach().clone())))
    with torch.no_grad():
        rows["image"] = model.encode_image(image)
        rows["text"] = model.encode_text(tokens)
    for h in hooks:
        h.remove()
    return rows


def main():
    sys.modules.setdefault("ftfy", types.SimpleNamespace(fix_text=lambda text: text))     # see the docstring
    ref = reference_module("model")
    ref_tok = reference_module("simple_tokenizer")
    write_small_merges()
    tok = ref_tok.SimpleTokenizer(bpe_path=recipe.BPE_SMALL)
    assert len(tok.encoder) == recipe.SMALL["vocab_size"], len(tok.encoder)
    ctx = recipe.SMALL["context_length"]
    short = [s for i, s in enumerate(recipe.STRINGS) if i != recipe.LONG_ROW]
    raised = False
    try:
        tokenize(tok, [recipe.STRINGS[recipe.LONG_ROW]], ctx)
    except RuntimeError:
        raised = True
    assert raised
    ids = np.concatenate([tokenize(tok, short, ctx), tokenize(tok, [recipe.STRINGS[recipe.LONG_ROW]], ctx, truncate=True)])
    out = {"ids": ids.astype(np.int32), "long_row": np.int64(recipe.LONG_ROW)}

    def config(c):
        return (c["embed_dim"], c["image_resolution"], c["vision_layers"], c["vision_width"], c["vision_patch_size"],
                c["context_length"], c["vocab_size"], c["transformer_width"], c["transformer_heads"], c["transformer_layers"])
    jsonable = lambda c: {k: list(v) if isinstance(v, tuple) else v for k, v in c.items()}       # noqa: E731
    torch.manual_seed(0)
    meta = {"vit_b16_config": jsonable(recipe.VIT_B16), "vit_b16_state_dict": shapes(ref.CLIP(*config(recipe.VIT_B16))),
            "rn50_config": jsonable(recipe.RN50), "rn50_state_dict": shapes(ref.CLIP(*config(recipe.RN50))),
            "small_config": jsonable(recipe.SMALL), "seed": recipe.SEED, "input_seed": recipe.INPUT_SEED, "batch": recipe.BATCH,
            "n_merges": recipe.N_MERGES, "strings": len(recipe.STRINGS)}
    small = ref.CLIP(*config(recipe.SMALL)).eval()
    meta["weights_sha256"] = recipe.fill(small)
    meta["small_state_dict"] = shapes(small)
    image = recipe.make_image()
    meta["image_sha256"] = recipe.sha256(image)
    tokens = torch.from_numpy(ids)
    r32 = run(small, image, tokens)
    ref.LayerNorm.forward = torch.nn.LayerNorm.forward                                    # the float64 pass: see the docstring
    r64 = run(small.double(), image.double(), tokens)
    for k in r32:
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, k
        out[k + "_f32"], out[k + "_f64"] = r32[k].numpy(), r64[k].numpy()
    meta["torch"] = torch.__version__
    np.savez_compressed(os.path.join(HERE, "openai_clip.npz"), **out)
    with open(os.path.join(HERE, "openai_clip_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: v.shape for k, v in out.items()})
    print({k: float(np.abs(out[k + "_f32"] - out[k + "_f64"]).max() / np.abs(out[k + "_f64"]).max()) for k in r32})


if __name__ == "__main__":
    main()
