"""The weights, the inputs and the strings of the OpenAI-CLIP fixture (tests/golden/openai_clip.npz), written once: the
generator (tests/golden/make_golden_openai_clip.py) fills the reference's CLIP with them, the tests fill the mirror
(data_utils.OpenAIClip).  Nothing is stored but the sha256 of what this produces (openai_clip_meta.json).

One seeded torch.Generator, the state dict walked in key order:
  * LayerNorm (ln_1, ln_2, ln_pre, ln_post, ln_final): weight 1 + 0.2 * randn, bias 0.1 * randn;
  * a linear / convolution weight and in_proj_weight: randn / sqrt(fan_in) (the product of all dimensions but the first);
  * a linear bias and in_proj_bias: 0.1 * randn;
  * token_embedding.weight: randn; positional_embedding (both towers) and class_embedding: 0.5 * randn -- token and position
    both matter to every row;
  * proj and text_projection ([width, embed_dim]): randn / sqrt(width);
  * logit_scale is left alone.
"""
import hashlib
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
BPE_SMALL = os.path.join(HERE, "golden", "clip_bpe_small.txt.gz")     # the header + the first N_MERGES merge lines
N_MERGES = 4000
# the small configuration: 2 heads, 2 layers, 16 patches + the class token, context 77 = three query waves of K9A
SMALL = dict(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=128, vision_patch_size=16, context_length=77,
             vocab_size=256 + 256 + N_MERGES + 2, transformer_width=128, transformer_heads=2, transformer_layers=2)
VIT_B16 = dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=16, context_length=77,
               vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12)
RN50 = dict(embed_dim=1024, image_resolution=224, vision_layers=(3, 4, 6, 3), vision_width=64, vision_patch_size=None,
            context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12)
SEED, INPUT_SEED, BATCH = 2025, 11, 3

LONG = " ".join(["architectural distortion with spiculated margins and pleomorphic calcifications"] * 6)
# Strings on which ftfy.fix_text is the identity (NFC, no curly quotes, no ligatures, no control characters but a tab and a
# newline, which it keeps): the generator runs the reference's tokenizer with a stub for it.
STRINGS = [
    # concepts of Concepts/Specific_concepts_sorted.txt
    "Australian terrier", "axe", "breast", "dots", "high-density mass low-density mass", "mammary gland", "penguins",
    "scooters", "thick vessels", "keyhole sign (teardrop, noose)", "postoperative seroma/hematoma",
    "postoperative seroma or hematoma",
    # contractions, apostrophes elsewhere
    "the patient's scan", "it isn't dense", "they're benign", "we've seen", "I'm sure", "she'll return", "he'd said",
    "'quoted'", "rock 'n' roll", "don't!'s",
    # digits (one piece each), a number character that is no digit
    "BI-RADS 4", "12345 67", "3.5 cm x 2 cm", "area in cm\u00b2 10\u00b2", "4th of 2nd",
    # letters outside ASCII
    "caf\u00e9 cr\u00e8me", "stra\u00dfe", "\u00c5ngstr\u00f6m", "na\u00efve CAF\u00c9",
    # punctuation runs, the special strings' neighbourhood
    "wait... what?!", "a--b__c", "(((nested)))", "#1 @home $5 50%", "<|x|> <a|b>",
    # entities, once and twice escaped
    "salt &amp; pepper", "a &amp;lt; b", "&lt;tag&gt;",
    # white space
    "  leading", "trailing   ", "doubled  spaces\there\nnewline", "non\u00a0breaking\u2003space", "",
    LONG,
]
LONG_ROW = len(STRINGS) - 1       # raises at context 77; its truncate=True row is stored


def fill(model, seed=SEED):
    """Fill `model` (any module with CLIP's state dict) in place; returns the sha256 over all filled tensors."""
    g = torch.Generator().manual_seed(seed)
    h = hashlib.sha256()
    with torch.no_grad():
        for key, t in model.state_dict().items():
            mod, _, leaf = key.rpartition(".")
            name = mod.rpartition(".")[2]
            if key == "logit_scale" or leaf == "num_batches_tracked":
                continue
            r = torch.randn(t.shape, generator=g)
            if name.startswith("ln_"):
                v = 1 + 0.2 * r if leaf == "weight" else 0.1 * r
            elif leaf in ("bias", "in_proj_bias"):
                v = 0.1 * r
            elif key == "token_embedding.weight":
                v = r
            elif leaf in ("positional_embedding", "class_embedding"):
                v = 0.5 * r
            elif leaf in ("proj", "text_projection"):
                v = r / t.shape[0] ** 0.5
            else:
                v = r / t[0].numel() ** 0.5
            t.copy_(v.to(t.dtype))
            h.update(v.float().contiguous().numpy().tobytes())
    return h.hexdigest()


def make_image(res=SMALL["image_resolution"], batch=BATCH, seed=INPUT_SEED):
    return torch.randn(batch, 3, res, res, generator=torch.Generator().manual_seed(seed))


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
