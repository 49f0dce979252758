"""The weights and the inputs of the CLIPForImageClassification fixture (tests/golden/hf_clip.npz), written once: the
generator (tests/golden/make_golden_hf_clip.py) fills transformers' model with them, the tests fill the mirror
(data_utils.HFClip).  Nothing is stored but the sha256 of what this produces (hf_clip_meta.json).

One seeded torch.Generator, the state dict walked in SORTED key order (the order in which a module registers its
parameters is then no part of the recipe):
  * LayerNorm (pre_layrnorm, post_layernorm, layer_norm1, layer_norm2): weight 1 + 0.2 * randn, bias 0.1 * randn;
  * a linear / convolution weight: randn / sqrt(fan_in) (the product of all dimensions but the first);
  * a linear bias: 0.1 * randn;
  * class_embedding and position_embedding.weight: 0.5 * randn.
"""
import hashlib

import torch

# constructor arguments of data_utils.HFClip
# SMALL: 2 heads, 2 layers, 16 patches + the class token = 17 tokens, no multiple of K9's 32-query block
SMALL = dict(num_labels=5, image_size=64, patch=16, hidden=128, layers=2, heads=2, mlp=512)
# LONG: 17 x 17 patches + the class token = 290 tokens: K9L's second query block, K26 over more than 256 rows
LONG = dict(num_labels=5, image_size=272, patch=16, hidden=128, layers=1, heads=2, mlp=512)
VIT_B16 = dict(num_labels=2, image_size=224, patch=16, hidden=768, layers=12, heads=12, mlp=3072)
CONFIGS = {"small": SMALL, "long": LONG, "vit_b16": VIT_B16}
BATCH = {"small": 3, "long": 2}
SEED = {"small": 2026, "long": 2027}
INPUT_SEED = {"small": 13, "long": 14}


def hf_config_kwargs(cfg):
    """The same configuration as the arguments of transformers' CLIPVisionConfig."""
    return dict(hidden_size=cfg["hidden"], intermediate_size=cfg["mlp"], num_hidden_layers=cfg["layers"],
                num_attention_heads=cfg["heads"], image_size=cfg["image_size"], patch_size=cfg["patch"],
                hidden_act="quick_gelu", layer_norm_eps=1e-5)


def fill(model, seed):
    """Fill `model` (any module with CLIPForImageClassification's state dict) in place; returns the sha256 over all filled
    tensors."""
    g = torch.Generator().manual_seed(seed)
    h = hashlib.sha256()
    sd = model.state_dict()
    with torch.no_grad():
        for key in sorted(sd):
            t = sd[key]
            mod, _, leaf = key.rpartition(".")
            name = mod.rpartition(".")[2]
            if not t.is_floating_point():
                continue
            r = torch.randn(t.shape, generator=g)
            if "norm" in name:                                   # pre_layrnorm, post_layernorm, layer_norm1, layer_norm2
                v = 1 + 0.2 * r if leaf == "weight" else 0.1 * r
            elif leaf == "class_embedding" or name == "position_embedding":
                v = 0.5 * r
            elif leaf == "bias":
                v = 0.1 * r
            else:
                v = r / t[0].numel() ** 0.5
            t.copy_(v.to(t.dtype))
            h.update(v.float().contiguous().numpy().tobytes())
    return h.hexdigest()


def make_image(name):
    res = CONFIGS[name]["image_size"]
    return torch.randn(BATCH[name], 3, res, res, generator=torch.Generator().manual_seed(INPUT_SEED[name]))


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
