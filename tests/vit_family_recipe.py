"""The weights and the inputs of the HF ViT / DINOv2 fixture (tests/golden/vit_family.npz), written once: the generator
(tests/golden/make_golden_vit_family.py) fills transformers' ViTForImageClassification / Dinov2ForImageClassification with
them, the tests fill the mirrors in concept_vit/data_utils.py (HFViT, HFDinov2) through the checkpoint loader.  Weights
are not stored, only the sha256 of what this produces (vit_family_meta.json).

Weights are keyed by the module names of transformers 4.41.1, the reference's pin (keys()), which is what a checkpoint of
the reference's models carries.  One seeded torch.Generator, the keys walked in order:
  * a linear / convolution weight: randn / sqrt(fan_in) (fan_in = the product of all dimensions but the first);
  * a LayerNorm weight: 1 + 0.2 * randn; every bias: 0.1 * randn;
  * LayerScale's lambda1: 1 + 0.2 * randn -- around 1, not transformers' constant init, so that a dropped or a doubled
    lambda moves every output;
  * cls_token, position_embeddings, mask_token: 0.5 * randn (a position table that interpolation visibly changes).
Inputs are multiples of 1/16 in [-3, 3], so that the 224 x 224 one can be stored as int8 (inputs()).
"""
import hashlib

import torch

SEED, INPUT_SEED, BATCH = 2025, 11, 2
# head width 64 everywhere (hidden / heads): the width K9 / K9L / K9C are built for
VIT_SMALL = dict(hidden=128, heads=2, layers=2, mlp=512, image=64, patch=16, labels=2)
DINO_SMALL = dict(hidden=128, heads=2, layers=2, mlp=512, image=70, patch=14, labels=2)
VIT_BASE = dict(hidden=768, heads=12, layers=12, mlp=3072, image=224, patch=16, labels=2)
DINO_BASE = dict(hidden=768, heads=12, layers=12, mlp=3072, image=224, patch=14, labels=2)
CONFIGS = {"vit_small": ("vit", VIT_SMALL), "dino_small": ("dino", DINO_SMALL), "vit_base": ("vit", VIT_BASE),
           "dino_base": ("dino", DINO_BASE)}
# case -> (configuration, H, W): 17 tokens; 26 (the table as it is); 25 and 257 (interpolated; 257: K9L, one-query last block)
CASES = {"vit": ("vit_small", 64, 64), "dino70": ("dino_small", 70, 70), "dino56x84": ("dino_small", 56, 84),
         "dino224": ("dino_small", 224, 224)}
INPUT_SCALE = 16.0


def keys(kind, cfg):
    """[(key, shape)] of the 4.41.1 state dict of ViTForImageClassification (kind 'vit') or Dinov2ForImageClassification
    ('dino') in the configuration cfg, in that release's order."""
    D, M, P = cfg["hidden"], cfg["mlp"], cfg["patch"]
    n = (cfg["image"] // P) ** 2
    top = "vit" if kind == "vit" else "dinov2"
    out = [(top + ".embeddings.cls_token", (1, 1, D))]
    if kind == "dino":
        out.append((top + ".embeddings.mask_token", (1, D)))
    out += [(top + ".embeddings.position_embeddings", (1, n + 1, D)),
            (top + ".embeddings.patch_embeddings.projection.weight", (D, 3, P, P)),
            (top + ".embeddings.patch_embeddings.projection.bias", (D,))]

    def lin(name, o, i):
        return [(name + ".weight", (o, i)), (name + ".bias", (o,))]

    def norm(name):
        return [(name + ".weight", (D,)), (name + ".bias", (D,))]
    for i in range(cfg["layers"]):
        b = "%s.encoder.layer.%d." % (top, i)
        attn = (lin(b + "attention.attention.query", D, D) + lin(b + "attention.attention.key", D, D)
                + lin(b + "attention.attention.value", D, D) + lin(b + "attention.output.dense", D, D))
        if kind == "vit":
            out += (attn + lin(b + "intermediate.dense", M, D) + lin(b + "output.dense", D, M)
                    + norm(b + "layernorm_before") + norm(b + "layernorm_after"))
        else:
            out += (norm(b + "norm1") + attn + [(b + "layer_scale1.lambda1", (D,))] + norm(b + "norm2")
                    + lin(b + "mlp.fc1", M, D) + lin(b + "mlp.fc2", D, M) + [(b + "layer_scale2.lambda1", (D,))])
    out += norm(top + ".layernorm")
    out += lin("classifier", cfg["labels"], D if kind == "vit" else 2 * D)
    return out


def weights(kind, cfg, seed=SEED):
    """({4.41.1 key: tensor}, sha256 over all of them in order)."""
    g = torch.Generator().manual_seed(seed)
    sd, h = {}, hashlib.sha256()
    for key, shape in keys(kind, cfg):
        leaf = key.rpartition(".")[2]
        r = torch.randn(shape, generator=g)
        if leaf == "bias":
            v = 0.1 * r
        elif leaf == "lambda1" or (leaf == "weight" and len(shape) == 1):
            v = 1 + 0.2 * r
        elif leaf == "weight":
            v = r / r[0].numel() ** 0.5
        else:
            v = 0.5 * r
        sd[key] = v
        h.update(v.contiguous().numpy().tobytes())
    return sd, h.hexdigest()


def mirror_kwargs(cfg):
    """The constructor arguments of data_utils.HFViT / HFDinov2 for cfg."""
    return dict(num_labels=cfg["labels"], image_size=cfg["image"], patch=cfg["patch"], dim=cfg["hidden"],
                depth=cfg["layers"], heads=cfg["heads"], mlp=cfg["mlp"])


def make_input_q(case, seed=INPUT_SEED):
    """The int8 form of a case's input: x = q / INPUT_SCALE."""
    _, H, W = CASES[case]
    g = torch.Generator().manual_seed(seed * 1000 + sorted(CASES).index(case))
    return torch.randint(-48, 49, (BATCH, 3, H, W), generator=g, dtype=torch.int64).to(torch.int8)


def dequantize(q):
    return torch.as_tensor(q).float() / INPUT_SCALE


def make_input(case, seed=INPUT_SEED):
    return dequantize(make_input_q(case, seed))


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
