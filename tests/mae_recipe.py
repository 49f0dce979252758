"""The weights and the inputs of the ViTMAEForPreTraining fixture (tests/golden/mae.npz), written once: the generator
(tests/golden/make_golden_mae.py) fills transformers' model with them, the tests fill the mirror (data_utils.HFMae) through
its checkpoint loader.  Weights are not stored, only the sha256 of what this produces (mae_meta.json).

Weights are keyed by the module names of transformers 4.41.1, the reference's pin (keys()), which is what a real
facebook/vit-mae-base checkpoint carries.  One seeded torch.Generator, the keys walked in order:
  * a linear / convolution weight: randn / sqrt(fan_in) (fan_in = the product of all dimensions but the first);
  * a LayerNorm weight: 1 + 0.2 * randn; every bias: 0.1 * randn;
  * cls_token, mask_token, position_embeddings, decoder_pos_embed: 0.5 * randn -- the two tables are NOT the sin-cos tables
    a model builds for itself, so a mirror that regenerated them instead of loading them misses every number.
The noise of a configuration is a seeded random permutation of 0 .. L-1 divided by L for every image: distinct values, so
argsort has no ties on any device.
"""
import hashlib

import torch

# constructor arguments of data_utils.HFMae
# SMALL: 4 x 4 patches of 8 pixels (K11's 16-byte path), len_keep = 4: 5 encoder tokens, 17 decoder tokens
SMALL = dict(image_size=32, patch=8, hidden=128, layers=2, heads=2, mlp=512, decoder_hidden=64, decoder_layers=1,
             decoder_heads=2, decoder_mlp=256)
# ODD: 5 x 5 patches of 6 pixels (K11's 8-byte path), len_keep = int(6.25) = 6: 7 encoder tokens, 26 decoder tokens
ODD = dict(image_size=30, patch=6, hidden=128, layers=2, heads=2, mlp=512, decoder_hidden=64, decoder_layers=1,
           decoder_heads=2, decoder_mlp=256)
BASE = dict(image_size=224, patch=16, hidden=768, layers=12, heads=12, mlp=3072, decoder_hidden=512, decoder_layers=8,
            decoder_heads=16, decoder_mlp=2048)                              # facebook/vit-mae-base
CONFIGS = {"small": SMALL, "odd": ODD, "vit-mae-base": BASE}
NORM_PIX_LOSS = {"small": False, "odd": True}
MASK_RATIO = 0.75
BATCH = 3
SEED = {"small": 2031, "odd": 2032}
INPUT_SEED = {"small": 21, "odd": 22}
NOISE_SEED = {"small": 31, "odd": 32}


def hf_config_kwargs(cfg, norm_pix_loss=False):
    """The same configuration as the arguments of transformers' ViTMAEConfig."""
    return dict(hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                intermediate_size=cfg["mlp"], image_size=cfg["image_size"], patch_size=cfg["patch"],
                decoder_hidden_size=cfg["decoder_hidden"], decoder_num_hidden_layers=cfg["decoder_layers"],
                decoder_num_attention_heads=cfg["decoder_heads"], decoder_intermediate_size=cfg["decoder_mlp"],
                mask_ratio=MASK_RATIO, norm_pix_loss=norm_pix_loss, hidden_act="gelu", layer_norm_eps=1e-12)


def _layer(base, D, M):
    def lin(name, o, i):
        return [(base + name + ".weight", (o, i)), (base + name + ".bias", (o,))]

    def norm(name):
        return [(base + name + ".weight", (D,)), (base + name + ".bias", (D,))]
    return (lin("attention.attention.query", D, D) + lin("attention.attention.key", D, D)
            + lin("attention.attention.value", D, D) + lin("attention.output.dense", D, D) + lin("intermediate.dense", M, D)
            + lin("output.dense", D, M) + norm("layernorm_before") + norm("layernorm_after"))


def keys(cfg):
    """[(key, shape)] of the 4.41.1 state dict of ViTMAEForPreTraining in the configuration cfg, in that release's order."""
    D, P, W = cfg["hidden"], cfg["patch"], cfg["decoder_hidden"]
    n = (cfg["image_size"] // P) ** 2
    out = [("vit.embeddings.cls_token", (1, 1, D)), ("vit.embeddings.position_embeddings", (1, n + 1, D)),
           ("vit.embeddings.patch_embeddings.projection.weight", (D, 3, P, P)),
           ("vit.embeddings.patch_embeddings.projection.bias", (D,))]
    for i in range(cfg["layers"]):
        out += _layer("vit.encoder.layer.%d." % i, D, cfg["mlp"])
    out += [("vit.layernorm.weight", (D,)), ("vit.layernorm.bias", (D,)), ("decoder.mask_token", (1, 1, W)),
            ("decoder.decoder_pos_embed", (1, n + 1, W)), ("decoder.decoder_embed.weight", (W, D)),
            ("decoder.decoder_embed.bias", (W,))]
    for i in range(cfg["decoder_layers"]):
        out += _layer("decoder.decoder_layers.%d." % i, W, cfg["decoder_mlp"])
    out += [("decoder.decoder_norm.weight", (W,)), ("decoder.decoder_norm.bias", (W,)),
            ("decoder.decoder_pred.weight", (P * P * 3, W)), ("decoder.decoder_pred.bias", (P * P * 3,))]
    return out


def weights(cfg, seed):
    """({4.41.1 key: tensor}, sha256 over all of them in order)."""
    g = torch.Generator().manual_seed(seed)
    sd, h = {}, hashlib.sha256()
    for key, shape in keys(cfg):
        leaf = key.rpartition(".")[2]
        r = torch.randn(shape, generator=g)
        if leaf == "bias":
            v = 0.1 * r
        elif leaf == "weight" and len(shape) == 1:
            v = 1 + 0.2 * r
        elif leaf == "weight":
            v = r / r[0].numel() ** 0.5
        else:                                            # cls_token, mask_token, the two position tables
            v = 0.5 * r
        sd[key] = v
        h.update(v.contiguous().numpy().tobytes())
    return sd, h.hexdigest()


def len_keep(cfg):
    return int((cfg["image_size"] // cfg["patch"]) ** 2 * (1 - MASK_RATIO))


def make_image(name):
    res = CONFIGS[name]["image_size"]
    return torch.randn(BATCH, 3, res, res, generator=torch.Generator().manual_seed(INPUT_SEED[name]))


def make_noise(name, batch=BATCH):
    L = (CONFIGS[name]["image_size"] // CONFIGS[name]["patch"]) ** 2
    g = torch.Generator().manual_seed(NOISE_SEED[name])
    return torch.stack([torch.randperm(L, generator=g) for _ in range(batch)]).float() / L


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
