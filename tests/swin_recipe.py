"""The weights and the inputs of the SwinModel fixture (tests/golden/swin.npz), written once: the generator
(tests/golden/make_golden_swin.py) fills transformers' model with them, the tests fill the mirror (data_utils.SwinTower)
through its checkpoint loader.  Weights are not stored, only the sha256 of what this produces (swin_meta.json).

Weights are keyed by the module names of transformers 4.41.1, the reference's pin (keys()), which is what a Mammo-CLIP
Swin checkpoint carries under image_encoder.image_encoder.  One seeded torch.Generator, the keys walked in order:
  * a linear / convolution weight: randn / sqrt(fan_in) (fan_in = the product of all dimensions but the first);
  * a LayerNorm weight: 1 + 0.2 * randn; every bias: 0.1 * randn;
  * relative_position_bias_table: 0.5 * randn -- a mirror that read the table through a wrong index misses every number.
relative_position_index, the buffer a 4.41.1 state dict also carries for every block, is no weight: index_buffers() builds
it the way transformers does, for the test that loads a state dict with it present.
"""
import hashlib

import torch

# constructor arguments of data_utils.SwinTower plus the image size; heads are 32 wide throughout
# SMALL: a 14 x 14 grid under window 7 with shift 3, then 7 x 7: one unshifted window (the small-grid rule)
SMALL = dict(image_size=56, patch=4, width=32, depths=(2, 2), heads=(1, 2), window=7, mlp_ratio=4.0)
# PADDED: 10 x 10 pads to 12 x 12 under window 3, then 5 x 5 pads to 6 x 6; both stages shifted by 1; 5 x 5 merges odd
PADDED = dict(image_size=40, patch=4, width=32, depths=(2, 2), heads=(1, 2), window=3, mlp_ratio=4.0)
TINY = dict(image_size=224, patch=4, width=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), window=7, mlp_ratio=4.0)   # microsoft/swin-tiny-patch4-window7-224
CONFIGS = {"small": SMALL, "padded": PADDED, "swin-tiny": TINY}
BATCH = 2
SEED = {"small": 3131, "padded": 3132}
INPUT_SEED = {"small": 41, "padded": 42}
# the stand-alone SwinPatchMerging: a 5 x 7 grid (odd both ways) of 32 channels
MERGE = dict(grid=(5, 7), dim=32)
MERGE_SEED, MERGE_INPUT_SEED = 3133, 43
EPS = 1e-5


def tower_kwargs(cfg):
    """The configuration as the arguments of data_utils.SwinTower."""
    return {k: v for k, v in cfg.items() if k != "image_size"}


def hf_config_kwargs(cfg):
    """The same configuration as the arguments of transformers' SwinConfig."""
    return dict(image_size=cfg["image_size"], patch_size=cfg["patch"], num_channels=3, embed_dim=cfg["width"],
                depths=list(cfg["depths"]), num_heads=list(cfg["heads"]), window_size=cfg["window"], mlp_ratio=cfg["mlp_ratio"],
                qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.1,
                hidden_act="gelu", use_absolute_embeddings=False, layer_norm_eps=EPS)


def _lin(name, o, i, bias=True):
    return [(name + ".weight", (o, i))] + ([(name + ".bias", (o,))] if bias else [])


def _norm(name, d):
    return [(name + ".weight", (d,)), (name + ".bias", (d,))]


def merge_keys(base, dim):
    return _lin(base + "reduction", 2 * dim, 4 * dim, bias=False) + _norm(base + "norm", 4 * dim)


def keys(cfg):
    """[(key, shape)] of the parameters of the 4.41.1 state dict of SwinModel (no pooler parameters exist) in the
    configuration cfg."""
    C, P, w = cfg["width"], cfg["patch"], cfg["window"]
    out = [("embeddings.patch_embeddings.projection.weight", (C, 3, P, P)), ("embeddings.patch_embeddings.projection.bias", (C,))]
    out += _norm("embeddings.norm", C)
    for i, (depth, heads) in enumerate(zip(cfg["depths"], cfg["heads"])):
        D = C << i
        M = int(cfg["mlp_ratio"] * D)
        for j in range(depth):
            b = "encoder.layers.%d.blocks.%d." % (i, j)
            out += _norm(b + "layernorm_before", D)
            out += [(b + "attention.self.relative_position_bias_table", ((2 * w - 1) ** 2, heads))]
            out += _lin(b + "attention.self.query", D, D) + _lin(b + "attention.self.key", D, D)
            out += _lin(b + "attention.self.value", D, D) + _lin(b + "attention.output.dense", D, D)
            out += _norm(b + "layernorm_after", D) + _lin(b + "intermediate.dense", M, D) + _lin(b + "output.dense", D, M)
        if i < len(cfg["depths"]) - 1:
            out += merge_keys("encoder.layers.%d.downsample." % i, D)
    return out + _norm("layernorm", C << (len(cfg["depths"]) - 1))


def index_buffers(cfg):
    """{key: tensor}: the relative_position_index buffer of every block, [w^2, w^2] int64, as transformers builds it."""
    w = cfg["window"]
    coords = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(w), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    index = rel.sum(-1)
    return {"encoder.layers.%d.blocks.%d.attention.self.relative_position_index" % (i, j): index.clone()
            for i, depth in enumerate(cfg["depths"]) for j in range(depth)}


def _fill(key_list, seed):
    g = torch.Generator().manual_seed(seed)
    sd, h = {}, hashlib.sha256()
    for key, shape in key_list:
        leaf = key.rpartition(".")[2]
        r = torch.randn(shape, generator=g)
        if leaf == "bias":
            v = 0.1 * r
        elif leaf == "weight" and len(shape) == 1:
            v = 1 + 0.2 * r
        elif leaf == "weight":
            v = r / r[0].numel() ** 0.5
        else:                                            # relative_position_bias_table
            v = 0.5 * r
        sd[key] = v
        h.update(v.contiguous().numpy().tobytes())
    return sd, h.hexdigest()


def weights(cfg, seed):
    """({4.41.1 key: tensor}, sha256 over all of them in order)."""
    return _fill(keys(cfg), seed)


def merge_weights():
    return _fill(merge_keys("", MERGE["dim"]), MERGE_SEED)


def make_image(name):
    res = CONFIGS[name]["image_size"]
    return torch.randn(BATCH, 3, res, res, generator=torch.Generator().manual_seed(INPUT_SEED[name]))


def make_merge_input():
    (H, W), C = MERGE["grid"], MERGE["dim"]
    return torch.randn(BATCH, H * W, C, generator=torch.Generator().manual_seed(MERGE_INPUT_SEED))


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
