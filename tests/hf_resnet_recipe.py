"""The weights and the inputs of the ResNetForImageClassification fixture (tests/golden/hf_resnet.npz), written once: the
generator (tests/golden/make_golden_hf_resnet.py) fills transformers' model with them, the tests fill the mirror
(data_utils.HFResNet) through its checkpoint loader.  Weights are not stored, only the sha256 of what this produces
(hf_resnet_meta.json).

Weights are keyed by transformers' own module names (keys()), which is what a real microsoft/resnet-50 checkpoint carries.
One seeded torch.Generator, the keys walked in order:
  * a convolution / linear weight: randn * sqrt(2 / fan_in) (fan_in = the product of all dimensions but the first);
  * a batch norm's weight: 1 + 0.2 * randn, every bias: 0.1 * randn, running_mean: 0.2 * randn,
    running_var: 0.5 + rand (positive and not 1: a mirror that folds the statistics wrongly misses every number),
    num_batches_tracked: 0.
"""
import hashlib

import torch

# constructor arguments of data_utils.HFResNet (and, by the same names, of transformers' ResNetConfig)
# BOTTLENECK: widths 32 and 64; stage 0's first layer has a stride-1 shortcut (32 -> 128), stage 1 a 1x1 / 2 shortcut
BOTTLENECK = dict(num_channels=3, embedding_size=32, hidden_sizes=[128, 256], depths=[2, 1], layer_type="bottleneck",
                  downsample_in_first_stage=False, downsample_in_bottleneck=False, num_labels=7)
# BASIC: stage 0 (32 -> 32, stride 1) has no shortcut at all, stage 1 a 1x1 / 2 shortcut
BASIC = dict(num_channels=3, embedding_size=32, hidden_sizes=[32, 64], depths=[2, 1], layer_type="basic",
             downsample_in_first_stage=False, downsample_in_bottleneck=False, num_labels=5)
RESNET50 = dict(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=[3, 4, 6, 3],
                layer_type="bottleneck", downsample_in_first_stage=False, downsample_in_bottleneck=False,
                num_labels=1000)                                             # microsoft/resnet-50
CONFIGS = {"bottleneck": BOTTLENECK, "basic": BASIC}
SEED = {"bottleneck": 3051, "basic": 3052}
INPUT_SEED = {"bottleneck": 51, "basic": 52}
BATCH, HEIGHT, WIDTH = 2, 32, 40
HOOKS = ("resnet.embedder", "resnet.embedder.embedder")      # and resnet.encoder.stages.<i> for every stage


def hook_names(cfg):
    return list(HOOKS) + ["resnet.encoder.stages.%d" % i for i in range(len(cfg["depths"]))]


def _unit(base, cout, cin, k):
    n = base + "normalization."
    return [(base + "convolution.weight", (cout, cin, k, k)), (n + "weight", (cout,)), (n + "bias", (cout,)),
            (n + "running_mean", (cout,)), (n + "running_var", (cout,)), (n + "num_batches_tracked", ())]


def keys(cfg):
    """[(key, shape)] of the state dict of ResNetForImageClassification in the configuration cfg, in its own order."""
    out = _unit("resnet.embedder.embedder.", cfg["embedding_size"], cfg["num_channels"], 7)
    cin = cfg["embedding_size"]
    for s, (cout, depth) in enumerate(zip(cfg["hidden_sizes"], cfg["depths"])):
        stride = 2 if s or cfg["downsample_in_first_stage"] else 1
        for l in range(depth):
            base = "resnet.encoder.stages.%d.layers.%d." % (s, l)
            if cin != cout or (l == 0 and stride != 1):
                out += _unit(base + "shortcut.", cout, cin, 1)
            if cfg["layer_type"] == "bottleneck":
                mid = cout // 4
                out += (_unit(base + "layer.0.", mid, cin, 1) + _unit(base + "layer.1.", mid, mid, 3)
                        + _unit(base + "layer.2.", cout, mid, 1))
            else:
                out += _unit(base + "layer.0.", cout, cin, 3) + _unit(base + "layer.1.", cout, cout, 3)
            cin = cout
    return out + [("classifier.1.weight", (cfg["num_labels"], cin)), ("classifier.1.bias", (cfg["num_labels"],))]


def weights(cfg, seed):
    """({key: tensor}, sha256 over all of them in order)."""
    g = torch.Generator().manual_seed(seed)
    sd, h = {}, hashlib.sha256()
    for key, shape in keys(cfg):
        leaf = key.rpartition(".")[2]
        if leaf == "num_batches_tracked":
            v = torch.zeros((), dtype=torch.int64)
        elif leaf == "running_var":
            v = 0.5 + torch.rand(shape, generator=g)
        elif leaf == "running_mean":
            v = 0.2 * torch.randn(shape, generator=g)
        elif leaf == "bias":
            v = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:                            # a batch norm's weight
            v = 1 + 0.2 * torch.randn(shape, generator=g)
        else:
            r = torch.randn(shape, generator=g)
            v = r * (2.0 / r[0].numel()) ** 0.5
        sd[key] = v
        h.update(v.contiguous().numpy().tobytes())
    return sd, h.hexdigest()


def make_image(name, batch=BATCH, height=HEIGHT, width=WIDTH):
    return torch.randn(batch, CONFIGS[name]["num_channels"], height, width,
                       generator=torch.Generator().manual_seed(INPUT_SEED[name]))


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
