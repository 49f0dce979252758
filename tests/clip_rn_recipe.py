"""The weights and the input of the CLIP-ResNet fixture (tests/golden/clip_rn.npz), written once: the generator
(tests/golden/make_golden_clip_rn.py) fills the reference's ModifiedResNet with them, the tests fill the mirror.  Nothing is
stored but the sha256 of what this produces (clip_rn_meta.json).

One seeded torch.Generator, the state dict walked in key order:
  * a convolution / linear weight and positional_embedding: randn / sqrt(fan_in) (fan_in = the product of all dimensions
    but the first; for positional_embedding its width);
  * a linear bias: 0.1 * randn;
  * batch norm: running_mean 0.1 * randn, running_var rand + 0.5, weight 1 + 0.2 * randn, bias 0.1 * randn (the ranges
    of util.mild_bn: a whole tower's activations stay in range, and bn3.weight is not the zero CLIP's own init gives it);
  * num_batches_tracked is left alone.
"""
import hashlib

import torch

SMALL = dict(layers=(1, 1, 1, 1), output_dim=64, heads=32, input_resolution=64, width=64)
RN50 = dict(layers=(3, 4, 6, 3), output_dim=1024, heads=32, input_resolution=224, width=64)
SEED, INPUT_SEED, BATCH = 2024, 7, 2
LAYERS = ("layer1", "layer2", "layer3", "layer4")


def fill(model, seed=SEED, conv_gain=1.0):
    """Fill `model` (any module with ModifiedResNet's state dict) in place; returns the sha256 over all filled tensors.
    conv_gain multiplies the convolution weights (1: the fixture's; sqrt(2), He's gain for a ReLU network, keeps the
    differences between images alive through the depth of RN50: the driver test's choice)."""
    g = torch.Generator().manual_seed(seed)
    bn = {n for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    h = hashlib.sha256()
    with torch.no_grad():
        for key, t in model.state_dict().items():
            mod, _, leaf = key.rpartition(".")
            if leaf == "num_batches_tracked":
                continue
            if mod in bn:
                r = torch.rand(t.shape, generator=g) + 0.5 if leaf == "running_var" else torch.randn(t.shape, generator=g)
                v = {"running_mean": 0.1 * r, "running_var": r, "weight": 1 + 0.2 * r, "bias": 0.1 * r}[leaf]
            elif leaf == "bias":
                v = 0.1 * torch.randn(t.shape, generator=g)
            else:
                fan_in = t[0].numel() if leaf == "weight" else t.shape[-1]
                v = torch.randn(t.shape, generator=g) / fan_in ** 0.5
                if t.dim() == 4 and conv_gain != 1.0:
                    v = v * conv_gain
            t.copy_(v.to(t.dtype))
            h.update(v.float().contiguous().numpy().tobytes())
    return h.hexdigest()


def make_input(res=SMALL["input_resolution"], batch=BATCH, seed=INPUT_SEED):
    return torch.randn(batch, 3, res, res, generator=torch.Generator().manual_seed(seed))


def sha256(t):
    return hashlib.sha256(t.detach().float().contiguous().numpy().tobytes()).hexdigest()
