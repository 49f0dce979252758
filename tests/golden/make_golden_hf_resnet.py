"""Generator of tests/golden/hf_resnet.npz and hf_resnet_meta.json: what transformers' own ResNetForImageClassification --
the class the reference's AutoModelForImageClassification instantiates for its `resnet` targets
(concept_vit/data_utils.py:21-36, :63-69) -- says about the mirror in concept_vit/data_utils.py (HFResNet).

Run once on the CPU where transformers is installed:
    python tests/golden/make_golden_hf_resnet.py
The models are built from a ResNetConfig (nothing is downloaded) and filled with the recipe's weights
(tests/hf_resnet_recipe.py) by a strict load.  The fixture is what the INSTALLED transformers computes; its version is
recorded in the meta.
Outputs are data only:
  * hf_resnet_meta.json: the key / shape lists of the bottleneck, the basic and the microsoft/resnet-50 configuration, read
    from the transformers models and checked against the recipe's, the configurations, the sha256 of the recipe's
    weights and images, the transformers and torch versions;
  * hf_resnet.npz, per configuration (bottleneck, basic) on a batch of 2 at 32 x 40: the output of resnet.embedder,
    resnet.embedder.embedder and every stage (<name>_<module path>) and the logits (<name>_logits), each as _f32 (the
    model as built) and _f64 (the same model after .double()).
Weights are not stored: the recipe regenerates them.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hf_resnet_recipe as recipe  # noqa: E402


def build(cfg):
    import transformers
    config = transformers.ResNetConfig(hidden_act="relu", **cfg)
    return transformers.ResNetForImageClassification(config).eval()


def key_list(cfg, model):
    """[[key, shape]] read from the transformers model; it must be the recipe's list, in the recipe's order."""
    out = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert out == [[k, list(s)] for k, s in recipe.keys(cfg)]
    return out


def run(model, cfg, image):
    got, hooks = {}, []
    for name in recipe.hook_names(cfg):
        hooks.append(model.get_submodule(name).register_forward_hook(
            lambda m, a, o, name=name: got.__setitem__(name, o.detach().clone())))
    with torch.no_grad():
        got["logits"] = model(pixel_values=image).logits.detach().clone()
    for h in hooks:
        h.remove()
    return got


def main():
    import transformers
    torch.manual_seed(0)
    meta = {"transformers": transformers.__version__, "torch": torch.__version__, "configs": recipe.CONFIGS,
            "resnet-50_config": recipe.RESNET50, "batch": [recipe.BATCH, recipe.HEIGHT, recipe.WIDTH],
            "seed": recipe.SEED, "input_seed": recipe.INPUT_SEED,
            "resnet-50_state_dict": key_list(recipe.RESNET50, build(recipe.RESNET50))}
    out = {}
    for name, cfg in recipe.CONFIGS.items():
        model = build(cfg)
        meta[name + "_state_dict"] = key_list(cfg, model)
        sd, meta[name + "_weights_sha256"] = recipe.weights(cfg, recipe.SEED[name])
        model.load_state_dict(sd, strict=True)
        image = recipe.make_image(name)
        meta[name + "_image_sha256"] = recipe.sha256(image)
        r32 = run(model, cfg, image)
        r64 = run(model.double(), cfg, image.double())
        for k in r32:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, k
            out["%s_%s_f32" % (name, k)], out["%s_%s_f64" % (name, k)] = r32[k].numpy(), r64[k].numpy()
    np.savez_compressed(os.path.join(HERE, "hf_resnet.npz"), **out)
    with open(os.path.join(HERE, "hf_resnet_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: v.shape for k, v in out.items()})
    print({k[:-4]: float(np.abs(out[k] - out[k[:-4] + "_f64"]).max() / np.abs(out[k[:-4] + "_f64"]).max())
           for k in out if k.endswith("_f32")})


if __name__ == "__main__":
    main()
