"""Generator of tests/golden/vit_family.npz + vit_family_meta.json: what transformers' ViTForImageClassification and
Dinov2ForImageClassification -- the classes the reference's AutoModelForImageClassification instantiates for its `vit` and
`dino` targets (concept_vit/data_utils.py:21-36, :63-69) -- say about the mirrors HFViT / HFDinov2 in concept_vit/data_utils.py.

    python tests/golden/make_golden_vit_family.py

The models are built from configs (nothing is downloaded) with the installed transformers, and filled with the recipe's
weights (tests/vit_family_recipe.py), which are keyed by the module names of transformers 4.41.1, the reference's pin.
transformers 5 renamed ViT's modules (vit.layers.N.attention.q_proj, ...; DINOv2 kept its names): V5_NAMES is the explicit
table, used only where the installed release does not have the 4.41.1 name.  Outputs are data only:
  * vit_family_meta.json: the 4.41.1 key / shape lists of the small and the base configurations -- read back from the
    transformers models through the same table and checked against the recipe's --, the configurations, the sha256 of
    the recipe's weights and inputs, the versions;
  * vit_family.npz: per case of the recipe, the input (int8: x = q / 16), the logits and the class-token row of every
    encoder layer's output [layers, batch, hidden], each in float64 and in fp32.
"""
import json
import os
import re
import sys

import numpy as np
import torch
import transformers
from transformers import Dinov2Config, Dinov2ForImageClassification, ViTConfig, ViTForImageClassification

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vit_family_recipe as recipe  # noqa: E402

# transformers 4.41.1 -> 5.x, ViT only (regular expressions on the whole key)
V5_NAMES = [(r"^vit\.encoder\.layer\.(\d+)\.attention\.attention\.query\.", r"vit.layers.\1.attention.q_proj."),
            (r"^vit\.encoder\.layer\.(\d+)\.attention\.attention\.key\.", r"vit.layers.\1.attention.k_proj."),
            (r"^vit\.encoder\.layer\.(\d+)\.attention\.attention\.value\.", r"vit.layers.\1.attention.v_proj."),
            (r"^vit\.encoder\.layer\.(\d+)\.attention\.output\.dense\.", r"vit.layers.\1.attention.o_proj."),
            (r"^vit\.encoder\.layer\.(\d+)\.intermediate\.dense\.", r"vit.layers.\1.mlp.fc1."),
            (r"^vit\.encoder\.layer\.(\d+)\.output\.dense\.", r"vit.layers.\1.mlp.fc2."),
            (r"^vit\.encoder\.layer\.(\d+)\.layernorm_(before|after)\.", r"vit.layers.\1.layernorm_\2.")]


def installed_name(key, have):
    """The installed release's name of the 4.41.1 key."""
    if key in have:
        return key
    for pat, new in V5_NAMES:
        k2, n = re.subn(pat, new, key)
        if n and k2 in have:
            return k2
    raise KeyError("no name in transformers %s for %s" % (transformers.__version__, key))


def build(kind, cfg):
    common = dict(hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"], num_hidden_layers=cfg["layers"],
                  image_size=cfg["image"], patch_size=cfg["patch"], num_labels=cfg["labels"])
    if kind == "vit":
        return ViTForImageClassification(ViTConfig(intermediate_size=cfg["mlp"], **common)).eval()
    assert cfg["mlp"] % cfg["hidden"] == 0
    return Dinov2ForImageClassification(Dinov2Config(mlp_ratio=cfg["mlp"] // cfg["hidden"], **common)).eval()


def key_list(kind, cfg, model):
    """[[4.41.1 key, shape]] read from the transformers model, in the recipe's order; the two must describe one dict."""
    sd = model.state_dict()
    out = [[k, list(sd[installed_name(k, sd)].shape)] for k, _ in recipe.keys(kind, cfg)]
    assert len(out) == len(sd) and out == [[k, list(s)] for k, s in recipe.keys(kind, cfg)], kind
    return out


def layers_of(kind, model):
    if kind == "dino":
        return model.dinov2.encoder.layer
    return model.vit.layers if hasattr(model.vit, "layers") else model.vit.encoder.layer


def run(kind, model, x):
    rows = []
    hs = [m.register_forward_hook(lambda m, i, o: rows.append((o[0] if isinstance(o, tuple) else o).detach()[:, 0].clone()))
          for m in layers_of(kind, model)]
    with torch.no_grad():
        y = model(x).logits
    for h in hs:
        h.remove()
    return y.numpy(), torch.stack(rows).numpy()


def main():
    meta = {"seed": recipe.SEED, "input_seed": recipe.INPUT_SEED, "batch": recipe.BATCH, "input_scale": recipe.INPUT_SCALE,
            "configs": {}, "cases": {}, "transformers": transformers.__version__, "torch": torch.__version__,
            "key_names": "transformers 4.41.1"}
    models = {}
    for name, (kind, cfg) in recipe.CONFIGS.items():
        torch.manual_seed(0)
        model = build(kind, cfg)
        entry = {"kind": kind, "config": cfg, "state_dict": key_list(kind, cfg, model)}
        if name.endswith("_small"):
            sd, entry["weights_sha256"] = recipe.weights(kind, cfg)
            have = model.state_dict()
            model.load_state_dict({installed_name(k, have): v for k, v in sd.items()}, strict=True)
            models[name] = (kind, model)
        meta["configs"][name] = entry
    out = {}
    for case, (name, H, W) in recipe.CASES.items():
        kind, model = models[name]
        q = recipe.make_input_q(case)
        x = recipe.dequantize(q)
        meta["cases"][case] = {"config": name, "H": H, "W": W, "input_sha256": recipe.sha256(x)}
        out["q_" + case] = q.numpy()
        out["logits_f32_" + case], out["cls_f32_" + case] = run(kind, model.float(), x)
        out["logits_f64_" + case], out["cls_f64_" + case] = run(kind, model.double(), x.double())
        model.float()
        print(case, out["cls_f64_" + case].shape, float(np.abs(out["logits_f64_" + case]).max()),
              float(np.abs(out["logits_f32_" + case] - out["logits_f64_" + case]).max()))
    np.savez_compressed(os.path.join(HERE, "vit_family.npz"), **out)
    with open(os.path.join(HERE, "vit_family_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
