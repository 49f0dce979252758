"""Generator of tests/golden/hf_clip.npz and hf_clip_meta.json: what transformers' own CLIPForImageClassification says
about the mirror in concept_vit/data_utils.py (HFClip).

Run once on the CPU where transformers is installed:
    python tests/golden/make_golden_hf_clip.py
The model is built from a CLIPConfig (nothing is downloaded) with attn_implementation="eager" and filled by
tests/hf_clip_recipe.py.  The fixture is what the INSTALLED transformers computes (its version is recorded in the meta;
it was a 5.x release).  The reference pins transformers 4.41.1: that release cannot be run here, so nobody has checked
offline that it names the state-dict keys identically or returns the same numbers; what is known from its documentation is
that its encoder layers return a 1-tuple where 5.x returns the tensor.
One thing is put in transformers' way, stated here because it bounds what the fixture proves: its eager attention asks
for its softmax in fp32 whatever the model's dtype (softmax(..., dtype=torch.float32)), which would leave fp32 rounding in
the float64 pass; for that pass alone torch.nn.functional.softmax ignores the dtype argument.  The fp32 pass is untouched.
Outputs are data only:
  * hf_clip_meta.json: the state-dict keys and shapes of the small, the long and the ViT-B/16 configuration, the sha256
    of the recipe's weights and inputs, the transformers and torch versions;
  * hf_clip.npz, per configuration (small, long), each as _f32 and _f64: the class-token row of every layer's output
    (<name>_layer<i>), the mean of the patch tokens (<name>_mean) and the logits (<name>_logits).
Weights are not stored: the recipe regenerates them.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hf_clip_recipe as recipe  # noqa: E402


def build(cfg):
    import transformers
    vision = recipe.hf_config_kwargs(cfg)
    config = transformers.CLIPConfig(vision_config=vision, num_labels=cfg["num_labels"])
    config._attn_implementation = "eager"
    try:
        return transformers.CLIPForImageClassification._from_config(config, attn_implementation="eager").eval()
    except TypeError:
        return transformers.CLIPForImageClassification(config).eval()


def shapes(model):
    return [[k, list(v.shape)] for k, v in sorted(model.state_dict().items())]


def run(model, image):
    rows, hooks = {}, []
    for i, layer in enumerate(model.vision_model.encoder.layers):
        hooks.append(layer.register_forward_hook(
            lambda m, a, o, i=i: rows.__setitem__("layer%d" % i, (o[0] if isinstance(o, tuple) else o)[:, 0].detach().clone())))
    # the classifier's input IS the mean of the patch tokens
    hooks.append(model.classifier.register_forward_hook(lambda m, a, o: rows.__setitem__("mean", a[0].detach().clone())))
    with torch.no_grad():
        rows["logits"] = model(pixel_values=image).logits.detach().clone()
    for h in hooks:
        h.remove()
    return rows


def main():
    import transformers
    torch.manual_seed(0)
    meta = {"transformers": transformers.__version__, "torch": torch.__version__, "configs": recipe.CONFIGS,
            "batch": recipe.BATCH, "seed": recipe.SEED, "input_seed": recipe.INPUT_SEED,
            "vit_b16_state_dict": shapes(build(recipe.VIT_B16))}
    out = {}
    for name in ("small", "long"):
        model = build(recipe.CONFIGS[name])
        assert type(model.vision_model.encoder.layers[0].mlp.activation_fn).__name__ == "QuickGELUActivation"
        meta[name + "_state_dict"] = shapes(model)
        meta[name + "_weights_sha256"] = recipe.fill(model, recipe.SEED[name])
        image = recipe.make_image(name)
        meta[name + "_image_sha256"] = recipe.sha256(image)
        r32 = run(model, image)
        real_softmax = torch.nn.functional.softmax          # the float64 pass: see the docstring
        torch.nn.functional.softmax = lambda x, dim=None, dtype=None, **kw: real_softmax(x, dim=dim)
        try:
            r64 = run(model.double(), image.double())
        finally:
            torch.nn.functional.softmax = real_softmax
        for k in r32:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, k
            out["%s_%s_f32" % (name, k)], out["%s_%s_f64" % (name, k)] = r32[k].numpy(), r64[k].numpy()
    np.savez_compressed(os.path.join(HERE, "hf_clip.npz"), **out)
    with open(os.path.join(HERE, "hf_clip_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: v.shape for k, v in out.items()})
    print({k[:-4]: float(np.abs(out[k] - out[k[:-4] + "_f64"]).max() / np.abs(out[k[:-4] + "_f64"]).max())
           for k in out if k.endswith("_f32")})


if __name__ == "__main__":
    main()
