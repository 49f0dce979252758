"""Generator of tests/golden/mae.npz and mae_meta.json: what transformers' own ViTMAEForPreTraining -- the class the
reference's AutoModelForPreTraining instantiates for its `mae` target (concept_vit/data_utils.py:21-36, :65-66) -- says about
the mirror in concept_vit/data_utils.py (HFMae).

Run once on the CPU where transformers is installed:
    python tests/golden/make_golden_mae.py
The model is built from a ViTMAEConfig (nothing is downloaded) with attn_implementation="eager" and filled with the
recipe's weights (tests/mae_recipe.py), which are keyed by the module names of transformers 4.41.1, the reference's pin.
The fixture is what the INSTALLED transformers computes (its version is recorded in the meta; it was a 5.x release, which
names the layers vit.layers.N.attention.q_proj and so on: V5_NAMES is the explicit table, used only where the installed
release does not have the 4.41.1 name).  transformers 4.41.1 itself cannot be run here, so nobody has checked offline that
it names the state-dict keys as the recipe does or returns the same numbers.
One thing is put in transformers' way, stated here because it bounds what the fixture proves: its eager attention asks
for its softmax in fp32 whatever the model's dtype (softmax(..., dtype=torch.float32)), which would leave fp32 rounding in
the float64 pass; for that pass alone torch.nn.functional.softmax ignores the dtype argument.  The fp32 pass is untouched.
Outputs are data only:
  * mae_meta.json: the 4.41.1 key / shape lists of the small, the odd and the vit-mae-base configuration -- read back from
    the transformers models through the table and checked against the recipe's --, the sha256 of the recipe's weights,
    images and noise, the transformers and torch versions;
  * mae.npz, per configuration (small, odd): <name>_mask and <name>_ids_restore, and each as _f32 and _f64 the class-token
    row of every encoder layer's output (<name>_layer<i>), vit.layernorm's output (<name>_norm), the logits and the loss.
Weights are not stored: the recipe regenerates them.
"""
import json
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mae_recipe as recipe  # noqa: E402

# transformers 4.41.1 -> 5.x (regular expressions on the whole key)
_LAYER = r"^(vit\.encoder\.layer|decoder\.decoder_layers)\.(\d+)\."
_NEW = lambda m: ("vit.layers" if m.group(1).startswith("vit") else "decoder.decoder_layers") + "." + m.group(2) + "."  # noqa: E731
V5_NAMES = [(_LAYER + r"attention\.attention\.query\.", "attention.q_proj."),
            (_LAYER + r"attention\.attention\.key\.", "attention.k_proj."),
            (_LAYER + r"attention\.attention\.value\.", "attention.v_proj."),
            (_LAYER + r"attention\.output\.dense\.", "attention.o_proj."),
            (_LAYER + r"intermediate\.dense\.", "mlp.fc1."),
            (_LAYER + r"output\.dense\.", "mlp.fc2."),
            (_LAYER + r"layernorm_before\.", "layernorm_before."),
            (_LAYER + r"layernorm_after\.", "layernorm_after.")]


def installed_name(key, have):
    """The installed release's name of the 4.41.1 key."""
    if key in have:
        return key
    for pat, new in V5_NAMES:
        k2, n = re.subn(pat, lambda m: _NEW(m) + new, key)
        if n and k2 in have:
            return k2
    import transformers
    raise KeyError("no name in transformers %s for %s" % (transformers.__version__, key))


def build(cfg, norm_pix_loss=False):
    import transformers
    config = transformers.ViTMAEConfig(**recipe.hf_config_kwargs(cfg, norm_pix_loss))
    config._attn_implementation = "eager"
    try:
        return transformers.ViTMAEForPreTraining._from_config(config, attn_implementation="eager").eval()
    except TypeError:
        return transformers.ViTMAEForPreTraining(config).eval()


def key_list(cfg, model):
    """[[4.41.1 key, shape]] read from the transformers model, in the recipe's order; the two must describe one dict."""
    sd = model.state_dict()
    out = [[k, list(sd[installed_name(k, sd)].shape)] for k, _ in recipe.keys(cfg)]
    assert len(out) == len(sd) and out == [[k, list(s)] for k, s in recipe.keys(cfg)]
    return out


def layers_of(model):
    return model.vit.layers if hasattr(model.vit, "layers") else model.vit.encoder.layer


def run(model, image, noise):
    rows, hooks = {}, []
    for i, layer in enumerate(layers_of(model)):
        hooks.append(layer.register_forward_hook(
            lambda m, a, o, i=i: rows.__setitem__("layer%d" % i, (o[0] if isinstance(o, tuple) else o)[:, 0].detach().clone())))
    hooks.append(model.vit.layernorm.register_forward_hook(lambda m, a, o: rows.__setitem__("norm", o.detach().clone())))
    with torch.no_grad():
        out = model(pixel_values=image, noise=noise)
    for h in hooks:
        h.remove()
    rows.update(logits=out.logits.detach().clone(), loss=out.loss.detach().clone().reshape(1))
    return rows, out.mask.detach().clone(), out.ids_restore.detach().clone()


def main():
    import transformers
    torch.manual_seed(0)
    meta = {"transformers": transformers.__version__, "torch": torch.__version__, "key_names": "transformers 4.41.1",
            "configs": recipe.CONFIGS, "norm_pix_loss": recipe.NORM_PIX_LOSS, "mask_ratio": recipe.MASK_RATIO,
            "batch": recipe.BATCH, "seed": recipe.SEED, "input_seed": recipe.INPUT_SEED, "noise_seed": recipe.NOISE_SEED,
            "vit-mae-base_state_dict": key_list(recipe.BASE, build(recipe.BASE))}
    out = {}
    for name in ("small", "odd"):
        cfg = recipe.CONFIGS[name]
        model = build(cfg, recipe.NORM_PIX_LOSS[name])
        assert type(layers_of(model)[0].mlp.activation_fn).__name__ == "GELUActivation"
        meta[name + "_state_dict"] = key_list(cfg, model)
        sd, meta[name + "_weights_sha256"] = recipe.weights(cfg, recipe.SEED[name])
        have = model.state_dict()
        model.load_state_dict({installed_name(k, have): v for k, v in sd.items()}, strict=True)
        assert torch.equal(model.vit.embeddings.position_embeddings, sd["vit.embeddings.position_embeddings"])
        image, noise = recipe.make_image(name), recipe.make_noise(name)
        meta[name + "_image_sha256"], meta[name + "_noise_sha256"] = recipe.sha256(image), recipe.sha256(noise)
        r32, mask, ids = run(model, image, noise)
        real_softmax = torch.nn.functional.softmax          # the float64 pass: see the docstring
        torch.nn.functional.softmax = lambda x, dim=None, dtype=None, **kw: real_softmax(x, dim=dim)
        try:
            r64, mask64, ids64 = run(model.double(), image.double(), noise.double())
        finally:
            torch.nn.functional.softmax = real_softmax
        assert torch.equal(mask, mask64.to(mask.dtype)) and torch.equal(ids, ids64)
        assert int(mask.sum()) == recipe.BATCH * (mask.shape[1] - recipe.len_keep(cfg))
        out[name + "_mask"], out[name + "_ids_restore"] = mask.numpy().astype(np.float32), ids.numpy().astype(np.int64)
        for k in r32:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, k
            out["%s_%s_f32" % (name, k)], out["%s_%s_f64" % (name, k)] = r32[k].numpy(), r64[k].numpy()
    np.savez_compressed(os.path.join(HERE, "mae.npz"), **out)
    with open(os.path.join(HERE, "mae_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: v.shape for k, v in out.items()})
    print({k[:-4]: float(np.abs(out[k] - out[k[:-4] + "_f64"]).max() / np.abs(out[k[:-4] + "_f64"]).max())
           for k in out if k.endswith("_f32")})


if __name__ == "__main__":
    main()
