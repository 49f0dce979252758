"""Generator of tests/golden/swin.npz and swin_meta.json: what transformers' own SwinModel -- the class the reference's
HuggingfaceImageEncoder instantiates for `model_type: swin` (model/modules/image_encoder.py:27-28) -- says about the mirror
in concept_vit/data_utils.py (SwinTower).

Run once on the CPU where transformers is installed:
    python tests/golden/make_golden_swin.py
The model is built from a SwinConfig (nothing is downloaded) with attn_implementation="eager" and filled with the recipe's
weights (tests/swin_recipe.py), which are keyed by the module names of transformers 4.41.1, the reference's pin.  The
fixture is what the INSTALLED transformers computes (its version is recorded in the meta; it was a 5.x release, which names
the modules attention.q_proj, attention.o_proj, mlp.fc1, attention.relative_position_bias.relative_position_bias_table and
so on: V5_NAMES is the explicit table, used only where the installed release does not have the 4.41.1 name).  transformers
4.41.1 itself cannot be run here, so nobody has checked offline that it names the state-dict keys as the recipe does or
returns the same numbers.
One thing is put in transformers' way, as in make_golden_mae.py: its eager attention asks for its softmax in fp32 whatever
the model's dtype, which would leave fp32 rounding in the float64 pass; for that pass alone torch.nn.functional.softmax
ignores the dtype argument.  The fp32 pass is untouched.
Outputs are data only:
  * swin_meta.json: the 4.41.1 key / shape lists of the small, the padded and the swin-tiny configuration -- read back from
    the transformers models through the table and checked against the recipe's --, the sha256 of the recipe's weights and
    images, the transformers and torch versions;
  * swin.npz, per configuration (small, padded), each as _f32 and _f64: token 0 of every block's output
    (<name>_stage<i>_block<j>) and of every stage's output, downsampling included (<name>_stage<i>), and layernorm's output
    (<name>_norm, all tokens); merge_f32 / merge_f64: a stand-alone SwinPatchMerging on a 5 x 7 grid.
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
import swin_recipe as recipe  # noqa: E402

# transformers 4.41.1 -> 5.x (regular expressions on the whole key)
_BLOCK = r"^(encoder\.layers\.\d+\.blocks\.\d+\.)"
V5_NAMES = [(_BLOCK + r"attention\.self\.query\.", r"\1attention.q_proj."),
            (_BLOCK + r"attention\.self\.key\.", r"\1attention.k_proj."),
            (_BLOCK + r"attention\.self\.value\.", r"\1attention.v_proj."),
            (_BLOCK + r"attention\.output\.dense\.", r"\1attention.o_proj."),
            (_BLOCK + r"intermediate\.dense\.", r"\1mlp.fc1."),
            (_BLOCK + r"output\.dense\.", r"\1mlp.fc2."),
            (_BLOCK + r"attention\.self\.relative_position_bias_table$",
             r"\1attention.relative_position_bias.relative_position_bias_table")]


def installed_name(key, have):
    """The installed release's name of the 4.41.1 key."""
    if key in have:
        return key
    for pat, new in V5_NAMES:
        k2, n = re.subn(pat, new, key)
        if n and k2 in have:
            return k2
    import transformers
    raise KeyError("no name in transformers %s for %s" % (transformers.__version__, key))


def build(cfg):
    import transformers
    config = transformers.SwinConfig(**recipe.hf_config_kwargs(cfg))
    config._attn_implementation = "eager"
    try:
        return transformers.SwinModel._from_config(config, attn_implementation="eager", add_pooling_layer=False).eval()
    except TypeError:
        return transformers.SwinModel(config, add_pooling_layer=False).eval()


def key_list(cfg, model):
    """[[4.41.1 key, shape]] read from the transformers model, in the recipe's order; the two must describe one dict."""
    sd = model.state_dict()
    out = [[k, list(sd[installed_name(k, sd)].shape)] for k, _ in recipe.keys(cfg)]
    assert len(out) == len(sd), (len(out), len(sd), sorted(sd)[:8])
    assert out == [[k, list(s)] for k, s in recipe.keys(cfg)]
    return out


def first(o):
    return o[0] if isinstance(o, tuple) else o


def run(model, image):
    rows, hooks = {}, []
    for i, stage in enumerate(model.encoder.layers):
        hooks.append(stage.register_forward_hook(
            lambda m, a, o, i=i: rows.__setitem__("stage%d" % i, first(o)[:, 0].detach().clone())))
        for j, blk in enumerate(stage.blocks):
            hooks.append(blk.register_forward_hook(
                lambda m, a, o, i=i, j=j: rows.__setitem__("stage%d_block%d" % (i, j), first(o)[:, 0].detach().clone())))
    with torch.no_grad():
        out = model(pixel_values=image, interpolate_pos_encoding=False)
    for h in hooks:
        h.remove()
    rows["norm"] = out.last_hidden_state.detach().clone()
    return rows


def float64_pass(fn):
    real_softmax = torch.nn.functional.softmax          # see the docstring
    torch.nn.functional.softmax = lambda x, dim=None, dtype=None, **kw: real_softmax(x, dim=dim)
    try:
        return fn()
    finally:
        torch.nn.functional.softmax = real_softmax


def main():
    import transformers
    from transformers.models.swin.modeling_swin import SwinPatchMerging
    torch.manual_seed(0)
    meta = {"transformers": transformers.__version__, "torch": torch.__version__, "key_names": "transformers 4.41.1",
            "configs": recipe.CONFIGS, "batch": recipe.BATCH, "seed": recipe.SEED, "input_seed": recipe.INPUT_SEED,
            "merge": recipe.MERGE, "merge_seed": recipe.MERGE_SEED, "merge_input_seed": recipe.MERGE_INPUT_SEED,
            "swin-tiny_state_dict": key_list(recipe.TINY, build(recipe.TINY))}
    out = {}
    for name in ("small", "padded"):
        cfg = recipe.CONFIGS[name]
        model = build(cfg)
        assert type(model.encoder.layers[0].blocks[0].mlp.activation_fn).__name__ == "GELUActivation"
        meta[name + "_state_dict"] = key_list(cfg, model)
        sd, meta[name + "_weights_sha256"] = recipe.weights(cfg, recipe.SEED[name])
        have = model.state_dict()
        model.load_state_dict({installed_name(k, have): v for k, v in sd.items()}, strict=True)
        image = recipe.make_image(name)
        meta[name + "_image_sha256"] = recipe.sha256(image)
        r32 = run(model, image)
        r64 = float64_pass(lambda: run(model.double(), image.double()))
        for k in r32:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, k
            out["%s_%s_f32" % (name, k)], out["%s_%s_f64" % (name, k)] = r32[k].numpy(), r64[k].numpy()
    # the stand-alone merging layer
    try:
        merge = SwinPatchMerging(recipe.MERGE["dim"]).eval()
    except TypeError:                                    # releases that also take the input resolution
        merge = SwinPatchMerging(tuple(recipe.MERGE["grid"]), recipe.MERGE["dim"]).eval()
    msd, meta["merge_weights_sha256"] = recipe.merge_weights()
    merge.load_state_dict(msd, strict=True)
    x = recipe.make_merge_input()
    meta["merge_input_sha256"] = recipe.sha256(x)
    with torch.no_grad():
        out["merge_f32"] = merge(x, tuple(recipe.MERGE["grid"])).numpy()
        out["merge_f64"] = merge.double()(x.double(), tuple(recipe.MERGE["grid"])).numpy()
    np.savez_compressed(os.path.join(HERE, "swin.npz"), **out)
    with open(os.path.join(HERE, "swin_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: v.shape for k, v in out.items()})
    print({k[:-4]: float(np.abs(out[k] - out[k[:-4] + "_f64"]).max() / np.abs(out[k[:-4] + "_f64"]).max())
           for k in out if k.endswith("_f32")})


if __name__ == "__main__":
    main()
