"""Generator of tests/golden/clip_rn.npz + clip_rn_meta.json: what the REFERENCE's ModifiedResNet (concept_vit/clip/model.py:93-150,
built for RN50 at :258-266) says about the mirror in concept_vit/data_utils.py.

Run where the reference is checked out (MCD_REFERENCE, default /root/reference); the GPU box never has it:
    python tests/golden/make_golden_clip_rn.py
The reference's clip/model.py is imported at generation time (by file path: the package's __init__ pulls in a tokenizer
this build does not need); no line of it is copied.  Outputs are data only:
  * clip_rn_meta.json: the state_dict keys and shapes of the reference's ModifiedResNet in RN50's configuration, the small
    configuration, and the sha256 of the recipe's weights and input (tests/clip_rn_recipe.py);
  * clip_rn.npz: for the small configuration on the recipe's weights, the input, the reference's output and the spatial
    means of its layer1..4 outputs, each in float64 and in fp32.
Weights are not stored: the recipe regenerates them.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_rn_recipe as recipe  # noqa: E402

REF = os.environ.get("MCD_REFERENCE", "/root/reference")


def reference_model_module():
    spec = importlib.util.spec_from_file_location("ref_clip_model", os.path.join(REF, "concept_vit", "clip", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(net, x):
    means = {}
    hs = [getattr(net, n).register_forward_hook(lambda m, i, o, n=n: means.__setitem__(n, o.detach().mean(dim=[2, 3])))
          for n in recipe.LAYERS]
    with torch.no_grad():
        y = net(x)
    for h in hs:
        h.remove()
    return y, means


def main():
    ref = reference_model_module()
    torch.manual_seed(0)
    rn50 = ref.ModifiedResNet(**recipe.RN50)
    meta = {"rn50_config": {k: list(v) if isinstance(v, tuple) else v for k, v in recipe.RN50.items()},
            "rn50_state_dict": [[k, list(v.shape)] for k, v in rn50.state_dict().items()],
            "small_config": {k: list(v) if isinstance(v, tuple) else v for k, v in recipe.SMALL.items()},
            "seed": recipe.SEED, "input_seed": recipe.INPUT_SEED, "batch": recipe.BATCH}
    small = ref.ModifiedResNet(**recipe.SMALL).eval()
    meta["weights_sha256"] = recipe.fill(small)
    meta["small_state_dict"] = [[k, list(v.shape)] for k, v in small.state_dict().items()]
    x = recipe.make_input()
    meta["input_sha256"] = recipe.sha256(x)
    out = {"x": x.numpy()}
    y32, m32 = run(small, x)
    y64, m64 = run(small.double(), x.double())
    out["y_f32"], out["y_f64"] = y32.numpy(), y64.numpy()
    for n in recipe.LAYERS:
        out[n + "_mean_f32"], out[n + "_mean_f64"] = m32[n].numpy(), m64[n].numpy()
    meta["torch"] = torch.__version__
    np.savez_compressed(os.path.join(HERE, "clip_rn.npz"), **out)
    with open(os.path.join(HERE, "clip_rn_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: v.shape for k, v in out.items()}, float(np.abs(y64).max()))


if __name__ == "__main__":
    main()
