"""What tests/test_preprocess_cpu.py and tests/test_gpu_preprocess.py share: the goldens of
tests/golden/make_golden_preprocess.py (PIL + torch) and a numpy restatement of K22's arithmetic."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def goldens():
    """(npz arrays as a dict, meta) -- loaded once, never written to."""
    if not _cache:
        with np.load(os.path.join(GOLDEN, "preprocess.npz")) as z:
            _cache["z"] = {k: z[k] for k in z.files}
        with open(os.path.join(GOLDEN, "preprocess_meta.json")) as f:
            _cache["meta"] = json.load(f)
    return _cache["z"], _cache["meta"]


def case_names(large=None):
    meta = json.load(open(os.path.join(GOLDEN, "preprocess_meta.json")))
    return [c["name"] for c in meta["cases"] if large is None or ("input" in c) == large]


def case(name):
    return next(c for c in goldens()[1]["cases"] if c["name"] == name)


def spec_of(core, c):
    """The core.Preprocess of a golden case / route view."""
    resize = c["resize"] if c["resize"] is None or isinstance(c["resize"], int) else tuple(c["resize"])
    return core.Preprocess(c["filter"], resize, c["crop"], c["mean"], c["std"])


def case_input(c):
    """uint8 [n, H, W, 3] of a case: stored, or regenerated from its seed."""
    if "input" in c:
        i = c["input"]
        return np.random.RandomState(i["seed"]).randint(0, 256, (i["H"], i["W"], 3)).astype(np.uint8)[None]
    return goldens()[0]["in_" + c["name"]]


def check_against_golden(c, out):
    """out fp32 [n, 3, OH, OW] (numpy) equals the case's golden bit for bit (large cases: sha256 + the stored head)."""
    z = goldens()[0]
    out = np.ascontiguousarray(out)
    assert out.dtype == np.float32 and list(out.shape) == c["shape"]
    if "input" in c:
        assert np.array_equal(out[:, :, :8].view(np.uint32), z["head_" + c["name"]].view(np.uint32))
        assert hashlib.sha256(out.tobytes()).hexdigest() == c["sha256"]
    else:
        assert np.array_equal(out.view(np.uint32), z["out_" + c["name"]].view(np.uint32))


def _pass(img, tab, axis):
    """One pass of PIL's 8-bit resampler along `axis` of uint8 [H, W, 3] with a core.resample_table table."""
    tab = np.asarray(tab, dtype=np.int64)
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((tab.shape[0],) + img.shape[1:], dtype=np.uint8)
    for o, row in enumerate(tab):
        first, count = int(row[0]), int(row[1])
        acc = (1 << 21) + np.tensordot(row[2:2 + count], img[first:first + count], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31                       # the kernel accumulates in int32
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def numpy_preprocess(core, arr, pre):
    """K22's arithmetic restated: uint8 [H, W, 3] -> fp32 [3, OH, OW]."""
    plan = pre.plan(arr.shape[0], arr.shape[1])
    if plan.xtab is not None:
        arr = _pass(arr, plan.xtab.numpy(), 1)
    if plan.ytab is not None:
        arr = _pass(arr, plan.ytab.numpy(), 0)
    arr = arr[plan.top:plan.top + plan.OH, plan.left:plan.left + plan.OW]
    lut = pre.lut().numpy()
    return np.stack([lut[c][arr[:, :, c]] for c in range(3)])
