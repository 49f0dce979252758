"""What tests/test_mammo_probe_cpu.py and tests/test_gpu_mammo_probe.py share: the goldens of
tests/golden/make_golden_mammo.py (the reference's own dataset classes) and a numpy restatement of K23's table."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def goldens():
    """(npz arrays as a dict, meta) -- loaded once, never written to."""
    if not _cache:
        with np.load(os.path.join(GOLDEN, "mammo_probe.npz")) as z:
            _cache["z"] = {k: z[k] for k in z.files}
        with open(os.path.join(GOLDEN, "mammo_probe_meta.json")) as f:
            _cache["meta"] = json.load(f)
    return _cache["z"], _cache["meta"]


def case_names(large=None):
    with open(os.path.join(GOLDEN, "mammo_probe_meta.json")) as f:
        meta = json.load(f)
    return [c["name"] for c in meta["cases"] if large is None or ("input" in c) == large]


def case(name):
    return next(c for c in goldens()[1]["cases"] if c["name"] == name)


def seeded_input(i):
    """uint8 [n, H, W] (channels 1) or [n, H, W, 3] from numpy's RandomState(seed).randint (stable across releases);
    image k is clipped to clip[k] = [lo, hi]."""
    shape = (i["n"], i["H"], i["W"]) + ((3,) if i["channels"] == 3 else ())
    a = np.random.RandomState(i["seed"]).randint(0, 256, shape).astype(np.uint8)
    for k, (lo, hi) in enumerate(i["clip"]):
        np.clip(a[k], lo, hi, out=a[k])
    return a


def case_input(c):
    """The uint8 source of a case: stored, or regenerated from its seed (cached: it is shared and left unchanged)."""
    if "input" in c:
        key = "seeded_" + c["name"]
        if key not in _cache:
            _cache[key] = seeded_input(c["input"])
            _cache[key].setflags(write=False)
        return _cache[key]
    return goldens()[0]["in_" + c["name"]]


def minmax_lut(mn, mx, mean, std):
    """The 256-entry table of one image: lut[v] = ((f32(v) - f32(mn)) / f32(mx - mn) - f32(mean)) / f32(std), four
    separately rounded fp32 operations.  mx == mn: 0 / 0, NaN in every entry that is read."""
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.arange(256, dtype=np.float32) - np.float32(mn)
        t = t / np.float32(mx - mn)
        t = t - np.float32(mean)
        return t / np.float32(std)


def numpy_apply(src, c):
    """K23 restated: uint8 [n, H, W(, 3)] -> fp32 [n, 3, H, W] by the table, per image."""
    out = []
    for a in src:
        if c["mode"] == "minmax":
            lut = minmax_lut(int(a.min()), int(a.max()), c["mean"], c["std"])
        else:
            lut = np.arange(256, dtype=np.float32)
        rgb = np.repeat(a[:, :, None], 3, axis=2) if a.ndim == 2 else a
        out.append(lut[rgb].transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


def _same_bits(a, b):
    """Equal fp32 bits, NaN compared as a mask (a NaN's sign and payload are not part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and bool(np.array_equal(np.where(na, 0, a.view(np.uint32)),
                                                                np.where(nb, 0, b.view(np.uint32))))


def check_against_golden(c, out):
    """out fp32 [n, 3, H, W] (numpy) equals the reference's output bit for bit (large cases: sha256 + the stored head;
    one_plane cases: every plane equals the stored one)."""
    z = goldens()[0]
    out = np.ascontiguousarray(out)
    assert out.dtype == np.float32 and list(out.shape) == c["shape"]
    assert bool(np.isnan(out).all()) == c["nan"] and bool(np.isnan(out).any()) == c["nan"]
    if "input" in c:
        assert np.array_equal(out[:, :, :8].view(np.uint32), z["head_" + c["name"]].view(np.uint32))
        assert hashlib.sha256(out.tobytes()).hexdigest() == c["sha256"]
        return
    want = z["out_" + c["name"]]
    if c["one_plane"]:
        want = np.repeat(want, 3, axis=1)
    assert _same_bits(out, want)
