"""Writes tests/golden/mammo_probe.npz + mammo_probe_meta.json: what the REFERENCE'S OWN dataset classes return for the
mammogram probe sets -- ImageClassificationZSDataset (vindr, vindr_alt: data/dataset/image_classification_zs.py) and
CSAWDataset (csaw, csaw_all_splits: data/dataset/CSAW_dataset.py) -- on small PNG files written here.  They are the
yardstick of K23 (mcd_image_minmax_normalize), of the host route (data_utils.host_minmax / host_raw) and of the table
restatement in tests/mammo_recipe.py.

    python tests/golden/make_golden_mammo.py <checkout of the reference>

The reference's three files are loaded BY FILE PATH (importlib.util.spec_from_file_location): its packages' __init__
files pull in tensorboard and torchvision.  `cv2` and `albumentations` are empty stand-in modules -- the vindr route
at 1520 x 912 with the tf_efficientnet_b5_ns-detect encoder type touches neither (Image.open(..).convert('RGB'), and
load_transform("valid", ..) falls through to None, which is recorded in the meta file) -- and `data` is a bare package
object that holds data.data_utils.  The csaw dataset is built with a transform_config of None: the reference's is
torchvision's ToTensor, which on a float32 [H, W, 3] array is the permute alone.  Nothing of the reference's text is
copied: the outputs are data.

Stored per case: the uint8 input(s) and the reference's output as fp32 [n, 3, H, W] (utils.py:176's permute applied).
The two workload-size cases are regenerated from their seed (tests/mammo_recipe.py: seeded_input); the npz holds the
first 8 rows of every plane and the meta file the sha256 of the whole output.  `extremes_last` stores one plane after
checking that the three are the same bits (a grey source).
"""
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mammo_recipe as recipe  # noqa: E402

MEAN, STD = 0.3089279, 0.25053555408335154                   # the reference's vindr constants (get_data)
CHUNK = 16384                                                # core.IMAGE_MINMAX_CHUNK; test_mammo_probe_cpu checks the case's size
TRANSFORM_CONFIG = {"valid": {"Resize": {"size_h": 1520, "size_w": 912}}}


def load_reference(root):
    """(load_transform, ImageClassificationZSDataset, CSAWDataset) from the reference's files, loaded by path."""
    for name in ("cv2", "albumentations"):
        sys.modules[name] = types.ModuleType(name)            # empty stand-ins: neither is touched on these routes
    data = types.ModuleType("data")
    data.__path__ = []                                        # a bare package object
    sys.modules["data"] = data

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    du = load("data.data_utils", "data/data_utils.py")
    data.data_utils = du
    zs = load("ref_image_classification_zs", "data/dataset/image_classification_zs.py")
    cs = load("ref_csaw_dataset", "data/dataset/CSAW_dataset.py")
    return du.load_transform, zs.ImageClassificationZSDataset, cs.CSAWDataset


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit(__doc__)
    load_transform, ZSDataset, CSAWDataset = load_reference(sys.argv[1])
    transform = load_transform("valid", TRANSFORM_CONFIG)
    assert transform is None, transform
    tmp = tempfile.mkdtemp(prefix="mammo_golden_")
    counter = [0]

    def vindr_item(arr):
        """One uint8 [H, W] (mode L) or [H, W, 3] (mode RGB) image through the reference's __getitem__."""
        counter[0] += 1
        pid, iid = "%03d" % counter[0], "img%d" % counter[0]              # no '.png': the reference appends it
        os.makedirs(os.path.join(tmp, "images", pid), exist_ok=True)
        Image.fromarray(arr, "L" if arr.ndim == 2 else "RGB").save(os.path.join(tmp, "images", pid, iid + ".png"))
        df = pd.DataFrame({"patient_id": [pid], "image_id": [iid], "Mass": [1], "Suspicious_Calcification": [0],
                           "density": [2], "split": ["test"]})
        ds = ZSDataset(tokenizer=None, split="valid", df=df, dataset="vindr", data_dir=tmp, image_dir="images",
                       transform_config=TRANSFORM_CONFIG, mean=MEAN, std=STD,
                       image_encoder_type="tf_efficientnet_b5_ns-detect")
        assert ds.transform is None
        with np.errstate(invalid="ignore", divide="ignore"):
            item = ds[0]
        img = item["images"]
        H, W = arr.shape[:2]
        assert img.dtype == torch.float32 and tuple(img.shape) == (1, H, W, 3) and int(item["mass"]) == 1
        return img[0].permute(2, 0, 1).contiguous().numpy()                # concept_vit/utils.py:176

    def csaw_item(arr):
        counter[0] += 1
        name = "c%d" % counter[0]
        os.makedirs(os.path.join(tmp, "csaw"), exist_ok=True)
        Image.fromarray(arr, "L").save(os.path.join(tmp, "csaw", name + ".png"))
        pd.DataFrame({"anon_filename": [name + ".dcm"], "Cancer_visible": [1], "split": ["test"]}).to_csv(
            os.path.join(tmp, "csaw.csv"), index=False)
        image, label = CSAWDataset(tmp, "csaw.csv", os.path.join(tmp, "csaw"), split="test", transform_config=None)[0]
        assert image.dtype == np.float32 and image.shape == arr.shape + (3,) and label == 1
        return np.ascontiguousarray(image.transpose(2, 0, 1))              # ToTensor on a float array: the permute

    arrays, cases = {}, []

    def add(name, inputs, mode="minmax", dst_gap=0, one_plane=False, **extra):
        """inputs: a uint8 array [n, H, W(, 3)] (stored) or a dict for recipe.seeded_input (regenerated)."""
        case = dict(name=name, mode=mode, dst_gap=dst_gap, mean=MEAN, std=STD, **extra)
        src = recipe.seeded_input(inputs) if isinstance(inputs, dict) else inputs
        out = np.stack([(vindr_item if mode == "minmax" else csaw_item)(a) for a in src])
        case["channels"] = 3 if src.ndim == 4 else 1
        case["shape"] = list(out.shape)
        case["nan"] = bool(np.isnan(out).any())
        assert not case["nan"] or bool(np.isnan(out).all())
        if isinstance(inputs, dict):
            case["input"] = inputs
            case["sha256"] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
            arrays["head_" + name] = out[:, :, :8].copy()
        else:
            arrays["in_" + name] = src
            if one_plane:
                assert all(np.array_equal(out[:, 0].view(np.uint32), out[:, c].view(np.uint32)) for c in (1, 2))
                out = out[:, :1]
            case["one_plane"] = bool(one_plane)
            arrays["out_" + name] = out
        cases.append(case)

    rs = np.random.RandomState(2024)
    add("rgb_odd", rs.randint(0, 256, (1, 37, 23, 3)).astype(np.uint8))
    assert arrays["in_rgb_odd"].min() == 0 and arrays["in_rgb_odd"].max() == 255
    add("gray_wide", rs.randint(9, 240, (1, 40, 24)).astype(np.uint8))
    assert arrays["in_gray_wide"].min() == 9 and arrays["in_gray_wide"].max() == 239
    b3 = np.stack([rs.randint(lo, hi + 1, (16, 16)) for lo, hi in ((0, 255), (100, 101), (17, 200))]).astype(np.uint8)
    for a, (lo, hi) in zip(b3, ((0, 255), (100, 101), (17, 200))):
        a[3, 5], a[11, 2] = lo, hi
    add("batch3", b3, dst_gap=8)
    add("constant", np.full((1, 8, 8), 7, dtype=np.uint8))
    add("tiny_1x1", np.full((1, 1, 1), 93, dtype=np.uint8))
    add("tiny_5x7", rs.randint(0, 256, (1, 5, 7)).astype(np.uint8))
    # just over two chunks of the reduction: the only 0 is the first byte of the first chunk, the only 255 the last byte
    ext = rs.randint(1, 255, (1, 5, (2 * CHUNK + 37) // 5)).astype(np.uint8)
    assert ext.size == 2 * CHUNK + 37
    ext.reshape(-1)[0], ext.reshape(-1)[-1] = 0, 255
    add("extremes_last", ext, one_plane=True)
    ch = rs.randint(50, 201, (1, 12, 20, 3)).astype(np.uint8)
    ch[0, 4, 7, 2], ch[0, 9, 13, 0] = 10, 240                               # min only in channel 2, max only in channel 0
    add("rgb_channels", ch)
    add("csaw_raw", rs.randint(0, 256, (1, 33, 17)).astype(np.uint8), mode="raw")
    # the workload shape; image 1 is clipped so that the two images of a call have different tables
    add("mammo_gray", dict(seed=31, n=2, H=1520, W=912, channels=1, clip=[[0, 255], [5, 250]]))
    add("mammo_rgb", dict(seed=32, n=2, H=1520, W=912, channels=3, clip=[[0, 255], [5, 250]]))

    meta = {"numpy_version": np.__version__, "torch_version": torch.__version__, "pil_version": PIL.__version__,
            "pandas_version": pd.__version__, "transform_config": TRANSFORM_CONFIG, "load_transform_valid": transform,
            "image_encoder_type": "tf_efficientnet_b5_ns-detect", "chunk": CHUNK, "cases": cases}
    np.savez_compressed(os.path.join(HERE, "mammo_probe.npz"), **arrays)
    with open(os.path.join(HERE, "mammo_probe_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote %d arrays, %d cases; npz %d bytes" % (len(arrays), len(cases),
                                                       os.path.getsize(os.path.join(HERE, "mammo_probe.npz"))))


if __name__ == "__main__":
    main()
