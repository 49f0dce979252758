"""Writes tests/golden/preprocess.npz + preprocess_meta.json: what PIL + torch give for the probe-set transforms of the
reference (Resize -> CenterCrop -> ToTensor -> Normalize on an RGB PIL image, torchvision's PIL path restated; torchvision
itself is not needed), on seeded uint8 images.  Nothing of the package is imported: the file is the yardstick of
tests/test_preprocess_cpu.py and tests/test_gpu_preprocess.py.

    python tests/golden/make_golden_preprocess.py

Small inputs are stored in the npz.  The two workload-sized inputs (375 x 500, 2294 x 1914) are regenerated from their
seed (numpy RandomState(seed).randint(0, 256, (H, W, 3)), stable across numpy releases); for them the npz holds the
first 8 output rows of every channel and the meta file the sha256 of the whole fp32 output.
"""
import hashlib
import json
import os

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGENET = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
CLIP = ([0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711])
FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def seeded(seed, H, W):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def resized_size(w, h, size):
    """torchvision Resize: an int -> the shorter side becomes size, the longer int(size * long / short); (h, w) as is."""
    if isinstance(size, int):
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long / short)
        return (new_short, new_long) if w <= h else (new_long, new_short)
    return size[1], size[0]


def transform(arr, filter, resize, crop, mean, std):
    """One RGB uint8 [H, W, 3] array -> fp32 [3, OH, OW], the way the reference's datasets do it."""
    img = Image.fromarray(arr, "RGB")
    if resize is not None:
        img = img.resize(resized_size(img.size[0], img.size[1], resize), FILTERS[filter])
    if crop is not None:
        w, h = img.size
        top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
        img = img.crop((left, top, left + crop, top + crop))
    t = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if mean is not None:
        t = t.sub(torch.as_tensor(mean, dtype=torch.float32)[:, None, None]).div(
            torch.as_tensor(std, dtype=torch.float32)[:, None, None])
    return t.numpy()


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def stripes(H, W):
    a = np.zeros((H, W, 3), dtype=np.uint8)
    a[:, ::2] = 255
    return a


def main():
    arrays, cases = {}, []

    def add(name, inputs, filter, resize, crop, norm, dst_gap=0):
        """inputs: list of arrays of one size (stored) or a dict(seed=, H=, W=) (regenerated)."""
        mean, std = norm if norm is not None else (None, None)
        case = {"name": name, "filter": filter, "resize": resize, "crop": crop, "mean": mean, "std": std,
                "dst_gap": dst_gap}
        if isinstance(inputs, dict):
            out = transform(seeded(**inputs), filter, resize, crop, mean, std)[None]
            case["input"] = inputs
            case["sha256"] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
            arrays["head_" + name] = out[:, :, :8].copy()
        else:
            arrays["in_" + name] = np.stack(inputs)
            out = np.stack([transform(a, filter, resize, crop, mean, std) for a in inputs])
            arrays["out_" + name] = out
        case["shape"] = list(out.shape)
        cases.append(case)
        return out

    a37, a53, a40 = seeded(1, 37, 53), seeded(2, 53, 37), [seeded(10 + i, 40, 56) for i in range(3)]
    a20 = seeded(3, 20, 20)
    # 1. a non-integer ratio, both orientations
    add("c1_37x53", [a37], "bilinear", 16, 12, IMAGENET)
    add("c1_53x37", [a53], "bilinear", 16, 12, IMAGENET)
    # 2. top = round(5.5) = 6, left = round(4.5) = 4
    add("c2_40x56", [a40[0]], "bilinear", [23, 21], 12, IMAGENET)
    # 3. up-scaling
    add("c3_20x20_up", [a20], "bilinear", [33, 47], None, None)
    # 4. skipped passes
    add("c4_17x16", [seeded(4, 17, 16)], "bilinear", [16, 16], None, IMAGENET)
    add("c4_16x17", [seeded(5, 16, 17)], "bilinear", [16, 16], None, IMAGENET)
    add("c4_16x16", [seeded(6, 16, 16)], "bilinear", [16, 16], None, IMAGENET)
    add("c4_100x7", [seeded(7, 100, 7)], "bilinear", [9, 7], None, IMAGENET)
    # 5. many taps: ratio 199 / 21 = 9.48
    a301 = seeded(8, 301, 199)
    add("c5_bilinear", [a301], "bilinear", 21, 16, IMAGENET)
    add("c5_bicubic", [a301], "bicubic", 21, 16, IMAGENET)
    # 6. 0 / 255 patterns.  One-pixel checkerboards and stripes average to grey at this ratio (3.08) and stay far from the
    # clamp; the 6-pixel blocks overshoot at every edge, so both ends of clip8 clamp -- asserted here on PIL's own float
    # resampler, which does not clamp
    for name, arr in (("c6_checker", checkerboard(37, 53)), ("c6_stripes", stripes(37, 53)),
                      ("c6_blocks", np.repeat(np.repeat(checkerboard(7, 9), 6, axis=0), 6, axis=1)[:37, :53].copy())):
        out = add(name, [arr], "bicubic", 12, 12, CLIP)
        if name == "c6_blocks":
            rw, rh = resized_size(53, 37, 12)
            f = np.asarray(Image.fromarray(arr[:, :, 0].astype(np.float32), "F").resize((rw, rh), Image.BICUBIC))
            assert f.min() < -1.0 and f.max() > 256.0, (f.min(), f.max())     # the unclamped resample leaves 0 .. 255
            lo, hi = (0 / 255 - CLIP[0][0]) / CLIP[1][0], (255 / 255 - CLIP[0][0]) / CLIP[1][0]
            assert np.isclose(out[0, 0].min(), lo) and np.isclose(out[0, 0].max(), hi)    # and the 8-bit one clamps
    # 7. three images in one call, a gap between the output images
    add("c7_three", a40, "bilinear", 16, 12, IMAGENET, dst_gap=5)
    # 8. the workload shapes
    add("c8_imagenet", dict(seed=20, H=375, W=500), "bilinear", 256, 224, IMAGENET)
    add("c8_clip", dict(seed=20, H=375, W=500), "bicubic", 224, 224, CLIP)
    add("c8_embed", dict(seed=21, H=2294, W=1914), "bilinear", [1520, 912], None, None)
    # the probe-set route: mixed source sizes, two views (the small-scale 'imagenet' and 'clip' transforms)
    route = [a37, a53] + a40 + [a20, a37[::-1].copy()]
    for i, a in enumerate(route):
        arrays["route_in_%d" % i] = a
    views = {"a": ("bilinear", 16, 12, IMAGENET), "b": ("bicubic", 12, 12, CLIP)}
    for v, (filter, resize, crop, norm) in views.items():
        arrays["route_out_" + v] = np.stack([transform(a, filter, resize, crop, norm[0], norm[1]) for a in route])
    meta = {"pil_version": PIL.__version__, "torch_version": torch.__version__, "cases": cases,
            "route": {"n": len(route), "views": {v: {"filter": s[0], "resize": s[1], "crop": s[2], "mean": s[3][0],
                                                     "std": s[3][1]} for v, s in views.items()}}}
    np.savez_compressed(os.path.join(HERE, "preprocess.npz"), **arrays)
    with open(os.path.join(HERE, "preprocess_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote %d arrays, %d cases; npz %d bytes" % (len(arrays), len(cases),
                                                       os.path.getsize(os.path.join(HERE, "preprocess.npz"))))


if __name__ == "__main__":
    main()
