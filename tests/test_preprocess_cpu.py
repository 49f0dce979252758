"""CPU: the host side of probe-image preprocessing (K22) -- resample tables, plans, look-up tables, the file probe sets'
listing order and shards, the host route, the registry -- against goldens made with PIL + torch
(tests/golden/make_golden_preprocess.py).  No GPU call is made here."""
import json
import os

import numpy as np
import pytest
import torch

import preprocess_recipe as R


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.mark.parametrize("name", R.case_names())
def test_numpy_restatement_equals_golden(core, name):
    """PIL's resampler restated in integers with core.resample_table, then the look-up table: every golden bit for bit
    (the 2294 x 1914 case included: the tables, not the image size, are what can go wrong)."""
    c = R.case(name)
    pre = R.spec_of(core, c)
    out = np.stack([R.numpy_preprocess(core, a, pre) for a in R.case_input(c)])
    R.check_against_golden(c, out)


def test_tap_counts_of_the_many_tap_case(core):
    """Case 5 is what sizes the kernel's tap cap: 199 -> 21 is ratio 9.48, PIL's ksize = 2 ceil(support) + 1 is 39
    (bicubic) and 21 (bilinear); a table is as wide as its widest row, one or two short of ksize."""
    assert 37 <= core.resample_table(199, 21, "bicubic").shape[1] - 2 <= 39
    assert 19 <= core.resample_table(199, 21, "bilinear").shape[1] - 2 <= 21
    assert core.resample_table(16 * 40, 40, "bilinear").shape[1] - 2 <= 33 <= core.IMAGE_MAX_TAPS     # ratio 16
    t = core.resample_table(20, 33, "bilinear")            # up-scaling: support 1, at most 3 taps
    assert t.shape[0] == 33 and 2 <= t.shape[1] - 2 <= 3 and t.dtype == torch.int32
    assert int((t[:, 0] + t[:, 1]).max()) <= 20 and int(t[:, 0].min()) == 0
    assert torch.equal(t[:, 2:].sum(dim=1), torch.full((33,), 1 << 22, dtype=torch.int64))


def test_plan_sizes_and_crop_offsets(core):
    P = core.Preprocess
    p = P("bilinear", 256, 224).plan(375, 500)             # Resize(256): the shorter side, int(256 * 500 / 375) = 341
    assert (p.RH, p.RW, p.top, p.left, p.OH, p.OW) == (256, 341, 16, 58, 224, 224)      # round(58.5) = 58: half to even
    p = P("bilinear", 256, 224).plan(500, 375)
    assert (p.RH, p.RW, p.top, p.left) == (341, 256, 58, 16)
    p = P("bilinear", (23, 21), 12).plan(40, 56)           # the two .5 roundings: round(5.5) = 6, round(4.5) = 4
    assert (p.RH, p.RW, p.top, p.left) == (23, 21, 6, 4)
    p = P("bilinear", 16, 12).plan(37, 53)
    assert (p.RH, p.RW) == (16, int(16 * 53 / 37))
    p = P("bilinear", (16, 16)).plan(17, 16)               # one axis unchanged: that pass is skipped
    assert p.xtab is None and p.ytab is not None and p.taps[0] == 0
    p = P("bilinear", (16, 16)).plan(16, 16)
    assert p.xtab is None and p.ytab is None and (p.OH, p.OW) == (16, 16)
    p = core.PRESETS["tensor"].plan(31, 47)                # no resize, no crop
    assert (p.RH, p.RW, p.top, p.left, p.OH, p.OW) == (31, 47, 0, 0, 31, 47)
    p = core.PRESETS["embed"].plan(2294, 1914)
    assert (p.OH, p.OW) == (1520, 912) and p.device_ok
    assert not P("bilinear", (4, 4)).plan(4 * 200, 4).device_ok        # 401 vertical taps: past the kernel's cap
    with pytest.raises(ValueError, match="crop"):
        P("bilinear", 16, 32).plan(37, 53)                 # torchvision would pad
    with pytest.raises(ValueError):
        core.get_preprocess("no_such_preset")


def test_presets_are_the_references(core):
    k = {n: p._key() for n, p in core.PRESETS.items()}
    assert k["imagenet"] == ("bilinear", 256, (224, 224), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert k["clip"] == ("bicubic", 224, (224, 224), (0.48145466, 0.4578275, 0.40821073),
                         (0.26862954, 0.26130258, 0.27577711))
    assert k["embed"] == ("bilinear", (1520, 912), None, None, None)
    assert k["tensor"] == ("bilinear", None, None, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def test_lut_equals_the_torch_ops(core):
    v = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).repeat(3, 1, 1)        # a [3, 256, 1] "image"
    t = v.to(torch.float32).div(255)
    assert torch.equal(core.PRESETS["embed"].lut(), t[:, :, 0])
    for name, (mean, std) in (("imagenet", (core.IMAGENET_MEAN, core.IMAGENET_STD)), ("clip", (core.CLIP_MEAN, core.CLIP_STD))):
        m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
        want = t.clone().sub_(m[:, None, None]).div_(s[:, None, None])              # Normalize's in-place form
        lut = core.PRESETS[name].lut()
        assert lut.dtype == torch.float32 and lut.shape == (3, 256) and torch.equal(lut, want[:, :, 0])


def test_image_preprocess_is_gpu_only(core):
    with pytest.raises(TypeError, match="GPU only"):
        core.image_preprocess(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), "tensor")


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_listing_order(du, tmp_path):
    root = str(tmp_path / "tree")
    for rel in ("b/2.png", "b/10.png", "a/z.JPG", "a/sub/c.jpeg", "a/k.txt", "a/sub2/x.webp", "c/1.bmp", "loose.png"):
        _touch(os.path.join(root, rel))
    got = [(os.path.relpath(p, root), l) for p, l in du.list_folder(root)]
    # classes sorted; inside a class the directories in sorted order, the files of each sorted by name (string order:
    # 10.png before 2.png); other extensions and files outside a class folder are not samples
    assert got == [("a/z.JPG", 0), ("a/sub/c.jpeg", 0), ("a/sub2/x.webp", 0), ("b/10.png", 1), ("b/2.png", 1), ("c/1.bmp", 2)]

    txt = tmp_path / "set.txt"
    txt.write_text("/x/b.png 3\n/x/a.png 1\n/x/c.png 2\n")
    assert du.list_txt(str(txt)) == [("/x/b.png", 3), ("/x/a.png", 1), ("/x/c.png", 2)]          # file order, not sorted

    csv = tmp_path / "set.csv"
    csv.write_text("filename,Implant_type,Marker\nq.png,implant,No\na.png,non-implant,Yes\nm.png,other,No\n")
    rows = du.list_csv("/r", str(csv), "Implant_type")
    assert [p for p, _ in rows] == ["/r/q.png", "/r/a.png", "/r/m.png"]
    assert rows[0][1] == 1 and rows[1][1] == 0 and np.isnan(rows[2][1])                           # pandas' map: NaN
    assert [l for _, l in du.list_csv("/r", str(csv), "Marker")] == [0, 1, 0]
    bad = tmp_path / "bad.csv"
    bad.write_text("filename,other\nq.png,1\n")
    with pytest.raises(ValueError, match="must contain"):
        du.list_csv("/r", str(bad), "Marker")


def _route_probe(du, core, **kw):
    z, meta = R.goldens()
    n = meta["route"]["n"]
    views = {v: R.spec_of(core, s) for v, s in meta["route"]["views"].items()}
    samples = [("route_in_%d" % i, i % 3) for i in range(n)]
    return du.ImageFileProbe(samples, views["a"], views["b"], decode=lambda key: z[key], **kw), z, n


def test_host_route_equals_goldens_and_shards(du, core):
    """dataset[i] on the host route (PIL + torch) is the golden pair; lo / hi select a shard of the sample list."""
    pytest.importorskip("PIL")
    ds, z, n = _route_probe(du, core)
    assert len(ds) == n and ds.device is None
    for i in range(n):
        (a, b), label = ds[i]
        assert label == i % 3
        assert torch.equal(a, torch.from_numpy(z["route_out_a"][i])) and torch.equal(b, torch.from_numpy(z["route_out_b"][i]))
    shard, _, _ = _route_probe(du, core, lo=2, hi=5)
    assert len(shard) == 3 and shard.n_total == n and [p for p, _ in shard.samples] == ["route_in_%d" % i for i in (2, 3, 4)]
    assert torch.equal(shard[0][0][0], torch.from_numpy(z["route_out_a"][2]))
    one = du.ImageFileProbe(ds.samples, ds.preprocess, ds.preprocess, decode=ds.decode)       # equal views collapse
    assert one.clip_preprocess is None and torch.equal(one[1][0], torch.from_numpy(z["route_out_a"][1]))
    with pytest.raises(RuntimeError, match="CUDA device"):
        next(ds.device_batches(4))


@pytest.mark.parametrize("name", R.case_names(large=False))
def test_host_route_equals_every_small_golden(du, core, name):
    pytest.importorskip("PIL")
    c = R.case(name)
    pre = R.spec_of(core, c)
    R.check_against_golden(c, np.stack([du.host_preprocess(a, pre).numpy() for a in R.case_input(c)]))


def test_registry(du, tmp_path, monkeypatch):
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.delenv("MCD_DATASETS", raising=False)
    with pytest.raises(ValueError, match="not available offline"):
        du.get_data("cifar100_train")                                  # unregistered, and not a probe set of this build
    with pytest.raises(ValueError, match="imagenet_val"):
        du.get_data("imagenet_val")                                    # a known set without a path
    missing = str(tmp_path / "nowhere")
    du.register_dataset("imagenet_val", path=missing)
    with pytest.raises(FileNotFoundError, match="nowhere"):            # the error names the path
        du.get_data("imagenet_val")
    for name, files in (("val", ("n1/a.png", "n2/b.png")), ("broden", ("x/c.png",))):
        for rel in files:
            _touch(str(tmp_path / name / rel))
    du.register_dataset("imagenet_val", path=str(tmp_path / "val"))
    table = tmp_path / "sets.json"
    table.write_text(json.dumps({"broden": {"path": str(tmp_path / "broden")}}))
    monkeypatch.setenv("MCD_DATASETS", str(table))                     # the JSON table serves what the code did not set
    ds = du.get_data("imagenet_broden", lo=1, hi=3)                    # the concatenation, val first
    assert [os.path.basename(p) for p, _ in ds.samples] == ["b.png", "c.png"] and ds.n_total == 3
    assert ds.preprocess == du.core.PRESETS["imagenet"] and ds.clip_preprocess is None
    ds = du.get_data("imagenet_val", "clip", clip_preprocess="default")
    assert ds.preprocess == du.core.PRESETS["clip"] and ds.clip_preprocess == du.core.PRESETS["imagenet"]
    assert {k: v[1] for k, v in du.DATASET_KINDS.items() if k.startswith("embed_")} == {
        k: "embed" for k in ("embed_png", "embed_marker_84", "embed_implant", "embed_marker_only", "embed_non_implant",
                             "embed_non_implant_100")}
    assert du.DATASET_KINDS["imagenet_subsets"] == ("txt", "tensor")
    assert du.target_preset("breastclip_classifier") is None and du.target_preset("resnet18") == "imagenet"


def test_synthetic_names_unchanged(du):
    ds = du.get_data("synthetic_6_32")
    assert isinstance(ds, du.SyntheticImages) and len(ds) == 6 and ds[2][0].shape == (3, 32, 32)
    g = torch.Generator().manual_seed(1234 * 1000003 + 2)
    assert torch.equal(ds[2][0], torch.randn(3, 32, 32, generator=g)) and ds[2][1] == 0
    sub = du.get_data("synthetic_6_8x12", None, None, 2, 5)
    assert isinstance(sub, torch.utils.data.Subset) and len(sub) == 3 and sub[0][0].shape == (3, 8, 12)
    with pytest.raises(ValueError, match="<S> or <H>x<W>"):
        du.get_data("synthetic_4_big")


def test_abi_table_has_the_entry(mcd):
    L = mcd._lib.load()
    assert "mcd_image_preprocess" in mcd._lib.SIGNATURES and hasattr(L, "mcd_image_preprocess")
    assert len(mcd._lib.SIGNATURES["mcd_image_preprocess"][1]) == 18 and L.mcd_abi_version() == 9
