"""CPU: the host side of the mammogram probe sets (vindr, vindr_alt, csaw, csaw_all_splits) and of K23 -- the table
restatement, the host route, listing, decoding, presets, the registry -- against goldens made by the reference's own
dataset classes (tests/golden/make_golden_mammo.py).  No GPU call is made here."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mammo_recipe as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _host(du, c, a):
    return du.host_minmax(a, c["mean"], c["std"]) if c["mode"] == "minmax" else du.host_raw(a)


@pytest.mark.parametrize("name", R.case_names())
def test_table_restatement_and_host_route_equal_the_reference(du, name):
    """The 256-entry table indexed by the image's bytes, and host_minmax / host_raw, are the reference's output bit for
    bit in every case (NaN as a mask for the constant images)."""
    c = R.case(name)
    src = R.case_input(c)
    R.check_against_golden(c, R.numpy_apply(src, c))
    out = [_host(du, c, a) for a in src]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == 3 for t in out)
    R.check_against_golden(c, np.stack([t.numpy() for t in out]))


def test_meta_records_what_the_reference_did(core):
    meta = R.goldens()[1]
    assert "load_transform_valid" in meta and meta["load_transform_valid"] is None      # nothing is resized at 1520 x 912
    assert meta["transform_config"]["valid"]["Resize"] == {"size_h": 1520, "size_w": 912}
    assert meta["chunk"] == core.IMAGE_MINMAX_CHUNK
    ext = R.case_input(R.case("extremes_last"))
    assert 2 * core.IMAGE_MINMAX_CHUNK < ext.size < 2 * core.IMAGE_MINMAX_CHUNK + 64            # just over two chunks
    flat = ext.reshape(-1)
    assert flat[0] == 0 and flat[-1] == 255 and flat[1:].min() > 0 and flat[:-1].max() < 255
    ch = R.case_input(R.case("rgb_channels"))[0]
    assert ch[:, :, 2].min() < ch[:, :, :2].min() and ch[:, :, 0].max() > ch[:, :, 1:].max()
    assert [int(a.min()) for a in R.case_input(R.case("batch3"))] == [0, 100, 17]
    assert [int(a.max()) for a in R.case_input(R.case("batch3"))] == [255, 101, 200]


def test_list_vindr(du, tmp_path):
    (tmp_path / "d").mkdir()
    (tmp_path / "d" / "folds.csv").write_text(
        "patient_id,image_id,laterality,view,split,Mass,fold\n"
        "007,b.png,L,CC,test,1,0\n"
        "12,zz,R,MLO,training,0,1\n"
        "007,a,R,CC,test,,2\n"
        "0100,c.PNG,L,MLO,test,0,3\n")
    got = du.list_vindr(str(tmp_path), "imgs", "d/folds.csv")
    base = os.path.join(str(tmp_path), "imgs")
    # the 'test' rows in file order (not sorted), patient_id kept as a string, '.png' appended unless the name ends in it
    # (case-sensitive, as the reference's endswith), a missing Mass is 0 (fillna)
    assert got == [(os.path.join(base, "007", "b.png"), 1), (os.path.join(base, "007", "a.png"), 0),
                   (os.path.join(base, "0100", "c.PNG.png"), 0)]
    assert all(isinstance(label, int) for _, label in got)
    assert du.VINDR_IMG_DIR == "VinDR_MammoCLIP/images_png" and du.VINDR_CSV == "VinDR-data/vindr_detection_v1_folds.csv"


def test_list_csaw(du, tmp_path):
    (tmp_path / "ann.csv").write_text("anon_filename,Cancer_visible,split\nq_1.dcm,1,test\na_2.dcm,0,train\nm_3.dcm,0,test\n")
    rows = du.list_csaw(str(tmp_path), "ann.csv", "/imgs", "test")
    assert rows == [("/imgs/q_1.png", 1), ("/imgs/m_3.png", 0)]
    assert [p for p, _ in du.list_csaw(str(tmp_path), "ann.csv", "/imgs", None)] == ["/imgs/q_1.png", "/imgs/a_2.png",
                                                                                    "/imgs/m_3.png"]


def test_decoding(du, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(5)
    grey, rgb = rs.randint(0, 256, (9, 6)).astype(np.uint8), rs.randint(0, 256, (9, 6, 3)).astype(np.uint8)
    Image.fromarray(grey, "L").save(str(tmp_path / "g.png"))
    Image.fromarray(rgb, "RGB").save(str(tmp_path / "c.png"))
    Image.fromarray(grey.astype(np.uint16) * 257).save(str(tmp_path / "w.png"))
    a = du.decode_vindr(str(tmp_path / "g.png"))
    assert a.dtype == np.uint8 and a.shape == (9, 6) and np.array_equal(a, grey)             # mode L stays 2-D
    with Image.open(str(tmp_path / "g.png")) as img:
        assert np.array_equal(np.asarray(img.convert("RGB")), np.repeat(grey[:, :, None], 3, axis=2))
    b = du.decode_vindr(str(tmp_path / "c.png"))
    assert b.dtype == np.uint8 and np.array_equal(b, rgb)
    assert np.array_equal(du.decode_csaw(str(tmp_path / "g.png")), grey)
    w = du.decode_csaw(str(tmp_path / "w.png"))                                              # 16 bit: converted on the host
    assert w.dtype == np.float32 and np.array_equal(w, grey.astype(np.float32) * 257)
    assert torch.equal(du.host_raw(w)[1], torch.from_numpy(w))
    with pytest.raises(ValueError, match="grey"):
        du.decode_csaw(str(tmp_path / "c.png"))


def test_presets_and_spec_equality(core):
    v, c = core.PRESETS["vindr"], core.PRESETS["csaw"]
    assert isinstance(v, core.MinMaxNormalize) and (v.mean, v.std) == (0.3089279, 0.25053555408335154)
    assert isinstance(c, core.RawGray)
    assert v == core.MinMaxNormalize(0.3089279, 0.25053555408335154) and hash(v) == hash(core.MinMaxNormalize(v.mean, v.std))
    assert v != core.MinMaxNormalize(0.3, 0.25) and v != c and c == core.RawGray() and hash(c) == hash(core.RawGray())
    assert v != core.PRESETS["tensor"] and core.PRESETS["tensor"] != v and len({v, c, core.RawGray()}) == 2
    assert repr(v) == "MinMaxNormalize(mean=0.3089279, std=0.25053555408335154)" and repr(c) == "RawGray()"
    assert core.get_preprocess("vindr") is v and core.get_preprocess(c) is c and core.get_preprocess(v) is v
    assert core.IMAGE_MODES == {"minmax": 0, "raw": 1}
    with pytest.raises(TypeError, match="GPU only"):
        core.image_minmax_normalize(torch.zeros((1, 4, 4), dtype=torch.uint8), v.mean, v.std)


def _write_vindr(tmp_path, arrays):
    Image = pytest.importorskip("PIL.Image")
    lines = ["patient_id,image_id,split,Mass"]
    for i, a in enumerate(arrays):
        d = tmp_path / "VinDR_MammoCLIP" / "images_png" / ("%03d" % i)
        d.mkdir(parents=True)
        Image.fromarray(a, "L" if a.ndim == 2 else "RGB").save(str(d / ("im%d.png" % i)))
        lines.append("%03d,im%d,test,%d" % (i, i, i % 2))
    (tmp_path / "VinDR-data").mkdir()
    (tmp_path / "VinDR-data" / "vindr_detection_v1_folds.csv").write_text("\n".join(lines) + "\n")


def test_registry_and_the_fixed_transform(du, core, tmp_path, monkeypatch):
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.delenv("MCD_DATASETS", raising=False)
    with pytest.raises(ValueError, match="register_dataset"):
        du.get_data("vindr")                                                   # known, but without a path
    with pytest.raises(ValueError, match="not available offline.*one size"):
        du.get_data("combined")
    assert {k: du.DATASET_KINDS[k][1] for k in du.FIXED_TRANSFORM} == {"vindr": "vindr", "vindr_alt": "vindr",
                                                                      "csaw": "csaw", "csaw_all_splits": "csaw"}
    srcs = [R.case_input(R.case("gray_wide"))[0], R.case_input(R.case("gray_wide"))[0][::-1].copy()]
    _write_vindr(tmp_path, srcs)
    du.register_dataset("vindr", root=str(tmp_path))                           # the reference's relative defaults
    for name in ("vindr", "vindr_alt"):                                        # the same samples, the same transform
        ds = du.get_data(name)
        assert len(ds) == 2 and ds.preprocess == core.PRESETS["vindr"] and ds.clip_preprocess is None
        assert ds.decode is du.decode_vindr and ds.samples[1] == (os.path.join(
            str(tmp_path), "VinDR_MammoCLIP/images_png", "001", "im1.png"), 1)
    # the set's own transform under any of its names is accepted, anything else is refused
    ds = du.get_data("vindr", "vindr", clip_preprocess="default")
    assert len(ds.views) == 1
    du.get_data("vindr", core.MinMaxNormalize(0.3089279, 0.25053555408335154), clip_preprocess="vindr")
    for kw in (dict(preprocess="imagenet"), dict(clip_preprocess="clip"), dict(preprocess=core.MinMaxNormalize(0.0, 1.0)),
               dict(preprocess="csaw")):
        with pytest.raises(ValueError, match="own transform"):
            du.get_data("vindr", **kw)
    # the host route's item is the golden
    c = R.case("gray_wide")
    item, label = ds[0]
    assert label == 0
    R.check_against_golden(c, item.numpy()[None])
    # path= and csv= override the defaults; the JSON table takes the same keys
    (tmp_path / "other").mkdir()
    os.rename(str(tmp_path / "VinDR-data" / "vindr_detection_v1_folds.csv"), str(tmp_path / "other" / "f.csv"))
    with pytest.raises(FileNotFoundError, match="vindr_detection_v1_folds"):
        du.get_data("vindr")
    table = tmp_path / "sets.json"
    table.write_text(json.dumps({"vindr": {"root": str(tmp_path), "csv": "other/f.csv", "path": "VinDR_MammoCLIP/images_png"}}))
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.setenv("MCD_DATASETS", str(table))
    assert len(du.get_data("vindr_alt", lo=1, hi=2)) == 1


def test_csaw_sets(du, core, tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    monkeypatch.setattr(du, "DATASET_ROOTS", {})
    monkeypatch.delenv("MCD_DATASETS", raising=False)
    c = R.case("csaw_raw")
    src = R.case_input(c)[0]
    (tmp_path / "png").mkdir()
    for name, a in (("t0", src), ("v0", src[::-1].copy()), ("t1", np.roll(src, 3, axis=0))):
        Image.fromarray(np.ascontiguousarray(a), "L").save(str(tmp_path / "png" / (name + ".png")))
    (tmp_path / "ann.csv").write_text("anon_filename,Cancer_visible,split\nt0.dcm,1,test\nv0.dcm,0,val\nt1.dcm,0,test\n")
    du.register_dataset("csaw", root=str(tmp_path), csv="ann.csv", path=str(tmp_path / "png"))
    ds = du.get_data("csaw")
    assert [os.path.basename(p) for p, _ in ds.samples] == ["t0.png", "t1.png"] and ds.preprocess == core.RawGray()
    item, label = ds[0]
    assert label == 1
    R.check_against_golden(c, item.numpy()[None])
    every = du.get_data("csaw_all_splits")                                     # CSV order, every split
    assert [os.path.basename(p) for p, _ in every.samples] == ["t0.png", "v0.png", "t1.png"]
    with pytest.raises(ValueError, match="own transform"):
        du.get_data("csaw", "embed")
    with pytest.raises(ValueError, match="both views"):
        du.ImageFileProbe(ds.samples, "csaw", "imagenet")


def test_abi_table_has_the_entries(mcd, core):
    L = mcd._lib.load()
    h = open(os.path.join(ROOT, "include", "mcd_hip.h")).read()
    for name, nargs in (("mcd_image_minmax_workspace", 4), ("mcd_image_minmax_normalize", 13)):
        assert name in mcd._lib.SIGNATURES and hasattr(L, name) and re.search(r"\b%s\(" % name, h)
        assert len(mcd._lib.SIGNATURES[name][1]) == nargs
    assert L.mcd_abi_version() == 9
    assert "#define MCD_IMAGE_MINMAX_CHUNK %d\n" % core.IMAGE_MINMAX_CHUNK in h
    assert "#define MCD_IMG_MINMAX 0\n" in h and "#define MCD_IMG_RAW 1\n" in h
    # the workspace: one int32 pair per chunk, at most 256 chunks per image (the chunk doubles past that)
    chunk = core.IMAGE_MINMAX_CHUNK
    assert L.mcd_image_minmax_workspace(1, 1, 1, 1) == 8
    assert L.mcd_image_minmax_workspace(3, 1, chunk + 1, 1) == 3 * 2 * 8
    assert L.mcd_image_minmax_workspace(16, 1520, 912, 3) == 16 * 254 * 8
    assert L.mcd_image_minmax_workspace(1, 1, 256 * chunk + 1, 1) == 129 * 8
    assert L.mcd_image_minmax_workspace(1, 4, 4, 2) == 0 and L.mcd_image_minmax_workspace(1, 0, 4, 1) == 0
