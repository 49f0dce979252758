"""CPU: concept_vit/checkpoint_io.py -- the safetensors reader against the `safetensors` package's writer (and the writer
against its reader), every malformed-file defect as a ValueError naming the file, and the resolution of snapshot
directories as the installed transformers' save_pretrained writes them: sharded safetensors, .bin, sharded .bin, a deleted
shard, an index that points outside, an empty directory, a hub cache's symlinked snapshots/<rev>/.

transformers and safetensors are test-side only; their absence is a failure, not a skip."""
import json
import os
import struct

import pytest
import torch


@pytest.fixture(scope="module")
def io(mcd):
    from mammo_clip_dissect_amd.concept_vit import checkpoint_io
    return checkpoint_io


def _tensors():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(6, 10, generator=g)
    t = {"f64": torch.randn(3, 5, generator=g, dtype=torch.float64), "f32": base.clone(), "f16": base.half(),
         "bf16": base.bfloat16(), "i64": torch.randint(-2 ** 40, 2 ** 40, (7,), generator=g),
         "i32": torch.randint(-2 ** 30, 2 ** 30, (2, 3), generator=g, dtype=torch.int32),
         "i16": torch.randint(-2 ** 15, 2 ** 15, (5,), generator=g, dtype=torch.int16),
         "i8": torch.randint(-128, 128, (9,), generator=g, dtype=torch.int8),
         "u8": torch.randint(0, 256, (11,), generator=g, dtype=torch.uint8),
         "bool": torch.randint(0, 2, (3, 3), generator=g).bool(),
         "scalar": torch.tensor(2.5), "scalar_i64": torch.tensor(-7), "empty": torch.empty(0, 4), "empty_f16": torch.empty(2, 0, 3).half()}
    assert t["scalar"].dim() == 0 and t["empty"].numel() == 0
    return t


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and tuple(got[k].shape) == tuple(v.shape) and torch.equal(got[k], v), k


def test_reader_against_the_safetensors_writer(io, tmp_path):
    from safetensors.torch import save_file
    t = _tensors()
    path = str(tmp_path / "a.safetensors")
    save_file({k: v.contiguous() for k, v in t.items()}, path, metadata={"format": "pt", "note": "ignored"})
    got = io.read_safetensors(path)
    _same(got, t)
    assert all(v.is_contiguous() and v.device.type == "cpu" for v in got.values())
    # nothing aliases the file: the tensors outlive it and can be written
    os.remove(path)
    got["f32"].add_(1.0)
    assert torch.equal(got["f32"], t["f32"] + 1.0)


def test_writer_against_the_safetensors_reader_with_non_contiguous_inputs(io, tmp_path):
    from safetensors.torch import load_file
    t = _tensors()
    t["transposed"] = t["f32"].t()
    t["strided"] = t["f64"][:, ::2]
    t["expanded"] = torch.arange(3.0).expand(4, 3)
    assert not t["transposed"].is_contiguous() and not t["strided"].is_contiguous() and not t["expanded"].is_contiguous()
    path = str(tmp_path / "b.safetensors")
    io.write_safetensors(path, t)
    _same(load_file(path), t)
    _same(io.read_safetensors(path), t)
    raw = open(path, "rb").read()
    (n,) = struct.unpack("<Q", raw[:8])
    header = json.loads(raw[8:8 + n])
    assert n % 8 == 0 and header["__metadata__"] == {"format": "pt"}
    names = [k for k in header if k != "__metadata__"]
    assert names == sorted(names)
    with pytest.raises(ValueError, match="complex"):
        io.write_safetensors(str(tmp_path / "c.safetensors"), {"complex": torch.zeros(2, dtype=torch.complex64)})


# ---- malformed files: bytes of a valid file edited by hand ------------------------------------------------------------------
def _valid(io, tmp_path):
    path = str(tmp_path / "valid.safetensors")
    io.write_safetensors(path, {"a": torch.arange(6, dtype=torch.float32).reshape(2, 3), "b": torch.arange(4, dtype=torch.int16)})
    raw = open(path, "rb").read()
    (n,) = struct.unpack("<Q", raw[:8])
    return json.loads(raw[8:8 + n]), raw[8 + n:]


def _write(tmp_path, name, header, data):
    raw = header if isinstance(header, bytes) else json.dumps(header).encode()
    path = tmp_path / name
    path.write_bytes(struct.pack("<Q", len(raw)) + raw + data)
    return str(path)


def _edited(header, name, **fields):
    h = json.loads(json.dumps(header))
    h[name].update(fields)
    return h


def test_malformed_files_are_value_errors_that_name_the_file(io, tmp_path):
    header, data = _valid(io, tmp_path)
    assert header["a"]["data_offsets"] == [0, 24] and header["b"]["data_offsets"] == [24, 32] and len(data) == 32
    good = _write(tmp_path, "good.safetensors", header, data)
    assert torch.equal(io.read_safetensors(good)["a"], torch.arange(6.0).reshape(2, 3))
    raw = open(good, "rb").read()
    cases = {}
    (tmp_path / "short.safetensors").write_bytes(raw[:5])
    cases["short"] = (str(tmp_path / "short.safetensors"), "shorter than")
    (tmp_path / "empty.safetensors").write_bytes(b"")
    cases["empty"] = (str(tmp_path / "empty.safetensors"), "shorter than")
    (tmp_path / "past_end.safetensors").write_bytes(struct.pack("<Q", len(raw)) + raw[8:])
    cases["past_end"] = (str(tmp_path / "past_end.safetensors"), "past the end")
    (tmp_path / "huge.safetensors").write_bytes(struct.pack("<Q", 100 * 1000 * 1000 + 1) + raw[8:])
    cases["huge"] = (str(tmp_path / "huge.safetensors"), "limit")
    (tmp_path / "all_ones.safetensors").write_bytes(b"\xff" * 8 + raw[8:])
    cases["all_ones"] = (str(tmp_path / "all_ones.safetensors"), "limit")
    cases["list"] = (_write(tmp_path, "list.safetensors", b"[1, 2, 3]", data), "not a JSON object")
    cases["not_json"] = (_write(tmp_path, "not_json.safetensors", b"{\"a\": ", data), "not JSON")
    cases["not_utf8"] = (_write(tmp_path, "not_utf8.safetensors", b"\xff\xfe{}", data), "not JSON")
    cases["entry"] = (_write(tmp_path, "entry.safetensors", dict(header, a=[1]), data), "not an object")
    cases["dtype"] = (_write(tmp_path, "dtype.safetensors", _edited(header, "a", dtype="F8_E4M3"), data), "unknown dtype")
    cases["no_dtype"] = (_write(tmp_path, "no_dtype.safetensors", _edited(header, "a", dtype=None), data), "unknown dtype")
    cases["oob"] = (_write(tmp_path, "oob.safetensors", _edited(header, "b", data_offsets=[24, 40], shape=[8]), data), "outside")
    cases["truncated"] = (_write(tmp_path, "truncated.safetensors", header, data[:-2]), "outside")
    cases["negative_offset"] = (_write(tmp_path, "negative_offset.safetensors", _edited(header, "a", data_offsets=[-24, 0]), data),
                                "outside")
    cases["reversed"] = (_write(tmp_path, "reversed.safetensors", _edited(header, "a", data_offsets=[24, 0]), data), "reversed")
    cases["overlap"] = (_write(tmp_path, "overlap.safetensors", _edited(header, "b", data_offsets=[16, 24]), data), "overlap")
    cases["span"] = (_write(tmp_path, "span.safetensors", _edited(header, "a", shape=[2, 4]), data), "spans 24 bytes")
    cases["span_dtype"] = (_write(tmp_path, "span_dtype.safetensors", _edited(header, "a", dtype="F64"), data), "spans 24 bytes")
    cases["negative_dim"] = (_write(tmp_path, "negative_dim.safetensors", _edited(header, "a", shape=[-2, -3]), data), "negative")
    cases["float_dim"] = (_write(tmp_path, "float_dim.safetensors", _edited(header, "a", shape=[2.0, 3]), data), "integers")
    cases["offsets_shape"] = (_write(tmp_path, "offsets_shape.safetensors", _edited(header, "a", data_offsets=[0]), data), "pair")
    for name, (path, what) in cases.items():
        with pytest.raises(ValueError, match=what) as e:
            io.read_safetensors(path)
        assert os.path.basename(path) in str(e.value), (name, str(e.value))


# ---- resolution -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """One 128-wide two-layer ViT classifier saved four ways by the installed transformers."""
    import transformers                                  # its absence is a failure: the formats under test are its own
    root = tmp_path_factory.mktemp("snapshots")
    torch.manual_seed(3)
    model = transformers.ViTForImageClassification(transformers.ViTConfig(
        hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256, image_size=32, patch_size=16,
        num_labels=3)).eval()
    dirs = {k: str(root / k) for k in ("single", "sharded", "bin", "sharded_bin")}
    model.save_pretrained(dirs["single"])
    model.save_pretrained(dirs["sharded"], max_shard_size="200KB")
    model.save_pretrained(dirs["bin"], safe_serialization=False)
    model.save_pretrained(dirs["sharded_bin"], safe_serialization=False, max_shard_size="200KB")
    from safetensors.torch import load_file
    # (the saved names are the checkpoint format's, vit.encoder.layer.0.attention.attention.query...; transformers 5.x
    # keeps other names in memory, so the reference is the single file as the safetensors package reads it)
    want = load_file(os.path.join(dirs["single"], "model.safetensors"))
    if not os.path.isfile(os.path.join(dirs["bin"], "pytorch_model.bin")):
        # transformers 5.x (5.15.0 here) no longer writes the pickle forms and ignores safe_serialization=False: the two
        # directories hold safetensors again.  The .bin layouts are 4.x's -- pytorch_model.bin, or pytorch_model-0000k-of-
        # 0000n.bin + pytorch_model.bin.index.json with the same weight_map -- so they are rewritten here by that rule,
        # with the shards transformers chose for the safetensors form.
        os.remove(os.path.join(dirs["bin"], "model.safetensors"))
        torch.save(want, os.path.join(dirs["bin"], "pytorch_model.bin"))
        d = dirs["sharded_bin"]
        table = json.load(open(os.path.join(d, "model.safetensors.index.json")))
        rename = {s: s.replace("model-", "pytorch_model-").replace(".safetensors", ".bin") for s in set(table["weight_map"].values())}
        for old, new in rename.items():
            torch.save({k: want[k] for k, s in table["weight_map"].items() if s == old}, os.path.join(d, new))
            os.remove(os.path.join(d, old))
        table["weight_map"] = {k: rename[s] for k, s in table["weight_map"].items()}
        json.dump(table, open(os.path.join(d, "pytorch_model.bin.index.json"), "w"))
        os.remove(os.path.join(d, "model.safetensors.index.json"))
    return dirs, want


def test_the_four_layouts_give_the_same_state_dict(io, saved):
    dirs, want = saved
    assert os.path.isfile(os.path.join(dirs["single"], "model.safetensors"))
    assert os.path.isfile(os.path.join(dirs["sharded"], "model.safetensors.index.json"))
    assert len([f for f in os.listdir(dirs["sharded"]) if f.endswith(".safetensors")]) > 1
    assert os.path.isfile(os.path.join(dirs["bin"], "pytorch_model.bin"))
    assert os.path.isfile(os.path.join(dirs["sharded_bin"], "pytorch_model.bin.index.json"))
    single = io.resolve_checkpoint(dirs["single"])
    assert single.root == dirs["single"] and single.config["model_type"] == "vit" and single.config["num_attention_heads"] == 4
    base = single.state_dict()
    assert single.state_dict() is base                                  # read once
    _same(base, want)
    for k in ("sharded", "bin", "sharded_bin"):
        snap = io.resolve_checkpoint(dirs[k])
        assert snap.config == single.config
        _same(snap.state_dict(), base)
    # a single file resolves too and takes the config.json beside it; a torch file carries none
    one = io.resolve_checkpoint(os.path.join(dirs["single"], "model.safetensors"))
    assert one.config == single.config and one.root == dirs["single"]
    _same(one.state_dict(), base)
    assert io.resolve_checkpoint(os.path.join(dirs["bin"], "pytorch_model.bin")).config is None


def test_lookup_order_is_from_pretraineds(io, saved, tmp_path):
    import shutil
    dirs, want = saved
    d = str(tmp_path / "both")
    shutil.copytree(dirs["bin"], d)
    marked = {k: v + 1 for k, v in want.items()}
    io.write_safetensors(os.path.join(d, "model.safetensors"), marked)
    _same(io.resolve_checkpoint(d).state_dict(), marked)               # model.safetensors wins over pytorch_model.bin


def test_broken_directories(io, saved, tmp_path):
    import shutil
    dirs, _ = saved
    d = str(tmp_path / "missing_shard")
    shutil.copytree(dirs["sharded"], d)
    shards = sorted(f for f in os.listdir(d) if f.endswith(".safetensors"))
    os.remove(os.path.join(d, shards[1]))
    with pytest.raises(FileNotFoundError, match=shards[1].replace(".", r"\.")):
        io.resolve_checkpoint(d).state_dict()
    for bad in ("../x.safetensors", "..", "sub/x.safetensors", "/etc/x.safetensors"):
        d = str(tmp_path / ("outside_%d" % len(os.listdir(str(tmp_path)))))
        shutil.copytree(dirs["sharded"], d)
        index = os.path.join(d, "model.safetensors.index.json")
        table = json.load(open(index))
        table["weight_map"][sorted(table["weight_map"])[0]] = bad
        json.dump(table, open(index, "w"))
        with pytest.raises(ValueError, match="plain file name"):
            io.resolve_checkpoint(d).state_dict()
    # a key the index gives to a shard that does not hold it
    d = str(tmp_path / "moved_key")
    shutil.copytree(dirs["sharded"], d)
    index = os.path.join(d, "model.safetensors.index.json")
    table = json.load(open(index))
    keys = sorted(table["weight_map"])
    other = next(k for k in keys if table["weight_map"][k] != table["weight_map"][keys[0]])
    table["weight_map"][keys[0]] = table["weight_map"][other]
    json.dump(table, open(index, "w"))
    with pytest.raises(ValueError, match="not in the shard"):
        io.resolve_checkpoint(d).state_dict()
    # a key listed twice in the index, and a key held by two shards
    d = str(tmp_path / "listed_twice")
    shutil.copytree(dirs["sharded"], d)
    index = os.path.join(d, "model.safetensors.index.json")
    table = json.load(open(index))
    text = json.dumps(table)
    first = '"%s": "%s"' % (keys[0], table["weight_map"][keys[0]])
    assert first in text
    open(index, "w").write(text.replace(first, first + ", " + '"%s": "%s"' % (keys[0], table["weight_map"][other]), 1))
    with pytest.raises(ValueError, match="listed twice"):
        io.resolve_checkpoint(d).state_dict()
    d = str(tmp_path / "in_two_shards")
    shutil.copytree(dirs["sharded"], d)
    a, b = os.path.join(d, table["weight_map"][keys[0]]), os.path.join(d, table["weight_map"][other])
    extra = io.read_safetensors(b)
    extra[keys[0]] = io.read_safetensors(a)[keys[0]]
    io.write_safetensors(b, extra)
    with pytest.raises(ValueError, match="two shards"):
        io.resolve_checkpoint(d).state_dict()
    empty = tmp_path / "empty_dir"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        io.resolve_checkpoint(str(empty))
    with pytest.raises(FileNotFoundError):
        io.resolve_checkpoint(str(tmp_path / "nowhere"))


def test_a_hub_cache_snapshot_of_symlinks_resolves(io, saved, tmp_path):
    dirs, want = saved
    cache = tmp_path / "models--someone--tiny-vit"
    blobs, rev = cache / "blobs", cache / "snapshots" / "0123abcd"
    blobs.mkdir(parents=True)
    rev.mkdir(parents=True)
    for i, name in enumerate(sorted(os.listdir(dirs["sharded"]))):
        blob = blobs / ("%040x" % i)
        blob.write_bytes(open(os.path.join(dirs["sharded"], name), "rb").read())
        os.symlink(os.path.join("..", "..", "blobs", blob.name), str(rev / name))
    link = tmp_path / "link_to_rev"
    os.symlink(str(rev), str(link))
    for path in (str(rev), str(link)):
        snap = io.resolve_checkpoint(path)
        assert snap.config["model_type"] == "vit"
        _same(snap.state_dict(), want)
