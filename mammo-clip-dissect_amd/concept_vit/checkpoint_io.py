"""Checkpoints as they are distributed: a `.safetensors` file, or a Hugging Face snapshot directory (config.json beside
model.safetensors, a sharded model-0000k-of-0000n.safetensors set with its index, or the pytorch_model.bin forms).

read_safetensors / write_safetensors implement the format themselves (8 bytes little-endian header length, a JSON header
{name: {dtype, shape, data_offsets}}, raw little-endian data): nothing from a file is executed, and the `safetensors`
package is not imported.  resolve_checkpoint turns a path -- a file or a directory, symlinks followed -- into a Snapshot:
the state dict (read lazily, once), the parsed config.json (or None) and the directory.  Torch files are still read with
torch.load(weights_only=True)."""
import json
import math
import mmap
import os
import struct

import torch

MAX_HEADER_BYTES = 100 * 1000 * 1000
_DTYPES = {"F64": torch.float64, "F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16, "I64": torch.int64,
           "I32": torch.int32, "I16": torch.int16, "I8": torch.int8, "U8": torch.uint8, "BOOL": torch.bool}
_NAMES = {v: k for k, v in _DTYPES.items()}
# the order transformers' from_pretrained looks a directory up in
SNAPSHOT_FILES = ("model.safetensors", "model.safetensors.index.json", "pytorch_model.bin", "pytorch_model.bin.index.json")


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _parse_header(path, raw, data_len):
    """The validated entries [(name, dtype, shape, begin, end)] of a header's bytes; every defect is a ValueError."""
    def bad(what):
        return ValueError("%s: not a valid safetensors file: %s" % (path, what))
    try:
        header = json.loads(raw.decode("utf-8"))
    except (UnicodeDecodeError, ValueError) as e:
        raise bad("the header is not JSON (%s)" % e) from None
    if not isinstance(header, dict):
        raise bad("the header is not a JSON object but a %s" % type(header).__name__)
    entries = []
    for name, info in header.items():
        if name == "__metadata__":
            continue
        if not isinstance(info, dict):
            raise bad("the entry of %r is not an object" % name)
        dtype, shape, span = info.get("dtype"), info.get("shape"), info.get("data_offsets")
        if not isinstance(dtype, str) or dtype not in _DTYPES:
            raise bad("%r has the unknown dtype %r" % (name, dtype))
        if not isinstance(shape, list) or not all(_is_int(d) for d in shape):
            raise bad("the shape of %r, %r, is not a list of integers" % (name, shape))
        if any(d < 0 for d in shape):
            raise bad("%r has a negative dimension: %r" % (name, shape))
        if not isinstance(span, list) or len(span) != 2 or not all(_is_int(o) for o in span):
            raise bad("data_offsets of %r, %r, is not a pair of integers" % (name, span))
        begin, end = span
        if begin > end:
            raise bad("data_offsets of %r are reversed: %r" % (name, span))
        if begin < 0 or end > data_len:
            raise bad("data_offsets of %r, %r, lie outside the file's %d data bytes" % (name, span, data_len))
        want = math.prod(shape) * torch.empty((), dtype=_DTYPES[dtype]).element_size()
        if end - begin != want:
            raise bad("%r spans %d bytes, its shape %r of %s needs %d" % (name, end - begin, shape, dtype, want))
        entries.append((name, _DTYPES[dtype], tuple(shape), begin, end))
    last_name, last_end = None, 0
    for name, _, _, begin, end in sorted(entries, key=lambda e: (e[3], e[4])):
        if begin < last_end:
            raise bad("the data of %r and %r overlap" % (last_name, name))
        if end > begin:
            last_name, last_end = name, end
    return entries


def read_safetensors(path, device="cpu"):
    """{name: tensor} of a .safetensors file, every tensor a copy on `device` (nothing aliases the file).  F64, F32, F16,
    BF16, I64, I32, I16, I8, U8 and BOOL; 0-dim and empty tensors; __metadata__ is ignored.  A malformed file is a
    ValueError that names the file and the defect: a short tensor is never returned."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    if size < 8:
        raise ValueError("%s: not a valid safetensors file: %d bytes, shorter than the 8-byte header length" % (path, size))
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        if n > MAX_HEADER_BYTES:
            raise ValueError("%s: not a valid safetensors file: a header of %d bytes (the limit is %d)" % (path, n, MAX_HEADER_BYTES))
        if 8 + n > size:
            raise ValueError("%s: not a valid safetensors file: the header length %d reaches past the end of the file (%d bytes)"
                             % (path, n, size))
        entries = _parse_header(path, f.read(n), size - 8 - n)
        out = {}
        if not any(end > begin for _, _, _, begin, end in entries):
            return {name: torch.empty(shape, dtype=dtype, device=device) for name, dtype, shape, _, _ in entries}
        # a private copy-on-write mapping: torch.frombuffer wants a writable buffer, the file is never written
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY) as mm:
            for name, dtype, shape, begin, end in entries:
                if end == begin:
                    out[name] = torch.empty(shape, dtype=dtype, device=device)
                    continue
                # the bytes are copied out first (fresh, aligned storage), then reinterpreted: no alignment is asked of the file
                raw = torch.frombuffer(mm, dtype=torch.uint8, count=end - begin, offset=8 + n + begin).clone()
                out[name] = raw.view(dtype).reshape(shape).to(device)
                del raw
    return out


def write_safetensors(path, tensors):
    """The matching minimal writer: sorted names, contiguous little-endian data, {"format": "pt"} metadata, the header padded
    with spaces to a multiple of 8 bytes."""
    header, blobs, at = {"__metadata__": {"format": "pt"}}, [], 0
    for name in sorted(tensors):
        t = tensors[name]
        if not torch.is_tensor(t) or t.dtype not in _NAMES:
            raise ValueError("write_safetensors: %r is not a tensor of a supported dtype (%s)"
                             % (name, getattr(t, "dtype", type(t).__name__)))
        t = t.detach().cpu().contiguous()
        blob = t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""
        header[name] = {"dtype": _NAMES[t.dtype], "shape": list(t.shape), "data_offsets": [at, at + len(blob)]}
        blobs.append(blob)
        at += len(blob)
    raw = json.dumps(header, separators=(",", ":")).encode("utf-8")
    raw += b" " * (-len(raw) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(raw)))
        f.write(raw)
        for blob in blobs:
            f.write(blob)


def _read_weights(path):
    """One weights file: .safetensors by the reader above, anything else by torch.load(weights_only=True)."""
    if path.endswith(".safetensors"):
        return read_safetensors(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def _unique_pairs(index):
    def hook(pairs):
        seen = {}
        for k, v in pairs:
            if k in seen:
                raise ValueError("%s: the key %r is listed twice (in %r and in %r)" % (index, k, seen[k], v))
            seen[k] = v
        return seen
    return hook


def _read_index(index):
    """The merged state dict of an index file (model.safetensors.index.json / pytorch_model.bin.index.json)."""
    root = os.path.dirname(index)
    with open(index, "r", encoding="utf-8") as f:
        table = json.load(f, object_pairs_hook=_unique_pairs(index))
    weight_map = table.get("weight_map") if isinstance(table, dict) else None
    if not isinstance(weight_map, dict) or not weight_map:
        raise ValueError("%s: no 'weight_map' object {tensor name: shard file}" % index)
    shards = []
    for key, shard in weight_map.items():
        if not isinstance(shard, str) or shard in ("", ".", "..") or "/" in shard or "\\" in shard or os.sep in shard:
            raise ValueError("%s: the shard %r of %r is not a plain file name inside the directory" % (index, shard, key))
        if shard not in shards:
            shards.append(shard)
    for shard in shards:
        if not os.path.isfile(os.path.join(root, shard)):
            raise FileNotFoundError("%s names the shard %r, which is not in %s" % (index, shard, root))
    out, origin = {}, {}
    for shard in shards:
        part = _read_weights(os.path.join(root, shard))
        if not isinstance(part, dict):
            raise ValueError("%s: the shard %r does not hold a state dict" % (index, shard))
        for key, value in part.items():
            if key in out:
                raise ValueError("%s: the key %r is in two shards, %r and %r" % (index, key, origin[key], shard))
            out[key], origin[key] = value, shard
    for key, shard in weight_map.items():
        if origin.get(key) != shard:
            raise ValueError("%s: the key %r is not in the shard %r that should hold it%s"
                             % (index, key, shard, "" if key not in origin else " but in %r" % origin[key]))
    return {key: out[key] for key in weight_map} | {k: v for k, v in out.items() if k not in weight_map}


class Snapshot:
    """A resolved checkpoint: `root` (the directory), `weights` (the file or index the tensors come from), `config` (the
    parsed config.json, or None) and state_dict(), which reads the weights on its first call and keeps them."""

    def __init__(self, root, weights, config=None):
        self.root, self.weights, self.config = root, weights, config
        self._loaded = None

    def state_dict(self):
        if self._loaded is None:
            self._loaded = (_read_index(self.weights) if self.weights.endswith(".index.json") else _read_weights(self.weights),)
        return self._loaded[0]

    def __repr__(self):
        return "Snapshot(%r, config=%s)" % (self.weights, "None" if self.config is None else "{...}")


def _read_config(root):
    path = os.path.join(root, "config.json")
    if not os.path.isfile(path):
        return None
    with open(path, "r", encoding="utf-8") as f:
        config = json.load(f)
    if not isinstance(config, dict):
        raise ValueError("%s: config.json must hold one JSON object" % path)
    return config


def is_snapshot_path(path):
    """Whether `path` is a form that carries a config.json with it: a directory, a .safetensors file or an index file."""
    return isinstance(path, str) and (os.path.isdir(path) or path.endswith((".safetensors", ".index.json")))


def resolve_checkpoint(path):
    """The Snapshot of a file or a directory (symlinks are followed: a hub cache's snapshots/<rev>/ is a directory of
    links).  A directory is looked up as from_pretrained does: model.safetensors, model.safetensors.index.json,
    pytorch_model.bin, pytorch_model.bin.index.json; one holding none of them is a FileNotFoundError.  A .safetensors
    file or an index file takes the config.json of its directory when there is one; any other file is a torch file, read
    with weights_only=True, and carries no configuration (as before)."""
    path = os.fspath(path)
    if os.path.isdir(path):
        for name in SNAPSHOT_FILES:
            if os.path.isfile(os.path.join(path, name)):
                return Snapshot(path, os.path.join(path, name), _read_config(path))
        raise FileNotFoundError("%s: a directory without a checkpoint (looked for %s)" % (path, ", ".join(SNAPSHOT_FILES)))
    if not os.path.isfile(path):
        raise FileNotFoundError("%s: no such checkpoint file or directory" % path)
    root = os.path.dirname(os.path.abspath(path))
    return Snapshot(root, path, _read_config(root) if is_snapshot_path(path) else None)
