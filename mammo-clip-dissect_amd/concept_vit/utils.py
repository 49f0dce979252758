"""Mirror of the reference's concept_vit/utils.py (Mammo-CLIP dissector orchestration) for the hot path.

Kept names and contracts (reference concept_vit/utils.py):
    get_activation(outputs, mode)                                   :27-52
    get_save_names(clip_name, target_name, target_layer, d_probe, concept_set, pool_mode, save_dir)  :54-62
    save_activations(clip_name, target_name, target_layers, d_probe, concept_set, batch_size, device,
                     pool_mode, save_dir, breast_clip_ckh=None, fine_tuned_ckh=None, args=None)       :430-564
    get_similarity_from_activations(target_save_name, clip_save_name, text_save_name, similarity_fn,
                                    return_target_feats=True, device="cuda", d_probe="vindr", top_k=100)  :566-612
    get_clip_feats(clip_save_name, text_save_name, device="cuda", d_probe="vindr")                    :670-702
    _all_saved / _make_save_dir                                                                       :648-668
    get_cos_similarity(preds, gt, clip_model, mpnet_model, device="cuda", batch_size=200)             :618-646

What differs, deliberately:
  * models and probe data come from the offline factory (data_utils): nothing is downloaded;
  * hooks pool with the K0 HIP kernel straight into ONE activation matrix (no list + torch.cat), and
    when the target IS the dissector the images are encoded once, not twice (reference :550-552);
  * the per-layer P = I_hat @ T_hat^T of get_similarity_from_activations is computed by the HIP GEMM and
    cached for the run (the reference recomputes it for each of the 12-39 layers);
  * failures raise (the reference swallows them with `except Exception: print`, :336-337).
The activation-cache files keep the reference's names and format: torch.save of float32 tensors
[N, U_layer] / [N, 512] / [C, 512], so caches are interchangeable.
"""
import os
import re
import threading

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import core
from ..pipeline import Dissector
from . import data_utils

PM_SUFFIX = {"max": "_max", "avg": ""}
_P_CACHE = {}


# ---- hooks (reference :27-52) ---------------------------------------------------------------------
def get_activation(outputs, mode):
    '''
    mode: how to pool activations: one of avg, max
    for fc or ViT neurons does no pooling
    (same semantics as the reference; the pooling itself is the K0 HIP kernel)
    '''
    if mode not in ("avg", "max"):
        raise ValueError("pool mode must be 'avg' or 'max'")

    def hook(model, input, output):
        if mode == 'avg' and type(output) is tuple:   # the reference unwraps tuples only in 'avg' mode
            output = output[0]
        out = output.detach()
        if out.dim() not in (2, 3, 4):
            return
        width = out.shape[1] if out.dim() in (2, 4) else out.shape[2]
        dst = torch.empty((out.shape[0], width), dtype=torch.float32, device=out.device)
        core.hook_pool(out, mode, dst, 0, 0, False)
        outputs.append(dst)
    hook.token0_only = True   # of a 3-D output only token 0 is read: see data_utils.cls_tail_route
    return hook


def get_save_names(clip_name, target_name, target_layer, d_probe, concept_set, pool_mode, save_dir):
    """The three cache-file names of a (dissector, target, layer, probe set, concept set) combination.  The format
    strings ARE the contract (reference utils.py:54-62): caches written by either implementation must be found by the
    other."""
    target_save_name = "{}/{}_{}_{}{}.pt".format(save_dir, d_probe, target_name, target_layer,
                                                 PM_SUFFIX[pool_mode])
    clip_save_name = "{}/{}_{}.pt".format(save_dir, d_probe, clip_name.replace('/', ''))
    concept_set_name = (concept_set.split("/")[-1]).split(".")[0]
    text_save_name = "{}/{}_{}.pt".format(save_dir, concept_set_name, clip_name.replace('/', ''))
    return target_save_name, clip_save_name, text_save_name


def save_prefix(d_probe, breast_clip_ckh=None, fine_tuned_ckh=None):
    """The prefix the reference's writer puts in front of the save names (:456-468)."""
    if breast_clip_ckh is not None:
        if fine_tuned_ckh is not None:
            return "/newest_{}_cancer_finetuned_".format(d_probe)
        return "/latest_{}_mammo_pretrained_".format(d_probe)
    return "/Latest_{}_not_mammo_pretrained_".format(d_probe)


def resolve_layer(model, name):
    """'image_encoder._blocks[3]' -> the module (the reference evals the string, :135-136)."""
    obj = model
    for part in re.findall(r"[A-Za-z_][A-Za-z_0-9]*|\[\d+\]", name.strip()):
        obj = obj[int(part[1:-1])] if part.startswith("[") else getattr(obj, part)
    return obj


def _all_saved(save_names):
    """True when every cache file named in the {layer: path} dict is already on disk -- the reference's test for skipping
    the target-model pass (utils.py:648-657)."""
    return all(os.path.exists(path) for path in save_names.values())


def _make_save_dir(save_name):
    """Create the directory part of a cache-file path if it is missing (utils.py:659-668)."""
    save_dir = os.path.dirname(save_name)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)


def _read_concepts(concept_set):
    with open(concept_set, 'r') as f:
        words = (f.read()).split('\n')
    return [i for i in words if i != ""]   # reference :495-498


def _layer_widths(model, layers, sample, forward):
    """Neurons a hook on each of `layers` yields: ONE tiny forward with a probe on every layer, cached on the model
    (the widths are a property of the architecture)."""
    cache = model.__dict__.setdefault("_mcd_layer_widths", {})
    missing = [m for m in layers if id(m) not in cache]
    if missing:
        got = {}
        hs = [m.register_forward_hook(lambda mod, i, o, k=id(m): got.__setitem__(k, o[0] if type(o) is tuple else o))
              for m in missing]
        with torch.no_grad():
            forward(sample)
        for h in hs:
            h.remove()
        for m in missing:
            o = got[id(m)]
            cache[id(m)] = int(o.shape[1] if o.dim() in (2, 4) else o.shape[2])
    return [cache[id(m)] for m in layers]


class Extraction:
    """What one extraction pass leaves resident in HBM: the Dissector (activation matrix of all target layers + the
    dissector's image embeddings) and the text embeddings.  The drivers score it in ONE fused pass
    (Dissector.finish) instead of re-loading the cache files layer by layer; the cache files are still written, by a
    background thread, as the reference's side output."""

    def __init__(self, dis, E_txt, target_layers, writer=None, stream=None):
        self.dis, self.E_txt, self.target_layers, self.writer = dis, E_txt, list(target_layers), writer
        self.stream = stream      # CacheStream: the files were streamed out during the pass, only their finalisation is left

    def start_writer(self):
        """Start the cache-file writer (idempotent).  The drivers call it once the scoring kernels are queued, so the
        writer's device -> host copies run beside the CSV writing on the host, not beside the scoring kernels.
        Nothing to start on the streaming route."""
        if self.writer is not None and not self.writer.is_alive() and not self.writer.started:
            self.writer.begin()

    def wait(self):
        if self.stream is not None:
            stream, self.stream = self.stream, None
            stream.close()        # raises the first error of the pass's copies, appends and finalisations
        if self.writer is not None:
            self.start_writer()
            self.writer.join()
            if self.writer.error is not None:
                raise self.writer.error
            self.writer = None


# ---- the streaming route of the cache files (include/mcd_cache.h) --------------------------------------------------
CACHE_STREAM_SLOTS = 8     # pinned slots of the ring (one holds a batch of one layer); tests shrink it to meet the back-pressure


def _placeholder_archive(part_path, n_rows, width):
    """torch.save of an UNINITIALISED float32 [n_rows, width] tensor as `part_path`: the complete archive of the cache file,
    with placeholder bytes where the rows will go.  Returns (data offset, CRC field offset a, CRC field offset b) of the
    tensor's record, read back from the zip structures: the central-directory entry's CRC-32, and the local header's or -- when
    the writer set general-purpose bit 3, as torch's does -- the data descriptor's behind the data.  (The archive's
    .data/serialization_id record is a hash that torch derives from the record names and CRCs at save time; it stays the
    placeholder's.  Nothing reads it back.)"""
    import struct
    import zipfile
    torch.save(torch.empty((n_rows, width), dtype=torch.float32), part_path)
    nbytes = n_rows * width * 4
    with zipfile.ZipFile(part_path) as z:
        recs = [i for i in z.infolist() if i.filename.endswith("/data/0")]
        start_dir = z.start_dir
    with open(part_path, "rb") as f:
        def at(off, n):
            f.seek(off)
            return f.read(n)
        ok = len(recs) == 1 and recs[0].compress_type == zipfile.ZIP_STORED and recs[0].file_size == nbytes
        if ok:
            zi = recs[0]
            head = at(zi.header_offset, 30)
            ok = head[:4] == b"PK\x03\x04"
        if ok:
            n_name, n_extra = struct.unpack("<HH", head[26:30])
            data_off = zi.header_offset + 30 + n_name + n_extra
            if zi.flag_bits & 0x8:
                crc_b = data_off + nbytes + (4 if at(data_off + nbytes, 4) == b"PK\x07\x08" else 0)
            else:
                crc_b = zi.header_offset + 14
            crc_a, pos = None, start_dir
            while crc_a is None:
                ent = at(pos, 46)
                if len(ent) < 46 or ent[:4] != b"PK\x01\x02":
                    break
                n_name, n_extra, n_comment = struct.unpack("<HHH", ent[28:34])
                if at(pos + 46, n_name) == zi.orig_filename.encode("utf-8"):
                    crc_a = pos + 16
                pos += 46 + n_name + n_extra + n_comment
            want = struct.pack("<I", zi.CRC)
            ok = crc_a is not None and at(crc_a, 4) == want and at(crc_b, 4) == want
    if not ok:
        os.unlink(part_path)
        raise RuntimeError("torch.save wrote an archive whose tensor record was not found where the zip format puts it: %s "
                           "(MCD_CACHE_STREAM=0 writes the cache files without the streaming route)" % part_path)
    return data_off, crc_a, crc_b


class CacheStream:
    """The cache files of one extraction pass, written while it runs: every (batch, layer) block leaves the device as soon as
    its K0 hook has run and a native worker thread appends it to the layer's file (mcd_cache_stream_*, libmcd_hip.so, with the
    container of libmcd_host.so); close() only waits for the last blocks and finalises.  Files are `<name>.part` until they are
    complete.
    The archives themselves are laid out by torch.save (_placeholder_archive), once the first batch's kernels are queued, so
    that the host time of it lies behind that batch's GPU time: the pushes of the first batch wait in `pending` until begin()."""

    def __init__(self, device, n_rows, files, batch_rows, slots=None):
        """files: [(path, width)], pushed to by index.  batch_rows: the largest number of rows of one push."""
        d = torch.device(device)
        self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        self.n_rows, self.files = int(n_rows), list(files)
        self.slots = int(slots if slots is not None else CACHE_STREAM_SLOTS)
        self.slot_bytes = max(4, int(batch_rows) * max(w for _, w in self.files) * 4)
        self.handle, self.pending, self.closed, self.keep = None, [], False, {}
        self.L, self.H = core._lib.load(), core._lib.load_cache_host()

    def begin(self):
        if self.handle is not None or self.closed:
            return
        import ctypes
        H, n = self.H, len(self.files)
        handles = (ctypes.c_void_p * n)()
        try:
            for i, (path, width) in enumerate(self.files):
                part = path + ".part"
                data_off, crc_a, crc_b = _placeholder_archive(part, self.n_rows, width)
                h = ctypes.c_void_p()
                if H.mcd_cachefile_open(os.fsencode(part), os.fsencode(path), self.n_rows, width, data_off, crc_a, crc_b,
                                        ctypes.byref(h)) != 0:
                    raise OSError(H.mcd_cachefile_last_error().decode("utf-8", "replace"))
                handles[i] = h
        except BaseException:
            self.closed = True
            for h in handles:
                if h:
                    H.mcd_cachefile_abort(h)
            raise
        widths = (ctypes.c_int64 * n)(*[w for _, w in self.files])
        io = core._lib.cache_io(H)
        out = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.L.mcd_cache_stream_open(n, handles, widths, ctypes.byref(io), self.slots, self.slot_bytes, ctypes.byref(out))
        if rc != 0:            # (the native side has removed the .part files)
            self.closed = True
            core.check(rc)
        self.handle = out
        # The first batch's blocks: each is ready at the event its hook recorded, not only now that the whole batch is queued.
        # A side stream that waits for that event stands in for the launch stream, so the copies of the early layers start at
        # once and their slots come back while the GPU is still inside the batch (pushed from the launch stream, all of them
        # would wait for the end of the batch and the launch thread would sit in the back-pressure until then).
        pending, self.pending = self.pending, []
        if pending:
            with torch.cuda.device(self.device):
                self._side = torch.cuda.Stream(device=self.device)
                for file, block, row0, n, ready in pending:
                    self._side.wait_event(ready)
                    with torch.cuda.stream(self._side):
                        self.push(file, block, row0, n)

    def reserve(self, file):
        """Before the kernel that rewrites the staging block of `file`: the current stream waits until the copy of the block's
        previous content has been taken."""
        if self.handle is not None:
            with torch.cuda.device(self.device):
                core.check(self.L.mcd_cache_stream_reserve(self.handle, file, core._stream()))

    def push(self, file, block, row0, n):
        """`block`: contiguous float32 device rows [>= n, width of the file], final once the current stream's queued work has run."""
        if self.closed:
            raise RuntimeError("CacheStream is closed")
        if block.dtype != torch.float32 or not block.is_contiguous() or block.dim() != 2 or block.shape[0] < n \
                or block.shape[1] != self.files[file][1] or block.device != self.device:
            raise TypeError("CacheStream.push: block must be contiguous float32 [>= %d, %d] on %s" % (n, self.files[file][1], self.device))
        if self.handle is None:
            with torch.cuda.device(self.device):
                ready = torch.cuda.Event()
                ready.record()
            self.pending.append((file, block, row0, n, ready))
            return
        # the copy stream reads the block behind torch's back: it stays referenced (not handed back to the caching allocator)
        # until close() or abort() has drained the copies
        self.keep[file] = block
        with torch.cuda.device(self.device):
            core.check(self.L.mcd_cache_stream_push(self.handle, file, block.data_ptr(), int(row0), int(n), core._stream()))

    def _end(self, entry):
        if self.closed:
            return
        self.closed = True
        self.pending = []
        if self.handle is not None:
            handle, self.handle = self.handle, None
            try:
                core.check(entry(handle))
            finally:
                self.keep = {}

    def close(self):
        """Wait for the last blocks, finalise every file and rename it into place; raises the first error."""
        if not self.closed and self.handle is None:
            self.begin()          # a pass of no complete batch: the native close then reports the missing rows
        self._end(self.L.mcd_cache_stream_close)

    def abort(self):
        """Drop the pass: no file appears under its final name."""
        try:
            self._end(self.L.mcd_cache_stream_abort)
        except core._lib.McdError:
            pass

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class _CacheWriter(threading.Thread):
    """torch.save of the reference-format cache files ([N, U_layer] per layer, [N, 512] image embeddings) off the main
    thread, while the main thread scores and writes the CSV: device -> PINNED host copies on a stream of its own (370 MB
    at config 2: 7 ms pinned against 100 ms pageable), then the file writes on two threads (torch.save releases the GIL
    for part of its work: 96 ms serial, 46 ms on two threads, no better on more)."""

    def __init__(self, device, jobs):
        super().__init__(daemon=True)
        self.device, self.jobs, self.error, self.started = device, jobs, None, False
        self.ready = None

    def begin(self):
        self.started = True
        if torch.device(self.device).type == "cuda":
            with torch.cuda.device(self.device):
                self.ready = torch.cuda.Event()
                self.ready.record()           # everything queued so far (extraction, scoring) precedes the copies
        self.start()

    def _save_some(self, items):
        try:
            for t, path in items:
                torch.save(t, path)
        except Exception as e:
            self.error = e

    def run(self):
        try:
            staged = []
            if self.ready is not None:
                with torch.cuda.device(self.device):
                    side = torch.cuda.Stream(device=self.device)
                    side.wait_event(self.ready)
                    with torch.cuda.stream(side):
                        for make, path in self.jobs:
                            src = make()
                            dst = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
                            dst.copy_(src, non_blocking=True)
                            staged.append((dst, path))
                    side.synchronize()
            else:
                staged = [(make().cpu(), path) for make, path in self.jobs]
            helper = threading.Thread(target=self._save_some, args=(staged[1::2],), daemon=True)
            helper.start()
            self._save_some(staged[0::2])
            helper.join()
        except Exception as e:   # surfaced by Extraction.wait(): a failed save must not pass silently (reference :336-337 does)
            self.error = e


def _dist_info():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def extract_and_save(clip_model, target_model, encode_target, target_layers, dataset, words, tokenize, batch_size,
                     device, pool_mode, target_tmpl, clip_save_name, text_save_name, write_caches=None, gather=None):
    """Shared body of the three save_activations variants: one pass over D_probe with the K0 hooks writing the
    activation matrix, dissector image/text embeddings, then the reference-format cache files.
    Returns an Extraction (everything still resident on the device) when the pass ran, None when every cache file
    already existed (reference: skip, utils.py:128,162,318).
    Multi-rank (torch.distributed initialised): `dataset` is this rank's shard; the cache files are a single-process
    feature and are not written."""
    world, rank = _dist_info()
    if write_caches is None:
        write_caches = world == 1 and os.environ.get("MCD_ACTIVATION_CACHE", "1") != "0"
    layer_files = {l: target_tmpl.format(l) for l in target_layers}
    need_target = not _all_saved(layer_files) or world > 1
    need_clip = not os.path.exists(clip_save_name) or world > 1
    need_text = not os.path.exists(text_save_name) or world > 1
    if write_caches:
        for n in list(layer_files.values()) + [clip_save_name, text_save_name]:
            _make_save_dir(n)

    with torch.no_grad():
        E_txt = None
        if need_text:   # reference :390-414
            tok = tokenize(["{}".format(word) for word in words])
            tok = {k: v.to(device) for k, v in tok.items()} if isinstance(tok, dict) else tok.to(device)
            feats = []
            keys = list(tok.keys()) if isinstance(tok, dict) else None
            n_txt = tok[keys[0]].shape[0] if keys else tok.shape[0]
            for i in range(0, n_txt, batch_size):
                chunk = {k: v[i:i + batch_size] for k, v in tok.items()} if keys else tok[i:i + batch_size]
                t = clip_model.encode_text(chunk)
                if getattr(clip_model, "projection", False):
                    t = clip_model.text_projection(t)
                feats.append(t.float())
            E_txt = torch.cat(feats)
            if write_caches:
                torch.save(E_txt.cpu(), text_save_name)
        if not (need_target or need_clip):
            return None
        if E_txt is None:
            E_txt = _load_feats(text_save_name, device)
        N = len(dataset)
        on_device = hasattr(dataset, "device_batches") and getattr(dataset, "device", None) is not None
        if on_device:
            batches = dataset.device_batches(batch_size)
            first = (dataset.sample() if hasattr(dataset, "sample") else dataset.images()[:1]) if N > 0 else None
        else:
            batches = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=0)
            first = _views(dataset[0][0])[0].unsqueeze(0).to(device) if N > 0 else None
        if first is None:   # a rank without images still needs the layer widths
            first = torch.zeros((1, 3, 224, 224), dtype=torch.float32, device=device)
        layers = [resolve_layer(target_model, l) for l in target_layers]
        widths = _layer_widths(target_model, layers, first, encode_target)
        same = target_model is clip_model
        # the embedding width is the text features' (512 for the ViT-shaped dissectors, 1024 for CLIP RN50)
        dis = Dissector(N, list(target_layers), widths, len(words), E_txt.shape[1], device,
                        pool_mode=pool_mode, gather=gather)
        handles = [m.register_forward_hook(dis.hook(i)) for i, m in enumerate(layers)] if need_target else []
        # the streaming route of the cache files: a GPU pass that computes the activations, with the native container built.
        # Everything else -- a non-GPU device, activations loaded from existing files, no libmcd_host.so, MCD_CACHE_STREAM=0
        # (the A/B knob) -- keeps the writer thread below.
        stream = None
        if write_caches and need_target and N > 0 and torch.device(device).type == "cuda" \
                and os.environ.get("MCD_CACHE_STREAM", "1") != "0" and core._lib.load_cache_host() is not None:
            files = [(layer_files[l], w) for l, w in zip(target_layers, widths)]
            if need_clip:
                files.append((clip_save_name, int(E_txt.shape[1])))
            stream = CacheStream(dis.device, N, files, batch_size)
            dis.attach_cache_stream(stream, batch_size, image_file=len(files) - 1 if need_clip else None)
        try:
            for batch in batches:
                if not on_device:
                    batch = batch[0] if isinstance(batch, (list, tuple)) else batch["images"]
                # one view, or the pair (target view, dissector view) of a probe set with two transforms
                target_view, clip_view = _views(batch)
                images = target_view.to(device)
                clip_images = images if clip_view is target_view else clip_view.to(device)
                if need_target:
                    out = encode_target(images)                    # hooks fire (reference :174-181)
                if need_clip:
                    if same and need_target and clip_images is images:
                        f = out                                    # one pass when the target is the dissector
                    else:
                        f = clip_model.encode_image(clip_images)
                    if getattr(clip_model, "projection", False):
                        f = clip_model.image_projection(f)
                    dis.add_image_features(f.float())
                dis.advance(images.shape[0])
        except BaseException:
            if stream is not None:
                stream.abort()       # no half-written file is left under a name a later run would take for a cache
            raise
        finally:
            for h in handles:
                h.remove()
            dis.cache_stream = None
        if not need_clip:
            dis.E_img.copy_(_load_feats(clip_save_name, device))
        if not need_target:   # the layers' cache files exist, the dissector embeddings did not: load the activations
            for i, l in enumerate(target_layers):
                A = torch.load(layer_files[l], map_location='cpu', weights_only=True).float().to(device)
                core.transpose(A, out=dis.At[dis.offsets[i]:dis.offsets[i + 1], :N])
        writer = None
        if stream is not None:
            return Extraction(dis, E_txt, target_layers, stream=stream)
        if write_caches:
            jobs = []
            if need_clip:
                jobs.append((lambda: dis.E_img, clip_save_name))
            if need_target:   # cache format: [N, U_layer] float32 (reference :188-196)
                for i, l in enumerate(target_layers):
                    jobs.append((lambda i=i: dis.At[dis.offsets[i]:dis.offsets[i + 1], :N].t(), layer_files[l]))
            writer = _CacheWriter(device, jobs)
        return Extraction(dis, E_txt, target_layers, writer)


def _views(batch):
    """(target view, dissector view) of a batch or an item: a probe set with two transforms yields pairs, every other
    one a single tensor that serves both."""
    if isinstance(batch, (list, tuple)):
        target, clip = batch
        return target, clip
    return batch, batch


def _probe_data(d_probe, device, preprocess=None, clip_preprocess=None):
    """D_probe for the extraction loop: generated (synthetic sets) or preprocessed (file sets, K22) on the device when
    `device` is a GPU (this rank's shard of it in a multi-rank run); MCD_PROBE_ON_HOST=1 keeps the host dataset +
    DataLoader path.  preprocess / clip_preprocess: the target's and the dissector's transform of a file set
    (data_utils.get_data); synthetic sets ignore them."""
    from ..pipeline import shard_bounds
    world, rank = _dist_info()
    n = len(data_utils.get_data(d_probe, None))
    lo, hi = shard_bounds(n, world, rank)
    on_host = os.environ.get("MCD_PROBE_ON_HOST", "0") == "1"
    return data_utils.get_data(d_probe, preprocess, None if on_host else device, lo, hi, clip_preprocess=clip_preprocess)


def build_mammo_models(target_name, device, breast_clip_ckh=None, fine_tuned_ckh=None, args=None, text_tower=None):
    """The model side of save_activations (reference :443-483): (dissector, target).  Separate so that a caller that
    dissects repeatedly (bench.py) builds the models once.  text_tower: the dissector's text tower, passed to
    data_utils.get_target_model (None: the BERT tower exactly when the checkpoint carries one)."""
    finetuned = fine_tuned_ckh
    tower = "vit" if target_name.startswith("breastclip_vit") else "swin" if target_name == "breastclip_swin" else "cnn"
    clip_model, _ = data_utils.get_target_model(target_name if tower != "cnn" else "breastclip", device,
                                                ckpt=breast_clip_ckh, text_tower=text_tower)
    if (target_name == "breastclip" or tower != "cnn") and finetuned is None:
        target_model = clip_model          # same weights: encode the probe set once
    elif target_name == "breastclip_classifier":
        target_model, _ = data_utils.get_target_model(target_name, device, args=args, ckpt=breast_clip_ckh,
                                                      n_class=getattr(args, "num_class", 1), finetuned_ckpt=finetuned)
    else:       # a checkpoint registered for the target (data_utils.register_target_checkpoint) takes the Mammo-CLIP file's place
        target_model, _ = data_utils.get_target_model(target_name, device,
                                                      ckpt=data_utils.target_ckpt_or(target_name, breast_clip_ckh))
    return clip_model, target_model


def save_activations(clip_name, target_name, target_layers, d_probe,
                     concept_set, batch_size, device, pool_mode, save_dir, breast_clip_ckh=None, fine_tuned_ckh=None,
                     args=None, prebuilt=None):
    """Mammo-CLIP dissector + target (reference :430-564).  Dissector = BreastClip; the target is built by
    data_utils.get_target_model.  `clip_name` only names files, as in the reference.
    prebuilt: optional dict(clip_model=, target_model=, data=) from an earlier call (models and the resident probe set
    are then reused).  Returns the Extraction (None when every cache file existed)."""
    if prebuilt is not None:
        clip_model, target_model, data = prebuilt["clip_model"], prebuilt["target_model"], prebuilt["data"]
    else:
        clip_model, target_model = build_mammo_models(target_name, device, breast_clip_ckh, fine_tuned_ckh, args)
        # reference :472-490: the dissector gets the set's own transform (clip_preprocess = None), the target its own
        data = _probe_data(d_probe, device, data_utils.target_preset(target_name), "default")
    words = _read_concepts(concept_set)
    t_name, c_name, x_name = get_save_names(clip_name=clip_name, target_name=target_name, target_layer='{}',
                                            d_probe=d_probe, concept_set=concept_set, pool_mode=pool_mode,
                                            save_dir=save_dir)
    pre = save_dir + save_prefix(d_probe, breast_clip_ckh, fine_tuned_ckh)   # reference :508-516
    return extract_and_save(clip_model, target_model, target_model.encode_image, target_layers, data, words,
                            clip_model.tokenize, batch_size, device, pool_mode, pre + t_name, pre + c_name, pre + x_name,
                            gather=(prebuilt or {}).get("gather"))


def _load_feats(path, device):
    return torch.load(path, map_location='cpu', weights_only=True).float().to(device)


def get_clip_feats(clip_save_name, text_save_name, device="cuda", d_probe="vindr"):
    """P = I_hat @ T_hat^T from the cached embeddings (reference :670-702), on the GPU, cached per run."""
    key = (os.path.abspath(clip_save_name), os.path.abspath(text_save_name), str(device),
           os.path.getmtime(clip_save_name), os.path.getmtime(text_save_name))
    if key not in _P_CACHE:
        _P_CACHE.clear()
        with torch.no_grad():
            image_features = _load_feats(clip_save_name, device)
            text_features = _load_feats(text_save_name, device)
            image_features = core.normalize_rows(image_features.contiguous())   # :577
            text_features = core.normalize_rows(text_features.contiguous())     # :578
            _P_CACHE[key] = core.embed_gemm(image_features, text_features)   # :594
    return _P_CACHE[key]


def get_similarity_from_activations(target_save_name, clip_save_name, text_save_name, similarity_fn,
                                    return_target_feats=True, device="cuda", d_probe="vindr", top_k=100):
    clip_feats = get_clip_feats(clip_save_name, text_save_name, device=device, d_probe=d_probe)
    target_feats = torch.load(target_save_name, map_location='cpu', weights_only=True).to(device)
    similarity = similarity_fn(clip_feats, target_feats, device=device, top_k=top_k)   # reference :602
    if return_target_feats:
        return similarity, target_feats
    return similarity


def _unit_text_rows(clip_model, tokenizer, strings, context, device, batch_size):
    """[n, embed_dim]: clip_model.encode_text of `strings`, batch_size rows a call, every row divided by its L2 norm."""
    ids = tokenizer(strings, context_length=context).to(device)
    with torch.no_grad():
        rows = torch.cat([clip_model.encode_text(chunk) for chunk in ids.split(batch_size)])
    return rows / rows.norm(dim=-1, keepdim=True)


def get_cos_similarity(preds, gt, clip_model, mpnet_model, device="cuda", batch_size=200):
    """reference :618-646: the mean cosine between predicted and ground-truth concept strings (two lists of one length) in
    CLIP text space and in sentence space, as two Python floats.  clip_model: anything with encode_text (OpenAIClip: K9A,
    K25); the ids come from the registered CLIP merges file at the model's context length (data_utils.clip_tokenizer --
    without one an error that names register_tokenizer('clip', ...), never the hashing tokenizer), and a string over that
    length is an error, as in clip.tokenize.  mpnet_model: anything with SentenceTransformer's encode
    (data_utils.sentence_encoder: K9B, K27), which returns unit rows.  The row norms and the row-wise dot products are
    torch's and numpy's: n x 512 numbers."""
    preds, gt = list(preds), list(gt)
    if len(preds) != len(gt):
        raise ValueError("get_cos_similarity: %d predictions for %d ground-truth strings" % (len(preds), len(gt)))
    tokenizer = data_utils.clip_tokenizer()
    context = getattr(clip_model, "context_length", 77)
    in_clip = (_unit_text_rows(clip_model, tokenizer, preds, context, device, batch_size)
               * _unit_text_rows(clip_model, tokenizer, gt, context, device, batch_size)).sum(dim=1).mean()
    in_mpnet = (np.asarray(mpnet_model.encode(preds)) * np.asarray(mpnet_model.encode(gt))).sum(axis=1).mean()
    return float(in_clip), float(in_mpnet)
