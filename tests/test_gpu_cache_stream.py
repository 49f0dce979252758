"""GPU: the activation-cache streaming route (include/mcd_cache.h).

  * K0 with two stores (mcd_hook_pool_rows) against mcd_hook_pool: the activation-matrix part on the bits, the rows block on the
    bits of the transposed slab, on every path of the two kernels (copy kernel: token 0 of a 3-D input, a 2-D input; plane kernel:
    avg and max, scalar and float4 loads, a NaN plane, more planes than one block holds), at row0 = col0 = 0 and at row0, col0 > 0,
    neuron-major and image-major, with a rows block wider and longer than the data (the surplus must stay untouched);
  * the stream and capture contracts of mcd_hook_pool_rows with test_gpu_stream_contracts' machinery, and the stream contract of
    the writer: push takes the block as the work queued on ITS stream leaves it, reserve orders a rewrite of the block behind the
    copy, and nothing of it waits for the NULL stream;
  * end to end: describe_broad_neurons.main on synthetic_37_224 at batch 16 (batches of 16, 16 and 5) with the streaming route,
    with MCD_CACHE_STREAM=0, and with a ring of two pinned slots (every batch's four pushes meet the back-pressure): all cache
    files load to bit-equal tensors, the CSV bytes are equal."""
import ctypes
import glob
import os
import zipfile

import pytest
import torch

import test_gpu_stream_contracts as S
import util
from util import OUT_FILL, int_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
AVG, MAX, CLS, NONE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def L(mcd, dev):
    return mcd._lib.load()


@pytest.fixture(scope="module")
def utils(mcd):
    from mammo_clip_dissect_amd.concept_vit import utils
    return utils


# ---- K0 with two stores ------------------------------------------------------------------------------------------------
# (name, input shape, mode, B, Cout, HW): the issue's shapes; 4-D inputs at 3 images x 5 channels = 15 planes, four blocks of
# four waves with one wave idle
K0_CASES = [("cls", (3, 2, 5), CLS, 3, 5, 2), ("2d", (2, 7), NONE, 2, 7, 1),
            ("avg-hw6", (3, 5, 2, 3), AVG, 3, 5, 6), ("max-hw6", (3, 5, 2, 3), MAX, 3, 5, 6),
            ("avg-hw8", (3, 5, 2, 4), AVG, 3, 5, 8), ("max-hw8", (3, 5, 2, 4), MAX, 3, 5, 8)]


def k0_input(shape, dev):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(len(shape) * 100 + shape[-1]))
    if len(shape) == 4:
        x[1, 2, 0, 1] = float("nan")          # one NaN plane: image 1, channel 2
        x[2, 0] = -x[2, 0].abs()              # an all-negative plane (max must not start from 0)
    else:
        x.view(-1)[3] = float("nan")
        x.view(-1)[4] = -0.0
    return x.to(dev)


@pytest.mark.parametrize("neuron_major", [True, False], ids=["neuron-major", "image-major"])
@pytest.mark.parametrize("row0,col0", [(0, 0), (2, 3)])
@pytest.mark.parametrize("case", K0_CASES, ids=[c[0] for c in K0_CASES])
def test_dual_write_equals_hook_pool(L, dev, case, row0, col0, neuron_major):
    _, shape, mode, B, Cout, HW = case
    x = k0_input(shape, dev)
    n_img, n_neu = row0 + B + 1, col0 + Cout + 2            # the matrix is larger than the block on every side
    dims = (n_neu, n_img + 3) if neuron_major else (n_img, n_neu + 3)
    sn, su = (1, dims[1]) if neuron_major else (dims[1], 1)
    a0 = torch.full(dims, OUT_FILL, device=dev)
    a1 = torch.full(dims, OUT_FILL, device=dev)
    width = Cout + 2
    rows = torch.full((B + 1, width), OUT_FILL, device=dev)
    assert L.mcd_hook_pool(x.data_ptr(), B, Cout, HW, mode, a0.data_ptr(), row0, col0, sn, su, None) == 0
    assert L.mcd_hook_pool_rows(x.data_ptr(), B, Cout, HW, mode, a1.data_ptr(), row0, col0, sn, su, rows.data_ptr(), width, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(int_bits(a1), int_bits(a0))                                     # the At part: mcd_hook_pool's bits, fill included
    slab = a0[col0:col0 + Cout, row0:row0 + B].t() if neuron_major else a0[row0:row0 + B, col0:col0 + Cout]
    assert not bool((slab == OUT_FILL).any())
    assert torch.equal(int_bits(rows[:B, :Cout]), int_bits(slab.contiguous()))         # the rows block: the transposed slab
    assert bool((rows[:B, Cout:] == OUT_FILL).all()) and bool((rows[B:] == OUT_FILL).all())
    if len(shape) == 4:
        assert bool(torch.isnan(rows[1, 2])) and int(torch.isnan(rows[:B, :Cout]).sum()) == 1
    else:
        assert int(torch.isnan(rows[:B, :Cout]).sum()) == 1


def test_dual_write_refusals_and_binding(L, dev, mcd):
    from mammo_clip_dissect_amd import core
    x = k0_input((3, 5, 2, 4), dev)
    a = torch.full((9, 8), OUT_FILL, device=dev)
    rows = torch.full((3, 5), OUT_FILL, device=dev)
    ok = (x.data_ptr(), 3, 5, 8, AVG, a.data_ptr(), 0, 0, 1, 8)
    assert L.mcd_hook_pool_rows(*ok, None, 5, None) == -1                       # rows NULL
    assert L.mcd_hook_pool_rows(*ok, rows.data_ptr(), 4, None) == -1            # width < Cout
    assert b"mcd_hook_pool_rows" in L.mcd_last_error()
    assert L.mcd_hook_pool_rows(x.data_ptr(), 0, 5, 8, AVG, a.data_ptr(), 0, 0, 1, 8, rows.data_ptr(), 5, None) == 0    # B == 0
    torch.cuda.synchronize()
    assert bool((a == OUT_FILL).all()) and bool((rows == OUT_FILL).all())
    # core.hook_pool(rows=): the same kernel behind the binding; a channels-last input goes through K0n and the transpose kernel
    want = torch.full((9, 8), OUT_FILL, device=dev)
    assert core.hook_pool(x, "avg", want, 1, 2, True) == 5
    for inp in (x, x.contiguous(memory_format=torch.channels_last)):
        a.fill_(OUT_FILL)
        rows.fill_(OUT_FILL)
        assert core.hook_pool(inp, "avg", a, 1, 2, True, rows=rows) == 5
        assert torch.equal(int_bits(a), int_bits(want))
        assert torch.equal(int_bits(rows), int_bits(want[2:7, 1:4].t().contiguous()))
    with pytest.raises(TypeError):
        core.hook_pool(x, "avg", a, 1, 2, True, rows=torch.empty(3, 6, device=dev))
    with pytest.raises(TypeError):
        core.hook_pool(x, "avg", a, 1, 2, True, rows=torch.empty(2, 5, device=dev))


# ---- the stream and capture contracts of the kernel entry ---------------------------------------------------------------
def b_hook_pool_rows(L, dev):
    B, Cout, HW = 5, 70, 16                                  # test_gpu_stream_contracts' K0 shape
    return S.simple(L, dev, "K0 rows", [S._gen((B, Cout, HW))], [(B, Cout), (B, Cout)],
                    lambda i, o, st: L.mcd_hook_pool_rows(i[0], B, Cout, HW, 0, o[0], 0, 0, Cout, 1, o[1], Cout, st))


CACHE_STREAM_ROWS = {"mcd_hook_pool_rows": b_hook_pool_rows}
# the writer's entries take a stream too (or queue work): they are not capturable by contract (mcd_cache.h) and have the tests
# of their own below
WRITER_ENTRIES = {"mcd_cache_stream_open", "mcd_cache_stream_reserve", "mcd_cache_stream_push", "mcd_cache_stream_close",
                  "mcd_cache_stream_abort"}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(set(CACHE_STREAM_ROWS) | WRITER_ENTRIES) == sorted(mcd._lib.CACHE_SIGNATURES)


@pytest.fixture(scope="module")
def spin_cycles(dev):
    """A spin of at least S.MIN_SPIN_MS, in the cycles of torch.cuda._sleep (test_gpu_hf_clip's)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 20_000_000
    for _ in range(4):
        torch.cuda.synchronize()
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        e1.synchronize()
        real = e0.elapsed_time(e1)
        if S.MIN_SPIN_MS <= real <= 4 * S.MIN_SPIN_MS:
            break
        cycles = int(cycles * 2 * S.MIN_SPIN_MS / max(real, 1e-3))
    assert real >= S.MIN_SPIN_MS
    return cycles


@pytest.mark.parametrize("entry", sorted(CACHE_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):
    r = S.Run(entry, CACHE_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)      # (the control -- a launch on another stream IS seen -- is test_gpu_stream_contracts.py's)


@pytest.mark.parametrize("entry", sorted(CACHE_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    r = S.Run(entry, CACHE_STREAM_ROWS[entry](L, dev), dev)
    data = [r.stage(3003), r.stage(4004)]
    want = [r.eager(d) for d in data]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert r.call(st.cuda_stream) == 0               # the warm-up on the stream
    st.synchronize()
    r.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=st):
            rc = r.call(torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert r.untouched(), "the call ran during the capture"
        for d, w in zip(data, want):
            r.poison()
            r.refill(d)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            r.same(r.outs, w, entry)
    finally:
        g.reset()


# ---- the stream contract of the writer -------------------------------------------------------------------------------------
def test_writer_honours_the_callers_stream(utils, dev, spin_cycles, tmp_path):
    """On a side stream S behind a spin: fresh rows into the block, push, reserve, other rows into the same block, push.  The file
    must hold the fresh rows, then the other rows: a push that recorded its event anywhere but on S copies the stale block while S
    still spins.  Meanwhile the NULL stream spins five times as long, and close() -- which waits for the copies and the file --
    returns while it still does: nothing of the writer waits for the NULL stream."""
    n, u = 6, 40
    g = torch.Generator().manual_seed(11)
    stale, fresh, other = (torch.randn(3, u, generator=g) for _ in range(3))
    fresh[0, 0], fresh[0, 1] = float("nan"), -0.0
    block = stale.to(dev)
    fresh_d, other_d = fresh.to(dev), other.to(dev)
    path = str(tmp_path / "w.pt")
    w = utils.CacheStream(dev, n, [(path, u)], 3, slots=2)
    w.begin()
    assert os.path.exists(path + ".part") and not os.path.exists(path)
    st = torch.cuda.Stream()
    null_done = torch.cuda.Event()
    torch.cuda.synchronize()
    torch.cuda._sleep(5 * spin_cycles)                     # the NULL stream is busy from here on
    null_done.record()
    with torch.cuda.stream(st):
        torch.cuda._sleep(spin_cycles)
        block.copy_(fresh_d)
        w.push(0, block, 0, 3)
        w.reserve(0)
        block.copy_(other_d)
        w.push(0, block, 3, 3)
    w.close()
    still_spinning = not null_done.query()
    torch.cuda.synchronize()
    assert still_spinning, "close() returned only after the NULL stream's work: something of the writer is ordered behind it"
    assert os.listdir(str(tmp_path)) == ["w.pt"]
    got = torch.load(path, weights_only=True)
    assert torch.equal(int_bits(got), int_bits(torch.cat([fresh, other])))
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None


def test_writer_errors_come_out_of_close(utils, dev, tmp_path, mcd):
    """Rows out of order: the worker's append fails, close() raises that first error, and no file appears under either name.  A
    push larger than a slot is refused at once.  abort() leaves nothing."""
    u = 8
    block = torch.randn(4, u).to(dev)
    path = str(tmp_path / "e.pt")
    w = utils.CacheStream(dev, 8, [(path, u)], 2)
    w.begin()
    with pytest.raises(mcd._lib.McdError) as e:
        w.push(0, block, 0, 4)                              # 4 rows, slots sized for 2
    assert e.value.code == -1
    w.push(0, block, 0, 2)
    w.push(0, block, 4, 2)                                  # rows 2..3 were skipped
    with pytest.raises(mcd._lib.McdError, match="out of order"):
        w.close()
    assert os.listdir(str(tmp_path)) == []
    w = utils.CacheStream(dev, 8, [(path, u)], 2)
    w.begin()
    w.push(0, block, 0, 2)
    with pytest.raises(mcd._lib.McdError, match="2 of 8 rows"):   # a close before all rows arrived
        w.close()
    assert os.listdir(str(tmp_path)) == []
    w = utils.CacheStream(dev, 8, [(path, u)], 2)
    w.begin()
    w.push(0, block, 0, 2)
    w.abort()
    assert os.listdir(str(tmp_path)) == []


# ---- end to end ----------------------------------------------------------------------------------------------------------------
LAYERS = ["image_encoder.encoder.layer[0]", "image_encoder.encoder.layer[5]", "image_encoder.encoder.layer[11]"]
D_PROBE = "synthetic_37_224"


@pytest.fixture(scope="module")
def runs(mcd, dev, utils, tmp_path_factory):
    """describe_broad_neurons.main three times in this process on prebuilt models: the streaming route, MCD_CACHE_STREAM=0, the
    streaming route with a ring of two slots.  Per run: {cache file's base name: path}, the CSV bytes, the pushes counted."""
    from mammo_clip_dissect_amd.concept_vit import data_utils
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    clip_model, target_model = utils.build_mammo_models("breastclip_vit", str(dev))
    data = utils._probe_data(D_PROBE, str(dev), data_utils.target_preset("breastclip_vit"), "default")
    prebuilt = dict(clip_model=clip_model, target_model=target_model, data=data)
    base = tmp_path_factory.mktemp("cache_stream")
    out = {}
    for name, env, slots in (("stream", None, None), ("thread", "0", None), ("ring2", None, 2)):
        mp = pytest.MonkeyPatch()
        pushes = []
        try:
            if env is not None:
                mp.setenv("MCD_CACHE_STREAM", env)
            else:
                mp.delenv("MCD_CACHE_STREAM", raising=False)
            if slots is not None:
                mp.setattr(utils, "CACHE_STREAM_SLOTS", slots)
            push = utils.CacheStream.push
            mp.setattr(utils.CacheStream, "push", lambda self, f, b, r0, n: (pushes.append((f, r0, n)), push(self, f, b, r0, n))[1])
            act, res = str(base / name / "acts"), str(base / name / "results")
            got = drv.main(["--target_model", "breastclip_vit", "--target_layers", ",".join(LAYERS), "--d_probe", D_PROBE,
                            "--concept_set", CONCEPTS, "--batch_size", "16", "--device", str(dev), "--activation_dir", act,
                            "--result_dir", res, "--top_k", "20"], prebuilt=prebuilt)
        finally:
            mp.undo()
        csvs = glob.glob(os.path.join(got, "*.csv"))
        assert len(csvs) == 1
        everything = sorted(glob.glob(act + "/**/*", recursive=True))
        files = [f for f in everything if os.path.isfile(f)]
        # (the reference's name format repeats the directory inside the file's path: the files are told apart by their base names)
        assert len({os.path.basename(f) for f in files}) == len(files)
        out[name] = dict(files={os.path.basename(f): f for f in files}, csv=open(csvs[0], "rb").read(), pushes=pushes)
    return out


def test_the_two_routes_were_taken(runs):
    # 3 batches x (3 layers + the image embeddings); the first batch's pushes are sent again when the files are laid out
    per_file = {f: sorted({(r0, n) for ff, r0, n in runs["stream"]["pushes"] if ff == f}) for f in range(4)}
    assert all(v == [(0, 16), (16, 16), (32, 5)] for v in per_file.values()), per_file
    assert runs["thread"]["pushes"] == []
    assert sorted(set(runs["ring2"]["pushes"])) == sorted(set(runs["stream"]["pushes"]))


@pytest.mark.parametrize("other", ["thread", "ring2"])
def test_cache_files_and_csv_are_bit_equal(runs, other):
    a, b = runs["stream"], runs[other]
    assert sorted(a["files"]) == sorted(b["files"]) and len(a["files"]) == len(LAYERS) + 2
    assert all(f.endswith(".pt") for f in a["files"]), sorted(a["files"])             # no .part left behind
    widths = []
    for rel in sorted(a["files"]):
        ta = torch.load(a["files"][rel], weights_only=True)
        tb = torch.load(b["files"][rel], weights_only=True)
        assert ta.dtype == tb.dtype == torch.float32 and ta.shape == tb.shape and ta.is_contiguous(), rel
        assert torch.equal(int_bits(ta), int_bits(tb)), rel
        assert bool(ta.abs().sum() > 0), rel
        widths.append(tuple(ta.shape))
        with zipfile.ZipFile(a["files"][rel]) as z:
            assert z.testzip() is None, rel
    assert sorted(widths).count((37, 768)) == len(LAYERS)
    assert a["csv"] == b["csv"] and len(a["csv"]) > 1000
