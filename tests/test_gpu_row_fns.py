"""GPU: the fused and image-sharded route for rank_reorder, cos_similarity and cos_similarity_cubed.
  * mcd_prepare_rows_gathered (K1a / K7 on rows that arrive in pieces) is bit-equal to normalize_rows /
    center_cube_normalize_rows on the concatenated rows, for any number and sizes of pieces;
  * Dissector.finish for the three functions equals the per-layer drop-in calls bit for bit, and the goldens;
  * 2, 3 and 4 ranks (gloo rendezvous, host-staged all-gather: tests/util.py) give the one-rank bits;
  * the og and clip drivers take the fused route for them (same CSV bytes as the per-layer route), also with two ranks,
    where the per-layer route has no cache files to read; the broad driver still raises the reference's TypeError."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
ROW_FNS = ("rank_reorder", "cos_similarity", "cos_similarity_cubed")
MODES = {"normalize": "normalize_rows", "center_cube": "center_cube_normalize_rows"}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pieces(rng, n, G):
    """G uneven piece lengths adding up to n, one of them 0 when G > 1."""
    if G == 1:
        return [n]
    cuts = np.sort(rng.integers(0, n + 1, size=G - 2))
    c = np.diff(np.concatenate([[0], cuts, [n]])).tolist()
    c.insert(int(rng.integers(0, G)), 0)
    return [int(v) for v in c]


# ---- 1. the kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_prepare_rows_gathered_bit_equal(mcd, dev, G):
    """Rows of N = 1..8 (every N % 8 tail of K1a), <= 128, <= 1 024 and > 1 024 images, 13 rows of 17 (not a multiple of
    8) in a sub-range, pieces of uneven length including an empty one: the same bits as the one-piece kernels on the
    concatenated rows, NaN rows (an all-zero row under mode 0) included."""
    from mammo_clip_dissect_amd import core
    rng = np.random.default_rng(G)
    R, r0, r1 = 17, 2, 15
    for n in [1, 2, 3, 4, 5, 6, 7, 8, 61, 126, 128, 300, 517, 1021, 1024, 1029, 2050, 10003]:
        X = torch.randn(R, n, generator=torch.Generator().manual_seed(n)) * 3 + 0.5
        X[5] = 0.0
        X = X.to(dev)
        counts = _pieces(rng, n, G)
        ld = max(counts) + 3
        src = torch.full((G, R, ld), float("nan"), device=dev)       # padding never read
        o = 0
        for g, c in enumerate(counts):
            src[g, :, :c] = X[:, o:o + c]
            o += c
        for mode, ref_fn in MODES.items():
            ref = getattr(core, ref_fn)(X[r0:r1].contiguous())
            got = core.prepare_rows_gathered(src, counts, (r0, r1), mode)
            assert got.shape == (r1 - r0, n)
            assert torch.equal(_bits(got), _bits(ref)), (G, n, mode, counts)
            if G == 1:   # a plain padded matrix (the dissector's At) as the one piece; the source is left as it was
                At = torch.zeros((R, n + 64), device=dev)
                At[:, :n] = X
                keep = At.clone()
                got = core.prepare_rows_gathered(At, [n], (r0, r1), mode)
                assert torch.equal(_bits(got), _bits(ref)) and torch.equal(At, keep), (n, mode)


def test_prepare_rows_gathered_rejects_bad_arguments(mcd, dev):
    """Bad arguments are error codes from the host side of the call, never a launch."""
    import ctypes
    from mammo_clip_dissect_amd import _lib, core
    L = _lib.load()
    src = torch.ones((3, 4, 10), device=dev)
    dst = torch.zeros((4, 30), device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(src_p=src.data_ptr(), ld_src=10, ld_block=40, G=3, counts=(10, 0, 9), n=19, row0=0, row1=4, mode=0,
             dst_p=dst.data_ptr(), ldd=30):
        arr = (ctypes.c_int64 * max(len(counts), 1))(*counts)
        return L.mcd_prepare_rows_gathered(src_p, ld_src, ld_block, G, arr, n, row0, row1, mode, 1e-3, dst_p, ldd, s)

    assert call() == 0
    assert call(src_p=None) == -1 and "NULL" in L.mcd_last_error().decode()
    assert call(dst_p=None) == -1
    assert call(ldd=18) == -1                                  # ldd < N
    assert call(counts=(10, 0, 8)) == -1 and "add up" in L.mcd_last_error().decode()
    assert call(counts=(11, 0, 8)) == -1                       # a piece longer than the row pitch
    assert call(counts=(10, -1, 10)) == -1
    assert call(G=0) == -1
    assert call(G=65, counts=(0,) * 64 + (19,)) == -5          # more pieces than the kernel argument holds
    assert call(mode=2) == -1
    assert call(row0=3, row1=2) == -1
    assert call(ld_block=30) == -1                             # blocks would overlap
    assert call(n=0, counts=(0, 0, 0)) == -1
    torch.cuda.synchronize()
    assert float(dst.abs().sum()) > 0                          # only the valid call wrote
    with pytest.raises(ValueError):
        core.prepare_rows_gathered(src, [10, 0], (0, 4), "normalize")
    with pytest.raises(ValueError):
        core.prepare_rows_gathered(src, [10, 0, 11], (0, 4), "normalize")


# ---- 2. fused == per layer -----------------------------------------------------------------------------------------
def _problem(N, widths, C, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sum(widths), N, generator=g), torch.randn(N, D, generator=g), torch.randn(C, D, generator=g)


def _fused(dev, At, E_img, E_txt, widths, fn, seed=None):
    from mammo_clip_dissect_amd.pipeline import Dissector
    N = At.shape[1]
    dis = Dissector(N, ["l%d" % i for i in range(len(widths))], widths, E_txt.shape[0], E_txt.shape[1], dev, similarity_fn=fn)
    dis.At[:, :N] = At.to(dev)
    dis.E_img[:] = torch.as_tensor(E_img).to(dev)
    dis.cursor = N
    keep = dis.At.clone()
    if seed is not None:
        torch.manual_seed(seed)
    res = dis.finish(torch.as_tensor(E_txt).to(dev))
    torch.cuda.synchronize()
    assert torch.equal(dis.At, keep)                 # the cache writer reads At after finish()
    return res


@pytest.mark.parametrize("fn", ROW_FNS)
def test_fused_row_fns_equal_per_layer_api(mcd, dev, fn):
    """One pass over all layers == the per-layer drop-in calls (similarity.<fn>; rank_reorder under the same seed), bit
    for bit: similarities, top-10 concepts, top-5 images; the CPU generator ends in the same state."""
    from mammo_clip_dissect_amd import core
    from mammo_clip_dissect_amd.concept_vit import similarity
    widths, N, C, D = [64, 33, 7, 130], 600, 763, 512
    At, E_img, E_txt = _problem(N, widths, C, D, 3)
    res = _fused(dev, At, E_img, E_txt, widths, fn, seed=77)
    state = torch.get_rng_state()
    P = core.embed_gemm(core.normalize_rows(E_img.to(dev)), core.normalize_rows(E_txt.to(dev)))
    torch.manual_seed(77)
    o = 0
    for w in widths:
        A = At[o:o + w].t().contiguous().to(dev)
        sim = getattr(similarity, fn)(P, A, device=str(dev))
        assert torch.equal(_bits(sim), _bits(res.sim[o:o + w])), (fn, w)
        v, i = core.row_topk(sim, 10)
        assert torch.equal(_bits(v), _bits(res.vals[o:o + w])) and torch.equal(i, res.ids[o:o + w])
        t5v, t5 = core.col_topk(A, 5)
        assert torch.equal(t5, res.top_ids[o:o + w]) and torch.equal(t5v, res.top_vals[o:o + w])
        o += w
    assert torch.equal(torch.get_rng_state(), state)


def test_fused_row_fns_against_goldens(mcd, dev):
    """The reference's own outputs on the golden 'main' case (256 images x 64 neurons x 763 concepts), within the
    tolerances of the drop-in tests (test_gpu_e2e.py): cosines 5e-7; rank_reorder NaN pattern identical, 5e-6 relative."""
    z = util.golden("main")
    At = torch.from_numpy(z["A"]).t().contiguous()
    w = [At.shape[0]]
    for fn in ("cos_similarity", "cos_similarity_cubed"):
        got = _fused(dev, At, z["E_img"], z["E_txt"], w, fn).sim.cpu().numpy()
        assert np.abs(got - z[fn]).max() <= 5e-7, fn
    got = _fused(dev, At, z["E_img"], z["E_txt"], w, "rank_reorder", seed=1234).sim.cpu().numpy()
    ref = z["rank_reorder_seed1234"]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    m = ~np.isnan(ref)
    assert (np.abs(got[m] - ref[m]) / np.abs(ref[m])).max() <= 5e-6


# ---- 3. ranks == one rank ------------------------------------------------------------------------------------------
def _run(world, rank, N, widths, C, D, seed, top_fraction):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mammo_clip_dissect_amd  # noqa: F401
    import util as u
    from mammo_clip_dissect_amd.pipeline import Dissector, shard_bounds
    dev = torch.device("cuda:0")
    At, E_img, E_txt = _problem(N, widths, C, D, seed)
    lo, hi = shard_bounds(N, world, rank)
    dis = Dissector(hi - lo, ["l%d" % i for i in range(len(widths))], widths, C, D, dev,
                    gather=u.host_staged_gather() if world > 1 else None)
    dis.At[:, :hi - lo] = At[:, lo:hi].to(dev)
    dis.E_img[:] = E_img[lo:hi].to(dev)
    dis.cursor = hi - lo
    out = {}
    for fn in ROW_FNS:
        if fn == "rank_reorder":
            dis.set_scoring(fn, top_fraction=top_fraction)
        else:
            dis.set_scoring(fn)
        torch.manual_seed(seed)
        r = dis.finish(E_txt.to(dev), k_desc=10, k_img=5)
        torch.cuda.synchronize()
        out[fn] = [t.cpu().numpy() for t in (r.sim, r.vals, r.ids, r.top_ids, r.top_vals)]
    out["rng"] = torch.get_rng_state().numpy()
    return out


@pytest.mark.parametrize("world,case", [(2, (1200, [96, 40, 7], 763, 512, 21, 0.05)),
                                        (3, (1001, [64, 33], 763, 512, 23, 0.05)),    # 334 + 334 + 333 images
                                        (4, (250, [40, 9], 763, 512, 24, 0.5))])      # top_n = 125 > every shard (63)
def test_row_fns_ranks_on_hip_bit_identical_to_one(mcd, world, case):
    single = _run(1, 0, *case)
    got = util.run_ranks(world, _run, case, timeout=600)
    for r in range(world):
        for fn in ROW_FNS:
            for a, b in zip(single[fn], got[r][fn]):
                assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), (r, fn)
        assert np.array_equal(single["rng"], got[r]["rng"])


# ---- 4. drivers ----------------------------------------------------------------------------------------------------
def _csv_bytes(out):
    return open(glob.glob(os.path.join(out, "*.csv"))[0], "rb").read()


@pytest.mark.parametrize("fn", ROW_FNS)
@pytest.mark.parametrize("variant", ["og", "clip"])
def test_driver_fused_route_equals_per_layer_route(mcd, dev, tmp_path, monkeypatch, variant, fn):
    """describe_og_neurons / describe_clip_neurons with --similarity_fn rank_reorder | cos_similarity | cos_similarity_cubed:
    the fused route's CSV is the per-layer route's (MCD_DRIVER_PER_LAYER=1) byte for byte.  The second run scores the
    first run's cache files: two extractions of the ResNet-50 target need not give the same bits (its deepest
    convolutions), and the comparison is about the scoring routes."""
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons, describe_og_neurons
    drv = describe_og_neurons if variant == "og" else describe_clip_neurons
    argv = ["--target_model", "resnet50", "--target_layers", "layer1,layer4", "--d_probe", "synthetic_128_224",
            "--concept_set", CONCEPTS, "--batch_size", "64", "--device", str(dev), "--similarity_fn", fn]
    torch.manual_seed(5)
    fused = drv.main(argv + ["--activation_dir", str(tmp_path / "a1"), "--result_dir", str(tmp_path / "r1")])
    monkeypatch.setenv("MCD_DRIVER_PER_LAYER", "1")
    torch.manual_seed(5)
    per_layer = drv.main(argv + ["--activation_dir", str(tmp_path / "a1"), "--result_dir", str(tmp_path / "r2")])
    a, b = _csv_bytes(fused), _csv_bytes(per_layer)
    assert a == b and len(a) > 10000


def _og_driver(world, rank, tmp, fn):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mammo_clip_dissect_amd  # noqa: F401
    import util as u
    from mammo_clip_dissect_amd import pipeline
    from mammo_clip_dissect_amd.concept_vit import describe_og_neurons
    if world > 1:   # one GPU holds every rank: the RCCL transport cannot, the host-staged rehearsal of it can
        staged = u.host_staged_gather()
        pipeline.rccl_all_gather_rows = lambda t, group=None: staged(t)
    layers = ["image_encoder.encoder.layer[%d]" % i for i in (0, 11)]
    torch.manual_seed(11)
    out = describe_og_neurons.main(
        ["--target_model", "breastclip_vit", "--target_layers", ",".join(layers), "--d_probe", "synthetic_200_224",
         "--concept_set", CONCEPTS, "--batch_size", "50", "--device", "cuda:0", "--similarity_fn", fn,
         "--activation_dir", os.path.join(tmp, "acts%d_%d" % (world, rank)), "--result_dir", os.path.join(tmp, "res%d" % world)])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fn", ["cos_similarity", "rank_reorder"])
def test_og_driver_two_ranks_equal_one(mcd, dev, tmp_path, monkeypatch, fn):
    """describe_og_neurons under two ranks with cos_similarity / rank_reorder: a multi-rank run writes no activation cache,
    so only the fused route can score it -- rank 0's CSV is the one-rank CSV, byte for byte (encoder bits pinned as in
    test_gpu_multirank.py: heuristic hipBLASLt picks, shard boundaries on batch multiples)."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    monkeypatch.setenv("MCD_SHARD_ALIGN", "50")
    tmp = str(tmp_path)
    one = _csv_bytes(_og_driver(1, 0, tmp, fn))
    got = util.run_ranks(2, _og_driver, (tmp, fn), timeout=900, env=util.TORCHRUN_ENV)
    assert _csv_bytes(got[0]) == one and len(one) > 10000
    assert not glob.glob(os.path.join(tmp, "acts2_*", "**", "*.pt"), recursive=True)     # no cache files at two ranks


def test_broad_driver_rank_reorder_still_raises_type_error(mcd, dev, tmp_path):
    """describe_broad_neurons passes top_k to the similarity function (reference utils.py:602); rank_reorder takes none:
    TypeError, as in the reference."""
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    with pytest.raises(TypeError, match="top_k"):
        drv.main(["--target_model", "breastclip_vit", "--target_layers", "image_encoder.encoder.layer[0]", "--d_probe",
                  "synthetic_64_224", "--concept_set", CONCEPTS, "--batch_size", "64", "--device", str(dev),
                  "--activation_dir", str(tmp_path / "a"), "--result_dir", str(tmp_path / "r"), "--similarity_fn",
                  "rank_reorder"])
