"""GPU: the EfficientNet-B5 tower's HIP route -- K12 (stem), K13 (depthwise + BN + SiLU + SE partial sums), K14 (SE gate),
K15 (channel scale) and K0n (hook pooling of channels-last outputs) against float64 and against torch / K0, batch
invariance, one block of every stage and the whole tower against a float64 CPU forward, and the driver and its
multi-rank form through the new route."""
import glob
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import util
from util import mild_bn as _mild_bn, nerr as _nerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _dw_ref(x64, w_tap, bias, k, s, silu_in):
    """float64 CPU depthwise conv on NHWC x64 with TF-SAME padding: [B, Ho, Wo, C]."""
    from mammo_clip_dissect_amd import core
    B, H, W, C = x64.shape
    a = x64.permute(0, 3, 1, 2)
    if silu_in:
        a = F.silu(a)
    _, pt, pb = core.same_pad(H, k, s)
    _, pl, pr = core.same_pad(W, k, s)
    w = w_tap.double().cpu().t().reshape(C, 1, k, k)
    y = F.conv2d(F.pad(a, [pl, pr, pt, pb]), w, bias.double().cpu(), s, 0, 1, C)
    return F.silu(y).permute(0, 2, 3, 1)


# (C, H, W, k, s): the 224 x 224 shapes of the tower and odd sizes of Mammo-CLIP's 1520 x 912 and 200 x 136 inputs
DW_SHAPES = [(48, 112, 112, 3, 1), (24, 112, 112, 3, 1), (144, 112, 112, 3, 2), (240, 56, 56, 3, 1), (240, 56, 56, 5, 2),
             (384, 28, 28, 5, 1), (384, 28, 28, 3, 2), (768, 14, 14, 3, 1), (1056, 14, 14, 5, 1), (1056, 14, 14, 5, 2),
             (1824, 7, 7, 5, 1), (3072, 7, 7, 3, 1), (24, 95, 57, 3, 1), (144, 95, 57, 3, 2), (240, 24, 15, 5, 2),
             (8, 13, 9, 5, 1), (4, 5, 6, 3, 2), (36, 17, 3, 5, 2)]


@pytest.mark.parametrize("C,H,W,k,s", DW_SHAPES)
@pytest.mark.parametrize("silu_in", [True, False])
def test_k13_against_float64(core, dev, C, H, W, k, s, silu_in):
    g = torch.Generator().manual_seed(C * 7 + H + k * 3 + s + int(silu_in))
    B = 2
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(k * k, C, generator=g) / k
    b = torch.randn(C, generator=g) * 0.1
    y, psum = core.dwconv_bn_silu(x.to(dev), w.to(dev), b.to(dev), k, s, silu_in)
    torch.cuda.synchronize()
    ref = _dw_ref(x.double(), w, b, k, s, silu_in)
    assert tuple(y.shape) == tuple(ref.shape)
    assert _nerr(y, ref) < 2e-6, _nerr(y, ref)
    Ho, Wo = ref.shape[1:3]
    assert tuple(psum.shape) == (B, core.dwconv_tiles(Ho, Wo), C)
    mean = psum.double().cpu().sum(1) / (Ho * Wo)
    assert _nerr(mean, ref.mean(dim=(1, 2))) < 2e-6


@pytest.mark.parametrize("H,W", [(224, 224), (200, 136), (95, 57), (7, 9)])
def test_k12_against_float64(core, dev, H, W):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(3, 3, H, W, generator=g)
    w = torch.randn(48, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(48, generator=g) * 0.1
    y = core.conv_stem_nhwc(x.to(dev), w.permute(1, 2, 3, 0).contiguous().to(dev), b.to(dev))
    torch.cuda.synchronize()
    _, pt, pb = core.same_pad(H, 3, 2)
    _, pl, pr = core.same_pad(W, 3, 2)
    ref = F.silu(F.conv2d(F.pad(x.double(), [pl, pr, pt, pb]), w.double(), b.double(), 2)).permute(0, 2, 3, 1)
    assert tuple(y.shape) == tuple(ref.shape) and _nerr(y, ref) < 2e-6


@pytest.mark.parametrize("C,sq,T,hw", [(144, 6, 196, 12544), (3072, 128, 1, 49), (24, 1, 4, 30), (1056, 44, 4, 196)])
def test_k14_against_float64(core, dev, C, sq, T, hw):
    g = torch.Generator().manual_seed(C + sq)
    B = 3
    psum = torch.randn(B, T, C, generator=g) * (hw / T) ** 0.5
    wr, br = torch.randn(sq, C, generator=g) / C ** 0.5, torch.randn(sq, generator=g) * 0.1
    we, be = torch.randn(C, sq, generator=g) / sq ** 0.5, torch.randn(C, generator=g) * 0.1
    s = core.se_gate(psum.to(dev), hw, wr.to(dev), br.to(dev), we.t().contiguous().to(dev), be.to(dev))
    torch.cuda.synchronize()
    mean = psum.double().sum(1) / hw
    ref = torch.sigmoid(F.silu(mean @ wr.double().t() + br.double()) @ we.double().t() + be.double())
    assert _nerr(s, ref) < 2e-6


@pytest.mark.parametrize("B,H,W,C", [(3, 56, 56, 240), (2, 7, 7, 3072), (5, 13, 9, 4)])
def test_k15_bit_equal_to_torch(core, dev, B, H, W, C):
    g = torch.Generator().manual_seed(C)
    y = torch.randn(B, H, W, C, generator=g).to(dev)
    s = torch.rand(B, C, generator=g).to(dev)
    want = y * s[:, None, None, :]
    got = core.channel_scale_(y.clone(), s)
    assert torch.equal(got, want)


def test_batch_invariance(core, dev):
    """Images [0:3] through K12, K13, K14, K15 give the bits of the first three images of the same kernels on [0:7]."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(7, 3, 95, 57, generator=g).to(dev)
    w12, b12 = (torch.randn(3, 3, 3, 48, generator=g) * 0.3).to(dev), torch.randn(48, generator=g).to(dev) * 0.1
    e = torch.randn(7, 48, 29, 240, generator=g).to(dev)
    w13, b13 = (torch.randn(25, 240, generator=g) / 5).to(dev), (torch.randn(240, generator=g) * 0.1).to(dev)
    wr, br = (torch.randn(10, 240, generator=g) / 15).to(dev), (torch.randn(10, generator=g) * 0.1).to(dev)
    we, be = (torch.randn(10, 240, generator=g) / 3).to(dev), (torch.randn(240, generator=g) * 0.1).to(dev)

    def run(n):
        stem = core.conv_stem_nhwc(x[:n].contiguous(), w12, b12)
        d, psum = core.dwconv_bn_silu(e[:n].contiguous(), w13, b13, 5, 2, True)
        s = core.se_gate(psum, d.shape[1] * d.shape[2], wr, br, we, be)
        core.channel_scale_(d, s)
        return stem, psum, s, d
    small, full = run(3), run(7)
    for a, b in zip(small, full):
        assert torch.equal(a, b[:3])


# ---- K0n ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(3, 40, 28, 28), (2, 24, 95, 57), (2, 2048, 7, 7), (4, 100, 5, 4), (1, 8, 1, 3)])
@pytest.mark.parametrize("mode", ["avg", "max"])
@pytest.mark.parametrize("neuron_major", [False, True])
def test_k0n_bit_equal_to_k0(core, dev, B, C, H, W, mode, neuron_major):
    g = torch.Generator().manual_seed(B * C + H * W)
    x = torch.randn(B, C, H, W, generator=g) * 3
    if mode == "max":
        x[0, 1, H // 2, W // 2] = float("nan")          # NaN in some planes
        x[B - 1, C - 1, 0, 0] = float("nan")
    x = x.to(dev).contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous() or H * W == 1
    shape = (C + 5, B + 3) if neuron_major else (B + 3, C + 5)
    d1 = torch.full(shape, -7.0, device=dev)
    d2 = d1.clone()
    L = core._lib.load()
    xc = x.contiguous()
    sn, su = (1, d1.stride(0)) if neuron_major else (d1.stride(0), 1)
    m = core.POOL_MODES[mode]
    core.check(L.mcd_hook_pool(xc.data_ptr(), B, C, H * W, m, d1.data_ptr(), 2, 3, sn, su, core._stream()))
    core.check(L.mcd_hook_pool_nhwc(x.data_ptr(), B, C, H * W, m, d2.data_ptr(), 2, 3, sn, su, core._stream()))
    torch.cuda.synchronize()
    assert torch.equal(d1.isnan(), d2.isnan())
    assert torch.equal(torch.nan_to_num(d1), torch.nan_to_num(d2))
    if mode == "max":
        assert d2.isnan().sum() == 2
    # core.hook_pool sends the channels_last tensor to K0n: the same bits as on the contiguous copy
    d3, d4 = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
    core.hook_pool(x, mode, d3, 1, 2, neuron_major)
    core.hook_pool(xc, mode, d4, 1, 2, neuron_major)
    assert torch.equal(torch.nan_to_num(d3), torch.nan_to_num(d4)) and torch.equal(d3.isnan(), d4.isnan())


def test_k0n_silu_avg_against_float64(core, dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 7, 5, 2048, generator=g) * 2
    got = core.silu_avg_pool_nhwc(x.to(dev))
    assert _nerr(got, F.silu(x.double()).mean(dim=(1, 2))) < 2e-6


# ---- blocks and the tower ---------------------------------------------------------------------------------------------
B5_WRAPPERS = ("conv_stem_nhwc", "dwconv_bn_silu", "se_gate", "channel_scale_", "silu_avg_pool_nhwc")


def _block_cases(du):
    """One _MBConv of every stage: (stage, block index in the tower, first block of its stage)."""
    t = du.EfficientNetB5Tower()
    seen, cases = set(), []
    for i, b in enumerate(t._blocks):
        st = (b.k, b.cout)
        first = st not in seen
        if first or (b.skip and (st, "skip") not in seen):
            cases.append((i, first))
            seen.add(st)
            if b.skip:
                seen.add((st, "skip"))
    return cases


@pytest.mark.parametrize("size", [(224, 224), (200, 136)])
def test_blocks_against_float64(du, core, dev, monkeypatch, size):
    torch.manual_seed(0)
    tower = du.EfficientNetB5Tower()
    _mild_bn(tower, 1)
    tower.eval()
    cases = _block_cases(du)
    assert len(cases) >= 13         # every stage's first block, and a skip block of every stage that has one
    # the blocks' input sizes at this image size: from a shape pass of the ATen tower on the host
    sizes = {}
    hs = [b.register_forward_pre_hook(lambda m, i, k=j: sizes.__setitem__(k, tuple(i[0].shape[1:])))
          for j, b in enumerate(tower._blocks)]
    with torch.no_grad():
        tower(torch.zeros(1, 3, *size))
    for h in hs:
        h.remove()
    tower.to(dev)
    cnt = util.CallCounter(core, monkeypatch, B5_WRAPPERS)
    for i, first in cases:
        blk = tower._blocks[i]
        C, H, W = sizes[i]
        g = torch.Generator().manual_seed(i)
        x = torch.randn(2, C, H, W, generator=g)
        with torch.no_grad():
            ref = blk.double().cpu()(x.double())
            blk.float().to(dev)
            xg = x.to(dev).contiguous(memory_format=torch.channels_last)
            x0 = xg.clone()
            before = cnt.n.get("dwconv_bn_silu", 0)
            got = blk(xg)
            assert cnt.n["dwconv_bn_silu"] == before + 1, i          # the HIP route was taken
            assert torch.equal(xg, x0)                                # the block's input is left alone
            monkeypatch.setattr(du, "HIP_MBCONV", False)
            aten = blk(x.to(dev))
            monkeypatch.setattr(du, "HIP_MBCONV", True)
        assert tuple(got.shape) == tuple(ref.shape) and got.is_contiguous(memory_format=torch.channels_last)
        e_hip, e_aten = _nerr(got, ref), _nerr(aten, ref)
        assert e_hip <= 2 * e_aten + 1e-6, (i, first, blk.skip, e_hip, e_aten)


@pytest.mark.parametrize("size", [(224, 224), (200, 136)])
def test_tower_against_float64(du, core, dev, monkeypatch, size):
    torch.manual_seed(0)
    tower = du.EfficientNetB5Tower()
    _mild_bn(tower, 2)
    tower.eval()
    keys = list(tower.state_dict().keys())
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, *size, generator=g)

    def hooked(model, xin):
        outs = []
        hs = [b.register_forward_hook(lambda m, i, o: outs.append(o.detach().double().cpu())) for b in model._blocks]
        with torch.no_grad():
            y = model(xin)
        for h in hs:
            h.remove()
        return y, outs
    ref, ref_outs = hooked(tower.double(), x.double())
    tower.float().to(dev)
    monkeypatch.setattr(du, "HIP_MBCONV", False)
    aten, aten_outs = hooked(tower, x.to(dev))
    monkeypatch.setattr(du, "HIP_MBCONV", True)
    cnt = util.CallCounter(core, monkeypatch, B5_WRAPPERS)
    xg = x.to(dev)
    got, got_outs = hooked(tower, xg)
    assert cnt.n == {"conv_stem_nhwc": 1, "dwconv_bn_silu": 39, "se_gate": 39, "channel_scale_": 39,
                     "silu_avg_pool_nhwc": 1}
    assert torch.equal(xg, x.to(dev))
    assert list(tower.state_dict().keys()) == keys
    assert len(got_outs) == 39 and [o.shape for o in got_outs] == [o.shape for o in ref_outs]
    assert all(o.dim() == 4 for o in got_outs)
    for j, (a, b, r) in enumerate(zip(got_outs, aten_outs, ref_outs)):
        assert _nerr(a, r) <= 2 * _nerr(b, r) + 1e-6, (j, _nerr(a, r), _nerr(b, r))
    assert _nerr(got, ref) <= 2 * _nerr(aten, ref) + 1e-6, (_nerr(got, ref), _nerr(aten, ref))
    # a hook on a submodule the route skips: that block takes ATen, the hook fires and sees ATen's values
    seen = []
    h = tower._blocks[5]._depthwise_conv.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    cnt.n.clear()
    with torch.no_grad():
        y2 = tower(xg)
        monkeypatch.setattr(du, "HIP_MBCONV", False)
        tower(x.to(dev))
        monkeypatch.setattr(du, "HIP_MBCONV", True)
    h.remove()
    assert cnt.n["dwconv_bn_silu"] == 38 and len(seen) == 2
    assert _nerr(seen[0], seen[1]) < 1e-4
    assert _nerr(y2, ref) <= 2 * _nerr(aten, ref) + 1e-6


# ---- the driver ------------------------------------------------------------------------------------------------------
def _run_b5_driver(dev, tmp, tag, n=160, batch=40):
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    layers = ["image_encoder._blocks[%d]" % i for i in range(39)]
    act, res = os.path.join(tmp, "acts_" + tag), os.path.join(tmp, "results_" + tag)
    out = drv.main(["--target_model", "breastclip", "--target_layers", ", ".join(layers), "--d_probe",
                    "synthetic_%d_224" % n, "--concept_set", CONCEPTS, "--batch_size", str(batch), "--device", str(dev),
                    "--activation_dir", act, "--result_dir", res, "--top_k", "100"])
    return layers, act, glob.glob(os.path.join(out, "*.csv"))[0]


def test_driver_b5_all_blocks_through_the_route(du, core, dev, oracle, tmp_path, monkeypatch):
    import test_gpu_pipeline as tp
    cnt = util.CallCounter(core, monkeypatch, B5_WRAPPERS)
    layers, act, csv = _run_b5_driver(dev, str(tmp_path), "hip")
    assert cnt.n.get("dwconv_bn_silu", 0) >= 39 * 4 and cnt.n.get("conv_stem_nhwc", 0) >= 4
    words = open(CONCEPTS).read().split("\n")
    tp._check_csv_against_oracle(csv, act + "/**/*.pt", [layers[0], layers[9], layers[20], layers[38]], oracle, "og",
                                 100, words)
    # the cache files against the same run on the ATen route
    monkeypatch.setattr(du, "HIP_MBCONV", False)
    _, act2, _ = _run_b5_driver(dev, str(tmp_path), "aten")
    f1 = sorted(glob.glob(act + "/**/*.pt", recursive=True))
    f2 = sorted(glob.glob(act2 + "/**/*.pt", recursive=True))
    assert [os.path.basename(f) for f in f1] == [os.path.basename(f) for f in f2] and len(f1) == 39 + 2
    for a, b in zip(f1, f2):
        if "Specific_concepts" in a:
            continue
        ta, tb = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
        assert ta.shape == tb.shape
        assert _nerr(ta, tb) < 1e-4, (os.path.basename(a), _nerr(ta, tb))


def _b5_driver_csv(world, rank, tmp, n_images, batch):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd.concept_vit import data_utils, describe_broad_neurons, utils
    from mammo_clip_dissect_amd.pipeline import shard_bounds
    dev = torch.device("cuda:0")
    clip_model, target_model = utils.build_mammo_models("breastclip", dev)
    lo, hi = shard_bounds(n_images, world, rank)
    d_probe = "synthetic_%d_224" % n_images
    data = data_utils.get_data(d_probe, None, dev, lo, hi)
    layers = ["image_encoder._blocks[%d]" % i for i in (0, 7, 20, 38)]
    out = describe_broad_neurons.main(
        ["--target_model", "breastclip", "--target_layers", ",".join(layers), "--d_probe", d_probe, "--concept_set",
         CONCEPTS, "--batch_size", str(batch), "--device", "cuda:0", "--activation_dir",
         os.path.join(tmp, "acts%d_%d" % (world, rank)), "--result_dir", os.path.join(tmp, "res%d" % world), "--top_k", "50"],
        prebuilt={"clip_model": clip_model, "target_model": target_model, "data": data,
                  "gather": util.host_staged_gather() if world > 1 else None})
    torch.cuda.synchronize()
    return out


def test_b5_driver_csv_bytes_one_vs_two_ranks(mcd, tmp_path, monkeypatch):
    """The whole B5 job through the HIP route at 1 rank and at 2 ranks (equal batch shapes, the heuristic hipBLASLt pick):
    rank 0's CSV is the same bytes -- an image's activations do not depend on which rank or batch encodes it."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    tmp = str(tmp_path)
    csv = {}
    for world in (1, 2):        # fresh processes: this one may keep timed GEMM picks for these shapes from other tests
        got = util.run_ranks(world, _b5_driver_csv, (tmp, 160, 40), timeout=900, env=util.TORCHRUN_ENV)
        csv[world] = open(glob.glob(os.path.join(got[0], "*.csv"))[0], "rb").read()
    assert csv[1] == csv[2] and len(csv[1]) > 10000
