"""GPU: the OpenAI-CLIP RN50 / RN101 dissector on its HIP route -- K19 (3x3 / 2 stem), K20 (2x2 average pooling) and K21
(attention-pool tokens) as kernels, then the attention pool, the anti-aliased Bottleneck, the small tower of the reference
fixture and RN50 itself against float64 CPU forwards, routing and call counts, and the driver with --clip_model RN50.

The bound is the project's (test_gpu_resnet.py): normalised error max|got - ref| / max|ref| against float64 at most twice
that of ATen's fp32 result on the same inputs (measured in the same test) plus 1e-6.  Where the kernel's order is ATen's
(K20, K21's rows 1..) the check is torch.equal."""
import glob
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import clip_rn_recipe as recipe
import util
from util import mild_bn as _mild_bn, nerr as _nerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
LAYERS = ["layer1", "layer2", "layer3", "layer4", "attnpool"]
WRAPPERS = ("conv3x3s2_nhwc", "avgpool2_nhwc", "attnpool_tokens", "conv_igemm_nhwc", "vit_attention_cls", "linear_residual")


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _bound(e_hip, e_aten, what):
    print("%s: hip %.3e aten %.3e ratio to the bound %.3f" % (what, e_hip, e_aten, e_hip / (2 * e_aten + 1e-6)))
    assert e_hip <= 2 * e_aten + 1e-6, (what, e_hip, e_aten)


# ---- 1. K19 -------------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout): partial tiles on both axes and odd sizes; one pixel; the 4-channel pass; whole tiles, four of them
K19_SHAPES = [(2, 3, 35, 37, 32), (1, 3, 1, 1, 32), (3, 1, 16, 16, 8), (2, 3, 64, 64, 32)]


@pytest.mark.parametrize("shape", K19_SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_k19_against_float64(core, dev, shape, relu):
    B, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(H + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    bias = torch.randn(Cout, generator=g)
    act = F.relu if relu else (lambda t: t)
    r64 = act(F.conv2d(x.double(), w.double(), bias.double(), 2, 1)).permute(0, 2, 3, 1)
    aten = act(F.conv2d(x.to(dev), w.to(dev), bias.to(dev), 2, 1)).permute(0, 2, 3, 1)
    xg = x.to(dev)
    got = core.conv3x3s2_nhwc(xg, w.permute(1, 2, 3, 0).contiguous().to(dev), bias.to(dev), relu=relu)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout) == tuple(r64.shape) and got.is_contiguous()
    assert torch.equal(xg.cpu(), x)
    if relu:
        assert (got >= 0).all() and (got.cpu()[r64 > 1e-4] > 0).all()
    else:
        assert (got < 0).any()
    _bound(_nerr(got, r64), _nerr(aten, r64), "K19 %s relu %s" % (shape, relu))


@pytest.mark.parametrize("shape", K19_SHAPES)
def test_k19_exact_on_integer_data(core, dev, shape):
    """Small integers in x, w and bias: every product and partial sum is exact in fp32 in any order, so the result equals
    the float64 one bit for bit, and any difference is an indexing or padding error."""
    B, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(7 + H)
    x = torch.randint(-8, 9, (B, Cin, H, W), generator=g).float()
    w = torch.randint(-8, 9, (Cout, Cin, 3, 3), generator=g).float()
    bias = torch.randint(-64, 65, (Cout,), generator=g).float()
    ref = F.conv2d(x.double(), w.double(), bias.double(), 2, 1).permute(0, 2, 3, 1)
    for relu in (False, True):
        got = core.conv3x3s2_nhwc(x.to(dev), w.permute(1, 2, 3, 0).contiguous().to(dev), bias.to(dev), relu=relu).cpu()
        assert torch.equal(got.double(), F.relu(ref) if relu else ref), relu


def test_k19_batch_invariance_and_nan(core, dev):
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(3, 3, 3, 32, generator=g) / 5).to(dev)
    b = torch.randn(32, generator=g).to(dev)
    x = torch.randn(3, 3, 35, 37, generator=g).to(dev)
    full = core.conv3x3s2_nhwc(x, w, b, relu=True)
    for i in range(3):
        assert torch.equal(core.conv3x3s2_nhwc(x[i:i + 1].contiguous(), w, b, relu=True)[0], full[i]), i
    x[1, 0, 4, 4] = float("nan")                                           # relu1 keeps a NaN
    y = core.conv3x3s2_nhwc(x, w, b, relu=True)
    assert torch.isnan(y[1, 2, 2]).all() and not torch.isnan(y[0]).any() and not torch.isnan(y[1, 5, 5]).any()


# ---- 2. K20 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 9, 11, 32), (1, 2, 2, 4), (3, 56, 56, 64), (1, 1, 5, 8)])
def test_k20_is_avg_pool2d_bit_for_bit(core, dev, shape):
    """(1, 1, 5, 8): one row pools to an empty [1, 0, 2, 8] output, accepted (the entry launches nothing), as torch's
    own AvgPool2d gives it."""
    B, H, W, C = shape
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W)) * 3
    ref = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) if H >= 2 and W >= 2 else x.new_zeros(B, H // 2, W // 2, C)
    xg = x.to(dev)
    got = core.avgpool2_nhwc(xg)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, H // 2, W // 2, C) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref.contiguous()) and torch.equal(xg.cpu(), x)
    if got.numel():                                                        # and ATen's own GPU pooling of NHWC memory
        assert torch.equal(got, F.avg_pool2d(xg.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


def test_k20_batch_invariance(core, dev):
    x = torch.randn(3, 9, 11, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    full = core.avgpool2_nhwc(x)
    assert torch.equal(core.avgpool2_nhwc(x[:1].contiguous())[0], full[0])
    assert torch.equal(core.avgpool2_nhwc(x[2:].contiguous())[0], full[2])


# ---- 3. K21 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 49, 2048), (2, 1, 64), (5, 4, 128)])
def test_k21_tokens(core, dev, shape):
    B, HW, C = shape
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(B, HW, C, generator=g) + 0.5                           # a mean that is not near zero
    pos = torch.randn(HW + 1, C, generator=g) / C ** 0.5
    xg, pg = x.to(dev), pos.to(dev)
    tok = core.attnpool_tokens(xg, pg)
    torch.cuda.synchronize()
    assert tuple(tok.shape) == (B, HW + 1, C) and tok.is_contiguous()
    assert torch.equal(tok[:, 1:].cpu(), x + pos[1:])                      # one fp32 add: torch's bits
    r64 = x.double().mean(dim=1) + pos[0].double()
    _bound(_nerr(tok[:, 0], r64), _nerr(xg.mean(dim=1) + pg[0], r64), "K21 row 0 %s" % (shape,))
    assert torch.equal(xg.cpu(), x) and torch.equal(pg.cpu(), pos)
    # a 4-D channels-last-memory input is the same call
    if HW == 49:
        assert torch.equal(core.attnpool_tokens(xg.view(B, 7, 7, C), pg), tok)
    for i in (0, B - 1):                                                   # batch invariance, bit for bit
        assert torch.equal(core.attnpool_tokens(xg[i:i + 1].contiguous(), pg)[0], tok[i]), i


def test_wrappers_reject_bad_tensors(core, dev):
    x = torch.randn(2, 3, 8, 8, device=dev)
    w, b = torch.randn(3, 3, 3, 32, device=dev), torch.zeros(32, device=dev)
    with pytest.raises(ValueError):
        core.conv3x3s2_nhwc(x, torch.randn(3, 3, 3, 30, device=dev), torch.zeros(30, device=dev))
    with pytest.raises(ValueError):
        core.conv3x3s2_nhwc(torch.randn(2, 5, 8, 8, device=dev), torch.randn(5, 3, 3, 32, device=dev), b)
    with pytest.raises(TypeError):
        core.conv3x3s2_nhwc(x.double(), w, b)
    with pytest.raises(TypeError):
        core.conv3x3s2_nhwc(x, w, torch.zeros(31, device=dev))
    with pytest.raises(ValueError):
        core.avgpool2_nhwc(torch.randn(1, 4, 4, 6, device=dev))
    with pytest.raises(TypeError):
        core.avgpool2_nhwc(torch.randn(1, 4, 4, 8, device=dev).permute(0, 2, 1, 3)[:, :, :3])
    with pytest.raises(ValueError):
        core.avgpool2_nhwc(torch.zeros(4 * 4 * 8 + 1, device=dev)[1:].view(1, 4, 4, 8))      # 4-byte aligned
    with pytest.raises(TypeError):
        core.attnpool_tokens(torch.randn(2, 4, 64, device=dev), torch.randn(4, 64, device=dev))
    with pytest.raises(ValueError):
        core.attnpool_tokens(torch.randn(2, 4, 62, device=dev), torch.randn(5, 62, device=dev))


# ---- 4. the attention pool ----------------------------------------------------------------------------------------------
def _mha64(pool, x):
    """The reference's computation in float64 on the host: F.multi_head_attention_forward over (HW+1) N C with separate
    projection weights, read at token 0."""
    p = {k: v.detach().double().cpu() for k, v in pool.state_dict().items()}
    t = x.double().cpu().flatten(2).permute(2, 0, 1)
    t = torch.cat([t.mean(dim=0, keepdim=True), t], dim=0) + p["positional_embedding"][:, None, :]
    out, _ = F.multi_head_attention_forward(
        t, t, t, t.shape[-1], pool.num_heads, None, torch.cat([p["q_proj.bias"], p["k_proj.bias"], p["v_proj.bias"]]),
        None, None, False, 0.0, p["c_proj.weight"], p["c_proj.bias"], training=False, need_weights=False,
        use_separate_proj_weight=True, q_proj_weight=p["q_proj.weight"], k_proj_weight=p["k_proj.weight"],
        v_proj_weight=p["v_proj.weight"])
    return out[0]


@pytest.mark.parametrize("embed,heads,side,out", [(128, 2, 3, 40), (2048, 32, 7, 1024)])
def test_attention_pool_against_float64(du, core, dev, monkeypatch, embed, heads, side, out):
    g = torch.Generator().manual_seed(embed)
    pool = du.AttentionPool2d(side, embed, heads, out).eval()
    with torch.no_grad():
        for p in pool.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
        x = F.relu(torch.randn(3, embed, side, side, generator=g))         # layer4's output is behind a ReLU
        ref = _mha64(pool, x)
        pool.to(dev)
        xg = x.to(dev).contiguous(memory_format=torch.channels_last)
        x0 = xg.clone()
        cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
        monkeypatch.setattr(du, "HIP_CLIP_RN", False)
        aten = pool(xg)
        assert cnt.n == {}
        monkeypatch.setattr(du, "HIP_CLIP_RN", True)
        assert du.clip_rn_route(pool, xg) == "hip"
        got = pool(xg)
        torch.cuda.synchronize()
    assert cnt.n == {"attnpool_tokens": 1, "vit_attention_cls": 1, "linear_residual": 3} and cnt.relu_gemms == 0
    assert tuple(got.shape) == (3, out) == tuple(ref.shape) and torch.equal(xg, x0)
    assert float(ref.abs().max()) > 1e-2
    _bound(_nerr(got, ref), _nerr(aten, ref), "attention pool %d / %d heads / %dx%d" % (embed, heads, side, side))


# ---- 5. the block -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,width,stride,hw", [(64, 64, 1, (16, 16)), (256, 128, 2, (16, 16)), (256, 128, 2, (7, 9))])
def test_bottleneck_against_float64(du, core, dev, monkeypatch, cin, width, stride, hw):
    torch.manual_seed(cin + stride)
    blk = du._ClipBottleneck(cin, width, stride)
    _mild_bn(blk, 3)
    blk.eval()
    x = F.relu(torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(hw[0])))
    with torch.no_grad():
        ref = blk.double()(x.double())
        blk.float().to(dev)
        xg = x.to(dev).contiguous(memory_format=torch.channels_last)
        x0 = xg.clone()
        cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
        assert du.clip_rn_route(blk, xg) == "hip"
        got = blk(xg)
        assert cnt.n == {"conv_igemm_nhwc": 1, "linear_residual": 3, **({"avgpool2_nhwc": 2} if stride == 2 else {})}
        assert cnt.relu_gemms == 1 and torch.equal(xg, x0)
        monkeypatch.setattr(du, "HIP_CLIP_RN", False)
        aten = blk(x.to(dev))
        monkeypatch.setattr(du, "HIP_CLIP_RN", True)
    assert tuple(got.shape) == (2, width * 4, hw[0] // stride, hw[1] // stride) == tuple(ref.shape)
    assert got.is_contiguous(memory_format=torch.channels_last) and (got >= 0).all() and (got == 0).any()
    _bound(_nerr(got, ref), _nerr(aten, ref), "clip bottleneck %d -> %d * 4 / %d at %s" % (cin, width, stride, hw))


# ---- 6. towers ----------------------------------------------------------------------------------------------------------
def _hooked(net, xin):
    """(embedding, {hook point: float64 spatial mean on the host}) of one forward."""
    outs = {}

    def keep(n):
        def hook(m, i, o):
            o = o.detach().double().cpu()
            outs[n] = o.mean(dim=[2, 3]) if o.dim() == 4 else o
        return hook
    hs = [getattr(net, n).register_forward_hook(keep(n)) for n in LAYERS]
    with torch.no_grad():
        y = net(xin)
    for h in hs:
        h.remove()
    return y, outs


def _tower_counts(layers, hooked_blocks=0, hooked_stride2=0):
    """The wrapper calls of one HIP-route forward of a ModifiedResNet with `layers` blocks per stage (every stage's first
    block has a downsample; stages 2-4 start with a stride-2 block); hooked_blocks of them (hooked_stride2 of stride 2,
    with a downsample) on ATen."""
    blocks = sum(layers) - hooked_blocks
    down = 4 - hooked_stride2
    n = {"conv3x3s2_nhwc": 1, "conv_igemm_nhwc": 2 + blocks, "avgpool2_nhwc": 1 + 2 * (3 - hooked_stride2),
         "attnpool_tokens": 1, "vit_attention_cls": 1, "linear_residual": 2 * blocks + down + 3}
    return n, blocks


def _check_tower(du, core, dev, monkeypatch, net, x, layers, what, hook_block=True):
    ref, ref_outs = _hooked(net.double(), x.double())
    net.float().to(dev)
    keys = list(net.state_dict().keys())
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    monkeypatch.setattr(du, "HIP_CLIP_RN", False)                      # toggled through the module attribute
    aten, aten_outs = _hooked(net, x.to(dev))
    assert cnt.n == {} and cnt.relu_gemms == 0                          # the flag off: no kernel of the route is called
    monkeypatch.setattr(du, "HIP_CLIP_RN", True)
    xg = x.to(dev)
    got, got_outs = _hooked(net, xg)
    assert (cnt.n, cnt.relu_gemms) == _tower_counts(layers)
    assert torch.equal(xg, x.to(dev)) and list(net.state_dict().keys()) == keys
    for n in LAYERS:
        assert got_outs[n].shape == ref_outs[n].shape and float(ref_outs[n].abs().max()) > 1e-3
        _bound(_nerr(got_outs[n], ref_outs[n]), _nerr(aten_outs[n], ref_outs[n]), "%s %s mean" % (what, n))
    _bound(_nerr(got, ref), _nerr(aten, ref), "%s embedding" % what)
    assert torch.equal(got.double().cpu(), got_outs["attnpool"])       # the hook on attnpool sees the embedding
    y2, outs2 = _hooked(net, xg)                                        # the same forward twice: the same bits
    assert torch.equal(y2, got) and all(torch.equal(outs2[n], got_outs[n]) for n in LAYERS)
    if not hook_block:
        return
    # a hook on layer2[0].conv2: that one block takes ATen, the hook fires once, the outputs agree
    seen = []
    h = net.layer2[0].conv2.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    cnt.n.clear()
    cnt.relu_gemms = 0
    y3, outs3 = _hooked(net, xg)
    h.remove()
    assert len(seen) == 1 and seen[0][1] == net.layer2[0].conv2.out_channels
    assert (cnt.n, cnt.relu_gemms) == _tower_counts(layers, 1, 1)
    for n in LAYERS:
        _bound(_nerr(outs3[n], ref_outs[n]), _nerr(aten_outs[n], ref_outs[n]), "%s %s mean, one block on ATen" % (what, n))
    _bound(_nerr(y3, ref), _nerr(aten, ref), "%s embedding, one block on ATen" % what)


def test_small_tower_against_float64_and_the_reference(du, core, dev, monkeypatch):
    """The fixture's configuration on the recipe weights: the float64 CPU forward of the mirror is the reference here, and
    it is itself the reference implementation's float64 output (tests/golden/clip_rn.npz) to 1e-12."""
    z = np.load(os.path.join(util.GOLDEN, "clip_rn.npz"))
    meta = json.load(open(os.path.join(util.GOLDEN, "clip_rn_meta.json")))
    net = du.ModifiedResNet(**recipe.SMALL).eval()
    assert recipe.fill(net) == meta["weights_sha256"]
    x = recipe.make_input()
    with torch.no_grad():
        y64 = net.double()(x.double())
    assert _nerr(y64, torch.from_numpy(z["y_f64"])) <= 1e-12
    _check_tower(du, core, dev, monkeypatch, net, x, recipe.SMALL["layers"], "small tower")
    with torch.no_grad():
        got = net(x.to(dev))
    _bound(_nerr(got, torch.from_numpy(z["y_f64"])), _nerr(torch.from_numpy(z["y_f32"]), torch.from_numpy(z["y_f64"])),
           "small tower against the reference's float64 output")


def test_rn50_against_float64_and_routing(du, core, dev, monkeypatch):
    model, _ = du.get_target_model("clip_rn50", "cpu")
    net = model.visual
    _mild_bn(net, 2)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    _check_tower(du, core, dev, monkeypatch, net, x, (3, 4, 6, 3), "RN50")
    with torch.no_grad():
        e = model.to(dev).encode_image(x.to(dev))
    assert tuple(e.shape) == (2, 1024) and bool(torch.isfinite(e).all())


# ---- 7. the driver ------------------------------------------------------------------------------------------------------
def _words():
    with open(CONCEPTS) as f:
        return f.read().split("\n")


def _run_driver(dev, tmp, tag, clip_model, layers, fn="soft_wpmi"):
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons as drv
    act, res = os.path.join(tmp, "acts_" + tag), os.path.join(tmp, "results_" + tag)
    out = drv.main(["--clip_model", clip_model, "--target_model", "clip", "--target_layers", ",".join(layers),
                    "--d_probe", "synthetic_128_224", "--concept_set", CONCEPTS, "--batch_size", "64", "--device", str(dev),
                    "--similarity_fn", fn, "--activation_dir", act, "--result_dir", res])
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    return act, csvs[0]


def _check_csv_against_oracle(csv_path, act, layers, oracle, clip_suffix, top_k, words):
    """tests/test_gpu_pipeline.py's _check_csv_against_oracle (the rules test_gpu_configs.py applies) for the 'clip' variant
    and a dissector whose cache files end in `clip_suffix`: images exact, every similarity within 1e-4 of the oracle's on
    the driver's own cache files, every decided rank the oracle's, and more than half of the ranks decided."""
    df = pd.read_csv(csv_path)
    assert list(df.columns) == ["layer", "unit", "description", "similarity", "images"]
    files = glob.glob(act + "/**/*.pt", recursive=True)
    clip_f = [f for f in files if f.endswith("_%s.pt" % clip_suffix) and "Specific_concepts" not in f]
    text_f = [f for f in files if "Specific_concepts" in f and f.endswith("_%s.pt" % clip_suffix)]
    assert len(clip_f) == 1 and len(text_f) == 1 and len(files) == len(layers) + 2
    E_img = torch.load(clip_f[0], weights_only=True).numpy()
    E_txt = torch.load(text_f[0], weights_only=True).numpy()
    n_decided = n_ranks = 0
    for layer in layers:
        tf = [f for f in files if f.endswith("_%s.pt" % layer)][0]
        A = torch.load(tf, weights_only=True).numpy()
        assert A.ndim == 2 and A.shape[0] == E_img.shape[0]
        ref = oracle.dissect_layer(E_img, E_txt, A, top_k=top_k, k_desc=1, blas=False)
        sub = df[df.layer == layer].reset_index(drop=True)
        assert len(sub) == A.shape[1] and sub.unit.tolist() == list(range(A.shape[1]))
        assert sub.images.tolist() == [str(r) for r in ref["top_ids"].T.astype(np.int64)]
        got_ids = np.array([[words.index(w)] for w in sub.description])
        got_sim = np.array([[float(t)] for t in sub.similarity], np.float32)
        srt = np.sort(ref["sim"], axis=1)[:, ::-1][:, :1]
        assert np.abs(got_sim.astype(np.float64) - srt).max() <= util.SIM_ATOL
        frac = util.assert_topk_ids(got_ids, None, ref["ids"], ref["sim"], 1, "clip %s" % layer)
        n_decided += frac * got_ids.size
        n_ranks += got_ids.size
    print("driver CSV against the oracle: %d of %d top-1 ranks decided" % (round(n_decided), n_ranks))
    assert n_decided > 0.5 * n_ranks, (n_decided, n_ranks)
    return E_img, E_txt


def _he_filled_rn50(du, monkeypatch):
    """The factory's seeded default init (PyTorch's, gain 1/3 per convolution) maps the synthetic noise images to RN50
    embeddings whose pairwise cosine is 0.9999994: every concept then scores within 2.4e-4 of the best and 0.4 % of the
    top-1 ranks are decided (measured with the oracle on the host), so a CSV check would pass on anything.  The driver
    therefore gets visual weights through the factory's own `ckpt=` path, as a local OpenAI checkpoint would come: the
    fixture recipe with He's gain sqrt(2) on the convolutions, under which the cosines are 0.95-0.98 and 93-98 % of the
    ranks are decided (same measurement)."""
    net = du.ModifiedResNet(**recipe.RN50)
    recipe.fill(net, recipe.SEED, conv_gain=2 ** 0.5)
    ckpt = {"visual." + k: v.clone() for k, v in net.state_dict().items()}
    real = du.get_target_model

    def filled(name, device, *args, **kw):
        if name == "clip_rn50" and kw.get("ckpt") is None:
            kw["ckpt"] = ckpt
        return real(name, device, *args, **kw)
    monkeypatch.setattr(du, "get_target_model", filled)
    return ckpt


def test_driver_with_clip_model_rn50(du, core, dev, oracle, tmp_path, monkeypatch):
    """describe_clip_neurons --clip_model RN50 --target_model clip: the dissector is the ClipResNet and it dissects itself
    (reference CLIP_og_utils.py:128-129) at visual.layer1, visual.layer4 and visual.attnpool.  The cache files carry RN50
    in their names and hold 1024-wide embeddings; the CSV is the oracle's on the driver's own cache files."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    _he_filled_rn50(du, monkeypatch)
    layers = ["visual.layer1", "visual.layer4", "visual.attnpool"]
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    act, csv = _run_driver(dev, str(tmp_path), "rn50", "RN50", layers)
    assert cnt.n.get("conv3x3s2_nhwc", 0) >= 2 and cnt.n.get("attnpool_tokens", 0) >= 2 and cnt.relu_gemms >= 32
    names = sorted(os.path.basename(f) for f in glob.glob(act + "/**/*.pt", recursive=True))
    assert names == sorted(["synthetic_128_224_RN50.pt", "Specific_concepts_sorted_RN50.pt"]
                           + ["synthetic_128_224_clip_%s.pt" % l for l in layers])
    E_img, E_txt = _check_csv_against_oracle(csv, act, layers, oracle, "RN50", 100, _words())
    assert E_img.shape == (128, 1024) and E_txt.shape[1] == 1024 and E_img.dtype == np.float32
    df = pd.read_csv(csv)
    assert [int((df.layer == l).sum()) for l in layers] == [256, 2048, 1024]
    # visual.attnpool's activations are the image embeddings themselves: one forward serves both
    A = torch.load(os.path.join(act, "synthetic_128_224_clip_visual.attnpool.pt"), weights_only=True).numpy()
    assert np.array_equal(A, E_img)


def test_driver_default_clip_model_is_unchanged(du, dev, tmp_path, monkeypatch):
    """--clip_model ViT-B/16 (the default) builds the ClipViT as before and none of this route's code runs for it: the
    CSV and the cache files are the same bytes with HIP_CLIP_RN on and off, and carry ViT-B16 in their names."""
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    layers = ["vision_model.encoder.layers[0]", "vision_model.encoder.layers[11]"]
    runs = {}
    for flag in (True, False):
        monkeypatch.setattr(du, "HIP_CLIP_RN", flag)
        act, csv = _run_driver(dev, str(tmp_path), "vit_%s" % flag, "ViT-B/16", layers)
        files = sorted(glob.glob(act + "/**/*.pt", recursive=True))
        runs[flag] = (open(csv, "rb").read(), [os.path.basename(f) for f in files],
                      [torch.load(f, weights_only=True) for f in files])
    assert runs[True][0] == runs[False][0] and len(runs[True][0]) > 10000
    assert runs[True][1] == runs[False][1] and "synthetic_128_224_ViT-B16.pt" in runs[True][1]
    assert all(torch.equal(a, b) for a, b in zip(runs[True][2], runs[False][2]))
    assert tuple(torch.load(os.path.join(act, "synthetic_128_224_ViT-B16.pt"), weights_only=True).shape) == (128, 512)
