"""GPU: the HF ViT / DINOv2 targets (`vit`, `dino`) on the HIP tower route -- K11 at even patch sizes that are not
multiples of 4 (14 for DINOv2), K9L where the last query block is ragged (257 tokens: one live query), a DINOv2-style
block (eps 1e-6, LayerScale folded into the residual GEMMs), the small towers of the transformers fixture
(tests/golden/vit_family.npz), the kernels each tower really runs, and the driver on `--target_model dino`.

The bound is the project's (test_gpu_clip_rn._bound): normalised error max|got - ref| / max|ref| against float64 at most
twice that of the fp32 ATen side on the same inputs, plus 1e-6.  K11 is a permutation: torch.equal."""
import glob
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import util
import vit_family_recipe as recipe
from test_gpu_attention_long import _attention
from test_gpu_clip_rn import _bound, _check_csv_against_oracle, _words
from test_vit_family_cpu import cls_rows, small_mirror
from util import nerr as _nerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")
WRAPPERS = ("patchify", "layer_norm", "vit_attention", "vit_attention_long", "vit_attention_cls")
ATEN_FLAGS = ("HIP_ATTENTION", "FUSED_RESIDUAL", "HIP_LAYER_NORM")
GUARD = 4096                      # floats in front of and behind a guarded output


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    assert core.linear_residual_available(), "libmcd_blaslt.so did not load"
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "vit_family.npz")), json.load(open(os.path.join(util.GOLDEN, "vit_family_meta.json")))


def _counter(core, monkeypatch):
    """util.CallCounter on this route's wrappers, plus n['linear_residual']."""
    cnt = util.CallCounter(core, monkeypatch, WRAPPERS)
    lr = core.linear_residual

    def lin(*a, **kw):
        cnt.n["linear_residual"] = cnt.n.get("linear_residual", 0) + 1
        return lr(*a, **kw)
    monkeypatch.setattr(core, "linear_residual", lin)
    return cnt


# ---- 1. K11 -------------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, P): DINOv2's patch on a non-square grid; the smallest call there is; one patch per image; P = 6.  The last
# one is a P % 4 == 0 shape, which keeps the 16-byte kernel.
K11_SHAPES = [(2, 3, 28, 42, 14), (1, 1, 2, 2, 2), (3, 3, 14, 14, 14), (1, 3, 12, 18, 6), (2, 3, 32, 48, 16)]


@pytest.mark.parametrize("shape", K11_SHAPES)
def test_k11_even_patch_sizes(core, mcd, dev, shape):
    """Bit-equal to the view / permute operand of test_patchify_is_the_conv_operand, with a zero class-token row, into a
    pre-filled output with guards on both sides: nothing but the output is written, all of it is."""
    B, Cin, H, W, P = shape
    x = torch.randn(B, Cin, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(H + P))
    x0 = x.clone()
    nH, nW = H // P, W // P
    ref = x.view(B, Cin, nH, P, nW, P).permute(0, 2, 4, 1, 3, 5).reshape(B, nH * nW, Cin * P * P)
    want = torch.cat([torch.zeros(B, 1, Cin * P * P, device=dev), ref], dim=1)
    got = core.patchify(x, P)
    assert got.shape == (B, 1 + nH * nW, Cin * P * P) and got.is_contiguous()
    assert torch.equal(got[:, 1:], ref) and float(got[:, 0].abs().max()) == 0.0
    flat, view, spec = util.framed_dense(tuple(want.shape), 0, GUARD, util.OUT_FILL, torch.float32, dev)
    assert mcd._lib.load().mcd_patchify(x.data_ptr(), B, Cin, H, W, P, view.data_ptr(), None) == 0
    torch.cuda.synchronize()
    util.check_frame(flat, spec, want, what="K11 %s" % (shape,))
    assert torch.equal(x, x0)


def test_k11_refuses_an_odd_patch(core, mcd, dev):
    x = torch.randn(1, 3, 14, 14, device=dev)
    for P in (7, 1):
        with pytest.raises(mcd._lib.McdError) as e:
            core.patchify(x, P)
        assert e.value.code == mcd._lib.MCD_E_UNSUPPORTED and "bad shape" in str(e.value)


# ---- 2. K9L with a ragged last query block --------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [257, 289, 300])
def test_k9l_ragged_last_block(core, dev, T):
    """(B, H) = (2, 2).  The second query block of every (image, head) holds 1 query (257: seven of its eight compute
    waves own none), 33 (289: two live waves, the second with one query) or 44 (300: a partial second wave).  Against
    float64 with test_long_attention_matches_float64's bound, into a guarded output: every row is written, nothing
    beside them is, and an image's rows do not depend on the batch it sits in."""
    B, H = 2, 2
    g = torch.Generator(device=dev).manual_seed(T)
    for scale in (1.0, 6.0):
        qkv = torch.randn(B, T, 3 * H * 64, device=dev, generator=g) * scale
        flat, view, spec = util.framed_dense((B, T, H * 64), 0, GUARD, util.OUT_FILL, torch.float32, dev)
        assert core.vit_attention_long(qkv, H, out=view) is view
        torch.cuda.synchronize()
        ref = _attention(qkv, H, torch.float64)
        err = (view.double() - ref).abs().max().item()
        err32 = (_attention(qkv, H, torch.float32).double() - ref).abs().max().item()
        print("K9L T=%d scale %g: err %.3e err32 %.3e" % (T, scale, err, err32))
        assert err <= 3e-6 * max(1.0, ref.abs().max().item()) + 3 * err32, (T, scale, err, err32)
        assert not (view == util.OUT_FILL).any()
        util.check_frame(flat, spec, view.clone(), what="K9L T=%d" % T)     # the guards kept their fill
        assert torch.equal(core.vit_attention_long(qkv, H), view)
        # the second image alone: its workgroups sit elsewhere in the grid, its rows keep their bits
        assert torch.equal(core.vit_attention_long(qkv[1:].contiguous(), H), view[1:])


# ---- 3. a DINOv2-style block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [26, 257])
def test_dinov2_block_against_float64(du, core, dev, monkeypatch, T):
    """eps 1e-6 and random LayerScales: the HIP route (K10, the fused GEMMs with lambda folded into proj and fc2, K9 at 26
    tokens, K9L at 257) against the float64 host forward, relative to the ATen route of the same module."""
    g = torch.Generator().manual_seed(T)
    blk = du._Block(128, 2, 512, eps=1e-6, layer_scale=1.0).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / max(1, p.shape[-1]) ** 0.5)
        for m in (blk.norm1, blk.norm2):
            m.weight.copy_(1 + 0.2 * torch.randn(128, generator=g))
            m.bias.copy_(0.1 * torch.randn(128, generator=g))
        blk.layer_scale1.lambda1.copy_(1 + 0.3 * torch.randn(128, generator=g))
        blk.layer_scale2.lambda1.copy_(1 + 0.3 * torch.randn(128, generator=g))
        x = torch.randn(2, T, 128, generator=g)
        ref = blk.double()(x.double())
        blk.float().to(dev)
        xg = x.to(dev)
        keys = list(blk.state_dict())
        cnt = _counter(core, monkeypatch)
        for f in ATEN_FLAGS:
            monkeypatch.setattr(du, f, False)
        aten = blk(xg)
        assert cnt.n == {}
        for f in ATEN_FLAGS:
            monkeypatch.setattr(du, f, True)
        got = blk(xg)
        torch.cuda.synchronize()
    attn = "vit_attention" if T <= 256 else "vit_attention_long"
    assert cnt.n == {"layer_norm": 2, attn: 1, "linear_residual": 4}
    assert torch.equal(xg.cpu(), x) and list(blk.state_dict()) == keys
    _bound(_nerr(got, ref), _nerr(aten, ref), "DINOv2-style block at %d tokens" % T)
    # without lambda the answer is another one: the bound would catch a dropped fold
    with torch.no_grad():
        blk.layer_scale1.lambda1.fill_(1.0)
        assert _nerr(blk(xg), ref) > 1e-3


def test_hook_inside_a_block_fires_and_the_other_block_stays_on_hip(du, core, dev, monkeypatch):
    """--target_layers may name any module path.  A forward hook on encoder.layer[0].attn.proj, .attn.qkv or .fc1 of a
    two-block tower (dim 128, 2 heads, 32 x 32 images at patch 16: 5 tokens): block 0 calls its modules, so the hook fires
    once with that module's output; block 1 keeps the HIP route (its four GEMMs on top of the embedding's, its K9 launch);
    the tower's output stays within the bound of the unhooked one; with the hook removed the counts are the plain ones."""
    g = torch.Generator().manual_seed(11)
    tower = du.ViTTower(image_size=32, patch=16, dim=128, depth=2, heads=2, mlp=512).eval()
    with torch.no_grad():
        for p in tower.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / max(1, p.shape[-1]) ** 0.5)
        for m in tower.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1 + 0.2 * torch.randn(128, generator=g))
        x = torch.randn(2, 3, 32, 32, generator=g)
        ref = tower.double()(x.double())
        tower.float().to(dev)
        xg = x.to(dev)
        cnt = _counter(core, monkeypatch)
        for f in ATEN_FLAGS:
            monkeypatch.setattr(du, f, False)
        aten = tower(xg)
        assert cnt.n == {}
        for f in ATEN_FLAGS:
            monkeypatch.setattr(du, f, True)
        plain = {"patchify": 1, "layer_norm": 5, "vit_attention": 2, "linear_residual": 1 + 2 * 4}
        got = tower(xg)
        assert cnt.n == plain, cnt.n
        _bound(_nerr(got, ref), _nerr(aten, ref), "two-block tower")
        for name, width in (("attn.proj", 128), ("attn.qkv", 384), ("fc1", 512)):
            seen = []
            h = tower.encoder.layer[0].get_submodule(name).register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
            cnt.n.clear()
            try:
                hooked = tower(xg)
            finally:
                h.remove()
            assert seen == [(2, 5, width)], (name, seen)
            # block 0 on its modules -- its two _LayerNorms and its _Attention still pick K10 and K9 for themselves, as
            # with FUSED_RESIDUAL off -- and no GEMM of the fused route; block 1 on the HIP route: K9 and four GEMMs
            assert cnt.n == dict(plain, linear_residual=1 + 4), (name, cnt.n)
            _bound(_nerr(hooked, ref), _nerr(aten, ref), "two-block tower, a hook on layer[0].%s" % name)
            cnt.n.clear()
            assert torch.equal(tower(xg), got) and cnt.n == plain, (name, cnt.n)
    assert torch.equal(xg.cpu(), x)


# ---- 4. the small towers against transformers' output -----------------------------------------------------------------------
def _expected_calls(case, depth=2):
    T = 1 + (recipe.CASES[case][1] // 14) * (recipe.CASES[case][2] // 14) if case != "vit" else 17
    attn = "vit_attention" if T <= 256 else "vit_attention_long"
    # patchify; norm1 / norm2 per block + the final norm; qkv, proj, fc1, fc2 per block + the embedding + the classifier
    return {"patchify": 1, "layer_norm": 2 * depth + 1, attn: depth, "linear_residual": 4 * depth + 2}


@pytest.mark.parametrize("case", sorted(recipe.CASES))
def test_small_tower_on_the_hip_route_matches_the_fixture(du, core, dev, monkeypatch, fixture, case):
    """The fixture's configuration on the recipe's weights, loaded through the checkpoint loader: the logits and every
    layer's class-token row against transformers' float64 output, relative to transformers' own fp32 error.  K11 runs
    for patch 14 as for 16, K9L at 257 tokens, K9 below; the same forward twice gives the same bits."""
    z, meta = fixture
    name, H, W = recipe.CASES[case]
    net, sha = small_mirror(du, name)
    assert sha == meta["configs"][name]["weights_sha256"]
    net.to(dev)
    x = recipe.make_input(case).to(dev)
    y64, c64 = torch.from_numpy(z["logits_f64_" + case]), torch.from_numpy(z["cls_f64_" + case])
    y32, c32 = torch.from_numpy(z["logits_f32_" + case]), torch.from_numpy(z["cls_f32_" + case])
    cnt = _counter(core, monkeypatch)
    y, c = cls_rows(net, x)                                                # plain hooks: every block runs whole
    torch.cuda.synchronize()
    assert cnt.n == _expected_calls(case), cnt.n
    assert tuple(y.shape) == tuple(y64.shape) and tuple(c.shape) == tuple(c64.shape)
    _bound(_nerr(y, y64), _nerr(y32, y64), "%s logits" % case)
    for i in range(c64.shape[0]):
        _bound(_nerr(c[i], c64[i]), _nerr(c32[i], c64[i]), "%s layer %d class-token row" % (case, i))
    y2, c2 = cls_rows(net, x)
    assert torch.equal(y2, y) and torch.equal(c2, c)
    assert torch.equal(x.cpu(), recipe.make_input(case))


@pytest.mark.parametrize("case", ["vit", "dino224"])
def test_class_token_tail_vit_only(du, core, dev, monkeypatch, fixture, case):
    """With the dissection's own hooks (utils.get_activation: token 0 readers) on every layer, `vit` prunes its last block
    to the class token -- K9C once, K9 for the block in front of it -- and `dino`, whose classifier reads the mean of the
    patch tokens, never does.  The hooked activations and the logits are still the fixture's."""
    from mammo_clip_dissect_amd.concept_vit import utils
    z, _ = fixture
    name, H, W = recipe.CASES[case]
    net, _ = small_mirror(du, name)
    net.to(dev)
    x = recipe.make_input(case).to(dev)
    acts = [[] for _ in range(2)]
    hs = [b.register_forward_hook(utils.get_activation(acts[i], "avg")) for i, b in enumerate(net.tower.encoder.layer)]
    cnt = _counter(core, monkeypatch)
    with torch.no_grad():
        y = net(x)
    torch.cuda.synchronize()
    for h in hs:
        h.remove()
    want = _expected_calls(case)
    if case == "vit":
        # the last block: K|V and q as two GEMMs instead of one qkv (+1), K9C instead of K9
        want.update({"vit_attention": 1, "vit_attention_cls": 1, "linear_residual": want["linear_residual"] + 1})
    assert cnt.n == want, cnt.n
    y64, c64 = torch.from_numpy(z["logits_f64_" + case]), torch.from_numpy(z["cls_f64_" + case])
    y32, c32 = torch.from_numpy(z["logits_f32_" + case]), torch.from_numpy(z["cls_f32_" + case])
    _bound(_nerr(y, y64), _nerr(y32, y64), "%s logits, hooked" % case)
    for i in range(2):
        assert len(acts[i]) == 1 and tuple(acts[i][0].shape) == (recipe.BATCH, 128)
        _bound(_nerr(acts[i][0], c64[i]), _nerr(c32[i], c64[i]), "%s layer %d activation" % (case, i))


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------
class _WpmiOracle:
    """The oracle with wpmi as dissect_layer's similarity function: 64 images are fewer than the top_k = 100 soft_wpmi
    selects (torch.topk raises there, in the reference as here), so the driver runs --similarity_fn wpmi (top_k 28)."""

    def __init__(self, oracle):
        self.oracle = oracle

    def dissect_layer(self, *a, **kw):
        return self.oracle.dissect_layer(*a, similarity_fn="wpmi", **kw)


def test_driver_with_target_model_dino(du, core, dev, oracle, tmp_path, monkeypatch):
    """describe_clip_neurons --target_model dino at dinov2.encoder.layer[0] and [11], 64 synthetic 224 x 224 images (257
    tokens: K11 at patch 14 and K9L in every block): the CSV is the oracle's on the run's own cache files."""
    from mammo_clip_dissect_amd.concept_vit import describe_clip_neurons as drv
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    layers = ["dinov2.encoder.layer[0]", "dinov2.encoder.layer[11]"]
    act, res = str(tmp_path / "acts"), str(tmp_path / "results")
    cnt = _counter(core, monkeypatch)
    out = drv.main(["--target_model", "dino", "--target_layers", ",".join(layers), "--d_probe", "synthetic_64_224",
                    "--concept_set", CONCEPTS, "--batch_size", "32", "--device", str(dev), "--similarity_fn", "wpmi",
                    "--activation_dir", act, "--result_dir", res])
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    # two batches and the one-image width probe of the 12-block dino tower, K9L in every block (the dissector's 197
    # tokens go to K9 and K9C); K11 for the dissector's patch 16 and for dino's patch 14
    assert cnt.n.get("vit_attention_long", 0) == 36 and cnt.n.get("patchify", 0) >= 5, cnt.n
    names = sorted(os.path.basename(f) for f in glob.glob(act + "/**/*.pt", recursive=True))
    assert names == sorted(["synthetic_64_224_ViT-B16.pt", "Specific_concepts_sorted_ViT-B16.pt"]
                           + ["synthetic_64_224_dino_%s.pt" % l for l in layers])
    E_img, E_txt = _check_csv_against_oracle(csvs[0], act, layers, _WpmiOracle(oracle), "ViT-B16", 28, _words())
    assert E_img.shape == (64, 512)
    df = pd.read_csv(csvs[0])
    assert [int((df.layer == l).sum()) for l in layers] == [768, 768]
