"""CPU: the one transformer-block sequence of the HIP route (data_utils._block_hip) wired to float64 torch stand-ins of
the core wrappers, for the three block classes that feed it -- _Block (DINOv2-style: eps 1e-6, LayerScale), _ClipResBlock
(causal and not) and _BertLayer (ragged key counts) -- against the same module's ATen forward; and the hook gate of _Block.

Both sides are float64 and differ in summation order only (a fused qkv projection instead of three, LayerScale folded into
the weights): the bound 1e-10 on max |got - ref| / max |ref| leaves several orders of magnitude over 128- and 512-term
float64 sums, and a swapped norm, a missing fold or a wrong activation misses it by eight."""
import pytest
import torch
import torch.nn.functional as F

from util import nerr

DIM, HEADS, MLP, B = 128, 2, 512, 3
BOUND = 1e-10


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _sdpa(qkv, heads, **kw):
    b, t, d3 = qkv.shape
    q, k, v = qkv.view(b, t, 3, heads, d3 // 3 // heads).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, **kw).transpose(1, 2).reshape(b, t, d3 // 3)


@pytest.fixture
def standins(mcd, monkeypatch):
    """The wrappers _block_hip calls, as torch on whatever dtype and device they are given; the list of calls made."""
    from mammo_clip_dissect_amd import core
    calls = []

    def linear_residual(res, h, weight, bias=None, out=None, relu=False):
        calls.append("linear_residual")
        y = h @ weight.T
        if bias is not None:
            y = y + bias
        if res is not None:
            y = res + y
        return y if out is None else out.copy_(y)

    def layer_norm(x, weight, bias, eps):
        calls.append("layer_norm")
        return F.layer_norm(x, x.shape[-1:], weight, bias, eps)

    def keylen(qkv, heads, lens, out=None):
        calls.append("vit_attention_keylen")
        t = qkv.shape[1]
        mask = None if lens is None else (torch.arange(t)[None, :] < lens.clamp(1, t)[:, None])[:, None, None, :]
        return _sdpa(qkv, heads, attn_mask=mask)

    def cls(q, k, v, out=None):
        calls.append("vit_attention_cls")
        b, t, heads, hd = k.shape
        o = F.scaled_dot_product_attention(q.reshape(b, heads, 1, hd), k.transpose(1, 2), v.transpose(1, 2))
        return o.reshape(b, heads * hd)

    def quick_gelu(x, out=None):
        calls.append("quick_gelu")
        y = x * torch.sigmoid(1.702 * x)
        return y if out is None else out.copy_(y)

    def plain(name, **kw):
        def f(qkv, heads, out=None):
            calls.append(name)
            return _sdpa(qkv, heads, **kw)
        return f
    for name, fn in (("linear_residual", linear_residual), ("layer_norm", layer_norm), ("vit_attention_keylen", keylen),
                     ("vit_attention_cls", cls), ("quick_gelu", quick_gelu), ("vit_attention", plain("vit_attention")),
                     ("vit_attention_long", plain("vit_attention_long")),
                     ("vit_attention_causal", plain("vit_attention_causal", is_causal=True)),
                     ("linear_residual_available", lambda: True)):
        monkeypatch.setattr(core, name, fn)
    return calls


def _fill(mod, seed):
    """Seeded float64 weights: every matrix at 1 / sqrt(fan-in), biases that are not zero, LayerNorms and LayerScales
    that are not the identity."""
    g = torch.Generator().manual_seed(seed)
    mod.double().eval()
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / max(1, p.shape[-1]) ** 0.5)
        for m in mod.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1 + 0.2 * torch.randn(DIM, generator=g, dtype=torch.float64))
                m.bias.copy_(0.1 * torch.randn(DIM, generator=g, dtype=torch.float64))
        for name, p in mod.named_parameters():
            if name.endswith("lambda1"):
                p.copy_(1 + 0.3 * torch.randn(DIM, generator=g, dtype=torch.float64))
    return mod


def _check(got, ref, what):
    e = nerr(got, ref)
    print("%s: %.3e" % (what, e))
    assert tuple(got.shape) == tuple(ref.shape) and e <= BOUND, (what, e)


@pytest.mark.parametrize("T", [5, 17])
def test_vit_block_on_the_shared_sequence(du, standins, monkeypatch, T):
    blk = _fill(du._Block(DIM, HEADS, MLP, eps=1e-6, layer_scale=1.0), T)
    keys = list(blk.state_dict())
    x = torch.randn(B, T, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(T + 1))
    x0 = x.clone()
    with torch.no_grad():
        mask = torch.ones(B, 1, 1, T, dtype=torch.bool)
        mask[1, ..., T - 2:] = False
        ref, ref_masked = blk(x), blk(x, mask)                             # CPU: the ATen forward
        assert standins == [] and nerr(ref_masked, ref) > 1e-3
        for attn in ("k9", "long", "sdpa"):
            _check(du._block_hip(blk._ops(), x, attn), ref, "_Block, %s, T=%d" % (attn, T))
        assert standins.count("layer_norm") == 6 and standins.count("linear_residual") == 12
        _check(du._block_hip(blk._ops(), x, "sdpa", k10=False), ref, "_Block, ATen LayerNorm, T=%d" % T)
        assert standins.count("layer_norm") == 6
        del standins[:]
        _check(du._block_hip(blk._ops(), x, "k9", cls_only=True), ref[:, :1], "_Block, row 0, T=%d" % T)
        assert standins == ["layer_norm", "linear_residual", "linear_residual", "vit_attention_cls", "linear_residual",
                            "layer_norm", "linear_residual", "linear_residual"]
        # the block's own dispatch, with the fused route's gate held open: the same operands, the same arguments
        monkeypatch.setattr(du, "_fused_residual_ok", lambda t: True)
        del standins[:]
        _check(blk(x), ref, "_Block.forward, T=%d" % T)
        assert standins == ["layer_norm", "linear_residual", "linear_residual", "layer_norm", "linear_residual", "linear_residual"]
        _check(blk(x, mask, cls_only=True), ref_masked, "_Block.forward, masked, T=%d" % T)
        _check(blk(x, cls_only=True), ref[:, :1], "_Block.forward, row 0, T=%d" % T)
        # without lambda the answer is another one
        blk.layer_scale1.lambda1.fill_(1.0)
        assert nerr(du._block_hip(blk._ops(), x, "k9"), ref) > 1e-3
    assert torch.equal(x, x0) and list(blk.state_dict()) == keys


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", [5, 17])
def test_clip_block_on_the_shared_sequence(du, standins, T, causal):
    blk = _fill(du._ClipResBlock(DIM, HEADS, causal=causal), 10 + T)
    keys = list(blk.state_dict())
    x = torch.randn(B, T, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(T + 2))
    x0 = x.clone()
    with torch.no_grad():
        ref = blk(x)
        assert standins == []
        attn = "causal" if causal else "k9"
        _check(du._block_hip(blk._ops(), x, attn, act=du._quick_gelu_), ref, "_ClipResBlock, %s, T=%d" % (attn, T))
        del standins[:]
        _check(blk(x, hip=True), ref, "_ClipResBlock.forward, %s, T=%d" % (attn, T))
        assert standins == ["layer_norm", "linear_residual", "vit_attention_causal" if causal else "vit_attention",
                            "linear_residual", "layer_norm", "linear_residual", "quick_gelu", "linear_residual"]
        if not causal:
            _check(du._block_hip(blk._ops(), x, "long", act=du._quick_gelu_), ref, "_ClipResBlock, long, T=%d" % T)
            _check(du._block_hip(blk._ops(), x, attn, act=du._quick_gelu_, cls_only=True), ref[:, :1],
                   "_ClipResBlock, row 0, T=%d" % T)
            del standins[:]
            _check(blk(x, hip=True, cls_only=True), ref[:, :1], "_ClipResBlock.forward, row 0, T=%d" % T)
            assert standins == ["layer_norm", "linear_residual", "linear_residual", "vit_attention_cls", "linear_residual",
                                "layer_norm", "linear_residual", "quick_gelu", "linear_residual"]
        assert nerr(du._block_hip(blk._ops(), x, attn), ref) > 1e-3         # erf GELU is another block
    assert torch.equal(x, x0) and list(blk.state_dict()) == keys


@pytest.mark.parametrize("T", [5, 17])
def test_bert_layer_on_the_shared_sequence(du, standins, T):
    layer = _fill(du._BertLayer(DIM, HEADS, MLP, 1e-12), 20 + T)
    keys = list(layer.state_dict())
    x = torch.randn(B, T, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(T + 3))
    x0 = x.clone()
    lens = torch.tensor([T, 1, T - 3], dtype=torch.int32)
    mask = (torch.arange(T)[None, :] < lens[:, None])[:, None, None, :]
    with torch.no_grad():
        for ln, m in ((lens, mask), (None, None)):
            ref = layer(x, m)
            del standins[:]
            _check(du._block_hip(layer._ops(), x, "keylen", ln, post=True), ref, "_BertLayer, lens %s, T=%d" % (ln, T))
            assert standins == ["linear_residual", "vit_attention_keylen", "linear_residual", "layer_norm", "linear_residual",
                                "linear_residual", "layer_norm"]
            _check(layer(x, m, ln, hip=True), ref, "_BertLayer.forward, lens %s, T=%d" % (ln, T))
        assert nerr(du._block_hip(layer._ops(), x, "keylen", lens), layer(x, mask)) > 1e-3     # pre-norm is another block
        assert nerr(du._block_hip(layer._ops(), x, "keylen", None, post=True), layer(x, mask)) > 1e-3      # the mask matters
    assert torch.equal(x, x0) and list(layer.state_dict()) == keys


def test_block_hook_gate(du):
    """_hooks_on(block, _BLOCK_SKIPPED): a forward hook or a pre-hook on any module inside a _Block sends it to its ATen
    modules; a hook on the block itself (what the dissector registers) does not."""
    plain, scaled = du._Block(DIM, HEADS, MLP), du._Block(DIM, HEADS, MLP, layer_scale=1.0)
    assert set(du._BLOCK_SKIPPED) == {"norm1", "attn", "norm2", "fc1", "fc2", "layer_scale1", "layer_scale2"}
    for blk in (plain, scaled):
        assert not du._hooks_on(blk, du._BLOCK_SKIPPED)
        targets = [blk.norm1, blk.attn, blk.attn.qkv, blk.attn.proj, blk.norm2, blk.fc1, blk.fc2]
        if blk.scaled:
            targets += [blk.layer_scale1, blk.layer_scale2]
        for m in targets:
            for pre in (False, True):
                h = m.register_forward_pre_hook(lambda m, i: None) if pre else m.register_forward_hook(lambda m, i, o: None)
                assert du._hooks_on(blk, du._BLOCK_SKIPPED), (m, pre)
                h.remove()
                assert not du._hooks_on(blk, du._BLOCK_SKIPPED)
        for h in (blk.register_forward_hook(lambda m, i, o: None), blk.register_forward_pre_hook(lambda m, i: None)):
            assert not du._hooks_on(blk, du._BLOCK_SKIPPED)
            h.remove()
        h = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
        try:
            assert du._hooks_on(blk, du._BLOCK_SKIPPED)
        finally:
            h.remove()
        assert not du._hooks_on(blk, du._BLOCK_SKIPPED)


@pytest.mark.parametrize("name", ["attn.proj", "attn.qkv", "fc1", "layer_scale2"])
def test_block_with_a_hook_inside_calls_its_modules(du, standins, monkeypatch, name):
    """With the fused route's gate held open, a hook inside the block still takes it to its ATen modules: the hook fires once
    with that module's own output, no wrapper is called, and the output is the ATen forward's to the bit."""
    blk = _fill(du._Block(DIM, HEADS, MLP, eps=1e-6, layer_scale=1.0), 7)
    x = torch.randn(B, 5, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        ref = blk(x)
        monkeypatch.setattr(du, "_fused_residual_ok", lambda t: True)
        monkeypatch.setattr(du, "HIP_LAYER_NORM", False)
        mod = blk.get_submodule(name)
        seen = []
        h = mod.register_forward_hook(lambda m, i, o: seen.append((i[0], o)))
        try:
            got = blk(x)
        finally:
            h.remove()
        assert standins == [] and torch.equal(got, ref)
        assert len(seen) == 1 and torch.equal(seen[0][1], mod(seen[0][0]))
        assert len(blk(x)) == B and standins != []                     # the hook gone: the shared sequence again
