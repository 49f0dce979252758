"""GPU: the class-token-only tail of the ViT towers -- K9C (mcd_vit_attention_cls) against float64 and against K9's
token-0 row, row-strided operands of core.linear_residual, the pruned last block against the full one, the GEMMs it
really runs, and the gate that keeps every other caller on the full path."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 197, 12), (2, 1, 2), (2, 5, 1), (2, 33, 2), (1, 256, 2), (1, 257, 2), (1, 5416, 2)]


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core as c
    assert c.linear_residual_available(), "libmcd_blaslt.so did not load"
    return c


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _operands(layout, B, T, H, scale, dev, g):
    """(q [B, H, 64], k, v [B, T, H, 64], qkv or None): views of one buffer in the given layout."""
    if layout == "qkv":
        qkv = torch.randn(B, T, 3, H, 64, device=dev, generator=g) * scale
        return qkv[:, 0, 0], qkv[:, :, 1], qkv[:, :, 2], qkv
    q = torch.randn(B, H * 64, device=dev, generator=g) * scale
    kv = torch.randn(B, T, 2, H, 64, device=dev, generator=g) * scale
    return q.view(B, H, 64), kv[:, :, 0], kv[:, :, 1], None


def _chain(q, k, v):
    s = torch.einsum("bhd,bthd->bht", q, k) / 8.0
    return torch.einsum("bht,bthd->bhd", torch.softmax(s, dim=-1), v).reshape(q.shape[0], -1)


@pytest.mark.parametrize("layout", ["split", "qkv"])
@pytest.mark.parametrize("shape", SHAPES)
def test_k9c_matches_float64(core, dev, shape, layout):
    """K9C against softmax(q k^T / 8) v in float64, from the [B, T, 2, H, 64] K|V layout (q apart) and from a plain
    [B, T, 3, H, 64] qkv through strides, at unit and at large score magnitudes (the online softmax must rescale).
    The bound is test_vit_attention_matches_sdpa's: 3e-6 * max(1, |ref|max) + 3 * (the error of the same chain in fp32
    torch); where K9 runs (T <= 256) its token-0 row is held to the same bound."""
    B, T, H = shape
    g = torch.Generator(device=dev).manual_seed(B * 1000 + T)
    for scale in (1.0, 6.0):
        q, k, v, qkv = _operands(layout, B, T, H, scale, dev, g)
        out = core.vit_attention_cls(q, k, v)
        assert out.shape == (B, H * 64)
        ref = _chain(q.double(), k.double(), v.double())
        err = (out.double() - ref).abs().max().item()
        err32 = (_chain(q, k, v).double() - ref).abs().max().item()
        bound = 3e-6 * max(1.0, ref.abs().max().item()) + 3 * err32
        print("K9C %s %s scale %g: err %.3e err32 %.3e bound %.3e" % (shape, layout, scale, err, err32, bound))
        assert err <= bound, (shape, layout, scale, err, err32)
        if qkv is not None and T <= core.VIT_ATTENTION_MAX_T:
            k9 = core.vit_attention(qkv.view(B, T, 3 * H * 64), H)[:, 0]
            d = (out.double() - k9.double()).abs().max().item()
            print("K9C %s against K9's token 0: %.3e" % (shape, d))
            assert d <= bound, (shape, scale, d, bound)


def test_k9c_rejects_bad_arguments(mcd, core, dev):
    """A misaligned pointer, T = 0 and T past the limit return an error and launch nothing (out keeps its bytes)."""
    L = mcd._lib.load()
    H, T = 2, 8
    W = H * 64
    buf = torch.randn(4 * T * 3 * W + 64, device=dev)
    out = torch.full((4, W), 7.0, device=dev)
    p, o = buf.data_ptr(), out.data_ptr()

    def call(q=p, k=p + 4 * W, v=p + 8 * W, T=T, row=3 * W, out=o):
        return L.mcd_vit_attention_cls(q, T * row, k, row, T * row, v, row, T * row, 4, T, H, out, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == 7.0).any()
    out.fill_(7.0)
    assert call(q=p + 4) == mcd._lib.MCD_E_ARG
    assert call(k=p + 4 * W + 8) == mcd._lib.MCD_E_ARG
    assert call(out=o + 4) == mcd._lib.MCD_E_ARG
    assert call(row=3 * W + 2) == mcd._lib.MCD_E_ARG          # rows that are not 16-byte aligned
    assert call(row=W - 4) == mcd._lib.MCD_E_ARG
    assert call(T=0) == mcd._lib.MCD_E_ARG
    assert call(T=core.VIT_ATTENTION_CLS_MAX_T + 1) == mcd._lib.MCD_E_UNSUPPORTED
    assert L.mcd_vit_attention_cls(None, W, p, W, W, p, W, W, 1, 1, H, o, None) == mcd._lib.MCD_E_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises((TypeError, ValueError)):
        core.vit_attention_cls(torch.zeros(2, H, 64, device=dev), torch.zeros(2, T, H, 60, device=dev),
                               torch.zeros(2, T, H, 60, device=dev))
    with pytest.raises(ValueError):
        core.vit_attention_cls(torch.zeros(3, H * 64, device=dev), torch.zeros(2, T, H, 64, device=dev),
                               torch.zeros(2, T, H, 64, device=dev))


@pytest.mark.parametrize("shape", [(40, 7, 768, 768), (64, 5, 768, 3072), (33, 3, 40, 100), (1, 4, 128, 64)])
def test_linear_residual_takes_strided_rows(core, dev, shape):
    """h (and res) as rows T*K (T*N) apart inside a larger tensor give what the contiguous call gives on the gathered
    rows, within test_linear_residual_matches_torch's 2e-5 * |ref|max; nothing is written outside out."""
    B, T, N, K = shape
    g = torch.Generator(device=dev).manual_seed(B + N)
    big_h = torch.randn(B, T, K, device=dev, generator=g)
    big_r = torch.randn(B, T, N, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.05
    b = torch.randn(N, device=dev, generator=g)
    keep_h, keep_r = big_h.clone(), big_r.clone()
    h, res = big_h[:, 0], big_r[:, 0]
    for hh, rr in ((h, None), (h, res), (h, res.contiguous()), (h.contiguous(), res)):
        ref = core.linear_residual(None if rr is None else rr.contiguous(), hh.contiguous(), W, b)
        out = core.linear_residual(rr, hh, W, b)
        assert out.shape == (B, N) and out.is_contiguous()
        err = (out - ref).abs().max().item()
        tol = 2e-5 * ref.abs().max().item()
        print("strided linear_residual %s h %s res %s: err %.3e tol %.3e"
              % (shape, tuple(hh.stride()), None if rr is None else tuple(rr.stride()), err, tol))
        assert err <= tol
    assert torch.equal(big_h, keep_h) and torch.equal(big_r, keep_r)
    with pytest.raises(TypeError):
        core.linear_residual(None, big_h[:, :, ::2][:, 0], W[:, :(K + 1) // 2].contiguous(), b)   # inner stride 2
    with pytest.raises(TypeError):
        core.linear_residual(None, big_h[:, ::2], W, b)       # 3-D with tokens 2K apart: not contiguous for any B


def _tower(du, dev, image_size, depth, seed):
    torch.manual_seed(seed)
    tower = du.ViTTower(image_size=image_size, depth=depth).to(dev).eval()
    for p in tower.parameters():
        torch.nn.init.normal_(p, std=0.05)
    return tower


def _dissect(mcd, du, dev, encode, blocks, x, flag):
    """encode(x) with a Dissector hook on every block, CLS_ONLY_TAIL = flag: (features, activation matrix [U, N])."""
    from mammo_clip_dissect_amd.pipeline import Dissector
    dis = Dissector(x.shape[0], ["b%d" % i for i in range(len(blocks))], [768] * len(blocks), 8, du.PROJ_DIM, dev)
    hs = [m.register_forward_hook(dis.hook(i)) for i, m in enumerate(blocks)]
    keep = du.CLS_ONLY_TAIL
    du.CLS_ONLY_TAIL = flag
    try:
        with torch.no_grad():
            f = encode(x).clone()
    finally:
        du.CLS_ONLY_TAIL = keep
        for h in hs:
            h.remove()
    return f, dis.At[:, :x.shape[0]].clone()


def _close(a, b):
    return (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("case", ["tower64", "tower320x224", "breastclip224"])
def test_pruned_tail_matches_the_full_tower(mcd, core, du, dev, case):
    """encode_image with the class-token tail on and off: the features and every hooked layer's activations agree within
    the tower tests' 1e-4 * max(1, |b|max), the layers before the last bit for bit.  320 x 224 is 281 tokens: K9L in
    the earlier blocks."""
    if case == "breastclip224":
        torch.manual_seed(3)
        model = du.BreastClip("vit", image_size=224, text_depth=1).to(dev).eval()
        tower, encode = model.image_encoder, model.encode_image
        x = torch.randn(5, 3, 224, 224, device=dev)
    else:
        size = 64 if case == "tower64" else (320, 224)
        tower = _tower(du, dev, size, 2, 2)
        encode = lambda im: tower(im, cls_only=True)[:, 0]
        x = torch.randn(3, 3, *du.image_hw(size), device=dev)
    blocks = list(tower.encoder.layer)
    calls = []
    spy = core.vit_attention_cls
    core.vit_attention_cls = lambda *a, **kw: calls.append(1) or spy(*a, **kw)
    try:
        f1, A1 = _dissect(mcd, du, dev, encode, blocks, x, True)
        assert len(calls) == 1                                   # the pruned route was taken, once
        f0, A0 = _dissect(mcd, du, dev, encode, blocks, x, False)
        assert len(calls) == 1
    finally:
        core.vit_attention_cls = spy
    assert f1.shape == f0.shape == (x.shape[0], 768)
    print("%s: max |d features| %.3e, max |d activations| %.3e" % (case, (f1 - f0).abs().max().item(),
                                                                  (A1 - A0).abs().max().item()))
    assert _close(f1, f0)
    last = 768 * (len(blocks) - 1)
    assert torch.equal(A1[:last], A0[:last])
    assert _close(A1[last:], A0[last:])
    assert _close(A1, A0)


def test_pruned_tail_runs_only_the_rows_it_needs(core, du, dev):
    """core.LINEAR_EVENTS: the last block is K|V for all tokens, then q, proj, fc1 and fc2 for one row per image, and no
    other GEMM of B * T rows; K9 runs depth - 1 times, K9C once."""
    depth, B, D = 3, 4, 768
    tower = _tower(du, dev, 64, depth, 5)
    x = torch.randn(B, 3, 64, 64, device=dev)
    T = 17
    counts = {"k9": 0, "k9c": 0}
    k9, k9c = core.vit_attention, core.vit_attention_cls
    core.vit_attention = lambda *a, **kw: counts.__setitem__("k9", counts["k9"] + 1) or k9(*a, **kw)
    core.vit_attention_cls = lambda *a, **kw: counts.__setitem__("k9c", counts["k9c"] + 1) or k9c(*a, **kw)
    core.LINEAR_EVENTS = ev = []
    try:
        with torch.no_grad():
            out = tower(x, cls_only=True)
    finally:
        core.LINEAR_EVENTS = None
        core.vit_attention, core.vit_attention_cls = k9, k9c
    assert out.shape == (B, 1, D)
    shapes = [e[2:] for e in ev]
    full = [(B * T, 3 * D, D), (B * T, D, D), (B * T, 4 * D, D), (B * T, D, 4 * D)]
    assert shapes == [(B * T, D, 3 * 16 * 16)] + full * (depth - 1) + [
        (B * T, 2 * D, D), (B, D, D), (B, D, D), (B, 4 * D, D), (B, D, 4 * D)]
    assert [s for s in shapes[-5:] if s[0] == B * T] == [(B * T, 2 * D, D)]
    assert counts == {"k9": depth - 1, "k9c": 1}


def test_gate_keeps_everything_else_on_the_full_path(core, du, dev):
    """Each of these sends a cls_only call down the full path, where a foreign hook on the last block receives
    [B, T, D]; tower(x) itself is the same bits with the flag on and off and never pruned."""
    tower = _tower(du, dev, 64, 2, 7)
    B, T, D = 3, 17, 768
    x = torch.randn(B, 3, 64, 64, device=dev)
    last = tower.encoder.layer[-1]

    def shape_of(**kw):
        with torch.no_grad():
            return tuple(tower(x, **kw).shape)

    assert shape_of(cls_only=True) == (B, 1, D)                  # the route is open to begin with
    assert shape_of() == (B, T, D)
    with torch.no_grad():
        a = tower(x)
        du.CLS_ONLY_TAIL = False
        try:
            b = tower(x)
            assert shape_of(cls_only=True) == (B, T, D)
        finally:
            du.CLS_ONLY_TAIL = True
    assert torch.equal(a, b)

    seen = []
    foreign = lambda m, i, o: seen.append(tuple(o.shape))
    marked = lambda m, i, o: seen.append(tuple(o.shape))
    marked.token0_only = True
    h = last.register_forward_hook(marked)
    assert shape_of(cls_only=True) == (B, 1, D) and seen == [(B, 1, D)]
    h.remove()
    for target, pre in ((last, False), (last.fc1, False), (tower.layernorm, False), (tower.encoder, False),
                        (last.attn.qkv, False), (last, True), (tower.layernorm, True)):
        del seen[:]
        hs = [target.register_forward_pre_hook(lambda m, i: None) if pre else target.register_forward_hook(lambda m, i, o: None),
              last.register_forward_hook(foreign)]
        try:
            assert shape_of(cls_only=True) == (B, T, D), (target, pre)
            assert seen == [(B, T, D)]
        finally:
            for k in hs:
                k.remove()
    h = tower.encoder.layer[0].register_forward_hook(foreign)    # a foreign hook on an earlier block does not matter
    assert shape_of(cls_only=True) == (B, 1, D)
    h.remove()

    assert tuple(tower(x, cls_only=True).shape) == (B, T, D)      # grad enabled
    tower.train()
    assert shape_of(cls_only=True) == (B, T, D)
    tower.eval()
    du.FUSED_RESIDUAL = False
    try:
        assert shape_of(cls_only=True) == (B, T, D)
    finally:
        du.FUSED_RESIDUAL = True
    with torch.no_grad():                                         # a mask: the block keeps its full form
        emb = tower.embed(x)
        mask = torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev)
        assert tuple(tower.encoder(emb, mask, cls_only=True).shape) == (B, T, D)
        assert tuple(last(emb, mask, cls_only=True).shape) == (B, T, D)
    assert not du.cls_tail_route(True, True, True, False, T, D, 12, 2, True, True)
    assert shape_of(cls_only=True) == (B, 1, D)                  # and nothing above left the gate shut
