"""GPU: the folded class-token tail -- K30 (mcd_cls_token_mix, include/mcd_clsfold.h) against float64 and against the route it
replaces (the K|V GEMM + K9C) on the same operands, its softmax range, batch independence, strides, frames, refusals, the
stream and capture contracts, and the towers with CLS_FOLD on against off.

The operands of a case are what the block has at that point: n [B, T, D] (LN1's output), the qkv weight w [3D, D] and the
class token's query q [B, D].  The float64 reference is row 0 of softmax(q k^T / 8) v.  K30's side is u = W_k^T q * log2(e)/8
(float64, rounded to fp32), K30, and W_v applied in float64, so its error is K30's own; err32 is the error of
core.linear_residual (K|V) + core.vit_attention_cls against the same reference.  The bound is test_gpu_cls_tail's for K9C:
3e-6 * max(1, |ref|max) + 3 * err32."""
import pytest
import torch

import test_gpu_stream_contracts as S

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
HEADS = [(1, 64), (2, 128), (12, 768)]
TOKENS = [1, 5, 31, 32, 33, 197, 257]
# further head counts, one per heads-per-pass instance of the kernel (4, 8, 16, 12 x 2) and a head count that none divides
MORE = [(2, 33, 4, 256), (2, 33, 8, 512), (2, 33, 16, 1024), (1, 33, 24, 1536), (2, 5, 3, 192)]


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core as c
    assert c.linear_residual_available(), "libmcd_blaslt.so did not load"
    return c


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def _operands(B, T, H, D, dev, seed, q_scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    n = torch.randn(B, T, D, device=dev, generator=g)
    w = torch.randn(3 * D, D, device=dev, generator=g) / D ** 0.5
    q = torch.randn(B, D, device=dev, generator=g) * q_scale
    return n, w, q


def _u64(w, q, H):
    """u [B, H, D] in float64: W_k,h^T q_h * log2(e) / 8."""
    D = q.shape[1]
    u = torch.einsum("bhe,hed->bhd", q.double().view(-1, H, 64), w[D:2 * D].double().view(H, 64, D)) * (LOG2E / 8.0)
    return u.contiguous()


def _mix64(u, n):
    """K30's own formula in float64."""
    s = torch.einsum("bhd,btd->bht", u.double(), n.double())
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    return torch.einsum("bht,btd->bhd", p, n.double()) / p.sum(dim=-1, keepdim=True)


def _row64(n, w, q, H):
    """Row 0 of softmax(q k^T / 8) v in float64, from K and V of every token."""
    B, T, D = n.shape
    kv = (n.double() @ w[D:].double().T).view(B, T, 2, H, 64)
    s = torch.einsum("bhe,bthe->bht", q.double().view(B, H, 64), kv[:, :, 0]) / 8.0
    return torch.einsum("bht,bthe->bhe", torch.softmax(s, dim=-1), kv[:, :, 1]).reshape(B, D)


def _errors(core, n, w, q, H):
    """(err of K30 in the output's space, err32 of the K|V GEMM + K9C, |ref|max, err of K30 on its own formula, |m ref|max)."""
    B, T, D = n.shape
    ref = _row64(n, w, q, H)
    u = _u64(w, q, H).float()
    m = core.cls_token_mix(u, n)
    assert m.shape == (B, H, D) and m.is_contiguous()
    o = torch.einsum("bhd,hed->bhe", m.double(), w[2 * D:].double().view(H, 64, D)).reshape(B, D)
    kv = core.linear_residual(None, n, w[D:].contiguous()).view(B, T, 2, H, 64)
    o32 = core.vit_attention_cls(q.view(B, H, 64), kv[:, :, 0], kv[:, :, 1])
    m_ref = _mix64(u, n)
    return ((o - ref).abs().max().item(), (o32.double() - ref).abs().max().item(), ref.abs().max().item(),
            (m.double() - m_ref).abs().max().item(), m_ref.abs().max().item(), m)


def _check(core, n, w, q, H, what):
    err, err32, top, err_m, top_m, m = _errors(core, n, w, q, H)
    bound = 3e-6 * max(1.0, top) + 3 * err32
    bound_m = 3e-6 * max(1.0, top_m) + 3 * err32
    print("K30 %s: err %.3e err32 %.3e bound %.3e; on its own formula err %.3e bound %.3e" % (what, err, err32, bound, err_m,
                                                                                              bound_m))
    assert torch.isfinite(m).all()
    assert err <= bound, (what, err, err32)
    assert err_m <= bound_m, (what, err_m, err32)


@pytest.mark.parametrize("hd", HEADS, ids=lambda hd: "H%d-D%d" % hd)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("B", [1, 3])
def test_k30_matches_float64(core, dev, B, T, hd):
    H, D = hd
    _check(core, *_operands(B, T, H, D, dev, 1000 * T + 10 * H + B), H, "B=%d T=%d H=%d D=%d" % (B, T, H, D))


@pytest.mark.parametrize("shape", MORE, ids=lambda s: "B%d-T%d-H%d-D%d" % s)
def test_k30_every_heads_per_pass(core, dev, shape):
    B, T, H, D = shape
    _check(core, *_operands(B, T, H, D, dev, T + H), H, "B=%d T=%d H=%d D=%d" % shape)


@pytest.mark.parametrize("hd", HEADS, ids=lambda hd: "H%d-D%d" % hd)
def test_k30_softmax_range(core, dev, hd):
    """Scores that span +-100 in the log2 domain stay finite and within the bound; with one token far above the rest m is
    that token's row."""
    H, D = hd
    B, T = 3, 197
    n, w, q = _operands(B, T, H, D, dev, 77 + H)
    s = torch.einsum("bhd,btd->bht", _u64(w, q, H), n.double())
    q = q * (100.0 / min(s.max().item(), -s.min().item()))
    s = torch.einsum("bhd,btd->bht", _u64(w, q, H).float().double(), n.double())
    assert s.max().item() > 99 and s.min().item() < -99
    _check(core, n, w, q, H, "scores +-100, H=%d D=%d" % (H, D))
    pick = torch.tensor([[(7 * b + 5 * h) % T for h in range(H)] for b in range(B)], device=dev)
    rows = n[torch.arange(B, device=dev)[:, None], pick]                       # [B, H, D]
    m = core.cls_token_mix((rows * (300.0 / D)).contiguous(), n)               # s = 300 |n_t|^2 / D at the picked token
    d = (m - rows).abs().max().item()
    print("K30 one token far above, H=%d D=%d: max |m - row| %.3e" % (H, D, d))
    assert d <= 1e-6


def test_k30_does_not_depend_on_the_batch(core, dev):
    H, D, T = 12, 768, 197
    n, w, q = _operands(3, T, H, D, dev, 9)
    u = _u64(w, q, H).float()
    together = core.cls_token_mix(u, n)
    for b in range(3):
        alone = core.cls_token_mix(u[b:b + 1].clone(), n[b:b + 1].clone())
        assert torch.equal(alone[0], together[b]), b


@pytest.mark.parametrize("hd", [(2, 128), (12, 768)], ids=lambda hd: "H%d-D%d" % hd)
def test_k30_strides_and_frames(core, dev, hd):
    """n as a view inside a larger tensor, u and m with padded image strides: the bits of the packed call, the padding of m
    untouched, out= returned."""
    H, D = hd
    B, T = 3, 33
    n, w, q = _operands(B, T, H, D, dev, 21)
    u = _u64(w, q, H).float()
    want = core.cls_token_mix(u, n)
    big = torch.full((B, T + 2, D + 64), float("nan"), device=dev)
    big[:, 1:T + 1, 32:32 + D] = n
    n_view = big[:, 1:T + 1, 32:32 + D]
    assert n_view.stride() == ((T + 2) * (D + 64), D + 64, 1)
    u_big = torch.full((B, H * D + 64), float("nan"), device=dev)
    u_big[:, :H * D] = u.view(B, H * D)
    m_big = torch.full((B, H * D + 64), 7.0, device=dev)
    out = m_big[:, :H * D].unflatten(1, (H, D))
    got = core.cls_token_mix(u_big[:, :H * D].unflatten(1, (H, D)), n_view, out=out)
    assert got is out
    assert torch.equal(got, want)
    assert (m_big[:, H * D:] == 7.0).all()
    assert torch.equal(core.cls_token_mix(u, n_view), want)
    with pytest.raises((TypeError, ValueError)):
        core.cls_token_mix(u, n[:, :, ::2])
    with pytest.raises((TypeError, ValueError)):
        core.cls_token_mix(u[:, :, :D - 64], n)
    with pytest.raises(TypeError):
        core.cls_token_mix(u.double(), n)


def test_k30_rejects_bad_arguments(mcd, core, dev):
    """The limits (MCD_E_UNSUPPORTED), a NULL and a misaligned pointer and short strides (MCD_E_ARG): nothing is launched."""
    L = mcd._lib.load()
    E_ARG, E_UNS = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_UNSUPPORTED
    B, T, H, D = 2, 8, 2, 128
    u = torch.randn(B, H, D, device=dev)
    n = torch.randn(B, T + 1, D, device=dev)
    out = torch.full((B, H, D), 7.0, device=dev)
    pu, pn, po = u.data_ptr(), n.data_ptr(), out.data_ptr()

    def call(u=pu, u_img=H * D, n=pn, n_row=D, n_img=(T + 1) * D, B=B, T=T, H=H, D=D, m=po, m_img=H * D):
        return L.mcd_cls_token_mix(u, u_img, n, n_row, n_img, B, T, H, D, m, m_img, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == 7.0).any()
    out.fill_(7.0)
    max_t = core.cls_token_mix_max_t(H, D)
    assert max_t >= 1024 and core.cls_token_mix_max_t(32, 2048) >= 1024 and core.cls_token_mix_max_t(12, 768) >= 1024
    assert core.cls_token_mix_max_t(2, 192) == 0 and core.cls_token_mix_max_t(33, 2112) == 0
    assert call(D=192) == E_UNS and call(H=1, D=2112) == E_UNS and call(H=3) == E_UNS
    assert call(T=0) == E_UNS and call(T=max_t + 1) == E_UNS
    assert call(B=65536) == E_UNS
    assert call(u=None) == E_ARG and call(n=None) == E_ARG and call(m=None) == E_ARG
    assert call(u=pu + 4) == E_ARG and call(n=pn + 8) == E_ARG and call(m=po + 4) == E_ARG
    assert call(n_row=D + 2) == E_ARG and call(n_row=D - 4) == E_ARG and call(u_img=H * D - 4) == E_ARG
    assert call(m_img=H * D - 4) == E_ARG and call(m_img=H * D + 1) == E_ARG
    assert call(B=-1) == E_ARG and call(H=0) == E_ARG
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(mcd._lib.McdError):
        core.cls_token_mix(torch.zeros(1, 2, 192, device=dev), torch.zeros(1, 4, 192, device=dev))


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery (as test_gpu_text_tower.py) --------------------
def b_cls_token_mix(L, dev):
    B, T, H, D = 2, 5, 2, 128
    return S.simple(L, dev, "K30", [S._gen((B, H, D)), S._gen((B, T, D))], [(B, H, D)],
                    lambda i, o, st: L.mcd_cls_token_mix(i[0], H * D, i[1], D, T * D, B, T, H, D, o[0], H * D, st))


CLSFOLD_STREAM_ROWS = {"mcd_cls_token_mix": b_cls_token_mix}


def test_stream_rows_cover_the_header(mcd):
    """Every entry of the header that takes a stream (its last argument) has a row."""
    with_stream = [name for name, (res, args) in mcd._lib.CLSFOLD_SIGNATURES.items() if name != "mcd_cls_token_mix_max_t"]
    assert sorted(CLSFOLD_STREAM_ROWS) == sorted(with_stream)


@pytest.fixture(scope="module")
def spin_cycles(dev):
    """A spin of at least S.MIN_SPIN_MS (the entry runs in well under a millisecond), in the cycles of torch.cuda._sleep."""
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


@pytest.mark.parametrize("entry", sorted(CLSFOLD_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(mcd, dev, spin_cycles, entry):
    L = mcd._lib.load()
    r = S.Run(entry, CLSFOLD_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)


@pytest.mark.parametrize("entry", sorted(CLSFOLD_STREAM_ROWS))
def test_capture_and_replay(mcd, dev, entry):
    L = mcd._lib.load()
    r = S.Run(entry, CLSFOLD_STREAM_ROWS[entry](L, dev), dev)
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


# ---- the towers: CLS_FOLD on against off ------------------------------------------------------------------------------------------
def _tower(du, dev, case, seed, qkv_bias=True):
    torch.manual_seed(seed)
    if case == "D128":
        tower = du.ViTTower(image_size=64, dim=128, depth=2, heads=2, mlp=512)          # T = 17
    else:
        tower = du.ViTTower(image_size=224, depth=2)                                    # 12 heads, T = 197
    tower = tower.to(dev).eval()
    for p in tower.parameters():
        torch.nn.init.normal_(p, std=0.05)
    if not qkv_bias:
        for blk in tower.encoder.layer:
            blk.attn.qkv.bias = None
    return tower


def _dissect(du, dev, tower, x, fold, monkeypatch, core):
    """tower(x, cls_only=True)[:, 0] with a Dissector hook on every block: (features, activations [U, B], the calls made)."""
    from mammo_clip_dissect_amd.pipeline import Dissector
    blocks = list(tower.encoder.layer)
    D = tower.out_dim
    dis = Dissector(x.shape[0], ["b%d" % i for i in range(len(blocks))], [D] * len(blocks), 8, du.PROJ_DIM, dev)
    hs = [m.register_forward_hook(dis.hook(i)) for i, m in enumerate(blocks)]
    calls = {"k30": 0, "k9c": 0}
    k30, k9c = core.cls_token_mix, core.vit_attention_cls
    with monkeypatch.context() as mp:
        mp.setattr(du, "CLS_FOLD", fold)
        mp.setattr(du, "CLS_FOLD_MIN_ROWS", 0)
        mp.setattr(core, "cls_token_mix", lambda *a, **kw: calls.__setitem__("k30", calls["k30"] + 1) or k30(*a, **kw))
        mp.setattr(core, "vit_attention_cls", lambda *a, **kw: calls.__setitem__("k9c", calls["k9c"] + 1) or k9c(*a, **kw))
        mp.setattr(core, "LINEAR_EVENTS", [])
        try:
            with torch.no_grad():
                f = tower(x, cls_only=True)[:, 0].clone()
            shapes = [e[2:] for e in core.LINEAR_EVENTS]
        finally:
            for h in hs:
                h.remove()
    return f, dis.At[:, :x.shape[0]].clone(), calls, shapes


def _close(a, b):
    return (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("case", ["D128", "D768", "D128-no-qkv-bias"])
def test_folded_tail_matches_the_kv_tail(core, du, dev, monkeypatch, case):
    """encode_image's features and the hooked token-0 activations with the fold on against off, within test_gpu_cls_tail's
    1e-4 * max(1, |ref|max); the blocks before the last bit for bit; the folded tail runs K30 and no GEMM of B*T rows behind
    LN1, the other one the K|V GEMM and K9C."""
    tower = _tower(du, dev, case[:4], 11, qkv_bias=not case.endswith("no-qkv-bias"))
    D = tower.out_dim
    B, size = (3, 64) if D == 128 else (2, 224)
    T = 1 + (size // 16) ** 2
    x = torch.randn(B, 3, size, size, device=dev)
    f1, A1, calls1, shapes1 = _dissect(du, dev, tower, x, True, monkeypatch, core)
    f0, A0, calls0, shapes0 = _dissect(du, dev, tower, x, False, monkeypatch, core)
    assert calls1 == {"k30": 1, "k9c": 0} and calls0 == {"k30": 0, "k9c": 1}
    H = D // 64
    tail = [(B, D, D)] + [(B, D, 64)] * H + [(B, 64, D)] * H + [(B, D, D), (B, 4 * D, D), (B, D, 4 * D)]
    assert shapes1[-len(tail):] == tail and (B * T, 2 * D, D) not in shapes1
    assert shapes0[-5:] == [(B * T, 2 * D, D), (B, D, D), (B, D, D), (B, 4 * D, D), (B, D, 4 * D)]
    print("%s: max |d features| %.3e, max |d activations| %.3e" % (case, (f1 - f0).abs().max().item(),
                                                                  (A1 - A0).abs().max().item()))
    assert f1.shape == f0.shape == (B, D)
    assert _close(f1, f0)
    assert torch.equal(A1[:D], A0[:D])
    assert _close(A1, A0)


def test_fold_off_and_small_batches_keep_the_parents_tail(core, du, dev, monkeypatch):
    """With CLS_FOLD off, and below CLS_FOLD_MIN_ROWS with it on, the tail is the K|V GEMM + K9C sequence bit for bit: what
    _block_hip computes for operands that name no owner."""
    tower = _tower(du, dev, "D128", 13)
    x = torch.randn(3, 3, 64, 64, device=dev)
    last = tower.encoder.layer[-1]
    with torch.no_grad():
        emb = tower.encoder.layer[0](tower.embed(x))
        want = du._block_hip(last._ops()._replace(owner=None), emb, "k9", cls_only=True)
        assert du.CLS_FOLD and 3 * 17 < du.CLS_FOLD_MIN_ROWS
        assert torch.equal(last(emb, cls_only=True), want)                       # a small batch, the fold on
        monkeypatch.setattr(du, "CLS_FOLD_MIN_ROWS", 0)
        folded = last(emb, cls_only=True)
        assert _close(folded, want)
        monkeypatch.setattr(du, "CLS_FOLD", False)
        assert torch.equal(last(emb, cls_only=True), want)


def test_a_foreign_hook_keeps_the_full_block(core, du, dev, monkeypatch):
    """A user hook without token0_only on the last block: the tower runs the full block, K30 is not called."""
    tower = _tower(du, dev, "D128", 17)
    x = torch.randn(3, 3, 64, 64, device=dev)
    monkeypatch.setattr(du, "CLS_FOLD_MIN_ROWS", 0)
    calls, seen = [], []
    k30 = core.cls_token_mix
    monkeypatch.setattr(core, "cls_token_mix", lambda *a, **kw: calls.append(1) or k30(*a, **kw))
    with torch.no_grad():
        assert tuple(tower(x, cls_only=True).shape) == (3, 1, 128) and calls == [1]
        h = tower.encoder.layer[-1].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
        try:
            assert tuple(tower(x, cls_only=True).shape) == (3, 17, 128)
        finally:
            h.remove()
    assert calls == [1] and seen == [(3, 17, 128)]


def test_folded_weight_follows_the_parameter(core, du, dev, monkeypatch):
    """The transposed W_k copy is rebuilt when the qkv weight changes in place."""
    tower = _tower(du, dev, "D128", 19)
    x = torch.randn(3, 3, 64, 64, device=dev)
    monkeypatch.setattr(du, "CLS_FOLD_MIN_ROWS", 0)
    us = []
    k30 = core.cls_token_mix
    monkeypatch.setattr(core, "cls_token_mix", lambda u, n, **kw: us.append(u.clone()) or k30(u, n, **kw))
    with torch.no_grad():
        tower(x, cls_only=True)
        tower.encoder.layer[-1].attn.qkv.weight[128:256].mul_(-1.0)       # W_k -> -W_k: u -> -u
        tower(x, cls_only=True)
        tower(x, cls_only=True)
    top = us[0].abs().max().item()
    assert top > 0 and (us[1] + us[0]).abs().max().item() <= 1e-6 * top    # a stale copy would leave us[1] at us[0]
    assert torch.equal(us[2], us[1])
