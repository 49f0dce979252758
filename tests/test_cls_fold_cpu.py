"""CPU: the algebra of the folded class-token tail in float64 with plain torch -- the class token's
row of softmax(q k^T / 8) v computed from K and V, against the same row computed without them:
    u_h = W_k,h^T q_h,  p = softmax_t(u_h . n_t / 8),  o_h = W_v,h (sum_t p_t n_t) + b_v,h
(q . b_k,h is the same for every key and the softmax cancels it; sum_t p_t = 1 carries b_v,h through) -- and the gate of
the route.  Both sides are float64 and differ in summation order only: the bound 1e-11 * max(1, |ref|max) leaves more than
an order of magnitude over the worst case seen (3e-13), and a kept key bias, a dropped value bias or a wrong scale misses it
by eight."""
import pytest
import torch

B, HD = 3, 64


def _operands(T, H, bias, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * HD
    n = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    w = torch.randn(3 * D, D, generator=g, dtype=torch.float64) / D ** 0.5
    b = torch.randn(3 * D, generator=g, dtype=torch.float64) if bias else None
    return n, w, b


def _plain(n, w, b, H):
    """Row 0 of softmax(q k^T / 8) v, from the K|V projection of every token."""
    Bn, T, D = n.shape
    qkv = n @ w.T if b is None else n @ w.T + b
    q, k, v = qkv.view(Bn, T, 3, H, HD).permute(2, 0, 3, 1, 4)                    # [B, H, T, 64]
    p = torch.softmax(q[:, :, :1] @ k.transpose(2, 3) / 8.0, dim=-1)             # [B, H, 1, T]
    return (p @ v).reshape(Bn, D)


def _folded(n, w, b, H):
    """The same row without K and V: what _attend_cls_folded and K30 compute, the log2-domain scale included."""
    Bn, T, D = n.shape
    q = n[:, 0] @ w[:D].T if b is None else n[:, 0] @ w[:D].T + b[:D]
    wkt = w[D:2 * D].view(H, HD, D).transpose(1, 2) * (1.4426950408889634 / 8.0)  # [H, D, 64]
    u = torch.einsum("bhe,hde->bhd", q.view(Bn, H, HD), wkt)
    s = torch.einsum("bhd,btd->bht", u, n)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    m = torch.einsum("bht,btd->bhd", p, n) / p.sum(dim=-1, keepdim=True)
    o = torch.einsum("bhd,hed->bhe", m, w[2 * D:].view(H, HD, D))
    if b is not None:
        o = o + b[2 * D:].view(H, HD)
    return o.reshape(Bn, D)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("H", [1, 2, 12])
@pytest.mark.parametrize("T", [1, 5, 33, 197, 257])
def test_folded_row_is_the_attention_row(T, H, bias):
    n, w, b = _operands(T, H, bias, 1000 * T + H)
    ref = _plain(n, w, b, H)
    err = (_folded(n, w, b, H) - ref).abs().max().item()
    bound = 1e-11 * max(1.0, ref.abs().max().item())
    print("T=%d H=%d bias=%s: err %.3e bound %.3e" % (T, H, bias, err, bound))
    assert err <= bound


def test_the_key_bias_cancels_and_the_value_bias_does_not():
    n, w, b = _operands(33, 2, True, 5)
    ref = _plain(n, w, b, 2)
    D = 128
    other = b.clone()
    other[D:2 * D] += 3.0
    assert (_plain(n, w, other, 2) - ref).abs().max().item() <= 1e-11
    other = b.clone()
    other[2 * D:] += 3.0
    assert (_plain(n, w, other, 2) - ref - 3.0).abs().max().item() <= 1e-11
    assert (_folded(n, w, other, 2) - ref - 3.0).abs().max().item() <= 1e-11


def test_fold_gate(mcd, monkeypatch):
    """cls_fold_route: the switch, the row threshold and K30's limits; MCD_NO_CLS_FOLD is read beside MCD_NO_CLS_ONLY_TAIL."""
    from mammo_clip_dissect_amd import core
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    monkeypatch.setattr(core, "cls_token_mix_max_t", lambda heads, D: 3007 if D == 64 * heads and D <= 2048 else 0)
    assert du.CLS_FOLD is True and du.CLS_FOLD_MIN_ROWS > 985            # on by default; small batches keep the K|V GEMM
    assert du.cls_fold_route(True, 2500, 197, 768, 12, du.CLS_FOLD_MIN_ROWS)
    assert not du.cls_fold_route(False, 2500, 197, 768, 12, du.CLS_FOLD_MIN_ROWS)
    assert not du.cls_fold_route(True, 5, 197, 768, 12, du.CLS_FOLD_MIN_ROWS)
    assert du.cls_fold_route(True, 5, 197, 768, 12, 0)
    assert du.cls_fold_route(True, 1, 1, 64, 1, 0)
    assert not du.cls_fold_route(True, 5, 197, 768, 6, 0)                 # D != 64 * heads
    assert not du.cls_fold_route(True, 5, 197, 4096, 64, 0)               # past K30's width
    assert not du.cls_fold_route(True, 5, 3008, 768, 12, 0)               # past K30's token count
    assert not du.cls_fold_route(True, 65536, 1, 768, 12, 0)              # past K30's grid
    ops = du._Block(128, 2, 512)._ops()
    assert ops.owner is not None and ops.heads == 2
    assert du._BlockOps(1, 2, 3, 4, 5, 6, 7).owner is None                # a block class that does not name one: no fold
