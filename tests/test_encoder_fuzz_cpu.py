"""CPU: the encoder fuzzer (tests/encoder_fuzz.py) held to account without a GPU.

1. Its float64 references against F.scaled_dot_product_attention in float64 under masks built explicitly as [B, H, T, T]
   tensors (key padding, causal, the additive Toeplitz bias), and its K26 / K27 replays against float64 means.
2. Coverage: at the committed seeds every stratum of the plan is in the generated lists.
3. Mutants: fp32 torch emulations of the entries, built so that the headers' bit relations hold by construction (every image
   on its own; K9M / K9B's valid rows ARE the K9 emulation on the truncated sequence; a K9A row IS the K9 emulation on t + 1
   tokens).  The checker finds nothing on them over the whole committed lists, and finds every mutant of MUTANTS."""
import pytest
import torch
import torch.nn.functional as F

import encoder_fuzz as E

NAN = float("nan")


def case_list(entry):
    return E.cases(entry, E.SEEDS[entry])


# =========================================================================================================================
# 1. the references
# =========================================================================================================================
def _sdpa64(qkv, H, mask):
    B, T, _ = qkv.shape
    q, k, v = qkv.double().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, T, H * 64)


@pytest.mark.parametrize("shape", [(2, 1, 1, [1, 1]), (3, 7, 2, [7, 1, 4]), (2, 33, 3, [32, 33]), (2, 70, 2, [1, 45])])
def test_attention_references_match_sdpa_under_explicit_masks(shape):
    B, T, H, Ls = shape
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B, T, 3 * H * 64, generator=g)
    rel = torch.randn(H, 2 * T - 1, generator=g).double()
    NEG = float("-inf")
    none = torch.zeros(B, H, T, T, dtype=torch.float64)
    pad, causal, bias = none.clone(), none.clone(), none.clone()
    for b in range(B):
        for t in range(T):
            for j in range(T):
                if j >= Ls[b]:
                    pad[b, :, t, j] = NEG
                    bias[b, :, t, j] = NEG
                else:                                   # mcd_sentence.h: distance j - t, below -(L-1) that entry's value
                    bias[b, :, t, j] = rel[:, max(j - t, -(Ls[b] - 1)) + T - 1]
                if j > t:
                    causal[b, :, t, j] = NEG
    x = qkv.double()
    for what, got, mask in (("K9", E.attention_ref(x, H), none), ("K9M", E.attention_ref(x, H, Ls), pad),
                            ("K9A", E.attention_ref(x, H, None, True), causal), ("K9B", E.attention_ref(x, H, Ls, False, rel), bias)):
        err = float((got - _sdpa64(qkv, H, mask)).abs().max())
        assert err <= 1e-12, (what, shape, err)
    q, k, v = (t.reshape(B, T, H * 64) for t in x.view(B, T, 3, H * 64).unbind(2))
    assert float((E.cls_ref(q[:, 0], k, v, H) - E.attention_ref(x, H)[:, 0]).abs().max()) <= 1e-12


def test_k30_references_agree_with_each_other():
    """W_v applied to K30's own formula on u = W_k^T q log2(e) / 8 is row 0 of the attention (mcd_clsfold.h), in float64."""
    B, T, H, D = 2, 19, 3, 192
    g = torch.Generator().manual_seed(3)
    n, w, q = (torch.randn(*s, generator=g).double() for s in ((B, T, D), (3 * D, D), (B, D)))
    w = w / D ** 0.5
    u = torch.einsum("bhe,hed->bhd", q.view(B, H, 64), w[D:2 * D].view(H, 64, D)) * (E.LOG2E / 8.0)
    o = torch.einsum("bhd,hed->bhe", E.mix_ref(u, n), w[2 * D:].view(H, 64, D)).reshape(B, D)
    assert float((o - E.cls_row_ref(n, w, q, H)).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", [(2, 1, 4), (3, 5, 132), (2, 197, 768), (1, 256, 2048)])
def test_mean_replays_are_means_to_fp32_rounding(shape):
    """At most ceil(n / 4) + 3 additions and one division lie on an element's path, each rounding by 2^-24 of a partial sum
    that sum |x| bounds; the normalised row: that error over ||m||, the 71 roundings of the sum of squares, sqrt and division."""
    B, n, D = shape
    x = torch.randn(B, n, D, generator=torch.Generator().manual_seed(n + D)) * 1.5 + 0.25
    ref = x.double().mean(dim=1)
    delta = 1.01 * (-(-n // 4) + 4) * 2.0 ** -24 * x.double().abs().sum(dim=1) / n
    got = E.mean_replay(x)
    assert bool(((got.double() - ref).abs() <= delta).all())
    unit = E.masked_mean_l2_replay(x, [n] * B, 1)
    want = F.normalize(ref, dim=1)
    tol = 2 * delta.norm(dim=1) / ref.norm(dim=1) + 80 * 2.0 ** -24
    assert bool(((unit.double() - want).abs().amax(dim=1) <= tol).all())
    assert torch.equal(E.masked_mean_l2_replay(x, [n] * B, 0), got)
    short = E.masked_mean_l2_replay(x, [1] * B, 0)
    assert torch.equal(short, x[:, 0])


# =========================================================================================================================
# 2. coverage
# =========================================================================================================================
def _need(entry):
    need = set()
    if entry in ("K9", "K9A"):
        need = {("tile", t, f) for t in range(1, 9) for f in E.FILLS}
    elif entry == "K9L":
        need = {("T", T, cl) for T in E.K9L_T for cl in ("below", "equal", "above")}
        assert len([T for T in E.K9L_T if T <= 256]) == 4 and {257, 288, 300, 511, 512, 513, 545} <= set(E.K9L_T)
    elif entry in ("K9M", "K9B"):
        need = {("tile", w, t, f) for w in range(1, 9) for t in range(1, w + 1) for f in E.FILLS}
        assert len(need) == 36 * 3
        need |= {("mixed", w) for w in range(1, 9)} | {("null", w) for w in range(1, 9)} | {("low",), ("high",)}
        if entry == "K9B":
            need |= {("rel", m) for m in ("null", "zero", "rand")}
    elif entry == "K9C":
        need = {("T", T) for T in (1, 3, 5, 17, 64, 511, 512, 513, 530, 1025)}
        need |= {("row", o, p) for o in "kv" for p in (1, 2, 3, "W+4")}
    elif entry == "K30":
        need = {("shape", H, D, T) for H, D in E.K30_HD for T in (1, 5, 33, 197, 257)}
        need |= {("hc", 12, 768, hc) for hc in (4, 2, 1)} | {("hc", 32, 2048, hc) for hc in (8, 4, 2, 1)}
        need |= {("u_img",), ("n_row",), ("n_img",), ("m_img",)}
    elif entry in ("K10", "K24"):
        need = {("rows", r) for r in range(1, 10)} | {("D", D) for D in (4, 260, 768, 1028, 1540, 2048)}
    elif entry == "K25":
        need = {("n%4", r) for r in range(4)} | {("blocks", b, w) for b in (1, 2) for w in ("whole", "part")} | {("blocks", 3, "part")}
    elif entry == "K26":
        need = {("n", n, D) for n in (1, 2, 3, 4, 5, 8, 9, 197, 256) for D in (4, 252, 256, 260, 768, 2048)} | {("strided",)}
    elif entry == "K27":
        need = {("n", n, D) for n in (1, 2, 3, 4, 5, 8, 9, 197, 256) for D in (4, 252, 256, 260, 768, 2048)}
        need |= {("null",), ("low",), ("high",)}
    elif entry == "K28":
        need = {(P, lk) for P in (2, 6, 8, 14, 16) for lk in ("zero", "one", "all", "more")}
    elif entry == "K29":
        need = {(D, f, a, s) for D in (4, 128, 132) for f in (False, True) for a in (False, True) for s in ("shared", "tight", "padded")}
    if entry in E.ATTENTION or entry == "K9C":
        need |= {("regime", r) for r in E.REGIMES}
    return need


@pytest.mark.parametrize("entry", E.ENTRIES)
def test_every_stratum_is_in_the_committed_list(entry):
    cl = case_list(entry)
    missing = _need(entry) - E.strata(entry, cl)
    assert not missing, (entry, sorted(missing, key=str))
    assert cl == case_list(entry), "the list is not deterministic"
    for c in cl:                                                 # what the plan bounds
        assert 1 <= c.get("B", 1) <= 4 and c.get("H", 1) in E.HEADS + (4, 16, 24, 32)
        if entry == "K30" and c["T"] not in E.K30_T:
            assert c["B"] == 1 and c["T"] in E.cf_boundaries(c["H"], c["D"])
            assert E.cf_heads_per_pass(c["T"], c["H"], c["D"]) < E.cf_heads_per_pass(c["T"] - 1, c["H"], c["D"])
            assert c["T"] <= E.cf_max_t(c["H"], c["D"])


def test_the_heads_per_pass_formula_is_the_librarys(mcd):
    """cf_max_t restates mcd_cls_token_mix_max_t (a host function): the LDS budget the boundaries are computed from."""
    L = mcd._lib.load()
    for H, D in E.K30_HD:
        assert int(L.mcd_cls_token_mix_max_t(H, D)) == E.cf_max_t(H, D), (H, D)


# =========================================================================================================================
# 3. emulations and mutants
# =========================================================================================================================
MUTANTS = {
    "keylen_drops_last_tile": ("K9M", "K9B"),      # 1. the last key tile is dropped when L % 32 == 1
    "keylen_plus_one": ("K9M", "K9B"),             # 2. L + 1 keys
    "causal_sees_next": ("K9A",),                  # 3. key t + 1 is visible for queries with t % 32 == 31
    "rel_off_by_one": ("K9B",),                    # 4. the bias index is off by one distance
    "rel_head_minus_one": ("K9B",),                # 5. head h uses row h - 1
    "l_not_rescaled": ("K9", "K9L", "K9M", "K9A", "K9B"),   # 6. l is not rescaled when the maximum rises in the last tile
    "k9l_block_head": ("K9L",),                    # 7. the second query block reads head (h + 1) % H
    "row_stride_packed": ("K9C", "K30"),           # 8. the row stride is taken as the packed width
    "k30_first_group_u": ("K30",),                 # 9. heads beyond the first pass reuse the first group's u
    "k27_divides_by_t": ("K27",),                  # 10. the sum is divided by T
    "k28_clamp_to_l": ("K28",),                    # 11. indices are clamped to L instead of L - 1
    "k29_lk_is_a_row": ("K29",),                   # 12. r == Lk is treated as a source row
    "k26_one_chain": ("K26",),                     # further: one ascending chain instead of the four partial sums
    "k10_biased_by_d_minus_one": ("K10",),         # further: the variance divided by D - 1
    "k24_add_order": ("K24",),                     # further: word + (type + pos) for (word + type) + pos
    "k25_constant": ("K25",),                      # further: 1.7 for 1.702
}


def _lay(t, row, img):
    """[B, T, W] laid out with the strides (img, row, 1), NaN in the gaps: (flat, the as_strided reader)."""
    B, T, W = t.shape
    flat = torch.full(((B - 1) * img + (T - 1) * row + W,), NAN)
    torch.as_strided(flat, (B, T, W), (img, row, 1)).copy_(t)
    return flat


class Emu:
    """call(name, ...) in fp32 torch, one image at a time on fresh contiguous operands (so that the same image gives the same
    bits whatever call it is part of); `mutant` switches one of MUTANTS on."""

    def __init__(self, mutant=None):
        self.m = mutant

    def __call__(self, name, **a):
        return getattr(self, name)(**a)

    def _rows(self, q, k, v, bias=None):
        """q [H, Tq, 64] on k, v [H, L, 64] (+ bias [H, Tq, L]) -> [Tq, H*64]."""
        q, k, v = q.contiguous().clone(), k.contiguous().clone(), v.contiguous().clone()
        s = torch.matmul(q, k.transpose(1, 2)) / 8.0
        if bias is not None:
            s = s + bias
        out = torch.matmul(torch.softmax(s, dim=-1), v)
        L = k.shape[1]
        if self.m == "l_not_rescaled" and L > 32:
            cut = 32 * (E.tiles_of(L) - 1)
            m_prev, m_last = s[..., :cut].amax(-1, keepdim=True), s[..., cut:].amax(-1, keepdim=True)
            m_new = torch.maximum(m_prev, m_last)
            l_prev, l_last = torch.exp(s[..., :cut] - m_prev).sum(-1, keepdim=True), torch.exp(s[..., cut:] - m_new).sum(-1, keepdim=True)
            right = l_prev * torch.exp(m_prev - m_new) + l_last
            out = out * torch.where(m_last > m_prev, right / (l_prev + l_last), torch.ones_like(right))
        return out.transpose(0, 1).reshape(q.shape[1], -1)

    @staticmethod
    def _heads(qkv_b, H):
        return [t.transpose(0, 1) for t in qkv_b.view(-1, 3, H, 64).unbind(1)]           # q, k, v [H, T, 64]

    def K9(self, qkv, H):
        return self.K9B(qkv, H, None, None)

    def K9M(self, qkv, H, lens):
        return self.K9B(qkv, H, lens, None)

    def K9L(self, qkv, H):
        out = self.K9(qkv, H)
        if self.m == "k9l_block_head" and qkv.shape[1] > 256:
            for b in range(qkv.shape[0]):
                q, k, v = self._heads(qkv[b], H)
                out[b, 256:512] = self._rows(q[:, 256:512], k.roll(-1, 0), v.roll(-1, 0))
        return out

    def K9B(self, qkv, H, lens, rel):
        B, T, _ = qkv.shape
        if rel is not None and self.m == "rel_head_minus_one":
            rel = rel.roll(1, 0)
        t = torch.arange(T)
        d = t[None, :] - t[:, None]
        out = []
        for b, L in enumerate(E.clamp_lens(lens, B, T)):
            q, k, v = self._heads(qkv[b], H)
            nk = L
            if self.m == "keylen_drops_last_tile" and L % 32 == 1 and L > 1:
                nk = L - 1
            if self.m == "keylen_plus_one":
                nk = min(L + 1, T)
            bias = None
            if rel is not None:
                idx = torch.clamp(d, min=-(L - 1)) + T - 1 + (self.m == "rel_off_by_one")
                bias = rel[:, idx.clamp(max=2 * T - 2)][:, :, :nk]                       # [H, T, nk]
            rows = [self._rows(q[:, :L], k[:, :nk], v[:, :nk], None if bias is None else bias[:, :L].contiguous())]
            if L < T:
                rows.append(self._rows(q[:, L:], k[:, :nk], v[:, :nk], None if bias is None else bias[:, L:].contiguous()))
            out.append(torch.cat(rows))
        return torch.stack(out)

    def K9A(self, qkv, H):
        B, T, _ = qkv.shape
        out = torch.empty(B, T, H * 64)
        for b in range(B):
            q, k, v = self._heads(qkv[b], H)
            for t in range(T):
                n = t + 2 if self.m == "causal_sees_next" and t % 32 == 31 and t + 1 < T else t + 1
                out[b, t] = self._rows(q[:, :n], k[:, :n], v[:, :n])[t]
        return out

    def K9C(self, q, k, v, H, st):
        B, T, W = k.shape
        q_img, k_row, k_img, v_row, v_img = st
        packed = self.m == "row_stride_packed"
        k = torch.as_strided(_lay(k, k_row, k_img), (B, T, W), (k_img, W if packed else k_row, 1))
        v = torch.as_strided(_lay(v, v_row, v_img), (B, T, W), (v_img, W if packed else v_row, 1))
        return torch.cat([self._rows(q[b].view(H, 1, 64), k[b].view(T, H, 64).transpose(0, 1), v[b].view(T, H, 64).transpose(0, 1))
                          for b in range(B)])

    def K30(self, u, n, st):
        (B, H, D), T = u.shape, n.shape[1]
        u_img, n_row, n_img, m_img = st
        n = torch.as_strided(_lay(n, n_row, n_img), (B, T, D), (n_img, D if self.m == "row_stride_packed" else n_row, 1))
        out = []
        for b in range(B):
            ub, nb = u[b].contiguous().clone(), n[b].contiguous().clone()
            if self.m == "k30_first_group_u":
                ub = ub[torch.arange(H) % E.cf_heads_per_pass(T, H, D)]
            s = ub @ nb.T
            p = torch.exp2(s - s.amax(dim=-1, keepdim=True))
            out.append((p @ nb) / p.sum(dim=-1, keepdim=True))
        return torch.stack(out)

    def K10(self, x, g, b, eps):
        if self.m == "k10_biased_by_d_minus_one" and x.shape[1] > 1:
            D = x.shape[1]
            mu = x.mean(dim=1, keepdim=True)
            return (x - mu) / torch.sqrt(((x - mu) ** 2).sum(dim=1, keepdim=True) / (D - 1) + eps) * g + b
        return torch.cat([F.layer_norm(x[r:r + 1].clone(), (x.shape[1],), g, b, eps) for r in range(x.shape[0])])

    def K24(self, ids, tids, word, pos, typ, g, b, eps):
        B, T = ids.shape
        typed = typ[tids if tids is not None else torch.zeros_like(ids)]
        x = word[ids] + (typed + pos[:T][None]) if self.m == "k24_add_order" else (word[ids] + typed) + pos[:T][None]
        return self.K10(x.reshape(B * T, -1), g, b, eps)

    def K25(self, x, in_place):
        return x * torch.sigmoid((1.7 if self.m == "k25_constant" else 1.702) * x)

    def K26(self, x, t0, st):
        if self.m == "k26_one_chain":
            s = torch.zeros(x.shape[0], x.shape[2])
            for r in range(t0, x.shape[1]):
                s = s + x[:, r]
            return s / float(x.shape[1] - t0)
        return E.mean_replay(x[:, t0:])

    def K27(self, x, lens, normalize):
        B, T, D = x.shape
        Ls = E.clamp_lens(lens, B, T)
        if self.m != "k27_divides_by_t":
            return E.masked_mean_l2_replay(x, Ls, normalize)
        m = torch.cat([E.mean_replay(x[b:b + 1, :L]) * float(L) / float(T) for b, L in enumerate(Ls)])
        return E.l2_replay(m) if normalize else m

    def K11(self, x, P):
        rows = E.patch_rows(x, P)
        return torch.cat([torch.zeros_like(rows[:, :1]), rows], dim=1)

    def K28(self, x, keep, P):
        rows = E.patch_rows(x, P)
        L = rows.shape[1]
        if self.m == "k28_clamp_to_l":                                           # patch L: whatever lies behind the image
            rows, L = torch.cat([rows, torch.full_like(rows[:, :1], NAN)], dim=1), L + 1
        got = rows.gather(1, keep.long().clamp(0, L - 1)[:, :, None].expand(-1, -1, rows.shape[2]))
        return torch.cat([torch.zeros_like(rows[:, :1]), got], dim=1)

    def K29(self, src, pad, restore, fill, add):
        B = restore.shape[0]
        src = src[None].expand(B, -1, -1) if src.dim() == 2 else src
        Lk = src.shape[1] - 1
        if self.m == "k29_lk_is_a_row" and fill is not None:                     # row 1 + Lk: whatever lies behind the source
            src, Lk = torch.cat([src, torch.full_like(src[:, :1], NAN)], dim=1), Lk + 1
        return E.token_restore_ref(src, restore, fill, add, Lk)


@pytest.mark.parametrize("entry", E.ENTRIES)
def test_the_checker_finds_nothing_on_the_emulations(entry):
    findings, ratio = E.run(entry, case_list(entry), Emu())
    print("%s: %d cases, max err / bound %.3f" % (entry, len(case_list(entry)), ratio))
    assert not findings, findings[:5]
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant,entry", [(m, e) for m, es in MUTANTS.items() for e in es])
def test_the_checker_finds_the_mutant(mutant, entry):
    call = Emu(mutant)
    for c in case_list(entry):
        findings, _ = E.check(entry, c, call)
        if findings:
            print(findings[0])
            return
    pytest.fail("no case of %s's committed list notices %s" % (entry, mutant))
