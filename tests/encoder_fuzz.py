"""The encoder-side fuzzer: a stratified case generator, float64 references written from the headers (include/mcd_*.h) and a
checker that takes the entries as a callable, for the attention family (K9, K9L, K9M, K9A, K9B), the one-row entries (K9C,
K30) and the token / row operations (K10, K24, K25, K26, K27, K28, K29).  Importing this module touches no GPU.

  cases(entry, seed)        a deterministic list of plain dicts: every stratum first (strata() names them), the remaining
                            parameters from the seeded generator.  SEEDS holds the seeds the tests are committed to.
  check(entry, case, call)  draws the operands of the case, calls call(name, **operands) -> tensor for the entry and for the
                            entries its relations name, and returns (findings, err / bound).  The same checker runs on the
                            library (gpu_call: every operand in a frame of test_gpu_encoder_frames) and on the fp32 torch
                            emulations of tests/test_encoder_fuzz_cpu.py.

What call(name, ...) is given, per name (tensors on the device check() was given; lens / strides are plain Python values):
  K9, K9L, K9A   qkv [B, T, 3*H*64], H                              -> [B, T, H*64]
  K9M            qkv, H, lens (list of B ints | None)               -> [B, T, H*64]
  K9B            qkv, H, lens, rel ([H, 2T-1] | None)               -> [B, T, H*64]
  K9C            q [B, W], k, v [B, T, W], H, st = (q_img, k_row, k_img, v_row, v_img)          -> [B, W]
  K30            u [B, H, D], n [B, T, D], st = (u_img, n_row, n_img, m_img)                    -> [B, H, D]
  K10            x [rows, D], g, b [D], eps                         -> [rows, D]
  K24            ids, tids ([B, T] int64, tids | None), word, pos, typ, g, b, eps               -> [B*T, D]
  K25            x [n], in_place                                    -> [n]
  K26            x [B, T, D], t0, st = (x_tok, x_img, out_img)      -> [B, D]
  K27            x [B, T, D], lens, normalize                       -> [B, D]
  K11            x [B, Cin, Hh, Ww], P                              -> [B, 1 + L, Cin*P*P]
  K28            x, keep [B, Lk] int32, P                           -> [B, 1 + Lk, Cin*P*P]
  K29            src ([B, 1+Lk, D] | [1+Lk, D] shared), pad (floats between two images of src), restore [B, L] int32,
                 fill ([D] | None), add ([1+L, D] | None)           -> [B, 1 + L, D]

Only inputs the headers define are drawn: finite values, lens of any sign (the clamp is in the contract), indices of any value
where the header clamps them."""
import numpy as np
import torch
import torch.nn.functional as F

NAN = float("nan")
LOG2E = 1.4426950408889634
ATTENTION = ("K9", "K9L", "K9M", "K9A", "K9B")
CLS_ROW = ("K9C", "K30")
TOKEN_OPS = ("K10", "K24", "K25", "K26", "K27", "K28", "K29")
ENTRIES = ATTENTION + CLS_ROW + TOKEN_OPS
SEEDS = {e: 7001 + i for i, e in enumerate(ENTRIES)}          # the committed seed of every entry's test

HEADS = (1, 2, 3, 5, 8, 12)
FILLS = (1, 31, 32)                                           # keys in the last 32-key tile
REGIMES = ("r0.01", "r1", "r6", "rise", "fall", "dominant", "zerok", "voff")
K9L_T = (257, 288, 300, 511, 512, 513, 545, 1, 33, 200, 256)
K9C_T = (1, 3, 5, 17, 64, 511, 512, 513, 530, 1025)
K30_HD = ((1, 64), (2, 128), (3, 192), (4, 256), (8, 512), (12, 768), (16, 1024), (24, 1536), (32, 2048))
K30_T = (1, 5, 33, 197, 257)
CF_LDS_FLOATS = 144 * 1024 // 4       # K30's LDS budget in floats: heads-per-pass rows of u, H*T scores, H sums (mcd_clsfold.h;
CF_INSTANCES = (16, 12, 8, 4, 2, 1)   # mcd_cls_token_mix_max_t(H, D) = (CF_LDS_FLOATS - D - H) / H is the count of 1 at its limit)
LN_D = (4, 260, 768, 1028, 1540, 2048)
MEAN_N = (1, 2, 3, 4, 5, 8, 9, 197, 256)
MEAN_D = (4, 252, 256, 260, 768, 2048)
K25_BLOCK = 4096                      # floats a workgroup of K25 takes (256 threads x 4 float4s)
K25_N = (1, 2, 3, 4, 5, 7, 8, 9, 4093, 4095, 4096, 4097, 4100, 8191, 8192, 8193, 12289, 12294)
K28_P = (2, 6, 8, 14, 16)
K29_D = (4, 128, 132)
LENS_GAP = 1 << 20                    # what surrounds an index list in its frame (test_gpu_text_tower.LENS_GAP)


# =========================================================================================================================
# 1. cases
# =========================================================================================================================
def _pick(rng, xs):
    return xs[int(rng.integers(len(xs)))]


def _tile_len(tiles, fill):
    return 32 * (tiles - 1) + fill


def tiles_of(n):
    return -(-n // 32)


def fill_of(n):
    return n - 32 * (tiles_of(n) - 1)


def clamp_lens(lens, B, T):
    """The header's L = clamp(lens[b], 1, T); lens None: every length is T."""
    return [T] * B if lens is None else [min(max(int(v), 1), T) for v in lens]


def cf_heads_per_pass(T, H, D):
    """K30: the largest instantiated head count that divides H and whose u rows fit LDS beside the scores."""
    for hc in CF_INSTANCES:
        if H % hc == 0 and hc * D + H * T + H <= CF_LDS_FLOATS:
            return hc
    return 1


def cf_max_t(H, D):
    return (CF_LDS_FLOATS - D - H) // H


def cf_boundaries(H, D):
    """The token counts just above every point where cf_heads_per_pass falls to a smaller instance."""
    out, T = [], 1
    while T < cf_max_t(H, D):
        hc = cf_heads_per_pass(T, H, D)
        if hc == 1:
            break
        T = (CF_LDS_FLOATS - hc * D - H) // H + 1          # the first T at which hc no longer fits
        if T <= cf_max_t(H, D):
            out.append(T)
    return out


def _other_lens(rng, T):
    """A length of a sequence that is not the stratum's: mostly valid, sometimes one the header clamps."""
    r = rng.random()
    if r < 0.12:
        return int(_pick(rng, (0, -1, -7)))
    if r < 0.24:
        return T + int(_pick(rng, (1, 5, 1000)))
    return int(rng.integers(1, T + 1))


def _attn_cases(entry, rng):
    out = []
    reg = [REGIMES[i] for i in rng.permutation(len(REGIMES))]

    def add(T, **kw):
        c = dict(B=int(rng.integers(1, 5)), T=int(T), H=int(_pick(rng, HEADS)), regime=reg[len(out) % len(reg)])
        c.update(kw)
        out.append(c)
        return c

    if entry in ("K9", "K9A"):
        for tiles in range(1, 9):
            for fill in FILLS:
                add(_tile_len(tiles, fill))
        for _ in range(8):
            add(rng.integers(1, 257))
    elif entry == "K9L":
        classes = ("below", "equal", "above")
        for T in K9L_T:
            nqb = -(-T // 256)
            for cl in classes:
                ok = [(b, h) for b in range(1, 5) for h in HEADS if _xcd_class(b * h * nqb) == cl]
                b, h = ok[int(rng.integers(min(len(ok), 4)))]              # (the smaller batches: the long sequences stay cheap)
                add(T, B=b, H=h)
    else:                                                                    # K9M, K9B
        for waves in range(1, 9):
            for tiles in range(1, waves + 1):
                for fill in FILLS:
                    L = _tile_len(tiles, fill)
                    T = int(rng.integers(max(L, 32 * (waves - 1) + 1), 32 * waves + 1))
                    c = add(T)
                    lens = [_other_lens(rng, T) for _ in range(c["B"])]
                    lens[int(rng.integers(c["B"]))] = L
                    c["lens"] = lens
        for waves in range(1, 9):                                            # per wave count: lens = NULL; a batch of four that mixes
            T = int(rng.integers(32 * (waves - 1) + 1, 32 * waves + 1))      # lengths, a clamped one of either kind among them
            add(T, lens=None)
            add(T, B=4, lens=[T, 0 if waves % 2 else -3, T + 1 + waves, int(rng.integers(1, T + 1))])
        if entry == "K9B":
            modes = ("rand", "rand", "null", "rand", "zero")
            for i, c in enumerate(out):
                c["rel"] = modes[i % len(modes)]
    return out


def _xcd_class(total):
    return "equal" if total % 8 == 0 else ("above" if total % 8 <= 3 else "below")


def _k9c_cases(rng):
    out = []
    reg = [REGIMES[i] for i in rng.permutation(len(REGIMES))]
    for T in K9C_T:
        for _ in range(3):
            B, H = int(rng.integers(1, 5)), int(_pick(rng, HEADS))
            W = H * 64
            pitch = lambda: int(_pick(rng, (W, W + 4, 2 * W, 3 * W)))
            q_img, k_row, v_row = pitch(), pitch(), pitch()
            st = (q_img, k_row, (T - 1) * k_row + W + int(_pick(rng, (0, 4))), v_row, (T - 1) * v_row + W + int(_pick(rng, (0, 4))))
            out.append(dict(B=B, T=T, H=H, regime=reg[len(out) % len(reg)], st=st))
    return out


def _k30_cases(rng):
    out = []

    def add(B, T, H, D):
        u_img = H * D + int(_pick(rng, (0, 4, 64)))
        n_row = D + int(_pick(rng, (0, 4, D)))
        n_img = (T - 1) * n_row + D + int(_pick(rng, (0, 8)))
        out.append(dict(B=B, T=T, H=H, D=D, q_scale=float(_pick(rng, (1.0, 6.0))),
                        st=(u_img, n_row, n_img, H * D + int(_pick(rng, (0, 4))))))

    for H, D in K30_HD:
        for T in K30_T:
            add(int(rng.integers(1, 5 if D < 1024 else 3)), T, H, D)
    for H, D in ((12, 768), (32, 2048)):
        for T in cf_boundaries(H, D):
            add(1, T, H, D)
    return out


def _ln_cases(entry, rng):
    out = []
    shapes = [(r, LN_D[(r - 1) % len(LN_D)]) for r in range(1, 10)] + [(int(rng.integers(1, 10)), D) for D in LN_D]
    shapes += [(int(rng.integers(1, 10)), 4 * int(rng.integers(1, 513))) for _ in range(5)]
    for rows, D in shapes:
        c = dict(rows=rows, D=D, offset=float(_pick(rng, (0.0, 50.0))), eps=float(_pick(rng, (1e-12, 1e-5))))
        if entry == "K24":
            c["T"] = int(_pick(rng, [t for t in range(1, rows + 1) if rows % t == 0]))
            c["vocab"], c["n_type"], c["tids"] = int(rng.integers(1, 40)), int(rng.integers(1, 4)), bool(rng.random() < 0.7)
        out.append(c)
    return out


def _mean_cases(entry, rng):
    out = []
    for n in MEAN_N:
        for D in MEAN_D:
            B = int(rng.integers(1, 5))
            if entry == "K26":
                t0 = int(rng.integers(0, 4))
                T = n + t0
                x_tok = D + int(_pick(rng, (0, 4, D)))
                out.append(dict(B=B, T=T, D=D, t0=t0, st=(x_tok, (T - 1) * x_tok + D + int(_pick(rng, (0, 8))),
                                                            D + int(_pick(rng, (0, 4))))))
            else:
                T = n + int(rng.integers(0, 6))
                lens = [_other_lens(rng, T) for _ in range(B)]
                lens[int(rng.integers(B))] = n
                out.append(dict(B=B, T=T, D=D, lens=lens, normalize=int(rng.integers(0, 2))))
    if entry == "K27":
        for i, n in enumerate(MEAN_N):                                        # lens = NULL; both clamped kinds in one batch
            D = MEAN_D[i % len(MEAN_D)]
            out.append(dict(B=int(rng.integers(1, 5)), T=n, D=D, lens=None, normalize=i % 2))
            out.append(dict(B=3, T=n + 2, D=D, lens=[0 if i % 2 else -4, n + 2 + 1 + i, n], normalize=1 - i % 2))
    return out


def _k28_cases(rng):
    out = []
    for P in K28_P:
        for lk in ("zero", "one", "all", "more"):
            hp, wp = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            L = hp * wp
            Lk = {"zero": 0, "one": 1, "all": L, "more": L + int(rng.integers(1, 6))}[lk]
            out.append(dict(B=int(rng.integers(1, 5)), Cin=int(rng.integers(1, 4)), P=P, hp=hp, wp=wp, Lk=Lk, lk=lk))
    return out


def _k29_cases(rng):
    out = []
    for D in K29_D:
        for fill in (False, True):
            for add in (False, True):
                for src in ("shared", "tight", "padded"):
                    Lk = int(rng.integers(0 if fill else 1, 7))
                    out.append(dict(B=int(rng.integers(1, 5)), D=D, L=int(rng.integers(1, 12)), Lk=Lk, fill=fill, add=add, src=src,
                                    pad=0 if src != "padded" else int(_pick(rng, (4, D)))))
    return out


def cases(entry, seed):
    rng = np.random.default_rng([int(seed), ENTRIES.index(entry)])
    if entry in ATTENTION:
        out = _attn_cases(entry, rng)
    elif entry == "K9C":
        out = _k9c_cases(rng)
    elif entry == "K30":
        out = _k30_cases(rng)
    elif entry in ("K10", "K24"):
        out = _ln_cases(entry, rng)
    elif entry == "K25":
        out = [dict(n=n) for n in K25_N] + [dict(n=int(rng.integers(1, 3 * K25_BLOCK))) for _ in range(6)]
    elif entry in ("K26", "K27"):
        out = _mean_cases(entry, rng)
    elif entry == "K28":
        out = _k28_cases(rng)
    elif entry == "K29":
        out = _k29_cases(rng)
    else:
        raise KeyError(entry)
    for i, c in enumerate(out):
        c.update(entry=entry, i=i, ds=int(seed) * 100003 + 977 * ENTRIES.index(entry) + i)
    return out


def random_cases(entry, count, seed):
    """`count` cases for the command line: the stratified lists of consecutive seeds, one after the other."""
    out, s = [], int(seed)
    while len(out) < count:
        out += cases(entry, s)
        s += 1
    return out[:count]


def strata(entry, case_list):
    """The strata of section 1 of the fuzzer's plan that a case list covers, as a set of tuples (the CPU test holds the
    committed lists to the full sets)."""
    s = set()
    for c in case_list:
        if entry in ("K9", "K9A"):
            s.add(("tile", tiles_of(c["T"]), fill_of(c["T"])))
        elif entry == "K9L":
            s.add(("T", c["T"], _xcd_class(c["B"] * c["H"] * -(-c["T"] // 256))))
        elif entry in ("K9M", "K9B"):
            B, T = c["B"], c["T"]
            if c["lens"] is None:
                s.add(("null", tiles_of(T)))
            else:
                Ls = clamp_lens(c["lens"], B, T)
                for L in Ls:
                    s.add(("tile", tiles_of(T), tiles_of(L), fill_of(L)))
                if len(set(Ls)) > 1:
                    s.add(("mixed", tiles_of(T)))
                s |= {("low",)} if min(c["lens"]) <= 0 else set()
                s |= {("high",)} if max(c["lens"]) > T else set()
            if entry == "K9B":
                s.add(("rel", c["rel"]))
        elif entry == "K9C":
            s.add(("T", c["T"]))
            s |= {("row", n, c["st"][i] // (c["H"] * 64) if c["st"][i] % (c["H"] * 64) == 0 else "W+4") for n, i in (("k", 1), ("v", 3))}
        elif entry == "K30":
            s.add(("shape", c["H"], c["D"], c["T"]) if c["T"] in K30_T else ("hc", c["H"], c["D"], cf_heads_per_pass(c["T"], c["H"], c["D"])))
            u_img, n_row, n_img, m_img = c["st"]
            s |= {(n,) for n, on in (("u_img", u_img > c["H"] * c["D"]), ("n_row", n_row > c["D"]), ("m_img", m_img > c["H"] * c["D"]),
                                     ("n_img", n_img > (c["T"] - 1) * n_row + c["D"])) if on}
        elif entry in ("K10", "K24"):
            s |= {("rows", c["rows"]), ("D", c["D"])}
        elif entry == "K25":
            s |= {("n%4", c["n"] % 4), ("blocks", -(-c["n"] // K25_BLOCK), "whole" if c["n"] % K25_BLOCK == 0 else "part")}
        elif entry == "K26":
            s |= {("n", c["T"] - c["t0"], c["D"])} | ({("strided",)} if c["st"][0] > c["D"] else set())
        elif entry == "K27":
            if c["lens"] is None:
                s.add(("null",))
            else:
                s |= {("n", L, c["D"]) for L in clamp_lens(c["lens"], c["B"], c["T"])}
                s |= {("low",)} if min(c["lens"]) <= 0 else set()
                s |= {("high",)} if max(c["lens"]) > c["T"] else set()
        elif entry == "K28":
            s.add((c["P"], c["lk"]))
        elif entry == "K29":
            s.add((c["D"], c["fill"], c["add"], c["src"]))
        if "regime" in c:
            s.add(("regime", c["regime"]))
    return s


# =========================================================================================================================
# 2. operands and float64 references (from the headers' formulas)
# =========================================================================================================================
def _gen(case, salt=0):
    return torch.Generator().manual_seed(case["ds"] * 16 + salt)


def attention_operands(case, Ls):
    """qkv [B, T, 3*H*64] of the case's value regime (finite throughout) and, for the dominant-key regime, the dominant key
    of every sequence: one of the last tile of its L keys.  Under K9A's mask only the rows that see that key get q = 50 k_j.
    (With q = 50 k_j on every row the rows in front of key j are ONE query vector per head repeated, with scores of +-150 and
    no dominant key among them: the plain rule's yardstick err32 is then a maximum over a single draw, and the MI355X measured
    err = 1.10 x bound on one such case -- 3.9e-5 against 3.5e-5 -- where the N(0, 6) regime, whose scores are as large, stays
    below 0.7.  Those rows keep N(0, 1) queries and are held to the plain rule.)"""
    B, T, H, r = case["B"], case["T"], case["H"], case["regime"]
    g = _gen(case)
    x = torch.randn(B, T, 3, H, 64, generator=g)
    dom = None
    if r[0] == "r" and r[1].isdigit():
        x *= float(r[1:])
    elif r in ("rise", "fall"):                      # score(t, j) = j * (+-0.5) * (1 + noise(t)) + small: every tile / no tile rescales
        e = F.normalize(torch.randn(B, 1, H, 64, generator=g), dim=-1)
        j = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1)
        x[:, :, 0] = 8.0 * e * (1.0 + 0.1 * torch.rand(B, T, H, 1, generator=g)) + 0.3 * x[:, :, 0]
        x[:, :, 1] = e * (j * (0.5 if r == "rise" else -0.5)) + 0.05 * x[:, :, 1]
    elif r == "dominant":                            # test_attention_dominant_key_in_the_last_partial_tile: q = 50 k_j
        dom = [int(torch.randint(32 * (tiles_of(L) - 1), L, (1,), generator=g)) for L in Ls]
        for b, j in enumerate(dom):                  # under the causal mask: the rows that see key j; the rows in front of it keep
            x[b, (j if case["entry"] == "K9A" else 0):, 0] = 50.0 * x[b, j, 1]          # their N(0, 1) queries (the plain rule)
    elif r == "zerok":
        for b, L in enumerate(Ls):
            x[b, int(torch.randint(0, L, (1,), generator=g)), 1] = 0.0
    elif r == "voff":
        x[:, :, 2] += 100.0
    return x.reshape(B, T, 3 * H * 64), dom


def relbias_full(rel, T, Ls):
    """[B, H, T, T]: entry (b, h, t, j) = rel[h, max(j - t, -(L_b - 1)) + T - 1] -- the header's text, padded rows included
    (for t < L_b and j < L_b the clamp never acts)."""
    t = torch.arange(T, device=rel.device)
    d = t[None, :] - t[:, None]                                                    # [t, j] = j - t
    return torch.stack([rel[:, torch.clamp(d, min=-(L - 1)) + T - 1] for L in Ls])


def attention_ref(qkv, H, Ls=None, causal=False, rel=None):
    """softmax(q k^T / 8 [+ bias]) v per head in qkv's dtype: bmm, masked softmax, bmm.  float64 operands: the reference;
    float32 operands: the plain chain whose error is the yardstick (err32)."""
    B, T, _ = qkv.shape
    q, k, v = qkv.reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    if rel is not None:
        s = s + relbias_full(rel, T, Ls or [T] * B)
    t = torch.arange(T, device=qkv.device)
    if Ls is not None:
        keep = t[None, :] < torch.tensor(Ls, device=qkv.device)[:, None]           # [B, j]
        s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill((t[None, :] > t[:, None])[None, None], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, H * 64)


def cls_ref(q, k, v, H):
    """K9C: out[b, h] = softmax_j(q[b, h] . k[b, j, h] / 8) v[b, j, h] in the operands' dtype."""
    B, T, W = k.shape
    s = torch.einsum("bhe,bthe->bht", q.view(B, H, 64), k.view(B, T, H, 64)) / 8.0
    return torch.einsum("bht,bthe->bhe", torch.softmax(s, dim=-1), v.view(B, T, H, 64)).reshape(B, W)


def mix_ref(u, n):
    """K30's own formula (mcd_clsfold.h) in the operands' dtype."""
    s = torch.einsum("bhd,btd->bht", u, n)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    return torch.einsum("bht,btd->bhd", p, n) / p.sum(dim=-1, keepdim=True)


def cls_row_ref(n, w, q, H):
    """Row 0 of softmax(q k^T / 8) v with K | V = n w[D:]^T, in the operands' dtype (test_gpu_cls_fold._row64)."""
    B, T, D = n.shape
    kv = (n @ w[D:].T).view(B, T, 2, H, 64)
    s = torch.einsum("bhe,bthe->bht", q.view(B, H, 64), kv[:, :, 0]) / 8.0
    return torch.einsum("bht,bthe->bhe", torch.softmax(s, dim=-1), kv[:, :, 1]).reshape(B, D)


def mean_replay(rows):
    """K26's order (mcd_tokens.h) in fp32 on rows [B, n, D]: four strided partial sums from +0 in ascending row order,
    ((p0 + p1) + p2) + p3, one division by (float)n."""
    B, n, D = rows.shape
    parts = []
    for w in range(4):
        p = torch.zeros(B, D, dtype=torch.float32, device=rows.device)
        for r in range(w, n, 4):
            p = p + rows[:, r]
        parts.append(p)
    # (a tensor divisor: ATen divides by a device tensor, but multiplies by the reciprocal of a Python scalar on the GPU)
    return (((parts[0] + parts[1]) + parts[2]) + parts[3]) / torch.full((1,), float(n), dtype=torch.float32, device=rows.device)


def masked_mean_l2_replay(x, Ls, normalize):
    """K27's order (mcd_sentence.h) in fp32: K26's mean with n = L; lane l adds the squares of its columns 4 (64 cb + l) + e,
    cb = 0 .. 7, e = 0 .. 3, from +0 (columns >= D count as zero); the xor butterfly 32, 16, 8, 4, 2, 1; den =
    max(sqrtf(sum), 1e-12f); one division."""
    B, T, D = x.shape
    m = torch.cat([mean_replay(x[b:b + 1, :L]) for b, L in enumerate(Ls)])
    return l2_replay(m) if normalize else m


def l2_replay(m):
    """Steps 2 - 4 of K27's order on the means m [B, D]."""
    B, D = m.shape
    x = m
    sq = torch.zeros(B, 2048, dtype=torch.float32, device=x.device)
    sq[:, :D] = m * m
    sq = sq.view(B, 8, 64, 4)                                                       # [cb, lane, e]
    lane = torch.zeros(B, 64, dtype=torch.float32, device=x.device)
    for cb in range(8):
        for e in range(4):
            lane = lane + sq[:, cb, :, e]
    idx = torch.arange(64, device=x.device)
    for s in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, idx ^ s]
    den = torch.clamp(torch.sqrt(lane[:, :1]), min=1e-12)
    return m / den


def patch_rows(x, P):
    """K11's rows without the class-token slot: [B, L, Cin*P*P], patches row-major, (c, dy, dx) inside (mcd_hip.h)."""
    B, Cin, Hh, Ww = x.shape
    nh, nw = Hh // P, Ww // P
    return x.view(B, Cin, nh, P, nw, P).permute(0, 2, 4, 1, 3, 5).reshape(B, nh * nw, Cin * P * P)


def token_restore_ref(src, restore, fill, add, Lk):
    """K29's expression (mcd_mask.h); src [B, 1 + Lk, D] (a shared table already expanded)."""
    r = restore.long()
    if fill is None:
        rows = src[:, 1:].gather(1, r.clamp(0, Lk - 1)[:, :, None].expand(-1, -1, src.shape[2]))
    else:
        padded = torch.cat([src[:, 1:], fill[None, None].expand(src.shape[0], 1, -1)], dim=1)       # row Lk = fill
        rows = padded.gather(1, torch.where(r < Lk, r.clamp(min=0), torch.full_like(r, Lk))[:, :, None].expand(-1, -1, src.shape[2]))
    out = torch.cat([src[:, :1], rows], dim=1)
    return out if add is None else out + add[None]


# =========================================================================================================================
# 3. the checker
# =========================================================================================================================
def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _tag(case):
    return " ".join("%s=%s" % (k, case[k]) for k in case if k not in ("entry", "ds"))


class _Ck:
    def __init__(self, entry, case):
        self.head, self.findings, self.ratio = "%s #%d [%s]" % (entry, case["i"], _tag(case)), [], 0.0

    def note(self, what):
        self.findings.append("%s: %s" % (self.head, what))

    def acc(self, what, err, bound):
        err = float(err)
        self.ratio = max(self.ratio, err / bound) if err == err else float("inf")
        if not err <= bound:
            self.note("%s: err %.3e > bound %.3e" % (what, err, bound))

    def same(self, what, got, want):
        if got.shape != want.shape:
            return self.note("%s: shape %s against %s" % (what, tuple(got.shape), tuple(want.shape)))
        bad = (bits(got) != bits(want)).nonzero()
        if bad.numel():
            self.note("%s: %d elements differ in their bits, the first at %s" % (what, bad.shape[0], tuple(int(v) for v in bad[0])))


def _general(ck, what, out, ref, ref32):
    """The project's rule (test_vit_attention_matches_sdpa, test_gpu_cls_tail): err <= 3e-6 max(1, |ref|max) + 3 err32."""
    err32 = float((ref32.double() - ref).abs().max())
    ck.acc(what, (out.double() - ref).abs().max(), 3e-6 * max(1.0, float(ref.abs().max())) + 3 * err32)


def _check_attention(ck, entry, case, call, dev):
    B, T, H = case["B"], case["T"], case["H"]
    lens = case.get("lens")
    Ls = clamp_lens(lens, B, T) if entry in ("K9M", "K9B") else [T] * B
    masked = Ls if entry in ("K9M", "K9B") else None
    causal = entry == "K9A"
    x, dom = attention_operands(case, Ls)
    x = x.to(dev)
    rel = None
    if case.get("rel") in ("rand", "zero"):
        rel = (torch.randn(H, 2 * T - 1, generator=_gen(case, 1)) * (case["rel"] == "rand")).to(dev)

    def run(name, xx, ll=None, rr=None):
        kw = dict(qkv=xx.contiguous(), H=H)
        if name in ("K9M", "K9B"):
            kw["lens"] = ll
        if name == "K9B":
            kw["rel"] = None if rr is None else rr.contiguous()
        return call(name, **kw)

    out = run(entry, x, lens, rel)
    ref = attention_ref(x.double(), H, masked, causal, None if rel is None else rel.double())
    if dom is not None:           # every row that sees key j is v_j to 3e-6 max|v| (the dominance test's rule); the reference says so too
        v = x.view(B, T, 3, H, 64)[:, :, 2]
        tol = 3e-6 * float(v.abs().max())
        for b, j in enumerate(dom):
            t0 = j if causal else 0
            want = v[b, j].double().reshape(1, H * 64)
            if float((ref[b, t0:] - want).abs().max()) > 1e-9 * max(1.0, float(want.abs().max())):
                ck.note("generator: key %d of sequence %d does not dominate" % (j, b))
            ck.acc("dominant key %d of sequence %d" % (j, b), (out[b, t0:].double() - want).abs().max(), tol)
            if t0:
                ref32 = attention_ref(x[b:b + 1, :t0], H, None, True)
                _general(ck, "rows in front of the dominant key", out[b:b + 1, :t0], ref[b:b + 1, :t0], ref32)
    else:
        _general(ck, "float64", out, ref, attention_ref(x, H, masked, causal, rel))

    # ---- the headers' bit relations
    if entry == "K9L" and T <= 256:
        ck.same("K9L == K9 (T <= 256)", out, run("K9", x))
    if entry == "K9M":
        ck.same("K9M(lens NULL) == K9", run("K9M", x, None), run("K9", x))
        for b, L in enumerate(Ls):
            ck.same("rows < L of sequence %d == K9 truncated to %d" % (b, L), out[b:b + 1, :L], run("K9", x[b:b + 1, :L]))
    if entry == "K9B":
        k9m = run("K9M", x, lens)
        ck.same("K9B(rel NULL) == K9M", run("K9B", x, lens, None), k9m)
        ck.same("K9B(rel zero) == K9M", run("K9B", x, lens, torch.zeros(H, 2 * T - 1, device=dev)), k9m)
        if rel is not None:
            for b, L in enumerate(Ls):
                ck.same("rows < L of sequence %d == the B = 1, T = %d call" % (b, L), out[b:b + 1, :L],
                        run("K9B", x[b:b + 1, :L], [L], rel[:, T - L:T + L - 1]))
    if entry == "K9A":
        ts = sorted({t for t in (0, 31, 32, T - 1, int(torch.randint(0, T, (1,), generator=_gen(case, 2)))) if t < T})
        for t in ts:
            ck.same("row %d == K9 on %d tokens" % (t, t + 1), out[:, t], run("K9", x[:, :t + 1])[:, t])
    if B > 1:
        for b in range(B):
            ck.same("image %d alone" % b, run(entry, x[b:b + 1], None if lens is None else lens[b:b + 1], rel), out[b:b + 1])

    # ---- read sets
    if entry in ("K9M", "K9B") and case["i"] % 4 == 0:
        poisoned = x.clone().view(B, T, 3, H, 64)
        for b, L in enumerate(Ls):
            poisoned[b, L:, 1:] = NAN
        ck.same("NaN in every K and V row >= L", run(entry, poisoned.view(B, T, -1), lens, rel), out)
        if rel is not None:
            far, longest = rel.clone(), max(Ls)
            far[:, :T - longest] = NAN
            far[:, T - 1 + longest:] = NAN
            ck.same("NaN in every rel entry with |d| >= %d" % longest, run(entry, x, lens, far), out)


def _check_k9c(ck, case, call, dev):
    B, T, H = case["B"], case["T"], case["H"]
    W = H * 64
    x, dom = attention_operands(case, [T] * B)
    q, k, v = (t.reshape(B, T, W).to(dev) for t in x.view(B, T, 3, W).unbind(2))
    q = q[:, 0].contiguous()
    out = call("K9C", q=q, k=k, v=v, H=H, st=case["st"])
    ref = cls_ref(q.double(), k.double(), v.double(), H)
    if dom is not None:
        want = torch.stack([v[b, j] for b, j in enumerate(dom)]).double()
        if float((ref - want).abs().max()) > 1e-9 * max(1.0, float(want.abs().max())):
            ck.note("generator: the chosen key does not dominate")
        ck.acc("dominant key", (out.double() - want).abs().max(), 3e-6 * float(v.abs().max()))
    else:
        _general(ck, "float64", out, ref, cls_ref(q, k, v, H))
    if B > 1:
        for b in range(B):
            ck.same("image %d alone" % b, call("K9C", q=q[b:b + 1], k=k[b:b + 1], v=v[b:b + 1], H=H, st=case["st"]), out[b:b + 1])


def _check_k30(ck, case, call, dev):
    """test_gpu_cls_fold._check: K30 on u = W_k^T q log2(e) / 8 (float64, rounded once), W_v applied in float64, against row 0
    of the attention; and K30 against its own formula.  err32: the same row through fp32 K | V = n w^T, softmax, sum."""
    B, T, H, D = case["B"], case["T"], case["H"], case["D"]
    g = _gen(case)
    n = torch.randn(B, T, D, generator=g).to(dev)
    w = (torch.randn(3 * D, D, generator=g) / D ** 0.5).to(dev)
    q = (torch.randn(B, D, generator=g) * case["q_scale"]).to(dev)
    u = (torch.einsum("bhe,hed->bhd", q.double().view(B, H, 64), w[D:2 * D].double().view(H, 64, D)) * (LOG2E / 8.0)).float()
    m = call("K30", u=u, n=n, st=case["st"])
    if not bool(torch.isfinite(m).all()):
        ck.note("m is not finite")
    ref = cls_row_ref(n.double(), w.double(), q.double(), H)
    err32 = float((cls_row_ref(n, w, q, H).double() - ref).abs().max())
    o = torch.einsum("bhd,hed->bhe", m.double(), w[2 * D:].double().view(H, 64, D)).reshape(B, D)
    ck.acc("row 0 of the attention", (o - ref).abs().max(), 3e-6 * max(1.0, float(ref.abs().max())) + 3 * err32)
    m_ref = mix_ref(u.double(), n.double())
    ck.acc("its own formula", (m.double() - m_ref).abs().max(), 3e-6 * max(1.0, float(m_ref.abs().max())) + 3 * err32)
    if B > 1:
        for b in range(B):
            ck.same("image %d alone" % b, call("K30", u=u[b:b + 1], n=n[b:b + 1], st=case["st"]), m[b:b + 1])


def _ln_operands(case, dev):
    g = _gen(case)
    D = case["D"]
    return g, (torch.randn(D, generator=g).to(dev), torch.randn(D, generator=g).to(dev))


def _check_k10(ck, case, call, dev):
    """test_layer_norm_matches_torch's tolerance: 3e-6 max(1, |ref|max) (1 + offset) against float64."""
    rows, D, off, eps = case["rows"], case["D"], case["offset"], case["eps"]
    g, (w, b) = _ln_operands(case, dev)
    x = (torch.randn(rows, D, generator=g) * 2.0 + off).to(dev)
    out = call("K10", x=x, g=w, b=b, eps=eps)
    ref = F.layer_norm(x.double(), (D,), w.double(), b.double(), eps)
    ck.acc("float64", (out.double() - ref).abs().max(), 3e-6 * max(1.0, float(ref.abs().max())) * (1 + off))
    for r in sorted({0, rows // 2, rows - 1}) if rows > 1 else []:
        ck.same("row %d alone" % r, call("K10", x=x[r:r + 1].contiguous(), g=w, b=b, eps=eps), out[r:r + 1])


def _check_k24(ck, case, call, dev):
    rows, D, T, eps = case["rows"], case["D"], case["T"], case["eps"]
    B = rows // T
    g, (w, b) = _ln_operands(case, dev)
    word = (torch.randn(case["vocab"], D, generator=g) * 2.0 + case["offset"]).to(dev)
    pos = torch.randn(T + int(torch.randint(0, 3, (1,), generator=g)), D, generator=g).to(dev)
    typ = torch.randn(case["n_type"], D, generator=g).to(dev)
    ids = torch.randint(0, case["vocab"], (B, T), generator=g).to(dev)
    tids = torch.randint(0, case["n_type"], (B, T), generator=g).to(dev) if case["tids"] else None
    out = call("K24", ids=ids, tids=tids, word=word, pos=pos, typ=typ, g=w, b=b, eps=eps)
    summed = (word[ids] + typ[tids if tids is not None else torch.zeros_like(ids)]) + pos[:T][None]
    ck.same("K24 == K10 on ATen's sum", out, call("K10", x=summed.reshape(rows, D).contiguous(), g=w, b=b, eps=eps))
    if B > 1:
        ck.same("sequence 0 alone", call("K24", ids=ids[:1].contiguous(), tids=None if tids is None else tids[:1].contiguous(),
                                         word=word, pos=pos, typ=typ, g=w, b=b, eps=eps), out[:T])


def _check_k25(ck, case, call, dev):
    """test_k25_against_float64_and_in_place's tolerance (test_gpu_text_tower._bound): nerr <= 2 nerr(ATen fp32) + 1e-6."""
    x = (torch.randn(case["n"], generator=_gen(case)) * 3.0).to(dev)
    out = call("K25", x=x, in_place=False)
    ref = x.double() * torch.sigmoid(1.702 * x.double())
    top = float(ref.abs().max().clamp_min(1e-30))
    aten = x * torch.sigmoid(1.702 * x)
    ck.acc("float64", float((out.double() - ref).abs().max()) / top, 2 * float((aten.double() - ref).abs().max()) / top + 1e-6)
    ck.same("in place", call("K25", x=x, in_place=True), out)


def _check_k26(ck, case, call, dev):
    B, T, D, t0 = case["B"], case["T"], case["D"], case["t0"]
    x = (torch.randn(B, T, D, generator=_gen(case)) * 1.5 + 0.25).to(dev)
    out = call("K26", x=x, t0=t0, st=case["st"])
    ck.same("the header's order replayed in fp32", out, mean_replay(x[:, t0:]))
    if B > 1:
        for b in range(B):
            ck.same("image %d alone" % b, call("K26", x=x[b:b + 1].contiguous(), t0=t0, st=case["st"]), out[b:b + 1])


def _check_k27(ck, case, call, dev):
    B, T, D, lens, nz = case["B"], case["T"], case["D"], case["lens"], case["normalize"]
    Ls = clamp_lens(lens, B, T)
    x = (torch.randn(B, T, D, generator=_gen(case)) * 1.5 + 0.25).to(dev)
    out = call("K27", x=x, lens=lens, normalize=nz)
    ck.same("the header's order replayed in fp32", out, masked_mean_l2_replay(x, Ls, nz))
    if B > 1:
        for b in range(B):
            ck.same("sequence %d alone" % b, call("K27", x=x[b:b + 1].contiguous(), lens=None if lens is None else lens[b:b + 1],
                                                  normalize=nz), out[b:b + 1])
    if case["i"] % 4 == 0:
        poisoned = x.clone()
        for b, L in enumerate(Ls):
            poisoned[b, L:] = NAN
        ck.same("NaN in every row >= L", call("K27", x=poisoned, lens=lens, normalize=nz), out)


def _check_k28(ck, case, call, dev):
    B, Cin, P, hp, wp, Lk = (case[k] for k in ("B", "Cin", "P", "hp", "wp", "Lk"))
    L = hp * wp
    g = _gen(case)
    x = torch.randn(B, Cin, hp * P, wp * P, generator=g).to(dev)
    keep = torch.randint(0, L, (B, Lk), generator=g, dtype=torch.int32)
    if Lk:                                                                   # indices outside [0, L-1]: the header clamps them
        wild = torch.tensor([-1, -1000, L, L + 7, 2 ** 31 - 1, -2 ** 31], dtype=torch.int64)
        hit = torch.rand(B, Lk, generator=g) < 0.3
        keep = torch.where(hit, wild[torch.randint(0, 6, (B, Lk), generator=g)], keep.long()).int()
    keep = keep.to(dev)
    out = call("K28", x=x, keep=keep, P=P)
    full = call("K11", x=x, P=P)
    ck.same("K11 == the permutation", full[:, 1:], patch_rows(x, P))
    rows = full[:, 1:].gather(1, keep.long().clamp(0, L - 1)[:, :, None].expand(-1, -1, Cin * P * P))
    ck.same("K28 == K11 followed by the gather", out, torch.cat([full[:, :1], rows], dim=1))
    if B > 1:
        ck.same("image %d alone" % (B - 1), call("K28", x=x[B - 1:].contiguous(), keep=keep[B - 1:].contiguous(), P=P), out[B - 1:])


def _check_k29(ck, case, call, dev):
    B, D, L, Lk = case["B"], case["D"], case["L"], case["Lk"]
    g = _gen(case)
    shared = case["src"] == "shared"
    src = torch.randn(*((1 + Lk, D) if shared else (B, 1 + Lk, D)), generator=g).to(dev)
    special = torch.tensor([-1, -9, Lk - 1, Lk, Lk + 1, Lk + 50, 0], dtype=torch.int32)
    r = torch.randint(0, max(Lk, 1), (B, L), generator=g, dtype=torch.int32)
    r = torch.where(torch.rand(B, L, generator=g) < 0.5, special[torch.randint(0, 7, (B, L), generator=g)], r)
    r.view(-1)[:min(B * L, 6)] = special[:min(B * L, 6)]                    # r < 0, = Lk - 1, = Lk, > Lk: every kind in every case
    r = r.to(dev)
    fill = torch.randn(D, generator=g).to(dev) if case["fill"] else None
    add = torch.randn(1 + L, D, generator=g).to(dev) if case["add"] else None
    out = call("K29", src=src, pad=case["pad"], restore=r, fill=fill, add=add)
    ck.same("the header's expression", out, token_restore_ref(src[None].expand(B, -1, -1) if shared else src, r, fill, add, Lk))
    if B > 1:
        ck.same("image %d alone" % (B - 1), call("K29", src=src if shared else src[B - 1:].contiguous(), pad=case["pad"],
                                                 restore=r[B - 1:].contiguous(), fill=fill, add=add), out[B - 1:])


def check(entry, case, call, device="cpu"):
    """(findings, the largest err / bound of the case's accuracy checks -- 0.0 for an entry that is held to bits alone)."""
    ck = _Ck(entry, case)
    try:
        if entry in ATTENTION:
            _check_attention(ck, entry, case, call, device)
        else:
            {"K9C": _check_k9c, "K30": _check_k30, "K10": _check_k10, "K24": _check_k24, "K25": _check_k25, "K26": _check_k26,
             "K27": _check_k27, "K28": _check_k28, "K29": _check_k29}[entry](ck, case, call, device)
    except AssertionError as e:                      # a frame that did not come back intact, an entry that returned an error
        ck.note("the call failed: %s" % (e,))
    return ck.findings, ck.ratio


def run(entry, case_list, call, device="cpu", progress=None):
    """check() over a list: (all findings, the largest err / bound)."""
    findings, top = [], 0.0
    for i, c in enumerate(case_list):
        f, r = check(entry, c, call, device)
        findings += f
        top = max(top, r)
        if progress:
            progress(i, f, top)
    return findings, top


# =========================================================================================================================
# 4. the library behind call(): every operand in a frame (GPU only; nothing above needs it)
# =========================================================================================================================
def _ptr(a):
    return None if a is None else a.ptr


def _finish(name, o, ins):
    """The output frame o after the call: its guards intact, every logical element written, the input frames `ins` unchanged;
    returns a copy of the logical region."""
    import util
    out = o.view.clone()
    o.check(out, what=name)
    fill_bits = int(util.int_bits(torch.full((1,), util.OUT_FILL))[0])
    assert not bool((util.int_bits(out) == fill_bits).any()), "%s: an output element was not written" % name
    for a in ins:
        if a is not None:
            a.same()
    return out


def gpu_call(L):
    """call(name, ...) on libmcd_hip.so: inputs through In / Strided of test_gpu_encoder_frames with NaN in their guards and
    gaps (LENS_GAP around index lists), outputs in OUT_FILL frames.  The guards must come back intact, every logical element
    written, the inputs unchanged (AssertionError otherwise: check() reports it)."""
    import test_gpu_encoder_frames as EF
    import util

    def ints(values, dev, dtype=torch.int32):
        return None if values is None else EF.In(torch.as_tensor(values, dtype=dtype, device=dev), LENS_GAP)

    ptr, finish = _ptr, _finish

    def rows3(t, row, img):
        return EF.Strided(t, row, img, NAN)

    def call(name, **a):
        st = EF.st()
        if name in ("K9", "K9L", "K9A", "K9M", "K9B"):
            qkv, H = a["qkv"], a["H"]
            B, T, _ = qkv.shape
            x_, o_ = EF.In(qkv, NAN), EF.Out((B, T, H * 64), qkv.device)
            l_ = ints(a.get("lens"), qkv.device)
            r_ = None if a.get("rel") is None else EF.In(a["rel"], NAN)
            if name == "K9M":
                rc = L.mcd_vit_attention_keylen(x_.ptr, B, T, H, ptr(l_), o_.ptr, st)
            elif name == "K9B":
                rc = L.mcd_vit_attention_relbias(x_.ptr, B, T, H, ptr(l_), ptr(r_), o_.ptr, st)
            else:
                entry = {"K9": L.mcd_vit_attention, "K9L": L.mcd_vit_attention_long, "K9A": L.mcd_vit_attention_causal}[name]
                rc = entry(x_.ptr, B, T, H, o_.ptr, st)
            EF.ok(rc, L)
            return finish(name, o_, (x_, l_, r_))
        if name == "K9C":
            q, k, v, H = a["q"], a["k"], a["v"], a["H"]
            B, T, W = k.shape
            q_img, k_row, k_img, v_row, v_img = a["st"]
            q_, k_, v_ = rows3(q.view(B, 1, W), W, q_img), rows3(k, k_row, k_img), rows3(v, v_row, v_img)
            o_ = EF.Out((B, W), k.device)
            EF.ok(L.mcd_vit_attention_cls(q_.ptr, q_img, k_.ptr, k_row, k_img, v_.ptr, v_row, v_img, B, T, H, o_.ptr, st), L)
            return finish(name, o_, (q_, k_, v_))
        if name == "K30":
            u, n = a["u"], a["n"]
            (B, H, D), T = u.shape, n.shape[1]
            u_img, n_row, n_img, m_img = a["st"]
            u_, n_ = rows3(u.reshape(B, 1, H * D), H * D, u_img), rows3(n, n_row, n_img)
            o_ = util.FramedOut(B, H * D, m_img, 0, torch.float32, n.device)
            EF.ok(L.mcd_cls_token_mix(u_.ptr, u_img, n_.ptr, n_row, n_img, B, T, H, D, o_.ptr, m_img, st), L)
            return finish(name, o_, (u_, n_)).view(B, H, D)
        if name == "K10":
            x = a["x"]
            ins = [EF.In(t, NAN) for t in (x, a["g"], a["b"])]
            o_ = EF.Out(tuple(x.shape), x.device)
            EF.ok(L.mcd_layer_norm(ins[0].ptr, x.shape[0], x.shape[1], ins[1].ptr, ins[2].ptr, a["eps"], o_.ptr, st), L)
            return finish(name, o_, ins)
        if name == "K24":
            ids, word = a["ids"], a["word"]
            (B, T), D = ids.shape, word.shape[1]
            i_, t_ = ints(ids, word.device, torch.int64), ints(a["tids"], word.device, torch.int64)
            ins = [EF.In(a[k], NAN) for k in ("word", "pos", "typ", "g", "b")]
            o_ = EF.Out((B * T, D), word.device)
            EF.ok(L.mcd_text_embed_ln(i_.ptr, ptr(t_), ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, a["eps"], B * T, T, D,
                                      word.shape[0], a["typ"].shape[0], o_.ptr, st), L)
            return finish(name, o_, ins + [i_, t_])
        if name == "K25":
            x = a["x"]
            if a["in_place"]:
                y_ = EF.In(x, util.OUT_FILL)
                EF.ok(L.mcd_quick_gelu(y_.ptr, x.numel(), y_.ptr, st), L)
                y_.check = lambda e, what="": util.check_frame(y_.flat, y_.spec, e, what=str(what))
                return finish(name, y_, ())
            x_, o_ = EF.In(x, NAN), EF.Out(tuple(x.shape), x.device)
            EF.ok(L.mcd_quick_gelu(x_.ptr, x.numel(), o_.ptr, st), L)
            return finish(name, o_, (x_,))
        if name == "K26":
            x = a["x"]
            B, T, D = x.shape
            x_tok, x_img, out_img = a["st"]
            x_, o_ = rows3(x, x_tok, x_img), util.FramedOut(B, D, out_img, 0, torch.float32, x.device)
            EF.ok(L.mcd_token_mean(x_.ptr, B, T, D, x_img, x_tok, a["t0"], o_.ptr, out_img, st), L)
            return finish(name, o_, (x_,))
        if name == "K27":
            x = a["x"]
            B, T, D = x.shape
            x_, l_, o_ = EF.In(x, NAN), ints(a["lens"], x.device), EF.Out((B, D), x.device)
            EF.ok(L.mcd_masked_mean_l2(x_.ptr, B, T, D, ptr(l_), int(a["normalize"]), o_.ptr, st), L)
            return finish(name, o_, (x_, l_))
        if name in ("K11", "K28"):
            x, P = a["x"], a["P"]
            B, Cin, Hh, Ww = x.shape
            x_ = EF.In(x, NAN)
            if name == "K11":
                o_ = EF.Out((B, 1 + (Hh // P) * (Ww // P), Cin * P * P), x.device)
                EF.ok(L.mcd_patchify(x_.ptr, B, Cin, Hh, Ww, P, o_.ptr, st), L)
                return finish(name, o_, (x_,))
            keep = a["keep"]
            k_ = EF.In(keep, LENS_GAP) if keep.numel() else None
            o_ = EF.Out((B, 1 + keep.shape[1], Cin * P * P), x.device)
            EF.ok(L.mcd_patchify_kept(x_.ptr, ptr(k_), B, Cin, Hh, Ww, P, keep.shape[1], o_.ptr, st), L)
            return finish(name, o_, (x_, k_))
        if name == "K29":
            src, r = a["src"], a["restore"]
            (B, Lr), D = r.shape, src.shape[-1]
            if src.dim() == 2:
                s_, src_img = EF.In(src, NAN), 0
            else:
                src_img = src.shape[1] * D + a["pad"]
                s_ = rows3(src.reshape(B, 1, src.shape[1] * D), src.shape[1] * D, src_img)
            r_ = EF.In(r, LENS_GAP)
            f_, a_ = (None if a[k] is None else EF.In(a[k], NAN) for k in ("fill", "add"))
            o_ = EF.Out((B, 1 + Lr, D), src.device)
            EF.ok(L.mcd_token_restore(s_.ptr, src_img, r_.ptr, ptr(f_), ptr(a_), B, Lr, src.shape[-2] - 1, D, o_.ptr, st), L)
            return finish(name, o_, (s_, r_, f_, a_))
        raise KeyError(name)

    return call
