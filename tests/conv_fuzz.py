"""The convolution-side fuzzer, the twin of tests/encoder_fuzz.py for the channels-last towers -- EfficientNet (K12 - K15, K0n),
ResNet (K16 - K18, K18 with a residual: K18R), CLIP-RN (K19 - K21) -- and the Swin pair (K31, K32): stratified case lists built
from each kernel's own tiling, float64 references written from the headers (include/mcd_hip.h, include/mcd_swin.h), the
headers' bit relations, read sets, and a checker that takes the entries as a callable.  Importing this module touches no GPU.

  cases(entry, seed)        a deterministic list of plain dicts: every stratum first (strata() names them), the rest from the
                            seeded generator.  SEEDS holds the seeds the tests are committed to.
  check(entry, case, call)  draws the operands, calls call(name, **operands) and returns (findings, err / bound).  The same
                            checker runs on the library (gpu_call: every operand in a frame of test_gpu_encoder_frames) and on
                            the fp32 torch emulations of tests/test_conv_fuzz_cpu.py.

What call(name, ...) is given, per name (tensors on the device check() was given, in the kernels' own layouts):
  K12   x [B, Cin, H, W], w [Cin, 3, 3, Cout], b [Cout]                               -> [B, ceil(H/2), ceil(W/2), Cout]
  K13   x [B, H, W, C], w [k*k, C], b [C], k, s, silu_in                             -> (y [B, Ho, Wo, C], psum [B, T, C])
  K14   psum [B, T, C], hw, wr [sq, C], br [sq], wet [sq, C], be [C]                  -> [B, C]
  K15   y [B, HW, C], s [B, C]  (in place in the library)                             -> [B, HW, C]
  K0N   x [B, HW, C], mode ("avg" | "max" | "silu_avg"), place = (row0, col0, neuron_major)   -> [B, C]
  K0    x [B, C, HW], mode ("avg" | "max")      (mcd_hook_pool, what K0N must equal)   -> [B, C]
  K16   x [B, Cin, H, W], w [Cin, 7, 7, Cout]                                         -> [B, Ho, Wo, Cout]
  K17   x [B, H, W, C], scale [C], shift [C]                                          -> [B, Ho, Wo, C]
  K18   x [B, H, W, Cin], w [Cout, k*k*Cin], b [Cout], k, s, relu_in, relu_out        -> [B, Ho, Wo, Cout]
  K18R  the same and res ([B, Ho, Wo, Cout] | None)                                   -> [B, Ho, Wo, Cout]
  K19   x [B, Cin, H, W], w [Cin, 3, 3, Cout], b [Cout], relu                         -> [B, Ho, Wo, Cout]
  K20   x [B, H, W, C]                                                                -> [B, H // 2, W // 2, C]
  K21   x [B, HW, C], pos [HW + 1, C]                                                 -> [B, HW + 1, C]
  K31   qkv [B, H*W, 3*heads*32], pad ([3*heads*32] | None), H, W, heads, w, s, table -> [B, H*W, heads*32]
  K32   x [B, H*W, C], H, W, g [4C], b [4C], eps                                      -> [B, ceil(H/2)*ceil(W/2), 4C]
  K10   x [rows, D], g, b, eps  (mcd_layer_norm, what K32 must equal)                 -> [rows, D]

Only inputs the headers define are drawn (finite values; a NaN only where the header says where it goes)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import encoder_fuzz as E
from encoder_fuzz import NAN, _Ck, _finish, _gen, _general, _pick, _ptr

TOWERS = ("K12", "K13", "K14", "K15", "K0N", "K16", "K17", "K18", "K18R", "K19", "K20", "K21")
SWIN = ("K31", "K32")
ENTRIES = TOWERS + SWIN
SEEDS = {e: 8001 + i for i, e in enumerate(ENTRIES)}          # the committed seed of every entry's test

# items (one thread's unit of work) a capped grid covers in one trip: cap * 256 threads (k_mbconv.hip, k_resnet.hip,
# k_clip_rn.hip: grid_for(items, 256, cap); K15: grid_for(quads, 1024, 1024) -- the cap is reached past 1024 * 1024 quads and
# the stride is then 1024 * 256)
GRID_ITEMS = {"K12": 2048 * 256, "K15": 1024 * 1024, "K17": 4096 * 256, "K20": 4096 * 256}
K12_COUT = (4, 48)
K13_KS = ((3, 1), (3, 2), (5, 1), (5, 2))
K13_OUT = ((8, 8), (1, 9), (7, 15), (16, 9), (17, 15), (9, 17), (2, 3), (3, 1), (15, 16), (4, 4))      # (Ho, Wo)
K14_T = (1, 15, 16, 17, 33)
K14_C = (4, 60, 64, 68, 260, 1028)
K14_SQ = (1, 3, 4, 5, 9)
K15_NQ = (1, 3, 60, 64)
K0N_HW = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260)
K0N_C = (64, 1, 63, 65, 127, 128)
K0N_MODES = ("avg", "max", "silu_avg")
STEM_COUT = (4, 8, 36, 32, 64)
K17_NQ = (1, 5, 16)
K17_REGIMES = ("unit", "rand", "negwin")
K18_KS = ((3, 1), (3, 2), (1, 2))
K18_COUT = (32, 64, 96, 128, 160, 256)
K18_FILL = (0, 1, 63, 64, 65, 127)
K18_CIN = {1: (32, 256, 288), 3: (32, 64, 128)}             # k-steps k*k*Cin/32 = 1, 8, 9 and 9, 18, 36
K18_REGIMES = ("exact", "randn", "offset", "dead")
K18R_REGIMES = K18_REGIMES + ("negres",)
K21_HW = (1, 2, 3, 4, 5, 49, 50)
K21_C = (4, 252, 256, 260, 2048)
K31_AXIS = ("exact", "pad1", "padw1", "one", "three")
K31_HEADS = (1, 2, 3, 5)
K31_REGIMES = ("r1", "r6", "table20", "dominant")
K32_C = (4, 8, 96, 260, 512)
K32_HW = ((1, 1), (1, 6), (1, 7), (2, 2), (3, 5), (4, 6), (5, 4), (6, 7), (7, 1), (14, 14))


def k13_qmax(k, s):
    """The most channel quads a K13 workgroup stages: mcd_dwconv_bn_silu's qmax = clamp(40960 / (it * it * 16), 1, 16) with
    it = 7 s + k, the input window's edge -- 16, 8, 16 and 7 for (3, 1), (3, 2), (5, 1) and (5, 2); the coverage test holds
    this restatement to those four values."""
    it = 7 * s + k
    return max(1, min(16, 40960 // (it * it * 16)))


def k13_slices(nq, k, s):
    """(slices, quads a slice), as the entry cuts nq channel quads."""
    n = -(-nq // k13_qmax(k, s))
    return n, -(-nq // n)


def same_pad(n, k, s):
    """TF-SAME padding of one axis (mcd_hip.h): (output size, pad in front -- the smaller half --, pad behind)."""
    o = -(-n // s)
    p = max((o - 1) * s + k - n, 0)
    return o, p // 2, p - p // 2


def k18_out(n, k, s):
    return (n + 2 * (k == 3) - k) // s + 1


def stem_out(n):
    return (n - 1) // 2 + 1


_K18_SHAPES = {}


def k18_shapes(k, s):
    """{(pixel tiles, B Ho Wo mod 128): [(B, H, W), ...]} over B <= 4 and sides <= 40, for the fills of K18_FILL and 1 - 3 tiles."""
    if (k, s) not in _K18_SHAPES:
        d = {}
        for B in range(1, 5):
            for H in range(1, 41):
                for W in range(1, 41):
                    M = B * k18_out(H, k, s) * k18_out(W, k, s)
                    if M <= 384 and M % 128 in K18_FILL:
                        d.setdefault((-(-M // 128), M % 128), []).append((B, H, W))
        _K18_SHAPES[(k, s)] = d
    return _K18_SHAPES[(k, s)]


# =========================================================================================================================
# 1. cases
# =========================================================================================================================
def _side(rng, kind):
    if kind == "odd":
        return int(rng.integers(2, 20)) * 2 + 1
    if kind == "even":
        return int(rng.integers(2, 21)) * 2
    return int(kind)


def _k12_cases(rng):
    out, kinds, i = [], ("odd", "even", 1, 2), 0
    for cin in range(1, 5):
        for cout in K12_COUT:
            out.append(dict(B=int(rng.integers(1, 4)), Cin=cin, H=_side(rng, kinds[i % 4]), W=_side(rng, kinds[(i // 4 + i + 1) % 4]),
                            Cout=cout))
            i += 1
    out.append(dict(B=1, Cin=3, H=420, W=420, Cout=48, big=True))                     # 529 200 items against 524 288
    for _ in range(4):
        out.append(dict(B=int(rng.integers(1, 5)), Cin=int(rng.integers(1, 5)), H=int(rng.integers(1, 41)), W=int(rng.integers(1, 41)),
                        Cout=4 * int(rng.integers(1, 13))))
    return out


def _k13_cases(rng):
    out = []
    for k, s in K13_KS:
        q = k13_qmax(k, s)
        for nq in (1, 3, q, q + 1, 2 * q + 1):
            i = len(out)
            Ho, Wo = K13_OUT[i % len(K13_OUT)]
            par = (i // 2) % 2                                                        # stride 2: an odd side (2 o - 1) or an even one
            H, W = (Ho, Wo) if s == 1 else (2 * Ho - par, 2 * Wo - (1 - par))
            out.append(dict(B=int(rng.integers(1, 4)), H=H, W=W, C=4 * nq, k=k, s=s, silu_in=(i + i // 4) % 2))
    for _ in range(6):
        k, s = _pick(rng, K13_KS)
        out.append(dict(B=int(rng.integers(1, 5)), H=int(rng.integers(1, 41)), W=int(rng.integers(1, 41)), C=4 * int(rng.integers(1, 40)),
                        k=k, s=s, silu_in=int(rng.integers(0, 2))))
    return out


def _k14_cases(rng):
    out = []
    for i in range(10):
        T = K14_T[i % 5]
        out.append(dict(B=int(rng.integers(1, 5)), T=T, C=K14_C[i % 6], sq=K14_SQ[(2 * i) % 5], hw=7 * T + int(rng.integers(0, 9))))
    out.append(dict(B=2, T=3, C=16380, sq=4, hw=150))                                 # C + sq = 16384, the limit
    for _ in range(4):
        T = int(rng.integers(1, 40))
        out.append(dict(B=int(rng.integers(1, 5)), T=T, C=4 * int(rng.integers(1, 300)), sq=int(rng.integers(1, 12)),
                        hw=int(rng.integers(1, 64 * T + 1))))
    return out


def _k15_cases(rng):
    out = []
    for nq in K15_NQ:
        for m in (0, 1, 1023):
            hw = [v for v in range(1, 1601) if (v * nq) % 1024 == m]
            if hw:                                                                    # (60 v and 64 v are multiples of 4: only 0)
                out.append(dict(B=int(rng.integers(1, 4)), HW=int(_pick(rng, hw[:3])), C=4 * nq))
    out.append(dict(B=1, HW=1025, C=4096, big=True))                                  # 1 049 600 quads; the stride 262 144 = 256 nq
    out.append(dict(B=1, HW=349526, C=12, big=True))                                  # 1 048 578 quads; 262 144 mod 3 = 1
    for _ in range(4):
        out.append(dict(B=int(rng.integers(1, 5)), HW=int(rng.integers(1, 1601)), C=4 * int(rng.integers(1, 80))))
    return out


def _k0n_cases(rng):
    out = []
    for i, hw in enumerate(K0N_HW):
        for j, mode in enumerate(K0N_MODES):
            n = 3 * i + j
            out.append(dict(B=int(rng.integers(1, 5)), HW=hw, C=K0N_C[(n + n // 6) % 6], mode=mode,
                            place=((0, 2)[n % 2], (0, 3)[(n // 2) % 2], bool((n // 4 + n) % 2)), nan=bool(mode == "max" and i % 2)))
    return out


def _stem_cases(entry, rng):
    shapes = []

    def side(tiles, mod, even):
        return 2 * (16 * (tiles - 1) + (mod or 16)) - 1 + even

    combos = [(t, m) for t in (1, 2, 3) for m in (0, 1, 15)]
    for i, (t, m) in enumerate(combos):
        t2, m2 = combos[(2 * i + 1) % 9]
        shapes.append((side(t, m, i % 2), side(t2, m2, (i // 2) % 2)))
    shapes += [(1, 1), (1, 2), (2, 1), (2, 7), (6, 1)]
    shapes += [(int(rng.integers(1, 41)), int(rng.integers(1, 41))) for _ in range(4)]
    out = []
    for i, (H, W) in enumerate(shapes):
        c = dict(B=1 + i % (2 if max(H, W) > 40 else 4), Cin=1 + i % 4, H=H, W=W, Cout=STEM_COUT[i % 5], regime=("exact", "randn")[(i + i // 2) % 2])
        if entry == "K19":
            c["relu"] = (i // 3 + i) % 2
        if max(H, W) > 40:
            c["big"] = True                        # three 16-pixel tiles a side need an output side >= 33
        out.append(c)
    return out


def _k17_cases(rng):
    out, kinds = [], (1, 2, 3, "odd", "even")
    for i in range(15):
        out.append(dict(B=int(rng.integers(1, 4)), H=_side(rng, kinds[i % 5]), W=_side(rng, kinds[(2 * i + i // 5) % 5]), C=4 * K17_NQ[i % 3],
                        regime=K17_REGIMES[(i + i // 3) % 3]))
    out.append(dict(B=1, H=515, W=515, C=64, regime="unit", big=True))                # 1 065 024 items against 1 048 576
    return out


def _k18_cases(entry, rng):
    out = []
    regs = K18R_REGIMES if entry == "K18R" else K18_REGIMES

    def add(B, H, W, Cin, Cout, k, s):
        i = len(out)
        r = regs[i % len(regs)]
        f = (i // len(regs) + i) % 4
        out.append(dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=s, relu_in=1 if r == "dead" else f >> 1, relu_out=f & 1, regime=r))

    for k, s in K18_KS:                                                               # every instance
        for Cout in K18_COUT:
            add(int(rng.integers(1, 4)), int(rng.integers(1, 13)), int(rng.integers(1, 13)), 32, Cout, k, s)
    for tiles in (1, 2, 3):                                                           # the last pixel tile's fill
        for fill in K18_FILL:
            ok = [ks for ks in K18_KS if (tiles, fill) in k18_shapes(*ks)]
            if ok:
                k, s = ok[int(rng.integers(len(ok)))]
                B, H, W = _pick(rng, k18_shapes(k, s)[(tiles, fill)])
                add(B, H, W, 32, int(_pick(rng, K18_COUT)), k, s)
    add(3, 7, 7, 32, 64, 3, 1)                                                        # 49 pixels an image: one tile, three images
    add(2, 13, 13, 32, 32, 3, 2)                                                      # and under stride 2
    for k in (1, 3):                                                                  # the k-steps
        for Cin in K18_CIN[k]:
            add(int(rng.integers(1, 3)), int(rng.integers(3, 10)), int(rng.integers(3, 10)), Cin, int(_pick(rng, (32, 64, 128))), k,
                2 if k == 1 else 1 + int(rng.integers(0, 2)))
    for i, (H, W) in enumerate(((1, 1), (1, 9), (2, 2), (3, 2), (8, 3), (2, 11), (7, 8), (10, 5))):          # geometry
        k, s = K18_KS[1 + i % 2] if i >= 4 else K18_KS[i % 3]
        add(int(rng.integers(1, 5)), H, W, 32, 64, k, s)
    for _ in range(4):
        k, s = _pick(rng, K18_KS)
        add(int(rng.integers(1, 5)), int(rng.integers(1, 21)), int(rng.integers(1, 21)), 32 * int(rng.integers(1, 4)),
            32 * int(rng.integers(1, 7)), k, s)
    return out


def _k20_cases(rng):
    out = [dict(B=int(rng.integers(1, 4)), H=H, W=W, C=C) for H, W, C in ((2, 2, 4), (9, 11, 32), (8, 10, 8), (7, 6, 20), (6, 7, 4), (1, 5, 8),
                                                                          (6, 1, 4), (1, 1, 4), (3, 2, 260))]
    out.append(dict(B=1, H=1024, W=1028, C=16, big=True))                             # 1 052 672 items against 1 048 576
    out += [dict(B=int(rng.integers(1, 5)), H=int(rng.integers(1, 41)), W=int(rng.integers(1, 41)), C=4 * int(rng.integers(1, 40))) for _ in range(4)]
    return out


def _k21_cases(rng):
    out = [dict(B=int(rng.integers(1, 5)), HW=K21_HW[i % 7], C=K21_C[i % 5]) for i in range(14)]
    out += [dict(B=int(rng.integers(1, 5)), HW=int(rng.integers(1, 200)), C=4 * int(rng.integers(1, 100))) for _ in range(4)]
    return out


def k31_axis(kind, w, nw):
    """A grid side of its kind under window w: an exact multiple, padded by 1, padded by w - 1, one window, three or more."""
    if kind == "pad1" and w > 1:
        return w * nw - 1
    if kind == "padw1" and w > 1:
        return w * (nw - 1) + 1
    if kind == "one":
        return w
    if kind == "three":
        return 2 * w + 1 if w > 1 else 3
    return w * nw


def k31_axis_kinds(n, w):
    Hp = -(-n // w) * w
    s = {"exact"} if n == Hp else set()
    s |= {"pad1"} if Hp - n == 1 else set()
    s |= {"padw1"} if w > 1 and Hp - n == w - 1 else set()
    s |= {"one"} if Hp == w else set()
    s |= {"three"} if Hp >= 3 * w else set()
    return s


def _k31_cases(rng):
    out = []
    for w in range(1, 9):
        for s in range(w):
            i = len(out)
            H = k31_axis(K31_AXIS[i % 5], w, 1 + i % 3)
            W = k31_axis(K31_AXIS[(2 * i + i // 5) % 5], w, 1 + (i // 2) % 3)
            out.append(dict(B=1 + i % 3, H=H, W=W, heads=K31_HEADS[(i + i // 4) % 4], w=w, s=s, regime=K31_REGIMES[(i + i // 3) % 4],
                            pad_null=bool(H % w == 0 and W % w == 0 and i % 2 == 0)))
    for _ in range(6):
        w = int(rng.integers(1, 9))
        out.append(dict(B=int(rng.integers(1, 4)), H=int(rng.integers(1, 25)), W=int(rng.integers(1, 25)), heads=int(_pick(rng, K31_HEADS)), w=w,
                        s=int(rng.integers(0, w)), regime=str(_pick(rng, K31_REGIMES)), pad_null=False))
    return out


def _k32_cases(rng):
    out = [dict(B=1 + i % 3, H=H, W=W, C=K32_C[i % 5]) for i, (H, W) in enumerate(K32_HW)]
    out += [dict(B=int(rng.integers(1, 5)), H=int(rng.integers(1, 21)), W=int(rng.integers(1, 21)), C=4 * int(rng.integers(1, 129)))
            for _ in range(4)]
    return out


def cases(entry, seed):
    rng = np.random.default_rng([int(seed), 100 + ENTRIES.index(entry)])
    if entry in ("K16", "K19"):
        out = _stem_cases(entry, rng)
    elif entry in ("K18", "K18R"):
        out = _k18_cases(entry, rng)
    else:
        out = {"K12": _k12_cases, "K13": _k13_cases, "K14": _k14_cases, "K15": _k15_cases, "K0N": _k0n_cases, "K17": _k17_cases,
               "K20": _k20_cases, "K21": _k21_cases, "K31": _k31_cases, "K32": _k32_cases}[entry](rng)
    for i, c in enumerate(out):
        c.update(entry=entry, i=i, ds=int(seed) * 100003 + 977 * (100 + ENTRIES.index(entry)) + i)
    return out


def random_cases(entry, count, seed):
    """`count` cases for the command line: the stratified lists of consecutive seeds, one after the other."""
    out, s = [], int(seed)
    while len(out) < count:
        out += cases(entry, s)
        s += 1
    return out[:count]


def _par(n):
    return "odd" if n % 2 else "even"


def strata(entry, case_list):
    """The strata a case list covers, as a set of tuples (tests/test_conv_fuzz_cpu.py holds the committed lists to the full sets)."""
    s = set()
    for c in case_list:
        if entry == "K12":
            s |= {("cin", c["Cin"]), ("cout", c["Cout"]), ("parity", c["H"] % 2, c["W"] % 2)} | {("side", v) for v in (c["H"], c["W"]) if v <= 2}
            s |= {("overcap",)} if same_pad(c["H"], 3, 2)[0] * same_pad(c["W"], 3, 2)[0] * (c["Cout"] // 4) > GRID_ITEMS[entry] else set()
        elif entry == "K13":
            k, st, nq = c["k"], c["s"], c["C"] // 4
            Ho, Wo = same_pad(c["H"], k, st)[0], same_pad(c["W"], k, st)[0]
            q = k13_qmax(k, st)
            s |= {("inst", k, st, n) for n, v in (("1", 1), ("3", 3), ("qmax", q), ("qmax+1", q + 1), ("2qmax+1", 2 * q + 1)) if nq == v}
            s |= {("mod", "y", Ho % 8), ("mod", "x", Wo % 8), ("T", -(-Ho // 8) * -(-Wo // 8)), ("silu", c["silu_in"])}
            s |= {("below_k",)} if min(c["H"], c["W"]) < k else set()
            s |= {("s2", _par(c["H"])), ("s2", _par(c["W"]))} if st == 2 else set()
            s |= {("idle",)} if 256 % k13_slices(nq, k, st)[1] else set()
        elif entry == "K14":
            s |= {("T", c["T"]), ("C", c["C"]), ("sq", c["sq"])} | ({("limit",)} if c["C"] + c["sq"] == 16384 else set())
        elif entry == "K15":
            nq, n4 = c["C"] // 4, c["HW"] * c["C"] // 4
            s |= {("nq", nq), ("mod", n4 % 1024)} | ({("overcap", (1024 * 256) % nq != 0)} if n4 > GRID_ITEMS[entry] else set())
        elif entry == "K0N":
            row0, col0, nm = c["place"]
            s |= {("HW", c["HW"]), ("C%64", c["C"] % 64), ("mode", c["mode"]), ("row0", row0 > 0), ("col0", col0 > 0), ("neuron_major", nm)}
        elif entry in ("K16", "K19"):
            Ho, Wo = stem_out(c["H"]), stem_out(c["W"])
            s |= {("cout", c["Cout"]), ("cin", c["Cin"]), ("mod", "y", Ho % 16), ("mod", "x", Wo % 16), ("tiles", "y", -(-Ho // 16)),
                  ("tiles", "x", -(-Wo // 16)), ("parity", _par(c["H"])), ("parity", _par(c["W"])), ("regime", c["regime"])}
            s |= {("side", v) for v in (c["H"], c["W"]) if v <= 2} | ({("relu", c["relu"])} if entry == "K19" else set())
        elif entry == "K17":
            s |= {("H", v) for v in (c["H"] if c["H"] <= 3 else _par(c["H"]),)} | {("W", v) for v in (c["W"] if c["W"] <= 3 else _par(c["W"]),)}
            s |= {("nq", c["C"] // 4), ("regime", c["regime"])}
            s |= {("overcap",)} if stem_out(c["H"]) * stem_out(c["W"]) * (c["C"] // 4) > GRID_ITEMS[entry] else set()
        elif entry in ("K18", "K18R"):
            k, st = c["k"], c["s"]
            HoWo = k18_out(c["H"], k, st) * k18_out(c["W"], k, st)
            M = c["B"] * HoWo
            s |= {("inst", k, st, c["Cout"]), ("fill", M % 128), ("tiles", -(-M // 128)), ("fill", -(-M // 128), M % 128),
                  ("ksteps", k * k * c["Cin"] // 32), ("relu", c["relu_in"], c["relu_out"]), ("regime", c["regime"])}
            s |= {("span",)} if any((b * HoWo) % 128 for b in range(1, c["B"])) else set()
            s |= {("span16",)} if any((b * HoWo) % 16 for b in range(1, c["B"])) else set()
            s |= {("side", v) for v in (c["H"], c["W"]) if v <= 3}
            s |= {("s2", _par(c["H"])), ("s2", _par(c["W"]))} if st == 2 else set()
        elif entry == "K20":
            s |= {("parity", c["H"] % 2, c["W"] % 2)} | ({("empty",)} if min(c["H"], c["W"]) == 1 else set())
            s |= {("overcap",)} if (c["H"] // 2) * (c["W"] // 2) * (c["C"] // 4) > GRID_ITEMS[entry] else set()
        elif entry == "K21":
            s |= {("HW", c["HW"]), ("C", c["C"])}
        elif entry == "K31":
            s |= {("ws", c["w"], c["s"]), ("heads", c["heads"]), ("B", c["B"]), ("regime", c["regime"])}
            s |= {("axis", a) for n in (c["H"], c["W"]) for a in k31_axis_kinds(n, c["w"])} | ({("pad_null",)} if c["pad_null"] else set())
        elif entry == "K32":
            s |= {("parity", c["H"] % 2, c["W"] % 2), ("C", c["C"])} | ({("1x1",)} if (c["H"], c["W"]) == (1, 1) else set())
            s |= {("1xn",)} if c["H"] == 1 and c["W"] > 1 else set()
    return s


# =========================================================================================================================
# 2. float64 references (from the headers' formulas; the operands' dtype decides the precision)
# =========================================================================================================================
def nerr(got, ref):
    """max |got - ref| / max |ref| in float64 (util.nerr)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def relu_keep(t):
    """The kernels' ReLU: v < 0 ? 0 : v (a NaN and a -0 stay)."""
    return torch.where(t < 0, torch.zeros_like(t), t)


def silu(t):
    return t / (1.0 + torch.exp(-t))


def conv_ref(x, wt, s, front, out):
    """The headers' sum, tap by tap: x NHWC [B, H, W, Cin], wt [kh, kw, Cin, Cout], stride s, `front` = the zero rows / columns in
    front of the image, `out` = (Ho, Wo); y[b, oy, ox] = sum over (dy, dx) of x[b, oy s - pt + dy, ox s - pl + dx] . wt[dy, dx]."""
    B, H, W, Cin = x.shape
    (kh, kw), (pt, pl), (Ho, Wo) = wt.shape[:2], front, out
    xp = x.new_zeros(B, max((Ho - 1) * s + kh, pt + H), max((Wo - 1) * s + kw, pl + W), Cin)
    xp[:, pt:pt + H, pl:pl + W] = x
    y = x.new_zeros(B, Ho, Wo, wt.shape[3])
    for dy in range(kh):
        for dx in range(kw):
            y = y + xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s] @ wt[dy, dx]
    return y


def stem_same_ref(x, w, b):
    """K12 before its SiLU: x NCHW, w [Cin, 3, 3, Cout] -> NHWC, TF-SAME padding, stride 2."""
    (Ho, pt, _), (Wo, pl, _) = same_pad(x.shape[2], 3, 2), same_pad(x.shape[3], 3, 2)
    return conv_ref(x.permute(0, 2, 3, 1), w.permute(1, 2, 0, 3), 2, (pt, pl), (Ho, Wo)) + b


def stem_sym_ref(x, w, b=None):
    """K16 / K19 before the ReLU: x NCHW, w [Cin, k, k, Cout] -> NHWC, pad k // 2 on every side, stride 2."""
    k = w.shape[1]
    y = conv_ref(x.permute(0, 2, 3, 1), w.permute(1, 2, 0, 3), 2, (k // 2, k // 2), (stem_out(x.shape[2]), stem_out(x.shape[3])))
    return y if b is None else y + b


def igemm_ref(x, w, b, k, s, relu_in, relu_out, res=None):
    """K18 / K18R: x NHWC, w [Cout, k*k*Cin] tap-major then channel."""
    Cin, Cout = x.shape[3], w.shape[0]
    y = conv_ref(relu_keep(x) if relu_in else x, w.view(Cout, k, k, Cin).permute(1, 2, 3, 0), s, (int(k == 3),) * 2,
                 (k18_out(x.shape[1], k, s), k18_out(x.shape[2], k, s))) + b
    y = y if res is None else y + res
    return relu_keep(y) if relu_out else y


def dw_ref(x, w, b, k, s, silu_in):
    """K13's y: x NHWC, w [k*k, C] tap-major, TF-SAME padding."""
    B, H, W, C = x.shape
    (Ho, pt, _), (Wo, pl, _) = same_pad(H, k, s), same_pad(W, k, s)
    xp = x.new_zeros(B, max((Ho - 1) * s + k, pt + H), max((Wo - 1) * s + k, pl + W), C)
    xp[:, pt:pt + H, pl:pl + W] = silu(x) if silu_in else x
    y = x.new_zeros(B, Ho, Wo, C)
    for dy in range(k):
        for dx in range(k):
            y = y + xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s] * w[dy * k + dx]
    return silu(y + b)


def tile_sums(y):
    """[B, Ho, Wo, C] -> [B, T, C]: the sums over the 8 x 8 output tiles, row-major (K13's psum)."""
    B, Ho, Wo, C = y.shape
    nty, ntx = -(-Ho // 8), -(-Wo // 8)
    p = y.new_zeros(B, nty * 8, ntx * 8, C)
    p[:, :Ho, :Wo] = y
    return p.view(B, nty, 8, ntx, 8, C).sum(dim=(2, 4)).reshape(B, nty * ntx, C)


def se_ref(psum, hw, wr, br, wet, be):
    mean = psum.sum(1) / hw
    return torch.sigmoid(silu(mean @ wr.t() + br) @ wet + be)


def maxpool_ref(x, sc, sh):
    """K17: x NHWC; the padding never wins."""
    return F.max_pool2d(relu_keep(x * sc + sh).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def gathered(x, H, W):
    """K32's rows before the LayerNorm: [B, H*W, C] -> [B, ceil(H/2) ceil(W/2), 4C], zeros past an odd edge (mcd_swin.h)."""
    B, _, C = x.shape
    g = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    g = torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], dim=-1)
    return g.reshape(B, -1, 4 * C).contiguous()


def region(r, n, w, s):
    return 0 if r < n - w else (1 if r < n - s else 2)


def reference64(qkv, pad, H, W, heads, w, s, table, dtype=torch.float64):
    """K31's rules (mcd_swin.h) on the CPU, in float64 unless told otherwise: zero padding of the token grid after the
    projection's input (a padded token's q, k, v are pad_qkv), roll by (-s, -s), windows in row-major order, the bias
    table[(i-i'+w-1)(2w-1) + (j-j'+w-1), head], -100 between tokens of different (row region, column region) pairs, softmax over
    the window's keys, times v, back to the original positions.  qkv [B, H*W, 3*heads*32] -> [B, H*W, heads*32]."""
    qkv, table = qkv.to(dtype).cpu(), table.to(dtype).cpu()
    B, T = qkv.shape[0], w * w
    Hp, Wp = -(-H // w) * w, -(-W // w) * w
    if (Hp, Wp) != (H, W):
        full = pad.to(dtype).cpu().view(1, 1, 1, 3, heads, 32).expand(B, Hp, Wp, 3, heads, 32).clone()
    else:
        full = torch.empty(B, Hp, Wp, 3, heads, 32, dtype=dtype)
    full[:, :H, :W] = qkv.view(B, H, W, 3, heads, 32)
    rolled = torch.roll(full, (-s, -s), (1, 2))
    ii, jj = torch.arange(T) // w, torch.arange(T) % w
    bias = table[(ii[:, None] - ii[None, :] + w - 1) * (2 * w - 1) + (jj[:, None] - jj[None, :] + w - 1)]       # [T, T, heads]
    out = torch.zeros(B, Hp, Wp, heads, 32, dtype=dtype)
    for wr in range(Hp // w):
        for wc in range(Wp // w):
            blk = rolled[:, wr * w:(wr + 1) * w, wc * w:(wc + 1) * w].reshape(B, T, 3, heads, 32)
            q, k, v = blk.permute(2, 0, 3, 1, 4)                                          # each [B, heads, T, 32]
            sc = q @ k.transpose(-1, -2) / math.sqrt(32.0) + bias.permute(2, 0, 1)[None]
            if s > 0:
                reg = torch.tensor([3 * region(wr * w + int(i), Hp, w, s) + region(wc * w + int(j), Wp, w, s) for i, j in zip(ii, jj)])
                sc = sc + (reg[:, None] != reg[None, :]).to(dtype) * -100.0
            o = torch.softmax(sc, dim=-1) @ v                                             # [B, heads, T, 32]
            out[:, wr * w:(wr + 1) * w, wc * w:(wc + 1) * w] = o.permute(0, 2, 1, 3).reshape(B, w, w, heads, 32)
    return torch.roll(out, (s, s), (1, 2))[:, :H, :W].reshape(B, H * W, heads * 32)


def window_map(H, W, w, s, n_rows=None, n_cols=None):
    """For the real tokens [H, W]: (the window each lies in on the rolled, padded grid, its region code 3 row + column -- 0
    throughout when s == 0).  n_rows / n_cols: the sizes the regions are taken from (the padded ones)."""
    Hp, Wp = -(-H // w) * w, -(-W // w) * w
    r = ((torch.arange(H) - s) % Hp)[:, None].expand(H, W)
    c = ((torch.arange(W) - s) % Wp)[None, :].expand(H, W)
    win = (r // w) * (Wp // w) + c // w
    if s == 0:
        return win, torch.zeros_like(win)
    nr, nc = n_rows or Hp, n_cols or Wp
    reg = 3 * ((r >= nr - w).long() + (r >= nr - s).long()) + (c >= nc - w).long() + (c >= nc - s).long()
    return win, reg


# =========================================================================================================================
# 3. the checker
# =========================================================================================================================
def _cat_outs(o):
    return o if isinstance(o, tuple) else (o,)


def _batch(ck, f, xs, out):
    """The relations every entry has: f(*xs) -> out with the batch in dimension 0 of every x and of every output; each image
    alone is its slice of the batch, and the batch reversed gives the outputs reversed."""
    outs = _cat_outs(out)
    B = xs[0].shape[0]
    if B < 2:
        return
    for b in range(B):
        for j, (got, want) in enumerate(zip(_cat_outs(f(*[x[b:b + 1].contiguous() for x in xs])), outs)):
            ck.same("image %d alone, output %d" % (b, j), got, want[b:b + 1])
    for j, (got, want) in enumerate(zip(_cat_outs(f(*[x.flip(0).contiguous() for x in xs])), outs)):
        ck.same("the batch reversed, output %d" % j, got, want.flip(0))


def _read_set(ck, what, got, ref_dirty, clean):
    """One NaN in an input: it reaches exactly the outputs the float64 reference makes NaN; the rest keep their bits."""
    got, clean = got.cpu(), clean.cpu()
    want = torch.isnan(ref_dirty).reshape(got.shape)
    if not torch.equal(torch.isnan(got), want):
        return ck.note("%s: %d outputs are NaN, the reference has %d (%d differ)" % (what, int(torch.isnan(got).sum()), int(want.sum()),
                                                                                   int((torch.isnan(got) != want).sum())))
    ck.same(what + ": the other outputs", got[~want], clean[~want])


def _nan_at(x, case, salt=5):
    """A copy of x with one NaN at a seeded place in its last image."""
    d = x.clone()
    g = _gen(case, salt)
    idx = (x.shape[0] - 1,) + tuple(int(torch.randint(0, n, (1,), generator=g)) for n in x.shape[1:])
    d[idx] = NAN
    return d


def _aten_rule(ck, what, out, ref, aten):
    """test_gpu_resnet._bound: nerr <= 2 nerr(ATen fp32 on the same device) + 1e-6."""
    ck.acc(what, nerr(out, ref), 2 * nerr(aten, ref) + 1e-6)


def _check_k12(ck, case, call, dev):
    B, Cin, H, W, Cout = (case[k] for k in ("B", "Cin", "H", "W", "Cout"))
    g = _gen(case)
    x, w = torch.randn(B, Cin, H, W, generator=g).to(dev), (torch.randn(Cin, 3, 3, Cout, generator=g) * 0.3).to(dev)
    b = (torch.randn(Cout, generator=g) * 0.1).to(dev)
    run = lambda xx: call("K12", x=xx, w=w, b=b)
    out = run(x)
    ck.acc("float64", nerr(out, silu(stem_same_ref(x.double().cpu(), w.double().cpu(), b.double().cpu()))), 2e-6)
    _batch(ck, run, (x,), out)
    if case["i"] % 4 == 0:
        d = _nan_at(x, case)
        _read_set(ck, "a NaN pixel", run(d), silu(stem_same_ref(d.double().cpu(), w.double().cpu(), b.double().cpu())), out)


def _check_k13(ck, case, call, dev):
    B, H, W, C, k, s, si = (case[n] for n in ("B", "H", "W", "C", "k", "s", "silu_in"))
    g = _gen(case)
    x, w = torch.randn(B, H, W, C, generator=g).to(dev), (torch.randn(k * k, C, generator=g) / k).to(dev)
    b = (torch.randn(C, generator=g) * 0.1).to(dev)
    run = lambda xx: call("K13", x=xx, w=w, b=b, k=k, s=s, silu_in=si)
    y, psum = run(x)
    ref = dw_ref(x.double().cpu(), w.double().cpu(), b.double().cpu(), k, s, si)
    if tuple(y.shape) != tuple(ref.shape) or tuple(psum.shape) != (B, tile_sums(ref).shape[1], C):
        return ck.note("shapes %s, %s" % (tuple(y.shape), tuple(psum.shape)))
    ck.acc("y against float64", nerr(y, ref), 2e-6)
    ck.acc("psum, tile by tile, against float64", nerr(psum, tile_sums(ref)), 2e-6)
    own, mass = tile_sums(y.double().cpu()), tile_sums(y.double().cpu().abs())       # no path has more than 64 + 256 additions
    ck.acc("psum against the kernel's own y", ((psum.double().cpu() - own).abs() / (320 * 2.0 ** -24 * mass).clamp_min(1e-300)).max(), 1.0)
    _batch(ck, run, (x,), (y, psum))


def _check_k14(ck, case, call, dev):
    B, T, C, sq, hw = (case[n] for n in ("B", "T", "C", "sq", "hw"))
    g = _gen(case)
    ops = [(torch.randn(B, T, C, generator=g) * (hw / T) ** 0.5), torch.randn(sq, C, generator=g) / C ** 0.5, torch.randn(sq, generator=g) * 0.1,
           torch.randn(sq, C, generator=g) / sq ** 0.5, torch.randn(C, generator=g) * 0.1]
    psum, wr, br, wet, be = (t.to(dev) for t in ops)
    run = lambda p: call("K14", psum=p, hw=hw, wr=wr, br=br, wet=wet, be=be)
    out = run(psum)
    ck.acc("float64", nerr(out, se_ref(*(t.double() for t in ops[:1]), hw, *(t.double() for t in ops[1:]))), 2e-6)
    _batch(ck, run, (psum,), out)


def _check_k15(ck, case, call, dev):
    B, HW, C = case["B"], case["HW"], case["C"]
    g = _gen(case)
    y, s = torch.randn(B, HW, C, generator=g).to(dev), torch.rand(B, C, generator=g).to(dev)
    run = lambda yy, ss: call("K15", y=yy, s=ss)
    out = run(y, s)
    ck.same("y * s[:, None, :]", out, y * s[:, None, :])
    _batch(ck, run, (y, s), out)


def _check_k0n(ck, case, call, dev):
    B, HW, C, mode = case["B"], case["HW"], case["C"], case["mode"]
    g = _gen(case)
    x = torch.randn(B, HW, C, generator=g) * (2.0 if mode == "silu_avg" else 3.0)
    if case["nan"]:
        x[0, HW // 2, C // 2] = NAN
        x[B - 1, 0, C - 1] = NAN
    x = x.to(dev)
    run = lambda xx: call("K0N", x=xx, mode=mode, place=case["place"])
    out = run(x)
    if mode == "silu_avg":
        ck.acc("float64", nerr(out, silu(x.double().cpu()).mean(dim=1)), 2e-6)
    else:
        k0 = call("K0", x=x.transpose(1, 2).contiguous(), mode=mode)
        if not torch.equal(torch.isnan(out), torch.isnan(k0)):
            ck.note("K0N's NaNs are not K0's")
        ck.same("K0 on the NCHW copy", torch.nan_to_num(out), torch.nan_to_num(k0))
        if case["nan"] and int(torch.isnan(out).sum()) != (2 if (B > 1 or C // 2 != C - 1) else 1):
            ck.note("a NaN in a plane must make its max NaN: %d NaNs" % int(torch.isnan(out).sum()))
    if not case["nan"]:
        _batch(ck, run, (x,), out)


def _stem_operands(case, k, dev):
    B, Cin, H, W, Cout = (case[n] for n in ("B", "Cin", "H", "W", "Cout"))
    g = _gen(case)
    if case["regime"] == "exact":                  # dyadic data: every product and partial sum is exact in fp32 in any order
        x = torch.randint(-8, 9, (B, Cin, H, W), generator=g).float() / 4
        w = torch.randint(-8, 9, (Cin, k, k, Cout), generator=g).float() / 8
        b = torch.randint(-8, 9, (Cout,), generator=g).float() / 2
    else:
        x, w = torch.randn(B, Cin, H, W, generator=g), torch.randn(Cin, k, k, Cout, generator=g) / (k * k * Cin) ** 0.5
        b = torch.randn(Cout, generator=g)
    return x.to(dev), w.to(dev), b.to(dev), torch.randperm(Cout, generator=g).to(dev)


def _check_stem(ck, case, call, dev):
    entry = case["entry"]
    k = 7 if entry == "K16" else 3
    x, w, b, perm = _stem_operands(case, k, dev)
    relu = case.get("relu", 0)
    if entry == "K16":
        run = lambda xx, ww=w, bb=b, r=0: call("K16", x=xx, w=ww)
    else:
        run = lambda xx, ww=w, bb=b, r=relu: call("K19", x=xx, w=ww, b=bb, relu=r)
    act = relu_keep if relu else (lambda t: t)
    ref_of = lambda xx: act(stem_sym_ref(xx.double().cpu(), w.double().cpu(), None if entry == "K16" else b.double().cpu()))
    out, ref = run(x), ref_of(x)
    if case["regime"] == "exact":
        ck.same("float64 on exact data", out.cpu().double(), ref)
    aten = F.conv2d(x, w.permute(3, 0, 1, 2), None if entry == "K16" else b, 2, k // 2).permute(0, 2, 3, 1)
    _aten_rule(ck, "float64", out, ref, act(aten))
    ck.same("w's output channels permuted", run(x, w[..., perm].contiguous(), b[perm].contiguous()), out[..., perm])
    if relu:
        ck.same("relu of relu = 0", out, relu_keep(run(x, w, b, 0)))
    _batch(ck, run, (x,), out)
    if case["i"] % 4 == 0:
        d = _nan_at(x, case)
        _read_set(ck, "a NaN pixel", run(d), ref_of(d), out)


def _k18_operands(case, dev):
    B, H, W, Cin, Cout, k, s, r = (case[n] for n in ("B", "H", "W", "Cin", "Cout", "k", "s", "regime"))
    g = _gen(case)
    K = k * k * Cin
    oshape = (B, k18_out(H, k, s), k18_out(W, k, s), Cout)
    if r == "exact":                               # test_k18_exact_on_exact_data's: sums of multiples of 1/32 below 2^24 / 32
        x = torch.randint(-8, 9, (B, H, W, Cin), generator=g).float() / 4
        w = torch.randint(-8, 9, (Cout, K), generator=g).float() / 8
        b = torch.randint(-8, 9, (Cout,), generator=g).float() / 2
        res = torch.randint(-8, 9, oshape, generator=g).float() / 2
    else:
        x, w, b = torch.randn(B, H, W, Cin, generator=g), torch.randn(Cout, K, generator=g) / K ** 0.5, torch.randn(Cout, generator=g)
        res = torch.randn(oshape, generator=g) * 1.5
        if r == "offset":
            x = x + 3.0
        elif r == "dead":
            x = -x.abs() - 0.01
        elif r == "negres":
            res = -3.0 * res.abs() / 1.5
    return x.to(dev), w.to(dev), b.to(dev), res.to(dev), torch.randperm(Cout, generator=g).to(dev)


# (entry, regime) pairs held to the derivable per-element bound instead of the ATen rule, with the measurement that put them
# here (none so far: every regime passes the rule it was given)
DERIVED = {}


def _check_k18(ck, case, call, dev):
    entry, k, s, ri, ro, r = (case[n] for n in ("entry", "k", "s", "relu_in", "relu_out", "regime"))
    x, w, b, res, perm = _k18_operands(case, dev)
    with_res = entry == "K18R"

    def run(xx, rr=res, ww=w, bb=b, i=ri, o=ro, name=entry):
        kw = dict(x=xx, w=ww, b=bb, k=k, s=s, relu_in=i, relu_out=o)
        if name == "K18R":
            kw["res"] = rr
        return call(name, **kw)

    out = run(x)
    c64 = lambda t: t.double().cpu()
    ref = igemm_ref(c64(x), c64(w), c64(b), k, s, ri, ro, c64(res) if with_res else None)
    if tuple(out.shape) != tuple(ref.shape):
        return ck.note("shape %s" % (tuple(out.shape),))
    Cin, Cout = x.shape[3], w.shape[0]
    act_in, act_out = (relu_keep if ri else (lambda t: t)), (relu_keep if ro else (lambda t: t))
    aten = F.conv2d(act_in(x).permute(0, 3, 1, 2), w.view(Cout, k, k, Cin).permute(0, 3, 1, 2), b, s, int(k == 3)).permute(0, 2, 3, 1)
    aten = act_out(aten + res if with_res else aten)
    if (entry, r) in DERIVED:                      # (chain length + chunks + 2) 2^-24 (sum |w| |x| + |bias| + |res|), per element
        K = k * k * Cin
        mass = igemm_ref(c64(act_in(x)).abs(), c64(w).abs(), c64(b).abs(), k, s, 0, 0, c64(res).abs() if with_res else None)
        ck.acc("float64, per element", ((out.double().cpu() - ref).abs() / ((min(K, 256) + -(-K // 256) + 2) * 2.0 ** -24 * mass)).max(), 1.0)
    else:
        _aten_rule(ck, "float64", out, ref, aten)
    if r == "exact":
        ck.same("float64 on exact data", out.cpu().double(), ref)
    if r == "dead":                                # every act_in(x) is +0: the sum is +0 and the output the bias (+ res), bit for bit
        ck.same("the bias alone", out, act_out((b + res) if with_res else b.expand_as(out)))
    ck.same("w's output channels permuted", run(x, res[..., perm].contiguous(), w[perm].contiguous(), b[perm].contiguous()), out[..., perm])
    base = run(x, o=0, name="K18")
    if ro and not with_res:
        ck.same("relu of relu_out = 0", out, relu_keep(base))
    if ri:
        ck.same("relu_in = 0 on relu(x)", run(relu_keep(x), i=0), out)
    if with_res:
        ck.same("res = NULL is K18", run(x, None), run(x, name="K18"))
        ck.same("(total + bias) + res in fp32", out, act_out(base + res))
    _batch(ck, (lambda xx, rr: run(xx, rr)), (x, res), out)


def _check_k17(ck, case, call, dev):
    B, H, W, C, r = (case[n] for n in ("B", "H", "W", "C", "regime"))
    g = _gen(case)
    x = torch.randn(B, H, W, C, generator=g)
    if r == "unit":
        sc, sh = torch.ones(C), torch.zeros(C)
    elif r == "rand":
        sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    else:                                          # every pixel of the top-left windows is far below zero: their maximum is 0
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        x[:, :4, :4] = -50.0
    x, sc, sh = x.to(dev), sc.to(dev), sh.to(dev)
    run = lambda xx: call("K17", x=xx, scale=sc, shift=sh)
    out = run(x)
    if r == "unit":
        ck.same("max_pool2d(relu(x), 3, 2, 1)", out, F.max_pool2d(F.relu(x.permute(0, 3, 1, 2)), 3, 2, 1).permute(0, 2, 3, 1))
    if case.get("big"):
        return
    ref_of = lambda xx: maxpool_ref(xx.double().cpu(), sc.double().cpu(), sh.double().cpu())
    ref = ref_of(x)
    _aten_rule(ck, "float64", out, ref, maxpool_ref(x, sc, sh))
    if r == "negwin" and float(out[:, 0, 0].abs().max()) != 0.0:
        ck.note("a window of negative values must give 0")
    _batch(ck, run, (x,), out)
    if case["i"] % 4 == 0:
        d = _nan_at(x, case)
        _read_set(ck, "a NaN pixel", run(d), ref_of(d), out)


def _check_k20(ck, case, call, dev):
    B, H, W, C = (case[n] for n in ("B", "H", "W", "C"))
    x = (torch.randn(B, H, W, C, generator=_gen(case)) * 3.0).to(dev)
    run = lambda xx: call("K20", x=xx)
    out = run(x)
    if min(H, W) == 1:                             # MCD_OK, nothing written (the frame says so)
        if tuple(out.shape) != (B, H // 2, W // 2, C):
            ck.note("shape %s" % (tuple(out.shape),))
        return
    ck.same("F.avg_pool2d(x, 2)", out, F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    if case.get("big"):
        return
    _batch(ck, run, (x,), out)
    if case["i"] % 4 == 0:
        d = _nan_at(x, case)
        _read_set(ck, "a NaN pixel", run(d), F.avg_pool2d(d.double().cpu().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), out)


def _check_k21(ck, case, call, dev):
    B, HW, C = case["B"], case["HW"], case["C"]
    g = _gen(case)
    x, pos = (torch.randn(B, HW, C, generator=g) + 0.5).to(dev), (torch.randn(HW + 1, C, generator=g) / C ** 0.5).to(dev)
    run = lambda xx: call("K21", x=xx, pos=pos)
    out = run(x)
    if tuple(out.shape) != (B, HW + 1, C):
        return ck.note("shape %s" % (tuple(out.shape),))
    ck.same("rows 1..: x + pos[1:]", out[:, 1:], x + pos[1:])
    r0 = x.double().cpu().mean(dim=1) + pos[0].double().cpu()
    _aten_rule(ck, "row 0 against float64", out[:, 0], r0, x.mean(dim=1) + pos[0])
    _batch(ck, run, (x,), out)


def k31_operands(case):
    """(qkv [B, H*W, 3*heads*32], pad_qkv, table, the rows that must equal one value row: a list of (b, row mask, j)) of the
    case's regime, on the CPU.  `dominant`: in every image one token j; the tokens of j's window that see key j without the
    mask get q = 50 k_j, so that key j leads their scores by ~ 280 against a spread of ~ 50 and the -100 of the mask: their
    rows are v_j.  The other tokens keep N(0, 1) queries (encoder_fuzz.attention_operands says why)."""
    B, H, W, heads, w, s, r = (case[n] for n in ("B", "H", "W", "heads", "w", "s", "regime"))
    g = _gen(case)
    qkv = torch.randn(B, H * W, 3, heads, 32, generator=g)
    pad = torch.randn(3, heads, 32, generator=g) + (0.0 if r == "dominant" else 3.0)        # unlike every real row (mean 3)
    table = torch.randn((2 * w - 1) ** 2, heads, generator=g)
    dom = []
    if r == "r6":
        qkv *= 6.0
    elif r == "table20":
        table *= 20.0
    elif r == "dominant":
        win, reg = (t.reshape(-1) for t in window_map(H, W, w, s))
        for b in range(B):
            j = int(torch.randint(0, H * W, (1,), generator=g))
            rows = (win == win[j]) & (reg == reg[j])
            qkv[b, rows, 0] = 50.0 * qkv[b, j, 1]
            dom.append((b, rows, j))
    return qkv.reshape(B, H * W, 3 * heads * 32), pad.reshape(-1), table, dom


def _check_k31(ck, case, call, dev):
    B, H, W, heads, w, s = (case[n] for n in ("B", "H", "W", "heads", "w", "s"))
    qkv, pad, table, dom = k31_operands(case)
    D = heads * 32
    qkv, table = qkv.to(dev), table.to(dev)
    pad = None if case["pad_null"] else pad.to(dev)
    run = lambda q, hh=H, ww=W, ss=s, pp=pad: call("K31", qkv=q, pad=pp, H=hh, W=ww, heads=heads, w=w, s=ss, table=table)
    out = run(qkv)
    ref = reference64(qkv, pad, H, W, heads, w, s, table)
    ref32 = reference64(qkv, pad, H, W, heads, w, s, table, torch.float32)
    o = out.cpu()
    plain = torch.ones(B, H * W, dtype=torch.bool)
    v = qkv.cpu().view(B, H * W, 3, D)[:, :, 2]
    for b, rows, j in dom:
        want = v[b, j].double()
        if float((ref[b, rows] - want).abs().max()) > 1e-9 * max(1.0, float(want.abs().max())):
            ck.note("generator: key %d of image %d does not dominate" % (j, b))
        ck.acc("dominant key %d of image %d" % (j, b), (o[b, rows].double() - want).abs().max(), 3e-6 * float(v.abs().max()))
        plain[b, rows] = False
    if bool(plain.any()):
        _general(ck, "float64", o[plain], ref[plain], ref32[plain])
    _batch(ck, run, (qkv,), out)
    if s == 0 and (H > w or W > w):                # a window does not know where it is: each one alone, as a one-window call
        grid, og = qkv.view(B, H, W, 3 * D), out.view(B, H, W, D)
        for y0 in range(0, H, w):
            for x0 in range(0, W, w):
                hr, wc = min(w, H - y0), min(w, W - x0)
                alone = run(grid[:, y0:y0 + hr, x0:x0 + wc].reshape(B, hr * wc, 3 * D).contiguous(), hr, wc, 0,
                            None if (hr, wc) == (w, w) and case["i"] % 2 else pad)
                ck.same("the window at (%d, %d) alone" % (y0, x0), alone, og[:, y0:y0 + hr, x0:x0 + wc].reshape(B, hr * wc, D))
    if case["i"] % 4 == 0:
        g = _gen(case, 5)
        d = qkv.clone()
        t, h, e = (int(torch.randint(0, n, (1,), generator=g)) for n in (H * W, heads, 32))
        d.view(B, H * W, 3, heads, 32)[B - 1, t, 1, h, e] = NAN
        _read_set(ck, "a NaN in a key", run(d), reference64(d, pad, H, W, heads, w, s, table), out)


def _check_k32(ck, case, call, dev):
    B, H, W, C = (case[n] for n in ("B", "H", "W", "C"))
    g = _gen(case)
    x = (torch.randn(B, H * W, C, generator=g) * 2.0 + 0.5).to(dev)
    gam, bet = (torch.randn(4 * C, generator=g) * 0.2 + 1.0).to(dev), (torch.randn(4 * C, generator=g) * 0.1).to(dev)
    run = lambda xx: call("K32", x=xx, H=H, W=W, g=gam, b=bet, eps=1e-5)
    out = run(x)
    rows = gathered(x, H, W)
    if tuple(out.shape) != tuple(rows.shape):
        return ck.note("shape %s" % (tuple(out.shape),))
    ck.same("K10 on the gathered rows", out, call("K10", x=rows.view(-1, 4 * C), g=gam, b=bet, eps=1e-5).view(rows.shape))
    ck.acc("float64", nerr(out, F.layer_norm(rows.double().cpu(), (4 * C,), gam.double().cpu(), bet.double().cpu(), 1e-5)), 2e-6)
    _batch(ck, run, (x,), out)


_CHECKS = {"K12": _check_k12, "K13": _check_k13, "K14": _check_k14, "K15": _check_k15, "K0N": _check_k0n, "K16": _check_stem, "K17": _check_k17,
           "K18": _check_k18, "K18R": _check_k18, "K19": _check_stem, "K20": _check_k20, "K21": _check_k21, "K31": _check_k31, "K32": _check_k32}


def check(entry, case, call, device="cpu"):
    """(findings, the largest err / bound of the case's accuracy checks -- 0.0 for an entry that is held to bits alone)."""
    ck = _Ck(entry, case)
    try:
        _CHECKS[entry](ck, case, call, device)
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
def gpu_call(L):
    """call(name, ...) on libmcd_hip.so: inputs through In of test_gpu_encoder_frames with NaN in their guards, outputs in
    OUT_FILL frames (K0N's destination a util.FramedOut matrix at a pitch, of which only its block may change; K15's y in
    place, as K25 in encoder_fuzz).  The guards must come back intact, every logical element written, the inputs unchanged
    (AssertionError otherwise: check() reports it)."""
    import test_gpu_encoder_frames as EF
    import util

    encoder = E.gpu_call(L)
    modes = {"avg": 0, "max": 1, "silu_avg": 4}     # MCD_POOL_AVG, MCD_POOL_MAX, MCD_POOL_SILU_AVG

    def call(name, **a):
        st = EF.st()
        I = lambda t: None if t is None else EF.In(t, NAN)      # noqa: E731, E741
        if name in ("K12", "K16", "K19"):
            x, w = a["x"], a["w"]
            (B, Cin, H, W), Cout = x.shape, w.shape[3]
            x_, w_, b_ = I(x), I(w), I(a.get("b"))
            if name == "K12":
                o_ = EF.Out((B, (H + 1) // 2, (W + 1) // 2, Cout), x.device)
                EF.ok(L.mcd_conv_stem_nhwc(x_.ptr, B, Cin, H, W, w_.ptr, b_.ptr, Cout, o_.ptr, st), L)
            else:
                o_ = EF.Out((B, stem_out(H), stem_out(W), Cout), x.device)
                if name == "K16":
                    EF.ok(L.mcd_conv7x7s2_nhwc(x_.ptr, B, Cin, H, W, w_.ptr, Cout, o_.ptr, st), L)
                else:
                    EF.ok(L.mcd_conv3x3s2_nhwc(x_.ptr, B, Cin, H, W, w_.ptr, b_.ptr, Cout, int(a["relu"]), o_.ptr, st), L)
            return _finish(name, o_, (x_, w_, b_))
        if name == "K13":
            x, k, s = a["x"], a["k"], a["s"]
            B, H, W, C = x.shape
            Ho, Wo = same_pad(H, k, s)[0], same_pad(W, k, s)[0]
            T = -(-Ho // 8) * -(-Wo // 8)
            x_, w_, b_ = I(x), I(a["w"]), I(a["b"])
            y_, p_ = EF.Out((B, Ho, Wo, C), x.device), EF.Out((B, T, C), x.device)
            EF.ok(L.mcd_dwconv_bn_silu(x_.ptr, B, H, W, C, w_.ptr, b_.ptr, k, s, int(a["silu_in"]), y_.ptr, p_.ptr, T, st), L)
            return _finish(name, y_, (x_, w_, b_)), _finish(name + " psum", p_, ())
        if name == "K14":
            psum = a["psum"]
            B, T, C = psum.shape
            ins = [I(a[n]) for n in ("psum", "wr", "br", "wet", "be")]
            o_ = EF.Out((B, C), psum.device)
            EF.ok(L.mcd_se_gate(ins[0].ptr, B, T, C, a["hw"], ins[1].ptr, ins[2].ptr, a["wr"].shape[0], ins[3].ptr, ins[4].ptr, o_.ptr, st), L)
            return _finish(name, o_, ins)
        if name == "K15":
            y = a["y"]
            B, HW, C = y.shape
            y_, s_ = EF.In(y, util.OUT_FILL), I(a["s"])
            EF.ok(L.mcd_channel_scale(y_.ptr, B, HW, C, s_.ptr, st), L)
            y_.check = lambda e, what="": util.check_frame(y_.flat, y_.spec, e, what=str(what))
            return _finish(name, y_, (s_,))
        if name == "K0":
            x = a["x"]
            B, C, HW = x.shape
            x_, o_ = I(x), EF.Out((B, C), x.device)
            EF.ok(L.mcd_hook_pool(x_.ptr, B, C, HW, modes[a["mode"]], o_.ptr, 0, 0, C, 1, st), L)
            return _finish(name, o_, (x_,))
        if name == "K0N":
            x = a["x"]
            B, HW, C = x.shape
            row0, col0, neuron_major = a["place"]
            rows, width = (col0 + C, row0 + B) if neuron_major else (row0 + B, col0 + C)
            pitch = width + 4
            d_ = util.FramedOut(rows, width, pitch, 0, torch.float32, x.device)
            x_ = I(x)
            sn, su = (1, pitch) if neuron_major else (pitch, 1)
            EF.ok(L.mcd_hook_pool_nhwc(x_.ptr, B, C, HW, modes[a["mode"]], d_.ptr, row0, col0, sn, su, st), L)
            full = d_.view.clone()
            block = (full[col0:, row0:].t() if neuron_major else full[row0:, col0:]).contiguous()
            want = torch.full_like(full, util.OUT_FILL)                      # the block alone may change
            (want[col0:, row0:] if neuron_major else want[row0:, col0:]).copy_(block.t() if neuron_major else block)
            d_.check(want, what=name)
            assert not bool((block == util.OUT_FILL).any()), "K0N: an output element was not written"
            x_.same()
            return block
        if name == "K17":
            x = a["x"]
            B, H, W, C = x.shape
            ins = [I(x), I(a["scale"]), I(a["shift"])]
            o_ = EF.Out((B, stem_out(H), stem_out(W), C), x.device)
            EF.ok(L.mcd_bn_relu_maxpool_nhwc(ins[0].ptr, B, H, W, C, ins[1].ptr, ins[2].ptr, o_.ptr, st), L)
            return _finish(name, o_, ins)
        if name in ("K18", "K18R"):
            x, w, k, s = a["x"], a["w"], a["k"], a["s"]
            (B, H, W, Cin), Cout = x.shape, w.shape[0]
            ins = [I(x), I(w), I(a["b"]), I(a.get("res"))]
            o_ = EF.Out((B, k18_out(H, k, s), k18_out(W, k, s), Cout), x.device)
            if name == "K18":
                EF.ok(L.mcd_conv_igemm_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, Cout, k, s, int(a["relu_in"]), int(a["relu_out"]),
                                            o_.ptr, st), L)
            else:
                EF.ok(L.mcd_conv_igemm_res_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, _ptr(ins[3]), Cout, k, s, int(a["relu_in"]),
                                                int(a["relu_out"]), o_.ptr, st), L)
            return _finish(name, o_, ins)
        if name == "K20":
            x = a["x"]
            B, H, W, C = x.shape
            x_, o_ = I(x), EF.Out((B, H // 2, W // 2, C), x.device)
            EF.ok(L.mcd_avgpool2_nhwc(x_.ptr, B, H, W, C, o_.ptr, st), L)
            return _finish(name, o_, (x_,))
        if name == "K21":
            x = a["x"]
            B, HW, C = x.shape
            x_, p_, o_ = I(x), I(a["pos"]), EF.Out((B, HW + 1, C), x.device)
            EF.ok(L.mcd_attnpool_tokens(x_.ptr, B, HW, C, p_.ptr, o_.ptr, st), L)
            return _finish(name, o_, (x_, p_))
        if name == "K31":
            qkv, heads = a["qkv"], a["heads"]
            B = qkv.shape[0]
            q_, p_, t_ = I(qkv), I(a["pad"]), I(a["table"])
            o_ = EF.Out((B, a["H"] * a["W"], heads * 32), qkv.device)
            EF.ok(L.mcd_window_attention(q_.ptr, _ptr(p_), B, a["H"], a["W"], heads, a["w"], a["s"], t_.ptr, o_.ptr, st), L)
            return _finish(name, o_, (q_, p_, t_))
        if name == "K32":
            x, H, W = a["x"], a["H"], a["W"]
            B, _, C = x.shape
            ins = [I(x), I(a["g"]), I(a["b"])]
            o_ = EF.Out((B, ((H + 1) // 2) * ((W + 1) // 2), 4 * C), x.device)
            EF.ok(L.mcd_patch_merge_ln(ins[0].ptr, B, H, W, C, ins[1].ptr, ins[2].ptr, a["eps"], o_.ptr, st), L)
            return _finish(name, o_, ins)
        return encoder(name, **a)

    return call
