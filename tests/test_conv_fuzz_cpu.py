"""CPU: the convolution-side fuzzer (tests/conv_fuzz.py) held to account without a GPU, in the three parts of
test_encoder_fuzz_cpu.py.

1. Its references: reference64 (K31) against data_utils._window_attend_aten in float64; the tap-by-tap convolution references
   against an independent F.pad + F.conv2d formulation; K13's tile sums against F.avg_pool2d(..., 8, ceil_mode=True) x counts.
2. Coverage: at the committed seeds every stratum of the plan is in the generated lists, the lists are deterministic and stay
   inside the plan's sizes.
3. Mutants: fp32 torch emulations of the entries in which the headers' bit relations hold by construction (an output element's
   arithmetic depends on its own operands alone: explicit k-ordered sums for K16 / K18 / K19, one image or one window at a time
   wherever a library reduction is used).  The checker finds nothing on them over the whole committed lists, with err / bound
   <= 1, and finds every mutant of MUTANTS."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_fuzz as C
import test_encoder_fuzz_cpu as TE

NAN = float("nan")


def case_list(entry):
    return C.cases(entry, C.SEEDS[entry])


# =========================================================================================================================
# 1. the references
# =========================================================================================================================
@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


# (B, heads, H, W, w, s): padded and shifted; one window; shifted; padded both ways; all 64 tokens; no shift, padded; 1 x 1
@pytest.mark.parametrize("shape", [(2, 3, 10, 9, 7, 3), (1, 2, 7, 7, 7, 0), (3, 1, 4, 6, 2, 1), (2, 2, 5, 5, 3, 1), (1, 2, 16, 24, 8, 4),
                                   (2, 1, 5, 7, 3, 0), (1, 1, 1, 1, 1, 0), (2, 2, 3, 3, 3, 2)])
def test_reference64_against_the_aten_route_in_float64(du, shape):
    B, heads, H, W, w, s = shape
    g = torch.Generator().manual_seed(H * W + w)
    qkv = torch.randn(B, H * W, 3 * heads * 32, generator=g).double()
    pad = (torch.randn(3 * heads * 32, generator=g) + 3.0).double()
    table = torch.randn((2 * w - 1) ** 2, heads, generator=g).double()
    want = du._window_attend_aten(qkv, heads, (H, W), w, s, table, pad)
    assert float((C.reference64(qkv, pad, H, W, heads, w, s, table) - want).abs().max()) <= 1e-12
    win, reg = C.window_map(H, W, w, s)                      # the map the dominant regime is drawn with: the reference's regions
    Hp, Wp = -(-H // w) * w, -(-W // w) * w
    for y in range(H):
        for x in range(W):
            r, c = (y - s) % Hp, (x - s) % Wp
            assert int(win[y, x]) == (r // w) * (Wp // w) + c // w
            assert int(reg[y, x]) == (3 * C.region(r, Hp, w, s) + C.region(c, Wp, w, s) if s else 0)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (7, 6), (8, 9)])
def test_the_padding_references_against_pad_and_conv2d(H, W):
    g = torch.Generator().manual_seed(H + W)
    B, Cin, Cout = 2, 3, 8
    x = torch.randn(B, Cin, H, W, generator=g).double()
    b = torch.randn(Cout, generator=g).double()
    for k in (3, 7):                                         # K16 / K19: symmetric, pad k // 2
        w = torch.randn(Cout, Cin, k, k, generator=g).double()
        want = F.conv2d(F.pad(x, (k // 2,) * 4), w, b, 2).permute(0, 2, 3, 1)
        assert float((C.stem_sym_ref(x, w.permute(1, 2, 3, 0), b) - want).abs().max()) <= 1e-12
    w = torch.randn(Cout, Cin, 3, 3, generator=g).double()   # K12: TF-SAME, the smaller half on top and left
    (Ho, pt, pb), (Wo, pl, pr) = C.same_pad(H, 3, 2), C.same_pad(W, 3, 2)
    assert (Ho, Wo) == (-(-H // 2), -(-W // 2)) and pt <= pb <= pt + 1 and pl <= pr <= pl + 1
    want = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b, 2).permute(0, 2, 3, 1)
    assert float((C.stem_same_ref(x, w.permute(1, 2, 3, 0), b) - want).abs().max()) <= 1e-12
    xn = torch.randn(B, H, W, 32, generator=g).double()      # K18 / K18R
    for k, s in C.K18_KS:
        w = torch.randn(64, 32, k, k, generator=g).double() / 8
        bb, res = torch.randn(64, generator=g).double(), None
        for ri, ro, with_res in ((0, 0, False), (1, 1, True), (0, 1, True)):
            a = F.relu(xn) if ri else xn
            want = F.conv2d(F.pad(a.permute(0, 3, 1, 2), (int(k == 3),) * 4), w, bb, s).permute(0, 2, 3, 1)
            if with_res:
                res = -2.0 * torch.randn(want.shape, generator=g).double().abs()
                want = want + res
            want = F.relu(want) if ro else want
            got = C.igemm_ref(xn, w.permute(0, 2, 3, 1).reshape(64, -1), bb, k, s, ri, ro, res if with_res else None)
            assert float((got - want).abs().max()) <= 1e-12
    for k, s in C.K13_KS:                                    # K13: depthwise, TF-SAME
        w = torch.randn(32, 1, k, k, generator=g).double()
        bb = torch.randn(32, generator=g).double()
        (_, pt, pb), (_, pl, pr) = C.same_pad(H, k, s), C.same_pad(W, k, s)
        for si in (0, 1):
            a = (F.silu(xn) if si else xn).permute(0, 3, 1, 2)
            want = F.silu(F.conv2d(F.pad(a, (pl, pr, pt, pb)), w, bb, s, 0, 1, 32)).permute(0, 2, 3, 1)
            got = C.dw_ref(xn, w.reshape(32, k * k).t(), bb, k, s, si)
            assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("Ho,Wo", [(1, 1), (8, 8), (9, 7), (17, 15), (16, 24)])
def test_the_tile_sums_against_avg_pool2d(Ho, Wo):
    y = torch.randn(2, Ho, Wo, 12, generator=torch.Generator().manual_seed(Ho)).double()
    pool = lambda t: F.avg_pool2d(t.permute(0, 3, 1, 2), 8, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    ones = torch.ones(1, Ho, Wo, 1, dtype=torch.float64)
    counts = F.avg_pool2d(ones.permute(0, 3, 1, 2), 8, ceil_mode=True, count_include_pad=True, divisor_override=1).permute(0, 2, 3, 1)
    want = (pool(y) * counts).reshape(2, -1, 12)
    assert float((C.tile_sums(y) - want).abs().max()) <= 1e-12
    assert float(counts.sum()) == Ho * Wo


def test_the_gather_of_k32_is_the_headers():
    x = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).view(2, 15, 4)
    g = C.gathered(x, 3, 5).view(2, 2, 3, 16)
    v = x.view(2, 3, 5, 4)
    assert torch.equal(g[:, 0, 1], torch.cat([v[:, 0, 2], v[:, 1, 2], v[:, 0, 3], v[:, 1, 3]], -1))
    assert torch.equal(g[:, 1, 2], torch.cat([v[:, 2, 4], torch.zeros(2, 12)], -1))          # past both odd edges: zeros


# =========================================================================================================================
# 2. coverage
# =========================================================================================================================
def _need(entry):
    par = {("parity", a, b) for a in (0, 1) for b in (0, 1)}
    if entry == "K12":
        return {("cin", c) for c in (1, 2, 3, 4)} | {("cout", 4), ("cout", 48), ("side", 1), ("side", 2), ("overcap",)} | par
    if entry == "K13":
        need = {("inst", k, s, n) for k, s in ((3, 1), (3, 2), (5, 1), (5, 2)) for n in ("1", "3", "qmax", "qmax+1", "2qmax+1")}
        need |= {("mod", a, m) for a in "yx" for m in (0, 1, 7)} | {("T", t) for t in (1, 2, 4, 6)}
        return need | {("below_k",), ("s2", "odd"), ("s2", "even"), ("silu", 0), ("silu", 1), ("idle",)}
    if entry == "K14":
        need = {("T", t) for t in (1, 15, 16, 17, 33)} | {("C", c) for c in (4, 60, 64, 68, 260, 1028)}
        return need | {("sq", q) for q in (1, 3, 4, 5, 9)} | {("limit",)}
    if entry == "K15":
        return {("nq", n) for n in (1, 3, 60, 64)} | {("mod", m) for m in (0, 1, 1023)} | {("overcap", False), ("overcap", True)}
    if entry == "K0N":
        need = {("HW", v) for v in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260)} | {("C%64", m) for m in (0, 1, 63)}
        need |= {("mode", m) for m in ("avg", "max", "silu_avg")}
        return need | {(n, f) for n in ("row0", "col0", "neuron_major") for f in (False, True)}
    if entry in ("K16", "K19"):
        need = {("cout", c) for c in (4, 8, 36, 32, 64)} | {("cin", c) for c in (1, 2, 3, 4)}
        need |= {("mod", a, m) for a in "yx" for m in (0, 1, 15)} | {("tiles", a, t) for a in "yx" for t in (1, 2, 3)}
        need |= {("side", 1), ("side", 2), ("parity", "odd"), ("parity", "even"), ("regime", "exact"), ("regime", "randn")}
        return need | ({("relu", 0), ("relu", 1)} if entry == "K19" else set())
    if entry == "K17":
        need = {(a, v) for a in "HW" for v in (1, 2, 3, "odd", "even")} | {("nq", n) for n in (1, 5, 16)}
        return need | {("regime", r) for r in ("unit", "rand", "negwin")} | {("overcap",)}
    if entry in ("K18", "K18R"):
        need = {("inst", k, s, co) for k, s in ((3, 1), (3, 2), (1, 2)) for co in (32, 64, 96, 128, 160, 256)}
        need |= {("fill", f) for f in (0, 1, 63, 64, 65, 127)} | {("tiles", t) for t in (1, 2, 3)}
        need |= {("fill",) + key for ks in C.K18_KS for key in C.k18_shapes(*ks)}          # every (tiles, fill) pair small shapes reach
        need |= {("span",), ("span16",)} | {("ksteps", n) for n in (1, 8, 9, 18, 36)} | {("side", v) for v in (1, 2, 3)}
        need |= {("s2", "odd"), ("s2", "even")} | {("relu", i, o) for i in (0, 1) for o in (0, 1)}
        return need | {("regime", r) for r in ("exact", "randn", "offset", "dead") + (("negres",) if entry == "K18R" else ())}
    if entry == "K20":
        return par | {("empty",), ("overcap",)}
    if entry == "K21":
        return {("HW", v) for v in (1, 2, 3, 4, 5, 49, 50)} | {("C", c) for c in (4, 252, 256, 260, 2048)}
    if entry == "K31":
        need = {("ws", w, s) for w in range(1, 9) for s in range(w)}
        assert len(need) == 36
        need |= {("axis", a) for a in ("exact", "pad1", "padw1", "one", "three")} | {("pad_null",)}
        need |= {("heads", h) for h in (1, 2, 3, 5)} | {("B", b) for b in (1, 2, 3)}
        return need | {("regime", r) for r in ("r1", "r6", "table20", "dominant")}
    if entry == "K32":
        return par | {("C", c) for c in (4, 8, 96, 260, 512)} | {("1x1",), ("1xn",)}
    raise KeyError(entry)


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_every_stratum_is_in_the_committed_list(entry):
    cl = case_list(entry)
    missing = _need(entry) - C.strata(entry, cl)
    assert not missing, (entry, sorted(missing, key=str))
    assert cl == case_list(entry), "the list is not deterministic"
    big = [c for c in cl if c.get("big")]
    for c in cl:                                             # what the plan bounds
        assert 1 <= c["B"] <= 4
        if not c.get("big"):
            assert max(c.get("H", 1), c.get("W", 1)) <= 40 and c.get("HW", 1) <= 1600, c
    # the named cases past the bounds: one past every grid cap (K15: one whose stride is a multiple of nq and one whose is not), and
    # the stems' second and third 16-pixel tiles a side (an output side of 17 .. 48 is an input side of up to 96), B <= 2 there
    if entry in ("K16", "K19"):
        assert all(40 < max(c["H"], c["W"]) <= 96 and max(C.stem_out(c["H"]), C.stem_out(c["W"])) > 20 and c["B"] <= 2 for c in big), big
    else:
        assert len(big) == {"K12": 1, "K15": 2, "K17": 1, "K20": 1}.get(entry, 0) and all(c["B"] == 1 for c in big), big


def test_the_slicing_of_k13_is_the_entrys():
    """k13_qmax restates mcd_dwconv_bn_silu's host formula: the four values the plan names, and slices that cover nq."""
    assert [C.k13_qmax(k, s) for k, s in C.K13_KS] == [16, 8, 16, 7]
    for k, s in C.K13_KS:
        for nq in range(1, 60):
            n, qs = C.k13_slices(nq, k, s)
            assert qs <= C.k13_qmax(k, s) and (n - 1) * qs < nq <= n * qs


def test_the_over_cap_cases_are_past_their_caps():
    assert C.GRID_ITEMS == {"K12": 524288, "K15": 1048576, "K17": 1048576, "K20": 1048576}
    c = [c for c in case_list("K12") if c.get("big")][0]
    assert (c["H"] + 1) // 2 * ((c["W"] + 1) // 2) * (c["Cout"] // 4) == 529200
    assert sorted(c["HW"] * c["C"] // 4 for c in case_list("K15") if c.get("big")) == [1048578, 1049600]
    c = [c for c in case_list("K17") if c.get("big")][0]
    assert C.stem_out(c["H"]) * C.stem_out(c["W"]) * (c["C"] // 4) == 1065024
    c = [c for c in case_list("K20") if c.get("big")][0]
    assert (c["H"] // 2) * (c["W"] // 2) * (c["C"] // 4) == 1052672


# =========================================================================================================================
# 3. emulations and mutants
# =========================================================================================================================
MUTANTS = {
    "k18_drops_last_tile": ("K18", "K18R"),        # the last pixel tile is dropped when Mtot % 128 == 1
    "k18_first_image": ("K18", "K18R"),            # a tile that spans images reads every pixel from its first image
    "k18_second_chunk": ("K18", "K18R"),           # the second chunk's partial sum is dropped
    "k18_dy_dx": ("K18", "K18R"),                  # dy / dx swapped
    "k18r_relu_first": ("K18R",),                  # the ReLU before the residual
    "stem_pad_minus_one": ("K16", "K19"),          # pad K / 2 - 1
    "stem_first_pass_weights": ("K16", "K19"),     # channels >= 32 reuse the first pass's weights
    "k12_larger_half_on_top": ("K12",),            # TF-SAME's larger half on top and left
    "k12_cap": ("K12",),                           # items past cap * 256 are not written
    "k13_column_major": ("K13",),                  # psum tiles column-major
    "k13_last_slice": ("K13",),                    # the last channel slice is skipped when nq % QS != 0
    "k13_no_silu_in": ("K13",),                    # SiLU missing on the way in
    "k14_64t": ("K14",),                           # divides by 64 T
    "k14_untransposed": ("K14",),                  # w_et read as [C, sq]
    "k15_image_0": ("K15",),                       # the scale row of image 0 for every image
    "k15_mod_restarts": ("K15",),                  # i % nq restarted at each grid-stride trip
    "k0n_float4": ("K0N",),                        # the float4 grouping used when HW % 4 != 0
    "k17_pad_is_zero": ("K17",),                   # padding counted as 0 before the ReLU shift
    "k20_pitch": ("K20",),                         # row pitch 2 Wo for W
    "k21_hw_plus_one": ("K21",),                   # the mean over HW + 1
    "k31_regions_from_h": ("K31",),                # regions from H, W instead of Hp, Wp
    "k31_bias_transposed": ("K31",),               # the bias index transposed
    "k31_mask_at_s0": ("K31",),                    # a shift mask (that of shift w // 2) applied at s = 0
    "k31_pad_zeros": ("K31",),                     # padded keys read as zeros
    "k32_neighbour": ("K32",),                     # an odd edge reads the neighbouring row
}


def _chain(cols, w, chunk=None, skip=None):
    """cols [M, K] x w [Cout, K] -> [M, Cout]: every element an explicit sum in ascending k -- chunks of `chunk` values from 0,
    added in ascending order -- whose bits depend on its own row of cols and row of w alone.  skip: a chunk to leave out."""
    (M, K), ct, wt = cols.shape, cols.t().contiguous(), w.t().contiguous()
    total = None
    for n, c0 in enumerate(range(0, K, chunk or K)):
        acc = torch.zeros(M, w.shape[0])
        for k in range(c0, min(K, c0 + (chunk or K))):
            acc.addcmul_(ct[k][:, None], wt[k][None, :])
        if n != skip:
            total = acc if total is None else total + acc
    return total


class Emu:
    """call(name, ...) in fp32 torch; `mutant` switches one of MUTANTS on."""

    def __init__(self, mutant=None):
        self.m = mutant
        self.enc = TE.Emu()

    def __call__(self, name, **a):
        return getattr(self, name)(**a)

    def K10(self, **a):
        return self.enc.K10(**a)

    def K12(self, x, w, b):
        B, Cin, H, W = x.shape
        (Ho, pt, pb), (Wo, pl, pr) = C.same_pad(H, 3, 2), C.same_pad(W, 3, 2)
        if self.m == "k12_larger_half_on_top":
            pt, pb, pl, pr = pb, pt, pr, pl
        y = torch.cat([F.silu(F.conv2d(F.pad(x[i:i + 1], (pl, pr, pt, pb)), w.permute(3, 0, 1, 2).contiguous(), b, 2)) for i in range(B)])
        y = y.permute(0, 2, 3, 1).contiguous()
        if self.m == "k12_cap":
            y.view(B, -1)[:, 4 * C.GRID_ITEMS["K12"]:] = 0.0
        return y

    def K13(self, x, w, b, k, s, silu_in):
        B, H, W, Cc = x.shape
        y = C.dw_ref(x, w, b, k, s, silu_in and self.m != "k13_no_silu_in")
        nq = Cc // 4
        n, qs = C.k13_slices(nq, k, s)
        if self.m == "k13_last_slice" and nq % qs:
            y[..., 4 * (n - 1) * qs:] = 0.0
        psum = torch.cat([C.tile_sums(y[i:i + 1].clone()) for i in range(B)])
        if self.m == "k13_column_major":
            nty, ntx = -(-y.shape[1] // 8), -(-y.shape[2] // 8)
            psum = psum.view(B, nty, ntx, Cc).transpose(1, 2).reshape(B, nty * ntx, Cc)
        return y, psum

    def K14(self, psum, hw, wr, br, wet, be):
        B, T, Cc = psum.shape
        if self.m == "k14_untransposed":
            wet = wet.reshape(Cc, -1).t()
        out = []
        for i in range(B):
            acc = torch.zeros(Cc)
            for t in range(T):
                acc = acc + psum[i, t]
            mean = acc / float(64 * T if self.m == "k14_64t" else hw)
            hid = F.silu((wr * mean[None]).sum(1) + br)
            out.append(torch.sigmoid((wet * hid[:, None]).sum(0) + be))
        return torch.stack(out)

    def K15(self, y, s):
        B, HW, Cc = y.shape
        if self.m == "k15_image_0":
            return y * s[:1, None, :]
        if self.m == "k15_mod_restarts":
            nq, n4 = Cc // 4, HW * Cc // 4
            stride = 256 * min(-(-n4 // 1024), 1024)
            q = (torch.arange(n4) % stride) % nq
            return (y.view(B, n4, 4) * s.view(B, nq, 4)[:, q]).view(B, HW, Cc)
        return y * s[:, None, :]

    def _pool(self, x, mode):
        """x [B, C, HW] -> [B, C], K0's value."""
        if mode == "max":
            m = x.amax(dim=-1)
            return torch.where(torch.isnan(x).any(dim=-1), torch.full_like(m, NAN), m)
        act = F.silu if mode == "silu_avg" else (lambda t: t)
        return torch.cat([act(x[i:i + 1].clone()).sum(dim=-1) for i in range(x.shape[0])]) / float(x.shape[-1])

    def K0(self, x, mode):
        return self._pool(x, mode)

    def K0N(self, x, mode, place):
        x = x.transpose(1, 2).contiguous()
        if self.m == "k0n_float4" and x.shape[-1] % 4:       # the HW >> 2 whole groups, the tail never read
            HW = x.shape[-1]
            x = x[..., :HW - HW % 4]
            if mode == "max":
                return self._pool(x, mode) if x.shape[-1] else torch.full(x.shape[:2], -math.inf)
            return self._pool(x, mode) * float(x.shape[-1]) / float(HW) if x.shape[-1] else torch.zeros(x.shape[:2])
        return self._pool(x, mode)

    def _stem(self, x, w, b, relu):
        B, Cin, H, W = x.shape
        k, Cout = w.shape[1], w.shape[3]
        p = k // 2
        xp = F.pad(x, (p - 1, p + 1, p - 1, p + 1)) if self.m == "stem_pad_minus_one" else F.pad(x, (p,) * 4)
        cols = F.unfold(xp, k, stride=2).transpose(1, 2).reshape(-1, Cin * k * k)          # (channel, row, column), as the kernel's chain
        wm = w.reshape(Cin * k * k, Cout).t()
        if self.m == "stem_first_pass_weights":
            wm = wm[torch.arange(Cout) % 32]
        y = _chain(cols, wm).view(B, C.stem_out(H), C.stem_out(W), Cout)
        y = y if b is None else y + b
        return C.relu_keep(y) if relu else y

    def K16(self, x, w):
        return self._stem(x, w, None, 0)

    def K19(self, x, w, b, relu):
        return self._stem(x, w, b, relu)

    def K17(self, x, scale, shift):
        z = C.relu_keep(x * scale + shift).permute(0, 3, 1, 2)
        if self.m == "k17_pad_is_zero":
            zp = F.pad(z, (1, 1, 1, 1))
            edge = C.relu_keep(shift).view(1, -1, 1)
            zp[:, :, 0], zp[:, :, -1], zp[:, :, :, 0], zp[:, :, :, -1] = edge, edge, edge, edge
            return F.max_pool2d(zp, 3, 2, 0).permute(0, 2, 3, 1).contiguous()
        return F.max_pool2d(z, 3, 2, 1).permute(0, 2, 3, 1).contiguous()

    def K18(self, x, w, b, k, s, relu_in, relu_out, res=None):
        B, H, W, Cin = x.shape
        Cout, Ho, Wo = w.shape[0], C.k18_out(H, k, s), C.k18_out(W, k, s)
        a = (C.relu_keep(x) if relu_in else x).permute(0, 3, 1, 2)
        cols = F.unfold(a, k, padding=int(k == 3), stride=s).view(B, Cin, k * k, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, k * k * Cin)
        M = B * Ho * Wo
        if self.m == "k18_first_image":                      # pixel m of a tile: its place in its image, the tile's first image
            m = torch.arange(M)
            cols = cols[((m // 128) * 128 // (Ho * Wo)) * (Ho * Wo) + m % (Ho * Wo)]
        if self.m == "k18_dy_dx" and k == 3:
            w = w.view(Cout, k, k, Cin).transpose(1, 2).reshape(Cout, -1)
        y = _chain(cols, w, 256, 1 if self.m == "k18_second_chunk" else None) + b
        if res is not None and self.m == "k18r_relu_first":
            y = C.relu_keep(y) + res.reshape(M, Cout)
        else:
            y = y if res is None else y + res.reshape(M, Cout)
            y = C.relu_keep(y) if relu_out else y
        if self.m == "k18_drops_last_tile" and M % 128 == 1:
            y[M - 1] = 0.0
        return y.view(B, Ho, Wo, Cout)

    def K18R(self, **a):
        return self.K18(**a)

    def K20(self, x):
        B, H, W, Cc = x.shape
        if min(H, W) == 1:
            return x.new_zeros(B, H // 2, W // 2, Cc)
        if self.m == "k20_pitch":
            Ho, Wo = H // 2, W // 2
            flat = x.reshape(B, H * W, Cc)
            at = lambda dy, dx: flat[:, ((2 * torch.arange(Ho)[:, None] + dy) * 2 * Wo + 2 * torch.arange(Wo)[None, :] + dx).reshape(-1)]
            return ((((at(0, 0) + at(0, 1)) + at(1, 0)) + at(1, 1)) * 0.25).view(B, Ho, Wo, Cc)
        return F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()

    def K21(self, x, pos):
        B, HW, Cc = x.shape
        n = HW + 1 if self.m == "k21_hw_plus_one" else HW
        mean = torch.stack([x[i].sum(0) for i in range(B)]) * torch.full((1,), 1.0 / n)
        return torch.cat([(mean + pos[0])[:, None], x + pos[1:]], dim=1)

    def K31(self, qkv, pad, H, W, heads, w, s, table):
        B, T, D = qkv.shape[0], w * w, heads * 32
        Hp, Wp = -(-H // w) * w, -(-W // w) * w
        padv = torch.zeros(3 * D) if pad is None or self.m == "k31_pad_zeros" else pad
        full = padv.view(1, 1, 1, 3 * D).expand(B, Hp, Wp, 3 * D).clone()
        full[:, :H, :W] = qkv.view(B, H, W, 3 * D)
        rolled = torch.roll(full, (-s, -s), (1, 2))
        ii, jj = torch.arange(T) // w, torch.arange(T) % w
        di, dj = ii[:, None] - ii[None, :] + w - 1, jj[:, None] - jj[None, :] + w - 1
        bias = table[dj * (2 * w - 1) + di if self.m == "k31_bias_transposed" else di * (2 * w - 1) + dj].permute(2, 0, 1)
        ms = w // 2 if self.m == "k31_mask_at_s0" and s == 0 else s
        nr, nc = (H, W) if self.m == "k31_regions_from_h" else (Hp, Wp)
        out = torch.zeros(B, Hp, Wp, D)
        for b in range(B):
            for wr in range(Hp // w):
                for wc in range(Wp // w):
                    blk = rolled[b, wr * w:(wr + 1) * w, wc * w:(wc + 1) * w].reshape(T, 3, heads, 32)
                    q, k, v = (t.contiguous().clone() for t in blk.permute(1, 2, 0, 3))          # [heads, T, 32]
                    sc = q @ k.transpose(1, 2) / math.sqrt(32.0) + bias
                    if ms > 0:
                        reg = torch.tensor([3 * C.region(wr * w + int(i), nr, w, ms) + C.region(wc * w + int(j), nc, w, ms) for i, j in zip(ii, jj)])
                        sc = sc + (reg[:, None] != reg[None, :]).float() * -100.0
                    o = torch.softmax(sc, dim=-1) @ v
                    out[b, wr * w:(wr + 1) * w, wc * w:(wc + 1) * w] = o.permute(1, 0, 2).reshape(w, w, D)
        return torch.roll(out, (s, s), (1, 2))[:, :H, :W].reshape(B, H * W, D)

    def K32(self, x, H, W, g, b, eps):
        B, _, Cc = x.shape
        rows = C.gathered(x, H, W)
        if self.m == "k32_neighbour" and (H % 2 or W % 2):   # no edge test: whatever lies behind the row, behind the image
            flat = torch.cat([x, torch.full((B, W + 2, Cc), NAN)], dim=1)
            oy, ox = torch.arange((H + 1) // 2)[:, None], torch.arange((W + 1) // 2)[None, :]
            at = lambda dy, dx: flat[:, ((2 * oy + dy) * W + 2 * ox + dx).reshape(-1)]
            rows = torch.cat([at(0, 0), at(1, 0), at(0, 1), at(1, 1)], dim=-1)
        return self.enc.K10(x=rows.reshape(-1, 4 * Cc), g=g, b=b, eps=eps).view(B, -1, 4 * Cc)


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_the_checker_finds_nothing_on_the_emulations(entry):
    findings, ratio = C.run(entry, case_list(entry), Emu())
    print("%s: %d cases, max err / bound %.3f" % (entry, len(case_list(entry)), ratio))
    assert not findings, findings[:5]
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant,entry", [(m, e) for m, es in MUTANTS.items() for e in es])
def test_the_checker_finds_the_mutant(mutant, entry):
    call = Emu(mutant)
    for c in case_list(entry):
        findings, _ = C.check(entry, c, call)
        if findings:
            print(findings[0])
            return
    pytest.fail("no case of %s's committed list notices %s" % (entry, mutant))
