"""CPU: the scoring-side fuzzer (tests/scoring_fuzz.py) held to account without a GPU.

1. References: dispatch() against examples worked by hand here; the float64 references against independent formulations
   (torch.logsumexp, torch.softmax, a direct loop of rank_reorder restated from the reference file); the conditions of the
   numeric rules (K4's 99.5 % share, K5's column cap) on the oracle itself against float64 for the inputs the lists draw.
2. Coverage: at the committed seeds every dispatch class and stratum of the plan is in the generated lists (_need spells the
   set out), at most one `big` case, the operand bytes of an entry's list under a stated budget.
3. Mutants: oracle-backed emulations of the entries (tests/cpu_ops.py), on which the bit relations hold by construction.  The
   checker finds nothing on them over the whole committed lists, and finds every mutant of MUTANTS -- each aimed at a stratum
   that only these lists reach."""
import numpy as np
import pytest
import torch

import cpu_ops as OPS
import scoring_fuzz as SF

O = OPS.O
NAN = float("nan")
OUT_FILL = -7.0e30
BUDGET = 160 << 20                       # bytes of operands per entry's list (a `big` case apart): seconds on the GPU


def case_list(entry):
    return SF.cases(entry, SF.SEEDS[entry])


# =========================================================================================================================
# 1. the references
# =========================================================================================================================
def _k4(C, U=37, K=8, ldS=None, off=0, trusted=0, N=50, big=None):
    return SF.dispatch("K4", dict(C=C, U=U, K=K, ldS=ldS or -(-C // 96) * 96, off=off, trusted=trusted, N=N, big=big, soft=1))


def test_dispatch_matches_examples_worked_by_hand():
    # K4: C = 763 -> split 736 = 7 * 96 + 64, 27 columns behind it: rs_ok, 8 slices; 100 -> split 96, a slice boundary: rs_cut + tail
    assert _k4(763)[:3] == ("slice", "64", 8) and _k4(763)[7] is None
    assert _k4(100)[:3] == ("slice", "cut", 1) and _k4(100)[7] == 2            # 4 tail columns: gw_log2 2
    assert _k4(300)[:3] == ("slice", "cut", 3) and _k4(300)[7] == 4            # 12 tail columns
    assert _k4(864)[:3] == ("slice", "full", 9) and _k4(96)[:3] == ("slice", "full", 1) and _k4(91)[:3] == ("slice", "64", 1)
    assert _k4(96, U=1536)[5:7] == (1, "whole") and _k4(96, U=1537)[5:7] == (2, "part") and _k4(96, U=3072)[5:7] == (2, "whole")
    assert _k4(96, U=2048, trusted=1)[4:7] == (True, 1, "whole") and _k4(96, U=2049, trusted=1)[5:7] == (2, "part")
    assert _k4(96, U=2048, trusted=0)[5:7] == (2, "part")                      # 128 groups on 96 workgroups
    assert _k4(96, N=50, trusted=1, big=(12_000_000, None))[3:5] == (False, False)   # 4.6e9 bytes: 64-bit offsets, the checked form
    assert _k4(96, N=11_184_810)[3] is True and _k4(96, N=11_184_811)[3] is False
    assert _k4(763, ldS=763) == ("main", ("ldS",), False, 5) and _k4(763, ldS=764)[2] is True
    assert _k4(763, K=5)[:2] == ("main", ("K%4",)) and _k4(96, K=256)[:2] == ("main", ("K>=256",))
    assert _k4(33) == ("main", ("rs",), True, 0) and _k4(63)[3] == 5 and _k4(44)[3] == 4
    assert _k4(3) == ("tail-only", ("rs",), None, 2) and _k4(5) == ("main", ("rs",), True, 0)
    # K5: the largest segment picks the route; an empty segment is no segment
    k5 = lambda segs, C=20, ld=20, off=0: SF.dispatch("K5", dict(segs=segs, C=C, ld=ld, ldo=ld, off=off))
    assert k5([0, 1920]) == ("panel", 16, True, 2, 1) and k5([0, 1921]) == ("panel", 8, False, 3, 1)
    assert k5([0, 3840])[1] == 8 and k5([0, 3841])[0] == "three" and k5([0, 3841])[1] is False
    assert k5([0, 3841, 3841, 4241, 4246])[:2] == ("three", True) and k5([0, 40, 40, 110])[4] == 2
    assert k5([0, 70], C=33, ld=33)[2] is False and k5([0, 70], C=33, ld=36)[2:4] == (True, 3) and k5([0, 70], off=1)[2] is False
    # K1: 512 = 2 x 256 (whole K tiles: dma, K-blocks), 416 = 2 x 208 (no K tile boundary at 208: the plain form), 384: no blocks
    k1 = lambda N, C, D, ldi=None, ldp=None, off=0: SF.dispatch("K1", dict(N=N, C=C, D=D, ldi=ldi or D, ldt=D, ldp=ldp or C, off=off))
    assert k1(130, 140, 512) == ("dma<bst>", True, 2, 1, 2) and k1(130, 140, 384)[:2] == ("dma<bst>", False)
    assert k1(130, 140, 416)[:2] == ("f32<aligned>", True) and k1(130, 140, 100)[:2] == ("f32<aligned>", False)
    assert k1(130, 140, 800)[:2] == ("dma<bst>", True) and k1(130, 140, 388)[:2] == ("f32<aligned>", True)
    assert k1(37, 50, 512, ldi=513)[:2] == ("f32<unaligned>", True) and k1(130, 140, 64, off=1)[0] == "f32<unaligned>"
    assert k1(2, 130, 64, ldp=(1 << 22) + 4)[0] == "dma<plain>" and k1(2, 130, 64, ldp=(1 << 22) - 4)[0] == "dma<bst>"
    assert k1(1024, 100, 64)[2:] == (8, 1, 1) and k1(1025, 800, 64)[2:] == (9, 2, 7) and k1(2100, 300, 64)[2:] == (17, 3, 3)
    assert SF.gemm_kblocks(768) == (True, 384, 0) and SF.gemm_kblocks(769) == (True, 384, 384) and SF.gemm_kblocks(385) == (True, 196, 0)
    # K1A, K2, K8
    assert [SF.dispatch("K1A", dict(n=9, d=d))[0] for d in (128, 129, 512, 513, 1024, 1025)] == [16, 64, 64, 128, 128, 0]
    k2 = lambda C, lds, ldp=None, off=0: SF.dispatch("K2", dict(C=C, lds=lds, ldp=ldp or C, off=off))
    assert k2(8, 1024)[0] == "reg<16>" and k2(200, 200)[0] == "reg<16>" and k2(16, 192)[0] == "reg<16>" and k2(255, 384) == ("lds<128>", False)
    assert k2(1024, 1152, ldp=1024) == ("lds<128>", True) and k2(1025, 1152)[0] == "lds<256>" and k2(16384, 16512, 16384) == ("lds<256>", True)
    assert k2(16385, 16512)[0] == "stream" and k2(764, 768, 764, off=1) == ("lds<128>", False)
    k8 = lambda top_n, C, ldP=None, off=0: SF.dispatch("K8", dict(top_n=top_n, C=C, ldP=ldP or C, off=off))
    assert k8(1, 8) == (2, False, True, 0) and k8(1024, 8)[:2] == (1024, False) and k8(1025, 8)[:2] == (2048, True) and k8(4096, 8)[0] == 4096
    assert k8(5, 7)[2:] == (False, 4) and k8(5, 7, ldP=8)[2] is True and k8(5, 763, ldP=764, off=1)[2] is False and k8(5, 33)[3] == 32


def test_float64_references_against_independent_formulations():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 37, generator=g) * 3 - 400
    x[:, 1] = float("-inf")
    segs = [0, 70, 70, 300]
    want = torch.cat([x[a:b].double() - 0.6 * (torch.logsumexp(x[a:b].double(), 0, keepdim=True) - np.log(b - a)) for a, b in ((0, 70), (70, 300))])
    got = SF.lse_ref64(x, segs, 0.6)
    fin = torch.isfinite(want)
    assert float((got - want)[fin].abs().max()) <= 1e-10 and torch.equal(torch.isnan(got), torch.isnan(want))
    P = torch.randn(9, 50, generator=g)
    assert float((SF.softmax_ref64(P, 10.0) - torch.softmax(10.0 * P.double(), 1)).abs().max()) <= 1e-15
    S = torch.softmax(torch.randn(20, 7, generator=g), 1)
    idx = torch.randint(0, 20, (3, 4), generator=g, dtype=torch.int32)
    p = torch.from_numpy(O.p_in_examples(4))
    for soft in (0, 1):
        want = torch.zeros(3, 7, dtype=torch.float64)
        for u in range(3):
            for j in range(4):
                gj = S[int(idx[u, j])]                                           # the term in fp32, its log in float64
                want[u] += torch.log(((1 + p[j] * (gj - 1)) + np.float32(1e-7) if soft else gj + np.float32(1e-7)).double())
        assert float((SF.wpmi_ref64(S, idx, p, 1e-7, soft) - want).abs().max()) <= 1e-12
    x = torch.randn(4, 33, generator=g)
    d = x.double() - x.double().mean(1, keepdim=True)
    assert float((SF.ccn_ref64(x, 1e-3) - d ** 3 / (d ** 3).norm(dim=1, keepdim=True)).abs().max()) <= 1e-15


def _rank_reorder_loop(P, tvals, tidx, perms, p, scale_p):
    """similarity.py:107-132 restated: per neuron, the gathered rows' column-wise ranks pick sorted activations."""
    U, top_n = tvals.shape
    out = np.zeros((U, P.shape[1]))
    for u in range(U):
        t = [float(v) for v in tvals[u]]
        st = sorted(t)
        base = np.mean([abs(st[j] - st[int(perms[u, k, j])]) ** p for k in range(perms.shape[1]) for j in range(top_n)])
        for c in range(P.shape[1]):
            col = [float(P[int(tidx[u, j]), c]) for j in range(top_n)]
            ranks = [sum(1 for v in col if v < col[j]) for j in range(top_n)]
            err = np.mean([abs(t[j] - st[ranks[j]]) ** p for j in range(top_n)]) / base
            out[u, c] = -err / np.mean(col) ** scale_p
    return out


@pytest.mark.parametrize("p,scale_p", [(3.0, 0.5), (2.5, 1.0), (1.0, 0.5)])
def test_rank_reorder_references_against_a_direct_loop(p, scale_p):
    case = dict(N=40, C=6, U=2, top_n=17, n_perm=3, regime="softmax", ds=11)
    P, tvals, tidx, perms = SF.k8_operands(case)
    want = _rank_reorder_loop(P.double().numpy(), tvals.double().numpy(), tidx.numpy(), perms.numpy(), p, scale_p)
    assert np.abs(SF.rank_reorder_ref64(P, tvals, tidx, perms, p, scale_p).numpy() - want).max() <= 1e-9 * np.abs(want).max()
    got = OPS.rank_reorder(P, tvals, tidx, perms, p, scale_p).double().numpy()                # the oracle's primitives, fp32
    assert (np.abs(got - want) <= 5e-6 * np.abs(want) + 1e-9).all()


def test_the_oracle_meets_the_rules_conditions_on_the_drawn_inputs():
    """K4's 99.5 % share and K5's column cap are conditions on the inputs as much as on the kernels: what may differ between two
    faithful implementations is the last bit of a log or an exp.  The oracle against float64 -- its fp32 terms, their log / exp
    taken in float64 and rounded once, then ATen's summation order (oracle.sum0) -- stays inside the tolerance on every drawn
    case, equals those bits on 99.5 % of a case's entries (K4) and differs on at most max(1, C // 200) columns (K5)."""
    f32 = np.float32
    for c in case_list("K4"):
        S, idx, p, _ = SF.k4_operands(c)
        g = S[idx.long()]                                                        # [U, K, C]
        w = (1.0 + p[None, :, None] * (g - 1.0)) + f32(SF.MIN_PROB) if c["soft"] else g + f32(SF.MIN_PROB)
        assert w.dtype == torch.float32
        logs = torch.log(w.double()).float().numpy()
        ref = torch.from_numpy(np.stack([O.sum0(np.ascontiguousarray(logs[u])) for u in range(c["U"])]))
        err, tol, exact = SF.k4_rule(OPS.wpmi_score(S, idx, p, f32(SF.MIN_PROB), c["soft"]), ref)
        assert err <= tol and exact >= 0.995, (c["i"], err, tol, exact)
        far = float((ref.double() - SF.wpmi_ref64(S, idx, p if p is not None else torch.zeros(c["K"]), SF.MIN_PROB, c["soft"])).abs().max())
        assert far <= 2.0 ** -24 * c["K"] * float(ref.abs().max()), (c["i"], far)     # the fp32 sum of K terms against the float64 one
    with np.errstate(all="ignore"):
        for c in case_list("K5"):
            x = SF.k5_operands(c)[c["segs"][0]:]
            segs = [s - c["segs"][0] for s in c["segs"]]
            ref = np.empty(tuple(x.shape), f32)
            for a, b in zip(segs[:-1], segs[1:]):
                if b > a:
                    v = x[a:b].numpy()
                    m = v.max(axis=0)
                    m = np.where(np.isinf(m), f32(0), m)
                    s = O.sum0(np.exp((v - m).astype(np.float64)).astype(f32))
                    prob_d = (np.log(s.astype(np.float64)).astype(f32) + m) - f32(np.log(np.float64(f32(b - a))))
                    ref[a:b] = v - f32(c["lam"]) * prob_d
            ck = SF._Ck("K5", c)
            SF.k5_rule(ck, "the oracle against float64 in ATen's order", OPS.logsumexp_sub(x, c["lam"], segs), torch.from_numpy(ref), x, c["C"])
            assert not ck.findings, ck.findings


# =========================================================================================================================
# 2. coverage
# =========================================================================================================================
def _need(entry):
    need = {("regime", r) for r in SF.REGIMES}
    if entry == "K1":
        need |= {("form", f, kb) for f in ("dma<bst>", "dma<plain>", "f32<aligned>", "f32<unaligned>") for kb in (False, True)}
        need |= {("tiles", t, n) for t in (1, 8, 9, 17) for n in (1, 2, 3, 7)}
        need |= {("D", D) for D in (32, 64, 384, 416, 512, 768, 800, 100, 388)}
        need |= {("ragged row tile",), ("ragged column tile",), ("ldp > C",), ("N < 128",), ("band 1",)}
    elif entry == "K1A":
        need |= {("NV", 16, 16), ("NV", 64, 17), ("NV", 64, 64), ("NV", 128, 65), ("NV", 128, 128), ("NV", 0, 129)}
        need |= {("n % 8", r) for r in range(8)} | {("ldx",), ("ldy",), ("in place",)}
    elif entry == "K2":
        need |= {("reg by", "lds"), ("reg by", "C < 16 wide")}
        need |= {("form", "lds<128>", v, C) for v in (False, True) for C in (16, 255, 256, 763, 1024)}
        need |= {("form", "lds<256>", v, C) for v in (False, True) for C in (1025, 4099, 16384)}
        need |= {("form", "stream", None, 16385), ("pad_to", 192), ("pad_to", None)} | {("N % 16", r) for r in (0, 1, 15)}
        need |= {("regression: a NaN row keeps its +0 padding", "reg<16>", short) for short in (False, True)}
    elif entry == "K4":
        need |= {("rs", "full", 96), ("rs", "full", 768), ("rs", "full", 864), ("rs", "64", 763), ("rs", "64", 91), ("rs", "cut", 100),
                 ("rs", "cut", 300), ("slice + tail", 2), ("slice + tail", 4)}
        need |= {("n_slices", n) for n in (1, 8, 9)} | {("OFF32", False), ("OFF32", True), ("U % 16",), ("big",)}
        need |= {("passes", False, 1, "whole", 1536), ("passes", False, 2, "part", 1537), ("passes", False, 2, "part", 1552),
                 ("passes", False, 2, "whole", 3072), ("passes", True, 1, "whole", 2048), ("passes", True, 2, "part", 2049),
                 ("passes", True, 2, "part", 2064), ("passes", True, 2, "whole", 4096)}
        need |= {("form", s, t) for s in (0, 1) for t in (False, True)} | {("soft", s) for s in (0, 1)} | {("trusted", t) for t in (0, 1)}
        need |= {("route", r) for r in ("slice", "main", "tail-only")}
        need |= {("cause", n) for n in ("ldS", "K%4", "K>=256", "rs", "align")} | {("vec2", False), ("vec2", True)}
        need |= {("K", K) for K in (256, 260, 333)}
        need |= {("tail", w, g) for w, g in ((1, 0), (2, 1), (3, 2), (5, 3), (12, 4), (31, 5))}
    elif entry == "K5":
        need |= {("Umax", U) for U in (1, 63, 64, 65, 1920, 1921, 3840, 3841)}
        need |= {("route", "panel", 16), ("route", "panel", 8), ("route", "three", False), ("route", "three", True)}
        need |= {("vec_ok", 16, True), ("vec_ok", 16, False), ("n_panels", 0), ("n_panels", 1)}
        need |= {("segments", k) for k in (1, "empty middle", 64)} | {("C", C) for C in (15, 16, 17, 31, 32, 33, 63, 64, 65)}
        need |= {("the same rows under three routes",)}
    elif entry in ("K7", "K7G"):
        need |= {("n", n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 61, 126, 128, 300, 517, 1021, 1024, 1029, 2050, 10003)} | {("dead rows",)}
        if entry == "K7G":
            need |= {("G", G) for G in (1, 2, 3, 64)} | {("empty piece",)}
    elif entry == "K8":
        need = {("regime", r) for r in ("softmax", "cancel", "randn")}
        need |= {("top_n", t, n, b) for t, n, b in ((1, 2, False), (2, 2, False), (3, 4, False), (4, 4, False), (5, 8, False), (255, 256, False),
                                                    (256, 256, False), (257, 512, False), (1024, 1024, False), (1025, 2048, True),
                                                    (4096, 4096, True))}
        need |= {("VEC4", True, r) for r in range(4)} | {("VEC4", False, r) for r in range(4)} | {("ragged tile, scalar",), ("one NaN",)}
        need |= {("C", C, s) for C, s in ((1, 0), (3, 0), (4, 4), (7, 4), (8, 0), (31, 0), (32, 32), (33, 32), (763, 736))}
        need |= {("n_perm", n) for n in (1, 5)} | {("p", p) for p in (1.0, 2.0, 3.0, 2.5)} | {("scale_p", s) for s in (0.5, 1.0)}
        need |= {("U", 1), ("U", 5)}
    return need


@pytest.mark.parametrize("entry", SF.ENTRIES)
def test_every_stratum_is_in_the_committed_list(entry):
    cl = case_list(entry)
    missing = _need(entry) - SF.strata(entry, cl)
    assert not missing, (entry, sorted(missing, key=str))
    assert cl == case_list(entry), "the list is not deterministic"
    assert sum(1 for c in cl if c.get("big")) <= 1
    total = sum(SF.case_bytes(entry, c) for c in cl if not c.get("big"))
    print("%s: %d cases, %.1f MB of operands" % (entry, len(cl), total / 2 ** 20))
    assert total <= BUDGET, (entry, total)
    for c in cl:
        if c.get("big"):                                            # OFF32 = false and nothing more: a few rows of 96 concepts
            assert entry == "K4" and c["big"][0] * c["ldS"] * 4 >= 1 << 32 and c["big"][0] < 1 << 24 and c["U"] * c["C"] <= 4096


def test_sum_split_is_the_oracles():
    """sum_split restates ATen's rule the oracle carries (mcd_o_sum_split)."""
    for C in (1, 3, 4, 7, 8, 31, 32, 33, 100, 763, 10000):
        assert SF.sum_split(C) == O.sum_split(C), C


# =========================================================================================================================
# 3. emulations and mutants
# =========================================================================================================================
MUTANTS = {
    "k1_band1_rows_from_band0": "K1",            # row tiles 8.. computed from the rows of tiles 0..
    "k4_second_pass_skipped": "K4",              # the persistent loop ends after its first neuron group
    "k4_dead_lane_writes_row_u": "K4",           # a dead lane of the partly dead last pass writes row U
    "k4_offset_wraps_at_2_32": "K4",             # 32-bit gather offsets on a matrix of 4.6e9 bytes
    "k5_panel8_plain_order": "K5",               # panel <8> adds its column in plain order
    "k5_empty_segment_shifts_table": "K5",       # an empty segment keeps its slot: the last live one falls off the table
    "k8_padding_key_first": "K8",                # the padding keys sort in front: the sorted positions move by npad - top_n
    "k8_plain_column_mean_below_8": "K8",        # the column mean in plain order where C < 8
    "k2_lds256_drops_last_quad": "K2",           # lds<256> leaves the last partial quad out of the row
    "k5_three_pass_first_z_only": "K5",          # further: blockIdx.z > 0 adds nothing (super-chunks past the first four)
    "k7g_piece_order": "K7G",                    # further: the pieces concatenated in reverse order
    "k1a_nv_edge": "K1A",                        # further: the last element of a row past 128 lanes' worth is left out of the norm
}


class Emu:
    """call(name, ...) on the oracle (tests/cpu_ops.py), one row / neuron / segment at a time by the oracle's own construction;
    `mutant` switches one of MUTANTS on."""

    def __init__(self, mutant=None):
        self.m = mutant

    def __call__(self, name, gap=NAN, **a):
        return getattr(self, name)(**a)

    def K1A(self, x, ldx, ldy, in_place):
        out = OPS.normalize_rows(x)
        if self.m == "k1a_nv_edge" and x.shape[1] > 1024:
            out = torch.cat([OPS.normalize_rows(x[:, :-1].contiguous()), x[:, -1:] / x[:, :-1].norm(dim=1, keepdim=True)], dim=1)
        return out

    def K1(self, I, T, ldi, ldt, ldp, off):
        out = OPS.embed_gemm(I, T)
        if self.m == "k1_band1_rows_from_band0" and I.shape[0] > 1024:
            out[1024:] = out[:I.shape[0] - 1024].clone()
        return out

    def K2(self, P, a, ldp, lds, off):
        N, C = P.shape
        out = torch.from_numpy(O.row_softmax(P.numpy(), a))
        if self.m == "k2_lds256_drops_last_quad" and C % 4 and SF.dispatch("K2", dict(C=C, ldp=ldp, lds=lds, off=off))[0] == "lds<256>":
            out[:, :C - C % 4] = torch.from_numpy(O.row_softmax(P[:, :C - C % 4].contiguous().numpy(), a))
        return out

    def K4(self, S, idx, p, min_prob, soft, trusted, ldS, off, big):
        (N, C), (U, K) = S.shape, idx.shape
        d = SF.dispatch("K4", dict(C=C, U=U, K=K, ldS=ldS, off=off, trusted=trusted, N=N, big=big, soft=soft))
        if self.m == "k4_offset_wraps_at_2_32" and big:
            S = S.clone()
            S[[r for r, row in enumerate(big[1]) if row * ldS * 4 >= 1 << 32]] = 0.0
        buf = torch.full((U + 1, C), OUT_FILL)
        buf[:U] = OPS.wpmi_score(S, idx, p, np.float32(min_prob), soft)
        if d[0] == "slice" and d[5] > 1:
            first = 16 * (128 if d[4] else 96)
            if self.m == "k4_second_pass_skipped":
                buf[first:U] = OUT_FILL
            if self.m == "k4_dead_lane_writes_row_u" and d[6] == "part" and U % 16:
                buf[U] = buf[U - 1]
        assert bool((buf[U] == OUT_FILL).all()), "K4: elements outside the logical region changed"
        assert not bool((buf[:U] == OUT_FILL).any()), "K4: an output element was not written"
        return buf[:U].clone()

    def K5(self, x, segs, lam, ld, ldo, off):
        U, C = x.shape
        d = SF.dispatch("K5", dict(segs=segs, C=C, ld=ld, ldo=ldo, off=off))
        out = torch.full((U, C), OUT_FILL)
        out[:segs[0]] = 0.0
        live = [(a, b) for a, b in zip(segs[:-1], segs[1:]) if b > a]
        if self.m == "k5_empty_segment_shifts_table" and any(b == a for a, b in zip(segs[1:-2], segs[2:-1])):
            live = live[:-1]
        for a, b in live:
            v = x[a:b].contiguous()
            if self.m == "k5_panel8_plain_order" and d[:2] == ("panel", 8):
                out[a:b] = self._lse_plain(v, lam, b - a)
            elif self.m == "k5_three_pass_first_z_only" and d[0] == "three" and b - a >= 320:
                m = v.max(dim=0, keepdim=True).values
                s = (torch.exp(v[:256] - m).sum(dim=0, keepdim=True) + torch.exp(v[(b - a) // 64 * 64:] - m).sum(dim=0, keepdim=True))
                out[a:b] = v - lam * (torch.log(s) + m - float(np.log(b - a)))
            else:
                out[a:b] = OPS.logsumexp_sub(v, lam)
        assert not bool((out == OUT_FILL).any()), "K5: an output element was not written"
        return out

    @staticmethod
    def _lse_plain(v, lam, n):
        f32 = np.float32
        a = v.numpy()
        with np.errstate(all="ignore"):
            m = a.max(axis=0)
            m = np.where(np.isinf(m), f32(0), m)
            s = np.exp(a - m).cumsum(axis=0, dtype=f32)[-1]
            scaled = f32(lam) * ((np.log(s).astype(f32) + m) - np.log(f32(n)).astype(f32))
            return torch.from_numpy((a - scaled).astype(f32))

    def K7(self, x, min_norm, ldx, ldy):
        return OPS.center_cube_normalize_rows(x, min_norm)

    def K7G(self, pieces, rows, mode, min_norm, pad):
        if self.m == "k7g_piece_order":
            pieces = pieces[::-1]
        return OPS.prepare_rows_gathered(pieces, rows, mode, min_norm)

    def K8(self, P, ldP, off, tvals, tidx, perms, p, scale_p):
        C, top_n = P.shape[1], tvals.shape[1]
        npad = SF.dispatch("K8", dict(C=C, ldP=ldP, off=off, top_n=top_n))[0]
        order = colsum = None
        if self.m == "k8_padding_key_first":
            order = lambda G: np.roll(np.argsort(G, axis=0, kind="stable"), (npad - top_n) % top_n, axis=0)
        if self.m == "k8_plain_column_mean_below_8" and C < 8:
            colsum = lambda G: G.cumsum(axis=0, dtype=np.float32)[-1]
        return OPS.rank_reorder(P, tvals, tidx, perms, p, scale_p, order=order, colsum=colsum)


@pytest.mark.parametrize("entry", SF.ENTRIES)
def test_the_checker_finds_nothing_on_the_emulations(entry):
    findings, ratio = SF.run(entry, case_list(entry), Emu())
    print("%s: %d cases, max err / bound %.3f" % (entry, len(case_list(entry)), ratio))
    assert not findings, findings[:5]
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant,entry", list(MUTANTS.items()))
def test_the_checker_finds_the_mutant(mutant, entry):
    call = Emu(mutant)
    for c in case_list(entry):
        findings, _ = SF.check(entry, c, call)
        if findings:
            print(findings[0])
            return
    pytest.fail("no case of %s's committed list notices %s" % (entry, mutant))
