"""The scoring-side fuzzer, by dispatch class: the third twin of encoder_fuzz.py and conv_fuzz.py, for K1A (mcd_normalize_rows),
K1 (mcd_embed_gemm, f32 mode), K2 (mcd_row_softmax), K4 (mcd_wpmi_score), K5 (mcd_logsumexp_sub), K7
(mcd_center_cube_normalize_rows), K7G (mcd_prepare_rows_gathered) and K8 (mcd_rank_reorder).  Importing it touches no GPU.

  dispatch(entry, case)     a Python restatement of the entry's HOST dispatch (the .hip host functions, file and lines beside each):
                            a tuple naming the kernel form, its template flags, passes, panel width, npad ...  strata() is built
                            from it, so a changed threshold in the library shows as a missing stratum in the CPU test once the
                            restatement follows it -- and as a restatement that no longer matches its source until then.
  cases(entry, seed)        every stratum first (the smallest shapes that reach it), a few random cases behind them.
  check(entry, case, call)  the oracle's bits where DESIGN.md claims bits (K1A, K1, K2, K7G), the existing numeric rules elsewhere
                            (K4, K5: scripts/fuzz_core.py; K7: cos_similarity_cubed at 5e-7 and float64 at conv_fuzz's rule; K8:
                            scripts/fuzz_sim.py), and the bit relations that hold by construction of the kernels: a row / neuron /
                            segment alone, the batch reversed, both guard fills, the entry's own (pitch, route, trusted) twins.

What call(name, gap=..., **operands) is given (tensors on check()'s device, pitches and base offsets in elements; gap is the
fill of the frames' guards and pitch gaps -- an emulation ignores it):
  K1A  x [n, d], ldx, ldy, in_place                                                        -> [n, d]
  K1   I [N, D], T [C, D], ldi, ldt, ldp, off (base offset of I and T)                      -> [N, C]
  K2   P [N, C], a, ldp, lds, off                                                           -> [N, C] (pad columns must be +0)
  K4   S [N, C], idx [U, K] int32, p [K] | None, min_prob, soft, trusted, ldS, off, big     -> [U, C]
       big = None | (N_big, rows): S's row r is row rows[r] of an [N_big, ldS] matrix nothing else of which is written
  K5   x [U, C], segs (list), lam, ld, ldo, off                                             -> [U, C]
  K7   x [rows, n], min_norm, ldx, ldy                                                      -> [rows, n]
  K7G  pieces (list of [R, counts[g]]), rows (row0, row1), mode, min_norm                   -> [row1 - row0, n]
  K8   P [N, C], ldP, off, tvals [U, top_n], tidx int32, perms int32 [U, n_perm, top_n], p, scale_p -> [U, C]"""
import numpy as np
import torch

import cpu_ops as OPS
from encoder_fuzz import _Ck, _finish, _ptr, bits  # noqa: F401  (the frame helpers and bits() are the encoder fuzzer's)

O = OPS.O
NAN = float("nan")
GAPS = (NAN, 1.0e30)                                   # util.GAP_FILLS
ENTRIES = ("K1A", "K1", "K2", "K4", "K5", "K7", "K7G", "K8")
SEEDS = {e: 9001 + i for i, e in enumerate(ENTRIES)}  # the committed seed of every entry's test
REGIMES = ("unit", "x30", "x1e-3", "off100")
MIN_PROB = 1e-7

K1_D = (32, 64, 384, 416, 512, 768, 800, 100, 388)
K1_N = (100, 1024, 1025, 2100)                         # 1, 8, 9 (the last ragged) and 17 row tiles
K1_C = (100, 200, 300, 800)                            # 1, 2, 3 and 7 column tiles
K1A_D = (128, 129, 512, 513, 1024, 1025)               # per_lane = ceil(d / 8) at 16 | 17, 64 | 65, 128 | 129
K2_C = (5, 15, 16, 255, 256, 763, 1024, 1025, 4099, 16384, 16385)
K4_SLICED_C = (96, 768, 864, 763, 91, 100, 300)
K4_U_CHECKED = (1536, 1537, 1552, 3072)
K4_U_TRUSTED = (2048, 2049, 2064, 4096)
K4_TAIL_C = (33, 34, 35, 37, 44, 63)                   # tail widths 1, 2, 3, 5, 12, 31: gw_log2 0, 1, 2, 3, 4, 5
K4_BIG_N = 12_000_000                                  # N * 96 * 4 = 4.6e9 >= 2^32 with N < 2^24: OFF32 = false
K5_UMAX = (1, 63, 64, 65, 1920, 1921, 3840, 3841)
K5_C = (15, 16, 17, 31, 32, 33, 63, 64, 65)
ROW_N = (1, 2, 3, 4, 5, 6, 7, 8, 61, 126, 128, 300, 517, 1021, 1024, 1029, 2050, 10003)   # test_prepare_rows_gathered_bit_equal
K7G_G = (1, 2, 3, 64)
K8_TOP = (1, 2, 3, 4, 5, 255, 256, 257, 1024, 1025, 4096)
K8_C = (1, 3, 4, 7, 8, 31, 32, 33, 763)
K8_P = (1.0, 2.0, 3.0, 2.5)


def cdiv(a, b):
    return -(-a // b)


def sum_split(C):
    """ATen's cascade / row_sum column split (k_wpmi.hip:1073, :1194; k_rank.hip:232)."""
    return (C // 32) * 32 if C >= 8 else (C // 4) * 4


# =========================================================================================================================
# 1. the host dispatch, restated
# =========================================================================================================================
def gemm_kblocks(D):
    """k_gemm.hip:376-386 (gemm_kblocks): (kblocks, first, step)."""
    if D <= 384:
        return False, D, 0
    if D <= 768:
        return True, ((D + 1) // 2 + 3) // 4 * 4, 0
    return True, 384, 384


def _dispatch_k1(c):
    """k_gemm.hip:1109-1135 (mcd_embed_gemm, MCD_GEMM_F32) and :27-33 (xcd_tile): (form, KBLOCKS, row tiles, bands, ncol)."""
    N, C, D, ldi, ldt, ldp = (c[k] for k in ("N", "C", "D", "ldi", "ldt", "ldp"))
    aligned = ldi % 4 == 0 and ldt % 4 == 0 and c["off"] % 4 == 0
    kb, first, step = gemm_kblocks(D)
    dma = aligned and D % 32 == 0 and first % 32 == 0 and step % 32 == 0 and N * ldi < (1 << 29) and C * ldt < (1 << 29)
    bst = max(N, 128) * ldp * 4 < (1 << 31)
    form = ("dma<bst>" if bst else "dma<plain>") if dma else ("f32<aligned>" if aligned else "f32<unaligned>")
    tiles = cdiv(N, 128)
    return form, kb, tiles, cdiv(tiles, 8), cdiv(C, 128)


def _dispatch_k1a(c):
    """k_rows.hip:392-399 (mcd_normalize_rows): (NV, per_lane, workgroups of 8 rows)."""
    per_lane = cdiv(c["d"], 8)
    return (16 if per_lane <= 16 else 64 if per_lane <= 64 else 128 if per_lane <= 128 else 0), per_lane, cdiv(c["n"], 8)


def _dispatch_k2(c):
    """k_rows.hip:411-426 (mcd_row_softmax): (form, vec4)."""
    C, ldp, lds = c["C"], c["ldp"], c["lds"]
    vec4 = ldp % 4 == 0 and lds % 4 == 0 and c["off"] % 4 == 0
    if lds <= 256 or C < 16:
        return "reg<16>", None
    if C <= 1024:
        return "lds<128>", vec4
    if C <= 16384:
        return "lds<256>", vec4
    return "stream", None


def _dispatch_k4(c):
    """k_wpmi.hip:1073-1155 (mcd_wpmi_score): ("slice", rs, n_slices, OFF32, TRUSTED, passes, last pass, tail gw_log2 | None) or
    ("main" | "tail-only", causes, vec2, tail gw_log2 | None)."""
    C, ldS, K, U, off = c["C"], c["ldS"], c["K"], c["U"], c["off"]
    N = c["big"][0] if c.get("big") else c["N"]
    split = min(sum_split(C), C)
    trusted = bool(c["trusted"]) and 2.0 ** -25 <= MIN_PROB < 1.0                      # log_table.inc: MCD_LOG_E_MIN = -25
    vec2 = ldS % 2 == 0 and off % 2 == 0 and split % 2 == 0
    rs_ok = split >= C or (split % 96 == 64 and C - split < 32)
    rs_cut = not rs_ok and split > 0 and split % 96 == 0
    gl = None if split >= C else max(C - split - 1, 0).bit_length()                    # ilog2_ceil(C - split)
    if ldS % 96 == 0 and off % 4 == 0 and K % 4 == 0 and K < 256 and (rs_ok or rs_cut):
        Cs = split if rs_cut else C
        groups = cdiv(U, 16)
        off32 = N < (1 << 24) and ldS * 4 < (1 << 24) and N * ldS * 4 < (1 << 32)
        wg = min(groups, 128 if trusted and off32 else 96)
        rs = "cut" if rs_cut else ("full" if split >= C else "64")
        return ("slice", rs, cdiv(Cs, 96), off32, trusted and off32, cdiv(groups, wg), "whole" if groups % wg == 0 else "part",
                gl if rs_cut else None)
    causes = tuple(n for n, on in (("ldS", ldS % 96 != 0), ("align", off % 4 != 0), ("K%4", K % 4 != 0), ("K>=256", K >= 256),
                                   ("rs", not (rs_ok or rs_cut))) if on)
    return ("main" if split > 0 else "tail-only", causes, vec2 if split > 0 else None, gl)


def k5_live(segs):
    """The rows of the segments that have any (k_wpmi.hip:1178-1189: an empty segment is left out of the table)."""
    return [b - a for a, b in zip(segs[:-1], segs[1:]) if b > a]


def _dispatch_k5(c):
    """k_wpmi.hip:1173-1237 (mcd_logsumexp_sub): ("panel", W, vec_ok, n_panels, live segments) or ("three", blockIdx.z > 0 works)."""
    rows = k5_live(c["segs"])
    Umax, C = max(rows), c["C"]
    W = 16 if Umax <= 1920 else (8 if Umax <= 3840 else 0)
    if W:
        vec_ok = W == 16 and c["ld"] % 4 == 0 and c["ldo"] % 4 == 0 and c["off"] % 4 == 0
        return "panel", W, vec_ok, cdiv(C, W), len(rows)
    max_super = max(r >> 6 for r in rows)
    return "three", cdiv(max_super, 4) > 1 and sum(1 for r in rows if (r >> 6) > 4) > 1, None, cdiv(C, 64), len(rows)   # K5_SB = 4


def _dispatch_k8(c):
    """k_rank.hip:232-253 (mcd_rank_reorder): (npad, the > 48 KB attribute branch, VEC4, split)."""
    C, ldP, top_n = c["C"], c["ldP"], c["top_n"]
    npad = 2
    while npad < top_n:
        npad <<= 1
    vec4 = ldP % 4 == 0 and c["off"] % 4 == 0 and cdiv(C, 4) * 4 <= ldP
    return npad, 4 * npad * 8 > 48 * 1024, vec4, sum_split(C)


def dispatch(entry, case):
    if entry == "K7":
        return ("ccn", case["rows"])                       # k_rows.hip:431-440: one kernel, one workgroup per row
    if entry == "K7G":
        return ("gathered", case["G"])                     # k_rows.hip:442-480: one kernel per mode
    return {"K1": _dispatch_k1, "K1A": _dispatch_k1a, "K2": _dispatch_k2, "K4": _dispatch_k4, "K5": _dispatch_k5,
            "K8": _dispatch_k8}[entry](case)


# =========================================================================================================================
# 2. cases
# =========================================================================================================================
def _pick(rng, xs):
    return xs[int(rng.integers(len(xs)))]


def _k1_cases(rng):
    out = []

    def add(N, C, D, ldi=None, ldt=None, ldp=None, off=0, **kw):
        out.append(dict(N=N, C=C, D=D, ldi=ldi or D, ldt=ldt or D, ldp=ldp or C, off=off, **kw))

    for D in K1_D:                                     # the forms by D: dma / plain, KBLOCKS on / off
        add(130, 140, D)
        add(37, 50, D, ldi=D + 1, ldt=D + 3)           # unaligned pitches: f32<unaligned>
    for D in (64, 512):                                # dma<plain>: 128 * ldp * 4 >= 2^31, two rows so that the frame stays 16 MB
        add(2, 130, D, ldp=(1 << 22) + 4)
    add(130, 140, 64, off=1)                           # an unaligned base alone
    for N in K1_N:                                     # row tiles per band x column tiles; 1025 and 2100 leave a ragged row tile
        for C in K1_C:
            add(N, C, 32 if N > 1024 else 64, ldp=C + 4 * int(rng.integers(0, 3)))
    add(2100, 129, 512)                                # the KBLOCKS dma form past the first band
    for _ in range(4):
        D = int(_pick(rng, K1_D))
        add(int(rng.integers(1, 400)), int(rng.integers(1, 300)), D, ldi=D + int(rng.integers(0, 4)))
    return out


def _k1a_cases(rng):
    out = []
    for i, d in enumerate(K1A_D + (5, 2049)):
        for j in range(2):
            n = 8 + (2 * i + j) % 8 + 8 * int(rng.integers(0, 3))
            out.append(dict(n=n, d=d, ldx=d + (0, 1, 4)[(i + j) % 3], ldy=d + (0, 3, 8)[(i + 2 * j) % 3], in_place=(i + j) % 4 == 3))
    for r in range(8):
        out.append(dict(n=r + 1, d=int(_pick(rng, (7, 64, 130, 520))), ldx=0, ldy=0, in_place=r % 2 == 0))
    for c in out:
        c["ldx"], c["ldy"] = c["ldx"] or c["d"], c["ldy"] or c["d"]
        if c["in_place"]:
            c["ldy"] = c["ldx"]
    return out


def _k2_cases(rng):
    out = []

    def add(N, C, pad_to, ldp=None, off=0, **kw):
        lds = cdiv(C, pad_to) * pad_to if pad_to else C
        out.append(dict(N=N, C=C, a=float(_pick(rng, (10.0, 2.0))), pad_to=pad_to, ldp=ldp or C, lds=lds, off=off, **kw))

    ns = (16, 1, 15, 33)
    for i, C in enumerate(K2_C):
        add(ns[i % 3], C, 192 if i % 2 == 0 else None)
    add(33, 16, 320)                                   # 16 concepts at a pitch past 256: the shortest row of the LDS form ...
    add(33, 16, 320, ldp=17)                           # ... with vec4 on and off
    add(17, 8, 1024)                                   # C < 16 at a wide pitch: the register form
    add(31, 200, None)                                 # lds <= 256 with C >= 16
    for C in (255, 256, 763, 1024, 1025, 4099, 16384):              # the LDS forms with vec4 on and off
        add(int(_pick(rng, ns)), C, 192, ldp=cdiv(C, 4) * 4)        # on (lds % 192 == 0)
        add(int(_pick(rng, ns)), C, 192, ldp=cdiv(C, 4) * 4 + 1)    # off by the pitch
    add(16, 763, 192, ldp=764, off=1)                  # off by the base
    add(15, 16385, 192)
    add(3, 5, 192, nan=True)                           # regression: the register form wrote 0 * (1 / NaN) into the padding of a NaN row,
    add(3, 40, 192, nan=True)                          # on both of its paths (C < 16 and the rows held in registers)
    for _ in range(4):
        add(int(rng.integers(1, 40)), int(rng.integers(1, 1500)), _pick(rng, (192, None)))
    return out


def _k4_cases(rng):
    out = []
    combos = ((1, 1), (0, 0), (1, 0), (0, 1))          # (soft, trusted)

    def add(N, C, U, K, ldS=None, off=0, combo=None, **kw):
        soft, trusted = combo if combo is not None else combos[len(out) % 4]
        out.append(dict(N=N, C=C, U=U, K=K, ldS=ldS or cdiv(C, 96) * 96, off=off, soft=soft, trusted=trusted, **kw))

    for C in K4_SLICED_C:                              # rs_ok by split >= C / by split % 96 == 64, rs_cut; 1, 8, 9 slices
        add(50, C, 37, 8)
        add(50, C, 48, 4)
    for U in K4_U_CHECKED:                             # passes per workgroup: 96 groups in flight (checked) ...
        add(64, 96, U, 4, combo=(len(out) % 2, 0))
    for U in K4_U_TRUSTED:                             # ... 128 (trusted)
        add(64, 96, U, 4, combo=(len(out) % 2, 1))
    add(24, 96, 40, 4, combo=(1, 1), big=(K4_BIG_N, None))          # OFF32 = false: 64-bit gather offsets
    add(50, 763, 37, 8, ldS=763)                       # main + tail by ldS % 96 != 0: vec2 off ...
    add(50, 763, 37, 8, ldS=764)                       # ... and on
    add(50, 763, 37, 5, ldS=768)                       # by K % 4 != 0
    add(50, 763, 21, 7, ldS=768, off=1)                # an unaligned base: vec2 off
    for K in (256, 260, 333):                          # by K >= 256: the three-level cascade
        add(340, 96, 5, K)
    for C in K4_TAIL_C:                                # by split on no slice boundary: the tail widths
        add(40, C, 37, 8)
    for C in (1, 2, 3, 5):                             # split == 0 (C < 4): the tail kernel alone; 5: split 4
        add(40, C, 300, 4)
    for _ in range(4):
        K = int(_pick(rng, (1, 3, 4, 8, 16, 28, 100)))
        add(int(rng.integers(K, 300)), int(_pick(rng, (7, 40, 96, 130, 192, 500, 763))), int(rng.integers(1, 70)), K,
            ldS=None if rng.random() < 0.7 else int(rng.integers(0, 3)) or None)
    for c in out:
        c["ldS"] = max(c["ldS"], c["C"])
    return out


def _k5_cases(rng):
    out = []

    def add(segs, C, ld=None, ldo=None, off=0, **kw):
        out.append(dict(segs=list(segs), C=C, ld=ld or C, ldo=ldo or C, off=off, lam=float(_pick(rng, (1.0, 0.6))), **kw))

    for i, U in enumerate(K5_UMAX):                    # the routes by the largest segment, one segment
        C = K5_C[i % len(K5_C)] if U > 1000 else K5_C[(3 * i) % len(K5_C)]
        add([0, U], C)
        add([0, U], 64 if U < 1000 else 32, ld=68, ldo=64)          # whole 16-byte rows: vec_ok
    for C in K5_C:                                     # C around 16, 64 and split; odd and even panel counts
        add([0, 70], C, ld=cdiv(C, 4) * 4, ldo=cdiv(C, 4) * 4)
        add([0, 70], C, ld=C + 1)
    add([0, 70], 64, off=1)                            # vec_ok off by the base
    add([0, 40, 40, 110], 33)                          # three segments, the middle one empty
    add([5, 45, 45, 110], 20, ld=20, ldo=24)           # (a first offset that is not 0)
    add(list(range(0, 65)), 17)                        # 64 segments of one row
    add([0] + [int(v) for v in np.cumsum(rng.integers(1, 200, 64))], 40)   # 64 uneven segments, some past a 64-row chunk
    add([0, 2000, 2000, 2040, 2045], 24)               # panel <8> beside short and empty segments
    add([0, 3841, 3841, 4241, 4246], 20)               # three-pass: uneven max_super, blockIdx.z > 0 works on two segments
    add([0, 40], 20, routes=(2000, 3900))              # the same 40 rows under the three routes
    for _ in range(4):
        n = int(rng.integers(1, 5))
        add([0] + [int(v) for v in np.cumsum(rng.integers(0, 300, n))] + [int(rng.integers(1200, 1300))], int(rng.integers(1, 130)))
    return out


def _row_cases(entry, rng):
    out = []
    for i, n in enumerate(ROW_N):
        c = dict(n=n, rows=7, dead=i % 3 == 0)
        if entry == "K7":
            c.update(ldx=n + (0, 1, 4)[i % 3], ldy=n + (0, 3)[i % 2])
        else:
            c.update(G=K7G_G[i % 4], R=9, row0=i % 2, pad=int(rng.integers(0, 4)))
            cuts = sorted(int(v) for v in rng.integers(0, n + 1, c["G"] - 1))
            c["counts"] = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        out.append(c)
    if entry == "K7G":                                 # every G at a short, a middle and a long row
        for G in K7G_G:
            for n in (5, 300, 2050):
                cuts = sorted(int(v) for v in rng.integers(0, n + 1, G - 1))
                out.append(dict(n=n, rows=7, dead=G == 2, G=G, R=9, row0=1, pad=1, counts=[b - a for a, b in zip([0] + cuts, cuts + [n])]))
    return out


def _k8_cases(rng):
    out = []

    def add(top_n, C, U, n_perm, p, scale_p, ldP=None, off=0, regime="softmax"):
        N = top_n + int(rng.integers(0, 40))
        out.append(dict(N=N, C=C, U=U, top_n=top_n, n_perm=n_perm, p=p, scale_p=scale_p, ldP=ldP or C, off=off, regime=regime))

    for i, t in enumerate(K8_TOP):                     # npad and the > 48 KB branch
        C = K8_C[i % len(K8_C)] if t < 4096 else 8
        add(t, C, 1 if t >= 1024 else (1, 5)[i % 2], (5, 1)[i % 2], K8_P[i % 4], (0.5, 1.0)[i % 2], ldP=cdiv(C, 4) * 4 if i % 2 else C)
    for i, C in enumerate(K8_C):                       # the split rule, C % 4, VEC4 on (padded rows) and off (a ragged last tile)
        t = (255, 257, 1025)[i % 3] if C < 8 else int(rng.integers(6, 200))
        add(t, C, (5, 1)[i % 2], 5, K8_P[(i + 1) % 4], (1.0, 0.5)[i % 2], ldP=cdiv(C, 4) * 4, regime="cancel" if C < 8 else "softmax")
        add(t, C, 1, (1, 5)[i % 2], K8_P[(i + 2) % 4], 0.5, ldP=C + (C % 4 == 0), regime="cancel" if C < 8 else "softmax")
    add(40, 764, 2, 5, 3.0, 0.5, ldP=764, off=1)       # VEC4 off by the base alone
    for C in (5, 6, 7):                                # C % 4 in 1, 2, 3 with padded rows (VEC4) and without (the scalar kernel)
        add(int(rng.integers(6, 60)), C, 2, 5, 3.0, 0.5, regime="randn")
        add(int(rng.integers(6, 60)), C, 2, 5, 3.0, 0.5, ldP=8, regime="randn")
    for _ in range(4):
        C = int(_pick(rng, (5, 31, 64, 100, 255)))
        add(int(rng.integers(5, 150)), C, int(rng.integers(1, 6)), 5, 3.0, 0.5, ldP=cdiv(C, 4) * 4)
    return out


def cases(entry, seed):
    rng = np.random.default_rng([int(seed), 50 + ENTRIES.index(entry)])
    out = {"K1": _k1_cases, "K1A": _k1a_cases, "K2": _k2_cases, "K4": _k4_cases, "K5": _k5_cases, "K8": _k8_cases,
           "K7": lambda r: _row_cases("K7", r), "K7G": lambda r: _row_cases("K7G", r)}[entry](rng)
    for i, c in enumerate(out):
        c.setdefault("regime", REGIMES[i % len(REGIMES)])
        c.update(entry=entry, i=i, ds=int(seed) * 100003 + 977 * (50 + ENTRIES.index(entry)) + i)
    return out


def random_cases(entry, count, seed):
    """`count` cases for the command line: the stratified lists of consecutive seeds, one after the other."""
    out, s = [], int(seed)
    while len(out) < count:
        out += cases(entry, s)
        s += 1
    return out[:count]


def case_bytes(entry, c):
    """The bytes of a case's largest operands (what one call moves; the CPU test bounds their sum per entry)."""
    if entry == "K1":
        return 4 * (c["N"] * c["ldi"] + c["C"] * c["ldt"] + (c["N"] - 1) * c["ldp"] + c["C"])
    if entry == "K1A":
        return 4 * c["n"] * (c["ldx"] + c["ldy"])
    if entry == "K2":
        return 4 * c["N"] * (c["ldp"] + c["lds"])
    if entry == "K4":
        return 4 * ((c["big"][0] if c.get("big") else c["N"]) * c["ldS"] + c["U"] * (c["C"] + c["K"]))
    if entry == "K5":
        return 4 * (c["segs"][-1] + sum(c.get("routes", ()))) * (c["ld"] + c["ldo"])
    if entry in ("K7", "K7G"):
        return 8 * c.get("R", c["rows"]) * (c["n"] + 64 * 4)
    return 4 * (c["N"] * c["ldP"] + c["U"] * (c["C"] + c["top_n"] * (2 + c["n_perm"])))


def strata(entry, case_list):
    """The dispatch classes and shape strata a case list covers, as a set of tuples (the CPU test spells out the needed set)."""
    s = set()
    for c in case_list:
        d = dispatch(entry, c)
        if entry == "K1":
            form, kb, tiles, bands, ncol = d
            s |= {("form", form, kb), ("tiles", tiles, ncol), ("D", c["D"])}
            s |= {(n,) for n, on in (("ragged row tile", c["N"] % 128 != 0 and tiles > 1), ("ragged column tile", c["C"] % 128 != 0),
                                     ("ldp > C", c["ldp"] > c["C"]), ("N < 128", c["N"] < 128), ("band 1", bands > 1)) if on}
        elif entry == "K1A":
            s |= {("NV", d[0], d[1]), ("n % 8", c["n"] % 8)}
            s |= {(n,) for n, on in (("ldx", c["ldx"] > c["d"]), ("ldy", c["ldy"] > c["d"]), ("in place", c["in_place"])) if on}
        elif entry == "K2":
            s |= {("form", d[0], d[1], c["C"]), ("pad_to", c["pad_to"]), ("N % 16", c["N"] % 16)}
            if c.get("nan"):
                s.add(("regression: a NaN row keeps its +0 padding", d[0], c["C"] < 16))
            if d[0] == "reg<16>":
                s.add(("reg by", "lds" if c["lds"] <= 256 and c["C"] >= 16 else "C < 16 wide" if c["lds"] > 256 else "both"))
        elif entry == "K4":
            s |= {("soft", c["soft"]), ("trusted", c["trusted"]), ("route", d[0])}
            if d[0] == "slice":
                _, rs, n_slices, off32, tr, passes, last, gl = d
                s |= {("rs", rs, c["C"]), ("n_slices", n_slices), ("OFF32", off32), ("form", c["soft"], tr)}
                if c["U"] >= 1536:
                    s.add(("passes", tr, passes, last, c["U"]))
                if c["U"] % 16:
                    s.add(("U % 16",))
                if gl is not None:
                    s.add(("slice + tail", gl))
            else:
                s |= {("cause", n) for n in d[1]} | {("vec2", d[2])}
                if d[3] is not None:
                    s.add(("tail", c["C"] - min(sum_split(c["C"]), c["C"]), d[3]))
                if c["K"] >= 256:
                    s.add(("K", c["K"]))
        elif entry == "K5":
            rows, live = [b - a for a, b in zip(c["segs"][:-1], c["segs"][1:])], k5_live(c["segs"])
            s |= {("route", d[0], d[1]), ("C", c["C"])}
            if len(live) == 1:
                s.add(("Umax", max(live)))
            if d[0] == "panel":
                s |= {("vec_ok", d[1], d[2]), ("n_panels", d[3] % 2)}
            s.add(("segments", 1 if len(rows) == 1 else 64 if len(rows) == 64 else "empty middle" if 0 in rows[1:-1] else "some"))
            if "routes" in c:
                s.add(("the same rows under three routes",))
        elif entry in ("K7", "K7G"):
            s.add(("n", c["n"]))
            s |= {("dead rows",)} if c["dead"] else set()
            if entry == "K7G":
                s |= {("G", c["G"])} | ({("empty piece",)} if 0 in c["counts"] else set())
        elif entry == "K8":
            npad, big_lds, vec4, split = d
            s |= {("top_n", c["top_n"], npad, big_lds), ("VEC4", vec4, c["C"] % 4), ("C", c["C"], split), ("n_perm", c["n_perm"]),
                  ("p", c["p"]), ("scale_p", c["scale_p"]), ("U", c["U"])}
            s |= {("ragged tile, scalar",)} if not vec4 and c["C"] % 4 else set()
            s |= {("one NaN",)} if c["i"] % 4 == 0 else set()
        s.add(("regime", c["regime"]))
        if c.get("big"):
            s.add(("big",))
    return s


# =========================================================================================================================
# 3. operands and references
# =========================================================================================================================
def _gen(case, salt=0):
    return torch.Generator().manual_seed(case["ds"] * 16 + salt)


def _regime(x, r):
    return {"unit": x, "x30": x * 30.0, "x1e-3": x * 1e-3, "off100": x + 100.0}[r]


def _t(a, dev):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def lse_ref64(x, segs, lam):
    """K5's formula (mcd_hip.h) in float64, per segment: out = x - lam (logsumexp_u x - log U), the maximum taken out first and
    an infinite maximum replaced by 0 (ATen's masked_fill)."""
    out = torch.empty_like(x, dtype=torch.float64)
    for a, b in zip(segs[:-1], segs[1:]):
        if b > a:
            v = x[a:b].double()
            m = v.max(dim=0, keepdim=True).values
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            out[a:b] = v - lam * (torch.log(torch.exp(v - m).sum(dim=0, keepdim=True)) + m - float(np.log(float(b - a))))
    return out


def softmax_ref64(P, a):
    """K2's formula in float64: exp(a P - max) over its row sum."""
    z = P.double() * a
    e = torch.exp(z - z.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def wpmi_ref64(S, idx, p, min_prob, soft):
    """K4's formula (mcd_hip.h): the fp32 terms w_j as the header defines them, their logs and the sum in float64."""
    g = S.float()[idx.long()]                                               # [U, K, C]
    mp = torch.tensor(min_prob, dtype=torch.float32)
    w = (1.0 + p.float()[None, :, None] * (g - 1.0)) + mp if soft else g + mp      # the terms: fp32, every operation rounded
    return torch.log(w.double()).sum(dim=1)


def ccn_ref64(x, min_norm):
    d = x.double() - x.double().mean(dim=1, keepdim=True)
    c = d ** 3
    return c / c.norm(dim=1, keepdim=True).clamp_min(min_norm)


def rank_reorder_ref64(P, tvals, tidx, perms, p, scale_p):
    """rank_reorder as the reference file writes it (similarity.py:107-132), in float64 torch on given top lists."""
    P, tv = P.double(), tvals.double()
    U, top_n = tv.shape
    out = torch.empty(U, P.shape[1], dtype=torch.float64)
    for u in range(U):
        G = P[tidx[u].long()]
        avg = G.mean(dim=0, keepdim=True)
        rank = torch.argsort(torch.argsort(G, dim=0), dim=0)
        t = tv[u][:, None]
        st = t.flip(0)
        base = (st - torch.cat([st[perms[u, k].long()] for k in range(perms.shape[1])], dim=1)).abs().pow(p).mean()
        err = (t - st[:, 0][rank]).abs().pow(p).mean(dim=0, keepdim=True) / base
        out[u] = -(err / avg.pow(scale_p))[0]
    return out


def k4_operands(case):
    """S [N, C] (softmax rows: true probabilities; the checked form also gets entries of exactly 0 and 1), idx [U, K], p [K]."""
    g = _gen(case)
    N, C, U, K = case["N"], case["C"], case["U"], case["K"]
    z = _regime(torch.randn(N, C, generator=g) * 0.3, case["regime"] if case["regime"] != "off100" else "unit")
    S = torch.from_numpy(O.row_softmax(_np(z), 10.0 if case["soft"] else 2.0))
    if not case["trusted"]:
        hit = torch.rand(N, C, generator=g)
        S = torch.where(hit < 0.02, torch.zeros_like(S), torch.where(hit > 0.98, torch.ones_like(S), S))
    idx = torch.randint(0, N, (U, K), generator=g, dtype=torch.int32)
    p = torch.from_numpy(O.p_in_examples(K)) if case["soft"] else None
    rows = None
    if case.get("big"):                                # rows on both sides of byte offset 2^32, the last row among them
        n_big, ld = case["big"][0], case["ldS"]
        edge = (1 << 32) // (4 * ld)
        rows = [0, 1, edge - 1, edge, edge + 1, n_big - 1]
        for v in torch.randint(2, n_big - 1, (4 * N,), generator=g).tolist():
            if len(rows) < N and v not in rows:
                rows.append(v)
    return S, idx, p, rows


def k5_operands(case, rows=None, salt=0):
    g = _gen(case, salt)
    U, C, r = rows or case["segs"][-1], case["C"], case["regime"]
    x = torch.randn(U, C, generator=g) * {"unit": 3.0, "x30": 30.0, "x1e-3": 1e-3, "off100": 3.0}[r] + (100.0 if r == "off100" else -400.0)
    if case["i"] % 5 == 1 and C > 2 and not salt:      # a column of -inf, and one +inf: logsumexp's masked_fill branch
        x[:, 1] = float("-inf")
        x[int(torch.randint(0, U, (1,), generator=g)), 2] = float("inf")
    return x


def k8_operands(case):
    """P, tvals / tidx (descending activations, distinct images), perms; no exact tie in a gathered column (torch.argsort's order
    among ties is unstable, and so is the reference's): a draw with one is rejected, and check() verifies what it got."""
    N, C, U, top_n = case["N"], case["C"], case["U"], case["top_n"]
    for salt in range(8):
        g = _gen(case, 100 + salt)
        if case["regime"] == "randn":
            P = torch.randn(N, C, generator=g)
        else:
            P = torch.softmax(4 * torch.randn(N, C, generator=g), dim=1) if C >= 8 else torch.rand(N, C, generator=g) + 0.05
        tidx = torch.stack([torch.randperm(N, generator=g)[:top_n] for _ in range(U)]).int()
        if case["regime"] == "cancel":                 # similarities of both signs whose column sums cancel to 1e-4 of their terms
            h = torch.randn(top_n // 2, C, generator=g)
            G = torch.cat([h, -h, torch.rand(top_n % 2, C, generator=g) * 1e-3])[torch.randperm(top_n, generator=g)] + 1e-4
            P = torch.randn(N, C, generator=g)
            P[tidx[0].long()] = G                      # every neuron: the same images in an order of its own
            tidx = torch.stack([tidx[0][torch.randperm(top_n, generator=g)] for _ in range(U)])
        tvals = torch.sort(torch.randn(U, top_n, generator=g), dim=1, descending=True).values
        perms = torch.stack([torch.stack([torch.randperm(top_n, generator=g) for _ in range(case["n_perm"])]) for _ in range(U)]).int()
        if all(len(np.unique(_np(P[tidx[u].long()][:, c]))) == top_n for u in range(U) for c in range(C)):
            return P, tvals, tidx, perms
    raise AssertionError("no tie-free draw")


# =========================================================================================================================
# 4. the checker
# =========================================================================================================================
def _nan_mask(ck, what, got, ref):
    if not torch.equal(torch.isnan(got).cpu(), torch.isnan(ref).cpu()):
        ck.note("%s: the NaN mask differs from the reference's" % what)


def _both_fills(ck, run, out):
    ck.same("guards of 1e30 for NaN", run(gap=GAPS[1]), out)


def _check_k1a(ck, case, call, dev):
    n, d = case["n"], case["d"]
    x = _regime(torch.randn(n, d, generator=_gen(case)), case["regime"]).to(dev)
    run = lambda xx, gap=NAN: call("K1A", gap=gap, x=xx, ldx=case["ldx"], ldy=case["ldy"], in_place=case["in_place"])
    out = run(x)
    ck.same("the oracle's bits", out, _t(O.normalize_rows(_np(x)), dev))
    _both_fills(ck, lambda gap: run(x, gap), out)
    ck.same("not in place" if case["in_place"] else "in place",
            call("K1A", gap=NAN, x=x, ldx=case["ldx"], ldy=case["ldx"], in_place=not case["in_place"]), out)
    for r in sorted({0, n - 1}):
        ck.same("row %d alone" % r, run(x[r:r + 1].contiguous()), out[r:r + 1])
    ck.same("the batch reversed", run(x.flip(0).contiguous()), out.flip(0))
    if case["i"] % 4 == 0:
        bad = x.clone()
        bad[n // 2, d // 2] = NAN
        _nan_mask(ck, "one NaN", run(bad), _t(O.normalize_rows(_np(bad)), dev))


def _check_k1(ck, case, call, dev):
    N, C, D = case["N"], case["C"], case["D"]
    g = _gen(case)
    I = _regime(torch.randn(N, D, generator=g), case["regime"]).to(dev)
    T = torch.randn(C, D, generator=g).to(dev)
    run = lambda ii, tt, gap=NAN: call("K1", gap=gap, I=ii.contiguous(), T=tt.contiguous(), ldi=case["ldi"], ldt=case["ldt"],
                                       ldp=case["ldp"], off=case["off"])
    out = run(I, T)
    ck.same("the oracle's bits", out, OPS.embed_gemm(I, T).to(dev))
    _both_fills(ck, lambda gap: run(I, T, gap), out)
    for r in sorted({0, N - 1}):
        ck.same("row %d alone" % r, run(I[r:r + 1], T), out[r:r + 1])
    r0 = 128 * ((N - 1) // 128)                        # the last row tile alone: what a band-mapping error moves
    if r0:
        ck.same("rows %d.. alone" % r0, run(I[r0:], T), out[r0:])
    if N > 1024:
        ck.same("rows 1024..1151 alone", run(I[1024:1152], T), out[1024:1152])
    ck.same("the batch reversed", run(I.flip(0), T), out.flip(0))
    perm = torch.randperm(C, generator=g).to(dev)
    ck.same("T's rows permuted", run(I, T[perm]), out[:, perm])
    if case["i"] % 4 == 0:
        bad = I.clone()
        bad[N - 1, D // 2] = NAN
        _nan_mask(ck, "one NaN", run(bad, T), OPS.embed_gemm(bad, T))


def _check_k2(ck, case, call, dev):
    N, C, a = case["N"], case["C"], case["a"]
    P = _regime(torch.randn(N, C, generator=_gen(case)) * 0.05, case["regime"]).to(dev)
    run = lambda pp, gap=NAN, **kw: call("K2", gap=gap, P=pp.contiguous(), a=a, **{**dict(ldp=case["ldp"], lds=case["lds"], off=case["off"]), **kw})
    out = run(P)
    ck.same("the oracle's bits", out, _t(O.row_softmax(_np(P), a), dev))
    _both_fills(ck, lambda gap: run(P, gap), out)
    form = dispatch("K2", case)[0]                     # the other pitch / alignment of the same form: vec4 on against off
    if form.startswith("lds"):
        ck.same("vec4 on", run(P, ldp=cdiv(C, 4) * 4, off=0), out)
        ck.same("vec4 off by the pitch", run(P, ldp=cdiv(C, 4) * 4 + 1, off=0), out)
        ck.same("vec4 off by the base", run(P, ldp=cdiv(C, 4) * 4 + 4, off=1), out)
    for r in sorted({0, N - 1}):
        ck.same("row %d alone" % r, run(P[r:r + 1]), out[r:r + 1])
    ck.same("the batch reversed", run(P.flip(0)), out.flip(0))
    if case["i"] % 4 == 0 or case.get("nan"):
        bad = P.clone()
        bad[N // 2, C - 1] = NAN
        _nan_mask(ck, "one NaN", run(bad), _t(O.row_softmax(_np(bad), a), dev))


def k4_rule(out, ref):
    """scripts/fuzz_core.py's rule: (the largest deviation, its tolerance 1.3e-4 max(1, |ref|max / 512), the bit-equal share)."""
    d = (out.double() - ref.double()).abs()
    d = torch.where(torch.isnan(d), torch.zeros_like(d), d)
    top = float(ref[torch.isfinite(ref)].abs().max()) if bool(torch.isfinite(ref).any()) else 0.0
    return float(d.max()), 1.3e-4 * max(1.0, top / 512.0), float((d == 0).double().mean())


def _check_k4(ck, case, call, dev):
    S, idx, p, rows = k4_operands(case)
    S, idx, p = S.to(dev), idx.to(dev), None if p is None else p.to(dev)
    U, soft = case["U"], case["soft"]
    big = (case["big"][0], rows) if rows else None
    kw = dict(min_prob=MIN_PROB, soft=soft, ldS=case["ldS"], off=case["off"])
    run = lambda ss, ii, gap=NAN, trusted=case["trusted"], bg=None: call("K4", gap=gap, S=ss, idx=ii.contiguous(), p=p, trusted=trusted, big=bg, **kw)
    small = run(S, idx)
    ref = OPS.wpmi_score(S, idx, p, np.float32(MIN_PROB), soft).to(dev)
    err, tol, exact = k4_rule(small, ref)
    ck.acc("the oracle", err, tol)
    if exact < 0.995:
        ck.note("only %.5f of the entries equal the oracle's bits" % exact)
    out = small
    if big:                                            # the same rows at their places in the large matrix: 64-bit offsets
        out = run(S, idx, bg=big)
        ck.same("the rows compacted", out, small)
        return
    _both_fills(ck, lambda gap: run(S, idx, gap), out)
    if case["trusted"]:
        ck.same("trusted == checked", run(S, idx, trusted=0), out)
    d = dispatch("K4", case)
    wg = 16 * (128 if d[0] == "slice" and d[4] else 96)
    for u in sorted({0, U - 1, min(U - 1, wg), min(U - 1, wg + 17)}):      # (a neuron of the second persistent pass among them)
        ck.same("neuron %d alone" % u, run(S, idx[u:u + 1]), out[u:u + 1])
    ck.same("the neurons reversed", run(S, idx.flip(0)), out.flip(0))
    if case["i"] % 4 == 0:
        bad = S.clone()
        bad[int(idx[U // 2, 0]), case["C"] // 2] = NAN
        _nan_mask(ck, "one NaN", run(bad, idx), OPS.wpmi_score(bad, idx, p, np.float32(MIN_PROB), soft))


def k5_rule(ck, what, out, ref, x, C):
    """scripts/fuzz_core.py's rule: K4's tolerance on the finite entries, at most max(1, C // 200) columns that differ at all;
    what is not finite must be the same value."""
    fin = torch.isfinite(ref)
    if not torch.equal(torch.where(fin, torch.zeros_like(out), out).nan_to_num(nan=7.0), torch.where(fin, torch.zeros_like(ref), ref).nan_to_num(nan=7.0)) \
            or not bool(torch.isfinite(out)[fin].all()):
        ck.note("%s: the non-finite entries differ from the reference's" % what)
        return
    d = torch.where(fin, (out.double() - ref.double()).abs(), torch.zeros_like(out, dtype=torch.float64))
    xf = x[torch.isfinite(x)]
    ck.acc(what, d.max(), 1.3e-4 * max(1.0, float(xf.abs().max()) / 512.0))
    cols = int((d.max(dim=0).values > 0).sum())
    if cols > max(1, C // 200):
        ck.note("%s: %d columns differ (cap %d)" % (what, cols, max(1, C // 200)))


def _check_k5(ck, case, call, dev):
    segs, C, lam = case["segs"], case["C"], case["lam"]
    x = torch.cat([torch.zeros(segs[0], C), k5_operands(case)[segs[0]:]]).to(dev)
    run = lambda xx, ss, gap=NAN: call("K5", gap=gap, x=xx.contiguous(), segs=list(ss), lam=lam, ld=case["ld"], ldo=case["ldo"], off=case["off"])
    full = run(x, segs)
    out, xs = full[segs[0]:], x[segs[0]:]
    k5_rule(ck, "the oracle", out, OPS.logsumexp_sub(x, lam, segs).to(dev), xs, C)
    ck.same("guards of 1e30 for NaN", run(x, segs, GAPS[1])[segs[0]:], out)
    live = [(a, b) for a, b in zip(segs[:-1], segs[1:]) if b > a]
    for a, b in live[:2] + live[-2:] if len(live) > 1 else []:
        ck.same("segment %d..%d alone" % (a, b), run(x[a:b], [0, b - a]), full[a:b])
    if len(live) > 1:                                  # the segments in reverse order (the rows of one keep theirs)
        rev = torch.cat([x[a:b] for a, b in reversed(live)])
        offs = [0] + [int(v) for v in np.cumsum([b - a for a, b in reversed(live)])]
        ck.same("the segments reversed", run(rev, offs), torch.cat([full[a:b] for a, b in reversed(live)]))
    for extra in case.get("routes", ()):               # the same rows beside a segment that moves the call to another route
        y = k5_operands(case, extra, salt=extra).to(dev)
        ck.same("beside a %d-row segment" % extra, run(torch.cat([x, y]), [0, segs[-1], segs[-1] + extra])[:segs[-1]], full)
    if case["i"] % 4 == 0:
        bad = x.clone()
        bad[(live[-1][0] + live[-1][1]) // 2, C // 2] = NAN
        got, want = run(bad, segs)[segs[0]:], OPS.logsumexp_sub(bad, lam, segs)
        _nan_mask(ck, "one NaN", got, want)


def _aten_rule(ck, what, out, ref, aten):
    """conv_fuzz's general rule (test_gpu_resnet._bound): nerr <= 2 nerr(ATen fp32) + 1e-6."""
    top = float(ref.abs().max().clamp_min(1e-30))
    ck.acc(what, float((out.double().cpu() - ref).abs().max()) / top, 2 * float((aten.double().cpu() - ref).abs().max()) / top + 1e-6)


def row_operands(case, rows):
    x = _regime(torch.randn(rows, case["n"], generator=_gen(case)) * 3 + 0.5, case["regime"] if case["regime"] != "off100" else "unit")
    if case["dead"]:
        x[1] = 0.0                                     # an all-zero row, and a constant one: centred to zero, the min_norm clamp
        x[2] = 0.75
    return x


def _ccn32(x, min_norm):
    d = x - x.mean(dim=1, keepdim=True)
    c = d * d * d
    return c / c.norm(dim=1, keepdim=True).clamp_min(min_norm)


def _check_k7(ck, case, call, dev):
    rows, n = case["rows"], case["n"]
    x = row_operands(case, rows).to(dev)
    run = lambda xx, gap=NAN: call("K7", gap=gap, x=xx.contiguous(), min_norm=1e-3, ldx=case["ldx"], ldy=case["ldy"])
    out = run(x)
    _aten_rule(ck, "float64", out, ccn_ref64(x.cpu(), 1e-3), _ccn32(x, 1e-3))
    cos = out[:3].double().cpu() @ out[3:].double().cpu().T            # cos_similarity_cubed of 3 neurons and 4 concepts at 5e-7
    ck.acc("cos_similarity_cubed", np.abs(cos.numpy() - O.cos_similarity_cubed(_np(x[3:]).T, _np(x[:3]).T).astype(np.float64)).max(), 5e-7)
    _both_fills(ck, lambda gap: run(x, gap), out)
    for r in (0, 1, rows - 1):
        ck.same("row %d alone" % r, run(x[r:r + 1]), out[r:r + 1])
    ck.same("the batch reversed", run(x.flip(0)), out.flip(0))
    if case["i"] % 4 == 0:
        bad = x.clone()
        bad[3, n // 2] = NAN
        _nan_mask(ck, "one NaN", run(bad), ccn_ref64(bad.cpu(), 1e-3))


def _check_k7g(ck, case, call, dev):
    R, n, row0 = case["R"], case["n"], case["row0"]
    row1 = row0 + case["rows"]
    x = row_operands(case, R).to(dev)
    cuts = np.cumsum([0] + case["counts"])
    pieces = [x[:, a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]
    want = x[row0:row1].contiguous()
    for mode, twin in (("normalize", "K1A"), ("center_cube", "K7")):
        run = lambda pp, gap=NAN: call("K7G", gap=gap, pieces=pp, rows=(row0, row1), mode=mode, min_norm=1e-3, pad=case["pad"])
        out = run(pieces)
        if mode == "normalize":
            ck.same("the oracle's bits", out, _t(O.normalize_rows(_np(want)), dev))
            ck.same("K1A on the concatenated rows", out, call("K1A", gap=NAN, x=want, ldx=n, ldy=n, in_place=False))
        else:
            ck.same("K7 on the concatenated rows", out, call("K7", gap=NAN, x=want, min_norm=1e-3, ldx=n, ldy=n))
        _both_fills(ck, lambda gap: run(pieces, gap), out)
        ck.same("%s: one piece" % mode, call("K7G", gap=NAN, pieces=[x], rows=(row0, row1), mode=mode, min_norm=1e-3, pad=case["pad"]), out)
        ck.same("%s: the rows reversed" % mode, call("K7G", gap=NAN, pieces=[q.flip(0).contiguous() for q in pieces], rows=(R - row1, R - row0),
                                                    mode=mode, min_norm=1e-3, pad=case["pad"]), out.flip(0))
        if case["i"] % 4 == 0:
            bad = x.clone()
            bad[row0 + 3, n // 2] = NAN
            ref = OPS.prepare_rows_gathered([bad.cpu()], (row0, row1), mode)
            _nan_mask(ck, "%s: one NaN" % mode, run([bad[:, a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]), ref)


def k8_rule(ck, what, got, ref):
    """scripts/fuzz_sim.py's rule: the oracle's NaN mask, and 5e-6 relative (+ 1e-9) elsewhere."""
    got, ref = got.double().cpu(), ref.double().cpu()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return ck.note("%s: the NaN mask differs from the reference's" % what)
    inf = torch.isinf(ref)                             # (a baseline of 0 -- a permutation that moves nothing -- divides by it)
    if not torch.equal(got[inf], ref[inf]):
        return ck.note("%s: an infinite entry of the reference is another value" % what)
    m = torch.isfinite(ref)
    if bool(m.any()):
        ck.acc(what, float(((got[m] - ref[m]).abs() / (5e-6 * ref[m].abs() + 1e-9)).max()), 1.0)


def _check_k8(ck, case, call, dev):
    P, tvals, tidx, perms = k8_operands(case)
    U, C = case["U"], case["C"]
    if case["i"] % 4 == 0:                             # a single NaN in a gathered row: that column of that neuron, nothing else
        P[int(tidx[0, case["top_n"] // 2]), C // 2] = NAN
    for u in range(U):
        G = _np(P[tidx[u].long()])
        if any(len(np.unique(G[:, c][~np.isnan(G[:, c])])) + int(np.isnan(G[:, c]).sum()) != G.shape[0] for c in range(C)):
            ck.note("generator: a tie in a gathered column")
    P, tvals, tidx, perms = (t.to(dev) for t in (P, tvals, tidx, perms))
    kw = dict(ldP=case["ldP"], off=case["off"], p=case["p"], scale_p=case["scale_p"])
    run = lambda tv, ti, pm, gap=NAN: call("K8", gap=gap, P=P, tvals=tv.contiguous(), tidx=ti.contiguous(), perms=pm.contiguous(), **kw)
    out = run(tvals, tidx, perms)
    k8_rule(ck, "the oracle", out, OPS.rank_reorder(P, tvals, tidx, perms, case["p"], case["scale_p"]))
    _both_fills(ck, lambda gap: run(tvals, tidx, perms, gap), out)
    for u in sorted({0, U - 1}):
        ck.same("neuron %d alone" % u, run(tvals[u:u + 1], tidx[u:u + 1], perms[u:u + 1]), out[u:u + 1])
    ck.same("the neurons reversed", run(tvals.flip(0), tidx.flip(0), perms.flip(0)), out.flip(0))


_CHECKS = {"K1A": _check_k1a, "K1": _check_k1, "K2": _check_k2, "K4": _check_k4, "K5": _check_k5, "K7": _check_k7, "K7G": _check_k7g,
           "K8": _check_k8}


def check(entry, case, call, device="cpu"):
    """(findings, the largest err / bound of the case's accuracy checks -- 0.0 for an entry that is held to bits alone)."""
    ck = _Ck(entry, case)
    try:
        _CHECKS[entry](ck, case, call, device)
    except AssertionError as e:                        # a frame that did not come back intact, an entry that returned an error
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
        if any("illegal memory access" in x for x in f):           # a faulted device: nothing more is launched on it
            break
    return findings, top


# =========================================================================================================================
# 5. the library behind call(): every operand in a frame (GPU only; nothing above needs it)
# =========================================================================================================================
def gpu_call(L):
    """call(name, gap, ...) on libmcd_hip.so: every matrix through util.FramedIn / FramedOut at the case's pitch and base offset,
    `gap` in the guards and between the rows (a valid row in the gaps of an index matrix).  The guards must come back intact,
    every logical element written, the inputs unchanged (AssertionError otherwise: check() reports it)."""
    import ctypes
    import test_gpu_encoder_frames as EF
    import util

    def fin(t, pitch, off, gap):
        return util.FramedIn(t if t.dim() == 2 else t.reshape(1, -1), pitch, off, gap)

    def fout(rows, width, pitch, dev, zero_pad=False):
        o = util.FramedOut(rows, width, pitch, 0, torch.float32, dev, tail=pitch - width if zero_pad else 0)
        if zero_pad:
            o.check = lambda e, what="", _c=o.check: _c(e, zero_pad=True, what=what)
        return o

    def call(name, gap=NAN, **a):
        st = EF.st()
        if name in ("K1A", "K7"):
            x = a["x"]
            n, d = x.shape
            entry = (lambda xp, ldx, yp, ldy: L.mcd_normalize_rows(xp, ldx, n, d, yp, ldy, st)) if name == "K1A" else \
                (lambda xp, ldx, yp, ldy: L.mcd_center_cube_normalize_rows(xp, ldx, n, d, a["min_norm"], yp, ldy, st))
            if a.get("in_place"):
                y_ = fin(x, a["ldx"], 0, gap)
                EF.ok(entry(y_.ptr, a["ldx"], y_.ptr, a["ldx"]), L)
                out = y_.view.clone()
                util.check_frame(y_.flat, y_.spec, out, what=name + " in place")
                return out
            x_, o_ = fin(x, a["ldx"], 0, gap), fout(n, d, a["ldy"], x.device)
            EF.ok(entry(x_.ptr, a["ldx"], o_.ptr, a["ldy"]), L)
            return _finish(name, o_, (x_,))
        if name == "K1":
            I, T = a["I"], a["T"]
            (N, D), C = I.shape, T.shape[0]
            i_, t_, o_ = fin(I, a["ldi"], a["off"], gap), fin(T, a["ldt"], a["off"], gap), fout(N, C, a["ldp"], I.device)
            EF.ok(L.mcd_embed_gemm(i_.ptr, a["ldi"], t_.ptr, a["ldt"], N, C, D, 0, o_.ptr, a["ldp"], None, 0, st), L)
            return _finish(name, o_, (i_, t_))
        if name == "K2":
            P = a["P"]
            N, C = P.shape
            p_, o_ = fin(P, a["ldp"], a["off"], gap), fout(N, C, a["lds"], P.device, zero_pad=True)
            EF.ok(L.mcd_row_softmax(p_.ptr, a["ldp"], N, C, a["a"], o_.ptr, a["lds"], st), L)
            return _finish(name, o_, (p_,))
        if name == "K4":
            S, idx, p = a["S"], a["idx"], a["p"]
            (N, C), (U, K) = S.shape, idx.shape
            flags = (1 if a["soft"] else 0) | (4 if a["trusted"] else 0)
            i_ = fin(idx, K, 0, 0)
            p_ = None if p is None else fin(p, K, 0, gap)
            o_ = fout(U, C, C, S.device)
            if a["big"]:                               # torch.empty: only the gathered rows are written
                n_big, rows = a["big"]
                ld = a["ldS"]
                flat = torch.empty(n_big * ld, device=S.device)
                rows_t = torch.tensor(rows, device=S.device)
                flat.view(n_big, ld)[rows_t, :C] = S
                i_ = fin(rows_t[idx.long()].int(), K, 0, 0)
                EF.ok(L.mcd_wpmi_score(flat.data_ptr(), ld, n_big, C, i_.ptr, K, U, K, _ptr(p_), a["min_prob"], flags, -1, o_.ptr, C, st), L)
                out = _finish(name, o_, (i_, p_))
                del flat
                return out
            s_ = fin(S, a["ldS"], a["off"], gap)
            EF.ok(L.mcd_wpmi_score(s_.ptr, a["ldS"], N, C, i_.ptr, K, U, K, _ptr(p_), a["min_prob"], flags, -1, o_.ptr, C, st), L)
            return _finish(name, o_, (s_, i_, p_))
        if name == "K5":
            x, segs = a["x"], a["segs"]
            U, C = x.shape
            x_, o_ = fin(x, a["ld"], a["off"], gap), fout(U, C, a["ldo"], x.device)
            o_.view[:segs[0]] = 0.0                     # rows in front of the first segment belong to no segment: not written
            for s0, s1 in zip(segs[:-1], segs[1:]):
                assert s1 >= s0
            arr = (ctypes.c_int64 * len(segs))(*segs)
            nws = int(L.mcd_logsumexp_sub_workspace(segs[-1] - segs[0], C, len(segs) - 1))
            ws = torch.empty(max(nws, 4) // 4, device=x.device)
            EF.ok(L.mcd_logsumexp_sub(x_.ptr, a["ld"], C, arr, len(segs) - 1, a["lam"], -1, o_.ptr, a["ldo"], ws.data_ptr(), nws, st), L)
            return _finish(name, o_, (x_,))
        if name == "K7G":
            pieces, (row0, row1) = a["pieces"], a["rows"]
            G, R = len(pieces), pieces[0].shape[0]
            counts = [int(q.shape[1]) for q in pieces]
            n, dev = sum(counts), pieces[0].device
            ld_src = max(max(counts) + a["pad"], 1)
            ld_block = R * ld_src + a["pad"]
            flat = torch.full((2 * util.FRAME_GUARD + G * ld_block,), gap, device=dev)
            for g_, q in enumerate(pieces):
                torch.as_strided(flat, (R, counts[g_]), (ld_src, 1), util.FRAME_GUARD + g_ * ld_block).copy_(q)
            snap = flat.clone()
            o_ = fout(row1 - row0, n, n, dev)
            arr = (ctypes.c_int64 * G)(*counts)
            EF.ok(L.mcd_prepare_rows_gathered(flat.data_ptr() + 4 * util.FRAME_GUARD, ld_src, ld_block, G, arr, n, row0, row1,
                                              0 if a["mode"] == "normalize" else 1, a["min_norm"], o_.ptr, n, st), L)
            assert torch.equal(util.int_bits(flat), util.int_bits(snap)), "the call changed an input"
            return _finish(name, o_, ())
        if name == "K8":
            P, tvals, tidx, perms = a["P"], a["tvals"], a["tidx"], a["perms"]
            (N, C), (U, top_n) = P.shape, tvals.shape
            p_ = fin(P, a["ldP"], a["off"], gap)
            tv_, ti_, pm_ = fin(tvals, top_n, 0, gap), fin(tidx, top_n, 0, 0), EF.In(perms, 0)
            base, o_ = torch.empty(U, device=P.device), fout(U, C, C, P.device)
            EF.ok(L.mcd_rank_reorder(p_.ptr, a["ldP"], N, C, tv_.ptr, ti_.ptr, top_n, U, top_n, pm_.ptr, perms.shape[1], a["p"],
                                     a["scale_p"], base.data_ptr(), o_.ptr, C, st), L)
            return _finish(name, o_, (p_, tv_, ti_, pm_))
        raise KeyError(name)

    return call
