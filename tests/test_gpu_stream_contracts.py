"""GPU: the stream and hipGraph-capture contracts of the C ABI (include/mcd_hip.h: "every call is asynchronous on `stream` ...
and is hipGraph-capturable"; include/mcd_blaslt.h adopts them, its first call per shape excepted).

Every other kernel test passes torch's current stream, which in the suite is the default stream: a launch that ignored its
`stream` argument would pass all of them.  STREAM_TABLE has a row for every prototype that takes a stream (test_exec_contract_cpu.py
checks it against the headers), the multi-launch entries once per launch sequence (the cases of test_gpu_workspace_contracts.py,
plus mcd_wpmi_score's sliced + tail pair), the single-launch entries at the smallest shape of their frame tests.  Each case:

  a. ordering on a side stream S (the default stream idle): a spin, in-place copies of fresh data into the inputs, the call,
     copies of the outputs -- all enqueued on S in that order.  The copies must be bit-equal to the eager result of the same
     entry on the fresh data: a launch on another stream runs while S still spins, on the stale inputs.  The control case calls
     mcd_layer_norm with stream NULL in the same arrangement and must NOT give the expected bits (the test can fail).
  b. capture and replay: the call captured alone into a hipGraph on S (after one eager warm-up: first-call attributes, the
     device-property query and the linear entries' plan are allowed outside a capture) returns MCD_OK and runs nothing; with
     every host array it took zeroed, two replays on new inputs and a re-poisoned workspace are bit-equal to the eager results.

The linear entries are compared at test_linear_residual_matches_torch's 2e-5 * max|ref| (ref = the eager result): hipBLASLt may
order its sums differently; everything else is compared on the bits."""
import ctypes

import pytest
import torch

import test_gpu_workspace_contracts as W
from util import OUT_FILL, int_bits

pytestmark = pytest.mark.gpu

Case = W.Case
F32 = torch.float32


def rnd(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def simple(L, dev, what, gens, out_shapes, call, host=(), inout=None, n_ins=None, out_dtypes=None):
    """A single-launch entry: gens[i](seed) -> the CPU tensor of input i; call(input pointers, output pointers, stream) -> status.
    inout {output index: gens index}: an output the entry updates in place starts as that tensor (it is not among the inputs)."""
    n_ins = len(gens) if n_ins is None else n_ins
    ins = [g(7).to(dev) for g in gens[:n_ins]]
    dts = [(out_dtypes or {}).get(j, F32) for j in range(len(out_shapes))]
    outs = [(1, numel(s), numel(s), dt, OUT_FILL if dt.is_floating_point else W.IDX_FILL, False) for s, dt in zip(out_shapes, dts)]
    return Case(what, lambda ws, nb, o, st: call([t.data_ptr() for t in ins], o, st), outs, 0, ins=ins,
                gen=lambda s: [g(s + 100 * i) for i, g in enumerate(gens)], host=host, inout=inout)


def _gen(shape, scale=1.0, shift=0.0, off=0):
    return lambda s: rnd(shape, s + off, scale, shift)


# ---- the single-launch entries, each at the first (smallest) shape of its frame test ---------------------------------------------
def b_normalize_rows(L, dev):
    n, d = 37, 5
    return simple(L, dev, "K1a", [_gen((n, d))], [(n, d)], lambda i, o, st: L.mcd_normalize_rows(i[0], d, n, d, o[0], d, st))


def b_center_cube(L, dev):
    rows, n = 9, 37
    return simple(L, dev, "K7", [_gen((rows, n))], [(rows, n)],
                  lambda i, o, st: L.mcd_center_cube_normalize_rows(i[0], n, rows, n, 1e-3, o[0], n, st))


def b_gathered(L, dev, mode):
    counts, R, row0, row1, ld_src = [40, 0, 23], 11, 2, 9, 44          # test_prepare_rows_gathered_pitches' pieces
    n, rows, ld_block = sum(counts), row1 - row0, R * ld_src + 5
    arr = (ctypes.c_int64 * 3)(*counts)
    return simple(L, dev, ("gathered", mode), [_gen((3 * ld_block,))], [(rows, n)],
                  lambda i, o, st: L.mcd_prepare_rows_gathered(i[0], ld_src, ld_block, 3, arr, n, row0, row1, mode, 1e-3, o[0], n, st),
                  host=[arr])


def b_gemm_small(L, dev, mode):
    N, C, D = 37, 50, 70                                                # one launch: no workspace at this size
    return simple(L, dev, ("K1 small", mode), [lambda s: W.unit_rows(N, D, s), lambda s: W.unit_rows(C, D, s + 1)], [(N, C)],
                  lambda i, o, st: L.mcd_embed_gemm(i[0], D, i[1], D, N, C, D, mode, o[0], C, None, 0, st))


def b_softmax(L, dev):
    N, C, lds = 37, 5, 192
    c = simple(L, dev, "K2", [_gen((N, C), 0.3)], [(N, lds)], lambda i, o, st: L.mcd_row_softmax(i[0], C, N, C, 10.0, o[0], lds, st))
    return c


def b_transpose(L, dev):
    N, U = 300, 41
    return simple(L, dev, "transpose", [_gen((N, U))], [(U, N)], lambda i, o, st: L.mcd_transpose(i[0], U, N, U, o[0], N, st))


def b_wpmi(L, dev, N, C, U, K):
    """(64, 10000, 17), K = 20: ldS = 10176 = 106 * 96 and split = 9984 = 104 * 96 -- the sliced kernel, then the tail kernel;
    (37, 40, 5), K = 5: the generic main kernel, then the tail kernel."""
    ldS = W.ceil_to(C, 192) if C > 1000 else C
    p = torch.linspace(0.998, 0.97, K).float().to(dev)

    def S(s):
        x = torch.zeros(N, ldS)
        x[:, :C] = torch.softmax(rnd((N, C), s, 3.0), dim=1)
        return x
    idx = lambda s: torch.randint(0, N, (U, K), generator=torch.Generator().manual_seed(s), dtype=torch.int32)
    return simple(L, dev, ("K4", N, C, U, K), [S, idx], [(U, C)],
                  lambda i, o, st: L.mcd_wpmi_score(i[0], ldS, N, C, i[1], K, U, K, p.data_ptr(), 1e-7, 1, -1, o[0], C, st))


def b_row_topk_short(L, dev):
    U, C, k = 9, 763, 10                                                # the wave-per-row register kernel of short rows
    return simple(L, dev, "K6 short", [_gen((U, C))], [(U, k), (U, k)], lambda i, o, st: L.mcd_row_topk(i[0], C, U, C, k, o[0], o[1], st),
                  out_dtypes={1: torch.int32})


def b_hook_pool(L, dev, nhwc):
    B, Cout, HW = 5, 70, 16
    entry = L.mcd_hook_pool_nhwc if nhwc else L.mcd_hook_pool
    return simple(L, dev, "K0n" if nhwc else "K0", [_gen((B, Cout, HW))], [(B, Cout)],
                  lambda i, o, st: entry(i[0], B, Cout, HW, 0, o[0], 0, 0, Cout, 1, st))


def b_attention(L, dev, long):
    B, T, H = 2, 1, 1
    entry = L.mcd_vit_attention_long if long else L.mcd_vit_attention
    return simple(L, dev, "K9L" if long else "K9", [_gen((B, T, 3 * H * 64))], [(B, T, H * 64)], lambda i, o, st: entry(i[0], B, T, H, o[0], st))


def b_attention_cls(L, dev):
    B, H, T = 2, 2, 1
    Wd = H * 64
    return simple(L, dev, "K9C", [_gen((B, 1, Wd)), _gen((B, T, Wd)), _gen((B, T, Wd))], [(B, Wd)],
                  lambda i, o, st: L.mcd_vit_attention_cls(i[0], Wd, i[1], Wd, T * Wd, i[2], Wd, T * Wd, B, T, H, o[0], st))


def b_layer_norm(L, dev):
    rows, D = 1, 4
    return simple(L, dev, "K10", [_gen((rows, D), 2.0, 1.0), _gen((D,)), _gen((D,))], [(rows, D)],
                  lambda i, o, st: L.mcd_layer_norm(i[0], rows, D, i[1], i[2], 1e-5, o[0], st))


def b_patchify(L, dev):
    B, Cin, H, Wd, P = 2, 1, 8, 8, 4
    return simple(L, dev, "K11", [_gen((B, Cin, H, Wd))], [(B, 1 + (H // P) * (Wd // P), Cin * P * P)],
                  lambda i, o, st: L.mcd_patchify(i[0], B, Cin, H, Wd, P, o[0], st))


def b_conv_stem(L, dev):
    B, Cin, H, Wd, Cout = 2, 1, 1, 1, 4
    return simple(L, dev, "K12", [_gen((B, Cin, H, Wd)), _gen((Cin, 3, 3, Cout), 0.3), _gen((Cout,), 0.1)], [(B, 1, 1, Cout)],
                  lambda i, o, st: L.mcd_conv_stem_nhwc(i[0], B, Cin, H, Wd, i[1], i[2], Cout, o[0], st))


def b_dwconv(L, dev):
    C, H, Wd, B, k, s = 4, 1, 1, 2, 3, 1                               # one output tile of 8 x 8 pixels per image: T = 1
    return simple(L, dev, "K13", [_gen((B, H, Wd, C)), _gen((k * k, C), 1.0 / k), _gen((C,), 0.1)], [(B, 1, 1, C), (B, 1, C)],
                  lambda i, o, st: L.mcd_dwconv_bn_silu(i[0], B, H, Wd, C, i[1], i[2], k, s, 0, o[0], o[1], 1, st))


def b_se_gate(L, dev):
    B, Tt, C, sq = 2, 1, 4, 1
    return simple(L, dev, "K14", [_gen((B, Tt, C), 3.0), _gen((sq, C), 0.5), _gen((sq,), 0.1), _gen((sq, C)), _gen((C,), 0.1)], [(B, C)],
                  lambda i, o, st: L.mcd_se_gate(i[0], B, Tt, C, 7, i[1], i[2], sq, i[3], i[4], o[0], st))


def b_channel_scale(L, dev):
    B, HW, C = 2, 1, 4                                                  # y is scaled in place: an output that starts as gens[1]
    return simple(L, dev, "K15", [_gen((B, C)), _gen((B, HW, C))], [(B, HW, C)],
                  lambda i, o, st: L.mcd_channel_scale(o[0], B, HW, C, i[0], st), inout={0: 1}, n_ins=1)


def b_conv7x7(L, dev):
    B, Cin, H, Wd, Cout = 2, 1, 1, 1, 4
    return simple(L, dev, "K16", [_gen((B, Cin, H, Wd)), _gen((Cin, 7, 7, Cout), 0.1)], [(B, 1, 1, Cout)],
                  lambda i, o, st: L.mcd_conv7x7s2_nhwc(i[0], B, Cin, H, Wd, i[1], Cout, o[0], st))


def b_maxpool(L, dev):
    B, H, Wd, C = 2, 1, 1, 4
    return simple(L, dev, "K17", [_gen((B, H, Wd, C)), _gen((C,)), _gen((C,), 0.3)], [(B, 1, 1, C)],
                  lambda i, o, st: L.mcd_bn_relu_maxpool_nhwc(i[0], B, H, Wd, C, i[1], i[2], o[0], st))


def b_igemm(L, dev, with_res):
    B, H, Wd, Cin, Cout, k, s = 1, 1, 1, 32, 32, 3, 1
    gens = [_gen((B, H, Wd, Cin)), _gen((Cout, k * k * Cin), (k * k * Cin) ** -0.5), _gen((Cout,))]
    if with_res:
        return simple(L, dev, "K18 res", gens + [_gen((B, 1, 1, Cout), 1.5)], [(B, 1, 1, Cout)],
                      lambda i, o, st: L.mcd_conv_igemm_res_nhwc(i[0], B, H, Wd, Cin, i[1], i[2], i[3], Cout, k, s, 0, 0, o[0], st))
    return simple(L, dev, "K18", gens, [(B, 1, 1, Cout)],
                  lambda i, o, st: L.mcd_conv_igemm_nhwc(i[0], B, H, Wd, Cin, i[1], i[2], Cout, k, s, 0, 0, o[0], st))


def b_conv3x3(L, dev):
    B, Cin, H, Wd, Cout = 2, 1, 1, 1, 4
    return simple(L, dev, "K19", [_gen((B, Cin, H, Wd)), _gen((Cin, 3, 3, Cout), 0.2), _gen((Cout,))], [(B, 1, 1, Cout)],
                  lambda i, o, st: L.mcd_conv3x3s2_nhwc(i[0], B, Cin, H, Wd, i[1], i[2], Cout, 0, o[0], st))


def b_avgpool(L, dev):
    B, H, Wd, C = 1, 2, 2, 4
    return simple(L, dev, "K20", [_gen((B, H, Wd, C), 3.0)], [(B, 1, 1, C)], lambda i, o, st: L.mcd_avgpool2_nhwc(i[0], B, H, Wd, C, o[0], st))


def b_attnpool(L, dev):
    B, HW, C = 2, 1, 4
    return simple(L, dev, "K21", [_gen((B, HW, C), 1.0, 0.5), _gen((HW + 1, C), 0.5)], [(B, HW + 1, C)],
                  lambda i, o, st: L.mcd_attnpool_tokens(i[0], B, HW, C, i[1], o[0], st))


def b_preprocess(L, dev):
    n, H, Wd = 2, 5, 7                                                 # no resampling tables: the crop + look-up launch alone
    img = lambda s: torch.randint(0, 256, (n, H, Wd, 3), generator=torch.Generator().manual_seed(s), dtype=torch.uint8)
    return simple(L, dev, "K22", [img, _gen((3, 256))], [(n, 3, H, Wd)],
                  lambda i, o, st: L.mcd_image_preprocess(i[0], n, H, Wd, None, 0, Wd, None, 0, H, 0, 0, H, Wd, i[1], o[0], 3 * H * Wd, st))


def _ws(builder, cases):
    return [(builder, p) for p in cases]


# entry -> [(builder, parameters)]; a builder of test_gpu_workspace_contracts takes (library, device, *parameters, top=False)
STREAM_TABLE = {
    "mcd_normalize_rows": [(b_normalize_rows, ())],
    "mcd_center_cube_normalize_rows": [(b_center_cube, ())],
    "mcd_prepare_rows_gathered": [(b_gathered, (0,)), (b_gathered, (1,))],
    "mcd_embed_gemm": [(b_gemm_small, (m,)) for m in (0, 1, 2)] + _ws(W.gemm_case, W.GEMM_CASES),
    "mcd_row_softmax": [(b_softmax, ())],
    "mcd_col_topk": _ws(W.col_topk_case, W.TOPK_CASES),
    "mcd_transpose": [(b_transpose, ())],
    "mcd_wpmi_score": [(b_wpmi, (64, 10000, 17, 20)), (b_wpmi, (37, 40, 5, 5))],
    "mcd_embed_gemm_exp": _ws(W.gexp_case, W.GEXP_CASES),
    "mcd_wpmi_score_bf16": _ws(W.wpmi_bf16_case, W.WPMI_BF16_CASES),
    "mcd_logsumexp_sub": _ws(W.lse_case, W.LSE_CASES),
    "mcd_row_topk": [(b_row_topk_short, ())] + _ws(W.row_topk_case, W.ROW_TOPK_CASES),
    "mcd_hook_pool": [(b_hook_pool, (False,))],
    "mcd_rank_reorder": _ws(W.rank_case, W.RANK_CASES),
    "mcd_vit_attention": [(b_attention, (False,))],
    "mcd_vit_attention_long": [(b_attention, (True,))],
    "mcd_vit_attention_cls": [(b_attention_cls, ())],
    "mcd_layer_norm": [(b_layer_norm, ())],
    "mcd_patchify": [(b_patchify, ())],
    "mcd_conv_stem_nhwc": [(b_conv_stem, ())],
    "mcd_dwconv_bn_silu": [(b_dwconv, ())],
    "mcd_se_gate": [(b_se_gate, ())],
    "mcd_channel_scale": [(b_channel_scale, ())],
    "mcd_hook_pool_nhwc": [(b_hook_pool, (True,))],
    "mcd_conv7x7s2_nhwc": [(b_conv7x7, ())],
    "mcd_bn_relu_maxpool_nhwc": [(b_maxpool, ())],
    "mcd_conv_igemm_nhwc": [(b_igemm, (False,))],
    "mcd_conv_igemm_res_nhwc": [(b_igemm, (True,))],
    "mcd_conv3x3s2_nhwc": [(b_conv3x3, ())],
    "mcd_avgpool2_nhwc": [(b_avgpool, ())],
    "mcd_attnpool_tokens": [(b_attnpool, ())],
    "mcd_image_preprocess": [(b_preprocess, ())],
    "mcd_image_minmax_normalize": _ws(W.minmax_case, W.MINMAX_CASES),
    "mcd_linear_residual": _ws(W.linear_case, [c for c in W.LINEAR_CASES if not c[0]]),
    "mcd_linear_residual_relu": _ws(W.linear_case, [c for c in W.LINEAR_CASES if c[0]]),
}
BLASLT = ("mcd_linear_residual", "mcd_linear_residual_relu")
ROWS = [(entry, j) for entry, rows in STREAM_TABLE.items() for j in range(len(rows))]
MIN_SPIN_MS, SPIN_FACTOR = 10.0, 20.0


class Run:
    """A case with frame-free outputs and its workspace: what both checks share."""

    def __init__(self, entry, case, dev):
        self.entry, self.c, self.dev = entry, case, dev
        self.outs = [torch.full((r * p,), f, dtype=dt, device=dev) for (r, w, p, dt, f, zp) in case.outs]
        self.ws = torch.full((max(case.need, 256),), 0xFF, dtype=torch.uint8, device=dev)
        self.tol = case.tol

    def call(self, stream):
        return self.c.call(self.ws.data_ptr() if self.c.need else None, self.c.need, [o.data_ptr() for o in self.outs], stream)

    def stage(self, seed):
        return [t.to(self.dev) for t in self.c.gen(seed)]

    def refill(self, data):
        for t, f in zip(self.c.ins, data):
            t.copy_(f)
        for j, g in self.c.inout.items():
            self.outs[j].copy_(data[g].reshape(-1))

    def poison(self):
        for o, spec in zip(self.outs, self.c.outs):
            o.fill_(spec[4])
        self.ws.fill_(0xFF)

    def untouched(self):
        return all(bool((o == spec[4]).all()) for o, spec in zip(self.outs, self.c.outs))

    def eager(self, data):
        """The entry on `data` on the default stream: clones of the outputs."""
        self.poison()
        self.refill(data)
        assert self.call(None) == 0
        torch.cuda.synchronize()
        return [o.clone() for o in self.outs]

    def same(self, got, want, what):
        for j, (a, b) in enumerate(zip(got, want)):
            if self.tol:
                bound = self.tol * float(b.abs().max())
                assert float((a - b).abs().max()) <= bound, (what, j, bound)
            else:
                assert torch.equal(int_bits(a), int_bits(b)), (what, "output %d differs from the eager result" % j)


@pytest.fixture(scope="module")
def env():
    """The libraries, every case built once, and the spin: the eager call of every case timed with a pair of events; the spin
    lasts SPIN_FACTOR times the slowest and at least MIN_SPIN_MS, converted to cycles with the device's clock_rate (kHz; where
    torch does not expose it, with the measured rate of the spin's counter) and checked against the spin's own event time."""
    import mammo_clip_dissect_amd as mcd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    L, B = mcd._lib.load(), mcd._lib.load_blaslt()
    assert B is not None, "libmcd_blaslt.so not built"
    assert L.mcd_embed_gemm_exp_time_kernel(0) == 0      # the measurement hook off (its default): reps > 0 is outside the promise
    mp = pytest.MonkeyPatch()
    mp.setenv("MCD_BLASLT_PICK", "heuristic")
    cases, slowest = {}, (0.0, None)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for entry, j in ROWS:
        builder, params = STREAM_TABLE[entry][j]
        lib = B if entry in BLASLT else L
        c = builder(lib, dev, *params, top=False) if builder.__module__ == W.__name__ else builder(lib, dev, *params)
        cases[(entry, j)] = c
        r = Run(entry, c, dev)
        r.refill(r.stage(5))
        assert r.call(None) == 0, (entry, params)
        torch.cuda.synchronize()
        e0.record()
        assert r.call(None) == 0
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms > slowest[0]:
            slowest = (ms, c.what)
        del r
    spin_ms = max(MIN_SPIN_MS, SPIN_FACTOR * slowest[0])
    rate = getattr(torch.cuda.get_device_properties(dev), "clock_rate", None)       # kHz = cycles per ms
    if not rate:                      # a torch build that does not expose it: the rate of the spin's own counter, measured
        probe = 20_000_000
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        rate = probe / e0.elapsed_time(e1)
    cycles = int(spin_ms * rate)
    for _ in range(2):
        torch.cuda.synchronize()
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        e1.synchronize()
        real = e0.elapsed_time(e1)
        if spin_ms <= real <= 2 * spin_ms:
            break
        cycles = int(cycles * 1.25 * spin_ms / real)
    print("stream contracts: slowest eager call %.3f ms (%s); spin %.1f ms = %d cycles at %.0f cycles / ms, measured %.1f ms" % (
        slowest[0], slowest[1], spin_ms, cycles, rate, real))
    assert real >= spin_ms
    yield dict(L=L, B=B, dev=dev, cases=cases, cycles=cycles)
    mp.undo()


def side_stream(r, cycles, stream_for_call):
    """Stale inputs; then on S: spin, fresh data into the inputs, the call on stream_for_call(S), copies of the outputs.  Returns
    (copies, the eager result on the fresh data)."""
    fresh, stale = r.stage(1001), r.stage(2002)
    want = r.eager(fresh)
    r.poison()
    r.refill(stale)
    snaps = [torch.empty_like(o) for o in r.outs]
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        r.refill(fresh)
        rc = r.call(stream_for_call(S))
        for s, o in zip(snaps, r.outs):
            s.copy_(o)
    S.synchronize()
    torch.cuda.synchronize()
    assert rc == 0
    return snaps, want


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-%d" % r)
def test_the_call_is_ordered_on_its_stream(env, row):
    r = Run(row[0], env["cases"][row], env["dev"])
    snaps, want = side_stream(r, env["cycles"], lambda S: S.cuda_stream)
    r.same(snaps, want, r.c.what)


def test_a_launch_on_another_stream_is_seen(env):
    """The control: mcd_layer_norm given stream NULL while its inputs are written on S behind the spin.  It runs at once, on
    the stale inputs, and the copy taken on S is not the expected result."""
    r = Run("mcd_layer_norm", env["cases"][("mcd_layer_norm", 0)], env["dev"])
    snaps, want = side_stream(r, env["cycles"], lambda S: None)
    assert not torch.equal(int_bits(snaps[0]), int_bits(want[0])), "a launch on the NULL stream went unnoticed"


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-%d" % r)
def test_capture_and_replay(env, row):
    r = Run(row[0], env["cases"][row], env["dev"])
    data = [r.stage(3003), r.stage(4004)]
    want = [r.eager(d) for d in data]
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):                  # the warm-up on S
        assert r.call(S.cuda_stream) == 0
    S.synchronize()
    r.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    kept = [bytes(arr) for arr in r.c.host]      # (the cases are shared: the host arrays are put back at the end)
    try:
        with torch.cuda.graph(g, stream=S):
            rc = r.call(torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (r.c.what, rc)
        torch.cuda.synchronize()
        assert r.untouched(), (r.c.what, "the call ran during the capture")
        for arr in r.c.host:
            ctypes.memset(arr, 0, ctypes.sizeof(arr))
        for d, w in zip(data, want):
            r.poison()
            r.refill(d)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            r.same(r.outs, w, r.c.what)
    finally:
        g.reset()
        for arr, b in zip(r.c.host, kept):
            ctypes.memmove(arr, b, len(b))
