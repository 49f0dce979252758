"""Shared helpers for the tests: golden loading and the stated tolerances, the rank-spawn harness of the multi-rank
tests, and the helpers the two tower test files (EfficientNet-B5, ResNet-50) share."""
import os
import socket
import sys
import time
from multiprocessing.connection import wait

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["tiny", "main", "relu", "kfull", "one_neuron", "n1000"]

# ---- tolerances (DESIGN.md section 6 explains each) ------------------------------------------------
# north_star: "similarity scores within 1e-4 fp32".  The scores are differences of two fp32 numbers of
# magnitude 256..1024 (prob_d_given_e and prob_d), whose ulp is 3.05e-5 .. 6.1e-5, so 1e-4 is 1.6 ulp of
# the intermediates: an implementation whose exp/log differ from SLEEF's in the last bit lands exactly on
# the oracle for >99.9% of the entries and 1 or 2 intermediate ulps away on the rest.
SIM_BOUNDARY_ATOL = 6.2e-5   # soft_wpmi(P, A) at the drop-in boundary (same P as the reference): ONE ulp of the
                             # intermediates; nothing may exceed it, and SIM_BOUNDARY_EXACT of the entries are bit-identical
SIM_BOUNDARY_EXACT = 0.9995   # measured: 99.998 % (main: 1 entry of 48 832), 100 % on every other case
SIM_ATOL = 1e-4          # the stated tolerance; must hold for all but SIM_OUTLIER_FRAC of the entries
SIM_OUTLIER_FRAC = 1e-3  # entries allowed between SIM_ATOL and SIM_HARD_ATOL
SIM_HARD_ATOL = 2.5e-4   # 4 ulp of an intermediate in [512, 1024): nothing may exceed this
SIM_MEAN_ATOL = 2e-5
ARGMAX_GAP = 2.5e-4      # integer matches are asserted on rows whose reference gap exceeds this
P_ATOL = 5e-7            # P = I_hat @ T_hat^T entries are in [-1, 1]; fp32 dot of 512 terms
S_RTOL = 2e-6            # softmax entries, relative
PDGE_ATOL = 1.3e-4       # 2 ulp at [512,1024) for the un-normalised sums given identical inputs


def golden(name):
    return np.load(os.path.join(GOLDEN, "sim_%s.npz" % name))


def regen_n1000():
    """Inputs of the n1000 case are regenerated from the seed (make_golden.py: make_inputs).  P is recomputed with
    the oracle's restatement of the fixture host's normalise + matmul order (bit-identical to every stored P): torch's
    own matmul on the host running the tests may cut K differently (MKL picks per CPU model)."""
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), os.pardir, "oracle"))
    import oracle as O
    N, C, U, D, seed = 1000, 763, 48, 512, 61
    g = torch.Generator().manual_seed(seed)
    E_img = torch.randn(N, D, generator=g)
    g = torch.Generator().manual_seed(seed + 1)
    E_txt = torch.randn(C, D, generator=g)
    g = torch.Generator().manual_seed(seed + 2)
    A = torch.randn(N, U, generator=g)
    P = O.embed_gemm(E_img.numpy(), E_txt.numpy(), blas=False)
    return E_img.numpy(), E_txt.numpy(), A.numpy(), P


def regen_inputs(N, C, U, D, seed):
    """make_golden.py: make_inputs(..., act="gauss") regenerated from the seed; P by the oracle's restatement of the
    fixture host's normalise + matmul order."""
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), os.pardir, "oracle"))
    import oracle as O
    E_img = torch.randn(N, D, generator=torch.Generator().manual_seed(seed)).numpy()
    E_txt = torch.randn(C, D, generator=torch.Generator().manual_seed(seed + 1)).numpy()
    A = torch.randn(N, U, generator=torch.Generator().manual_seed(seed + 2)).numpy()
    return E_img, E_txt, A, O.embed_gemm(E_img, E_txt, blas=False)


def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_N10K = {}


def n10k_inputs():
    """The real-size golden (configs[1]'s layer shape: 10 000 images x 768 neurons x 763 concepts): inputs from the
    seed, every one of them checked against the sha256 the generator stored (P: the bits torch computed there)."""
    if not _N10K:
        z = golden("n10k")
        meta = __import__("json").load(open(os.path.join(GOLDEN, "golden_meta.json")))["cases"]["n10k"]
        E_img, E_txt, A, P = regen_inputs(meta["N"], meta["C"], meta["U"], meta["D"], meta["seed"])
        for name, arr in (("E_img", E_img), ("E_txt", E_txt), ("A", A), ("P", P)):
            assert sha256(arr) == str(z[name + "_sha256"]), name
        _N10K.update(z=z, E_img=E_img, E_txt=E_txt, A=A, P=P, K=int(z["top_k"]))
    return _N10K


def assert_top10_decided(got_ids, got_vals, ref_ids, ref_vals, what=""):
    """Top-k lists given only the reference's top-k VALUES (no full similarity matrix): rank j is decided when the
    reference's gaps to rank j-1 and rank j+1 both exceed ARGMAX_GAP (the last rank needs only the gap above: what
    lies below it is unknown, so it is compared as a set member instead)."""
    ref_vals = np.asarray(ref_vals)
    gaps = ref_vals[:, :-1] - ref_vals[:, 1:]
    clear = gaps > ARGMAX_GAP                                    # [U, k-1]
    above = np.concatenate([np.ones((clear.shape[0], 1), bool), clear], axis=1)[:, :-1]
    decided = above & clear                                      # ranks 0..k-2
    same = np.asarray(got_ids)[:, :decided.shape[1]] == np.asarray(ref_ids)[:, :decided.shape[1]]
    bad = decided & ~same
    assert not bad.any(), "%s: %d decided ranks differ" % (what, int(bad.sum()))
    assert np.abs(np.asarray(got_vals) - ref_vals).max() <= SIM_ATOL, what
    return float(decided.mean())


SCORE_ULP = 2.0 ** -15   # one ulp of soft_wpmi's fp32 intermediates (prob_d_given_e and prob_d are ~ -420): the
                         # reference's scores are multiples of it, and so are the gaps between them


def assert_topk_against_full_sim(got_ids, ref_sim, k, what=""):
    """Top-k lists against the reference's FULL similarity matrix.  Rank j of a row is decided when the reference's gaps to
    rank j-1 and to rank j+1 both exceed ONE ulp of the scores (SCORE_ULP; a 1-ulp gap is what a single last-bit difference
    in one log can close -- the reference's own `torch.log` is not correctly rounded in 0.02 % of its results);
    every decided rank must carry the reference's concept, and rank 0 must do so on every row that has a decided rank 0.
    Returns (decided ranks, undecided ranks)."""
    ref = np.asarray(ref_sim, np.float32)
    got = np.asarray(got_ids)
    order = np.argsort(-ref, axis=1, kind="stable")[:, :k + 1]
    v = np.take_along_axis(ref, order, axis=1).astype(np.float64)
    gaps = v[:, :-1] - v[:, 1:]                     # [U, k]: gap between rank j and rank j+1
    below = gaps > SCORE_ULP * 1.001
    above = np.concatenate([np.ones((ref.shape[0], 1), bool), below[:, :-1]], axis=1)
    decided = above & below                         # [U, k]
    bad = decided & (got[:, :k] != order[:, :k])
    n_dec, n_und = int(decided.sum()), int((~decided).sum())
    msg = "%s: top-%d ranks decided %d, undecided %d (gap <= 1 ulp = %.3g), decided-but-different %d" % (
        what, k, n_dec, n_und, SCORE_ULP, int(bad.sum()))
    if os.environ.get("MCD_STATS_FILE"):
        with open(os.environ["MCD_STATS_FILE"], "a") as f:
            f.write("ranks " + msg + "\n")
    assert not bad.any(), msg
    return n_dec, n_und


def case_inputs(name):
    z = golden(name)
    if name == "n1000":
        E_img, E_txt, A, P = regen_n1000()
        assert abs(float(P.astype(np.float64).sum()) - float(z["P_checksum"])) < 1e-3
        assert abs(float(A.astype(np.float64).sum()) - float(z["A_checksum"])) < 1e-6
        return z, E_img, E_txt, A, P
    return z, z["E_img"], z["E_txt"], z["A"], z["P"]


def assert_sim_boundary(got, ref, what=""):
    """Same inputs as the reference (its own P / S): bit-exact softmax and top-K, near correctly rounded log."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    exact = float((d == 0).mean())
    msg = "%s max=%.3e mean=%.3e exact=%.4f" % (what, d.max(), d.mean(), exact)
    if os.environ.get("MCD_STATS_FILE"):
        with open(os.environ["MCD_STATS_FILE"], "a") as f:
            f.write("boundary " + msg + "\n")
    assert d.max() <= SIM_BOUNDARY_ATOL, msg
    assert exact >= SIM_BOUNDARY_EXACT or d.size < 2000, msg
    return d.max(), exact


def assert_sim_close(got, ref, what=""):
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    frac = float((d > SIM_ATOL).mean())
    msg = "%s max=%.3e mean=%.3e frac>1e-4=%.2e exact=%.4f" % (what, d.max(), d.mean(), frac, float((d == 0).mean()))
    if os.environ.get("MCD_STATS_FILE"):
        with open(os.environ["MCD_STATS_FILE"], "a") as f:
            f.write(msg + "\n")
    assert d.max() <= SIM_HARD_ATOL, msg
    assert (d > SIM_ATOL).sum() <= max(2, SIM_OUTLIER_FRAC * d.size), msg   # small cases: 2 entries at most
    assert d.mean() <= SIM_MEAN_ATOL, msg
    return d.max(), d.mean(), frac


def assert_topk_ids(got_ids, got_sim, ref_ids, ref_sim, k, what=""):
    """Integer match of the top-k concept ids per neuron wherever the reference ranking is separated by
    more than ARGMAX_GAP; elsewhere the two orders may swap neighbours that are closer than the gap."""
    ref_sim = np.asarray(ref_sim)
    order = np.sort(ref_sim, axis=1)[:, ::-1][:, :k + 1]
    gaps = order[:, :-1] - order[:, 1:]            # [U,k] gap below each of the k ranks
    if gaps.shape[1] < k:                          # k == C: nothing ranks below the last entry
        gaps = np.concatenate([gaps, np.full((gaps.shape[0], k - gaps.shape[1]), np.inf, gaps.dtype)], axis=1)
    clear = gaps > ARGMAX_GAP
    same = np.asarray(got_ids)[:, :k] == np.asarray(ref_ids)[:, :k]
    # a rank is "decided" when the gaps above and below it are clear
    above = np.concatenate([np.ones((gaps.shape[0], 1), bool), clear[:, :-1]], axis=1)
    decided = clear & above
    bad = decided & ~same
    assert not bad.any(), "%s: %d decided ranks differ" % (what, int(bad.sum()))
    return float(decided.mean())


def host_staged_gather(group=None):
    """A `gather` for pipeline.Dissector that rehearses several ranks on ONE GPU: RCCL cannot put two ranks on one
    device, so the ranks rendezvous over gloo and the payload is staged through the host.  Test/bench rehearsal only --
    the package's own transport is rccl_all_gather_rows (device memory, backend "nccl")."""
    import torch.distributed as dist

    def gather(t):
        world = dist.get_world_size(group)
        host = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype)
        dist.all_gather_into_tensor(host, t.contiguous().cpu(), group=group)
        return host.to(t.device)
    return gather


# ---- the reference's own outputs on off-golden shapes (make_golden.py --fuzz; round 5) -------------------------
FUZZ_ATOL = 1e-4          # north_star's tolerance, asserted against the REFERENCE's output directly (not through the oracle)
FUZZ_TOP1_GAP = 1.3e-4    # a top-1 / top-10 rank is decided when the reference's own gaps exceed two ulps of its sums (6.1e-5 each)
_FUZZ = {}


def fuzz_cases():
    import json
    return json.load(open(os.path.join(GOLDEN, "sim_fuzz_meta.json")))["cases"]


def fuzz_case(i):
    """Case i of tests/golden/sim_fuzz.npz: inputs regenerated from the stored recipe (torch's CPU generator; every byte checked
    against the sha256 the generator script stored), the reference's soft_wpmi / wpmi outputs and top-10 lists."""
    if "z" not in _FUZZ:
        _FUZZ["z"] = np.load(os.path.join(GOLDEN, "sim_fuzz.npz"))
        _FUZZ["meta"] = fuzz_cases()
    z, r = _FUZZ["z"], _FUZZ["meta"][i]
    if r["kind"] == "scaled":
        g = torch.Generator().manual_seed(r["gen_seed"])
        P = (torch.randn(r["N"], r["C"], generator=g) * 0.05).numpy()
        A = torch.randn(r["N"], r["U"], generator=g).numpy()
    else:
        _, _, A, P = regen_inputs(r["N"], r["C"], r["U"], 512, r["gen_seed"])
    assert sha256(A) == r["A_sha256"], "A of fuzz case %d" % i
    assert sha256(P) == r["P_sha256"], "P of fuzz case %d (the oracle's restatement of the fixture host's normalise + matmul)" % i
    ref = {k: z["%s_%d" % (k, i)] for k in ("soft", "wpmi", "soft_ids10", "wpmi_ids10", "soft_vals10", "wpmi_vals10")}
    return r, P, A, ref


def fuzz_compare(got, ref_full, what, stats):
    """got against the reference's output: everything within FUZZ_ATOL; the top concept of every neuron whose reference gap to
    the runner-up exceeds FUZZ_TOP1_GAP; the top-10 ranks decided by that gap.  Appends (entries, bit-identical, max |diff|) to stats."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref_full, np.float32)
    assert got.shape == ref.shape, what
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert np.isfinite(got).all() and float(d.max()) <= FUZZ_ATOL, "%s: max |diff| %.3g" % (what, float(d.max()))
    k = min(10, ref.shape[1])
    order = np.argsort(-ref, axis=1, kind="stable")[:, :min(k + 1, ref.shape[1])]
    v = np.take_along_axis(ref, order, axis=1).astype(np.float64)
    gorder = np.argsort(-got, axis=1, kind="stable")[:, :k]
    n_dec = n_bad = 0
    if ref.shape[1] > 1:
        gaps = v[:, :-1] - v[:, 1:]
        below = gaps > FUZZ_TOP1_GAP
        if below.shape[1] < k:
            below = np.concatenate([below, np.ones((ref.shape[0], k - below.shape[1]), bool)], axis=1)
        above = np.concatenate([np.ones((ref.shape[0], 1), bool), below[:, :-1]], axis=1)
        decided = (above & below)[:, :k]
        bad = decided & (gorder != order[:, :k])
        n_dec, n_bad = int(decided.sum()), int(bad.sum())
        assert not bad[:, 0].any(), "%s: the top concept differs on %d neurons whose reference gap exceeds %.2g" % (what, int(bad[:, 0].sum()), FUZZ_TOP1_GAP)
        assert n_bad == 0, "%s: %d decided top-10 ranks differ" % (what, n_bad)
    stats.append((what, int(d.size), int((got == ref).sum()), float(d.max()), n_dec))


# ---- the rank-spawn harness ---------------------------------------------------------------------------------------------
RANK_EXIT_GRACE = 120     # seconds the ranks get to leave the barrier and exit once every result is in
TORCHRUN_ENV = {"WORLD_SIZE": "{world}", "RANK": "{rank}", "LOCAL_RANK": "0"}    # what the drivers read (all ranks on cuda:0)


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_main(rank, world, port, body, args, env, conn):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **{k: str(v).format(world=world, rank=rank)
                                                                          for k, v in (env or {}).items()})
    dist.init_process_group("gloo", rank=rank, world_size=world)
    conn.send(body(world, rank, *args))
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(world, body, args=(), timeout=600, env=None):
    """body(world, rank, *args) in `world` spawned processes that form one gloo group; returns {rank: result}.

    Each process sets the rendezvous variables and `env` ("{world}" / "{rank}" in a value are filled in; TORCHRUN_ENV is
    the set the drivers read), joins the group, sends body's result, then meets the others in a barrier and leaves.  The
    parent waits on the result pipes and on the processes together: `timeout` seconds for the results, RANK_EXIT_GRACE
    more for the exits.  The moment a process exits non-zero or the time is up, the remaining ones -- blocked in a
    collective that can no longer complete, each with its device open -- are terminated (killed after 5 s), joined, and
    the call fails with the rank and its exit code."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = free_port()
    procs, pipes = [], {}
    for r in range(world):
        rd, wr = ctx.Pipe(duplex=False)
        procs.append(ctx.Process(target=_rank_main, args=(r, world, port, body, tuple(args), env, wr)))
        procs[-1].start()
        wr.close()
        pipes[rd] = r
    running = {p.sentinel: r for r, p in enumerate(procs)}
    results, failed, t0 = {}, [], time.monotonic()
    try:
        while not failed and (running or pipes):
            left = t0 + timeout + (RANK_EXIT_GRACE if len(results) == world else 0) - time.monotonic()
            ready = wait(list(pipes) + list(running), max(left, 0))
            if not ready:
                failed.append("rank(s) %s still running after %d s" % (sorted(running.values()), time.monotonic() - t0))
            for x in ready:
                if x in pipes:
                    r = pipes.pop(x)
                    try:
                        results[r] = x.recv()
                    except EOFError:          # the process ended without a result: its exit code says why
                        pass
                else:
                    r = running.pop(x)
                    procs[r].join()
                    if procs[r].exitcode != 0:
                        failed.append("rank %d exited with code %s" % (r, procs[r].exitcode))
        if not failed and len(results) < world:
            failed.append("rank(s) %s exited with code 0 without a result" % sorted(set(range(world)) - set(results)))
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(5)
            if p.is_alive():
                p.kill()
                p.join()
    assert not failed, "run_ranks(%d ranks, %s): %s" % (world, getattr(body, "__name__", body), "; ".join(failed))
    return results


# ---- shared by the EfficientNet-B5 and ResNet-50 tower tests ------------------------------------------------------------
def nerr(got, ref):
    """max |got - ref| / max |ref| in float64."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def mild_bn(mod, seed):
    """Random BN statistics, gamma and beta that keep a whole tower's activations in range (the defaults hide folding
    errors)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.weight.copy_(1 + 0.2 * torch.randn(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))


def randomise_bn(mod, g):
    """Random running statistics, gamma and beta on every BatchNorm2d (the defaults make BN nearly an identity)."""
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n, generator=g, dtype=m.running_mean.dtype))
            m.running_var.copy_(torch.rand(n, generator=g, dtype=m.running_var.dtype) * 2 + 0.05)
            m.weight.data.copy_(torch.randn(n, generator=g, dtype=m.weight.dtype))
            m.bias.data.copy_(torch.randn(n, generator=g, dtype=m.bias.dtype))


class CallCounter:
    """Counts the calls of the named core wrappers (n[name], absent until the first call) and the core.linear_residual
    calls with relu=True (relu_gemms), by monkeypatching the module attributes the routes call through."""

    def __init__(self, core, monkeypatch, names):
        self.n = {}
        self.relu_gemms = 0
        for name in names:
            fn = getattr(core, name)

            def wrap(*a, _fn=fn, _name=name, **kw):
                self.n[_name] = self.n.get(_name, 0) + 1
                return _fn(*a, **kw)
            monkeypatch.setattr(core, name, wrap)
        lr = core.linear_residual

        def lin(*a, **kw):
            if kw.get("relu"):
                self.relu_gemms += 1
            return lr(*a, **kw)
        monkeypatch.setattr(core, "linear_residual", lin)


class FakeCuda(torch.Tensor):
    """A host tensor that says it is on the GPU: lets the route's other conditions be checked one at a time on the CPU."""

    @property
    def is_cuda(self):
        return True


def nhwc_input(c, h=9, w=7):
    return torch.randn(2, c, h, w).contiguous(memory_format=torch.channels_last).as_subclass(FakeCuda)


def entry_rc(mcd, name, *args):
    """The return code of the C entry `name` called with raw arguments (the argument checks: no device call happens)."""
    return getattr(mcd._lib.load(), name)(*args)


# ---- framed buffers: the C ABI's pitch, padding and aliasing contracts (test_gpu_abi_contracts.py, test_abi_frame_cpu.py) -----
OUT_FILL = -7.0e30                    # what an output frame holds before the call: finite, and no kernel here produces it
GAP_FILLS = (float("nan"), 1.0e30)    # what the gaps of an input frame hold, one run each: the outputs must not differ


def int_bits(t):
    """The integer view of a tensor or numpy array (int32 / int16 for 4- / 2-byte floats), so that NaNs compare."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.is_floating_point():
        return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])
    return t


def framed(rows, width, pitch, base_off, guard, fill, dtype, device, tail=0):
    """(flat, view): ONE allocation of `guard` elements, `base_off` elements, (rows-1)*pitch + width elements (+ `tail` more
    that the last row's padding may take: an entry that is entitled to write the pad columns of the last row needs them)
    and `guard` elements again, all of it `fill`; view = the [rows, width] matrix of pitch `pitch` that starts behind
    guard + base_off.  guard is kept a multiple of 16 bytes, so base_off alone decides the alignment of the view."""
    assert rows >= 1 and pitch >= width >= 1 and 0 <= tail <= pitch - width
    flat = torch.full((2 * guard + base_off + (rows - 1) * pitch + width + tail,), fill, dtype=dtype, device=device)
    assert flat.data_ptr() % 16 == 0 and (guard * flat.element_size()) % 16 == 0
    return flat, torch.as_strided(flat, (rows, width), (pitch, 1), guard + base_off)


def framed_dense(shape, base_off, guard, fill, dtype, device):
    """(flat, view, view_spec) for a CONTIGUOUS N-d operand (an NHWC activation, a [B, T, C] token block): a frame of one row
    of prod(shape) elements -- guard, base_off, the elements, guard, all of it `fill` -- view = the contiguous `shape` tensor
    behind guard + base_off, view_spec what check_frame() takes.  An empty shape (an output nothing is written to) is a row of
    no elements: check_frame() then wants the whole allocation to keep its fill."""
    n = 1
    for s in shape:
        n *= int(s)
    assert n >= 0 and base_off >= 0
    flat = torch.full((2 * guard + base_off + n,), fill, dtype=dtype, device=device)
    assert flat.data_ptr() % 16 == 0 and (guard * flat.element_size()) % 16 == 0
    return flat, flat[guard + base_off:guard + base_off + n].view(*shape), (1, n, max(n, 1), base_off, guard, fill)


def check_frame(flat, view_spec, expected_bits, zero_pad=False, what=""):
    """view_spec = (rows, width, pitch, base_off, guard, fill) of framed().  On the integer views:
    (a) the logical [rows, width] region equals expected_bits;
    (b) every other element of flat still holds the fill -- except, with zero_pad, the padding columns width..pitch-1 of
        every row (the last row's as far as flat holds them in front of the trailing guard), which must be +0."""
    rows, width, pitch, base_off, guard, fill = view_spec
    fb = int_bits(flat)
    start, end = guard + base_off, fb.numel() - guard
    assert start + (rows - 1) * pitch + width <= end
    exp = int_bits(expected_bits).to(fb.device).reshape(rows, width)
    got = torch.as_strided(fb, (rows, width), (pitch, 1), start)
    bad = (got != exp).nonzero()
    assert bad.numel() == 0, "%s: %d elements of the logical region differ, the first at (row %d, column %d)" % (
        what, bad.shape[0], int(bad[0, 0]), int(bad[0, 1]))
    want = torch.full_like(fb, int(int_bits(torch.full((1,), fill, dtype=flat.dtype))[0]))
    if zero_pad and pitch > width:
        if rows > 1:
            torch.as_strided(want, (rows - 1, pitch - width), (pitch, 1), start + width).zero_()
        last = start + (rows - 1) * pitch
        want[last + width:min(last + pitch, end)] = 0
    torch.as_strided(want, (rows, width), (pitch, 1), start).copy_(exp)
    bad = (fb != want).nonzero()
    if bad.numel():
        o = int(bad[0, 0]) - start
        where = "row %d, column %d of the pitch" % (o // pitch, o % pitch) if 0 <= o < end - start else \
            ("the leading guard / base offset" if o < 0 else "the trailing guard")
        raise AssertionError("%s: %d elements outside the logical region changed (or a promised zero is not +0), the first "
                             "at flat[%d] = %s" % (what, bad.shape[0], int(bad[0, 0]), where))


FRAME_GUARD = 64    # elements of guard on each side of a FramedIn / FramedOut: 256 bytes of fp32 / int32, 128 of bf16


class FramedIn:
    """A matrix inside a framed allocation whose gaps hold `gap`; .same() says the call left the allocation untouched."""

    def __init__(self, data, pitch, off, gap):
        rows, width = data.shape      # (the last row whole, as a caller's matrix has it: a 16-byte path may read its padding)
        self.flat, self.view = framed(rows, width, pitch, off, FRAME_GUARD, gap, data.dtype, data.device, tail=pitch - width)
        self.view.copy_(data)
        self.snap = self.flat.clone()
        self.ptr, self.ld = self.view.data_ptr(), pitch
        self.spec = (rows, width, pitch, off, FRAME_GUARD, gap)

    def same(self):
        assert torch.equal(int_bits(self.flat), int_bits(self.snap)), "the call changed an input"


class FramedOut:
    def __init__(self, rows, width, pitch, off, dtype, dev, tail=0, fill=OUT_FILL):
        self.spec = (rows, width, pitch, off, FRAME_GUARD, fill)
        self.flat, self.view = framed(*self.spec, dtype, dev, tail=tail)
        self.ptr, self.ld = self.view.data_ptr(), pitch

    def check(self, expected, zero_pad=False, what=""):
        check_frame(self.flat, self.spec, expected, zero_pad=zero_pad, what=str(what))


# ---- framed workspaces: the C ABI's workspace contract (test_gpu_workspace_contracts.py, test_exec_contract_cpu.py) ---------
WS_GUARD = 4096                   # bytes of guard on each side of a workspace frame
WS_ALIGN = 256                    # alignment of a framed workspace's interior
WS_FILLS = (0x00, 0xFF, 0x7F)     # what a workspace (and its guards) holds before the call, one run each: 0xFF.. is int32 -1 (K3's
                                  # mark) and a NaN as fp32 and as bf16; 0x7F.. is a large finite fp32 (3.4e38) and a bf16 NaN


def framed_ws(nbytes, guard_bytes=WS_GUARD, fill_byte=0xFF, device="cpu"):
    """(flat, ptr, nbytes): ONE uint8 allocation -- guard | nbytes | guard, the interior WS_ALIGN-byte aligned -- all of it,
    the interior included, `fill_byte`; ptr = the address of the interior.  (The bytes in front of the leading guard that the
    alignment costs and those behind the trailing guard belong to the guards: check_ws_guards() wants all of them kept.)"""
    assert nbytes >= 0 and guard_bytes >= 0 and 0 <= fill_byte <= 255
    flat = torch.full((guard_bytes + nbytes + guard_bytes + WS_ALIGN,), fill_byte, dtype=torch.uint8, device=device)
    start = guard_bytes + (-(flat.data_ptr() + guard_bytes)) % WS_ALIGN
    flat.ws_start = start
    return flat, flat.data_ptr() + start, nbytes


def ws_interior(flat, nbytes):
    return flat[flat.ws_start:flat.ws_start + nbytes]


def check_ws_guards(flat, nbytes, fill_byte, what=""):
    """Both guards of a framed_ws() allocation -- every byte outside the `nbytes` of the interior -- still hold the fill."""
    start = flat.ws_start
    for name, part, base in (("leading", flat[:start], 0), ("trailing", flat[start + nbytes:], start + nbytes)):
        bad = (part != fill_byte).nonzero()
        assert bad.numel() == 0, "%s: %d bytes of the workspace's %s guard changed, the first %d bytes %s" % (
            what, bad.shape[0], name, (start - int(bad[0, 0])) if name == "leading" else int(bad[0, 0]) + 1,
            "in front of the workspace" if name == "leading" else "past its end")


def check_ws_untouched(flat, fill_byte, what=""):
    """A refused call: the whole allocation, interior and guards, still holds the fill."""
    bad = (flat != fill_byte).nonzero()
    assert bad.numel() == 0, "%s: a refused call wrote %d bytes of its workspace" % (what, bad.shape[0])


def assert_same_bits(runs, what=""):
    """runs: [(label, [output tensors / arrays])], one entry per run of the same call under another workspace fill, another
    stale output content or on another stream.  Every run's outputs must equal the first run's bit for bit (NaNs by payload):
    a result that depends on what a workspace or an output held before the call differs between two of them."""
    label0, first = runs[0]
    for label, outs in runs[1:]:
        assert len(outs) == len(first), what
        for j, (a, b) in enumerate(zip(first, outs)):
            a, b = int_bits(a), int_bits(b)
            assert a.shape == b.shape, (what, label, j)
            bad = (a.reshape(-1) != b.reshape(-1).to(a.device)).nonzero()
            assert bad.numel() == 0, "%s: output %d of run %r differs from run %r in %d elements, the first at flat index %d" % (
                what, j, label, label0, bad.shape[0], int(bad[0, 0]))
