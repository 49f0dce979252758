"""GPU: K9B (mcd_vit_attention_relbias) and K27 (mcd_masked_mean_l2) of include/mcd_sentence.h through the C ABI, and the HIP
route of data_utils.MPNetSentenceEncoder behind get_cos_similarity.

K9B against float64 under test_gpu_text_tower's K9M bound (twice SDPA's own error), its bit contracts against K9M (rel NULL,
rel zero), against itself (a sequence alone with its slice of rel, swapped neighbours), what it must not read (padded K / V
rows, rel beyond the longest sequence), the guarded frames and the head a rel row lands on.  K27 against float64 under
test_gpu_hf_clip's K26 bound (twice ATen's own error), its independence of neighbours, what it must not read and the zero row.
Both entries on a side stream and captured alone into a graph.  Then the fixture model (tests/golden/mpnet.npz) on the HIP
route against the ATen route and transformers' numbers, and get_cos_similarity against its CPU value.

Padded query rows t >= L of K9B are written but unspecified against MPNet (mcd_sentence.h): the float64 comparisons look at
the valid rows, the bit comparisons at every row."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import openai_clip_recipe as clip_recipe
import test_gpu_encoder_frames as EF
import test_gpu_stream_contracts as S
import test_gpu_text_tower as TT
import util
from test_gpu_text_tower import spin_cycles  # noqa: F401  (the fixture)
from util import int_bits, nerr

pytestmark = pytest.mark.gpu

NAN = float("nan")
VOCAB = os.path.join(util.GOLDEN, "mpnet_vocab.txt")
_bound = TT._bound                      # e <= 2 * (ATen's error against float64) + 1e-6


@pytest.fixture(scope="module")
def L(mcd, dev):
    return mcd._lib.load()


@pytest.fixture(scope="module")
def core(mcd):
    from mammo_clip_dissect_amd import core
    return core


@pytest.fixture(scope="module")
def du(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils
    return data_utils


def written(out):
    assert not bool((int_bits(out) == int(int_bits(torch.full((1,), util.OUT_FILL))[0])).any()), "an output element was not written"


# ---- K9B -----------------------------------------------------------------------------------------------------------------
def k9b(L, qkv, H, lens, rel, gap=NAN):
    """K9B on framed operands: qkv, lens and rel inside guards of `gap` / LENS_GAP / `gap`, the output in a frame of OUT_FILL
    whose guards must come back intact and whose every element must have been written; the inputs untouched."""
    B, T, _ = qkv.shape
    q_ = EF.In(qkv, gap)
    l_ = None if lens is None else EF.In(torch.tensor(lens, dtype=torch.int32, device=qkv.device), TT.LENS_GAP)
    r_ = None if rel is None else EF.In(rel, gap)
    o_ = EF.Out((B, T, H * 64), qkv.device)
    EF.ok(L.mcd_vit_attention_relbias(q_.ptr, B, T, H, None if l_ is None else l_.ptr, None if r_ is None else r_.ptr, o_.ptr,
                                      EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K9B", tuple(qkv.shape), lens))          # the guards: the pre-fill intact outside [B, T, H*64]
    written(out)
    for a in (q_, l_, r_):
        if a is not None:
            a.same()
    return out


def full_bias(rel, T):
    t = torch.arange(T, device=rel.device)
    return rel[:, (t[None, :] - t[:, None]) + T - 1]                                   # [H, T, T]: entry (t, j) = rel[h, j - t + T - 1]


def reference64(qkv, H, lens, rel):
    B, T, _ = qkv.shape
    q, k, v = qkv.double().cpu().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0 + full_bias(rel.double().cpu(), T)[None]
    keep = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, H * 64)


def sdpa(qkv, H, lens, rel):
    B, T, _ = qkv.shape
    q, k, v = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    keep = (torch.arange(T, device=qkv.device)[None, :] < torch.tensor(lens, device=qkv.device)[:, None])[:, None, None, :]
    mask = full_bias(rel, T)[None].expand(B, -1, -1, -1).masked_fill(~keep, float("-inf"))
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, T, H * 64)


def valid(lens, T, dev="cpu"):
    return torch.arange(T, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None]          # [B, T]


# B = 3, H = 2; T: one key, one short of a tile, a tile, one over, three waves of queries, the 8-wave maximum; the lengths mix T,
# 1 and a value that is no multiple of 32
K9B_T = [1, 31, 32, 33, 77, 256]
K9B_LENS = {1: [1, 1, 1], 31: [31, 1, 17], 32: [32, 1, 19], 33: [33, 1, 20], 77: [77, 1, 45], 256: [256, 1, 200]}
_K9B = {}


def k9b_case(L, dev, T):
    """(qkv, rel, the framed K9B output) of a case, computed once and left unchanged."""
    if T not in _K9B:
        B, H = 3, 2
        qkv = EF.rnd((B, T, 3 * H * 64), 300 + T, dev)
        rel = EF.rnd((H, 2 * T - 1), 900 + T, dev)                                    # N(0, 1)
        _K9B[T] = (qkv, rel, k9b(L, qkv, H, K9B_LENS[T], rel))
    return _K9B[T]


@pytest.mark.parametrize("T", K9B_T)
def test_k9b_against_float64(L, dev, T):
    qkv, rel, out = k9b_case(L, dev, T)
    lens = K9B_LENS[T]
    ref = reference64(qkv, 2, lens, rel)
    rows = valid(lens, T)
    _bound(nerr(out.cpu()[rows], ref[rows]), nerr(sdpa(qkv, 2, lens, rel).cpu()[rows], ref[rows]), ("K9B", T, lens))
    plain = TT.reference64(qkv, 2, lens)
    assert nerr(plain[rows], ref[rows]) > 1e-2 or T == 1                              # the bias matters to the case


@pytest.mark.parametrize("T", K9B_T)
def test_k9b_without_rel_and_with_zero_rel_is_k9m(L, dev, T):
    qkv, _, _ = k9b_case(L, dev, T)
    lens = K9B_LENS[T]
    want = int_bits(TT.k9m(L, qkv, 2, lens))
    assert torch.equal(int_bits(k9b(L, qkv, 2, lens, None)), want), "rel = NULL"
    assert torch.equal(int_bits(k9b(L, qkv, 2, lens, torch.zeros(2, 2 * T - 1, device=dev))), want), "rel = 0"
    assert torch.equal(int_bits(k9b(L, qkv, 2, None, None)), int_bits(TT.k9m(L, qkv, 2, None))), "no lens, no rel"


@pytest.mark.parametrize("T", K9B_T)
def test_k9b_valid_rows_are_the_sequence_alone(L, dev, T):
    """Rows t < L of sequence b: a B = 1, T = L call with the 2L-1 entries of every rel row around distance 0."""
    qkv, rel, out = k9b_case(L, dev, T)
    for b, n in enumerate(K9B_LENS[T]):
        want = k9b(L, qkv[b:b + 1, :n].contiguous(), 2, [n], rel[:, T - n:T + n - 1].contiguous())
        assert torch.equal(int_bits(out[b:b + 1, :n]), int_bits(want)), (T, "sequence %d" % b)


@pytest.mark.parametrize("T", [33, 256])
def test_k9b_swapping_batch_neighbours_changes_nothing(L, dev, T):
    qkv, rel, out = k9b_case(L, dev, T)
    perm = [2, 0, 1]
    got = k9b(L, qkv[perm].contiguous(), 2, [K9B_LENS[T][i] for i in perm], rel)
    assert torch.equal(int_bits(got), int_bits(out[perm]))


@pytest.mark.parametrize("T", [33, 77])
def test_k9b_reads_nothing_past_the_lengths(L, dev, T):
    """NaN in every K and V row >= L, and in every rel entry whose distance no sequence of the batch has: no output bit moves."""
    qkv, rel, _ = k9b_case(L, dev, T)
    lens = [n if n < T else T - 9 for n in K9B_LENS[T]]                               # the longest is short of T
    longest = max(lens)
    out = k9b(L, qkv, 2, lens, rel)
    poisoned = qkv.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:, 2 * 64:] = NAN                                                # k and v of the padded tokens
    assert torch.equal(int_bits(k9b(L, poisoned, 2, lens, rel)), int_bits(out)), "a padded K or V row reached the output"
    far = rel.clone()
    far[:, :T - longest] = NAN                                                        # d <= -longest
    far[:, T - 1 + longest:] = NAN                                                    # d >= longest
    assert int(torch.isnan(far).sum()) == 2 * 2 * (T - longest)
    assert torch.equal(int_bits(k9b(L, qkv, 2, lens, far)), int_bits(out)), "a rel entry no sequence has reached the output"
    near = rel.clone()
    near[0, T - 1 + longest - 1] = NAN                                                # d = longest - 1: the longest sequence reads it
    b = lens.index(longest)
    got = k9b(L, qkv, 2, lens, near)
    assert bool(torch.isnan(got[b, 0, :64]).all()) and not bool(torch.isnan(got[b, :longest, 64:]).any())


def test_k9b_a_rel_row_lands_on_its_head(L, dev):
    """H = 3; head 1's row is 0 at distance 0 and -1e4 elsewhere, so every valid query of head 1 returns its own value row,
    bit for bit (p = 1 for itself, exp2 of -14 427 is 0 for the rest); heads 0 and 2 keep their own N(0, 1) rows."""
    B, T, H = 2, 45, 3
    lens = [45, 20]
    qkv = EF.rnd((B, T, 3 * H * 64), 41, dev)
    rel = EF.rnd((H, 2 * T - 1), 42, dev)
    rel[1] = -1.0e4
    rel[1, T - 1] = 0.0
    out = k9b(L, qkv, H, lens, rel)
    v = qkv.view(B, T, 3, H, 64)[:, :, 2]
    rows = valid(lens, T, dev)
    assert torch.equal(int_bits(out.view(B, T, H, 64)[:, :, 1][rows]), int_bits(v[:, :, 1][rows]))
    ref = reference64(qkv, H, lens, rel)
    _bound(nerr(out.cpu()[rows.cpu()], ref[rows.cpu()]), nerr(sdpa(qkv, H, lens, rel).cpu()[rows.cpu()], ref[rows.cpu()]), "H = 3")
    for h in (0, 2):
        assert nerr(out.view(B, T, H, 64)[:, :, h][rows], v[:, :, h][rows]) > 1e-1


def test_k9b_binding(core, L, dev):
    qkv, rel, out = k9b_case(L, dev, 33)
    ld = torch.tensor(K9B_LENS[33], dtype=torch.int32, device=dev)
    assert torch.equal(int_bits(core.vit_attention_relbias(qkv, 2, ld, rel)), int_bits(out))
    into = torch.empty_like(out)
    assert core.vit_attention_relbias(qkv, 2, ld, None, out=into) is into
    assert torch.equal(int_bits(into), int_bits(core.vit_attention_keylen(qkv, 2, ld)))
    for bad in (rel.double(), rel[:, 1:], rel.t(), rel.cpu()):
        with pytest.raises(TypeError):
            core.vit_attention_relbias(qkv, 2, ld, bad)
    with pytest.raises(TypeError):
        core.vit_attention_relbias(qkv, 2, ld.long(), rel)


# ---- K27 -----------------------------------------------------------------------------------------------------------------
# (B, T, D): one row of one float4; odd sizes with a third column block of one live lane; the 256-row
# maximum of the route at all-mpnet-base-v2's width; K10's widest row.  The lengths include 1 and T.
K27_CASES = [(1, 1, 4, [1]), (3, 33, 132, [33, 1, 20]), (2, 256, 768, [256, 1]), (5, 7, 2048, [7, 1, 4, 5, 2])]
K27_IDS = ["B%d-T%d-D%d" % c[:3] for c in K27_CASES]
_K27 = {}


def k27(L, x, lens, normalize, gap=NAN):
    B, T, D = x.shape
    x_ = EF.In(x, gap)
    l_ = None if lens is None else EF.In(torch.tensor(lens, dtype=torch.int32, device=x.device), TT.LENS_GAP)
    o_ = EF.Out((B, D), x.device)
    EF.ok(L.mcd_masked_mean_l2(x_.ptr, B, T, D, None if l_ is None else l_.ptr, int(normalize), o_.ptr, EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K27", tuple(x.shape), lens, normalize))
    written(out)
    x_.same()
    if l_ is not None:
        l_.same()
    return out


def k27_case(L, dev, case):
    if case not in _K27:
        B, T, D, lens = K27_CASES[case]
        x = EF.rnd((B, T, D), 700 + T + D, dev, 1.5, 0.25)
        _K27[case] = (x, k27(L, x, lens, True), k27(L, x, lens, False))
    return _K27[case]


def pooled(x, lens, normalize):
    """sentence-transformers' Pooling(mean) + Normalize in x's dtype and on its device."""
    m = valid(lens, x.shape[1], x.device).unsqueeze(-1).expand(x.size()).to(x.dtype)
    e = torch.sum(x * m, 1) / torch.clamp(m.sum(1), min=1e-9)
    return F.normalize(e, p=2, dim=1) if normalize else e


@pytest.mark.parametrize("normalize", [True, False], ids=["unit", "mean"])
@pytest.mark.parametrize("case", range(len(K27_CASES)), ids=K27_IDS)
def test_k27_against_float64(L, dev, case, normalize):
    B, T, D, lens = K27_CASES[case]
    x, unit, mean = k27_case(L, dev, case)
    out = unit if normalize else mean
    ref = pooled(x.double().cpu(), lens, normalize)
    _bound(nerr(out, ref), nerr(pooled(x, lens, normalize), ref), ("K27", K27_CASES[case], normalize))
    if normalize:
        assert float((out.double().norm(dim=1) - 1).abs().max()) < 1e-6
    if max(lens) == T:
        assert torch.equal(int_bits(k27(L, x[lens.index(T):lens.index(T) + 1].contiguous(), None, normalize)),
                           int_bits(out[lens.index(T):lens.index(T) + 1])), "lens = NULL is L = T"


@pytest.mark.parametrize("case", [1, 2, 3], ids=K27_IDS[1:])
def test_k27_reads_no_row_past_the_length_and_no_neighbour(L, dev, case):
    B, T, D, lens = K27_CASES[case]
    x, unit, mean = k27_case(L, dev, case)
    poisoned = x.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:] = NAN
    assert torch.equal(int_bits(k27(L, poisoned, lens, True)), int_bits(unit)), "a padded row reached the output"
    assert torch.equal(int_bits(k27(L, poisoned, lens, False)), int_bits(mean))
    for b, n in enumerate(lens):                                                       # alone, and without its padding
        assert torch.equal(int_bits(k27(L, x[b:b + 1].contiguous(), [n], True)), int_bits(unit[b:b + 1])), (b, "B = 1")
        assert torch.equal(int_bits(k27(L, x[b:b + 1, :n].contiguous(), None, True)), int_bits(unit[b:b + 1])), (b, "T = L")
    other = EF.rnd((B + 2, T, D), 78, dev, 30.0)                                       # row 0 last in a longer batch of others
    other[B + 1] = x[0]
    assert torch.equal(int_bits(k27(L, other, [3] * (B + 1) + [lens[0]], True)[B + 1]), int_bits(unit[0]))
    assert torch.equal(int_bits(k27(L, x, [0, -5] + lens[2:], True)[:2]), int_bits(k27(L, x, [1, 1] + lens[2:], True)[:2]))   # the clamp
    assert torch.equal(int_bits(k27(L, x, [T + 9] + lens[1:], True)[0]), int_bits(k27(L, x, [T] + lens[1:], True)[0]))


def test_k27_a_zero_row_gives_zeros(L, dev):
    x = EF.rnd((3, 9, 132), 5, dev)
    x[1, :4] = 0.0
    x[1, 4:] = NAN
    out = k27(L, x, [9, 4, 2], True)
    assert bool((out[1] == 0).all()) and not bool(torch.isnan(out).any())
    assert bool((k27(L, x, [9, 4, 2], False)[1] == 0).all())


def test_k27_binding(core, L, dev):
    B, T, D, lens = K27_CASES[1]
    x, unit, mean = k27_case(L, dev, 1)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    assert torch.equal(int_bits(core.masked_mean_l2(x, ld)), int_bits(unit))
    into = torch.empty(B, D, device=dev)
    assert core.masked_mean_l2(x, ld, normalize=False, out=into) is into and torch.equal(int_bits(into), int_bits(mean))
    assert torch.equal(int_bits(core.masked_mean_l2(x[:, :lens[0]].contiguous(), None)[0]), int_bits(unit[0]))
    for bad in (x.double(), x.transpose(1, 2), x[0]):
        with pytest.raises(TypeError):
            core.masked_mean_l2(bad, None)
    with pytest.raises(TypeError):
        core.masked_mean_l2(x, ld.long())


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery -------------------------------------------------
def b_relbias(L, dev):
    B, T, H = 3, 40, 1
    lens = lambda s: torch.tensor([[40, 33, 1], [7, 40, 32]][s % 2], dtype=torch.int32)
    return S.simple(L, dev, "K9B", [S._gen((B, T, 3 * H * 64)), lens, S._gen((H, 2 * T - 1))], [(B, T, H * 64)],
                    lambda i, o, st: L.mcd_vit_attention_relbias(i[0], B, T, H, i[1], i[2], o[0], st))


def b_masked_mean(L, dev):
    B, T, D = 3, 37, 132
    lens = lambda s: torch.tensor([[37, 20, 1], [5, 37, 36]][s % 2], dtype=torch.int32)
    return S.simple(L, dev, "K27", [S._gen((B, T, D)), lens], [(B, D)],
                    lambda i, o, st: L.mcd_masked_mean_l2(i[0], B, T, D, i[1], 1, o[0], st))


SENTENCE_STREAM_ROWS = {"mcd_vit_attention_relbias": b_relbias, "mcd_masked_mean_l2": b_masked_mean}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(SENTENCE_STREAM_ROWS) == sorted(mcd._lib.SENTENCE_SIGNATURES)


@pytest.mark.parametrize("entry", sorted(SENTENCE_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):  # noqa: F811
    r = S.Run(entry, SENTENCE_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)


@pytest.mark.parametrize("entry", sorted(SENTENCE_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    """The entry alone in a captured graph (one kernel node: no parallel branches), replayed on fresh data to the eager bits."""
    r = S.Run(entry, SENTENCE_STREAM_ROWS[entry](L, dev), dev)
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


# ---- the model -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "mpnet.npz")), json.load(open(os.path.join(util.GOLDEN, "mpnet_meta.json")))


def state_dict(z):
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}


@pytest.fixture(scope="module")
def model(du, fixture, dev):
    return du.sentence_encoder(dev, ckpt=state_dict(fixture[0]))


def batch(z, dev):
    return {"input_ids": torch.from_numpy(z["input_ids"].astype(np.int64)).to(dev),
            "attention_mask": torch.from_numpy(z["attention_mask"].astype(np.int64)).to(dev)}


class Calls(util.CallCounter):
    """util.CallCounter on the sentence route's wrappers, and the SDPA calls beside them."""

    def __init__(self, du, monkeypatch):
        super().__init__(du.core, monkeypatch, ["text_embed_ln", "vit_attention_relbias", "vit_attention_keylen", "layer_norm",
                                                "masked_mean_l2"])
        self.sdpa = 0
        fn = F.scaled_dot_product_attention

        def wrap(*a, **kw):
            self.sdpa += 1
            return fn(*a, **kw)
        monkeypatch.setattr(du.F, "scaled_dot_product_attention", wrap)

    def reset(self):
        self.n.clear()
        self.sdpa = 0


HIP_FORWARD = {"text_embed_ln": 1, "vit_attention_relbias": 2, "layer_norm": 4}


def test_hip_route_against_aten_and_transformers(du, model, fixture, dev, monkeypatch):
    z, _ = fixture
    tok = batch(z, dev)
    rows = tok["attention_mask"].bool()
    assert len(set(rows.sum(1).tolist())) > 4                                          # a ragged batch
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    with torch.no_grad():
        assert model.route(tok["input_ids"], tok["attention_mask"])[0] == "hip"
        h = model(tok)
        assert calls.n == HIP_FORWARD and calls.sdpa == 0                              # K24, K9B per layer, K10 behind each GEMM
        calls.reset()
        e = model.embed(tok)
        assert calls.n == dict(HIP_FORWARD, masked_mean_l2=1) and calls.sdpa == 0      # ... and K27
        calls.reset()
        monkeypatch.setattr(du, "HIP_SENTENCE", False)                                 # MCD_NO_HIP_SENTENCE=1: ATen everywhere
        h_aten = model(tok)
        e_aten = model.embed(tok)
        assert calls.n == {} and calls.sdpa == 4
        monkeypatch.setattr(du, "HIP_SENTENCE", True)
    f64, e64 = torch.from_numpy(z["hidden_f64"]), torch.from_numpy(z["embed_f64"])
    a_h, a_e = nerr(torch.from_numpy(z["hidden_f32"]), f64), nerr(torch.from_numpy(z["embed_f32"]), e64)
    _bound(nerr(h[rows], f64), a_h, "last_hidden_state on the HIP route, valid rows")
    _bound(nerr(h_aten[rows], f64), a_h, "last_hidden_state on the ATen route on the GPU")
    _bound(nerr(e, e64), a_e, "sentence vectors on the HIP route")
    _bound(nerr(e_aten, e64), a_e, "sentence vectors on the ATen route on the GPU")
    _bound(nerr(h[rows], h_aten[rows].double()), nerr(h_aten[rows], f64) + a_h, "HIP against ATen, valid rows")
    assert float((e.norm(dim=1) - 1).abs().max()) < 1e-6


def left_padded(tok):
    ids, mask = tok["input_ids"], tok["attention_mask"]
    T = ids.shape[1]
    out_ids, out_mask = torch.ones_like(ids), torch.zeros_like(mask)                   # <pad> is id 1
    for b, n in enumerate(mask.sum(1).tolist()):
        out_ids[b, T - n:] = ids[b, :n]
        out_mask[b, T - n:] = 1
    return {"input_ids": out_ids, "attention_mask": out_mask}


def test_other_masks_hooks_and_autograd_take_aten(du, model, fixture, dev, monkeypatch):
    z, _ = fixture
    tok = batch(z, dev)
    f64, e64 = torch.from_numpy(z["hidden_f64"]), torch.from_numpy(z["embed_f64"])
    a_h, a_e = nerr(torch.from_numpy(z["hidden_f32"]), f64), nerr(torch.from_numpy(z["embed_f32"]), e64)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    # a batch that is not right-padded: ATen throughout (the position ids follow the tokens, the distances are the same), and the
    # valid rows -- sequence after sequence, as the fixture stores them -- still match
    left = left_padded(tok)
    with torch.no_grad():
        h = model(left)
        e = model.embed(left)
    assert calls.n == {} and calls.sdpa == 4
    _bound(nerr(h[left["attention_mask"].bool()], f64), a_h, "left-padded batch, valid rows")
    _bound(nerr(e, e64), a_e, "left-padded batch, sentence vectors")
    # a hook inside layer 0: that layer runs its ATen modules (the hook fires), layer 1 stays on the HIP route
    calls.reset()
    seen = []
    handle = model.encoder.layer[0].attention.attn.o.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    try:
        with torch.no_grad():
            e = model.embed(tok)
    finally:
        handle.remove()
    assert seen == [(12, 27, 128)] and calls.sdpa == 1
    assert calls.n == {"text_embed_ln": 1, "vit_attention_relbias": 1, "layer_norm": 2, "masked_mean_l2": 1}
    _bound(nerr(e, e64), a_e, "layer 0 on ATen, layer 1 on the HIP route")
    # no mask: every token is a key.  Ids that hold <pad> go to ATen (MPNet gives those tokens position row 1, K24 would give
    # them row t + 2); ids without one take the HIP route, and both agree with the masked batch's full-length sequence
    calls.reset()
    with torch.no_grad():
        model({"input_ids": tok["input_ids"]})
        assert calls.n == {} and calls.sdpa == 2
        calls.reset()
        full = int(tok["attention_mask"].sum(1).argmax())
        assert int(tok["attention_mask"][full].sum()) == tok["input_ids"].shape[1]
        e1 = model.embed({"input_ids": tok["input_ids"][full:full + 1]})
        assert calls.n == {"text_embed_ln": 1, "vit_attention_relbias": 2, "layer_norm": 4, "masked_mean_l2": 1} and calls.sdpa == 0
    _bound(nerr(e1, e64[full:full + 1]), a_e, "no mask, no padding: the HIP route")
    # autograd: ATen
    calls.reset()
    h = model(tok)
    assert h.requires_grad and calls.n == {} and calls.sdpa == 2


def test_encode_on_the_gpu(du, model, fixture, dev, monkeypatch):
    z, meta = fixture
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    du.register_tokenizer("mpnet", VOCAB)
    monkeypatch.setattr(model, "tokenizer", None)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    a = model.encode(meta["strings"], batch_size=5)
    assert calls.n["masked_mean_l2"] == 3 and calls.n["vit_attention_relbias"] == 6 and calls.sdpa == 0
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (12, 128)
    e64 = torch.from_numpy(z["embed_f64"])
    a_e = nerr(torch.from_numpy(z["embed_f32"]), e64)
    _bound(nerr(torch.from_numpy(a), e64), a_e, "encode() on the HIP route")
    # Another batch size: other paddings and other batch neighbours.  K9B and K27 give a valid row the same bits whatever its
    # batch (the kernel tests above); the GEMMs between them run at another row count, where hipBLASLt may cut K differently,
    # so the rows are not claimed bit-equal: every batch size is held to the fixture's bound, in input order.
    order = [7, 0, 11, 3, 3, 1]
    for bs in (1, 12):
        b = model.encode(meta["strings"], batch_size=bs)
        print("batch_size %d against 5: max |diff| %.3e, bit-equal rows %d of 12" % (bs, float(np.abs(a - b).max()),
                                                                                  int((a == b).all(axis=1).sum())))
        _bound(nerr(torch.from_numpy(b), e64), a_e, "encode(batch_size=%d) on the HIP route" % bs)
    c = model.encode([meta["strings"][i] for i in order], batch_size=4)
    _bound(nerr(torch.from_numpy(c), e64[order]), a_e, "encode() of a reordered list")
    assert calls.sdpa == 0


def test_get_cos_similarity_on_the_gpu_is_its_cpu_value(mcd, du, model, fixture, dev, monkeypatch):
    """Both cosines on the GPU (OpenAIClip on K9A / K25, the sentence encoder on K9B / K27) against the float64 value, held to
    twice the error of the CPU run of the same function."""
    from mammo_clip_dissect_amd.concept_vit import utils
    z, meta = fixture
    strings = meta["strings"]
    preds, gt = strings, strings[3:] + strings[:3]
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    du.register_tokenizer("mpnet", VOCAB)
    du.register_tokenizer("clip", clip_recipe.BPE_SMALL)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    clip_cpu = du.OpenAIClip(**clip_recipe.SMALL).eval()
    clip_recipe.fill(clip_cpu)
    clip_gpu = du.OpenAIClip(**clip_recipe.SMALL).eval()
    clip_gpu.load_state_dict(clip_cpu.state_dict())
    clip_gpu.to(dev)
    cpu_model = du.sentence_encoder("cpu", ckpt=state_dict(z))
    calls = Calls(du, monkeypatch)
    gpu = utils.get_cos_similarity(preds, gt, clip_gpu, model, device=dev)
    assert calls.n.get("masked_mean_l2") == 2 and calls.n.get("vit_attention_relbias") == 4
    cpu = utils.get_cos_similarity(preds, gt, clip_cpu, cpu_model, device="cpu")
    assert all(type(v) is float for v in gpu + cpu)
    # float64: the sentence side from the fixture, the CLIP side from the same model in double
    e64 = z["embed_f64"]
    order = list(range(3, 12)) + [0, 1, 2]
    want_mpnet = float(np.mean(np.sum(e64 * e64[order], axis=1)))
    tok = du.clip_tokenizer()
    clip64 = clip_cpu.double()
    with torch.no_grad():
        p = clip64.encode_text(tok(preds, context_length=77))
        g = clip64.encode_text(tok(gt, context_length=77))
    want_clip = float(((p / p.norm(dim=-1, keepdim=True)) * (g / g.norm(dim=-1, keepdim=True))).sum(1).mean())
    _bound(abs(gpu[0] - want_clip), abs(cpu[0] - want_clip), "CLIP cosine, GPU against CPU")
    _bound(abs(gpu[1] - want_mpnet), abs(cpu[1] - want_mpnet), "sentence cosine, GPU against CPU")
    one = utils.get_cos_similarity(preds, preds, clip_gpu, model, device=dev)
    assert abs(one[0] - 1) <= 2.4e-5 and abs(one[1] - 1) <= 2.4e-5, one              # test_mpnet_cpu.UNIT_DOT_TOL
