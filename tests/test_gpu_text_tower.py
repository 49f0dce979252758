"""GPU: the text side's two entries (include/mcd_text.h) and the BERT tower's HIP route.

K9M (mcd_vit_attention_keylen) against float64 at the project's bound, its bit-for-bit rule (rows < L are K9's on the
truncated sequence; lens NULL is K9; the clamp), its independence of everything past L; K24 (mcd_text_embed_ln) on the bits of
K10 over ATen's sum; both on torch's current stream with their operands in the guarded, pre-filled frames of util.py, and both
held to the stream and capture contracts of test_gpu_stream_contracts.py (its own machinery, on rows of this file's).  Then
BertTextTower's HIP route on the fixture's ragged batch against transformers' float64 output, the route's switches by counted
calls, and describe_broad_neurons.main with a checkpoint made from the recipe and the registered vocabulary."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_encoder_frames as EF
import test_gpu_stream_contracts as S
import text_recipe as recipe
import util
from util import int_bits, nerr

pytestmark = pytest.mark.gpu

NAN = float("nan")
VOCAB = os.path.join(util.GOLDEN, "text_vocab.txt")
LENS_GAP = 1 << 20          # what surrounds lens in its frame: a neighbour read as a length would be clamped to T -- and show


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


def _bound(e_hip, e_aten, what):       # test_gpu_clip_rn's
    print("%s: hip %.3e aten %.3e ratio to the bound %.3f" % (what, e_hip, e_aten, e_hip / (2 * e_aten + 1e-6)))
    assert e_hip <= 2 * e_aten + 1e-6, (what, e_hip, e_aten)


def k9(L, qkv, H):
    B, T, _ = qkv.shape
    out = torch.empty(B, T, H * 64, device=qkv.device)
    EF.ok(L.mcd_vit_attention(qkv.data_ptr(), B, T, H, out.data_ptr(), EF.st()), L)
    return out


def k9m(L, qkv, H, lens, gap=NAN):
    """K9M on framed operands: qkv and lens inside guards of `gap` / LENS_GAP, the output in a frame of OUT_FILL whose guards
    must come back intact and whose every element must have been written; the inputs untouched.  Returns the output."""
    B, T, _ = qkv.shape
    q_ = EF.In(qkv, gap)
    l_ = None if lens is None else EF.In(torch.tensor(lens, dtype=torch.int32, device=qkv.device), LENS_GAP)
    o_ = EF.Out((B, T, H * 64), qkv.device)
    EF.ok(L.mcd_vit_attention_keylen(q_.ptr, B, T, H, None if l_ is None else l_.ptr, o_.ptr, EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K9M", tuple(qkv.shape), lens))          # the guards
    assert not bool((int_bits(out) == int(int_bits(torch.full((1,), util.OUT_FILL))[0])).any()), "an output element was not written"
    q_.same()
    if l_ is not None:
        l_.same()
    return out


def reference64(qkv, H, lens):
    """softmax over the first lens[b] keys, every query row, in float64 on the host."""
    B, T, _ = qkv.shape
    q, k, v = qkv.double().cpu().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    keep = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, H * 64)


def sdpa(qkv, H, lens):
    B, T, _ = qkv.shape
    q, k, v = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    keep = (torch.arange(T, device=qkv.device)[None, :] < torch.tensor(lens, device=qkv.device)[:, None])[:, None, None, :]
    return F.scaled_dot_product_attention(q, k, v, attn_mask=keep).transpose(1, 2).reshape(B, T, H * 64)


# ---- K9M -----------------------------------------------------------------------------------------------------------------
# (B, T, H, lens): one key; odd sizes under one tile; a last tile of 1 key, whole tiles, a short one and a single key beside
# them (the padded tile skipped); two waves of queries over 1 - 3 key tiles; 8 heads with a 9-key sequence in a 77-token
# batch; the 8-wave maximum with 8, 8 and 1 key tiles
K9M_CASES = [(1, 1, 1, [1]), (3, 7, 2, [7, 4, 3]), (4, 33, 2, [33, 32, 31, 1]), (5, 65, 1, [65, 64, 33, 32, 2]),
             (2, 77, 8, [77, 9]), (3, 256, 2, [256, 255, 1])]
_K9M = {}


def k9m_case(L, dev, case):
    """(qkv, the framed K9M output) of a case, computed once and left unchanged."""
    if case not in _K9M:
        B, T, H, lens = K9M_CASES[case]
        qkv = EF.rnd((B, T, 3 * H * 64), 100 + T + H, dev)
        _K9M[case] = (qkv, k9m(L, qkv, H, lens))
    return _K9M[case]


@pytest.mark.parametrize("case", range(len(K9M_CASES)), ids=lambda c: "B%d-T%d-H%d" % K9M_CASES[c][:3])
def test_k9m_against_float64(L, dev, case):
    B, T, H, lens = K9M_CASES[case]
    qkv, out = k9m_case(L, dev, case)
    ref = reference64(qkv, H, lens)
    _bound(nerr(out, ref), nerr(sdpa(qkv, H, lens), ref), ("K9M", K9M_CASES[case]))


@pytest.mark.parametrize("case", range(len(K9M_CASES)), ids=lambda c: "B%d-T%d-H%d" % K9M_CASES[c][:3])
def test_k9m_valid_rows_are_k9_on_the_truncated_sequence(L, dev, case):
    B, T, H, lens = K9M_CASES[case]
    qkv, out = k9m_case(L, dev, case)
    for b, n in enumerate(lens):
        want = k9(L, qkv[b:b + 1, :n].contiguous(), H)
        assert torch.equal(int_bits(out[b:b + 1, :n]), int_bits(want)), (K9M_CASES[case], "sequence %d" % b)


def test_k9m_without_lens_is_k9(L, dev):
    B, T, H = 2, 197, 3
    qkv = EF.rnd((B, T, 3 * H * 64), 5, dev)
    assert torch.equal(int_bits(k9m(L, qkv, H, None)), int_bits(k9(L, qkv, H)))


def test_k9m_clamps_the_lengths(L, dev):
    B, T, H = 1, 33, 2
    qkv = EF.rnd((B, T, 3 * H * 64), 6, dev)
    assert torch.equal(int_bits(k9m(L, qkv, H, [0])), int_bits(k9m(L, qkv, H, [1])))
    assert torch.equal(int_bits(k9m(L, qkv, H, [-7])), int_bits(k9m(L, qkv, H, [1])))
    assert torch.equal(int_bits(k9m(L, qkv, H, [T + 5])), int_bits(k9m(L, qkv, H, [T])))
    assert not torch.equal(int_bits(k9m(L, qkv, H, [1])), int_bits(k9m(L, qkv, H, [T])))


@pytest.mark.parametrize("case", [2, 3], ids=["T33", "T65"])
def test_k9m_reads_nothing_past_the_length(L, dev, case):
    """NaN in every K and V row >= L: the output bits do not move.  One NaN in a padded query row: that output row of that
    head is NaN and nothing else changes."""
    B, T, H, lens = K9M_CASES[case]
    qkv, out = k9m_case(L, dev, case)
    W = H * 64
    poisoned = qkv.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:, W:] = NAN                        # k and v of the padded tokens
    assert torch.equal(int_bits(k9m(L, poisoned, H, lens)), int_bits(out)), "a padded K or V row reached the output"
    b = max(range(B), key=lambda i: T - lens[i])         # the sequence with the most padding
    t, h = lens[b], H - 1                                # its first padded query row
    assert t < T
    one = qkv.clone()
    one[b, t, h * 64 + 17] = NAN
    got = k9m(L, one, H, lens)
    assert bool(torch.isnan(got[b, t, h * 64:(h + 1) * 64]).all())
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[b, t, h * 64:(h + 1) * 64] = False
    assert torch.equal(int_bits(got)[keep], int_bits(out)[keep]), "the NaN of a padded query row reached another row"


def test_k9m_binding(core, L, dev):
    B, T, H, lens = K9M_CASES[1]
    qkv, out = k9m_case(L, dev, 1)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    assert torch.equal(int_bits(core.vit_attention_keylen(qkv, H, ld)), int_bits(out))
    into = torch.empty_like(out)
    assert core.vit_attention_keylen(qkv, H, None, out=into) is into and torch.equal(int_bits(into), int_bits(k9(L, qkv, H)))
    for bad in (ld.long(), ld[:2], ld.cpu()):
        with pytest.raises(TypeError):
            core.vit_attention_keylen(qkv, H, bad)
    with pytest.raises(ValueError):
        core.vit_attention_keylen(qkv, H + 1, ld)


# ---- K24 -----------------------------------------------------------------------------------------------------------------
K24_SHAPES = [(1, 1, 4), (21, 7, 128), (6, 3, 768), (5, 5, 2048)]       # (rows, T, D): every register count's ends, 7 waves
VOCAB_N, N_TYPE, EPS = 11, 2, 1e-12


def k24_operands(shape, dev):
    rows, T, D = shape
    g = torch.Generator().manual_seed(rows * 1000 + D)
    ids = torch.randint(0, VOCAB_N, (rows // T, T), generator=g).to(dev)
    tids = torch.randint(0, N_TYPE, (rows // T, T), generator=g).to(dev)
    tabs = [EF.rnd((n, D), 7 + n + D, dev) for n in (VOCAB_N, T + 2, N_TYPE)]
    gamma, beta = EF.rnd((D,), 3 + D, dev, 0.2, 1.0), EF.rnd((D,), 4 + D, dev, 0.1)
    return ids, tids, tabs, gamma, beta


def k24(L, ids, tids, tabs, gamma, beta, vocab=VOCAB_N, n_type=N_TYPE):
    """K24 on framed operands (tables, gamma, beta and the ids inside guards; the tables' NaN gaps would show in the output if a
    clamped-away id were read); returns the output after the frame's guards and the inputs have been checked."""
    B, T = ids.shape
    D = tabs[0].shape[1]
    fi = [EF.In(t, NAN) for t in tabs + [gamma, beta]]
    ii = [EF.In(ids, -1), None if tids is None else EF.In(tids, -1)]
    o_ = EF.Out((B, T, D), ids.device)
    EF.ok(L.mcd_text_embed_ln(ii[0].ptr, None if ii[1] is None else ii[1].ptr, fi[0].ptr, fi[1].ptr, fi[2].ptr, fi[3].ptr, fi[4].ptr,
                              EPS, B * T, T, D, vocab, n_type, o_.ptr, EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K24", (B * T, T, D)))
    for a in fi + ii:
        if a is not None:
            a.same()
    return out


def k24_expected(core, ids, tids, tabs, gamma, beta):
    word, pos, typ = tabs
    T = ids.shape[1]
    t = typ[torch.zeros_like(ids)] if tids is None else typ[tids]
    return core.layer_norm(((word[ids] + t) + pos[torch.arange(T, device=ids.device)][None]).contiguous(), gamma, beta, EPS)


@pytest.mark.parametrize("with_types", [False, True], ids=["type_ids-NULL", "type_ids"])
@pytest.mark.parametrize("shape", K24_SHAPES)
def test_k24_bits_are_k10_on_the_aten_sum(L, core, dev, shape, with_types):
    ids, tids, tabs, gamma, beta = k24_operands(shape, dev)
    tids = tids if with_types else None
    want = k24_expected(core, ids, tids, tabs, gamma, beta)
    got = k24(L, ids, tids, tabs, gamma, beta)
    assert torch.equal(int_bits(got), int_bits(want)), shape
    assert torch.equal(int_bits(core.text_embed_ln(ids, tids, *tabs, gamma, beta, EPS)), int_bits(want))
    ref = F.layer_norm(((tabs[0][ids] + (tabs[2][tids] if with_types else tabs[2][0])) + tabs[1][:ids.shape[1]]).double(),
                       (shape[2],), gamma.double(), beta.double(), EPS)
    assert nerr(got, ref) <= 2e-6                                   # and K10's own accuracy contract, against float64


def test_k24_clamps_ids_and_reads_nothing_out_of_range(L, core, dev):
    shape = (21, 7, 128)
    ids, tids, tabs, gamma, beta = k24_operands(shape, dev)
    bad_ids, bad_t = ids.clone(), tids.clone()
    bad_ids[0, 0], bad_ids[1, 3], bad_ids[2, 6] = -1, VOCAB_N, 1 << 40
    bad_t[0, 1], bad_t[2, 2] = -1, N_TYPE
    want = k24_expected(core, bad_ids.clamp(0, VOCAB_N - 1), bad_t.clamp(0, N_TYPE - 1), tabs, gamma, beta)
    got = k24(L, bad_ids, bad_t, tabs, gamma, beta)                 # (the NaN gaps around the tables: none of them was read)
    assert torch.equal(int_bits(got), int_bits(want)) and bool(torch.isfinite(got).all())
    # the binding refuses such ids while they are on the host, and a T past the position table anywhere
    for ids_, t_ in ((bad_ids.cpu(), tids.cpu()), (ids.cpu(), bad_t.cpu())):
        with pytest.raises(ValueError, match=r"outside \[0, "):
            core.text_embed_ln(ids_, t_, *tabs, gamma, beta, EPS)
    with pytest.raises(ValueError, match="position table has 9 rows"):
        core.text_embed_ln(torch.zeros(1, 10, dtype=torch.long, device=dev), None, *tabs, gamma, beta, EPS)
    host = core.text_embed_ln(ids.cpu(), tids.cpu(), *tabs, gamma, beta, EPS)          # host ids in range: moved, then run
    assert torch.equal(int_bits(host), int_bits(k24_expected(core, ids, tids, tabs, gamma, beta)))


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery -------------------------------------------------
def b_keylen(L, dev):
    B, T, H = 3, 40, 1
    lens = lambda s: torch.tensor([[40, 33, 1], [7, 40, 32]][s % 2], dtype=torch.int32)      # fresh lengths are part of the data
    return S.simple(L, dev, "K9M", [S._gen((B, T, 3 * H * 64)), lens], [(B, T, H * 64)],
                    lambda i, o, st: L.mcd_vit_attention_keylen(i[0], B, T, H, i[1], o[0], st))


def b_text_embed(L, dev):
    rows, T, D, V = 6, 3, 8, 5
    ids = lambda s: torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(s))
    return S.simple(L, dev, "K24", [ids, S._gen((V, D)), S._gen((T, D)), S._gen((2, D)), S._gen((D,)), S._gen((D,))], [(rows, D)],
                    lambda i, o, st: L.mcd_text_embed_ln(i[0], None, i[1], i[2], i[3], i[4], i[5], 1e-12, rows, T, D, V, 2, o[0], st))


TEXT_STREAM_ROWS = {"mcd_vit_attention_keylen": b_keylen, "mcd_text_embed_ln": b_text_embed}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(TEXT_STREAM_ROWS) == sorted(mcd._lib.TEXT_SIGNATURES)


@pytest.fixture(scope="module")
def spin_cycles(dev):
    """A spin of at least S.MIN_SPIN_MS (both entries run in well under a millisecond), in the cycles of torch.cuda._sleep."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 20_000_000
    for _ in range(4):
        torch.cuda.synchronize()
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        e1.synchronize()
        real = e0.elapsed_time(e1)
        if S.MIN_SPIN_MS <= real <= 4 * S.MIN_SPIN_MS:
            break
        cycles = int(cycles * 2 * S.MIN_SPIN_MS / max(real, 1e-3))
    assert real >= S.MIN_SPIN_MS
    return cycles


@pytest.mark.parametrize("entry", sorted(TEXT_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):
    r = S.Run(entry, TEXT_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)      # (the control -- a launch on another stream IS seen -- is test_gpu_stream_contracts.py's)


@pytest.mark.parametrize("entry", sorted(TEXT_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    r = S.Run(entry, TEXT_STREAM_ROWS[entry](L, dev), dev)
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


# ---- the tower -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "text_tower.npz")), json.load(open(os.path.join(util.GOLDEN, "text_tower_meta.json")))


@pytest.fixture(scope="module")
def bert_clip(du, dev):
    sd, _ = recipe.weights()
    model, _ = du.get_target_model("breastclip_vit", dev, ckpt={"model": sd})
    assert model.text_tower == "bert"
    return model


def tower_batch(z, dev):
    rows, T = z["tower_rows"].astype(np.int64), int(z["tower_T"])
    return {k: torch.from_numpy(z[k + "_256"].astype(np.int64)[rows][:, :T].copy()).to(dev)
            for k in ("input_ids", "token_type_ids", "attention_mask")}


class Calls(util.CallCounter):
    """util.CallCounter on the text route's wrappers, and the SDPA calls beside them."""

    def __init__(self, du, monkeypatch):
        super().__init__(du.core, monkeypatch, ["text_embed_ln", "vit_attention_keylen", "layer_norm"])
        self.sdpa = 0
        fn = F.scaled_dot_product_attention

        def wrap(*a, **kw):
            self.sdpa += 1
            return fn(*a, **kw)
        monkeypatch.setattr(du.F, "scaled_dot_product_attention", wrap)


def test_tower_hip_route_against_float64(du, bert_clip, fixture, dev, monkeypatch):
    z, _ = fixture
    tok = tower_batch(z, dev)
    assert len(set(tok["attention_mask"].sum(1).tolist())) > 4           # a ragged batch
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    with torch.no_grad():
        h = bert_clip.text_encoder(tok)
        f = bert_clip.text_projection(bert_clip.encode_text(tok))
    assert calls.n == {"text_embed_ln": 2, "vit_attention_keylen": 4, "layer_norm": 8} and calls.sdpa == 0   # two forwards
    f64 = torch.from_numpy(z["hidden_f64"])
    _bound(nerr(h, f64), nerr(torch.from_numpy(z["hidden_f32"]), f64), "last_hidden_state on the HIP route")
    g64 = torch.from_numpy(z["feat_eos_f64"])
    _bound(nerr(f, g64), nerr(torch.from_numpy(z["feat_eos_f32"]), g64), "projected eos features on the HIP route")


def test_tower_switch_mask_and_hooks_take_aten(du, bert_clip, fixture, dev, monkeypatch):
    z, _ = fixture
    tok = tower_batch(z, dev)
    f64 = torch.from_numpy(z["hidden_f64"])
    e_aten = nerr(torch.from_numpy(z["hidden_f32"]), f64)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    tower = bert_clip.text_encoder.text_encoder
    # MCD_NO_HIP_TEXT=1 (the module flag it sets): ATen everywhere, SDPA under the mask
    calls = Calls(du, monkeypatch)
    monkeypatch.setattr(du, "HIP_TEXT", False)
    with torch.no_grad():
        h = bert_clip.text_encoder(tok)
    assert calls.n == {} and calls.sdpa == 2
    _bound(nerr(h, f64), e_aten, "the ATen route on the GPU")
    monkeypatch.setattr(du, "HIP_TEXT", True)
    # a mask that is no prefix mask: K24 still writes the embedding rows, every layer takes SDPA
    holed = dict(tok, attention_mask=tok["attention_mask"].clone())
    holed["attention_mask"][0, 1] = 0
    calls.n.clear()
    calls.sdpa = 0
    with torch.no_grad():
        tower(holed)
    assert calls.n == {"text_embed_ln": 1} and calls.sdpa == 2
    # a hook inside layer 0: that layer runs its ATen modules (the hook fires), layer 1 stays on the HIP route
    seen = []
    handle = tower.encoder.layer[0].attention.output.dense.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    calls.n.clear()
    calls.sdpa = 0
    try:
        with torch.no_grad():
            h = tower(tok)
    finally:
        handle.remove()
    assert seen == [tuple(f64.shape)] and calls.sdpa == 1
    assert calls.n == {"text_embed_ln": 1, "vit_attention_keylen": 1, "layer_norm": 2}
    _bound(nerr(h, f64), e_aten, "layer 0 on ATen, layer 1 on the HIP route")


# ---- the driver ------------------------------------------------------------------------------------------------------------
def test_describe_broad_neurons_with_a_bert_checkpoint(du, fixture, dev, tmp_path, monkeypatch):
    """describe_broad_neurons.main, one layer, 16 synthetic images: the checkpoint's text keys select the BERT tower, the
    registered vocabulary its tokenizer, and the text cache holds the fixture's projected eos features."""
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    z, _ = fixture
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    monkeypatch.delenv("MCD_BERT_VOCAB", raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    du.register_tokenizer("bert", VOCAB)
    rows = [j for j, i in enumerate(z["tower_rows"])                    # the strings that are one plain line of a concept file
            if recipe.STRINGS[i] and recipe.STRINGS[i].isprintable() and recipe.STRINGS[i].isascii()]
    assert len(rows) >= 16
    concepts = tmp_path / "fixture_concepts.txt"
    concepts.write_text("\n".join(recipe.STRINGS[z["tower_rows"][j]] for j in rows) + "\n", encoding="utf-8")
    sd, _ = recipe.weights()
    sd = dict(sd, **recipe.image_projection(2048))
    ckpt = tmp_path / "mammo_clip.tar"
    torch.save({"model": sd}, str(ckpt))
    act, res = str(tmp_path / "acts"), str(tmp_path / "results")
    out = drv.main(["--target_model", "breastclip", "--target_layers", "image_encoder._blocks[0]", "--d_probe", "synthetic_16",
                    "--concept_set", str(concepts), "--batch_size", "8", "--top_k", "8", "--device", str(dev),
                    "--activation_dir", act, "--result_dir", res, "--Breast_clip_chkpt", str(ckpt)])
    assert len(glob.glob(os.path.join(out, "*.csv"))) == 1
    cache = glob.glob(os.path.join(act, "**", "*fixture_concepts_*.pt"), recursive=True)
    assert len(cache) == 1, os.listdir(act)
    got = torch.load(cache[0], map_location="cpu", weights_only=True)
    f64 = torch.from_numpy(z["feat_eos_f64"][rows])
    assert tuple(got.shape) == tuple(f64.shape)
    _bound(nerr(got, f64), nerr(torch.from_numpy(z["feat_eos_f32"][rows]), f64), "the driver's text cache")
