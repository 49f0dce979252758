"""GPU: the two OpenAI-CLIP entries (include/mcd_clip.h) and OpenAIClip's HIP route.

K9A (mcd_vit_attention_causal) against float64 at the project's bound, its bit-for-bit rule (row t is K9's on the sequence
truncated to t + 1 tokens), its independence of batch neighbours and of every tile above the diagonal; K25 (mcd_quick_gelu)
against float64, on its tail sizes, on the ends of the fp32 range and in place; both on torch's current stream with their
operands in the guarded, pre-filled frames of util.py, and both held to the stream and capture contracts of
test_gpu_stream_contracts.py (its own machinery, on rows of this file's).  Then both towers of OpenAIClip on the fixture of
tests/golden/openai_clip.npz against the reference's float64 outputs, the route's switches by counted calls, and
og_utils.save_activations with a synthesized OpenAI-format checkpoint as --clip_model."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import openai_clip_recipe as recipe
import test_gpu_encoder_frames as EF
import test_gpu_stream_contracts as S
import util
from util import int_bits, nerr

pytestmark = pytest.mark.gpu

NAN = float("nan")


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


def _bound(e_hip, e_aten, what):       # test_gpu_text_tower's
    print("%s: hip %.3e aten %.3e ratio to the bound %.3f" % (what, e_hip, e_aten, e_hip / (2 * e_aten + 1e-6)))
    assert e_hip <= 2 * e_aten + 1e-6, (what, e_hip, e_aten)


def all_written(out):
    fill = int(int_bits(torch.full((1,), util.OUT_FILL))[0])
    return not bool((int_bits(out) == fill).any())


def k9(L, qkv, H):
    B, T, _ = qkv.shape
    out = torch.empty(B, T, H * 64, device=qkv.device)
    EF.ok(L.mcd_vit_attention(qkv.data_ptr(), B, T, H, out.data_ptr(), EF.st()), L)
    return out


def k9a(L, qkv, H, gap=NAN):
    """K9A on framed operands: qkv inside guards of `gap`, the output in a frame of OUT_FILL whose guards must come back
    intact and whose every element must have been written; the input untouched.  Returns the output."""
    B, T, _ = qkv.shape
    q_ = EF.In(qkv, gap)
    o_ = EF.Out((B, T, H * 64), qkv.device)
    EF.ok(L.mcd_vit_attention_causal(q_.ptr, B, T, H, o_.ptr, EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K9A", tuple(qkv.shape)))            # the guards
    assert all_written(out), "an output element was not written"
    q_.same()
    return out


def reference64(qkv, H):
    """softmax over keys 0 .. t for query t, in float64 on the host."""
    B, T, _ = qkv.shape
    q, k, v = qkv.double().cpu().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, H * 64)


def sdpa_causal(qkv, H):
    B, T, _ = qkv.shape
    q, k, v = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, H * 64)


# ---- K9A -----------------------------------------------------------------------------------------------------------------
# (B, T, H): one token; odd sizes under one tile; one whole tile; a second wave of one query; two whole tiles; a third wave
# of one query; CLIP's own 77 tokens with 8 heads; the 8-wave maximum
K9A_CASES = [(1, 1, 1), (3, 7, 2), (2, 32, 1), (2, 33, 2), (2, 64, 1), (2, 65, 1), (2, 77, 8), (1, 256, 2)]
_K9A = {}


def k9a_case(L, dev, case):
    """(qkv, the framed K9A output) of a case, computed once and left unchanged."""
    if case not in _K9A:
        B, T, H = K9A_CASES[case]
        qkv = EF.rnd((B, T, 3 * H * 64), 300 + T + H, dev)
        _K9A[case] = (qkv, k9a(L, qkv, H))
    return _K9A[case]


CASE_IDS = ["B%d-T%d-H%d" % c for c in K9A_CASES]


@pytest.mark.parametrize("case", range(len(K9A_CASES)), ids=CASE_IDS)
def test_k9a_against_float64(L, dev, case):
    B, T, H = K9A_CASES[case]
    qkv, out = k9a_case(L, dev, case)
    ref = reference64(qkv, H)
    _bound(nerr(out, ref), nerr(sdpa_causal(qkv, H), ref), ("K9A", K9A_CASES[case]))


@pytest.mark.parametrize("case", range(len(K9A_CASES)), ids=CASE_IDS)
def test_k9a_row_t_is_k9_on_the_sequence_truncated_to_t_plus_1(L, dev, case):
    B, T, H = K9A_CASES[case]
    qkv, out = k9a_case(L, dev, case)
    for t in sorted({0, 1, 31, 32, 33, 63, 64, T - 1} & set(range(T))):
        want = k9(L, qkv[:, :t + 1].contiguous(), H)[:, t]
        assert torch.equal(int_bits(out[:, t]), int_bits(want)), (K9A_CASES[case], "row %d" % t)


@pytest.mark.parametrize("case", [1, 5, 6], ids=[CASE_IDS[i] for i in (1, 5, 6)])
def test_k9a_a_sequence_does_not_see_its_batch_neighbours(L, dev, case):
    B, T, H = K9A_CASES[case]
    qkv, out = k9a_case(L, dev, case)
    for b in range(B):
        assert torch.equal(int_bits(k9a(L, qkv[b:b + 1].contiguous(), H)), int_bits(out[b:b + 1])), (K9A_CASES[case], b)


@pytest.mark.parametrize("case,first", [(6, 64), (5, 64)], ids=["T77-tokens-64..76", "T65-token-64"])
def test_k9a_never_touches_a_tile_above_the_diagonal(L, dev, case, first):
    """NaN in q, k and v of every token of the last 32-key tile: the rows of the earlier query blocks carry the clean
    run's bits (their waves stop at their own tile); the poisoned block's rows are NaN."""
    B, T, H = K9A_CASES[case]
    qkv, out = k9a_case(L, dev, case)
    poisoned = qkv.clone()
    poisoned[:, first:] = NAN
    got = k9a(L, poisoned, H)
    assert torch.equal(int_bits(got[:, :first]), int_bits(out[:, :first])), "a tile above the diagonal reached an earlier row"
    assert bool(torch.isnan(got[:, first:]).all())


def test_k9a_refuses_bad_arguments_and_writes_nothing(L, dev):
    B, T, H = 1, 8, 1
    qkv = EF.In(EF.rnd((B, T, 3 * H * 64), 1, dev), NAN)
    out = EF.Out((B, 257, H * 64), dev)
    for args, code in (((qkv.ptr, B, 0, H, out.ptr), -1), ((qkv.ptr, B, 257, H, out.ptr), -5), ((qkv.ptr, B, T, 0, out.ptr), -1),
                       ((qkv.ptr + 4, B, T, H, out.ptr), -1), ((qkv.ptr, B, T, H, out.ptr + 8), -1),
                       ((None, B, T, H, out.ptr), -1)):
        assert L.mcd_vit_attention_causal(*args, EF.st()) == code, args
    torch.cuda.synchronize()
    assert bool((out.flat == util.OUT_FILL).all())
    qkv.same()


def test_k9a_binding(core, L, dev):
    B, T, H = K9A_CASES[3]
    qkv, out = k9a_case(L, dev, 3)
    assert torch.equal(int_bits(core.vit_attention_causal(qkv, H)), int_bits(out))
    into = torch.empty_like(out)
    assert core.vit_attention_causal(qkv, H, out=into) is into and torch.equal(int_bits(into), int_bits(out))
    with pytest.raises(ValueError):
        core.vit_attention_causal(qkv, H + 1)
    with pytest.raises(TypeError):
        core.vit_attention_causal(qkv.transpose(0, 1), H)


# ---- K25 -----------------------------------------------------------------------------------------------------------------
# nothing, a tail alone, one float4 (+ 1), odd counts inside one workgroup (256 lanes x 4 float4s = 4096 floats), then a
# whole workgroup plus a tail and three workgroups with a short last one
K25_SIZES = [0, 1, 3, 4, 5, 255, 1025, 64 * 4 * 5 + 3, 4096 + 3, 2 * 4096 + 4 * 300 + 1]
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 20.0, -20.0, 88.0, -88.0, 1e4, -1e4, 3e38, -3e38]


def gelu64(x):
    return x.double() * torch.sigmoid(1.702 * x.double())


def k25(L, x, in_place=False):
    """K25 on framed operands; in place, the frame is the input's own."""
    n = x.numel()
    if in_place:
        o_ = EF.Out((n,), x.device)
        o_.view.copy_(x)
        EF.ok(L.mcd_quick_gelu(o_.ptr, n, o_.ptr, EF.st()), L)
    else:
        x_ = EF.In(x, NAN)
        o_ = EF.Out((n,), x.device)
        EF.ok(L.mcd_quick_gelu(x_.ptr, n, o_.ptr, EF.st()), L)
        x_.same()
    out = o_.view.clone()
    o_.check(out, what=("K25", n, in_place))
    assert all_written(out)
    return out


def k25_input(n, dev):
    """Random data of a few units with the special values at its head (as many as fit)."""
    x = EF.rnd((n,), 40 + n, dev, 3.0)
    k = min(n, len(SPECIALS))
    x[:k] = torch.tensor(SPECIALS[:k], device=dev)
    return x


@pytest.mark.parametrize("n", K25_SIZES)
def test_k25_against_float64_and_in_place(L, dev, n):
    x = k25_input(n, dev)
    out = k25(L, x)
    assert torch.equal(int_bits(k25(L, x, in_place=True)), int_bits(out))
    if n == 0:
        return
    assert bool(torch.isfinite(out).all())
    ref = gelu64(x)
    _bound(nerr(out, ref), nerr(x * torch.sigmoid(1.702 * x), ref), ("K25", n))
    # without the special values of 20 and more (they set the scale of nerr above): the random data on its own scale
    body = x.abs() <= 10
    _bound(nerr(out[body], ref[body]), nerr((x * torch.sigmoid(1.702 * x))[body], ref[body]), ("K25 body", n))


def test_k25_special_values(L, dev):
    """Every finite input gives a finite result; a large negative one gives a zero of either sign.  For |x| <= 20 the
    result is within 1e-5 of float64, relatively: the exponent -1.702 x log2(e) is at most 2^6 and carries two fp32
    roundings (2 * 2^-24 * 49.1 * ln 2 = 4.1e-6 on the power), v_exp_f32, the add, the division and the product about an
    ulp each (4 * 6e-8)."""
    x = torch.tensor(SPECIALS + [-5.0, 5.0, -0.3], device=dev)
    out = k25(L, x)
    assert bool(torch.isfinite(out).all())
    ref = gelu64(x).cpu()
    got = out.double().cpu()
    xs = x.cpu()
    assert bool((got[xs <= -88] == 0).all()) and bool((got[xs == 0] == 0).all())
    big = xs >= 88
    assert torch.equal(out.cpu()[big], xs[big])
    small = (xs.abs() <= 20) & (xs.abs() >= 0.1)
    assert bool(((got[small] - ref[small]).abs() <= 1e-5 * ref[small].abs()).all()), (got[small], ref[small])
    tiny = xs.abs() == 1e-40                                  # a denormal: half of it, or a flushed zero
    assert bool((got[tiny].abs() <= 1e-40).all())


def test_k25_binding(core, L, dev):
    x = k25_input(1025, dev).view(25, 41)
    want = k25(L, x.reshape(-1)).view(25, 41)
    assert torch.equal(int_bits(core.quick_gelu(x)), int_bits(want))
    y = x.clone()
    assert core.quick_gelu(y, out=y) is y and torch.equal(int_bits(y), int_bits(want))
    with pytest.raises(TypeError):
        core.quick_gelu(x.t())
    with pytest.raises(TypeError):
        core.quick_gelu(x.double())


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery -------------------------------------------------
def b_causal(L, dev):
    B, T, H = 3, 40, 1
    return S.simple(L, dev, "K9A", [S._gen((B, T, 3 * H * 64))], [(B, T, H * 64)],
                    lambda i, o, st: L.mcd_vit_attention_causal(i[0], B, T, H, o[0], st))


def b_quick_gelu(L, dev):
    n = 1027
    return S.simple(L, dev, "K25", [S._gen((n,), 3.0)], [(n,)], lambda i, o, st: L.mcd_quick_gelu(i[0], n, o[0], st))


CLIP_STREAM_ROWS = {"mcd_vit_attention_causal": b_causal, "mcd_quick_gelu": b_quick_gelu}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(CLIP_STREAM_ROWS) == sorted(mcd._lib.CLIP_SIGNATURES)


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


@pytest.mark.parametrize("entry", sorted(CLIP_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):
    r = S.Run(entry, CLIP_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)      # (the control -- a launch on another stream IS seen -- is test_gpu_stream_contracts.py's)


@pytest.mark.parametrize("entry", sorted(CLIP_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    r = S.Run(entry, CLIP_STREAM_ROWS[entry](L, dev), dev)
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


# ---- the towers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "openai_clip.npz")), json.load(open(os.path.join(util.GOLDEN, "openai_clip_meta.json")))


@pytest.fixture(scope="module")
def clip(du, dev, fixture):
    m = du.OpenAIClip(**recipe.SMALL)
    assert recipe.fill(m) == fixture[1]["weights_sha256"]
    return m.to(dev).eval()


TEXT_HIP = {"vit_attention_causal": 2, "quick_gelu": 2, "layer_norm": 4}
# K11, ln_pre + two per block + ln_post on K10, K9 in block 0, the class-token tail of block 1 on K9C, K25 in both
IMAGE_HIP = {"patchify": 1, "layer_norm": 6, "vit_attention": 1, "vit_attention_cls": 1, "quick_gelu": 2}


class Calls(util.CallCounter):
    """util.CallCounter on the route's wrappers, and the SDPA calls beside them."""

    def __init__(self, du, monkeypatch):
        super().__init__(du.core, monkeypatch, ["vit_attention_causal", "quick_gelu", "layer_norm", "vit_attention",
                                                "vit_attention_long", "vit_attention_cls", "patchify"])
        self.sdpa = 0
        fn = F.scaled_dot_product_attention

        def wrap(*a, **kw):
            self.sdpa += 1
            return fn(*a, **kw)
        monkeypatch.setattr(du.F, "scaled_dot_product_attention", wrap)

    def clear(self):
        self.n.clear()
        self.sdpa = 0


def test_text_tower_hip_route_against_float64(du, clip, fixture, dev, monkeypatch):
    z, _ = fixture
    ids = torch.from_numpy(z["ids"].astype(np.int64)).to(dev)
    f64 = torch.from_numpy(z["text_f64"])
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    with torch.no_grad():
        hip = clip.encode_text(ids)
    assert calls.n == TEXT_HIP and calls.sdpa == 0
    calls.clear()
    monkeypatch.setattr(du, "HIP_CLIP_TEXT", False)
    with torch.no_grad():
        aten = clip.encode_text(ids)
    assert calls.n == {} and calls.sdpa == 2
    _bound(nerr(hip, f64), nerr(aten, f64), "encode_text on the HIP route")
    _bound(nerr(aten, f64), nerr(torch.from_numpy(z["text_f32"]), f64), "encode_text on the ATen route on the GPU")


def test_image_tower_hip_route_against_float64(du, clip, fixture, dev, monkeypatch):
    z, _ = fixture
    image = recipe.make_image().to(dev)
    f64 = torch.from_numpy(z["image_f64"])
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    with torch.no_grad():
        hip = clip.encode_image(image)
        assert torch.equal(clip(image), hip)
    assert calls.n == {k: 2 * v for k, v in IMAGE_HIP.items()} and calls.sdpa == 0          # two forwards
    calls.clear()
    monkeypatch.setattr(du, "HIP_CLIP_TEXT", False)
    with torch.no_grad():
        aten = clip.encode_image(image)
    assert calls.n == {} and calls.sdpa == 2
    _bound(nerr(hip, f64), nerr(aten, f64), "encode_image on the HIP route")
    _bound(nerr(aten, f64), nerr(torch.from_numpy(z["image_f32"]), f64), "encode_image on the ATen route on the GPU")


def test_block_rows_on_the_hip_route(du, clip, fixture, dev, monkeypatch):
    """The hook points: per block the class-token row (image; the pruned last block returns that row alone) and the
    end-of-text row (text), against the reference's float64 rows, the ATen route's error as the measure."""
    z, _ = fixture
    ids = torch.from_numpy(z["ids"].astype(np.int64)).to(dev)
    image = recipe.make_image().to(dev)
    eot = ids.argmax(-1)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")

    def run():
        rows, hooks = {}, []
        for i, blk in enumerate(clip.visual.transformer.resblocks):
            hook = lambda m, a, o, i=i: rows.__setitem__("img_block%d" % i, o[:, 0].clone())       # noqa: E731
            hook.token0_only = True
            hooks.append(blk.register_forward_hook(hook))
        for i, blk in enumerate(clip.transformer.resblocks):
            hooks.append(blk.register_forward_hook(
                lambda m, a, o, i=i: rows.__setitem__("txt_block%d" % i, o[torch.arange(o.shape[0], device=o.device), eot].clone())))
        with torch.no_grad():
            clip.encode_image(image)
            clip.encode_text(ids)
        for h in hooks:
            h.remove()
        return rows
    calls = Calls(du, monkeypatch)
    hip = run()
    assert calls.n == dict(IMAGE_HIP, **{k: v + IMAGE_HIP.get(k, 0) for k, v in TEXT_HIP.items()}) and calls.sdpa == 0
    monkeypatch.setattr(du, "HIP_CLIP_TEXT", False)
    aten = run()
    for k in sorted(hip):
        f64 = torch.from_numpy(z[k + "_f64"])
        _bound(nerr(hip[k], f64), nerr(aten[k], f64), k + " on the HIP route")


def test_switch_hooks_and_autograd_take_aten(du, clip, fixture, dev, monkeypatch):
    z, _ = fixture
    ids = torch.from_numpy(z["ids"].astype(np.int64)).to(dev)[:5]
    image = recipe.make_image().to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    with torch.no_grad():
        want_t, want_i = clip.encode_text(ids), clip.encode_image(image)
    # autograd on: ATen everywhere
    calls.clear()
    clip.encode_text(ids)
    clip.encode_image(image)
    assert calls.n == {} and calls.sdpa == 4
    # a hook inside block 0 of either tower: that block runs its ATen modules (the hook fires), block 1 stays on the HIP route
    for tower, run, arg, hip_rest in ((clip.transformer, clip.encode_text, ids, {"vit_attention_causal": 1, "quick_gelu": 1, "layer_norm": 2}),
                                      (clip.visual.transformer, clip.encode_image, image,
                                       {"patchify": 1, "layer_norm": 4, "vit_attention_cls": 1, "quick_gelu": 1})):
        seen = []
        handle = tower.resblocks[0].attn.out_proj.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
        calls.clear()
        try:
            with torch.no_grad():
                got = run(arg)
        finally:
            handle.remove()
        assert len(seen) == 1 and calls.sdpa == 1 and calls.n == hip_rest, (calls.n, calls.sdpa)
        want = want_t if arg is ids else want_i
        assert nerr(got, want) <= 1e-5
    # a hook on the last image block that reads every token: no class-token tail, the full block on K9
    handle = clip.visual.transformer.resblocks[1].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    calls.clear()
    try:
        with torch.no_grad():
            clip.encode_image(image)
    finally:
        handle.remove()
    assert seen[-1] == (recipe.BATCH, 17, 128) and calls.n == {"patchify": 1, "layer_norm": 6, "vit_attention": 2, "quick_gelu": 2}
    # training mode: ATen
    clip.train()
    try:
        calls.clear()
        with torch.no_grad():
            clip.encode_text(ids)
        assert calls.n == {} and calls.sdpa == 2
    finally:
        clip.eval()


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E = dict(recipe.SMALL, image_resolution=224, vision_patch_size=32)       # 7 x 7 patches + the class token = 50 tokens


def openai_checkpoint(du, path):
    """What OpenAI distributes, in the small: fp16 tensors and the three scalar keys."""
    m = du.OpenAIClip(**E2E)
    recipe.fill(m, seed=77)
    sd = {k: (v.half() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    sd.update(input_resolution=torch.tensor(224), context_length=torch.tensor(77), vocab_size=torch.tensor(E2E["vocab_size"]))
    torch.save(sd, path)


CONCEPTS = [s for s in recipe.STRINGS[:12]]


def save(og_utils, clip_name, dev, tmp, tag):
    concepts = tmp / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    ex = og_utils.save_activations(clip_name=clip_name, target_name="resnet18", target_layers=["layer4"], d_probe="synthetic_8",
                                   concept_set=str(concepts), batch_size=8, device=str(dev), pool_mode="avg",
                                   save_dir=str(tmp / tag))
    ex.wait()
    torch.cuda.synchronize()
    return ex


def test_save_activations_with_an_openai_checkpoint(du, dev, tmp_path, monkeypatch):
    from mammo_clip_dissect_amd.concept_vit import og_utils
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_CLIP_CKPTS", raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    du.register_tokenizer("clip", recipe.BPE_SMALL)
    ckpt = str(tmp_path / "openai_small.pt")
    openai_checkpoint(du, ckpt)
    calls = Calls(du, monkeypatch)
    ex = save(og_utils, ckpt, dev, tmp_path, "with")
    # 12 concepts in chunks of 8 and 4 through two causal blocks; 8 images in one batch through K11 and two blocks
    assert calls.n["vit_attention_causal"] == 4 and calls.n["quick_gelu"] == 6 and calls.n["patchify"] == 1
    model, _ = du.get_target_model("openai_clip", dev, ckpt=ckpt)
    assert all(v.dtype == torch.float32 for v in model.state_dict().values() if v.is_floating_point())
    ids = model.tokenize(CONCEPTS).to(dev)
    assert tuple(ids.shape) == (12, 77)
    with torch.no_grad():
        want = torch.cat([model.encode_text(ids[:8]), model.encode_text(ids[8:])])           # the extraction's chunks
    assert tuple(ex.E_txt.shape) == (12, 64) and torch.equal(int_bits(ex.E_txt), int_bits(want))
    assert tuple(ex.dis.E_img.shape) == (8, 64)                                             # the checkpoint's embed_dim
    assert bool(torch.isfinite(ex.dis.E_img).all()) and float(ex.dis.E_img.abs().max()) > 0


def test_save_activations_without_a_checkpoint_is_unchanged(du, dev, tmp_path, monkeypatch):
    """No checkpoint for the name: the dissector is the ClipViT with the hashing tokenizer as before, none of this route's
    kernels runs for it, and its features do not depend on the feature's switch."""
    from mammo_clip_dissect_amd.concept_vit import og_utils
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.delenv("MCD_CLIP_CKPTS", raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    on = save(og_utils, "ViT-B/16", dev, tmp_path, "on")
    assert "vit_attention_causal" not in calls.n and "quick_gelu" not in calls.n
    monkeypatch.setattr(du, "HIP_CLIP_TEXT", False)
    off = save(og_utils, "ViT-B/16", dev, tmp_path, "off")
    assert tuple(on.E_txt.shape) == (12, 512)
    assert torch.equal(int_bits(on.E_txt), int_bits(off.E_txt)) and torch.equal(int_bits(on.dis.E_img), int_bits(off.dis.E_img))
