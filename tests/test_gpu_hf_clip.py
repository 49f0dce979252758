"""GPU: K26 (mcd_token_mean, include/mcd_tokens.h) and the HIP route of data_utils.HFClip.

K26 against float64 with ATen's mean of the same tensor as the measure, contiguous and with padded strides inside framed
allocations (the gaps and the guards must come back intact), its independence of batch neighbours, its refusals, the
core.token_mean binding, and the stream and capture contracts with test_gpu_stream_contracts' machinery.  Then HFClip on the
fixture of tests/golden/hf_clip.npz (what the installed transformers computed) against the float64 goldens, the route's
switches by counted calls, and the two CLIP-dissector drivers with a checkpoint registered for the `clip` target."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hf_clip_recipe as recipe
import openai_clip_recipe as openai_recipe
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


def _bound(e_hip, e_aten, what):       # test_gpu_tower_openai_clip's
    print("%s: hip %.3e aten %.3e ratio to the bound %.3f" % (what, e_hip, e_aten, e_hip / (2 * e_aten + 1e-6)))
    assert e_hip <= 2 * e_aten + 1e-6, (what, e_hip, e_aten)


# ---- K26 -----------------------------------------------------------------------------------------------------------------
# (B, T, D, t0): one row of one float4; HFClip's small and long configurations (17 tokens; 289 rows: more than 256, a row
# count that is 1 mod 4 and 1 mod 32); a second column block with one live lane (65 float4s) and 32 rows, a whole number of
# unrolled steps; four column blocks from token 0; ViT-B/16's own 196 rows of 768
K26_CASES = [(1, 2, 4, 1), (3, 17, 128, 1), (2, 290, 128, 1), (3, 33, 260, 1), (2, 50, 1024, 0), (5, 197, 768, 1)]
CASE_IDS = ["B%d-T%d-D%d-t%d" % c for c in K26_CASES]
_K26 = {}


def strides(case, padded):
    B, T, D, t0 = case
    if not padded:
        return D, T * D, D
    x_tok = D + 4
    return x_tok, T * x_tok + 8, D + 4


def k26(L, x, t0, padded, gap=NAN):
    """K26 on framed operands: x behind guards (and, padded, with `gap` between its tokens and images), out in a frame of
    OUT_FILL whose guards and gaps must come back intact; the input untouched.  Returns the [B, D] output."""
    B, T, D = x.shape
    x_tok, x_img, out_img = strides((B, T, D, t0), padded)
    x_ = EF.Strided(x, x_tok, x_img, gap)
    o_ = util.FramedOut(B, D, out_img, 0, torch.float32, x.device)
    EF.ok(L.mcd_token_mean(x_.ptr, B, T, D, x_img, x_tok, t0, o_.ptr, out_img, EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K26", tuple(x.shape), t0, padded))
    assert not bool((int_bits(out) == int(int_bits(torch.full((1,), util.OUT_FILL))[0])).any()), "an element was not written"
    x_.same()
    return out


def k26_case(L, dev, case):
    """(x, the framed contiguous K26 output) of a case, computed once and left unchanged."""
    if case not in _K26:
        B, T, D, t0 = K26_CASES[case]
        x = EF.rnd((B, T, D), 500 + T + D, dev, 1.5, 0.25)
        _K26[case] = (x, k26(L, x, t0, False))
    return _K26[case]


@pytest.mark.parametrize("case", range(len(K26_CASES)), ids=CASE_IDS)
def test_k26_against_float64(L, dev, case):
    B, T, D, t0 = K26_CASES[case]
    x, out = k26_case(L, dev, case)
    ref = x.double().cpu()[:, t0:].mean(dim=1)
    e_aten = nerr(x[:, t0:].mean(dim=1), ref)
    _bound(nerr(out, ref), e_aten, ("K26", K26_CASES[case]))
    for gap in util.GAP_FILLS:          # the padded strides: the same bits, whatever the gaps hold
        assert torch.equal(int_bits(k26(L, x, t0, True, gap)), int_bits(out)), (K26_CASES[case], "padded", gap)


@pytest.mark.parametrize("case", [1, 2, 5], ids=[CASE_IDS[i] for i in (1, 2, 5)])
def test_k26_an_image_does_not_see_its_batch_neighbours(L, dev, case):
    B, T, D, t0 = K26_CASES[case]
    x, out = k26_case(L, dev, case)
    for b in range(B):
        assert torch.equal(int_bits(k26(L, x[b:b + 1].contiguous(), t0, False)), int_bits(out[b:b + 1])), (K26_CASES[case], b)
    other = EF.rnd((B + 2, T, D), 77, dev, 30.0)          # image 0 in last place of a longer batch of other neighbours
    other[B + 1] = x[0]
    assert torch.equal(int_bits(k26(L, other, t0, True)[B + 1]), int_bits(out[0]))


def test_k26_row_order_is_the_headers(L, dev):
    """The order written down in mcd_tokens.h, replayed on the host in fp32: four strided partial sums in ascending row order,
    ((p0 + p1) + p2) + p3, one division."""
    for case in (1, 2, 3):
        B, T, D, t0 = K26_CASES[case]
        x, out = k26_case(L, dev, case)
        rows = x.cpu()[:, t0:]
        parts = []
        for w in range(4):
            p = torch.zeros(B, D)
            for r in range(w, T - t0, 4):
                p = p + rows[:, r]
            parts.append(p)
        want = (((parts[0] + parts[1]) + parts[2]) + parts[3]) / float(T - t0)
        assert torch.equal(int_bits(out.cpu()), int_bits(want)), K26_CASES[case]


def test_k26_refuses_bad_arguments_and_writes_nothing(L, dev):
    B, T, D = 2, 17, 128
    x = EF.Strided(EF.rnd((B, T, D), 1, dev), D, T * D, NAN)
    out = util.FramedOut(B, D, D, 0, torch.float32, dev)
    ARG, UNSUPPORTED = -1, -5
    good = dict(x=x.ptr, B=B, T=T, D=D, x_img=T * D, x_tok=D, t0=1, out=out.ptr, out_img=D)
    inside = x.ptr + 4 * D                      # out on token 1 of image 0: overlaps x
    for change, code in ((dict(x=None), ARG), (dict(out=None), ARG), (dict(D=126), ARG), (dict(D=0), ARG), (dict(T=0), ARG),
                         (dict(t0=-1), ARG), (dict(t0=T), ARG), (dict(x_tok=D - 4), ARG), (dict(out_img=D - 4), ARG),
                         (dict(x_img=T * D - 4), ARG), (dict(x_img=T * D + 2), ARG), (dict(x_tok=D + 2, x_img=T * (D + 2) + 2), ARG),
                         (dict(out_img=D + 2), ARG), (dict(x=x.ptr + 4), ARG), (dict(out=out.ptr + 8), ARG),
                         (dict(out=inside), ARG), (dict(B=65536), UNSUPPORTED), (dict(B=-1), ARG)):
        a = dict(good, **change)
        rc = L.mcd_token_mean(a["x"], a["B"], a["T"], a["D"], a["x_img"], a["x_tok"], a["t0"], a["out"], a["out_img"], EF.st())
        assert rc == code, (change, rc)
    assert L.mcd_token_mean(x.ptr, 0, T, D, T * D, D, 1, out.ptr, D, EF.st()) == 0          # B == 0: a no-op
    torch.cuda.synchronize()
    assert bool((out.flat == util.OUT_FILL).all())
    x.same()


def test_token_mean_binding(core, L, dev, mcd):
    B, T, D, t0 = K26_CASES[3]
    x, out = k26_case(L, dev, 3)
    assert torch.equal(int_bits(core.token_mean(x, t0)), int_bits(out))
    assert torch.equal(int_bits(core.token_mean(x)), int_bits(out))                         # t0 defaults to 1
    assert torch.equal(int_bits(core.token_mean(x, 0)), int_bits(k26(L, x, 0, False)))
    # row-strided views: tokens D + 4 apart inside a wider tensor, out the left columns of a wider matrix
    wide = torch.full((B, T, D + 4), NAN, device=dev)
    wide[:, :, :D] = x
    into = torch.full((B, D + 4), util.OUT_FILL, device=dev)
    got = core.token_mean(wide[:, :, :D], t0, out=into[:, :D])
    assert got.data_ptr() == into.data_ptr() and torch.equal(int_bits(into[:, :D]), int_bits(out))
    assert bool((into[:, D:] == util.OUT_FILL).all())
    assert torch.equal(int_bits(core.token_mean(x[1:, 2:], 0)), int_bits(k26(L, x[1:, 2:].contiguous(), 0, False)))
    with pytest.raises(TypeError):
        core.token_mean(x.double())
    with pytest.raises(TypeError):
        core.token_mean(x.transpose(1, 2))
    with pytest.raises(TypeError):
        core.token_mean(x[0])
    with pytest.raises(TypeError):
        core.token_mean(x, out=torch.empty(B, D + 4, device=dev))
    with pytest.raises(mcd._lib.McdError) as e:
        core.token_mean(x, T)
    assert e.value.code == -1


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery -------------------------------------------------
def b_token_mean(L, dev):
    B, T, D = 3, 37, 132
    return S.simple(L, dev, "K26", [S._gen((B, T, D))], [(B, D)],
                    lambda i, o, st: L.mcd_token_mean(i[0], B, T, D, T * D, D, 1, o[0], D, st))


TOKEN_STREAM_ROWS = {"mcd_token_mean": b_token_mean}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(TOKEN_STREAM_ROWS) == sorted(mcd._lib.TOKEN_SIGNATURES)


@pytest.fixture(scope="module")
def spin_cycles(dev):
    """A spin of at least S.MIN_SPIN_MS (the entry runs in well under a millisecond), in the cycles of torch.cuda._sleep."""
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


@pytest.mark.parametrize("entry", sorted(TOKEN_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):
    r = S.Run(entry, TOKEN_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)      # (the control -- a launch on another stream IS seen -- is test_gpu_stream_contracts.py's)


@pytest.mark.parametrize("entry", sorted(TOKEN_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    r = S.Run(entry, TOKEN_STREAM_ROWS[entry](L, dev), dev)
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


# ---- HFClip ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "hf_clip.npz")), json.load(open(os.path.join(util.GOLDEN, "hf_clip_meta.json")))


_MODELS = {}


def model_of(du, dev, fixture, name):
    if name not in _MODELS:
        m = du.HFClip(**recipe.CONFIGS[name])
        assert recipe.fill(m, recipe.SEED[name]) == fixture[1][name + "_weights_sha256"]
        _MODELS[name] = m.to(dev).eval()
    return _MODELS[name]


# per forward: K11; pre_layrnorm + two per layer on K10; K9 (17 tokens) or K9L (290) per layer; K25 per layer; K26
HIP_CALLS = {"small": {"patchify": 1, "layer_norm": 5, "vit_attention": 2, "quick_gelu": 2, "token_mean": 1},
             "long": {"patchify": 1, "layer_norm": 3, "vit_attention_long": 1, "quick_gelu": 1, "token_mean": 1}}


class Calls(util.CallCounter):
    """util.CallCounter on the route's wrappers, the SDPA calls beside them, and K26's last result."""

    def __init__(self, du, monkeypatch):
        super().__init__(du.core, monkeypatch, ["layer_norm", "vit_attention", "vit_attention_long", "vit_attention_cls",
                                                "quick_gelu", "patchify", "token_mean"])
        self.sdpa, self.mean = 0, None
        fn, counted = F.scaled_dot_product_attention, du.core.token_mean

        def wrap(*a, **kw):
            self.sdpa += 1
            return fn(*a, **kw)
        monkeypatch.setattr(du.F, "scaled_dot_product_attention", wrap)

        def mean(*a, **kw):
            self.mean = counted(*a, **kw)
            return self.mean
        monkeypatch.setattr(du.core, "token_mean", mean)

    def clear(self):
        self.n.clear()
        self.sdpa, self.mean = 0, None


def run_rows(model, image, classifier_hook):
    """{layer<i>: class-token rows, logits[, mean: the classifier's input]} of one forward."""
    rows, hooks = {}, []
    for i, layer in enumerate(model.vision_model.encoder.layers):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: rows.__setitem__("layer%d" % i, o[:, 0].clone())))
    if classifier_hook:
        hooks.append(model.classifier.register_forward_hook(lambda m, a, o: rows.__setitem__("mean", a[0].clone())))
    try:
        with torch.no_grad():
            rows["logits"] = model(image)
    finally:
        for h in hooks:
            h.remove()
    return rows


@pytest.mark.parametrize("name", ["small", "long"])
def test_hf_clip_hip_route_against_float64(du, fixture, dev, monkeypatch, name):
    z, _ = fixture
    m = model_of(du, dev, fixture, name)
    image = recipe.make_image(name).to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    assert m.route(image) == "aten"                       # autograd is recording here
    hip = run_rows(m, image, False)
    assert calls.n == HIP_CALLS[name] and calls.sdpa == 0, (calls.n, calls.sdpa)
    hip["mean"] = calls.mean
    with torch.no_grad():
        assert m.route(image) == "hip" and torch.equal(m.encode_image(image), hip["logits"])
    calls.clear()
    hooked = run_rows(m, image, True)                     # a hook on the classifier: the module is called, with K26's result
    assert calls.n == HIP_CALLS[name] and torch.equal(hooked["mean"], hip["mean"])
    _bound(nerr(hooked["logits"], torch.from_numpy(z[name + "_logits_f64"])), nerr(hip["logits"], torch.from_numpy(z[name + "_logits_f64"])),
           "the classifier as a module")
    calls.clear()
    monkeypatch.setattr(du, "HIP_HF_CLIP", False)
    aten = run_rows(m, image, True)
    assert calls.n == {} and calls.sdpa == recipe.CONFIGS[name]["layers"]
    for k in sorted(hip):
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        _bound(nerr(hip[k], f64), nerr(aten[k], f64), "%s %s on the HIP route" % (name, k))
        _bound(nerr(aten[k], f64), nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64), "%s %s on the ATen route on the GPU" % (name, k))


def test_a_hook_inside_a_layer_sends_that_layer_to_aten(du, fixture, dev, monkeypatch):
    z, _ = fixture
    m = model_of(du, dev, fixture, "small")
    image = recipe.make_image("small").to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    f64 = torch.from_numpy(z["small_logits_f64"])
    seen = []
    fc1 = m.vision_model.encoder.layers[1].mlp.fc1
    handle = fc1.register_forward_hook(lambda mod, a, o: seen.append((a[0].clone(), o.clone())))
    try:
        with torch.no_grad():
            got = m(image)
    finally:
        handle.remove()
    # layer 0 on the HIP route (K10 twice, K9, K25), layer 1 on its ATen modules (one SDPA call), embedding, pre_layrnorm and head on HIP
    assert calls.n == {"patchify": 1, "layer_norm": 3, "vit_attention": 1, "quick_gelu": 1, "token_mean": 1} and calls.sdpa == 1
    assert len(seen) == 1 and tuple(seen[0][1].shape) == (3, 17, 512)
    with torch.no_grad():
        assert torch.equal(seen[0][1], fc1(seen[0][0]))
    calls.clear()
    monkeypatch.setattr(du, "HIP_HF_CLIP", False)
    with torch.no_grad():
        aten = m(image)
    _bound(nerr(got, f64), nerr(aten, f64), "a hook on layers[1].mlp.fc1")


def test_switch_autograd_and_double_take_aten(du, fixture, dev, monkeypatch):
    z, _ = fixture
    m = model_of(du, dev, fixture, "small")
    image = recipe.make_image("small").to(dev)
    f64 = torch.from_numpy(z["small_logits_f64"])
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    with torch.no_grad():
        hip = m(image)
    assert calls.n == HIP_CALLS["small"]
    e_hip = nerr(hip, f64)
    calls.clear()
    grad = m(image)                                       # autograd on
    assert calls.n == {} and calls.sdpa == 2 and grad.requires_grad
    calls.clear()
    m64 = du.HFClip(**recipe.SMALL).double().to(dev).eval()
    m64.load_state_dict(m.state_dict())
    with torch.no_grad():
        dbl = m64(image)
        assert dbl.dtype == torch.float64 and calls.n == {} and calls.sdpa == 2
        calls.clear()
        m.train()
        try:
            m(image)
        finally:
            m.eval()
        assert calls.n == {} and calls.sdpa == 2
        calls.clear()
        monkeypatch.setattr(du, "HIP_HF_CLIP", False)     # what MCD_NO_HIP_HF_CLIP=1 sets at import (test_hf_clip_cpu.py)
        off = m(image)
        assert calls.n == {} and calls.sdpa == 2
    e_aten = nerr(off, f64)
    _bound(e_hip, e_aten, "the HIP route")
    for what, got in (("MCD_NO_HIP_HF_CLIP", off), ("autograd", grad), ("double", dbl)):
        _bound(nerr(got, f64), e_aten, what + " takes ATen")
        _bound(nerr(got, hip.double()), e_hip + e_aten, what + " against the HIP result")
    with pytest.raises(ValueError, match="doesn't match model"):
        m(torch.zeros(1, 3, 80, 80, device=dev))


# ---- the drivers -----------------------------------------------------------------------------------------------------------
CONCEPTS = list(openai_recipe.STRINGS[:12])
LAYERS = ["vision_model.encoder.layers[0]", "vision_model.encoder.layers[1]"]
PROBE = "synthetic_64_64"


@pytest.fixture
def registries(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    for name in ("MCD_TARGET_CKPTS", "MCD_CLIP_CKPTS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")


def watch_extraction(monkeypatch):
    """The (dissector, target) pairs the drivers hand to utils.extract_and_save."""
    from mammo_clip_dissect_amd.concept_vit import utils
    pairs, real = [], utils.extract_and_save

    def spy(clip_model, target_model, *a, **kw):
        pairs.append((clip_model, target_model))
        return real(clip_model, target_model, *a, **kw)
    monkeypatch.setattr(utils, "extract_and_save", spy)
    return pairs


def drive(drv, tmp, tag, probe, dev, concepts, target="clip", layers=LAYERS):
    act, res = str(tmp / (tag + "_acts")), str(tmp / (tag + "_results"))
    out = drv.main(["--clip_model", "ViT-B/16", "--target_model", target, "--target_layers", ",".join(layers), "--d_probe", probe,
                    "--concept_set", str(concepts), "--batch_size", "32", "--device", str(dev), "--activation_dir", act,
                    "--result_dir", res, "--similarity_fn", "wpmi"])
    torch.cuda.synchronize()
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    return act, open(csvs[0], "rb").read()


@pytest.mark.parametrize("driver", ["describe_clip_neurons", "describe_og_neurons"])
def test_drivers_with_a_registered_clip_checkpoint(du, fixture, dev, tmp_path, monkeypatch, registries, driver):
    """Fails on the parent commit: there is no registry, and with an OpenAI checkpoint as the dissector the documented layer
    names do not resolve.  The dissector is a small OpenAI CLIP from a registered checkpoint (64 x 64 images, as the target's)."""
    import importlib
    drv = importlib.import_module("mammo_clip_dissect_amd.concept_vit." + driver)
    z, _ = fixture
    small = model_of(du, dev, fixture, "small")
    ckpt = str(tmp_path / "hf_clip_small.pt")
    torch.save({k: v.cpu() for k, v in small.state_dict().items()}, ckpt)
    du.register_target_checkpoint("clip", ckpt)
    dissector = du.OpenAIClip(**openai_recipe.SMALL)
    openai_recipe.fill(dissector, seed=77)
    torch.save(dissector.state_dict(), str(tmp_path / "openai_small.pt"))
    du.register_clip_checkpoint("ViT-B/16", str(tmp_path / "openai_small.pt"))
    du.register_tokenizer("clip", openai_recipe.BPE_SMALL)
    concepts = tmp_path / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    pairs = watch_extraction(monkeypatch)
    calls = Calls(du, monkeypatch)
    act, csv = drive(drv, tmp_path, "with", PROBE, dev, concepts)
    assert len(pairs) == 1 and isinstance(pairs[0][0], du.OpenAIClip) and isinstance(pairs[0][1], du.HFClip)
    assert calls.n["token_mean"] == 3                                   # the width probe and two batches of 32
    import io
    import pandas as pd
    df = pd.read_csv(io.BytesIO(csv))
    assert [int((df.layer == layer).sum()) for layer in LAYERS] == [128, 128] and len(df) == 256
    # the cache files of the two layers: the class-token rows of a direct forward of the registered model, batch by batch
    model, _ = du.get_target_model("clip", dev)
    assert isinstance(model, du.HFClip) and all(torch.equal(v, small.state_dict()[k]) for k, v in model.state_dict().items())
    images = du.get_data(PROBE, None, dev).images()
    want = [run_rows(model, images[i:i + 32], False) for i in (0, 32)]
    for i, layer in enumerate(LAYERS):
        files = glob.glob(os.path.join(act, "**", "*%s_clip_%s.pt" % (PROBE, glob.escape(layer))), recursive=True)
        assert len(files) == 1, os.listdir(act)
        got = torch.load(files[0], map_location="cpu", weights_only=True)
        rows = torch.cat([w["layer%d" % i] for w in want]).cpu()
        assert tuple(got.shape) == (64, 128) and torch.equal(int_bits(got), int_bits(rows)), layer
    # and that model on the recipe's input gives the goldens' rows
    direct = run_rows(model, recipe.make_image("small").to(dev), False)
    monkeypatch.setattr(du, "HIP_HF_CLIP", False)
    aten = run_rows(model, recipe.make_image("small").to(dev), False)
    for k in sorted(direct):
        f64 = torch.from_numpy(z["small_%s_f64" % k])
        _bound(nerr(direct[k], f64), nerr(aten[k], f64), "the registered model, " + k)


@pytest.mark.parametrize("driver", ["describe_clip_neurons", "describe_og_neurons"])
def test_drivers_without_a_registration_are_unchanged(du, dev, tmp_path, monkeypatch, registries, driver):
    """No checkpoint registered for `clip`: the target is the dissector object, a ClipViT, as before, none of HFClip's route
    runs, and the CSV does not depend on the feature's switch.  (The stand-in's position table is 224 x 224's, so this half
    runs on 224 x 224 images: 64 x 64 ones never went through it.)"""
    import importlib
    drv = importlib.import_module("mammo_clip_dissect_amd.concept_vit." + driver)
    concepts = tmp_path / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    pairs = watch_extraction(monkeypatch)
    calls = Calls(du, monkeypatch)
    _, on = drive(drv, tmp_path, "on", "synthetic_64_224", dev, concepts)
    assert "token_mean" not in calls.n and "quick_gelu" not in calls.n
    monkeypatch.setattr(du, "HIP_HF_CLIP", False)
    _, off = drive(drv, tmp_path, "off", "synthetic_64_224", dev, concepts)
    assert on == off
    assert len(pairs) == 2 and all(t is c and isinstance(t, du.ClipViT) for c, t in pairs)


# 7 x 7 patches of 32 pixels + the class token = 50 tokens at the stand-in dissector's 224 x 224
WIDE = dict(num_labels=5, image_size=224, patch=32, hidden=128, layers=2, heads=2, mlp=512)


def register_only_the_target(du, tmp_path):
    m = du.HFClip(**WIDE)
    recipe.fill(m, 31)
    ckpt = str(tmp_path / "hf_clip_wide.pt")
    torch.save(m.state_dict(), ckpt)
    du.register_target_checkpoint("clip", ckpt)
    concepts = tmp_path / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    return m, concepts


@pytest.mark.parametrize("driver", ["describe_clip_neurons", "describe_og_neurons"])
def test_drivers_with_only_the_target_registered(du, dev, tmp_path, monkeypatch, registries, driver):
    """What INTEGRATION.md shows: a checkpoint for the `clip` target, none for the dissector.  The dissector stays the ClipViT
    stand-in with its text side, the target is an HFClip of its own, and its cache holds that model's class-token rows."""
    import importlib
    import io
    import pandas as pd
    drv = importlib.import_module("mammo_clip_dissect_amd.concept_vit." + driver)
    filled, concepts = register_only_the_target(du, tmp_path)
    pairs = watch_extraction(monkeypatch)
    calls = Calls(du, monkeypatch)
    act, csv = drive(drv, tmp_path, "only", "synthetic_32_224", dev, concepts)
    assert len(pairs) == 1 and isinstance(pairs[0][0], du.ClipViT) and isinstance(pairs[0][1], du.HFClip)
    assert calls.n["token_mean"] == 2                                   # the width probe and one batch of 32
    df = pd.read_csv(io.BytesIO(csv))
    assert [int((df.layer == layer).sum()) for layer in LAYERS] == [128, 128]
    model = pairs[0][1]
    assert all(torch.equal(v.cpu(), filled.state_dict()[k]) for k, v in model.state_dict().items())
    want = run_rows(model, du.get_data("synthetic_32_224", None, dev).images(), False)
    for i, layer in enumerate(LAYERS):
        files = glob.glob(os.path.join(act, "**", "*synthetic_32_224_clip_%s.pt" % glob.escape(layer)), recursive=True)
        assert len(files) == 1, os.listdir(act)
        got = torch.load(files[0], map_location="cpu", weights_only=True)
        assert torch.equal(int_bits(got), int_bits(want["layer%d" % i].cpu())), layer


def test_driver_with_another_target_while_clip_is_registered(du, dev, tmp_path, monkeypatch, registries):
    """A registration for `clip` (a shared MCD_TARGET_CKPTS table, say) leaves a run on another target alone: the dissector is
    the ClipViT stand-in, the target a seeded ResNet, none of HFClip's route runs."""
    from mammo_clip_dissect_amd.concept_vit import describe_og_neurons as drv
    _, concepts = register_only_the_target(du, tmp_path)
    pairs = watch_extraction(monkeypatch)
    calls = Calls(du, monkeypatch)
    _, csv = drive(drv, tmp_path, "other", "synthetic_32_224", dev, concepts, target="resnet18", layers=["layer4"])
    assert len(pairs) == 1 and isinstance(pairs[0][0], du.ClipViT) and isinstance(pairs[0][1], du.ResNet)
    assert "token_mean" not in calls.n and "quick_gelu" not in calls.n and csv.count(b"layer4") == 512


def test_a_global_hook_sees_every_module(du, fixture, dev, monkeypatch):
    """A global module hook: embedding, pre_layrnorm, every layer and the classifier go through their modules (the hook sees
    each of them); K26 still computes the mean, and the logits are the HIP route's within the bound."""
    z, _ = fixture
    m = model_of(du, dev, fixture, "small")
    image = recipe.make_image("small").to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    f64 = torch.from_numpy(z["small_logits_f64"])
    with torch.no_grad():
        hip = m(image)
    calls = Calls(du, monkeypatch)
    seen = []
    handle = torch.nn.modules.module.register_module_forward_hook(lambda mod, a, o: seen.append(mod))
    try:
        with torch.no_grad():
            got = m(image)
    finally:
        handle.remove()
    vm = m.vision_model
    for mod in (vm.embeddings, vm.embeddings.patch_embedding, vm.pre_layrnorm, vm.encoder.layers[0].self_attn.q_proj,
                vm.encoder.layers[1].mlp.fc1, vm.encoder.layers[1], m.classifier, m):
        assert sum(s is mod for s in seen) == 1, type(mod).__name__
    assert vm.post_layernorm not in seen
    assert calls.n == {"token_mean": 1} and calls.sdpa == 2
    _bound(nerr(got, f64), nerr(hip, f64), "under a global hook")
