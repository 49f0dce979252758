"""GPU: K28 (mcd_patchify_kept) and K29 (mcd_token_restore) of include/mcd_mask.h against torch on the same fp32 inputs, bit
for bit; their stream, capture and refusal contracts with test_gpu_stream_contracts' machinery; data_utils.HFMae's HIP route
against the float64 fixture of tests/golden/mae.npz by the rule of tests/test_mae_cpu.py, against its ATen route, under hooks and
under MCD_NO_HIP_MAE=1 in a child process; one driver run with a registered checkpoint, twice under one seed."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mae_recipe as recipe
import test_gpu_stream_contracts as S
import util
from util import OUT_FILL, int_bits, nerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def perms(B, L_, n, seed):
    """int32 [B, n]: the first n entries of a seeded permutation of 0 .. L_-1 per image (in range, distinct)."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(L_, generator=g)[:n] for _ in range(B)]).to(torch.int32)


def images(B, size, seed):
    return torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(seed))


# ---- K28 -------------------------------------------------------------------------------------------------------------------------
# (B, image size, patch, kept patches): the fixture's small and odd shapes (16- and 8-byte accesses, several workgroups), one
# kept patch, one image, a patch of 2 pixels
K28_CASES = [(3, 32, 8, 4), (3, 30, 6, 6), (2, 32, 8, 1), (1, 30, 6, 6), (2, 12, 2, 9)]


@pytest.mark.parametrize("case", K28_CASES, ids=lambda c: "B%d-%dpx-P%d-Lk%d" % c)
def test_k28_is_k11_followed_by_a_row_gather(core, dev, case):
    B, size, P, Lk = case
    x = images(B, size, 40 + Lk).to(dev)
    n = (size // P) ** 2
    keep = perms(B, n, Lk, 50 + P).to(dev)
    full = core.patchify(x, P)                                                     # K11: [B, 1 + n, 3 P P]
    want = torch.cat([full[:, :1], torch.gather(full[:, 1:], 1, keep.long().unsqueeze(-1).expand(-1, -1, full.shape[2]))], 1)
    got = core.patchify_kept(x, P, keep)
    assert tuple(got.shape) == (B, 1 + Lk, 3 * P * P) and torch.equal(int_bits(got), int_bits(want))
    assert not bool(got[:, 0].any())


@pytest.mark.parametrize("size,P", [(32, 8), (30, 6)])
def test_k28_with_every_patch_in_order_is_k11(core, dev, size, P):
    x = images(3, size, 41).to(dev)
    n = (size // P) ** 2
    keep = torch.arange(n, dtype=torch.int32, device=dev).expand(3, -1).contiguous()
    assert torch.equal(int_bits(core.patchify_kept(x, P, keep)), int_bits(core.patchify(x, P)))


def test_k28_with_no_kept_patch_writes_the_zero_rows(core, dev):
    got = core.patchify_kept(images(2, 32, 42).to(dev), 8, torch.zeros(2, 0, dtype=torch.int32, device=dev))
    assert tuple(got.shape) == (2, 1, 192) and not bool(got.any())


# ---- K29 -------------------------------------------------------------------------------------------------------------------------
def restore_ref(src, restore, fill, add):
    """transformers' ViTMAEDecoder steps on the same fp32 inputs: repeat, cat, gather over an expanded index, cat, add."""
    B, L_ = restore.shape
    D = src.shape[2]
    tokens = src[:, 1:]
    if L_ + 1 - src.shape[1] > 0:
        tokens = torch.cat([tokens, fill.view(1, 1, D).repeat(B, L_ + 1 - src.shape[1], 1)], dim=1)
    tokens = torch.gather(tokens, 1, restore.long().unsqueeze(-1).repeat(1, 1, D))
    out = torch.cat([src[:, :1], tokens], dim=1)
    return out if add is None else out + add


# (B, L, Lk, D, with add): the fixture's two decoder shapes, no add, Lk = L (nothing filled), the narrowest row, a row that is
# no multiple of a wave's 256 floats, one image
K29_CASES = [(3, 16, 4, 64, True), (3, 25, 6, 64, True), (3, 16, 4, 64, False), (2, 16, 16, 64, True), (2, 9, 3, 4, True),
             (2, 25, 6, 132, True), (1, 16, 4, 132, False)]


@pytest.mark.parametrize("case", K29_CASES, ids=lambda c: "B%d-L%d-Lk%d-D%d-%s" % (c[:4] + ("add" if c[4] else "noadd",)))
def test_k29_is_cat_gather_add(core, dev, case):
    B, L_, Lk, D, with_add = case
    g = torch.Generator().manual_seed(60 + L_ + D)
    src = torch.randn(B, 1 + Lk, D, generator=g).to(dev)
    fill, add = torch.randn(D, generator=g).to(dev), torch.randn(1 + L_, D, generator=g).to(dev)
    restore = perms(B, L_, L_, 70 + Lk).to(dev)                                     # a permutation of 0 .. L-1, as argsort gives
    add = add if with_add else None
    got = core.token_restore(src, restore, fill, add)
    assert tuple(got.shape) == (B, 1 + L_, D)
    assert torch.equal(int_bits(got), int_bits(restore_ref(src, restore, fill, add)))
    if Lk == L_:                                                                    # no row is filled: fill may be left out
        assert torch.equal(int_bits(core.token_restore(src, restore, None, add)), int_bits(got))
    out = torch.full_like(got, OUT_FILL)
    assert core.token_restore(src, restore, fill, add, out=out) is out and torch.equal(int_bits(out), int_bits(got))


@pytest.mark.parametrize("L_,Lk,D", [(16, 4, 128), (25, 6, 132)])
def test_k29_gathers_the_position_rows_of_the_kept_patches(core, dev, L_, Lk, D):
    """One table for all images (image stride 0), restore = the kept patch numbers, no fill, no add: row 0 and the rows
    1 + keep[b, j] of the table, per image."""
    table = torch.randn(1 + L_, D, generator=torch.Generator().manual_seed(80 + D)).to(dev)
    keep = perms(3, L_, Lk, 81).to(dev)
    got = core.token_restore(table, keep)
    want = torch.cat([table[:1].expand(3, -1, -1), table[1:][keep.long()]], dim=1)
    assert tuple(got.shape) == (3, 1 + Lk, D) and torch.equal(int_bits(got), int_bits(want))
    assert torch.equal(int_bits(got), int_bits(core.token_restore(table.expand(3, -1, -1).contiguous(), keep)))


# ---- refusals: a status, the message, nothing written ------------------------------------------------------------------------------
def test_refused_calls_write_nothing(L, core, mcd, dev):
    ARG, UNSUPPORTED = mcd._lib.MCD_E_ARG, mcd._lib.MCD_E_UNSUPPORTED
    x, keep = images(2, 30, 43).to(dev), perms(2, 25, 6, 44).to(dev)
    out = torch.full((2, 7, 3 * 36), OUT_FILL, device=dev)
    src, restore = torch.randn(2, 5, 64, device=dev), perms(2, 16, 16, 45).to(dev)
    fill, add = torch.randn(64, device=dev), torch.randn(17, 64, device=dev)
    dst = torch.full((2, 17, 64), OUT_FILL, device=dev)

    def k28(B=2, H=30, W=30, P=6, Lk=6):
        return L.mcd_patchify_kept(x.data_ptr(), keep.data_ptr(), B, 3, H, W, P, Lk, out.data_ptr(), None)

    def k29(B=2, L_=16, Lk=4, D=64, src_img=5 * 64):
        return L.mcd_token_restore(src.data_ptr(), src_img, restore.data_ptr(), fill.data_ptr(), add.data_ptr(), B, L_, Lk, D,
                                   dst.data_ptr(), None)
    assert k28(P=5) == UNSUPPORTED and k28(P=3) == UNSUPPORTED and k28(H=32) == UNSUPPORTED          # odd P, no whole patches
    assert k28(B=-1) == ARG and k28(Lk=-2) == ARG
    assert b"mcd_patchify_kept" in L.mcd_last_error()
    assert k29(D=62, src_img=5 * 62) == ARG and k29(D=2, src_img=12) == ARG                          # D % 4
    assert k29(B=-1) == ARG and k29(L_=-1) == ARG and k29(Lk=-1) == ARG and k29(src_img=4 * 64) == ARG
    assert b"mcd_token_restore" in L.mcd_last_error()
    assert k28(B=0) == 0 and k29(B=0) == 0                                                          # no image: a no-op
    torch.cuda.synchronize()
    assert bool((out == OUT_FILL).all()) and bool((dst == OUT_FILL).all())
    with pytest.raises(mcd._lib.McdError) as e:
        core.patchify_kept(images(1, 30, 46).to(dev)[:, :, :25, :25].contiguous(), 5, perms(1, 25, 6, 47).to(dev))
    assert e.value.code == UNSUPPORTED
    with pytest.raises(mcd._lib.McdError) as e:
        core.token_restore(torch.zeros(1, 3, 6, device=dev), perms(1, 4, 4, 48).to(dev), torch.zeros(6, device=dev))
    assert e.value.code == ARG


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery -------------------------------------------------
def b_patchify_kept(L, dev):
    B, size, P, Lk = 2, 16, 4, 5
    return S.simple(L, dev, "K28", [S._gen((B, 3, size, size)), lambda s: perms(B, (size // P) ** 2, Lk, s)], [(B, 1 + Lk, 3 * P * P)],
                    lambda i, o, st: L.mcd_patchify_kept(i[0], i[1], B, 3, size, size, P, Lk, o[0], st))


def b_token_restore(L, dev):
    B, L_, Lk, D = 2, 16, 4, 132
    return S.simple(L, dev, "K29", [S._gen((B, 1 + Lk, D)), lambda s: perms(B, L_, L_, s), S._gen((D,)), S._gen((1 + L_, D))],
                    [(B, 1 + L_, D)],
                    lambda i, o, st: L.mcd_token_restore(i[0], (1 + Lk) * D, i[1], i[2], i[3], B, L_, Lk, D, o[0], st))


MASK_STREAM_ROWS = {"mcd_patchify_kept": b_patchify_kept, "mcd_token_restore": b_token_restore}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(MASK_STREAM_ROWS) == sorted(mcd._lib.MASK_SIGNATURES)


@pytest.fixture(scope="module")
def spin_cycles(dev):
    """A spin of at least S.MIN_SPIN_MS (the entries run in well under a millisecond), in the cycles of torch.cuda._sleep."""
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


@pytest.mark.parametrize("entry", sorted(MASK_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):
    r = S.Run(entry, MASK_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)      # (the control -- a launch on another stream IS seen -- is test_gpu_stream_contracts.py's)


@pytest.mark.parametrize("entry", sorted(MASK_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    r = S.Run(entry, MASK_STREAM_ROWS[entry](L, dev), dev)
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


# ---- HFMae -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "mae.npz")), json.load(open(os.path.join(util.GOLDEN, "mae_meta.json")))


_MODELS = {}


def model_of(du, dev, fixture, name):
    if name not in _MODELS:
        sd, sha = recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])
        assert sha == fixture[1][name + "_weights_sha256"]
        _MODELS[name] = du.HFMae.from_state_dict(sd, norm_pix_loss=recipe.NORM_PIX_LOSS[name]).to(dev).eval()
    return _MODELS[name]


# per forward: K28; K29 twice (the position rows, the decoder's restore); K10 twice per layer (2 + 1 layers), vit.layernorm and
# decoder_norm; K9 in the two encoder layers (64-wide heads), SDPA in the decoder layer (32-wide heads)
HIP_CALLS = {"patchify_kept": 1, "token_restore": 2, "layer_norm": 8, "vit_attention": 2}


class Calls(util.CallCounter):
    """util.CallCounter on the route's wrappers, with the GEMM and the SDPA calls beside them."""

    def __init__(self, du, monkeypatch):
        super().__init__(du.core, monkeypatch, ["layer_norm", "vit_attention", "vit_attention_long", "vit_attention_cls",
                                                "patchify", "patchify_kept", "token_restore"])
        self.sdpa = self.gemms = 0
        fn, lin = F.scaled_dot_product_attention, du.core.linear_residual

        def wrap(*a, **kw):
            self.sdpa += 1
            return fn(*a, **kw)
        monkeypatch.setattr(du.F, "scaled_dot_product_attention", wrap)

        def gemm(*a, **kw):
            self.gemms += 1
            return lin(*a, **kw)
        monkeypatch.setattr(du.core, "linear_residual", gemm)

    def clear(self):
        self.n.clear()
        self.sdpa = self.gemms = 0


def run_rows(model, image, noise, extra=()):
    """({layer<i>: class-token rows, norm, logits, loss}, mask, ids_restore, shapes seen on layer[1]) of one forward."""
    rows, seen, hooks = {}, [], list(extra)
    for i, layer in enumerate(model.vit.encoder.layer):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: rows.__setitem__("layer%d" % i, o[:, 0].clone())))
    hooks.append(model.vit.encoder.layer[1].register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape))))
    hooks.append(model.vit.layernorm.register_forward_hook(lambda m, a, o: rows.__setitem__("norm", o.clone())))
    try:
        with torch.no_grad():
            out = model(image, noise)
    finally:
        for h in hooks:
            h.remove()
    rows.update(logits=out.logits, loss=out.loss.reshape(1))
    return rows, out.mask, out.ids_restore, seen


def accept(got, z, name, what):
    """The rule of tests/test_mae_cpu.py (tests/test_hf_clip_cpu.py's): within twice the fp32 fixture's own distance to the
    float64 fixture, plus 1e-6.  Returns the distances."""
    dist = {}
    for k in ["layer%d" % i for i in range(recipe.CONFIGS[name]["layers"])] + ["norm", "logits", "loss"]:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        e_ref = nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64)
        dist[k] = nerr(got[k], f64)
        print("%s %s %s: %.3e, fixture's fp32 %.3e, ratio to the bound %.3f" % (what, name, k, dist[k], e_ref,
                                                                                 dist[k] / (2 * e_ref + 1e-6)))
        assert tuple(got[k].shape) == tuple(f64.shape), (name, k)
        assert dist[k] <= 2 * e_ref + 1e-6, (what, name, k, dist[k], e_ref)
    return dist


@pytest.mark.parametrize("name", ["small", "odd"])
def test_hip_route_against_float64_and_against_aten(du, fixture, dev, monkeypatch, name):
    z, _ = fixture
    m = model_of(du, dev, fixture, name)
    cfg = recipe.CONFIGS[name]
    image, noise = recipe.make_image(name).to(dev), recipe.make_noise(name).to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    assert m.route(image) == "aten"                       # autograd is recording here
    with torch.no_grad():
        assert m.route(image) == "hip"
    hip, mask, ids, seen = run_rows(m, image, noise)
    # the embedding, qkv / proj / fc1 / fc2 per layer, decoder_embed, decoder_pred
    assert calls.n == HIP_CALLS and calls.sdpa == 1 and calls.gemms == 1 + 4 * 3 + 2, (calls.n, calls.sdpa, calls.gemms)
    shape = (recipe.BATCH, 1 + recipe.len_keep(cfg), cfg["hidden"])
    assert seen == [shape] and tuple(hip["norm"].shape) == shape
    assert torch.equal(mask.cpu(), torch.from_numpy(z[name + "_mask"]))
    assert torch.equal(ids.cpu(), torch.from_numpy(z[name + "_ids_restore"])) and ids.dtype == torch.int64
    e_hip = accept(hip, z, name, "HIP route")
    calls.clear()
    monkeypatch.setattr(du, "HIP_MAE", False)             # what MCD_NO_HIP_MAE=1 sets at import
    aten, mask2, ids2, seen2 = run_rows(m, image, noise)
    assert "patchify_kept" not in calls.n and "token_restore" not in calls.n and calls.gemms == 0 and calls.sdpa == 1
    assert seen2 == [shape] and torch.equal(mask2, mask) and torch.equal(ids2, ids)
    e_aten = accept(aten, z, name, "ATen route on the GPU")
    for k in sorted(hip):                                  # the two routes against each other, float64 the arbiter: the project's
        print("%s %s: HIP %.3e, ATen %.3e" % (name, k, e_hip[k], e_aten[k]))          # bound of a HIP route on its ATen route
        assert e_hip[k] <= 2 * e_aten[k] + 1e-6, (name, k, e_hip[k], e_aten[k])


def test_a_hook_inside_a_layer_sends_that_layer_to_aten(du, fixture, dev, monkeypatch):
    z, _ = fixture
    m = model_of(du, dev, fixture, "small")
    image, noise = recipe.make_image("small").to(dev), recipe.make_noise("small").to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = Calls(du, monkeypatch)
    seen = []
    fc1 = m.vit.encoder.layer[1].fc1
    handle = fc1.register_forward_hook(lambda mod, a, o: seen.append((a[0].clone(), o.clone())))
    got, _, _, shapes = run_rows(m, image, noise, extra=[handle])
    # layer[1] runs its own modules (its four GEMMs are nn.Linear calls); everything else stays on the route
    assert calls.n == HIP_CALLS and calls.gemms == 1 + 4 * 2 + 2 and shapes == [(3, 5, 128)], (calls.n, calls.gemms)
    assert len(seen) == 1 and tuple(seen[0][1].shape) == (3, 5, 512)
    with torch.no_grad():
        assert torch.equal(seen[0][1], fc1(seen[0][0]))
    accept(got, z, "small", "a hook on vit.encoder.layer[1].fc1")
    calls.clear()
    inner = m.decoder.decoder_embed.register_forward_hook(lambda mod, a, o: seen.append(tuple(o.shape)))
    got, _, _, _ = run_rows(m, image, noise, extra=[inner])
    assert seen[-1] == (3, 5, 64) and calls.gemms == 1 + 4 * 3 + 1 and calls.n == HIP_CALLS
    accept(got, z, "small", "a hook on decoder.decoder_embed")


def test_autograd_double_and_training_take_aten(du, fixture, dev, monkeypatch):
    z, _ = fixture
    m = model_of(du, dev, fixture, "small")
    image, noise = recipe.make_image("small").to(dev), recipe.make_noise("small").to(dev)
    calls = Calls(du, monkeypatch)
    out = m(image, noise)                                  # autograd on
    assert out.loss.requires_grad and calls.gemms == 0 and "patchify_kept" not in calls.n and "token_restore" not in calls.n
    m64 = du.HFMae(**recipe.SMALL).double().to(dev).eval()
    m64.load_state_dict(m.state_dict())
    with torch.no_grad():
        dbl = m64(image, noise)
        assert dbl.logits.dtype == torch.float64 and calls.gemms == 0 and "token_restore" not in calls.n
        assert nerr(dbl.logits, torch.from_numpy(z["small_logits_f64"])) <= 1e-10
        f64 = torch.from_numpy(z["small_logits_f64"])
        assert nerr(out.logits, f64) <= 2 * nerr(torch.from_numpy(z["small_logits_f32"]), f64) + 1e-6
        m.train()
        try:
            assert m.route(image) == "aten"
        finally:
            m.eval()


CHILD = """
import json, sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import mae_recipe as recipe
from mammo_clip_dissect_amd import core
from mammo_clip_dissect_amd.concept_vit import data_utils as du
n = {}
for name in ("patchify_kept", "token_restore", "linear_residual"):
    def wrap(*a, _fn=getattr(core, name), _name=name, **kw):
        n[_name] = n.get(_name, 0) + 1
        return _fn(*a, **kw)
    setattr(core, name, wrap)
sd, _ = recipe.weights(recipe.SMALL, recipe.SEED["small"])
m = du.HFMae.from_state_dict(sd).cuda().eval()
with torch.no_grad():
    out = m(recipe.make_image("small").cuda(), recipe.make_noise("small").cuda())
torch.save({"logits": out.logits.cpu(), "loss": out.loss.cpu().reshape(1), "mask": out.mask.cpu()}, %(out)r)
with torch.no_grad():
    route = m.route(recipe.make_image("small").cuda())
print(json.dumps({"flag": du.HIP_MAE, "route": route, "calls": n}))
"""


def test_the_environment_switch_keeps_aten_in_a_child_process(fixture, dev, tmp_path):
    z, _ = fixture
    out = str(tmp_path / "child.pt")
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MCD_NO_HIP_MAE="1"), capture_output=True, text=True,
                          timeout=240)
    assert done.returncode == 0, done.stderr[-2000:]
    said = json.loads(done.stdout.strip().splitlines()[-1])
    assert said == {"flag": False, "route": "aten", "calls": {}}, said
    got = torch.load(out, weights_only=True)
    assert torch.equal(got["mask"], torch.from_numpy(z["small_mask"]))
    for k in ("logits", "loss"):
        f64 = torch.from_numpy(z["small_%s_f64" % k])
        assert nerr(got[k], f64) <= 2 * nerr(torch.from_numpy(z["small_%s_f32" % k]), f64) + 1e-6, k


# ---- one driver run ----------------------------------------------------------------------------------------------------------------
LAYERS = ["vit.encoder.layer[0]", "vit.encoder.layer[1]"]
PROBE = "synthetic_64_224"
DRIVER_CFG = dict(image_size=224, patch=16, hidden=128, layers=2, heads=2, mlp=512, decoder_hidden=64, decoder_layers=1,
                  decoder_heads=2, decoder_mlp=256)
CONCEPTS = ["a mass", "a calcification", "dense tissue", "a lymph node", "a scar", "a clip", "skin", "a nipple", "fat",
            "a vessel", "a pacemaker", "an implant"]


@pytest.fixture
def registries(du, monkeypatch):
    monkeypatch.setattr(du, "TARGET_CHECKPOINTS", {})
    monkeypatch.setattr(du, "CLIP_CHECKPOINTS", {})
    monkeypatch.setattr(du, "TOKENIZER_VOCABS", {})
    for name in ("MCD_TARGET_CKPTS", "MCD_CLIP_CKPTS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")


def drive(drv, tmp, tag, dev, concepts):
    act, res = str(tmp / (tag + "_acts")), str(tmp / (tag + "_results"))
    torch.manual_seed(1234)                                # the mask is torch's global generator's: see DESIGN.md
    out = drv.main(["--clip_model", "ViT-B/16", "--target_model", "mae", "--target_layers", ",".join(LAYERS), "--d_probe", PROBE,
                    "--concept_set", str(concepts), "--batch_size", "32", "--device", str(dev), "--activation_dir", act,
                    "--result_dir", res, "--similarity_fn", "wpmi"])
    torch.cuda.synchronize()
    csvs = glob.glob(os.path.join(out, "*.csv"))
    assert len(csvs) == 1
    return act, open(csvs[0], "rb").read()


def test_driver_with_a_registered_mae_checkpoint(du, dev, tmp_path, monkeypatch, registries):
    import importlib
    drv = importlib.import_module("mammo_clip_dissect_amd.concept_vit.describe_clip_neurons")
    sd, _ = recipe.weights(DRIVER_CFG, 2033)
    ckpt = str(tmp_path / "mae_224.pt")
    torch.save(sd, ckpt)
    du.register_target_checkpoint("mae", ckpt)
    concepts = tmp_path / "twelve_concepts.txt"
    concepts.write_text("\n".join(CONCEPTS) + "\n", encoding="utf-8")
    calls = Calls(du, monkeypatch)
    act, first = drive(drv, tmp_path, "first", dev, concepts)
    assert calls.n["patchify_kept"] == 3 and calls.n["token_restore"] == 6          # the width probe and two batches of 32
    _, second = drive(drv, tmp_path, "second", dev, concepts)
    assert first == second
    import io
    import pandas as pd
    df = pd.read_csv(io.BytesIO(first))
    assert [int((df.layer == layer).sum()) for layer in LAYERS] == [128, 128] and len(df) == 256
    for layer in LAYERS:
        files = glob.glob(os.path.join(act, "**", "*%s_mae_%s.pt" % (PROBE, glob.escape(layer))), recursive=True)
        assert len(files) == 1, os.listdir(act)
        got = torch.load(files[0], map_location="cpu", weights_only=True)
        assert tuple(got.shape) == (64, DRIVER_CFG["hidden"]) and bool(torch.isfinite(got).all())
