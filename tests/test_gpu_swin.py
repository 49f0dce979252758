"""GPU: the Swin tower's HIP route -- K31 (mcd_window_attention) and K32 (mcd_patch_merge_ln) through the C ABI on framed,
pre-filled operands, then data_utils.SwinTower on both routes against transformers' fixture (tests/golden/swin.npz), and
the EfficientNet-B2 tower a B2 checkpoint builds.

K31's reference is a float64 restatement of the rules written here (conv_fuzz.reference64): zero padding of the token grid after the
projection's input (a padded token's q, k, v are pad_qkv), roll by (-s, -s), windows in row-major order, the bias
table[(i-i'+w-1)(2w-1) + (j-j'+w-1), head], -100 between tokens of different (row region, column region) pairs -- region 0, 1,
2 for a rolled index below n-w, below n-s, or past it --, softmax over the window's keys, times v, back to the original
positions.  The bound is the project's for a HIP kernel on its ATen route: error against float64 at most twice ATen's on
the same input, plus 1e-6 (test_gpu_text_tower._bound); both errors are printed."""
import json
import os

import numpy as np
import pytest
import torch

import swin_recipe as recipe
import test_gpu_encoder_frames as EF
import test_gpu_stream_contracts as S
import test_gpu_text_tower as TT
import util
from conv_fuzz import reference64, region  # noqa: F401  (K31's float64 reference: the fuzzer's)
from test_gpu_text_tower import spin_cycles  # noqa: F401  (the fixture)
from util import int_bits, nerr

pytestmark = pytest.mark.gpu

NAN = float("nan")
_bound = TT._bound                      # e <= 2 * (ATen's error against float64) + 1e-6
MCD_E_ARG, MCD_E_UNSUPPORTED = -1, -5
FILL_BITS = int(int_bits(torch.full((1,), util.OUT_FILL))[0])


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
    assert not bool((int_bits(out) == FILL_BITS).any()), "an output element was not written"


# ---- K31 ------------------------------------------------------------------------------------------------------------------
def k31(L, qkv, pad, H, W, heads, w, s, table, gap=NAN):
    """K31 on framed operands: qkv, pad_qkv and the table inside guards of `gap`, the output in a frame of OUT_FILL whose
    guards must come back intact and whose every element must have been written; the inputs untouched."""
    B = qkv.shape[0]
    q_, t_ = EF.In(qkv, gap), EF.In(table, gap)
    p_ = None if pad is None else EF.In(pad, gap)
    o_ = EF.Out((B, H * W, heads * 32), qkv.device)
    EF.ok(L.mcd_window_attention(q_.ptr, None if p_ is None else p_.ptr, B, H, W, heads, w, s, t_.ptr, o_.ptr, EF.st()), L)
    out = o_.view.clone()
    o_.check(out, what=("K31", tuple(qkv.shape), H, W, w, s))
    written(out)
    for a in (q_, t_, p_):
        if a is not None:
            a.same()
    return out


# H, W, w, s
K31_SHAPES = [(21, 21, 7, 3),       # nine windows: interior, edge and corner masks
              (14, 21, 7, 0),
              (16, 24, 8, 4),       # all 64 lanes
              (4, 6, 2, 1),
              (7, 7, 7, 0),         # one window
              (10, 9, 7, 3),        # padded both ways
              (5, 5, 3, 1)]         # padded
_K31 = {}


def k31_inputs(dev, B, heads, H, W, w, seed):
    qkv = EF.rnd((B, H * W, 3 * heads * 32), seed, dev)
    pad = EF.rnd((3 * heads * 32,), seed + 1, dev, 1.0, 3.0)        # random, and unlike every real row (mean 3)
    table = EF.rnd(((2 * w - 1) ** 2, heads), seed + 2, dev)
    return qkv, pad, table


def k31_case(L, dev, shape, B, heads):
    """(qkv, pad_qkv, table, the framed K31 output) of a case, computed once and left unchanged."""
    key = (shape, B, heads)
    if key not in _K31:
        H, W, w, s = shape
        qkv, pad, table = k31_inputs(dev, B, heads, H, W, w, 7000 + 10 * K31_SHAPES.index(shape) + heads)
        _K31[key] = (qkv, pad, table, k31(L, qkv, pad, H, W, heads, w, s, table))
    return _K31[key]


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", K31_SHAPES, ids=lambda s: "%dx%d-w%d-s%d" % s)
def test_k31_against_float64(L, du, dev, shape, B, heads):
    H, W, w, s = shape
    qkv, pad, table, out = k31_case(L, dev, shape, B, heads)
    ref = reference64(qkv, pad, H, W, heads, w, s, table)
    aten = du._window_attend_aten(qkv, heads, (H, W), w, s, table, pad)
    _bound(nerr(out, ref), nerr(aten, ref), ("K31", shape, B, heads))
    if H % w or W % w:
        assert nerr(reference64(qkv, torch.zeros_like(pad), H, W, heads, w, s, table), ref) > 1e-3       # the padded keys matter
    if s > 0:
        assert nerr(reference64(qkv, pad, H, W, heads, w, 0, table), ref) > 1e-2                         # and so does the shift


def test_k31_one_token(L, du, dev):
    qkv, pad, table = k31_inputs(dev, 1, 1, 1, 1, 1, 7900)
    out = k31(L, qkv, None, 1, 1, 1, 1, 0, table)
    ref = reference64(qkv, None, 1, 1, 1, 1, 0, table)
    _bound(nerr(out, ref), nerr(du._window_attend_aten(qkv, 1, (1, 1), 1, 0, table, pad), ref), "K31 1x1")
    assert torch.equal(int_bits(out.view(-1)), int_bits(qkv.view(-1)[64:96]))          # one key: the output is v


def test_k31_a_window_does_not_know_where_it_is(L, dev):
    """The bit claims of the header: a window's rows depend on its own q, k, v, its mask pattern and the table alone."""
    B, heads = 3, 3
    qkv, pad, table = k31_inputs(dev, B, heads, 21, 21, 7, 7100)
    D = heads * 32
    grid = qkv.view(B, 21, 21, 3 * D)
    plain = k31(L, qkv, pad, 21, 21, heads, 7, 0, table).view(B, 21, 21, D)
    centre = k31(L, grid[:, 7:14, 7:14].reshape(B, 49, 3 * D).contiguous(), None, 7, 7, heads, 7, 0, table)
    assert torch.equal(int_bits(plain[:, 7:14, 7:14].reshape(B, 49, D)), int_bits(centre))
    # shifted by 3: the window at the rolled origin holds the tokens of rows and columns 3 .. 9 and no mask
    shifted = k31(L, qkv, pad, 21, 21, heads, 7, 3, table).view(B, 21, 21, D)
    inner = k31(L, grid[:, 3:10, 3:10].reshape(B, 49, 3 * D).contiguous(), None, 7, 7, heads, 7, 0, table)
    assert torch.equal(int_bits(shifted[:, 3:10, 3:10].reshape(B, 49, D)), int_bits(inner))
    assert not torch.equal(int_bits(shifted), int_bits(plain))
    # an image alone and inside a batch; with padding too
    for shape in ((21, 21, 7, 3), (10, 9, 7, 3)):
        H, W, w, s = shape
        q3, p3, t3, out3 = k31_case(L, dev, shape, 3, 3)
        for b in range(3):
            alone = k31(L, q3[b:b + 1].contiguous(), p3, H, W, 3, w, s, t3)
            assert torch.equal(int_bits(alone[0]), int_bits(out3[b])), (shape, b)


def test_k31_a_nan_stays_in_its_window_and_head(L, dev):
    H = W = 21
    w, s, heads = 7, 3, 3
    qkv, pad, table, clean = k31_case(L, dev, (H, W, w, s), 1, heads)
    dirty = qkv.clone()
    y, x, h = 12, 5, 1                                    # rolled to (9, 2): the window of rolled rows 7 .. 13, columns 0 .. 6
    dirty.view(1, H, W, 3, heads, 32)[0, y, x, 1, h, 17] = NAN        # one element of that token's k
    out = k31(L, dirty, pad, H, W, heads, w, s, table).view(H, W, heads, 32)
    hit = torch.zeros(H, W, heads, 32, dtype=torch.bool)
    hit[10:17, 3:10, h] = True                            # the original positions of that rolled window
    assert torch.equal(torch.isnan(out).cpu(), hit)
    assert torch.equal(torch.isnan(reference64(dirty, pad, H, W, heads, w, s, table)).view(H, W, heads, 32), hit)
    assert torch.equal(int_bits(out.cpu()[~hit]), int_bits(clean.view(H, W, heads, 32).cpu()[~hit]))


def test_k31_argument_errors_come_without_a_launch(L, mcd, dev):
    B, heads, H, W, w = 2, 2, 5, 5, 3
    qkv, pad, table = k31_inputs(dev, B, heads, H, W, w, 7200)
    out = torch.full((B, H * W, heads * 32), util.OUT_FILL, device=dev)
    q, p, t, o = qkv.data_ptr(), pad.data_ptr(), table.data_ptr(), out.data_ptr()

    def rc(*a):
        return util.entry_rc(mcd, "mcd_window_attention", *a, EF.st())
    bad = [((q, p, B, H, W, heads, 9, 0, t, o), MCD_E_UNSUPPORTED),            # a window of 81 tokens
           ((q, p, B, H, W, heads, w, w, t, o), MCD_E_ARG),                    # s >= w
           ((q, p, B, H, W, heads, w, -1, t, o), MCD_E_ARG),
           ((q, p, B, H, W, heads, 0, 0, t, o), MCD_E_ARG),
           ((q, p, 65536, H, W, heads, w, 1, t, o), MCD_E_UNSUPPORTED),
           ((q, p, B, H, W, 65536, w, 1, t, o), MCD_E_UNSUPPORTED),
           ((q, p, B, 4096, 4096, 3, 8, 0, t, o), MCD_E_UNSUPPORTED),          # one image's qkv: 18 GiB
           ((q, p, B, 2048, 2731, 1, 8, 0, t, o), MCD_E_UNSUPPORTED),          # the first width past 2^31 bytes an image
           ((q, p, -1, H, W, heads, w, 1, t, o), MCD_E_ARG),
           ((q, p, B, 0, W, heads, w, 1, t, o), MCD_E_ARG),
           ((q, p, B, H, W, 0, w, 1, t, o), MCD_E_ARG),
           ((None, p, B, H, W, heads, w, 1, t, o), MCD_E_ARG),
           ((q, p, B, H, W, heads, w, 1, None, o), MCD_E_ARG),
           ((q, p, B, H, W, heads, w, 1, t, None), MCD_E_ARG),
           ((q, None, B, H, W, heads, w, 1, t, o), MCD_E_ARG),                 # 5 x 5 under window 3 is padded
           ((q + 4, p, B, H, W, heads, w, 1, t, o), MCD_E_ARG),
           ((q, p + 4, B, H, W, heads, w, 1, t, o), MCD_E_ARG),
           ((q, p, B, H, W, heads, w, 1, t, o + 8), MCD_E_ARG),
           ((q, p, B, H, W, heads, w, 1, t + 2, o), MCD_E_ARG)]
    for args, code in bad:
        assert rc(*args) == code, (args[2:8], code)
        assert L.mcd_last_error().decode().startswith("mcd_window_attention")
    assert rc(q, p, 0, H, W, heads, w, 1, t, o) == 0                            # B == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((int_bits(out) == FILL_BITS).all()), "a refused call wrote to its output"
    assert rc(q, p, B, H, W, heads, w, 1, t, o) == 0
    torch.cuda.synchronize()
    written(out)


def test_core_window_attention(core, L, dev):
    H, W, w, s = 10, 9, 7, 3
    qkv, pad, table, out = k31_case(L, dev, (H, W, w, s), 3, 3)
    assert torch.equal(int_bits(core.window_attention(qkv, (H, W), w, s, table, pad)), int_bits(out))
    into = torch.empty_like(out)
    assert core.window_attention(qkv, (H, W), w, s, table, pad.view(3, 3, 32), out=into) is into and torch.equal(int_bits(into), int_bits(out))
    with pytest.raises(core.McdError):
        core.window_attention(qkv, (H, W), w, s, table)               # a padded grid needs pad_qkv
    for bad in (dict(qkv=qkv.double()), dict(qkv=qkv.transpose(0, 1)), dict(table=table.t()), dict(pad_qkv=pad[:-1])):
        with pytest.raises(TypeError):
            core.window_attention(**dict(dict(qkv=qkv, grid=(H, W), window=w, shift=s, table=table, pad_qkv=pad), **bad))
    for bad in (dict(grid=(H, W + 1)), dict(window=6), dict(table=table[:, :2].contiguous())):
        with pytest.raises(ValueError):
            core.window_attention(**dict(dict(qkv=qkv, grid=(H, W), window=w, shift=s, table=table, pad_qkv=pad), **bad))
    with pytest.raises(TypeError):
        core.window_attention(qkv.cpu(), (H, W), w, s, table.cpu(), pad.cpu())


# ---- K32 ------------------------------------------------------------------------------------------------------------------
def gathered(x, H, W):
    """transformers' gather in torch: [B, H*W, C] -> [B, ceil(H/2)*ceil(W/2), 4C], zeros past an odd edge."""
    B, _, C = x.shape
    g = torch.nn.functional.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    g = torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], dim=-1)
    return g.reshape(B, -1, 4 * C).contiguous()


K32_SHAPES = [(2, 4, 6, 8), (1, 2, 2, 4), (3, 14, 14, 96), (2, 5, 7, 32), (1, 1, 1, 4), (2, 2, 2, 512)]


@pytest.mark.parametrize("shape", K32_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_k32_is_k10_on_the_gathered_rows(L, core, dev, shape):
    B, H, W, C = shape
    x = EF.rnd((B, H * W, C), 8000 + C + H, dev, 2.0, 0.5)
    g, b = EF.rnd((4 * C,), 8001 + C, dev, 0.2, 1.0), EF.rnd((4 * C,), 8002 + C, dev, 0.1)
    want = core.layer_norm(gathered(x, H, W), g, b, 1e-5)
    rows = ((H + 1) // 2) * ((W + 1) // 2)
    assert tuple(want.shape) == (B, rows, 4 * C)
    EF.run_framed(L, lambda i, o: L.mcd_patch_merge_ln(i[0], B, H, W, C, i[1], i[2], 1e-5, o[0], EF.st()), [x, g, b],
                  [(B, rows, 4 * C)], ("K32", shape), expect=[want])          # the guards stay intact, the bits are K10's
    assert torch.equal(int_bits(core.patch_merge_ln(x, (H, W), g, b, 1e-5)), int_bits(want))
    ref = torch.nn.functional.layer_norm(gathered(x, H, W).double().cpu(), (4 * C,), g.double().cpu(), b.double().cpu(), 1e-5)
    assert nerr(want, ref) < 2e-6


def test_k32_argument_errors(L, mcd, core, dev):
    x, g, b = EF.rnd((2, 16, 520), 1, dev), EF.rnd((2080,), 2, dev), EF.rnd((2080,), 3, dev)
    out = torch.full((2, 4, 2080), util.OUT_FILL, device=dev)

    def rc(*a):
        return util.entry_rc(mcd, "mcd_patch_merge_ln", *a, EF.st())
    X, G, Bt, O = x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr()
    assert rc(X, 2, 4, 4, 516, G, Bt, 1e-5, O) == MCD_E_UNSUPPORTED              # 4C = 2064 > 2048
    assert rc(X, 2, 4, 4, 6, G, Bt, 1e-5, O) == MCD_E_ARG                        # C % 4
    assert rc(X, 2, 4, 4, 0, G, Bt, 1e-5, O) == MCD_E_ARG
    assert rc(X, -1, 4, 4, 8, G, Bt, 1e-5, O) == MCD_E_ARG
    assert rc(X, 2, 0, 4, 8, G, Bt, 1e-5, O) == MCD_E_ARG
    assert rc(None, 2, 4, 4, 8, G, Bt, 1e-5, O) == MCD_E_ARG
    assert rc(X, 2, 4, 4, 8, G, Bt, 1e-5, None) == MCD_E_ARG
    assert rc(X + 4, 2, 4, 4, 8, G, Bt, 1e-5, O) == MCD_E_ARG
    assert rc(X, 2, 32768, 32768, 8, G, Bt, 1e-5, O) == MCD_E_UNSUPPORTED        # one image of 2^33 bytes
    assert rc(X, 0, 4, 4, 8, G, Bt, 1e-5, O) == 0
    torch.cuda.synchronize()
    assert bool((int_bits(out) == FILL_BITS).all())
    with pytest.raises(ValueError):
        core.patch_merge_ln(x, (4, 5), g, b, 1e-5)
    with pytest.raises(TypeError):
        core.patch_merge_ln(x, (4, 4), g[:-4], b[:-4], 1e-5)


# ---- the stream and capture contracts, with test_gpu_stream_contracts' machinery ---------------------------------------------
def b_window(L, dev):
    B, H, W, heads, w, s = 2, 5, 5, 2, 3, 1
    return S.simple(L, dev, "K31", [S._gen((B, H * W, 3 * heads * 32)), S._gen((3 * heads * 32,), 1.0, 3.0), S._gen(((2 * w - 1) ** 2, heads))],
                    [(B, H * W, heads * 32)], lambda i, o, st: L.mcd_window_attention(i[0], i[1], B, H, W, heads, w, s, i[2], o[0], st))


def b_merge(L, dev):
    B, H, W, C = 2, 5, 7, 32
    return S.simple(L, dev, "K32", [S._gen((B, H * W, C), 2.0, 0.5), S._gen((4 * C,), 0.2, 1.0), S._gen((4 * C,), 0.1)],
                    [(B, 3 * 4, 4 * C)], lambda i, o, st: L.mcd_patch_merge_ln(i[0], B, H, W, C, i[1], i[2], 1e-5, o[0], st))


SWIN_STREAM_ROWS = {"mcd_window_attention": b_window, "mcd_patch_merge_ln": b_merge}


def test_stream_rows_cover_the_header(mcd):
    assert sorted(SWIN_STREAM_ROWS) == sorted(mcd._lib.SWIN_SIGNATURES)


@pytest.mark.parametrize("entry", sorted(SWIN_STREAM_ROWS))
def test_the_call_is_ordered_on_its_stream(L, dev, spin_cycles, entry):  # noqa: F811
    r = S.Run(entry, SWIN_STREAM_ROWS[entry](L, dev), dev)
    snaps, want = S.side_stream(r, spin_cycles, lambda st: st.cuda_stream)
    r.same(snaps, want, entry)


@pytest.mark.parametrize("entry", sorted(SWIN_STREAM_ROWS))
def test_capture_and_replay(L, dev, entry):
    """The entry alone in a captured graph (one kernel node: no parallel branches), replayed on fresh data to the eager bits."""
    r = S.Run(entry, SWIN_STREAM_ROWS[entry](L, dev), dev)
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


# ---- the tower --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(util.GOLDEN, "swin.npz")), json.load(open(os.path.join(util.GOLDEN, "swin_meta.json")))


def tower_of(du, dev, name):
    sd, _ = recipe.weights(recipe.CONFIGS[name], recipe.SEED[name])
    return du.SwinTower.from_state_dict(sd).eval().to(dev)


def rows_of(tower, image):
    rows, hooks = {}, []
    for i, stage in enumerate(tower.encoder.layers):
        hooks.append(stage.register_forward_hook(lambda m, a, o, i=i: rows.__setitem__("stage%d" % i, o[:, 0].detach().clone())))
        for j, blk in enumerate(stage.blocks):
            hooks.append(blk.register_forward_hook(
                lambda m, a, o, i=i, j=j: rows.__setitem__("stage%d_block%d" % (i, j), o[:, 0].detach().clone())))
    with torch.no_grad():
        rows["norm"] = tower(image)
    for h in hooks:
        h.remove()
    return rows


def accept(got, z, name, what):
    """test_gpu_mae.accept's rule on this fixture's rows: within twice the fp32 fixture's own distance to the float64
    fixture, plus 1e-6.  Returns the distances."""
    keys = sorted(k[len(name) + 1:-4] for k in z.files if k.startswith(name + "_") and k.endswith("_f64"))
    assert sorted(got) == keys
    dist = {}
    for k in keys:
        f64 = torch.from_numpy(z["%s_%s_f64" % (name, k)])
        e_ref = nerr(torch.from_numpy(z["%s_%s_f32" % (name, k)]), f64)
        dist[k] = nerr(got[k], f64)
        print("%s %s %s: %.3e, fixture's fp32 %.3e, ratio to the bound %.3f" % (what, name, k, dist[k], e_ref,
                                                                                 dist[k] / (2 * e_ref + 1e-6)))
        assert tuple(got[k].shape) == tuple(f64.shape), (name, k)
        assert dist[k] <= 2 * e_ref + 1e-6, (what, name, k, dist[k], e_ref)
    return dist


SWIN_WRAPPERS = ["window_attention", "patch_merge_ln", "layer_norm"]


@pytest.mark.parametrize("name", ["small", "padded"])
def test_hip_route_against_float64_and_against_aten(du, fixture, dev, monkeypatch, name):
    z, _ = fixture
    tower = tower_of(du, dev, name)
    image = recipe.make_image(name).to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    with torch.no_grad():
        assert tower.route(image) == "hip"
    calls = util.CallCounter(du.core, monkeypatch, SWIN_WRAPPERS)
    hip = rows_of(tower, image)
    blocks, merges = sum(recipe.CONFIGS[name]["depths"]), len(recipe.CONFIGS[name]["depths"]) - 1
    assert calls.n["window_attention"] == blocks and calls.n["patch_merge_ln"] == merges          # every block on K31, every merge on K32
    assert calls.n["layer_norm"] == 2 * blocks + 2                     # layernorm_before / after, embeddings.norm, layernorm
    e_hip = accept(hip, z, name, "HIP route")
    calls.n.clear()
    monkeypatch.setattr(du, "HIP_SWIN", False)                         # what MCD_NO_HIP_SWIN=1 sets at import
    with torch.no_grad():
        assert tower.route(image) == "aten"
    aten = rows_of(tower, image)
    assert "window_attention" not in calls.n and "patch_merge_ln" not in calls.n
    e_aten = accept(aten, z, name, "ATen route on the GPU")
    for k in sorted(hip):                                              # the two routes against each other, float64 the arbiter
        print("%s %s: HIP %.3e, ATen %.3e" % (name, k, e_hip[k], e_aten[k]))
        assert e_hip[k] <= 2 * e_aten[k] + 1e-6, (name, k, e_hip[k], e_aten[k])


def test_a_hook_inside_a_block_sends_that_block_alone_to_aten(du, fixture, dev, monkeypatch):
    z, _ = fixture
    tower = tower_of(du, dev, "small")
    image = recipe.make_image("small").to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    calls = util.CallCounter(du.core, monkeypatch, SWIN_WRAPPERS)
    seen = []
    h = tower.encoder.layers[0].blocks[1].attention.register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape)))
    h2 = tower.encoder.layers[0].downsample.norm.register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape)))
    try:
        got = rows_of(tower, image)
    finally:
        h.remove()
        h2.remove()
    assert seen == [(recipe.BATCH * 4, 49, 32), (recipe.BATCH, 49, 128)]        # the windows of a 14 x 14 grid; the merged rows
    assert calls.n["window_attention"] == 3 and "patch_merge_ln" not in calls.n
    accept(got, z, "small", "HIP route, one block and the merge on ATen")


def test_the_dissection_hooks_see_token_0_on_both_routes(du, mcd, fixture, dev, monkeypatch):
    from mammo_clip_dissect_amd.concept_vit import utils
    z, _ = fixture
    tower = tower_of(du, dev, "padded")
    image = recipe.make_image("padded").to(dev)
    monkeypatch.setenv("MCD_BLASLT_PICK", "heuristic")
    got = {}
    for route in ("hip", "aten"):
        monkeypatch.setattr(du, "HIP_SWIN", route == "hip")
        outs = [[] for _ in tower.encoder.layers]
        hooks = [st.register_forward_hook(utils.get_activation(o, "avg")) for st, o in zip(tower.encoder.layers, outs)]
        direct = rows_of(tower, image)
        for hk in hooks:
            hk.remove()
        assert all(len(o) == 1 for o in outs)
        for i, o in enumerate(outs):                                   # K0 on a 3-D output: token 0, bit for bit
            assert torch.equal(int_bits(o[0]), int_bits(direct["stage%d" % i]))
        got[route] = [o[0] for o in outs]
    for i, (a, b) in enumerate(zip(got["hip"], got["aten"])):
        f64 = torch.from_numpy(z["padded_stage%d_f64" % i])
        assert tuple(a.shape) == tuple(f64.shape)
        assert nerr(a, f64) <= 2 * nerr(b, f64) + 1e-6, (i, nerr(a, f64), nerr(b, f64))


def test_breastclip_swin_encodes_on_the_hip_route(du, fixture, dev, monkeypatch):
    z, _ = fixture
    cfg = recipe.CONFIGS["small"]
    sd, _ = recipe.weights(cfg, recipe.SEED["small"])
    ckpt = {du.SWIN_PREFIX + k: v for k, v in dict(sd, **recipe.index_buffers(cfg)).items()}
    model, _ = du.get_target_model("breastclip_swin", dev, ckpt=ckpt)
    calls = util.CallCounter(du.core, monkeypatch, SWIN_WRAPPERS)
    with torch.no_grad():
        feat = model.encode_image(recipe.make_image("small").to(dev))
    assert calls.n["window_attention"] == 4
    f64 = torch.from_numpy(z["small_norm_f64"])[:, 0]
    assert nerr(feat, f64) <= 2 * nerr(torch.from_numpy(z["small_norm_f32"])[:, 0], f64) + 1e-6


# ---- B2 ---------------------------------------------------------------------------------------------------------------------
def test_the_b2_tower_runs_on_the_mbconv_route(du, core, dev, monkeypatch):
    """A seeded breastclip at B2's scaling (width 1.1, depth 1.2) built from its own state dict: every block on the HIP
    route, and the tower within test_gpu_mbconv's bound -- error against a float64 CPU forward at most twice the ATen
    route's, plus 1e-6, block by block and at the output."""
    torch.manual_seed(11)
    src = du.EfficientNetTower(width=1.1, depth=1.2)
    util.mild_bn(src, 2)
    model, _ = du.get_target_model("breastclip", "cpu", ckpt={"image_encoder." + k: v for k, v in src.state_dict().items()})
    tower = model.image_encoder
    assert tower.out_dim == 1408 and len(tower._blocks) == 23
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))

    def hooked(net, xin, routes=None):
        outs = []
        hs = [b.register_forward_hook(lambda m, i, o: outs.append(o.detach().double().cpu())) for b in net._blocks]
        if routes is not None:
            hs += [b.register_forward_pre_hook(lambda m, i: routes.append(du.mbconv_route(m, i[0]))) for b in net._blocks]
        with torch.no_grad():
            y = net(xin)
        for h in hs:
            h.remove()
        return y, outs
    ref, ref_outs = hooked(tower.double(), x.double())
    tower.float().to(dev)
    monkeypatch.setattr(du, "HIP_MBCONV", False)
    aten, aten_outs = hooked(tower, x.to(dev))
    monkeypatch.setattr(du, "HIP_MBCONV", True)
    routes = []
    cnt = util.CallCounter(core, monkeypatch, ["conv_stem_nhwc", "dwconv_bn_silu", "se_gate", "channel_scale_", "silu_avg_pool_nhwc"])
    got, got_outs = hooked(tower, x.to(dev), routes)
    assert routes == ["hip"] * 23
    assert cnt.n == {"conv_stem_nhwc": 1, "dwconv_bn_silu": 23, "se_gate": 23, "channel_scale_": 23, "silu_avg_pool_nhwc": 1}
    assert tuple(got.shape) == (2, 1408) and len(got_outs) == 23
    for j, (a, b, r) in enumerate(zip(got_outs, aten_outs, ref_outs)):
        assert nerr(a, r) <= 2 * nerr(b, r) + 1e-6, (j, nerr(a, r), nerr(b, r))
    assert nerr(got, ref) <= 2 * nerr(aten, ref) + 1e-6, (nerr(got, ref), nerr(aten, ref))
