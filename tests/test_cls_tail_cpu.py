"""CPU: the gate of the class-token-only tail (data_utils.cls_tail_route), the token0_only marker on the package's own
activation hooks, and encode_image on CPU tensors, which never leaves the full path."""
import itertools

import torch


def test_cls_tail_route_predicate(mcd):
    from mammo_clip_dissect_amd import core
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    ok = dict(flag=True, fused_ok=True, masked=False, training=False, T=197, D=768, heads=12, depth=12, hooks_clear=True,
              last_hooks_token0=True)
    assert du.cls_tail_route(**ok)
    for name, bad in (("flag", False), ("fused_ok", False), ("masked", True), ("training", True), ("T", 0),
                      ("T", core.VIT_ATTENTION_CLS_MAX_T + 1), ("D", 760), ("heads", 8), ("depth", 0),
                      ("hooks_clear", False), ("last_hooks_token0", False)):
        assert not du.cls_tail_route(**dict(ok, **{name: bad})), name
    assert du.cls_tail_route(**dict(ok, T=1, depth=1))
    assert du.cls_tail_route(**dict(ok, T=core.VIT_ATTENTION_CLS_MAX_T, D=512, heads=8))
    for flags in itertools.product([False, True], repeat=6):     # the six switches: all of them, or not taken
        f, fo, m, t, hc, h0 = flags
        want = f and fo and not m and not t and hc and h0
        assert du.cls_tail_route(f, fo, m, t, 197, 768, 12, 12, hc, h0) == want
    keep = du.HIP_ATTENTION
    du.HIP_ATTENTION = False
    try:
        assert not du.cls_tail_route(**ok)
    finally:
        du.HIP_ATTENTION = keep


def test_package_hooks_declare_token0_only(mcd):
    import cpu_ops
    from mammo_clip_dissect_amd.concept_vit import CLIP_og_utils, og_utils, utils
    from mammo_clip_dissect_amd.pipeline import Dissector
    for mod in (utils, og_utils, CLIP_og_utils):
        for mode in ("avg", "max"):
            assert mod.get_activation([], mode).token0_only is True
    dis = Dissector(4, ["a", "b"], [8, 8], 5, 16, "cpu", top_k=2, ops=cpu_ops)
    assert dis.hook(0).token0_only is True and dis.hook(1).token0_only is True


def test_token0_hooks_reads_the_marker(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    m = torch.nn.Linear(2, 2)
    assert du._token0_hooks(m)
    marked = lambda mod, i, o: None
    marked.token0_only = True
    h1 = m.register_forward_hook(marked)
    assert du._token0_hooks(m)
    h2 = m.register_forward_hook(lambda mod, i, o: None)
    assert not du._token0_hooks(m)
    h2.remove()
    h1.remove()


def test_encode_image_on_cpu_is_the_full_tower(mcd):
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    assert du.CLS_ONLY_TAIL
    torch.manual_seed(0)
    x = torch.randn(2, 3, 32, 32)
    tower = du.ViTTower(image_size=32, depth=2).eval()
    for p in tower.parameters():
        torch.nn.init.normal_(p, std=0.05)
    with torch.no_grad():
        full = tower(x)
        assert full.shape == (2, 5, 768)
        assert not tower._cls_tail_ok(tower.embed(x))
        assert torch.equal(tower(x, cls_only=True), full)
    for model, t in ((du.BreastClip("vit", image_size=32, text_depth=1), "image_encoder"),
                     (du.ClipViT(image_size=32, text_depth=1), "vision_model")):
        model.eval()
        seen = []
        h = getattr(model, t).encoder._modules[getattr(model, t).encoder._list_name][-1].register_forward_hook(
            lambda m, i, o: seen.append(tuple(o.shape)))
        with torch.no_grad():
            f = model.encode_image(x)
            ref = getattr(model, t)(x)[:, 0]
            if t == "vision_model":
                ref = model.visual_projection(ref)
        h.remove()
        assert torch.equal(f, ref)
        assert seen == [(2, 5, 768)] * 2
