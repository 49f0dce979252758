"""The Swin tower's HIP route (HIP_SWIN) on one MI355X, fp32:
  * swin-tiny (data_utils.SwinTower's defaults, seeded weights) at 224 x 224, batch 250, and at Mammo-CLIP's 1520 x 912,
    batch 8: the forward on the HIP route against the ATen route of the same modules (what MCD_NO_HIP_SWIN=1 selects), the
    two alternated inside one process, mean of MCD_SWIN_REPS forwards after 2 warm-ups each, HIP events; and the largest
    difference between the two outputs;
  * K31 (mcd_window_attention) alone on the qkv of every stage of both shapes, shifted and unshifted: ms, and the achieved
    bytes/s on the bytes the op has to move -- qkv read once, the output written once, B*T*4C*4 -- against the HBM peak
    (8.0 TB/s; a float4 copy reaches 6.3); beside it the same operands through ATen (data_utils._window_attend_aten);
  * K32 (mcd_patch_merge_ln) alone on every merge of both shapes: ms and bytes/s on B*T*C*4 read + the same written.
Writes profiles/swin_timing.txt.  Dev tool.
    MCD_SWIN_REPS=<n>   timed forwards per route (default 10)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import mammo_clip_dissect_amd as m  # noqa: F401
from mammo_clip_dissect_amd import core
from mammo_clip_dissect_amd.concept_vit import data_utils as du

dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12
REPS = int(os.environ.get("MCD_SWIN_REPS", "10"))
SHAPES = [(250, 224, 224), (8, 1520, 912)]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timeit(fn, n=REPS, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def forward(tower, x, hip):
    du.HIP_SWIN = hip
    with torch.no_grad():
        return tower(x)


def stage_grids(H, W, patch, stages):
    g = [(-(-H // patch), -(-W // patch))]
    for _ in range(stages - 1):
        g.append(((g[-1][0] + 1) // 2, (g[-1][1] + 1) // 2))
    return g


torch.manual_seed(0)
tower = du.SwinTower().to(dev).eval()
cfg = tower.config
say("Swin-T tower, fp32, %s" % torch.cuda.get_device_name(0))
for B, H, W in SHAPES:
    x = torch.randn(B, 3, H, W, device=dev)
    du.HIP_SWIN = True
    with torch.no_grad():
        assert tower.route(x) == "hip"
    t = {True: [], False: []}
    for _ in range(2):                               # alternated: HIP, ATen, HIP, ATen
        for hip in (True, False):
            t[hip].append(timeit(lambda: forward(tower, x, hip)))
    d = (forward(tower, x, True) - forward(tower, x, False)).abs().max().item()
    ref = forward(tower, x, False).abs().max().item()
    say("tower B=%3d %4dx%-4d: HIP route %8.2f ms (%.2f, %.2f)   ATen route %8.2f ms (%.2f, %.2f)   x%.2f   max |d| %.2e of %.2e"
        % (B, H, W, min(t[True]), t[True][0], t[True][1], min(t[False]), t[False][0], t[False][1], min(t[False]) / min(t[True]),
           d, ref))
    del x
    for i, (gh, gw) in enumerate(stage_grids(H, W, cfg["patch"], len(cfg["depths"]))):
        C, heads, w = cfg["width"] << i, cfg["heads"][i], cfg["window"][i]
        T = gh * gw
        if min(gh, gw) < w:
            say("  stage %d grid %dx%d is under the window %d" % (i, gh, gw, w))
            continue
        qkv = torch.randn(B, T, 3 * C, device=dev)
        pad = torch.randn(3 * C, device=dev)
        table = torch.randn((2 * w - 1) ** 2, heads, device=dev)
        nbytes = B * T * 4 * C * 4.0
        for s in ((0,) if min(gh, gw) == w else (0, w // 2)):
            ms = timeit(lambda: core.window_attention(qkv, (gh, gw), w, s, table, pad))
            with torch.no_grad():
                ms_aten = timeit(lambda: du._window_attend_aten(qkv, heads, (gh, gw), w, s, table, pad), n=max(2, REPS // 3))
            say("  K31 stage %d grid %3dx%-3d C=%3d heads=%2d shift %d: %7.3f ms  %6.2f TB/s on %.3f GB = %4.1f %% of the HBM peak;"
                "  ATen %8.3f ms" % (i, gh, gw, C, heads, s, ms, nbytes / ms / 1e9, nbytes / 1e9, 100 * nbytes / (ms * 1e-3) / HBM_PEAK,
                                    ms_aten))
        if i < len(cfg["depths"]) - 1 and du.swin_merge_route(C, T) == "k32":
            xs = torch.randn(B, T, C, device=dev)
            g, b = torch.randn(4 * C, device=dev), torch.randn(4 * C, device=dev)
            ms = timeit(lambda: core.patch_merge_ln(xs, (gh, gw), g, b, 1e-5))
            say("  K32 stage %d grid %3dx%-3d C=%3d: %7.3f ms  %6.2f TB/s on read + write" % (i, gh, gw, C, ms, 2 * B * T * C * 4.0 / ms / 1e9))
            del xs
        del qkv

out = os.path.join(ROOT, "profiles", "swin_timing.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
