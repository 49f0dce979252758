"""The OpenAI-CLIP RN50 / RN101 dissectors' HIP route (K19 in csrc/k_resnet.hip, K20-K21 in csrc/k_clip_rn.hip, with K18,
K9C and the library GEMMs) measured against the ATen route of the same modules.  Dev tool.

  --target NAME   clip_rn50 (default) or clip_rn101.
  --kernels [B]   K19 at the stem's shape, K20 at every shape the network pools (the stem, the three stride-2 blocks'
                  conv2 outputs and inputs) and K21 at the head's, batch B (default 250), 224 x 224: device events after a
                  warm-up; ms and GB/s (K19: TFLOP/s too), and beside each the ATen ops it replaces on the same device
                  (F.conv2d + batch norm + ReLU on the NCHW image; F.avg_pool2d on channels-last memory; cat(mean, x) +
                  pos).
  --tower [B]     the visual tower's forward (image -> embedding) at batch B (default 250), HIP route and ATen route of the
                  same module in alternation (--rounds R, default 5, of --iters N forwards each, default 5): ms per
                  forward of every round, the medians, their ratio and the run-to-run spread of each side.  The stages
                  (stem, layer1..4, attnpool) are timed the same way with device events around each.

Every measurement runs in a fresh child process of this script, started with subprocess (nothing replaces a process
image).  The route flag data_utils.HIP_CLIP_RN is a module attribute read at every call, so one child alternates the two
routes on the same weights and the same input."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 157.3
TARGETS = ("clip_rn50", "clip_rn101")
# (name, H, W, C) of every 2x2 pooling at a 224 x 224 input, width 64
POOLS = [("stem 112^2 x 64", 112, 112, 64), ("layer2 conv2 56^2 x 128", 56, 56, 128), ("layer2 skip 56^2 x 256", 56, 56, 256),
         ("layer3 conv2 28^2 x 256", 28, 28, 256), ("layer3 skip 28^2 x 512", 28, 28, 512),
         ("layer4 conv2 14^2 x 512", 14, 14, 512), ("layer4 skip 14^2 x 1024", 14, 14, 1024)]


def arg_n(flag, default):
    i = sys.argv.index(flag)
    return int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else default


def opt(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=timeout)
    if r.returncode != 0:
        sys.exit(r.returncode)


def timeit(fn, n=10):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def kernels_child(B):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd import core
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)

    def line(name, gb, ms, ms_aten, flop=None):
        extra = "" if flop is None else "  %6.1f TFLOP/s (%.3f of peak)" % (flop / ms / 1e9, flop / ms / 1e9 / PEAK)
        print("B=%d %-26s %7.3f GB  %8.3f ms  %5.2f TB/s%s   ATen %8.3f ms  ATen / HIP %.2f"
              % (B, name, gb, ms, gb / ms, extra, ms_aten, ms_aten / ms), flush=True)
    x = torch.randn(B, 3, 224, 224, device=dev, generator=g)
    w = torch.randn(32, 3, 3, 3, device=dev, generator=g) / 27 ** 0.5
    bn = torch.nn.BatchNorm2d(32).to(dev).eval()
    wt, bias = w.permute(1, 2, 3, 0).contiguous(), torch.randn(32, device=dev, generator=g)
    with torch.no_grad():
        ms = timeit(lambda: core.conv3x3s2_nhwc(x, wt, bias, relu=True))
        ms_a = timeit(lambda: F.relu(bn(F.conv2d(x, w, None, 2, 1))))
    line("K19 stem 3x3/2 3 -> 32", 4.0 * B * (3 * 224 * 224 + 32 * 112 * 112) / 1e9, ms, ms_a, 2.0 * B * 112 * 112 * 32 * 27)
    for name, H, W, C in POOLS:
        y = torch.randn(B, H, W, C, device=dev, generator=g)
        yn = y.permute(0, 3, 1, 2)                                   # channels-last memory, as the ATen route holds it
        ms = timeit(lambda: core.avgpool2_nhwc(y))
        ms_a = timeit(lambda: F.avg_pool2d(yn, 2))
        line("K20 " + name, 4.0 * B * C * H * W * 1.25 / 1e9, ms, ms_a)
    y = torch.randn(B, 49, 2048, device=dev, generator=g)
    pos = torch.randn(50, 2048, device=dev, generator=g)
    ms = timeit(lambda: core.attnpool_tokens(y, pos))
    ms_a = timeit(lambda: torch.cat([y.mean(dim=1, keepdim=True), y], dim=1) + pos)
    line("K21 tokens 49 x 2048", 4.0 * B * 2048 * 99 / 1e9, ms, ms_a)


def tower_child(B, target, rounds, iters):
    sys.path.insert(0, ROOT)
    import torch
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    dev = torch.device("cuda:0")
    net = du.get_target_model(target, dev)[0].visual
    x = torch.randn(B, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    stages = ["stem", "layer1", "layer2", "layer3", "layer4", "attnpool"]

    def forward_staged(marks):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        ev[0].record()
        if du.clip_rn_route(net, x) == "hip":
            h = net._stem_hip(x)
        else:
            h = net.stem(x)
        ev[1].record()
        for i, n in enumerate(stages[1:], 2):
            h = getattr(net, n)(h)
            ev[i].record()
        marks.append(ev)
        return h

    res = {"hip": [], "aten": []}
    per_stage = {"hip": [], "aten": []}
    with torch.no_grad():
        for route in ("hip", "aten"):                                # warm-up: library plans, MIOpen's searches, the folds
            du.HIP_CLIP_RN = route == "hip"
            for _ in range(3):
                net(x)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for route in ("hip", "aten"):
                du.HIP_CLIP_RN = route == "hip"
                res[route].append(timeit(lambda: net(x), iters))
        for route in ("hip", "aten"):
            du.HIP_CLIP_RN = route == "hip"
            marks = []
            for _ in range(iters):
                forward_staged(marks)
            torch.cuda.synchronize()
            per_stage[route] = [statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in marks) for i in range(len(stages))]
    med = {r: statistics.median(v) for r, v in res.items()}
    print(json.dumps({"tool": "scripts/clip_rn_timing.py --tower", "target": target, "batch": B, "rounds": rounds, "iters": iters,
                      "hip_ms": [round(v, 3) for v in res["hip"]], "aten_ms": [round(v, 3) for v in res["aten"]],
                      "hip_median_ms": round(med["hip"], 3), "aten_median_ms": round(med["aten"], 3),
                      "aten_over_hip": round(med["aten"] / med["hip"], 3),
                      "hip_spread": round((max(res["hip"]) - min(res["hip"])) / med["hip"], 4),
                      "aten_spread": round((max(res["aten"]) - min(res["aten"])) / med["aten"], 4),
                      "images_per_s_hip": round(B / med["hip"] * 1e3, 1), "images_per_s_aten": round(B / med["aten"] * 1e3, 1),
                      "stages": stages, "hip_stage_ms": [round(v, 3) for v in per_stage["hip"]],
                      "aten_stage_ms": [round(v, 3) for v in per_stage["aten"]]}), flush=True)


if __name__ == "__main__":
    target = opt("--target", "clip_rn50")
    if target not in TARGETS:
        sys.exit("--target: one of %s" % ", ".join(TARGETS))
    if "--child-kernels" in sys.argv:
        kernels_child(int(sys.argv[2]))
    elif "--child-tower" in sys.argv:
        tower_child(int(sys.argv[2]), target, int(opt("--rounds", "5")), int(opt("--iters", "5")))
    elif "--kernels" in sys.argv:
        child(["--child-kernels", str(arg_n("--kernels", 250))], 300)
    elif "--tower" in sys.argv:
        child(["--child-tower", str(arg_n("--tower", 250)), "--target", target, "--rounds", opt("--rounds", "5"), "--iters",
               opt("--iters", "5")], 600)
    else:
        print(__doc__)
