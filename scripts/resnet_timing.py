"""The ResNet targets' HIP route (K16-K18, csrc/k_resnet.hip) measured.  Dev tool.

  --target NAME   the network: resnet50 (default), resnet101, resnet152 (the same convolution shapes, other counts), or
                  a BasicBlock one, resnet18 / resnet34 / resnet18_places (K18 alone, conv2 with the skip as its residual
                  operand).  Applies to --kernels, --driver and --forwards.
  --kernels [B]   K16, K17 and K18 at every shape the network has at a 224 x 224 input (batch B, default 250): device
                  events after a warm-up; flop, ms, TFLOP/s and the fraction of the fp32 peak (157.3 TFLOP/s, the MFMA's
                  and the packed VALU's alike), and beside each convolution ATen's F.conv2d alone on the NCHW tensor
                  (MIOpen, the route the kernel replaces; its batch norm, ReLU and skip add are further kernels) on the
                  same device.
  --driver [N]    describe_clip_neurons.main() on synthetic_<N>_224 (default 10000), batch --batch (default 250), conv1 +
                  layer1..4, after a warm-up run on 2 batches: prints one JSON line with images/s.  --keep DIR copies the
                  CSV there (for --compare).
  --forwards [N]  N (default 4) forwards of the tower at batch 250, for a rocprofv3 --kernel-trace --stats pass.
  --compare A B   two descriptions.csv: how many neurons agree on the top-1 concept and on the top-5 images.
  --hf [R]        data_utils.HFResNet in microsoft/resnet-50's configuration (seeded weights, mild batch-norm statistics) at
                  batch --batch (default 250), 224 x 224, with the five hook points of a dissection (resnet.embedder,
                  resnet.encoder.stages[0..3]) pooled by K0 / K0n into an activation matrix as the drivers' hooks do; beside
                  it the torchvision-layout resnet50 with conv1 + layer1..4.  One child process: a warm-up of both routes,
                  then R rounds (default 3, at least 3) that alternate the HIP route and the ATen route (HIP_RESNET off,
                  what MCD_NO_HIP_RESNET=1 sets) of the same module on the same tree, --forwards-per-round (default 5)
                  forwards each, timed with device events.  Prints every round, then per model and route the median and
                  the spread (max - min) of the rounds in ms per forward, and one JSON line.  Every step (the warm-up, each
                  round of each route) runs under its own time limit: an alarm whose default action ends the process.

Every measurement of --kernels / --driver runs in a fresh child process of this script (the route flag MCD_NO_HIP_RESNET
is read at import, and MIOpen / hipBLASLt keep per-process state); the child is started with subprocess, nothing replaces
a process image.  The script only needs what the parent of the route had, so it can be copied into an older tree."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 157.3
LAYERS = "conv1,layer1,layer2,layer3,layer4"
# (name, Cin, Cout, H, W, k, stride, how many of them in the network)
CONVS = [("layer1 3x3", 64, 64, 56, 56, 3, 1, 3), ("layer2 3x3/2", 128, 128, 56, 56, 3, 2, 1),
         ("layer2 3x3", 128, 128, 28, 28, 3, 1, 3), ("layer3 3x3/2", 256, 256, 28, 28, 3, 2, 1),
         ("layer3 3x3", 256, 256, 14, 14, 3, 1, 5), ("layer4 3x3/2", 512, 512, 14, 14, 3, 2, 1),
         ("layer4 3x3", 512, 512, 7, 7, 3, 1, 2), ("layer2 ds 1x1/2", 256, 512, 56, 56, 1, 2, 1),
         ("layer3 ds 1x1/2", 512, 1024, 28, 28, 1, 2, 1), ("layer4 ds 1x1/2", 1024, 2048, 14, 14, 1, 2, 1)]
DEPTHS = {"resnet18": [2, 2, 2, 2], "resnet34": [3, 4, 6, 3], "resnet18_places": [2, 2, 2, 2], "resnet50": [3, 4, 6, 3],
          "resnet101": [3, 4, 23, 3], "resnet152": [3, 8, 36, 3]}
BASIC = ("resnet18", "resnet34", "resnet18_places")


def convs_of(target):
    """(name, Cin, Cout, H, W, k, stride, count, res) for every distinct K18 call of the network at 224 x 224; res: the
    call carries the skip as its residual operand (a BasicBlock's conv2)."""
    n = DEPTHS[target]
    if target not in BASIC:
        per = {"layer%d 3x3" % (i + 1): n[i] - (1 if i else 0) for i in range(4)}
        return [(c[0],) + c[1:7] + (per.get(c[0], 1), False) for c in CONVS]
    out, hw = [], 56
    for i, w in enumerate((64, 128, 256, 512)):
        name = "layer%d" % (i + 1)
        if i:
            out.append((name + " conv1 3x3/2", w // 2, w, hw, hw, 3, 2, 1, False))
            out.append((name + " ds 1x1/2", w // 2, w, hw, hw, 1, 2, 1, False))
            hw //= 2
        if n[i] - (1 if i else 0):
            out.append((name + " conv1 3x3", w, w, hw, hw, 3, 1, n[i] - (1 if i else 0), False))
        out.append((name + " conv2 3x3+res", w, w, hw, hw, 3, 1, n[i], True))
    return out


def arg_n(flag, default):
    i = sys.argv.index(flag)
    return int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else default


def opt(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def child(args, timeout):
    """Run this script again with `args` in a fresh process and pass its output through."""
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


def kernels_child(B, which, target):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd import core
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)

    def line(name, flop, ms, ms_aten):
        tf = flop / ms / 1e9
        print("B=%d %-16s %8.2f GFLOP  %8.3f ms  %6.1f TFLOP/s  %.3f of peak   ATen %8.3f ms  ATen / HIP %.2f"
              % (B, name, flop / 1e9, ms, tf, tf / PEAK, ms_aten, ms_aten / ms), flush=True)
    if which == "stem":
        x = torch.randn(B, 3, 224, 224, device=dev, generator=g)
        w = torch.randn(64, 3, 7, 7, device=dev, generator=g) / 12
        wt = w.permute(1, 2, 3, 0).contiguous()
        ms = timeit(lambda: core.conv7x7s2_nhwc(x, wt))
        ms_a = timeit(lambda: F.conv2d(x, w, None, 2, 3))
        line("K16 stem 7x7/2", 2.0 * B * 112 * 112 * 64 * 147, ms, ms_a)
        y = torch.randn(B, 112, 112, 64, device=dev, generator=g)
        sc, sh = torch.rand(64, device=dev, generator=g) + 0.5, torch.randn(64, device=dev, generator=g)
        ms = timeit(lambda: core.bn_relu_maxpool_nhwc(y, sc, sh))
        yn = y.permute(0, 3, 1, 2).contiguous()
        ms_a = timeit(lambda: F.max_pool2d(F.relu(yn * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), 3, 2, 1))
        gb = 4.0 * B * 64 * (112 * 112 + 56 * 56) / 1e9
        print("B=%d %-16s %8.2f GB     %8.3f ms  %6.2f TB/s                       ATen %8.3f ms  ATen / HIP %.2f"
              % (B, "K17 bn+relu+pool", gb, ms, gb / ms, ms_a, ms_a / ms), flush=True)
        return
    name, Cin, Cout, H, W, k, s, count, with_res = convs_of(target)[int(which)]
    pad = 1 if k == 3 else 0
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    x = torch.randn(B, H, W, Cin, device=dev, generator=g)
    w = torch.randn(Cout, Cin, k, k, device=dev, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, device=dev, generator=g)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    relu = k == 3
    if target in BASIC:      # conv1: ReLU on the way out; conv2: the skip, then the ReLU; the downsample bare
        res = torch.randn(B, Ho, Wo, Cout, device=dev, generator=g) if with_res else None
        ms = timeit(lambda: core.conv_igemm_nhwc(x, wt, b, k, s, relu_out=relu, res=res))
    else:
        ms = timeit(lambda: core.conv_igemm_nhwc(x, wt, b, k, s, relu_in=relu, relu_out=relu))
    xn = x.permute(0, 3, 1, 2).contiguous()
    ms_a = timeit(lambda: F.conv2d(xn, w, None, s, pad))             # the convolution alone: bn and relu are extra kernels
    line("K18 %s (x%d)" % (name, count), 2.0 * B * Ho * Wo * Cout * k * k * Cin, ms, ms_a)


def driver_child(n, batch, keep, target):
    sys.path.insert(0, ROOT)
    import torch
    import mammo_clip_dissect_amd as m
    from mammo_clip_dissect_amd.concept_vit import data_utils, describe_clip_neurons as drv
    concepts = os.path.join(os.path.dirname(m.__file__), "Concepts", "Specific_concepts_sorted.txt")
    route = "hip" if getattr(data_utils, "HIP_RESNET", False) else "aten"
    for count in (2 * batch, n):
        tmp = tempfile.mkdtemp()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = drv.main(["--target_model", target, "--target_layers", LAYERS, "--d_probe",
                            "synthetic_%d_224" % count, "--concept_set", concepts, "--batch_size", str(batch), "--device",
                            "cuda:0", "--activation_dir", tmp + "/acts", "--result_dir", tmp + "/results"])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if keep and count == n:
                os.makedirs(keep, exist_ok=True)
                shutil.copy(os.path.join(out, "descriptions.csv"), os.path.join(keep, "descriptions_%s.csv" % route))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({"tool": "scripts/resnet_timing.py --driver", "target": target, "route": route, "images": n, "batch": batch,
                      "layers": LAYERS, "seconds": round(dt, 3), "images_per_s": round(n / dt, 1)}), flush=True)


def forwards_child(n, target):
    sys.path.insert(0, ROOT)
    import torch
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd.concept_vit import data_utils
    dev = torch.device("cuda:0")
    net, _ = data_utils.get_target_model(target, dev)
    x = torch.randn(250, 3, 224, 224, device=dev)
    with torch.no_grad():
        for _ in range(n):
            net(x)
    torch.cuda.synchronize()
    print("%d forwards done, route %s" % (n, "hip" if getattr(data_utils, "HIP_RESNET", False) else "aten"))


def hf_child(rounds, batch, per_round, limit):
    import signal
    import statistics
    sys.path.insert(0, ROOT)
    import torch
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd import core
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    dev = torch.device("cuda:0")

    def seeded(net):
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    n = m.num_features
                    m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                    m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                    m.weight.copy_(1 + 0.2 * torch.randn(n, generator=g))
                    m.bias.copy_(0.1 * torch.randn(n, generator=g))
        return net.eval().to(dev)
    torch.manual_seed(0)
    models = {"HFResNet (microsoft/resnet-50)": (seeded(du.HFResNet()), ["resnet.embedder"]
                                                 + ["resnet.encoder.stages.%d" % i for i in range(4)]),
              "resnet50 (torchvision layout)": (seeded(du.ResNet50()), ["conv1", "layer1", "layer2", "layer3", "layer4"])}
    x = torch.randn(batch, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for name, (net, layers) in models.items():
        for layer in layers:
            dst = {}

            def hook(m, a, o, dst=dst):                  # the drivers' hook body: pool into the activation matrix
                if "t" not in dst:
                    dst["t"] = torch.empty((o.shape[0], o.shape[1]), dtype=torch.float32, device=o.device)
                core.hook_pool(o, "avg", dst["t"], 0, 0, False)
            net.get_submodule(layer).register_forward_hook(hook)

    def step(net, hip, n):
        """n forwards on one route under the step's own time limit; ms per forward by device events."""
        signal.alarm(limit)
        du.HIP_RESNET = hip
        with torch.no_grad():
            net(x)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                net(x)
            e.record()
            torch.cuda.synchronize()
        signal.alarm(0)
        return s.elapsed_time(e) / n
    result = {"tool": "scripts/resnet_timing.py --hf", "batch": batch, "rounds": rounds, "forwards_per_round": per_round}
    for name, (net, layers) in models.items():
        for hip in (True, False):                        # the warm-up: plans, picks, MIOpen's find, the folded weights
            step(net, hip, 2)
        ms = {True: [], False: []}
        for r in range(rounds):
            for hip in (True, False):
                ms[hip].append(step(net, hip, per_round))
                print("%-32s round %d  %-4s %9.3f ms / forward" % (name, r, "hip" if hip else "aten", ms[hip][-1]), flush=True)
        for hip in (True, False):
            med, spread = statistics.median(ms[hip]), max(ms[hip]) - min(ms[hip])
            print("%-32s %-4s median %9.3f ms  spread %7.3f ms  (%d rounds of %d forwards, batch %d, %d hook points)"
                  % (name, "hip" if hip else "aten", med, spread, rounds, per_round, batch, len(layers)), flush=True)
            result["%s %s" % (name, "hip" if hip else "aten")] = {"median_ms": round(med, 3), "spread_ms": round(spread, 3),
                                                                   "rounds_ms": [round(v, 3) for v in ms[hip]]}
    print(json.dumps(result), flush=True)


def compare(a, b):
    import pandas as pd
    da, db = pd.read_csv(a), pd.read_csv(b)
    assert len(da) == len(db) and (da.layer == db.layer).all() and (da.unit == db.unit).all()
    same_c = da.description == db.description
    same_i = da.images.astype(str) == db.images.astype(str)
    print("neurons %d  top-1 concept agrees %d  top-5 images agree %d" % (len(da), int(same_c.sum()), int(same_i.sum())))
    for i in da.index[~same_c][:40]:
        print("  %s[%d]: %r (%.6f) vs %r (%.6f)" % (da.layer[i], da.unit[i], da.description[i], da.similarity[i],
                                                      db.description[i], db.similarity[i]))


if __name__ == "__main__":
    target = opt("--target", "resnet50")
    if target not in DEPTHS:
        sys.exit("--target: one of %s" % ", ".join(sorted(DEPTHS)))
    if "--child-hf" in sys.argv:
        hf_child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    elif "--hf" in sys.argv:
        child(["--child-hf", str(max(arg_n("--hf", 3), 3)), opt("--batch", "250"), opt("--forwards-per-round", "5"),
               opt("--step-limit", "120")], 900)
    elif "--child-kernels" in sys.argv:
        kernels_child(int(sys.argv[2]), sys.argv[3], target)
    elif "--child-driver" in sys.argv:
        driver_child(int(sys.argv[2]), int(sys.argv[3]), opt("--keep", None), target)
    elif "--kernels" in sys.argv:
        B = arg_n("--kernels", 250)
        for which in ["stem"] + [str(i) for i in range(len(convs_of(target)))]:
            child(["--child-kernels", str(B), which, "--target", target], 300)
    elif "--driver" in sys.argv:
        keep = opt("--keep", None)
        child(["--child-driver", str(arg_n("--driver", 10000)), opt("--batch", "250"), "--target", target]
              + (["--keep", keep] if keep else []), 900)
    elif "--forwards" in sys.argv:
        forwards_child(arg_n("--forwards", 4), target)
    elif "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        compare(sys.argv[i + 1], sys.argv[i + 2])
    else:
        print(__doc__)
