"""The HF ViT / DINOv2 targets' HIP route measured: K9L with a ragged last query block against another build of the
library, and the `dino` tower forward against the ATen route of the same module.  Dev tool.

  --k9l --other-lib PATH   mcd_vit_attention_long at (B, 12 heads, T) for T in 256, 257, 512, 5416 (--batch B, default 250)
                  from this tree's libmcd_hip.so and from the libmcd_hip.so at PATH (a build of the parent commit, say),
                  both loaded into ONE child process and timed in alternation on the same buffers (--rounds R, default 7,
                  of --iters N calls each, default 10; 3 at T = 5416): ms per call of every round, the medians, each side's
                  run-to-run spread (max - min over the median) and other / tree.  T = 256 and 512 are whole-block shapes
                  (the two builds should tie); 257 has a one-query last block; 5416 a last block of 2 live waves of 8.
  --tower [B]     the `dino` target's forward (image -> logits) at batch B (default 250), 224 x 224 (257 tokens): HIP route
                  and ATen route (HIP_ATTENTION, FUSED_RESIDUAL, HIP_LAYER_NORM off) of the same module in alternation
                  (--rounds, --iters, defaults 5 and 5): ms per forward, medians, ratio, spreads -- and the HIP route's
                  time by kernel (device events around every wrapper call of one forward): K11, K10, K9L, the library
                  GEMMs, and the rest (GELU, the patch mean, cat).

Every measurement runs in a fresh child process of this script, started with subprocess (nothing replaces a process
image)."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K9L_T = (256, 257, 512, 5416)


def arg_n(flag, default):
    i = sys.argv.index(flag)
    return int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else default


def opt(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=timeout)
    if r.returncode != 0:
        sys.exit(r.returncode)


def timeit(fn, n, warm=3):
    import torch
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


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def k9l_child(other, B, rounds, iters):
    sys.path.insert(0, ROOT)
    import torch
    import mammo_clip_dissect_amd as m
    dev = torch.device("cuda:0")
    libs = {"tree": m._lib.load(), "other": ctypes.CDLL(other)}
    fn = libs["other"].mcd_vit_attention_long
    fn.restype, fn.argtypes = m._lib.SIGNATURES["mcd_vit_attention_long"]
    H = 12
    g = torch.Generator(device=dev).manual_seed(0)
    for T in K9L_T:
        qkv = torch.randn(B, T, 3 * H * 64, device=dev, generator=g)
        out = {k: torch.empty(B, T, H * 64, device=dev) for k in libs}
        stream = torch.cuda.current_stream().cuda_stream

        def call(k):
            rc = libs[k].mcd_vit_attention_long(qkv.data_ptr(), B, T, H, out[k].data_ptr(), stream)
            assert rc == 0, (k, rc)
        n = iters if T < 2048 else max(1, min(iters, 3))
        res = {k: [] for k in libs}
        for _ in range(rounds):
            for k in ("tree", "other"):
                res[k].append(timeit(lambda: call(k), n, warm=2))
        med = {k: statistics.median(v) for k, v in res.items()}
        flop = 4.0 * B * H * T * T * 64
        print(json.dumps({"tool": "scripts/vit_family_timing.py --k9l", "B": B, "H": H, "T": T, "rounds": rounds, "iters": n,
                          "same_bits": bool(torch.equal(out["tree"], out["other"])),
                          "tree_ms": [round(v, 4) for v in res["tree"]], "other_ms": [round(v, 4) for v in res["other"]],
                          "tree_median_ms": round(med["tree"], 4), "other_median_ms": round(med["other"], 4),
                          "other_over_tree": round(med["other"] / med["tree"], 4),
                          "tree_spread": round(spread(res["tree"]), 4), "other_spread": round(spread(res["other"]), 4),
                          "tree_tflops": round(flop / med["tree"] / 1e9, 1)}), flush=True)
        del qkv, out


def tower_child(B, rounds, iters):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    import mammo_clip_dissect_amd  # noqa: F401
    from mammo_clip_dissect_amd import core
    from mammo_clip_dissect_amd.concept_vit import data_utils as du
    dev = torch.device("cuda:0")
    net = du.get_target_model("dino", dev)[0]
    with torch.no_grad():                      # the factory's LayerScale is the constant 1: a fold that did nothing would not show
        for blk in net.dinov2.encoder.layer:
            blk.layer_scale1.lambda1.uniform_(0.5, 1.5)
            blk.layer_scale2.lambda1.uniform_(0.5, 1.5)
    x = torch.randn(B, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    flags = ("HIP_ATTENTION", "FUSED_RESIDUAL", "HIP_LAYER_NORM")

    def route(hip):
        for f in flags:
            setattr(du, f, hip)

    res = {"hip": [], "aten": []}
    with torch.no_grad():
        for r in ("hip", "aten"):                                   # warm-up: library plans and picks, MIOpen's search, folds
            route(r == "hip")
            for _ in range(3):
                y = net(x)
            res[r + "_out"] = y
        torch.cuda.synchronize()
        diff = float((res.pop("hip_out") - res.pop("aten_out")).abs().max())
        for _ in range(rounds):
            for r in ("hip", "aten"):
                route(r == "hip")
                res[r].append(timeit(lambda: net(x), iters, warm=1))
        # the HIP route by kernel: events around every wrapper call of one forward
        route(True)
        marks = []

        def timed(name, fn):
            def wrap(*a, **kw):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = fn(*a, **kw)
                e.record()
                marks.append((name, s, e))
                return r
            return wrap
        real = {n: getattr(core, n) for n in ("patchify", "layer_norm", "vit_attention_long", "vit_attention", "linear_residual")}
        names = {"patchify": "K11 patchify", "layer_norm": "K10 layer norm", "vit_attention_long": "K9L attention",
                 "vit_attention": "K9 attention", "linear_residual": "hipBLASLt GEMMs"}
        gelu = F.gelu
        try:
            for n, fn in real.items():
                setattr(core, n, timed(names[n], fn))
            F.gelu = timed("GELU (ATen)", gelu)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            net(x)
            e.record()
            torch.cuda.synchronize()
        finally:
            for n, fn in real.items():
                setattr(core, n, fn)
            F.gelu = gelu
        total = s.elapsed_time(e)
        by = {}
        for n, a, b in marks:
            ms, k = by.get(n, (0.0, 0))
            by[n] = (ms + a.elapsed_time(b), k + 1)
        by["rest (mean, cat, gaps)"] = (total - sum(v[0] for v in by.values()), 0)
    med = {r: statistics.median(v) for r, v in res.items()}
    print(json.dumps({"tool": "scripts/vit_family_timing.py --tower", "target": "dino", "batch": B, "tokens": 257,
                      "rounds": rounds, "iters": iters, "max_abs_diff_hip_aten": diff,
                      "hip_ms": [round(v, 3) for v in res["hip"]], "aten_ms": [round(v, 3) for v in res["aten"]],
                      "hip_median_ms": round(med["hip"], 3), "aten_median_ms": round(med["aten"], 3),
                      "aten_over_hip": round(med["aten"] / med["hip"], 3),
                      "hip_spread": round(spread(res["hip"]), 4), "aten_spread": round(spread(res["aten"]), 4),
                      "images_per_s_hip": round(B / med["hip"] * 1e3, 1), "images_per_s_aten": round(B / med["aten"] * 1e3, 1),
                      "hip_forward_with_events_ms": round(total, 3),
                      "hip_by_kernel": {n: {"ms": round(v[0], 3), "calls": v[1], "share": round(v[0] / total, 4)}
                                        for n, v in by.items()}}), flush=True)


if __name__ == "__main__":
    if "--child-k9l" in sys.argv:
        k9l_child(sys.argv[2], int(opt("--batch", "250")), int(opt("--rounds", "7")), int(opt("--iters", "10")))
    elif "--child-tower" in sys.argv:
        tower_child(int(sys.argv[2]), int(opt("--rounds", "5")), int(opt("--iters", "5")))
    elif "--k9l" in sys.argv:
        other = opt("--other-lib", None)
        if other is None or not os.path.isfile(other):
            sys.exit("--k9l needs --other-lib PATH, the libmcd_hip.so to compare this tree's with")
        child(["--child-k9l", os.path.abspath(other), "--batch", opt("--batch", "250"), "--rounds", opt("--rounds", "7"),
               "--iters", opt("--iters", "10")], 900)
    elif "--tower" in sys.argv:
        child(["--child-tower", str(arg_n("--tower", 250)), "--rounds", opt("--rounds", "5"), "--iters", opt("--iters", "5")], 600)
    else:
        print(__doc__)
