"""Timing of rank_reorder / cos_similarity / cos_similarity_cubed at 10 000 images x 12 x 768 neurons x 763 concepts, one GPU:
  fused     Dissector.finish over all 12 layers, with HIP events at its stage marks
  per_layer the drop-in similarity.<fn> called once per layer on the same resident tensors (P, image-major activations),
            plus the K6 / K3 selections the per-layer driver route runs
  reload    what the per-layer driver route adds on top: torch.load of every layer's [N, 768] cache file, to the device
Prints one JSON line per function (milliseconds, medians over --reps runs after one warm-up).  Dev tool, not the bench."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mammo_clip_dissect_amd  # noqa: E402,F401
from mammo_clip_dissect_amd import core, pipeline  # noqa: E402
from mammo_clip_dissect_amd.concept_vit import similarity  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=10000)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--width", type=int, default=768)
ap.add_argument("--concepts", type=int, default=763)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--fns", default="rank_reorder,cos_similarity,cos_similarity_cubed")
args = ap.parse_args()

dev = torch.device("cuda:0")
N, C, D, L, W = args.images, args.concepts, 512, args.layers, args.width
g = torch.Generator(device=dev).manual_seed(0)
E_img = torch.randn(N, D, device=dev, generator=g)
E_txt = torch.randn(C, D, device=dev, generator=g)
dis = pipeline.Dissector(N, ["l%d" % i for i in range(L)], [W] * L, C, D, dev)
dis.At[:, :N] = torch.randn(L * W, N, device=dev, generator=g)
dis.E_img.copy_(E_img)
dis.cursor = N
A_layers = [dis.At[i * W:(i + 1) * W, :N].t().contiguous() for i in range(L)]   # what the cache files hold, resident


class Marks:
    def __init__(self):
        self.ev = []

    def __call__(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append((name, e))

    def stages(self):
        torch.cuda.synchronize()
        out, prev = {}, self.ev[0][1]
        for name, e in self.ev[1:]:
            if ":" in name:
                continue
            out[name] = out.get(name, 0.0) + prev.elapsed_time(e)
            prev = e
        return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def per_layer(fn):
    P = core.embed_gemm(core.normalize_rows(E_img), core.normalize_rows(E_txt))
    for A in A_layers:
        sim = getattr(similarity, fn)(P, A, device=str(dev))
        core.row_topk(sim, 10)
        core.col_topk(A, 5, want_vals=False)


tmp = tempfile.mkdtemp()
files = []
for i, A in enumerate(A_layers):
    files.append(os.path.join(tmp, "layer%d.pt" % i))
    torch.save(A.cpu(), files[-1])


def reload():
    for f in files:
        torch.load(f, map_location="cpu", weights_only=True).to(dev)


for fn in args.fns.split(","):
    dis.set_scoring(fn)
    fused, stage_runs, layered = [], [], []
    for r in range(args.reps + 1):
        m = Marks()
        torch.manual_seed(0)
        ms = wall(lambda: dis.finish(E_txt, marks=m))
        if r:
            fused.append(ms)
            stage_runs.append(m.stages())
    for r in range(args.reps + 1):
        torch.manual_seed(0)
        ms = wall(lambda: per_layer(fn))
        if r:
            layered.append(ms)
    stages = {k: round(statistics.median(s[k] for s in stage_runs), 3) for k in stage_runs[0]}
    reload_ms = statistics.median(wall(reload) for _ in range(args.reps))
    print(json.dumps({"fn": fn, "shape": [N, L * W, C], "fused_ms": round(statistics.median(fused), 3), "fused_stage_ms": stages,
                      "per_layer_ms": round(statistics.median(layered), 3), "per_layer_reload_ms": round(reload_ms, 3)}),
          flush=True)
for f in files:
    os.remove(f)
os.rmdir(tmp)
