"""K22 (mcd_image_preprocess) against the host route (PIL + torch on 16 threads), on the two workload shapes:

    256 images of 375 x 500  ->  the `imagenet` and the `clip` view (one upload, two launches)
     16 images of 2294 x 1914 ->  the `embed` view

K22 alone: device events around `reps` back-to-back launches on resident uint8 images, warmed, at least 0.5 s of work per
figure; bytes/s are the algorithmic bytes (3 n H W read + 12 n OH OW written per view) over that time, against the
8 TB/s HBM peak.  The host route runs on the same arrays, alternated with K22, and is a wall-clock figure.  With --files
the script also writes the 256 images as PNG files and reports images/s of ImageFileProbe.device_batches from files:
that figure is bounded by the CPU decode and is an end-to-end number, not a kernel's.

    python scripts/preprocess_timing.py [--files DIR] [--out profiles/NAME.txt]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mammo_clip_dissect_amd import core                                   # noqa: E402
from mammo_clip_dissect_amd.concept_vit import data_utils                 # noqa: E402

HBM_PEAK = 8.0e12
WORKLOADS = [("imagenet+clip 256 x (375 x 500)", 256, 375, 500, ("imagenet", "clip")),
             ("embed 16 x (2294 x 1914)", 16, 2294, 1914, ("embed",))]


def algorithmic_bytes(n, H, W, views):
    plans = [core.get_preprocess(v).plan(H, W) for v in views]
    return sum(3 * n * H * W + 12 * n * p.OH * p.OW for p in plans)


def time_k22(src, views, outs, min_seconds=0.5):
    def launch():
        for v, o in zip(views, outs):
            core.image_preprocess(src, v, out=o)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    reps, total = 4, 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1) / 1e3
        if total >= min_seconds:
            return total / reps
        reps *= 4


def time_host(arrays, views, pool):
    t0 = time.perf_counter()
    for v in views:
        pre = core.get_preprocess(v)
        list(pool.map(lambda a: data_utils.host_preprocess(a, pre), arrays))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default=None, help="directory to write the 256 PNG files to (end-to-end figure)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "preprocess_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
    torch.set_num_threads(1)          # the host route's parallelism is the pool's: one torch thread per worker
    for name, n, H, W, views in WORKLOADS:
        rs = np.random.RandomState(7)
        arrays = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]
        src = torch.from_numpy(np.stack(arrays)).to(dev)
        plans = [core.get_preprocess(v).plan(H, W) for v in views]
        outs = [torch.empty((n, 3, p.OH, p.OW), dtype=torch.float32, device=dev) for p in plans]
        nbytes = algorithmic_bytes(n, H, W, views)
        k22, host = [], []
        for _ in range(3):                                   # alternated: K22, host, K22, host, ...
            k22.append(time_k22(src, views, outs))
            host.append(time_host(arrays, views, pool))
        want = torch.stack([data_utils.host_preprocess(arrays[0], core.get_preprocess(views[0]))])
        assert torch.equal(outs[0][:1].cpu(), want), "K22 and the host route disagree"
        tk, th = min(k22), min(host)
        say("%s: taps %s" % (name, [p.taps for p in plans]))
        say("  K22        %9.3f ms per call (runs: %s)  %7.1f GB/s algorithmic = %.1f %% of the 8 TB/s HBM peak"
            % (tk * 1e3, ", ".join("%.3f" % (t * 1e3) for t in k22), nbytes / tk / 1e9, 100 * nbytes / tk / HBM_PEAK))
        say("  host route %9.1f ms per call (runs: %s), PIL + torch on %d threads: %.0f x K22"
            % (th * 1e3, ", ".join("%.1f" % (t * 1e3) for t in host), pool._max_workers, th / tk))
        if args.files and n == 256:
            from PIL import Image
            for i, a in enumerate(arrays):
                d = os.path.join(args.files, "class_%d" % (i % 8))
                os.makedirs(d, exist_ok=True)
                Image.fromarray(a, "RGB").save(os.path.join(d, "img_%03d.png" % i))
            ds = data_utils.ImageFileProbe(data_utils.list_folder(args.files), "imagenet", "clip", device=dev)
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for batch in ds.device_batches(64):
                    pass
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            say("  end to end from PNG files (CPU decode on %d threads + upload + K22, two views): %.0f images/s"
                % (pool._max_workers, n / dt))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
