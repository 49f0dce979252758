"""K23 (mcd_image_minmax_normalize) at the mammogram workload, 16 images of 1520 x 912, from a grey and from an RGB source:

    K23        two launches (the partial min / max reduction, then the table look-up and the three fp32 planes)
    copy       Tensor.copy_ between two fp32 tensors of the output's size: the yardstick.  It reads and writes
               12 n H W bytes each, K23 reads channels n H W and writes 12 n H W
    host       data_utils.host_minmax (the reference's four numpy passes) on the same arrays, on 16 threads

Device events around `reps` back-to-back launches, warmed, at least 0.5 s of launches per figure; K23, the copy and the
host route alternate over three rounds and the spread of the rounds is printed.  Bytes/s are the algorithmic bytes
(channels n H W read + 12 n H W written) over the time, against the 8 TB/s HBM peak.  The grey source is timed on uniform
random bytes (every look-up of a wave on its own table entry: the worst case for LDS bank conflicts) and on a smooth
image (neighbouring pixels on the same few entries); if the two agree, the look-up is not what bounds the kernel.
With --files the script writes 32 of the grey images as PNG files in a vindr tree and reports images/s of
ImageFileProbe.device_batches from them: that figure is bounded by the CPU decode and is an end-to-end number.

    python scripts/minmax_timing.py [--files DIR] [--out profiles/NAME.txt]
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
N, H, W = 16, 1520, 912


def timed(launch, min_seconds=0.5):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    reps = 4
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


def smooth_images(rs):
    """A vertical ramp plus a little noise: what a wave looks up is a handful of neighbouring table entries."""
    ramp = np.linspace(8, 240, H)[:, None] + np.zeros((1, W))
    return [np.clip(ramp + rs.randint(-3, 4, (H, W)), 0, 255).astype(np.uint8) for _ in range(N)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default=None, help="directory to write 32 PNG files to (end-to-end figure)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "minmax_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    spec = core.PRESETS["vindr"]
    pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
    torch.set_num_threads(1)          # the host route's parallelism is the pool's
    rs = np.random.RandomState(7)
    sources = [("grey, random bytes", [rs.randint(0, 256, (H, W)).astype(np.uint8) for _ in range(N)]),
               ("grey, smooth image", smooth_images(rs)),
               ("RGB, random bytes", [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(N)])]
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    other = torch.randn((N, 3, H, W), dtype=torch.float32, device=dev)
    for name, arrays in sources:
        src = torch.from_numpy(np.stack(arrays)).to(dev)
        channels = 3 if src.dim() == 4 else 1
        nbytes = channels * N * H * W + 12 * N * H * W
        k23, cp, host = [], [], []
        for _ in range(3):                                   # alternated: K23, copy, host, K23, ...
            k23.append(timed(lambda: core.image_minmax_normalize(src, spec.mean, spec.std, out=out)))
            cp.append(timed(lambda: out.copy_(other)))
            t0 = time.perf_counter()
            list(pool.map(lambda a: data_utils.host_minmax(a, spec.mean, spec.std), arrays))
            host.append(time.perf_counter() - t0)
        core.image_minmax_normalize(src, spec.mean, spec.std, out=out)
        want = data_utils.host_minmax(arrays[N - 1], spec.mean, spec.std)
        assert torch.equal(out[N - 1].cpu().view(torch.int32), want.view(torch.int32)), "K23 and the host route disagree"
        tk, tc, th = min(k23), min(cp), min(host)
        say("%s, %d x (%d x %d):" % (name, N, H, W))
        say("  K23        %8.4f ms per call (rounds: %s)  %7.1f GB/s algorithmic = %.1f %% of the 8 TB/s HBM peak"
            % (tk * 1e3, ", ".join("%.4f" % (t * 1e3) for t in k23), nbytes / tk / 1e9, 100 * nbytes / tk / HBM_PEAK))
        say("  copy_      %8.4f ms per call (rounds: %s)  %7.1f GB/s (24 n H W bytes) = %.1f %% of the peak; K23 / copy_ = %.3f"
            % (tc * 1e3, ", ".join("%.4f" % (t * 1e3) for t in cp), 24 * N * H * W / tc / 1e9,
               100 * 24 * N * H * W / tc / HBM_PEAK, tk / tc))
        say("  host route %8.1f ms per call (rounds: %s), numpy on %d threads: %.0f x K23"
            % (th * 1e3, ", ".join("%.1f" % (t * 1e3) for t in host), pool._max_workers, th / tk))
    if args.files:
        from PIL import Image
        rows = ["patient_id,image_id,split,Mass"]
        for i in range(32):
            d = os.path.join(args.files, data_utils.VINDR_IMG_DIR, "%03d" % i)
            os.makedirs(d, exist_ok=True)
            Image.fromarray(sources[1][1][i % N], "L").save(os.path.join(d, "im%02d.png" % i), compress_level=1)
            rows.append("%03d,im%02d,test,0" % (i, i))
        os.makedirs(os.path.dirname(os.path.join(args.files, data_utils.VINDR_CSV)), exist_ok=True)
        with open(os.path.join(args.files, data_utils.VINDR_CSV), "w") as f:
            f.write("\n".join(rows) + "\n")
        ds = data_utils.ImageFileProbe(data_utils.list_vindr(args.files), "vindr", device=dev)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for batch in ds.device_batches(16):
                pass
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        say("end to end from 32 grey PNG files of %d x %d (CPU decode on %d threads + 1 byte / pixel upload + K23): %.0f images/s"
            % (H, W, pool._max_workers, 32 / dt))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
