"""K9L (mcd_vit_attention_long) against PyTorch's fp32 SDPA at the high-resolution tower's lengths (B = 8 images x 12
heads, T = 1 025 / 4 097 / 5 416: 512 x 512, 1024 x 1024 and Mammo-CLIP's 1520 x 912 at patch 16).  Dev tool.

For each T: the kernel's time, TFLOP/s (4 T^2 64 per head) and the fraction of the 157.3 TFLOP/s fp32 MFMA peak; the
same for SDPA's default pick in this process, which backend that is (the explicit backend that returns the same bits),
and the peak memory each one allocates beyond its inputs (torch.cuda.max_memory_allocated).
  --tower [N]   only N (default 4) forwards of a 1024 x 1024 ViT-B/16 tower on 8 images, for a rocprofv3 --kernel-trace
                --stats pass (the attention's share of the tower's GPU time)
  --driver [N]  describe_broad_neurons.main at breastclip_vit_1024 on N (default 256) probe images, batch 32 (after a
                32-image warm-up run): the whole driver's images/s
"""
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import mammo_clip_dissect_amd as m
from mammo_clip_dissect_amd import core

dev = torch.device("cuda:0")
PEAK = 157.3
B, H = 8, 12


def timeit(fn, n=10):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    o = fn()
    torch.cuda.synchronize()
    del o
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def arg_n(flag, default):
    i = sys.argv.index(flag)
    return int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else default


if "--tower" in sys.argv:
    from mammo_clip_dissect_amd.concept_vit import data_utils
    tower = data_utils.ViTTower(image_size=1024).to(dev).eval()
    x = torch.randn(8, 3, 1024, 1024, device=dev)
    with torch.no_grad():
        for _ in range(arg_n("--tower", 4)):
            tower(x)
    torch.cuda.synchronize()
    print("tower forwards done")
    sys.exit(0)

if "--driver" in sys.argv:
    from mammo_clip_dissect_amd.concept_vit import describe_broad_neurons as drv
    concepts = os.path.join(os.path.dirname(m.__file__), "Concepts", "Specific_concepts_sorted.txt")
    layers = ",".join("image_encoder.encoder.layer[%d]" % i for i in range(12))
    for n in (32, arg_n("--driver", 256)):
        tmp = tempfile.mkdtemp()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            drv.main(["--target_model", "breastclip_vit_1024", "--target_layers", layers, "--d_probe",
                      "synthetic_%d_1024" % n, "--concept_set", concepts, "--batch_size", "32", "--device", "cuda:0",
                      "--activation_dir", tmp + "/acts", "--result_dir", tmp + "/results", "--top_k", "20"])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print("driver breastclip_vit_1024: %d images, batch 32, 12 layers: %.2f s  %.2f images/s" % (n, dt, n / dt),
              flush=True)
    sys.exit(0)

from torch.nn.attention import sdpa_kernel, SDPBackend
for T in (1025, 4097, 5416):
    g = torch.Generator(device=dev).manual_seed(T)
    qkv = torch.randn(B, T, 3 * H * 64, device=dev, generator=g)
    flops = 4.0 * B * H * T * T * 64
    q, k, v = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, H * 64)

    ms = timeit(lambda: core.vit_attention_long(qkv, H))
    mb = peak_mb(lambda: core.vit_attention_long(qkv, H))
    print("T=%5d  K9L mcd_vit_attention_long %8.3f ms  %6.1f TFLOP/s  %.3f of peak  peak mem %7.1f MB"
          % (T, ms, flops / ms / 1e9, flops / ms / 1e9 / PEAK, mb), flush=True)
    ref = sdpa()
    used = "unknown"
    for name, be in (("flash", SDPBackend.FLASH_ATTENTION), ("efficient", SDPBackend.EFFICIENT_ATTENTION),
                     ("math", SDPBackend.MATH)):
        try:
            with sdpa_kernel(be):
                if torch.equal(sdpa(), ref):
                    used = name
                    break
        except RuntimeError:
            continue
    ms_s = timeit(sdpa, n=3)
    mb_s = peak_mb(sdpa)
    print("T=%5d  torch SDPA (%s)%s %8.3f ms  %6.1f TFLOP/s  %.3f of peak  peak mem %7.1f MB"
          % (T, used, " " * max(0, 14 - len(used)), ms_s, flops / ms_s / 1e9, flops / ms_s / 1e9 / PEAK, mb_s), flush=True)
    print("T=%5d  max |K9L - SDPA| %.2e   SDPA / K9L time %.2f" % (T, (ref - core.vit_attention_long(qkv, H)).abs().max().item(),
                                                                    ms_s / ms), flush=True)
    del qkv, q, k, v, ref
    torch.cuda.empty_cache()
