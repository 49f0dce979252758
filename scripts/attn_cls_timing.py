"""K9C (mcd_vit_attention_cls) alone at the headline batch (2 500 images x 12 heads x 197 tokens, fp32) and at one
high-resolution length: time, and the achieved rate over its algorithmic bytes (every K and V head row once,
2 * B * T * H * 256) as a fraction of the 8 TB/s HBM peak.  K9 on the same batch for comparison.  Dev tool.
    MCD_ATTN_B=<images>   batch of the headline shape (default 2500)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mammo_clip_dissect_amd as m
from mammo_clip_dissect_amd import core

dev = torch.device("cuda:0")
H = 12


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n


for B, T in ((int(os.environ.get("MCD_ATTN_B", "2500")), 197), (16, 5416)):
    kv = torch.randn(B, T, 2, H, 64, device=dev)        # the pruned block's K|V projection
    q = torch.randn(B, H * 64, device=dev)
    nbytes = 2.0 * B * T * H * 256
    ms = timeit(lambda: core.vit_attention_cls(q, kv[:, :, 0], kv[:, :, 1]))
    print("K9C B=%d T=%d split K|V    %8.3f ms  %6.2f TB/s  %.2f of 8 TB/s  (%.2f GB)"
          % (B, T, ms, nbytes / ms / 1e9, nbytes / ms / 1e9 / 8.0, nbytes / 1e9), flush=True)
    del kv
    qkv = torch.randn(B, T, 3, H, 64, device=dev)       # a plain qkv through strides
    ms = timeit(lambda: core.vit_attention_cls(qkv[:, 0, 0], qkv[:, :, 1], qkv[:, :, 2]))
    print("K9C B=%d T=%d strided qkv  %8.3f ms  %6.2f TB/s  %.2f of 8 TB/s"
          % (B, T, ms, nbytes / ms / 1e9, nbytes / ms / 1e9 / 8.0), flush=True)
    if T <= core.VIT_ATTENTION_MAX_T:
        ms9 = timeit(lambda: core.vit_attention(qkv.view(B, T, 3 * H * 64), H), n=5)
        print("K9  B=%d T=%d all rows     %8.3f ms  (K9C: %.1fx less)" % (B, T, ms9, ms9 / ms), flush=True)
    del qkv
