"""The folded class-token tail (CLS_FOLD) on one MI355X, fp32:
  * K30 (mcd_cls_token_mix) alone at the headline batch (2 500 images x 197 tokens x 768, 12 heads): ms and GB/s on its
    B*T*D*4 bytes, mean of 10 launches after 2 warm-ups, HIP events;
  * the two groups of 12 small GEMMs around it (u: M = B, N = 768, K = 64; o: M = B, N = 64, K = 768);
  * the whole class-token tail block (_block_hip(cls_only=True)), with the K|V GEMM + K9C and folded, at the headline batch
    and at smaller ones: where the fold starts to pay (data_utils.CLS_FOLD_MIN_ROWS).
Writes profiles/cls_fold_timing.txt.  Dev tool.
    MCD_FOLD_B=<images>   batch of the headline shape (default 2500)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import mammo_clip_dissect_amd as m
from mammo_clip_dissect_amd import core
from mammo_clip_dissect_amd.concept_vit import data_utils as du

dev = torch.device("cuda:0")
H, D, T = 12, 768, 197
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timeit(fn, n=10, warm=2):
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


def tail(blk, x, fold):
    du.CLS_FOLD = fold
    du.CLS_FOLD_MIN_ROWS = 0
    with torch.no_grad():
        return blk(x, cls_only=True)


B0 = int(os.environ.get("MCD_FOLD_B", "2500"))
torch.manual_seed(0)
blk = du._Block(D, H, 4 * D).to(dev).eval()
say("folded class-token tail, fp32, %s" % torch.cuda.get_device_name(0))

n = torch.randn(B0, T, D, device=dev)
u = torch.randn(B0, H, D, device=dev) * 0.05
nbytes = B0 * T * D * 4.0
ms = timeit(lambda: core.cls_token_mix(u, n))
say("K30 B=%d T=%d H=%d D=%d            %8.3f ms  %7.1f GB/s on B*T*D*4 = %.2f GB" % (B0, T, H, D, ms, nbytes / ms / 1e6, nbytes / 1e9))
q = torch.randn(B0, D, device=dev)
wkt = torch.randn(H, D, 64, device=dev) * 0.05
wv = torch.randn(D, D, device=dev) * 0.05
bv = torch.randn(D, device=dev)
mm = torch.randn(B0, H, D, device=dev)
o = torch.empty(B0, D, device=dev)


def group_u():
    for h in range(H):
        core.linear_residual(None, q[:, 64 * h:64 * h + 64], wkt[h], None, out=u[:, h])


def group_o():
    for h in range(H):
        core.linear_residual(None, mm[:, h], wv[64 * h:64 * h + 64], bv[64 * h:64 * h + 64], out=o[:, 64 * h:64 * h + 64])


say("u GEMMs, %d x (M=%d N=%d K=64)          %8.3f ms" % (H, B0, D, timeit(group_u)))
say("o GEMMs, %d x (M=%d N=64 K=%d)          %8.3f ms" % (H, B0, D, timeit(group_o)))
del n, u, q, mm, o

for B in (B0, 256, 128, 64, 32, 8):
    x = torch.randn(B, T, D, device=dev)
    old = timeit(lambda: tail(blk, x, False))
    new = timeit(lambda: tail(blk, x, True))
    d = (tail(blk, x, True) - tail(blk, x, False)).abs().max().item()
    say("tail block B=%5d (%7d rows): K|V GEMM + K9C %8.3f ms   folded %8.3f ms   (%+.3f ms)   max |d| %.2e"
        % (B, B * T, old, new, new - old, d))
    del x

out = os.path.join(ROOT, "profiles", "cls_fold_timing.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
