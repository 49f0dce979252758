"""The `mae` target (data_utils.HFMae, transformers' ViTMAEForPreTraining) at ViT-MAE-base size on the ATen route and on the
HIP route (HIP_MAE), 250 images of 224 x 224, and its two new stages alone on the same tensors:

  * the embedding: the patch convolution over all 196 patches + position add + gather of the 49 kept rows + cat (ATen) against
    K28 + K29 (the position rows) + one GEMM with 50 rows an image;
  * the decoder's restore: repeat, cat, gather over an expanded index, cat, + decoder_pos_embed (ATen) against K29, at
    (B, L, Lk, D) = (250, 196, 49, 512);
  * the whole forward (seeded weights: a time does not depend on them), the two routes alternated in one process.

Device events around `reps` back-to-back calls, both sides warmed, at least 0.5 s of calls per figure; the two sides
alternate over --rounds rounds, every round is printed; a side's figure is the median of its rounds and its spread is
(max - min) / min over them.  The outputs of the two sides are compared first.

    python scripts/mae_timing.py [--rounds 5] [--out profiles/NAME.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mammo_clip_dissect_amd import core                          # noqa: E402
from mammo_clip_dissect_amd.concept_vit import data_utils       # noqa: E402


def timed(launch, min_seconds=0.5):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    reps = 2
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
        reps *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mae_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def compare(what, sides):
        """sides: [(name, launch)], alternated over the rounds; the first is the ATen side the others are held against."""
        times = {name: [] for name, _ in sides}
        for _ in range(args.rounds):
            for name, launch in sides:
                times[name].append(timed(launch))
        say(what)
        base = statistics.median(times[sides[0][0]])
        for name, _ in sides:
            t = times[name]
            med = statistics.median(t)
            say("  %-28s median %9.4f ms (rounds: %s; spread %.1f %%)  / %s = %.3f"
                % (name, med * 1e3, ", ".join("%.4f" % (x * 1e3) for x in t), 100 * (max(t) - min(t)) / min(t), sides[0][0],
                   med / base))

    def close(a, b, what, tol=1e-4):
        err = float((a.double() - b.double()).abs().max() / a.double().abs().max())
        say("%s: max |diff| / max |ATen| = %.2e" % (what, err))
        assert err < tol, what

    B = args.batch
    g = torch.Generator().manual_seed(0)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        model = data_utils.HFMae().eval()
        with torch.no_grad():                      # the tables and tokens a checkpoint would bring (zeros by construction)
            for p in (model.vit.embeddings.position_embeddings, model.vit.embeddings.cls_token, model.decoder.decoder_pos_embed,
                      model.decoder.mask_token):
                p.copy_(0.5 * torch.randn(p.shape))
        model = model.to(dev)
    images = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    noise = torch.rand(B, model.num_patches, generator=g).to(dev)
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    ids_keep = ids_shuffle[:, :int(model.num_patches * (1 - model.mask_ratio))]

    def embed(hip):
        def run():
            with torch.no_grad():
                return model.vit.embed(images, ids_keep, hip)
        return run
    close(embed(False)(), embed(True)(), "the embedding [%d, %d, 768]: K28 + K29 + GEMM against ATen" % (B, 1 + ids_keep.shape[1]))
    compare("the embedding of %d images, %d of %d patches kept:" % (B, ids_keep.shape[1], model.num_patches),
            [("ATen conv, add, gather, cat", embed(False)), ("K28 + K29 + one GEMM", embed(True))])

    d = model.decoder
    h = torch.randn(B, 1 + ids_keep.shape[1], d.decoder_embed.out_features, generator=g).to(dev)
    restore32 = ids_restore.to(torch.int32).contiguous()
    fill, add = d.mask_token.detach().view(-1), d.decoder_pos_embed.detach()[0]

    def aten_restore():
        L = ids_restore.shape[1]
        tokens = torch.cat([h[:, 1:], d.mask_token.detach().repeat(B, L + 1 - h.shape[1], 1)], dim=1)
        tokens = torch.gather(tokens, 1, ids_restore.unsqueeze(-1).repeat(1, 1, h.shape[2]))
        return torch.cat([h[:, :1], tokens], dim=1) + d.decoder_pos_embed.detach()

    def k29():
        return core.token_restore(h, restore32, fill, add)
    assert torch.equal(aten_restore(), k29())
    say("the decoder's restore at (B, L, Lk, D) = (%d, %d, %d, %d): K29 equals ATen's steps bit for bit"
        % (B, ids_restore.shape[1], ids_keep.shape[1], h.shape[2]))
    compare("the decoder's restore (%.1f MB written):" % (B * (1 + ids_restore.shape[1]) * h.shape[2] * 4 / 1e6),
            [("ATen repeat, cat, gather, +", aten_restore), ("K29", k29)])

    def forward(hip):
        def run():
            data_utils.HIP_MAE = hip
            with torch.no_grad():
                assert model.route(images) == ("hip" if hip else "aten")
                return model(images, noise).logits
        return run
    close(forward(False)(), forward(True)(), "HFMae logits: HIP route against the ATen route")
    compare("ViT-MAE-base-sized HFMae, %d images of 224 x 224, one forward:" % B,
            [("ATen route", forward(False)), ("HIP route", forward(True))])
    data_utils.HIP_MAE = True
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
