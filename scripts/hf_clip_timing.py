"""The HF `clip` target (data_utils.HFClip, transformers' CLIPForImageClassification) on the ATen route and on the HIP route
(HIP_HF_CLIP), and K26 (mcd_token_mean) alone:

  * K26 at (B, T, D, t0) = (250, 197, 768, 1) -- the mean of ViT-B/16's patch tokens for a batch of 250 -- against ATen's
    x[:, 1:].mean(dim=1) on the same tensors, with the bytes the reduction needs (B * (T - t0) * D floats read, B * D written)
    over the time as GB/s and as a share of the HBM peak (8.0 TB/s by the data sheet; a float4 copy reaches 6.3).  The
    151 MB input fits the 256 MB last-level cache, so each side walks a ring of --ring distinct inputs (4: 605 MB);
    --ring 1 gives the cache-resident figure;
  * the ViT-B/16-sized HFClip (seeded weights: a time does not depend on them) on a batch of 250 images of 224 x 224:
    forwards of the two routes alternated in one process.

Device events around `reps` back-to-back calls, both sides warmed, at least 0.5 s of calls per figure; the two sides
alternate over --rounds rounds, every round is printed; a side's figure is the median of its rounds and its spread is
(max - min) / min over them.  The outputs of the two sides are compared first.

    python scripts/hf_clip_timing.py [--rounds 5] [--ring 4] [--out profiles/NAME.txt]
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

HBM_PEAK = 8.0e12      # bytes / s, MI355X data sheet


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
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hf_clip_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def compare(what, sides, unit_bytes=None):
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
            extra = "" if unit_bytes is None else "  %6.0f GB/s = %.1f %% of the %.1f TB/s HBM peak" % (
                unit_bytes / med / 1e9, 100 * unit_bytes / med / HBM_PEAK, HBM_PEAK / 1e12)
            say("  %-28s median %9.4f ms (rounds: %s; spread %.1f %%)  / %s = %.3f%s"
                % (name, med * 1e3, ", ".join("%.4f" % (x * 1e3) for x in t), 100 * (max(t) - min(t)) / min(t), sides[0][0],
                   med / base, extra))

    def close(a, b, what, tol=1e-4):
        err = float((a.double() - b.double()).abs().max() / a.double().abs().max())
        say("%s: max |diff| / max |ATen| = %.2e" % (what, err))
        assert err < tol, what

    g = torch.Generator().manual_seed(0)
    # ---- K26
    B, T, D, t0 = args.batch, 197, 768, 1
    ring = [torch.randn(B, T, D, generator=g).to(dev) for _ in range(args.ring)]
    out = torch.empty(B, D, device=dev)
    for x in ring[:1]:
        close(x[:, t0:].mean(dim=1), core.token_mean(x, t0), "K26 against ATen's mean at (%d, %d, %d, t0 = %d)" % (B, T, D, t0))
    turn = {"aten": 0, "k26": 0}

    def aten_mean():
        turn["aten"] = (turn["aten"] + 1) % len(ring)
        return ring[turn["aten"]][:, t0:].mean(dim=1)

    def k26():
        turn["k26"] = (turn["k26"] + 1) % len(ring)
        return core.token_mean(ring[turn["k26"]], t0, out=out)
    need = (B * (T - t0) * D + B * D) * 4
    compare("mean of the patch tokens at (%d, %d, %d, t0 = %d), a ring of %d inputs (%.0f MB read, %.2f MB written per call):"
            % (B, T, D, t0, len(ring), B * (T - t0) * D * 4 / 1e6, B * D * 4 / 1e6),
            [("ATen x[:, 1:].mean(dim=1)", aten_mean), ("K26", k26)], unit_bytes=need)
    del ring, out
    # ---- the model
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        model = data_utils.HFClip().to(dev).eval()
    images = torch.randn(B, 3, 224, 224, generator=g).to(dev)

    def forward(hip):
        def run():
            data_utils.HIP_HF_CLIP = hip
            with torch.no_grad():
                assert model.route(images) == ("hip" if hip else "aten")
                return model(images)
        return run
    close(forward(False)(), forward(True)(), "HFClip logits: HIP route against the ATen route")
    compare("ViT-B/16-sized HFClip, %d images of 224 x 224, one forward:" % B, [("ATen route", forward(False)), ("HIP route", forward(True))])
    data_utils.HIP_HF_CLIP = True
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
