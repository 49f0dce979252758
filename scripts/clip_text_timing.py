"""OpenAI CLIP's dissector on the ATen route and on the HIP route (data_utils.OpenAIClip, HIP_CLIP_TEXT), kernel by kernel
and end to end:

  * K9A (mcd_vit_attention_causal) at B = 763 concepts, T = 77 tokens, H = 8 heads against SDPA with is_causal=True on the
    layout the ATen route gives it, and against K9M with full lengths (the same kernel body without the causal early exit:
    what skipping the tiles above the diagonal buys);
  * K25 (mcd_quick_gelu, in place) against the three ATen launches x * sigmoid(1.702 * x) at [250 * 197, 3072] (the image
    tower's c_fc output for a batch of 250) and [763 * 77, 2048] (the text tower's), with the algorithmic GB/s of each;
  * the ViT-B/16-shaped OpenAIClip: encode_image on a batch of 250 and encode_text on the 763 concepts in one chunk.

The weights are seeded random numbers (a time does not depend on them).  The tokens come from the test fixture's small
merges file, tests/golden/clip_bpe_small.txt.gz, unless --bpe names a full one; the text tower computes all 77 positions
whatever the ids, so the choice does not move a time.  Device events around `reps` back-to-back calls, both sides warmed, at
least 0.5 s of calls per figure; the two sides alternate over --rounds rounds, every round is printed, and the spread of a
side is (max - min) / min over its rounds.  The outputs of the two sides are compared first.

    python scripts/clip_text_timing.py [--rounds 3] [--bpe FILE] [--out profiles/NAME.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mammo_clip_dissect_amd import core                                # noqa: E402
from mammo_clip_dissect_amd.concept_vit import data_utils, utils      # noqa: E402

CONCEPTS = os.path.join(ROOT, "mammo-clip-dissect_amd", "Concepts", "Specific_concepts_sorted.txt")


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bpe", default=os.path.join(ROOT, "tests", "golden", "clip_bpe_small.txt.gz"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clip_text_timing.py measures on the GPU"
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
        base = min(times[sides[0][0]])
        for name, _ in sides:
            t = times[name]
            extra = "" if unit_bytes is None else "  %6.0f GB/s" % (unit_bytes / min(t) / 1e9)
            say("  %-28s %9.4f ms (rounds: %s; spread %.1f %%)  / %s = %.3f%s"
                % (name, min(t) * 1e3, ", ".join("%.4f" % (x * 1e3) for x in t), 100 * (max(t) - min(t)) / min(t), sides[0][0],
                   min(t) / base, extra))

    def close(a, b, what, tol=1e-4):
        err = float((a.double() - b.double()).abs().max() / a.double().abs().max())
        say("%s: max |diff| / max |ATen| = %.2e" % (what, err))
        assert err < tol, what

    g = torch.Generator().manual_seed(0)
    # ---- K9A
    B, T, H = 763, 77, 8
    qkv = torch.randn(B, T, 3 * H * 64, generator=g).to(dev)

    def sdpa():
        q, k, v = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        return F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, H * 64)
    out = torch.empty(B, T, H * 64, device=dev)
    close(sdpa(), core.vit_attention_causal(qkv, H), "K9A against SDPA is_causal")
    compare("causal attention, B = %d, T = %d, H = %d:" % (B, T, H),
            [("SDPA is_causal", sdpa), ("K9A", lambda: core.vit_attention_causal(qkv, H, out=out)),
             ("K9M, full lengths (no mask)", lambda: core.vit_attention_keylen(qkv, H, None, out=out))])
    del qkv, out
    # ---- K25
    for rows, width in ((250 * 197, 3072), (763 * 77, 2048)):
        x = (3 * torch.randn(rows, width, generator=g)).to(dev)
        y = torch.empty_like(x)
        close(x * torch.sigmoid(1.702 * x), core.quick_gelu(x), "K25 against the ATen form at [%d, %d]" % (rows, width))
        compare("QuickGELU at [%d, %d] (%.0f MB read, %.0f MB written per pass):" % (rows, width, x.numel() * 4 / 1e6, x.numel() * 4 / 1e6),
                [("ATen mul, sigmoid, mul", lambda: x * torch.sigmoid(1.702 * x)), ("K25", lambda: core.quick_gelu(x, out=y))],
                unit_bytes=2 * x.numel() * 4)
        del x, y
    # ---- the towers
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        model = data_utils.OpenAIClip(**data_utils.VIT_B16).to(dev).eval()
    words = utils._read_concepts(CONCEPTS)
    tok = data_utils.ClipBPETokenizer(args.bpe)
    ids = tok(words, context_length=77).to(dev)
    say("%d concepts, merges file of %d entries: longest sequence %d tokens of 77 (start and end ids included)"
        % (len(words), tok.vocab_size, int(ids.argmax(1).max()) + 1))
    images = torch.randn(250, 3, 224, 224, generator=g).to(dev)

    def tower(fn, arg, hip):
        def run():
            data_utils.HIP_CLIP_TEXT = hip
            with torch.no_grad():
                return fn(arg)
        return run
    for what, fn, arg in (("encode_text, %d concepts" % len(words), model.encode_text, ids),
                          ("encode_image, 250 images of 224 x 224", model.encode_image, images)):
        close(tower(fn, arg, False)(), tower(fn, arg, True)(), "%s: HIP route against the ATen route" % what)
        compare("ViT-B/16-shaped OpenAIClip, %s:" % what, [("ATen route", tower(fn, arg, False)), ("HIP route", tower(fn, arg, True))])
    data_utils.HIP_CLIP_TEXT = True
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
