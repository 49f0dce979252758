"""The text pass of a dissection -- the package's 763 concepts through the BERT text tower at BERT-base size (hidden 768,
12 layers, 12 heads, intermediate 3072) -- on the ATen route and on the HIP route (K24, K9M, the fused GEMMs, K10):

    tokenise (host, timed apart) -> per chunk of --batch concepts: encode_text ('eos' pooling) + text_projection -> cat

which is what utils.extract_and_save runs once per dissection.  The weights are seeded random numbers (a time does not
depend on them); the vocabulary is the test fixture's tests/golden/text_vocab.txt, the only one in the tree: it has every
letter as a piece, so a word it lacks becomes one token per letter and the sequences are LONGER than Bio_ClinicalBERT's
would be (the padded length and the mean length are printed).  A real vocabulary: --vocab /path/vocab.txt.

Device events around `reps` back-to-back passes, both routes warmed (plans picked, code objects loaded), at least 0.5 s of
passes per figure; the routes alternate over three rounds and every round is printed.  The two outputs are compared
first.  --step-ms: the time of one bench.py step (10 000 images / its images/s), for the share the text pass amounts to.

    python scripts/text_timing.py [--batch 250] [--vocab FILE] [--step-ms MS] [--out profiles/NAME.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--vocab", default=os.path.join(ROOT, "tests", "golden", "text_vocab.txt"))
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "text_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    words = utils._read_concepts(CONCEPTS)
    data_utils.register_tokenizer("bert", args.vocab)
    tok = data_utils.bert_tokenizer()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        model = data_utils.BreastClip("vit", image_size=32, text_tower="bert",
                                      bert_config=dict(vocab=tok.vocab_size)).to(dev).eval()
    t0 = time.perf_counter()
    tokens = model.tokenize(words)
    t_tok = time.perf_counter() - t0
    lens = tokens["attention_mask"].sum(1)
    say("%d concepts, vocabulary of %d entries: padded to %d tokens, mean length %.1f; tokenising on the host %.1f ms"
        % (len(words), tok.vocab_size, tokens["input_ids"].shape[1], float(lens.float().mean()), t_tok * 1e3))
    tokens = {k: v.to(dev) for k, v in tokens.items()}

    def text_pass():
        with torch.no_grad():
            return torch.cat([model.text_projection(model.encode_text({k: v[i:i + args.batch] for k, v in tokens.items()}))
                              for i in range(0, len(words), args.batch)])

    def route(hip):
        data_utils.HIP_TEXT = hip
        return text_pass

    a, h = route(False)(), route(True)()
    err = float((a.double() - h.double()).abs().max() / a.double().abs().max())
    say("HIP route against the ATen route: max |diff| / max |ATen| = %.2e" % err)
    assert err < 1e-4, "the two routes disagree"
    aten, hip = [], []
    for _ in range(3):                                           # alternated: ATen, HIP, ATen, ...
        aten.append(timed(route(False)))
        hip.append(timed(route(True)))
    ta, th = min(aten), min(hip)
    say("text pass, BERT-base size, chunks of %d:" % args.batch)
    say("  ATen route %8.3f ms (rounds: %s)" % (ta * 1e3, ", ".join("%.3f" % (t * 1e3) for t in aten)))
    say("  HIP route  %8.3f ms (rounds: %s)   HIP / ATen = %.3f" % (th * 1e3, ", ".join("%.3f" % (t * 1e3) for t in hip), th / ta))
    if args.step_ms:
        say("  a bench.py step of %.1f ms: the text pass is %.2f %% of it on the ATen route, %.2f %% on the HIP route"
            % (args.step_ms, 100 * ta * 1e3 / args.step_ms, 100 * th * 1e3 / args.step_ms))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
