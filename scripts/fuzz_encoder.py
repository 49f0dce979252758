"""Randomised differential test with the three fuzzers under tests/ (the scoring side: scoring_fuzz.py -- K1A, K1, K2, K4, K5, K7, K7G,
K8 by dispatch class, against the oracle's bits or the entry's numeric rule); the encoder-side entries: encoder_fuzz.py -- the attention
family (K9, K9L, K9M, K9A, K9B), the one-row entries (K9C, K30) and the token / row operations (K10, K24, K25, K26, K27, K28,
K29) -- and conv_fuzz.py -- the channels-last towers (K12 - K15, K0N, K16 - K18, K18R, K19 - K21) and the Swin pair (K31, K32):
stratified case lists of consecutive seeds, float64 references from the headers, the headers' bit relations and read sets, every
operand in a frame.
argv: [cases per entry] [seed] [--entries K9 K9M K18 K31 K4 K5 ...]"""
import argparse
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import mammo_clip_dissect_amd as mcd
import conv_fuzz as C
import encoder_fuzz as E
import scoring_fuzz as S

ap = argparse.ArgumentParser()
ap.add_argument("cases", nargs="?", type=int, default=600)
ap.add_argument("seed", nargs="?", type=int, default=0)
ap.add_argument("--entries", nargs="+", default=list(E.ENTRIES + C.ENTRIES + S.ENTRIES),
                choices=E.ENTRIES + C.ENTRIES + S.ENTRIES)
args = ap.parse_args()
dev = torch.device("cuda:0")
calls = {E: E.gpu_call(mcd._lib.load()), C: C.gpu_call(mcd._lib.load()), S: S.gpu_call(mcd._lib.load())}
bad, top, done = 0, {}, 0
for entry in args.entries:
    top[entry] = 0.0
    F = E if entry in E.ENTRIES else (C if entry in C.ENTRIES else S)
    for case in F.random_cases(entry, args.cases, args.seed):
        findings, ratio = F.check(entry, case, calls[F], dev)
        for f in findings:
            print("MISMATCH " + f, flush=True)
        bad += len(findings)
        top[entry] = max(top[entry], ratio)
        done += 1
        if done % 50 == 0:
            print("%d cases, %d mismatches; max err / bound: %s" % (done, bad, " ".join("%s %.3f" % kv for kv in top.items())), flush=True)
print("done: %d cases, %d mismatches; max err / bound: %s" % (done, bad, " ".join("%s %.3f" % kv for kv in top.items())))
sys.exit(1 if bad else 0)
