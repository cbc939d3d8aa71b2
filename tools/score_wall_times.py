#!/usr/bin/env python
"""Wall times of the ways to a loss / token scores on one MI355X: VCoder-DS 7b, B = 8, the COST-shaped prompt of bench.py (S = 1216),
seeded synthetic weights.  Every figure: 2 warm-up calls, then `--reps` timed calls (host clock around the synchronous call),
median and min .. max.  usage: python tools/score_wall_times.py [--reps 7] [--out profiles/score_wall_times.md]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vcoder_amd import config as vcfg, synth  # noqa: E402
from vcoder_amd.engine import HipEngine  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, K, NC = 8, 8, 16
    cfg = vcfg.vicuna_7b("vcoder_ds")
    eng = HipEngine(cfg)
    eng.load_synthetic(42)
    eng.finalize()
    V = cfg.vocab_size
    ids = np.stack([synth.synth_prompt_ids(V, "vcoder_ds", sample=b) for b in range(B)])
    px = tuple(torch.from_numpy(a).cuda() for a in synth.synth_batch(B, cfg.vit_image_size))
    T = ids.shape[1]
    text = [np.nonzero(ids[b] >= 0)[0] for b in range(B)]
    lab16 = np.full_like(ids, -100)
    lab_all = np.full_like(ids, -100)
    for b in range(B):
        lab16[b, text[b][-16:]] = ids[b, text[b][-16:]]
        lab_all[b, text[b]] = ids[b, text[b]]
    rng = np.random.RandomState(0)
    cands = [rng.randint(3, V, size=(B, NC)).astype(np.int64) for _ in range(K)]
    S = eng.prefill(ids, *px)[2]
    rows = []

    def add(name, fn, note=""):
        med, lo, hi = timed(fn, args.reps)
        rows.append((name, med, lo, hi, note))
        print(f"{name}: {med:.1f} ms (min {lo:.1f} .. max {hi:.1f}) {note}", flush=True)

    add("plain prefill (last-row logits)", lambda: eng.prefill(ids, *px))

    def parent_way():
        _, full, _ = eng.prefill(ids, *px, all_logits=True)
        lp = torch.log_softmax(torch.from_numpy(full)[:, :-1], -1)
        return lp

    add("prefill(all_logits=True) + host log-softmax (the all-logits route)", parent_way,
        f"[{B}, {S}, {V}] fp32 = {B * S * V * 4 / 1e9:.2f} GB to the host")
    add("score: prefill(labels=), 16 labelled positions per sequence", lambda: eng.prefill(ids, *px, labels=lab16))
    add(f"score: prefill(labels=), every text position labelled ({int((lab_all != -100).sum())} rows)",
        lambda: eng.prefill(ids, *px, labels=lab_all))

    def extend_way():
        eng.prefill(ids, *px, reserve=NC + 1)
        for c in cands:
            eng.extend(c, all_logits=False, labels=c)
            eng.rewind(S)

    def reprefill_way():
        for c in cands:
            full_ids = np.concatenate([ids, c], 1)
            lab = np.concatenate([np.full_like(ids, -100), c], 1)
            eng.prefill(full_ids, *px, labels=lab)

    add(f"prefill once + {K} x (extend a {NC}-token candidate with labels, rewind)", extend_way)
    add(f"{K} labelled prefills of cat(prompt, candidate)", reprefill_way)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Wall times of scoring target tokens\n\n")
            f.write(f"One MI355X, VCoder-DS 7b, B = {B}, prompt of {T} ids -> S = {S} spliced rows, V = {V}, seeded synthetic weights "
                    f"and pixels as `bench.py` uses, pixels resident on the device, bf16 mode.  `tools/score_wall_times.py --reps "
                    f"{args.reps}`: per line 2 warm-up calls, then {args.reps} timed calls (host clock around the synchronous call, "
                    "host post-processing included where named); median and the spread.\n\n")
            f.write("| what | median ms | min .. max ms | note |\n|---|---|---|---|\n")
            for name, med, lo, hi, note in rows:
                f.write(f"| {name} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {note} |\n")
    eng.close()


if __name__ == "__main__":
    main()
