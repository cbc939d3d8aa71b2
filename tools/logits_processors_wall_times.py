#!/usr/bin/env python
"""Wall times of generate() with logits processors on one MI355X: VCoder-DS 7b, the COST-shaped prompt of bench.py (S = 1216), seeded
synthetic weights, no EOS besides the one min_new_tokens bans (every call runs all its steps), B = 1 and B = 8, 128 new tokens.  Per
batch size: greedy generate without processors (the decode pool, as the benchmark), the same call on the session's own loop (a
log-prob request with K = 0 moves it there: the loop a processed call runs on), with all five processors on the device loop, and
the same call on the host loop (processors_on_device=False).  Every figure: 1 warm-up call, then `--reps` timed calls (host clock
around the synchronous call), median and min .. max.
usage: python tools/logits_processors_wall_times.py [--reps 7] [--host-reps 7] [--batches 1,8] [--new 128] [--out FILE.md]"""
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
from vcoder_amd.model import language_model as lm  # noqa: E402


def timed(fn, reps, warm=1):
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
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = vcfg.vicuna_7b("vcoder_ds")
    model = lm.VCoderDSLlavaLlamaForCausalLM(cfg, device="cuda")
    model.engine.load_synthetic(42)
    model.finalize_weights()
    new = args.new
    rows = []
    spliced = lambda: int(model.engine.lib.vc_last_spliced_len(model.engine._model))
    for B in (int(x) for x in args.batches.split(",")):
        ids = torch.from_numpy(np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b) for b in range(B)]))
        imgs, segs, deps = (torch.from_numpy(a).cuda() for a in synth.synth_batch(B, cfg.vit_image_size))
        kw = dict(images=imgs, segs=segs, depths=deps, max_new_tokens=new, pad_token_id=0)
        plain = model.generate(ids, eos_token_id=-1, **kw)[:, ids.shape[1]:]
        five = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=new, min_length=ids.shape[1] + new,
                    eos_token_id=int(plain[0, 1]), bad_words_ids=[[int(plain[0, 0])], [int(plain[0, 2]), int(plain[0, 3])]])

        def add(name, fn, reps):
            if reps <= 0:
                return
            med, lo, hi = timed(fn, reps)
            rows.append((f"B = {B}: {name}", reps, med, lo, hi, med / new))
            print(f"B = {B}: {name}: {med:.1f} ms (min {lo:.1f} .. max {hi:.1f}), {med / new:.3f} ms per token", flush=True)

        add("greedy generate, no processors (decode pool)", lambda: model.generate(ids, eos_token_id=-1, **kw), args.reps)
        add("greedy generate, no processors, session loop (output_logprobs=True)",
            lambda: model.generate(ids, eos_token_id=-1, output_logprobs=True, **kw), args.reps)
        add("all five processors, device loop", lambda: model.generate(ids, **five, **kw), args.reps)
        add("all five processors, host loop (processors_on_device=False)",
            lambda: model.generate(ids, processors_on_device=False, **five, **kw), args.host_reps)
        S = spliced()
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"One MI355X, VCoder-DS 7b, prompts of bench.py (S = {S} spliced rows), {new} new tokens, seeded synthetic weights and "
                    "pixels, pixels resident on the device, bf16 mode.  `tools/logits_processors_wall_times.py`: per line 1 warm-up call, "
                    "then the timed calls (host clock around the synchronous `generate`, encode and prefill included); median and the "
                    "spread.  The five processors: repetition_penalty 1.3, no_repeat_ngram_size 3, two bad words, min_new_tokens and "
                    "min_length that keep the EOS id banned for the whole call.\n\n")
            f.write("| what | calls | median ms | min .. max ms | ms per token |\n|---|---|---|---|---|\n")
            for name, reps, med, lo, hi, per in rows:
                f.write(f"| {name} | {reps} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {per:.3f} |\n")
    model.engine.close()


if __name__ == "__main__":
    main()
