#!/usr/bin/env python
"""Wall times of guided generate() on one MI355X: VCoder-DS 7b, the COST-shaped prompt of bench.py (S = 1216), seeded synthetic
weights, no EOS (every call runs all its steps), B = 1 and B = 4, 128 new tokens, greedy.  The negative prompt is the text-only one
(mm_utils.strip_placeholders: the question without its pictures).  Per batch size: the plain call (the decode pool, as the
benchmark), the plain call on the session's own loop (a log-prob request with K = 0 moves it there), the plain session-loop call over
2 B rows — what the guided step's forward costs without the new launches — guidance_scale on the device loop, and on the host loop
(processors_on_device=False).  Every figure: 1 warm-up call, then the timed calls (host clock around the synchronous call), median
and min .. max.
usage: python tools/guidance_wall_times.py [--reps 7] [--host-reps 3] [--batches 1,4] [--new 128] [--out FILE.md]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vcoder_amd import config as vcfg, mm_utils, synth  # noqa: E402
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
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = vcfg.vicuna_7b("vcoder_ds")
    model = lm.VCoderDSLlavaLlamaForCausalLM(cfg, device="cuda")
    model.engine.load_synthetic(42)
    model.finalize_weights()
    new = args.new
    rows = []
    S = Sn = 0
    for B in (int(x) for x in args.batches.split(",")):
        def inputs(n):
            ids = torch.from_numpy(np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b % B) for b in range(n)]))
            imgs, segs, deps = (torch.from_numpy(np.concatenate([x] * (n // B))).cuda() for x in synth.synth_batch(B, cfg.vit_image_size))
            return ids, dict(images=imgs, segs=segs, depths=deps, max_new_tokens=new, pad_token_id=0, eos_token_id=-1)

        ids, kw = inputs(B)
        ids2, kw2 = inputs(2 * B)
        neg = mm_utils.strip_placeholders(ids)
        gkw = dict(guidance_scale=args.scale, negative_prompt_ids=neg)
        dev = model.generate(ids, **gkw, **kw)
        S, Sn = model.engine.last_guidance["prompt_len"], model.engine.last_guidance["negative_len"]
        assert dev.shape[1] == ids.shape[1] + new

        def add(name, fn, reps, device_loop=True):
            if reps <= 0:
                return
            med, lo, hi = timed(fn, reps)
            # the engine's own event pair around the decode steps of the last call (vc_last_timings): the loop without encode and prefill
            dec = model.engine.last_timings()["decode_ms"] if device_loop else float("nan")
            rows.append((f"B = {B}: {name}", reps, med, lo, hi, dec, dec / max(new - 1, 1)))
            print(f"B = {B}: {name}: {med:.1f} ms (min {lo:.1f} .. max {hi:.1f}); decode loop of the last call {dec:.1f} ms = "
                  f"{dec / max(new - 1, 1):.3f} ms per step", flush=True)

        add("greedy generate, no guidance (decode pool)", lambda: model.generate(ids, **kw), args.reps)
        add("greedy generate, no guidance, session loop (output_logprobs=True)", lambda: model.generate(ids, output_logprobs=True, **kw), args.reps)
        add(f"greedy generate, no guidance, session loop over 2 B = {2 * B} rows (output_logprobs=True)",
            lambda: model.generate(ids2, output_logprobs=True, **kw2), args.reps)
        add("guidance_scale (text-only negative prompt), device loop", lambda: model.generate(ids, **gkw, **kw), args.reps)
        add("guidance_scale (text-only negative prompt), host loop (processors_on_device=False)",
            lambda: model.generate(ids, processors_on_device=False, **gkw, **kw), args.host_reps, device_loop=False)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"One MI355X, VCoder-DS 7b, prompts of bench.py (S = {S} spliced rows; text-only negative prompt of {Sn} ids), {new} new "
                    f"tokens, greedy, guidance scale {args.scale}, seeded synthetic weights and pixels, pixels resident on the device, bf16 "
                    "mode.  `tools/guidance_wall_times.py`: per line 1 warm-up call, then the timed calls (host clock around the "
                    "synchronous `generate`, encode and prefill included); median and the spread.  The 2 B-row plain call prefills 2 B "
                    "image prompts (the guided call prefills B image prompts and B text-only ones), so the whole calls are not "
                    "comparable; the last two columns are the engine's own event pair around the decode steps of the last timed call "
                    f"(vc_last_timings: the {new - 1} graph-replayed steps without encode and prefill).\n\n")
            f.write("| what | calls | median ms | min .. max ms | decode loop ms | ms per step |\n|---|---|---|---|---|---|\n")
            for name, reps, med, lo, hi, dec, per in rows:
                f.write(f"| {name} | {reps} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {dec:.1f} | {per:.3f} |\n")
    model.engine.close()


if __name__ == "__main__":
    main()
