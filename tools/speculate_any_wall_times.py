#!/usr/bin/env python
"""Whole-call wall times of sampled generate() with prompt-lookup speculation (speculate_selection="any") on one MI355X: VCoder-DS 7b,
the COST-shaped prompt of bench.py (S = 1216), seeded synthetic weights, no EOS (every call runs all its tokens), 128 new tokens, the
CLI's sampler (temperature 0.2, top_k 50), a fixed seed.  Per (weight format, batch size), every call on the session's own loop (a
log-prob request with K = 0 keeps the plain call there too, so that only the speculation differs): the plain call; k = 1 / 3 / 7 with the
call's own output as lookup_ids (the ceiling: every draft is accepted) and with random lookup_ids (the floor: the verify step's cost
with next to nothing accepted); then the same with all five logits processors on.  The ids of every speculated call are compared with
the plain call's.  Every figure: 1 warm-up call, then `--reps` timed calls (host clock around the synchronous call, encode and prefill
included), the median and the spread, and the call's acceptance counters (summed over the rows).
usage: python tools/speculate_any_wall_times.py [--reps 7] [--cases bf16:1,bf16:4,w4a16:1] [--new 128] [--out FILE.md]"""
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
    ap.add_argument("--cases", default="bf16:1,bf16:4,w4a16:1")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--ks", default="1,3,7")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    new, ks = args.new, [int(k) for k in args.ks.split(",")]
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    rows, S = [], 0
    for fmt in dict.fromkeys(f for f, _ in cases):
        cfg = vcfg.vicuna_7b("vcoder_ds")
        model = lm.VCoderDSLlavaLlamaForCausalLM(cfg, device="cuda")
        model.engine.load_synthetic(42)
        if fmt != "bf16":
            model.engine.set_weight_format(fmt)
        model.finalize_weights()
        for B in (b for f, b in cases if f == fmt):
            ids = torch.from_numpy(np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b) for b in range(B)]))
            T = ids.shape[1]
            imgs, segs, deps = (torch.from_numpy(a).cuda() for a in synth.synth_batch(B, cfg.vit_image_size))
            base = dict(images=imgs, segs=segs, depths=deps, max_new_tokens=new, pad_token_id=0, eos_token_id=-1, do_sample=True,
                        temperature=0.2, top_k=50, seed=7, output_logprobs=True)
            greedy = model.generate(ids, **dict(base, do_sample=False)).sequences[:, T:]
            five = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=new, min_length=T + new, eos_token_id=int(greedy[0, 1]),
                        bad_words_ids=[[int(greedy[0, 0])], [int(greedy[0, 2]), int(greedy[0, 3])]])
            rng = np.random.RandomState(3)
            for pname, pkw in (("no processors", {}), ("all five processors", five)):
                kw = dict(base, **pkw)
                plain = model.generate(ids, **kw).sequences[:, T:]
                looks = {"own output": [list(map(int, r)) for r in plain.numpy()],
                         "random": [list(map(int, rng.randint(0, cfg.vocab_size, size=new))) for _ in range(B)]}

                def add(name, fn):
                    out = fn()
                    assert torch.equal(out.sequences[:, T:], plain), f"{fmt} B {B} {pname} {name}: the ids differ from the plain call's"
                    sp = out.speculation
                    cnt = "" if sp is None else f"{int(sp['steps'].sum())} steps, {int(sp['accepted'].sum())} of {int(sp['drafted'].sum())} drafts accepted"
                    med, lo, hi = timed(fn, args.reps)
                    rows.append((f"{fmt}, B = {B}, {pname}: {name}", med, lo, hi, cnt))
                    print(f"{fmt} B = {B} {pname}: {name}: {med:.1f} ms (min {lo:.1f} .. max {hi:.1f}) {cnt}", flush=True)
                    return med

                t_plain = add("plain sampled call", lambda: model.generate(ids, **kw))
                for lname, look in looks.items():
                    for k in ks:
                        t = add(f"k = {k}, lookup_ids = {lname}", lambda: model.generate(ids, prompt_lookup_num_tokens=k, speculate_selection="any",
                                                                                         lookup_ids=look, **kw))
                        rows[-1] = rows[-1] + (t_plain / t,)
            S = int(model.engine.lib.vc_last_spliced_len(model.engine._model))
        model.engine.close()
        del model
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"One MI355X, VCoder-DS 7b, prompts of bench.py (S = {S} spliced rows), {new} new tokens, seeded synthetic weights and pixels, "
                    "pixels resident on the device.  `tools/speculate_any_wall_times.py`: sampled calls (temperature 0.2, top_k 50, seed 7) on the "
                    f"session's own loop; per line 1 warm-up call, then {args.reps} timed calls (host clock around the synchronous `generate`, encode "
                    "and prefill included): median and spread.  Every speculated call returned the plain call's ids.\n\n")
            f.write("| what | median ms | min .. max ms | counters (all rows) | plain / this |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r[0]} | {r[1]:.1f} | {r[2]:.1f} .. {r[3]:.1f} | {r[4]} | {'' if len(r) < 6 else '%.2f' % r[5]} |\n")


if __name__ == "__main__":
    main()
