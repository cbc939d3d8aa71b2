#!/usr/bin/env python
"""Wall times of constrained generate() on one MI355X: VCoder-DS 7b, the COST-shaped prompt of bench.py (S = 1216), seeded synthetic
weights, no EOS (every call runs all its steps), B = 1 and B = 8, 128 new tokens.  The constraint is a TokenAutomaton.from_list over a
133-entry class list (items of 1 .. 3 ids, one separator id, at least 64 items: the list cannot end within the call).  Per batch size:
greedy generate without it (the decode pool, as the benchmark), the same call on the session's own loop (a log-prob request with
K = 0 moves it there: the loop a constrained call runs on), with constraint= on the device loop, and the host loop under the
equivalent callable (prefix_allowed_tokens_fn).  Every figure: 1 warm-up call, then the timed calls (host clock around the synchronous
call), median and min .. max.
usage: python tools/constraint_wall_times.py [--reps 7] [--host-reps 3] [--batches 1,8] [--new 128] [--out FILE.md]"""
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
from vcoder_amd.constraints import TokenAutomaton  # noqa: E402
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


def class_list(V, n_items=133, min_items=64, seed=5):
    rng = np.random.RandomState(seed)
    pool = [int(t) for t in rng.choice(np.arange(1000, V), size=3 * n_items + 4, replace=False)]
    items = [pool[3 * i: 3 * i + 1 + i % 3] for i in range(n_items)]
    sep, term, end, pre = pool[3 * n_items:]
    return TokenAutomaton.from_list([pre], items, [sep], [term], [end], min_items=min_items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = vcfg.vicuna_7b("vcoder_ds")
    model = lm.VCoderDSLlavaLlamaForCausalLM(cfg, device="cuda")
    model.engine.load_synthetic(42)
    model.finalize_weights()
    new = args.new
    a = class_list(cfg.vocab_size)
    rows = []
    for B in (int(x) for x in args.batches.split(",")):
        ids = torch.from_numpy(np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b) for b in range(B)]))
        T = ids.shape[1]
        imgs, segs, deps = (torch.from_numpy(x).cuda() for x in synth.synth_batch(B, cfg.vit_image_size))
        kw = dict(images=imgs, segs=segs, depths=deps, max_new_tokens=new, pad_token_id=0, eos_token_id=-1)
        dev = model.generate(ids, constraint=a, **kw)[:, T:]
        assert all(a.walk(r) >= 0 for r in dev.tolist()) and dev.shape[1] == new

        def add(name, fn, reps):
            if reps <= 0:
                return
            med, lo, hi = timed(fn, reps)
            rows.append((f"B = {B}: {name}", reps, med, lo, hi, med / new))
            print(f"B = {B}: {name}: {med:.1f} ms (min {lo:.1f} .. max {hi:.1f}), {med / new:.3f} ms per token", flush=True)

        add("greedy generate, no constraint (decode pool)", lambda: model.generate(ids, **kw), args.reps)
        add("greedy generate, no constraint, session loop (output_logprobs=True)", lambda: model.generate(ids, output_logprobs=True, **kw), args.reps)
        add("constraint= (133-entry class list), device loop", lambda: model.generate(ids, constraint=a, **kw), args.reps)
        add("prefix_allowed_tokens_fn (the same automaton's callable), host loop",
            lambda: model.generate(ids, prefix_allowed_tokens_fn=a.as_prefix_allowed_tokens_fn(T), **kw), args.host_reps)
        S = int(model.engine.lib.vc_last_spliced_len(model.engine._model))
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"One MI355X, VCoder-DS 7b, prompts of bench.py (S = {S} spliced rows), {new} new tokens, seeded synthetic weights and "
                    "pixels, pixels resident on the device, bf16 mode.  `tools/constraint_wall_times.py`: per line 1 warm-up call, then the "
                    "timed calls (host clock around the synchronous `generate`, encode and prefill included); median and the spread.  "
                    f"The automaton: `from_list` over 133 items of 1 .. 3 ids, at least 64 items ({a.num_states} states, {a.num_edges} "
                    "edges).\n\n")
            f.write("| what | calls | median ms | min .. max ms | ms per token |\n|---|---|---|---|---|\n")
            for name, reps, med, lo, hi, per in rows:
                f.write(f"| {name} | {reps} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {per:.3f} |\n")
    model.engine.close()


if __name__ == "__main__":
    main()
