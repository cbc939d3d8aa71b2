#!/usr/bin/env python
"""Wall times of generate(num_return_sequences=n) on one MI355X: VCoder-DS 7b, the COST-shaped prompt of bench.py (S = 1216), seeded
synthetic weights, sampling with a fixed seed, no EOS (every call runs all its steps), 128 new tokens.  Per (B, n) and weight
format: the fan-out call (one prefill over the B prompts, the fan-out attention) and the replicated call of the same tree
(fan_out=False: the engine repeats the prompts n times), each with the engine's own split of the call into encode, prefill and decode
(vc_last_timings).  Both run in the batch-invariant mode, which the fan-out form needs at these dims.  Every figure: 1 warm-up call, then `--reps` timed calls (host clock around the synchronous call), median and
min .. max; the phase times are the medians of the same calls.
usage: python tools/fanout_wall_times.py [--reps 7] [--cases 1x2,1x4,1x8,2x8] [--formats bf16,w8a16] [--new 128] [--out FILE.md]"""
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


def timed(eng, fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts, ph = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        ph.append(eng.last_timings())
    med = lambda k: statistics.median(p[k] for p in ph)
    return statistics.median(ts), min(ts), max(ts), med("encode_ms"), med("prefill_ms"), med("decode_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="1x2,1x4,1x8,2x8")
    ap.add_argument("--formats", default="bf16,w8a16")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    new = args.new
    rows, S = [], 0
    for fmt in args.formats.split(","):
        cfg = vcfg.vicuna_7b("vcoder_ds")
        eng = HipEngine(cfg)
        eng.load_synthetic(42)
        if fmt != "bf16":
            eng.set_weight_format(fmt)
        eng.finalize()
        eng.set_batch_invariant(True)   # at 7b dims the fan-out form is served in this mode only; the replicated call runs in it too
        for case in args.cases.split(","):
            B, n = (int(x) for x in case.split("x"))
            ids = np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b) for b in range(B)])
            px = tuple(torch.from_numpy(a).cuda() for a in synth.synth_batch(B, cfg.vit_image_size))
            kw = dict(max_new_tokens=new, do_sample=True, temperature=1.0, top_k=50, seed=7, num_return_sequences=n)
            a = eng.generate(ids, *px, fan_out=True, **kw)
            shared = eng.last_fanout["shared"]
            b = eng.generate(ids, *px, fan_out=False, **kw)
            same = bool(np.array_equal(a, b))
            S = int(eng.lib.vc_last_spliced_len(eng._model))
            for name, extra in (("fan-out", dict(fan_out=True)), ("replicated (fan_out=False)", dict(fan_out=False))):
                r = timed(eng, lambda: eng.generate(ids, *px, **kw, **extra), args.reps)
                rows.append((fmt, B, n, name, args.reps) + r)
                print(f"{fmt} B = {B} n = {n} {name}: {r[0]:.1f} ms (min {r[1]:.1f} .. max {r[2]:.1f}); encode {r[3]:.1f} prefill {r[4]:.1f} "
                      f"decode {r[5]:.1f} ms [served {shared}, ids equal to the replicated call's {same}]", flush=True)
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"One MI355X, VCoder-DS 7b, prompts of bench.py (S = {S} spliced rows), {new} new tokens, sampling (temperature 1.0, top-k "
                    "50, fixed seed), batch-invariant mode, seeded synthetic weights and pixels, pixels resident on the device.  `tools/fanout_wall_times.py`: per "
                    "line 1 warm-up call, then the timed calls (host clock around the synchronous `generate`); median and the spread; "
                    "encode / prefill / decode: medians of vc_last_timings over the same calls.\n\n")
            f.write("| weights | B | n | call | calls | median ms | min .. max ms | encode ms | prefill ms | decode ms |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for fmt, B, n, name, reps, med, lo, hi, e, p, d in rows:
                f.write(f"| {fmt} | {B} | {n} | {name} | {reps} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {e:.1f} | {p:.1f} | {d:.1f} |\n")


if __name__ == "__main__":
    main()
