#!/usr/bin/env python
"""Wall times of generate(num_beams=n) on one MI355X: VCoder-DS 7b, B = 1, the COST-shaped prompt of bench.py (S = 1216), seeded
synthetic weights, no EOS (every call runs all its steps).  Per (n, new tokens): the device beam loop (vc_generate_beam) and the host
loop this tree keeps for beam-sample / stopping criteria / strict mode (generate(..., beam_on_device=False) — the only beam path of
the parent commit, unchanged here), with greedy generate at the same shape as the floor.  Every figure: 1 warm-up call, then `--reps`
timed calls (host clock around the synchronous call), median and min .. max; the host loop gets `--host-reps` calls (0 of either kind skips it).
usage: python tools/beam_wall_times.py [--reps 3] [--host-reps 1] [--beams 2,5] [--new 128,512] [--out profiles/beam_wall_times.md]
`--trace-shape n,new`: only that device-loop call, three times (for a rocprofv3 --kernel-trace --stats run around this tool; feed the
database to tools/rocpd_summary.py for the per-launch cost of beam_step_kernel and kv_permute_tail_kernel)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--beams", default="2,5")
    ap.add_argument("--new", default="128,512")
    ap.add_argument("--trace-shape", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = vcfg.vicuna_7b("vcoder_ds")
    model = lm.VCoderDSLlavaLlamaForCausalLM(cfg, device="cuda")
    model.engine.load_synthetic(42)
    model.finalize_weights()
    ids = torch.from_numpy(np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=0)]))
    imgs, segs, deps = (torch.from_numpy(a).cuda() for a in synth.synth_batch(1, cfg.vit_image_size))
    kw = dict(images=imgs, segs=segs, depths=deps, eos_token_id=-1)
    spliced = lambda: int(model.engine.lib.vc_last_spliced_len(model.engine._model))
    if args.trace_shape:
        n, new = (int(x) for x in args.trace_shape.split(","))
        for _ in range(3):
            model.generate(ids, num_beams=n, max_new_tokens=new, **kw)
        print(f"3 device-loop calls of num_beams {n}, {new} new tokens, S = {spliced()}")
        return
    rows = []

    def add(name, fn, reps, steps):
        med, lo, hi = timed(fn, reps)
        rows.append((name, med, lo, hi, med / steps))
        print(f"{name}: {med:.1f} ms (min {lo:.1f} .. max {hi:.1f}), {med / steps:.2f} ms per token", flush=True)

    for new in (int(x) for x in args.new.split(",")):
        if args.reps > 0:
            add(f"greedy generate, {new} new tokens (the floor)", lambda: model.generate(ids, max_new_tokens=new, **kw), args.reps, new)
        for n in (int(x) for x in args.beams.split(",")):
            if args.reps > 0:
                add(f"num_beams {n}, {new} new tokens: device loop", lambda: model.generate(ids, num_beams=n, max_new_tokens=new, **kw),
                    args.reps, new)
            if args.host_reps > 0:
                add(f"num_beams {n}, {new} new tokens: host loop (the parent's path)",
                    lambda: model.generate(ids, num_beams=n, max_new_tokens=new, beam_on_device=False, **kw), args.host_reps, new)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Wall times of beam search\n\n")
            f.write(f"One MI355X, VCoder-DS 7b, B = 1, prompt of {ids.shape[1]} ids -> S = {spliced()} spliced rows, seeded synthetic "
                    "weights and pixels as `bench.py` uses, pixels resident on the device, bf16 mode, no EOS.  `tools/beam_wall_times.py "
                    f"--reps {args.reps} --host-reps {args.host_reps}`: per line 1 warm-up call, then the timed calls (host clock around "
                    "the synchronous `generate`, encode and prefill of the expanded rows included); median and the spread.  The host "
                    "loop is `generate(..., beam_on_device=False)`: the parent commit's only beam path, unchanged in this tree.\n\n")
            f.write("| what | calls | median ms | min .. max ms | ms per token |\n|---|---|---|---|---|\n")
            for name, med, lo, hi, per in rows:
                reps = args.host_reps if "host loop" in name else args.reps
                f.write(f"| {name} | {reps} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {per:.2f} |\n")
    model.engine.close()


if __name__ == "__main__":
    main()
