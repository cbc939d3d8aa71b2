#!/usr/bin/env python
"""Wall time of generate() per decoder weight format on an MI355X: the synthetic 7b (or 13b) VCoder-DS checkpoint, the benchmark's
prompt (S = 1216 after the splice), greedy decoding of --new-tokens tokens at each batch size, one engine per format.  Prints, per
format and batch: the wall time of a 1-token and of the full call (median of --reps) and the decode step that follows from them;
and, against the first format listed, the first-step logits' largest deviation and Pearson correlation (how far the quantisation
moves the model on this checkpoint).

usage: python tools/format_wall.py [--model 7b] [--formats bf16,w8a16,w4a16] [--batches 1,8] [--new-tokens 128] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from vcoder_amd import config as vcfg, synth  # noqa: E402
from vcoder_amd.engine import HipEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["7b", "13b"])
    ap.add_argument("--formats", default="bf16,w8a16,w4a16")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    cfg = vcfg.vicuna_7b("vcoder_ds") if args.model == "7b" else vcfg.vicuna_13b("vcoder_ds")
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches)
    ids = np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=b) for b in range(Bmax)])
    px = tuple(torch.from_numpy(a).cuda() for a in synth.synth_batch(Bmax, cfg.vit_image_size, 0))
    base = None
    for fmt in args.formats.split(","):
        eng = HipEngine(cfg)
        eng.load_synthetic(42)
        if fmt != "bf16":
            eng.set_weight_format(fmt)
        eng.finalize()
        last, _, S = eng.prefill(ids[:1], *(p[:1] for p in px))
        if base is None:
            base = last
        else:
            d = float(np.abs(last - base).max())
            c = float(np.corrcoef(last.ravel().astype(np.float64), base.ravel().astype(np.float64))[0, 1])
            print(f"{args.model} {fmt:6s} first-step logits vs {args.formats.split(',')[0]}: max |diff| {d:.4f} of max |logit| "
                  f"{float(np.abs(base).max()):.4f}, correlation {c:.6f}, same argmax {bool(np.argmax(last) == np.argmax(base))}", flush=True)
        for B in batches:
            def wall(n):
                ts = []
                for _ in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eng.generate_greedy(ids[:B], *(p[:B] for p in px), max_new_tokens=n, eos_token_id=None)
                    ts.append(time.perf_counter() - t0)
                return float(np.median(ts[1:])) * 1e3   # the first call warms (graph capture, pool)
            t1, tn = wall(1), wall(args.new_tokens)
            print(f"{args.model} {fmt:6s} S={S} B={B}: generate(1) {t1:8.1f} ms | generate({args.new_tokens}) {tn:8.1f} ms | "
                  f"decode {tn - t1:7.1f} ms = {(tn - t1) / (args.new_tokens - 1):6.3f} ms / step", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
