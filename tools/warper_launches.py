#!/usr/bin/env python
"""Per-launch time of the sampled selection (select_embed_kernel, ONE row at V = 32000: what a plain sampled step pays) with the
further warpers off, each on alone and all on, on one MI355X.  The base setting is serve/cli.py's (temperature 0.2, top_k 50); the
`nucleus` lines add top_p 0.95, the phase typical sampling is compared with.  Each setting is launched `--reps` times back to back
between two device events (the mean includes the gap between launches), `--rounds` times in turn, so that the spread of a setting's
own repeats stands beside the differences.  --lib PATH times another build of the library (the parent commit's, which knows only the
`off` records) for the alternating comparison.
usage: python tools/warper_launches.py [--lib PATH] [--only-off] [--reps 200] [--rounds 5]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

RS = dict(ACTIVE=0, STEP=2, MAXNEW=4, EOS=5, SAMPLE=8, INVTEMP=9, TOPK=10, TOPP=11, SEED_LO=12, SEED_HI=13, MINP=114, TYPICAL=115, EPS=116,
          ETA=117, STRIDE=128)   # csrc/kernels.h RowStateField
f32_bits = lambda x: int(np.float32(x).view(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    if args.lib:
        lib = C.CDLL(args.lib)
    else:
        from vcoder_amd import _lib

        lib = _lib.load()
    V = 32000
    rng = np.random.RandomState(0)
    P = lambda t: C.c_void_p(t.data_ptr())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    lg = torch.from_numpy((rng.randn(4, V) * 3).astype(np.float32)).to(dev)   # four rows in turn

    def record(top_p=1.0, **warp):
        r = np.zeros((1, RS["STRIDE"]), np.int32)
        r[:, RS["ACTIVE"]], r[:, RS["EOS"]], r[:, RS["STEP"]], r[:, RS["MAXNEW"]] = 1, 2, 64, 0   # MAXNEW 0: nothing is recorded
        r[:, RS["SAMPLE"]], r[:, RS["INVTEMP"]], r[:, RS["TOPK"]], r[:, RS["TOPP"]] = 1, f32_bits(5.0), 50, f32_bits(top_p)
        r[:, RS["SEED_LO"]], r[:, RS["SEED_HI"]] = 11, 12
        for k, v in warp.items():
            r[:, RS[k]] = f32_bits(v)
        return i32(r)

    kinds = {"off": record(), "off, nucleus": record(0.95)}
    if not args.only_off:
        kinds.update({"min_p 0.05": record(MINP=0.05), "typical_p 0.9": record(TYPICAL=0.9), "epsilon_cutoff 3e-4": record(EPS=3e-4),
                      "eta_cutoff 2e-3": record(ETA=2e-3), "all four": record(MINP=0.02, TYPICAL=0.95, EPS=1e-3, ETA=2e-3),
                      "all four, nucleus": record(0.95, MINP=0.02, TYPICAL=0.95, EPS=1e-3, ETA=2e-3)})
    nxt, gen = i32(np.zeros(1)), i32(np.zeros(256))
    it = [0]

    def launch(rec):
        it[0] += 1
        lib.vck_select_embed(P(lg[it[0] % 4]), V, P(rec), P(nxt), P(gen), None, None, None, None, None, 4096, 16, V, 1, 0, None)

    times = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for name, rec in kinds.items():
            for _ in range(10):
                launch(rec)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch(rec)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    for name, t in times.items():
        print(f"{name}: median {np.median(t):.1f} us per launch, {min(t):.1f} .. {max(t):.1f} over {args.rounds} rounds of {args.reps}", flush=True)


if __name__ == "__main__":
    main()
