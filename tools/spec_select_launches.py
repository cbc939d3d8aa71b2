#!/usr/bin/env python
"""Per-launch times of what a verify step of speculate_selection="any" adds, on one MI355X at V = 32000: spec_select_kernel (sampled:
temperature 0.2, top_k 50; and greedy) and the verify form of logits_process_kernel (all processors on, a history of 600 prompt + 64
generated ids) over R = B * Q rows, beside select_embed_kernel sampling ONE row (what a plain sampled step pays) and spec_accept_kernel
taking the argmax of the rows itself (the greedy verify step) or walking given selections.  Each kernel is launched `--reps` times back
to back between two device events (the mean includes the gap between launches); run it under
`rocprofv3 --kernel-trace --stats -- python tools/spec_select_launches.py --rows R` for the kernels' own durations, one run per R (the
names do not carry the row count).
usage: python tools/spec_select_launches.py --rows 2|8|32 [--reps 200]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vcoder_amd import _lib  # noqa: E402

RS = dict(ACTIVE=0, STEP=2, MAXNEW=4, EOS=5, SAMPLE=8, INVTEMP=9, TOPK=10, TOPP=11, SEED_LO=12, SEED_HI=13, OUT_OFF=14, LP_PENALTY=15,
          LP_NGRAM=96, LP_MINNEW=97, LP_HIST_OFF=98, LP_HIST_LEN=99, LP_NBAD=100, STRIDE=128)   # csrc/kernels.h RowStateField
f32_bits = lambda x: int(np.float32(x).view(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V, R = 32000, args.rows
    Q = min(R, 8)
    B = R // Q
    assert B * Q == R and R <= 32
    rng = np.random.RandomState(0)
    P = lambda t: C.c_void_p(t.data_ptr())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    lg = torch.from_numpy((rng.randn(4, R, V) * 3).astype(np.float32)).to(dev)   # four buffers in turn: 16 MB at 32 rows
    out = torch.empty(R, V, dtype=torch.float32, device=dev)

    def records(sample, step, max_new):
        r = np.zeros((B, RS["STRIDE"]), np.int32)
        r[:, RS["ACTIVE"]], r[:, RS["EOS"]], r[:, RS["STEP"]], r[:, RS["MAXNEW"]] = 1, 2, step, max_new
        r[:, RS["SAMPLE"]], r[:, RS["INVTEMP"]], r[:, RS["TOPK"]], r[:, RS["TOPP"]] = sample, f32_bits(5.0), 50, f32_bits(1.0)
        r[:, RS["SEED_LO"]], r[:, RS["SEED_HI"]] = 11, 12
        r[:, RS["OUT_OFF"]] = np.arange(B) * 256
        r[:, RS["LP_PENALTY"]], r[:, RS["LP_NGRAM"]], r[:, RS["LP_MINNEW"]] = f32_bits(1.3), 3, 1000
        r[:, RS["LP_HIST_LEN"]], r[:, RS["LP_NBAD"]] = 600, 2
        return i32(r)

    sampled, greedy, idle = records(1, 64, 200), records(0, 64, 200), records(1, 64, 0)   # idle: MAXNEW 0, nothing is recorded
    prompt, gen = i32(rng.randint(0, V, 600)), i32(rng.randint(0, V, B * 256))
    tab = np.zeros((32, 9), np.int32)
    tab[0, :2], tab[1, :3] = (1, 17), (2, 5, 19)
    tab = i32(tab)
    tok, nq, sel, nxt = i32(rng.randint(0, V, R)), i32(np.full(B, Q)), i32(rng.randint(0, V, R)), i32(np.zeros(B))
    one = i32(records(1, 64, 0).cpu().numpy()[:1])
    it = [0]

    def cur():
        it[0] += 1
        return lg[it[0] % 4]

    kinds = {
        "spec_select, sampled, %d rows" % R: lambda: lib.vck_spec_select(P(cur()), V, V, P(sampled), P(nq), P(sel), B, Q, -1, None),
        "spec_select, greedy, %d rows" % R: lambda: lib.vck_spec_select(P(cur()), V, V, P(greedy), P(nq), P(sel), B, Q, -1, None),
        "logits_process (verify form), all on, %d rows" % R: lambda: lib.vck_logits_process_verify(
            P(cur()), V, P(out), V, P(sampled), P(prompt), P(gen), P(tab), P(tok), P(nq), B, Q, V, None),
        "select_embed, sampled, 1 row (a plain step's selection)": lambda: lib.vck_select_embed(
            P(cur()), V, P(one), P(nxt), P(gen), None, None, None, None, None, 4096, 16, V, 1, 0, None),
        "spec_accept, argmax of its rows (the greedy verify step), %d rows" % R: lambda: lib.vck_spec_accept(
            P(cur()), V, V, P(idle), P(nxt), P(gen), P(tok), P(nq), B, Q, None, None, None, 1, None, None, None, 0, None),
        "spec_accept on given selections, %d rows" % R: lambda: lib.vck_spec_accept_sel(
            P(cur()), V, V, P(idle), P(nxt), P(gen), P(tok), P(nq), B, Q, None, None, None, 1, None, None, None, 0, P(sel), None, None),
    }
    for name, fn in kinds.items():
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name}: {e0.elapsed_time(e1) / args.reps * 1e3:.1f} us per launch ({args.reps} back to back)", flush=True)


if __name__ == "__main__":
    main()
