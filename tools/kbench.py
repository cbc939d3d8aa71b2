#!/usr/bin/env python
"""Per-kernel micro-benchmark on an MI355X through the vck_* C ABI (include/vcoder_kernels.h), timed with events on the
default stream.  usage: python tools/kbench.py [gemm] [gemv] [attn] [dattn]   (env knobs are read by the library)"""
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from vcoder_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def bf16(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def bench_gemm():
    for (M, N, K, epi, name) in [(9728, 12288, 4096, 0, "llm qkv"), (9728, 4096, 4096, 4, "llm o"),
                                 (9728, 22016, 4096, 5, "llm gate-up"), (9728, 22016, 4096, 0, "gate-up/bf16"),
                                 (9728, 22016, 4096, 3, "gate-up/f32"), (9728, 4096, 11008, 4, "llm down"),
                                 (13848, 3072, 1024, 0, "vit qkv"), (13848, 4096, 1024, 1, "vit fc1"),
                                 (13848, 1024, 4096, 4, "vit fc2"), (13824, 4096, 4096, 0, "adapter 2")]:
        A, W = bf16(M, K), bf16(N, K, scale=0.02)
        out = torch.zeros((M, N), dtype=torch.float32 if epi in (3, 4) else torch.bfloat16, device=dev)
        ldo = N // 2 if epi == 5 else N
        us = timeit(lambda: lib.vck_gemm(P(A), P(W), None, P(out), M, N, K, K, K, ldo, epi, None), iters=10)
        print(f"gemm {name:12s} M{M} N{N} K{K} epi{epi}: {us:9.1f} us  {2 * M * N * K / us / 1e6:7.1f} TFLOP/s", flush=True)
        ws = torch.zeros(16 << 20, device=dev)   # 64 MiB fp32 workspace: split-K of a short last round of tiles
        us = timeit(lambda: lib.vck_gemm_ws(P(A), P(W), None, P(out), M, N, K, K, K, ldo, epi, P(ws), C.c_size_t(64 << 20), None),
                    iters=10)
        print(f"gemm+ws {name:9s}                         : {us:9.1f} us  {2 * M * N * K / us / 1e6:7.1f} TFLOP/s", flush=True)


def bench_gemm_qkv():
    """Round 6: the QKV projection of a prefill layer as GEMM (EPI_BF16) + qkv_split against the GEMM with RoPE + head split + KV write
    in its epilogue (vck_gemm_qkv), with / without the split-K workspace."""
    for (B, T, H, K, name) in [(8, 1216, 32, 4096, "7b B=8"), (16, 1216, 40, 5120, "13b B=16"), (8, 1217, 32, 4096, "7b B=8 S=1217")]:
        D, M = H * 128, B * T
        Ts, S_cap = (T + 63) // 64 * 64, 1344
        A, W = bf16(M, K), bf16(3 * D, K, scale=0.02)
        qkv = torch.zeros((M, 3 * D), dtype=torch.bfloat16, device=dev)
        q, vt = torch.zeros((B, H, Ts, 128), dtype=torch.bfloat16, device=dev), torch.zeros((B, H, 128, Ts), dtype=torch.bfloat16, device=dev)
        k, v = torch.zeros((B, H, S_cap, 128), dtype=torch.bfloat16, device=dev), torch.zeros((B, H, S_cap, 128), dtype=torch.bfloat16, device=dev)
        cos, sin = torch.rand(S_cap, 64, device=dev), torch.rand(S_cap, 64, device=dev)
        ws = torch.zeros(16 << 20, device=dev)
        for wsb in (64 << 20, 0):
            wp = P(ws) if wsb else None
            g = timeit(lambda: lib.vck_gemm_ws(P(A), P(W), None, P(qkv), M, 3 * D, K, K, K, 3 * D, 0, wp, C.c_size_t(wsb), None), iters=10)
            sp = timeit(lambda: lib.vck_qkv_split_kv(P(qkv), P(q), P(k), P(v), P(vt), B, T, H, 128, Ts, S_cap, Ts, P(cos), P(sin), None), iters=10)
            f = timeit(lambda: lib.vck_gemm_qkv(P(A), None, P(W), None, None, B, T, H, K, K, P(q), P(k), P(v), P(vt), None, None, Ts, S_cap,
                                                 Ts, 0, P(cos), P(sin), 0, wp, C.c_size_t(wsb), None), iters=10)
            print(f"gemm_qkv {name:14s} ws={wsb >> 20:2d}MiB: gemm {g:8.1f} + split {sp:6.1f} = {g + sp:8.1f} us   fused {f:8.1f} us   "
                  f"({2 * M * 3 * D * K / f / 1e6:6.1f} TF/s)", flush=True)


def bench_gemm_f8():
    """W8A8 prefill linears (weight format 2): the activation quantiser and the e4m3 x e4m3 GEMM, next to the bf16 GEMM of the
    same shape (7b B=8 and 13b B=16 prefill shapes)."""
    ws = torch.zeros(16 << 20, device=dev)
    for (M, N, K, epi, name) in [(9728, 12288, 4096, 0, "7b qkv"), (9728, 4096, 4096, 4, "7b o"),
                                 (9728, 22016, 4096, 5, "7b gate-up"), (9728, 4096, 11008, 4, "7b down"),
                                 (19456, 15360, 5120, 0, "13b qkv"), (19456, 5120, 5120, 4, "13b o"),
                                 (19456, 27648, 5120, 5, "13b gate-up"), (19456, 5120, 13824, 4, "13b down")]:
        A, W = bf16(M, K), bf16(N, K, scale=0.02)
        out = torch.zeros((M, N), dtype=torch.float32 if epi in (3, 4) else torch.bfloat16, device=dev)
        ldo = N // 2 if epi == 5 else N
        us16 = timeit(lambda: lib.vck_gemm_ws(P(A), P(W), None, P(out), M, N, K, K, K, ldo, epi, P(ws), C.c_size_t(64 << 20), None),
                      iters=10)
        Q = torch.zeros((M, K), dtype=torch.uint8, device=dev)
        sa = torch.zeros(M, device=dev)
        Wq = torch.zeros(N * K, dtype=torch.uint8, device=dev)
        Wrow = torch.zeros((N, K), dtype=torch.uint8, device=dev)
        sw = torch.zeros(N, device=dev)
        lib.vck_quantize_fp8_rows(P(W), P(Wq), P(sw), P(Wrow), N, K, None)
        usq = timeit(lambda: lib.vck_quant_act_rows(P(A), K, P(Q), P(sa), M, K, None), iters=10)
        us8 = timeit(lambda: lib.vck_gemm_f8(P(Q), P(sa), P(Wrow), P(sw), P(out), M, N, K, ldo, epi, P(ws), C.c_size_t(64 << 20),
                                             None), iters=10)
        fl = 2 * M * N * K / 1e6
        print(f"gemm_f8 {name:12s} M{M} N{N} K{K}: bf16 {us16:8.1f} us {fl / us16:7.1f} TF | quant {usq:6.1f} us "
              f"({M * K * 3 / usq / 1e3:6.0f} GB/s) + e4m3 {us8:8.1f} us {fl / us8:7.1f} TF  => x{us16 / (usq + us8):.2f}", flush=True)


def bench_gemv():
    M = 8
    for (N, K, epi, name) in [(12288, 4096, 0, "qkv"), (4096, 4096, 2, "o"), (22016, 4096, 3, "gate-up"),
                              (4096, 11008, 2, "down"), (32000, 4096, 1, "lm_head")]:
        X = bf16(M, K)
        # rotate over 8 weight copies so the 256 MB Infinity Cache cannot hold them
        Ws = [bf16(N * K, scale=0.02) for _ in range(8)]
        out = torch.zeros((M, N), dtype=torch.float32 if epi in (1, 2) else torch.bfloat16, device=dev)
        ldo = N // 2 if epi == 3 else N
        it = [0]

        def f():
            it[0] += 1
            lib.vck_gemv(P(X), P(Ws[it[0] % 8]), P(out), M, N, K, ldo, epi, None)
        us = timeit(f, iters=40)
        print(f"gemv {name:8s} N{N} K{K} epi{epi}: {us:7.1f} us  {2 * N * K / us / 1e3:7.1f} GB/s", flush=True)
        if epi == 2:
            scratch = torch.zeros(4 * (N // 16) * 2 * 256, device=dev)
            counters = torch.zeros(N // 16 * 2, dtype=torch.int32, device=dev)
            for ks in (2, 3, 4):
                def h():
                    it[0] += 1
                    lib.vck_gemv_ex(P(X), P(Ws[it[0] % 8]), None, P(out), None, None, None, None, 16, C.c_float(1e-5), P(scratch),
                                    P(counters), ks, M, N, K, ldo, epi, None)
                us = timeit(h, iters=40)
                print(f"gemv {name:8s} split-K {ks}: {us:7.1f} us  {2 * N * K / us / 1e3:7.1f} GB/s", flush=True)
        if epi in (0, 1, 3):
            xf = torch.randn(16, K, device=dev)
            w = torch.rand(K, device=dev) + 0.5
            npart = (K // 16 + 15) // 16 * 16
            ssq = torch.rand(16, npart, device=dev)

            def g():
                it[0] += 1
                lib.vck_gemv_ex(P(X), P(Ws[it[0] % 8]), None, P(out), P(ssq), None, None, None, npart, C.c_float(1e-5), None, None,
                                0, M, N, K, ldo, epi, None)
            us = timeit(g, iters=40)
            print(f"gemv+rstd {name:8s}          : {us:7.1f} us  {2 * N * K / us / 1e3:7.1f} GB/s", flush=True)


def bench_gemv_rows():
    """The decode pool's question: what does a weight pass cost at M = 8 / 16 (one row group) and M = 24 / 32 (two)?
    7b shapes with the folded-RMSNorm operands the engine uses (consumers scale by rstd; producers publish partials + xg)."""
    for M in (8, 16, 24, 32):
        tot = 0.0
        for (N, K, epi, name, cnt) in [(12288, 4096, 0, "qkv", 32), (4096, 4096, 2, "o", 32), (22016, 4096, 3, "gate-up", 32),
                                       (4096, 11008, 2, "down", 32), (32000, 4096, 1, "lm_head", 1)]:
            X = bf16(32, K)
            Ws = [bf16(N * K, scale=0.02) for _ in range(8)]
            out = torch.zeros((32, N), dtype=torch.float32 if epi in (1, 2) else torch.bfloat16, device=dev)
            ldo = N // 2 if epi == 3 else N
            npart = (4096 // 16 + 15) // 16 * 16
            ssq = torch.rand(32, npart, device=dev)
            gw = torch.rand(N, device=dev) + 0.5
            xg = torch.zeros((32, N), dtype=torch.bfloat16, device=dev)
            scratch = torch.zeros(4 * (N // 16) * 2 * 256, device=dev)
            counters = torch.zeros(N // 16 * 2, dtype=torch.int32, device=dev)
            it = [0]

            def f():
                it[0] += 1
                if epi == 2:
                    lib.vck_gemv_ex(P(X), P(Ws[it[0] % 8]), None, P(out), None, P(ssq), P(gw), P(xg), npart, C.c_float(1e-5),
                                    P(scratch), P(counters), 0, M, N, K, ldo, epi, None)
                else:
                    lib.vck_gemv_ex(P(X), P(Ws[it[0] % 8]), None, P(out), P(ssq), None, None, None, npart, C.c_float(1e-5),
                                    None, None, 0, M, N, K, ldo, epi, None)
            us = timeit(f, iters=40)
            tot += us * cnt
            print(f"gemv_rows M{M:2d} {name:8s} N{N} K{K}: {us:7.1f} us  {2 * N * K / us / 1e3:7.1f} GB/s", flush=True)
        print(f"gemv_rows M{M:2d} all GEMVs of a 7b decode step: {tot / 1e3:6.3f} ms = {tot / 1e3 / M:6.4f} ms per row", flush=True)


def bench_gemv_wg():
    """the GEMV of precision mode "split" (gemv_wg_kernel: hi / lo activation rows in one weight pass) at the 7b shapes, 8 and 32 rows:
    four waves per workgroup everywhere (vck_set_gemv_variant(2), rounds 4-5) against the launcher's choice (six where that balances
    the launch: qkv, gate / up)"""
    lib.vck_gemv_full.restype = None
    for M, G in ((8, 8), (32, 32)):
        tot = {2: 0.0, -1: 0.0}
        for (N, K, epi, name, cnt) in [(12288, 4096, 1, "qkv", 32), (4096, 4096, 2, "o", 32), (22016, 4096, 3, "gate-up", 32),
                                       (4096, 11008, 2, "down", 32), (32000, 4096, 1, "lm_head", 1)]:
            X = bf16(2 * G, K)
            Ws = [bf16(N * K, scale=0.02) for _ in range(8)]
            rows_out = 2 * G if epi == 3 else 32
            out = torch.zeros((max(rows_out, 32), N), dtype=torch.float32 if epi in (1, 2) else torch.bfloat16, device=dev)
            ldo = N // 2 if epi == 3 else N
            npart = (max(K, N) // 16 + 15) // 16 * 16
            ssq = torch.rand(32, npart, device=dev)
            ssq_out = torch.zeros(32, npart, device=dev)
            gw = torch.rand(N, device=dev) + 0.5
            xg = torch.zeros((2 * G, N), dtype=torch.bfloat16, device=dev)
            nsk = 4 * (N // 16) * 2 * 256
            scratch = torch.zeros(nsk, device=dev)
            counters = torch.zeros(N // 16 * 2, dtype=torch.int32, device=dev)
            row = []
            for v in (2, -1):
                lib.vck_set_gemv_variant(v)
                it = [0]

                def f():
                    it[0] += 1
                    prod = epi == 2
                    lib.vck_gemv_full(P(X), P(Ws[it[0] % 8]), None, P(out), None if prod else P(ssq), P(ssq_out) if prod else None,
                                      P(gw) if prod else None, P(xg) if prod else None, C.c_int(npart), C.c_float(1e-5), P(scratch),
                                      C.c_ulonglong(nsk), P(counters), C.c_int(N // 16 * 2), C.c_int(0), M, N, K, ldo, epi, G, None)
                us = timeit(f, iters=60)
                tot[v] += us * cnt
                row.append(f"{'4 waves' if v == 2 else 'chosen '} {us:6.2f} us {2 * N * K / us / 1e3:6.0f} GB/s")
            print(f"gemv_wg M{M:2d} {name:8s} N{N} K{K}: " + " | ".join(row), flush=True)
        print(f"gemv_wg M{M:2d} all GEMVs of a 7b split step: 4 waves {tot[2] / 1e3:6.3f} ms | chosen {tot[-1] / 1e3:6.3f} ms", flush=True)
    lib.vck_set_gemv_variant(-1)


def bench_gemv_wide():
    """ring-kernel GEMV, pair geometry (vck_set_gemv_wide 0) vs the "wide" one (2: ceil(tiles / 256) tiles per workgroup, one deep
    ring per CU, every class) on every > 512-tile matrix of the 7b and 13b models at 8 / 16 / 24 / 32 rows; same bits?"""
    for (N, K, epi, name) in [(12288, 4096, 0, "7b qkv"), (22016, 4096, 3, "7b gate-up"), (15360, 5120, 0, "13b qkv"),
                              (27648, 5120, 3, "13b gate-up")]:
        X = bf16(32, K)
        Ws = [bf16(N * K, scale=0.02) for _ in range(6)]
        ldo = N // 2 if epi == 3 else N
        npart = (K // 16 + 15) // 16 * 16
        ssq = torch.rand(32, npart, device=dev)
        it = [0]
        for M in (8, 16, 24, 32):
            outs, t = {}, {}
            for wide in (0, 2):
                lib.vck_set_gemv_wide(wide)
                out = torch.zeros((32, ldo), dtype=torch.float32 if epi == 1 else torch.bfloat16, device=dev)

                def f():
                    it[0] += 1
                    lib.vck_gemv_ex(P(X), P(Ws[it[0] % 6]), None, P(out), P(ssq), None, None, None, npart, C.c_float(1e-5),
                                    None, None, 0, M, N, K, ldo, epi, None)
                t[wide] = timeit(f, iters=40)
                it[0] = 5
                f()
                torch.cuda.synchronize()
                outs[wide] = out.clone()
            same = torch.equal(outs[0].view(torch.int32 if epi == 1 else torch.int16), outs[2].view(torch.int32 if epi == 1 else torch.int16))
            print(f"gemv_wide M{M:2d} {name:12s}: default {t[0]:6.1f} us ({2 * N * K / t[0] / 1e3:6.0f} GB/s)  wide {t[2]:6.1f} us "
                  f"({2 * N * K / t[2] / 1e3:6.0f} GB/s)  same bits {same}", flush=True)
    lib.vck_set_gemv_wide(-1)


def bench_gemm_chunk():
    """go / no-go of the chunked-prefill idea: the decoder GEMMs at M = 288 / 320 / 384 rows (a prefill chunk plus
    the pool's 32 decode rows) with the weights streamed from HBM (4 rotating copies); the sum per layer against 150 us."""
    for M in (288, 320, 384, 512):
        tot = 0.0
        for (N, K, epi, name) in [(12288, 4096, 0, "qkv"), (4096, 4096, 4, "o"), (22016, 4096, 5, "gate-up"), (4096, 11008, 4, "down")]:
            A = bf16(M, K)
            Ws = [bf16(N, K, scale=0.02) for _ in range(4)]
            out = torch.zeros((M, N), dtype=torch.float32 if epi in (3, 4) else torch.bfloat16, device=dev)
            ldo = N // 2 if epi == 5 else N
            ws = torch.zeros(16 << 20, device=dev)
            it = [0]

            def f():
                it[0] += 1
                lib.vck_gemm_ws(P(A), P(Ws[it[0] % 4]), None, P(out), M, N, K, K, K, ldo, epi, P(ws), C.c_size_t(64 << 20), None)
            us = timeit(f, iters=20)
            tot += us
            print(f"gemm_chunk M{M} {name:8s}: {us:7.1f} us  {2 * M * N * K / us / 1e6:7.1f} TFLOP/s  weights {2 * N * K / us / 1e3:6.0f} GB/s", flush=True)
        print(f"gemm_chunk M{M} layer sum: {tot:7.1f} us (go if <= 150)", flush=True)


def bench_gemv_rows8():
    """W8A16 weights at 17..32 rows (the pool's rows under the fp8 weight formats): qkv and gate / up of the 7b and 13b models — the pair
    geometry (vck_set_gemv_wide(0)) against the one-workgroup-per-CU geometry (default since round 6 for > 512 tiles)"""
    for M in (12, 16, 24, 32):
        for (N, K, epi, name) in [(12288, 4096, 0, "7b qkv"), (22016, 4096, 3, "7b gate-up"), (15360, 5120, 0, "13b qkv"),
                                  (27648, 5120, 3, "13b gate-up")]:
            X = bf16(32, K)
            Ws = []
            sc = torch.zeros(N, device=dev)
            for _ in range(6):
                W = bf16(N, K, scale=0.02)
                Wq = torch.zeros(N * K, dtype=torch.uint8, device=dev)
                lib.vck_quantize_fp8(P(W), P(Wq), P(sc), N, K, None)
                Ws.append(Wq)
            torch.cuda.synchronize()
            out = torch.zeros((32, N), dtype=torch.bfloat16, device=dev)
            ldo = N // 2 if epi == 3 else N
            npart = (K // 16 + 15) // 16 * 16
            ssq = torch.rand(32, npart, device=dev)
            row = []
            for wide in (0, -1, 2):
                lib.vck_set_gemv_wide(wide)
                it = [0]

                def f():
                    it[0] += 1
                    lib.vck_gemv_ex(P(X), P(Ws[it[0] % 6]), P(sc), P(out), P(ssq), None, None, None, npart, C.c_float(1e-5),
                                    None, None, 0, M, N, K, ldo, epi, None)
                us = timeit(f, iters=60)
                row.append(f"{'pairs' if wide == 0 else 'default' if wide < 0 else 'wide everywhere'} {us:6.1f} us {N * K / us / 1e3:6.0f} GB/s")
            print(f"gemv_rows8 M{M:2d} {name:12s} N{N} K{K}: " + " | ".join(row), flush=True)
    lib.vck_set_gemv_wide(-1)


def bench_gemv_fp8_ks():
    """13b o_proj / down with W8A16 weights (320 tiles: the 257..512-tile class, tile pairs x KS_MID = 3 K-slices by default — a choice
    measured with bf16 weights): explicit K-slice counts at 8 / 16 / 32 rows"""
    for (N, K, name) in [(5120, 5120, "13b o"), (5120, 13824, "13b down")]:
        X = bf16(32, K)
        Ws = []
        sc = torch.zeros(N, device=dev)
        for _ in range(6):
            W = bf16(N, K, scale=0.02)
            Wq = torch.zeros(N * K, dtype=torch.uint8, device=dev)
            lib.vck_quantize_fp8(P(W), P(Wq), P(sc), N, K, None)
            Ws.append(Wq)
        torch.cuda.synchronize()
        out = torch.zeros((32, N), dtype=torch.float32, device=dev)
        npart = (max(K, N) // 16 + 15) // 16 * 16
        ssq_out = torch.zeros(32, npart, device=dev)
        gw = torch.rand(N, device=dev) + 0.5
        xg = torch.zeros((32, N), dtype=torch.bfloat16, device=dev)
        scratch = torch.zeros(8 * (N // 16) * 2 * 256, device=dev)
        counters = torch.zeros(N // 16 * 2, dtype=torch.int32, device=dev)
        for M in (8, 16, 32):
            row = []
            for ks in (0, 1, 2, 3, 4, 6):
                it = [0]

                def f():
                    it[0] += 1
                    lib.vck_gemv_ex(P(X), P(Ws[it[0] % 6]), P(sc), P(out), None, P(ssq_out), P(gw), P(xg), npart, C.c_float(1e-5),
                                    P(scratch), P(counters), ks, M, N, K, N, 2, None)
                us = timeit(f, iters=60)
                row.append(f"ks {'default' if ks == 0 else ks}: {us:5.1f} us")
            print(f"gemv_fp8_ks {name:8s} N{N} K{K} M{M:2d}: " + " | ".join(row), flush=True)


def bench_dattn_rows():
    """decode attention over B rows with per-row positions (the pool's form), ctx ~1280"""
    H, hd, S = 32, 128, 2048
    D = H * hd
    cos, sin = torch.rand(S, hd // 2, device=dev), torch.rand(S, hd // 2, device=dev)
    for B in (8, 16, 24, 32):
        qkv = bf16(B, 3 * D)
        ks = [bf16(B, H, S, hd) for _ in range(2)]
        vs = [bf16(B, H, S, hd) for _ in range(2)]
        out = torch.zeros((B, D), dtype=torch.bfloat16, device=dev)
        pos = torch.tensor([1216 + (7 * b) % 128 for b in range(B)], dtype=torch.int32, device=dev)
        act = torch.ones(B, dtype=torch.int32, device=dev)
        it = [0]

        def f():
            it[0] += 1
            lib.vck_attention_decode_rows(P(qkv), P(ks[it[0] % 2]), P(vs[it[0] % 2]), P(out), B, H, hd, S, P(pos), 1, P(act),
                                          P(cos), P(sin), C.c_float(1 / math.sqrt(hd)), None)
        us = timeit(f, iters=40)
        byts = 4.0 * float((pos + 1).sum().item()) * D
        print(f"decode attention rows B={B:2d} ctx~1280: {us:7.1f} us  {byts / us / 1e3:7.1f} GB/s", flush=True)


def bench_dattn_split():
    """decode attention of precision mode split: fp32 caches vs fp24 caches (3 bytes per element), rows as the pool spans them"""
    H, hd, S = 32, 128, 2048
    D = H * hd
    cos, sin = torch.rand(S, hd // 2, device=dev), torch.rand(S, hd // 2, device=dev)
    for B in (8, 16, 32):
        G = 8 if B <= 8 else (16 if B <= 16 else 32)
        qkv = torch.randn(B, 3 * D, device=dev)
        out = torch.zeros((2 * G, D), dtype=torch.bfloat16, device=dev)
        pos = torch.tensor([1216 + (7 * b) % 128 for b in range(B)], dtype=torch.int32, device=dev)
        act = torch.ones(B, dtype=torch.int32, device=dev)
        keys = float((pos + 1).sum().item())
        for name, es, fn in (("fp32", 4, lib.vck_attention_decode_kv32), ("fp24", 3, lib.vck_attention_decode_kv24)):
            ks = [torch.randint(0, 255, (B, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(2)]
            vs = [torch.randint(0, 255, (B, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(2)]
            for t in ks + vs:   # keep exponents sane: clear the top exponent bits of every element's high byte
                t.view(B, H, S, -1)[...] &= 0x3F
            it = [0]

            def f():
                it[0] += 1
                fn(P(qkv), P(ks[it[0] % 2]), P(vs[it[0] % 2]), P(out), B, H, hd, S, P(pos), 1, P(act), P(cos), P(sin),
                   C.c_float(1 / math.sqrt(hd)), G, None)
            us = timeit(f, iters=30)
            byts = 2.0 * keys * D * es
            print(f"decode attention split {name} B={B:2d} ctx~1280: {us:7.1f} us  {byts / us / 1e3:7.1f} GB/s", flush=True)


def bench_dattn_kv8():
    """decode attention of the bf16 step: bf16 caches vs the e4m3 caches of the fp8 weight format, 13b heads (40 x 128)"""
    H, hd, S = 40, 128, 2048
    D = H * hd
    cos, sin = torch.rand(S, hd // 2, device=dev), torch.rand(S, hd // 2, device=dev)
    for B in (8, 16, 32):
        qkv = bf16(B, 3 * D)
        out = torch.zeros((B, D), dtype=torch.bfloat16, device=dev)
        pos = torch.tensor([1216 + (7 * b) % 128 for b in range(B)], dtype=torch.int32, device=dev)
        act = torch.ones(B, dtype=torch.int32, device=dev)
        keys = float((pos + 1).sum().item())
        for name, es, fn in (("bf16", 2, lib.vck_attention_decode_rows), ("e4m3", 1, lib.vck_attention_decode_kv8)):
            ks = [torch.randint(0, 120, (B, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(2)]
            vs = [torch.randint(0, 120, (B, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(2)]
            it = [0]

            def f():
                it[0] += 1
                fn(P(qkv), P(ks[it[0] % 2]), P(vs[it[0] % 2]), P(out), B, H, hd, S, P(pos), 1, P(act), P(cos), P(sin),
                   C.c_float(1 / math.sqrt(hd)), None)
            us = timeit(f, iters=30)
            byts = 2.0 * keys * D * es
            print(f"decode attention 13b heads {name} B={B:2d} ctx~1280: {us:7.1f} us  {byts / us / 1e3:7.1f} GB/s", flush=True)


def bench_gemv_pair():
    """Two streams run the SAME GEMV (same weights, different activations / outputs) at the same time: does the second
    reader hit the Infinity Cache / merge with the first?  pair time ~ single time => yes."""
    M = 8
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for (N, K, epi, name) in [(12288, 4096, 0, "qkv"), (22016, 4096, 3, "gate-up"), (4096, 11008, 1, "down(f32)")]:
        X1, X2 = bf16(M, K), bf16(M, K)
        Ws = [bf16(N * K, scale=0.02) for _ in range(8)]
        dt = torch.float32 if epi in (1, 2) else torch.bfloat16
        o1 = torch.zeros((M, N), dtype=dt, device=dev)
        o2 = torch.zeros((M, N), dtype=dt, device=dev)
        ldo = N // 2 if epi == 3 else N
        it = [0]

        def single():
            it[0] += 1
            lib.vck_gemv(P(X1), P(Ws[it[0] % 8]), P(o1), M, N, K, ldo, epi, C.c_void_p(s1.cuda_stream))

        def pair_same():
            it[0] += 1
            w = Ws[it[0] % 8]
            lib.vck_gemv(P(X1), P(w), P(o1), M, N, K, ldo, epi, C.c_void_p(s1.cuda_stream))
            lib.vck_gemv(P(X2), P(w), P(o2), M, N, K, ldo, epi, C.c_void_p(s2.cuda_stream))

        def pair_diff():
            it[0] += 1
            lib.vck_gemv(P(X1), P(Ws[it[0] % 8]), P(o1), M, N, K, ldo, epi, C.c_void_p(s1.cuda_stream))
            lib.vck_gemv(P(X2), P(Ws[(it[0] + 4) % 8]), P(o2), M, N, K, ldo, epi, C.c_void_p(s2.cuda_stream))

        def wall(fn, iters=40):
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
            import time
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e6
        print(f"pair {name:10s}: single {wall(single):6.1f} us | two streams, same weights {wall(pair_same):6.1f} us | "
              f"two streams, different weights {wall(pair_diff):6.1f} us", flush=True)


def bench_gemv13():
    """VCoder-DS 13b decode shapes at M = 16 and M = 8 (config C3 runs M = 16)."""
    for M in (16, 8):
        for (N, K, epi, name) in [(15360, 5120, 0, "qkv"), (5120, 5120, 2, "o"), (27648, 5120, 3, "gate-up"),
                                  (5120, 13824, 2, "down"), (32000, 5120, 1, "lm_head")]:
            X = bf16(M, K)
            Ws = [bf16(N * K, scale=0.02) for _ in range(4)]
            out = torch.zeros((M, N), dtype=torch.float32 if epi in (1, 2) else torch.bfloat16, device=dev)
            ldo = N // 2 if epi == 3 else N
            it = [0]

            def f():
                it[0] += 1
                lib.vck_gemv(P(X), P(Ws[it[0] % 4]), P(out), M, N, K, ldo, epi, None)
            us = timeit(f, iters=40)
            print(f"gemv13 M{M} {name:8s} N{N} K{K} epi{epi}: {us:7.1f} us  {2 * N * K / us / 1e3:7.1f} GB/s", flush=True)
            if epi == 2:
                scratch = torch.zeros(4 * (N // 16) * 2 * 256, device=dev)
                counters = torch.zeros(N // 16 * 2, dtype=torch.int32, device=dev)
                for ks in (2, 3, 4):
                    def h():
                        it[0] += 1
                        lib.vck_gemv_ex(P(X), P(Ws[it[0] % 4]), None, P(out), None, None, None, None, 16, C.c_float(1e-5),
                                        P(scratch), P(counters), ks, M, N, K, ldo, epi, None)
                    us = timeit(h, iters=40)
                    print(f"gemv13 M{M} {name:8s} split-K {ks}: {us:7.1f} us  {2 * N * K / us / 1e3:7.1f} GB/s", flush=True)


def bench_gemv_fp8():
    """W8A16 form: same shapes, e4m3 bytes (random bytes: the kernel's speed does not depend on the values)."""
    for M in (8, 16):
        for (N, K, epi, name) in [(12288, 4096, 0, "qkv"), (4096, 4096, 2, "o"), (22016, 4096, 3, "gate-up"),
                                  (4096, 11008, 2, "down")]:
            X = bf16(M, K)
            Ws = [torch.randint(0, 120, (N * K,), dtype=torch.uint8, device=dev) for _ in range(8)]
            sc = torch.ones(N, device=dev)
            out = torch.zeros((M, N), dtype=torch.float32 if epi in (1, 2) else torch.bfloat16, device=dev)
            ldo = N // 2 if epi == 3 else N
            it = [0]
            xf = torch.randn(16, K, device=dev)
            w = torch.rand(K, device=dev) + 0.5
            npart = (K // 16 + 15) // 16 * 16
            ssq = torch.rand(16, npart, device=dev)
            norm = epi in (0, 1, 3)

            def f():
                it[0] += 1
                lib.vck_gemv_ex(P(X), P(Ws[it[0] % 8]), P(sc), P(out), P(ssq) if norm else None, None, None, None, npart,
                                C.c_float(1e-5), None, None, 0, M, N, K, ldo, epi, None)
            us = timeit(f, iters=40)
            print(f"gemv_fp8 M{M} {name:8s} N{N} K{K} epi{epi} norm{int(norm)}: {us:7.1f} us  {N * K / us / 1e3:7.1f} GB/s",
                  flush=True)


def bench_gemv_formats(formats=("bf16", "w8", "w4")):
    """The decoder linears of the 7b and 13b models at 1 / 8 / 16 / 32 rows in the three weight formats of the decode GEMV: bf16,
    W8A16 (e4m3 bytes + row scales) and W4A16 (MXFP4 nibbles + block scale bytes): us per launch and the achieved fraction of the
    8 TB/s HBM peak over the weight bytes of the format.  Random bytes (speed does not depend on the values); enough copies of a
    matrix are rotated that a launch never finds its weights in the 256 MiB last-level cache.  KBENCH_W4_NT = 1 / 2 / 4 forces the
    W4A16 tile geometry (A/B)."""
    if os.environ.get("KBENCH_W4_NT"):
        lib.vck_set_gemv_w4_nt(int(os.environ["KBENCH_W4_NT"]))
    shapes = [("7b", 12288, 4096, 0, "qkv"), ("7b", 4096, 4096, 2, "o"), ("7b", 22016, 4096, 3, "gate-up"), ("7b", 4096, 11008, 2, "down"),
              ("13b", 15360, 5120, 0, "qkv"), ("13b", 5120, 5120, 2, "o"), ("13b", 27648, 5120, 3, "gate-up"), ("13b", 5120, 13824, 2, "down")]
    bpw = {"bf16": 2.0, "w8": 1.0, "w4": 0.5 + 1.0 / 32.0}
    for (model, N, K, epi, name) in shapes:
        npart = (K // 16 + 15) // 16 * 16
        ssq = torch.rand(32, npart, device=dev)
        norm = epi in (0, 3)
        sc8 = torch.ones(N, device=dev)
        sc4 = torch.full((N * K // 32,), 127, dtype=torch.uint8, device=dev)
        for fmt in formats:
            nbytes = int(N * K * bpw[fmt])
            copies = max(4, min(64, (1 << 30) // nbytes))
            Ws = [torch.randint(0, 120, (N * K * (2 if fmt == "bf16" else 1) // (2 if fmt == "w4" else 1),), dtype=torch.uint8, device=dev)
                  for _ in range(copies)]
            row = []
            for M in (1, 8, 16, 32):
                X = bf16(M, K)
                out = torch.zeros((M, N), dtype=torch.float32 if epi in (1, 2) else torch.bfloat16, device=dev)
                ldo = N // 2 if epi == 3 else N
                it = [0]

                def f():
                    it[0] += 1
                    W = Ws[it[0] % copies]
                    common = (P(out), P(ssq) if norm else None, None, None, None, npart, C.c_float(1e-5), None, None, 0, M, N, K, ldo, epi, None)
                    if fmt == "w4":
                        lib.vck_gemv_w4(P(X), P(W), P(sc4), *common)
                    else:
                        lib.vck_gemv_ex(P(X), P(W), P(sc8) if fmt == "w8" else None, *common)
                us = timeit(f, iters=3 * copies if copies < 14 else 40)
                row.append(f"M{M:2d} {us:6.1f} us {nbytes / us / 1e6 / 8.0 * 100:5.1f}%")
            print(f"gemv_formats {model:3s} {name:8s} N{N} K{K} {fmt:4s} ({nbytes / 2 ** 20:6.1f} MiB): " + " | ".join(row), flush=True)


def bench_extend_linears():
    """vc_extend's routing question: one 7b decoder layer's linears (qkv, o, gate-up, down) over M token rows as
    ceil(M / 32) passes of the weight-streaming decode GEMV (folded-RMSNorm operands, as decode_linears runs them) against
    one prefill GEMM per matrix (with the split-K workspace, as the engine calls it)."""
    shapes = [(12288, 4096, 0, 0, "qkv"), (4096, 4096, 2, 4, "o"), (22016, 4096, 3, 5, "gate-up"), (4096, 11008, 2, 4, "down")]
    npart = (4096 // 16 + 15) // 16 * 16
    ws = torch.zeros(16 << 20, device=dev)
    Ws = {N * K: [bf16(N * K, scale=0.02) for _ in range(4)] for (N, K, _, _, _) in shapes}
    for M in (32, 48, 64, 96, 128, 160, 192, 256):
        t_gemv = t_gemm = 0.0
        for (N, K, epi_v, epi_g, name) in shapes:
            W = Ws[N * K]
            X = bf16(M, K)
            outv = torch.zeros((M, N), dtype=torch.float32 if epi_v == 2 else torch.bfloat16, device=dev)
            ldo = N // 2 if epi_v == 3 else N
            ssq = torch.rand(M, npart, device=dev)
            gw = torch.rand(N, device=dev) + 0.5
            xg = torch.zeros((M, N), dtype=torch.bfloat16, device=dev)
            scratch = torch.zeros(8 * (N // 16 + 1) * 2 * 256, device=dev)
            counters = torch.zeros((N // 16 + 1) * 2, dtype=torch.int32, device=dev)
            it = [0]

            def passes():
                it[0] += 1
                w = W[it[0] % 4]
                for m0 in range(0, M, 32):
                    mr = min(32, M - m0)
                    if epi_v == 2:
                        lib.vck_gemv_ex(P(X[m0:]), P(w), None, P(outv[m0:]), None, P(ssq[m0:]), P(gw), P(xg[m0:]), npart,
                                        C.c_float(1e-5), P(scratch), P(counters), 0, mr, N, K, ldo, epi_v, None)
                    else:
                        lib.vck_gemv_ex(P(X[m0:]), P(w), None, P(outv[m0:]), P(ssq[m0:]), None, None, None, npart, C.c_float(1e-5),
                                        None, None, 0, mr, N, K, ldo, epi_v, None)
            uv = timeit(passes, iters=20)
            outg = torch.zeros((M, N), dtype=torch.float32 if epi_g == 4 else torch.bfloat16, device=dev)
            ldg = N // 2 if epi_g == 5 else N

            def gemm():
                it[0] += 1
                lib.vck_gemm_ws(P(X), P(W[it[0] % 4]), None, P(outg), M, N, K, K, K, ldg, epi_g, P(ws), C.c_size_t(64 << 20), None)
            ug = timeit(gemm, iters=20)
            t_gemv += uv
            t_gemm += ug
            print(f"extend_linears M{M:3d} {name:8s}: GEMV x{(M + 31) // 32} {uv:7.1f} us | GEMM {ug:7.1f} us", flush=True)
        print(f"extend_linears M{M:3d} layer: GEMV passes {t_gemv:7.1f} us | GEMM {t_gemm:7.1f} us -> "
              f"{'GEMV' if t_gemv < t_gemm else 'GEMM'}", flush=True)


def bench_extend_attn():
    """attention_extend_kernel at 7b (32 heads, hd 128) over a VCoder-DS prompt (P = 1216): time and the K / V bytes it must
    read (every cached key once per (b, h): 2 (P + n) hd bytes-per-element) over the 8 TB/s HBM peak"""
    H, hd, Pp = 32, 128, 1216
    for kv8 in (0, 1):
        es = 1 if kv8 else 2
        for B in (1, 8):
            for n in (1, 8, 32, 64, 128, 512):
                S = (Pp + n + 63) // 64 * 64
                q = bf16(B, H, n, hd)
                k = torch.randint(0, 120, (B, H, S, hd * es), dtype=torch.uint8, device=dev) if kv8 else bf16(B, H, S, hd)
                v = torch.randint(0, 120, (B, H, S, hd * es), dtype=torch.uint8, device=dev) if kv8 else bf16(B, H, S, hd)
                out = torch.zeros((B * n, H * hd), dtype=torch.bfloat16, device=dev)
                us = timeit(lambda: lib.vck_attention_extend(P(q), P(k), P(v), P(out), B, H, n, Pp, hd, n, S, kv8,
                                                             C.c_float(1 / math.sqrt(hd)), None, 0, None), iters=20)
                byts = 2.0 * B * H * (Pp + n) * hd * es
                print(f"extend_attn kv8={kv8} B{B} n{n:3d} P{Pp}: {us:8.1f} us  {byts / us / 1e3:7.1f} GB/s = "
                      f"{byts / us / 1e3 / 8000:.2f} of 8 TB/s", flush=True)


def bench_token_logprob():
    """token_logprob_kernel over [rows, 32000] fp32 logits: time and the fraction of the 8 TB/s HBM peak its one pass over the rows is;
    beside it the greedy row scan of select_embed_kernel (argmax, one workgroup of 1024 threads per row) over the same buffer"""
    V = 32000
    stride = int(lib.vck_row_state_stride())
    for rows in (128, 1024):
        lg = [torch.randn(rows, V, device=dev) * 3 for _ in range(4)]   # 4 x 131 MB at 1024 rows: past the 256 MB MALL in rotation
        tgt = torch.randint(0, V, (rows,), dtype=torch.int32, device=dev)
        out = torch.zeros(rows, device=dev)
        it = [0]

        def f():
            it[0] += 1
            lib.vck_token_logprob(P(lg[it[0] % 4]), V, P(tgt), P(out), rows, V, None)
        us = timeit(f, iters=40)
        gbs = rows * V * 4 / us / 1e3
        print(f"token_logprob rows {rows:4d} V {V}: {us:7.1f} us  {gbs:7.1f} GB/s = {gbs / 8000:.2f} of 8 TB/s", flush=True)
        rs = torch.zeros((rows, stride), dtype=torch.int32, device=dev)
        rs[:, 0] = 1    # RS_ACTIVE
        rs[:, 5] = -1   # RS_EOS: none
        rs[:, 14] = torch.arange(rows, dtype=torch.int32, device=dev)   # RS_OUT_OFF
        nxt = torch.zeros(rows, dtype=torch.int32, device=dev)
        ids = torch.zeros(rows, dtype=torch.int32, device=dev)

        def g():
            it[0] += 1
            lib.vck_select_embed(P(lg[it[0] % 4]), V, P(rs), P(nxt), P(ids), None, None, None, None, None, 4096, 16, V, rows, 0, None)
        us = timeit(g, iters=40)
        gbs = rows * V * 4 / us / 1e3
        print(f"argmax scan   rows {rows:4d} V {V}: {us:7.1f} us  {gbs:7.1f} GB/s = {gbs / 8000:.2f} of 8 TB/s", flush=True)


def bench_topk_logprob():
    """topk_logprob_kernel over [rows, 32000] fp32 logits at K = 0 / 5 / 32 (rows 8 / 32: a decode step's launch; 1024: a score chunk), beside
    token_logprob_kernel, the greedy row scan of select_embed_kernel and its sampled path at top_k = 50 (the same 32-pass bisection
    over the row in LDS) over the same buffers"""
    V = 32000
    stride = int(lib.vck_row_state_stride())
    for rows in (8, 32, 1024):
        lg = [torch.randn(rows, V, device=dev) * 3 for _ in range(4)]
        tgt = torch.randint(0, V, (rows,), dtype=torch.int32, device=dev)
        out = torch.zeros(rows, device=dev)
        tlp = torch.zeros((rows, 32), device=dev)
        tid = torch.zeros((rows, 32), dtype=torch.int32, device=dev)
        it = [0]
        for K in (0, 5, 32):
            for lds in (-1, 0):
                if K == 0 and lds == 0:
                    continue

                def f():
                    it[0] += 1
                    lib.vck_topk_logprob(P(lg[it[0] % 4]), V, P(tgt), P(out), P(tlp), P(tid), rows, V, K, lds, None)
                us = timeit(f, iters=40)
                print(f"topk_logprob  rows {rows:4d} V {V} K {K:2d} {'staged  ' if lds else 'unstaged'}: {us:7.1f} us", flush=True)

        def tl():
            it[0] += 1
            lib.vck_token_logprob(P(lg[it[0] % 4]), V, P(tgt), P(out), rows, V, None)
        print(f"token_logprob rows {rows:4d} V {V}: {timeit(tl, iters=40):7.1f} us", flush=True)
        for sample in (0, 1):
            rs = torch.zeros((rows, stride), dtype=torch.int32, device=dev)
            rs[:, 0] = 1    # RS_ACTIVE
            rs[:, 5] = -1   # RS_EOS: none
            rs[:, 8] = sample
            rs[:, 9] = 0x3F800000   # RS_INVTEMP: 1.0
            rs[:, 10] = 50          # RS_TOPK
            rs[:, 11] = 0x3F800000  # RS_TOPP: 1.0 (off)
            rs[:, 14] = torch.arange(rows, dtype=torch.int32, device=dev)   # RS_OUT_OFF
            nxt = torch.zeros(rows, dtype=torch.int32, device=dev)
            ids = torch.zeros(rows, dtype=torch.int32, device=dev)

            def g():
                it[0] += 1
                lib.vck_select_embed(P(lg[it[0] % 4]), V, P(rs), P(nxt), P(ids), None, None, None, None, None, 4096, 16, V, rows, 0, None)
            print(f"{'select top_k=50' if sample else 'argmax scan    '} rows {rows:4d} V {V}: {timeit(g, iters=40):7.1f} us", flush=True)


def bench_logits_process():
    """logits_process_kernel over [rows, 32000] fp32 logits (rows 1 / 8 / 16: a decode step's launch): everything off (the copy), and all
    processors on over a history of 1216 prompt ids + 64 / 127 generated ids (repetition penalty 1.3, n-gram 3, 2 bad words, min_new)"""
    V, T = 32000, 1216
    stride = int(lib.vck_row_state_stride())
    f32 = lambda x: int(torch.tensor(x, dtype=torch.float32).view(torch.int32))
    tab = torch.zeros((32, 9), dtype=torch.int32, device=dev)
    tab[0, :2] = torch.tensor([1, 7])
    tab[1, :3] = torch.tensor([2, 5, 9])
    for rows in (1, 8, 16):
        lg = [torch.randn(rows, V, device=dev) * 3 for _ in range(4)]
        out = torch.empty(rows, V, device=dev)
        prompt = torch.randint(0, V, (rows, T), dtype=torch.int32, device=dev)
        gen = torch.randint(0, V, (rows, 128), dtype=torch.int32, device=dev)
        it = [0]
        for on, step in ((0, 0), (1, 64), (1, 127)):
            rs = torch.zeros((rows, stride), dtype=torch.int32, device=dev)
            rs[:, 0] = 1                  # RS_ACTIVE
            rs[:, 2] = step               # RS_STEP
            rs[:, 4] = 128                # RS_MAXNEW
            rs[:, 5] = 2                  # RS_EOS
            rs[:, 14] = torch.arange(rows, dtype=torch.int32, device=dev) * 128   # RS_OUT_OFF
            if on:
                rs[:, 15] = f32(1.3)      # RS_LP_PENALTY
                rs[:, 96] = 3             # RS_LP_NGRAM
                rs[:, 97] = 128           # RS_LP_MINNEW
                rs[:, 98] = torch.arange(rows, dtype=torch.int32, device=dev) * T     # RS_LP_HIST_OFF
                rs[:, 99] = T             # RS_LP_HIST_LEN
                rs[:, 100] = 2            # RS_LP_NBAD

            def f():
                it[0] += 1
                lib.vck_logits_process(P(lg[it[0] % 4]), V, P(out), V, P(rs), P(prompt), P(gen), P(tab), rows, V, None)
            us = timeit(f, iters=40)
            print(f"logits_process rows {rows:3d} V {V} {'all on, step %3d' % step if on else 'all off (copy) '}: {us:7.1f} us", flush=True)


def bench_guidance_combine():
    """guidance_combine_kernel over B pairs of [32000] fp32 rows laid out as a guided step's lm_head leaves them (2 B rows, the
    unconditional ones behind the conditional ones), B = 1 / 8"""
    V = 32000
    stride = int(lib.vck_row_state_stride())
    f32 = lambda x: int(torch.tensor(x, dtype=torch.float32).view(torch.int32))
    for B in (1, 8):
        lg = [torch.randn(2 * B, V, device=dev) * 3 for _ in range(4)]
        out = torch.empty(B, V, device=dev)
        sc = torch.empty(B, 4, device=dev)
        rs = torch.zeros((B, stride), dtype=torch.int32, device=dev)
        rs[:, 0] = 1                  # RS_ACTIVE
        rs[:, 113] = f32(1.5)         # RS_GD_SCALE
        it = [0]
        def f():
            it[0] += 1
            x = lg[it[0] % 4]
            lib.vck_guidance_combine(P(x), P(x[B:]), V, P(out), V, P(rs), P(sc), B, V, None)
        print(f"guidance_combine pairs {B} V {V}: {timeit(f, iters=40):7.1f} us", flush=True)


def bench_guidance_follow():
    """guidance_follow_kernel at 7b dims (D 4096, 256 sum-of-squares partials): B = 1 / 8 followers"""
    D, npart = 4096, 256
    stride = int(lib.vck_row_state_stride())
    for B in (1, 8):
        rs = torch.zeros((2 * B, stride), dtype=torch.int32, device=dev)
        rs[:, 0] = 1
        tok = torch.zeros(2 * B, dtype=torch.int32, device=dev)
        x = torch.randn(2 * B, D, device=dev)
        ssq = torch.rand(2 * B, npart, device=dev)
        xg = torch.zeros(2 * B, D, dtype=torch.int16, device=dev)

        def f():
            lib.vck_guidance_follow(P(rs), P(tok), P(x), P(ssq), P(xg), B, D, npart, 0, None)
        print(f"guidance_follow followers {B} D {D}: {timeit(f, iters=40):7.1f} us", flush=True)


def bench_logits_process_constrained():
    """logits_process_kernel with a token automaton (phase 4) over [rows, 32000] fp32 logits, the other processors off: the launch
    without tables (the copy), a free-text state, and states of 1 / 133 / 4096 / 32000 edges (ids spread evenly over the vocabulary);
    the stored state is current (one launch of a decode step: nothing to walk)"""
    V = 32000
    stride = int(lib.vck_row_state_stride())
    counts = (1, 133, 4096, 32000)
    off, tok, dflt = [0], [], []
    for n in counts:
        tok += sorted({int(t) for t in torch.linspace(0, V - 1, n, dtype=torch.float64).round().tolist()}) if n > 1 else [V // 2]
        off.append(len(tok))
        dflt.append(-1)
    off.append(len(tok))          # the free-text state: no edges, default_next = itself
    dflt.append(len(counts))
    t_off, t_tok, t_dflt = (torch.tensor(a, dtype=torch.int32, device=dev) for a in (off, tok, dflt))
    t_next = torch.zeros(len(tok), dtype=torch.int32, device=dev)
    gen = torch.zeros(16 * 128, dtype=torch.int32, device=dev)
    for rows in (1, 8, 16):
        lg = [torch.randn(rows, V, device=dev) * 3 for _ in range(4)]
        out = torch.empty(rows, V, device=dev)
        it = [0]
        for name, state in [("no tables (copy)", None), ("free-text state", len(counts))] + [(f"{n:5d} edges", i) for i, n in enumerate(counts)]:
            rs = torch.zeros((rows, stride), dtype=torch.int32, device=dev)
            rs[:, 0] = 1                  # RS_ACTIVE
            rs[:, 2] = 64                 # RS_STEP
            rs[:, 4] = 128                # RS_MAXNEW
            rs[:, 5] = -1                 # RS_EOS
            rs[:, 14] = torch.arange(rows, dtype=torch.int32, device=dev) * 128   # RS_OUT_OFF
            if state is not None:
                rs[:, 110] = 1            # RS_CN_ON
                rs[:, 111] = state        # RS_CN_STATE
                rs[:, 112] = 64           # RS_CN_POS = RS_STEP
            tabs = (P(t_off), P(t_tok), P(t_next), P(t_dflt), len(dflt)) if state is not None else (None, None, None, None, 0)

            def f():
                it[0] += 1
                lib.vck_logits_process_constrained(P(lg[it[0] % 4]), V, P(out), V, P(rs), None, P(gen), None, *tabs, rows, V, None)
            print(f"logits_process_constrained rows {rows:3d} V {V} {name:17s}: {timeit(f, iters=40):7.1f} us", flush=True)


def bench_score_head():
    """The score path's chunk at 7b dims (D 4096, V 32000): gathered final RMSNorm + lm_head + token_logprob over M scored rows (16 .. 1024), the
    lm_head as ceil(M / 32) passes of the weight-streaming GEMV (packed weights) against one GEMM — the crossover behind
    SCORE_GEMV_ROWS (engine_llm.inc) at the lm_head's shape."""
    D, V = 4096, 32000
    x = torch.randn(8 * 1216, D, device=dev)
    gw = torch.rand(D, device=dev) + 0.5
    Ws = [bf16(V, D, scale=0.02) for _ in range(2)]
    Wp = [torch.zeros_like(w) for w in Ws]
    for w, wp in zip(Ws, Wp):
        lib.vck_pack_weight(P(w), P(wp), V, D, None)
    ws = torch.zeros(16 << 20, device=dev)
    for M in (16, 32, 64, 128, 160, 1024):
        idx = torch.randperm(8 * 1216, device=dev)[:M].to(torch.int32)
        tgt = torch.randint(0, V, (M,), dtype=torch.int32, device=dev)
        xn = torch.zeros((M + 32, D), dtype=torch.bfloat16, device=dev)
        lg = torch.zeros((M + 32, V), device=dev)
        out = torch.zeros(M, device=dev)
        it = [0]

        def run(gemv):
            it[0] += 1
            lib.vck_rmsnorm(P(x), P(idx), P(gw), P(xn), M, D, C.c_float(1e-5), None)
            if gemv:
                for m0 in range(0, M, 32):
                    lib.vck_gemv_ex(P(xn[m0:]), P(Wp[it[0] % 2]), None, P(lg[m0:]), None, None, None, None, 16, C.c_float(1e-5),
                                    None, None, 0, min(32, M - m0), V, D, V, 1, None)
            else:
                lib.vck_gemm_ws(P(xn), P(Ws[it[0] % 2]), None, P(lg), M, V, D, D, D, V, 3, P(ws), C.c_size_t(64 << 20), None)
            lib.vck_token_logprob(P(lg), V, P(tgt), P(out), M, V, None)
        uv = timeit(lambda: run(True), iters=20)
        ug = timeit(lambda: run(False), iters=20)
        print(f"score_head M{M:5d}: norm + GEMV x{(M + 31) // 32:2d} + logprob {uv:8.1f} us | norm + GEMM + logprob {ug:8.1f} us -> "
              f"{'GEMV' if uv < ug else 'GEMM'}", flush=True)


def bench_attn():
    for (B, H, T, hd, causal, name) in [(8, 32, 1216, 128, 1, "llm prefill"), (24, 16, 577, 64, 0, "vit")]:
        Ts = (T + 63) // 64 * 64
        q, k, vt = bf16(B, H, Ts, hd), bf16(B, H, Ts, hd), bf16(B, H, hd, Ts)
        out = torch.zeros((B * T, H * hd), dtype=torch.bfloat16, device=dev)
        us = timeit(lambda: lib.vck_attention(P(q), P(k), P(vt), P(out), B, H, T, hd, Ts, Ts, causal,
                                              C.c_float(1 / math.sqrt(hd)), None), iters=10)
        fl = 4.0 * B * H * T * T * hd * (0.5 if causal else 1.0)
        print(f"attention {name:12s}: {us:8.1f} us  {fl / us / 1e6:7.1f} TFLOP/s", flush=True)


def bench_dattn():
    B, H, hd, pos = 8, 32, 128, 1280
    S = 1344
    D = H * hd
    qkv = bf16(B, 3 * D)
    ks = [bf16(B, H, S, hd) for _ in range(4)]
    vs = [bf16(B, H, S, hd) for _ in range(4)]
    out = torch.zeros((B, D), dtype=torch.bfloat16, device=dev)
    posd = torch.tensor([pos], dtype=torch.int32, device=dev)
    cos, sin = torch.rand(S, hd // 2, device=dev), torch.rand(S, hd // 2, device=dev)
    it = [0]

    def f():
        it[0] += 1
        lib.vck_attention_decode_fused(P(qkv), P(ks[it[0] % 4]), P(vs[it[0] % 4]), P(out), B, H, hd, S, P(posd), P(cos),
                                       P(sin), C.c_float(1 / math.sqrt(hd)), None)
    us = timeit(f, iters=40)
    print(f"decode attention ctx={pos + 1}: {us:7.1f} us  {4.0 * B * (pos + 1) * D / us / 1e3:7.1f} GB/s", flush=True)


def bench_attention_verify():
    """attention_verify_kernel (Q query rows per sequence, one read of the K / V streams) beside the fused decode attention it
    replaces Q launches of: 7b heads, a context of 1216 keys, bf16 and e4m3 caches; B = 1 at Q = 2 / 4 / 8 and B = 4 at Q = 8"""
    H, hd, pos, S = 32, 128, 1216, 1408
    D = H * hd
    cos, sin = torch.rand(S, hd // 2, device=dev), torch.rand(S, hd // 2, device=dev)
    scale = C.c_float(1 / math.sqrt(hd))
    for kv8 in (0, 1):
        for B, Q in ((1, 2), (1, 4), (1, 8), (4, 8)):
            es = 1 if kv8 else 2
            ks = [torch.randint(0, 120, (B, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(4)]
            vs = [torch.randint(0, 120, (B, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(4)]
            qkv, qkv1 = bf16(B * Q, 3 * D), bf16(B, 3 * D)
            out, out1 = torch.zeros((B * Q, D), dtype=torch.bfloat16, device=dev), torch.zeros((B, D), dtype=torch.bfloat16, device=dev)
            rec = torch.tensor([[1, pos]] * B, dtype=torch.int32, device=dev)
            nq = torch.full((B,), Q, dtype=torch.int32, device=dev)
            it = [0]

            def verify():
                it[0] += 1
                lib.vck_attention_verify(P(qkv), P(ks[it[0] % 4]), P(vs[it[0] % 4]), P(out), B, H, hd, S, Q, C.c_void_p(rec.data_ptr() + 4), 2,
                                         P(nq), P(cos), P(sin), scale, 3 if kv8 else 0, None, 0, None)

            def plain():
                it[0] += 1
                lib.vck_attention_decode_masked(P(qkv1), P(ks[it[0] % 4]), P(vs[it[0] % 4]), P(out1), B, H, hd, S, C.c_void_p(rec.data_ptr() + 4),
                                                2, C.c_void_p(rec.data_ptr()), P(cos), P(sin), scale, 3 if kv8 else 0, 0, None, 0, None)
            uv, up = timeit(verify, iters=40), timeit(plain, iters=40)
            print(f"attention_verify {'e4m3' if kv8 else 'bf16'} B {B} Q {Q} ctx {pos + Q}: {uv:7.1f} us | decode attention B {B} ctx {pos + 1}: "
                  f"{up:7.1f} us  (x{uv / up:4.2f}; {Q} plain launches {Q * up:7.1f} us)", flush=True)


def bench_attention_fanout():
    """attention_fanout_kernel (n rows per prompt; the prompt's keys and values read once per group and head) beside the fused decode
    attention over the same n B rows: 7b heads, a prompt of 1216 keys and 64 tail keys, bf16 and e4m3 caches; B = 1 at n = 2 / 4 / 8
    and B = 2 at n = 8"""
    H, hd, Pn, pos, S = 32, 128, 1216, 1216 + 64, 1408
    D = H * hd
    cos, sin = torch.rand(S, hd // 2, device=dev), torch.rand(S, hd // 2, device=dev)
    scale = C.c_float(1 / math.sqrt(hd))
    for kv8 in (0, 1):
        for B, n in ((1, 2), (1, 4), (1, 8), (2, 8)):
            es, R = 1 if kv8 else 2, B * n
            ks = [torch.randint(0, 120, (R, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(4)]
            vs = [torch.randint(0, 120, (R, H, S, hd * es), dtype=torch.uint8, device=dev) for _ in range(4)]
            qkv = bf16(R, 3 * D)
            out = torch.zeros((R, D), dtype=torch.bfloat16, device=dev)
            rec = torch.tensor([[1, pos]] * R, dtype=torch.int32, device=dev)
            plen = torch.full((B,), Pn, dtype=torch.int32, device=dev)
            it = [0]

            def fanout():
                it[0] += 1
                lib.vck_attention_fanout(P(qkv), P(ks[it[0] % 4]), P(vs[it[0] % 4]), P(out), B, H, hd, S, n, R, C.c_void_p(rec.data_ptr() + 4), 2,
                                         P(plen), None, P(cos), P(sin), scale, 3 if kv8 else 0, None)

            def plain():
                it[0] += 1
                lib.vck_attention_decode_masked(P(qkv), P(ks[it[0] % 4]), P(vs[it[0] % 4]), P(out), R, H, hd, S, C.c_void_p(rec.data_ptr() + 4),
                                                2, C.c_void_p(rec.data_ptr()), P(cos), P(sin), scale, 3 if kv8 else 0, 0, None, 0, None)
            uf, up = timeit(fanout, iters=40), timeit(plain, iters=40)
            print(f"attention_fanout {'e4m3' if kv8 else 'bf16'} B {B} n {n} prompt {Pn} ctx {pos + 1}: {uf:7.1f} us | decode attention over {R} rows: "
                  f"{up:7.1f} us  (x{uf / up:4.2f})", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["gemm", "gemv", "attn", "dattn"]
    table = {"gemm_qkv": bench_gemm_qkv, "gemm": bench_gemm, "gemv": bench_gemv, "attn": bench_attn, "dattn": bench_dattn, "gemv_fp8": bench_gemv_fp8,
             "gemv13": bench_gemv13, "gemv_pair": bench_gemv_pair, "gemv_rows": bench_gemv_rows, "dattn_rows": bench_dattn_rows,
             "gemm_f8": bench_gemm_f8, "gemv_rows8": bench_gemv_rows8, "gemv_wide": bench_gemv_wide, "gemm_chunk": bench_gemm_chunk,
             "dattn_split": bench_dattn_split, "dattn_kv8": bench_dattn_kv8, "gemv_wg": bench_gemv_wg, "gemv_fp8_ks": bench_gemv_fp8_ks,
             "extend_linears": bench_extend_linears, "extend_attn": bench_extend_attn, "token_logprob": bench_token_logprob,
             "topk_logprob": bench_topk_logprob, "logits_process": bench_logits_process,
             "logits_process_constrained": bench_logits_process_constrained,
             "guidance_combine": bench_guidance_combine, "guidance_follow": bench_guidance_follow,
             "score_head": bench_score_head, "attention_verify": bench_attention_verify, "attention_fanout": bench_attention_fanout, "gemv_formats": bench_gemv_formats, "gemv_w4": lambda: bench_gemv_formats(("w4",))}
    for w in what:
        table[w]()
