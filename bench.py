#!/usr/bin/env python
"""bench.py — images/sec of the VCoder-DS LLaVA-1.5-7b hot path on MI355X (BASELINE.json metric).

One "step" = one full pass of the hot path over one batch per GPU:
    3x CLIP ViT-L/14@336 encode (RGB, seg, depth) + adapters + splice + Llama prefill (S=1216)
    + 128 greedy tokens (1 from the prefill + 127 hipGraph-replayed decode steps), EOS disabled.
Synthetic COST-shaped inputs, seeded synthetic weights (no network), bf16 MFMA compute, fp32 accumulate.
`value`: inputs resident in HBM when the timed region starts (the task contract).

A plain run does what `value` needs and no more: it builds the model, generates the batch once alone (the ids every timed step
must reproduce), warms up, times `--steps` steps, checks their ids, writes `--dump-outputs` / `--dump-ids`, and prints the line.
`--full` appends, outside the timed region and without changing it, everything else the benchmark measures: the PCIe-inclusive
rate (pixels handed over as host buffers) as `pcie_inclusive`, inter-token latency, one batch at a time, the
composite and per-kernel rooflines, the precision-mode / fp16-library / 13b legs, and the CPU baseline (minutes in all).

N > 1: one process per GPU, batch sharded data-parallel with no collective on the data path; the only exchange is
one all-gather of the generated token ids per step over RCCL/xGMI.  `python bench.py --gpus N` starts its own N
ranks (torch.distributed.run on 127.0.0.1); under an external torchrun (WORLD_SIZE set) it is one of the ranks.

Prints ONE JSON line (rank 0).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_PEAK_TFLOPS = 2500.0    # dense bf16
MFMA_FP8_PEAK_TFLOPS = 5000.0  # dense fp8 (K=128 scaled MFMA)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8, help="samples per GPU (BASELINE configs[1]: 8)")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--model", default="7b", choices=["7b", "13b"])
    ap.add_argument("--weights", default="bf16", choices=["bf16", "w8a16", "fp8"],
                    help="decoder weight storage: bf16 (BASELINE configs[1], the default metric); w8a16 = e4m3 bytes with "
                         "per-row power-of-two scales, bf16 activations; fp8 = the same weights with the prefill linears on the "
                         "K=128 scaled fp8 MFMA (W8A8) - BASELINE configs[4]")
    ap.add_argument("--inflight", type=int, default=4,
                    help="batches in flight per GPU: independent generate() calls (own stream + prefill workspaces, shared "
                         "weights) driven by host threads.  1 = strictly one batch at a time")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure and report everything beside the headline: the other residency of the "
                         "inputs, inter-token latency, one batch at a time, the composite and per-kernel rooflines (isolated replays), "
                         "the compact legs (see --no-extra-legs) and the CPU baseline.  `value`, `ms_per_step` and the dumped outputs "
                         "are those of the plain run")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: do not time the CPU baseline")
    ap.add_argument("--cpu-c1", action="store_true",
                    help="with --full: additionally run BASELINE configs[0] IN FULL on the host cores (VCoder 7b shape, B=1, RGB+seg, 32 "
                         "greedy tokens through oracle/cpu_ref.py; minutes) and report it as cpu_c1")
    ap.add_argument("--host-pixels", action="store_true",
                    help="make the PCIe-inclusive form the timed one (pixels handed over as pageable host fp32 buffers)")
    ap.add_argument("--gather", default="torch", choices=["torch", "cabi"],
                    help="all-gather of the token ids: torch.distributed (backend nccl = RCCL) or the library's own "
                         "vc_allgather_tokens (RCCL called through the C ABI)")
    ap.add_argument("--force-dist", action="store_true",
                    help="with --gpus 1: still initialise torch.distributed on the real backend (nccl = RCCL, world_size 1), run the "
                         "per-step id all-gather, the device barriers and the MAX all-reduce of the timing (and with --gather cabi "
                         "a one-rank RCCL communicator inside the library): the multi-GPU code path on a one-GPU box")
    ap.add_argument("--dump-ids", default=None, help="write the gathered ids of the last timed step to this .npy (tests)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path returned in its last timed step to DIR/<name>.npy as float32 (the new token ids "
                         "[n_gpus * batch, new_tokens] of every rank, gathered; exact in float32): inputs and weights are seeded, "
                         "so two builds can be compared output for output")
    ap.add_argument("--no-pool-hold", action="store_true",
                    help="pool policy A/B: step whatever rows are active even while another call is prefilling (vc_pool_set_hold(0))")
    ap.add_argument("--no-qkv-fused", action="store_true",
                    help="A/B: the prefill's QKV projection as the separate GEMM + split / RoPE launches of rounds 1-5 (vc_model_set_qkv_fused(0))")
    ap.add_argument("--gemv-variant", type=int, default=None,
                    help="A/B: vck_set_gemv_variant — 2 = four waves per workgroup in the split step's GEMV everywhere (rounds 4-5), default = the launcher's choice")
    ap.add_argument("--no-insitu", action="store_true",
                    help="do not stamp the pool's decode-step launches (the roofline of --full then reports the isolated replay); A/B of the stamps' cost")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="with --full: skip the compact legs a single-GPU run appends outside the timed region: parity_mode "
                         "(images/s of the precision modes that meet the 1e-3 / bit-exact-ids bar), BASELINE configs[2] "
                         "(13b bf16, batch 16) and the per-GPU slice of configs[4] (13b fp8, batch 16)")
    ap.add_argument("--extra-steps", type=int, default=2, help="with --full: steps of each compact leg")
    ap.add_argument("--pmc-traffic-bytes", type=float, default=None,
                    help="with --full: HBM bytes per launch of the dominant kernel from a separate rocprofv3 --pmc pass "
                         "(default: the committed FETCH_SIZE pass of this kernel under profiles/)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full and (args.cpu_c1 or args.pmc_traffic_bytes is not None):
        ap.error("--cpu-c1 and --pmc-traffic-bytes belong to the legs that only --full runs")
    return args


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks of this script on this node."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: required by RCCL on this host driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.call(cmd, env=env)


# ---- algorithmic work of one sample --------------------------------------------------------------
def work_per_sample(cfg, S, n_new, weight_bytes=2.0):
    D, F, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size
    Dv, Fv, Lv, P = cfg.mm_hidden_size, cfg.vit_intermediate_size, cfg.vit_layers_used, cfg.num_patches
    T = P + 1
    vit = 2 * P * 588 * Dv + Lv * (8 * T * Dv * Dv + 4 * T * T * Dv + 4 * T * Dv * Fv)
    adapter = 2 * P * (Dv * D + D * D)
    prefill = 2 * S * L * (4 * D * D + 3 * D * F) + 2 * S * S * D * L + 2 * D * V
    mfma_flops = 3 * (vit + adapter) + prefill
    dec_weight_bytes = weight_bytes * L * (4 * D * D + 3 * D * F) + 2 * D * V      # per decode step, shared by the rows in it
    kv_bytes_per_pos = 4 * L * D                                                   # K + V, bf16, per sample and position
    kv_bytes = sum(kv_bytes_per_pos * (S + t) for t in range(1, n_new))            # per sample over the decode steps
    return mfma_flops, dec_weight_bytes, kv_bytes


def cpu_baseline(cfg, n_new: int, decode_steps: int = 8):
    """The oracle (oracle/cpu_ref.py, torch fp32, kind='port') timed on the host cores at the TRUE 7b dimensions, B = 1:
    EVERY layer of the path — 3 x 23 ViT layers + adapters, all decoder layers of the S=1216 prefill, and `decode_steps`
    complete cached decode steps (all layers + lm_head) — the decode leg extrapolated linearly from `decode_steps` to
    n_new - 1 steps ("B=1 / N=8 and extrapolated").  Weights are constant fills (the arithmetic does not
    depend on the values; distinct memory per layer, so nothing is served from cache that the real model would miss)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import cpu_ref

    pool = torch.get_num_threads()
    cores = cpu_ref.fit_threads()      # the cgroup CPU quota, not the machine: an oversubscribed pool is throttled (r04_o)
    D, F, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    Dv, Fv = cfg.mm_hidden_size, cfg.vit_intermediate_size
    fill = lambda *s: torch.empty(*s).fill_(0.01)
    vp = "vision_model."
    sd = {vp + "embeddings.class_embedding": fill(Dv),
          vp + "embeddings.patch_embedding.weight": fill(Dv, 3, cfg.vit_patch_size, cfg.vit_patch_size),
          vp + "embeddings.position_embedding.weight": fill(cfg.num_patches + 1, Dv),
          vp + "pre_layrnorm.weight": torch.ones(Dv), vp + "pre_layrnorm.bias": torch.zeros(Dv)}
    for j in range(cfg.vit_layers_used):
        p = vp + f"encoder.layers.{j}."
        for ln in ("layer_norm1", "layer_norm2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = torch.ones(Dv), torch.zeros(Dv)
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{nm}.weight"], sd[p + f"self_attn.{nm}.bias"] = fill(Dv, Dv), fill(Dv)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = fill(Fv, Dv), fill(Fv)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = fill(Dv, Fv), fill(Dv)
    for pj in ("model.mm_projector", "model.seg_mm_projector"):
        sd[pj + ".0.weight"], sd[pj + ".0.bias"] = fill(D, Dv), fill(D)
        sd[pj + ".2.weight"], sd[pj + ".2.bias"] = fill(D, D), fill(D)
    for i in range(L):
        lp = f"model.layers.{i}."
        sd[lp + "input_layernorm.weight"] = torch.ones(D)
        sd[lp + "post_attention_layernorm.weight"] = torch.ones(D)
        for nm in ("q", "k", "v", "o"):
            sd[lp + f"self_attn.{nm}_proj.weight"] = fill(D, D)
        sd[lp + "mlp.gate_proj.weight"], sd[lp + "mlp.up_proj.weight"] = fill(F, D), fill(F, D)
        sd[lp + "mlp.down_proj.weight"] = fill(D, F)
    sd["model.norm.weight"], sd["lm_head.weight"], sd["model.embed_tokens.weight"] = torch.ones(D), fill(V, D), fill(V, D)
    S = 64 + 2 * cfg.num_patches
    px = torch.randn(3, 3, cfg.vit_image_size, cfg.vit_image_size)   # the three modalities of one sample
    with torch.no_grad():
        cpu_ref.vit_forward(px[:1], {k: v for k, v in sd.items()}, _one_vit_layer(cfg))   # thread-pool warm-up
        t0 = time.perf_counter()
        feats = cpu_ref.vit_forward(px, sd, cfg)
        for pj in ("model.mm_projector", "model.seg_mm_projector", "model.seg_mm_projector"):
            cpu_ref.projector_forward(feats[:1], sd, pj, "mlp2x_gelu")
        t_enc = time.perf_counter() - t0
        x = torch.randn(1, S, D) * 0.02
        cache = cpu_ref.KVCache(L)
        t0 = time.perf_counter()
        logits = cpu_ref.llama_forward(x, sd, cfg, cache, last_only=True)
        t_pre = time.perf_counter() - t0
        xd = torch.randn(1, 1, D) * 0.02
        step_t = []
        for _ in range(decode_steps):
            t0 = time.perf_counter()
            cpu_ref.llama_forward(xd, sd, cfg, cache, last_only=True)
            step_t.append(time.perf_counter() - t0)
        t_dec = sorted(step_t)[len(step_t) // 2]   # median: one step stalled by the host does not move the estimate
    per_sample = t_enc + t_pre + (n_new - 1) * t_dec
    torch.set_num_threads(pool)
    return {"value": 1.0 / per_sample, "unit": "images/s", "cores": cores, "kind": "port",
            "sample": (f"oracle/cpu_ref.py fp32 at true {cfg.hidden_size}-wide dims, B=1, every layer: 3 modalities x "
                       f"{cfg.vit_layers_used} ViT layers + adapters ({t_enc:.2f}s), {L}-layer prefill S={S} ({t_pre:.1f}s), "
                       f"{decode_steps} full cached decode steps (median {t_dec * 1e3:.0f}ms) extrapolated linearly to "
                       f"{n_new - 1} steps; {cores} torch threads = the CPUs this process may use "
                       f"(affinity and cgroup quota; the machine has {os.cpu_count()})")}


def _pmc_traffic_file():
    """the newest committed PMC FETCH_SIZE pass of the decode-step kernels (profiles/rNN_pmc_traffic.json; tools/profile_round.sh)"""
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))
    files = [f for f in files if "hbm_read_bytes_per_launch_by_rows" in open(f).read()]
    return files[-1] if files else None


def _one_vit_layer(cfg):
    class C1:
        pass
    c1 = C1()
    for k in ("vit_patch_size", "vit_image_size", "vit_num_heads", "vit_layer_norm_eps", "mm_vision_select_feature"):
        setattr(c1, k, getattr(cfg, k))
    c1.vit_layers_used = 1
    return c1


WEIGHTS_DESC = {"bf16": "bf16",
                "w8a16": "bf16 activations / fp8-e4m3 decoder weights (W8A16)",
                "fp8": "fp8-e4m3 decoder weights: W8A8 prefill on the K=128 scaled fp8 MFMA, W8A16 decode steps, e4m3 KV cache"}


def cpu_c1_full(new_tokens: int = 32):
    """BASELINE configs[0] in full on the host cores: VCoder (non-DS) LLaVA-1.5-7b shape, ONE 336x336 RGB+seg pair, prompt
    [1] + 34 text + [IMG, SEG] + 29 text (S = 1216), `new_tokens` greedy tokens through the oracle — the reference's CPU
    plumbing case.  Weights: the seeded synthetic checkpoint generated on the GPU and copied back."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import torch
    import cpu_ref
    from device_weights import device_state_dict
    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine

    cfg = vcfg.vicuna_7b("vcoder")
    eng = HipEngine(cfg)
    sd = device_state_dict(eng, cfg, 42)
    eng.close()
    ids = synth.synth_prompt_ids(cfg.vocab_size, "vcoder")[None]
    imgs, segs, _ = synth.synth_batch(1, cfg.vit_image_size)
    om = cpu_ref.OracleModel(cfg, sd)
    cpu_ref.fit_threads()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = om.generate_greedy(ids.tolist(), torch.from_numpy(imgs), torch.from_numpy(segs), None, max_new_tokens=new_tokens)
    dt = time.perf_counter() - t0
    return {"config": "VCoder LLaVA-1.5-7b, single 336x336 RGB+seg pair, greedy %d tokens, oracle fp32 on the host cores" % new_tokens,
            "seconds": dt, "images_per_s": 1.0 / dt, "cores": torch.get_num_threads(), "first_ids": out[0, :8].tolist()}


def run_leg(eng, cfg, ids, px, n_new, steps, inflight, check_against=None, precision=None):
    """`steps` complete hot-path passes over one batch (ids, px) with `inflight` generate() calls in flight (sessions forked
    from `eng`), one untimed warm-up pass per session first.  -> images/s, ms per step, the ids of the last step, and whether
    every step's ids equal `check_against` (default: the first warm-up pass, a batch generated alone)."""
    import threading

    import numpy as np
    import torch

    n_sess = max(1, min(inflight, steps))
    sessions = [eng] + [eng.fork() for _ in range(n_sess - 1)]
    if precision is not None:
        for s_ in sessions:
            s_.set_precision(precision)   # the arithmetic mode is a property of the session
    lone = eng.generate_greedy(ids, *px, max_new_tokens=n_new, eos_token_id=None)
    want = lone if check_against is None else check_against

    def sweep(k):
        outs, errs = [None] * k, []

        def worker(si):
            try:
                for j in range(si, k, n_sess):
                    outs[j] = sessions[si].generate_greedy(ids, *px, max_new_tokens=n_new, eos_token_id=None)
            except BaseException as e:
                errs.append(e)

        ths = [threading.Thread(target=worker, args=(si,)) for si in range(n_sess)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if errs:
            raise errs[0]
        return outs

    if n_sess > 1:
        sweep(n_sess)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = sweep(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if n_sess == 1 and steps == 1:   # the timed pass WAS one batch at a time (the strict leg: 13 s per pass)
        solo_ids, solo = outs[0], dt
    else:
        t0 = time.perf_counter()
        solo_ids = eng.generate_greedy(ids, *px, max_new_tokens=n_new, eos_token_id=None)
        torch.cuda.synchronize()
        solo = time.perf_counter() - t0
    timings = eng.last_timings()
    ok = all(np.array_equal(o, want) for o in outs + [solo_ids])
    for s_ in sessions[1:]:
        s_.close()
    B = ids.shape[0]
    return {"value": B * steps / dt, "unit": "images/s", "steps": steps, "ms_per_step": dt / steps * 1e3,
            "in_flight_batches": n_sess, "one_batch_at_a_time": {"value": B / solo, "ms_per_step": solo * 1e3, **timings},
            "ids_checked": bool(ok)}, lone


def extra_legs(args, eng7, cfg7, ids7, dev_px7, lone_ids7, fast_value, n_new):
    """The compact legs of a single-GPU --full run (outside the timed region): parity_mode on the benchmark model, then —
    the 7b engine released — BASELINE configs[2] and the per-GPU slice of configs[4] on a 13b model."""
    import numpy as np
    import torch

    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine

    out = {}
    # ---- parity_mode: the precision modes that meet BASELINE.json's "logits within 1e-3, greedy ids bit-exact" bar
    # (tests/test_gpu_e2e.py, tests/test_gpu_fulldepth.py), timed on the SAME batch as `value`
    pm = {"bar": "logits within 1e-3 of the fp32 CPU reference, greedy ids bit-exact (tests: test_fixture_strict_mode, "
                 "test_fixture_split_mode, test_gpu_fulldepth)", "fast_path_value": fast_value}
    strict_ids = None
    for mode, steps, inflight in (("strict", 1, 1), ("split", max(args.extra_steps, args.inflight), args.inflight)):
        try:
            eng7.set_precision(mode)
        except (KeyError, ValueError) as e:
            pm[mode] = {"error": "mode not available: %r" % (e,)}
            continue
        try:
            leg, ids_ = run_leg(eng7, cfg7, ids7, dev_px7, n_new, steps, inflight, precision=mode)
            leg["frac_of_fast_path"] = leg["value"] / fast_value
            leg["ids_equal_fast_path"] = float((ids_ == lone_ids7).mean())
            if mode == "strict":
                strict_ids = ids_
                leg["what"] = "fp32 activations end to end on v_mfma_f32_16x16x4_f32 (csrc/strict.hip)"
            else:
                leg["what"] = ("fp32 activations in HBM, every MFMA operand split into bf16 hi + lo fragments on the fast kernels "
                               "(2 MFMAs per weight k-step, 3 per attention product)")
                if strict_ids is not None:
                    leg["ids_equal_strict"] = bool(np.array_equal(ids_, strict_ids))
            pm[mode] = leg
        finally:
            eng7.set_precision("bf16")
    out["parity_mode"] = pm
    eng7.close()
    torch.cuda.empty_cache()
    # ---- the fp16-operand library (round 6): the same kernels built with -DVC_F16 — IEEE fp16 MFMA operands, the operand precision of
    # the reference's own GPU path (vcoder_llava/model/builder.py:39 torch_dtype=float16, :142).  Not a mode that meets 1e-3 at full
    # depth (2.9e-3 of |logit|max at 32 layers against the bf16 library's 3.2e-2: tests/test_gpu_fulldepth.py::
    # test_full_depth_7b_fp16_operand_library); reported here for what it costs: the same batch, the same four calls in flight
    try:
        e16 = HipEngine(cfg7, operands="fp16")
        e16.load_synthetic(42)
        e16.finalize()
        leg, ids16 = run_leg(e16, cfg7, ids7, dev_px7, n_new, max(args.extra_steps, args.inflight), args.inflight)
        leg["frac_of_fast_path"] = leg["value"] / fast_value
        leg["ids_equal_fast_path"] = float((ids16 == lone_ids7).mean())
        if strict_ids is not None:
            leg["ids_equal_strict_fraction"] = float((ids16 == strict_ids).mean())
            leg["ids_equal_strict_fraction_of_the_bf16_library"] = float((lone_ids7 == strict_ids).mean())
        leg["what"] = ("libvcoder_hip_f16.so: every MFMA operand and stored activation in IEEE fp16 (11 significant bits; bf16: 8) on "
                       "v_mfma_f32_16x16x32_f16, conversions saturating at 65504; weights of an fp16 checkpoint held exactly")
        leg["logit_deviation_vs_fp32_reference"] = {"fixtures": "5.0e-4 of |logit|max (bf16 library 3.4e-3 ... 4.3e-3)",
                                                    "7b_full_depth": "2.9e-3 of |logit|max (bf16 library 3.2e-2)",
                                                    "tests": ["tests/test_gpu_e2e.py::test_fixture_fp16_operand_library",
                                                              "tests/test_gpu_fulldepth.py::test_full_depth_7b_fp16_operand_library"]}
        pm["fp16"] = leg
        e16.close()
    except Exception as e:      # the fp16 library is optional for the headline: say so instead of failing the line
        pm["fp16"] = {"error": repr(e)}
    torch.cuda.empty_cache()
    # ---- BASELINE configs[2] (13b bf16, batch 16, one GPU) and the per-GPU slice of configs[4] (13b fp8 weights, batch 16)
    cfg13 = vcfg.vicuna_13b("vcoder_ds")
    B13 = 16
    ids13 = np.stack([synth.synth_prompt_ids(cfg13.vocab_size, "vcoder_ds", sample=b) for b in range(B13)])
    px13 = tuple(torch.from_numpy(a).cuda() for a in synth.synth_batch(B13, cfg13.vit_image_size))
    for key, weights, desc in (("c3_13b_bf16_b16", "bf16", "BASELINE configs[2]: VCoder-DS LLaVA-1.5-13b bf16, batch=16, 128-tok decode on one MI355X"),
                               ("c5_slice_13b_fp8_b16", "fp8", "per-GPU slice of BASELINE configs[4]: VCoder-DS LLaVA-1.5-13b fp8-e4m3 weights "
                                                               "(W8A8 prefill on the K=128 scaled fp8 MFMA, W8A16 decode, e4m3 KV cache), batch=16 per GPU")):
        e13 = HipEngine(cfg13)
        e13.load_synthetic(42)
        if weights != "bf16":
            e13.set_weight_format(weights)
        e13.finalize()
        leg, lone13 = run_leg(e13, cfg13, ids13, px13, n_new, args.extra_steps, 2)
        leg["config"] = desc
        leg["dtype"] = "bf16" if weights == "bf16" else "fp8-e4m3 prefill linears / bf16"
        if weights == "bf16":
            # the mode that meets the 1e-3 / bit-exact bar at this size (tests/test_gpu_fulldepth.py::test_full_size_13b_c3 checks
            # it against the fp32 oracle), timed on the same batch
            try:
                sp, ids_sp = run_leg(e13, cfg13, ids13, px13, n_new, args.extra_steps, 2, precision="split")
                sp["frac_of_fast_path"] = sp["value"] / leg["value"]
                sp["ids_equal_fast_path"] = float((ids_sp == lone13).mean())
                leg["parity_mode"] = {"bar": "logits within 1e-3 of the fp32 CPU reference, greedy ids bit-exact "
                                             "(tests/test_gpu_fulldepth.py::test_full_size_13b_c3)", "split": sp}
            finally:
                e13.set_precision("bf16")
        else:
            leg["parity"] = {"what": "e4m3 weights + e4m3 activation rows in the prefill linears: no fp32-reference tolerance applies "
                                     "end to end (the format's own re-rounding noise compounds over 40 layers); pinned PER LAYER, "
                                     "teacher-forced on the oracle's own layer inputs at these dimensions",
                             "tests": ["tests/test_gpu_e2e.py::test_fp8_formats_per_layer_teacher_forced (tolerances asserted there: W8A16 rms 2e-3 / "
                                       "max 2e-2 of |x_out|max, fp8 rms 1.5e-2 / max 8e-2)",
                                       "tests/test_gpu_e2e.py::test_fp8_formats_per_layer_with_massive_activation_channels (three hidden channels 300 x "
                                       "the rest, deviations relative to the layer update)",
                                       "tests/test_gpu_fulldepth.py::test_fp8_formats_vs_bf16_full_depth_13b (40 layers: logit correlation with the bf16 "
                                       "path >= 0.75; e4m3 KV against bf16 KV >= 0.98)"],
                             "measured": "the runs of these tests on MI355X are committed under profiles/ (r05_g_fp8_*.txt); no figure is restated here",
                             "quantiser_bytes_and_scales_vs_torch_float8_e4m3fn": "bit-exact",
                             "kv_cache": "e4m3 rows (no scale): bytes == torch's e4m3 cast of the bf16 rows, decode attention == the fp32 "
                                         "oracle on the dequantised cache to one bf16 rounding (tests/kernel_cases.py::check_kv8); the "
                                         "oracle's fp8 mode models the cache in the fixtures' cached steps",
                             "e4m3_gemm_vs_fp64_of_same_operands": "<= 3.9e-5 rel"}
        out[key] = leg
        e13.close()
        torch.cuda.empty_cache()
    return out


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import numpy as np
    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start bench.py directly (it launches its own ranks) or "
                         f"with torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False and there is no CPU fallback")
    # debugging knobs for exercising the multi-process path on a 1-GPU box: all ranks on one device, gloo gather
    if os.environ.get("VC_BENCH_FORCE_DEVICE") is not None:
        local = int(os.environ["VC_BENCH_FORCE_DEVICE"])
    backend = os.environ.get("VC_BENCH_BACKEND", "nccl")   # "nccl" IS RCCL on ROCm
    torch.cuda.set_device(local)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist_mod

        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:   # --force-dist without a launcher: a rendezvous of one
            with socket.socket() as s_:
                s_.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(s_.getsockname()[1]))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine
    from vcoder_amd.parallel import TokenComm, gather_token_ids, shard_range

    cfg = vcfg.vicuna_7b("vcoder_ds") if args.model == "7b" else vcfg.vicuna_13b("vcoder_ds")
    eng = HipEngine(cfg, device_index=local)
    eng.load_synthetic(42)
    if args.weights != "bf16":
        eng.set_weight_format(args.weights)
    eng.finalize()
    B, N_new = args.batch, args.new_tokens
    first, _ = shard_range(world * B, rank, world)   # contiguous shard of the global batch
    ids = np.stack([synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=first + b) for b in range(B)])
    host_px = synth.synth_batch(B, cfg.vit_image_size, first)
    dev_px = tuple(torch.from_numpy(a).cuda() for a in host_px)

    comm = None
    if args.gather == "cabi":
        if args.force_dist and world == 1:
            os.environ["VC_COMM_FORCE_RCCL"] = "1"   # a one-rank RCCL communicator inside the library (csrc/comm.hip)

        def exchange(raw: bytes) -> bytes:      # rank 0's RCCL unique id -> every rank, through the rendezvous store
            box = [raw]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        comm = TokenComm(eng, rank, world, exchange if world > 1 else None)

    def gather(local_ids):
        if comm is not None:
            return comm.allgather(local_ids)
        return gather_token_ids(local_ids, dist, device="cuda" if backend == "nccl" else None, force=args.force_dist)

    import threading

    n_sess = max(1, min(args.inflight, args.steps))
    # in-situ timing of the pool's decode-step kernels (vc_pool_profile): every launch of the timed region stamps its earliest
    # workgroup start / latest workgroup end with the device's wall clock; the `roofline` of --full is computed from those sums.
    # A plain run leaves the stamps on as well and does not read them: the timed steps are the same launches with and without --full
    pooled_run = os.environ.get("VC_POOL", "1") != "0"
    insitu_on = not args.no_insitu and pooled_run
    if insitu_on:
        eng.pool_profile(True)
    if args.no_pool_hold:
        eng.pool_set_hold(False)
    if args.no_qkv_fused:
        eng.set_qkv_fused(0)
    if args.gemv_variant is not None:
        from vcoder_amd import _lib as _vlib
        _vlib.load().vck_set_gemv_variant(int(args.gemv_variant))
    sessions = [eng] + [eng.fork() for _ in range(n_sess - 1)]

    def run_steps(k: int, px):
        """k steps (= k batches of B per GPU), distributed round-robin over the in-flight sessions; every step is the
        complete hot path for its batch.  Token ids are all-gathered across ranks once per step, in step order."""
        outs = [None] * k
        errs = []

        def worker(si):
            try:
                for j in range(si, k, n_sess):
                    outs[j] = sessions[si].generate_greedy(ids, *px, max_new_tokens=N_new, eos_token_id=None)
            except BaseException as e:  # surface failures of a session thread in the main thread
                errs.append(e)

        ths = [threading.Thread(target=worker, args=(si,)) for si in range(n_sess)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if errs:
            raise errs[0]
        # the one exchange: all-gather of the token stream (RCCL over xGMI), once per batch; no-op for N=1
        return [gather(o) for o in outs]

    def fence():
        if dist is not None:
            if backend == "nccl":
                dist.barrier(device_ids=[local])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    def timed(k: int, px) -> float:
        fence()
        t0 = time.perf_counter()
        outs = run_steps(k, px)
        fence()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, outs

    timed_px = host_px if args.host_pixels else dev_px
    # what every step must produce: the ids of this rank's batch generated ALONE (one generate() call, nothing else in
    # flight).  Every timed step feeds the same inputs, so each of its outputs has to equal this, whoever shared its decode
    # steps in the pool — checked below for every step of the timed region (`ids_checked`), the run fails on a mismatch.
    lone_ids = sessions[0].generate_greedy(ids, *dev_px, max_new_tokens=N_new, eos_token_id=None)
    lone_gathered = gather(lone_ids)
    if args.warmup > 0:
        run_steps(max(args.warmup, n_sess), timed_px)  # every session captures its decode graph before the timed region
    steps0 = eng.pool_step_counts()
    if insitu_on:
        torch.cuda.synchronize()
        eng.pool_profile_read(reset=True)      # drop the warm-up's launches
    dt, outs = timed(args.steps, timed_px)
    step_mix = [a - b for a, b in zip(eng.pool_step_counts(), steps0)]   # pooled decode steps of the timed region by 8/16/24/32 rows
    insitu = eng.pool_profile_read(reset=True) if insitu_on and args.full else None   # every decode-step launch of the timed region, as it ran
    if insitu is not None:
        # the side legs below run without the stamps (their fold launch costs a lone batch ~1 %: 34 us of a 3.4-ms step); the pool is
        # re-captured without them by the next call, outside any timed region
        eng.pool_profile(False)
        sessions[0].generate_greedy(ids, *dev_px, max_new_tokens=2, eos_token_id=None)
    bad_steps = [j for j, o in enumerate(outs) if not np.array_equal(np.asarray(o), np.asarray(lone_gathered))]
    ids_checked = len(bad_steps) == 0 and all(np.asarray(o).shape == (world * B, N_new) for o in outs)
    if args.dump_ids and rank == 0:
        np.save(args.dump_ids, outs[-1])
    if args.dump_outputs and rank == 0:
        last = np.asarray(outs[-1])
        assert last.max() < 2 ** 24   # token ids are exact in float32
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "new_token_ids.npy"), last.astype(np.float32))
    pooled = pooled_run and sum(step_mix) > 0
    S_prompt = 64 + 2 * cfg.num_patches
    res = None
    if rank == 0:   # the headline: all of a plain run's line, and the head of a --full one
        res = {
            "metric": "images/sec (3xViT encode + 128-tok decode), VCoder-DS-7b" if args.model == "7b"
                      else "images/sec (3xViT encode + 128-tok decode), VCoder-DS-13b",
            "value": world * B * args.steps / dt, "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16" if args.weights != "fp8" else "fp8-e4m3 prefill linears / bf16", "data": "synthetic",
            "config": {"workload": f"VCoder-DS LLaVA-1.5-{args.model} {WEIGHTS_DESC[args.weights]}, batch={B}/GPU RGB+seg+depth 336x336, "
                                   f"prefill S={S_prompt}, {N_new}-token greedy decode", "global_batch": world * B,
                       "parallelism": f"dp{world}", "weights": "seeded synthetic (vcoder_amd/synth.py)",
                       "in_flight_batches_per_gpu": n_sess,
                       "value_is": (f"{n_sess} generate() calls of batch {B} in flight per GPU, each a complete, independent hot-path "
                                    f"pass; their cached decode steps " + ("share weight passes in the decode pool" if pooled else "run on private loops (VC_POOL=0)")
                                    + "; --full adds one_batch_at_a_time for a lone batch") if n_sess > 1 else "one batch at a time",
                       "decode_pool": pooled,
                       "inputs": "host buffers (PCIe inclusive)" if args.host_pixels else "resident in HBM",
                       "token_gather": ("vc_allgather_tokens (RCCL via the C ABI%s)" % ("" if comm.uses_rccl else "; world 1: host copy")) if comm is not None else
                                       ("torch.distributed all_gather_into_tensor (%s)" % backend if dist is not None else "none (1 GPU)"),
                       "force_dist": bool(args.force_dist),
                       "in_situ_timing_stamps": bool(insitu_on), "qkv_epilogue_fused": not args.no_qkv_fused},
            "ids_checked": bool(ids_checked),
            "ids_check": {"what": "ids of EVERY step of the timed region == ids of the same batch generated alone, bit for bit",
                          "steps_checked": args.steps, "mismatching_timed_steps": bad_steps},
        }

    def teardown():
        if comm is not None:
            comm.close()
        if dist is not None:
            fence()
            dist.destroy_process_group()

    def fail_if_ids_differ():
        if not ids_checked:
            raise SystemExit("bench.py: the ids of the timed region differ from the ids of the same batch generated alone "
                             "(steps %s) - the measurement is void" % bad_steps)

    if not args.full:
        teardown()
        if rank == 0:
            print(json.dumps(res), flush=True)
        fail_if_ids_differ()
        return
    # ---- transparency legs of --full, outside the timed region --------------------------------------------------------
    # (a) the other residency of the inputs (PCIe-inclusive when `value` is resident, and vice versa)
    k_side = max(n_sess, min(args.steps, 2 * n_sess))
    other_px = dev_px if args.host_pixels else host_px
    dt_other, outs_other = timed(k_side, other_px)
    ids_checked = ids_checked and all(np.array_equal(np.asarray(o), np.asarray(lone_gathered)) for o in outs_other)
    # (a2) inter-token latency of the SAME configuration (the hold policy and the pool trade it for throughput —
    # say how much): every call streams its new column after every pooled step (vc_generate's token callback, stream_every = 1) and
    # the host stamps the arrivals; two batches per session, so that every call also sees the others' joins (a hold = one pause of
    # about a prefill).  Outside the timed region: the callbacks cost a D2H copy per step and call.
    lat = None
    if pooled_run and n_sess > 1:
        stamps = [[] for _ in range(n_sess)]

        def lat_worker(si):
            for _ in range(2):
                arr = stamps[si]
                arr.append(None)   # call boundary
                sessions[si].generate(ids, *dev_px, max_new_tokens=N_new, eos_token_id=None,
                                      on_tokens=lambda first, cols, arr=arr: arr.append((time.perf_counter(), first, cols.shape[1])), stream_every=1)
        ths = [threading.Thread(target=lat_worker, args=(si,)) for si in range(n_sess)]
        for t_ in ths:
            t_.start()
        for t_ in ths:
            t_.join()
        gaps = []
        for arr in stamps:
            prev = None
            for ev in arr:
                if ev is None:
                    prev = None
                    continue
                if prev is not None and ev[2] > 0:
                    gaps.extend([(ev[0] - prev[0]) * 1e3 / ev[2]] * ev[2])   # a report that carries k columns: k tokens, gap / k each
                prev = ev
        if gaps:
            g_ = np.sort(np.asarray(gaps))
            lat = {"unit": "ms between consecutive tokens of one generate() call, as its streamer callback sees them",
                   "p50": float(g_[len(g_) // 2]), "p90": float(g_[int(len(g_) * 0.9)]), "p99": float(g_[int(len(g_) * 0.99)]),
                   "max": float(g_[-1]), "tokens": int(len(g_)), "calls_in_flight": n_sess,
                   "pool_hold_policy": not args.no_pool_hold,
                   "note": "max = a step that waited for another call's encode + prefill (the hold policy) — vc_pool_set_hold(m, 0) steps "
                           "whatever rows are active instead"}
    # (b) the same step strictly one batch at a time on this rank
    fence()
    t1 = time.perf_counter()
    for _ in range(2):
        o_ = sessions[0].generate_greedy(ids, *dev_px, max_new_tokens=N_new, eos_token_id=None)
        ids_checked = ids_checked and np.array_equal(o_, lone_ids)
    torch.cuda.synchronize()
    solo = (time.perf_counter() - t1) / 2
    timings = sessions[0].last_timings()
    # The two HBM-bound kernels of a decode step, measured live (HIP events on the engine's stream, real arguments, all
    # layers) at every row count the timed region ran its steps at: the pool steps over 8 / 16 / 24 / 32 rows as requests
    # join and leave (step_mix), a private loop over the batch's own rows.
    if pooled:
        mix = {8 * (i + 1): n for i, n in enumerate(step_mix) if n > 0}
    else:
        mix = {min(B, 16): args.steps * (N_new - 1)}
    prof_by_rows, att_by_rows = {}, {}
    for r_ in sorted(set(mix) | {min(B, 16)}):
        prof_by_rows[r_] = eng.profile_decode_gemv(r_, reps=3)
        att_by_rows[r_] = eng.profile_decode_attention(r_, S_prompt + N_new // 2, reps=3)   # mid-generation context
    rows_step = max(mix, key=lambda r_: mix[r_])          # the row count most steps ran at
    prof, prof_one, prof_att = prof_by_rows[rows_step], prof_by_rows[min(B, 16)], att_by_rows[rows_step]

    if rank == 0:
        traffic = args.pmc_traffic_bytes
        if traffic is None and args.model == "7b" and B == 8 and args.weights == "bf16":
            # separate --pmc FETCH_SIZE pass of this kernel at this row count (gfx950 x2 correction applied, see the file)
            f_ = _pmc_traffic_file()
            if f_ and os.path.exists(f_):
                with open(f_) as f:
                    traffic_by_rows = json.load(f).get("hbm_read_bytes_per_launch_by_rows", {})
                traffic = traffic_by_rows.get(str(rows_step))
            if traffic is None and rows_step == 8 and os.path.exists(os.path.join(ROOT, "profiles", "r01_pmc_traffic.json")):
                with open(os.path.join(ROOT, "profiles", "r01_pmc_traffic.json")) as f:
                    traffic = json.load(f)["hbm_read_bytes_per_launch"]
        S = 64 + 2 * cfg.num_patches
        ms_step = dt / args.steps * 1e3
        # composite roofline of ONE batch of B alone: MFMA leg (encode + prefill) + HBM leg (decode)
        flops, w_bytes, kv_bytes = work_per_sample(cfg, S, N_new, 1.0 if args.weights != "bf16" else 2.0)
        mfma_ms = B * flops / (MFMA_PEAK_TFLOPS * 1e12) * 1e3
        if args.weights == "fp8":   # the prefill's decoder linears run on the scaled fp8 MFMA: priced at its dense peak
            lin = 2 * S * cfg.num_hidden_layers * (4 * cfg.hidden_size ** 2 + 3 * cfg.hidden_size * cfg.intermediate_size)
            mfma_ms = B * ((flops - lin) / (MFMA_PEAK_TFLOPS * 1e12) + lin / (MFMA_FP8_PEAK_TFLOPS * 1e12)) * 1e3
        hbm_ms = ((N_new - 1) * w_bytes + B * kv_bytes) / (HBM_PEAK_GBS * 1e9) * 1e3
        # with k batches in flight whose decode steps share one weight pass, the HBM leg of a batch shrinks to
        # weights / k + its own KV: the bound of what `value` measures
        # (rows that shared a weight pass, averaged over the timed region's steps) / B
        share = sum(n * r_ for r_, n in mix.items()) / sum(mix.values()) / B if pooled else 1
        hbm_ms_shared = ((N_new - 1) * w_bytes / share + B * kv_bytes) / (HBM_PEAK_GBS * 1e9) * 1e3
        # time-weighted over the step mix of the timed region: total kernel time and algorithmic bytes per kernel family;
        # `roofline` is the family with more time
        def family(by_rows):
            steps = sum(mix.values())
            t_us = sum(mix[r_] * by_rows[r_]["avg_us"] * by_rows[r_]["launches_per_step"] for r_ in mix)
            byts = sum(mix[r_] * by_rows[r_]["avg_bytes"] * by_rows[r_]["launches_per_step"] for r_ in mix)
            nl = sum(mix[r_] * by_rows[r_]["launches_per_step"] for r_ in mix)
            return {"avg_launch_us": t_us / nl, "algorithmic_bytes_per_launch": byts / nl, "achieved": byts / (t_us * 1e-6) / 1e9,
                    "frac": byts / (t_us * 1e-6) / 1e9 / HBM_PEAK_GBS, "us_per_step": t_us / steps,
                    "by_rows": {str(r_): {"steps": mix[r_], "avg_launch_us": by_rows[r_]["avg_us"],
                                          "algorithmic_bytes_per_launch": by_rows[r_]["avg_bytes"],
                                          "frac": by_rows[r_]["avg_bytes"] / (by_rows[r_]["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS}
                                for r_ in sorted(mix)}}
        fam_g, fam_a = family(prof_by_rows), family(att_by_rows)
        t_gemv, t_att = fam_g["us_per_step"], fam_a["us_per_step"]
        pmc = {}
        f_ = _pmc_traffic_file()
        if args.model == "7b" and B == 8 and args.weights == "bf16" and f_ and os.path.exists(f_):
            with open(f_) as f:
                pmc = json.load(f)

        def traffic_avg(key, by_rows):   # PMC FETCH_SIZE bytes per launch (separate pass, see the file), weighted like the times
            t = pmc.get(key, {})
            if not all(str(r_) in t for r_ in mix):
                return None
            nl = sum(mix[r_] * by_rows[r_]["launches_per_step"] for r_ in mix)
            return sum(mix[r_] * by_rows[r_]["launches_per_step"] * t[str(r_)] for r_ in mix) / nl
        fam_g["traffic"] = traffic if args.pmc_traffic_bytes is not None else traffic_avg("hbm_read_bytes_per_launch_by_rows", prof_by_rows)
        fam_a["traffic"] = traffic_avg("attention_hbm_read_bytes_per_launch_by_rows", att_by_rows)
        fam_g["what"] = f"decode weight streaming, {prof['launches_per_step']} launches per step, weights of one step shared by the rows in it"
        fam_a["what"] = f"KV streaming, {prof_att['launches_per_step']} launches per step, context ~{S_prompt + N_new // 2}"
        fam_g["one_batch_alone"] = {"rows": min(B, 16), "avg_launch_us": prof_one["avg_us"],
                                    "achieved": prof_one["avg_bytes"] / (prof_one["avg_us"] * 1e-6) / 1e9}
        kernels = {"gemv_dma_kernel": fam_g, "attention_decode_fused_kernel": fam_a}
        for f_ in (fam_g, fam_a):
            f_["measured"] = ("isolated replay AFTER the timed region: HIP events around back-to-back sweeps of this kernel alone, real arguments, "
                              "all layers (vc_profile_decode_gemv / _attention)")
        how = fam_g["measured"]
        if insitu is not None and sum(v["launches"] for r_ in insitu.values() for v in r_.values()) > 0:
            # ---- IN SITU: every launch of the timed region as it ran there (beside whatever the other sessions had on the GPU) ----
            L_, D_, F_, V_ = cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
            wb = 2.0 if args.weights == "bf16" else 1.0
            kind_bytes = {"qkv": wb * 3 * D_ * D_, "o_proj": wb * D_ * D_, "gate_up": wb * 2 * F_ * D_, "down": wb * D_ * F_, "lm_head": 2.0 * V_ * D_}

            def situ(kinds, total_bytes=None):
                rows_ = [r_ for r_ in sorted(insitu) if sum(insitu[r_][k_]["launches"] for k_ in kinds) > 0]
                us = sum(insitu[r_][k_]["us"] for r_ in rows_ for k_ in kinds)
                nl = sum(insitu[r_][k_]["launches"] for r_ in rows_ for k_ in kinds)
                byts = total_bytes if total_bytes is not None else sum(insitu[r_][k_]["launches"] * kind_bytes[k_] for r_ in rows_ for k_ in kinds)
                by_rows = {}
                for r_ in rows_:
                    u_ = sum(insitu[r_][k_]["us"] for k_ in kinds)
                    n_ = sum(insitu[r_][k_]["launches"] for k_ in kinds)
                    e_ = {"launches": n_, "avg_launch_us": u_ / n_,
                          "avg_exec_us": sum(insitu[r_][k_]["exec_us"] for k_ in kinds) / n_,
                          "by_kind_avg_us": {k_: insitu[r_][k_]["us"] / max(insitu[r_][k_]["launches"], 1) for k_ in kinds}}
                    if total_bytes is None:
                        b_ = sum(insitu[r_][k_]["launches"] * kind_bytes[k_] for k_ in kinds)
                        e_["frac"] = b_ / (u_ * 1e-6) / 1e9 / HBM_PEAK_GBS
                        e_["us_per_layer"] = sum(insitu[r_][k_]["us"] / max(insitu[r_][k_]["launches"], 1) for k_ in kinds if k_ != "lm_head")
                    by_rows[str(r_)] = e_
                ex_ = sum(insitu[r_][k_]["exec_us"] for r_ in rows_ for k_ in kinds)
                return {"launches": nl, "total_ms": us / 1e3, "avg_launch_us": us / nl, "algorithmic_bytes_per_launch": byts / nl,
                        "avg_exec_us": ex_ / nl, "frac_exec_only": byts / (ex_ * 1e-6) / 1e9 / HBM_PEAK_GBS,
                        "achieved": byts / (us * 1e-6) / 1e9, "frac": byts / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, "by_rows": by_rows}
            n_steps_pool = sum(step_mix)
            sum_ctx = (N_new - 1) * (S_prompt + 1) + (N_new - 1) * (N_new - 2) / 2.0     # keys read by one row over its cached steps
            kv_es = 1.0 if args.weights == "fp8" and getattr(eng, "fp8_kv", True) else 2.0
            att_bytes = args.steps * B * 2.0 * kv_es * D_ * sum_ctx * L_                 # every request of the timed region, all layers
            sg = situ(("qkv", "o_proj", "gate_up", "down", "lm_head"))
            sa = situ(("attention",), att_bytes)
            consistent = sa["launches"] == n_steps_pool * L_ and sg["launches"] == n_steps_pool * (4 * L_ + 1)
            for f_, s_ in ((fam_g, sg), (fam_a, sa)):
                f_["isolated_replay"] = {k_: f_[k_] for k_ in ("avg_launch_us", "algorithmic_bytes_per_launch", "achieved", "frac", "us_per_step", "by_rows")}
                f_.update({k_: s_[k_] for k_ in ("avg_launch_us", "algorithmic_bytes_per_launch", "achieved", "frac", "by_rows", "avg_exec_us", "frac_exec_only")})
                f_["us_per_step"] = s_["total_ms"] * 1e3 / max(n_steps_pool, 1)
                f_["launches_in_timed_region"] = s_["launches"]
                f_["measured"] = ("IN SITU: every launch of the timed region on the device's 100-MHz wall clock (vc_pool_profile), beside whatever "
                                  "the other in-flight calls had on the GPU.  avg_launch_us / achieved / frac use the launch PERIOD = latest "
                                  "workgroup end of the previous launch of the step -> latest workgroup end of this one (dispatch, drain and the "
                                  "inter-kernel gap included; rocprofv3's per-kernel duration is <= it); *_exec* = earliest workgroup start -> "
                                  "latest workgroup end only (<= rocprofv3's)")
            fam_a["algorithmic_bytes"] = "K + V rows of every cached key of every request of the timed region (context %d..%d), all layers" % (S_prompt + 1, S_prompt + N_new - 1)
            t_gemv, t_att = fam_g["us_per_step"], fam_a["us_per_step"]
            how = fam_g["measured"] + ("" if consistent else " [WARNING: launch counts differ from the pool's step histogram]")
        dom = "attention_decode_fused_kernel" if t_att > t_gemv else "gemv_dma_kernel"
        k = kernels[dom]
        roofline = {"bound": "hbm", "kernel": f"{dom} ({k['what']}; {k['us_per_step'] / (t_att + t_gemv) * 100:.0f}% of the decode steps' "
                                              f"kernel time; over the timed region's pool steps: " +
                                              ", ".join(f"{n} over {r_} rows" for r_, n in sorted(mix.items())) + ")",
                    "achieved": k["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": k["frac"], "traffic": k["traffic"],
                    "avg_launch_us": k["avg_launch_us"], "algorithmic_bytes_per_launch": k["algorithmic_bytes_per_launch"],
                    "measured": how, "rows_per_launch": {str(r_): n for r_, n in sorted(mix.items())}}
        if "isolated_replay" in k:
            roofline["isolated_replay"] = {"frac": k["isolated_replay"]["frac"], "avg_launch_us": k["isolated_replay"]["avg_launch_us"]}
        # the whole story in the one object a reader of the parsed line keeps: what `value` is NOT
        res["config"]["c2_as_written_images_per_s"] = B / solo
        res["ids_checked"] = bool(ids_checked)
        res["ids_check"].update({"what": "ids of EVERY step of the timed region (and of the side legs) == ids of the same batch generated "
                                         "alone, bit for bit", "steps_checked": args.steps + k_side + 2})
        res.update({
            "inter_token_latency_ms": lat,
            "phase_ms_one_session": timings,  # encode / prefill / decode wall time of one batch run alone
            "one_batch_at_a_time": {"value": B / solo, "unit": "images/s per GPU", "ms_per_step": solo * 1e3,
                                    "label": "c2_as_written" if (args.model == "7b" and B == 8 and args.weights == "bf16") else "one generate() call at a time",
                                    "what": "BASELINE configs[1] as written: ONE batch of %d in the GPU at a time" % B},
            ("resident_inputs" if args.host_pixels else "pcie_inclusive"): {
                "value": world * B * k_side / dt_other, "unit": "images/s", "ms_per_step": dt_other / k_side * 1e3, "steps": k_side,
                "note": "same loop, pixels %s" % ("resident in HBM" if args.host_pixels else
                                                  "handed over as pageable host fp32 buffers (3 x %.1f MB per batch)" % (host_px[0].nbytes / 1e6))},
            "composite_roofline": {"mfma_leg_ms": mfma_ms, "hbm_leg_ms": hbm_ms, "t_roof_ms": mfma_ms + hbm_ms,
                                   "frac_one_batch": (mfma_ms + hbm_ms) / (solo * 1e3),
                                   "hbm_leg_ms_weights_shared": hbm_ms_shared,
                                   "frac_value": (mfma_ms + hbm_ms_shared) / ms_step,
                                   "peaks": {"mfma_tflops": MFMA_PEAK_TFLOPS, "mfma_fp8_tflops": MFMA_FP8_PEAK_TFLOPS, "hbm_gbs": HBM_PEAK_GBS},
                                   "measured_legs_ms": {"mfma": timings["encode_ms"] + timings["prefill_ms"], "hbm": timings["decode_ms"]}},
            "roofline": roofline,
            "decode_step_kernels": kernels,
        })
        if args.cpu_c1 and world == 1:
            res["cpu_c1"] = cpu_c1_full()
        if world == 1 and not args.no_extra_legs and args.model == "7b" and args.weights == "bf16" and not args.force_dist:
            for s_ in sessions[1:]:
                s_.close()
            res.update(extra_legs(args, eng, cfg, ids, dev_px, lone_ids, res["value"], N_new))
            pm_ = res.get("parity_mode", {})
            res["config"]["parity_mode_split_images_per_s"] = pm_.get("split", {}).get("value")   # the mode that meets the 1e-3 / bit-exact bar
            res["config"]["fp16_operand_library_images_per_s"] = pm_.get("fp16", {}).get("value")
    teardown()
    if rank == 0:
        # The CPU baseline is TIMED at N = 1 only (the contract: rank 0, N = 1) and cached on the box; a world > 1 line carries that
        # cached N = 1 measurement when the box has one (the driver runs N = 1, 2, 4, 8 back to back) and says so otherwise — it
        # never times the oracle inside a multi-rank job (minutes of host work under the launcher's thread settings).
        if not args.no_cpu_baseline:
            cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"vcoder_amd_cpu_baseline_{args.model}_{N_new}.json")
            if world == 1:
                cb = cpu_baseline(cfg, N_new)
                cb["measured_at"] = "this run (N = 1, rank 0)"
                try:
                    with open(cache, "w") as f:
                        json.dump(cb, f)
                except OSError:
                    pass
            else:
                cb = None
                if os.path.exists(cache):
                    try:
                        with open(cache) as f:
                            cb = json.load(f)
                        cb["measured_at"] = "the N = 1 run of bench.py on this box (cached)"
                    except (OSError, ValueError):
                        cb = None
                if cb is None:
                    cb = {"value": None, "unit": "images/s", "kind": "port",
                          "note": "the CPU baseline is timed at N = 1 only; this box holds no cached N = 1 run of bench.py"}
            res["cpu_baseline"] = cb
        print(json.dumps(res), flush=True)
    fail_if_ids_differ()


if __name__ == "__main__":
    main()
