"""Multi-token continuation of a cached sequence (vc_extend / HipEngine.extend / forward with a past and n > 1 ids): the
checks shared by the CPU-emulator tests (tests/test_extend_emu.py) and the `-m gpu` tests (tests/test_gpu_extend.py)."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

import cpu_ref  # oracle (test infrastructure)
import e2e_cases
import kernel_cases as kc
from vcoder_amd import quant, synth
from vcoder_amd.engine import HipEngine


# ---- kernel: vck_attention_extend against an fp64 attention ------------------------------------------------------------
def _u8(be, a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if isinstance(be, kc.EmuBackend):
        return be._guard(a)
    return torch.from_numpy(a).to(be.dev)


def check_attention_extend(be, B, H, P, n, kv8, masked=False, seed=0, tail=8, needle=False, patterns=None, beta=None):
    """n queries per (b, h) at positions P .. P+n-1 over a key-major cache of P + n + `tail` rows (the tail holds values that
    must not be read: huge in bf16, NaN bytes in e4m3).  Reference: fp64 softmax attention over the values the kernel was given
    (kernel_cases.attention_reference), judged by the historical 2^-7 bound and by the signal-scaled bars of kernel_cases.
    needle: chunk key P + t = beta * q[t - 1] (t >= 1) — query t - 1 would score the key right behind its causal range >= 10 nats
    above every key it sees; patterns: kernel_cases.MASK_PATTERNS names, row b takes patterns[b % len], mask stride MASK_STRIDE, the
    hidden keys hold the largest finite magnitudes of the cache format."""
    hd = 128
    rng = np.random.RandomState(seed)
    S = P + n + tail
    q = rng.randn(B, H, n, hd)
    k = rng.randn(B, H, S, hd)
    v = rng.randn(B, H, S, hd)
    big = kc.POISON_E4M3 if kv8 else kc.POISON
    prow = np.zeros(hd)
    prow[0] = big
    if patterns:
        q[..., 0] = kc.Q_SHARED
    if needle:
        kc._needle_keys(q, k[:, :, :P + n], beta, first=P + 1)
    if patterns:
        pkm = kc.key_masks(kc._names_for(B, patterns), [P + n] * B)
        for b in range(B):
            k[b][:, :P + n][:, pkm[b, :P + n] == 0], v[b][:, :P + n][:, pkm[b, :P + n] == 0] = prow, big
    qd = be.bf16(q)
    q_used = be.host_f32(qd).reshape(B, H, n, hd).astype(np.float64)
    if kv8:
        kb, vb = kc.e4m3_bytes(k), kc.e4m3_bytes(v)
        kb[:, :, P + n:] = 0x7F   # e4m3 NaN
        vb[:, :, P + n:] = 0x7F
        kd, vd = _u8(be, kb), _u8(be, vb)
        k_used, v_used = kc.e4m3_from_bytes(kb).astype(np.float64), kc.e4m3_from_bytes(vb).astype(np.float64)
    else:
        k[:, :, P + n:] = 3e4
        v[:, :, P + n:] = 3e4
        kd, vd = be.bf16(k), be.bf16(v)
        k_used = be.host_f32(kd).reshape(B, H, S, hd).astype(np.float64)
        v_used = be.host_f32(vd).reshape(B, H, S, hd).astype(np.float64)
    Tk = P + n
    mstride = ((Tk + 63) // 64) * 64
    km = np.ones((B, mstride), np.uint8)
    if masked:   # hide some cached keys per row (key 0 stays visible: the engine's precondition)
        for b in range(B):
            hide = rng.choice(np.arange(1, max(P, 2)), size=max(1, P // 3), replace=False) if P > 1 else []
            km[b, hide] = 0
    if patterns:
        masked, km, mstride = True, pkm, kc.MASK_STRIDE
    out = be.zeros((B * n, H * hd), "bf16")
    scale = 1.0 / math.sqrt(hd)
    hidden = kc.attention_hidden(B, n, Tk, True, P, km)
    if needle and n > 1:
        kc._assert_needle(q_used, k_used[:, :, :Tk], scale, hidden, P)
    if patterns:
        kc._assert_poison(q_used, k_used[:, :, :Tk], scale, hidden, prow)
    kc._call(be, "vck_attention_extend", qd, kd, vd, out, B, H, n, P, hd, n, S, int(kv8), scale,
             _u8(be, km) if masked else None, mstride)
    got = be.host_f32(out).reshape(B * n, H * hd)
    assert np.isfinite(got).all(), "extend attention: non-finite output (the cache tail was read)"
    what = f"extend attention B{B} H{H} P{P} n{n} kv8={int(kv8)} masked{int(masked)} needle{int(needle)} mask {patterns} [{be.operands}]"
    fig, ref = kc.attention_judge(what, got.reshape(B, n, H, hd).transpose(0, 2, 1, 3), q_used, k_used[:, :, :Tk], v_used[:, :, :Tk], scale,
                                  hidden, "flash", be.operands)
    ref = ref.transpose(0, 2, 1, 3).reshape(B * n, H * hd)
    err = float(np.abs(got - ref).max())
    assert err < 2 ** -7 * max(1.0, float(np.abs(ref).max())), f"extend attention B{B} H{H} P{P} n{n} kv8={kv8}: abs err {err}"
    return err


# ---- engine: prefill, steps, extend, steps against the oracle's continuation ------------------------------------------
# the fp8 format: the continuation's queries read the chunk's own keys / values as e4m3 rows of the cache (as its decode steps
# do), and above 128 rows its GEMMs quantise the activation rows; the oracle keeps both in bf16.  Measured on the emulator
# (GEMMs then from 33 rows on): 5.3e-2 of max|logit| at B n = 80 rows (1.7e-2 for the steps behind it) -> twice that
REL_TOL_FP8_EXTEND = 1.1e-1


def fixture(name):
    """(cfg, seed, (ids, imgs, segs, deps), attention_mask or None) of a golden fixture's inputs"""
    g = np.load(os.path.join(e2e_cases.GOLD, name + ".npz"))
    if "attention_mask" in g.files:   # the padded-batch fixture (e2e_cases.check_masked_fixture)
        cfg = e2e_cases.tiny_cfg(str(g["variant"]))
        ids = g["input_ids"]
        imgs, segs, deps = synth.synth_batch(ids.shape[0], cfg.vit_image_size)
        return cfg, int(g["seed"]), (ids, imgs, segs, deps), g["attention_mask"]
    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    return cfg, int(g["seed"]), (ids, imgs, segs, deps), None


def make_engine(name, lib, fmt="bf16", precision="bf16"):
    """-> (engine, cfg, inputs, state dict the oracle computes with, attention_mask)"""
    cfg, seed, inputs, mask = fixture(name)
    eng = HipEngine(cfg, lib=lib)
    eng.load_synthetic(seed)
    if fmt != "bf16":
        eng.set_weight_format(fmt)
    eng.finalize()
    if precision != "bf16":
        eng.set_precision(precision)
    sd = synth.synth_state_dict(cfg, seed)
    if fmt != "bf16":
        sd = quant.effective_state_dict(sd)
    return eng, cfg, inputs, sd, mask


def run_sequence(eng, om, inputs, n, B_tok_rng, pre_steps=3, post_steps=3, mask=None, reorder=None, hidden=False, attn=False,
                 reserve=None):
    """prefill -> pre_steps decode steps -> extend(n) -> post_steps decode steps on the engine, the same on the oracle
    (OracleModel.forward's cache continued by cpu_ref.llama_forward).  Tokens are drawn from B_tok_rng (teacher forcing).
    -> dict of per-phase max abs errors and the scale."""
    ids, imgs, segs, deps = inputs
    t = lambda a: None if a is None else torch.from_numpy(a)
    last, _, S = eng.prefill(ids, imgs, segs, deps, attention_mask=mask, reserve=reserve)
    ol, cache = om.forward(ids.tolist(), t(imgs), t(segs), t(deps), last_only=True, attention_mask=mask)
    B = ids.shape[0]
    V = eng.cfg.vocab_size
    km = om.mask_ext
    errs = {"prefill": float(np.abs(last - ol[:, -1].numpy()).max())}
    scale = float(np.abs(ol.numpy()).max())

    def okey(extra):
        if km is None:
            return None
        return torch.cat([km, torch.ones(B, cache.length + extra - km.shape[1], dtype=torch.bool)], 1)

    e = 0.0
    for _ in range(pre_steps):
        tok = B_tok_rng.randint(0, V, size=B).astype(np.int32)
        lg, _ = eng.decode_step(tok)
        o = cpu_ref.llama_forward(om.embed_tokens(tok.tolist()).reshape(B, 1, -1) if B > 0 else None, om.sd, om.cfg, cache, om.emu,
                                  last_only=True, key_mask=okey(1))
        e = max(e, float(np.abs(lg - o[:, -1].numpy()).max()))
    errs["pre_steps"] = e
    if reorder is not None:
        eng.reorder_cache(reorder)
        idx = torch.as_tensor(np.asarray(reorder), dtype=torch.long)
        for l in range(len(cache.k)):
            cache.k[l], cache.v[l] = cache.k[l][idx], cache.v[l][idx]
        if km is not None:
            km = km[idx]
    toks = B_tok_rng.randint(0, V, size=(B, n)).astype(np.int32)
    x = torch.stack([om.embed_tokens(r.tolist()) for r in toks], 0)
    ho, ao = ([] if hidden else None), ([] if attn else None)
    P = cache.length
    o = cpu_ref.llama_forward(x, om.sd, om.cfg, cache, om.emu, key_mask=okey(n), hidden_out=ho, attn_out=ao).numpy()
    last, full = eng.extend(toks, hidden_states=hidden, attentions=attn)
    errs["extend"] = float(np.abs(full - o).max())
    errs["extend_last"] = float(np.abs(last - o[:, -1]).max())
    errs["P"] = P
    if hidden:
        hs = eng.last_hidden_states
        assert hs.shape == (eng.cfg.num_hidden_layers + 1, B, n, eng.cfg.hidden_size)
        errs["hidden"] = max(float(np.abs(hs[i] - ho[i].numpy()).max() / max(1.0, float(ho[i].abs().max())))
                             for i in range(len(ho)))
    if attn:
        at = eng.last_attentions
        assert at.shape == (eng.cfg.num_hidden_layers, B, eng.cfg.num_attention_heads, n, P + n)
        errs["attn"] = max(float(np.abs(at[i] - ao[i].numpy()).max()) for i in range(len(ao)))
    e = 0.0
    for _ in range(post_steps):
        tok = B_tok_rng.randint(0, V, size=B).astype(np.int32)
        lg, _ = eng.decode_step(tok)
        o = cpu_ref.llama_forward(om.embed_tokens(tok.tolist()).reshape(B, 1, -1), om.sd, om.cfg, cache, om.emu,
                                  last_only=True, key_mask=okey(1))
        e = max(e, float(np.abs(lg - o[:, -1].numpy()).max()))
    errs["post_steps"] = e
    errs["scale"] = scale
    return errs
