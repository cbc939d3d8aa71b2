"""Multi-token continuation of a cached sequence on the CPU emulator (tests/emu): the extend attention kernel against fp64,
the engine's vc_extend against the oracle's cache continuation, and forward() with a past and n > 1 ids."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cpu_ref
import e2e_cases
import extend_cases as xc
import kernel_cases as kc
from vcoder_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


@pytest.mark.parametrize("P", [1, 31, 64, 100])
@pytest.mark.parametrize("n", [1, 2, 17, 64, 65])
def test_attention_extend_kernel(be, P, n):
    xc.check_attention_extend(be, 2, 2, P, n, kv8=False, seed=P * 131 + n)
    xc.check_attention_extend(be, 1, 2, P, n, kv8=True, seed=P * 131 + n + 1)


@pytest.mark.parametrize("P,n", [(100, 17), (64, 65), (31, 2)])
@pytest.mark.parametrize("kv8", [False, True])
def test_attention_extend_kernel_key_mask(be, P, n, kv8):
    xc.check_attention_extend(be, 2, 2, P, n, kv8=kv8, masked=True, seed=P + n)


@pytest.mark.parametrize("P,n", [(100, 17), (139, 65), (200, 130)])
@pytest.mark.parametrize("kv8", [False, True])
def test_attention_extend_kernel_needle_and_mask_patterns(be, P, n, kv8):
    """chunk key P + t = 4 q[t - 1]: a query that sees one key too many is wrong in every element; poisoned hidden keys, a pattern per row"""
    xc.check_attention_extend(be, 1, 2, P, n, kv8=kv8, needle=True, seed=P + n)
    xc.check_attention_extend(be, 3, 1, P, n, kv8=kv8, needle=True, patterns=["straddle" if P + n > 130 else "singles", "pad63", "ones"], seed=P + n + 1)
    if P + n > 200:
        xc.check_attention_extend(be, 2, 1, P, n, kv8=kv8, needle=True, patterns=["pad200", "early"], seed=P + n + 2)


def test_attention_extend_under_another_wave_order():
    """the kernel tests once more with the emulator's waves in another order and the dynamic-LDS race check on (as
    tests/test_emu_orders.py does for the other kernels)"""
    env = dict(os.environ, VC_EMU_ORDER="11", VC_EMU_RACE="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_extend_emu.py"), "-x", "-q", "-p", "no:cacheprovider",
           "-k", "attention_extend_kernel"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def _oracle(cfg, sd):
    return cpu_ref.OracleModel(cfg, sd, emu_bf16=True)


REL_TOL_FP8_EXTEND = xc.REL_TOL_FP8_EXTEND


def _tol(fmt, scale):
    return (REL_TOL_FP8_EXTEND * scale) if fmt == "fp8" else e2e_cases.TOL_VS_FP32_REF


@pytest.mark.parametrize("fmt", ["bf16", "w8a16", "fp8"])
@pytest.mark.parametrize("n", [5, 64, 65])
def test_engine_extend_against_oracle(emu_lib, fmt, n):
    """prefill, 3 steps, extend(n), 3 steps over B = 2 rows: n = 5 / 64 (10 / 128 rows: the decode GEMVs) and 65 (130 rows:
    the prefill GEMMs)"""
    eng, cfg, inputs, sd, _ = xc.make_engine("ds_img_depth_seg", emu_lib, fmt)
    r = xc.run_sequence(eng, _oracle(cfg, sd), inputs, n, np.random.RandomState(n))
    tol = _tol(fmt, r["scale"])
    assert r["extend"] < tol and r["extend_last"] < tol, r
    assert r["post_steps"] < tol, r
    eng.close()


def test_engine_extend_hidden_states_and_attentions(emu_lib):
    eng, cfg, inputs, sd, _ = xc.make_engine("ds_img_only", emu_lib)
    om = _oracle(cfg, sd)
    for n in (6, 130):   # 1 row per position: GEMVs / GEMMs
        r = xc.run_sequence(eng, om, inputs, n, np.random.RandomState(7 + n), hidden=True, attn=True)
        assert r["extend"] < e2e_cases.TOL_VS_FP32_REF, r
        assert r["hidden"] < 1e-2 and r["attn"] < 2e-3, r
    eng.close()


def test_engine_extend_padded_prefill_keeps_mask(emu_lib):
    """a padded prefill's hidden keys stay hidden from the continuation (the mask the 1-token steps carry)"""
    eng, cfg, inputs, sd, mask = xc.make_engine("ds_padded_mask", emu_lib)
    assert not mask.all()
    for n in (3, 45):   # 3 rows: 9 / 135 token rows
        r = xc.run_sequence(eng, _oracle(cfg, sd), inputs, n, np.random.RandomState(n), mask=mask)
        assert r["extend"] < e2e_cases.TOL_VS_FP32_REF and r["post_steps"] < e2e_cases.TOL_VS_FP32_REF, r
    eng.close()


def test_engine_reorder_then_extend(emu_lib):
    eng, cfg, inputs, sd, _ = xc.make_engine("ds_img_depth_seg", emu_lib)
    B = inputs[0].shape[0]
    assert B >= 2
    reorder = np.arange(B)[::-1].copy()
    r = xc.run_sequence(eng, _oracle(cfg, sd), inputs, 4, np.random.RandomState(3), reorder=reorder)
    assert r["extend"] < e2e_cases.TOL_VS_FP32_REF and r["post_steps"] < e2e_cases.TOL_VS_FP32_REF, r
    eng.close()


def test_engine_extend_grows_the_cache(emu_lib):
    """a reserve of 1 slot: the extend runs past the cache and grows it (grow_kv), the steps behind it still match"""
    eng, cfg, inputs, sd, _ = xc.make_engine("ds_img_only", emu_lib)
    r = xc.run_sequence(eng, _oracle(cfg, sd), inputs, 140, np.random.RandomState(70), pre_steps=1, reserve=1)
    assert r["extend"] < e2e_cases.TOL_VS_FP32_REF and r["post_steps"] < e2e_cases.TOL_VS_FP32_REF, r
    eng.close()


@pytest.mark.parametrize("mode", ["strict", "split"])
def test_extend_equals_decode_steps_bitwise(emu_lib, mode):
    """precision modes 'strict' / 'split': extend(n) runs the n cached steps — the same bits as n decode_step calls"""
    ids, imgs, segs, deps = e2e_cases.fixture_inputs("ds_img_only")[2:]
    eng, cfg, _, _, _ = xc.make_engine("ds_img_only", emu_lib, precision=mode)
    B, n = ids.shape[0], 5
    toks = np.random.RandomState(5).randint(0, cfg.vocab_size, size=(B, n)).astype(np.int32)
    eng.prefill(ids, imgs, segs, deps)
    ref = np.stack([eng.decode_step(toks[:, t])[0] for t in range(n)], 1)
    after_ref, _ = eng.decode_step(toks[:, 0])
    eng.prefill(ids, imgs, segs, deps)
    last, full = eng.extend(toks)
    after, _ = eng.decode_step(toks[:, 0])
    assert np.array_equal(full, ref) and np.array_equal(last, ref[:, -1]) and np.array_equal(after, after_ref)
    eng.close()


# ---- model API ---------------------------------------------------------------------------------------------------------
def _model(emu_lib, name="ds_img_only"):
    from vcoder_amd.model.language_model import VCoderDSLlavaLlamaForCausalLM

    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs(name)
    sd = synth.synth_state_dict(cfg, int(g["seed"]))
    model = VCoderDSLlavaLlamaForCausalLM.from_tensors(cfg, sd.items(), device="cuda", _lib_override=emu_lib)
    return model, cfg, sd, (ids, imgs, segs, deps)


def test_forward_with_past_and_several_ids(emu_lib):
    model, cfg, sd, (ids, imgs, segs, deps) = _model(emu_lib)
    t = torch.from_numpy
    out = model(input_ids=t(ids), images=t(imgs), segs=t(segs) if segs is not None else None,
                depths=t(deps) if deps is not None else None, use_cache=True)
    pkv = out.past_key_values
    P, B, V = pkv.length, ids.shape[0], cfg.vocab_size
    new = torch.from_numpy(np.random.RandomState(1).randint(0, V, size=(B, 7)))
    out2 = model(input_ids=new, past_key_values=pkv, use_cache=True, output_hidden_states=True, output_attentions=True)
    assert tuple(out2.logits.shape) == (B, 7, V) and out2.past_key_values is pkv and pkv.length == P + 7
    assert len(out2.hidden_states) == cfg.num_hidden_layers + 1 and tuple(out2.hidden_states[0].shape) == (B, 7, cfg.hidden_size)
    assert len(out2.attentions) == cfg.num_hidden_layers
    assert tuple(out2.attentions[0].shape) == (B, cfg.num_attention_heads, 7, P + 7)
    # the oracle: the same prefill, then the 7 ids over its cache
    om = cpu_ref.OracleModel(cfg, sd, emu_bf16=True)
    _, cache = om.forward(ids.tolist(), t(imgs), t(segs) if segs is not None else None, t(deps) if deps is not None else None)
    x = torch.stack([om.embed_tokens(r.tolist()) for r in new.numpy()], 0)
    o = cpu_ref.llama_forward(x, om.sd, cfg, cache, True)
    assert float((out2.logits - o).abs().max()) < e2e_cases.TOL_VS_FP32_REF
    # a 1-token step continues at P + 7
    tok = torch.from_numpy(np.random.RandomState(2).randint(0, V, size=(B, 1)))
    out3 = model(input_ids=tok, past_key_values=pkv, use_cache=True)
    o3 = cpu_ref.llama_forward(om.embed_tokens(tok.reshape(-1).tolist()).reshape(B, 1, -1), om.sd, cfg, cache, True)
    assert pkv.length == P + 8 and float((out3.logits - o3).abs().max()) < e2e_cases.TOL_VS_FP32_REF


def test_forward_refusals_leave_the_cache_intact(emu_lib):
    model, cfg, sd, (ids, imgs, segs, deps) = _model(emu_lib)
    t = torch.from_numpy
    out = model(input_ids=t(ids), images=t(imgs), segs=t(segs) if segs is not None else None,
                depths=t(deps) if deps is not None else None, use_cache=True)
    pkv = out.past_key_values
    P, B, V = pkv.length, ids.shape[0], cfg.vocab_size
    probe = torch.from_numpy(np.random.RandomState(3).randint(0, V, size=(B, 1)))
    new = torch.from_numpy(np.random.RandomState(4).randint(0, V, size=(B, 3)))
    bad = new.clone()
    bad[0, 1] = V + 5
    mask_hiding_new = torch.ones(B, P + 3, dtype=torch.long)
    mask_hiding_new[0, -2] = 0
    with pytest.raises(IndexError):
        model(input_ids=bad, past_key_values=pkv)
    with pytest.raises(NotImplementedError):
        model(input_ids=new, past_key_values=pkv, attention_mask=mask_hiding_new)
    with pytest.raises(NotImplementedError):
        model(input_ids=new, past_key_values=pkv, images=t(imgs))
    with pytest.raises(RuntimeError, match="KV cache full"):   # past max_position_embeddings: refused before the mask is touched
        model(input_ids=torch.zeros(B, cfg.max_position_embeddings, dtype=torch.long), past_key_values=pkv)
    assert pkv.length == P
    got = model(input_ids=probe, past_key_values=pkv).logits
    # the same probe on a fresh prefill
    out_b = model(input_ids=t(ids), images=t(imgs), segs=t(segs) if segs is not None else None,
                  depths=t(deps) if deps is not None else None, use_cache=True)
    with pytest.raises(RuntimeError):
        model(input_ids=new, past_key_values=pkv)   # stale handle
    ref = model(input_ids=probe, past_key_values=out_b.past_key_values).logits
    assert torch.equal(got, ref)


def test_two_turn_chat_through_extend(emu_lib):
    """turn 1: a multimodal prompt + greedy steps through forward; turn 2: the user's next text as ONE continuation call —
    against the oracle teacher-forced over the whole conversation"""
    model, cfg, sd, (ids, imgs, segs, deps) = _model(emu_lib)
    t = torch.from_numpy
    V = cfg.vocab_size
    out = model(input_ids=t(ids), images=t(imgs), segs=t(segs) if segs is not None else None,
                depths=t(deps) if deps is not None else None, use_cache=True)
    pkv, B = out.past_key_values, ids.shape[0]
    om = cpu_ref.OracleModel(cfg, sd, emu_bf16=True)
    _, cache = om.forward(ids.tolist(), t(imgs), t(segs) if segs is not None else None, t(deps) if deps is not None else None)
    tok = out.logits[:, -1].argmax(-1, keepdim=True)
    for _ in range(4):   # turn 1's answer
        cpu_ref.llama_forward(om.embed_tokens(tok.reshape(-1).tolist()).reshape(B, 1, -1), om.sd, cfg, cache, True)
        tok = model(input_ids=tok, past_key_values=pkv).logits[:, -1].argmax(-1, keepdim=True)
    turn2 = torch.cat([tok, torch.from_numpy(np.random.RandomState(9).randint(0, V, size=(B, 11)))], 1)
    got = model(input_ids=turn2, past_key_values=pkv).logits
    x = torch.stack([om.embed_tokens(r.tolist()) for r in turn2.numpy()], 0)
    ref = cpu_ref.llama_forward(x, om.sd, cfg, cache, True)
    assert float((got - ref).abs().max()) < e2e_cases.TOL_VS_FP32_REF
