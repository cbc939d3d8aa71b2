"""Multi-token continuation of a cached sequence on the MI355X: the extend attention kernel at the true head counts and
context lengths in both libraries, and vc_extend through the engine and forward() (the checks of tests/test_extend_emu.py on
the device)."""
import numpy as np
import pytest
import torch

import cpu_ref
import e2e_cases
import extend_cases as xc
import kernel_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("H,P", [(32, 1215), (40, 2047)])   # 7b / 13b heads; a VCoder-DS prompt and a full cache
@pytest.mark.parametrize("n", [1, 32, 33, 257])
@pytest.mark.parametrize("kv8", [False, True])
def test_attention_extend_true_shapes(be, H, P, n, kv8):
    xc.check_attention_extend(be, 1, H, P, n, kv8=kv8, seed=P + n)


def test_attention_extend_key_mask(be):
    xc.check_attention_extend(be, 2, 32, 1215, 40, kv8=False, masked=True, seed=5)
    xc.check_attention_extend(be, 2, 32, 1215, 40, kv8=True, masked=True, seed=6)


@pytest.mark.parametrize("H,P", [(32, 1215), (40, 2047)])
@pytest.mark.parametrize("n", [33, 257])
@pytest.mark.parametrize("kv8", [False, True])
def test_attention_extend_needle(be, H, P, n, kv8):
    """chunk key P + t = 4 q[t - 1]: one key too many for one query is an O(1) error in every element of its row; the second launch
    under a key mask per batch row whose hidden keys hold the largest finite values of the cache format"""
    xc.check_attention_extend(be, 1, H, P, n, kv8=kv8, needle=True, seed=P + n)
    xc.check_attention_extend(be, 2, H, P, n, kv8=kv8, needle=True, patterns=["early", "pad200"], seed=P + n + 1)


@pytest.mark.parametrize("fmt", ["bf16", "w8a16", "fp8"])
@pytest.mark.parametrize("n", [5, 64, 65])
def test_engine_extend_against_oracle(fmt, n):
    """prefill, 3 steps, extend(n), 3 steps over B = 2 rows: both sides of the 128-row GEMV / GEMM split"""
    eng, cfg, inputs, sd, _ = xc.make_engine("ds_img_depth_seg", None, fmt)
    r = xc.run_sequence(eng, cpu_ref.OracleModel(cfg, sd, emu_bf16=True), inputs, n, np.random.RandomState(n))
    tol = (xc.REL_TOL_FP8_EXTEND * r["scale"]) if fmt == "fp8" else e2e_cases.TOL_VS_FP32_REF
    assert r["extend"] < tol and r["extend_last"] < tol and r["post_steps"] < tol, r
    eng.close()


def test_engine_extend_mask_reorder_grow_diagnostics():
    eng, cfg, inputs, sd, mask = xc.make_engine("ds_padded_mask", None)
    om = cpu_ref.OracleModel(cfg, sd, emu_bf16=True)
    for n in (3, 45):
        r = xc.run_sequence(eng, om, inputs, n, np.random.RandomState(n), mask=mask, hidden=True, attn=True)
        assert r["extend"] < e2e_cases.TOL_VS_FP32_REF and r["post_steps"] < e2e_cases.TOL_VS_FP32_REF, r
        assert r["hidden"] < 1e-2 and r["attn"] < 2e-3, r
    eng.close()
    eng, cfg, inputs, sd, _ = xc.make_engine("ds_img_depth_seg", None)
    om = cpu_ref.OracleModel(cfg, sd, emu_bf16=True)
    r = xc.run_sequence(eng, om, inputs, 4, np.random.RandomState(3), reorder=np.array([1, 0]))
    assert r["extend"] < e2e_cases.TOL_VS_FP32_REF and r["post_steps"] < e2e_cases.TOL_VS_FP32_REF, r
    r = xc.run_sequence(eng, om, inputs, 140, np.random.RandomState(70), pre_steps=1, reserve=1)   # grows the cache
    assert r["extend"] < e2e_cases.TOL_VS_FP32_REF and r["post_steps"] < e2e_cases.TOL_VS_FP32_REF, r
    eng.close()


@pytest.mark.parametrize("mode", ["strict", "split"])
def test_extend_equals_decode_steps_bitwise(mode):
    eng, cfg, (ids, imgs, segs, deps), _, _ = xc.make_engine("ds_img_depth_seg", None, precision=mode)
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


def test_forward_with_past_and_several_ids():
    from vcoder_amd import synth
    from vcoder_amd.model.language_model import VCoderDSLlavaLlamaForCausalLM

    g, cfg, ids, imgs, segs, deps = e2e_cases.fixture_inputs("ds_img_depth_seg")
    sd = synth.synth_state_dict(cfg, int(g["seed"]))
    model = VCoderDSLlavaLlamaForCausalLM.from_tensors(cfg, sd.items(), device="cuda")
    t = torch.from_numpy
    out = model(input_ids=t(ids), images=t(imgs), segs=t(segs), depths=t(deps), use_cache=True)
    pkv = out.past_key_values
    P, B, V = pkv.length, ids.shape[0], cfg.vocab_size
    new = t(np.random.RandomState(1).randint(0, V, size=(B, 9)))
    out2 = model(input_ids=new, past_key_values=pkv, use_cache=True)
    assert tuple(out2.logits.shape) == (B, 9, V) and pkv.length == P + 9
    om = cpu_ref.OracleModel(cfg, sd, emu_bf16=True)
    _, cache = om.forward(ids.tolist(), t(imgs), t(segs), t(deps))
    x = torch.stack([om.embed_tokens(r.tolist()) for r in new.numpy()], 0)
    o = cpu_ref.llama_forward(x, om.sd, cfg, cache, True)
    assert float((out2.logits.cpu() - o).abs().max()) < e2e_cases.TOL_VS_FP32_REF


# ---- true 7b dimensions (D 4096, F 11008, V 32000, 32 heads), cut to 2 decoder + 3 ViT layers as test_gpu_e2e.py's
# test_true_dims_against_oracle: the extend path at a real cache capacity, real GEMV / GEMM geometries and P = 1216
def _true_dims(fmt="bf16"):
    from vcoder_amd import config as vcfg, synth
    from vcoder_amd.engine import HipEngine

    cfg = vcfg.vicuna_7b("vcoder_ds")
    cfg.num_hidden_layers = 2
    cfg.vit_num_layers = 3
    eng = HipEngine(cfg)
    eng.load_synthetic(11)
    if fmt != "bf16":
        eng.set_weight_format(fmt)
    eng.finalize()
    ids = synth.synth_prompt_ids(cfg.vocab_size, "vcoder_ds", sample=3)[None]
    px = synth.synth_batch(1, 336, first=3)
    return cfg, eng, ids, px


# measured on MI355X: max |extend logits - oracle| over all B n rows, relative to max|logits|: decode GEMVs 8.2e-3 (B=1 n=40),
# 7.7e-3 (B=8 n=4), 7.3e-3 (B=8 n=5); prefill GEMMs 6.6e-3 (B=8 n=17).  The tolerance is twice the largest
TRUE_DIMS_REL_TOL = 1.7e-2


def test_true_dims_extend_against_oracle():
    """prefill S = 1216, then extend with B=1 n=40, B=8 n=4 and B=8 n=5 (40 / 32 / 40 rows: the decode GEMVs) and B=8 n=17
    (136 rows: the prefill GEMMs),
    against the bf16-emulating oracle continuing its own prefill's cache (the B rows of a batch share the prompt, so one
    oracle prefill serves every batch: its cache rows are repeated)"""
    from vcoder_amd import synth

    cfg, eng, ids, px = _true_dims()
    sd = synth.synth_state_dict(cfg, 11)
    om = cpu_ref.OracleModel(cfg, sd, emu_bf16=True)
    t = torch.from_numpy
    with torch.no_grad():
        _, base = om.forward(ids.tolist(), *(t(a) for a in px), last_only=True)
    rng = np.random.RandomState(0)
    errs = {}
    for B, n in [(1, 40), (8, 4), (8, 5), (8, 17)]:
        _, _, S = eng.prefill(np.repeat(ids, B, 0), *(np.repeat(a, B, 0) for a in px), reserve=8)
        assert S == 1216
        toks = rng.randint(0, cfg.vocab_size, size=(B, n)).astype(np.int32)
        _, full = eng.extend(toks)
        cache = cpu_ref.KVCache(cfg.num_hidden_layers)
        for l in range(cfg.num_hidden_layers):
            cache.k[l], cache.v[l] = base.k[l].repeat(B, 1, 1, 1), base.v[l].repeat(B, 1, 1, 1)
        with torch.no_grad():
            x = torch.stack([om.embed_tokens(r.tolist()) for r in toks], 0)
            o = cpu_ref.llama_forward(x, om.sd, cfg, cache, True).numpy()
        errs[(B, n)] = float(np.abs(full - o).max() / np.abs(o).max())
    print(f"true-dims extend vs oracle (relative to max|logits|): {errs}")
    assert max(errs.values()) < TRUE_DIMS_REL_TOL, errs
    eng.close()


# measured on MI355X: max |extend logits - logits of the same tokens as n decode steps| relative to max|logits|, fp8 format:
# through the W8A16 GEMVs the steps use 5.2e-3 (n = 8) and 5.5e-3 (n = 40); through the W8A8 GEMMs (e4m3 activation rows,
# which the steps do not quantise) 7.9e-2 (n = 136).  Tolerances twice those
FP8_SELF_TOL = {8: 1.1e-2, 40: 1.1e-2, 136: 1.6e-1}


def test_true_dims_fp8_extend_against_its_decode_steps():
    cfg, eng, ids, px = _true_dims("fp8")
    rng = np.random.RandomState(1)
    errs = {}
    for n in (8, 40, 136):
        toks = rng.randint(0, cfg.vocab_size, size=(1, n)).astype(np.int32)
        eng.prefill(ids, *px, reserve=n + 8)
        ref = np.stack([eng.decode_step(toks[:, i])[0] for i in range(n)], 1)
        eng.prefill(ids, *px, reserve=n + 8)
        _, full = eng.extend(toks)
        errs[n] = float(np.abs(full - ref).max() / np.abs(ref).max())
    print(f"true-dims fp8 extend vs its decode steps (relative to max|logits|): {errs}")
    for n, e in errs.items():
        assert e < FP8_SELF_TOL[n], errs
    eng.close()
