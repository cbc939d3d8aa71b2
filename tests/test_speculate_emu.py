"""Prompt-lookup speculative decoding on the CPU emulator (tests/emu): the verify attention against the per-row decode attention,
the draft and accept kernels against their numpy statements, generate(speculate=k) against the plain session loop."""
import pytest

import kernel_cases as kc
import speculate_cases as sc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def model(be):
    return sc.model_for("vcoder_ds", be.lib)


@pytest.mark.parametrize("hd,B,Q,kv8,where,nq,mask", sc.ATTN_VERIFY_CASES)
def test_attention_verify(be, hd, B, Q, kv8, where, nq, mask):
    sc.check_attention_verify(be, hd, B, Q, kv8, where, nq, mask, seed=hd + 7 * Q + B)


def test_attention_verify_fp16_operand_library():
    be16 = kc.EmuBackend("fp16")
    sc.check_attention_verify(be16, 128, 3, 5, 0, ("straddle", "zero", "end"), (5, 3, 0), True)
    sc.check_attention_verify(be16, 64, 1, 8, 1, ("straddle",))


def test_attention_verify_refused(be):
    sc.check_attention_verify_refused(be)


def test_spec_draft(be):
    sc.check_spec_draft(be)


@pytest.mark.parametrize("logprobs", [False, True])
def test_spec_accept(be, logprobs):
    sc.check_spec_accept(be, logprobs)


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_generate(model, k, B):
    sp, ref, _ = sc.check_generate(model, k, B, lookup="truth")
    assert (sp["steps"] < ref.shape[1] - 1).all()


def test_lookup_sources_and_counters(model):
    sc.check_lookup_sources(model, 3, 2)


@pytest.mark.parametrize("ng", [1, 4])
def test_ngram_sizes(model, ng):
    sc.check_generate(model, 3, 2, lookup="corrupted", ng=ng)


@pytest.mark.parametrize("lookup", ["truth", "none"])
def test_eos_and_stop_sequence(model, lookup):
    sc.check_generate(model, 3, 2, lookup=lookup, eos_from=6)
    sc.check_generate(model, 3, 2, lookup=lookup, stop_from=6)


@pytest.mark.parametrize("fmt", ["fp8", "w4a16"])
def test_weight_formats(be, fmt):
    sp, _, _ = sc.check_generate(sc.model_for("vcoder_ds", be.lib, fmt=fmt), 3, 2, lookup="corrupted")
    assert sp["accepted"].sum() > 0


def test_fp16_operand_library():
    sp, _, _ = sc.check_generate(sc.model_for("vcoder_ds", kc.EmuBackend("fp16").lib, "fp16"), 3, 2, lookup="corrupted")
    assert sp["accepted"].sum() > 0


def test_logprobs(model):
    sc.check_logprobs(model)


def test_streamer(model):
    sc.check_streamer(model)


def test_model_api(model):
    sc.check_model_api(model)


def test_not_served(model):
    sc.check_not_served(model)


def test_refusals(model):
    sc.check_refusals(model)


def test_captures(model):
    sc.check_captures(model)
