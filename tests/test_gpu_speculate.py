"""Prompt-lookup speculative decoding on the MI355X: the checks of tests/test_speculate_emu.py on the device, both libraries where the
kernels differ, and the bit-identity of a speculated call at 7b dims (2 layers, S = 1216)."""
import pytest

import kernel_cases as kc
import speculate_cases as sc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


def _model(operands="bf16", fmt="bf16"):
    return sc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands, fmt)


@pytest.mark.parametrize("hd,B,Q,kv8,where,nq,mask", sc.ATTN_VERIFY_CASES)
def test_attention_verify(be, hd, B, Q, kv8, where, nq, mask):
    sc.check_attention_verify(be, hd, B, Q, kv8, where, nq, mask, seed=hd + 7 * Q + B)


@pytest.mark.parametrize("hd,kv8", [(128, 0), (128, 1), (64, 0), (64, 1)])
def test_attention_verify_volume(be, hd, kv8):
    sc.check_attention_verify_volume(be, hd, kv8)


def test_attention_verify_refused(be):
    sc.check_attention_verify_refused(be)


def test_spec_draft(be):
    sc.check_spec_draft(be)


@pytest.mark.parametrize("logprobs", [False, True])
def test_spec_accept(be, logprobs):
    sc.check_spec_accept(be, logprobs)


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_generate(k, B):
    sp, ref, _ = sc.check_generate(_model(), k, B, lookup="truth")
    assert (sp["steps"] < ref.shape[1] - 1).all()


@pytest.mark.parametrize("k,B", [(3, 2), (7, 1)])
def test_lookup_sources_and_counters(k, B):
    sc.check_lookup_sources(_model(), k, B)


@pytest.mark.parametrize("ng", [1, 4])
def test_ngram_sizes(ng):
    sc.check_generate(_model(), 3, 2, lookup="corrupted", ng=ng)


@pytest.mark.parametrize("lookup", ["truth", "none"])
def test_eos_and_stop_sequence(lookup):
    sc.check_generate(_model(), 3, 2, lookup=lookup, eos_from=6)
    sc.check_generate(_model(), 3, 2, lookup=lookup, stop_from=6)


@pytest.mark.parametrize("fmt", ["fp8", "w4a16"])
def test_weight_formats(fmt):
    sc.check_lookup_sources(_model(fmt=fmt), 3, 2)


def test_fp16_operand_library():
    sc.check_lookup_sources(_model("fp16"), 3, 2)


def test_logprobs():
    sc.check_logprobs(_model())


def test_streamer():
    sc.check_streamer(_model())


def test_model_api():
    sc.check_model_api(_model())


def test_not_served():
    sc.check_not_served(_model())


def test_refusals():
    sc.check_refusals(_model())


def test_captures():
    sc.check_captures(_model())


@pytest.mark.parametrize("B", [1, 4])
def test_true_dims(B):
    sc.check_true_dims(B)
