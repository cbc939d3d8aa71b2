"""Prompt-lookup speculation for sampled and processor-carrying calls (speculate_selection="any") on the MI355X: the checks of
tests/test_speculate_any_emu.py on the device, the kernels in both operand libraries and at the true vocabulary size, and the
bit-identity of a sampled, penalised call at 7b dims (2 layers, S = 1216)."""
import pytest

import kernel_cases as kc
import speculate_any_cases as sa
import speculate_cases as sc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


def _model(operands="bf16", fmt="bf16"):
    return sa.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands, fmt)


@pytest.mark.parametrize("V,Q", [(64, 2), (64, 8), (1000, 2), (1000, 8), (32000, 2), (32000, 8)])
def test_spec_select(be, V, Q):
    sa.check_spec_select(be, V, Q, lds=(-1, 0))


@pytest.mark.parametrize("V,ldl", [(320, 320), (321, 352), (32000, 32000)])
def test_logits_process_verify(be, V, ldl):
    sa.check_logits_process_verify(be, V, ldl)


@pytest.mark.parametrize("logprobs", [False, True])
def test_spec_accept_sel(be, logprobs):
    sa.check_spec_accept_sel(be, logprobs)
    sc.check_spec_accept(be, logprobs)   # sel == nullptr: the argmax path as it was


def test_new_surface():
    sa.check_new_surface(_model())


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("sampler", list(sa.SAMPLERS))
def test_sampled(sampler, k, B):
    sa.check_sampled(_model(), sampler, k, B)


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("name", ["repetition_penalty", "no_repeat_ngram", "bad_word", "min_new_tokens", "all"])
def test_processors(name, sample):
    sa.check_processors(_model(), name, sample)


def test_eos_and_stop_sequence():
    sa.check_eos_and_stop(_model())


def test_num_return_sequences():
    sa.check_num_return_sequences(_model())


@pytest.mark.parametrize("fmt", ["fp8", "w4a16"])
def test_weight_formats(fmt):
    sa.check_sampled(_model(fmt=fmt), "t0.2_k50", 3, 2)


def test_fp16_operand_library():
    sa.check_sampled(_model("fp16"), "t0.2_k50", 3, 2)


def test_streamer():
    sa.check_streamer(_model())


def test_not_served():
    sa.check_not_served(_model())


def test_captures():
    sa.check_captures(_model())


@pytest.mark.parametrize("B", [1, 4])
def test_true_dims(B):
    sa.check_true_dims(B)
