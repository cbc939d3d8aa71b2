"""Prompt-lookup speculation for sampled and processor-carrying calls (speculate_selection="any") on the CPU emulator (tests/emu): the
selection, processor and accept kernels of the verify step against their references, generate(speculate=k,
speculate_selection="any") against the plain session loop of the same arguments and seed."""
import pytest

import kernel_cases as kc
import speculate_any_cases as sa
import speculate_cases as sc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def model(be):
    return sa.model_for("vcoder_ds", be.lib)


@pytest.mark.parametrize("V,Q", [(64, 2), (64, 8), (1000, 2), (1000, 8)])
def test_spec_select(be, V, Q):
    sa.check_spec_select(be, V, Q, lds=(-1, 0))


def test_spec_select_fp16_operand_library():
    sa.check_spec_select(kc.EmuBackend("fp16"), 1000, 8, lds=(-1, 0))


@pytest.mark.parametrize("V,ldl", [(320, 320), (321, 352)])
def test_logits_process_verify(be, V, ldl):
    sa.check_logits_process_verify(be, V, ldl)


@pytest.mark.parametrize("logprobs", [False, True])
def test_spec_accept_sel(be, logprobs):
    sa.check_spec_accept_sel(be, logprobs)
    sc.check_spec_accept(be, logprobs)   # sel == nullptr: the argmax path as it was


def test_new_surface(model):
    sa.check_new_surface(model)


# (the emulator runs every 1024-thread sampler pass lane by lane: a cross of the full matrix, which the device tests run whole)
@pytest.mark.parametrize("sampler,k,B", [("t0.2_k50", 1, 2), ("t0.2_k50", 3, 2), ("t0.2_k50", 7, 2), ("t0.2_k50", 3, 1), ("t0.2_k50", 3, 4),
                                         ("t0.8_k20_p0.9", 3, 2), ("t0.8_k20_p0.9", 7, 1), ("t0.8_k20_p0.9", 1, 4)])
def test_sampled(model, sampler, k, B):
    sa.check_sampled(model, sampler, k, B)


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("name", ["repetition_penalty", "no_repeat_ngram", "bad_word", "min_new_tokens", "all"])
def test_processors(model, name, sample):
    sa.check_processors(model, name, sample)


def test_eos_and_stop_sequence(model):
    sa.check_eos_and_stop(model)


def test_num_return_sequences(model):
    sa.check_num_return_sequences(model)


@pytest.mark.parametrize("fmt", ["fp8", "w4a16"])
def test_weight_formats(be, fmt):
    sa.check_sampled(sa.model_for("vcoder_ds", be.lib, fmt=fmt), "t0.2_k50", 3, 2)


def test_fp16_operand_library():
    sa.check_sampled(sa.model_for("vcoder_ds", kc.EmuBackend("fp16").lib, "fp16"), "t0.2_k50", 3, 2)


def test_streamer(model):
    sa.check_streamer(model)


def test_not_served(model):
    sa.check_not_served(model)
    sc.check_not_served(model)   # the default scope, as it was


def test_captures(model):
    sa.check_captures(model)
