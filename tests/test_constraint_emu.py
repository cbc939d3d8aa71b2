"""Constrained decoding on the CPU emulator (tests/emu): vck_logits_process_constrained against the numpy restatement, the torch
restatement against Transformers' PrefixConstrainedLogitsProcessor, the TokenAutomaton builders against brute force, generate() with
constraint= on the device loop against the host loop under the automaton's callable, with processors, log-probs, stops, a streamer,
num_return_sequences, beams, speculation, no leak between calls, refusals."""
import pytest

import constraint_cases as cc
import kernel_cases as kc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


@pytest.mark.parametrize("rows,V,ldl,shift", cc.KERNEL_SHAPES_EMU)
def test_constrained_kernel(be, rows, V, ldl, shift):
    cc.check_constrained_kernel(be, rows, V, ldl, shift)


def test_apply_prefix_constraint_against_transformers():
    pytest.importorskip("transformers")
    cc.check_apply_prefix_constraint_against_hf()


def test_builders():
    cc.check_builders()


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    cc.close_models()


def _model(emu_lib):
    return cc.model_for("vcoder_ds", emu_lib)


@pytest.mark.parametrize("mode,B,sample", [("bf16", 2, False), ("bf16", 3, True), ("strict", 3, False), ("strict", 2, True),
                                           ("split", 2, False), ("split", 3, True)])
def test_device_loop_against_host_loop(emu_lib, mode, B, sample):
    cc.check_device_vs_host(_model(emu_lib), mode, B, sample)


@pytest.mark.parametrize("mode,B", [("bf16", 3), ("strict", 2), ("split", 2)])
def test_with_all_processors(emu_lib, mode, B):
    cc.check_with_processors(_model(emu_lib), mode, B)


@pytest.mark.parametrize("mode,B", [("bf16", 2), ("strict", 3), ("split", 2)])
def test_with_logprobs(emu_lib, mode, B):
    cc.check_with_logprobs(_model(emu_lib), mode, B)


def test_stops_streamer_num_return_sequences(emu_lib):
    cc.check_stops_stream_fanout(_model(emu_lib))


def test_beams(emu_lib):
    cc.check_beams(_model(emu_lib))


def test_speculation_not_served(emu_lib):
    cc.check_speculation_not_served(_model(emu_lib))


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_no_leak_between_calls(emu_lib, mode):
    cc.check_no_leak(_model(emu_lib), mode)


def test_refusals(emu_lib):
    cc.check_refusals(_model(emu_lib))
