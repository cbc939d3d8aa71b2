"""Logits processors inside the decode loop on the CPU emulator (tests/emu): vck_logits_process against the numpy float32 restatement,
the restatement against Transformers' own processors, generate() with processors on the device loop against the host loop,
properties of the ids, log-probs of the raw rows, no leak between calls, refusals, streaming."""
import pytest

import kernel_cases as kc
import logits_processor_cases as pc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


@pytest.mark.parametrize("rows,V,ldl,shift", pc.KERNEL_SHAPES_EMU)
def test_logits_process_kernel(be, rows, V, ldl, shift):
    pc.check_logits_process(be, rows, V, ldl, shift)


def test_restatement_against_transformers():
    pytest.importorskip("transformers")
    pc.check_restatement_against_hf()


def _model(emu_lib):
    return pc.model_for("vcoder_ds", emu_lib)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_device_loop_against_host_loop(emu_lib, mode, B):
    pc.check_device_vs_host(_model(emu_lib), mode, B)


@pytest.mark.parametrize("mode,B,sample", [("bf16", 2, False), ("bf16", 3, True), ("strict", 2, True), ("strict", 3, False),
                                           ("split", 3, False), ("split", 2, True)])
def test_properties(emu_lib, mode, B, sample):
    pc.check_properties(_model(emu_lib), mode, B, sample)


@pytest.mark.parametrize("mode,B", [("bf16", 2), ("strict", 3), ("split", 2)])
def test_with_logprobs(emu_lib, mode, B):
    pc.check_with_logprobs(_model(emu_lib), mode, B)


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_no_leak_between_calls(emu_lib, mode):
    pc.check_no_leak(_model(emu_lib), mode)


def test_refusals(emu_lib):
    pc.check_refusals(_model(emu_lib))


def test_streaming(emu_lib):
    pc.check_streaming(_model(emu_lib))
