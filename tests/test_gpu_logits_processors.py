"""Logits processors inside the decode loop on the MI355X: vck_logits_process at the true vocabulary sizes in both libraries against
the numpy float32 restatement, generate() with processors on the device loop against the host loop in every precision mode,
properties of the ids, log-probs of the raw rows, no leak between calls, refusals, streaming (the checks of
tests/test_logits_processors_emu.py on the device)."""
import pytest

import kernel_cases as kc
import logits_processor_cases as pc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("rows,V,ldl,shift", pc.KERNEL_SHAPES_GPU)
def test_logits_process_kernel(be, rows, V, ldl, shift):
    pc.check_logits_process(be, rows, V, ldl, shift)


def _model(operands="bf16"):
    return pc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_device_loop_against_host_loop(mode, operands, B):
    pc.check_device_vs_host(_model(operands), mode, B)


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_properties(mode, operands, B, sample):
    pc.check_properties(_model(operands), mode, B, sample)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_with_logprobs(mode, B):
    pc.check_with_logprobs(_model(), mode, B)


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_no_leak_between_calls(mode):
    pc.check_no_leak(_model(), mode)


def test_refusals():
    pc.check_refusals(_model())


def test_streaming():
    pc.check_streaming(_model())
