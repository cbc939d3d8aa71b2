"""Constrained decoding on the MI355X: vck_logits_process_constrained at the true vocabulary sizes in both libraries against the numpy
restatement, generate() with constraint= on the device loop against the host loop in every precision mode and both libraries (the
checks of tests/test_constraint_emu.py on the device), and a 133-entry class list at 7b dims."""
import pytest

import constraint_cases as cc
import kernel_cases as kc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("rows,V,ldl,shift", cc.KERNEL_SHAPES_GPU)
def test_constrained_kernel(be, rows, V, ldl, shift):
    cc.check_constrained_kernel(be, rows, V, ldl, shift)


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    cc.close_models()


def _model(operands="bf16"):
    return cc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands)


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_device_loop_against_host_loop(mode, operands, B, sample):
    cc.check_device_vs_host(_model(operands), mode, B, sample)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_with_all_processors(mode, operands, B):
    cc.check_with_processors(_model(operands), mode, B)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_with_logprobs(mode, B):
    cc.check_with_logprobs(_model(), mode, B)


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_stops_streamer_num_return_sequences(operands):
    cc.check_stops_stream_fanout(_model(operands))


def test_beams():
    cc.check_beams(_model())


def test_speculation_not_served():
    cc.check_speculation_not_served(_model())


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_no_leak_between_calls(mode):
    cc.check_no_leak(_model(), mode)


def test_refusals():
    cc.check_refusals(_model())


def test_class_list_at_7b_dims():
    cc.check_true_dims()
