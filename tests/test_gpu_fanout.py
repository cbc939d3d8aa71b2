"""generate(num_return_sequences=n) on one prefill, on the MI355X: the checks of tests/test_fanout_emu.py on the device, both libraries
where the kernels differ, and the equality with the replicated call at 7b dims (2 layers, S = 1216)."""
import pytest

import fanout_cases as fc
import kernel_cases as kc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


_MODELS = {}


def _model(operands="bf16", fmt="bf16"):
    if (operands, fmt) not in _MODELS:
        _MODELS[operands, fmt] = fc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands, fmt)
    return _MODELS[operands, fmt]


@pytest.mark.parametrize("hd,kv8,n,groups", fc.FANOUT_KERNEL_CASES)
def test_attention_fanout(be, hd, kv8, n, groups):
    fc.check_attention_fanout(be, hd, kv8, n, groups, seed=hd + 7 * n + kv8)


@pytest.mark.parametrize("hd,kv8,n,groups,H,S", fc.FANOUT_7B_CASES)
def test_attention_fanout_7b_head_geometry(be, hd, kv8, n, groups, H, S):
    fc.check_attention_fanout(be, hd, kv8, n, groups, H=H, S=S, seed=5)


def test_attention_fanout_refused(be):
    fc.check_attention_fanout_refused(be)


@pytest.mark.parametrize("B,n", [(1, 2), (1, 5), (1, 8), (2, 4)])
def test_equals_replicated_call(B, n):
    fc.check_equal(_model().engine, B, n)


@pytest.mark.parametrize("fmt", ["fp8", "w4a16"])
def test_weight_formats(fmt):
    eng = _model(fmt=fmt).engine
    fc.check_equal(eng, 2, 4)
    fc.check_equal(eng, 1, 5)


def test_fp16_operand_library():
    fc.check_equal(_model("fp16").engine, 2, 4)


def test_rows_differ():
    fc.check_rows_differ(_model().engine)


def test_eos_and_stop_sequence():
    fc.check_eos_and_stop(_model().engine)


def test_logits_processors():
    fc.check_processors(_model().engine)


def test_engine_fallbacks():
    fc.check_engine_fallbacks(_model().engine)


def test_model_api_and_fallbacks():
    fc.check_model_fallbacks(_model())


def test_arguments():
    fc.check_arguments(_model())


def test_step_graphs():
    fc.check_captures(_model().engine)


def test_session_closing():
    fc.check_session_closing(_model())


@pytest.mark.parametrize("batch_invariant", [False, True])
def test_true_dims(batch_invariant):
    fc.check_true_dims(batch_invariant)
