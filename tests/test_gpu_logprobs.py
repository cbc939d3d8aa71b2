"""Per-token log-probs and top-K alternatives on the MI355X: vck_topk_logprob at the true vocabulary sizes in both libraries (staged in
LDS and re-read from global memory), generate() with log-probs in every precision mode / library / weight format against the engine's
own logits, finishing, streaming, score(top_logprobs=), the host fallback loop, refusals (the checks of tests/test_logprobs_emu.py on
the device)."""
import pytest

import kernel_cases as kc
import logprob_cases as lc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("K", lc.KS)
@pytest.mark.parametrize("rows,V,ldl,shift", lc.KERNEL_SHAPES_GPU)
def test_topk_logprob_kernel(be, rows, V, ldl, shift, K):
    lc.check_topk_logprob(be, rows, V, ldl, shift, K)


def _model(operands="bf16", fmt="bf16"):
    return lc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands, fmt)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_generate_greedy(mode, operands, B):
    lc.check_generate(_model(operands), mode, B)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_generate_sampled(mode, operands, B):
    lc.check_generate(_model(operands), mode, B, sample=True)


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("fmt", ["w8a16", "fp8"])
def test_generate_weight_formats(fmt, sample):
    lc.check_generate(_model(fmt=fmt), "bf16", 2, sample=sample)


def test_finishing():
    lc.check_finishing(_model())


def test_streaming():
    lc.check_streaming(_model())


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_followed_by_plain(mode):
    lc.check_followed_by_plain(_model(), mode)


@pytest.mark.parametrize("B,T,per_row", [(2, 80, 16), (2, 80, 17)])
def test_score_top_text_only(B, T, per_row):
    lc.check_score_text_only(_model(), B, T, per_row)


@pytest.mark.parametrize("fmt", ["bf16", "w8a16", "fp8"])
def test_score_top_multimodal(fmt):
    lc.check_score_case(_model(fmt=fmt))


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_score_top_continuation(mode):
    lc.check_score_continuation(_model(), mode)


def test_host_fallback():
    lc.check_host_fallback(_model())


def test_refusals():
    lc.check_refusals(_model())
