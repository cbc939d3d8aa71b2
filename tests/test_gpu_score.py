"""Scoring target tokens on the MI355X: vck_token_logprob at the true vocabulary sizes in both libraries, forward(labels=) / score()
against what the reference recorded in every precision mode, the quantised weight formats against the engine's own logits,
candidates behind one prompt (extend + crop), refusals (the checks of tests/test_score_emu.py on the device)."""
import pytest

import kernel_cases as kc
import score_cases as sc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("rows,V,ldl,shift", sc.KERNEL_SHAPES_GPU)
def test_token_logprob_kernel(be, rows, V, ldl, shift):
    sc.check_token_logprob(be, rows, V, ldl, shift)


def _model(variant, operands="bf16", fmt="bf16"):
    return sc.model_for(variant, _lib.load(operands) if operands != "bf16" else None, operands, fmt)


@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
@pytest.mark.parametrize("name", sc.CASES)
def test_case_against_reference(name, mode, operands):
    sc.check_case(name, _model(sc.case_inputs(name)[0], operands), mode)


@pytest.mark.parametrize("fmt", ["bf16", "w8a16", "fp8"])
def test_score_equals_own_logits(fmt):
    """the quantised formats are not bounded by the fp32-reference fixtures: against float64 log-softmax of the engine's own logits
    of the same call sequence, to the kernel bar"""
    for name in ("ds_img_seg_depth", "ds_unequal", "ds_img_text_seg"):
        sc.check_against_own_logits(_model("vcoder_ds", fmt=fmt), name, sc.KERNEL_BAR)


@pytest.mark.parametrize("B,T,per_row", [(2, 80, 16), (2, 80, 17), (2, 80, 64), (2, 80, 65), (4, 300, None)])
def test_text_only_gemv_gemm_split_and_chunks(B, T, per_row):
    """32 scored rows (one lm_head GEMV pass) and 34 (the GEMM): the score path's measured crossover; 128 and 130: either side of the layer
    linears' EXTEND_GEMV_ROWS, which the score path does not follow (both the GEMM); 1196: more than one chunk of 1024 rows"""
    n = sc.check_text_only(_model("vcoder_ds"), B, T, per_row, seed=T + B)
    assert n == (B * per_row if per_row else B * (T - 1))


@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_candidates_extend_and_crop(mode, operands):
    sc.check_candidates(_model("vcoder_ds", operands), mode=mode)


def test_crop_then_decode():
    sc.check_crop_then_decode(_model("vcoder_ds"))


def test_refusals():
    sc.check_refusals(_model("vcoder_ds"))
