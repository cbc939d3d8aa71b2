"""Classifier-free guidance on the MI355X: vck_guidance_combine at the true vocabulary size in both libraries bit for bit against the
numpy float32 restatement (its scalars against float64), vck_guidance_follow at the 7b / 13b row widths, generate(guidance_scale=) on
the device loop against the host loop (both tiny variants, the three weight formats, both libraries), the oracle anchor, the surface
(the checks of tests/test_guidance_emu.py on the device), and the device loop against the host loop at 7b dims."""
import pytest

import guidance_cases as gc
import kernel_cases as kc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    gc.close_models()


@pytest.mark.parametrize("B,V,ldl,ldo,shift,oshift,layout", gc.COMBINE_SHAPES_GPU)
def test_guidance_combine_kernel(be, B, V, ldl, ldo, shift, oshift, layout):
    gc.check_guidance_combine(be, B, V, ldl, ldo, shift, oshift, layout)


@pytest.mark.parametrize("B,D,npart,advance", gc.FOLLOW_SHAPES_GPU)
def test_guidance_follow_kernel(be, B, D, npart, advance):
    gc.check_guidance_follow(be, B, D, npart, advance)


def _model(variant="vcoder_ds", operands="bf16", fmt="bf16"):
    return gc.model_for(variant, _lib.load(operands) if operands != "bf16" else None, operands, fmt)


@pytest.mark.parametrize("variant,B,operands", [("vcoder_ds", 1, "bf16"), ("vcoder_ds", 2, "bf16"), ("vcoder", 2, "bf16"),
                                                ("vcoder_ds", 2, "fp16")])
def test_device_loop_against_host_loop(variant, B, operands):
    gc.check_device_vs_host(_model(variant, operands), variant, B)


@pytest.mark.parametrize("variant", ["vcoder_ds", "vcoder"])
def test_with_processors_automaton_logprobs_eos_streamer_nrs(variant):
    gc.check_with_everything(_model(variant), variant)


@pytest.mark.parametrize("fmt", ["w8a16", "w4a16", "fp8"])   # (fp8: the e4m3 KV cache)
def test_weight_formats(fmt):
    gc.check_device_vs_host(_model(fmt=fmt), "vcoder_ds", 2)


def test_sampled_ids_lie_in_the_warped_support():
    gc.check_sampled_support(_model(), "vcoder_ds")


def test_oracle_anchor():
    gc.check_oracle_anchor()


def test_surface():
    gc.check_surface(_model())
    gc.check_abi_exports(_lib.load())
    gc.check_abi_exports(_lib.load("fp16"))


@pytest.mark.parametrize("fmt", ["bf16", "w4a16"])
def test_device_loop_against_host_loop_at_7b_dims(fmt):
    gc.check_true_dims(fmt)
