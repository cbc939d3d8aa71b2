"""The sampler's further warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff) on the MI355X, both libraries: vck_warp_support
against the float64 restatement at V = 96 / 4100 / 32000 in the staged and the global-memory form, draws of vck_spec_select, one
selection at V = 32000, and generate() on the tiny models in every precision mode (the checks of tests/test_warpers_emu.py on the
device)."""
import pytest

import kernel_cases as kc
import warper_cases as wc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("lds", [-1, 0])
@pytest.mark.parametrize("V", wc.SIZES)
def test_kept_mask(be, V, lds):
    wc.check_kept_mask(be, V, lds)


@pytest.mark.parametrize("lds", [-1, 0])
@pytest.mark.parametrize("V", [96, 4100])
def test_survivor_rows(be, V, lds):
    wc.check_survivor_rows(be, V, lds)


@pytest.mark.parametrize("name", ["typ", "minp", "all"])
def test_draws(be, name):
    wc.check_draws(be, 4100, name)


def test_selection_at_32000(be):
    wc.check_selection_at_32000(be)


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    wc.close_models()


def _model(operands="bf16"):
    return wc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_single_survivor(mode, operands, B):
    wc.check_single_survivor(_model(operands), mode, B)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode,operands", [("bf16", "bf16"), ("bf16", "fp16"), ("strict", "bf16"), ("split", "bf16")])
def test_usual_settings(mode, operands, B):
    wc.check_usual_settings(_model(operands), mode, B)


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_combinations(operands):
    wc.check_combinations(_model(operands))


def test_pooled_sessions():
    wc.check_pooled_sessions(_model())


def test_no_leak_and_refusals():
    wc.check_no_leak_and_refusals(_model())


def test_beam_sample():
    wc.check_beam_sample(_model())
