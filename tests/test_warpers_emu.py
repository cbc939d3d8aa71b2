"""The sampler's further warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff) on the CPU emulator (tests/emu): the restatements
against Transformers' classes, vck_warp_support against the float64 restatement in the staged and the global-memory form, draws of
vck_spec_select, and generate() on the tiny model in every precision mode — device loop, host loop, decode pool, beam-sample."""
import pytest

import kernel_cases as kc
import warper_cases as wc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


def test_restatement_against_transformers():
    pytest.importorskip("transformers")
    wc.check_restatement_against_hf()


def test_torch_restatement_against_transformers():
    pytest.importorskip("transformers")
    wc.check_torch_restatement_against_hf()


def test_validation():
    wc.check_validation()


@pytest.mark.parametrize("lds", [-1, 0])
@pytest.mark.parametrize("V", wc.SIZES)
def test_kept_mask(be, V, lds):
    wc.check_kept_mask(be, V, lds)


def test_kept_mask_fp16_operand_library():
    wc.check_kept_mask(kc.EmuBackend("fp16"), 4100, -1)


@pytest.mark.parametrize("lds", [-1, 0])
@pytest.mark.parametrize("V", [96, 4100])
def test_survivor_rows(be, V, lds):
    wc.check_survivor_rows(be, V, lds)


@pytest.mark.parametrize("name", ["typ", "minp", "all"])
def test_draws(be, name):
    wc.check_draws(be, 4100, name, draws=128)   # (the emulator walks every thread of every workgroup: the 2048 draws run on the GPU)


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    wc.close_models()


def _model(emu_lib):
    return wc.model_for("vcoder_ds", emu_lib)


@pytest.mark.parametrize("mode,B", [("bf16", 2), ("bf16", 3), ("strict", 3), ("split", 2)])
def test_single_survivor(emu_lib, mode, B):
    wc.check_single_survivor(_model(emu_lib), mode, B)


@pytest.mark.parametrize("mode,B", [("bf16", 3), ("strict", 2), ("split", 2)])
def test_usual_settings(emu_lib, mode, B):
    wc.check_usual_settings(_model(emu_lib), mode, B)


def test_combinations(emu_lib):
    wc.check_combinations(_model(emu_lib))


def test_pooled_sessions(emu_lib):
    wc.check_pooled_sessions(_model(emu_lib))


def test_no_leak_and_refusals(emu_lib):
    wc.check_no_leak_and_refusals(_model(emu_lib))


def test_beam_sample(emu_lib):
    wc.check_beam_sample(_model(emu_lib))
