"""Classifier-free guidance on the CPU emulator (tests/emu): vck_guidance_combine bit for bit against the numpy float32 restatement
and its scalars against float64, vck_guidance_follow, the torch restatement against the formula (and Transformers' own class where it
exists), generate(guidance_scale=) on the device loop against the host loop, the oracle anchor, the surface."""
import pytest

import guidance_cases as gc
import kernel_cases as kc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


@pytest.mark.parametrize("B,V,ldl,ldo,shift,oshift,layout", gc.COMBINE_SHAPES_EMU)
def test_guidance_combine_kernel(be, B, V, ldl, ldo, shift, oshift, layout):
    gc.check_guidance_combine(be, B, V, ldl, ldo, shift, oshift, layout)


@pytest.mark.parametrize("B,D,npart,advance", gc.FOLLOW_SHAPES_EMU)
def test_guidance_follow_kernel(be, B, D, npart, advance):
    gc.check_guidance_follow(be, B, D, npart, advance)


def test_restatement():
    gc.check_restatement()


def test_restatement_against_transformers():
    if not gc.check_restatement_against_hf():
        pytest.skip("the installed Transformers has no UnbatchedClassifierFreeGuidanceLogitsProcessor")


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    gc.close_models()


# (the emulator runs a 1024-thread workgroup lane by lane: one variant and batch size here; B = 1, the non-DS variant, the weight
# formats and the fp16-operand library run in tests/test_gpu_guidance.py)
def test_device_loop_against_host_loop(emu_lib):
    gc.check_device_vs_host(gc.model_for("vcoder_ds", emu_lib), "vcoder_ds", 2)


def test_with_processors_automaton_logprobs_eos_streamer_nrs(emu_lib):
    gc.check_with_everything(gc.model_for("vcoder_ds", emu_lib), "vcoder_ds")


def test_sampled_ids_lie_in_the_warped_support(emu_lib):
    gc.check_sampled_support(gc.model_for("vcoder_ds", emu_lib), "vcoder_ds")


def test_oracle_anchor(emu_lib):
    gc.check_oracle_anchor(emu_lib)


def test_surface(emu_lib):
    gc.check_surface(gc.model_for("vcoder_ds", emu_lib))
    gc.check_abi_exports(emu_lib)
