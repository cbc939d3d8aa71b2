"""Per-token log-probs and top-K alternatives on the CPU emulator (tests/emu): vck_topk_logprob against float64, generate() with
log-probs against the engine's own logits, finishing / masking, score(top_logprobs=), the host fallback loop, refusals."""
import pytest

import kernel_cases as kc
import logprob_cases as lc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


@pytest.mark.parametrize("K", lc.KS)
@pytest.mark.parametrize("rows,V,ldl,shift", lc.KERNEL_SHAPES_EMU)
def test_topk_logprob_kernel(be, rows, V, ldl, shift, K):
    lc.check_topk_logprob(be, rows, V, ldl, shift, K)


def _model(emu_lib, fmt="bf16"):
    return lc.model_for("vcoder_ds", emu_lib, fmt=fmt)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_generate_greedy(emu_lib, mode, B):
    lc.check_generate(_model(emu_lib), mode, B)


@pytest.mark.parametrize("mode,B", [("bf16", 2), ("bf16", 3), ("split", 2)])
def test_generate_sampled(emu_lib, mode, B):
    lc.check_generate(_model(emu_lib), mode, B, sample=True)


@pytest.mark.parametrize("fmt", ["w8a16", "fp8"])
def test_generate_weight_formats(emu_lib, fmt):
    lc.check_generate(_model(emu_lib, fmt), "bf16", 2)


def test_generate_fp16_library():
    lc.check_generate(lc.model_for("vcoder_ds", kc.EmuBackend("fp16").lib, "fp16"), "bf16", 2)


def test_finishing(emu_lib):
    lc.check_finishing(_model(emu_lib))


def test_streaming(emu_lib):
    lc.check_streaming(_model(emu_lib))


@pytest.mark.parametrize("mode", ["bf16", "strict"])
def test_followed_by_plain(emu_lib, mode):
    lc.check_followed_by_plain(_model(emu_lib), mode)


@pytest.mark.parametrize("B,T,per_row", [(2, 80, 16), (2, 80, 17)])
def test_score_top_text_only(emu_lib, B, T, per_row):
    lc.check_score_text_only(_model(emu_lib), B, T, per_row)


def test_score_top_multimodal(emu_lib):
    lc.check_score_case(_model(emu_lib))


@pytest.mark.parametrize("mode", ["bf16", "strict"])
def test_score_top_continuation(emu_lib, mode):
    lc.check_score_continuation(_model(emu_lib), mode)


def test_host_fallback(emu_lib):
    lc.check_host_fallback(_model(emu_lib))


def test_refusals(emu_lib):
    lc.check_refusals(_model(emu_lib))
