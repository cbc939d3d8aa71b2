"""Scoring target tokens on the CPU emulator (tests/emu): vck_token_logprob against float64, the label splice / token log-probs /
loss of forward(labels=) and score() against what the reference recorded, candidates behind one prompt (extend + crop), refusals."""
import pytest

import kernel_cases as kc
import score_cases as sc


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def emu_lib(be):
    return be.lib


@pytest.mark.parametrize("rows,V,ldl,shift", sc.KERNEL_SHAPES_EMU)
def test_token_logprob_kernel(be, rows, V, ldl, shift):
    sc.check_token_logprob(be, rows, V, ldl, shift)


@pytest.mark.parametrize("mode", ["bf16", "strict"])
@pytest.mark.parametrize("name", sc.CASES)
def test_case_against_reference(emu_lib, name, mode):
    variant = sc.case_inputs(name)[0]
    sc.check_case(name, sc.model_for(variant, emu_lib), mode)


def test_score_equals_own_logits(emu_lib):
    for name in ("ds_img_seg_depth", "ds_unequal"):
        sc.check_against_own_logits(sc.model_for("vcoder_ds", emu_lib), name, sc.KERNEL_BAR)


@pytest.mark.parametrize("B,T,per_row", [(2, 80, 16), (2, 80, 17), (2, 80, 64), (2, 80, 65), (4, 300, None)])
def test_text_only_gemv_gemm_split_and_chunks(emu_lib, B, T, per_row):
    """32 scored rows (one lm_head GEMV pass) and 34 (the GEMM): the score path's measured crossover; 128 and 130: either side of the layer
    linears' EXTEND_GEMV_ROWS, which the score path does not follow (both the GEMM); 1196: more than one chunk of 1024 rows"""
    n = sc.check_text_only(sc.model_for("vcoder_ds", emu_lib), B, T, per_row, seed=T + B)
    assert n == (B * per_row if per_row else B * (T - 1))


@pytest.mark.parametrize("mode", ["bf16", "strict"])
def test_candidates_extend_and_crop(emu_lib, mode):
    # strict runs a chunk as n cached steps (no 128-row split to straddle): a shorter second candidate keeps the emulator quick
    sc.check_candidates(sc.model_for("vcoder_ds", emu_lib), mode=mode, ns=(5, 70) if mode == "bf16" else (5, 12))


def test_crop_then_decode(emu_lib):
    sc.check_crop_then_decode(sc.model_for("vcoder_ds", emu_lib))


def test_refusals(emu_lib):
    sc.check_refusals(sc.model_for("vcoder_ds", emu_lib))


def test_one_token_step_with_labels_has_nan_loss(emu_lib):
    import numpy as np
    import torch

    model = sc.model_for("vcoder_ds", emu_lib)
    variant, ids, labels, imgs, segs, deps = sc.case_inputs("ds_img_seg_depth")
    pre = model(input_ids=torch.from_numpy(ids), images=imgs, segs=segs, depths=deps, use_cache=True)
    tok = torch.full((ids.shape[0], 1), 9, dtype=torch.long)
    out = model(input_ids=tok, labels=tok, past_key_values=pre.past_key_values, images=imgs)
    assert bool(torch.isnan(out.loss)) and out.loss.dtype == torch.float32 and out.logits.shape[1] == 1
    s = model.score(tok, tok, past_key_values=pre.past_key_values)
    assert bool(torch.isnan(s.loss)) and np.array_equal(s.token_logprobs.numpy(), np.zeros((ids.shape[0], 1), np.float32))
