"""Beam search inside the device loop on the MI355X: vck_beam_step and vck_kv_permute_tail in both libraries (the cases of
tests/test_beam_emu.py on the device), generate(num_beams=n) through vc_generate_beam — the captured beam step replayed several
times — against model._beam_search on the same model, the plumbing and the refusals.  Nothing at 7b size."""
import pytest

import beam_cases as bc
import kernel_cases as kc
from vcoder_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def be(request):
    return kc.HipBackend(request.param)


@pytest.mark.parametrize("V", bc.KERNEL_VOCABS)
@pytest.mark.parametrize("B,n", bc.KERNEL_SHAPES)
def test_beam_step_shapes(be, B, n, V):
    bc.run_kernel_case(be, B, n, V, steps=5, eos_n=2, length_penalty=1.0)


@pytest.mark.parametrize("early", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.5])
@pytest.mark.parametrize("len_counts_prompt", [True, False])
def test_beam_step_modes(be, early, length_penalty, len_counts_prompt):
    ref = bc.run_kernel_case(be, 3, 3, 37, steps=8, eos_n=3, early=early, length_penalty=length_penalty,
                             len_counts_prompt=len_counts_prompt, seed=3)
    assert {"eos_rank_lt_n", "eos_rank_ge_n"} <= ref.events, ref.events


@pytest.mark.parametrize("early", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_beam_step_done_flips(be, early, length_penalty):
    ref = bc.run_kernel_case(be, 3, 3, 37, steps=8, eos_n=3, early=early, length_penalty=length_penalty, seed=3)
    assert f"done_{early}" in ref.events and any(ref.done), ref.events


def test_beam_step_coverage(be):
    seen = set()
    for early in (False, "never"):
        for seed in (3, 4):
            seen |= bc.run_kernel_case(be, 3, 3, 37, steps=8, eos_n=3, early=early, length_penalty=2.5, seed=seed).events
    assert {"evicted", "hyp_rejected", "done_beside_live", "eos_rank_lt_n", "eos_rank_ge_n"} <= seen, seen


@pytest.mark.parametrize("B,n", [(1, 2), (3, 5), (2, 8)])
def test_beam_step_ties(be, B, n):
    ref = bc.run_kernel_case(be, B, n, 37, steps=4, eos_n=2, quant=0.5, seed=1)
    assert "tie_across_beams" in ref.events, ref.events


def test_beam_step_done_beside_live(be):
    ref = bc.run_kernel_case(be, 3, 2, 37, steps=3, eos_n=1, done0=[False, True, False], seed=2)
    assert "done_beside_live" in ref.events
    assert all((t[2:4] == ref.pad).all() for t in ref.tok_tab) and all((p[2:4] == [2, 3]).all() for p in ref.parent_tab)


@pytest.mark.parametrize("B,n", bc.KERNEL_SHAPES)
def test_beam_step_error_flag(be, B, n):
    bc.check_error_flag(be, B, n)


@pytest.mark.parametrize("operands,es,R", [("bf16", 1, 12), ("bf16", 2, 12), ("bf16", 3, 12), ("bf16", 4, 12), ("bf16", 2, 16), ("fp16", 2, 12)])
def test_kv_permute_tail(operands, es, R):
    bc.check_permute_tail(kc.HipBackend(operands), es, R)


def _model(operands="bf16", fmt="bf16"):
    return bc.model_for("vcoder_ds", _lib.load(operands) if operands != "bf16" else None, operands, fmt)


@pytest.mark.parametrize("mode,kind,B,n,new,seed,eos,lp,early,masked", bc.ENGINE_CASES)
def test_generate_beam_equals_host_loop(mode, kind, B, n, new, seed, eos, lp, early, masked):
    bc.check_engine_case(_model(), mode, kind, B, n, new, seed, eos, lp, early, masked)


def test_generate_beam_fp16_library():
    bc.check_engine_case(_model("fp16"), *bc.ENGINE_CASE_FP16)


@pytest.mark.parametrize("mode,masked", [("bf16", False), ("bf16", True), ("split", True)])
def test_prompt_rows_interchangeable(mode, masked):
    bc.check_prompt_rows_interchangeable(_model(), mode, masked)


def test_prompt_rows_interchangeable_e4m3_cache():
    bc.check_prompt_rows_interchangeable(_model(fmt="fp8"), "bf16", True)


def test_refusals():
    bc.check_refusals(_model())


def test_plain_graph_undisturbed():
    bc.check_plain_graph_undisturbed(_model())


def test_host_loop_routes():
    bc.check_host_loop_routes(_model())
