"""The session's captured decode steps on the CPU emulator (tests/emu): replay without re-capture, one re-capture of the kind a call
uses per change of anything its step bakes in, the plain step behind a call with log-probs and processors, strict mode — every result
against a fresh session's (tests/step_graph_cases.py)."""
import pytest

import kernel_cases as kc
import step_graph_cases as sg


@pytest.fixture(scope="module")
def model():
    return sg.model_for("vcoder_ds", kc.EmuBackend().lib)


def test_replay_without_recapture(model):
    sg.check_replay(model)


def test_every_baked_change_recaptures_once(model):
    sg.check_recapture(model)


def test_grow_kv_recaptures_once(model):
    sg.check_grow_kv(model)


@pytest.mark.parametrize("mode", ["bf16", "strict", "split"])
def test_plain_step_behind_logprob_processor_call(model, mode):
    sg.check_plain_after_call(model, mode)


def test_strict_mode_never_captures(model):
    sg.check_strict(model)
