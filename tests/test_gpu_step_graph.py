"""The session's captured decode steps on the MI355X: the checks of tests/test_step_graph_emu.py on the device (a stale address or
size in a replayed hipGraph is wrong at any shape: the tiny model's)."""
import pytest

import step_graph_cases as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    return sg.model_for("vcoder_ds")


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
