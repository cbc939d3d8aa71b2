"""generate(num_return_sequences=n) on one prefill, on the CPU emulator (tests/emu): the fan-out attention against the per-row decode
attention, the fan-out call against the call on the prompts repeated n times."""
import os
import subprocess
import sys

import pytest

import fanout_cases as fc
import kernel_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be():
    return kc.EmuBackend()


@pytest.fixture(scope="module")
def model(be):
    return fc.model_for("vcoder_ds", be.lib)


@pytest.mark.parametrize("hd,kv8,n,groups", fc.FANOUT_KERNEL_CASES)
def test_attention_fanout(be, hd, kv8, n, groups):
    fc.check_attention_fanout(be, hd, kv8, n, groups, seed=hd + 7 * n + kv8)


@pytest.mark.parametrize("hd,kv8,n,groups,H,S", fc.FANOUT_7B_CASES)
def test_attention_fanout_7b_head_geometry(be, hd, kv8, n, groups, H, S):
    fc.check_attention_fanout(be, hd, kv8, n, groups, H=H, S=S, seed=5)


def test_attention_fanout_fp16_operand_library():
    be16 = kc.EmuBackend("fp16")
    fc.check_attention_fanout(be16, 128, 0, 5, (("round+1", "cross", 1), ("round", "one", None)))
    fc.check_attention_fanout(be16, 64, 1, 8, (("round+3kpw+1", "first", 0), ("round", "one", 1)))


def test_attention_fanout_refused(be):
    fc.check_attention_fanout_refused(be)


@pytest.mark.parametrize("order", ["1", "11"])   # descending; a seeded random order
def test_attention_fanout_under_other_wave_orders_and_race_check(order):
    """the small cases once more under the emulator's other wave interleavings with its LDS race check on (test_emu_orders.py)"""
    env = dict(os.environ, VC_EMU_ORDER=order, VC_EMU_RACE="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k",
           "test_attention_fanout and not other_wave and not fp16 and not 7b and (groups7 or groups29 or groups51 or groups80)"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("B,n", [(1, 2), (1, 5), (1, 8), (2, 4)])
def test_equals_replicated_call(model, B, n):
    fc.check_equal(model.engine, B, n)


@pytest.mark.parametrize("fmt", ["fp8", "w4a16"])
def test_weight_formats(be, fmt):
    eng = fc.model_for("vcoder_ds", be.lib, fmt=fmt).engine
    fc.check_equal(eng, 2, 4)
    fc.check_equal(eng, 1, 5)


def test_rows_differ(model):
    fc.check_rows_differ(model.engine)


def test_eos_and_stop_sequence(model):
    fc.check_eos_and_stop(model.engine)


def test_logits_processors(model):
    fc.check_processors(model.engine)


def test_engine_fallbacks(model):
    fc.check_engine_fallbacks(model.engine)


def test_model_api_and_fallbacks(model):
    fc.check_model_fallbacks(model)


def test_arguments(model):
    fc.check_arguments(model)


def test_step_graphs(model):
    fc.check_captures(model.engine)


def test_session_closing(model):
    fc.check_session_closing(model)
