"""Ragged batches through the Schroedinger-bridge sampler and the per-utterance Langevin corrector, and replayed noise in ragged
batches (ragged_samplers_checks.py), on the CPU workgroup emulator."""
import os

import pytest

import ragged_samplers_checks as R
import sampler_noise_checks as K

slow = pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="more than a minute of network evaluations on the emulator; set SGMSE_SLOW=1")


@pytest.fixture(scope="module")
def model(emu):
    return K.small_model(emu)


@pytest.fixture(scope="module")
def sb_model(emu):
    return K.small_sb_model(emu)


@pytest.fixture(scope="module")
def const_model(emu):
    return K.const_score_model(emu)


@pytest.mark.parametrize("stype", ["sde", "ode"])
def test_sb_ragged_batch_equals_the_single_utterance_runs(emu, sb_model, stype):
    R.check_sb_ragged_equals_singles(emu, sb_model, stype)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_langevin_per_utterance_equals_the_single_utterance_runs(emu, model, ragged):
    R.check_langevin_each_equals_singles(emu, model, ragged)


@pytest.mark.parametrize("frames", [(3, 64), [64, 128]], ids=["uniform", "ragged"])
def test_langevin_per_utterance_follows_the_fp64_closed_form(emu, const_model, frames):
    R.check_closed_form_langevin_each(emu, *const_model, frames)


def test_langevin_per_utterance_matches_the_oracle_on_each_utterance_alone(emu):
    R.check_langevin_each_oracle(emu)


@pytest.mark.parametrize("case", [pytest.param(c, marks=slow) if c != "sb_sde" else c for c in R.REPLAY_CASES])
def test_ragged_replayed_noise(emu, model, sb_model, case):
    R.check_ragged_replayed_noise(emu, sb_model if case == "sb_sde" else model, case)


@slow
@pytest.mark.parametrize("kind", ["sb", "langevin"])
def test_ragged_runs_with_use_graph_equal_the_eager_runs(emu, kind):
    assert R.check_captured_step(emu, kind) == [0, 0]      # no graphs on the emulator: the eager path


def test_interfaces(emu, model, sb_model):
    R.check_interfaces(emu, model, sb_model)


@slow
@pytest.mark.parametrize("kind", ["sbve", "langevin"])
def test_directory_job_keeps_ragged_batches(emu, tmp_path, kind):
    R.check_directory_job(emu, tmp_path, kind)
