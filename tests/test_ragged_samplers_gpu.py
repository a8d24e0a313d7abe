"""Ragged batches through the Schroedinger-bridge sampler and the per-utterance Langevin corrector, and replayed noise in ragged
batches (ragged_samplers_checks.py), on the hardware."""
import pytest

import ragged_samplers_checks as R
import sampler_noise_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip):
    return K.small_model(hip)


@pytest.fixture(scope="module")
def sb_model(hip):
    return K.small_sb_model(hip)


@pytest.fixture(scope="module")
def const_model(hip):
    return K.const_score_model(hip)


@pytest.mark.parametrize("stype", ["sde", "ode"])
def test_sb_ragged_batch_equals_the_single_utterance_runs(hip, sb_model, stype):
    R.check_sb_ragged_equals_singles(hip, sb_model, stype)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_langevin_per_utterance_equals_the_single_utterance_runs(hip, model, ragged):
    R.check_langevin_each_equals_singles(hip, model, ragged)


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("frames", [(3, 64), [64, 128]], ids=["uniform", "ragged"])
def test_langevin_per_utterance_follows_the_fp64_closed_form(hip, const_model, frames, denoise):
    R.check_closed_form_langevin_each(hip, *const_model, frames, denoise)


@pytest.mark.parametrize("use_graph", [True, False])
def test_langevin_per_utterance_matches_the_oracle_on_each_utterance_alone(hip, use_graph):
    R.check_langevin_each_oracle(hip, use_graph)


@pytest.mark.parametrize("case", R.REPLAY_CASES)
def test_ragged_replayed_noise(hip, model, sb_model, case):
    R.check_ragged_replayed_noise(hip, sb_model if case == "sb_sde" else model, case)


@pytest.mark.parametrize("kind", ["sb", "langevin"])
def test_captured_step_follows_the_ragged_composition(hip, kind):
    assert R.check_captured_step(hip, kind) == [1, 2]


def test_interfaces(hip, model, sb_model):
    R.check_interfaces(hip, model, sb_model)


@pytest.mark.parametrize("kind", ["sbve", "langevin"])
def test_directory_job_keeps_ragged_batches(hip, tmp_path, kind):
    R.check_directory_job(hip, tmp_path, kind)
