"""The samplers' in-kernel Philox noise, its draw schedule and the element-wise update kernels against host models
(philox_model.py, sampler_noise_checks.py): the generator model alone (no library), then the CPU workgroup emulator."""
import os

import pytest

import sampler_noise_checks as K

slow = pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="more than a minute of network evaluations on the emulator; set SGMSE_SLOW=1")


# ---- the generator model alone -------------------------------------------------------------------------------------------

def test_philox_model_reproduces_the_random123_known_answers():
    K.check_known_answers()


def test_philox_model_streams_are_uncorrelated_and_finite():
    K.check_stream_separation()


# ---- the emulator --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(emu):
    return K.small_model(emu)


@pytest.fixture(scope="module")
def sb_model(emu):
    return K.small_sb_model(emu)


@pytest.fixture(scope="module")
def const_model(emu):
    return K.const_score_model(emu)


@pytest.fixture(scope="module")
def const_sb_model(emu):
    return K.const_sb_model(emu)


def test_philox_noise_statistics(emu):
    K.check_philox_noise_statistics(emu)


@pytest.mark.parametrize("case", K.STREAM_CASES)
def test_in_kernel_stream_equals_the_model(emu, model, case):
    K.check_device_stream(emu, model, case)


@pytest.mark.parametrize("case", [pytest.param(c, marks=slow) if c in ("rd_ald_c2", "ode_native") else c
                                  for c in K.SCHEDULE_CASES if c != "sb_sde"])
def test_seeded_run_equals_replayed_model_noise(emu, model, case):
    K.check_seeded_equals_replayed(emu, model, case)


def test_seeded_run_equals_replayed_model_noise_sb_sde(emu, sb_model):
    K.check_seeded_equals_replayed(emu, sb_model, "sb_sde")


@slow
def test_seeded_run_equals_replayed_model_noise_without_graph(emu, model):
    K.check_seeded_equals_replayed(emu, model, "rd_ald_c1", use_graph=False)


def test_constant_score_models_are_constant(emu, const_model, const_sb_model):
    K.check_constant_score(emu, *const_model)
    K.check_constant_estimate(emu, *const_sb_model)


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("case", K.CLOSED_PC_CASES)
def test_update_kernels_follow_the_fp64_closed_form(emu, const_model, case, denoise):
    K.check_closed_form_pc(emu, *const_model, case, denoise)


def test_probability_flow_update_follows_the_fp64_closed_form(emu, const_model):
    K.check_closed_form_pf(emu, *const_model)


@pytest.mark.parametrize("stype", ["sde", "ode"])
def test_sb_update_follows_its_restatement(emu, const_sb_model, stype):
    K.check_closed_form_sb(emu, *const_sb_model, stype)
