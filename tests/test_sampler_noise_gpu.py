"""The samplers' in-kernel Philox noise, its draw schedule and the element-wise update kernels against host models
(philox_model.py, sampler_noise_checks.py) on the hardware."""
import pytest

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


@pytest.fixture(scope="module")
def const_sb_model(hip):
    return K.const_sb_model(hip)


@pytest.mark.parametrize("case", K.STREAM_CASES)
def test_in_kernel_stream_equals_the_model(hip, model, case):
    K.check_device_stream(hip, model, case)


@pytest.mark.parametrize("case", [c for c in K.SCHEDULE_CASES if c != "sb_sde"])
def test_seeded_run_equals_replayed_model_noise(hip, model, case):
    K.check_seeded_equals_replayed(hip, model, case)


def test_seeded_run_equals_replayed_model_noise_sb_sde(hip, sb_model):
    K.check_seeded_equals_replayed(hip, sb_model, "sb_sde")


def test_seeded_run_equals_replayed_model_noise_without_graph(hip, model):
    K.check_seeded_equals_replayed(hip, model, "rd_ald_c1", use_graph=False)


def test_constant_score_models_are_constant(hip, const_model, const_sb_model):
    K.check_constant_score(hip, *const_model)
    K.check_constant_estimate(hip, *const_sb_model)


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("case", K.CLOSED_PC_CASES)
def test_update_kernels_follow_the_fp64_closed_form(hip, const_model, case, denoise):
    K.check_closed_form_pc(hip, *const_model, case, denoise)


def test_probability_flow_update_follows_the_fp64_closed_form(hip, const_model):
    K.check_closed_form_pf(hip, *const_model)


@pytest.mark.parametrize("stype", ["sde", "ode"])
def test_sb_update_follows_its_restatement(hip, const_sb_model, stype):
    K.check_closed_form_sb(hip, *const_sb_model, stype)
