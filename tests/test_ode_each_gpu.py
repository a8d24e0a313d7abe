"""Per-utterance step control of the native adaptive sampler (get_ode_sampler(solver="native", step_control="utterance"),
sgmse_amd/csrc/kernels_ode.h) on the hardware."""
import pytest

import ode_each_checks as K
import ode_native_checks as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zero_score_model(hip):
    return N._zero_score_model(hip)


@pytest.mark.parametrize("tol,first_step", K.CLOSED_FORM_CASES)
def test_each_utterance_follows_its_own_scipy_run(hip, zero_score_model, tol, first_step):
    K.check_closed_form_each(hip, zero_score_model, tol, first_step)


def test_each_utterance_of_a_uniform_batch_equals_its_single_run(hip):
    K.check_bit_identity_uniform(hip)


def test_each_utterance_of_a_ragged_batch_equals_its_single_run(hip):
    K.check_bit_identity_ragged(hip)


def test_one_utterance_equals_the_batch_control_on_the_reference_run(hip):
    K.check_fixture_each(hip)


def test_score_wrapper_callback_sees_the_round_stage_major(hip):
    K.check_v2_callback_each(hip)


def test_step_control_interface(hip, zero_score_model):
    K.check_interface_each(hip, zero_score_model)
