"""Native adaptive probability-flow sampler (get_ode_sampler(solver="native"), sgmse_amd/csrc/kernels_ode.h) on the hardware."""
import pytest

import ode_native_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zero_score_model(hip):
    return K._zero_score_model(hip)


@pytest.mark.parametrize("tol,first_step", K.CLOSED_FORM_CASES)
def test_native_rk45_follows_scipy_on_a_closed_form_drift(hip, zero_score_model, tol, first_step):
    K.check_closed_form(hip, zero_score_model, tol, first_step)


def test_native_rk45_matches_the_reference_run(hip):
    """92 evaluations at rtol = atol = 1e-3; the distance from the scipy-driven path on the same device is printed."""
    K.check_fixture(hip, "ode_rk45")


def test_native_rk45_matches_the_reference_run_at_the_default_tolerance(hip):
    """722 evaluations at rtol = atol = 1e-5, end state within the samplers' tolerance."""
    K.check_fixture(hip, "ode_rk45_default", compare_scipy=False)


def test_native_rk45_is_bit_stable_and_refuses_what_it_cannot_do(hip):
    K.check_bit_stability_and_interface(hip)


def test_scipy_driven_path_is_still_the_default(hip):
    K.check_scipy_default_unchanged(hip)


def test_native_rk45_score_wrapper_callback_of_v2_models(hip):
    K.check_v2_callback(hip)


def test_native_rk45_batch_control_of_two_utterances(hip):
    K.check_batch_control_step(hip)


def test_enhancement_ode_solver_flag(hip):
    K.check_enhancement_flag(hip)
