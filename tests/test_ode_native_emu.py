"""Native adaptive probability-flow sampler (get_ode_sampler(solver="native"), sgmse_amd/csrc/kernels_ode.h) on the CPU workgroup
emulator: the step controller, the stage / error / norm kernels and the Python interface."""
import os

import pytest

import ode_native_checks as K


@pytest.fixture(scope="module")
def zero_score_model(emu):
    return K._zero_score_model(emu)


@pytest.mark.parametrize("tol,first_step", K.CLOSED_FORM_CASES)
def test_native_rk45_follows_scipy_on_a_closed_form_drift(emu, zero_score_model, tol, first_step):
    K.check_closed_form(emu, zero_score_model, tol, first_step)


@pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="92 network evaluations on the emulator (minutes); set SGMSE_SLOW=1")
def test_native_rk45_matches_the_reference_run(emu):
    K.check_fixture(emu, "ode_rk45")


def test_native_rk45_is_bit_stable_and_refuses_what_it_cannot_do(emu):
    K.check_bit_stability_and_interface(emu, quick=True)


def test_scipy_driven_path_is_still_the_default(emu):
    K.check_scipy_default_unchanged(emu)


def test_native_rk45_score_wrapper_callback_of_v2_models(emu):
    K.check_v2_callback(emu)


def test_native_rk45_batch_control_of_two_utterances(emu):
    K.check_batch_control_step(emu)


def test_enhancement_ode_solver_flag(emu):
    K.check_enhancement_flag(emu)
