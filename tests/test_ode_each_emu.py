"""Per-utterance step control of the native adaptive sampler (get_ode_sampler(solver="native", step_control="utterance"),
sgmse_amd/csrc/kernels_ode.h) on the CPU workgroup emulator.  The emulator takes seconds per evaluation: the closed-form cases run
in full on the zero-score network, the bit-identity cases with the quick settings of ode_each_checks (one half-interval attempt on the
random-weight network; the round that one utterance accepts and the other rejects on the zero-score network)."""
import os

import pytest

import ode_each_checks as K
import ode_native_checks as N


@pytest.fixture(scope="module")
def zero_score_model(emu):
    return N._zero_score_model(emu)


@pytest.mark.parametrize("tol,first_step", K.CLOSED_FORM_CASES)
def test_each_utterance_follows_its_own_scipy_run(emu, zero_score_model, tol, first_step):
    K.check_closed_form_each(emu, zero_score_model, tol, first_step)


def test_each_utterance_of_a_uniform_batch_equals_its_single_run(emu, zero_score_model):
    K.check_bit_identity_uniform(emu, quick=True, zero_model=zero_score_model)


def test_each_utterance_of_a_ragged_batch_equals_its_single_run(emu):
    K.check_bit_identity_ragged(emu, quick=True)


@pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="2 x 92 network evaluations on the emulator (minutes); set SGMSE_SLOW=1")
def test_one_utterance_equals_the_batch_control_on_the_reference_run(emu):
    K.check_fixture_each(emu)


def test_score_wrapper_callback_sees_the_round_stage_major(emu):
    K.check_v2_callback_each(emu)


def test_step_control_interface(emu, zero_score_model):
    K.check_interface_each(emu, zero_score_model, quick=True)
