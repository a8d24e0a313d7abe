"""The noise geometry of the in-kernel Philox noise and window_noise="recording" (window_noise_checks.py) on the CPU workgroup emulator."""
import os

import pytest

import long_recording_checks as L
import sampler_noise_checks as K
import window_noise_checks as WN

slow = pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="more than a minute of network evaluations on the emulator; set SGMSE_SLOW=1")
FAST_CONSUMERS = {("rd_ald", "uniform")}


@pytest.fixture(scope="module")
def model(emu):
    return K.small_model(emu)


@pytest.fixture(scope="module")
def sb_model(emu):
    return K.small_sb_model(emu, N=2)


@pytest.mark.parametrize("layout", WN.LAYOUTS)
def test_in_kernel_stream_under_a_geometry_equals_the_model(emu, model, layout):
    WN.check_device_stream_geometry(emu, model, layout)


@pytest.mark.parametrize("case", ["pc_ald", pytest.param("sb_sde", marks=slow), pytest.param("ode_each", marks=slow)])
def test_explicit_default_geometry_equals_none(emu, model, sb_model, case):
    WN.check_explicit_default(emu, sb_model if case == "sb_sde" else model, case)


def test_geometry_of_another_batch_size_is_ignored(emu, model):
    WN.check_other_batch_size_ignores(emu, model)


def test_overlapping_utterances_of_one_stream_share_draws(emu, model):
    WN.check_overlaps_share_draws(emu, model)


@pytest.mark.parametrize("case, layout", [c if c in FAST_CONSUMERS else pytest.param(*c, marks=slow) for c in WN.CONSUMER_CASES])
def test_every_noise_consumer_follows_the_geometry(emu, model, sb_model, case, layout):
    WN.check_consumer(emu, sb_model if case == "sb_sde" else model, case, layout)


@slow
@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_windowed_run_equals_the_whole_run_without_context(emu, kind):
    WN.check_windowed_equals_whole(emu, kind)


@slow
def test_recording_mode_does_not_depend_on_batch_size(emu):
    WN.check_batch_size_independence(emu)


def test_refusals(emu, model, tmp_path):
    WN.check_refusals(emu, model, tmp_path)


@slow
def test_directory_job_in_recording_mode(emu, tmp_path):
    WN.check_directory_job(emu, tmp_path)


@slow
def test_overlap_agreement_is_reported(emu):
    WN.check_overlap_agreement(emu)
