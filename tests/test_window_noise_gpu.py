"""The noise geometry of the in-kernel Philox noise and window_noise="recording" (window_noise_checks.py) on the hardware."""
import pytest

import sampler_noise_checks as K
import window_noise_checks as WN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip):
    return K.small_model(hip)


@pytest.fixture(scope="module")
def sb_model(hip):
    return K.small_sb_model(hip, N=2)


@pytest.mark.parametrize("layout", WN.LAYOUTS)
def test_in_kernel_stream_under_a_geometry_equals_the_model(hip, model, layout):
    WN.check_device_stream_geometry(hip, model, layout)


@pytest.mark.parametrize("case", WN.DEFAULT_CASES)
def test_explicit_default_geometry_equals_none(hip, model, sb_model, case):
    WN.check_explicit_default(hip, sb_model if case == "sb_sde" else model, case)


def test_geometry_of_another_batch_size_is_ignored(hip, model):
    WN.check_other_batch_size_ignores(hip, model)


def test_overlapping_utterances_of_one_stream_share_draws(hip, model):
    WN.check_overlaps_share_draws(hip, model)


@pytest.mark.parametrize("case, layout", WN.CONSUMER_CASES)
def test_every_noise_consumer_follows_the_geometry(hip, model, sb_model, case, layout):
    WN.check_consumer(hip, sb_model if case == "sb_sde" else model, case, layout)


def test_noise_consumers_follow_the_geometry_without_the_captured_step(hip, model):
    WN.check_consumer(hip, model, "rd_ald", "ragged", use_graph=False)


@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_windowed_run_equals_the_whole_run_without_context(hip, kind):
    WN.check_windowed_equals_whole(hip, kind)


def test_recording_mode_does_not_depend_on_batch_size_or_the_captured_step(hip):
    WN.check_batch_size_independence(hip, graphs=(True, False))


def test_a_new_geometry_needs_no_new_capture(hip, model):
    WN.check_no_new_capture(hip, model)


def test_refusals(hip, model, tmp_path):
    WN.check_refusals(hip, model, tmp_path)


def test_directory_job_in_recording_mode(hip, tmp_path):
    WN.check_directory_job(hip, tmp_path)


def test_overlap_agreement_is_reported(hip):
    WN.check_overlap_agreement(hip)
