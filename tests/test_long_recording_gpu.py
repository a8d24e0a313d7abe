"""Windowed enhancement of long recordings (long_recording_checks.py) on the hardware."""
import pytest

import long_recording_checks as L

pytestmark = pytest.mark.gpu
SHAPES = [(3, 203), (64, 250)]


@pytest.mark.parametrize("F_, K", SHAPES)
def test_split_windows_are_slices_of_spec_fwd(hip, F_, K):
    L.check_split(hip, F_, K)


@pytest.mark.parametrize("F_, K", SHAPES)
def test_split_then_merge_without_transform_is_the_identity(hip, F_, K):
    L.check_merge_roundtrip(hip, F_, K)


@pytest.mark.parametrize("tt", L.XF)
@pytest.mark.parametrize("F_, K", SHAPES)
def test_merge_blends_the_overlaps(hip, F_, K, tt):
    L.check_merge_blend(hip, F_, K, tt)


def test_refused_plans(hip):
    L.check_merge_refusals(hip)


@pytest.mark.parametrize("kind, stream", [("pc", 3), ("pc", L.STREAM_HI), ("sb", 3)])
def test_a_window_equals_its_own_run(hip, kind, stream):
    L.check_window_equals_own_run(hip, kind, stream)


def test_result_does_not_depend_on_batch_size_or_the_captured_step(hip):
    L.check_batch_size_independence(hip, graphs=(True, False))


@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_waveform_is_the_merge_of_the_returned_windows(hip, kind):
    L.check_composition(hip, kind)


@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_short_recording_takes_the_existing_path(hip, kind):
    L.check_short_input(hip, kind)


@pytest.mark.parametrize("case", L.COUPLED)
def test_coupling_configurations_are_refused_for_long_recordings(hip, case):
    L.check_refusal(hip, case)


def test_directory_job_windows_long_files(hip, tmp_path):
    L.check_directory_job(hip, tmp_path)
