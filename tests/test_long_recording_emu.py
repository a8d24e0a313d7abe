"""Windowed enhancement of long recordings (long_recording_checks.py) on the CPU workgroup emulator."""
import os

import pytest

import long_recording_checks as L

slow = pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="more than a minute of network evaluations on the emulator; set SGMSE_SLOW=1")
SHAPES = [(3, 203), (64, 250)]


@pytest.mark.parametrize("F_, K", SHAPES)
def test_split_windows_are_slices_of_spec_fwd(emu, F_, K):
    L.check_split(emu, F_, K)


@pytest.mark.parametrize("F_, K", SHAPES)
def test_split_then_merge_without_transform_is_the_identity(emu, F_, K):
    L.check_merge_roundtrip(emu, F_, K)


@pytest.mark.parametrize("tt", L.XF)
@pytest.mark.parametrize("F_, K", SHAPES)
def test_merge_blends_the_overlaps(emu, F_, K, tt):
    L.check_merge_blend(emu, F_, K, tt)


def test_refused_plans(emu):
    L.check_merge_refusals(emu)


@pytest.mark.parametrize("kind, stream", [("pc", 3), pytest.param("pc", L.STREAM_HI, marks=slow), pytest.param("sb", 3, marks=slow)])
def test_a_window_equals_its_own_run(emu, kind, stream):
    L.check_window_equals_own_run(emu, kind, stream)


@slow
def test_result_does_not_depend_on_batch_size(emu):
    L.check_batch_size_independence(emu)


def test_waveform_is_the_merge_of_the_returned_windows(emu):
    L.check_composition(emu, "pc")


@pytest.mark.parametrize("kind", ["pc", pytest.param("sb", marks=slow)])
def test_short_recording_takes_the_existing_path(emu, kind):
    L.check_short_input(emu, kind)


@pytest.mark.parametrize("case", [c if c == "langevin" else pytest.param(c, marks=slow) for c in L.COUPLED])
def test_coupling_configurations_are_refused_for_long_recordings(emu, case):
    L.check_refusal(emu, case)


@slow
def test_directory_job_windows_long_files(emu, tmp_path):
    L.check_directory_job(emu, tmp_path)
