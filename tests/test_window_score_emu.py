"""One reverse process over a long recording with the network on windows (window_score_checks.py) on the CPU workgroup emulator."""
import os

import pytest

import window_score_checks as WS

slow = pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="more than a minute of network evaluations on the emulator; set SGMSE_SLOW=1")


@pytest.mark.parametrize("K", [240, 256])
def test_gather_and_blend_kernels_against_the_host_model(emu, K):
    WS.check_kernels(emu, K)


def test_kernel_refusals(emu):
    WS.check_kernel_refusals(emu)


@pytest.mark.parametrize("kind", ["pc", pytest.param("sb", marks=slow)])
def test_one_window_plan_is_the_plain_run(emu, kind):
    WS.check_one_window_is_plain(emu, kind)


@slow
@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_score_mode_equals_the_whole_run_without_context(emu, kind):
    WS.check_context_free(emu, kind)


@slow
def test_chunking_never_matters(emu):
    WS.check_chunking(emu)


@slow
def test_wiring_against_a_host_composition(emu):
    WS.check_wiring(emu)


@slow
def test_langevin_at_batch_scope_runs_in_score_mode(emu):
    WS.check_context_free(emu, "langevin")


def test_refusals(emu):
    WS.check_refusals(emu)


@slow
def test_directory_job_in_score_mode(emu, tmp_path):
    WS.check_directory_job(emu, tmp_path)


@slow
def test_distance_to_the_whole_run_is_reported(emu):
    WS.check_distance_to_whole(emu)
