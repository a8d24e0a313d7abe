"""One reverse process over a long recording with the network on windows (window_score_checks.py) on the hardware."""
import pytest

import window_score_checks as WS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [240, 256])
def test_gather_and_blend_kernels_against_the_host_model(hip, K):
    WS.check_kernels(hip, K)


def test_kernel_refusals(hip):
    WS.check_kernel_refusals(hip)


@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_one_window_plan_is_the_plain_run(hip, kind):
    WS.check_one_window_is_plain(hip, kind)


@pytest.mark.parametrize("kind", ["pc", "sb"])
def test_score_mode_equals_the_whole_run_without_context(hip, kind):
    WS.check_context_free(hip, kind)


def test_chunking_never_matters_with_and_without_the_captured_step(hip):
    WS.check_chunking(hip, graphs=(True, False))


def test_wiring_against_a_host_composition(hip):
    WS.check_wiring(hip)


def test_langevin_at_batch_scope_runs_in_score_mode(hip):
    WS.check_context_free(hip, "langevin")


def test_refusals(hip):
    WS.check_refusals(hip)


def test_directory_job_in_score_mode(hip, tmp_path):
    WS.check_directory_job(hip, tmp_path)


def test_distance_to_the_whole_run_is_reported(hip):
    WS.check_distance_to_whole(hip)
