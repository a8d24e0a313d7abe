"""The uniform window plan of ``enhance_long(window_blend="score")`` (util/windows.plan_windows_uniform): pure host arithmetic."""
import pytest

import window_score_checks as WS


@pytest.mark.parametrize("K, W, O", WS.PLAN_CASES)
def test_uniform_plan(K, W, O):
    WS.check_plan(K, W, O)


def test_uniform_plan_checks_its_arguments_like_plan_windows():
    WS.check_plan_refusals()
