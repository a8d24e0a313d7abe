"""Operand feed of the Winograd F(4,3) K loop (sgmse_amd/csrc/kernels_conv_wino43.h, SGMSE_WINO43_FEED) on the hardware."""
import pytest

import wino43_feed_checks as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("args,kw", C.CASES, ids=[C.case_id(a, k) for a, k in C.CASES])
def test_wino43_feed_keeps_the_result(hip, args, kw):
    C.check_case(hip, args, kw)


def test_wino43_feed_both_co_blocks(hip):
    C.check_co_blocks(hip)


def test_wino43_feed_repeated_launches_agree(hip):
    C.check_race(hip)
